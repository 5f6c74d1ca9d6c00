// schur_common.hpp -- what the three units either side of the solve share (schur.hip: formation; schur_ginv.hip: primal recovery
// and gamma alone, the two steps that apply the stored G^-1; schur_residual.hip: the KKT residual norms): the packed KKT layout,
// the LDS need of every any-size kernel, the list of block sizes the four-knots-per-wave kernels are built for, and the two
// halves of every launcher -- the walk over that list and the launch of an any-size kernel.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "bt_device.hpp"
#include "internal.hpp"

namespace gbdpcg {

struct KktDims {
    uint32_t nx, nu, N;
    uint32_t sg, sc, sv;  // strides of one knot in G / C / g
    size_t szG, szC, szg, szc;
    __host__ __device__ KktDims(uint32_t nx_, uint32_t nu_, uint32_t N_) : nx(nx_), nu(nu_), N(N_)
    {
        sg = nx * nx + nu * nu;
        sc = nx * nx + nx * nu;
        sv = nx + nu;
        szG = (size_t)sg * N - nu * nu;
        szC = (size_t)sc * (N - 1);
        szg = (size_t)sv * N - nu;
        szc = (size_t)nx * N;
    }
};

// LDS elements one wave of each any-size kernel needs (kept a multiple of 4 so that every wave's block starts 16-byte aligned).
__host__ __device__ inline uint32_t schur_wave_elems(uint32_t nx, uint32_t nu)
{
    const uint32_t m = nx > nu ? nx : nu;
    const uint32_t e = 2 * m * m + 3 * m      // tableau, scaled pivot row, pivot column
                       + 5 * nx * nx          // Qc, Qp, Ap, Ac, W
                       + nu * nu              // Rp
                       + 2 * nx * nu          // Bp, V
                       + 3 * nx + nu;         // q_k, q_j, c_k, r_j
    return (e + 3u) & ~3u;
}
__host__ __device__ inline uint32_t recover_wave_elems(uint32_t nx, uint32_t nu)
{
    const uint32_t e = 2 * nx * nx + nu * nu + nx * nu + 3 * nx + nu;  // Qi, A, Ri, B, lambda_{k+1}, t_x, (spare), t_u
    return (e + 3u) & ~3u;
}
__host__ __device__ inline uint32_t gamma_wave_elems(uint32_t nx, uint32_t nu)
{
    const uint32_t e = 3 * nx * nx + nu * nu + nx * nu + 4 * nx + 2 * nu;  // Qi_k, Qi_j, A_j, Ri_j, B_j, q_k, q_j, w_j, (spare), r_j, v_j
    return (e + 3u) & ~3u;
}
__host__ __device__ inline uint32_t residual_wave_elems(uint32_t nx, uint32_t nu)
{
    const uint32_t e = 2 * nx * nx + nu * nu + nx * nu + 3 * nx + nu + 2;  // Q, A, R, B, x_k, -lambda_{k+1}, (spare), u_k, the wave's two maxima
    return (e + 3u) & ~3u;
}

// Waves per workgroup for a per-wave LDS need; 0 = does not fit one CU.
inline uint32_t waves_for(const DeviceInfo &dev, size_t wave_bytes)
{
    if (wave_bytes > dev.lds_per_wg_max) return 0;
    uint32_t w = 4;
    while (w > 1 && w * wave_bytes > 64 * 1024) --w;
    return w;
}

// The block sizes the four-knots-per-wave kernels are built for: stateSize = 2 x joints, controlSize = joints (a manipulator's
// positions and velocities against its torques; 14 / 7 is the BASELINE shape), and the pendulum (2 / 1), cart-pole (4 / 1) and
// quadrotor (12 / 4, 13 / 4 with a quaternion) shapes of the MPC literature.  Other sizes take the any-size LDS kernels.
#define GBDPCG_QUAD_SHAPES(X) X(2, 1) X(4, 1) X(4, 2) X(6, 3) X(8, 4) X(10, 5) X(12, 4) X(12, 6) X(13, 4) X(14, 7) \
    X(3, 1) X(5, 2) X(6, 1) X(6, 2) X(7, 3) X(8, 2) X(9, 3) X(10, 4) X(11, 4) X(12, 3)   /* round 3: under-actuated and odd shapes (9 / 3, 1024 x 128: formation 512 -> 95 us, recovery 95 -> 30 us) */

// The first half of a launcher.  True: the call is settled and `status` is its result -- (nx, nu) is in the list above and
// launch(NX, NU) (two std::integral_constant<int, .>, so that NX() is a template argument) returned it, or quad_grid, the
// workgroups of the four-knots-per-wave launch where the caller knows them beforehand (else 0), is more than a grid holds:
// refused before the list is looked at.  False: the any-size kernel is to take the call -- the shape is not in the list, or
// GBDPCG_SCHUR_GENERAL=1 (A/B runs, tests) asks for it.  The variable is read on EVERY call: the tests flip it inside one process.
template <typename F> bool quad_dispatch(uint32_t nx, uint32_t nu, uint64_t quad_grid, hipError_t &status, F &&launch)
{
    const char *env = getenv("GBDPCG_SCHUR_GENERAL");
    if (env && env[0] == '1') return false;
    if (quad_grid > 0x7fffffffull) {
        status = hipErrorInvalidValue;
        return true;
    }
#define GBDPCG_X(NX, NU)                                                                        \
    if (nx == NX && nu == NU) {                                                                 \
        status = launch(std::integral_constant<int, NX>{}, std::integral_constant<int, NU>{});   \
        return true;                                                                            \
    }
    GBDPCG_QUAD_SHAPES(GBDPCG_X)
#undef GBDPCG_X
    return false;
}

// The second half: an any-size kernel, one wavefront per row and as many of them per workgroup (four at most) as fit 64 KB of
// LDS at wave_bytes each.  grid_of(waves) is the number of workgroups.  Refused: a row that does not fit one compute unit's
// LDS, a grid of more than 0x7fffffff workgroups.
template <typename K, typename G, typename... A>
hipError_t launch_lds_rows(const DeviceInfo &dev, K kern, size_t wave_bytes, G &&grid_of, hipStream_t s, A... args)
{
    const uint32_t waves = waves_for(dev, wave_bytes);
    if (!waves) return hipErrorInvalidValue;
    const uint64_t grid = grid_of(waves);
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds = waves * wave_bytes;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(64 * waves), lds, s, args...);
    return hipGetLastError();
}

}  // namespace gbdpcg
