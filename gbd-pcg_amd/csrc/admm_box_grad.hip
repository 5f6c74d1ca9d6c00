// admm_box_grad.hip -- the elementwise launches of the backward pass behind the adjoint loops: the bound gradients of the hard box
// (gbdpcg_admm_grad_bounds_*), and for the SOFT (L1-penalised) box and rows QPs the mask in front of the loop and the bound gradients
// with kappa (gbdpcg_admm_soft_mask_*, gbdpcg_admm_lin_soft_mask_*, gbdpcg_admm_soft_grad_bounds_*).
//
// Bound gradients of the hard box, with yf the forward y, ya the adjoint's y (nu = rho ya), one multiplication and one negation:
//     glo_i = yf_i < 0 ? -(rho_b ya_i) : +0        ghi_i = yf_i > 0 ? -(rho_b ya_i) : +0
//
// Behind a soft update (soft_clip in ieee_once.hpp) the forward y (yf, read only) splits the rows of problem b into three sets, with
// theta_r = kappa_r / rho_b the ONE correctly rounded division of the update:
//     free        yf_r == 0                          inside its bounds, mu_r = 0
//     held        yf_r != 0 and |yf_r| < theta_r     on a bound, |mu_r| < kappa_r             (a NaN yf_r fails the comparison: held)
//     saturated   |yf_r| >= theta_r                  beyond its bound, mu_r = +-kappa_r: the update wrote +-theta itself
// A saturated multiplier does not move with z, so in the adjoint problem the row is as free as an inactive one: the adjoint is
// the HARD adjoint loop (the adjoint of admm.hip, the adjoint rows of admm_rows.hip) on the masked copy
//     ym_r = |yf_r| >= theta_r ? +0 : yf_r
// A tie |e| = theta takes the third branch of soft_clip with y = +-theta: saturated, that is free -- the convention of the weakly
// active row.  kappa = +Inf: ym has the bits of yf (nothing finite reaches theta); kappa = 0: theta = 0 and ym = +0 everywhere.
// rho must be the rho of the update that wrote yf: behind a rebalance with no update after it y has been rescaled and no longer
// sits on the theta of either rho.
//
// Bound gradients of the soft box (gbdpcg_admm_soft_grad_bounds_*), az the adjoint's z, with sat = |yf| >= theta, every line ONE
// IEEE operation or a comparison:
//     glo = (yf < 0 && !sat) ? -(rho_b ya) : +0      ghi = (yf > 0 && !sat) ? -(rho_b ya) : +0      the bits of admm_grad_bounds on ym
//     gkappa = sat ? (yf > 0 ? az : -az) : +0        mu_r = sign(yf_r) kappa_r enters the stationarity like g: dl/dkappa_r = sign a_z,r
// each output may be null (not written).  The two gradient kernels share one body (grad_bounds, forced inline into both __global__
// entries); SOFT is its compile-time switch, and kappa, az, gkappa are arguments of the soft entry alone.
//
// Shape: that of admm_update_kernel -- ONE WORKGROUP PER PROBLEM, one wave when the problem has at most 256 elements, otherwise
// four, 64-bit problem strides, rho_b once per workgroup through the scalar cache, no LDS, no atomics, no scratch.  With every base
// pointer in use 16-byte aligned (vec != 0, decided by the host) a scalar head, a 16-byte body and a scalar tail (for_each_split in
// elementwise_split.hpp), otherwise every element through the scalar form; the same operations per element either way: the same
// bits.  The mask makes 3 element accesses per element (2 reads, 1 write), the hard gradients 2 reads and 2 writes, the soft ones 4
// reads and up to 3 writes.  One mask kernel serves the box (nz elements per problem) and the rows (nw).
#include "elementwise_split.hpp"
#include "ieee_once.hpp"
#include "internal.hpp"

namespace gbdpcg {

namespace {

// The body of the two gradient kernels.  SOFT: with kappa, az and gk, and every output may be null; otherwise those three are not
// looked at and glo, ghi are written unconditionally.
template <typename T, bool SOFT>
__device__ __forceinline__ void grad_bounds(uint64_t nz, uint32_t vec, const T *__restrict__ yf, const T *__restrict__ kappa,
                                            const T *__restrict__ rho, const T *__restrict__ ya, const T *__restrict__ az,
                                            T *__restrict__ glo, T *__restrict__ ghi, T *__restrict__ gk)
{
    using V = typename Vec16<T>::type;
    const uint32_t prob = blockIdx.x;
    const uint64_t off = (uint64_t)prob * nz;
    yf += off, ya += off;
    if constexpr (SOFT) kappa += off, az += off;
    if (!SOFT || glo) glo += off;
    if (!SOFT || ghi) ghi += off;
    if (SOFT && gk) gk += off;
    const T r = rho[prob];

    auto element = [&](T f, T k, T a, T z, T &lo, T &hi, T &gkap) {
        bool sat = false;
        if constexpr (SOFT) sat = soft_saturated(f, k, r);
        const T n = -(r * a);
        lo = (f < T(0) && !sat) ? n : T(0);
        hi = (f > T(0) && !sat) ? n : T(0);
        if constexpr (SOFT) gkap = sat ? (f > T(0) ? z : -z) : T(0);
    };

    for_each_split<T>(
        vec, off, nz,
        [&](uint64_t i) {
            T k = T(0), z = T(0), lo, hi, gkap = T(0);
            if constexpr (SOFT) k = kappa[i], z = az[i];
            element(yf[i], k, ya[i], z, lo, hi, gkap);
            if (!SOFT || glo) glo[i] = lo;
            if (!SOFT || ghi) ghi[i] = hi;
            if (SOFT && gk) gk[i] = gkap;
        },
        [&](uint64_t i) {
            const V fv = load16(yf + i);
            V kv = {}, zv = {};
            if constexpr (SOFT) kv = load16(kappa + i);
            const V av = load16(ya + i);
            if constexpr (SOFT) zv = load16(az + i);
            V lv, hv, gv = {};
#pragma unroll
            for (uint32_t e = 0; e < Vec16<T>::N; ++e) {
                T lo, hi, gkap = T(0);
                element(fv[e], kv[e], av[e], zv[e], lo, hi, gkap);
                lv[e] = lo;
                hv[e] = hi;
                gv[e] = gkap;
            }
            if (!SOFT || glo) store16(glo + i, lv);
            if (!SOFT || ghi) store16(ghi + i, hv);
            if (SOFT && gk) store16(gk + i, gv);
        });
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void admm_soft_mask_kernel(uint64_t len, uint32_t vec, const T *__restrict__ yf,
                                                             const T *__restrict__ kappa, const T *__restrict__ rho,
                                                             T *__restrict__ ym)
{
    using V = typename Vec16<T>::type;
    const uint32_t prob = blockIdx.x;
    const uint64_t off = (uint64_t)prob * len;
    yf += off, kappa += off, ym += off;
    const T r = rho[prob];

    auto element = [&](T f, T k) { return soft_saturated(f, k, r) ? T(0) : f; };

    for_each_split<T>(
        vec, off, len, [&](uint64_t i) { ym[i] = element(yf[i], kappa[i]); },
        [&](uint64_t i) {
            const V fv = load16(yf + i), kv = load16(kappa + i);
            V mv;
#pragma unroll
            for (uint32_t e = 0; e < Vec16<T>::N; ++e) mv[e] = element(fv[e], kv[e]);
            store16(ym + i, mv);
        });
}

template <typename T>
__global__ __launch_bounds__(256) void admm_grad_bounds_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ yf,
                                                               const T *__restrict__ rho, const T *__restrict__ ya,
                                                               T *__restrict__ glo, T *__restrict__ ghi)
{
    grad_bounds<T, false>(nz, vec, yf, static_cast<const T *>(nullptr), rho, ya, static_cast<const T *>(nullptr), glo, ghi,
                          static_cast<T *>(nullptr));
}

template <typename T>
__global__ __launch_bounds__(256) void admm_soft_grad_bounds_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ yf,
                                                                    const T *__restrict__ kappa, const T *__restrict__ rho,
                                                                    const T *__restrict__ ya, const T *__restrict__ az,
                                                                    T *__restrict__ glo, T *__restrict__ ghi, T *__restrict__ gk)
{
    grad_bounds<T, true>(nz, vec, yf, kappa, rho, ya, az, glo, ghi, gk);
}

template <typename T>
hipError_t launch_admm_soft_mask(uint64_t len, uint32_t batch, const T *yf, const T *kappa, const T *rho, T *ym, hipStream_t s)
{
    if (batch > 0x7fffffffu || ym == yf) return hipErrorInvalidValue;   // one workgroup per problem; the unmasked yf is needed afterwards
    const uint32_t vec = all_aligned({yf, kappa, ym});
    const uint32_t threads = len <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_soft_mask_kernel<T>), dim3(batch), dim3(threads), 0, s, len, vec, yf, kappa, rho, ym);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_grad_bounds(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *yf, const T *rho, const T *ya, T *glo,
                                   T *ghi, hipStream_t s)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({yf, ya, glo, ghi});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_grad_bounds_kernel<T>), dim3(batch), dim3(threads), 0, s, nz, vec, yf, rho, ya, glo, ghi);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_soft_grad_bounds(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *yf, const T *kappa, const T *rho,
                                        const T *ya, const T *az, T *glo, T *ghi, T *gkappa, hipStream_t s)
{
    if (batch > 0x7fffffffu || (!glo && !ghi && !gkappa)) return hipErrorInvalidValue;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({yf, kappa, ya, az, glo, ghi, gkappa});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_soft_grad_bounds_kernel<T>), dim3(batch), dim3(threads), 0, s, nz, vec, yf, kappa, rho, ya, az, glo, ghi,
                       gkappa);
    return hipGetLastError();
}

template hipError_t launch_admm_soft_mask<float>(uint64_t, uint32_t, const float *, const float *, const float *, float *, hipStream_t);
template hipError_t launch_admm_soft_mask<double>(uint64_t, uint32_t, const double *, const double *, const double *, double *,
                                                  hipStream_t);
template hipError_t launch_admm_grad_bounds<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *, const float *,
                                                   float *, float *, hipStream_t);
template hipError_t launch_admm_grad_bounds<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *, const double *,
                                                    double *, double *, hipStream_t);
template hipError_t launch_admm_soft_grad_bounds<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                        const float *, const float *, const float *, float *, float *, float *,
                                                        hipStream_t);
template hipError_t launch_admm_soft_grad_bounds<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *,
                                                         const double *, const double *, const double *, double *, double *, double *,
                                                         hipStream_t);

}  // namespace gbdpcg
