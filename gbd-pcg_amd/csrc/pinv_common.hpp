// pinv_common.hpp -- what the three units of the Phi^-1 formation share (pinv.hip: the route, launch_form_pinv and the any-size LDS
// kernels; pinv_regs.hip: the compile-time-n two-pass kernels; pinv_fused.hip: the one-launch stair kernels): the synchronisation
// of a knot's threads, the device code more than one kernel runs, the route a shape takes and the walk over the size list.
// The device helpers are forced inline: no symbols, the same code in every kernel that used to spell them out.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "bt_device.hpp"
#include "internal.hpp"
#include "row16.hpp"

namespace gbdpcg {

constexpr int kPinvThreads = 256;

// Synchronise the GT threads that share one knot.
template <int GT> __device__ __forceinline__ void group_sync()
{
    if constexpr (GT == 64) wave_sync();
    else __syncthreads();
}

__device__ __forceinline__ uint32_t pinv_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint64_t pinv_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
__device__ __forceinline__ float lane_bcast(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ double lane_bcast(double v, int lane)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// The in-place Gauss-Jordan elimination of an n x n block held one column per lane of a 16-lane row (row16.hpp), as the kernels
// take it: the pivot's reciprocal is the division, and an odd n in fp32 takes the one-row-per-instruction loop.
template <int M, typename T> __device__ __forceinline__ void stair_invert(T (&col)[M], uint32_t l)
{
    row_eliminate<0, M, RcpDivide, false>(col, l);
}

// Pivot step j of the [D | I] tableau held one column per lane: cj is column j as every lane received it (a readlane broadcast
// in pinv_diag_reg_kernel, an LDS broadcast in pinv_diag_pair_kernel), col the lane's own column.
template <uint32_t n, typename T> __device__ __forceinline__ void tableau_pivot_step(T (&col)[n], const T (&cj)[n], uint32_t j)
{
    const T piv = T(1) / cj[j];
    const T pr = col[j] * piv;  // scaled pivot-row entry of this lane's column
#pragma unroll
    for (uint32_t r = 0; r < n; ++r) col[r] = (r == j) ? pr : fma_t(-cj[r], pr, col[r]);
}

// One 2 x 2 tile of a product of two n x n factors, n = 2 H: two rows of the first factor (a0, a1: contiguous, the factor is
// symmetric or stored transposed) and two columns of the second (b0, b1) feed four accumulators, half the LDS reads per FMA
// of one output per thread.  Every output sums q ascending, as the one-element loops do: the same bits.  tRC: row R, column C.
template <uint32_t H, typename T>
__device__ __forceinline__ void tile_product(const T *a0r, const T *a1r, const T *b0c, const T *b1c, T &t00, T &t01, T &t10, T &t11)
{
    using P2 = typename VecOf<T, 2>::type;
    const P2 *a0 = reinterpret_cast<const P2 *>(a0r), *a1 = reinterpret_cast<const P2 *>(a1r);
    const P2 *b0 = reinterpret_cast<const P2 *>(b0c), *b1 = reinterpret_cast<const P2 *>(b1c);
    t00 = T(0), t01 = T(0), t10 = T(0), t11 = T(0);
#pragma unroll
    for (uint32_t q = 0; q < H; ++q) {
        const P2 x0 = a0[q], x1 = a1[q], y0 = b0[q], y1 = b1[q];
        t00 = fma_t(x0.x, y0.x, t00); t00 = fma_t(x0.y, y0.y, t00);
        t01 = fma_t(x0.x, y1.x, t01); t01 = fma_t(x0.y, y1.y, t01);
        t10 = fma_t(x1.x, y0.x, t10); t10 = fma_t(x1.y, y0.y, t10);
        t11 = fma_t(x1.x, y1.x, t11); t11 = fma_t(x1.y, y1.y, t11);
    }
}

// Block sizes with compile-time formation kernels: the streaming kernels' list plus the odd sizes and 22, which otherwise take the
// runtime-n LDS kernels (stair of 1024 x 128 at n = 15: 1,093 us, at n = 22: 3,055 us).
#define GBDPCG_PINV_N(X) GBDPCG_SPECIALIZED_N(X) X(3) X(5) X(7) X(9) X(11) X(15) X(22)

// launch(NN) for the n of that list (a std::integral_constant<int, .>, so that NN() is a template argument); `unlisted` for
// every other n.
template <typename R, typename F> R pinv_dispatch_n(uint32_t n, R unlisted, F &&launch)
{
#define GBDPCG_X(NN) if (n == NN) return launch(std::integral_constant<int, NN>{});
    GBDPCG_PINV_N(GBDPCG_X)
#undef GBDPCG_X
    return unlisted;
}

// The kernels a shape takes (pinv_route in pinv.hip decides; tests/pinv_ref.py restates it line for line).
enum class PinvFamily {
    mfma,         // pinv_stair_mfma_kernel: the stair in one launch, fp32, products on the matrix cores
    fused,        // pinv_stair_fused_kernel: the stair in one launch
    quad,         // pinv_diag_quad_kernel, then pinv_stair_reg_kernel
    pair,         // pinv_diag_pair_kernel (+ pinv_stair_reg_kernel for the stair)
    reg,          // pinv_diag_reg_kernel (+ pinv_stair_reg_kernel)
    wide,         // pinv_diag_wide_kernel (+ pinv_stair_wide_kernel)
    lds64,        // pinv_diag_kernel<64, 16> (+ pinv_stair_kernel<64>): any n, one wavefront per knot
    lds256,       // pinv_diag_kernel<256, 16> (+ pinv_stair_kernel<256>): one workgroup per knot
    lds256_long,  // pinv_diag_kernel<256, 64> (+ pinv_stair_kernel<256>)
    refused
};
struct PinvRoute {
    PinvFamily family;
    uint32_t chunks;  // workgroups per problem of the one-launch families (one verdict byte each), else 0
};
PinvRoute pinv_route(size_t elem_size, uint32_t n, uint32_t N, int kind, bool s_aligned16, bool verdicts_wanted);

// pinv_regs.hip: the families quad, pair, reg and wide.  pinv_fused.hip: mfma and fused.
template <typename T>
hipError_t launch_pinv_regs(PinvFamily family, uint32_t n, uint32_t N, uint32_t batch, const T *S, T *Pinv, int kind, hipStream_t s);
template <typename T>
hipError_t launch_pinv_fused(PinvRoute route, uint32_t n, uint32_t N, uint32_t batch, const T *S, T *Pinv, hipStream_t s,
                             uint8_t *verdicts, bool s_symmetric);

}  // namespace gbdpcg
