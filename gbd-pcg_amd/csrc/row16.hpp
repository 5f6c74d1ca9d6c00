// row16.hpp -- what the kernels that put one small block (or one knot) into each 16-lane row of a wavefront share: the DPP row
// broadcast, the products that ride on it, and one pivot step of the in-place Gauss-Jordan elimination of a block held one
// column per lane.  Used by schur.hip, schur_ginv.hip, schur_residual.hip (the four-knots-per-wave kernels) and pinv_regs.hip / pinv_fused.hip (the
// quarter-wave and one-launch stair kernels).  Everything here is forced inline: no symbols, the same code in every unit.
#pragma once
#include <cstdint>

#include "bt_device.hpp"

namespace gbdpcg {

// The value lane J of every 16-lane row holds, in all lanes of that row: the DPP control row_newbcast (gfx90a and later) --
// a VALU move, no trip through the LDS crossbar (ds_swizzle in bit-mask mode does the same at an LDS instruction's cost:
// 294 of them per step and wave of the formation kernel, on a pipe the four waves of a compute unit share).
template <int J> __device__ __forceinline__ float row_bcast(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + J, 0xf, 0xf, true));
}
template <int J> __device__ __forceinline__ double row_bcast(double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), 0x150 + J, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x150 + J, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
// acc += coef[q] * (v of lane q of the row), q = Q0 .. QN-1 in ascending order: a dot product whose vector sits one entry per lane.
template <int Q0, int QN, int M, typename T> __device__ __forceinline__ void recover_dot(T &acc, const T (&coef)[M], T v)
{
    if constexpr (Q0 < QN) {
        acc = fma_t(coef[Q0], row_bcast<Q0>(v), acc);
        recover_dot<Q0 + 1, QN, M>(acc, coef, v);
    }
}
// acc[r] += (src[r] of lane q of the row) * coef[q] for q in [Q0, QN): a block product whose left factor lives one column per
// lane and whose right factor's column this lane holds in coef -- the broadcast rides on the fma as a DPP operand.
// (v_fmac_*_dpp written out: hipcc pairs the fmas into v_pk_fma_f32, which takes no DPP operand, and keeps a v_mov_b32_dpp per
// element next to them.  A VGPR a DPP operand reads must not have been written by the two preceding VALU instructions;
// the compiler does not look into asm for that, so every chain starts behind an s_nop and reads registers no instruction of
// the chain writes.)
template <int J> __device__ __forceinline__ void fmac_bcast(float &acc, float src, float coef)
{
    asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(coef), "n"(J));
}
template <int J> __device__ __forceinline__ void fmac_bcast(double &acc, double src, double coef)
{
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(coef), "n"(J));
}
template <int Q0, int QN, int M, int K, typename T>
__device__ __forceinline__ void bcast_mac_chain(const T (&src)[M], const T (&coef)[K], T (&acc)[M])
{
    if constexpr (Q0 < QN) {
#pragma unroll
        for (int r = 0; r < M; ++r) fmac_bcast<Q0>(acc[r], src[r], coef[Q0]);
        bcast_mac_chain<Q0 + 1, QN, M, K>(src, coef, acc);
    }
}
template <int Q0, int QN, int M, int K, typename T>
__device__ __forceinline__ void bcast_mac(const T (&src)[M], const T (&coef)[K], T (&acc)[M])
{
    asm volatile("s_nop 1");
    bcast_mac_chain<Q0, QN, M, K>(src, coef, acc);
}

// The two reciprocals a pivot is taken with.  They give different bits in fp32, and each caller keeps the one its results were
// pinned with: the formation kernels RcpNewton, the preconditioner kernels RcpDivide.
struct RcpDivide {
    template <typename T> static __device__ __forceinline__ T of(T x) { return T(1) / x; }
};
// The hardware reciprocal and one Newton step in fp32 (the division sequence is a dozen dependent instructions on the critical
// path of every pivot step), the division in fp64.
struct RcpNewton {
    static __device__ __forceinline__ float of(float x)
    {
        const float r = __builtin_amdgcn_rcpf(x);
        return fma_t(fma_t(-x, r, 1.0f), r, r);
    }
    static __device__ __forceinline__ double of(double x) { return 1.0 / x; }
};

// Pivot step J of the in-place Gauss-Jordan elimination of an M x M block held one column per lane (l: the lane's place in
// its row of 16): lane c < M owns column c.  The identity half of a [D | I] tableau is never stored: its column J stays e_J
// until step J and is created in that step in the place of column J of D, so lane J computes
// (r == J ? piv : fma(-cj[r], piv, 0)) -- what the tableau lane M + J computes from e_J -- and every other lane the usual
// update: pr = col[J] / pivot, col[r] = fma(-cj[r], pr, col[r]).
// fp32 takes two rows per instruction: the pivot lane's "start from zero" is a packed multiply by 0 or 1 (exact) instead of a
// select per row, the update a packed fma -- the same fma on the same numbers as the scalar loop, element for element.
// PACK_ODD: what an odd M does in fp32 -- true: pairs, then the last row alone (the formation kernels); false: the scalar loop
// (the preconditioner kernels).  The results are the same numbers; the instructions are not -- with true everywhere the seven
// pinv_diag_quad_kernel<float, odd n> change -- so each caller keeps the ones it was measured with.  One flag, not to be "fixed"
// without timing those kernels.
template <int J, int M, typename RCP, bool PACK_ODD, typename T> __device__ __forceinline__ void row_pivot(T (&col)[M], uint32_t l)
{
    T cj[M];
#pragma unroll
    for (int r = 0; r < M; ++r) cj[r] = row_bcast<J>(col[r]);
    const T piv = RCP::of(cj[J]);   // (before the compare: the register allocation of two fp64 kernels follows the order of these lines)
    const bool is_j = l == (uint32_t)J;
    const T pr = is_j ? piv : col[J] * piv;
    if constexpr (sizeof(T) == 4 && (M % 2 == 0 || PACK_ODD)) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const float keep = is_j ? 0.0f : 1.0f;
        const f2 kk = {keep, keep}, npr = {-pr, -pr};
#pragma unroll
        for (int r = 0; r + 1 < M; r += 2) {
            const f2 c = {col[r], col[r + 1]}, b = {cj[r], cj[r + 1]};
            const f2 v = __builtin_elementwise_fma(b, npr, c * kk);
            col[r] = v.x;
            col[r + 1] = v.y;
        }
        if constexpr (M & 1) col[M - 1] = fma_t(-cj[M - 1], pr, is_j ? T(0) : col[M - 1]);
        col[J] = pr;
    } else {
#pragma unroll
        for (int r = 0; r < M; ++r) col[r] = (r == J) ? pr : fma_t(-cj[r], pr, is_j ? T(0) : col[r]);
    }
}
// Steps J .. M-1 in a row: the whole elimination from J = 0.
template <int J, int M, typename RCP, bool PACK_ODD, typename T> __device__ __forceinline__ void row_eliminate(T (&col)[M], uint32_t l)
{
    if constexpr (J < M) {
        row_pivot<J, M, RCP, PACK_ODD>(col, l);
        row_eliminate<J + 1, M, RCP, PACK_ODD>(col, l);
    }
}

}  // namespace gbdpcg
