// pcg_persist_geom.hpp -- what the two persistent kernels (pcg_persist_2r.hpp, pcg_persist_1r.hpp) share inside a CU: the lane
// map of a knot, the row product, which columns of a block-row a thread keeps; and the thread coordinates of the two-reduction kernel.
#pragma once

#include "pcg_persist_handoff.hpp"

namespace gbdpcg {

// acc = sum_i m[i] * (A[i] + coef * B[i]) over this thread's COLS columns, ascending.  The operands come out of LDS
// in 16-byte pieces, STEP columns per step.  FENCED (three knots per workgroup: 960 threads, 128 VGPRs): the steps are
// pinned in order, because left alone hipcc hoists all 2 * COLS reads above the first multiply and spills; with fewer
// threads the hoisting is what we want (one LDS latency per product instead of one per step).
template <typename T, uint32_t COLS, bool FENCED, bool ALIGNED = true>
__device__ __forceinline__ T persist_row_dot(const T (&m)[COLS], const T *A, const T *B, T coef)
{
    T acc = T(0);
    if constexpr (ALIGNED) {
        constexpr uint32_t VW = 16 / sizeof(T), STEP = COLS % 4 == 0 ? 4 : VW;
        static_assert(COLS % STEP == 0 && STEP % VW == 0, "columns per thread come in whole 16-byte pieces");
        typedef T vec_t __attribute__((ext_vector_type(VW)));
#pragma unroll
        for (uint32_t i0 = 0; i0 < COLS; i0 += STEP) {
            T av[STEP], bv[STEP];
#pragma unroll
            for (uint32_t q = 0; q < STEP / VW; ++q) {
                const vec_t va = *reinterpret_cast<const vec_t *>(A + i0 + q * VW), vb = *reinterpret_cast<const vec_t *>(B + i0 + q * VW);
#pragma unroll
                for (uint32_t e = 0; e < VW; ++e) {
                    av[q * VW + e] = va[e];
                    bv[q * VW + e] = vb[e];
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < STEP; ++j) acc = fma_t(m[i0 + j], fma_t(coef, bv[j], av[j]), acc);
            if (FENCED) __builtin_amdgcn_sched_barrier(0);
        }
    } else {   // block sizes whose rows are not multiples of 16 bytes (n = 14 in fp32): element-wise LDS reads
#pragma unroll
        for (uint32_t i = 0; i < COLS; ++i) acc = fma_t(m[i], fma_t(coef, B[i], A[i]), acc);
    }
    return acc;
}

// Sum over the 8 lanes of an aligned group, in the VALU (DPP quad permutes + half mirror): every lane gets the total.
template <typename T> __device__ __forceinline__ T group_sum8(T v)
{
    v = dpp_add<0xB1>(v);    // quad_perm:[1,0,3,2]
    v = dpp_add<0x4E>(v);    // quad_perm:[2,3,0,1]
    return dpp_add<0x141>(v);  // row_half_mirror
}

// Diagnostic build only (-DGBDPCG_PERSIST_STAMPS): workgroup 1 leaves cycle stamps of the phases of iteration 3 in the
// unused control words of the workspace (read back by tools/persist_stamps.py).  No stamp exists in the shipped build.
#ifdef GBDPCG_PERSIST_STAMPS
#define GBDPCG_STAMP(IDX, COND)                                                                   \
    if ((COND) && lane == 0) ws[IDX] = __builtin_amdgcn_s_memtime();
#define GBDPCG_STAMP_RT(IDX, COND)                                                                \
    if ((COND) && lane == 0) ws[IDX] = __builtin_amdgcn_s_memrealtime();
// every workgroup's 100 MHz real-time clock at its publish (0) and at the end of its sweep (1), into the second halo region
#define GBDPCG_XSTAMP(WHICH, COND)                                                                \
    if ((COND) && lane == 0) (ws + kPersistCtrl + persist_part_words<T>(N) + persist_halo_words<T>(n, N))[2 * w + (WHICH)] = __builtin_amdgcn_s_memrealtime();
#else
#define GBDPCG_STAMP(IDX, COND)
#define GBDPCG_STAMP_RT(IDX, COND)
#define GBDPCG_XSTAMP(WHICH, COND)
#endif

// Lane map of one knot: aligned groups of 8 lanes share a row, lane g of the group holds columns [g*COLS, (g+1)*COLS) of
// that row of S and of Pinv in registers; a wave covers 8 rows, ceil(n/8) waves a knot (n = 36: 5 waves, 14 columns per
// lane, 56 VGPRs of fp64 matrix data).  The 8 partial sums of a row are folded with three DPP adds, so a product needs
// no LDS round trip and no barrier of its own.
template <typename T, int NCT> struct PersistGeom {
    static constexpr uint32_t n = NCT, G = 8, WPK = (n + 7) / 8, TPK = WPK * 64, VW = 16 / sizeof(T);
    static constexpr uint32_t CPL = (3 * n + G - 1) / G;   // columns per lane
    // 16-byte operand reads need the knots of a window and the lanes' column runs on 16-byte boundaries
    static constexpr bool ALIGNED = (n * sizeof(T)) % 16 == 0 && ((CPL + VW - 1) / VW * VW * sizeof(T)) % 16 == 0;
    static constexpr uint32_t COLS = ALIGNED ? (CPL + VW - 1) / VW * VW : CPL;
};


// Where a thread sits in its workgroup and the workgroup in its problem.  Workgroup w of the problem owns knots k0 .. k0 + K - 1;
// this thread works on row `row` of knot k (its `slot`-th), columns cbase .. cbase + COLS - 1 of the block-row.
struct PersistCoords {
    uint32_t tid, lane, wave, slot, g, row, cbase, prob, w, k0, k;
    bool row_live;
};
template <typename T, int NCT, int K> __device__ __forceinline__ PersistCoords persist_coords(uint32_t W)
{
    using Gm = PersistGeom<T, NCT>;
    PersistCoords c;
    c.tid = threadIdx.x;
    c.lane = c.tid & 63u;
    c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6);
    c.slot = c.wave / Gm::WPK;
    c.g = c.lane & 7u;
    c.row = (c.wave - c.slot * Gm::WPK) * 8 + (c.lane >> 3);
    c.row_live = c.row < Gm::n;
    c.cbase = c.g * Gm::COLS;
    // chunk index: blocks b and b + 8 share an XCD (round-robin dispatch), so consecutive chunks -- the ones that
    // exchange halo knots -- are put on one XCD.  Speed only: the protocol does not depend on placement.
    c.prob = blockIdx.x / W;
    const uint32_t b = blockIdx.x - c.prob * W;
    c.w = (W % 8 == 0) ? (b % 8) * (W / 8) + b / 8 : b;
    c.k0 = c.w * K;
    c.k = c.k0 + c.slot;
    return c;
}

// Is column c of the block-row [L|D|R] of knot kk a stored entry this thread keeps?  L_0 and R_{N-1} are never used
// (pcg.cuh:105-106) and knots outside [0, N) do not exist: zero, whatever the storage holds.  KI: uint32_t, or int64_t where
// a knot left of the first can be asked for.
template <uint32_t n, typename KI> __device__ __forceinline__ bool persist_col_ok(KI kk, uint32_t c, bool row_live, uint32_t N)
{
    return row_live && kk >= 0 && kk < (KI)N && c < 3 * n && !(kk == 0 && c < n) && !(kk == (KI)N - 1 && c >= 2 * n);
}

}  // namespace gbdpcg
