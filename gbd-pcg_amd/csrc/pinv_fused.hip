// pinv_fused.hip -- the STAIR kind of Phi^-1 formation in ONE launch, for even n <= 16: pinv_stair_fused_kernel (both
// precisions) and its fp32 form around LDS-DMA and the matrix cores, pinv_stair_mfma_kernel.  They are the only kernels that
// report symmetry verdicts.  pinv.hip holds the route that picks one of them; launch_pinv_fused starts it.
#include "pinv_common.hpp"

#ifndef GBDPCG_PINV_SKIP
#define GBDPCG_PINV_SKIP 0     // timing builds of pinv_stair_mfma_kernel (WRONG results): 1 no elimination, 2 no products, 4 no stores
#endif

namespace gbdpcg {

// A workgroup inverts the diagonal blocks of 16 consecutive knots of
// one problem (four per wavefront, pinv_diag_quad_kernel's in-place elimination), keeps the mirrored inverses
// in LDS and evaluates the 15 stair pairs between them from there -- the D^-1 blocks are neither re-read from
// memory nor waited for across a launch boundary.  Consecutive workgroups overlap by one knot (inverted
// twice, written once).  Same operations, same bits as the two-pass form.
// verdicts (optional): one byte per workgroup, 1 when every pair of the chunk had L_{k+1} == R_k^T bit for bit
// in S -- the pairs of Pinv were then written as mirror images, so the same holds for Pinv and a solve that
// follows needs no symmetry test of its own (gbdpcg_form_pinv_solve_*).  Written unconditionally.
// S_SYM: the caller KNOWS L_{k+1} == R_k^T in S (gbdpcg_kkt_step_*): L is never read.  A compile-time switch: as a kernel argument
// the same test cost the ordinary path 40 us of 150 (the compiler's schedule of the pair loop changed).
// (Held to 64 registers -- eight waves per SIMD instead of six, amdgpu_waves_per_eu(8) -- it spills 10 registers and takes 208 us
// instead of 162 for the 1024 x 128 batch: measured in round 3, dropped.)
template <typename T, int NCT, bool S_SYM>
__global__ __launch_bounds__(kPinvThreads) void pinv_stair_fused_kernel(uint32_t N, uint32_t chunks, const T *__restrict__ S,
                                                                       T *__restrict__ Pinv, uint8_t *__restrict__ verdicts)
{
    constexpr bool s_symmetric = S_SYM;
    constexpr uint32_t n = NCT, nn = n * n, H = n / 2, PAIRS = 15;
    static_assert(n <= 16 && n % 2 == 0, "quarter-wave elimination and 2 x 2 tiles");
    __shared__ __attribute__((aligned(16))) T inv[16][nn];      // mirrored D^-1 of knots k0 .. k0+15
    __shared__ __attribute__((aligned(16))) T work[4][2][nn];   // per wave: B (R_k or L_{k+1}^T) and W^T
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, quarter = lane >> 4, l = lane & 15u;
    const uint32_t prob = blockIdx.x / chunks, chunk = blockIdx.x - prob * chunks;
    const uint32_t k0 = chunk * PAIRS;
    const size_t pbase = (size_t)prob * 3 * nn * N;

    {   // ---- pass 1: invert D_{k0 + slot}, slot = 4 wave + quarter
        const uint32_t slot = wave * 4 + quarter, k = k0 + slot;
        const bool alive = k < N, owner = l < n;
        const T *D = S + pbase + (size_t)(alive ? k : 0) * 3 * nn + nn;
        T col[n];
#pragma unroll
        for (uint32_t r = 0; r < n; ++r) col[r] = (!alive || !owner) ? (r == l ? T(1) : T(0)) : D[l * n + r];
        stair_invert<(int)n>(col, l);
        if (owner) {  // mirrored on the way into LDS: element (r, c) with r > c takes the value of (c, r).  (Written out here and in
            // pinv_stair_mfma_kernel, leading dimension LD there: as one shared helper the two loops changed the instruction
            // stream of all 38 instantiations of the two kernels -- profiles/r16_pinv_split.txt.)
#pragma unroll
            for (uint32_t r = 0; r < n; ++r)
                if (r <= l) inv[slot][l * n + r] = col[r];       // upper triangle of column l, as computed
#pragma unroll
            for (uint32_t r = 0; r < n; ++r)
                if (r < l) inv[slot][r * n + l] = col[r];        // its mirror image: (l, r) := (r, l)
        }
    }
    __syncthreads();

    // ---- D slots: this workgroup owns knots k0 .. k0+14, and N-1 if it is the last.  D'_k leaves with R'_k and L'_{k+1} of its
    // pair below -- the three are one contiguous run of 3 n^2 elements, and memory that sees D' now and the other two blocks of
    // the row ten microseconds later pays for the row twice.  Here: the knot that ends the problem (it starts no pair) and the
    // two corner blocks nobody reads.
    const uint32_t own_end = (chunk == chunks - 1) ? N : min(N, k0 + PAIRS);
    if (own_end == N) {
        T *o = Pinv + pbase + (size_t)(N - 1) * 3 * nn;
        for (uint32_t i = threadIdx.x; i < nn; i += kPinvThreads) {
            o[nn + i] = inv[N - 1 - k0][i];
            o[2 * nn + i] = T(0);
        }
    }
    if (k0 == 0)
        for (uint32_t i = threadIdx.x; i < nn; i += kPinvThreads) Pinv[pbase + i] = T(0);

    // ---- pass 2: pairs (k, k+1), k = k0 + j, j = wave, wave + 4, ...
    T *B = work[wave][0], *Wt = work[wave][1];
    const uint32_t tr = lane / H, tc = lane - tr * H, r0 = 2 * tr, c0 = 2 * tc;
    const bool tile = lane < H * H;
    constexpr uint32_t EPL = (nn + 63) / 64;
    bool any_asymmetric = false;
    for (uint32_t j = wave; j < PAIRS && k0 + j + 1 < N; j += 4) {
        const uint32_t k = k0 + j;
        const T *A = inv[j], *C = inv[j + 1];
        const size_t blk = pbase + (size_t)k * 3 * nn, nb = blk + (size_t)3 * nn;
        // Both blocks are read as they lie in memory (a lane-strided read of L_{k+1}^T costs the address unit one cache line
        // per lane: with the strided R' stores below, that was most of this phase) and L_{k+1} is transposed through LDS.
        T lt[EPL];
        bool differs = false;
#pragma unroll
        for (uint32_t q = 0; q < EPL; ++q) {
            const uint32_t i = lane + 64 * q;
            if (i < nn) {
                B[i] = S[blk + 2 * (size_t)nn + i];   // R_k(r,c) at c n + r
                if (!s_symmetric) Wt[i] = S[nb + i];  // L_{k+1}, as stored (not read at all when the caller knows S symmetric)
            }
        }
        group_sync<64>();
#pragma unroll
        for (uint32_t q = 0; q < EPL; ++q) {
            const uint32_t i = lane + 64 * q;
            lt[q] = T(0);
            if (i < nn && !s_symmetric) {
                const uint32_t c = i / n, r = i - c * n;
                lt[q] = Wt[r * n + c];                // L_{k+1}(c,r)
                differs |= pinv_bits(B[i]) != pinv_bits(lt[q]);
            }
        }
        const bool symmetric = s_symmetric || __builtin_amdgcn_ballot_w64(differs) == 0;  // wave-uniform
        any_asymmetric |= !symmetric;
        group_sync<64>();
        for (int pass = 0; pass < (symmetric ? 1 : 2); ++pass) {
            if (pass == 1) {
#pragma unroll
                for (uint32_t q = 0; q < EPL; ++q) {
                    const uint32_t i = lane + 64 * q;
                    if (i < nn) B[i] = lt[q];
                }
                group_sync<64>();
            }
            if (tile) {
                T w00, w01, w10, w11;
                tile_product<H>(A + r0 * n, A + (r0 + 1) * n, B + c0 * n, B + (c0 + 1) * n, w00, w01, w10, w11);
                Wt[r0 * n + c0] = w00; Wt[r0 * n + c0 + 1] = w01;
                Wt[(r0 + 1) * n + c0] = w10; Wt[(r0 + 1) * n + c0 + 1] = w11;
            }
            group_sync<64>();
            if (tile) {
                T x00, x01, x10, x11;
                tile_product<H>(Wt + r0 * n, Wt + (r0 + 1) * n, C + c0 * n, C + (c0 + 1) * n, x00, x01, x10, x11);
                // -X' into LDS in the layout of R' (column c0 of X' = row c0 of X ...): R'_k(r,c) = -X(c,r) at c n + r
                Wt[c0 * n + r0] = -x00; Wt[c0 * n + r0 + 1] = -x10;
                Wt[(c0 + 1) * n + r0] = -x01; Wt[(c0 + 1) * n + r0 + 1] = -x11;
            }
            group_sync<64>();
            {   // dense stores: R'_k as it lies in Wt, L'_{k+1}(c,r) = R'_k(r,c) read transposed
                T *Rp = Pinv + blk + 2 * (size_t)nn, *Lp = Pinv + nb;
#pragma unroll
                for (uint32_t q = 0; q < EPL; ++q) {
                    const uint32_t i = lane + 64 * q;
                    if (i < nn) {
                        const uint32_t c = i / n, r = i - c * n;
                        if (pass == 0) {
                            Rp[i - (size_t)nn] = A[i];   // D'_k: the block in front of R'_k
                            Rp[i] = Wt[i];
                        }
                        if (pass == 1 || symmetric) Lp[i] = Wt[r * n + c];
                    }
                }
            }
            group_sync<64>();
        }
    }
    if (verdicts) {  // uniform branch: every wave reaches the barrier
        const int bad = __syncthreads_or(any_asymmetric ? 1 : 0);
        if (threadIdx.x == 0) verdicts[(size_t)prob * chunks + chunk] = bad ? 0 : 1;
    }
}

// (Used for stateSize 16, where the VALU products of the kernel above are the bound: 264 -> 180 us per 1024 x 128 knots.  At 14 and
// 12 the two kernels tie within the box-to-box spread -- neither is bound by its vector work there -- and the older kernel stays.
// GBDPCG_PINV_MFMA_FROM=<n> moves the threshold for A/B runs.)
// The one-launch stair for fp32, rebuilt around what the counters of the kernel above say (profiles/r03_pinv_ab.txt): it ran at
// half the HBM rate with NOTHING saturated -- vector pipes 47-64 % busy, LDS 28 %, 14 GB/s per compute unit -- because every wave
// walks a chain of dependent round trips (D blocks in, eliminate, then four pairs: R / L in, two products, results out) with a
// kilobyte or two in flight.  Two changes:
//   * ONE request per workgroup.  Everything a workgroup reads -- D_k0 .. D_k0+15 and the R_k / L_k+1 blocks between them -- is one
//     contiguous run of 46 n^2 elements of S.  It is pulled into LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave
//     instruction, no registers) before anything else happens: 36 KB in flight per workgroup, 108 KB per compute unit, and no
//     memory read after it.  Pass 1 and the pair phase read their operands where the DMA put them.
//   * The two n x n x n products of a pair on the MATRIX cores (v_mfma_f32_16x16x4_f32: exact fp32, an fma chain over k --
//     cdna_hip_programming.md, "FP32-input MFMA"): 12 MFMAs per pair (32 cycles of the matrix pipe each, 8 of
//     vector issue) instead of 2 x 56 fma + 56 LDS reads per lane.  The mirrored inverses lie in LDS as zero-padded 16 x 16
//     images (16-float rows): the operand of lane (i, q = lane / 16), A[i][4q .. 4q+3], is ONE ds_read_b128 and k = 4q + kk is
//     the k of MFMA step kk in both operands.  B (R_k, or L_{k+1}^T in the second pass of an asymmetric pair) is read straight
//     from the raw run; its k = 14, 15 "pads" are whatever follows in the run (finite matrix data) and meet the zero pads of
//     the inverse.  T1 = B^T Dk^-1 leaves W = Dk^-1 B in the registers as W[j][4q + i] on lane (j, q): exactly the A operand of
//     X = W Dk1^-1 and the B operand of X^T = Dk1^-1 W^T, so both orientations of the result come out of four more MFMAs
//     each without any lane movement: X^T (lane = row of X) is stored as R'_k, X (lane = column of X) as L'_{k+1} -- 56-byte
//     runs per quarter and register, no transposition through LDS.  Both chains multiply the same pairs of numbers in the same
//     k order (Dk1^-1 is mirrored exactly), so R'_k and L'_{k+1} are bit-for-bit transposes whenever S was: the property the
//     symmetric solve kernels rely on.
// Pass 1 (the inversions) is the DPP Gauss-Jordan of the kernel above; so are the verdict bytes and S_SYM.  S must be 16-byte
// aligned (the route checks).  54 KB of LDS per workgroup (n = 14): three workgroups per compute unit.
typedef float mf_f32x4 __attribute__((ext_vector_type(4)));
typedef float mf_f32x2 __attribute__((ext_vector_type(2)));

template <int NCT, bool S_SYM>
__global__ __launch_bounds__(kPinvThreads) void pinv_stair_mfma_kernel(uint32_t N, uint32_t chunks, const float *__restrict__ S,
                                                                      float *__restrict__ Pinv, uint8_t *__restrict__ verdicts)
{
    constexpr bool s_symmetric = S_SYM;
    constexpr uint32_t n = NCT, nn = n * n, PAIRS = 15, LD = 20, IMG = n * LD;   // images: n rows of 20 floats (16 used: 64-bank-friendly stride)
    static_assert(n <= 16 && n % 2 == 0, "quarter-wave elimination, 16 x 16 MFMA images, 16-byte blocks");
    constexpr uint32_t RAW = 46 * nn;                                  // D_k0 .. D_k0+15 with the R / L blocks between them
    constexpr uint32_t PIECES = RAW / 4, ROUNDS = (PIECES + kPinvThreads - 1) / kPinvThreads;   // 16-byte pieces, per-thread rounds
    __shared__ __attribute__((aligned(16))) float raw[RAW + 8];        // (+8: the k = 14, 15 over-read of the last block)
    __shared__ __attribute__((aligned(16))) float inv[16][IMG];        // mirrored D^-1 of knots k0 .. k0+15, (r, c) at r * 20 + c
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u, quarter = lane >> 4, l = lane & 15u;
    const uint32_t prob = blockIdx.x / chunks, chunk = blockIdx.x - prob * chunks;
    const uint32_t k0 = chunk * PAIRS;
    const size_t pbase = (size_t)prob * 3 * nn * N;

    {   // ---- the workgroup's whole input, one request: pieces past the end of the problem re-read its last piece (never used)
        const size_t g0 = pbase + (size_t)k0 * 3 * nn + nn;            // D_k0
        const size_t left = (size_t)3 * nn * N - ((size_t)k0 * 3 * nn + nn);   // elements from there to the end of the problem
        const uint32_t have = left / 4 < PIECES ? (uint32_t)(left / 4) : PIECES;
        const float *src = S + g0;
#pragma unroll
        for (uint32_t rd = 0; rd < ROUNDS; ++rd) {
            const uint32_t piece = rd * kPinvThreads + wave * 64 + lane;
            const uint32_t off = (piece < have ? piece : have - 1u) * 16u;
            const uint32_t dst = (uint32_t)(uintptr_t)raw + (rd * kPinvThreads + wave * 64) * 16u;   // wave-uniform; the lane's 16 bytes follow
            if (piece < PIECES) {   // (lanes past the run are masked off: an inactive lane of an LDS-DMA writes nothing)
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "s"(src), "v"(off), "s"(dst) : "memory");
            }
        }
        if (threadIdx.x < 8) raw[RAW + threadIdx.x] = 0.f;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    {   // ---- pass 1: invert D_{k0 + slot}, slot = 4 wave + quarter
        const uint32_t slot = wave * 4 + quarter, k = k0 + slot;
        const bool alive = k < N, owner = l < n;
        const float *D = raw + slot * 3 * nn;
        float col[n];
#pragma unroll
        for (uint32_t r = 0; r < n; ++r) col[r] = (!alive || !owner) ? (r == l ? 1.f : 0.f) : D[l * n + r];
#if !(GBDPCG_PINV_SKIP & 1)
        stair_invert<(int)n>(col, l);
#endif
        if (owner) {  // mirrored on the way into LDS, as in the kernel above
#pragma unroll
            for (uint32_t r = 0; r < n; ++r)
                if (r <= l) inv[slot][l * LD + r] = col[r];       // upper triangle of column l, as computed
#pragma unroll
            for (uint32_t r = 0; r < n; ++r)
                if (r < l) inv[slot][r * LD + l] = col[r];        // its mirror image: (l, r) := (r, l)
        }
        // zero pads: columns n .. 15 of the image (what they meet in the other operand is finite, so the sum is exact)
        if constexpr (n < 16) {
            if (owner) {
#pragma unroll
                for (uint32_t c = n; c < 16; ++c) inv[slot][l * LD + c] = 0.f;
            }
        }
    }
    __syncthreads();

    // ---- D slots of the knot that ends the problem and the two corner blocks nobody reads (see the kernel above)
    const uint32_t own_end = (chunk == chunks - 1) ? N : min(N, k0 + PAIRS);
    if (own_end == N) {
        float *o = Pinv + pbase + (size_t)(N - 1) * 3 * nn;
        for (uint32_t i = threadIdx.x; i < nn; i += kPinvThreads) {
            const uint32_t c = i / n, r = i - c * n;
            o[nn + i] = inv[N - 1 - k0][c * LD + r];
            o[2 * nn + i] = 0.f;
        }
    }
    if (k0 == 0)
        for (uint32_t i = threadIdx.x; i < nn; i += kPinvThreads) Pinv[pbase + i] = 0.f;

    // ---- pass 2: pairs (k, k+1), k = k0 + j, j = wave, wave + 4, ...: nothing but LDS reads, MFMAs and stores
    constexpr uint32_t EPL = (nn + 63) / 64;
    const uint32_t lc = l < n ? l : n - 1;   // lanes 14, 15 of a quarter compute rows / columns nobody stores: any finite operand
    bool any_asymmetric = false;
    for (uint32_t j = wave; j < PAIRS && k0 + j + 1 < N; j += 4) {
        const uint32_t k = k0 + j;
        const float *A = inv[j], *C = inv[j + 1];
        const float *Rk = raw + j * 3 * nn + nn, *Lk1 = Rk + nn;          // R_k(r,c) at c n + r, L_{k+1}(r,c) likewise
        const size_t blk = pbase + (size_t)k * 3 * nn, nb = blk + (size_t)3 * nn;
        bool differs = false;
        if (!s_symmetric) {
#pragma unroll
            for (uint32_t q = 0; q < EPL; ++q) {
                const uint32_t i = lane + 64 * q;
                if (i < nn) {
                    const uint32_t c = i / n, r = i - c * n;
                    differs |= pinv_bits(Rk[i]) != pinv_bits(Lk1[r * n + c]);   // R_k(r,c) against L_{k+1}(c,r)
                }
            }
        }
        const bool symmetric = s_symmetric || __builtin_amdgcn_ballot_w64(differs) == 0;  // wave-uniform
        any_asymmetric |= !symmetric;
        // the D'_k block goes out in front of R'_k (one contiguous run of the row)
        {
            float *Dp = Pinv + blk + (size_t)nn;
#pragma unroll
            for (uint32_t q = 0; q < EPL; ++q) {
                const uint32_t i = lane + 64 * q;
                if (i < nn) {
                    const uint32_t c = i / n, r = i - c * n;
#if GBDPCG_PINV_SKIP & 4
                    if (A[c * LD + r] == 1.2345f)
#endif
                    Dp[i] = A[c * LD + r];
                }
            }
        }
        const mf_f32x4 a4 = *reinterpret_cast<const mf_f32x4 *>(A + lc * LD + 4 * quarter);   // Dk^-1 (4q + kk, l), symmetric
        const mf_f32x4 c4 = *reinterpret_cast<const mf_f32x4 *>(C + lc * LD + 4 * quarter);   // Dk1^-1 (l, 4q + kk) = (4q + kk, l)
        for (int pass = 0; pass < (symmetric ? 1 : 2); ++pass) {
            mf_f32x4 b4;   // B(4q + kk, l): B = R_k, then (asymmetric pair) L_{k+1}^T
            if (pass == 0) {
                const mf_f32x2 lo = *reinterpret_cast<const mf_f32x2 *>(Rk + lc * n + 4 * quarter);
                const mf_f32x2 hi = *reinterpret_cast<const mf_f32x2 *>(Rk + lc * n + 4 * quarter + 2);
                b4 = mf_f32x4{lo.x, lo.y, hi.x, hi.y};
            } else {
                const float *col0 = Lk1 + (4 * quarter) * n + lc;     // L_{k+1}(l, 4q + kk) at (4q + kk) n + l
                b4 = mf_f32x4{col0[0], col0[n], col0[2 * n], col0[3 * n]};
            }
            mf_f32x4 t = {0.f, 0.f, 0.f, 0.f}, x = t, xt = t;
#if GBDPCG_PINV_SKIP & 2
            x = b4 + a4; xt = b4 + c4;
#else
            // T1 = B^T Dk^-1: t[i] on lane (j, q) = W[j][4q + i], W = Dk^-1 B
            t = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.x, a4.x, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.y, a4.y, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.z, a4.z, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.w, a4.w, t, 0, 0, 0);
            // X = W Dk1^-1 (lane = column of X) and X^T = Dk1^-1 W^T (lane = row of X): the same products in the same order
            x = __builtin_amdgcn_mfma_f32_16x16x4f32(t.x, c4.x, x, 0, 0, 0);
            xt = __builtin_amdgcn_mfma_f32_16x16x4f32(c4.x, t.x, xt, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f32_16x16x4f32(t.y, c4.y, x, 0, 0, 0);
            xt = __builtin_amdgcn_mfma_f32_16x16x4f32(c4.y, t.y, xt, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f32_16x16x4f32(t.z, c4.z, x, 0, 0, 0);
            xt = __builtin_amdgcn_mfma_f32_16x16x4f32(c4.z, t.z, xt, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f32_16x16x4f32(t.w, c4.w, x, 0, 0, 0);
            xt = __builtin_amdgcn_mfma_f32_16x16x4f32(c4.w, t.w, xt, 0, 0, 0);
#endif
            // R'_k(r, c) = -X(r, c) at c n + r: lane (j, q'), register i holds X^T[4q' + i][j] = X(j, 4q' + i)
            // L'_{k+1}(r, c) = -X(c, r) at c n + r: lane (j, q'), register i holds X[4q' + i][j]
            float *Rp = Pinv + blk + 2 * (size_t)nn, *Lp = Pinv + nb;
            const float xr[4] = {xt.x, xt.y, xt.z, xt.w}, xl[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t c = 4 * quarter + i;
#if GBDPCG_PINV_SKIP & 4
                if (l < n && c < n && xr[i] == 1.2345f && xl[i] == 5.4321f) {   // timing build: no result store
#else
                if (l < n && c < n) {
#endif
                    if (pass == 0) Rp[c * n + l] = -xr[i];
                    if (pass == 1 || symmetric) Lp[c * n + l] = -xl[i];
                }
            }
        }
    }
    if (verdicts) {  // uniform branch: every wave reaches the barrier
        const int bad = __syncthreads_or(any_asymmetric ? 1 : 0);
        if (threadIdx.x == 0) verdicts[(size_t)prob * chunks + chunk] = bad ? 0 : 1;
    }
}

// launch(std::true_type or std::false_type): the S_SYM template argument from the run-time flag.
template <typename F> static void with_s_sym(bool s_symmetric, F &&launch)
{
    if (s_symmetric) launch(std::true_type{});
    else launch(std::false_type{});
}

// One launch of route.chunks workgroups per problem.  Refused: more than 0x7fffffff workgroups (of this launch, or of the
// two-pass form the same call would take without it).
template <typename T>
hipError_t launch_pinv_fused(PinvRoute route, uint32_t n, uint32_t N, uint32_t batch, const T *S, T *Pinv, hipStream_t s,
                             uint8_t *verdicts, bool s_symmetric)
{
    const uint32_t chunks = route.chunks;
    if (((uint64_t)N * batch + 3) / 4 > 0x7fffffffull) return hipErrorInvalidValue;
    if ((uint64_t)chunks * batch > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid(chunks * batch), threads(kPinvThreads);
    return pinv_dispatch_n(n, hipErrorInvalidValue, [&](auto nct) {
        constexpr int NN = decltype(nct)::value;
        if constexpr (NN <= 16 && NN % 2 == 0) {
            with_s_sym(s_symmetric, [&](auto sym) {
                constexpr bool SYM = decltype(sym)::value;
                if constexpr (sizeof(T) == 4 && NN >= 12) {   // measured: -32 % at 16; a tie at 14 and 12 (profiles/r03_pinv_ab.txt)
                    if (route.family == PinvFamily::mfma) {
                        hipLaunchKernelGGL((pinv_stair_mfma_kernel<NN, SYM>), grid, threads, 0, s, N, chunks, (const float *)S, (float *)Pinv, verdicts);
                        return;
                    }
                }
                hipLaunchKernelGGL((pinv_stair_fused_kernel<T, NN, SYM>), grid, threads, 0, s, N, chunks, S, Pinv, verdicts);
            });
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;   // the route sends no other n here
        }
    });
}

template hipError_t launch_pinv_fused<float>(PinvRoute, uint32_t, uint32_t, uint32_t, const float *, float *, hipStream_t, uint8_t *, bool);
template hipError_t launch_pinv_fused<double>(PinvRoute, uint32_t, uint32_t, uint32_t, const double *, double *, hipStream_t, uint8_t *, bool);

}  // namespace gbdpcg
