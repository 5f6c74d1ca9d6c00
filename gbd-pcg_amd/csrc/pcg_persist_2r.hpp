// pcg_persist_2r.hpp -- the two-reduction kernel of the persistent family (GBDPCG_PATH_PERSISTENT): the recurrence of pcg.cuh:154-206,
// cut at its two inner products; each cut is one all-gather of pcg_persist_handoff.hpp.
#pragma once

#include "pcg_persist_geom.hpp"

namespace gbdpcg {

enum PersistPhase { PP_INIT = 0, PP_PRECOND = 1, PP_DIRECTION = 2 };

template <typename T, int NCT, int K, bool HAS_PINV>
__global__ __launch_bounds__((K * PersistGeom<T, NCT>::TPK)) void pcg_persist_kernel(PcgArgs<T> a, u64 *ws_all, uint32_t W,
                                                                                     uint32_t spin_limit, uint32_t staged,
                                                                                     uint32_t hold_wg, uint32_t hold_us)
{
    persist_hold(blockIdx.x % W, hold_wg, hold_us);
    using Gm = PersistGeom<T, NCT>;
    constexpr uint32_t n = NCT, G = Gm::G, WPK = Gm::WPK, COLS = Gm::COLS, PER = Gran<T>::PER;
    // PUB publishes the partial, HPUB the boundary knots (no global store by the polling wave 0 when there are others)
    constexpr uint32_t THREADS = K * Gm::TPK, NWAVES = K * WPK, PUB = NWAVES > 1 ? 1 : 0, HPUB = NWAVES > 2 ? 2 : PUB;
    constexpr uint32_t WIN = (K + 2) * n, WINP = align16<T>(WIN + G * COLS - 3 * n + 1), OWN = K * n;
    static_assert(3 * n <= G * COLS && THREADS <= 1024, "lane map");

    __shared__ __attribute__((aligned(16))) T rwin[2][WINP];
    __shared__ __attribute__((aligned(16))) T pwin[2][WINP];
    __shared__ __attribute__((aligned(16))) T uwin[WINP];   // upsilon = S p, window form
    __shared__ __attribute__((aligned(16))) T twin[WINP];   // r~ = Pinv r, window form
    __shared__ __attribute__((aligned(16))) T lwin[WINP];   // lambda window of the prologue
    __shared__ __attribute__((aligned(16))) T lam[OWN];
    __shared__ T dots[NWAVES];   // per-wave shares of the inner product
    __shared__ T bc[4];          // [0] coefficient of the next phase, [1] eta, [2] beta of the last direction update
    __shared__ uint32_t bci[4];  // [0] stop (1 converged, 2 hand-off timed out), [1] iterations, [3] persist_leave's flag
    __shared__ T rescue_red[2 * NWAVES];

    const PersistCoords at = persist_coords<T, NCT, K>(W);
    const uint32_t tid = at.tid, lane = at.lane, wave = at.wave, slot = at.slot, g = at.g, row = at.row, cbase = at.cbase;
    const uint32_t prob = at.prob, w = at.w, k0 = at.k0, k = at.k;
    const bool row_live = at.row_live, knot_live = k < a.N;
    const uint32_t N = a.N, len = n * N;
    const uint32_t oi = slot * n + (row_live ? row : 0u);   // this lane's row in the own part of a vector

    const size_t mstride = (size_t)3 * n * n * N;
    const T *S = a.S + prob * mstride;
    const T *P = HAS_PINV ? a.Pinv + prob * mstride : nullptr;
    const T *gamma = a.gamma + (size_t)prob * len;
    T *lambda = a.lambda + (size_t)prob * len;

    constexpr uint32_t PSW = kPartStrideWords > PER ? kPartStrideWords : PER;   // u64 words per partial slot
    const PersistWorkspace h = persist_workspace<T>(ws_all, prob, n, N);
    const __amdgpu_buffer_rsrc_t region = h.region;
    u64 *const ws = h.ws;
    const uint32_t halo_base = h.halo_base, base = h.base;
    if (persist_drop<T, NWAVES>(a, prob, ws, W, base, 2u * a.max_iter + 8u, hold_us, rescue_red, bci + 3)) return;

    // ---- resident matrices: this lane's COLS columns of its row, both matrices -----------------------------------
    T sreg[COLS], preg[COLS];
    {
        const T *Sk = S + (size_t)(knot_live ? k : 0u) * 3 * n * n;
        const T *Pk = (HAS_PINV ? P : S) + (size_t)(knot_live ? k : 0u) * 3 * n * n;
        // all 2 * COLS loads first (one memory round trip), the selections afterwards
        T sraw[COLS], praw[COLS];
        if (staged) {
            // The block-rows of the workgroup's K knots are contiguous in memory: LDS-DMA brings them in as dense 16-byte
            // pieces (the direct form below reads 8 bytes per lane at a stride of n elements) and the lanes pick their
            // elements up from LDS.  Knots past the end of the problem re-read the last one (masked below).
            extern __shared__ __attribute__((aligned(16))) unsigned char persist_stage[];
            constexpr uint32_t PPK = 3 * n * n * sizeof(T) / 16;   // 16-byte pieces per knot
            static_assert((3 * n * n * sizeof(T)) % 16 == 0, "whole pieces per knot");
            T *stS = reinterpret_cast<T *>(persist_stage), *stP = stS + K * 3 * n * n;
            uint32_t lo = lane;
            asm volatile("" : "+v"(lo));
            for (uint32_t q0 = wave * 64; q0 < K * PPK; q0 += THREADS) {
                const uint32_t q = q0 + lo;
                if (q < K * PPK) {
                    const uint32_t j = q / PPK, piece = q - j * PPK, kk = k0 + j < N ? k0 + j : N - 1;
                    const uint32_t off = (kk - (k0 < N ? k0 : N - 1)) * (3 * n * n * (uint32_t)sizeof(T)) + piece * 16;
                    const T *Sb = S + (size_t)(k0 < N ? k0 : N - 1) * 3 * n * n;
                    unsigned keep;
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "s"(Sb), "v"(off), "s"((uint32_t)(uintptr_t)stS + q0 * 16) : "memory");
                    if (HAS_PINV) {
                        const T *Pb = P + (size_t)(k0 < N ? k0 : N - 1) * 3 * n * n;
                        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1\n\ts_mov_b32 m0, %0"
                                     : "=&s"(keep) : "s"(Pb), "v"(off), "s"((uint32_t)(uintptr_t)stP + q0 * 16) : "memory");
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
#pragma unroll
            for (uint32_t i = 0; i < COLS; ++i) {
                const uint32_t c = cbase + i;
                const uint32_t idx = slot * 3 * n * n + (persist_col_ok<n>(k, c, row_live, N) ? c * n + row : n * n);
                sraw[i] = stS[idx];
                if (HAS_PINV) praw[i] = stP[idx];
            }
        } else {
            // (Written out here and in pcg_persist_1r.hpp: a shared load-one-run helper issued all loads of S before those of
            // Pinv, where this loop interleaves them column by column; with it, a shared select and a shared write-out, this
            // kernel measured 0.3 us slower at n = 14, N = 200, fp32 -- profiles/r18_persist_split.txt.)
#pragma unroll
            for (uint32_t i = 0; i < COLS; ++i) {
                const uint32_t c = cbase + i;
                const uint32_t idx = persist_col_ok<n>(k, c, row_live, N) ? c * n + row : n * n;   // else an element of D_k: always there
                sraw[i] = Sk[idx];
                if (HAS_PINV) praw[i] = Pk[idx];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t i = 0; i < COLS; ++i) {
            const uint32_t c = cbase + i;
            const bool valid = persist_col_ok<n>(k, c, row_live, N);
            sreg[i] = valid ? sraw[i] : T(0);
            if (HAS_PINV) preg[i] = valid ? praw[i] : T(0);
            else preg[i] = (valid && c == n + row) ? T(1) : T(0);   // d_Pinv == NULL: identity preconditioner
        }
    }

    // ---- LDS state ---------------------------------------------------------------------------------------------
    for (uint32_t i = tid; i < WINP; i += THREADS) {
        rwin[0][i] = rwin[1][i] = pwin[0][i] = pwin[1][i] = uwin[i] = twin[i] = T(0);
        const int64_t gi = (int64_t)k0 * n - n + i;   // window element i = vector element gi
        lwin[i] = (i < WIN && gi >= 0 && gi < (int64_t)len) ? lambda[gi] : T(0);
    }
    for (uint32_t i = tid; i < OWN; i += THREADS) lam[i] = (k0 * n + i < len) ? lambda[k0 * n + i] : T(0);
    if (tid == 0) {
        bc[0] = bc[1] = bc[2] = T(0);
        bci[0] = bci[1] = 0u;
    }
    __syncthreads();

    uint32_t rc = 0, pc = 0;   // current r / p window

    // One phase: y = M X over the own knots with X = A + coef * B formed on the fly; the row owners (lane 0 of each
    // group) store y, the new operand window NEW, publish the boundary knots and their share of the inner product; then
    // wave 0 publishes the workgroup's partial, gathers everybody's and decides what comes next.
    // PHASE_T: std::integral_constant<PersistPhase, ...>; NEW: a T *, or nullptr (as a type) for "no new window"; ITER: -1 in the
    // prologue.  Inlined at each of its four calls, like the macro it was.
    auto phase = [&](auto PHASE_T, const T(&MREG)[COLS], const T *A, const T *B, auto NEW, T *YWIN, uint32_t EPOCH,
                     int ITER) __attribute__((always_inline)) {
        constexpr PersistPhase PHASE = decltype(PHASE_T)::value;
        constexpr bool HAS_NEW = !std::is_null_pointer<decltype(NEW)>::value;
        const T coef = bc[0];
        const uint32_t tag = base + EPOCH, par = EPOCH & 1u;
        const bool stamp_here = w == 1 && wave == 0 && ITER == 3;
        const uint32_t sb = PHASE == PP_DIRECTION ? 2u : 8u;
        (void)stamp_here;
        (void)sb;
        GBDPCG_STAMP(sb + 0, stamp_here)
        GBDPCG_STAMP_RT(PHASE == PP_DIRECTION ? 14u : 15u, stamp_here)
        // operands of the row owners and the two halo knots of the new window first: their LDS round trips run under the
        // product's
        const T own_a = A[n + oi], own_b = B[n + oi], own_p = pwin[pc][n + oi], own_l = lam[oi];
        if constexpr (HAS_NEW) {
            for (uint32_t i = tid; i < 2 * n; i += THREADS) {
                const uint32_t j = i < n ? i : OWN + i;
                NEW[j] = fma_t(coef, B[j], A[j]);
            }
        }
        T y = persist_row_dot<T, COLS, (THREADS > 768), Gm::ALIGNED>(MREG, A + slot * n + cbase, B + slot * n + cbase, coef);
        GBDPCG_STAMP(1, stamp_here && PHASE == PP_DIRECTION)
        y = group_sum8(y);
        T d = T(0);
        if (g == 0 && row_live) {
            const T xo = fma_t(coef, own_b, own_a);   // this row of the operand
            if (PHASE == PP_INIT) y = (knot_live ? gamma[k * n + row] : T(0)) - y;   // r = gamma - S lambda
            YWIN[n + oi] = y;
            if constexpr (HAS_NEW) {
                NEW[n + oi] = xo;
                if (PHASE == PP_PRECOND) lam[oi] = fma_t(-coef, own_p, own_l);   // lambda += alpha p (pcg.cuh:172-174); coef = -alpha
            }
            if (PHASE != PP_INIT) d = xo * y;
        }
        d = wave_sum(d);
        if (lane == 0) dots[wave] = d;
        GBDPCG_STAMP(7, stamp_here && PHASE == PP_DIRECTION)
        GBDPCG_STAMP(13, stamp_here && PHASE == PP_DIRECTION)
        __syncthreads();
        GBDPCG_STAMP(sb + 1, stamp_here)
        // No global store is issued before the barrier above (it would make every wave wait for the write-through
        // acknowledgement), and none by the polling wave (its loads would queue behind them): wave PUB publishes.
        if (wave == PUB) {   // the partial first: every workgroup waits for it, the boundary knots concern two
            T dot = dots[0];
#pragma unroll
            for (uint32_t q = 1; q < NWAVES; ++q) dot += dots[q];
            GBDPCG_XSTAMP(0, PHASE == PP_DIRECTION && ITER == 3)
            if (lane == 0) slot_store(region, (par * N + w) * PSW * 8u, tag, dot);
        }
        if (wave == HPUB) {
            const uint32_t my_halo = halo_base + ((par * N + w) * 2) * n * PER * 8u;
            for (uint32_t i = lane; i < 2 * n; i += 64) {   // first knot -> left neighbour, last knot -> right
                const uint32_t src = i < n ? n + i : n + (K - 1) * n + (i - n);
                slot_store(region, my_halo + i * PER * 8u, tag, YWIN[src]);
            }
        }
        if (wave == 0) {
            GBDPCG_STAMP(sb + 2, stamp_here)
            T total;
            const bool ok = persist_sweep<T, NCT>(region, par * N * PSW * 8u,
                                                  w > 0 ? (int)(halo_base + ((par * N + (w - 1)) * 2 + 1) * n * PER * 8u) : -1,
                                                  w + 1 < W ? (int)(halo_base + ((par * N + (w + 1)) * 2) * n * PER * 8u) : -1, W, tag,
                                                  lane, spin_limit, total, YWIN, YWIN + n + OWN);
            GBDPCG_STAMP(sb + 3, stamp_here)
            GBDPCG_XSTAMP(1, PHASE == PP_DIRECTION && ITER == 3)
            if (lane == 0) {
                if (!ok) {
                    bci[0] = 2u;
                } else if (PHASE == PP_INIT) {
                    bc[0] = T(0);
                } else if (PHASE == PP_DIRECTION) {   // alpha = eta / (p . upsilon)      (pcg.cuh:169)
                    bc[0] = -(bc[1] / total);
                } else if (ITER < 0) {                // prologue: eta = r . r~, p = r~  (pcg.cuh:139-149)
                    bc[1] = total;
                    bc[0] = bc[2] = T(0);
                } else if (fabs(total) < a.tol) {     // pcg.cuh:195
                    bci[0] = 1u;
                    bci[1] = (uint32_t)ITER + 1u;
                } else {                              // beta = eta' / eta ; eta = eta'  (pcg.cuh:199-202)
                    bc[0] = bc[2] = total / bc[1];
                    bc[1] = total;
                }
            }
        }
        __syncthreads();
        GBDPCG_STAMP(sb + 4, stamp_here)
    };
    constexpr std::integral_constant<PersistPhase, PP_INIT> init{};
    constexpr std::integral_constant<PersistPhase, PP_PRECOND> precond{};
    constexpr std::integral_constant<PersistPhase, PP_DIRECTION> direction{};

    // r = gamma - S lambda (pcg.cuh:118-126); the boundary knots of r travel with epoch 1
    phase(init, sreg, lwin, lwin, nullptr, rwin[0], 1u, -1);
    // r~ = Pinv r ; eta = r . r~ (pcg.cuh:130-149)
    if (bci[0] == 0u) phase(precond, preg, rwin[0], rwin[0], nullptr, twin, 2u, -1);

    uint32_t iter = 0;
    bool ran_out = true;
    for (; iter < a.max_iter && bci[0] == 0u; ++iter) {   // pcg.cuh:154
        // p = r~ + beta p ; upsilon = S p ; alpha = eta / (p . upsilon)   (pcg.cuh:203-206,156-169)
        phase(direction, sreg, twin, pwin[pc], pwin[pc ^ 1], uwin, 3u + 2u * iter, (int)iter);
        pc ^= 1u;
        if (bci[0] != 0u) break;
        // lambda += alpha p ; r -= alpha upsilon ; r~ = Pinv r ; eta' = r . r~   (pcg.cuh:172-193)
        phase(precond, preg, rwin[rc], uwin, rwin[rc ^ 1], twin, 4u + 2u * iter, (int)iter);
        rc ^= 1u;
        if (bci[0] == 1u) {
            ran_out = false;
            break;
        }
    }

    // ---- outputs (pcg.cuh:212,215) --------------------------------------------------------------------------------
    const bool failed = bci[0] == 2u;   // (the same verdict in every workgroup of the problem: all of them wait for all)
    const T beta = ran_out ? bc[2] : T(0);   // the last iteration did not break: it still ran p = r~ + beta p
    for (uint32_t i = tid; i < OWN; i += THREADS) {
        const uint32_t gi = k0 * n + i;
        if (gi < len && !failed) {   // a launch that gave up leaves lambda, r, p as it found them: the rescue starts there
            lambda[gi] = lam[i];
            if (a.r) a.r[(size_t)prob * len + gi] = rwin[rc][n + i];
            if (a.p) a.p[(size_t)prob * len + gi] = ran_out ? fma_t(beta, pwin[pc][n + i], twin[n + i]) : pwin[pc][n + i];
        }
    }
    if (w == 0 && tid == 0 && (!failed || a.rescue_off)) {   // (rescue_off: hooks build only, to show the mark)
        a.iters[prob] = failed ? kItersGaveUp : (ran_out ? a.max_iter : bci[1]);
        if (a.max_iter_exit) a.max_iter_exit[prob] = failed ? 2 : (ran_out ? 1 : 0);
    }
    persist_leave<T, NWAVES>(a, prob, ws, W, base, 2u * a.max_iter + 8u, failed, rescue_red, bci + 3);
}

}  // namespace gbdpcg
