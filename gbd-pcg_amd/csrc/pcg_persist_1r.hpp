// pcg_persist_1r.hpp -- the single-reduction kernel of the persistent family (opt-in: GBDPCG_PATH_PERSISTENT_1R).
// The same solve in the Chronopoulos-Gear form of preconditioned CG, arranged so that an iteration crosses the chip
// ONCE (the north star's "single cross-CU reduction per iteration"):
//     u = Pinv r ; w = S u ; gamma = r.u ; delta = u.w ; chi = u.s + p.w    (all inner products in ONE all-gather)
//     beta = gamma / gamma_old ; q = delta + beta chi + beta^2 q_old ; alpha = gamma / q       (beta = 0, q = delta first)
//     p = u + beta p ; s = w + beta s ; lambda += alpha p ; r -= alpha s
// q is p.Sp of the NEW direction written out, (u + beta p).(w + beta s) with the old p and s = S p: it holds for ANY S and
// Pinv in the [L|D|R] storage.  (Chronopoulos and Gear replace chi by -2 gamma / alpha_old, which is what it equals when S
// and Pinv are symmetric matrices -- and only then: on operators that are not, that form computes other iterates, lambda off
// by its own size after four iterations, tests/test_gpu_layout.py.  chi costs two fma per row and a third value per slot.)
// w = S u needs u on the two knots next to the workgroup's own.  Instead of a second hand-off they are recomputed here:
// the workgroup also keeps the Pinv block-rows of those two knots in registers (the threads of its first / last own
// knot hold one more row run each: +28 VGPRs in fp64) and carries r, s and w on a TWO-knot halo; what travels with the
// all-gather is {gamma, delta, chi} and the two outer own knots of w on each side.  Redundant values are bit-identical: every
// copy is the same sequence of fma's on the same bits.
// In exact arithmetic p, lambda, r and the tested quantity gamma_i = r_i . Pinv r_i are those of pcg.cuh:154-206 (the exit
// test |gamma| < tol is the same test, seen one product pair later); the ROUNDING sequence differs (p . S p is
// assembled from four products, and s = S p is carried by recurrence), so this is not the reference's recurrence and AUTO does not
// pick it.  Against the oracle: equal iteration counts and fp64 lambda within 1e-10 on every shape of
// tests/test_gpu_persist.py (a = 0.5 and a = 0.9 generators).  Two or three knots per workgroup only.
#pragma once

#include "pcg_persist_geom.hpp"

namespace gbdpcg {

template <typename T, int NCT, int K, bool HAS_PINV>
__global__ __launch_bounds__((K * PersistGeom<T, NCT>::TPK)) void pcg_persist1r_kernel(PcgArgs<T> a, u64 *ws_all, uint32_t W,
                                                                                       uint32_t spin_limit, uint32_t hold_wg,
                                                                                       uint32_t hold_us)
{
    persist_hold(blockIdx.x % W, hold_wg, hold_us);
    using Gm = PersistGeom<T, NCT>;
    static_assert(K >= 2, "the first and the last own knot carry one halo block-row each");
    constexpr uint32_t n = NCT, G = Gm::G, WPK = Gm::WPK, COLS = Gm::COLS, PER = Gran<T>::PER;
    constexpr uint32_t THREADS = K * Gm::TPK, NWAVES = K * WPK, PUB = 1, HPUB = 2, HPUB2 = 3;   // publishing waves
    static_assert(NWAVES >= 4, "wave 0 polls, three others publish");
    // windows cover knots k0-2 .. k0+K+1: window knot j = vector knot k0 - 2 + j, own knots are j = 2 .. K+1
    constexpr uint32_t WIN = (K + 4) * n, WINP = align16<T>(WIN + G * COLS - 3 * n + 1), OWN = K * n, HN = 2 * n;
    static_assert(3 * n <= G * COLS && THREADS <= 1024, "lane map");

    __shared__ __attribute__((aligned(16))) T rwin[WINP], swin[WINP], uwin[WINP], wwin[WINP], lwin[WINP];
    __shared__ __attribute__((aligned(16))) T lam[OWN], pown[OWN];
    __shared__ T dots_g[NWAVES], dots_d[NWAVES], dots_c[NWAVES];
    __shared__ T bc[4];          // [0] alpha, [1] beta, [2] gamma_old, [3] q_old = p . S p of the direction in use
    __shared__ uint32_t bci[4];  // [0] stop (1 converged, 2 hand-off timed out, 3 ran out), [1] iterations, [3] persist_leave's flag
    __shared__ T rescue_red[2 * NWAVES];

    const uint32_t N = a.N, len = n * N;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t slot = wave / WPK, wv = wave - slot * WPK;
    const uint32_t g = lane & 7u, row = wv * 8 + (lane >> 3);
    const bool row_live = row < n;
    const uint32_t cbase = g * COLS;

    const uint32_t prob = blockIdx.x / W, b = blockIdx.x - prob * W;
    const uint32_t w = (W % 8 == 0) ? (b % 8) * (W / 8) + b / 8 : b;   // neighbours on one XCD (speed only)
    const uint32_t k0 = w * K, k = k0 + slot;
    // the halo knot whose Pinv block-row this thread carries as well: left of the first own knot / right of the last
    const bool has_halo = slot == 0 || slot == K - 1;
    const int64_t kh = slot == 0 ? (int64_t)k0 - 1 : (int64_t)k0 + K;
    const uint32_t jh = slot == 0 ? 1u : K + 2u;   // its window knot

    const size_t mstride = (size_t)3 * n * n * N;
    const T *S = a.S + prob * mstride;
    const T *P = HAS_PINV ? a.Pinv + prob * mstride : nullptr;
    const T *gamma = a.gamma + (size_t)prob * len;
    T *lambda = a.lambda + (size_t)prob * len;

    u64 *ws = ws_all + (size_t)prob * persist_words<T>(n, N);
    constexpr uint32_t PSW = kPartStrideWords > 3 * PER ? kPartStrideWords : 3 * PER;
    static_assert(PSW == kPartStrideWords, "three values per partial slot fit the slot stride");
    u64 *part = ws + kPersistCtrl;                       // [2][N] slots of {gamma, delta, chi}
    const __amdgpu_buffer_rsrc_t region = __builtin_amdgcn_make_buffer_rsrc(
        part, 0, (int)((persist_words<T>(n, N) - kPersistCtrl) * 8), 0x00020000);
    const uint32_t h_base = (uint32_t)(persist_part_words<T>(N) * 8);
    const uint32_t base = (uint32_t)__hip_atomic_load(ws, GBDPCG_RLX_AGENT);
    if (persist_drop<T, NWAVES>(a, prob, ws, W, base, 2u * a.max_iter + 8u, hold_us, rescue_red, bci + 3)) return;

    // ---- resident block-rows: S and Pinv of the own knot, Pinv of the thread's halo knot ---------------------------
    T sreg[COLS], preg[COLS], hreg[COLS];
    {
        auto col_ok = [&](int64_t kk, uint32_t c) { return persist_col_ok<n>(kk, c, row_live, N); };
        const uint32_t kc = k < N ? k : 0u, khc = (kh >= 0 && kh < (int64_t)N) ? (uint32_t)kh : 0u;
        const T *Sk = S + (size_t)kc * 3 * n * n;
        const T *Pk = (HAS_PINV ? P : S) + (size_t)kc * 3 * n * n;
        const T *Ph = (HAS_PINV ? P : S) + (size_t)khc * 3 * n * n;
        T sraw[COLS], praw[COLS], hraw[COLS];
#pragma unroll
        for (uint32_t i = 0; i < COLS; ++i) {
            const uint32_t c = cbase + i;
            sraw[i] = Sk[col_ok(k, c) ? c * n + row : n * n];
            if (HAS_PINV) {
                praw[i] = Pk[col_ok(k, c) ? c * n + row : n * n];
                hraw[i] = Ph[(has_halo && col_ok(kh, c)) ? c * n + row : n * n];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t i = 0; i < COLS; ++i) {
            const uint32_t c = cbase + i;
            const bool vk = col_ok(k, c), vh = has_halo && col_ok(kh, c);
            sreg[i] = vk ? sraw[i] : T(0);
            if (HAS_PINV) {
                preg[i] = vk ? praw[i] : T(0);
                hreg[i] = vh ? hraw[i] : T(0);
            } else {   // d_Pinv == NULL: identity preconditioner
                preg[i] = (vk && c == n + row) ? T(1) : T(0);
                hreg[i] = (vh && c == n + row) ? T(1) : T(0);
            }
        }
    }

    for (uint32_t i = tid; i < WINP; i += THREADS) {
        rwin[i] = swin[i] = uwin[i] = wwin[i] = T(0);
        const int64_t gi = (int64_t)k0 * n - 2 * (int64_t)n + i;
        lwin[i] = (i < WIN && gi >= 0 && gi < (int64_t)len) ? lambda[gi] : T(0);
    }
    for (uint32_t i = tid; i < OWN; i += THREADS) {
        lam[i] = (k0 * n + i < len) ? lambda[k0 * n + i] : T(0);
        pown[i] = T(0);
    }
    if (tid == 0) {
        bc[0] = bc[1] = bc[2] = bc[3] = T(0);
        bci[0] = bci[1] = 0u;
    }
    __syncthreads();

    // hand-off offsets (bytes from `part`): a workgroup publishes [side 0: its first two own knots | side 1: its last two]
    auto nbr_l = [&](uint32_t par) { return w > 0 ? (int)(h_base + ((par * W + (w - 1)) * 2 + 1) * HN * PER * 8u) : -1; };
    auto nbr_r = [&](uint32_t par) { return w + 1 < W ? (int)(h_base + ((par * W + (w + 1)) * 2) * HN * PER * 8u) : -1; };
    // (The publish of the halo knots is written out at its two places: as a lambda, capturing by reference or by value, it
    // changed the instruction text of every instantiation, and the changed text measured 0.3 us slower at n = 14, N = 200, fp32
    // and 4 % slower at n = 36, N = 256, fp64 with three knots per workgroup -- profiles/r18_persist_split.txt.  The same
    // holds for the coordinates and the workspace set-up, which pcg_persist_2r.hpp takes from pcg_persist_geom.hpp.)
    // r = gamma - S lambda (pcg.cuh:118-126) on the own knots; its two outer own knots go to the neighbours (epoch 1)
    {
        T y = group_sum8(persist_row_dot<T, COLS, (THREADS > 768), Gm::ALIGNED>(sreg, lwin + (slot + 1) * n + cbase,
                                                                               lwin + (slot + 1) * n + cbase, T(0)));
        if (g == 0 && row_live) rwin[(slot + 2) * n + row] = (k < N ? gamma[k * n + row] : T(0)) - y;
        __syncthreads();
        if (wave == HPUB || wave == HPUB2) {   // the two outer own knots of rwin on the left / right side, for the neighbours' two-knot halo
            const uint32_t side = wave == HPUB ? 0u : 1u;
            const uint32_t mh = h_base + ((1u * W + w) * 2 + side) * HN * PER * 8u;
            for (uint32_t i = lane; i < HN; i += 64)
                slot_store(region, mh + i * PER * 8u, base + 1u, rwin[(side ? 2 * n + (K - 2) * n : 2 * n) + i]);
        }
        if (wave == 0) {
            T dummy[1];
            const bool ok = persist_sweep_n<T, NCT, 0, HN>(region, 0u, nbr_l(1u), nbr_r(1u), W, base + 1u, lane, spin_limit, dummy,
                                                          rwin, rwin + (K + 2) * n);
            if (lane == 0 && !ok) bci[0] = 2u;
        }
        __syncthreads();
    }

    uint32_t iter = 0;
    for (; bci[0] == 0u; ++iter) {
        const uint32_t ew = 2u + iter, par = iter & 1u;
        const bool stamp_here = w == 1 && wave == 0 && iter == 3;
        (void)stamp_here;
        GBDPCG_STAMP(2, stamp_here)
        // u = Pinv r on the own knots and, redundantly, on the two knots next to them; share of gamma = r . u  (pcg.cuh:180-187)
        {
            T y = group_sum8(persist_row_dot<T, COLS, (THREADS > 768), Gm::ALIGNED>(preg, rwin + (slot + 1) * n + cbase,
                                                                                   rwin + (slot + 1) * n + cbase, T(0)));
            T yh = T(0);
            if (has_halo)   // wave-uniform
                yh = group_sum8(persist_row_dot<T, COLS, (THREADS > 768), Gm::ALIGNED>(hreg, rwin + (jh - 1) * n + cbase,
                                                                                       rwin + (jh - 1) * n + cbase, T(0)));
            T d = T(0);
            if (g == 0 && row_live) {
                uwin[(slot + 2) * n + row] = y;
                if (has_halo) uwin[jh * n + row] = yh;
                d = rwin[(slot + 2) * n + row] * y;
            }
            d = wave_sum(d);
            if (lane == 0) dots_g[wave] = d;
        }
        __syncthreads();
        GBDPCG_STAMP(3, stamp_here)
        // w = S u on the own knots ; shares of delta = u . w and of chi = u . s + p . w (s, p: still the old direction's)
        {
            T y = group_sum8(persist_row_dot<T, COLS, (THREADS > 768), Gm::ALIGNED>(sreg, uwin + (slot + 1) * n + cbase,
                                                                                   uwin + (slot + 1) * n + cbase, T(0)));
            T d = T(0), c = T(0);
            if (g == 0 && row_live) {
                const T uo = uwin[(slot + 2) * n + row];
                wwin[(slot + 2) * n + row] = y;
                d = uo * y;
                c = fma_t(uo, swin[(slot + 2) * n + row], pown[slot * n + row] * y);
            }
            d = wave_sum(d);
            c = wave_sum(c);
            if (lane == 0) {
                dots_d[wave] = d;
                dots_c[wave] = c;
            }
        }
        __syncthreads();
        GBDPCG_STAMP(4, stamp_here)
        // {gamma, delta, chi, the two outer own knots of w per side} in ONE all-gather
        if (wave == PUB) {   // the partials first: every workgroup waits for them
            T pg = dots_g[0], pd = dots_d[0], pc = dots_c[0];
#pragma unroll
            for (uint32_t q = 1; q < NWAVES; ++q) {
                pg += dots_g[q];
                pd += dots_d[q];
                pc += dots_c[q];
            }
            if (lane == 0) {
                slot_store(region, (par * N + w) * PSW * 8u, base + ew, pg);
                slot_store(region, (par * N + w) * PSW * 8u + PER * 8u, base + ew, pd);
                slot_store(region, (par * N + w) * PSW * 8u + 2 * PER * 8u, base + ew, pc);
            }
        }
        if (wave == HPUB || wave == HPUB2) {   // the two outer own knots of wwin on the left / right side, for the neighbours' two-knot halo
            const uint32_t side = wave == HPUB ? 0u : 1u;
            const uint32_t mh = h_base + ((par * W + w) * 2 + side) * HN * PER * 8u;
            for (uint32_t i = lane; i < HN; i += 64)
                slot_store(region, mh + i * PER * 8u, base + ew, wwin[(side ? 2 * n + (K - 2) * n : 2 * n) + i]);
        }
        if (wave == 0) {
            T tot[3];
            const bool ok = persist_sweep_n<T, NCT, 3, HN>(region, par * N * PSW * 8u, nbr_l(par), nbr_r(par), W, base + ew, lane,
                                                          spin_limit, tot, wwin, wwin + (K + 2) * n);
            GBDPCG_STAMP(5, stamp_here)
            if (lane == 0) {
                const T gam = tot[0], del = tot[1];
                if (!ok) {
                    bci[0] = 2u;
                } else if (iter > 0 && fabs(gam) < a.tol) {       // pcg.cuh:195, on gamma_iter = r . Pinv r after `iter` updates
                    bci[0] = 1u;
                    bci[1] = iter;
                } else if (iter >= a.max_iter) {
                    bci[0] = 3u;
                    bci[1] = a.max_iter;
                    bc[1] = iter > 0 ? gam / bc[2] : T(0);        // the beta of the direction update the reference still runs
                } else {
                    const T beta = iter > 0 ? gam / bc[2] : T(0);
                    const T q = iter > 0 ? fma_t(beta, fma_t(beta, bc[3], tot[2]), del) : del;   // (u + beta p).(w + beta s)
                    bc[0] = gam / q;
                    bc[1] = beta;
                    bc[2] = gam;
                    bc[3] = q;
                }
            }
        }
        __syncthreads();
        GBDPCG_STAMP(6, stamp_here)
        if (bci[0] != 0u) break;
        // s = w + beta s ; r -= alpha s on the own knots and the two-knot halo ; p = u + beta p ; lambda += alpha p on the own
        {
            const T alpha = bc[0], beta = bc[1];
            for (uint32_t i = tid; i < WIN; i += THREADS) {
                const T sn = fma_t(beta, swin[i], wwin[i]);
                swin[i] = sn;
                rwin[i] = fma_t(-alpha, sn, rwin[i]);
                if (i >= 2 * n && i < 2 * n + OWN) {
                    const T pn = fma_t(beta, pown[i - 2 * n], uwin[i]);
                    pown[i - 2 * n] = pn;
                    lam[i - 2 * n] = fma_t(alpha, pn, lam[i - 2 * n]);
                }
            }
        }
        __syncthreads();
        GBDPCG_STAMP(7, stamp_here)
    }

    // ---- outputs (pcg.cuh:212,215) --------------------------------------------------------------------------------
    const uint32_t stop = bci[0];
    const bool failed = stop == 2u, ran_out = stop == 3u;
    const T beta = ran_out ? bc[1] : T(0);   // max-iteration exit: the reference's last iteration still ran p = r~ + beta p
    for (uint32_t i = tid; i < OWN; i += THREADS) {
        const uint32_t gi = k0 * n + i;
        if (gi < len && !failed) {
            lambda[gi] = lam[i];
            if (a.r) a.r[(size_t)prob * len + gi] = rwin[2 * n + i];
            if (a.p) a.p[(size_t)prob * len + gi] = ran_out ? fma_t(beta, pown[i], uwin[2 * n + i]) : pown[i];
        }
    }
    if (w == 0 && tid == 0 && (!failed || a.rescue_off)) {
        a.iters[prob] = failed ? kItersGaveUp : bci[1];
        if (a.max_iter_exit) a.max_iter_exit[prob] = failed ? 2 : (ran_out ? 1 : 0);
    }
    persist_leave<T, NWAVES>(a, prob, ws, W, base, 2u * a.max_iter + 8u, failed, rescue_red, bci + 3);
}

}  // namespace gbdpcg
