// pcg_cluster.hip -- PCG with both GENERAL-storage matrices register-resident, a problem spread over a CLUSTER of up to eight
// (fp64: four) workgroups, each on a compute unit of its own or sharing one with another.
//
// Replaces pcg<T,n,N> (include/pcg.cuh:54-218 of the reference) for the BASELINE batch shape (n = 14, fp32, N = 128) when the
// storage is not bit-symmetric (pcg_resident_sym.hip does not apply) and in general for horizons beyond what one workgroup holds
// (pcg_resident.hip), up to cl_max_members times that: at n = 14 in fp32, 72 < N <= 576.  The reference keeps all three blocks
// [L|D|R] of a knot of S and Pinv next to the ALUs for the whole solve (pcg.cuh:104-110); at the batch shape that is 602 KB per
// problem, more than one CU holds (512 KB of registers + 160 KB of LDS), so the problem is cut into H = ceil(N / 72) runs of
// consecutive knots and each run is given to one 8-wave workgroup with the lane map of pcg_resident.hip (bt_dense.hpp: 2 x 84 VGPRs
// of matrix data per lane, no cross-lane fold).  The matrices are read from HBM once per solve; an iteration touches LDS, registers
// and the hand-off words.  What crosses between the workgroups of a cluster, and how: pcg_cluster_handoff.hpp.
#include <algorithm>
#include <cstdlib>

#include "pcg_cluster_handoff.hpp"
#include "pcg_stream.hpp"

namespace gbdpcg {

namespace {

// Columns of a lane's block-row of Pinv (its V rows each) that live in LDS instead of registers (dense_mv, TAIL): 2 x 3n x V x
// sizeof(T) / 4 matrix registers per lane must leave room for the working set.  They take the place of the staging buffers once
// every wave's tiles are in.
template <typename T, int NCT> constexpr int cluster_tail_cols()
{
    if (sizeof(T) == 4 && NCT == 18) return 36;   // the D and the R block: 9 lanes per knot, 2 x 108 registers otherwise
    if (sizeof(T) == 8 && NCT == 16) return 32;   // the D and the R block: 2 x 96 registers next to a working set of twice the width
    if (sizeof(T) == 4 && NCT == 16) return 16;   // the R block: 2 x 96 registers do not fit next to the working set, 96 + 64 do
    if (sizeof(T) == 8 && NCT == 14) return 14;   // the R block: 2 x 84 next to a working set of twice the width, 84 + 56 do
    return 0;                                     // everything in registers: the kernel compiles without scratch
}
template <typename T, int NCT> struct ClusterTail { static constexpr int COLS = cluster_tail_cols<T, NCT>(); };
// bytes between the tails of two waves in dynamic LDS
template <typename T, int NCT, int V, bool STAGED> struct ClusterTailBytes {
    static constexpr size_t PER_WAVE = STAGED ? (size_t)DenseStage<T, NCT, V>::BYTES : (size_t)ClusterTail<T, NCT>::COLS * 64 * 8;
};

// A problem this launch leaves to the rescue.  (hooks build only, rescue switched off: show the mark)
template <typename T> __device__ __forceinline__ void cl_mark_given_up(const PcgArgs<T> &a, uint32_t prob, bool writer)
{
    if (a.rescue_off && writer) {
        a.iters[prob] = kItersGaveUp;
        if (a.max_iter_exit) a.max_iter_exit[prob] = 2;
    }
}

// Diagnostic build only (-DGBDPCG_CL_STAMPS, tools/cluster_stamps.py): cycle stamps of iteration 3 of the first problem
// of block 0, left in the unused words of the control block.  No stamp exists in the shipped build.
#ifdef GBDPCG_CL_STAMPS
#define GBDPCG_CL_STAMP(IDX, WAVE, COND)                                                                             \
    if (blk == 0 && wave == (WAVE) && lane == 0 && (COND)) reinterpret_cast<u64 *>(ws)[IDX] = __builtin_amdgcn_s_memtime();
// ... and the 100 MHz real-time clock (wall time, whatever the shader clock does) for the problem-level stamps
#define GBDPCG_CL_STAMP_RT(IDX, WAVE, COND)                                                                          \
    if (blk == 0 && wave == (WAVE) && lane == 0 && (COND)) reinterpret_cast<u64 *>(ws)[IDX] = __builtin_amdgcn_s_memrealtime();
// start (0) / end (1) of every workgroup, behind the slots as sized for the device (256 CUs on the MI355X)
#define GBDPCG_CL_STAMP_WG(WHICH)                                                                                    \
    if (tid == 0) reinterpret_cast<u64 *>(ws + kClCtrlBytes + 2u * 512u * kClSlotBytes)[2 * blk + (WHICH)] = __builtin_amdgcn_s_memrealtime();
#else
#define GBDPCG_CL_STAMP_WG(WHICH)
#define GBDPCG_CL_STAMP(IDX, WAVE, COND)
#define GBDPCG_CL_STAMP_RT(IDX, WAVE, COND)
#endif

}  // namespace

// Instantiations light enough for two workgroups to share a compute unit (launch_pcg_cluster): held to 128 registers.  fp32 at
// stateSize 2, 3, 4, 5, 7, 9, 11 need 108-118 anyway; 6 (144), 13 (132) and fp64 at 2-5 (139) are asked to fit (2-12 registers
// spilled, and still 1.3-1.6x faster with two per CU: 1024 converged solves of 9 x 128: 516 -> 317 us, 13 x 128: 491 -> 367,
// 6 x 200: 212 -> 151, fp64 4 x 200: 208 -> 134).  stateSize 15 (143: 20 spilled) gains 14 % that way (531 -> 455 us) and never runs as
// a cluster of one, where the cap alone would cost 30 %: pcg_resident.hip has its short horizons.
template <typename T, int NCT> struct ClusterLight {
    static constexpr bool value = (sizeof(T) == 4 && (NCT <= 7 || NCT == 9 || NCT == 11 || NCT == 13 || NCT == 15)) || (sizeof(T) == 8 && NCT <= 5);
};
// ONE: a cluster of one workgroup (launch_pcg_cluster: only where the shape has such launches) -- nobody to hand anything to, the wave
// partials meet in LDS, in the same words and the same sum as in memory.  A compile-time switch: as a run-time test inside the
// hand-off it cost the clusters of two to four members 4 %.
// SHARED (gbdpcg_solve_shared_*): a.S and a.Pinv are one pair of matrices for the whole batch -- every cluster loads its tiles from
// it (zero problem stride; after the first round they come from L2 / Infinity Cache).
template <typename T, int NCT, int V, bool STAGED, bool ONE = false, bool SHARED = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(ClusterLight<T, NCT>::value ? 4 : 2)))
void pcg_cluster_kernel(PcgArgs<T> a, unsigned char *ws, uint32_t H, uint32_t C,
                                                          uint32_t clusters, uint32_t spin_limit, uint32_t drop_block, bool no_plain)
{
    // Behind a verifying launch that rejected nothing (PcgArgs::reject_count) this launch owns nothing: leave before anything is
    // set up.  Safe for the hand-off protocol only because EVERY workgroup of the launch reads the same count and so takes the
    // same branch: nobody is left polling for a member that has gone.  Such a launch touches neither the slots nor the launch
    // number: it publishes no tag, so it needs no number of its own, and the next launch that owns a problem still gets a
    // number no earlier launch has used (a launch that owned nothing used to take one; it left the slots alone as well).
    if (pcg_reject_none(a)) return;
#ifndef GBDPCG_TEST_HOOKS
    drop_block = 0xffffffffu;   // the hook that silences one workgroup exists in variants/libgbdpcg_hooks.so only
#endif
    using Dg = DenseGeom<T, NCT, V>;
    // lane roles of the hand-off: LPB = n / V lanes per knot (<= 16: a knot's boundary values are LPB 16-byte stores), a lane's rows
    // are 8 bytes of payload at most, 8 waves (partial lanes: 16 bytes of the 8 H wave partials each)
    static_assert(V * sizeof(T) <= 8 && NCT % V == 0 && Dg::LPB <= 16 && Dg::WAVES == 8, "lane roles of the hand-off");
    constexpr uint32_t n = NCT, LPB = Dg::LPB, THREADS = Dg::WAVES * 64, WINF = align16<T>((Dg::MAX_KNOTS + 2) * n);
    constexpr uint32_t PPM = cl_ppm<T>();
    // accumulator chains of a block-row product (bt_dense.hpp, dense_mv): one chain per block needs whole operand pairs per block
    constexpr int CHAINS = NCT % 2 == 0 ? 3 : 1;
    __shared__ __attribute__((aligned(16))) T xa[WINF];   // window of p (lambda in the prologue): halo knot, own knots, halo knot
    __shared__ __attribute__((aligned(16))) T xb[WINF];   // window of r
    __shared__ T bc[4];           // [0] alpha / eta' of the phase just gathered, [1] beta
    __shared__ uint32_t bci[4];   // [0] 0 go on, 1 converged, 2 hand-off timed out; [2], [3] the rescue's bookkeeping
    __shared__ T rescue_red[2 * Dg::WAVES];
    __shared__ u32x4 lpart[ONE ? Dg::WAVES : 1];   // ONE: the wave partials of a hand-off, laid out like the slot in memory
    extern __shared__ __attribute__((aligned(16))) unsigned char stage_raw[];   // STAGED: dense_stage_lds_bytes (bt_dense.hpp)
    constexpr int PTAIL = ClusterTail<T, NCT>::COLS;
    // Every wave keeps its own: in its first staging buffer when the tiles come in staged (bt_dense.hpp, dense_staged_load: the
    // block goes from the second buffer straight there, never through registers), else in PTAIL x 64 elements of its own.
    using TV = typename DenseTailElem<T, V>::type;
    static_assert(PTAIL == 0 || sizeof(TV) == 8, "a lane's rows of a tail column are 8 bytes");

    const uint32_t N = a.N, len = n * N;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    TV *ptail = reinterpret_cast<TV *>(stage_raw + (size_t)wave * ClusterTailBytes<T, NCT, V, STAGED>::PER_WAVE);
    // PTAIL <= n: columns of the R block, behind pt_lane.  PTAIL = 2n (stateSize 18): the D block behind ptd_lane (staged: re-laid inside
    // the wave's first staging buffer) and the R block behind pt_lane (staged: inside its second buffer).
    constexpr bool TWO = PTAIL > (int)NCT;
    static_assert(!TWO || PTAIL == 2 * (int)NCT, "the D and the R block, whole");
    const TV *ptd_lane = ptail + lane;
    const TV *pt_lane = !TWO ? ptail + lane
                        : STAGED ? reinterpret_cast<const TV *>(stage_raw + (size_t)(Dg::WAVES + wave) * ClusterTailBytes<T, NCT, V, STAGED>::PER_WAVE) + lane
                                 : ptail + NCT * 64 + lane;
    const uint32_t grid = gridDim.x, blk = blockIdx.x;
    // cluster c, member h.  Members sit 8 blocks apart where the cluster count allows it: blocks b and b + 8 share an XCD
    // under round-robin dispatch (a hand-off inside one L2 is ~20 % shorter).  Speed only: nothing depends on placement.
    const bool spread = clusters % 8 == 0;
    const uint32_t c = spread ? (blk / (8 * H)) * 8 + blk % 8 : blk / H;
    const uint32_t h = spread ? (blk % (8 * H)) / 8 : blk % H;
    const uint32_t bstride = spread ? 8u : 1u;   // block index distance of two neighbouring members
    const uint32_t blk0 = blk - h * bstride;     // member 0 of this cluster
    const uint32_t k_lo = h * C, cnt = k_lo < N ? (N - k_lo < C ? N - k_lo : C) : 0u;   // host: cnt >= 1 for every member
    const bool has_left = h > 0, has_right = h + 1 < H;

    const DenseCtx<T, NCT, V> dc(wave, lane, cnt, k_lo);
    // first of this lane's rows, counted from knot k_lo: (wave BPW + lane / LPB) n + (lane % LPB) V = wave BPW n + V lane (n = V LPB)
    const uint32_t row0 = dc.live ? wave * (Dg::BPW * n) + V * lane : 0u;
    // the same index inside a window, from an opaque copy of the lane number (see ClCoords: not worth a register)
    auto own_idx = [&]() {
        uint32_t lo = lane;
        asm volatile("" : "+v"(lo));
        return n + wave * (Dg::BPW * n) + V * lo;
    };
    const uint32_t wl = (cnt - 1) / Dg::BPW, lb = (cnt - 1) - wl * Dg::BPW;   // the last knot: wave wl, lanes [LPB lb, LPB lb + LPB)
    const uint32_t POLL = wl == 7 ? 6u : 7u;                          // the polling wave: never wave 0, never wave wl
    size_t mstride = (size_t)3 * n * n * N;
    if constexpr (SHARED) {   // zero, but not a constant the compiler may build on: the code, and with it the registers, of the per-problem kernel
        mstride = 0;
        asm volatile("" : "+s"(mstride));
    }

    // this launch's number, in the tag bits above the epoch (epochs of a launch fit kClEpochBits: the host checked)
    const uint32_t nonce = cl_nonce(__hip_atomic_load(reinterpret_cast<u64 *>(ws) + kClLaunchWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const ClCoords k = {__builtin_amdgcn_make_buffer_rsrc(ws + kClCtrlBytes, 0, (int)(2u * grid * kClSlotBytes), 0x00020000),
                        blk * kClSlotBytes, grid * kClSlotBytes, blk, blk0, bstride, H, cnt, wl, lb, has_left, has_right, POLL,
                        nonce, spin_limit, drop_block};

    bool greeted = false;     // HELLO done
    bool same_xcd = false;    // every member of the cluster runs on this XCD: publish with plain stores (set by HELLO)
    bool dead = false;        // a hand-off of this cluster timed out: its remaining problems are left to the member that leaves last
    uint32_t first_dead = 0xffffffffu;   // ... from this problem on
    // problems of this cluster SOLVED BY THIS LAUNCH so far: the epochs of a problem continue where the last one stopped.
    // Problems another launch owns do not count: the first epochs a launch polls for must be 1 and 2 whatever the batch
    // holds.
    uint32_t ordinal = 0;
    const uint32_t epochs_per_problem = 2u * a.max_iter + 4u;
    uint32_t xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    xcc_id = (xcc_id & 0xfu) + 1u;   // never 0: a payload of its own kind

    GBDPCG_CL_STAMP_RT(21, 0, true)
    GBDPCG_CL_STAMP_WG(0)
    // Does this launch own ANY problem of this cluster?  In the default (tested) symmetric mode it usually owns none, and the
    // launch should cost as little as possible: the verdicts of 64 problems are fetched in one round trip, instead of one
    // round trip per problem in the loop below.  (Using the masks inside the loop too made its iterations 2 % slower:
    // register allocation.)
    bool any = a.sel == nullptr;
    for (uint32_t first = c; !any && first < a.batch; first += 64 * clusters) {
        const uint32_t left = (a.batch - first + clusters - 1) / clusters;
        any = pcg_takes_mask<SHARED>(a, first, clusters, left < 64 ? left : 64u, lane) != 0ull;
    }
    if (any) cl_clear_slot<T, LPB>(k, wave, lane);
    if (any) for (uint32_t prob = c; prob < a.batch; prob += clusters) {
        if (!pcg_takes<SHARED>(a, prob)) continue;   // this launch is not the one that owns the problem (same verdict in every member)
        if (dead) {
            cl_mark_given_up(a, prob, h == 0 && tid == 0);
            continue;
        }
        GBDPCG_CL_STAMP_RT(14, 0, ordinal == 3)
        T part;
        if (!greeted) {
            // HELLO (epoch 1): where does everybody run?  The payload of every partial granule is the sender's XCD id.
            greeted = true;
            T my_id, zeros[V];   // a partial whose words both read xcc_id
#pragma unroll
            for (int j = 0; j < V; ++j) zeros[j] = T(0);
            if constexpr (sizeof(T) == 4) my_id = __builtin_bit_cast(float, xcc_id);
            else my_id = __builtin_bit_cast(double, ((u64)xcc_id << 32) | xcc_id);
            if (tid == 0) bci[0] = 0u;
            cl_wg_barrier();
            same_xcd ? cl_publish<0, NCT, ONE>(k, wave, lane, 1u, my_id, zeros, lpart) : cl_publish<kSc1, NCT, ONE>(k, wave, lane, 1u, my_id, zeros, lpart);
            if constexpr (ONE) cl_wg_barrier();
            if (wave == POLL) {
                const ClGathered<T, V> g = cl_gather<NCT, V, ONE>(k, lane, 1u, xa, lpart);
                uint32_t lo = lane;
                asm volatile("" : "+v"(lo));
                const bool mine = lo >= PPM * H || (g.gotx == xcc_id && g.gotz == xcc_id);
                const bool all_here = __all(mine);
                if (lane == 0) {
                    bci[0] = g.ok ? 0u : 2u;
                    bci[1] = g.ok && all_here ? 1u : 0u;
                }
            }
            cl_wg_barrier();
            same_xcd = bci[1] != 0u && !no_plain;
            if (bci[0] == 2u) {   // the cluster never got together: nothing of it is solved here
                dead = true;
                first_dead = prob;
                cl_mark_given_up(a, prob, h == 0 && tid == 0);
                cl_wg_barrier();
                continue;
            }
        }
        const uint32_t e0 = 1u + ordinal * epochs_per_problem;   // epochs e0 + 1 .. e0 + 2 max_iter + 2 belong to this problem
        const T *S = a.S + prob * mstride;
        const T *P = a.Pinv ? a.Pinv + prob * mstride : nullptr;   // nullptr: identity preconditioner
        const size_t voff = (size_t)prob * len;

        // lambda and gamma of this lane's rows and the two halo knots of lambda (straight from the input vector: no member
        // writes lambda before every member has passed its first hand-off) are requested next to the first tile stages, so
        // that their round trips run under the 300 KB of tile loads instead of in front of the first product
        T lamv[V], gamv[V], halo_lam = T(0);
        auto request_vectors = [&]() {
            uint32_t lo = lane;
            asm volatile("" : "+v"(lo));   // addresses from the lane number, not from registers held since the kernel started
            const size_t g0 = voff + (size_t)k_lo * n + wave * (Dg::BPW * n) + V * lo;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                lamv[j] = dc.live ? a.lambda[g0 + j] : T(0);
                gamv[j] = dc.live ? a.gamma[g0 + j] : T(0);
            }
            const uint32_t t = wave * 64 + lo;
            if (t < 2 * n) {   // threads [0, n): the knot before the own ones, [n, 2n): the knot after them
                const int64_t gi = t < n ? (int64_t)k_lo * n - n + t : (int64_t)(k_lo + cnt) * n + (t - n);
                if (gi >= 0 && gi < (int64_t)len) halo_lam = a.lambda[voff + gi];
            }
        };

        DenseTile<T, NCT, V> tS, tP;
        if constexpr (STAGED) {
            GBDPCG_CL_STAMP(12, 0, ordinal == 0)
            dense_staged_load<T, NCT, V, PTAIL>(S, P, N, dc, wave, lane, k_lo, cnt, stage_raw, tS, tP,
                                      request_vectors);   // the vectors are requested behind the first two tile stages
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the last picks are in registers before anything else happens
            GBDPCG_CL_STAMP(13, 0, ordinal == 0)
            GBDPCG_CL_STAMP_RT(15, 0, ordinal == 3)
        } else {
            request_vectors();
            dense_load<T, NCT, V>(S, N, dc, tS);
            if (P) {
                // (direct loads: the tail goes through the registers, once per problem -- and first, so that its registers are free
                // again when the columns that stay arrive)
                dense_load<T, NCT, V, Dg::COLS - PTAIL, Dg::COLS>(P, N, dc, tP);
                if constexpr (PTAIL > 0) {
#pragma unroll
                    for (int t = 0; t < PTAIL; ++t) {
                        if constexpr (V == 2) ptail[t * 64 + lane] = TV{tP.a[Dg::COLS - PTAIL + t][0], tP.a[Dg::COLS - PTAIL + t][1]};
                        else ptail[t * 64 + lane] = tP.a[Dg::COLS - PTAIL + t][0];
                    }
                    asm volatile("" ::: "memory");
                }
                dense_load<T, NCT, V, 0, Dg::COLS - PTAIL>(P, N, dc, tP);
            } else {
#pragma unroll
                for (uint32_t cc = 0; cc < Dg::COLS; ++cc)
#pragma unroll
                    for (int j = 0; j < V; ++j) tP.a[cc][j] = T(0);
            }
        }

        T rv[V], pv[V], yv[V];
        // windows: lambda on the own knots and the halos, zeros behind them (rows past the own knots, halos at the ends
        // of the problem); every entry has exactly one writer
        if (dc.live) {
#pragma unroll
            for (int j = 0; j < V; ++j) xa[n + row0 + j] = lamv[j];
        }
        if (tid < 2 * n) {
            const uint32_t i = tid < n ? tid : (cnt + 1) * n + (tid - n);
            xa[i] = halo_lam;
            xb[i] = T(0);
        }
        {
            uint32_t t = tid;
            asm volatile("" : "+v"(t));
            for (uint32_t i = (cnt + 2) * n + t; i < WINF; i += THREADS) xa[i] = xb[i] = T(0);
        }
        if (tid == 0) bci[0] = 0u;
        cl_wg_barrier();
        GBDPCG_CL_STAMP_RT(16, 0, ordinal == 3)

        // r = gamma - S lambda                                            (pcg.cuh:118-126); the boundary knots of r travel
        dense_mv<T, NCT, V, CHAINS>(tS, xa, dc, yv);
#pragma unroll
        for (int j = 0; j < V; ++j) rv[j] = dc.live ? gamv[j] - yv[j] : T(0);
        if (dc.live) {
#pragma unroll
            for (int j = 0; j < V; ++j) xb[n + row0 + j] = rv[j];
        }
        same_xcd ? cl_publish<0, NCT, ONE>(k, wave, lane, e0 + 1u, T(0), rv, lpart) : cl_publish<kSc1, NCT, ONE>(k, wave, lane, e0 + 1u, T(0), rv, lpart);
        if constexpr (ONE) cl_wg_barrier();
        if (wave == POLL) {
            const ClGathered<T, V> g = cl_gather<NCT, V, ONE>(k, lane, e0 + 1u, xb, lpart);
            if (!g.ok && lane == 0) bci[0] = 2u;
            if (g.ok && g.hidx != 0xffffffffu) {
#pragma unroll
                for (int j = 0; j < V; ++j) xb[g.hidx + j] = g.gv[j];
            }
        }
        cl_wg_barrier();
        bool failed = bci[0] == 2u;
        GBDPCG_CL_STAMP_RT(17, 0, ordinal == 3)

        // r~ = Pinv r ; p = r~ ; eta = r.r~                               (pcg.cuh:130-149)
        T eta = T(0);
        if (!failed) {
            if (P) dense_mv<T, NCT, V, CHAINS, PTAIL>(tP, xb, dc, yv, pt_lane, 64, ptd_lane);
            part = T(0);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                pv[j] = P ? yv[j] : rv[j];
                part = fma_t(rv[j], pv[j], part);
            }
            part = wave_sum(part);
            if (dc.live) {   // every read of xa (as lambda) happened before the last barrier
#pragma unroll
                for (int j = 0; j < V; ++j) xa[n + row0 + j] = pv[j];
            }
            same_xcd ? cl_publish<0, NCT, ONE>(k, wave, lane, e0 + 2u, part, pv, lpart) : cl_publish<kSc1, NCT, ONE>(k, wave, lane, e0 + 2u, part, pv, lpart);
            if constexpr (ONE) cl_wg_barrier();
            if (wave == POLL) {
                const ClGathered<T, V> g = cl_gather<NCT, V, ONE>(k, lane, e0 + 2u, xa, lpart);
                if (lane == 0) {
                    if (!g.ok) bci[0] = 2u;
                    bc[0] = g.total;
                }
                if (g.ok && g.hidx != 0xffffffffu) {
#pragma unroll
                    for (int j = 0; j < V; ++j) xa[g.hidx + j] = g.gv[j];
                }
            }
            cl_wg_barrier();
            failed = bci[0] == 2u;
            eta = bc[0];
        }

        GBDPCG_CL_STAMP_RT(18, 0, ordinal == 3)
        uint32_t iter = 0;
        bool max_iter_exit = true;
        for (; !failed && iter < a.max_iter; ++iter) {                    // pcg.cuh:154
            // upsilon = S p ; alpha = eta / (p.upsilon)                   (pcg.cuh:156-169)
            GBDPCG_CL_STAMP(1, POLL, iter == 3 && ordinal == 0)
            GBDPCG_CL_STAMP(8, 0, iter == 3 && ordinal == 0)
            dense_mv<T, NCT, V, CHAINS>(tS, xa, dc, yv);
            part = T(0);
#pragma unroll
            for (int j = 0; j < V; ++j) part = fma_t(pv[j], yv[j], part);
            part = wave_sum(part);
            GBDPCG_CL_STAMP(2, POLL, iter == 3 && ordinal == 0)
            GBDPCG_CL_STAMP(9, 0, iter == 3 && ordinal == 0)
            const uint32_t e1 = e0 + 3u + 2u * iter;
            same_xcd ? cl_publish<0, NCT, ONE>(k, wave, lane, e1, part, yv, lpart) : cl_publish<kSc1, NCT, ONE>(k, wave, lane, e1, part, yv, lpart);
            if constexpr (ONE) cl_wg_barrier();
            GBDPCG_CL_STAMP(10, 0, iter == 3 && ordinal == 0)
            if (wave == POLL) {
                const ClGathered<T, V> g = cl_gather<NCT, V, ONE>(k, lane, e1, xb, lpart);
                GBDPCG_CL_STAMP(3, POLL, iter == 3 && ordinal == 0)
                const T al = eta / g.total;
                if (lane == 0) {
                    if (!g.ok) bci[0] = 2u;
                    bc[0] = al;
                }
                // r -= alpha upsilon on the halo knots: the owner's fma on the owner's bits
                if (g.ok && g.hidx != 0xffffffffu) {
#pragma unroll
                    for (int j = 0; j < V; ++j) xb[g.hidx + j] = fma_t(-al, g.gv[j], g.hv[j]);
                }
            }
            cl_wg_barrier();
            GBDPCG_CL_STAMP(4, POLL, iter == 3 && ordinal == 0)
            if (bci[0] == 2u) { failed = true; break; }
            const T alpha = bc[0];
            // lambda += alpha p ; r -= alpha upsilon                      (pcg.cuh:172-176)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                lamv[j] = fma_t(alpha, pv[j], lamv[j]);
                rv[j] = fma_t(-alpha, yv[j], rv[j]);
            }
            if (dc.live) {
                const uint32_t oi = own_idx();
#pragma unroll
                for (int j = 0; j < V; ++j) xb[oi + j] = rv[j];
            }
            cl_wg_barrier();
            GBDPCG_CL_STAMP(5, POLL, iter == 3 && ordinal == 0)
            // r~ = Pinv r ; eta_new = r.r~                                (pcg.cuh:180-193)
            if (P) dense_mv<T, NCT, V, CHAINS, PTAIL>(tP, xb, dc, yv, pt_lane, 64, ptd_lane);
            part = T(0);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (!P) yv[j] = rv[j];
                part = fma_t(rv[j], yv[j], part);
            }
            part = wave_sum(part);
            same_xcd ? cl_publish<0, NCT, ONE>(k, wave, lane, e1 + 1u, part, yv, lpart) : cl_publish<kSc1, NCT, ONE>(k, wave, lane, e1 + 1u, part, yv, lpart);
            if constexpr (ONE) cl_wg_barrier();
            if (wave == POLL) {
                const ClGathered<T, V> g = cl_gather<NCT, V, ONE>(k, lane, e1 + 1u, xa, lpart);
                const bool conv = fabs(g.total) < a.tol;                 // pcg.cuh:195
                const T be = g.total / eta;                           // pcg.cuh:199
                if (lane == 0) {
                    bci[0] = !g.ok ? 2u : (conv ? 1u : 0u);
                    bc[0] = g.total;
                    bc[1] = be;
                }
                // p = r~ + beta p on the halo knots                       (pcg.cuh:203-206)
                if (g.ok && !conv && g.hidx != 0xffffffffu) {
#pragma unroll
                    for (int j = 0; j < V; ++j) xa[g.hidx + j] = fma_t(be, g.hv[j], g.gv[j]);
                }
            }
            cl_wg_barrier();
            const uint32_t verdict = bci[0];
            if (verdict == 2u) { failed = true; break; }
            if (verdict == 1u) {
                ++iter;
                max_iter_exit = false;
                break;
            }
            GBDPCG_CL_STAMP(6, POLL, iter == 3 && ordinal == 0)
            const T beta = bc[1];
            eta = bc[0];
#pragma unroll
            for (int j = 0; j < V; ++j) pv[j] = fma_t(beta, pv[j], yv[j]);
            if (dc.live) {
                const uint32_t oi = own_idx();
#pragma unroll
                for (int j = 0; j < V; ++j) xa[oi + j] = pv[j];
            }
            cl_wg_barrier();
            GBDPCG_CL_STAMP(7, POLL, iter == 3 && ordinal == 0)
        }

        GBDPCG_CL_STAMP_RT(19, 0, ordinal == 3)
        // outputs                                                         (pcg.cuh:212,215)
        if (dc.live && !failed) {
            // (the row index from an opaque copy of the lane number: as three 64-bit addresses computed in front of the problem
            // loop these were the kernel's last spills to scratch)
            uint32_t lo = lane;
            asm volatile("" : "+v"(lo));
            const size_t g = voff + (size_t)k_lo * n + wave * (Dg::BPW * n) + V * lo;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                a.lambda[g + j] = lamv[j];
                if (a.r) a.r[g + j] = rv[j];
                if (a.p) a.p[g + j] = pv[j];
            }
        }
        if (failed) cl_mark_given_up(a, prob, h == 0 && tid == 0);
        else if (h == 0 && tid == 0) {
            a.iters[prob] = iter;
            if (a.max_iter_exit) a.max_iter_exit[prob] = max_iter_exit ? 1 : 0;
        }
        dead = failed;
        if (failed) first_dead = prob;
        cl_wg_barrier();   // the windows and bci are reused by the next problem
        GBDPCG_CL_STAMP_RT(20, 0, ordinal == 3)
        ++ordinal;
    }

    GBDPCG_CL_STAMP_RT(22, 0, true)
    // ---- a cluster that could not meet: the member that leaves last solves what was given up, alone -------------------------
    // Every member that gave up did so on the same problem (nobody gets past a problem without everybody's hand-offs; the
    // one exception -- a member stalled for the whole spin bound exactly at a problem's last hand-off, which then finishes
    // that problem while its partner has given it up -- is why the members report the problem and the smallest one wins:
    // that problem is then solved again, by the streaming kernel, to the same tolerance).  The counter is bumped after the
    // report (s_waitcnt in between), both with agent-scope atomics; the last member puts both words back.  A healthy launch
    // pays one atomic per workgroup for it, and no caller ever sees an unsolved problem.
    if (any && !a.rescue_off && a.rescue_vec) {
        u64 *left = reinterpret_cast<u64 *>(ws + kClLeftOff) + 2 * c;
        if (tid == 0) {
            if (dead) __hip_atomic_fetch_max(left + 1, (u64)(0xffffffffu - first_dead), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const u64 before = __hip_atomic_fetch_add(left, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t from = 0xffffffffu;
            if (before == H - 1u) {
                const u64 worst = __hip_atomic_exchange(left + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(left, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (worst != 0ull) from = 0xffffffffu - (uint32_t)worst;
            }
            bci[2] = from;
        }
        __syncthreads();
        const uint32_t from = bci[2];
        if (from != 0xffffffffu) {
            T *vec = reinterpret_cast<T *>(a.rescue_vec) + (size_t)c * rescue_vec_elems<T>(n, N);
            for (uint32_t prob = from; prob < a.batch; prob += clusters)
                if (pcg_takes<SHARED>(a, prob)) stream_rescue<T, Dg::WAVES, SHARED>(a, prob, vec, rescue_red);
        }
    }
    // ---- the workgroup that finishes last gives the next launch its number ------------------------------------------------
    // (every workgroup of this launch has read the number by then; the counter and the number are only ever touched with
    // agent-scope atomics)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        u64 *ctl = reinterpret_cast<u64 *>(ws);
        const u64 before = __hip_atomic_fetch_add(ctl + kClFinishedWord, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == grid - 1u) {
            __hip_atomic_store(ctl + kClFinishedWord, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(ctl + kClLaunchWord, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    pcg_reject_leave(a);   // (a launch that got here behind a verifying launch: some problem was rejected)
    GBDPCG_CL_STAMP_WG(1)
}
#undef GBDPCG_CL_STAMP
#undef GBDPCG_CL_STAMP_WG
#undef GBDPCG_CL_STAMP_RT

// What the kernel is built for: X(element type, block size, rows per lane).  A lane's rows of one column are 8 bytes at most
// (two fp32 rows, or one fp64 / fp32 row), n / V <= 16 lanes make a knot, and the matrix registers per lane must leave room for
// the working set (cluster_tail_cols).  fp64 at the BASELINE block size runs one row per lane: 14 lanes per knot, 32 knots per
// workgroup, four workgroups for N = 128.  The odd sizes (one fp32 row per lane) take direct tile loads -- their blocks are not
// whole 16-byte pieces -- and one accumulator chain per row.
#define GBDPCG_CLUSTER_SHAPES(X) \
    X(float, 2, 2) X(float, 3, 1) X(float, 4, 2) X(float, 5, 1) X(float, 6, 2) X(float, 7, 1) \
    X(float, 8, 2) X(float, 9, 1) X(float, 10, 2) X(float, 11, 1) X(float, 12, 2) X(float, 13, 1) X(float, 14, 2) X(float, 15, 1) X(float, 16, 2) \
    X(float, 18, 2) \
    X(double, 2, 1) X(double, 3, 1) X(double, 4, 1) X(double, 5, 1) X(double, 6, 1) X(double, 7, 1) X(double, 8, 1) X(double, 9, 1) X(double, 10, 1) X(double, 11, 1) X(double, 12, 1) \
    X(double, 13, 1) X(double, 14, 1) X(double, 15, 1) X(double, 16, 1)
constexpr uint32_t kClusterMaxBlock = 18;   // the largest block size of the list

// What the host needs to know of a shape: knots per workgroup (0: not built for the block size), ClusterLight, whether it has the
// cluster-of-one instantiation, elements of the in-kernel rescue's vectors at the longest horizon the path takes.
struct ClusterShape { uint32_t per_wg; bool light, one; size_t rescue_elems; };
// A cluster of one exists where the block size has such launches: no single-workgroup kernel in pcg_resident.hip (fp32 16 and 18,
// fp64 14, 15, 16).
template <typename T, int NN> constexpr bool cluster_has_one()
{
    return !ClusterLight<T, NN>::value && ((sizeof(T) == 4 && NN >= 16) || (sizeof(T) == 8 && NN >= 14));
}
template <typename T, int NN, int VV> static ClusterShape cluster_shape_of()
{
    static_assert(NN <= kClusterMaxBlock, "kClusterMaxBlock");
    constexpr uint32_t per_wg = DenseGeom<T, NN, VV>::MAX_KNOTS;
    return {per_wg, ClusterLight<T, NN>::value, cluster_has_one<T, NN>(), rescue_vec_elems<T>(NN, cl_max_members<T>() * per_wg)};
}
static ClusterShape cluster_shape(size_t elem_size, uint32_t n)
{
#define GBDPCG_X(TT, NN, VV) if (elem_size == sizeof(TT) && n == NN) return cluster_shape_of<TT, NN, VV>();
    GBDPCG_CLUSTER_SHAPES(GBDPCG_X)
#undef GBDPCG_X
    return {0, false, false, 0};
}

// General storage, horizons beyond what ONE workgroup keeps in registers (pcg_resident.hip: 8 waves x floor(64 / (n / V)) knots
// -- 72 at n = 14 in fp32) up to eight (fp64: four) times that.  GBDPCG_NO_CLUSTER disables the path (tuning runs).
template <typename T> uint32_t cluster_members(uint32_t n, uint32_t N)
{
    static const bool off = getenv("GBDPCG_NO_CLUSTER") != nullptr;
    if (off) return 0;
    const uint32_t per_wg = cluster_shape(sizeof(T), n).per_wg;
    if (per_wg == 0) return 0;                  // not built for the block size
    // one workgroup holds the whole problem: pcg_resident.hip where it is built for the block size (its reductions stay in LDS); a
    // "cluster" of one elsewhere (16 and 18, fp64 from 14 on) -- the kernel's ONE instantiation, whose wave partials meet in LDS
    if (N <= per_wg && resident_shape<T>(n, N)) return 0;
    static const bool no_single = getenv("GBDPCG_NO_CLUSTER_OF_ONE") != nullptr;   // tuning runs
    // (n = 2 below 16 knots stays with the streaming kernel, as in pcg_resident.hip: the reference's own example system lives there)
    if (N <= per_wg && (no_single || N < 2 || (n == 2 && N < 16))) return 0;
    const uint32_t H = (N + per_wg - 1) / per_wg;
    return H <= cl_max_members<T>() ? H : 0;
}

// ... plus 16 bytes per CU behind the slots: start / end of every workgroup on the real-time clock (diagnostic build only)
// (slots for two workgroups per CU: the light instantiations run two -- cluster_wgs_per_cu)
size_t cluster_workspace_bytes(const DeviceInfo &dev) { return kClCtrlBytes + (size_t)2 * (2 * dev.num_cus) * kClSlotBytes + (size_t)(2 * dev.num_cus) * 16; }

// Device memory for the in-kernel rescue: one set of vectors per cluster, sized for the longest horizon the path takes.
size_t cluster_rescue_bytes(const DeviceInfo &dev)
{
    size_t bytes = 0;
    for (size_t elem_size : {sizeof(float), sizeof(double)})
        for (uint32_t n = 1; n <= kClusterMaxBlock; ++n) bytes = std::max(bytes, cluster_shape(elem_size, n).rescue_elems * elem_size);
    return (size_t)dev.num_cus * bytes;   // (a cluster may be a single workgroup)
}

// The instantiation for a launch: STAGED only where the tiles can be staged, ONE only where the shape has clusters of one.
template <typename T> using ClusterKernel = void (*)(PcgArgs<T>, unsigned char *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, bool);
template <typename T, int NN, int VV> static ClusterKernel<T> cluster_kernel(bool staged, bool one, bool shared)
{
    if constexpr (cluster_has_one<T, NN>()) {
        if (one) {
            if constexpr (DenseStage<T, NN, VV>::OK) {
                if (staged) return shared ? pcg_cluster_kernel<T, NN, VV, true, true, true> : pcg_cluster_kernel<T, NN, VV, true, true>;
            }
            return shared ? pcg_cluster_kernel<T, NN, VV, false, true, true> : pcg_cluster_kernel<T, NN, VV, false, true>;
        }
    }
    if constexpr (DenseStage<T, NN, VV>::OK) {
        if (staged) return shared ? pcg_cluster_kernel<T, NN, VV, true, false, true> : pcg_cluster_kernel<T, NN, VV, true>;
    }
    return shared ? pcg_cluster_kernel<T, NN, VV, false, false, true> : pcg_cluster_kernel<T, NN, VV, false>;
}

template <typename T, int NN, int VV>
static bool launch_pcg_cluster_n(const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool shared, uint32_t H, uint32_t C, uint32_t clusters,
                                 uint32_t spin_limit, uint32_t drop_block)
{
    // coalesced LDS-DMA tile loads need 16-byte aligned matrices (every hipMalloc'ed buffer is)
    static const bool no_staging = getenv("GBDPCG_CLUSTER_DIRECT_LOADS") != nullptr;   // tuning runs only
    static const bool no_plain = getenv("GBDPCG_CLUSTER_NO_PLAIN") != nullptr;          // tuning runs: always sc1 stores
    const bool aligned16 = !((reinterpret_cast<uintptr_t>(a.S) | reinterpret_cast<uintptr_t>(a.Pinv)) % 16);
    const bool staged = DenseStage<T, NN, VV>::OK && !no_staging && aligned16;
    size_t lds = (size_t)ClusterTail<T, NN>::COLS * 512 * 8;
    if (staged) lds = std::max(lds, dense_stage_lds_bytes<T, NN, VV>());
    const ClusterKernel<T> kern = cluster_kernel<T, NN, VV>(staged, H == 1, shared);
    // on every launch, like the other launchers: HIP keeps the attribute per device
    if (lds) {
        *err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (*err != hipSuccess) return true;
    }
    hipLaunchKernelGGL(kern, dim3(clusters * H), dim3(512), lds, s, a, static_cast<unsigned char *>(a.cluster_ws), H, C, clusters, spin_limit,
                       drop_block, no_plain);
    *err = hipGetLastError();
    return true;
}

template <typename T>
bool launch_pcg_cluster(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool shared)
{
    const uint32_t H = cluster_members<T>(a.n, a.N);
    if (H == 0 || !a.cluster_ws || a.symmetric) return false;
    if ((reinterpret_cast<uintptr_t>(a.S) % 8) || (a.Pinv && reinterpret_cast<uintptr_t>(a.Pinv) % 8)) return false;
    // one workgroup per CU: a cluster's members are resident together -- two where the instantiation is light enough for two to
    // share a CU (ClusterLight: at most 128 VGPRs, no dynamic LDS, and always two or more members, pcg_resident.hip having the
    // short horizons: so never more than CU-count clusters, which is what the control words hold)
    static const int per_cu_env = [] { const char *e = getenv("GBDPCG_CLUSTER_PER_CU"); return e ? atoi(e) : 0; }();   // tuning runs
    const bool light = cluster_shape(sizeof(T), a.n).light && H >= 2;
    const uint32_t per_cu = light ? (per_cu_env ? (uint32_t)per_cu_env : 2u) : 1u;
    uint32_t clusters = (uint32_t)dev.num_cus * (per_cu > 2 ? 2u : per_cu) / H;
    if (clusters > a.batch) clusters = a.batch;
    if (clusters == 0) return false;
    const uint32_t rounds = (a.batch + clusters - 1) / clusters;
    // a tag = {launch number, epoch}: the epochs of a launch take the low kClEpochBits of its 32 bits
    const double epochs = 2.0 + (double)rounds * (2.0 * a.max_iter + 4.0);
    if (epochs >= (double)(1u << kClEpochBits)) return false;
    const uint32_t C = (a.N + H - 1) / H;
    uint32_t spin_limit = 1u << 21;      // polls before a hand-off is given up (~1 us per poll: about two seconds per bound; a member
                                         // that arrives late spins its own bound after the others': up to two bounds, then the streaming solve)
    uint32_t drop_block = 0xffffffffu;
    PcgArgs<T> ka = a;
    ka.rescue_off = false;
#ifdef GBDPCG_TEST_HOOKS
    // variants/libgbdpcg_hooks.so only (tests/test_gpu_cluster.py): a short bound, and a workgroup that never publishes
    if (const char *e = getenv("GBDPCG_CLUSTER_SPIN_LIMIT")) spin_limit = (uint32_t)strtoul(e, nullptr, 10);
    if (const char *e = getenv("GBDPCG_CLUSTER_DROP_WG")) drop_block = (uint32_t)strtoul(e, nullptr, 10);
    ka.rescue_off = getenv("GBDPCG_RESCUE_OFF") != nullptr;   // show a test what a cluster that gave up leaves behind
#endif
#define GBDPCG_X(TT, NN, VV)                           \
    if constexpr (sizeof(T) == sizeof(TT)) {           \
        if (a.n == NN) return launch_pcg_cluster_n<T, NN, VV>(ka, s, err, shared, H, C, clusters, spin_limit, drop_block); \
    }
    GBDPCG_CLUSTER_SHAPES(GBDPCG_X)
#undef GBDPCG_X
    return false;
}

template uint32_t cluster_members<float>(uint32_t, uint32_t);
template uint32_t cluster_members<double>(uint32_t, uint32_t);
template bool launch_pcg_cluster<float>(const DeviceInfo &, const PcgArgs<float> &, hipStream_t, hipError_t *, bool);
template bool launch_pcg_cluster<double>(const DeviceInfo &, const PcgArgs<double> &, hipStream_t, hipError_t *, bool);

}  // namespace gbdpcg
