// pcg_persist_handoff.hpp -- what the persistent kernels (pcg_persist_2r.hpp, pcg_persist_1r.hpp) pass between CUs and how: the
// control words, the tagged value slots, the workspace layout, the polling sweep, leaving a launch.  Nothing else is in here.
//
// PCG for ONE large problem spread over many CUs inside a single persistent launch.
//
// Replaces pcg<T,n,N> (include/pcg.cuh:54-218 of the reference) for problems whose vectors do not fit one
// workgroup (BASELINE config 4: n = 36, N = 256, fp64).  The reference gives every knot a block, keeps the
// knot's block-rows of S and Pinv in shared memory for the whole solve (pcg.cuh:104-110) and crosses the grid
// four times per iteration with grid.sync() (pcg.cuh:166,178,190,207).  Here:
//
//   * a workgroup owns K consecutive knots (K = 2, 3 or 1, tried in that order; 64 * ceil(n / 8) threads per knot) and keeps
//     their block-rows [L|D|R] of S and Pinv in REGISTERS for the whole solve: 8 lanes share a row, each holds a contiguous
//     run of COLS columns of that row of both matrices (pcg_persist_geom.hpp; n = 36: 14 columns, 56 VGPRs in fp64).  The
//     matrices are read from HBM once per solve; an iteration touches only LDS and the hand-off words below.
//   * the iteration is cut at its two inner products, as in the split path, but the cut is an in-kernel
//     ALL-GATHER instead of a kernel boundary: after a product every workgroup publishes, in one go, its
//     partial of the inner product AND the two boundary knots of the product vector that its neighbours need
//     (the residual / direction of a neighbour's halo knot is then updated redundantly, so the two axpy
//     barriers of the reference disappear).  Every workgroup then sums all partials in the same order -> the same
//     bits everywhere -> the exit test of pcg.cuh:195 stays uniform, exactly what pcg.cuh:147,167,191 ensure.
//     Two such round trips per iteration: the inner products of textbook PCG depend on each other.
//   * hand-off words are data-tagged 8-byte granules {epoch, 32 value bits} written and polled with agent-scope
//     relaxed atomics (sc1 write-through stores / sc1 loads: MI355X_MICROARCH.md, "Valid forms", R2): the data is
//     the flag, so there is no fence and no separate flag round trip.  An fp64 value is two granules.  Slots are
//     double-buffered by epoch parity (a producer can be at most one epoch ahead of any consumer); epochs continue
//     from a per-problem base kept in the workspace, so nothing has to be cleared between launches and the whole
//     solve is ONE kernel node in a hipGraph.
//   * one workgroup per CU at most (grid <= CU count), every spin is bounded: a launch that cannot get all its
//     workgroups resident gives up instead of hanging -- nothing of the problem is written -- and the workgroup that
//     finishes LAST (an agent-scope counter tells it; the others have left by then) solves the problem alone,
//     streaming, inside this same launch (pcg_stream.hpp, stream_rescue): no caller sees an unsolved problem.  The
//     same workgroup stores the epoch base of the next launch: a workgroup that only got onto the device after the
//     others had given up still publishes under THIS launch's epochs, and whatever it leaves in its slots is older than
//     anything the next launch polls for.
#pragma once

#include <cstdlib>
#include <type_traits>

#include "handoff_words.hpp"
#include "pcg_stream.hpp"

namespace gbdpcg {

#define GBDPCG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// u64 control words per problem (lines of their own): [0] epoch base of the next launch, [1..15] stamps of the diagnostic
// build, [16] workgroups of the running launch that have finished
constexpr uint32_t kPersistCtrl = 32, kPersistFinished = 16;

// Leaving a problem's launch (all threads of the workgroup).  The last workgroup to get here stores the next launch's epoch
// base -- every workgroup has read `base` by then, and every granule this launch wrote carries a tag below base + span --
// and, if any workgroup reports that the launch gave up, solves the problem alone (the others have left and have written
// nothing).  [kPersistFinished] counts the workgroups that have left, [kPersistFinished + 1] is non-zero once one of them
// gave up; the last one puts both back.  red: 2 * WAVES elements of LDS, flag: one word of LDS.
template <typename T, int WAVES>
__device__ __forceinline__ void persist_leave(const PcgArgs<T> &a, uint32_t prob, u64 *ws, uint32_t W, uint32_t base, uint32_t span,
                                              bool failed, T *red, uint32_t *flag)
{
    if (threadIdx.x == 0) {
        if (failed) __hip_atomic_fetch_max(ws + kPersistFinished + 1, 1ull, GBDPCG_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 before = __hip_atomic_fetch_add(ws + kPersistFinished, 1ull, GBDPCG_RLX_AGENT);
        uint32_t rescue = 0u;
        if (before == W - 1u) {
            rescue = __hip_atomic_exchange(ws + kPersistFinished + 1, 0ull, GBDPCG_RLX_AGENT) != 0ull ? 1u : 0u;
            __hip_atomic_store(ws + kPersistFinished, 0ull, GBDPCG_RLX_AGENT);
            __hip_atomic_store(ws, (u64)(base + span), GBDPCG_RLX_AGENT);
        }
        *flag = rescue;
    }
    __syncthreads();
    if (*flag != 0u && !a.rescue_off && a.rescue_vec)
        stream_rescue<T, WAVES>(a, prob, reinterpret_cast<T *>(a.rescue_vec) + (size_t)prob * rescue_vec_elems<T>(a.n, a.N), red);
}

// tests/test_gpu_persist.py, variants/libgbdpcg_hooks.so only (-DGBDPCG_TEST_HOOKS): hold workgroup `hold_wg` of every
// problem back for `hold_us` microseconds before it reads anything -- a workgroup that gets onto the device late.
__device__ __forceinline__ void persist_hold(uint32_t block, uint32_t hold_wg, uint32_t hold_us)
{
#ifdef GBDPCG_TEST_HOOKS
    if (hold_us != 0u && block == hold_wg) {
        const u64 until = __builtin_amdgcn_s_memrealtime() + (hold_us == 0xffffffffu ? 0ull : (u64)hold_us * 100ull);
        while (__builtin_amdgcn_s_memrealtime() < until) __builtin_amdgcn_s_sleep(64);
    }
#endif
}
// ... and GBDPCG_PERSIST_DROP_WG (hold_us == 0xffffffff): the last workgroup of the grid leaves at once, publishing nothing.
// True when it has left: the kernel returns.
template <typename T, int WAVES>
__device__ __forceinline__ bool persist_drop(const PcgArgs<T> &a, uint32_t prob, u64 *ws, uint32_t W, uint32_t base, uint32_t span,
                                             uint32_t hold_us, T *red, uint32_t *flag)
{
#ifdef GBDPCG_TEST_HOOKS
    if (hold_us == 0xffffffffu && blockIdx.x == gridDim.x - 1u) {
        persist_leave<T, WAVES>(a, prob, ws, W, base, span, true, red, flag);
        return true;
    }
#endif
    return false;
}

template <typename T> struct Gran;
template <> struct Gran<float> { static constexpr uint32_t PER = 1; };
template <> struct Gran<double> { static constexpr uint32_t PER = 2; };

// One value slot = Gran<T>::PER adjacent granules; read with ONE sc1 buffer load (8 bytes for fp32, 16 for fp64: each
// 8-byte half carries its own tag, so a torn 16-byte read is detected, not consumed).  off = byte offset in the region.
__device__ __forceinline__ bool slot_load(__amdgpu_buffer_rsrc_t region, uint32_t off, uint32_t epoch, float &v)
{
    const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(region, (int)off, 0, kSc1);
    v = __builtin_bit_cast(float, x.x);
    return x.y == epoch;
}
__device__ __forceinline__ bool slot_load(__amdgpu_buffer_rsrc_t region, uint32_t off, uint32_t epoch, double &v)
{
    const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(region, (int)off, 0, kSc1);
    v = __builtin_bit_cast(double, ((u64)x.z << 32) | x.x);
    return x.y == epoch && x.w == epoch;
}

// ... and written with ONE sc1 (write-through) buffer store: 288 eight-byte stores from one wave were the longest leg
// of a hand-off; a 16-byte sc1 store keeps each 8-byte half whole (MI355X_MICROARCH.md, Valid forms, R2).
__device__ __forceinline__ void slot_store(__amdgpu_buffer_rsrc_t region, uint32_t off, uint32_t epoch, float v)
{
    const u32x2 x = {__builtin_bit_cast(uint32_t, v), epoch};
    __builtin_amdgcn_raw_buffer_store_b64(x, region, (int)off, 0, kSc1);
}
__device__ __forceinline__ void slot_store(__amdgpu_buffer_rsrc_t region, uint32_t off, uint32_t epoch, double v)
{
    const u64 b = __builtin_bit_cast(u64, v);
    const u32x4 x = {(uint32_t)b, epoch, (uint32_t)(b >> 32), epoch};
    __builtin_amdgcn_raw_buffer_store_b128(x, region, (int)off, 0, kSc1);
}

// Bytes between the partial-product slots of two workgroups.  A slot of its own 128-byte line keeps 8 producers from
// writing into one line that every consumer polls.
#ifndef GBDPCG_PERSIST_PSTRIDE
#define GBDPCG_PERSIST_PSTRIDE 128
#endif
constexpr uint32_t kPartStrideWords = GBDPCG_PERSIST_PSTRIDE / 8;
#ifndef GBDPCG_PERSIST_SLEEP0
#define GBDPCG_PERSIST_SLEEP0 0
#endif

// Workspace of one problem, in u64 words: [ctrl | part[2][N] slots | halo[2][N][2][n] values | halo2 (same)], sized for one knot
// per workgroup (the largest workgroup count), whatever K a launch uses.
template <typename T> __host__ __device__ inline size_t persist_part_words(uint32_t N)
{
    return (size_t)2 * N * (kPartStrideWords > Gran<T>::PER ? kPartStrideWords : Gran<T>::PER);
}
template <typename T> __host__ __device__ inline size_t persist_halo_words(uint32_t n, uint32_t N)
{
    return (size_t)2 * N * 2 * n * Gran<T>::PER;
}
// ... followed by a second halo region of the same size, used by the single-reduction kernel only (its extra hand-off)
template <typename T> __host__ __device__ inline size_t persist_words(uint32_t n, uint32_t N)
{
    return kPersistCtrl + persist_part_words<T>(N) + 2 * persist_halo_words<T>(n, N);
}

// Wave 0 of a workgroup: poll until every partial of this epoch and the two neighbour boundary vectors have
// arrived (sc1 loads, no fence: the data is the flag), then sum the partials in a fixed order.  Every lane re-reads
// only the slots it is still missing and sleeps between passes: polling traffic competes with the very stores it is
// waiting for (measured on config 4: keeping two / three polls in flight per slot made an iteration 19 % / 36 % slower).
// part_off: byte offset of this epoch parity's partial slots in the region; hl_off / hr_off: byte offsets of the left /
// right neighbour's boundary vector (negative: no neighbour).  Returns false when the spin bound is hit.
#ifndef GBDPCG_PERSIST_GAP
#define GBDPCG_PERSIST_GAP 1
#endif
template <typename T, int NCT, uint32_t PJ, uint32_t NV, uint32_t HN = NCT>
__device__ __forceinline__ bool persist_sweep_w(__amdgpu_buffer_rsrc_t region, uint32_t part_off, int hl_off, int hr_off,
                                                uint32_t W, uint32_t epoch, uint32_t lane, uint32_t spin_limit, T (&total)[NV ? NV : 1],
                                                T *yl, T *yr)
{
    // NV values per partial slot, adjacent (0: neighbours only, nothing is summed); HN values per neighbour boundary
    constexpr uint32_t PER = Gran<T>::PER, PSTRIDE = (kPartStrideWords > PER ? kPartStrideWords : PER) * 8;
    constexpr uint32_t NS = NV ? PJ * NV : 1, HV = (HN + 63) / 64;
    static_assert(NV * PER * 8 <= PSTRIDE, "the values of a slot share its line");
    T pv[NS], hl[HV], hr[HV];
    bool have[NS], have_l[HV], have_r[HV];
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j) {
        pv[j] = T(0);
        have[j] = NV == 0 || lane + 64 * (j / (NV ? NV : 1)) >= W;
    }
#pragma unroll
    for (uint32_t v = 0; v < HV; ++v) {
        hl[v] = hr[v] = T(0);
        have_l[v] = hl_off < 0 || lane + 64 * v >= HN;
        have_r[v] = hr_off < 0 || lane + 64 * v >= HN;
    }
    if (GBDPCG_PERSIST_SLEEP0) __builtin_amdgcn_s_sleep(GBDPCG_PERSIST_SLEEP0);
    // Two stages: the partials first (everybody's: the wait proper), the neighbours' boundary knots afterwards (published
    // at the same time, so normally one pass): the fewer loads are in flight during the wait, the sooner it ends.
    uint32_t spins = 0;
#ifdef GBDPCG_PERSIST_TWO_STAGE_ALWAYS
    constexpr bool TWO_STAGE = NV > 0;
#else
    constexpr bool TWO_STAGE = NV > 0 && NS + 2 * HV > 4;
#endif   // few loads per lane: one stage is as fast (measured, config 4)
    if constexpr (TWO_STAGE) {
        for (;; ++spins) {
            bool all = true;
#pragma unroll
            for (uint32_t j = 0; j < NS; ++j) {
                if (!have[j])
                    have[j] = slot_load(region, part_off + (lane + 64 * (j / (NV ? NV : 1))) * PSTRIDE + (j % (NV ? NV : 1)) * PER * 8,
                                        epoch, pv[j]);
                all = all && have[j];
            }
            if (__all(all)) break;
            if (spins >= spin_limit) return false;
            __builtin_amdgcn_s_sleep(GBDPCG_PERSIST_GAP);
        }
    }
    for (;; ++spins) {
        bool all = true;
        if constexpr (NV > 0 && !TWO_STAGE) {
#pragma unroll
            for (uint32_t j = 0; j < NS; ++j) {
                if (!have[j])
                    have[j] = slot_load(region, part_off + (lane + 64 * (j / (NV ? NV : 1))) * PSTRIDE + (j % (NV ? NV : 1)) * PER * 8,
                                        epoch, pv[j]);
                all = all && have[j];
            }
        }
#pragma unroll
        for (uint32_t v = 0; v < HV; ++v) {
            if (!have_l[v]) have_l[v] = slot_load(region, (uint32_t)hl_off + (lane + 64 * v) * PER * 8, epoch, hl[v]);
            if (!have_r[v]) have_r[v] = slot_load(region, (uint32_t)hr_off + (lane + 64 * v) * PER * 8, epoch, hr[v]);
            all = all && have_l[v] && have_r[v];
        }
        if (__all(all)) break;
        if (spins >= spin_limit) return false;
        __builtin_amdgcn_s_sleep(GBDPCG_PERSIST_GAP);
    }
    if constexpr (NV > 0) {
#pragma unroll
        for (uint32_t v = 0; v < NV; ++v) {
            T sum = pv[v];
#pragma unroll
            for (uint32_t j = 1; j < PJ; ++j) sum += pv[j * NV + v];
            total[v] = wave_sum(sum);
        }
    }
#pragma unroll
    for (uint32_t v = 0; v < HV; ++v)
        if (lane + 64 * v < HN) {
            yl[lane + 64 * v] = hl[v];
            yr[lane + 64 * v] = hr[v];
        }
    return true;
}
// partial slots per lane by workgroup count: the sums of the three forms differ only in how many zeros they add
template <typename T, int NCT, uint32_t NV, uint32_t HN = NCT>
__device__ __forceinline__ bool persist_sweep_n(__amdgpu_buffer_rsrc_t region, uint32_t part_off, int hl_off, int hr_off,
                                                uint32_t W, uint32_t epoch, uint32_t lane, uint32_t spin_limit,
                                                T (&total)[NV ? NV : 1], T *yl, T *yr)
{
    if (NV == 0 || W <= 64) return persist_sweep_w<T, NCT, 1, NV, HN>(region, part_off, hl_off, hr_off, W, epoch, lane, spin_limit, total, yl, yr);
    if (W <= 128) return persist_sweep_w<T, NCT, 2, NV, HN>(region, part_off, hl_off, hr_off, W, epoch, lane, spin_limit, total, yl, yr);
    return persist_sweep_w<T, NCT, 4, NV, HN>(region, part_off, hl_off, hr_off, W, epoch, lane, spin_limit, total, yl, yr);
}
template <typename T, int NCT>
__device__ __forceinline__ bool persist_sweep(__amdgpu_buffer_rsrc_t region, uint32_t part_off, int hl_off, int hr_off,
                                              uint32_t W, uint32_t epoch, uint32_t lane, uint32_t spin_limit, T &total,
                                              T *yl, T *yr)
{
    T tot[1];
    const bool ok = persist_sweep_n<T, NCT, 1>(region, part_off, hl_off, hr_off, W, epoch, lane, spin_limit, tot, yl, yr);
    total = tot[0];
    return ok;
}

// One problem's workspace as a kernel sees it.  region: the words behind the control words as a buffer resource for the slot
// loads and stores (byte offsets from `part`); halo_base: byte offset of the first halo region; base: the epochs of this
// launch continue from here.
struct PersistWorkspace {
    u64 *ws, *part;
    __amdgpu_buffer_rsrc_t region;
    uint32_t halo_base, base;
};
template <typename T> __device__ __forceinline__ PersistWorkspace persist_workspace(u64 *ws_all, uint32_t prob, uint32_t n, uint32_t N)
{
    PersistWorkspace h;
    h.ws = ws_all + (size_t)prob * persist_words<T>(n, N);
    h.part = h.ws + kPersistCtrl;   // [2][N] partial slots
    h.region = __builtin_amdgcn_make_buffer_rsrc(h.part, 0, (int)((persist_words<T>(n, N) - kPersistCtrl) * 8), 0x00020000);
    h.halo_base = (uint32_t)(persist_part_words<T>(N) * 8);
    h.base = (uint32_t)__hip_atomic_load(h.ws, GBDPCG_RLX_AGENT);
    return h;
}

}  // namespace gbdpcg
