// pcg_cluster_handoff.hpp -- what the workgroups of a cluster (pcg_cluster.hip) pass each other and how: the workspace layout, the
// tag format, the lane roles of the polling wave, the publish and the gather of one hand-off.  Nothing else is in here.
//
// WHAT CROSSES, twice per iteration (the two inner products of PCG depend on each other) and in ONE go each time: the 8 wave
// partials of the inner product and the boundary knot of the product vector that the neighbour needs; the neighbour then updates its
// halo copy of r / p with the same fma the owner uses (same bits).  Every workgroup sums all 8H partials in the same order -> the
// exit test of pcg.cuh:195 is uniform over the cluster -- what pcg.cuh:147,167,191 ensure with their redundant per-block sums.
// Hand-off words are data-tagged 8-byte granules {value, tag} (handoff_words.hpp) polled with sc1 loads: the data is the flag, no
// fence (MI355X_MICROARCH.md, Valid forms, R2).  One hand-off between two CUs costs 0.44-0.56 us (tools/hop_probe.hip), against
// 1.4-2 us for the chip-wide all-gather of the persistent path.
// WORKSPACE: [256-byte block: stamps of the diagnostic build, u64 words 30 / 31 = finish counter / launch number | from kClLeftOff,
// per cluster two u64 words: members that have left, and 2^32 - 1 - (first problem a member gave up on) maximised over the members
// (0: none) | from kClCtrlBytes, slots[2 epoch parities][grid blocks]].  One slot, written only by the workgroup that owns it:
//   +0            the 8 wave partials (fp32: 8 granules of 8 bytes; fp64: 8 pairs of granules, 128 bytes)
//   +kClFirstOff  the first own knot of the product vector, for the left neighbour: one 16-byte store {w0, tag, w1, tag} per lane of
//                 the knot (the lane's 8 bytes of payload: two fp32 rows, one fp64 row, or one fp32 row), up to 16 lanes
//   +kClLastOff   the last own knot, for the right neighbour
// TAGS.  Nothing is initialised or cleared by a launch (a solve stays ONE kernel node in a hipGraph).  Epochs start at 1 in every
// launch (1 is HELLO; the problems of a launch take 2 max_iter + 4 each from 2 on) and a tag is {launch number mod 4095, + 1 : 12
// bits | epoch : 20 bits}: a fixed split, so launches with different max_iter cannot produce each other's tags.  The launch number
// is control word 31, which the workgroup finishing LAST (word 30, an agent-scope counter, tells it) increments: every workgroup of
// a launch reads the same one, and whatever an earlier launch left in a slot -- or in some L2 -- carries another number.  Every
// workgroup of a launch that owns a problem clears its own slot (tag 0 is nobody's) before HELLO, so a granule outlives at most the
// launches that own nothing: a stale one can only carry the tag a launch polls for if it is 4095 k launches old AND no launch in
// between owned a problem.  (Two earlier forms: the last finisher zeroing all slots -- it wrote lines from one XCD that another
// XCD had written, which rules out plain stores; then every owner zeroing its slots behind a closing hand-off -- on one box a launch
// that followed one with another block-to-XCD mapping accepted stale granules, presumably out of an L2 line that had outlived the
// kernel boundary; with the launch number in the tag such a line is harmless.)
// HELLO (epoch 1): every member publishes the id of the XCD it runs on.  When every member sits on the SAME XCD (members are 8
// blocks apart for that, under round-robin dispatch) the cluster publishes with PLAIN stores: the line stays in the XCD's L2, where
// the partner's sc1 loads find it -- 0.25 us per hand-off instead of 0.44 (tools/hop_probe.hip; across XCDs a plain store is never
// seen, hence the check).  Otherwise stores are sc1 (write-through).  Nothing depends on placement.
// RESIDENCY.  A cluster's workgroups must be resident together: the grid never exceeds what the device holds at once, members of a
// cluster have neighbouring block indices (in-order dispatch then splits at most one cluster at a time, and that one only until
// any workgroup exits), and every spin is bounded: a cluster that cannot complete a hand-off gives its remaining problems up --
// nothing of them is written -- and the member that LEAVES LAST solves them alone in the same launch (pcg_cluster.hip).
#pragma once

#include "bt_dense.hpp"
#include "handoff_words.hpp"

namespace gbdpcg {

constexpr uint32_t kClLeftOff = 256, kClCtrlBytes = 256 + 256 * 16, kClSlotBytes = 640, kClFirstOff = 128, kClLastOff = 384;
constexpr uint32_t kClFinishedWord = 30, kClLaunchWord = 31;   // u64 words of the control block
constexpr uint32_t kClEpochBits = 20, kClLaunchMod = 4095;
// (launch: control word 31 as this launch read it)
__device__ __forceinline__ uint32_t cl_nonce(u64 launch) { return (uint32_t)(launch % kClLaunchMod + 1ull) << kClEpochBits; }
__device__ __forceinline__ uint32_t cl_tag(uint32_t nonce, uint32_t epoch) { return nonce | epoch; }

// Lane roles of the polling wave in one gather: lanes [0, PPM H) fetch 16 bytes of wave partials each (fp32: PPM = 4 lanes per
// member, two partials per lane; fp64: PPM = 8, one), lanes [32, 32 + LPB) the left neighbour's last knot, lanes
// [48, 48 + LPB) the right neighbour's first knot (LPB = lanes per knot <= 16).
constexpr uint32_t kClLeftLane = 32, kClRightLane = 48;
template <typename T> constexpr uint32_t cl_ppm() { return sizeof(T) == 4 ? 4u : 8u; }
// members of a cluster at most: the polling wave has 32 lanes for the partials
// (round 3: eight in fp32 -- 1024 converged solves of 14 x 300: 1,897 us streamed -> 997 us, one problem of 14 x 512: 85 -> 59 us)
template <typename T> constexpr uint32_t cl_max_members() { return kClLeftLane / cl_ppm<T>(); }

// A lane's payload in a boundary store: its V rows as two 32-bit words.
template <typename T, int V> __device__ __forceinline__ void cl_pack(const T (&v)[V], uint32_t &w0, uint32_t &w1)
{
    if constexpr (sizeof(T) == 8) {
        const u64 b = __builtin_bit_cast(u64, v[0]);
        w0 = (uint32_t)b;
        w1 = (uint32_t)(b >> 32);
    } else {
        w0 = __builtin_bit_cast(uint32_t, v[0]);
        w1 = V > 1 ? __builtin_bit_cast(uint32_t, v[V - 1]) : 0u;
    }
}
template <typename T, int V> __device__ __forceinline__ void cl_unpack(uint32_t w0, uint32_t w1, T (&v)[V])
{
    if constexpr (sizeof(T) == 8) {
        v[0] = __builtin_bit_cast(double, ((u64)w1 << 32) | w0);
    } else {
        v[0] = __builtin_bit_cast(float, w0);
        if constexpr (V > 1) v[1] = __builtin_bit_cast(float, w1);
    }
}
// The wave partials a partial lane fetched (16 bytes): two fp32 partials, or one fp64 partial.
template <typename T> __device__ __forceinline__ T cl_partials(uint32_t w0, uint32_t w1)
{
    if constexpr (sizeof(T) == 8) return __builtin_bit_cast(double, ((u64)w1 << 32) | w0);
    else return __builtin_bit_cast(float, w0) + __builtin_bit_cast(float, w1);
}

// LDS is workgroup-private and the hand-off stores must not be waited for: a barrier that drains only the LDS counter
__device__ __forceinline__ void cl_wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// What a workgroup knows about its place: wave-uniform, set up once.  What a LANE does in a hand-off follows from its lane number
// alone and is recomputed from an opaque copy of it, every time: kept in registers across the products (168 of 256 VGPRs hold
// matrix data) these few values were spilled, and each reload from scratch sat, with its s_waitcnt vmcnt(0), in front of the very
// stores the neighbour is waiting for.
struct ClCoords {
    __amdgpu_buffer_rsrc_t region;   // the slots, both parities
    uint32_t my_slot, par_stride;    // byte offset of the own slot in a parity, bytes of a parity
    uint32_t blk, blk0, bstride, H;  // own block, member 0 of the cluster, block distance of two neighbours, members
    uint32_t cnt, wl, lb;            // own knots; the last one: wave wl, lanes [lb LPB, lb LPB + LPB)
    bool has_left, has_right;
    uint32_t POLL;                   // the polling wave: never wave 0, never wave wl
    uint32_t nonce, spin_limit, drop_block;
};

// The words of its own slot that lane `lo` of wave `wave` writes (base = parity offset + my_slot): the wave's partial from lane 0, at
// o_part; where p_first / p_last, 16 bytes of the first / last own knot at o_first / o_last.  The clear in front of HELLO and
// every publish go through here: a wave's stores to one address arrive in order, so the same lanes must write the same words.
struct ClSlotLane { int o_part, o_first, o_last; bool p_first, p_last; };
template <typename T, uint32_t LPB> __device__ __forceinline__ ClSlotLane cl_slot_lane(const ClCoords &k, uint32_t base, uint32_t wave, uint32_t lo)
{
    ClSlotLane s;
    s.o_part = (int)(base + wave * (sizeof(T) == 4 ? 8u : 16u));
    s.o_first = (int)(base + kClFirstOff + lo * 16);
    s.o_last = (int)(base + kClLastOff + (lo - k.lb * LPB) * 16);
    s.p_first = wave == 0 && k.has_left && lo < LPB;
    s.p_last = wave == k.wl && k.has_right && lo - k.lb * LPB < LPB;
    return s;
}

// Tag 0 is nobody's: the own slot, both parities, before HELLO.
template <typename T, uint32_t LPB> __device__ __forceinline__ void cl_clear_slot(const ClCoords &k, uint32_t wave, uint32_t lane)
{
    const u32x2 z2 = {0u, 0u};
    const u32x4 z4 = {0u, 0u, 0u, 0u};
    uint32_t lo = lane;
    asm volatile("" : "+v"(lo));
#pragma unroll
    for (uint32_t par = 0; par < 2; ++par) {
        const ClSlotLane s = cl_slot_lane<T, LPB>(k, par * k.par_stride + k.my_slot, wave, lo);
        if (lo == 0) {
            if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b64(z2, k.region, s.o_part, 0, kSc1);
            else __builtin_amdgcn_raw_buffer_store_b128(z4, k.region, s.o_part, 0, kSc1);
        }
        if (s.p_first) __builtin_amdgcn_raw_buffer_store_b128(z4, k.region, s.o_first, 0, kSc1);
        if (s.p_last) __builtin_amdgcn_raw_buffer_store_b128(z4, k.region, s.o_last, 0, kSc1);
    }
}

// Publish (every wave): the wave's share `part` of the inner product, and from the lanes that own the first / last knot the values
// `vals` of their rows.  POLICY: the cache-policy bits of the stores -- 0: plain, the line stays in this XCD's L2, where every
// member of the cluster polls; kSc1: write-through, seen from any XCD.  ONE (a cluster of one workgroup): the partials meet in
// `lpart` in LDS, laid out like the slot in memory -- the caller puts a cl_wg_barrier behind it.
template <int POLICY, int NCT, bool ONE, typename T, int V>
__device__ __forceinline__ void cl_publish(const ClCoords &k, uint32_t wave, uint32_t lane, uint32_t epoch, T part, const T (&vals)[V], u32x4 *lpart)
{
    if (k.blk == k.drop_block) return;
    const uint32_t tag = cl_tag(k.nonce, epoch);
    uint32_t lo = lane;
    asm volatile("" : "+v"(lo));
    uint32_t w0, w1, q0, q1;
    cl_pack<T, V>(vals, w0, w1);
    const T part_[1] = {part};
    cl_pack<T, 1>(part_, q0, q1);
    const u32x2 x2 = {q0, tag};
    const u32x4 x4 = {q0, tag, q1, tag};
    const u32x4 bx = {w0, tag, w1, tag};
    if constexpr (ONE) {
        if (lo == 0) {
            if constexpr (sizeof(T) == 4) reinterpret_cast<u32x2 *>(lpart)[wave] = x2;
            else lpart[wave] = x4;
        }
    } else {
        const ClSlotLane s = cl_slot_lane<T, NCT / V>(k, (epoch & 1u) * k.par_stride + k.my_slot, wave, lo);
        if (lo == 0) {
            if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b64(x2, k.region, s.o_part, 0, POLICY);
            else __builtin_amdgcn_raw_buffer_store_b128(x4, k.region, s.o_part, 0, POLICY);
        }
        if (s.p_first) __builtin_amdgcn_raw_buffer_store_b128(bx, k.region, s.o_first, 0, POLICY);
        if (s.p_last) __builtin_amdgcn_raw_buffer_store_b128(bx, k.region, s.o_last, 0, POLICY);
    }
}

// What the polling wave has after a gather.  total: the 8H partials summed (wave-uniform, the same bits in every member).  In a
// halo lane: hidx = the entry of the window it rewrites afterwards (0xffffffff: not a halo lane), gv = the neighbour's values for
// it, hv = its current content.  ok: false when the spin bound was hit.  gotx / gotz: the lane's two payload words as fetched.
template <typename T, int V> struct ClGathered { T total, gv[V], hv[V]; uint32_t hidx, gotx, gotz; bool ok; };
// Gather (the polling wave only) the hand-off of `epoch`; hwin: the window (halo knot, own knots, halo knot) whose halos it feeds.
template <int NCT, int V, bool ONE, typename T>
__device__ __forceinline__ ClGathered<T, V> cl_gather(const ClCoords &k, uint32_t lane, uint32_t epoch, const T *hwin, const u32x4 *lpart)
{
    constexpr uint32_t n = NCT, LPB = NCT / V, PPM = cl_ppm<T>();
    const uint32_t tag = cl_tag(k.nonce, epoch), par_off = (epoch & 1u) * k.par_stride;
    uint32_t lo = lane;
    asm volatile("" : "+v"(lo));
    ClGathered<T, V> g;
    uint32_t poll_off = 0;
    bool have = true;
    g.hidx = 0xffffffffu;
    if (lo < PPM * k.H) {
        poll_off = (k.blk0 + (lo / PPM) * k.bstride) * kClSlotBytes + (lo % PPM) * 16;
        have = false;
    } else if (lo - kClLeftLane < LPB && k.has_left) {
        poll_off = (k.blk - k.bstride) * kClSlotBytes + kClLastOff + (lo - kClLeftLane) * 16;
        g.hidx = (lo - kClLeftLane) * V;
        have = false;
    } else if (lo - kClRightLane < LPB && k.has_right) {
        poll_off = (k.blk + k.bstride) * kClSlotBytes + kClFirstOff + (lo - kClRightLane) * 16;
        g.hidx = (k.cnt + 1) * n + (lo - kClRightLane) * V;
        have = false;
    }
    // the halo entries this lane is going to update: read now, under the wait
#pragma unroll
    for (int j = 0; j < V; ++j) g.hv[j] = T(0);
    if (g.hidx != 0xffffffffu) {
#pragma unroll
        for (int j = 0; j < V; ++j) g.hv[j] = hwin[g.hidx + j];
    }
    u32x4 got = {0u, 0u, 0u, 0u};
    g.ok = true;
    if constexpr (ONE) {
        got = lpart[lo < PPM ? lo : 0u];
        g.ok = k.blk != k.drop_block;
    } else
        for (uint32_t spins = 0;; ++spins) {
            asm volatile("" ::: "memory");   // the poll is re-issued on every pass
            if (!have) {                     // only the lanes that still miss their piece load again
                got = __builtin_amdgcn_raw_buffer_load_b128(k.region, (int)(par_off + poll_off), 0, kSc1);
                have = got.y == tag && got.w == tag;
            }
            if (__all(have)) break;
            if (spins >= k.spin_limit) { g.ok = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
    // by value: __builtin_bit_cast applied to the element expression got.z itself reads element 0 (hipcc, ROCm 7.2)
    g.gotx = got.x;
    g.gotz = got.z;
    cl_unpack<T, V>(g.gotx, g.gotz, g.gv);
    g.total = wave_sum(lo < PPM * k.H ? cl_partials<T>(g.gotx, g.gotz) : T(0));
    return g;
}

}  // namespace gbdpcg
