// pcg_resident_sym.hip -- PCG with both SYMMETRIC matrices resident on one CU (registers + LDS).
//
// Replaces pcg<T,n,N> (/root/reference/include/pcg.cuh:54-218) for the BASELINE batch shape
// (n = 14, fp32, N <= 128) when S and Pinv are symmetric in storage (L_{k+1} == R_k^T, tested on the
// device or asserted by the caller, gbdpcg_set_symmetric).  The symmetric halves [D_k | R_k] of BOTH
// matrices are 2 * 128 * 2n^2 * 4 B = 401 KB: three quarters live in the registers of one 8-wave
// workgroup (3 x 56 VGPRs per lane), the last quarter plus two pieces of the third in LDS (131 KB), the
// vectors lambda, r, p in LDS too (29 KB), so the matrices are read from HBM ONCE PER SOLVE and an
// iteration moves no bytes beyond the CU -- the reference's idea of
// keeping the block-rows next to the ALUs for the whole solve (pcg.cuh:104-110), with the whole
// problem inside one workgroup so that no grid barrier exists.
//
// Lane map: aligned groups of 8 lanes; lane rp = lane & 7 < 7 owns rows 2rp, 2rp+1 of TWO consecutive
// block-rows k0 = 2j, k1 = 2j+1 (j = 8*wave + group): all 2n columns of [D_k | R_k], 56 registers per
// block-row per matrix.  Per block-row and product
//     y_k     +=  [D_k | R_k] [x_k ; x_{k+1}]    2n FMAs per row, columns ascending, no cross-lane fold
//     y_{k+1} +=  R_k^T x_k                      n partial values per lane, reduce-scattered over the
//                                                8 lanes of the group with DPP (half-mirror, quad
//                                                perms): lane rp ends up with entries 2rp, 2rp+1
// The transposed product of k0 lands in the same lane's k1 rows (registers); the one of k1 belongs to
// the next group and goes through LDS.  Its share of the inner product is accounted on the producer
// side (u . x_{k1+1}), so the workgroup reduction needs no extra barrier: 4 barriers per iteration.
#include <cstdlib>

#include "bt_device.hpp"
#include "bt_sym.hpp"
#include "internal.hpp"

#ifndef GBDPCG_RS_TILE_NT
#define GBDPCG_RS_TILE_NT 1
#endif
#ifndef GBDPCG_RS_PREFETCH
#define GBDPCG_RS_PREFETCH 1
#endif
#ifndef GBDPCG_RS_LINEAR_PAIRS
#define GBDPCG_RS_LINEAR_PAIRS 0   // 1: the round-1 assignment of block-row pairs to groups (A/B builds)
#endif

namespace gbdpcg {

template <int NCT> struct SymResGeom {
    static constexpr uint32_t N_ = NCT;
    static constexpr uint32_t QUADS = N_;            // 16-byte pieces per lane per block-row: 2 columns x 2 rows
    static constexpr uint32_t WAVES = 8, GROUPS = 8, SLOTS = 2;
    static constexpr uint32_t THREADS = WAVES * 64;
    static constexpr uint32_t MAX_KNOTS = WAVES * GROUPS * SLOTS;
    static constexpr uint32_t P0_LDS_QUADS = 2;      // leading pieces of the Pinv k0 tile that also live in LDS
    // One LDS region per 8-lane group: [D_k | R_k] in memory order (2n^2 floats) -- the staging buffer of
    // the coalesced tile loads; the 8 regions of a wave then hold that wave's share of the Pinv k1 tile
    // (one float4 per lane and piece).  ROW_PIECES 16-byte pieces are real, a group loads STG_PIECES
    // (8 lanes x 13); the stride makes the 8 groups of a wave start 8 banks apart (2-way conflicts at
    // most on the 8-byte reads of the staging step).
    static constexpr uint32_t ROW_PIECES = 2 * N_ * N_ / 4, STG_ITERS = (ROW_PIECES + 7) / 8, STG_PIECES = 8 * STG_ITERS;
    static constexpr uint32_t REGION = 456;
    static_assert(REGION >= 4 * STG_PIECES && REGION % 64 == 8 && (2 * N_ * N_) % 4 == 0, "region layout");
    static_assert(GROUPS * REGION >= QUADS * 64 * 4, "a wave's block must hold its LDS-resident tile");
    static constexpr uint32_t REGIONS_FLOATS = WAVES * GROUPS * REGION;
    static constexpr uint32_t TILE_LDS_FLOATS = REGIONS_FLOATS + P0_LDS_QUADS * THREADS * 4;
};

// One block-row of one matrix as this lane sees it: q[i] = (M[2rp, 2i], M[2rp, 2i+1], M[2rp+1, 2i], M[2rp+1, 2i+1])
// over the 2n columns of [D | R] -- the two columns of a ROW adjacent, so that both the main product (a row
// pair times the x pair as it comes out of LDS, even and odd columns accumulated apart) and the transposed
// product (a row pair times one broadcast x entry) are single v_pk_fma_f32 instructions.
template <int NCT> struct SymResTile {
    float4 q[SymResGeom<NCT>::QUADS];
};

// Direct tile load (matrix base only 8-byte aligned): every lane reads its own 8-byte pairs.  Split in
// two so that the requests of three tiles are in flight together: symres_issue only issues the loads,
// symres_mask zeroes what must not be used (dead lanes, R_{N-1}) once the data is there.
template <int NCT>
__device__ __forceinline__ void symres_issue(const float *__restrict__ M, uint32_t k, uint32_t rp, bool live,
                                             SymResTile<NCT> &t)
{
    constexpr uint32_t n = NCT;
    const float *src = M + (size_t)(live ? k : 0u) * 3 * n * n + n * n + (live ? rp * 2 : 0u);
#pragma unroll
    for (uint32_t i = 0; i < n; ++i) {
        float a[2], b[2];
        VecIO<float, 2>::load<true>(src + (2 * i) * n, a);
        VecIO<float, 2>::load<true>(src + (2 * i + 1) * n, b);
        t.q[i] = make_float4(a[0], b[0], a[1], b[1]);
    }
}

template <int NCT>
__device__ __forceinline__ void symres_mask(uint32_t N, uint32_t k, bool live, SymResTile<NCT> &t)
{
    constexpr uint32_t n = NCT;
    const bool keep_r = live && k != N - 1;  // R_{N-1} is never used (pcg.cuh:106)
#pragma unroll
    for (uint32_t i = 0; i < n; ++i) {
        const bool keep = 2 * i < n ? live : keep_r;
        t.q[i] = make_float4(keep ? t.q[i].x : 0.f, keep ? t.q[i].y : 0.f, keep ? t.q[i].z : 0.f, keep ? t.q[i].w : 0.f);
    }
    // Pin the masked values here: hipcc otherwise sinks the selects to the first use and keeps the raw
    // and the masked copy of every tile alive across the prologue (spills).
#pragma unroll
    for (uint32_t i = 0; i < n; ++i) asm volatile("" : "+v"(t.q[i].x), "+v"(t.q[i].y), "+v"(t.q[i].z), "+v"(t.q[i].w));
}

// Coalesced tile load (matrix base 16-byte aligned): the 8 lanes of a group read the 2n^2 contiguous
// floats of [D_k | R_k] as 16-byte pieces, 128 contiguous bytes per group and instruction (the direct
// form touches 8 x 56 scattered bytes per instruction and is bound by the texture-address unit), park
// them in the group's LDS region and pick their own rows up from there.  Wave-local: no barrier.
// The group regions are written as 16-byte pieces and read back as 8-byte pairs: both through
// may_alias types, or type-based alias analysis lets hipcc move the reads above the writes.
typedef float4 __attribute__((may_alias)) float4_alias;
typedef float2 __attribute__((may_alias)) float2_alias;

template <int NCT> struct SymResStage {
    float4 b[SymResGeom<NCT>::STG_ITERS];
};
template <int NCT>
__device__ __forceinline__ void symres_stage_issue(const float *__restrict__ M, uint32_t k, bool group_live, uint32_t l8,
                                                   SymResStage<NCT> &st)
{
    using G = SymResGeom<NCT>;
    constexpr uint32_t n = NCT;
    const float4 *src = reinterpret_cast<const float4 *>(M + (size_t)(group_live ? k : 0u) * 3 * n * n + n * n);
#pragma unroll
    for (uint32_t i = 0; i < G::STG_ITERS; ++i) {
        const uint32_t piece = l8 + 8 * i;
        const uint32_t safe = (8 * i + 7 < G::ROW_PIECES || piece < G::ROW_PIECES) ? piece : 0u;  // never past the row
#if GBDPCG_RS_TILE_NT
        const auto v = __builtin_nontemporal_load(reinterpret_cast<const NtVec<float, 4>::type *>(src + safe));
        st.b[i] = make_float4(v.x, v.y, v.z, v.w);
#else
        st.b[i] = src[safe];
#endif
    }
}
// keep_d / keep_r: whether the D / R half may be used at all (dead group, R_{N-1}); zeros are parked otherwise.
template <int NCT>
__device__ __forceinline__ void symres_stage_park(const SymResStage<NCT> &st, float *region, uint32_t l8, bool keep_d,
                                                  bool keep_r)
{
    using G = SymResGeom<NCT>;
    float4_alias *dst = reinterpret_cast<float4_alias *>(region);
    // Lanes exchange data through the region: the compiler must not move LDS accesses across the
    // hand-over points just because the addresses of ONE lane do not overlap (the hardware keeps the
    // LDS operations of a wave in order).
    asm volatile("" ::: "memory");
#pragma unroll
    for (uint32_t i = 0; i < G::STG_ITERS; ++i) {
        const uint32_t piece = l8 + 8 * i;
        // D_k is pieces [0, n^2/4), R_k the rest (n^2 % 4 == 0 for n = 14)
        const bool keep = (8 * i + 7 < NCT * NCT / 4) ? keep_d : (8 * i >= NCT * NCT / 4 ? keep_r : (piece < NCT * NCT / 4 ? keep_d : keep_r));
        const float4 v = st.b[i];
        dst[piece] = make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
    }
    asm volatile("" ::: "memory");
}
template <int NCT>
__device__ __forceinline__ void symres_stage_pick(const float *region, uint32_t rp, bool lane_live, SymResTile<NCT> &t)
{
    constexpr uint32_t n = NCT;
    const float2_alias *src = reinterpret_cast<const float2_alias *>(region + rp * 2);
#pragma unroll
    for (uint32_t i = 0; i < n; ++i) {
        const float2 a = src[(2 * i) * n / 2], b = src[(2 * i + 1) * n / 2];
        t.q[i] = make_float4(lane_live ? a.x : 0.f, lane_live ? b.x : 0.f, lane_live ? a.y : 0.f, lane_live ? b.y : 0.f);
    }
#pragma unroll
    for (uint32_t i = 0; i < n; ++i) asm volatile("" : "+v"(t.q[i].x), "+v"(t.q[i].y), "+v"(t.q[i].z), "+v"(t.q[i].w));
}

// Both block-rows of the lane against the operand window [x_k0 ; x_k1 ; x_k1+1] (21 LDS pairs, x_k1 read once
// for both), in two phases of n/2 steps with six independent packed instructions per step:
//   phase 1, x_k1 pair j         : R_k0 piece j (+ its transposed share tt0) and D_k1 piece j
//   phase 2, x_k0 / x_k1+1 pair j: D_k0 piece j, and R_k1 piece j (+ tt1)
// (a pass in operand order -- D_k0 alone, then the shared middle, then R_k1 alone -- leaves two thin
// stretches in which a wave has only two dependent FMA chains to issue and waits on their latency: 3.5 %
// slower).  The x_k1 pairs are requested before anything else, later pairs AHX steps ahead, LDS-resident
// tile pieces AHT steps ahead (3 and 1: the measured optimum; deeper prefetch is slower).  tt0 is reduce-scattered between the two
// phases (u0), tt1 by the caller.
// LQ0 leading pieces of the k0 tile come from LDS (lt0, one float4 per lane and piece, stride THREADS);
// K1_FROM_LDS: the whole k1 tile is read from LDS (lt1, one float4 per lane and piece, stride 64).
// The steps are pinned in source order and the accumulators anchored: left to itself hipcc hoists all
// LDS reads to the top and sinks the accumulator chains below the reduce-scatter, and the operands of
// every step stay live (with three resident tiles, 168 VGPRs, that spills).
#ifndef GBDPCG_RS_AHX
#define GBDPCG_RS_AHX 3
#endif
#ifndef GBDPCG_RS_AHT
#define GBDPCG_RS_AHT 1
#endif
__device__ __forceinline__ void symres_reduce_scatter14(float (&t)[14], uint32_t lane, float (&out)[2]);

template <int NCT, uint32_t LQ0, bool K1_FROM_LDS>
__device__ __forceinline__ void symres_mv2(const SymResTile<NCT> &t0, const float4 *lt0, const SymResTile<NCT> &t1,
                                           const float4_alias *lt1, const float2 *xk2, float2 o0, float2 o1, uint32_t lane,
                                           float (&y0)[2], float (&y1)[2], float (&u0)[2], float (&tt1)[NCT])
{
    constexpr uint32_t n = NCT, H = n / 2, TH = SymResGeom<NCT>::THREADS;
    constexpr uint32_t AHX = GBDPCG_RS_AHX, AHT = GBDPCG_RS_AHT;
    typedef float v2f __attribute__((ext_vector_type(2)));
    static_assert(AHX <= H && AHT <= H, "prefetch distances are counted inside one phase");
    float2 xm[H], xa_[H], xc[H];  // sliding windows: only a few entries of each are ever live
    float4 q0[LQ0 > 0 ? LQ0 : 1], q1[n];
#pragma unroll
    for (uint32_t j = 0; j < H; ++j) xm[j] = xk2[H + j];
#pragma unroll
    for (uint32_t i = 0; i < LQ0; ++i) q0[i] = lt0[i * TH];
#pragma unroll
    for (uint32_t i = 0; i < AHT; ++i)
        if (K1_FROM_LDS) q1[i] = lt1[i * 64];
    v2f a00 = {0.f, 0.f}, a01 = {0.f, 0.f}, a10 = {0.f, 0.f}, a11 = {0.f, 0.f};
    float tt0[NCT];
#pragma unroll
    for (uint32_t j = 0; j < H; ++j) {
        if (K1_FROM_LDS && j + AHT < n) q1[j + AHT] = lt1[(j + AHT) * 64];
        if (j + AHX >= H && j + AHX - H < H) {  // requests for the first steps of phase 2
            xa_[j + AHX - H] = xk2[j + AHX - H];
            xc[j + AHX - H] = xk2[2 * H + j + AHX - H];
        }
        const v2f xv = {xm[j].x, xm[j].y};
        {
            const float4 v = t0.q[H + j];  // R_k0 (the LDS-resident leading pieces of a k0 tile are D pieces)
            a00 = __builtin_elementwise_fma(v2f{v.x, v.y}, xv, a00);
            a01 = __builtin_elementwise_fma(v2f{v.z, v.w}, xv, a01);
            const v2f tp = __builtin_elementwise_fma(v2f{v.z, v.w}, v2f{o0.y, o0.y}, v2f{v.x, v.y} * v2f{o0.x, o0.x});
            tt0[2 * j] = tp.x;
            tt0[2 * j + 1] = tp.y;
        }
        {
            const float4 v = K1_FROM_LDS ? q1[j] : t1.q[j];  // D_k1
            a10 = __builtin_elementwise_fma(v2f{v.x, v.y}, xv, a10);
            a11 = __builtin_elementwise_fma(v2f{v.z, v.w}, xv, a11);
        }
        asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    symres_reduce_scatter14(tt0, lane, u0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (uint32_t j = 0; j < H; ++j) {
        if (K1_FROM_LDS && H + j + AHT < n) q1[H + j + AHT] = lt1[(H + j + AHT) * 64];
        if (j + AHX < H) {
            xa_[j + AHX] = xk2[j + AHX];
            xc[j + AHX] = xk2[2 * H + j + AHX];
        }
        const v2f xd = {xa_[j].x, xa_[j].y}, xr = {xc[j].x, xc[j].y};
        {
            const float4 v = j < LQ0 ? q0[j] : t0.q[j];  // D_k0
            a00 = __builtin_elementwise_fma(v2f{v.x, v.y}, xd, a00);
            a01 = __builtin_elementwise_fma(v2f{v.z, v.w}, xd, a01);
        }
        {
            const float4 v = K1_FROM_LDS ? q1[H + j] : t1.q[H + j];  // R_k1
            a10 = __builtin_elementwise_fma(v2f{v.x, v.y}, xr, a10);
            a11 = __builtin_elementwise_fma(v2f{v.z, v.w}, xr, a11);
            const v2f tp = __builtin_elementwise_fma(v2f{v.z, v.w}, v2f{o1.y, o1.y}, v2f{v.x, v.y} * v2f{o1.x, o1.x});
            tt1[2 * j] = tp.x;
            tt1[2 * j + 1] = tp.y;
        }
        asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    y0[0] = a00.x + a00.y; y0[1] = a01.x + a01.y;
    y1[0] = a10.x + a10.y; y1[1] = a11.x + a11.y;
}

// Sum tt[c] over the 8 lanes of the aligned group and leave entries 2rp, 2rp+1 in lane rp:
// recursive halving, partner 7-i (row_half_mirror), then i^2 and i^1 (quad perms).  The DPP adds are
// written as asm blocks: hipcc otherwise pairs the adds into v_pk_add_f32 fed by v_mov_b32_dpp copies
// (3x the instructions).  Each block starts with the two wait states a DPP read of a freshly written
// VGPR needs; inside a block every instruction touches its own register.
__device__ __forceinline__ void symres_reduce_scatter14(float (&t)[14], uint32_t lane, float (&out)[2])
{
    // Stage 1 (partner 7-i) with the selection folded into the adds: the lower half of every 8-lane group is
    // DPP banks 0 and 2 of a row, the upper half banks 1 and 3, so two bank-masked adds into the same register
    // give each half the entries it keeps (c < 8 below, c >= 8 above) without any v_cndmask.
    float u0, u1, u2, u3, u4, u5, u6 = 0.f, u7 = 0.f;
#define LO(u, a) "v_add_f32_dpp %" #u ", %" #a ", %" #a " row_half_mirror row_mask:0xf bank_mask:0x5\n"
#define HI(u, a) "v_add_f32_dpp %" #u ", %" #a ", %" #a " row_half_mirror row_mask:0xf bank_mask:0xa\n"
    asm volatile("s_nop 1\n" LO(0, 8) HI(0, 16) LO(1, 9) HI(1, 17) LO(2, 10) HI(2, 18) LO(3, 11) HI(3, 19) LO(4, 12) HI(4, 20)
                 LO(5, 13) HI(5, 21) LO(6, 14) LO(7, 15)
                 : "=&v"(u0), "=&v"(u1), "=&v"(u2), "=&v"(u3), "=&v"(u4), "=&v"(u5), "+v"(u6), "+v"(u7)
                 : "v"(t[0]), "v"(t[1]), "v"(t[2]), "v"(t[3]), "v"(t[4]), "v"(t[5]), "v"(t[6]), "v"(t[7]), "v"(t[8]),
                   "v"(t[9]), "v"(t[10]), "v"(t[11]), "v"(t[12]), "v"(t[13]));
#undef LO
#undef HI
#define D(i) "v_add_f32_dpp %" #i ", %" #i ", %" #i " quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
    asm volatile("s_nop 1\n" D(0) D(1) D(2) D(3) D(4) D(5) D(6) D(7)
                 : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+v"(u4), "+v"(u5), "+v"(u6), "+v"(u7));
#undef D
    const bool b1 = (lane & 2u) != 0;
    float w0 = b1 ? u4 : u0, w1 = b1 ? u5 : u1, w2 = b1 ? u6 : u2, w3 = b1 ? u7 : u3;
#define D(i) "v_add_f32_dpp %" #i ", %" #i ", %" #i " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
    asm volatile("s_nop 1\n" D(0) D(1) D(2) D(3) : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3));
#undef D
    const bool b0 = (lane & 1u) != 0;
    out[0] = b0 ? w2 : w0;
    out[1] = b0 ? w3 : w1;
}

// Pull the NEXT problem's [D|R] blocks towards the Infinity Cache, one dword touched per 64 bytes (measured:
// a 128-byte stride leaves part of the stream in HBM and costs 3 us per batch), while this problem iterates: every CU finishes its solve at about the same time, so without this all 256 CUs hit HBM
// with their 401 KB tile loads in the same burst.  The load is an LDS-DMA (no VGPR destination, so
// nothing the compiler allocates can be clobbered when it lands) into a dump area of LDS that
// is never read; it is hidden from hipcc's waitcnt bookkeeping, so no barrier or LDS read waits for it.
template <int NCT>
__device__ __forceinline__ void symres_touch(const float *M, uint32_t N, uint32_t slot, uint32_t lds_dump)
{
    // slot -> (block-row k, 64-byte step j inside its [D_k | R_k]); L blocks are never touched
    constexpr uint32_t row_bytes = 2 * NCT * NCT * 4, steps = (row_bytes + 63) / 64 + 1;
    const uint32_t k = slot / steps, j = slot - k * steps;
    const uint32_t kk = k < N ? k : 0u;
    uint32_t off = j * 64;
    if (off > row_bytes - 4) off = row_bytes - 4;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(M) + ((size_t)kk * 3 * NCT * NCT + NCT * NCT) * 4 + off;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(addr), "s"(lds_dump) : "memory");
}

// Symmetry in storage, verified against the resident tile (verifying kernel only).  Columns 2rp, 2rp+1 of L_{k+1}
// (column-major: 2n contiguous floats at (k+1) 3n^2 + 2rp n, 16-byte aligned when the matrix is) are the transposes of the
// lane's rows 2rp, 2rp+1 of R_k.  cmp == false (dead lane, k >= N-1): block 0's first floats are read instead and ignored.
// Plain loads: non-temporal ones took 21 instead of 8.5 us per round of the tail.  (Touching the next problem's L blocks
// along with its [D|R] during the iterations, so that this read would find them in the Infinity Cache, cost the iterations
// as much as it saved here: not done.)
template <int NCT>
__device__ __forceinline__ void symres_lcols_issue(const float *__restrict__ M, uint32_t k, uint32_t rp, bool cmp,
                                                   float4 (&l)[NCT / 2])
{
    constexpr uint32_t n = NCT;
    const float4 *src = reinterpret_cast<const float4 *>(M + (cmp ? (size_t)(k + 1) * 3 * n * n + 2 * rp * n : (size_t)0));
#pragma unroll
    for (uint32_t m = 0; m < n / 2; ++m) l[m] = src[m];
}
// r[j] = the tile's R piece j: (R[2rp, 2j], R[2rp, 2j+1], R[2rp+1, 2j], R[2rp+1, 2j+1]).  True when some R_k(r, c) and
// L_{k+1}(c, r) differ bit for bit (the semantics of check_symmetric_pair_kernel: -0.0 != +0.0, NaNs by payload).
template <int NCT>
__device__ __forceinline__ bool symres_r_differs(const float4 (&r)[NCT / 2], const float4 (&l)[NCT / 2], bool cmp)
{
    constexpr uint32_t n = NCT;
    auto comp = [](const float4 &v, uint32_t i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; };
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t e = 0; e < 2 * n; ++e) {
        const uint32_t hi = e / n, c = e % n;   // L_{k+1}(c, 2rp + hi)  vs  R_k(2rp + hi, c)
        diff |= __builtin_bit_cast(uint32_t, comp(l[e / 4], e % 4)) ^ __builtin_bit_cast(uint32_t, comp(r[c / 2], 2 * hi + (c & 1)));
    }
    return cmp && diff != 0;
}

// One dword LDS-DMA instruction: the active lanes move 4 bytes each from base + off to lds_addr + 4 * lane.  Like the touch
// above it is invisible to hipcc's counters; the caller waits (s_waitcnt vmcnt(0)) before the barrier that precedes the
// first read of the destination.
__device__ __forceinline__ void symres_dma_dword(const float *base, uint32_t off, uint32_t lds_addr)
{
#ifdef GBDPCG_RS_STAMPS
    // (diagnostic build: with the stamps' stores in the problem loop hipcc no longer proves the base uniform and refuses the "s"
    // operand below; it is uniform)
    {
        const uint64_t b = reinterpret_cast<uint64_t>(base);
        base = reinterpret_cast<const float *>(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
                                               __builtin_amdgcn_readfirstlane((uint32_t)b));
    }
#endif
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %2, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(base), "v"(off), "s"(lds_addr) : "memory");
}

// Diagnostic build only (-DGBDPCG_RS_STAMPS, tools/rs_stamps.py): wave 0 of every workgroup leaves the 100 MHz real-time clock
// at the phase boundaries of each of its problems in the handle's (otherwise unused here) cluster workspace: 8 stamps per
// (workgroup, round).  No stamp exists in the shipped build.
#ifdef GBDPCG_RS_STAMPS
#define GBDPCG_RS_STAMP(IDX)                                                                                             \
    if (tid == 0 && a.cluster_ws && rs_round < 8)                                                                        \
        (reinterpret_cast<unsigned long long *>(a.cluster_ws) + 1024)[(blockIdx.x * 8 + rs_round) * 8 + (IDX)] = __builtin_amdgcn_s_memrealtime();
#else
#define GBDPCG_RS_STAMP(IDX)
#endif

// VERIFY: the launch takes EVERY problem (a.sel is not read) and tests L_{k+1} == R_k^T of both matrices itself, against
// the resident tiles, after the iterations: a problem that passes is written as by the plain kernel plus verdict byte 1 in
// a.verdict_out[prob]; one that fails gets verdict byte 0 and nothing else (lambda keeps the caller's warm start for the
// general launch that follows).  VERIFY = false is the plain kernel.
// SHARED (gbdpcg_solve_shared_*): a.S and a.Pinv are ONE pair of matrices for the whole batch.  The workgroup
// loads its four quarter-tiles once, before its problem loop, and keeps them in registers and LDS for all of its problems: a
// problem then costs its vectors, the prologue, the iterations and the write-back -- no tile ingest, nothing to prefetch.  The
// products are the same instructions on the same numbers: problem b gets the bits the plain kernel gives it on replicated matrices.
template <int NCT, bool STAGED, bool VERIFY = false, bool SHARED = false>
__global__ __launch_bounds__(512) void pcg_resident_sym_kernel(PcgArgs<float> a)
{
    using G = SymResGeom<NCT>;
    static_assert(!(VERIFY && SHARED), "a shared pair is tested once, before the launch (api.hip)");
    static_assert(G::THREADS == 512, "launch bounds above assume 8 waves");
    static_assert(NCT == 14, "the reduce-scatter is written for 7 live lanes x 2 rows");
    constexpr uint32_t n = NCT, WAVES = G::WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *smem = reinterpret_cast<float *>(smem_raw);

    const uint32_t N = a.N, len = n * N;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t padded = align16<float>((N + 3) * n);
    float *region = smem + (wave * G::GROUPS + (lane >> 3)) * G::REGION;  // this group's LDS region (Pinv k1 lives there)
    float4 *lt0 = reinterpret_cast<float4 *>(smem + G::REGIONS_FLOATS) + tid;  // first pieces of this lane's Pinv k0 tile
    float *xa = smem + G::TILE_LDS_FLOATS, *xb = xa + padded;  // padded mirrors of p (lambda in the prologue) and r
    float *zs = xb + padded;                                   // R_{k-1}^T x_{k-1} for the even block-rows
    float *red0 = zs + padded, *red1 = red0 + WAVES;
    float *ls = red1 + WAVES;                                  // lambda
    // LDS byte address of the 256-byte dump area of the prefetch loads (symres_touch), shared by all waves
    const uint32_t dump = (uint32_t)(uintptr_t)(ls + align16<float>(len));
    // verifying kernel: the workgroup's verdict on the current problem (1 = symmetric), right behind the dump area
    uint32_t *vword = reinterpret_cast<uint32_t *>(ls + align16<float>(len)) + 64;

    const size_t mstride = (size_t)3 * n * n * N;

    // zs: only the rows of even block-rows >= 2 are ever written; row 0 (nothing above block-row 0) and the odd
    // rows (read, harmlessly, by the lanes that own no rows) must hold zeros for the whole launch
    for (uint32_t i = tid; i < padded; i += G::THREADS) zs[i] = 0.f;
    __syncthreads();

    // which of this workgroup's problems this launch owns, 64 at a time (one memory round trip for all of them)
    unsigned long long takes = 0;
    uint32_t takes_from = 0;
#ifdef GBDPCG_RS_STAMPS
    uint32_t rs_round = 0xffffffffu;
#endif
    // The block-rows of a lane, from its number LANE_O (declares rp, grp, k0, k1, live0, live1).
    // Which pair of block-rows a group owns is free; it is chosen so that the four groups that share an LDS pass
    // (lanes 0-31 / 32-63 of a wave) own pairs j, j+4, j+8, j+12: their rows of a vector then start 48 banks apart
    // (a pair is 2n = 28 floats) and the 8-byte accesses of 4 x 7 lanes tile the 64 banks instead of colliding two by
    // two, as consecutive pairs do (bases 0, 28, 56, 20 mod 64: 13 % of an iteration's LDS-array cycles were conflicts).
#if GBDPCG_RS_LINEAR_PAIRS
#define GBDPCG_SYMRES_K0(GRP) (2 * (wave * G::GROUPS + (GRP)))
#else
#define GBDPCG_SYMRES_K0(GRP) (2 * (16 * (wave >> 1) + 4 * ((GRP) & 3u) + 2 * (wave & 1u) + ((GRP) >> 2)))
#endif
#define GBDPCG_SYMRES_LANE_ROWS(LANE_O)                                                                       \
        const uint32_t rp = (LANE_O) & 7u;                                                                    \
        const uint32_t grp = (LANE_O) >> 3;                                                                   \
        const uint32_t k0 = GBDPCG_SYMRES_K0(grp), k1 = k0 + 1;                                               \
        const bool live0 = rp < n / 2 && k0 < N, live1 = rp < n / 2 && k1 < N;

    // Resident for the whole solve (SHARED: for the whole launch): three tiles in registers, the fourth in LDS.
    SymResTile<NCT> s0, s1, p0;
    // The tiles of the matrices S and P into s0, s1, p0, the wave's block of regions (ltw) and lt0.  Wave-local: no barrier.
#define GBDPCG_SYMRES_LOAD_TILES()                                                                            \
        if constexpr (STAGED) {                                                                               \
            const uint32_t l8 = rp;                                                                           \
            const bool g0 = k0 < N, g1 = k1 < N;  /* whole group alive */                                     \
            /* all four tiles are requested at once (4 x 52 VGPRs, nothing else is live yet): one memory      \
               round trip per problem instead of one per tile */                                              \
            SymResStage<NCT> sa, sb, sc, sd;                                                                  \
            symres_stage_issue<NCT>(S, k0, g0, l8, sa);                                                       \
            symres_stage_issue<NCT>(S, k1, g1, l8, sb);                                                       \
            symres_stage_issue<NCT>(P, k0, g0, l8, sc);                                                       \
            symres_stage_issue<NCT>(P, k1, g1, l8, sd);                                                       \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            GBDPCG_RS_STAMP(1)                                                                                \
            symres_stage_park<NCT>(sa, region, l8, g0, g0 && k0 != N - 1);                                    \
            symres_stage_pick<NCT>(region, rp, live0, s0);                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            symres_stage_park<NCT>(sb, region, l8, g1, g1 && k1 != N - 1);                                    \
            symres_stage_pick<NCT>(region, rp, live1, s1);                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            symres_stage_park<NCT>(sc, region, l8, g0, g0 && k0 != N - 1);                                    \
            symres_stage_pick<NCT>(region, rp, live0, p0);                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            symres_stage_park<NCT>(sd, region, l8, g1, g1 && k1 != N - 1);                                    \
            {   /* the LDS-resident tile: picked up like the others, then put back one float4 per lane and    \
                   piece (conflict-free 16-byte reads in the products) over the wave's own staging block */   \
                SymResTile<NCT> p1;                                                                           \
                symres_stage_pick<NCT>(region, rp, live1, p1);                                                \
                asm volatile("" ::: "memory");                                                                \
                _Pragma("unroll")                                                                             \
                for (uint32_t i = 0; i < n; ++i) ltw[i * 64] = p1.q[i];                                       \
            }                                                                                                 \
        } else {                                                                                              \
            {                                                                                                 \
                SymResTile<NCT> p1;                                                                           \
                symres_issue<NCT>(P, k1, rp, live1, p1);                                                      \
                symres_issue<NCT>(S, k0, rp, live0, s0);                                                      \
                symres_issue<NCT>(S, k1, rp, live1, s1);                                                      \
                __builtin_amdgcn_sched_barrier(0);                                                            \
                symres_mask<NCT>(N, k1, live1, p1);                                                           \
                _Pragma("unroll")                                                                             \
                for (uint32_t i = 0; i < n; ++i) ltw[i * 64] = p1.q[i];                                       \
            }                                                                                                 \
            symres_issue<NCT>(P, k0, rp, live0, p0);  /* takes the registers the LDS-resident tile came through */ \
            __builtin_amdgcn_sched_barrier(0);                                                                \
            symres_mask<NCT>(N, k0, live0, s0);                                                               \
            symres_mask<NCT>(N, k1, live1, s1);                                                               \
            symres_mask<NCT>(N, k0, live0, p0);                                                               \
        }                                                                                                     \
        _Pragma("unroll")                                                                                     \
        for (uint32_t i = 0; i < G::P0_LDS_QUADS; ++i) lt0[i * G::THREADS] = p0.q[i];

    if constexpr (SHARED) {
        // the one pair, once per workgroup: every problem below finds its tiles where a plain solve leaves them after its load
        // (edge blocks zeroed, the Pinv k1 tile over the wave's staging block, which nothing touches again)
#ifdef GBDPCG_RS_STAMPS
        const uint32_t rs_round = 0;
#endif
        GBDPCG_SYMRES_LANE_ROWS(lane)
        (void)grp;
        float4_alias *ltw = reinterpret_cast<float4_alias *>(smem + wave * G::GROUPS * G::REGION) + lane;
        const float *S = a.S, *P = a.Pinv;
        GBDPCG_SYMRES_LOAD_TILES()
    }

    for (uint32_t prob = blockIdx.x, pi = 0; prob < a.batch; prob += gridDim.x, ++pi) {
#ifdef GBDPCG_RS_STAMPS
        ++rs_round;
#endif
        GBDPCG_RS_STAMP(0)
        if constexpr (!VERIFY) {
            if (pi == 0 || pi - takes_from >= 64) {
                const uint32_t left = (a.batch - prob + gridDim.x - 1) / gridDim.x;
                takes = pcg_takes_mask<SHARED>(a, prob, gridDim.x, left < 64 ? left : 64u, lane);
                takes_from = pi;
            }
            if (!((takes >> (pi - takes_from)) & 1ull)) continue;  // this launch is not the one that owns the problem
        } else {
            (void)takes;
            (void)takes_from;
            // (the previous problem's readers are past its last barrier; several barriers separate this from the tail)
            if (tid == 0) *vword = 1u;
        }
        // Everything a lane derives from its number is derived again for every problem, from an opaque copy: hoisted out of
        // the problem loop these dozen values were spilled to scratch (15 VGPRs) and reloaded in the tile-load phase.
        uint32_t lane_o = tid & 63u;
        asm volatile("" : "+v"(lane_o));
        GBDPCG_SYMRES_LANE_ROWS(lane_o)
        const uint32_t row0 = (live0 ? k0 * n + rp * 2 : 0u), row1 = (live1 ? k1 * n + rp * 2 : 0u);
        // x operand windows inside a padded mirror (n zeros before x_0 and after x_{N-1}); dead lanes read row 0
        const uint32_t xo0 = n + (live0 ? k0 : 0u) * n;
        // the LDS-resident tile (Pinv k1) of this lane: piece i at ltw[64 i], inside the wave's own block of regions
        float4_alias *ltw = reinterpret_cast<float4_alias *>(smem + wave * G::GROUPS * G::REGION) + lane_o;
        const uint32_t zo1 = n + (live1 ? k1 + 1 : 0u) * n + rp * 2;  // where this lane's k1 -> k1+1 products go
        const uint32_t zo0 = n + (live0 ? k0 : 0u) * n + rp * 2;      // ... and where the ones for its k0 rows arrive
        // the lane's own operand entries inside a mirror; dead lanes read the zero padding in front of x_0 instead, so
        // nothing downstream needs a select (v_cndmask with an SGPR mask turned out to be the costliest VALU op here)
        const uint32_t own0 = live0 ? n + row0 : 0u, own1 = live1 ? n + row1 : 0u;
        const float *S = a.S + (SHARED ? (size_t)0 : prob * mstride);   // (SHARED: not looked at again, the tiles are in)
        const float *P = a.Pinv + (SHARED ? (size_t)0 : prob * mstride);
        (void)S;
        (void)P;
        const size_t voff = (size_t)prob * len;
        // lambda (into its own array and into the operand mirror) and gamma (into the mirror of r, where r = gamma - S lambda
        // will replace it) are requested FIRST, by LDS-DMA -- no register, no instruction of the tile phase waits for them --
        // so that their round trips run under the 400 KB of tile loads instead of in front of the first product
        // (the cluster kernel's lesson: 3.5 us per problem were spent waiting for 21 KB of vectors).
        for (uint32_t q = wave; q * 64 < len; q += WAVES) {
            const uint32_t e = q * 64 + lane_o;
            if (e < len) {
                symres_dma_dword(a.lambda + voff, e * 4, (uint32_t)(uintptr_t)(ls + q * 64));
                symres_dma_dword(a.lambda + voff, e * 4, (uint32_t)(uintptr_t)(xa + n + q * 64));
                symres_dma_dword(a.gamma + voff, e * 4, (uint32_t)(uintptr_t)(xb + n + q * 64));
            }
        }

        // Everything but the tiles (lambda, r, p) lives in LDS between the phases; only y crosses a barrier in registers.
        if constexpr (!SHARED) {
            GBDPCG_SYMRES_LOAD_TILES()
        }
        GBDPCG_RS_STAMP(2)

        for (uint32_t i = tid; i < n; i += G::THREADS) {
            xa[i] = 0.f; xa[n + len + i] = 0.f; xa[2 * n + len + i] = 0.f;
            xb[i] = 0.f; xb[n + len + i] = 0.f; xb[2 * n + len + i] = 0.f;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of lambda and gamma has landed in LDS
        __syncthreads();
        GBDPCG_RS_STAMP(3)

        // One matrix-vector product over this lane's two block-rows.  XM: padded mirror of the operand.
        // Leaves y[1] complete and y[0] without the rows' share of R_{k0-1}^T x_{k0-1}, which the previous
        // group puts into zs (GBDPCG_SYMRES_FINISH_Y reads it after the next barrier); PART = the lane's
        // share of x . (M x) INCLUDING what it sent to zs.
#define GBDPCG_SYMRES_MV(T0, LQ0, T1, K1LDS, XM)                                                              \
            symres_mv2<NCT, LQ0, K1LDS>(T0, lt0, T1, ltw, reinterpret_cast<const float2 *>(XM + xo0), o0, o1, lane, \
                                        y[0], y[1], u0, tt);
#define GBDPCG_SYMRES_PRODUCT(T0, LQ0, T1, K1LDS, XM, PART)                                                  \
        {                                                                                                     \
            float tt[NCT], u0[2], u1[2];                                                                      \
            const float2 o0 = *reinterpret_cast<const float2 *>(XM + own0);                                   \
            const float2 o1 = *reinterpret_cast<const float2 *>(XM + own1);                                   \
            GBDPCG_SYMRES_MV(T0, LQ0, T1, K1LDS, XM)                                                            \
            symres_reduce_scatter14(tt, lane, u1);                                                            \
            y[1][0] += u0[0];                                                                                 \
            y[1][1] += u0[1];                                                                                 \
            if (live1) *reinterpret_cast<float2 *>(zs + zo1) = make_float2(u1[0], u1[1]);                     \
            const float2 xn = *reinterpret_cast<const float2 *>(XM + zo1);                                    \
            PART = o0.x * y[0][0];                                                                            \
            PART = fma_t(o0.y, y[0][1], PART);                                                                \
            PART = fma_t(o1.x, y[1][0], PART);                                                                \
            PART = fma_t(o1.y, y[1][1], PART);                                                                \
            PART = fma_t(u1[0], xn.x, PART);  /* dead lanes: u1 == 0 (zero tiles, zero own entries) */         \
            PART = fma_t(u1[1], xn.y, PART);                                                                  \
        }
#define GBDPCG_SYMRES_FINISH_Y()                                                                              \
        {                                                                                                     \
            const float2 z = *reinterpret_cast<const float2 *>(zs + zo0);                                     \
            y[0][0] += z.x;  /* lanes without rows read rows of zs nobody writes: zero since kernel start */  \
            y[0][1] += z.y;                                                                                   \
        }
        float2 *xa0 = reinterpret_cast<float2 *>(xa + n + row0), *xa1 = reinterpret_cast<float2 *>(xa + n + row1);
        float2 *xb0 = reinterpret_cast<float2 *>(xb + n + row0), *xb1 = reinterpret_cast<float2 *>(xb + n + row1);
        float2 *ls0 = reinterpret_cast<float2 *>(ls + row0), *ls1 = reinterpret_cast<float2 *>(ls + row1);

        float y[2][2], part;
        // r = gamma - S lambda                                            (pcg.cuh:118-126)
        GBDPCG_SYMRES_PRODUCT(s0, 0, s1, false, xa, part)
        __syncthreads();
        GBDPCG_SYMRES_FINISH_Y()
        if (live0) {   // gamma is waiting in the mirror of r
            const float2 gm = *xb0;
            *xb0 = make_float2(gm.x - y[0][0], gm.y - y[0][1]);
        }
        if (live1) {
            const float2 gm = *xb1;
            *xb1 = make_float2(gm.x - y[1][0], gm.y - y[1][1]);
        }
        __syncthreads();

        // Workgroup sum of PART (same order in every thread: the exit branch stays uniform) and the
        // completion of y[0]; the partials and the zs entries come back in one LDS round trip.
#define GBDPCG_SYMRES_SUM(RED, TOT)                                                                           \
        {                                                                                                     \
            const float ws = wave_sum(part);                                                                  \
            if (lane == 0) RED[wave] = ws;                                                                    \
            __syncthreads();                                                                                  \
            const float4 ra = reinterpret_cast<const float4 *>(RED)[0], rb = reinterpret_cast<const float4 *>(RED)[1]; \
            float2 zz = *reinterpret_cast<const float2 *>(zs + zo0);                                          \
            TOT = ((ra.x + ra.y) + (ra.z + ra.w)) + ((rb.x + rb.y) + (rb.z + rb.w));                          \
            /* pinned here: left alone, hipcc sinks this LDS read below the division that follows (a second  \
               round trip on the critical path) */                                                            \
            asm volatile("" : "+v"(zz.x), "+v"(zz.y));                                                        \
            y[0][0] += zz.x;                                                                                  \
            y[0][1] += zz.y;                                                                                  \
        }
        // r~ = Pinv r ; p = r~ ; eta = r.r~                               (pcg.cuh:130-149)
        GBDPCG_SYMRES_PRODUCT(p0, G::P0_LDS_QUADS, p0, true, xb, part)
        float eta;
        GBDPCG_SYMRES_SUM(red1, eta)
        if (live0) *xa0 = make_float2(y[0][0], y[0][1]);
        if (live1) *xa1 = make_float2(y[1][0], y[1][1]);
        __syncthreads();

        // prefetch schedule for the next problem of this workgroup: two lines per thread and iteration
        const uint32_t nprob = prob + gridDim.x;
        constexpr uint32_t pf_steps = (2 * n * n * 4 + 63) / 64 + 1;  // 64-byte steps per [D|R] row (symres_touch)
        // (SHARED: the next problem's matrices are the ones already here)
        const uint32_t pf_per_matrix = !SHARED && GBDPCG_RS_PREFETCH && nprob < a.batch ? (N * pf_steps + G::THREADS - 1) / G::THREADS : 0u;
        uint32_t pf = 0;
#define GBDPCG_SYMRES_PREFETCH()                                                                              \
        if (pf < pf_per_matrix) {                                                                             \
            symres_touch<NCT>(a.S + nprob * mstride, N, pf * G::THREADS + tid, dump);                         \
            symres_touch<NCT>(a.Pinv + nprob * mstride, N, pf * G::THREADS + tid, dump);                      \
            ++pf;                                                                                             \
        }

        uint32_t iter = 0;
        bool max_iter_exit = true;
        GBDPCG_RS_STAMP(4)
        for (; iter < a.max_iter; ++iter) {                               // pcg.cuh:154
            GBDPCG_SYMRES_PREFETCH()
            // upsilon = S p ; alpha = eta / (p.upsilon)                   (pcg.cuh:156-169)
            GBDPCG_SYMRES_PRODUCT(s0, 0, s1, false, xa, part)
            // the lane's own entries of p, lambda, r: requested before the reduction, used after it
            const float2 pa0 = *xa0, pa1 = *xa1, la0 = *ls0, la1 = *ls1, ra0 = *xb0, ra1 = *xb1;
            float den;
            GBDPCG_SYMRES_SUM(red0, den)
            const float alpha = eta / den;
            // lambda += alpha p ; r -= alpha upsilon                      (pcg.cuh:172-176)
            if (live0) {
                *ls0 = make_float2(fma_t(alpha, pa0.x, la0.x), fma_t(alpha, pa0.y, la0.y));
                *xb0 = make_float2(fma_t(-alpha, y[0][0], ra0.x), fma_t(-alpha, y[0][1], ra0.y));
            }
            if (live1) {
                *ls1 = make_float2(fma_t(alpha, pa1.x, la1.x), fma_t(alpha, pa1.y, la1.y));
                *xb1 = make_float2(fma_t(-alpha, y[1][0], ra1.x), fma_t(-alpha, y[1][1], ra1.y));
            }
            __syncthreads();
            // r~ = Pinv r ; eta_new = r.r~                                (pcg.cuh:180-193)
            GBDPCG_SYMRES_PRODUCT(p0, G::P0_LDS_QUADS, p0, true, xb, part)
            const float2 pb0 = *xa0, pb1 = *xa1;
            float eta_new;
            GBDPCG_SYMRES_SUM(red1, eta_new)
            if (fabsf(eta_new) < a.tol) {                                 // pcg.cuh:195
                ++iter;
                max_iter_exit = false;
                break;
            }
            const float beta = eta_new / eta;                             // pcg.cuh:199-206
            eta = eta_new;
            if (live0) *xa0 = make_float2(fma_t(beta, pb0.x, y[0][0]), fma_t(beta, pb0.y, y[0][1]));
            if (live1) *xa1 = make_float2(fma_t(beta, pb1.x, y[1][0]), fma_t(beta, pb1.y, y[1][1]));
            __syncthreads();
        }
#undef GBDPCG_SYMRES_SUM
#undef GBDPCG_SYMRES_PRODUCT
#undef GBDPCG_SYMRES_MV
#undef GBDPCG_SYMRES_FINISH_Y

        GBDPCG_RS_STAMP(5)
        if constexpr (VERIFY) {
            // L_{k+1} == R_k^T for both matrices and both of the lane's block-rows against the R halves of the tiles, S then
            // Pinv (all four sets of pieces in flight at once spill).  The Pinv k1 tile is compared from LDS.
            const bool cmp0 = live0 && k0 + 1 < N, cmp1 = live1 && k1 + 1 < N;
            bool bad;
            {
                float4 l0[n / 2], l1[n / 2], r0[n / 2], r1[n / 2];
                symres_lcols_issue<NCT>(S, k0, rp, cmp0, l0);
                symres_lcols_issue<NCT>(S, k1, rp, cmp1, l1);
#pragma unroll
                for (uint32_t j = 0; j < n / 2; ++j) {
                    r0[j] = s0.q[n / 2 + j];
                    r1[j] = s1.q[n / 2 + j];
                }
                bad = symres_r_differs<NCT>(r0, l0, cmp0);
                bad |= symres_r_differs<NCT>(r1, l1, cmp1);
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                float4 l0[n / 2], l1[n / 2], r0[n / 2], r1[n / 2];
                symres_lcols_issue<NCT>(P, k0, rp, cmp0, l0);
                symres_lcols_issue<NCT>(P, k1, rp, cmp1, l1);
#pragma unroll
                for (uint32_t j = 0; j < n / 2; ++j) {
                    r0[j] = p0.q[n / 2 + j];
                    r1[j] = ltw[(n / 2 + j) * 64];
                }
                bad |= symres_r_differs<NCT>(r0, l0, cmp0);
                bad |= symres_r_differs<NCT>(r1, l1, cmp1);
            }
            if (bad) *vword = 0u;   // (every writer writes the same value)
        }
        while (pf < pf_per_matrix) { GBDPCG_SYMRES_PREFETCH() }  // short solves: the rest of the prefetch
#undef GBDPCG_SYMRES_PREFETCH

        // outputs                                                         (pcg.cuh:212,215)
        __syncthreads();
        // verifying kernel: a problem that failed the test is left to the general launch, untouched
        const bool keep = VERIFY ? __builtin_amdgcn_readfirstlane(*reinterpret_cast<volatile uint32_t *>(vword)) != 0u : true;
        if (keep) {
            for (uint32_t i = tid; i < len; i += G::THREADS) {
                a.lambda[voff + i] = ls[i];
                if (a.r) a.r[voff + i] = xb[n + i];
                if (a.p) a.p[voff + i] = xa[n + i];
            }
            if (tid == 0) {
                a.iters[prob] = iter;
                if (a.max_iter_exit) a.max_iter_exit[prob] = max_iter_exit ? 1 : 0;
            }
        }
        if (VERIFY && tid == 0) {
            a.verdict_out[prob] = keep ? 1 : 0;
            // one more problem for the general launch, which returns at once while this count is 0 (pcg_reject_none)
            if (!keep && a.reject_count) __hip_atomic_fetch_add(a.reject_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();  // LDS (tile, vectors, verdict word) is reused by the next problem
        GBDPCG_RS_STAMP(6)
    }
#undef GBDPCG_SYMRES_LOAD_TILES
#undef GBDPCG_SYMRES_LANE_ROWS
#undef GBDPCG_SYMRES_K0
    // The prefetch loads are invisible to the compiler's counters; s_endpgm drains the wave's memory counters in
    // hardware, and this makes it explicit: none of them can still be in flight (towards this workgroup's LDS dump
    // area) when the workgroup's LDS is handed to another one.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// n = 14, fp32, N <= 128, a preconditioner given, matrices 8-byte aligned (16-byte for the verifying kernel).  GBDPCG_NO_RESIDENT_SYM
// disables the path (tuning runs).
template <typename T> bool resident_sym_shape(uint32_t n, uint32_t N)
{
    static const bool off = getenv("GBDPCG_NO_RESIDENT_SYM") != nullptr;
    if (off || sizeof(T) != 4 || n != 14) return false;
    return N <= SymResGeom<14>::MAX_KNOTS;
}

// (+ 256: the dump area of the prefetch loads; + 16: the verifying kernel's verdict word behind it)
static size_t resident_sym_lds(uint32_t n, uint32_t N, bool verify = false)
{
    return ((size_t)SymResGeom<14>::TILE_LDS_FLOATS + 3 * (size_t)align16<float>((N + 3) * n) +
            2 * SymResGeom<14>::WAVES + align16<float>(N * n)) * sizeof(float) + 256 + (verify ? 16 : 0);
}

static bool resident_sym_staged(const void *S, const void *Pinv)
{
    // coalesced 16-byte tile loads need 16-byte aligned matrices (every hipMalloc'ed buffer is)
    static const bool no_staging = getenv("GBDPCG_RS_DIRECT_LOADS") != nullptr;  // tuning runs only
    return !no_staging && !((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(Pinv)) % 16);
}

template <typename T>
bool resident_sym_verifies(const DeviceInfo &dev, uint32_t n, uint32_t N, const T *S, const T *Pinv)
{
    return sizeof(T) == 4 && S && Pinv && resident_sym_shape<T>(n, N) && resident_sym_staged(S, Pinv) &&
           resident_sym_lds(n, N, true) <= dev.lds_per_wg_max;
}

// verify: the verifying kernel (every problem, a.verdict_out written); the caller has checked resident_sym_verifies.
template <typename T>
static bool launch_pcg_resident_sym_impl(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool verify,
                                         bool shared = false)
{
    if constexpr (sizeof(T) == 4) {
        if (!a.symmetric || !a.Pinv || !resident_sym_shape<T>(a.n, a.N)) return false;
        if ((reinterpret_cast<uintptr_t>(a.S) % 8) || (reinterpret_cast<uintptr_t>(a.Pinv) % 8)) return false;
        const size_t lds = resident_sym_lds(a.n, a.N, verify);
        if (lds > dev.lds_per_wg_max) return false;
        const bool staged = resident_sym_staged(a.S, a.Pinv);
        if (verify && (!staged || !a.verdict_out)) return false;
        if (verify && shared) return false;   // a shared pair has ONE verdict, found before the launch
        auto kern = verify ? pcg_resident_sym_kernel<14, true, true>
                           : staged ? pcg_resident_sym_kernel<14, true, false> : pcg_resident_sym_kernel<14, false, false>;
        if (shared) kern = staged ? pcg_resident_sym_kernel<14, true, false, true> : pcg_resident_sym_kernel<14, false, false, true>;
        // on every launch, like the other launchers: HIP keeps the attribute per device, and a process may hold
        // handles on several devices (one host thread each)
        *err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (*err != hipSuccess) return true;
        uint32_t grid = (uint32_t)dev.num_cus;  // one workgroup owns a CU's register file and most of its LDS
        if (grid > a.batch) grid = a.batch;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SymResGeom<14>::THREADS), lds, s, a);
        *err = hipGetLastError();
        return true;
    } else {
        return false;
    }
}

template <typename T>
bool launch_pcg_resident_sym(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool shared)
{
    return launch_pcg_resident_sym_impl<T>(dev, a, s, err, false, shared);
}

template <typename T>
bool launch_pcg_resident_sym_verify(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err)
{
    return launch_pcg_resident_sym_impl<T>(dev, a, s, err, true);
}

template bool resident_sym_shape<float>(uint32_t, uint32_t);
template bool resident_sym_shape<double>(uint32_t, uint32_t);
template bool launch_pcg_resident_sym<float>(const DeviceInfo &, const PcgArgs<float> &, hipStream_t, hipError_t *, bool);
template bool launch_pcg_resident_sym<double>(const DeviceInfo &, const PcgArgs<double> &, hipStream_t, hipError_t *, bool);
template bool resident_sym_verifies<float>(const DeviceInfo &, uint32_t, uint32_t, const float *, const float *);
template bool resident_sym_verifies<double>(const DeviceInfo &, uint32_t, uint32_t, const double *, const double *);
template bool launch_pcg_resident_sym_verify<float>(const DeviceInfo &, const PcgArgs<float> &, hipStream_t, hipError_t *);
template bool launch_pcg_resident_sym_verify<double>(const DeviceInfo &, const PcgArgs<double> &, hipStream_t, hipError_t *);

}  // namespace gbdpcg
