// pcg_resident_sym_tiles.hpp -- where things are in the resident symmetric solve (pcg_resident_sym.hip): the geometry of the
// workgroup, the ONE description of its dynamic LDS (kernel pointers and host size both come from it), the block-rows of a lane,
// and the ingest of the four quarter-tiles.
#pragma once

#include "bt_device.hpp"

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
    // Prefetch distances of the product (symres_mv2), in steps: operand pairs AHX ahead, LDS-resident tile pieces AHT ahead.
    // 3 and 1: the measured optimum; deeper prefetch is slower.
    static constexpr uint32_t AHX = 3, AHT = 1;
};

// The dynamic LDS of one workgroup, in this order from its start; everything behind the tile blocks moves with N.
//   regions  WAVES x GROUPS staging regions; after the ingest a wave's block of 8 holds its share of the Pinv k1 tile
//   lt0      the P0_LDS_QUADS leading pieces of every lane's Pinv k0 tile (one float4 per lane and piece, stride THREADS)
//   xa, xb   padded mirrors of p (lambda in the prologue) and of r: n zeros in front of x_0, 2n behind x_{N-1}
//   zs       R_{k-1}^T x_{k-1} for the even block-rows, padded like a mirror
//   red0/1   one partial per wave for the two workgroup sums of an iteration
//   ls       lambda (vec floats)
//   dump     destination of the prefetch loads (symres_touch): one dword per lane, shared by all waves, never read
//   verdict  verifying kernel only: the workgroup's verdict on the current problem (1 = symmetric)
// lt0 and xa are float offsets; behind xa the kernel steps through the list with these sizes, and bytes() is where it ends.
template <int NCT> struct SymResLds {
    using G = SymResGeom<NCT>;
    static constexpr uint32_t DUMP_BYTES = 64 * 4, VERDICT_BYTES = 16;
    static constexpr uint32_t lt0 = G::WAVES * G::GROUPS * G::REGION, xa = lt0 + G::P0_LDS_QUADS * G::THREADS * 4;
    uint32_t padded, vec;
    __host__ __device__ constexpr explicit SymResLds(uint32_t N) : padded(align16<float>((N + 3) * NCT)), vec(align16<float>(N * NCT)) {}
    constexpr size_t bytes(bool verify) const
    {
        return ((size_t)xa + 3 * padded + 2 * G::WAVES + vec) * 4 + DUMP_BYTES + (verify ? VERDICT_BYTES : 0);
    }
};

// One block-row of one matrix as this lane sees it: q[i] = (M[2rp, 2i], M[2rp, 2i+1], M[2rp+1, 2i], M[2rp+1, 2i+1])
// over the 2n columns of [D | R] -- the two columns of a ROW adjacent, so that both the main product (a row
// pair times the x pair as it comes out of LDS, even and odd columns accumulated apart) and the transposed
// product (a row pair times one broadcast x entry) are single v_pk_fma_f32 instructions.
template <int NCT> struct SymResTile {
    float4 q[SymResGeom<NCT>::QUADS];
};

// Which pair of block-rows (2j, 2j+1) a group owns is free; it is chosen so that the four groups that share an LDS pass
// (lanes 0-31 / 32-63 of a wave) own pairs j, j+4, j+8, j+12: their rows of a vector then start 48 banks apart
// (a pair is 2n = 28 floats) and the 8-byte accesses of 4 x 7 lanes tile the 64 banks instead of colliding two by
// two, as consecutive pairs do (bases 0, 28, 56, 20 mod 64: 13 % of an iteration's LDS-array cycles were conflicts).
__host__ __device__ constexpr uint32_t symres_pair_of_group(uint32_t wave, uint32_t grp)
{
    return 16 * (wave >> 1) + 4 * (grp & 3u) + 2 * (wave & 1u) + (grp >> 2);
}

// What a lane derives from its number: rows 2rp, 2rp+1 (rp < n/2) of block-rows k0, k1 = k0 + 1, and its float offsets in LDS.
template <int NCT> struct SymResLane {
    uint32_t rp, k0, k1;
    bool live0, live1;     // the lane owns rows of k0 / k1 at this N
    uint32_t row0, row1;   // its rows inside a plain vector (dead lanes: 0)
    uint32_t xo0;          // the operand window [x_k0 ; x_k1 ; x_k1+1] inside a padded mirror; dead lanes read row 0
    uint32_t zo0, zo1;     // inside zs or a mirror: where the products for its k0 rows arrive, where its k1 -> k1+1 products go
    // the lane's own operand entries inside a mirror; dead lanes read the zero padding in front of x_0 instead, so
    // nothing downstream needs a select (v_cndmask with an SGPR mask turned out to be the costliest VALU op here)
    uint32_t own0, own1;
};
template <int NCT> __device__ __forceinline__ SymResLane<NCT> symres_lane(uint32_t lane, uint32_t wave, uint32_t N)
{
    constexpr uint32_t n = NCT;
    SymResLane<NCT> c;
    c.rp = lane & 7u;
    c.k0 = 2 * symres_pair_of_group(wave, lane >> 3);
    c.k1 = c.k0 + 1;
    c.live0 = c.rp < n / 2 && c.k0 < N;
    c.live1 = c.rp < n / 2 && c.k1 < N;
    c.row0 = c.live0 ? c.k0 * n + c.rp * 2 : 0u;
    c.row1 = c.live1 ? c.k1 * n + c.rp * 2 : 0u;
    c.xo0 = n + (c.live0 ? c.k0 : 0u) * n;
    c.zo1 = n + (c.live1 ? c.k1 + 1 : 0u) * n + c.rp * 2;
    c.zo0 = n + (c.live0 ? c.k0 : 0u) * n + c.rp * 2;
    c.own0 = c.live0 ? n + c.row0 : 0u;
    c.own1 = c.live1 ? n + c.row1 : 0u;
    return c;
}

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
// (non-temporal: a tile is read once per solve)
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
        const auto v = __builtin_nontemporal_load(reinterpret_cast<const NtVec<float, 4>::type *>(src + safe));
        st.b[i] = make_float4(v.x, v.y, v.z, v.w);
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

// The four quarter-tiles of one problem's S and P: three into registers (s0, s1, p0), the Pinv k1 tile into the wave's block of
// regions (ltw: this lane's piece i at ltw[64 i]), the leading pieces of p0 into lt0 as well.  region: the group's staging region.
// Wave-local: no barrier.  issued() runs once the staged requests are out (the diagnostic build's stamp; nothing when shipped).
template <int NCT, bool STAGED, class Issued>
__device__ __forceinline__ void symres_load_tiles(const float *S, const float *P, uint32_t N, const SymResLane<NCT> &c, float *region,
                                                  float4_alias *ltw, float4 *lt0, SymResTile<NCT> &s0, SymResTile<NCT> &s1,
                                                  SymResTile<NCT> &p0, Issued issued)
{
    using G = SymResGeom<NCT>;
    constexpr uint32_t n = NCT;
    const uint32_t rp = c.rp, k0 = c.k0, k1 = c.k1;
    if constexpr (STAGED) {
        const uint32_t l8 = rp;
        const bool g0 = k0 < N, g1 = k1 < N;  // whole group alive
        // all four tiles are requested at once (4 x 52 VGPRs, nothing else is live yet): one memory
        // round trip per problem instead of one per tile
        SymResStage<NCT> sa, sb, sc, sd;
        symres_stage_issue<NCT>(S, k0, g0, l8, sa);
        symres_stage_issue<NCT>(S, k1, g1, l8, sb);
        symres_stage_issue<NCT>(P, k0, g0, l8, sc);
        symres_stage_issue<NCT>(P, k1, g1, l8, sd);
        __builtin_amdgcn_sched_barrier(0);
        issued();
        symres_stage_park<NCT>(sa, region, l8, g0, g0 && k0 != N - 1);
        symres_stage_pick<NCT>(region, rp, c.live0, s0);
        __builtin_amdgcn_sched_barrier(0);
        symres_stage_park<NCT>(sb, region, l8, g1, g1 && k1 != N - 1);
        symres_stage_pick<NCT>(region, rp, c.live1, s1);
        __builtin_amdgcn_sched_barrier(0);
        symres_stage_park<NCT>(sc, region, l8, g0, g0 && k0 != N - 1);
        symres_stage_pick<NCT>(region, rp, c.live0, p0);
        __builtin_amdgcn_sched_barrier(0);
        symres_stage_park<NCT>(sd, region, l8, g1, g1 && k1 != N - 1);
        {   // the LDS-resident tile: picked up like the others, then put back one float4 per lane and
            // piece (conflict-free 16-byte reads in the products) over the wave's own staging block
            SymResTile<NCT> p1;
            symres_stage_pick<NCT>(region, rp, c.live1, p1);
            asm volatile("" ::: "memory");
#pragma unroll
            for (uint32_t i = 0; i < n; ++i) ltw[i * 64] = p1.q[i];
        }
    } else {
        {
            SymResTile<NCT> p1;
            symres_issue<NCT>(P, k1, rp, c.live1, p1);
            symres_issue<NCT>(S, k0, rp, c.live0, s0);
            symres_issue<NCT>(S, k1, rp, c.live1, s1);
            __builtin_amdgcn_sched_barrier(0);
            symres_mask<NCT>(N, k1, c.live1, p1);
#pragma unroll
            for (uint32_t i = 0; i < n; ++i) ltw[i * 64] = p1.q[i];
        }
        symres_issue<NCT>(P, k0, rp, c.live0, p0);  // takes the registers the LDS-resident tile came through
        __builtin_amdgcn_sched_barrier(0);
        symres_mask<NCT>(N, k0, c.live0, s0);
        symres_mask<NCT>(N, k1, c.live1, s1);
        symres_mask<NCT>(N, k0, c.live0, p0);
    }
#pragma unroll
    for (uint32_t i = 0; i < G::P0_LDS_QUADS; ++i) lt0[i * G::THREADS] = p0.q[i];
}

}  // namespace gbdpcg
