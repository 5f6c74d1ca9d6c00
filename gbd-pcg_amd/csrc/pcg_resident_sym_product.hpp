// pcg_resident_sym_product.hpp -- one matrix-vector product of the resident symmetric solve (pcg_resident_sym.hip) over a lane's
// two block-rows, with the lane's share of the inner product, and the workgroup sum that completes both.
#pragma once

#include "pcg_resident_sym_tiles.hpp"

namespace gbdpcg {

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

// Both block-rows of the lane against the operand window [x_k0 ; x_k1 ; x_k1+1] (21 LDS pairs, x_k1 read once
// for both), in two phases of n/2 steps with six independent packed instructions per step:
//   phase 1, x_k1 pair j         : R_k0 piece j (+ its transposed share tt0) and D_k1 piece j
//   phase 2, x_k0 / x_k1+1 pair j: D_k0 piece j, and R_k1 piece j (+ tt1)
// (a pass in operand order -- D_k0 alone, then the shared middle, then R_k1 alone -- leaves two thin
// stretches in which a wave has only two dependent FMA chains to issue and waits on their latency: 3.5 %
// slower).  The x_k1 pairs are requested before anything else, later pairs AHX steps ahead, LDS-resident
// tile pieces AHT steps ahead (SymResGeom).  tt0 is reduce-scattered between the two phases (u0), tt1 by the caller.
// LQ0 leading pieces of the k0 tile come from LDS (lt0, one float4 per lane and piece, stride THREADS);
// K1_FROM_LDS: the whole k1 tile is read from LDS (lt1, one float4 per lane and piece, stride 64).
// The steps are pinned in source order and the accumulators anchored: left to itself hipcc hoists all
// LDS reads to the top and sinks the accumulator chains below the reduce-scatter, and the operands of
// every step stay live (with three resident tiles, 168 VGPRs, that spills).
template <int NCT, uint32_t LQ0, bool K1_FROM_LDS>
__device__ __forceinline__ void symres_mv2(const SymResTile<NCT> &t0, const float4 *lt0, const SymResTile<NCT> &t1,
                                           const float4_alias *lt1, const float2 *xk2, float2 o0, float2 o1, uint32_t lane,
                                           float (&y0)[2], float (&y1)[2], float (&u0)[2], float (&tt1)[NCT])
{
    constexpr uint32_t n = NCT, H = n / 2, TH = SymResGeom<NCT>::THREADS;
    constexpr uint32_t AHX = SymResGeom<NCT>::AHX, AHT = SymResGeom<NCT>::AHT;
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

// One matrix-vector product y = M x over this lane's two block-rows (tiles t0, t1; lt0, ltw: their LDS-resident parts, see
// symres_mv2).  xm: padded mirror of the operand x.  Leaves y[1] complete and y[0] without the rows' share of
// R_{k0-1}^T x_{k0-1}, which the previous group puts into zs -- to be added after the next barrier (symres_sum_finish_y
// does).  Returns the lane's share of x . (M x) INCLUDING what it sent to zs: the transposed product of k1 is
// accounted on the producer side (u1 . x_{k1+1}), so the workgroup sum needs no barrier of its own.
template <int NCT, uint32_t LQ0, bool K1_FROM_LDS>
__device__ __forceinline__ float symres_product(const SymResTile<NCT> &t0, const float4 *lt0, const SymResTile<NCT> &t1,
                                                const float4_alias *ltw, const float *xm, float *zs, const SymResLane<NCT> &c,
                                                uint32_t lane, float (&y)[2][2])
{
    float tt[NCT], u0[2], u1[2];
    const float2 o0 = *reinterpret_cast<const float2 *>(xm + c.own0);
    const float2 o1 = *reinterpret_cast<const float2 *>(xm + c.own1);
    symres_mv2<NCT, LQ0, K1_FROM_LDS>(t0, lt0, t1, ltw, reinterpret_cast<const float2 *>(xm + c.xo0), o0, o1, lane, y[0], y[1], u0, tt);
    symres_reduce_scatter14(tt, lane, u1);
    y[1][0] += u0[0];
    y[1][1] += u0[1];
    if (c.live1) *reinterpret_cast<float2 *>(zs + c.zo1) = make_float2(u1[0], u1[1]);
    const float2 xn = *reinterpret_cast<const float2 *>(xm + c.zo1);
    float part = o0.x * y[0][0];
    part = fma_t(o0.y, y[0][1], part);
    part = fma_t(o1.x, y[1][0], part);
    part = fma_t(o1.y, y[1][1], part);
    part = fma_t(u1[0], xn.x, part);  // dead lanes: u1 == 0 (zero tiles, zero own entries)
    part = fma_t(u1[1], xn.y, part);
    return part;
}

// Workgroup sum of part (same order in every thread: a branch on it stays uniform) and the completion of y[0] (zs_own = zs + the lane's zo0; lanes without rows read
// rows of zs nobody writes: zero since kernel start): the partials
// (red: one float per wave) and the zs entries come back in one LDS round trip.  Contains the barrier that also publishes zs.
__device__ __forceinline__ float symres_sum_finish_y(float part, float *red, uint32_t wave, uint32_t lane, const float *zs_own,
                                                     float (&y0)[2])
{
    const float ws = wave_sum(part);
    if (lane == 0) red[wave] = ws;
    __syncthreads();
    const float4 ra = reinterpret_cast<const float4 *>(red)[0], rb = reinterpret_cast<const float4 *>(red)[1];
    float2 zz = *reinterpret_cast<const float2 *>(zs_own);
    const float tot = ((ra.x + ra.y) + (ra.z + ra.w)) + ((rb.x + rb.y) + (rb.z + rb.w));
    // pinned here: left alone, hipcc sinks this LDS read below the division that follows (a second
    // round trip on the critical path)
    asm volatile("" : "+v"(zz.x), "+v"(zz.y));
    y0[0] += zz.x;
    y0[1] += zz.y;
    return tot;
}

}  // namespace gbdpcg
