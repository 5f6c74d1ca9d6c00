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
// block-rows k0 = 2j, k1 = 2j+1 (group -> j: symres_pair_of_group): all 2n columns of [D_k | R_k], 56 registers per
// block-row per matrix.  Per block-row and product
//     y_k     +=  [D_k | R_k] [x_k ; x_{k+1}]    2n FMAs per row, columns ascending, no cross-lane fold
//     y_{k+1} +=  R_k^T x_k                      n partial values per lane, reduce-scattered over the
//                                                8 lanes of the group with DPP (half-mirror, quad
//                                                perms): lane rp ends up with entries 2rp, 2rp+1
// The transposed product of k0 lands in the same lane's k1 rows (registers); the one of k1 belongs to
// the next group and goes through LDS.  Its share of the inner product is accounted on the producer
// side (u . x_{k1+1}), so the workgroup reduction needs no extra barrier: 4 barriers per iteration.
//
// pcg_resident_sym_tiles.hpp: geometry, the LDS layout (SymResLds), a lane's block-rows, the tile ingest;
// pcg_resident_sym_product.hpp: the product, its reduce-scatter and the workgroup sum; here: the kernel and its launchers.
#include <cstdlib>

#include "bt_device.hpp"
#include "bt_sym.hpp"
#include "internal.hpp"
#include "pcg_resident_sym_product.hpp"
#include "pcg_resident_sym_tiles.hpp"

#ifndef GBDPCG_RS_PREFETCH
#define GBDPCG_RS_PREFETCH 1   // 0: variants/libgbdpcg_nopf.so (tests/test_gpu_multi.py)
#endif

namespace gbdpcg {

template <int NCT> constexpr uint32_t kSymResTouchSteps = (2 * NCT * NCT * 4 + 63) / 64 + 1;  // 64-byte steps per [D|R] row

// Pull the NEXT problem's [D|R] blocks towards the Infinity Cache, one dword touched per 64 bytes (measured:
// a 128-byte stride leaves part of the stream in HBM and costs 3 us per batch), while this problem iterates: every CU finishes its solve at about the same time, so without this all 256 CUs hit HBM
// with their 401 KB tile loads in the same burst.  The load is an LDS-DMA (no VGPR destination, so
// nothing the compiler allocates can be clobbered when it lands) into a dump area of LDS that
// is never read; it is hidden from hipcc's waitcnt bookkeeping, so no barrier or LDS read waits for it.
template <int NCT>
__device__ __forceinline__ void symres_touch(const float *M, uint32_t N, uint32_t slot, uint32_t lds_dump)
{
    // slot -> (block-row k, 64-byte step j inside its [D_k | R_k]); L blocks are never touched
    constexpr uint32_t row_bytes = 2 * NCT * NCT * 4, steps = kSymResTouchSteps<NCT>;
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
// L_{k+1} == R_k^T of ONE matrix M for both of the lane's block-rows: true when either differs.  r0(j), r1(j): R piece j of the
// resident k0 / k1 tile, wherever it lives (registers, or LDS for the Pinv k1 tile).
template <int NCT, class R0, class R1>
__device__ __forceinline__ bool symres_rows_differ(const float *M, const SymResLane<NCT> &c, bool cmp0, bool cmp1, R0 r0_piece,
                                                   R1 r1_piece)
{
    constexpr uint32_t n = NCT;
    float4 l0[n / 2], l1[n / 2], r0[n / 2], r1[n / 2];
    symres_lcols_issue<NCT>(M, c.k0, c.rp, cmp0, l0);
    symres_lcols_issue<NCT>(M, c.k1, c.rp, cmp1, l1);
#pragma unroll
    for (uint32_t j = 0; j < n / 2; ++j) {
        r0[j] = r0_piece(j);
        r1[j] = r1_piece(j);
    }
    bool bad = symres_r_differs<NCT>(r0, l0, cmp0);
    bad |= symres_r_differs<NCT>(r1, l1, cmp1);
    return bad;
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
__device__ __forceinline__ void symres_stamp(void *ws, uint32_t wg_round, uint32_t idx)
{
    if (ws) (reinterpret_cast<unsigned long long *>(ws) + 1024)[wg_round * 8 + idx] = __builtin_amdgcn_s_memrealtime();
}
#define GBDPCG_RS_STAMP(IDX) \
    if (tid == 0 && rs_round < 8) symres_stamp(a.cluster_ws, blockIdx.x * 8 + rs_round, IDX);
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
    const SymResLds<NCT> lds(N);
    float *region = smem + (wave * G::GROUPS + (lane >> 3)) * G::REGION;  // this group's LDS region
    float4 *lt0 = reinterpret_cast<float4 *>(smem + lds.lt0) + tid;  // first pieces of this lane's Pinv k0 tile
    // Behind xa the pointers step through the list of SymResLds, in its order and with its sizes (the host's size rests on that),
    // written out as a chain and not as smem + offset: with the offsets summed as integers hipcc no longer folds the constant
    // part of four DS addresses of the iteration into the instruction, and the caller-asserted kernel took 338.6 us against the
    // parent's 335.6 .. 337.7 for 1024 x (14, 128) x 25 iterations; as a chain 336.1 (profiles/r20_resident_sym_split.txt).
    float *xa = smem + lds.xa, *xb = xa + lds.padded, *zs = xb + lds.padded;
    float *red0 = zs + lds.padded, *red1 = red0 + WAVES, *ls = red1 + WAVES;
    const uint32_t dump = (uint32_t)(uintptr_t)(ls + lds.vec);  // LDS byte address, for symres_touch
    uint32_t *vword = reinterpret_cast<uint32_t *>(ls + lds.vec) + SymResLds<NCT>::DUMP_BYTES / 4;

    const size_t mstride = (size_t)3 * n * n * N;

    // zs: only the rows of even block-rows >= 2 are ever written; row 0 (nothing above block-row 0) and the odd
    // rows (read, harmlessly, by the lanes that own no rows) must hold zeros for the whole launch
    for (uint32_t i = tid; i < lds.padded; i += G::THREADS) zs[i] = 0.f;
    __syncthreads();

    // which of this workgroup's problems this launch owns, 64 at a time (one memory round trip for all of them)
    unsigned long long takes = 0;
    uint32_t takes_from = 0;
#ifdef GBDPCG_RS_STAMPS
    uint32_t rs_round = 0xffffffffu;
#endif

    // Resident for the whole solve (SHARED: for the whole launch): three tiles in registers, the fourth in LDS.
    SymResTile<NCT> s0, s1, p0;

    if constexpr (SHARED) {
        // the one pair, once per workgroup: every problem below finds its tiles where a plain solve leaves them after its load
        // (edge blocks zeroed, the Pinv k1 tile over the wave's staging block, which nothing touches again)
#ifdef GBDPCG_RS_STAMPS
        const uint32_t rs_round = 0;
#endif
        float4_alias *ltw = reinterpret_cast<float4_alias *>(smem + wave * G::GROUPS * G::REGION) + lane;
        symres_load_tiles<NCT, STAGED>(a.S, a.Pinv, N, symres_lane<NCT>(lane, wave, N), region, ltw, lt0, s0, s1, p0,
                                       [&] { GBDPCG_RS_STAMP(1) });
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
        const SymResLane<NCT> c = symres_lane<NCT>(lane_o, wave, N);
        // the LDS-resident tile (Pinv k1) of this lane: piece i at ltw[64 i], inside the wave's own block of regions
        float4_alias *ltw = reinterpret_cast<float4_alias *>(smem + wave * G::GROUPS * G::REGION) + lane_o;
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
        if constexpr (!SHARED) symres_load_tiles<NCT, STAGED>(S, P, N, c, region, ltw, lt0, s0, s1, p0, [&] { GBDPCG_RS_STAMP(1) });
        GBDPCG_RS_STAMP(2)

        for (uint32_t i = tid; i < n; i += G::THREADS) {
            xa[i] = 0.f; xa[n + len + i] = 0.f; xa[2 * n + len + i] = 0.f;
            xb[i] = 0.f; xb[n + len + i] = 0.f; xb[2 * n + len + i] = 0.f;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of lambda and gamma has landed in LDS
        __syncthreads();
        GBDPCG_RS_STAMP(3)

        const bool live0 = c.live0, live1 = c.live1;
        float2 *xa0 = reinterpret_cast<float2 *>(xa + n + c.row0), *xa1 = reinterpret_cast<float2 *>(xa + n + c.row1);
        float2 *xb0 = reinterpret_cast<float2 *>(xb + n + c.row0), *xb1 = reinterpret_cast<float2 *>(xb + n + c.row1);
        float2 *ls0 = reinterpret_cast<float2 *>(ls + c.row0), *ls1 = reinterpret_cast<float2 *>(ls + c.row1);

        float y[2][2], part;
        // r = gamma - S lambda                                            (pcg.cuh:118-126)
        part = symres_product<NCT, 0, false>(s0, lt0, s1, ltw, xa, zs, c, lane, y);
        __syncthreads();
        const float2 z = *reinterpret_cast<const float2 *>(zs + c.zo0);   // (lanes without rows: zero since kernel start)
        y[0][0] += z.x;
        y[0][1] += z.y;
        if (live0) {   // gamma is waiting in the mirror of r
            const float2 gm = *xb0;
            *xb0 = make_float2(gm.x - y[0][0], gm.y - y[0][1]);
        }
        if (live1) {
            const float2 gm = *xb1;
            *xb1 = make_float2(gm.x - y[1][0], gm.y - y[1][1]);
        }
        __syncthreads();

        // r~ = Pinv r ; p = r~ ; eta = r.r~                               (pcg.cuh:130-149)
        part = symres_product<NCT, G::P0_LDS_QUADS, true>(p0, lt0, p0, ltw, xb, zs, c, lane, y);
        float eta = symres_sum_finish_y(part, red1, wave, lane, zs + c.zo0, y[0]);
        if (live0) *xa0 = make_float2(y[0][0], y[0][1]);
        if (live1) *xa1 = make_float2(y[1][0], y[1][1]);
        __syncthreads();

        // prefetch schedule for the next problem of this workgroup: two lines per thread and iteration
        // (SHARED: the next problem's matrices are the ones already here)
        const uint32_t nprob = prob + gridDim.x;
        const uint32_t pf_per_matrix = !SHARED && GBDPCG_RS_PREFETCH && nprob < a.batch
                                           ? (N * kSymResTouchSteps<NCT> + G::THREADS - 1) / G::THREADS : 0u;
        uint32_t pf = 0;
        auto prefetch_step = [&] {
            symres_touch<NCT>(a.S + nprob * mstride, N, pf * G::THREADS + tid, dump);
            symres_touch<NCT>(a.Pinv + nprob * mstride, N, pf * G::THREADS + tid, dump);
            ++pf;
        };

        uint32_t iter = 0;
        bool max_iter_exit = true;
        GBDPCG_RS_STAMP(4)
        for (; iter < a.max_iter; ++iter) {                               // pcg.cuh:154
            if (pf < pf_per_matrix) prefetch_step();
            // upsilon = S p ; alpha = eta / (p.upsilon)                   (pcg.cuh:156-169)
            part = symres_product<NCT, 0, false>(s0, lt0, s1, ltw, xa, zs, c, lane, y);
            // the lane's own entries of p, lambda, r: requested before the reduction, used after it
            const float2 pa0 = *xa0, pa1 = *xa1, la0 = *ls0, la1 = *ls1, ra0 = *xb0, ra1 = *xb1;
            const float den = symres_sum_finish_y(part, red0, wave, lane, zs + c.zo0, y[0]);
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
            part = symres_product<NCT, G::P0_LDS_QUADS, true>(p0, lt0, p0, ltw, xb, zs, c, lane, y);
            const float2 pb0 = *xa0, pb1 = *xa1;
            const float eta_new = symres_sum_finish_y(part, red1, wave, lane, zs + c.zo0, y[0]);
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

        GBDPCG_RS_STAMP(5)
        if constexpr (VERIFY) {
            // L_{k+1} == R_k^T for both matrices and both of the lane's block-rows against the R halves of the tiles, S then
            // Pinv (all four sets of pieces in flight at once spill).  The Pinv k1 tile is compared from LDS.
            const bool cmp0 = live0 && c.k0 + 1 < N, cmp1 = live1 && c.k1 + 1 < N;
            bool bad = symres_rows_differ<NCT>(S, c, cmp0, cmp1, [&](uint32_t j) { return s0.q[n / 2 + j]; },
                                               [&](uint32_t j) { return s1.q[n / 2 + j]; });
            __builtin_amdgcn_sched_barrier(0);
            bad |= symres_rows_differ<NCT>(P, c, cmp0, cmp1, [&](uint32_t j) { return p0.q[n / 2 + j]; },
                                           [&](uint32_t j) -> float4 { return ltw[(n / 2 + j) * 64]; });
            if (bad) *vword = 0u;   // (every writer writes the same value)
        }
        while (pf < pf_per_matrix) prefetch_step();  // short solves: the rest of the prefetch

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

static bool resident_sym_aligned(const void *S, const void *Pinv, uintptr_t bytes)
{
    return !((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(Pinv)) % bytes);
}

static bool resident_sym_staged(const void *S, const void *Pinv)
{
    // coalesced 16-byte tile loads need 16-byte aligned matrices (every hipMalloc'ed buffer is)
    static const bool no_staging = getenv("GBDPCG_RS_DIRECT_LOADS") != nullptr;  // tuning runs only
    return !no_staging && resident_sym_aligned(S, Pinv, 16);
}

// The instantiation for a launch.  The verifying kernel exists staged and per-problem only (the launcher has checked both).
static auto resident_sym_kernel(bool staged, bool verify, bool shared) -> void (*)(PcgArgs<float>)
{
    if (verify) return pcg_resident_sym_kernel<14, true, true>;
    if (shared) return staged ? pcg_resident_sym_kernel<14, true, false, true> : pcg_resident_sym_kernel<14, false, false, true>;
    return staged ? pcg_resident_sym_kernel<14, true, false> : pcg_resident_sym_kernel<14, false, false>;
}

template <typename T>
bool resident_sym_verifies(const DeviceInfo &dev, uint32_t n, uint32_t N, const T *S, const T *Pinv)
{
    return sizeof(T) == 4 && S && Pinv && resident_sym_shape<T>(n, N) && resident_sym_staged(S, Pinv) &&
           SymResLds<14>(N).bytes(true) <= dev.lds_per_wg_max;
}

// verify: the verifying kernel (every problem, a.verdict_out written); the caller has checked resident_sym_verifies.
template <typename T>
static bool launch_pcg_resident_sym_impl(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool verify,
                                         bool shared = false)
{
    if constexpr (sizeof(T) == 4) {
        if (!a.symmetric || !a.Pinv || !resident_sym_shape<T>(a.n, a.N)) return false;
        if (!resident_sym_aligned(a.S, a.Pinv, 8)) return false;
        const size_t lds = SymResLds<14>(a.N).bytes(verify);
        if (lds > dev.lds_per_wg_max) return false;
        const bool staged = resident_sym_staged(a.S, a.Pinv);
        if (verify && (!staged || !a.verdict_out)) return false;
        if (verify && shared) return false;   // a shared pair has ONE verdict, found before the launch
        const auto kern = resident_sym_kernel(staged, verify, shared);
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
