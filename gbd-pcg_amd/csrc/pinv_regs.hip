// pinv_regs.hip -- Phi^-1 formation in two passes for the compile-time block sizes (GBDPCG_PINV_N): pass 1 inverts D_k with the
// block in REGISTERS, one column per lane (four forms, by how many knots share a wavefront), pass 2 (STAIR only) builds the
// off-diagonal slots from the D slots pass 1 wrote.  pinv.hip holds the route that picks a family; launch_pinv_regs starts it.
#include "pinv_common.hpp"

namespace gbdpcg {

// ---- n <= 32: the [D | I] tableau lives in REGISTERS, one column per lane ----
// Lane c < 2n owns tableau column c (n values).  Pivot step j needs column j (held by lane j) in every
// lane: n v_readlane broadcasts into scalars, then n FMAs per lane -- no LDS, no barrier, the pivot loop
// fully unrolled so every register index is static.  Same arithmetic, element for element, as the LDS
// kernel (pinv_diag_kernel).  One wavefront per knot, four knots per workgroup.
template <typename T, int NCT>
__global__ __launch_bounds__(kPinvThreads) void pinv_diag_reg_kernel(uint32_t N, uint64_t knots, const T *__restrict__ S,
                                                                    T *__restrict__ Pinv, int kind)
{
    constexpr uint32_t n = NCT, nn = n * n;
    __shared__ T stage_all[4][nn];  // D_k^-1 of each wave's knot, for the mirrored write-out
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t knot = (uint64_t)blockIdx.x * 4 + wave;
    if (knot >= knots) return;
    T *stage = stage_all[wave];
    const size_t blk = (size_t)knot * 3 * nn;
    const T *D = S + blk + nn;
    T *out = Pinv + blk;

    T col[n];
#pragma unroll
    for (uint32_t r = 0; r < n; ++r) {
        if (lane < n) col[r] = (kind == 0) ? (r == lane ? T(1) : T(0)) : D[lane * n + r];
        else col[r] = (lane - n == r) ? T(1) : T(0);
    }
    if (kind != 0) {
#pragma unroll
        for (uint32_t j = 0; j < n; ++j) {
            T cj[n];
#pragma unroll
            for (uint32_t r = 0; r < n; ++r) cj[r] = lane_bcast(col[r], (int)j);
            tableau_pivot_step<n>(col, cj, j);
        }
    }
    // lanes n .. 2n-1 hold the columns of D_k^-1; mirror the upper triangle (see the LDS kernel) on the way out
    if (lane >= n && lane < 2 * n) {
#pragma unroll
        for (uint32_t r = 0; r < n; ++r) stage[(lane - n) * n + r] = col[r];
    }
    group_sync<64>();
    // (The mirrored write-out is spelled out in the reg, pair and wide kernels; the quad kernel has its whole-wave form.  As one
    // shared helper it changed the store addressing of four instantiations, and n = 20 in fp32 then measured 2 % slower:
    // profiles/r16_pinv_split.txt.)
    for (uint32_t i = lane; i < nn; i += 64) {
        const uint32_t c = i / n, r = i - c * n;
        out[nn + i] = r <= c ? stage[c * n + r] : stage[r * n + c];
        // the stair pass overwrites every off-diagonal slot except the two never-read corner blocks
        const uint32_t kk = (uint32_t)(knot % N);
        if (kind != 2 || kk == 0) out[i] = T(0);
        if (kind != 2 || kk == N - 1) out[2 * nn + i] = T(0);
    }
}

// 2n <= 32: TWO knots per wavefront, one in each 32-lane half (lane c < 2n of a half owns tableau column c), so
// 28 + 28 of 64 lanes work instead of 28.  A pivot step needs column j of the half's own knot in every lane
// of that half, which v_readlane cannot give (one scalar per wave): lane j parks its column in LDS and the
// half reads it back as broadcast 16-byte reads -- 8 LDS instructions per step instead of 14 readlanes per
// knot, and a third of the VALU instructions per knot.  Same arithmetic, element for element.
template <typename T, int NCT>
__global__ __launch_bounds__(kPinvThreads) void pinv_diag_pair_kernel(uint32_t N, uint64_t knots, const T *__restrict__ S,
                                                                     T *__restrict__ Pinv, int kind)
{
    constexpr uint32_t n = NCT, nn = n * n, NP = (n + 3) / 4 * 4;  // column padded to whole 16-byte pieces (fp32)
    static_assert(2 * n <= 32, "two knots per wave need 2n lanes per half");
    __shared__ __attribute__((aligned(16))) T stage_all[4][2][nn];  // D_k^-1 of each half's knot, for the mirrored write-out
    __shared__ __attribute__((aligned(16))) T bcast_all[4][2][NP];  // the pivot column of the current step
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, half = lane >> 5, l = lane & 31u;
    const uint64_t knot = ((uint64_t)blockIdx.x * 4 + wave) * 2 + half;
    const bool alive = knot < knots;
    T *stage = stage_all[wave][half];
    T *bc = bcast_all[wave][half];
    const size_t blk = (size_t)(alive ? knot : 0) * 3 * nn;
    const T *D = S + blk + nn;
    T *out = Pinv + blk;

    T col[n];
#pragma unroll
    for (uint32_t r = 0; r < n; ++r) {
        if (l < n) col[r] = (kind == 0 || !alive) ? (r == l ? T(1) : T(0)) : D[l * n + r];
        else col[r] = (l - n == r) ? T(1) : T(0);
    }
    if (kind != 0) {
#pragma unroll
        for (uint32_t j = 0; j < n; ++j) {
            if (l == j) {
#pragma unroll
                for (uint32_t r = 0; r < n; ++r) bc[r] = col[r];
            }
            group_sync<64>();
            T cj[n];
#pragma unroll
            for (uint32_t r = 0; r < n; ++r) cj[r] = bc[r];
            group_sync<64>();  // everyone has the column before step j+1 overwrites it
            tableau_pivot_step<n>(col, cj, j);
        }
    }
    // lanes n .. 2n-1 of a half hold the columns of D_k^-1; mirror the upper triangle on the way out
    if (l >= n && l < 2 * n) {
#pragma unroll
        for (uint32_t r = 0; r < n; ++r) stage[(l - n) * n + r] = col[r];
    }
    group_sync<64>();
    if (alive) {
        const uint32_t kk = (uint32_t)(knot % N);
        for (uint32_t i = l; i < nn; i += 32) {
            const uint32_t c = i / n, r = i - c * n;
            out[nn + i] = r <= c ? stage[c * n + r] : stage[r * n + c];
            // the stair pass overwrites every off-diagonal slot except the two never-read corner blocks
            if (kind != 2 || kk == 0) out[i] = T(0);
            if (kind != 2 || kk == N - 1) out[2 * nn + i] = T(0);
        }
    }
}

// n <= 16: FOUR knots per wavefront, one per 16-lane quarter, with the IN-PLACE form of the same
// elimination: lane c < n of a quarter owns column c of the n x n block only.  The identity half of the
// [D | I] tableau is never stored: its column j stays the unit vector e_j until pivot step j (its pivot-row
// entries are zero up to then) and is created in that step in the place of column j of D, whose pivot-step
// update would only produce e_j.  So lane j computes (r == j ? piv : fma(-cj[r], piv, 0)) -- exactly what
// the tableau lane n+j computes from e_j -- and every other lane the usual update: the same floating-point
// operations on the same numbers as the tableau kernels, with 56 of 64 lanes busy instead of 28.
template <typename T, int NCT>
__global__ __launch_bounds__(kPinvThreads) void pinv_diag_quad_kernel(uint32_t N, uint64_t knots, const T *__restrict__ S,
                                                                     T *__restrict__ Pinv, int kind)
{
    constexpr uint32_t n = NCT, nn = n * n;
    static_assert(n <= 16, "four knots per wave need n lanes per quarter");
    __shared__ __attribute__((aligned(16))) T stage_all[4][4][nn];  // D_k^-1 of each quarter's knot, for the mirrored write-out
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, quarter = lane >> 4, l = lane & 15u;
    const uint64_t knot = ((uint64_t)blockIdx.x * 4 + wave) * 4 + quarter;
    const bool alive = knot < knots;
    T *stage = stage_all[wave][quarter];
    const size_t blk = (size_t)(alive ? knot : 0) * 3 * nn;
    const T *D = S + blk + nn;
    const bool owner = l < n;

    T col[n];
#pragma unroll
    for (uint32_t r = 0; r < n; ++r) col[r] = (kind == 0 || !alive || !owner) ? (r == l ? T(1) : T(0)) : D[l * n + r];
    if (kind != 0) stair_invert<(int)n>(col, l);   // (the pivot column reaches the quarter as a DPP row broadcast)
    if (owner) {
#pragma unroll
        for (uint32_t r = 0; r < n; ++r) stage[l * n + r] = col[r];
    }
    group_sync<64>();
    // write-out by the whole wave: its four knots are consecutive in memory, so the D slots (and, for the
    // identity / block-Jacobi kinds, the zeroed L and R slots) go out as dense 256-byte stores
    const uint64_t knot0 = ((uint64_t)blockIdx.x * 4 + wave) * 4;
    T *out0 = Pinv + (size_t)knot0 * 3 * nn;
    for (uint32_t e = lane; e < 4 * nn; e += 64) {
        const uint32_t q = e / nn, i = e - q * nn;
        if (knot0 + q >= knots) break;
        const uint32_t c = i / n, r = i - c * n;
        const T *st = stage_all[wave][q];
        T *o = out0 + (size_t)q * 3 * nn;
        o[nn + i] = r <= c ? st[c * n + r] : st[r * n + c];  // mirror the upper triangle: exactly symmetric
        // the stair pass overwrites every off-diagonal slot except the two never-read corner blocks
        const uint32_t kk = (uint32_t)((knot0 + q) % N);
        if (kind != 2 || kk == 0) o[i] = T(0);
        if (kind != 2 || kk == N - 1) o[2 * nn + i] = T(0);
    }
}

// 32 < n <= 64 (BASELINE config 4: n = 36, fp64): ONE knot per wavefront, lane c < n owns column c, the same
// in-place elimination as pinv_diag_quad_kernel (the [D | I] tableau kernels need 2n <= 64 lanes, and the
// LDS form that used to take these sizes spends a workgroup barrier pair per pivot step: 107 us for the 256
// knots of config 4 against a few us here).  The pivot column is broadcast with v_readlane (n scalars per
// step, no LDS, no barrier); the finished inverse is staged in LDS for the mirrored, dense write-out.
template <typename T, int NCT>
__global__ __launch_bounds__(kPinvThreads) void pinv_diag_wide_kernel(uint32_t N, uint64_t knots, const T *__restrict__ S,
                                                                     T *__restrict__ Pinv, int kind)
{
    constexpr uint32_t n = NCT, nn = n * n;
    static_assert(n > 32 && n <= 64, "one column per lane");
    __shared__ __attribute__((aligned(16))) T stage_all[4][nn];
    const uint32_t wave = threadIdx.x >> 6, l = threadIdx.x & 63u;
    const uint64_t knot = (uint64_t)blockIdx.x * 4 + wave;
    const bool alive = knot < knots;  // wave-uniform; dead waves still run the (cheap, branch-free) loop
    T *stage = stage_all[wave];
    const size_t blk = (size_t)(alive ? knot : 0) * 3 * nn;
    const T *D = S + blk + nn;
    const bool owner = l < n;

    T col[n];
#pragma unroll
    for (uint32_t r = 0; r < n; ++r) col[r] = (kind == 0 || !alive || !owner) ? (r == l ? T(1) : T(0)) : D[(owner ? l : 0u) * n + r];
    if (kind != 0) {
#pragma unroll
        for (uint32_t j = 0; j < n; ++j) {  // fully unrolled: every register index is static
            T cj[n];                        // column j, broadcast from lane j into scalars
#pragma unroll
            for (uint32_t r = 0; r < n; ++r) cj[r] = lane_bcast(col[r], (int)j);
            const T piv = T(1) / cj[j];
            const bool is_j = l == j;
            const T pr = is_j ? piv : col[j] * piv;  // scaled pivot-row entry of this lane's column
#pragma unroll
            for (uint32_t r = 0; r < n; ++r) col[r] = (r == j) ? pr : fma_t(-cj[r], pr, is_j ? T(0) : col[r]);
        }
    }
    if (owner) {
#pragma unroll
        for (uint32_t r = 0; r < n; ++r) stage[l * n + r] = col[r];
    }
    group_sync<64>();
    if (!alive) return;
    T *o = Pinv + (size_t)knot * 3 * nn;
    const uint32_t kk = (uint32_t)(knot % N);
    for (uint32_t i = l; i < nn; i += 64) {
        const uint32_t c = i / n, r = i - c * n;
        o[nn + i] = r <= c ? stage[c * n + r] : stage[r * n + c];  // mirror the upper triangle: exactly symmetric
        // the stair pass overwrites every off-diagonal slot except the two never-read corner blocks
        if (kind != 2 || kk == 0) o[i] = T(0);
        if (kind != 2 || kk == N - 1) o[2 * nn + i] = T(0);
    }
}

// Stair off-diagonal slots: one wavefront per knot PAIR (k, k+1), every inner product
// reads BOTH operands as contiguous pairs from LDS.  The wave of knot k produces the right slot of k,
// R'_k = -D_k^-1 R_k D_{k+1}^-1, and the left slot of k+1, L'_{k+1} = -D_{k+1}^-1 L_{k+1} D_k^-1, evaluated as
// the transpose of the same operation sequence with L_{k+1}^T in the place of R_k.  When S is symmetric in
// storage (L_{k+1} == R_k^T bit for bit, tested here by the wave) the second evaluation would repeat the
// first one operation for operation, so its result is written as the mirror image of the first: half the
// work, and Pinv comes out exactly symmetric whenever S is.  D^-1 blocks are exactly symmetric (mirrored by
// pass 1), so row r of the first factor is its column r; the intermediate W = A*B is stored transposed for the
// same reason.  Operation order is the LDS kernel's ((A*B)*C, q ascending), so both produce the same bits.
template <typename T, int NCT>
__global__ __launch_bounds__(kPinvThreads) void pinv_stair_reg_kernel(uint32_t N, uint64_t knots, const T *__restrict__ S,
                                                                     T *Pinv)
{
    constexpr uint32_t n = NCT, nn = n * n;
    using P2 = typename VecOf<T, 2>::type;
    __shared__ __attribute__((aligned(16))) T lds[4][4 * nn];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t knot = (uint64_t)blockIdx.x * 4 + wave;
    if (knot >= knots) return;
    T *A = lds[wave], *B = A + nn, *C = B + nn, *Wt = C + nn;
    const uint32_t k = (uint32_t)(knot % N);
    if (k == N - 1) return;  // the last knot of a problem has no right neighbour (wave-uniform)
    const size_t blk = (size_t)knot * 3 * nn, nb = blk + (size_t)3 * nn;

    constexpr uint32_t EPL = (nn + 63) / 64;  // elements per lane
    T lt[EPL];                                // L_{k+1}^T, element for element against R_k
    bool differs = false;
#pragma unroll
    for (uint32_t j = 0; j < EPL; ++j) {
        const uint32_t i = lane + 64 * j;
        if (i < nn) {
            const uint32_t c = i / n, r = i - c * n;
            const T rk = S[blk + 2 * (size_t)nn + i];  // R_k(r,c)
            lt[j] = S[nb + (size_t)r * n + c];         // L_{k+1}(c,r)
            differs |= pinv_bits(rk) != pinv_bits(lt[j]);
            A[i] = Pinv[blk + nn + i];                 // D_k^-1
            B[i] = rk;
            C[i] = Pinv[nb + nn + i];                  // D_{k+1}^-1
        }
    }
    const bool symmetric = __builtin_amdgcn_ballot_w64(differs) == 0;  // wave-uniform
    group_sync<64>();
    for (int pass = 0; pass < (symmetric ? 1 : 2); ++pass) {
        if (pass == 1) {  // general S: the left slot of k+1 from its own data
#pragma unroll
            for (uint32_t j = 0; j < EPL; ++j) {
                const uint32_t i = lane + 64 * j;
                if (i < nn) B[i] = lt[j];
            }
            group_sync<64>();
        }
        if constexpr (n % 2 == 0 && (n / 2) * (n / 2) <= 64) {
            // 2 x 2 output tiles, one per lane ((n/2)^2 lanes): the one-element form below is bound by LDS bandwidth
            constexpr uint32_t H = n / 2;
            const uint32_t tr = lane / H, tc = lane - tr * H, r0 = 2 * tr, c0 = 2 * tc;
            const bool tile = lane < H * H;
            if (tile) {
                T w00, w01, w10, w11;
                tile_product<H>(A + r0 * n, A + (r0 + 1) * n, B + c0 * n, B + (c0 + 1) * n, w00, w01, w10, w11);
                Wt[r0 * n + c0] = w00; Wt[r0 * n + c0 + 1] = w01;            // transposed: row r of W contiguous
                Wt[(r0 + 1) * n + c0] = w10; Wt[(r0 + 1) * n + c0 + 1] = w11;
            }
            group_sync<64>();
            if (tile) {
                T x00, x01, x10, x11;
                tile_product<H>(Wt + r0 * n, Wt + (r0 + 1) * n, C + c0 * n, C + (c0 + 1) * n, x00, x01, x10, x11);
                if (pass == 0) {  // R'_k(r,c) at column-major c*n + r
                    T *Rp = Pinv + blk + 2 * (size_t)nn;
                    Rp[c0 * n + r0] = -x00; Rp[c0 * n + r0 + 1] = -x10;
                    Rp[(c0 + 1) * n + r0] = -x01; Rp[(c0 + 1) * n + r0 + 1] = -x11;
                }
                if (pass == 1 || symmetric) {  // L'_{k+1}(c,r) = X(r,c) at column-major r*n + c
                    T *Lp = Pinv + nb;
                    Lp[r0 * n + c0] = -x00; Lp[r0 * n + c0 + 1] = -x01;
                    Lp[(r0 + 1) * n + c0] = -x10; Lp[(r0 + 1) * n + c0 + 1] = -x11;
                }
            }
        } else {
            for (uint32_t i = lane; i < nn; i += 64) {
                const uint32_t c = i / n, r = i - c * n;
                // W(r,c) = sum_q A(r,q) B(q,c);  A symmetric: A(r,q) = A(q,r) = A[r*n + q]
                T acc = T(0);
                if constexpr (n % 2 == 0) {
                    const P2 *ar = reinterpret_cast<const P2 *>(A + r * n), *bc = reinterpret_cast<const P2 *>(B + c * n);
#pragma unroll
                    for (uint32_t q = 0; q < n / 2; ++q) {
                        const P2 a2 = ar[q], b2 = bc[q];
                        acc = fma_t(a2.x, b2.x, acc);
                        acc = fma_t(a2.y, b2.y, acc);
                    }
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < n; ++q) acc = fma_t(A[r * n + q], B[c * n + q], acc);
                }
                Wt[r * n + c] = acc;  // transposed: row r of W contiguous
            }
            group_sync<64>();
            for (uint32_t i = lane; i < nn; i += 64) {
                const uint32_t c = i / n, r = i - c * n;
                T acc = T(0);
                if constexpr (n % 2 == 0) {
                    const P2 *wr = reinterpret_cast<const P2 *>(Wt + r * n), *cc = reinterpret_cast<const P2 *>(C + c * n);
#pragma unroll
                    for (uint32_t q = 0; q < n / 2; ++q) {
                        const P2 w2 = wr[q], c2 = cc[q];
                        acc = fma_t(w2.x, c2.x, acc);
                        acc = fma_t(w2.y, c2.y, acc);
                    }
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < n; ++q) acc = fma_t(Wt[r * n + q], C[c * n + q], acc);
                }
                if (pass == 0) Pinv[blk + 2 * (size_t)nn + i] = -acc;                 // R'_k(r,c)
                if (pass == 1 || symmetric) Pinv[nb + (size_t)r * n + c] = -acc;      // L'_{k+1}(c,r) = X(r,c)
            }
        }
        group_sync<64>();
    }
}

// Stair slots for 32 < n <= 64 (even n; BASELINE config 4): one WORKGROUP per knot pair (k, k+1).  The same
// operation sequence as the wave-per-pair kernels -- W = D_k^-1 R_k with 2 x 2 register tiles, X = W D_{k+1}^-1,
// R'_k = -X, and L'_{k+1} = -X^T written as the mirror image when the workgroup finds L_{k+1} == R_k^T in S (else a
// second pass on L_{k+1}^T) -- with the (n/2)^2 tiles dealt over 256 threads and the factors staged in LDS.  The
// runtime-n kernel this replaces evaluates every pair twice (once from each side), with scalar inner loops.
template <typename T, int NCT>
__global__ __launch_bounds__(kPinvThreads) void pinv_stair_wide_kernel(uint32_t N, const T *__restrict__ S, T *__restrict__ Pinv)
{
    constexpr uint32_t n = NCT, nn = n * n, H = n / 2, TILES = H * H;
    static_assert(n > 32 && n <= 64 && n % 2 == 0 && 4 * nn * sizeof(T) <= 64 * 1024, "four n x n factors in static LDS");
    __shared__ __attribute__((aligned(16))) T A[nn], B[nn], C[nn], Wt[nn];
    const uint32_t pairs_per_problem = N - 1;
    const uint32_t prob = blockIdx.x / pairs_per_problem, k = blockIdx.x - prob * pairs_per_problem;
    const size_t blk = ((size_t)prob * N + k) * 3 * nn, nb = blk + (size_t)3 * nn;
    constexpr uint32_t EPL = (nn + kPinvThreads - 1) / kPinvThreads;
    T lt[EPL];
    bool differs = false;
#pragma unroll
    for (uint32_t q = 0; q < EPL; ++q) {
        const uint32_t i = threadIdx.x + kPinvThreads * q;
        if (i < nn) {
            const uint32_t c = i / n, r = i - c * n;
            const T rk = S[blk + 2 * (size_t)nn + i];   // R_k(r,c)
            lt[q] = S[nb + (size_t)r * n + c];          // L_{k+1}(c,r)
            differs |= pinv_bits(rk) != pinv_bits(lt[q]);
            B[i] = rk;
            A[i] = Pinv[blk + nn + i];                  // D_k^-1 (mirrored by the diagonal pass: exactly symmetric)
            C[i] = Pinv[nb + nn + i];                   // D_{k+1}^-1
        }
    }
    const bool symmetric = __syncthreads_or(differs ? 1 : 0) == 0;  // also the barrier after the staging stores
    for (int pass = 0; pass < (symmetric ? 1 : 2); ++pass) {
        if (pass == 1) {
#pragma unroll
            for (uint32_t q = 0; q < EPL; ++q) {
                const uint32_t i = threadIdx.x + kPinvThreads * q;
                if (i < nn) B[i] = lt[q];
            }
            __syncthreads();
        }
        for (uint32_t t = threadIdx.x; t < TILES; t += kPinvThreads) {
            const uint32_t tr = t / H, tc = t - tr * H, r0 = 2 * tr, c0 = 2 * tc;
            T w00, w01, w10, w11;
            tile_product<H>(A + r0 * n, A + (r0 + 1) * n, B + c0 * n, B + (c0 + 1) * n, w00, w01, w10, w11);
            Wt[r0 * n + c0] = w00; Wt[r0 * n + c0 + 1] = w01;
            Wt[(r0 + 1) * n + c0] = w10; Wt[(r0 + 1) * n + c0 + 1] = w11;
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < TILES; t += kPinvThreads) {
            const uint32_t tr = t / H, tc = t - tr * H, r0 = 2 * tr, c0 = 2 * tc;
            T x00, x01, x10, x11;
            tile_product<H>(Wt + r0 * n, Wt + (r0 + 1) * n, C + c0 * n, C + (c0 + 1) * n, x00, x01, x10, x11);
            if (pass == 0) {
                T *Rp = Pinv + blk + 2 * (size_t)nn;
                Rp[c0 * n + r0] = -x00; Rp[c0 * n + r0 + 1] = -x10;
                Rp[(c0 + 1) * n + r0] = -x01; Rp[(c0 + 1) * n + r0 + 1] = -x11;
            }
            if (pass == 1 || symmetric) {
                T *Lp = Pinv + nb;
                Lp[r0 * n + c0] = -x00; Lp[r0 * n + c0 + 1] = -x01;
                Lp[(r0 + 1) * n + c0] = -x10; Lp[(r0 + 1) * n + c0 + 1] = -x11;
            }
        }
        __syncthreads();
    }
}

// Pass 1 by the family's diagonal kernel, then (STAIR) the stair kernel of that block size.  Refused: a pass of more than
// 0x7fffffff workgroups.
template <typename T>
hipError_t launch_pinv_regs(PinvFamily family, uint32_t n, uint32_t N, uint32_t batch, const T *S, T *Pinv, int kind, hipStream_t s)
{
    const uint64_t knots = (uint64_t)N * batch, blocks = (knots + 3) / 4;  // one wavefront per knot, or per knot pair (k, k+1)
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 threads(kPinvThreads);
    return pinv_dispatch_n(n, hipErrorInvalidValue, [&](auto nct) {
        constexpr int NN = decltype(nct)::value;
        if constexpr (2 * NN <= 64) {
            if constexpr (2 * NN > 32)
                hipLaunchKernelGGL((pinv_diag_reg_kernel<T, NN>), dim3((uint32_t)blocks), threads, 0, s, N, knots, S, Pinv, kind);
            else if (family == PinvFamily::quad)
                hipLaunchKernelGGL((pinv_diag_quad_kernel<T, NN>), dim3((uint32_t)((knots + 15) / 16)), threads, 0, s, N, knots, S, Pinv, kind);
            else
                hipLaunchKernelGGL((pinv_diag_pair_kernel<T, NN>), dim3((uint32_t)((knots + 7) / 8)), threads, 0, s, N, knots, S, Pinv, kind);
            if (kind != 2) return hipGetLastError();
            hipLaunchKernelGGL((pinv_stair_reg_kernel<T, NN>), dim3((uint32_t)blocks), threads, 0, s, N, knots, S, Pinv);
        } else {
            static_assert(NN <= 64 && NN % 2 == 0 && 4 * NN * NN * sizeof(T) <= 64 * 1024,
                          "every listed n above 32 takes pinv_diag_wide_kernel + pinv_stair_wide_kernel: one column per lane, even n, "
                          "four factors in 64 KiB of static LDS.  For a size that fails this, keep the diagonal kernel (n <= 64) and "
                          "give the stair pass to pinv_stair_kernel<T, 256> with the LDS check of launch_form_pinv_g");
            hipLaunchKernelGGL((pinv_diag_wide_kernel<T, NN>), dim3((uint32_t)blocks), threads, 0, s, N, knots, S, Pinv, kind);
            if (kind != 2 || N < 2) return hipGetLastError();
            if ((uint64_t)(N - 1) * batch > 0x7fffffffull) return hipErrorInvalidValue;
            hipLaunchKernelGGL((pinv_stair_wide_kernel<T, NN>), dim3((N - 1) * batch), threads, 0, s, N, S, Pinv);
        }
        return hipGetLastError();
    });
}

template hipError_t launch_pinv_regs<float>(PinvFamily, uint32_t, uint32_t, uint32_t, const float *, float *, int, hipStream_t);
template hipError_t launch_pinv_regs<double>(PinvFamily, uint32_t, uint32_t, uint32_t, const double *, double *, int, hipStream_t);

}  // namespace gbdpcg
