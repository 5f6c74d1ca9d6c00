// admm_optimality.hip -- the optimality test of the ADMM families (gbdpcg_admm_optimality_*, gbdpcg_admm_lin_optimality_* and their
// _shared twins): is (z, lambda, rho y) a solution of  min 1/2 z'Gz + g'z  subject to  Cz = c,  E z in the rows' set ?  Every update of
// every family (box, soft box, linear rows, soft rows, cones) writes w+ = P(s) and y+ = s - w+ with P the projection or prox of its
// set, so w lies in the set and rho y in the normal cone at w BY CONSTRUCTION: bounds, complementarity and the multipliers' signs need
// no test, and no bound or kappa is read here.  What is left is stationarity WITH the row multiplier, G z + g + C'lambda + rho E'y,
// the dynamics C z - c, and consensus E z - w -- each with the scale an OSQP-style test r <= eps_abs + eps_rel scale wants.  G is the
// HESSIAN (not Ginv, not Gt = G + rho E'E): the test does not assume that the z-step was solved exactly.  The packed layouts are
// those of schur_residual.hip (G, C, g, c, z, lambda) and admm_rows.hip (E, the rows).
// A CHAIN is acc = seed; acc = fma(a_i, b_i, acc) in ascending i; every line below is ONE IEEE operation or a comparison
// (ieee_once.hpp), so every output is defined to the bit whatever the launch shape:
//   x-entry r of knot k:   s = g + lambda_k[r];  s = fma(Q_k(r,q), x_q, s), q < nx;  if k + 1 < N: s = fma(A_k(q,r), -lambda_{k+1}[q], s)
//                          (the chain of schur_residual.hip);  a = the Q chain from +0;  t = lambda_k[r], then the A' chain
//   u-entry r of knot k:   the same with R_k, B_k and the seeds s = g, a = +0, t = +0   (the last knot has no C' terms and no u)
//   u = chain over the rows i of the entry's block of E(i,r) y_i, seed +0;      q = fma(rho_b, u, s);   p = fma(rho_b, u, t)
//   knot 0, entry r:       f = x_0[r] - c_0[r];  h = x_0[r]
//   knot k+1, entry r:     f = x_{k+1}[r] - c_{k+1}[r];  f = fma(A_k(r,q), -x_q, f), q < nx;  f = fma(B_k(r,q), -u_q, f), q < nu
//                          (the chain of schur_residual.hip);  h = the same chain seeded x_{k+1}[r]
//   row r:                 v_r = chain over the columns j of E(r,j) z_j, seed +0 (the chain of rows_update);  d_r = v_r - w_r
//   opt[6b..] = r_s = max |q|,  r_e = max |f|,  r_r = max |d|,  n_s = max(|a|, |p|, |g|),  n_e = max(|h|, |c|),  n_r = max(|v|, |w|)
//               (norm_fold.hpp: maxima over bit patterns, NaN on top, exact in any order)
//   done[b]   = (r_s <= fma(eps_rel, n_s, eps_abs) && r_e <= fma(eps_rel, n_e, eps_abs) && r_r <= fma(eps_rel, n_r, eps_abs)) ? 1 : 0
//               a NaN anywhere fails a comparison: 0
// BOX (the gbdpcg_admm_optimality_* calls): the rows are the entries of z, u = fma(1, y_r, +0) as in admm_infeas.hip and v_r = z_r:
// for finite data the bits of the rows launch with E = I, mx = nx, mu = nu (the zero entries of I add +-0 to a chain, and the sign of
// a zero does not reach a magnitude).
// So with y = 0, r_s and r_e are the pair of gbdpcg_kkt_residual_* (u = +-0 leaves s), and behind an update r_r is its res[2b]
// (v - w+ with the update's v chain; cone rows with a zero offset f, the call knows of no offset).
//
// admm_optimality_kernel<T, BOX>: ONE WORKGROUP PER PROBLEM, 64-bit problem strides, nothing crosses a workgroup: no atomics, no
// memset, no scratch, nothing read from opt or done.  The shape of admm_infeas_kernel: the horizon is walked in chunks of `kch` knots,
// as many as fit 4096 staged elements (16 KiB in fp32, 32 KiB in fp64: 8 resp. 5 workgroups of 256 lanes per compute unit).  Per chunk:
//   STAGE   Q_k, R_k (one contiguous range of G), [A_k | B_k], the E blocks, y, and -- because the entries behind the chunk are
//           contiguous with it -- z of the chunk plus x of the knot behind it, lambda of the chunk plus that of the knot behind it.
//           g, c and w are NOT staged: each element is used by the one lane that owns its entry, which reads it from memory at
//           consecutive addresses across lanes; a trip through LDS would only shorten the chunks.                         barrier
//   S       lanes own ENTRIES of z: the three chains s, a, t in one pass over the staged blocks, the E' chain, q and p.
//   D       lanes own ENTRIES of lambda: knot kk of the chunk evaluates the dynamics INTO knot kk + 1 (A_kk, B_kk, x_kk, u_kk serve
//           it, as a row of schur_residual.hip does), so no block of the knot before the chunk is needed; knot 0's line is the first
//           chunk's.
//   R       lanes own ROWS: the v chain, d.                 (no barrier between S, D and R: all three only read the staging)  barrier
// Six running maxima per lane, folded per wave through DPP (wave_umax), per workgroup through six LDS words per wave; lane 0 writes
// the six numbers and the flag.  Every global access is a scalar one at consecutive addresses across lanes, so the alignment of
// the base pointers plays no part.  In S consecutive lanes read columns of A_k and E, a stride of nx / mx elements: the bank
// conflict phase Q of admm_infeas_kernel has.  Global traffic per problem: everything gbdpcg_kkt_residual_* reads, plus E, w, y.
// Measured next to that launch (profiles/r26_admm_optimality.txt): 1.135 x its bytes in 3.6 x (fp32) and 2.8 x (fp64) its time -- the
// staged any-size form against its register kernel, 22 chunks of 6 knots at (14, 7, 128) with at most half the lanes busy; DESIGN.md
// section 3 says what would close it.
#include "ieee_once.hpp"
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

constexpr uint32_t kOptStage = 4096;         // elements staged per chunk, unless one knot needs more
constexpr uint32_t kOptMaxKnots = 64;        // knots per chunk at most
constexpr size_t kOptLdsBytes = 60 * 1024;   // what one knot may take at the outside (64 KB less the norm slots and slack)

struct OptShape {
    uint32_t nx, nu, mx, mu, N;
    uint32_t kch;      // knots per chunk
    uint32_t shared;   // G, C and E are one problem's
};

// what one knot takes of the staging: Q_k, R_k, [A_k | B_k], its E blocks, z, lambda, y (the chunk adds x and lambda behind it)
uint64_t opt_per_knot(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box)
{
    const uint64_t e = box ? 0 : (uint64_t)mx * nx + (uint64_t)mu * nu;
    return (uint64_t)nx * nx + (uint64_t)nu * nu + (uint64_t)nx * ((uint64_t)nx + nu) + e + 2ull * nx + nu + (uint64_t)mx + mu;
}

}  // namespace

template <typename T, bool BOX>
__global__ __launch_bounds__(256) void admm_optimality_kernel(OptShape s, const T *__restrict__ G, const T *__restrict__ C,
                                                              const T *__restrict__ g, const T *__restrict__ c,
                                                              const T *__restrict__ E, const T *__restrict__ rho,
                                                              const T *__restrict__ z, const T *__restrict__ lambda,
                                                              const T *__restrict__ w, const T *__restrict__ y, T eps_abs, T eps_rel,
                                                              T *__restrict__ opt, uint8_t *__restrict__ done)
{
    using U = decltype(abs_bits(T(0)));
    extern __shared__ __attribute__((aligned(16))) unsigned char opt_lds[];
    __shared__ U slots[24];   // six words per wave
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = BOX ? 0u : mx * nx + mu * nu, nn = nx * nx, sg = nn + nu * nu, sc = nx * sv;
    // Q_k R_k | [A_k | B_k] | E blocks | z (kch knots + one x) | lambda (kch + 1 knots) | y
    T *sG = reinterpret_cast<T *>(opt_lds);
    T *sC = sG + kch * sg, *sE = sC + kch * sc, *sz = sE + kch * se, *sl = sz + kch * sv + nx, *sy = sl + (kch + 1) * nx;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const uint64_t prob = blockIdx.x;
    const uint64_t nz = (uint64_t)sv * N - nu, nw = (uint64_t)sw * N - mu, nl = (uint64_t)nx * N;
    if (!s.shared) {
        G += prob * ((uint64_t)sg * N - nu * nu);
        C += prob * ((uint64_t)sc * (N - 1));
        if constexpr (!BOX) E += prob * ((uint64_t)se * N - mu * nu);
    }
    g += prob * nz, z += prob * nz, c += prob * nl, lambda += prob * nl, w += prob * nw, y += prob * nw;
    const T r = rho[prob];
    U rs = 0, re = 0, rr = 0, ns = 0, ne = 0, nr = 0;

    for (uint64_t k0 = 0; k0 < N; k0 += kch) {
        const uint32_t kc = (uint32_t)(N - k0 < kch ? N - k0 : kch);
        const bool end = k0 + kc == N;   // the last knot of the horizon: no R, no [A | B], no Eu block, no u, no knot behind it
        const uint32_t kd = kc - (end ? 1u : 0u);   // knots of the chunk with a knot behind them
        const uint32_t gc = kc * sg - (end ? nu * nu : 0u), cc = kd * sc, zc = kc * sv - (end ? nu : 0u),
                       wc = kc * sw - (end ? mu : 0u);
        const uint64_t z0 = k0 * sv, l0 = k0 * nx, w0 = k0 * sw;
        {
            const T *src = G + k0 * sg;
            for (uint32_t i = tid; i < gc; i += threads) sG[i] = src[i];
            src = C + k0 * sc;   // (cc == 0 where there is no C: never read)
            for (uint32_t i = tid; i < cc; i += threads) sC[i] = src[i];
            if constexpr (!BOX) {
                const uint32_t ec = kc * se - (end ? mu * nu : 0u);
                src = E + k0 * se;
                for (uint32_t i = tid; i < ec; i += threads) sE[i] = src[i];
            }
            const uint32_t zs = zc + (end ? 0u : nx), ls = (kd + 1) * nx;
            for (uint32_t i = tid; i < zs; i += threads) sz[i] = z[z0 + i];
            for (uint32_t i = tid; i < ls; i += threads) sl[i] = lambda[l0 + i];
            for (uint32_t i = tid; i < wc; i += threads) sy[i] = y[w0 + i];
        }
        __syncthreads();

        // S: entry e of the chunk's piece of z
        for (uint32_t e = tid; e < zc; e += threads) {
            const uint32_t kk = e / sv;
            const uint32_t col = e - kk * sv;
            const bool last = end && kk + 1 == kc;
            const T *nxt = sl + (kk + 1) * nx;   // lambda of the knot behind
            const T gv = g[z0 + e];
            T acc, a = T(0), t;
            if (col < nx) {
                const T lam = sl[kk * nx + col];
                const T *Q = sG + kk * sg + col, *x = sz + kk * sv;   // Q_k(col, q), q ascending: a stride of nx
                acc = gv + lam, t = lam;
                for (uint32_t q = 0; q < nx; ++q) {
                    acc = fma_once(Q[q * nx], x[q], acc);
                    a = fma_once(Q[q * nx], x[q], a);
                }
                if (!last) {
                    const T *A = sC + kk * sc + col * nx;   // A_k(q, col), q ascending
                    for (uint32_t q = 0; q < nx; ++q) {
                        acc = fma_once(A[q], -nxt[q], acc);
                        t = fma_once(A[q], -nxt[q], t);
                    }
                }
            } else {   // (the last knot has no u: never here)
                const uint32_t cu = col - nx;
                const T *R = sG + kk * sg + nn + cu, *u = sz + kk * sv + nx;
                const T *B = sC + kk * sc + nn + cu * nx;   // B_k(q, cu)
                acc = gv, t = T(0);
                for (uint32_t q = 0; q < nu; ++q) {
                    acc = fma_once(R[q * nu], u[q], acc);
                    a = fma_once(R[q * nu], u[q], a);
                }
                for (uint32_t q = 0; q < nx; ++q) {
                    acc = fma_once(B[q], -nxt[q], acc);
                    t = fma_once(B[q], -nxt[q], t);
                }
            }
            T u = T(0);
            if constexpr (BOX) {
                u = fma_once(T(1), sy[e], u);   // (sw == sv: the row IS the entry)
            } else {
                uint32_t cl = col, rows = mx;
                const T *blk = sE + kk * se, *yy = sy + kk * sw;
                if (col >= nx) cl -= nx, rows = mu, blk += mx * nx, yy += mx;
                blk += cl * rows;
                for (uint32_t i = 0; i < rows; ++i) u = fma_once(blk[i], yy[i], u);
            }
            rs = umax(rs, abs_bits(fma_once(r, u, acc)));
            ns = umax(ns, umax(umax(abs_bits(a), abs_bits(fma_once(r, u, t))), abs_bits(gv)));
        }
        // D: entry i of lambda; knot kk of the chunk evaluates the dynamics into knot kk + 1
        if (k0 == 0)
            for (uint32_t i = tid; i < nx; i += threads) {
                const T x0 = sz[i], c0 = c[i];
                re = umax(re, abs_bits(x0 - c0));
                ne = umax(ne, umax(abs_bits(x0), abs_bits(c0)));
            }
        for (uint32_t i = tid; i < kd * nx; i += threads) {
            const uint32_t kk = i / nx;
            const uint32_t row = i - kk * nx;
            const T xn = sz[(kk + 1) * sv + row], cv = c[l0 + nx + i];
            const T *A = sC + kk * sc + row, *x = sz + kk * sv;   // A_k(row, q): a stride of nx; B_k behind it
            T f = xn - cv, h = xn;
            for (uint32_t q = 0; q < sv; ++q) {   // x_k then u_k against [A_k | B_k]: one run of columns
                f = fma_once(A[q * nx], -x[q], f);
                h = fma_once(A[q * nx], -x[q], h);
            }
            re = umax(re, abs_bits(f));
            ne = umax(ne, umax(abs_bits(h), abs_bits(cv)));
        }
        // R: row q of the chunk
        for (uint32_t q = tid; q < wc; q += threads) {
            T v;
            if constexpr (BOX) {
                v = sz[q];
            } else {
                const uint32_t kk = q / sw;
                uint32_t row = q - kk * sw, cols = nx, ld = mx;
                const T *blk = sE + kk * se, *zz = sz + kk * sv;
                if (row >= mx) row -= mx, cols = nu, ld = mu, blk += mx * nx, zz += nx;
                v = T(0);
                for (uint32_t j = 0; j < cols; ++j) v = fma_once(blk[j * ld + row], zz[j], v);
            }
            const T wv = w[w0 + q];
            rr = umax(rr, abs_bits(v - wv));
            nr = umax(nr, umax(abs_bits(v), abs_bits(wv)));
        }
        __syncthreads();   // the next chunk may overwrite the staging
    }

    const uint32_t wave = tid >> 6, lane = tid & 63u, waves = threads >> 6;
    U m[6] = {wave_umax(rs), wave_umax(re), wave_umax(rr), wave_umax(ns), wave_umax(ne), wave_umax(nr)};
    if (lane == 0)
        for (uint32_t i = 0; i < 6; ++i) slots[6 * wave + i] = m[i];
    __syncthreads();
    if (tid == 0) {
        T o[6];
        for (uint32_t i = 0; i < 6; ++i) {
            U b = m[i];
            for (uint32_t wv = 1; wv < waves; ++wv) b = umax(b, slots[6 * wv + i]);
            o[i] = from_bits(b);
            opt[6 * prob + i] = o[i];
        }
        if (done)
            done[prob] = (o[0] <= fma_once(eps_rel, o[3], eps_abs) && o[1] <= fma_once(eps_rel, o[4], eps_abs) &&
                          o[2] <= fma_once(eps_rel, o[5], eps_abs))
                             ? 1
                             : 0;
    }
}

template <typename T> bool admm_optimality_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box)
{
    return (opt_per_knot(nx, nu, mx, mu, box) + 2ull * nx) * sizeof(T) <= kOptLdsBytes;
}

uint32_t admm_optimality_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box)
{
    const uint64_t kch = kOptStage / opt_per_knot(nx, nu, mx, mu, box);
    return (uint32_t)(kch < 1 ? 1 : (kch > kOptMaxKnots ? kOptMaxKnots : kch));
}

template <typename T>
hipError_t launch_admm_optimality(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *G, const T *C,
                                  const T *g, const T *c, const T *E, const T *rho, const T *z, const T *lambda, const T *w, const T *y,
                                  T eps_abs, T eps_rel, T *opt, uint8_t *done, hipStream_t s, bool box, bool shared)
{
    if (box) mx = nx, mu = nu;
    if (batch > 0x7fffffffu || !admm_optimality_shape_ok<T>(nx, nu, mx, mu, box)) return hipErrorInvalidValue;   // one workgroup per problem
    OptShape sh{nx, nu, mx, mu, N, admm_optimality_knot_chunk(nx, nu, mx, mu, box), shared ? 1u : 0u};
    if (sh.kch > N) sh.kch = N;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu, nw = ((uint64_t)mx + mu) * N - mu;
    const uint32_t threads = (nz > nw ? nz : nw) <= 256 ? 64 : 256;
    const size_t lds = ((size_t)sh.kch * opt_per_knot(nx, nu, mx, mu, box) + 2 * (size_t)nx) * sizeof(T);
    if (box)
        hipLaunchKernelGGL((admm_optimality_kernel<T, true>), dim3(batch), dim3(threads), lds, s, sh, G, C, g, c, E, rho, z, lambda, w, y,
                           eps_abs, eps_rel, opt, done);
    else
        hipLaunchKernelGGL((admm_optimality_kernel<T, false>), dim3(batch), dim3(threads), lds, s, sh, G, C, g, c, E, rho, z, lambda, w,
                           y, eps_abs, eps_rel, opt, done);
    return hipGetLastError();
}

template bool admm_optimality_shape_ok<float>(uint32_t, uint32_t, uint32_t, uint32_t, bool);
template bool admm_optimality_shape_ok<double>(uint32_t, uint32_t, uint32_t, uint32_t, bool);
template hipError_t launch_admm_optimality<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *,
                                                  const float *, const float *, const float *, const float *, const float *,
                                                  const float *, const float *, const float *, const float *, float, float, float *,
                                                  uint8_t *, hipStream_t, bool, bool);
template hipError_t launch_admm_optimality<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                   const double *, const double *, const double *, const double *, const double *,
                                                   const double *, const double *, const double *, const double *, double, double,
                                                   double *, uint8_t *, hipStream_t, bool, bool);

}  // namespace gbdpcg
