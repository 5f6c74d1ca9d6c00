// admm_infeas.hip -- the primal infeasibility certificate of the hard ADMM paths (gbdpcg_admm_infeas_*, gbdpcg_admm_lin_infeas_* and
// their _shared twins).  Problem b minimises 1/2 z'Gz + g'z subject to Cz = c and lo <= E z <= hi (the box: E = I).  It is infeasible
// iff some (dl, dm) has C'dl + E'dm = 0 and c'dl + sum_r (dm_r > 0 ? hi_r dm_r : lo_r dm_r) < 0 (Farkas).  On an infeasible problem
// the differences of two iterates of the splitting, dl = lambda1 - lambda0 and dm = rho (y1 - y0), tend to such a pair: this launch
// evaluates how close they are.  The packed layouts are those of admm_rows.hip (E, the rows) and schur_residual.hip (C, c, lambda).
// A CHAIN is acc = seed; acc = fma(a_i, b_i, acc) in ascending i; every line below is ONE IEEE operation or a comparison
// (ieee_once.hpp), so every output is defined to the bit whatever the launch shape:
//   dl = lambda1 - lambda0;   dy = y1 - y0;   m_r = rho_b dy_r
//   x-part of knot k, entry r:   s = dl_k[r];  s = fma(A_k(q,r), -dl_{k+1}[q], s), q < nx (absent at the last knot)
//   u-part of knot k, entry r:   s = +0;       s = fma(B_k(q,r), -dl_{k+1}[q], s), q < nx
//        (the signs and the order of the C' terms of schur_residual.hip's stationarity chain)
//   u = chain over the rows i of the entry's block of E(i,r) dy_i, seed +0;      q = fma(rho_b, u, s)
//   cert[3b]   = n = max(max |dl|, max_r |m_r|)      the scale            (norm_fold.hpp: over bit patterns, NaN on top)
//   cert[3b+1] = r = max_j |q_j|                     the residual of the certificate
//   t_k:  acc = +0;  over the knot's rows in storage order:  dy_r > 0: acc = fma(hi_r, m_r, acc);  dy_r < 0: acc = fma(lo_r, m_r, acc);
//         otherwise nothing (a zero or NaN dy_r never multiplies an infinite bound);  then acc = fma(c_k[i], dl_k[i], acc), i < nx
//   cert[3b+2] = sigma:  acc = +0;  acc = acc + t_k for k ascending        the support value; the two levels are part of the definition
//   flag[b] = (n > 0 && r <= eps n && sigma < -(eps n)) ? 1 : 0           eps n ONE product; a NaN anywhere fails a comparison: 0
// BOX (the gbdpcg_admm_infeas_* calls): the rows are the entries of z and the u chain is the single line u = fma(1, dy_r, +0): for
// finite data the bits of the rows launch with E = I, mx = nx, mu = nu (the zero entries of I add +-0 to a chain; the sign of a zero q
// does not reach its magnitude).  A NaN or Inf dy_i stays in ITS entry of q here; through the zero entries of an explicit I it
// reaches every entry of its block.
//
// admm_infeas_kernel<T, BOX>: ONE WORKGROUP PER PROBLEM, 64-bit problem strides, nothing crosses a workgroup: no atomics, no memset, no
// scratch, nothing read from cert or flag.  The horizon is walked in chunks of `kch` knots, the shape of rows_update (admm_rows.hip):
// the host takes as many knots as fit 4096 staged elements, at most 64 -- 16 KiB in fp32, 32 KiB in fp64, so 8 resp. 5 workgroups
// of 256 lanes share the 160 KiB of a compute unit and the launch keeps 20 to 32 waves per unit in flight, which a kernel that waits
// for memory wants more than it wants longer chunks.  Per chunk:
//   STAGE   [A_k | B_k] and the E blocks (one contiguous range of memory each), c, and dl for the chunk's knots AND the knot behind
//           them (the C' terms of the chunk's last knot); lanes own ROWS: dy, m, the bound dy's sign selects -> the row's three LDS
//           slots, |m| and |dl| folded into n.                                                                          barrier
//   Q       lanes own ENTRIES of z: the C' chain, the E' chain, q, |q| folded into r.
//   T       lanes own KNOTS: t_k out of LDS into the knot's slot (no barrier between Q and T: both only read the staging). barrier
//   SIGMA   lane 0 adds the chunk's t_k in ascending k.  (The next chunk's STAGE does not write the t slots; its barrier orders T.)
// Every global access is a scalar one at consecutive addresses across lanes, so the alignment of the base pointers plays no part.
// In Q consecutive lanes read columns of A_k / E, a stride of nx / mx elements: a bank conflict of that order on an LDS read, as in
// phase B of rows_update.  Global traffic per problem: C, E, c, lo or hi once, lambda and y twice -- no G, so strictly less than
// gbdpcg_kkt_residual_* reads.  Measured next to that launch: profiles/r25_admm_infeas.txt.
#include "ieee_once.hpp"
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

constexpr uint32_t kInfeasStage = 4096;         // elements staged per chunk, unless one knot needs more
constexpr uint32_t kInfeasMaxKnots = 64;        // knots per chunk at most
constexpr size_t kInfeasLdsBytes = 60 * 1024;   // what one knot may take at the outside (64 KB less the norm slots and slack)

struct InfeasShape {
    uint32_t nx, nu, mx, mu, N;
    uint32_t kch;      // knots per chunk
    uint32_t shared;   // C and E are one problem's
};

// what one knot takes of the staging: [A_k | B_k], its E blocks, dl, c, three slots per row, t_k
uint64_t infeas_per_knot(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box)
{
    const uint64_t e = box ? 0 : (uint64_t)mx * nx + (uint64_t)mu * nu;
    return (uint64_t)nx * ((uint64_t)nx + nu) + e + 2ull * nx + 3ull * ((uint64_t)mx + mu) + 1;
}

}  // namespace

template <typename T, bool BOX>
__global__ __launch_bounds__(256) void admm_infeas_kernel(InfeasShape s, const T *__restrict__ C, const T *__restrict__ c,
                                                          const T *__restrict__ E, const T *__restrict__ lo, const T *__restrict__ hi,
                                                          const T *__restrict__ rho, const T *__restrict__ lam0,
                                                          const T *__restrict__ lam1, const T *__restrict__ y0, const T *__restrict__ y1,
                                                          T eps, T *__restrict__ cert, uint8_t *__restrict__ flag)
{
    using U = decltype(abs_bits(T(0)));
    extern __shared__ __attribute__((aligned(16))) unsigned char infeas_lds[];
    __shared__ U slots[8];   // two words per wave
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = BOX ? 0u : mx * nx + mu * nu, sc = nx * sv;
    // [A_k | B_k] | E blocks | dl (kch + 1 knots) | c | dy | m | bound | t_k
    T *sC = reinterpret_cast<T *>(infeas_lds);
    T *sE = sC + kch * sc, *sl = sE + kch * se, *scc = sl + (kch + 1) * nx, *sdy = scc + kch * nx, *sm = sdy + kch * sw,
      *sb = sm + kch * sw, *stk = sb + kch * sw;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const uint64_t prob = blockIdx.x;
    const uint64_t nw = (uint64_t)sw * N - mu, nl = (uint64_t)nx * N;
    if (!s.shared) {
        C += prob * ((uint64_t)sc * (N - 1));
        if constexpr (!BOX) E += prob * ((uint64_t)se * N - mu * nu);
    }
    c += prob * nl, lam0 += prob * nl, lam1 += prob * nl;
    lo += prob * nw, hi += prob * nw, y0 += prob * nw, y1 += prob * nw;
    const T r = rho[prob];
    U mn = 0, mr = 0;
    T sigma = T(0);

    for (uint64_t k0 = 0; k0 < N; k0 += kch) {
        const uint32_t kc = (uint32_t)(N - k0 < kch ? N - k0 : kch);
        const bool end = k0 + kc == N;   // the last knot of the horizon: no [A | B], no Eu block, no u rows, no knot behind it
        const uint32_t cc = (kc - (end ? 1u : 0u)) * sc, lc = (kc + (end ? 0u : 1u)) * nx, zc = kc * sv - (end ? nu : 0u),
                       wc = kc * sw - (end ? mu : 0u);
        const uint64_t c0 = k0 * sc, l0 = k0 * nx, w0 = k0 * sw;
        for (uint32_t i = tid; i < cc; i += threads) sC[i] = C[c0 + i];
        if constexpr (!BOX) {
            const uint32_t ec = kc * se - (end ? mu * nu : 0u);
            const uint64_t e0 = k0 * se;
            for (uint32_t i = tid; i < ec; i += threads) sE[i] = E[e0 + i];
        }
        for (uint32_t i = tid; i < lc; i += threads) {
            const T dl = lam1[l0 + i] - lam0[l0 + i];
            sl[i] = dl;
            mn = umax(mn, abs_bits(dl));   // (the knot behind the chunk is folded twice: a maximum does not mind)
        }
        for (uint32_t i = tid; i < kc * nx; i += threads) scc[i] = c[l0 + i];
        // row q of the chunk
        for (uint32_t q = tid; q < wc; q += threads) {
            const T dy = y1[w0 + q] - y0[w0 + q];
            const T m = r * dy;
            T b = T(0);
            if (dy > T(0))
                b = hi[w0 + q];
            else if (dy < T(0))
                b = lo[w0 + q];
            sdy[q] = dy, sm[q] = m, sb[q] = b;
            mn = umax(mn, abs_bits(m));
        }
        __syncthreads();

        // Q: entry e of the chunk's piece of z
        for (uint32_t e = tid; e < zc; e += threads) {
            const uint32_t kk = e / sv;
            const uint32_t col = e - kk * sv;
            const bool last = end && kk + 1 == kc;
            const T *nxt = sl + (kk + 1) * nx;   // dl of the knot behind
            T acc;
            if (col < nx) {
                acc = sl[kk * nx + col];
                if (!last) {
                    const T *a = sC + kk * sc + col * nx;   // A_k(q, col), q ascending
                    for (uint32_t q = 0; q < nx; ++q) acc = fma_once(a[q], -nxt[q], acc);
                }
            } else {   // (the last knot has no u: never here)
                acc = T(0);
                const T *b = sC + kk * sc + nx * nx + (col - nx) * nx;   // B_k(q, col - nx)
                for (uint32_t q = 0; q < nx; ++q) acc = fma_once(b[q], -nxt[q], acc);
            }
            T u = T(0);
            if constexpr (BOX) {
                u = fma_once(T(1), sdy[e], u);   // (sw == sv: the row IS the entry)
            } else {
                uint32_t cl = col, rows = mx;
                const T *blk = sE + kk * se, *dd = sdy + kk * sw;
                if (col >= nx) cl -= nx, rows = mu, blk += mx * nx, dd += mx;
                blk += cl * rows;
                for (uint32_t i = 0; i < rows; ++i) u = fma_once(blk[i], dd[i], u);
            }
            mr = umax(mr, abs_bits(fma_once(r, u, acc)));
        }
        // T: knot kk of the chunk
        for (uint32_t kk = tid; kk < kc; kk += threads) {
            const uint32_t rows = (end && kk + 1 == kc) ? mx : sw;
            const T *dd = sdy + kk * sw, *mm = sm + kk * sw, *bb = sb + kk * sw, *ck = scc + kk * nx, *lk = sl + kk * nx;
            T acc = T(0);
            for (uint32_t i = 0; i < rows; ++i)
                if (dd[i] > T(0) || dd[i] < T(0)) acc = fma_once(bb[i], mm[i], acc);
            for (uint32_t i = 0; i < nx; ++i) acc = fma_once(ck[i], lk[i], acc);
            stk[kk] = acc;
        }
        __syncthreads();   // the t_k are there, and the next chunk may overwrite the staging
        if (tid == 0)
            for (uint32_t kk = 0; kk < kc; ++kk) sigma = sigma + stk[kk];
    }

    const uint32_t waves = threads >> 6;
    T *out = cert + 3 * prob;
    store_norms(mn, mr, tid >> 6, tid & 63u, waves, [&](uint32_t wv) { return slots + 2 * wv; }, out);
    if (tid == 0) {   // the folded pair again, out of the waves' slots: nothing is read from cert
        U bn = slots[0], br = slots[1];
        for (uint32_t wv = 1; wv < waves; ++wv) bn = umax(bn, slots[2 * wv]), br = umax(br, slots[2 * wv + 1]);
        const T n = from_bits(bn), rr = from_bits(br);
        const T en = eps * n;
        out[2] = sigma;
        if (flag) flag[prob] = (n > T(0) && rr <= en && sigma < -en) ? 1 : 0;
    }
}

template <typename T> bool admm_infeas_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box)
{
    return (infeas_per_knot(nx, nu, mx, mu, box) + nx) * sizeof(T) <= kInfeasLdsBytes;
}

uint32_t admm_infeas_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box)
{
    const uint64_t kch = kInfeasStage / infeas_per_knot(nx, nu, mx, mu, box);
    return (uint32_t)(kch < 1 ? 1 : (kch > kInfeasMaxKnots ? kInfeasMaxKnots : kch));
}

template <typename T>
hipError_t launch_admm_infeas(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *C, const T *c,
                              const T *E, const T *lo, const T *hi, const T *rho, const T *lam0, const T *lam1, const T *y0,
                              const T *y1, T eps, T *cert, uint8_t *flag, hipStream_t s, bool box, bool shared)
{
    if (box) mx = nx, mu = nu;
    if (batch > 0x7fffffffu || !admm_infeas_shape_ok<T>(nx, nu, mx, mu, box)) return hipErrorInvalidValue;   // one workgroup per problem
    InfeasShape sh{nx, nu, mx, mu, N, admm_infeas_knot_chunk(nx, nu, mx, mu, box), shared ? 1u : 0u};
    if (sh.kch > N) sh.kch = N;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu, nw = ((uint64_t)mx + mu) * N - mu;
    const uint32_t threads = (nz > nw ? nz : nw) <= 256 ? 64 : 256;
    const size_t lds = ((size_t)sh.kch * infeas_per_knot(nx, nu, mx, mu, box) + nx) * sizeof(T);
    if (box)
        hipLaunchKernelGGL((admm_infeas_kernel<T, true>), dim3(batch), dim3(threads), lds, s, sh, C, c, E, lo, hi, rho, lam0, lam1, y0,
                           y1, eps, cert, flag);
    else
        hipLaunchKernelGGL((admm_infeas_kernel<T, false>), dim3(batch), dim3(threads), lds, s, sh, C, c, E, lo, hi, rho, lam0, lam1, y0,
                           y1, eps, cert, flag);
    return hipGetLastError();
}

template bool admm_infeas_shape_ok<float>(uint32_t, uint32_t, uint32_t, uint32_t, bool);
template bool admm_infeas_shape_ok<double>(uint32_t, uint32_t, uint32_t, uint32_t, bool);
template hipError_t launch_admm_infeas<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                              const float *, const float *, const float *, const float *, const float *, const float *,
                                              const float *, const float *, float, float *, uint8_t *, hipStream_t, bool, bool);
template hipError_t launch_admm_infeas<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                               const double *, const double *, const double *, const double *, const double *,
                                               const double *, const double *, const double *, const double *, double, double *,
                                               uint8_t *, hipStream_t, bool, bool);

}  // namespace gbdpcg
