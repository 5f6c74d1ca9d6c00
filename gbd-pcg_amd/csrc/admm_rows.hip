// admm_rows.hip -- ADMM on a kept KKT factorisation with stage-wise rows on E z (gbdpcg_admm_lin_form_*; gbdpcg_admm_lin_init_*,
// gbdpcg_admm_lin_update_*, gbdpcg_admm_lin_adjoint_init_*, gbdpcg_admm_lin_adjoint_update_*, gbdpcg_admm_soc_init_*,
// gbdpcg_admm_soc_update_*, the last launch of gbdpcg_admm_lin_step_*, gbdpcg_admm_lin_adjoint_step_* and gbdpcg_admm_soc_step_*).
// Problem b minimises 1/2 z'Gz + g'z subject to Cz = c and, row by row, lo <= (E z)_r <= hi (a LINEAR
// row) or (E z + f)_cone in K_q = {(s_0, s_1 .. s_{q-1}) : ||(s_1 .. s_{q-1})||_2 <= s_0} (the rows of a SECOND-ORDER CONE).  E is
// block-diagonal with the blocks of G: Ex_k (mx x nx) on x_k, Eu_k (mu x nu) on u_k, column-major, packed [Ex_0 Eu_0 Ex_1 ...
// Ex_{N-1}]; the rows, and with them lo, hi, w, y, are packed [mx | mu | mx | ... | mx].  The matrices of the solve belong to
// Gt = G + rho_b E'E, w is the copy of E z (+ f) that lives in the set, y the scaled multiplier of E z (+ f) = w (mu = rho y).
// A CHAIN is acc = seed; acc = fma(a_i, b_i, acc) in ascending i, seed +0 unless said otherwise; every line below is one IEEE
// operation or a comparison (ieee_once.hpp; / and sqrt correctly rounded), so every output is defined to the bit whatever the
// launch shape.
//   FORM    P(i,j) = chain over rows r of E(r,i) E(r,j);  Gt(i,j) = fma(rho, P(i,j), G(i,j))     per diagonal block
//   UPDATE  v_r = chain over columns j of E(r,j) z_j;  s = v + y;  w+ = s < lo ? lo : (s > hi ? hi : s);  y+ = s - w+
//           t = w+ - y+;  d = w+ - w;  u_j = chain over rows r of E(r,j) t_r;  e_j likewise with d;  gt_j = fma(-rho, u_j, g_j)
//           res[2b] = max_r |v_r - w+_r|;  res[2b+1] = max_j |rho e_j|        (norm_fold.hpp: over bit patterns, NaN on top)
//   INIT    w <- clip(w), y not written, t = w - y, gt_j = fma(-rho, u_j, g_j); z and res are not looked at.
// CONES (the gbdpcg_admm_soc_* calls) add row classes: in every x block the first lx rows are linear as above, the other mx - lx
// rows are consecutive cones of dimension qx, head row first; lu, qu likewise for the u blocks.  On a cone row lo[r] holds the
// offset f_r and hi[r] is NOT READ:
//   UPDATE  cone row:   the v chain is SEEDED with f_r;  s_r = v_r + y_r
//           per cone:   n2 = chain over i = 1 .. q-1 of s_i s_i;  a = sqrt(n2)
//                       a <= s_0: w+ = s;   else a <= -s_0: w+ = +0;   else h = 0.5 (s_0 + a), c = h / a, w+_0 = h, w+_i = c s_i
//           y+ = s - w+;  t = (w+ - y+) - f;  d = w+ - w;  u, e, gt, res as above
//   INIT    w <- projection of w by the same lines with s := w, y not written, t = (w - y) - f.
// A NaN fails both comparisons and stays NaN through the third branch; q = 1 is the half-line s_0 >= 0 (an empty chain, a = +0).
// SOFT (the gbdpcg_admm_lin_soft_* calls; never together with CONES: cone rows stay hard) replaces the constraint on row r by the
// penalty kappa_r dist((E z)_r, [lo_r, hi_r]).  Only the lines of w+ and y+ change (soft_clip in ieee_once.hpp):
//   UPDATE  p = clip(s);  e = s - p;  theta = kappa / rho;  w+ = e > theta ? s - theta : (e < -theta ? s + theta : p)
//           y+ = e > theta ? theta : (e < -theta ? -theta : e)             kappa = +Inf: the third branch, the hard bits
//   INIT    w <- (kappa == +Inf) ? clip(w) : w
// ADJOINT (the gbdpcg_admm_lin_adjoint_* calls, the backward pass of the hard linear rows; never with CONES or SOFT) projects onto
// the degenerate rows a forward y (yf, read only) stands for: {0} where yf_r != 0 (a NaN included), the whole line elsewhere.  Only the
// line of w+ changes (pin in ieee_once.hpp), in UPDATE and INIT alike:
//   w+ = yf != 0 ? clip(s, +0, +0) : s          the bits of the hard lines with lo = hi = +0 where yf != 0, -Inf / +Inf elsewhere
// yf is read where lo is read and there is no hi: admm_rows_adjoint_kernel takes one pointer less and makes 3 row reads, not 4.  The
// body is shared (rows_update, forced inline into both __global__ entries); ADJ is its compile-time switch.
// kappa has the layout of lo and is read in phase A by the lane that owns the row, one more scalar global read per row; no LDS slot
// is added and phase B is untouched.  The hard instantiations take no kappa argument (an empty parameter pack).
//
// admm_lin_form_kernel: one lane per entry of Gt, 256 consecutive entries of one problem per workgroup; the entry is read and
// written by the same lane, so Gt may be G.  E is read through the caches (2 m values per entry against one element in, one out);
// the three index divisions per entry are plain divides, next to a chain of m fmas and 2 m loads they are not the cost.  It does
// not look at the set the rows are projected on.
//
// admm_rows_update_kernel<T, INIT, CONES>: ONE WORKGROUP PER PROBLEM, like admm.hip (the two norms are per problem: nothing crosses
// a workgroup, no atomics, no memset, no scratch, nothing read from res).  The horizon is walked in chunks of `kch` knots (the host:
// as many as fit 4096 staged elements, at most 64).  Per chunk: the chunk's E blocks and its piece of z go to LDS (each one
// contiguous range of memory); PHASE A, lanes own rows: w and y written, the primal norm folded, t and d left in the row's two LDS
// slots; barrier; PHASE B, lanes own entries of z: the two column chains out of LDS, gt written, the dual norm folded; barrier.
// CONES is a compile-time switch on phase A alone, so the linear instantiations hold nothing of the cones:
//   linear  one pass: the v chain out of LDS, the clip, w, y, t, d.
//   cones   A1  lanes own rows: v and s go to the row's two LDS slots (v where d will be, s where t will be).   barrier.
//           A2  lanes own rows again, in passes of blockDim.x rows.  A linear row is clipped; a cone row runs its cone's n2 chain
//               over the s slots in ascending order -- every lane of a cone holds identical bits, q LDS reads per row instead of a
//               second ownership map -- and writes only its own w, y, d.  Its t has to replace an s that other lanes of the cone
//               still read, and a cone may straddle two passes: so a pass is closed by a barrier, and the t of a pass is written
//               behind the barrier of the NEXT pass (a cone has at most 64 rows, it never reaches two passes back).  One carried
//               register, one barrier per pass.  Row -> (cone, position) is index arithmetic on lx, qx, lu, qu.
// Every global access is a scalar one at consecutive addresses across lanes, so the alignment of the base pointers plays no part.
// In phase A consecutive lanes read consecutive rows of a column of E (no bank conflict); in phase B consecutive lanes read
// columns, a stride of mx or mu elements -- a conflict of that order on an LDS read.  Global traffic: per row 4 reads and 2 writes,
// per entry of z 2 reads and 1 write, E once.  Measured at 1024 x (14, 7, 128), 4 + 2 rows (profiles/r11_admm_lin.txt): 31 us in
// fp32, 35 us in fp64 -- 0.46 and 0.77 of the box update's bytes over time, so the fp32 launch is not at its memory bound yet; with
// cones, profiles/r12_admm_soc.txt.
#include <type_traits>

#include "ieee_once.hpp"
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

constexpr uint32_t kRowsStage = 4096;          // elements staged per chunk (E, z, t, d together), unless one knot needs more
constexpr uint32_t kRowsMaxKnots = 64;         // knots per chunk at most
constexpr size_t kRowsLdsBytes = 60 * 1024;    // what one knot may take at the outside (64 KB less the norm slots and slack)

// The kernel's sizes.  The row classes sit between the two halves in the CONES instantiations and are absent from the linear
// ones, which therefore take the arguments, and compile to the code, of a kernel that knows nothing of cones.
struct RowsDims {
    uint32_t nx, nu, mx, mu;
};
struct RowsWalk {
    uint32_t N;
    uint32_t kch;        // knots per chunk
    uint32_t shared;     // E is one problem's
};
struct NoClasses {};
template <bool CONES> struct RowsShape : RowsDims, std::conditional_t<CONES, RowClasses, NoClasses>, RowsWalk {};

// what one knot takes of the staging: its E blocks, its piece of z, two slots per row
uint64_t rows_per_knot(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
{
    return (uint64_t)mx * nx + (uint64_t)mu * nu + nx + nu + 2ull * (mx + mu);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void admm_lin_form_kernel(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t bpp,
                                                            const T *G, const T *__restrict__ E, const T *__restrict__ rho, T *Gt)
{
    const uint32_t prob = blockIdx.x / bpp, f = (blockIdx.x - prob * bpp) * 256u + threadIdx.x;
    const uint32_t sg = nx * nx + nu * nu, se = mx * nx + mu * nu;
    const uint64_t LG = (uint64_t)sg * N - nu * nu, LE = (uint64_t)se * N - mu * nu;
    if (f >= LG) return;
    const uint32_t k = f / sg;
    uint32_t e = f - k * sg, d = nx, m = mx;
    const T *blk = E + prob * LE + (uint64_t)k * se;
    if (e >= nx * nx) e -= nx * nx, d = nu, m = mu, blk += mx * nx;
    const uint32_t j = e / d, i = e - j * d;
    const T *ci = blk + (uint64_t)i * m, *cj = blk + (uint64_t)j * m;
    T p = T(0);
    for (uint32_t r = 0; r < m; ++r) p = fma_once(ci[r], cj[r], p);
    const uint64_t at = prob * LG + f;
    Gt[at] = fma_once(rho[prob], p, G[at]);
}

// The body of the two kernels below.  ADJ (the adjoint instantiations, never with CONES or SOFT): lo is yf, hi is not looked at.
template <typename T, bool INIT, bool CONES, bool SOFT, bool ADJ, typename... K>
__device__ __forceinline__ void rows_update(const RowsShape<CONES> &s, const T *__restrict__ g, const T *__restrict__ E,
                                            const T *__restrict__ lo, const T *__restrict__ hi, const T *__restrict__ rho,
                                            const T *__restrict__ z, T *__restrict__ w, T *__restrict__ y, T *__restrict__ gt,
                                            T *__restrict__ res, K... kappa_arg)
{
    static_assert(!(SOFT && CONES), "cone rows stay hard");
    static_assert(!(ADJ && (SOFT || CONES)), "the adjoint rows are hard linear rows");
    static_assert(sizeof...(K) == (SOFT ? 1 : 0), "kappa is an argument of the soft instantiations alone");
    using U = decltype(abs_bits(T(0)));
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_lds[];
    __shared__ U slots[8];   // two words per wave
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = mx * nx + mu * nu;
    T *sE = reinterpret_cast<T *>(rows_lds);   // the chunk's E blocks | its piece of z | t (cones: s before) | d (cones: v before)
    T *sz = sE + kch * se, *st = sz + kch * sv, *sd = st + kch * sw;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t nz = (uint64_t)sv * N - nu, nw = (uint64_t)sw * N - mu, ne = (uint64_t)se * N - mu * nu;
    g += prob * nz, gt += prob * nz, lo += prob * nw, w += prob * nw, y += prob * nw;
    if constexpr (!ADJ) hi += prob * nw;
    if constexpr (!INIT) z += prob * nz;
    [[maybe_unused]] const T *__restrict__ kappa = nullptr;
    if constexpr (SOFT) kappa = kappa_of<T>(kappa_arg...) + prob * nw;
    if (!s.shared) E += prob * ne;
    const T r = rho[prob];
    U mp = 0, md = 0;

    for (uint64_t k0 = 0; k0 < N; k0 += kch) {
        const uint32_t kc = (uint32_t)(N - k0 < kch ? N - k0 : kch);
        const bool end = k0 + kc == N;   // the last knot of the horizon has no u: no Eu block, no u rows
        const uint32_t ec = kc * se - (end ? mu * nu : 0u), zc = kc * sv - (end ? nu : 0u), wc = kc * sw - (end ? mu : 0u);
        const uint64_t e0 = k0 * se, z0 = k0 * sv, w0 = k0 * sw;
        for (uint32_t i = tid; i < ec; i += threads) sE[i] = E[e0 + i];
        if constexpr (!INIT)
            for (uint32_t i = tid; i < zc; i += threads) sz[i] = z[z0 + i];
        if constexpr (INIT && CONES)
            for (uint32_t q = tid; q < wc; q += threads) st[q] = w[w0 + q];   // s := w
        __syncthreads();

        if constexpr (!CONES) {
            // phase A: row q of the chunk
            for (uint32_t q = tid; q < wc; q += threads) {
                const T wo = w[w0 + q], yo = y[w0 + q], l = lo[w0 + q];
                T wn, t, h = T(0), kap = T(0);
                if constexpr (!ADJ) h = hi[w0 + q];
                if constexpr (SOFT) kap = kappa[w0 + q];
                if constexpr (INIT) {
                    if constexpr (SOFT)
                        wn = soft_init(wo, l, h, kap);
                    else if constexpr (ADJ)
                        wn = pin(wo, l);
                    else
                        wn = clip(wo, l, h);
                    t = wn - yo;
                } else {
                    const uint32_t kk = q / sw;
                    uint32_t row = q - kk * sw, cols = nx, ld = mx;
                    const T *blk = sE + kk * se, *zz = sz + kk * sv;
                    if (row >= mx) row -= mx, cols = nu, ld = mu, blk += mx * nx, zz += nx;
                    T v = T(0);
                    for (uint32_t j = 0; j < cols; ++j) v = fma_once(blk[j * ld + row], zz[j], v);
                    const T sum = v + yo;
                    T yn;
                    if constexpr (SOFT) {
                        soft_clip(sum, l, h, kap, r, wn, yn);
                    } else {
                        if constexpr (ADJ)
                            wn = pin(sum, l);
                        else
                            wn = clip(sum, l, h);
                        yn = sum - wn;
                    }
                    t = wn - yn;
                    sd[q] = wn - wo;
                    mp = umax(mp, abs_bits(v - wn));
                    y[w0 + q] = yn;
                }
                w[w0 + q] = wn;
                st[q] = t;
            }
        } else {
            // phase A1: row q of the chunk, v and s
            if constexpr (!INIT) {
                for (uint32_t q = tid; q < wc; q += threads) {
                    const uint32_t kk = q / sw;
                    uint32_t row = q - kk * sw, cols = nx, ld = mx, lin = s.lx;
                    const T *blk = sE + kk * se, *zz = sz + kk * sv;
                    if (row >= mx) row -= mx, cols = nu, ld = mu, lin = s.lu, blk += mx * nx, zz += nx;
                    T v = row >= lin ? lo[w0 + q] : T(0);
                    for (uint32_t j = 0; j < cols; ++j) v = fma_once(blk[j * ld + row], zz[j], v);
                    sd[q] = v;
                    st[q] = v + y[w0 + q];
                }
                __syncthreads();
            }

            // phase A2: row q of the chunk again, pass by pass; tp is the t of the pass before, written behind this pass's barrier
            T tp = T(0);
            uint32_t qp = wc;
            for (uint32_t q0 = 0; q0 < wc; q0 += threads) {
                const uint32_t q = q0 + tid;
                T t = T(0);
                if (q < wc) {
                    const T sq = st[q], wo = w[w0 + q];
                    const uint32_t kk = q / sw;
                    uint32_t row = q - kk * sw, lin = s.lx, dim = s.qx;
                    if (row >= mx) row -= mx, lin = s.lu, dim = s.qu;
                    const bool cone = row >= lin;
                    T wn, f = T(0);
                    if (!cone) {
                        wn = clip(sq, lo[w0 + q], hi[w0 + q]);
                    } else {
                        f = lo[w0 + q];
                        const uint32_t pos = (row - lin) % dim;
                        const T *head = st + (q - pos);
                        T n2 = T(0);
                        for (uint32_t i = 1; i < dim; ++i) n2 = fma_once(head[i], head[i], n2);
                        const T a = sqrt_once(n2), s0 = head[0];
                        if (a <= s0) {
                            wn = sq;
                        } else if (a <= -s0) {
                            wn = T(0);
                        } else {
                            const T h = T(0.5) * (s0 + a);
                            const T c = h / a;
                            wn = pos == 0 ? h : c * sq;
                        }
                    }
                    if constexpr (INIT) {
                        t = wn - y[w0 + q];
                    } else {
                        const T yn = sq - wn;
                        t = wn - yn;
                        mp = umax(mp, abs_bits(sd[q] - wn));
                        sd[q] = wn - wo;
                        y[w0 + q] = yn;
                    }
                    if (cone) t = t - f;
                    w[w0 + q] = wn;
                }
                __syncthreads();   // every s of this pass and the one before has been read
                if (qp < wc) st[qp] = tp;
                tp = t, qp = q;
            }
            if (qp < wc) st[qp] = tp;
        }
        __syncthreads();

        // phase B: entry c of the chunk's piece of z
        for (uint32_t c = tid; c < zc; c += threads) {
            const uint32_t kk = c / sv;
            uint32_t col = c - kk * sv, rows = mx;
            const T *blk = sE + kk * se, *tt = st + kk * sw, *dd = sd + kk * sw;
            if (col >= nx) col -= nx, rows = mu, blk += mx * nx, tt += mx, dd += mx;
            blk += col * rows;
            T u = T(0), e = T(0);
            for (uint32_t i = 0; i < rows; ++i) {
                u = fma_once(blk[i], tt[i], u);
                if constexpr (!INIT) e = fma_once(blk[i], dd[i], e);
            }
            gt[z0 + c] = fma_once(-r, u, g[z0 + c]);
            if constexpr (!INIT) md = umax(md, abs_bits(r * e));
        }
        __syncthreads();   // the next chunk overwrites the staging
    }

    if constexpr (!INIT)
        store_norms(mp, md, tid >> 6, tid & 63u, threads >> 6, [&](uint32_t wv) { return slots + 2 * wv; }, res + 2 * (uint64_t)prob);
}

template <typename T, bool INIT, bool CONES, bool SOFT, typename... K>
__global__ __launch_bounds__(256) void admm_rows_update_kernel(RowsShape<CONES> s, const T *__restrict__ g, const T *__restrict__ E,
                                                               const T *__restrict__ lo, const T *__restrict__ hi,
                                                               const T *__restrict__ rho, const T *__restrict__ z, T *__restrict__ w,
                                                               T *__restrict__ y, T *__restrict__ gt, T *__restrict__ res, K... kappa_arg)
{
    rows_update<T, INIT, CONES, SOFT, false>(s, g, E, lo, hi, rho, z, w, y, gt, res, kappa_arg...);
}

// The adjoint of the hard linear rows: yf, the forward y, where lo stands, and no hi.
template <typename T, bool INIT>
__global__ __launch_bounds__(256) void admm_rows_adjoint_kernel(RowsShape<false> s, const T *__restrict__ gz, const T *__restrict__ E,
                                                                const T *__restrict__ yf, const T *__restrict__ rho,
                                                                const T *__restrict__ az, T *__restrict__ w, T *__restrict__ y,
                                                                T *__restrict__ gt, T *__restrict__ res)
{
    rows_update<T, INIT, false, false, true>(s, gz, E, yf, static_cast<const T *>(nullptr), rho, az, w, y, gt, res);
}

template <typename T> bool admm_rows_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
{
    return mx <= 64 && mu <= 64 && rows_per_knot(nx, nu, mx, mu) * sizeof(T) <= kRowsLdsBytes;
}

uint32_t admm_rows_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
{
    const uint64_t kch = kRowsStage / rows_per_knot(nx, nu, mx, mu);
    return (uint32_t)(kch < 1 ? 1 : (kch > kRowsMaxKnots ? kRowsMaxKnots : kch));
}

// The row classes: the linear part within the block, a cone dimension where there are cone rows, whole cones only.
bool admm_rows_classes_ok(uint32_t mx, uint32_t mu, const RowClasses &c)
{
    if (c.lx > mx || c.lu > mu) return false;
    if (c.lx < mx && (c.qx == 0 || (mx - c.lx) % c.qx != 0)) return false;
    if (c.lu < mu && (c.qu == 0 || (mu - c.lu) % c.qu != 0)) return false;
    return true;
}

template <typename T>
hipError_t launch_admm_lin_form(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *G, const T *E,
                                const T *rho, T *Gt, hipStream_t s)
{
    const uint64_t LG = ((uint64_t)nx * nx + (uint64_t)nu * nu) * N - (uint64_t)nu * nu;
    const uint64_t bpp = (LG + 255) / 256;
    if (!admm_rows_shape_ok<T>(nx, nu, mx, mu) || LG >= (1ull << 32) || bpp * batch > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((admm_lin_form_kernel<T>), dim3((uint32_t)(bpp * batch)), dim3(256), 0, s, nx, nu, mx, mu, N, (uint32_t)bpp,
                       G, E, rho, Gt);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_rows_update(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *g,
                                   const T *E, const T *lo, const T *hi, const T *rho, const T *z, T *w, T *y, T *gt, T *res,
                                   hipStream_t s, bool init, bool shared, const RowClasses *cones, const T *kappa, bool adjoint)
{
    if (batch > 0x7fffffffu || !admm_rows_shape_ok<T>(nx, nu, mx, mu) || (cones && !admm_rows_classes_ok(mx, mu, *cones)) ||
        (cones && kappa) || (adjoint && (cones || kappa || shared)))
        return hipErrorInvalidValue;   // one workgroup per problem; cone rows stay hard; the adjoint rows are hard, linear, per problem
    const RowsDims dims{nx, nu, mx, mu};
    RowsWalk walk{N, admm_rows_knot_chunk(nx, nu, mx, mu), shared ? 1u : 0u};
    if (walk.kch > N) walk.kch = N;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu, nw = ((uint64_t)mx + mu) * N - mu;
    const uint32_t threads = (nz > nw ? nz : nw) <= 256 ? 64 : 256;
    const size_t lds = (size_t)walk.kch * rows_per_knot(nx, nu, mx, mu) * sizeof(T);
    auto launch = [&](auto kernel, auto sh, auto... kap) {
        hipLaunchKernelGGL(kernel, dim3(batch), dim3(threads), lds, s, sh, g, E, lo, hi, rho, z, w, y, gt, res, kap...);
    };
    if (adjoint) {   // lo is yf: the mask stands where the bounds stand, hi is not an argument
        const RowsShape<false> sh{dims, {}, walk};
        if (init)
            hipLaunchKernelGGL((admm_rows_adjoint_kernel<T, true>), dim3(batch), dim3(threads), lds, s, sh, g, E, lo, rho, z, w, y, gt, res);
        else
            hipLaunchKernelGGL((admm_rows_adjoint_kernel<T, false>), dim3(batch), dim3(threads), lds, s, sh, g, E, lo, rho, z, w, y, gt, res);
    } else if (cones) {   // (q is ignored where there is no cone row)
        const RowClasses c{cones->lx, cones->lx < mx ? cones->qx : 1u, cones->lu, cones->lu < mu ? cones->qu : 1u};
        const RowsShape<true> sh{dims, c, walk};
        init ? launch(&admm_rows_update_kernel<T, true, true, false>, sh) : launch(&admm_rows_update_kernel<T, false, true, false>, sh);
    } else if (kappa) {   // the soft family: its own instantiations
        const RowsShape<false> sh{dims, {}, walk};
        init ? launch(&admm_rows_update_kernel<T, true, false, true, const T *>, sh, kappa)
             : launch(&admm_rows_update_kernel<T, false, false, true, const T *>, sh, kappa);
    } else {
        const RowsShape<false> sh{dims, {}, walk};
        init ? launch(&admm_rows_update_kernel<T, true, false, false>, sh) : launch(&admm_rows_update_kernel<T, false, false, false>, sh);
    }
    return hipGetLastError();
}

template bool admm_rows_shape_ok<float>(uint32_t, uint32_t, uint32_t, uint32_t);
template bool admm_rows_shape_ok<double>(uint32_t, uint32_t, uint32_t, uint32_t);
template hipError_t launch_admm_lin_form<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                const float *, float *, hipStream_t);
template hipError_t launch_admm_lin_form<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                 const double *, const double *, double *, hipStream_t);
template hipError_t launch_admm_rows_update<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *,
                                                   const float *, const float *, const float *, const float *, const float *, float *,
                                                   float *, float *, float *, hipStream_t, bool, bool, const RowClasses *,
                                                   const float *, bool);
template hipError_t launch_admm_rows_update<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                    const double *, const double *, const double *, const double *, const double *,
                                                    double *, double *, double *, double *, hipStream_t, bool, bool, const RowClasses *,
                                                    const double *, bool);

}  // namespace gbdpcg
