// admm_lin.hip -- ADMM on a kept KKT factorisation with stage-wise LINEAR inequality rows (gbdpcg_admm_lin_form_*,
// gbdpcg_admm_lin_init_*, gbdpcg_admm_lin_update_*, the last launch of gbdpcg_admm_lin_step_*).  Problem b minimises
// 1/2 z'Gz + g'z subject to Cz = c and lo <= E z <= hi, E block-diagonal with the blocks of G: Ex_k (mx x nx) on x_k, Eu_k
// (mu x nu) on u_k, column-major, packed [Ex_0 Eu_0 Ex_1 ... Ex_{N-1}]; the rows, and with them lo, hi, w, y, are packed
// [mx | mu | mx | ... | mx].  The matrices of the solve belong to Gt = G + rho_b E'E, w is the copy of E z that lives between the
// bounds, y the scaled multiplier of E z = w (mu = rho y).  A CHAIN is acc = +0; acc = fma(a_i, b_i, acc) in ascending i; every
// line below is one IEEE operation (the build runs with -ffp-contract=off, the fmas are written out), so every output is defined to
// the bit whatever the launch shape.
//   FORM    P(i,j) = chain over rows r of E(r,i) E(r,j);  Gt(i,j) = fma(rho, P(i,j), G(i,j))     per diagonal block
//   UPDATE  v_r = chain over columns j of E(r,j) z_j;  s = v + y;  w+ = s < lo ? lo : (s > hi ? hi : s);  y+ = s - w+
//           t = w+ - y+;  d = w+ - w;  u_j = chain over rows r of E(r,j) t_r;  e_j likewise with d;  gt_j = fma(-rho, u_j, g_j)
//           res[2b] = max_r |v_r - w+_r|;  res[2b+1] = max_j |rho e_j|        (norm_fold.hpp: over bit patterns, NaN on top)
//   INIT    w <- clip(w), y not written, t = w - y, gt_j = fma(-rho, u_j, g_j); z and res are not looked at.
//
// admm_lin_form_kernel: one lane per entry of Gt, 256 consecutive entries of one problem per workgroup; the entry is read and
// written by the same lane, so Gt may be G.  E is read through the caches (2 m values per entry against one element in, one out);
// the three index divisions per entry are plain divides, next to a chain of m fmas and 2 m loads they are not the cost.
//
// admm_lin_update_kernel: ONE WORKGROUP PER PROBLEM, like admm.hip (the two norms are per problem: nothing crosses a workgroup, no
// atomics, no memset, nothing read from res).  The horizon is walked in chunks of `kch` knots (the host: as many as fit 4096
// staged elements, at most 64).  Per chunk: the chunk's E blocks and its piece of z go to LDS (each one contiguous range of
// memory); PHASE A, lanes own rows: the v chain out of LDS, the clip, w and y written, the primal norm folded, t and d left in
// LDS; barrier; PHASE B, lanes own entries of z: the two column chains out of LDS, gt written, the dual norm folded; barrier.
// Every global access is a scalar one at consecutive addresses across lanes, so the alignment of the base pointers plays no part.
// In phase A consecutive lanes read consecutive rows of a column of E (no bank conflict); in phase B consecutive lanes read
// columns, a stride of mx or mu elements -- a conflict of that order on an LDS read.  Global traffic: per row 4 reads and 2 writes,
// per entry of z 2 reads and 1 write, E once.  Measured at 1024 x (14, 7, 128), 4 + 2 rows (profiles/r11_admm_lin.txt): 31 us in
// fp32, 35 us in fp64 -- 0.46 and 0.77 of the box update's bytes over time, so the fp32 launch is not at its memory bound yet.
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

constexpr uint32_t kLinStage = 4096;          // elements staged per chunk (E, z, t, d together), unless one knot needs more
constexpr uint32_t kLinMaxKnots = 64;         // knots per chunk at most
constexpr size_t kLinLdsBytes = 60 * 1024;    // what one knot may take at the outside (64 KB less the norm slots and slack)

struct LinShape {
    uint32_t nx, nu, mx, mu, N;
    uint32_t kch;        // knots per chunk
    uint32_t shared;     // E is one problem's
};

__device__ __forceinline__ float fma_once(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_once(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T> __device__ __forceinline__ T clip(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }

uint64_t lin_per_knot(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
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

template <typename T, bool INIT>
__global__ __launch_bounds__(256) void admm_lin_update_kernel(LinShape s, const T *__restrict__ g, const T *__restrict__ E,
                                                              const T *__restrict__ lo, const T *__restrict__ hi,
                                                              const T *__restrict__ rho, const T *__restrict__ z, T *__restrict__ w,
                                                              T *__restrict__ y, T *__restrict__ gt, T *__restrict__ res)
{
    using U = decltype(abs_bits(T(0)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lin_lds[];
    __shared__ U slots[8];   // two words per wave
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = mx * nx + mu * nu;
    T *sE = reinterpret_cast<T *>(lin_lds);   // the chunk's E blocks | its piece of z | t | d
    T *sz = sE + kch * se, *st = sz + kch * sv, *sd = st + kch * sw;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t nz = (uint64_t)sv * N - nu, nw = (uint64_t)sw * N - mu, ne = (uint64_t)se * N - mu * nu;
    g += prob * nz, gt += prob * nz, lo += prob * nw, hi += prob * nw, w += prob * nw, y += prob * nw;
    if constexpr (!INIT) z += prob * nz;
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
        __syncthreads();

        // phase A: row q of the chunk
        for (uint32_t q = tid; q < wc; q += threads) {
            const T wo = w[w0 + q], yo = y[w0 + q], l = lo[w0 + q], h = hi[w0 + q];
            T wn, t;
            if constexpr (INIT) {
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
                wn = clip(sum, l, h);
                const T yn = sum - wn;
                t = wn - yn;
                sd[q] = wn - wo;
                mp = umax(mp, abs_bits(v - wn));
                y[w0 + q] = yn;
            }
            w[w0 + q] = wn;
            st[q] = t;
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

template <typename T> bool admm_lin_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
{
    return mx <= 64 && mu <= 64 && lin_per_knot(nx, nu, mx, mu) * sizeof(T) <= kLinLdsBytes;
}

uint32_t admm_lin_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
{
    const uint64_t kch = kLinStage / lin_per_knot(nx, nu, mx, mu);
    return (uint32_t)(kch < 1 ? 1 : (kch > kLinMaxKnots ? kLinMaxKnots : kch));
}

template <typename T>
hipError_t launch_admm_lin_form(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *G, const T *E,
                                const T *rho, T *Gt, hipStream_t s)
{
    const uint64_t LG = ((uint64_t)nx * nx + (uint64_t)nu * nu) * N - (uint64_t)nu * nu;
    const uint64_t bpp = (LG + 255) / 256;
    if (!admm_lin_shape_ok<T>(nx, nu, mx, mu) || LG >= (1ull << 32) || bpp * batch > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((admm_lin_form_kernel<T>), dim3((uint32_t)(bpp * batch)), dim3(256), 0, s, nx, nu, mx, mu, N, (uint32_t)bpp,
                       G, E, rho, Gt);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_lin_update(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *g, const T *E,
                                  const T *lo, const T *hi, const T *rho, const T *z, T *w, T *y, T *gt, T *res, hipStream_t s,
                                  bool init, bool shared)
{
    if (batch > 0x7fffffffu || !admm_lin_shape_ok<T>(nx, nu, mx, mu)) return hipErrorInvalidValue;   // one workgroup per problem
    LinShape sh;
    sh.nx = nx, sh.nu = nu, sh.mx = mx, sh.mu = mu, sh.N = N, sh.shared = shared ? 1u : 0u;
    sh.kch = admm_lin_knot_chunk(nx, nu, mx, mu);
    if (sh.kch > N) sh.kch = N;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu, nw = ((uint64_t)mx + mu) * N - mu;
    const uint32_t threads = (nz > nw ? nz : nw) <= 256 ? 64 : 256;
    const size_t lds = (size_t)sh.kch * lin_per_knot(nx, nu, mx, mu) * sizeof(T);
    if (init)
        hipLaunchKernelGGL((admm_lin_update_kernel<T, true>), dim3(batch), dim3(threads), lds, s, sh, g, E, lo, hi, rho, z, w, y, gt, res);
    else
        hipLaunchKernelGGL((admm_lin_update_kernel<T, false>), dim3(batch), dim3(threads), lds, s, sh, g, E, lo, hi, rho, z, w, y, gt, res);
    return hipGetLastError();
}

template bool admm_lin_shape_ok<float>(uint32_t, uint32_t, uint32_t, uint32_t);
template bool admm_lin_shape_ok<double>(uint32_t, uint32_t, uint32_t, uint32_t);
template hipError_t launch_admm_lin_form<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                const float *, float *, hipStream_t);
template hipError_t launch_admm_lin_form<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                 const double *, const double *, double *, hipStream_t);
template hipError_t launch_admm_lin_update<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                  const float *, const float *, const float *, const float *, float *, float *, float *,
                                                  float *, hipStream_t, bool, bool);
template hipError_t launch_admm_lin_update<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                   const double *, const double *, const double *, const double *, const double *,
                                                   double *, double *, double *, double *, hipStream_t, bool, bool);

}  // namespace gbdpcg
