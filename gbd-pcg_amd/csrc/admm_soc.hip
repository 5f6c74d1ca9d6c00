// admm_soc.hip -- ADMM on a kept KKT factorisation with stage-wise rows that are LINEAR (lo <= (E z)_r <= hi) or lie in SECOND-ORDER
// CONES ((E z + f)_cone in K_q = {(s_0, s_1 .. s_{q-1}) : ||(s_1 .. s_{q-1})||_2 <= s_0}): gbdpcg_admm_soc_init_*,
// gbdpcg_admm_soc_update_*, the last launch of gbdpcg_admm_soc_step_*.  E, its layout, the packing of the rows, w, y, gt, rho and res
// are those of admm_lin.hip, and so is Gt = G + rho E'E (gbdpcg_admm_lin_form_* does not look at the set the rows are projected on).
// In every x block the first lx rows are linear, the other mx - lx rows are consecutive cones of dimension qx, head row first; lu, qu
// likewise for the u blocks.  On a cone row lo[r] holds the offset f_r and hi[r] is NOT READ.  Every line is one IEEE operation or a
// comparison (-ffp-contract=off, the fmas written out, / and sqrt correctly rounded), every chain runs in ascending index order:
//   UPDATE  linear row: the lines of admm_lin.hip.
//           cone row:   v_r = chain over columns j of E(r,j) z_j SEEDED with f_r;  s_r = v_r + y_r
//           per cone:   n2 = chain over i = 1 .. q-1 of s_i s_i;  a = sqrt(n2)
//                       a <= s_0: w+ = s;   else a <= -s_0: w+ = +0;   else h = 0.5 (s_0 + a), c = h / a, w+_0 = h, w+_i = c s_i
//           y+ = s - w+;  t = (w+ - y+) - f;  d = w+ - w;  then u, e, gt, res as in admm_lin.hip (res[2b] over |v_r - w+_r|)
//   INIT    w <- projection of w by the same lines with s := w, y not written, t = (w - y) - f; z and res are not looked at.
// A NaN fails both comparisons and stays NaN through the third branch; q = 1 is the half-line s_0 >= 0 (an empty chain, a = +0).
//
// admm_soc_update_kernel keeps the shape of admm_lin_update_kernel: one workgroup per problem, the horizon in the same chunks of
// knots, the chunk's E blocks and its piece of z staged in LDS once, the same LDS budget (E | z | two slots per row), no atomics,
// no memset, no scratch, nothing read from res, scalar coalesced global accesses, one code path.  Phase A is split in two:
//   A1  lanes own rows: v and s go to the row's two LDS slots (v where d will be, s where t will be).   barrier.
//   A2  lanes own rows again, in passes of blockDim.x rows.  A linear row is clipped; a cone row runs its cone's n2 chain over the
//       s slots in ascending order -- every lane of a cone holds identical bits, q LDS reads per row instead of a second ownership
//       map -- and writes only its own w, y, d.  Its t has to replace an s that other lanes of the cone still read, and a cone may
//       straddle two passes: so a pass is closed by a barrier, and the t of a pass is written behind the barrier of the NEXT pass
//       (a cone has at most 64 rows, it never reaches two passes back).  One carried register, one barrier per pass.
// Row -> (cone, position) is index arithmetic on lx, qx, lu, qu.  Phase B is that of admm_lin.hip.
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

struct SocShape {
    uint32_t nx, nu, mx, mu, lx, qx, lu, qu, N;
    uint32_t kch;        // knots per chunk (admm_lin_knot_chunk)
    uint32_t shared;     // E is one problem's
};

__device__ __forceinline__ float fma_once(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_once(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sqrt_once(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_once(double a) { return __builtin_sqrt(a); }

template <typename T> __device__ __forceinline__ T clip(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }

// what one knot takes of the staging: lin_per_knot of admm_lin.hip
uint64_t soc_per_knot(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu)
{
    return (uint64_t)mx * nx + (uint64_t)mu * nu + nx + nu + 2ull * (mx + mu);
}

}  // namespace

template <typename T, bool INIT>
__global__ __launch_bounds__(256) void admm_soc_update_kernel(SocShape s, const T *__restrict__ g, const T *__restrict__ E,
                                                              const T *__restrict__ lo, const T *__restrict__ hi,
                                                              const T *__restrict__ rho, const T *__restrict__ z, T *__restrict__ w,
                                                              T *__restrict__ y, T *__restrict__ gt, T *__restrict__ res)
{
    using U = decltype(abs_bits(T(0)));
    extern __shared__ __attribute__((aligned(16))) unsigned char soc_lds[];
    __shared__ U slots[8];   // two words per wave
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = mx * nx + mu * nu;
    T *sE = reinterpret_cast<T *>(soc_lds);   // the chunk's E blocks | its piece of z | s, then t | v, then d
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
        if constexpr (INIT)
            for (uint32_t q = tid; q < wc; q += threads) st[q] = w[w0 + q];   // s := w
        __syncthreads();

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

// The row classes: the linear part within the block, a cone dimension where there are cone rows, whole cones only.
bool admm_soc_classes_ok(uint32_t mx, uint32_t mu, uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu)
{
    if (lx > mx || lu > mu) return false;
    if (lx < mx && (qx == 0 || (mx - lx) % qx != 0)) return false;
    if (lu < mu && (qu == 0 || (mu - lu) % qu != 0)) return false;
    return true;
}

template <typename T>
hipError_t launch_admm_soc_update(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu,
                                  uint32_t N, uint32_t batch, const T *g, const T *E, const T *lo, const T *hi, const T *rho, const T *z,
                                  T *w, T *y, T *gt, T *res, hipStream_t s, bool init, bool shared)
{
    if (batch > 0x7fffffffu || !admm_lin_shape_ok<T>(nx, nu, mx, mu) || !admm_soc_classes_ok(mx, mu, lx, qx, lu, qu))
        return hipErrorInvalidValue;   // one workgroup per problem
    SocShape sh;
    sh.nx = nx, sh.nu = nu, sh.mx = mx, sh.mu = mu, sh.N = N, sh.shared = shared ? 1u : 0u;
    sh.lx = lx, sh.lu = lu, sh.qx = lx < mx ? qx : 1u, sh.qu = lu < mu ? qu : 1u;   // (ignored where there is no cone row)
    sh.kch = admm_lin_knot_chunk(nx, nu, mx, mu);
    if (sh.kch > N) sh.kch = N;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu, nw = ((uint64_t)mx + mu) * N - mu;
    const uint32_t threads = (nz > nw ? nz : nw) <= 256 ? 64 : 256;
    const size_t lds = (size_t)sh.kch * soc_per_knot(nx, nu, mx, mu) * sizeof(T);
    if (init)
        hipLaunchKernelGGL((admm_soc_update_kernel<T, true>), dim3(batch), dim3(threads), lds, s, sh, g, E, lo, hi, rho, z, w, y, gt, res);
    else
        hipLaunchKernelGGL((admm_soc_update_kernel<T, false>), dim3(batch), dim3(threads), lds, s, sh, g, E, lo, hi, rho, z, w, y, gt, res);
    return hipGetLastError();
}

template hipError_t launch_admm_soc_update<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                                                  uint32_t, const float *, const float *, const float *, const float *, const float *,
                                                  const float *, float *, float *, float *, float *, hipStream_t, bool, bool);
template hipError_t launch_admm_soc_update<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                                                   uint32_t, uint32_t, const double *, const double *, const double *, const double *,
                                                   const double *, const double *, double *, double *, double *, double *, hipStream_t,
                                                   bool, bool);

}  // namespace gbdpcg
