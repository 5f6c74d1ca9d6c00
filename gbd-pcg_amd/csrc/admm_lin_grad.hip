// admm_lin_grad.hip -- the gradients in the rows of the hard linear-row QP of admm_rows.hip (gbdpcg_admm_lin_grad_*), the last
// launch but one of its backward pass.  The forward problem is min 1/2 z'Gz + g'z, Cz = c, lo <= Ez <= hi with the stationarity
// G z + g + C'lambda + rho E'yf = 0 (yf the forward y, mu = rho yf); the adjoint loop (gbdpcg_admm_lin_adjoint_*) leaves az, its z, and
// ya, its y (nu = rho ya).  Row r is active iff yf_r != 0 (a NaN included), at lo where yf_r < 0, at hi where yf_r > 0.  Per problem b:
//     glo_r = yf_r < 0 ? -(rho_b ya_r) : +0        ghi_r = yf_r > 0 ? -(rho_b ya_r) : +0        (the lines of admm_grad_bounds_kernel)
//     p = ya_r z_j;   q = fma(yf_r, az_j, p);   gE(r, j) = yf_r != 0 ? rho_b q : +0            per block, in the layout of E
// every line ONE IEEE operation or a comparison (ieee_once.hpp), so every output is defined to the bit whatever the launch shape.
// glo, ghi have the layout of the rows [mx | mu | mx | ... | mx], gE that of E ([Ex_0 Eu_0 Ex_1 ... Ex_{N-1}], column-major blocks).
//
// admm_lin_grad_kernel: write-bound through gE ((mx nx + mu nu) N - mu nu elements out per problem against 2 (nz + nw) in).  ONE
// WORKGROUP PER PROBLEM, 64-bit problem strides, the horizon in chunks of `kch` knots (as many as fit 4096 staged elements, at most
// 64).  Per chunk the pieces of z, az, yf, ya go to LDS (each one contiguous range of memory), then the lanes walk the chunk's
// outputs in storage order -- the range of gE, of glo, of ghi, each contiguous -- through store_range (grad_store.hpp): a scalar
// head up to the first 16-byte boundary of the ADDRESS, 16-byte stores, a scalar tail; the same operations per element whichever
// store carries it, so the bits do not depend on the alignment of the bases.  Every output is written exactly once by one lane: no
// atomics, no memset, no scratch.  The element -> (knot, column, row) maps multiply by reciprocals the host prepared.
// In a column-major block consecutive elements are consecutive ROWS of a column: yf_r, ya_r vary per lane, z_j, az_j are LDS
// broadcasts (or two addresses where a wave straddles a column).  A lane owns the 4 (fp64: 2) consecutive elements of its 16-byte
// store, so neighbouring lanes read yf, ya 4 (2) elements apart: a 4-way conflict on a 4-byte LDS read (32 banks per half wave), 2-way
// on an 8-byte one.  That is 8 conflicted and 8 broadcast reads per 1 KB a wave stores -- about 40 LDS cycles, 25 B/clk per CU, twice
// what a CU's share of the memory system takes -- so the stores stay the bound and the rows are not re-laid out in LDS.
//
// SOFT (gbdpcg_admm_lin_soft_grad_*, a compile-time switch; the hard instantiation holds nothing of it): the rows of the soft QP,
// whose forward y splits them into free, held and saturated (admm_box_grad.hip).  With theta_r = kappa_r / rho_b (the division of
// soft_clip, once per row into a fifth LDS piece) and sat = |yf_r| >= theta_r:
//     glo_r = (yf_r < 0 && !sat) ? -(rho_b ya_r) : +0      ghi_r likewise with > 0         the lines of admm_soft_grad_bounds_kernel
//     gE(r, j): the lines above with the UNMASKED yf -- a saturated row keeps rho yf_r az_j (its ya_r is 0 behind the masked adjoint)
//     gkappa_r = sat ? (yf_r > 0 ? v : -v) : +0,   v the chain fma(E(r, j), az_j, acc) over the block's columns in ascending j, seed +0
// gkappa is the one output whose lanes own ROWS (phase A of admm_rows.hip): nw elements against gE's ne, scalar stores at
// consecutive addresses.  The lane reads its row of E straight from global memory -- consecutive lanes read consecutive rows of a
// column, a saturated row's entries once, the others never -- and az out of the staging; E takes no LDS.
#include "grad_store.hpp"
#include "ieee_once.hpp"
#include "internal.hpp"

namespace gbdpcg {

namespace {

constexpr uint32_t kLinGradStage = 4096;   // elements staged per chunk (z, az, yf, ya together), unless one knot needs more

struct LinGradShape {
    uint32_t nx, nu, mx, mu, N;
    uint32_t kch;                 // knots per chunk
    uint32_t m_se, m_mx, m_mu;    // magic() of the three divisors
};

}  // namespace

// The arguments the SOFT instantiation adds, ONE member of the kernel's trailing parameter pack (empty in the hard instantiation,
// which therefore takes the arguments, and compiles to the code, of a kernel that knows nothing of kappa; ieee_once.hpp).
template <typename T> struct SoftRows {
    const T *E;
    const T *kappa;
    T *gkappa;
};
template <typename S> __device__ __forceinline__ const S &only_of(const S &s) { return s; }

template <typename T, bool SOFT, typename... K>
__global__ __launch_bounds__(256) void admm_lin_grad_kernel(LinGradShape s, const T *__restrict__ z, const T *__restrict__ az,
                                                            const T *__restrict__ yf, const T *__restrict__ ya,
                                                            const T *__restrict__ rho, T *__restrict__ glo, T *__restrict__ ghi,
                                                            T *__restrict__ gE, K... soft_arg)
{
    static_assert(sizeof...(K) == (SOFT ? 1 : 0), "E, kappa and gkappa are arguments of the soft instantiation alone");
    extern __shared__ __attribute__((aligned(16))) unsigned char lin_grad_lds[];
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = mx * nx + mu * nu;
    T *sz = reinterpret_cast<T *>(lin_grad_lds);   // the chunk's pieces of z | az | yf | ya (| theta: SOFT)
    T *sa = sz + kch * sv, *sf = sa + kch * sv, *sy = sf + kch * sw;
    [[maybe_unused]] T *sk = sy + kch * sw;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t nz = (uint64_t)sv * N - nu, nw = (uint64_t)sw * N - mu, ne = (uint64_t)se * N - mu * nu;
    z += prob * nz, az += prob * nz, yf += prob * nw, ya += prob * nw;
    [[maybe_unused]] const T *__restrict__ E = nullptr, *__restrict__ kappa = nullptr;
    [[maybe_unused]] T *__restrict__ gk = nullptr;
    if constexpr (SOFT) {
        const SoftRows<T> &sr = only_of(soft_arg...);
        E = sr.E + prob * ne, kappa = sr.kappa + prob * nw, gk = sr.gkappa;
    }
    const T r = rho[prob];

    for (uint64_t k0 = 0; k0 < N; k0 += kch) {
        const uint32_t kc = (uint32_t)(N - k0 < kch ? N - k0 : kch);
        const bool end = k0 + kc == N;   // the last knot of the horizon has no u: no Eu block, no u rows
        const uint32_t ec = kc * se - (end ? mu * nu : 0u), zc = kc * sv - (end ? nu : 0u), wc = kc * sw - (end ? mu : 0u);
        const uint64_t e0 = k0 * se, z0 = k0 * sv, w0 = k0 * sw;
        if (gE || (SOFT && gk))
            for (uint32_t i = tid; i < zc; i += threads) sz[i] = z[z0 + i], sa[i] = az[z0 + i];
        for (uint32_t i = tid; i < wc; i += threads) {
            sf[i] = yf[w0 + i], sy[i] = ya[w0 + i];
            if constexpr (SOFT) sk[i] = kappa[w0 + i] / r;   // theta, the division of soft_clip
        }
        __syncthreads();

        if (gE)
            store_range<T>(gE + prob * ne + e0, ec, tid, threads, [&](uint32_t f) {
                const uint32_t kk = fast_div(f, se, s.m_se);
                uint32_t e = f - kk * se, ld = mx, m = s.m_mx;
                const T *zz = sz + kk * sv, *aa = sa + kk * sv, *ff = sf + kk * sw, *yy = sy + kk * sw;
                if (e >= mx * nx) e -= mx * nx, ld = mu, m = s.m_mu, zz += nx, aa += nx, ff += mx, yy += mx;
                const uint32_t j = fast_div(e, ld, m), row = e - j * ld;
                const T fr = ff[row];
                const T p = yy[row] * zz[j];
                const T q = fma_once(fr, aa[j], p);
                return fr != T(0) ? r * q : T(0);
            });
        if (glo)
            store_range<T>(glo + prob * nw + w0, wc, tid, threads, [&](uint32_t f) {
                const T n = -(r * sy[f]);
                if constexpr (SOFT)
                    return (sf[f] < T(0) && !(abs_once(sf[f]) >= sk[f])) ? n : T(0);
                else
                    return sf[f] < T(0) ? n : T(0);
            });
        if (ghi)
            store_range<T>(ghi + prob * nw + w0, wc, tid, threads, [&](uint32_t f) {
                const T n = -(r * sy[f]);
                if constexpr (SOFT)
                    return (sf[f] > T(0) && !(abs_once(sf[f]) >= sk[f])) ? n : T(0);
                else
                    return sf[f] > T(0) ? n : T(0);
            });
        if constexpr (SOFT) {
            // lanes own rows, as in phase A of admm_rows.hip: the chain of a saturated row over its block's columns, E out of global memory
            if (gk)
                for (uint32_t q = tid; q < wc; q += threads) {
                    const T f = sf[q];
                    T out = T(0);
                    if (abs_once(f) >= sk[q]) {
                        const uint32_t kk = q / sw;
                        uint32_t row = q - kk * sw, cols = nx, ld = mx;
                        const T *blk = E + e0 + (uint64_t)kk * se, *aa = sa + kk * sv;
                        if (row >= mx) row -= mx, cols = nu, ld = mu, blk += mx * nx, aa += nx;
                        T v = T(0);
                        for (uint32_t j = 0; j < cols; ++j) v = fma_once(blk[j * ld + row], aa[j], v);
                        out = f > T(0) ? v : -v;
                    }
                    gk[prob * nw + w0 + q] = out;
                }
        }
        __syncthreads();   // the next chunk overwrites the staging
    }
}

// kappa != null: the SOFT instantiation (E, kappa read, gkappa written where not null); null: the hard one, E and gkappa not looked at.
template <typename T>
hipError_t launch_admm_lin_grad(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *z, const T *az,
                                const T *yf, const T *ya, const T *rho, T *glo, T *ghi, T *gE, hipStream_t s, const T *E,
                                const T *kappa, T *gkappa)
{
    const bool soft = kappa != nullptr;
    if (batch > 0x7fffffffu || !admm_rows_shape_ok<T>(nx, nu, mx, mu) || (!glo && !ghi && !gE && !(soft && gkappa)) || (soft && !E))
        return hipErrorInvalidValue;   // one workgroup per problem
    const uint64_t sv = (uint64_t)nx + nu, sw = (uint64_t)mx + mu, se = (uint64_t)mx * nx + (uint64_t)mu * nu;
    const uint64_t per = 2 * (sv + sw) + (soft ? sw : 0);   // (SOFT: theta next to yf, ya)
    uint64_t kch = kLinGradStage / per;
    kch = kch < 1 ? 1 : (kch > 64 ? 64 : kch);
    kch = kch > N ? N : kch;
    LinGradShape g;
    g.nx = nx, g.nu = nu, g.mx = mx, g.mu = mu, g.N = N, g.kch = (uint32_t)kch;
    g.m_se = magic((uint32_t)se, kch * se), g.m_mx = magic(mx, se), g.m_mu = magic(mu, se);
    const uint64_t ne = se * N - (uint64_t)mu * nu, nw = sw * N - mu;
    const uint32_t threads = (ne > nw ? ne : nw) <= 256 ? 64 : 256;
    const size_t lds = (size_t)(kch * per * sizeof(T));
    if (soft) {
        if (lds > 64 * 1024) return hipErrorInvalidValue;   // a knot whose five pieces do not fit the default LDS window
        const SoftRows<T> sr{E, kappa, gkappa};
        hipLaunchKernelGGL((admm_lin_grad_kernel<T, true, SoftRows<T>>), dim3(batch), dim3(threads), lds, s, g, z, az, yf, ya, rho, glo,
                           ghi, gE, sr);
    } else {
        hipLaunchKernelGGL((admm_lin_grad_kernel<T, false>), dim3(batch), dim3(threads), lds, s, g, z, az, yf, ya, rho, glo, ghi, gE);
    }
    return hipGetLastError();
}

template hipError_t launch_admm_lin_grad<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                const float *, const float *, const float *, float *, float *, float *, hipStream_t,
                                                const float *, const float *, float *);
template hipError_t launch_admm_lin_grad<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                 const double *, const double *, const double *, const double *, double *, double *,
                                                 double *, hipStream_t, const double *, const double *, double *);

}  // namespace gbdpcg
