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

template <typename T>
__global__ __launch_bounds__(256) void admm_lin_grad_kernel(LinGradShape s, const T *__restrict__ z, const T *__restrict__ az,
                                                            const T *__restrict__ yf, const T *__restrict__ ya,
                                                            const T *__restrict__ rho, T *__restrict__ glo, T *__restrict__ ghi,
                                                            T *__restrict__ gE)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lin_grad_lds[];
    const uint32_t nx = s.nx, nu = s.nu, mx = s.mx, mu = s.mu, N = s.N, kch = s.kch;
    const uint32_t sv = nx + nu, sw = mx + mu, se = mx * nx + mu * nu;
    T *sz = reinterpret_cast<T *>(lin_grad_lds);   // the chunk's pieces of z | az | yf | ya
    T *sa = sz + kch * sv, *sf = sa + kch * sv, *sy = sf + kch * sw;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t nz = (uint64_t)sv * N - nu, nw = (uint64_t)sw * N - mu, ne = (uint64_t)se * N - mu * nu;
    z += prob * nz, az += prob * nz, yf += prob * nw, ya += prob * nw;
    const T r = rho[prob];

    for (uint64_t k0 = 0; k0 < N; k0 += kch) {
        const uint32_t kc = (uint32_t)(N - k0 < kch ? N - k0 : kch);
        const bool end = k0 + kc == N;   // the last knot of the horizon has no u: no Eu block, no u rows
        const uint32_t ec = kc * se - (end ? mu * nu : 0u), zc = kc * sv - (end ? nu : 0u), wc = kc * sw - (end ? mu : 0u);
        const uint64_t e0 = k0 * se, z0 = k0 * sv, w0 = k0 * sw;
        if (gE)
            for (uint32_t i = tid; i < zc; i += threads) sz[i] = z[z0 + i], sa[i] = az[z0 + i];
        for (uint32_t i = tid; i < wc; i += threads) sf[i] = yf[w0 + i], sy[i] = ya[w0 + i];
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
                return sf[f] < T(0) ? n : T(0);
            });
        if (ghi)
            store_range<T>(ghi + prob * nw + w0, wc, tid, threads, [&](uint32_t f) {
                const T n = -(r * sy[f]);
                return sf[f] > T(0) ? n : T(0);
            });
        __syncthreads();   // the next chunk overwrites the staging
    }
}

template <typename T>
hipError_t launch_admm_lin_grad(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *z, const T *az,
                                const T *yf, const T *ya, const T *rho, T *glo, T *ghi, T *gE, hipStream_t s)
{
    if (batch > 0x7fffffffu || !admm_rows_shape_ok<T>(nx, nu, mx, mu) || (!glo && !ghi && !gE))
        return hipErrorInvalidValue;   // one workgroup per problem
    const uint64_t sv = (uint64_t)nx + nu, sw = (uint64_t)mx + mu, se = (uint64_t)mx * nx + (uint64_t)mu * nu;
    const uint64_t per = 2 * (sv + sw);
    uint64_t kch = kLinGradStage / per;
    kch = kch < 1 ? 1 : (kch > 64 ? 64 : kch);
    kch = kch > N ? N : kch;
    LinGradShape g;
    g.nx = nx, g.nu = nu, g.mx = mx, g.mu = mu, g.N = N, g.kch = (uint32_t)kch;
    g.m_se = magic((uint32_t)se, kch * se), g.m_mx = magic(mx, se), g.m_mu = magic(mu, se);
    const uint64_t ne = se * N - (uint64_t)mu * nu, nw = sw * N - mu;
    const uint32_t threads = (ne > nw ? ne : nw) <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_lin_grad_kernel<T>), dim3(batch), dim3(threads), (size_t)(kch * per * sizeof(T)), s, g, z, az, yf, ya, rho,
                       glo, ghi, gE);
    return hipGetLastError();
}

template hipError_t launch_admm_lin_grad<float>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                const float *, const float *, const float *, float *, float *, float *, hipStream_t);
template hipError_t launch_admm_lin_grad<double>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                 const double *, const double *, const double *, const double *, double *, double *,
                                                 double *, hipStream_t);

}  // namespace gbdpcg
