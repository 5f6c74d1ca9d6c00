// admm_soft_grad.hip -- the elementwise launches of the backward pass of the SOFT (L1-penalised) box and rows QPs
// (gbdpcg_admm_soft_mask_*, gbdpcg_admm_lin_soft_mask_*, gbdpcg_admm_soft_grad_bounds_*).  Behind a soft update (soft_clip in
// ieee_once.hpp) the forward y (yf, read only) splits the rows of problem b into three sets, with theta_r = kappa_r / rho_b the ONE
// correctly rounded division of the update:
//     free        yf_r == 0                          inside its bounds, mu_r = 0
//     held        yf_r != 0 and |yf_r| < theta_r     on a bound, |mu_r| < kappa_r             (a NaN yf_r fails the comparison: held)
//     saturated   |yf_r| >= theta_r                  beyond its bound, mu_r = +-kappa_r: the update wrote +-theta itself
// A saturated multiplier does not move with z, so in the adjoint problem the row is as free as an inactive one: the adjoint is
// the HARD adjoint loop (admm_adjoint.hip, the adjoint rows of admm_rows.hip) on the masked copy
//     ym_r = |yf_r| >= theta_r ? +0 : yf_r
// A tie |e| = theta takes the third branch of soft_clip with y = +-theta: saturated, that is free -- the convention of the weakly
// active row.  kappa = +Inf: ym has the bits of yf (nothing finite reaches theta); kappa = 0: theta = 0 and ym = +0 everywhere.
// rho must be the rho of the update that wrote yf: behind a rebalance with no update after it y has been rescaled and no longer
// sits on the theta of either rho.
//
// Bound gradients of the soft box (gbdpcg_admm_soft_grad_bounds_*), ya the adjoint's y (nu = rho ya), az the adjoint's z, with
// sat = |yf| >= theta, every line ONE IEEE operation or a comparison:
//     glo = (yf < 0 && !sat) ? -(rho_b ya) : +0      ghi = (yf > 0 && !sat) ? -(rho_b ya) : +0      the bits of admm_grad_bounds on ym
//     gkappa = sat ? (yf > 0 ? az : -az) : +0        mu_r = sign(yf_r) kappa_r enters the stationarity like g: dl/dkappa_r = sign a_z,r
//
// Shape: that of admm_grad_bounds_kernel -- ONE WORKGROUP PER PROBLEM, one wave when the problem has at most 256 elements, otherwise
// four, 64-bit problem strides, rho_b once per workgroup through the scalar cache, no LDS, no atomics, no scratch.  With every base
// pointer in use 16-byte aligned (vec != 0, decided by the host) a scalar head, a 16-byte body and a scalar tail, otherwise every
// element through the scalar form; the same operations per element either way: the same bits.  The mask makes 3 element accesses
// per element (2 reads, 1 write), the gradients 4 reads and up to 3 writes.  One mask kernel serves the box (nz elements per
// problem) and the rows (nw).
#include "elementwise_split.hpp"
#include "ieee_once.hpp"
#include "internal.hpp"

namespace gbdpcg {

template <typename T>
__global__ __launch_bounds__(256) void admm_soft_mask_kernel(uint64_t len, uint32_t vec, const T *__restrict__ yf,
                                                             const T *__restrict__ kappa, const T *__restrict__ rho,
                                                             T *__restrict__ ym)
{
    using V = typename AdjVec<T>::type;
    constexpr uint32_t VN = AdjVec<T>::N;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t off = (uint64_t)prob * len;
    yf += off, kappa += off, ym += off;
    const T r = rho[prob];

    auto element = [&](T f, T k) { return soft_saturated(f, k, r) ? T(0) : f; };

    uint64_t head, body;
    split<VN>(vec, off, len, head, body);
    if (tid < head) ym[tid] = element(yf[tid], kappa[tid]);
    for (uint64_t q = tid; q < body; q += threads) {
        const uint64_t i = head + q * VN;
        const V fv = *reinterpret_cast<const V *>(yf + i), kv = *reinterpret_cast<const V *>(kappa + i);
        V mv;
#pragma unroll
        for (uint32_t e = 0; e < VN; ++e) mv[e] = element(fv[e], kv[e]);
        *reinterpret_cast<V *>(ym + i) = mv;
    }
    for (uint64_t i = head + body * VN + tid; i < len; i += threads) ym[i] = element(yf[i], kappa[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void admm_soft_grad_bounds_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ yf,
                                                                    const T *__restrict__ kappa, const T *__restrict__ rho,
                                                                    const T *__restrict__ ya, const T *__restrict__ az,
                                                                    T *__restrict__ glo, T *__restrict__ ghi, T *__restrict__ gk)
{
    using V = typename AdjVec<T>::type;
    constexpr uint32_t VN = AdjVec<T>::N;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t off = (uint64_t)prob * nz;
    yf += off, kappa += off, ya += off, az += off;
    if (glo) glo += off;
    if (ghi) ghi += off;
    if (gk) gk += off;
    const T r = rho[prob];

    auto element = [&](T f, T k, T a, T z, T &lo, T &hi, T &gkap) {
        const bool sat = soft_saturated(f, k, r);
        const T n = -(r * a);
        lo = (f < T(0) && !sat) ? n : T(0);
        hi = (f > T(0) && !sat) ? n : T(0);
        gkap = sat ? (f > T(0) ? z : -z) : T(0);
    };
    auto scalar = [&](uint64_t i) {
        T lo, hi, gkap;
        element(yf[i], kappa[i], ya[i], az[i], lo, hi, gkap);
        if (glo) glo[i] = lo;
        if (ghi) ghi[i] = hi;
        if (gk) gk[i] = gkap;
    };

    uint64_t head, body;
    split<VN>(vec, off, nz, head, body);
    if (tid < head) scalar(tid);
    for (uint64_t q = tid; q < body; q += threads) {
        const uint64_t i = head + q * VN;
        const V fv = *reinterpret_cast<const V *>(yf + i), kv = *reinterpret_cast<const V *>(kappa + i);
        const V av = *reinterpret_cast<const V *>(ya + i), zv = *reinterpret_cast<const V *>(az + i);
        V lv, hv, gv;
#pragma unroll
        for (uint32_t e = 0; e < VN; ++e) {
            T lo, hi, gkap;
            element(fv[e], kv[e], av[e], zv[e], lo, hi, gkap);
            lv[e] = lo;
            hv[e] = hi;
            gv[e] = gkap;
        }
        if (glo) *reinterpret_cast<V *>(glo + i) = lv;
        if (ghi) *reinterpret_cast<V *>(ghi + i) = hv;
        if (gk) *reinterpret_cast<V *>(gk + i) = gv;
    }
    for (uint64_t i = head + body * VN + tid; i < nz; i += threads) scalar(i);
}

template <typename T>
hipError_t launch_admm_soft_mask(uint64_t len, uint32_t batch, const T *yf, const T *kappa, const T *rho, T *ym, hipStream_t s)
{
    if (batch > 0x7fffffffu || ym == yf) return hipErrorInvalidValue;   // one workgroup per problem; the unmasked yf is needed afterwards
    const uint32_t vec = all_aligned({yf, kappa, ym});
    const uint32_t threads = len <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_soft_mask_kernel<T>), dim3(batch), dim3(threads), 0, s, len, vec, yf, kappa, rho, ym);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_soft_grad_bounds(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *yf, const T *kappa, const T *rho,
                                        const T *ya, const T *az, T *glo, T *ghi, T *gkappa, hipStream_t s)
{
    if (batch > 0x7fffffffu || (!glo && !ghi && !gkappa)) return hipErrorInvalidValue;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({yf, kappa, ya, az, glo, ghi, gkappa});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_soft_grad_bounds_kernel<T>), dim3(batch), dim3(threads), 0, s, nz, vec, yf, kappa, rho, ya, az, glo, ghi,
                       gkappa);
    return hipGetLastError();
}

template hipError_t launch_admm_soft_mask<float>(uint64_t, uint32_t, const float *, const float *, const float *, float *, hipStream_t);
template hipError_t launch_admm_soft_mask<double>(uint64_t, uint32_t, const double *, const double *, const double *, double *,
                                                  hipStream_t);
template hipError_t launch_admm_soft_grad_bounds<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                                        const float *, const float *, const float *, float *, float *, float *,
                                                        hipStream_t);
template hipError_t launch_admm_soft_grad_bounds<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *,
                                                         const double *, const double *, const double *, double *, double *, double *,
                                                         hipStream_t);

}  // namespace gbdpcg
