// admm_adjoint.hip -- the backward pass of the hard box QP of admm.hip (gbdpcg_admm_adjoint_init_*, gbdpcg_admm_adjoint_update_*, the
// third launch of gbdpcg_admm_adjoint_step_*, gbdpcg_admm_grad_bounds_*).  At a solution with the active set A (entries held at a
// bound) the adjoint pair (a_z, a_lambda) of a scalar l solves
//     G a_z + gz + C' a_lambda + nu = 0,   C a_z = -glam,   (a_z)_A = 0,   nu supported on A
// which are the optimality conditions of the box QP with the SAME G and C, g := gz = dl/dz, c := -dl/dlambda and the degenerate
// box lo = hi = 0 on A, (-Inf, +Inf) elsewhere: the kept S, Phi^-1, G^-1 of G + rho I serve it unchanged.  A is the sign pattern of
// the forward y (yf, read only): behind a hard update y_i is exactly 0 where nothing was clipped, so the mask is m = (yf_i != 0) --
// no threshold.  An entry that sits on its bound with yf_i = 0 (weakly active) counts as free; a NaN yf_i counts as active.
// Per element, with m in the place of lo and hi, the lines of the hard update, every one ONE IEEE operation or a comparison:
//     v   = az + y
//     w+  = m ? (v < 0 ? 0 : (v > 0 ? 0 : v)) : v        clip(v, +0, +0): a NaN v stays NaN, v = -0 stays -0
//     y+  = v - w+
//     t   = w+ - y+
//     gt+ = fma(-rho, t, gz)
//     res[2b] = max |az - w+|,  res[2b+1] = max |rho (w+ - w)|
// INIT (gbdpcg_admm_adjoint_init_*): w <- m ? clip(w, 0, 0) : w, y unchanged (not written), gt = fma(-rho, w - y, gz).
// w, y, gt, res are the bits of admm_update_kernel on the explicit degenerate box (lo = hi = +0 where m, -Inf / +Inf elsewhere).
//
// Shape: that of admm_update_kernel -- ONE WORKGROUP PER PROBLEM, one wave when nz <= 256, otherwise four, 64-bit problem stride,
// rho_b once per workgroup through the scalar cache, the norms through norm_fold.hpp, no atomics, no memset, nothing read from res.
// 8 element accesses per element of az (5 reads, 3 writes; INIT: 4 + 2).  The six arrays are indexed at the same offset b nz: with
// every base pointer 16-byte aligned (vec != 0, decided by the host) a scalar head, a 16-byte body and a scalar tail, otherwise
// every element through the scalar form.  Same operations per element either way: same bits.
//
// Bound gradients (gbdpcg_admm_grad_bounds_*), with ya the adjoint's y (nu = rho ya), one multiplication and one negation:
//     glo_i = yf_i < 0 ? -(rho_b ya_i) : +0        ghi_i = yf_i > 0 ? -(rho_b ya_i) : +0
// the same launch shape and head / body / tail scheme over yf, ya, glo, ghi.
#include "elementwise_split.hpp"
#include "ieee_once.hpp"
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

// One element.  w, y: in / out (INIT leaves y alone); mp, md: the running maxima of the two norms (not INIT).
template <typename T, bool INIT, typename U>
__device__ __forceinline__ T adjoint_element(T az, T &w, T &y, T yf, T gz, T rho, U &mp, U &md)
{
    if constexpr (INIT) {
        w = pin(w, yf);
        const T t = w - y;
        return fma_once(-rho, t, gz);
    } else {
        const T v = az + y;
        const T wn = pin(v, yf);
        const T yn = v - wn;
        const T t = wn - yn;
        mp = umax(mp, abs_bits(az - wn));
        md = umax(md, abs_bits(rho * (wn - w)));
        w = wn;
        y = yn;
        return fma_once(-rho, t, gz);
    }
}

}  // namespace

template <typename T, bool INIT>
__global__ __launch_bounds__(256) void admm_adjoint_update_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ gz,
                                                                  const T *__restrict__ yf, const T *__restrict__ rho,
                                                                  const T *__restrict__ az, T *__restrict__ w, T *__restrict__ y,
                                                                  T *__restrict__ gt, T *__restrict__ res)
{
    using U = decltype(abs_bits(T(0)));
    using V = typename AdjVec<T>::type;
    constexpr uint32_t VN = AdjVec<T>::N;
    __shared__ U slots[8];   // two words per wave
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t off = (uint64_t)prob * nz;   // 64-bit problem stride
    gz += off, yf += off, w += off, y += off, gt += off;
    if constexpr (!INIT) az += off;
    const T r = rho[prob];
    U mp = 0, md = 0;

    auto scalar = [&](uint64_t i) {
        T wi = w[i], yi = y[i];
        const T ai = INIT ? T(0) : az[i];
        gt[i] = adjoint_element<T, INIT>(ai, wi, yi, yf[i], gz[i], r, mp, md);
        w[i] = wi;
        if constexpr (!INIT) y[i] = yi;
    };

    uint64_t head, body;   // elements in front of the first 16-byte boundary, 16-byte groups behind it
    split<VN>(vec, off, nz, head, body);
    if (tid < head) scalar(tid);
    for (uint64_t q = tid; q < body; q += threads) {
        const uint64_t i = head + q * VN;
        V wv = *reinterpret_cast<const V *>(w + i), yv = *reinterpret_cast<const V *>(y + i);
        const V fv = *reinterpret_cast<const V *>(yf + i), gv = *reinterpret_cast<const V *>(gz + i);
        V av = {};
        if constexpr (!INIT) av = *reinterpret_cast<const V *>(az + i);
        V tv;
#pragma unroll
        for (uint32_t e = 0; e < VN; ++e) {
            T we = wv[e], ye = yv[e];
            tv[e] = adjoint_element<T, INIT>(av[e], we, ye, fv[e], gv[e], r, mp, md);
            wv[e] = we;
            yv[e] = ye;
        }
        *reinterpret_cast<V *>(w + i) = wv;
        if constexpr (!INIT) *reinterpret_cast<V *>(y + i) = yv;
        *reinterpret_cast<V *>(gt + i) = tv;
    }
    for (uint64_t i = head + body * VN + tid; i < nz; i += threads) scalar(i);   // the tail; all of it without vec

    if constexpr (!INIT)
        store_norms(mp, md, tid >> 6, tid & 63u, threads >> 6, [&](uint32_t wv) { return slots + 2 * wv; }, res + 2 * (uint64_t)prob);
}

template <typename T>
__global__ __launch_bounds__(256) void admm_grad_bounds_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ yf,
                                                               const T *__restrict__ rho, const T *__restrict__ ya,
                                                               T *__restrict__ glo, T *__restrict__ ghi)
{
    using V = typename AdjVec<T>::type;
    constexpr uint32_t VN = AdjVec<T>::N;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t off = (uint64_t)prob * nz;
    yf += off, ya += off, glo += off, ghi += off;
    const T r = rho[prob];

    auto element = [&](T f, T a, T &lo, T &hi) {
        const T n = -(r * a);
        lo = f < T(0) ? n : T(0);
        hi = f > T(0) ? n : T(0);
    };
    auto scalar = [&](uint64_t i) {
        T lo, hi;
        element(yf[i], ya[i], lo, hi);
        glo[i] = lo;
        ghi[i] = hi;
    };

    uint64_t head, body;
    split<VN>(vec, off, nz, head, body);
    if (tid < head) scalar(tid);
    for (uint64_t q = tid; q < body; q += threads) {
        const uint64_t i = head + q * VN;
        const V fv = *reinterpret_cast<const V *>(yf + i), av = *reinterpret_cast<const V *>(ya + i);
        V lv, hv;
#pragma unroll
        for (uint32_t e = 0; e < VN; ++e) {
            T lo, hi;
            element(fv[e], av[e], lo, hi);
            lv[e] = lo;
            hv[e] = hi;
        }
        *reinterpret_cast<V *>(glo + i) = lv;
        *reinterpret_cast<V *>(ghi + i) = hv;
    }
    for (uint64_t i = head + body * VN + tid; i < nz; i += threads) scalar(i);
}

template <typename T>
hipError_t launch_admm_adjoint_update(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *gz, const T *yf, const T *rho,
                                      const T *az, T *w, T *y, T *gt, T *res, hipStream_t s, bool init)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({gz, yf, w, y, gt, init ? (const void *)gz : (const void *)az});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    if (init)
        hipLaunchKernelGGL((admm_adjoint_update_kernel<T, true>), dim3(batch), dim3(threads), 0, s, nz, vec, gz, yf, rho, az, w, y, gt, res);
    else
        hipLaunchKernelGGL((admm_adjoint_update_kernel<T, false>), dim3(batch), dim3(threads), 0, s, nz, vec, gz, yf, rho, az, w, y, gt, res);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_grad_bounds(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *yf, const T *rho, const T *ya, T *glo,
                                   T *ghi, hipStream_t s)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({yf, ya, glo, ghi});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    hipLaunchKernelGGL((admm_grad_bounds_kernel<T>), dim3(batch), dim3(threads), 0, s, nz, vec, yf, rho, ya, glo, ghi);
    return hipGetLastError();
}

template hipError_t launch_admm_adjoint_update<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *, const float *,
                                                      const float *, float *, float *, float *, float *, hipStream_t, bool);
template hipError_t launch_admm_adjoint_update<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *,
                                                       const double *, const double *, double *, double *, double *, double *, hipStream_t,
                                                       bool);
template hipError_t launch_admm_grad_bounds<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *, const float *,
                                                   float *, float *, hipStream_t);
template hipError_t launch_admm_grad_bounds<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *, const double *,
                                                    double *, double *, hipStream_t);

}  // namespace gbdpcg
