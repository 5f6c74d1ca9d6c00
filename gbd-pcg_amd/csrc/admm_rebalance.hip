// admm_rebalance.hip -- adaptive rho for the ADMM families: residual balancing in powers of two, on the device, one launch
// (gbdpcg_admm_rebalance_*, the first launch of gbdpcg_admm_lin_rebalance_* / gbdpcg_admm_soc_rebalance_* and of every
// gbdpcg_admm*_restep_*).  Problem b reads r = res[2b], s = res[2b+1] as the last update launch wrote them and rho = rho[b]; with the
// host's ratio >= 1, tau = 2^shift and the limits rho_min <= rho_max, every line ONE IEEE operation or a comparison:
//     up = rho tau              dn = rho (1 / tau)            tau and 1 / tau are exact
//     if      r > ratio s  and  up <= rho_max :  rho' = up,  e = +shift
//     else if s > ratio r  and  dn >= rho_min :  rho' = dn,  e = -shift
//     else                                       rho' = rho, e = 0            a NaN in r, s or rho fails every comparison
//     y'_i = y_i 2^-e                            one multiplication, exact unless it lands in the subnormals; e = 0: y is not touched
// so the multiplier mu = rho y the iteration carries stays what it was.  BOX (the box family, whose arrays all have the layout of g):
// additionally gt_i = fma(-rho', w_i - y'_i, g_i), the INIT line of admm.hip for a w that lies in the box already (w is only read) --
// one launch for what the rows form and gbdpcg_admm_init_* do in two, with the same bits.  The rows form scales y alone; the
// families with rows rebuild gt with their own init launch (admm_rows.hip), which needs E.
//
// Shape: ONE WORKGROUP PER PROBLEM like admm_update_kernel, one wave when the vector has <= 256 elements, otherwise four; 64-bit
// problem stride; r, s and rho are uniform loads in front of every store, so they go through the scalar cache.  No LDS, no atomics,
// nothing initialised beforehand.  One lane writes rho' and e behind a barrier, when every lane that uses rho has stored what it
// computed from it.  res is read, never written.  The arrays of a problem start at the same offset b len, so they are misaligned
// alike: with every base 16-byte aligned (vec != 0, decided by the host) a scalar head, 16-byte loads and stores, a scalar tail
// (for_each_split in elementwise_split.hpp); otherwise every element goes through the scalar form.  Same operations per element
// either way: same bits.
#include "elementwise_split.hpp"
#include "ieee_once.hpp"
#include "internal.hpp"

namespace gbdpcg {

template <typename T, bool BOX>
__global__ __launch_bounds__(256) void admm_rebalance_kernel(uint64_t len, uint32_t vec, const T *g, const T *res, T *rho, const T *w,
                                                             T *y, T *gt, T ratio, T tau, T inv_tau, T rho_min, T rho_max,
                                                             int32_t shift, int32_t *expo)
{
    using V = typename Vec16<T>::type;
    const uint32_t prob = blockIdx.x;
    const uint64_t off = (uint64_t)prob * len;   // 64-bit problem stride
    const T r = res[2 * (uint64_t)prob], s = res[2 * (uint64_t)prob + 1], rh = rho[prob];

    const T up = rh * tau, dn = rh * inv_tau;
    T rn = rh, scale = T(1);
    int32_t e = 0;
    if (r > ratio * s && up <= rho_max) {
        rn = up, e = shift, scale = inv_tau;
    } else if (s > ratio * r && dn >= rho_min) {
        rn = dn, e = -shift, scale = tau;
    }

    if (BOX || e != 0) {   // (uniform over the workgroup)
        y += off;
        if constexpr (BOX) g += off, w += off, gt += off;
        const bool move = e != 0;

        for_each_split<T>(
            vec, off, len,
            [&](uint64_t i) {
                T yi = y[i];
                if (move) {
                    yi = yi * scale;
                    y[i] = yi;
                }
                if constexpr (BOX) {
                    const T t = w[i] - yi;
                    gt[i] = fma_once(-rn, t, g[i]);
                }
            },
            [&](uint64_t i) {
                V yv = load16(y + i);
                if (move) {
#pragma unroll
                    for (uint32_t k = 0; k < Vec16<T>::N; ++k) yv[k] = yv[k] * scale;
                    store16(y + i, yv);
                }
                if constexpr (BOX) {
                    const V wv = load16(w + i), gv = load16(g + i);
                    V tv;
#pragma unroll
                    for (uint32_t k = 0; k < Vec16<T>::N; ++k) {
                        const T t = wv[k] - yv[k];
                        tv[k] = fma_once(-rn, t, gv[k]);
                    }
                    store16(gt + i, tv);
                }
            });
    }

    __syncthreads();   // every lane's stores, which needed rho, are behind it
    if (threadIdx.x == 0) {
        rho[prob] = rn;
        expo[prob] = e;
    }
}

template <typename T>
hipError_t launch_admm_rebalance(uint64_t len, uint32_t batch, const T *g, const T *res, T *rho, const T *w, T *y, T *gt, T ratio,
                                 uint32_t shift, T rho_min, T rho_max, int32_t *expo, hipStream_t s, bool box)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    const uint32_t vec = box ? all_aligned({y, g, w, gt}) : all_aligned({y});
    const uint32_t threads = len <= 256 ? 64 : 256;
    const T tau = (T)(1u << shift), inv_tau = T(1) / tau;   // shift <= 16: both exact
    if (box)
        hipLaunchKernelGGL((admm_rebalance_kernel<T, true>), dim3(batch), dim3(threads), 0, s, len, vec, g, res, rho, w, y, gt, ratio, tau,
                           inv_tau, rho_min, rho_max, (int32_t)shift, expo);
    else
        hipLaunchKernelGGL((admm_rebalance_kernel<T, false>), dim3(batch), dim3(threads), 0, s, len, vec, g, res, rho, w, y, gt, ratio, tau,
                           inv_tau, rho_min, rho_max, (int32_t)shift, expo);
    return hipGetLastError();
}

template hipError_t launch_admm_rebalance<float>(uint64_t, uint32_t, const float *, const float *, float *, const float *, float *, float *,
                                                 float, uint32_t, float, float, int32_t *, hipStream_t, bool);
template hipError_t launch_admm_rebalance<double>(uint64_t, uint32_t, const double *, const double *, double *, const double *, double *,
                                                  double *, double, uint32_t, double, double, int32_t *, hipStream_t, bool);

}  // namespace gbdpcg
