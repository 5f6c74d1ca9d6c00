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
// alike: with every base 16-byte aligned (vec != 0, decided by the host) a scalar head, 16-byte loads and stores, a scalar tail;
// otherwise every element goes through the scalar form.  Same operations per element either way: same bits.
#include "ieee_once.hpp"
#include "internal.hpp"

namespace gbdpcg {

namespace {

template <typename T> struct RebalanceVec;
template <> struct RebalanceVec<float> {
    static constexpr uint32_t N = 4;
    typedef float type __attribute__((ext_vector_type(4)));
};
template <> struct RebalanceVec<double> {
    static constexpr uint32_t N = 2;
    typedef double type __attribute__((ext_vector_type(2)));
};

}  // namespace

template <typename T, bool BOX>
__global__ __launch_bounds__(256) void admm_rebalance_kernel(uint64_t len, uint32_t vec, const T *g, const T *res, T *rho, const T *w,
                                                             T *y, T *gt, T ratio, T tau, T inv_tau, T rho_min, T rho_max,
                                                             int32_t shift, int32_t *expo)
{
    using V = typename RebalanceVec<T>::type;
    constexpr uint32_t VN = RebalanceVec<T>::N;
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
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

        auto scalar = [&](uint64_t i) {
            T yi = y[i];
            if (move) {
                yi = yi * scale;
                y[i] = yi;
            }
            if constexpr (BOX) {
                const T t = w[i] - yi;
                gt[i] = fma_once(-rn, t, g[i]);
            }
        };

        uint64_t head = 0, body = 0;   // elements in front of the first 16-byte boundary, 16-byte groups behind it
        if (vec) {
            head = (VN - (uint32_t)(off % VN)) % VN;
            if (head > len) head = len;
            body = (len - head) / VN;
        }
        if (tid < head) scalar(tid);
        for (uint64_t q = tid; q < body; q += threads) {
            const uint64_t i = head + q * VN;
            V yv = *reinterpret_cast<const V *>(y + i);
            if (move) {
#pragma unroll
                for (uint32_t k = 0; k < VN; ++k) yv[k] = yv[k] * scale;
                *reinterpret_cast<V *>(y + i) = yv;
            }
            if constexpr (BOX) {
                const V wv = *reinterpret_cast<const V *>(w + i), gv = *reinterpret_cast<const V *>(g + i);
                V tv;
#pragma unroll
                for (uint32_t k = 0; k < VN; ++k) {
                    const T t = wv[k] - yv[k];
                    tv[k] = fma_once(-rn, t, gv[k]);
                }
                *reinterpret_cast<V *>(gt + i) = tv;
            }
        }
        for (uint64_t i = head + body * VN + tid; i < len; i += threads) scalar(i);   // the tail; all of it without vec
    }

    __syncthreads();   // every lane's stores, which needed rho, are behind it
    if (tid == 0) {
        rho[prob] = rn;
        expo[prob] = e;
    }
}

template <typename T>
hipError_t launch_admm_rebalance(uint64_t len, uint32_t batch, const T *g, const T *res, T *rho, const T *w, T *y, T *gt, T ratio,
                                 uint32_t shift, T rho_min, T rho_max, int32_t *expo, hipStream_t s, bool box)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    uint32_t vec = reinterpret_cast<uintptr_t>(y) % 16 ? 0 : 1;
    if (box)
        for (const void *p : {(const void *)g, (const void *)w, (const void *)gt})
            if (reinterpret_cast<uintptr_t>(p) % 16) vec = 0;
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
