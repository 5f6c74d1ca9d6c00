// admm.hip -- the splitting update of box-constrained ADMM on a kept KKT factorisation (gbdpcg_admm_init_*, gbdpcg_admm_update_*,
// the third launch of gbdpcg_admm_step_*) and its adjoint (gbdpcg_admm_adjoint_init_*, gbdpcg_admm_adjoint_update_*, the third launch
// of gbdpcg_admm_adjoint_step_*).  Problem b minimises 1/2 z'Gz + g'z subject to Cz = c and lo <= z <= hi; the matrices
// of the solve belong to G + rho_b I (gbdpcg_form_schur_reg_*), w is the copy of z that lives in the box, y the scaled multiplier
// of z = w (mu = rho y).  After the solve with the gradient gt has written z, per element, every line ONE IEEE operation or a
// comparison, so w, y and the norms are defined to the bit whatever the launch shape:
//     v   = z + y
//     w+  = v < lo ? lo : (v > hi ? hi : v)          comparisons: a NaN v stays NaN, +-Inf bounds never bind
//     y+  = v - w+                                   exactly 0 where nothing was clipped
//     t   = w+ - y+
//     gt+ = fma(-rho, t, g)                          ONE rounding: the build runs with -ffp-contract=off, the fma is written out
//     res[2b]   = max |z - w+|                       primal residual ||z - w||_inf
//     res[2b+1] = max |rho (w+ - w)|                 dual residual rho ||w+ - w||_inf
// INIT (gbdpcg_admm_init_*): w <- clip(w), y unchanged (not written), gt = fma(-rho, w - y, g); z and res are not looked at.
// The maxima are those of the KKT residual norms (norm_fold.hpp): over the bit pattern of |entry|, exact in any order, NaN on top.
// SOFT (gbdpcg_admm_soft_*; a compile-time switch next to INIT): element i pays kappa_i dist(z_i, [lo_i, hi_i]) instead of being
// bounded.  Only the two lines of w+ and y+ change (soft_clip in ieee_once.hpp):
//     p = clip(v);  e = v - p;  theta = kappa / rho              / correctly rounded
//     w+ = e > theta ? v - theta : (e < -theta ? v + theta : p);   y+ = e > theta ? theta : (e < -theta ? -theta : e)
// kappa = +Inf: the third branch, the operations of the hard update, the hard bits.  INIT: w <- (kappa == +Inf) ? clip(w) : w.
// kappa is an eighth array at the same offset b nz, loaded by the same head / body / tail scheme and part of the host's alignment
// test: 10 element accesses per element of z (INIT: 6 + 2).  It is not validated: negative or NaN is the caller's error.  The hard
// instantiations take no kappa argument (an empty parameter pack) and compile to the code of a kernel that knows nothing of it.
//
// ADJOINT (admm_adjoint_update_kernel, the backward pass of the hard box QP; never with SOFT).  At a solution with the active set A
// (entries held at a bound) the adjoint pair (a_z, a_lambda) of a scalar l solves
//     G a_z + gz + C' a_lambda + nu = 0,   C a_z = -glam,   (a_z)_A = 0,   nu supported on A
// which are the optimality conditions of the box QP with the SAME G and C, g := gz = dl/dz, c := -dl/dlambda and the degenerate
// box lo = hi = 0 on A, (-Inf, +Inf) elsewhere: the kept S, Phi^-1, G^-1 of G + rho I serve it unchanged.  A is the sign pattern of
// the forward y (yf, read only): behind a hard update y_i is exactly 0 where nothing was clipped, so the mask is m = (yf_i != 0) --
// no threshold.  An entry that sits on its bound with yf_i = 0 (weakly active) counts as free; a NaN yf_i counts as active.
// yf stands where lo stood, there is no hi (one array read fewer: 8 element accesses per element of az, INIT: 4 + 2), z is az, g is
// gz, and only the line of w+ changes (pin in ieee_once.hpp):
//     w+  = m ? (v < 0 ? 0 : (v > 0 ? 0 : v)) : v        clip(v, +0, +0): a NaN v stays NaN, v = -0 stays -0
// INIT (gbdpcg_admm_adjoint_init_*): w <- m ? clip(w, 0, 0) : w.  w, y, gt, res are the bits of admm_update_kernel on the explicit
// degenerate box (lo = hi = +0 where m, -Inf / +Inf elsewhere).  The body is shared (box_update, forced inline into both __global__
// entries); ADJ is its compile-time switch.
//
// Shape: ONE WORKGROUP PER PROBLEM (the two norms are per problem: nothing crosses a workgroup, no atomics, no memset, nothing
// read from res), one wave when nz <= 256, otherwise four.  9 element accesses per element of z (6 reads, 3 writes; INIT: 5 + 2),
// rho_b once per workgroup through the scalar cache, two numbers out per problem.  All seven arrays are indexed at the same
// offset b nz, so they are misaligned alike: when every base pointer is 16-byte aligned (vec != 0, decided by the host) the
// workgroup peels a scalar head of (-b nz) mod (16 / sizeof T) elements, runs the body with 16-byte loads and stores and finishes
// with a scalar tail (for_each_split in elementwise_split.hpp); otherwise every element goes through the scalar form.  Same
// operations per element either way: same bits.
// Default cache policy throughout: z was written by the recovery kernel just before, gt is read by the gamma kernel next.
#include "elementwise_split.hpp"
#include "ieee_once.hpp"
#include "internal.hpp"
#include "norm_fold.hpp"

namespace gbdpcg {

namespace {

// One element.  w, y: in / out (INIT leaves y alone); mp, md: the running maxima of the two norms (not INIT); kap: read where SOFT;
// ADJ: lo is yf, hi is not looked at.
template <typename T, bool INIT, bool SOFT, bool ADJ, typename U>
__device__ __forceinline__ T admm_element(T z, T &w, T &y, T lo, T hi, T kap, T g, T rho, U &mp, U &md)
{
    if constexpr (INIT) {
        if constexpr (SOFT)
            w = soft_init(w, lo, hi, kap);
        else if constexpr (ADJ)
            w = pin(w, lo);
        else
            w = clip(w, lo, hi);
        const T t = w - y;
        return fma_once(-rho, t, g);
    } else {
        const T v = z + y;
        T wn, yn;
        if constexpr (SOFT) {
            soft_clip(v, lo, hi, kap, rho, wn, yn);
        } else {
            if constexpr (ADJ)
                wn = pin(v, lo);
            else
                wn = clip(v, lo, hi);
            yn = v - wn;
        }
        const T t = wn - yn;
        mp = umax(mp, abs_bits(z - wn));
        md = umax(md, abs_bits(rho * (wn - w)));
        w = wn;
        y = yn;
        return fma_once(-rho, t, g);
    }
}

// The body of the two kernels below.  ADJ (the adjoint instantiations, never with SOFT): lo is yf, hi is not looked at.
template <typename T, bool INIT, bool SOFT, bool ADJ, typename... K>
__device__ __forceinline__ void box_update(uint64_t nz, uint32_t vec, const T *__restrict__ g, const T *__restrict__ lo,
                                           const T *__restrict__ hi, const T *__restrict__ rho, const T *__restrict__ z,
                                           T *__restrict__ w, T *__restrict__ y, T *__restrict__ gt, T *__restrict__ res, K... kappa_arg)
{
    static_assert(!(ADJ && SOFT), "the adjoint box is a hard box");
    static_assert(sizeof...(K) == (SOFT ? 1 : 0), "kappa is an argument of the soft instantiations alone");
    using U = decltype(abs_bits(T(0)));
    using V = typename Vec16<T>::type;
    __shared__ U slots[8];   // two words per wave
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const uint64_t off = (uint64_t)prob * nz;   // 64-bit problem stride
    g += off, lo += off, w += off, y += off, gt += off;
    if constexpr (!ADJ) hi += off;
    if constexpr (!INIT) z += off;
    [[maybe_unused]] const T *__restrict__ kappa = nullptr;
    if constexpr (SOFT) kappa = kappa_of<T>(kappa_arg...) + off;
    const T r = rho[prob];
    U mp = 0, md = 0;

    for_each_split<T>(
        vec, off, nz,
        [&](uint64_t i) {
            T wi = w[i], yi = y[i], hv = T(0), ki = T(0);
            if constexpr (!ADJ) hv = hi[i];
            const T zi = INIT ? T(0) : z[i];
            if constexpr (SOFT) ki = kappa[i];
            gt[i] = admm_element<T, INIT, SOFT, ADJ>(zi, wi, yi, lo[i], hv, ki, g[i], r, mp, md);
            w[i] = wi;
            if constexpr (!INIT) y[i] = yi;
        },
        [&](uint64_t i) {
            V wv = load16(w + i), yv = load16(y + i);
            const V lv = load16(lo + i);
            V hv = {}, zv = {}, kv = {};
            if constexpr (!ADJ) hv = load16(hi + i);
            const V gv = load16(g + i);
            if constexpr (!INIT) zv = load16(z + i);
            if constexpr (SOFT) kv = load16(kappa + i);
            V tv;
#pragma unroll
            for (uint32_t e = 0; e < Vec16<T>::N; ++e) {
                T we = wv[e], ye = yv[e];
                tv[e] = admm_element<T, INIT, SOFT, ADJ>(zv[e], we, ye, lv[e], hv[e], kv[e], gv[e], r, mp, md);
                wv[e] = we;
                yv[e] = ye;
            }
            store16(w + i, wv);
            if constexpr (!INIT) store16(y + i, yv);
            store16(gt + i, tv);
        });

    if constexpr (!INIT)
        store_norms(mp, md, tid >> 6, tid & 63u, threads >> 6, [&](uint32_t wv) { return slots + 2 * wv; }, res + 2 * (uint64_t)prob);
}

}  // namespace

template <typename T, bool INIT, bool SOFT, typename... K>
__global__ __launch_bounds__(256) void admm_update_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ g, const T *__restrict__ lo,
                                                          const T *__restrict__ hi, const T *__restrict__ rho, const T *__restrict__ z,
                                                          T *__restrict__ w, T *__restrict__ y, T *__restrict__ gt, T *__restrict__ res,
                                                          K... kappa_arg)
{
    box_update<T, INIT, SOFT, false>(nz, vec, g, lo, hi, rho, z, w, y, gt, res, kappa_arg...);
}

template <typename T, bool INIT>
__global__ __launch_bounds__(256) void admm_adjoint_update_kernel(uint64_t nz, uint32_t vec, const T *__restrict__ gz,
                                                                  const T *__restrict__ yf, const T *__restrict__ rho,
                                                                  const T *__restrict__ az, T *__restrict__ w, T *__restrict__ y,
                                                                  T *__restrict__ gt, T *__restrict__ res)
{
    box_update<T, INIT, false, true>(nz, vec, gz, yf, static_cast<const T *>(nullptr), rho, az, w, y, gt, res);
}

template <typename T>
hipError_t launch_admm_update(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *g, const T *lo, const T *hi, const T *rho,
                              const T *z, T *w, T *y, T *gt, T *res, hipStream_t s, bool init, const T *kappa)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({g, lo, hi, w, y, gt, init ? nullptr : z, kappa});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    if (kappa && init)   // the soft family: its own instantiations
        hipLaunchKernelGGL((admm_update_kernel<T, true, true, const T *>), dim3(batch), dim3(threads), 0, s, nz, vec, g, lo, hi, rho, z, w,
                           y, gt, res, kappa);
    else if (kappa)
        hipLaunchKernelGGL((admm_update_kernel<T, false, true, const T *>), dim3(batch), dim3(threads), 0, s, nz, vec, g, lo, hi, rho, z, w,
                           y, gt, res, kappa);
    else if (init)
        hipLaunchKernelGGL((admm_update_kernel<T, true, false>), dim3(batch), dim3(threads), 0, s, nz, vec, g, lo, hi, rho, z, w, y, gt, res);
    else
        hipLaunchKernelGGL((admm_update_kernel<T, false, false>), dim3(batch), dim3(threads), 0, s, nz, vec, g, lo, hi, rho, z, w, y, gt, res);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_admm_adjoint_update(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *gz, const T *yf, const T *rho,
                                      const T *az, T *w, T *y, T *gt, T *res, hipStream_t s, bool init)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu;
    const uint32_t vec = all_aligned({gz, yf, w, y, gt, init ? nullptr : az});
    const uint32_t threads = nz <= 256 ? 64 : 256;
    if (init)
        hipLaunchKernelGGL((admm_adjoint_update_kernel<T, true>), dim3(batch), dim3(threads), 0, s, nz, vec, gz, yf, rho, az, w, y, gt, res);
    else
        hipLaunchKernelGGL((admm_adjoint_update_kernel<T, false>), dim3(batch), dim3(threads), 0, s, nz, vec, gz, yf, rho, az, w, y, gt, res);
    return hipGetLastError();
}

template hipError_t launch_admm_update<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *, const float *,
                                              const float *, const float *, float *, float *, float *, float *, hipStream_t, bool,
                                              const float *);
template hipError_t launch_admm_update<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *, const double *,
                                               const double *, const double *, double *, double *, double *, double *, hipStream_t, bool,
                                               const double *);
template hipError_t launch_admm_adjoint_update<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *, const float *,
                                                      const float *, float *, float *, float *, float *, hipStream_t, bool);
template hipError_t launch_admm_adjoint_update<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *,
                                                       const double *, const double *, double *, double *, double *, double *, hipStream_t,
                                                       bool);

}  // namespace gbdpcg
