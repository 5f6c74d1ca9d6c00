// ieee_once.hpp -- the operations the ADMM updates (admm.hip, admm_rows.hip) are specified with, each ONE correctly rounded IEEE
// operation or a pair of comparisons.  The build runs with -ffp-contract=off, so an fma happens exactly where one is written.
#pragma once
#include <hip/hip_runtime.h>

namespace gbdpcg {

namespace {

__device__ __forceinline__ float fma_once(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_once(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sqrt_once(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_once(double a) { return __builtin_sqrt(a); }

// comparisons: a NaN v stays NaN, +-Inf bounds never bind
template <typename T> __device__ __forceinline__ T clip(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The projection onto the degenerate set of the adjoint updates (admm.hip, the adjoint rows of admm_rows.hip): {0} where the
// forward multiplier yf is not zero (a NaN included), the whole line elsewhere.  clip(v, +0, +0): a NaN v stays NaN, v = -0 stays -0.
template <typename T> __device__ __forceinline__ T pin(T v, T yf) { return yf != T(0) ? clip(v, T(0), T(0)) : v; }

// The soft (L1-penalised) bound of the gbdpcg_admm_soft_* / gbdpcg_admm_lin_soft_* calls: the prox of (kappa / rho) dist(., [lo, hi])
// at s, with the scaled multiplier it leaves.  theta = kappa / rho is ONE correctly rounded division; kappa = +Inf takes the third
// branch, whose operations (w = clip(s), y = s - w) are those of the hard update: the hard bits.  A tie e = +-theta takes it too;
// kappa = 0 frees the row; a NaN s fails every comparison and stays NaN.  |y| <= theta by construction.
template <typename T> __device__ __forceinline__ void soft_clip(T s, T lo, T hi, T kappa, T rho, T &w, T &y)
{
    const T p = clip(s, lo, hi);
    const T e = s - p;   // exactly 0 inside the bounds
    const T theta = kappa / rho;
    if (e > theta) {
        w = s - theta, y = theta;
    } else if (e < -theta) {
        w = s + theta, y = -theta;
    } else {
        w = p, y = e;
    }
}
// INIT of the soft families: a soft row admits any w, only a hard one (kappa = +Inf) is clipped -- init stays idempotent
template <typename T> __device__ __forceinline__ T soft_init(T w, T lo, T hi, T kappa)
{
    return kappa == T(__builtin_huge_val()) ? clip(w, lo, hi) : w;
}

// The rows a soft update left SATURATED (admm_box_grad.hip, the SOFT gradients of admm_lin_grad.hip): |yf| >= theta with the theta of
// soft_clip, the same ONE division -- the update wrote +-theta itself, so the comparison is exact; a NaN yf fails it.
__device__ __forceinline__ float abs_once(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double abs_once(double a) { return __builtin_fabs(a); }
template <typename T> __device__ __forceinline__ bool soft_saturated(T yf, T kappa, T rho)
{
    const T theta = kappa / rho;
    return abs_once(yf) >= theta;
}

// The kappa argument of a kernel with a compile-time SOFT switch is a trailing parameter PACK: one pointer in the soft
// instantiations, empty in the hard ones, which therefore take the arguments, and compile to the code, of a kernel that knows
// nothing of kappa (an empty struct in its place would still take a kernel-argument slot and move the hidden arguments).
template <typename T> __device__ __forceinline__ const T *kappa_of(const T *kappa) { return kappa; }

}  // namespace

}  // namespace gbdpcg
