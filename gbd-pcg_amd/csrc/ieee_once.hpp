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

}  // namespace

}  // namespace gbdpcg
