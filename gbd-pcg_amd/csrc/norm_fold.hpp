// norm_fold.hpp -- the NaN-propagating maximum of magnitudes that the per-problem norms are taken with (schur_residual.hip: the KKT
// residual kernels; admm.hip: the splitting update).  The maximum runs over the BIT PATTERN of |entry| as an unsigned integer:
// that orders the non-negative numbers as they are ordered, puts Inf above them and every NaN above Inf, and is exact in any fold
// order.  Every lane keeps its running maxima in registers, a wave folds them through DPP, the workgroup through one LDS slot per
// wave, and one lane writes the pair: nothing initialised beforehand, nothing read from the output.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gbdpcg {

namespace {

__device__ __forceinline__ uint32_t abs_bits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
__device__ __forceinline__ uint64_t abs_bits(double x) { return __builtin_bit_cast(uint64_t, x) & 0x7fffffffffffffffull; }
__device__ __forceinline__ float from_bits(uint32_t b) { return __builtin_bit_cast(float, b); }
__device__ __forceinline__ double from_bits(uint64_t b) { return __builtin_bit_cast(double, b); }
template <typename U> __device__ __forceinline__ U umax(U a, U b) { return a > b ? a : b; }

template <int CTRL> __device__ __forceinline__ uint32_t dpp_move(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL> __device__ __forceinline__ uint64_t dpp_move(uint64_t v)
{
    const uint32_t lo = dpp_move<CTRL>((uint32_t)v), hi = dpp_move<CTRL>((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
template <int L> __device__ __forceinline__ uint32_t lane_value(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, L); }
template <int L> __device__ __forceinline__ uint64_t lane_value(uint64_t v)
{
    return ((uint64_t)lane_value<L>((uint32_t)(v >> 32)) << 32) | lane_value<L>((uint32_t)v);
}
// The maximum over the 64 lanes of a wave, in every lane (all of them active): neighbours, pairs, the halves of an 8-lane group
// and of a 16-lane row by DPP, the four rows through scalar registers.
template <typename U> __device__ __forceinline__ U wave_umax(U v)
{
    v = umax(v, dpp_move<0xB1>(v));    // quad_perm:[1,0,3,2]
    v = umax(v, dpp_move<0x4E>(v));    // quad_perm:[2,3,0,1]
    v = umax(v, dpp_move<0x141>(v));   // row_half_mirror
    v = umax(v, dpp_move<0x140>(v));   // row_mirror
    return umax(umax(lane_value<0>(v), lane_value<16>(v)), umax(lane_value<32>(v), lane_value<48>(v)));
}
// The workgroup's two maxima -> res[0], res[1].  slot(w): two words of LDS that belong to wave w.
template <typename T, typename U, typename F>
__device__ __forceinline__ void store_norms(U ms, U mf, uint32_t wave, uint32_t lane, uint32_t waves, F &&slot, T *__restrict__ res)
{
    ms = wave_umax(ms);
    mf = wave_umax(mf);
    if (lane == 0) {
        U *s = slot(wave);
        s[0] = ms;
        s[1] = mf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < waves; ++w) {
            const U *s = slot(w);
            ms = umax(ms, s[0]);
            mf = umax(mf, s[1]);
        }
        res[0] = from_bits(ms);
        res[1] = from_bits(mf);
    }
}

}  // namespace

}  // namespace gbdpcg
