// grad_store.hpp -- what the write-bound gradient launches share (kkt_grad.hip, admm_lin_grad.hip): index divisions as
// multiplications by reciprocals the host prepared, and the store of one contiguous range of outputs in 16-byte vectors.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "elementwise_split.hpp"

namespace gbdpcg {

namespace {

// floor(n / d) for every n <= nmax as __umulhi(n, m): m = floor(2^32 / d) + 1, so m d = 2^32 + e with 0 < e <= d, and
// floor(n m / 2^32) = floor(n / d + n e / (d 2^32)) = floor(n / d) as long as n e < 2^32, which nmax d < 2^32 guarantees.
// 0: no such m in 32 bits (d == 1) or the bound fails -- the kernel then divides.
uint32_t magic(uint32_t d, uint64_t nmax)
{
    if (d <= 1 || nmax * d >= (1ull << 32)) return 0;
    return (uint32_t)((1ull << 32) / d) + 1u;
}

__device__ __forceinline__ uint32_t fast_div(uint32_t n, uint32_t d, uint32_t m) { return m ? __umulhi(n, m) : n / d; }

// `count` elements from `out` on, element f = fn(f): scalar head to the first 16-byte boundary, 16-byte body, scalar tail.
template <typename T, typename F> __device__ __forceinline__ void store_range(T *out, uint32_t count, uint32_t tid, uint32_t threads, F fn)
{
    using V = typename Vec16<T>::type;
    constexpr uint32_t VN = Vec16<T>::N;
    uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / (uint32_t)sizeof(T);
    if (head > count) head = count;
    const uint32_t body = (count - head) / VN;
    if (tid < head) out[tid] = fn(tid);
    for (uint32_t q = tid; q < body; q += threads) {
        const uint32_t f = head + q * VN;
        V v;
#pragma unroll
        for (uint32_t e = 0; e < VN; ++e) v[e] = fn(f + e);
        *reinterpret_cast<V *>(out + f) = v;
    }
    for (uint32_t f = head + body * VN + tid; f < count; f += threads) out[f] = fn(f);
}

}  // namespace

}  // namespace gbdpcg
