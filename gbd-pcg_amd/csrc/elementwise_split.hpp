// elementwise_split.hpp -- what the elementwise launches share (admm.hip, admm_box_grad.hip, admm_rebalance.hip; grad_store.hpp for
// the vector type): the 16-byte vector of a type, the head / body / tail loop over one problem's range, and the host's test that
// every base is aligned.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

namespace gbdpcg {

namespace {

template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr uint32_t N = 4;
    typedef float type __attribute__((ext_vector_type(4)));
};
template <> struct Vec16<double> {
    static constexpr uint32_t N = 2;
    typedef double type __attribute__((ext_vector_type(2)));
};

// One 16-byte group at an aligned address.
template <typename T> __device__ __forceinline__ typename Vec16<T>::type load16(const T *p)
{
    return *reinterpret_cast<const typename Vec16<T>::type *>(p);
}
template <typename T> __device__ __forceinline__ void store16(T *p, typename Vec16<T>::type v)
{
    *reinterpret_cast<typename Vec16<T>::type *>(p) = v;
}

// The head / body / tail split of a problem that starts `off` elements behind 16-byte aligned bases.
template <uint32_t VN> __device__ __forceinline__ void split(uint32_t vec, uint64_t off, uint64_t nz, uint64_t &head, uint64_t &body)
{
    head = 0, body = 0;
    if (vec) {
        head = (VN - (uint32_t)(off % VN)) % VN;
        if (head > nz) head = nz;
        body = (nz - head) / VN;
    }
}

// The loop of one workgroup over its problem's nz elements, which start `off` elements behind the bases: one(i) handles element i,
// group(i) the 16-byte group that starts at element i.  With vec != 0 (every base 16-byte aligned, decided by the host) a scalar
// head up to the first 16-byte boundary, the groups behind it, a scalar tail; otherwise every element through one().
template <typename T, typename One, typename Group>
__device__ __forceinline__ void for_each_split(uint32_t vec, uint64_t off, uint64_t nz, One one, Group group)
{
    constexpr uint32_t VN = Vec16<T>::N;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    uint64_t head, body;   // elements in front of the first 16-byte boundary, 16-byte groups behind it
    split<VN>(vec, off, nz, head, body);
    if (tid < head) one(tid);
    for (uint64_t q = tid; q < body; q += threads) group(head + q * VN);
    for (uint64_t i = head + body * VN + tid; i < nz; i += threads) one(i);   // the tail; all of it without vec
}

// 1 when every pointer is 16-byte aligned (a null pointer is: an output that is not written does not decide)
[[maybe_unused]] uint32_t all_aligned(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % 16) return 0;
    return 1;
}

}  // namespace

}  // namespace gbdpcg
