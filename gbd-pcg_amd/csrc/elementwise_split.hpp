// elementwise_split.hpp -- what the elementwise launches of the backward passes share (admm_adjoint.hip, admm_soft_grad.hip): the
// 16-byte vector of a type, the head / body / tail split of one problem's range, and the host's test that every base is aligned.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

namespace gbdpcg {

namespace {

template <typename T> struct AdjVec;
template <> struct AdjVec<float> {
    static constexpr uint32_t N = 4;
    typedef float type __attribute__((ext_vector_type(4)));
};
template <> struct AdjVec<double> {
    static constexpr uint32_t N = 2;
    typedef double type __attribute__((ext_vector_type(2)));
};

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

// 1 when every pointer is 16-byte aligned (a null pointer is: an output that is not written does not decide)
[[maybe_unused]] uint32_t all_aligned(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % 16) return 0;
    return 1;
}

}  // namespace

}  // namespace gbdpcg
