// pcg_persist_kernels.hpp -- the kernels of the persistent family and their launch, in headers so that the instantiations -- 20
// kernels per block size, the longest compile of the library -- build in three units side by side: pcg_persist.hip (block sizes
// 14 - 20), pcg_persist_b.hip (22 - 28), pcg_persist_c.hip (30 - 36).  What the kernels do: pcg_persist_handoff.hpp.
#pragma once

#include "pcg_persist_1r.hpp"
#include "pcg_persist_2r.hpp"

namespace gbdpcg {

// ---- launch of one instantiation (host) ----------------------------------------------------------------------------

template <typename T, int NCT, int K>
static hipError_t launch_persist_k(const PcgArgs<T> &a, void *workspace, hipStream_t s, bool one_reduction)
{
    const uint32_t W = (a.N + K - 1) / K;
    // ~1 us per failed pass: a workgroup gives up after about two seconds of waiting.  One that only arrives when the others
    // are about to give up waits its own bound after theirs: up to two bounds, then the streaming solve of the last to leave.
    uint32_t spin_limit = 1u << 21, hold_wg = 0u, hold_us = 0u;
#ifdef GBDPCG_TEST_HOOKS
    // variants/libgbdpcg_hooks.so only (tests/test_gpu_persist.py): a short spin bound, a launch that is missing its last
    // workgroup, a workgroup that arrives late -- to drive the give-up path.  The shipped library has none of this.
    if (const char *e = getenv("GBDPCG_PERSIST_SPIN_LIMIT")) spin_limit = (uint32_t)atoi(e);
    if (const char *e = getenv("GBDPCG_PERSIST_HOLD_US")) {
        hold_us = (uint32_t)atoi(e);
        hold_wg = W - 1u;
    }
    if (getenv("GBDPCG_PERSIST_DROP_WG")) hold_us = 0xffffffffu;
    const bool rescue_off = getenv("GBDPCG_RESCUE_OFF") != nullptr;   // show a test what a launch that gave up leaves behind
#else
    const bool rescue_off = false;
#endif
    PcgArgs<T> ka = a;
    ka.rescue_off = rescue_off;
    const dim3 grid(W * a.batch), block(K * PersistGeom<T, NCT>::TPK);
    u64 *ws = reinterpret_cast<u64 *>(workspace);
    if (one_reduction) {
        if constexpr (K >= 2) {
            if (a.Pinv) hipLaunchKernelGGL((pcg_persist1r_kernel<T, NCT, K, true>), grid, block, 0, s, ka, ws, W, spin_limit, hold_wg, hold_us);
            else hipLaunchKernelGGL((pcg_persist1r_kernel<T, NCT, K, false>), grid, block, 0, s, ka, ws, W, spin_limit, hold_wg, hold_us);
        } else {
            return hipErrorInvalidValue;
        }
    } else {
        // staged matrix loads (LDS-DMA) when both block-row sets of a workgroup fit the dynamic LDS next to the windows
        // and the matrices are 16-byte aligned
        static const bool no_staging = getenv("GBDPCG_PERSIST_DIRECT_LOADS") != nullptr;   // tuning runs only
        const size_t stage = (size_t)(a.Pinv ? 2 : 1) * K * 3 * NCT * NCT * sizeof(T);
        const bool staged = !no_staging && stage <= 128 * 1024 && !(reinterpret_cast<uintptr_t>(a.S) % 16) &&
                            !(a.Pinv && reinterpret_cast<uintptr_t>(a.Pinv) % 16);
        const size_t lds = staged ? stage : 0;
        auto kern = a.Pinv ? pcg_persist_kernel<T, NCT, K, true> : pcg_persist_kernel<T, NCT, K, false>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, block, lds, s, ka, ws, W, spin_limit, staged ? 1u : 0u, hold_wg, hold_us);
    }
    return hipGetLastError();
}

// One block size: the kernels of K = 1, 2 or 3 knots per workgroup
template <typename T, int NN>
static hipError_t launch_persist_n(const PcgArgs<T> &a, void *workspace, hipStream_t s, bool one_reduction, uint32_t K)
{
    if (K == 1) return launch_persist_k<T, NN, 1>(a, workspace, s, one_reduction);
    if (K == 2) return launch_persist_k<T, NN, 2>(a, workspace, s, one_reduction);
    return launch_persist_k<T, NN, 3>(a, workspace, s, one_reduction);
}

// Block sizes with persistent kernels: BASELINE's 14 and 36 and every even size in between (one problem of any other size
// takes the split path, whose hipGraph is 2 max_iter + 4 launches whatever the iteration count), in the three groups that
// compile side by side.
template <int... NN> struct PersistSizes {
    static bool has(uint32_t n) { return ((n == (uint32_t)NN) || ...); }
};
template <int G> struct PersistGroup;
template <> struct PersistGroup<0> : PersistSizes<14, 16, 18, 20> {};   // pcg_persist.hip
template <> struct PersistGroup<1> : PersistSizes<22, 24, 26, 28> {};   // pcg_persist_b.hip
template <> struct PersistGroup<2> : PersistSizes<30, 32, 34, 36> {};   // pcg_persist_c.hip

template <typename T, int... NN>
static hipError_t launch_persist_sizes(PersistSizes<NN...>, const PcgArgs<T> &a, void *workspace, hipStream_t s, bool one_reduction,
                                       uint32_t K)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((a.n == (uint32_t)NN && (e = launch_persist_n<T, NN>(a, workspace, s, one_reduction, K), true)) || ...);
    return e;
}

// The kernels of group G.  Not inline, and declared extern below: only the unit that instantiates a group explicitly compiles
// its kernels.
template <typename T, int G>
hipError_t launch_pcg_persist_group(const PcgArgs<T> &a, void *workspace, hipStream_t s, bool one_reduction, uint32_t K)
{
    return launch_persist_sizes<T>(PersistGroup<G>{}, a, workspace, s, one_reduction, K);
}
#define GBDPCG_PERSIST_GROUP(KEYWORD, G)                                                                                           \
    KEYWORD template hipError_t launch_pcg_persist_group<float, G>(const PcgArgs<float> &, void *, hipStream_t, bool, uint32_t);   \
    KEYWORD template hipError_t launch_pcg_persist_group<double, G>(const PcgArgs<double> &, void *, hipStream_t, bool, uint32_t);
GBDPCG_PERSIST_GROUP(extern, 0)
GBDPCG_PERSIST_GROUP(extern, 1)
GBDPCG_PERSIST_GROUP(extern, 2)

}  // namespace gbdpcg
