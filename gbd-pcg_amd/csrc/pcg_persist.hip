// pcg_persist.hip -- PCG for ONE large problem spread over many CUs inside a single persistent launch: the host side, and
// the kernels of the first group of block sizes.  The kernels themselves are in the headers behind pcg_persist_kernels.hpp
// (protocol: pcg_persist_handoff.hpp; lane map and shared steps: pcg_persist_geom.hpp; pcg_persist_2r.hpp, pcg_persist_1r.hpp);
// their instantiations -- 20 kernels per block size, the longest compile of the library -- are spread over three units that
// build side by side: this one (stateSize 14 - 20), pcg_persist_b.hip (22 - 28) and pcg_persist_c.hip (30 - 36).
#include "pcg_persist_kernels.hpp"

namespace gbdpcg {

// ---- host side ---------------------------------------------------------------------------------------------------

template <typename T> static bool persist_has_kernel(uint32_t n)
{
    return PersistGroup<0>::has(n) || PersistGroup<1>::has(n) || PersistGroup<2>::has(n);
}

// Knots per workgroup for this launch (0: the shape cannot run persistently): every workgroup must be resident at
// once, one per CU.
template <typename T> uint32_t persist_knots_per_wg(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch, bool one_reduction)
{
    static const bool off = getenv("GBDPCG_NO_PERSIST") != nullptr;   // tuning runs only
    if (off || !persist_has_kernel<T>(n)) return 0;
    static const int forced = [] {
        const char *e = getenv("GBDPCG_PERSIST_K");   // tuning runs only
        return e ? atoi(e) : 0;
    }();
    // two knots per workgroup measured fastest on config 4 (5.7 us per iteration; 6.2 with three, 6.9 with one)
    for (uint32_t K : {2u, 3u, 1u}) {
        if (forced && (uint32_t)forced != K) continue;
        if (one_reduction && K < 2) continue;   // its first and last own knots carry one halo block-row each
        if ((uint64_t)((N + K - 1) / K) * batch <= (uint64_t)dev.num_cus && (N + K - 1) / K <= 256) return K;
    }
    return 0;
}

template <typename T> size_t persist_workspace_bytes(uint32_t n, uint32_t N, uint32_t batch)
{
    return persist_words<T>(n, N) * sizeof(u64) * batch;
}

template <typename T> size_t persist_rescue_bytes(uint32_t n, uint32_t N, uint32_t batch)
{
    return rescue_vec_elems<T>(n, N) * sizeof(T) * batch;
}

template <typename T>
hipError_t launch_pcg_persist(const DeviceInfo &dev, const PcgArgs<T> &a, void *workspace, hipStream_t s, bool one_reduction)
{
    const uint32_t K = persist_knots_per_wg<T>(dev, a.n, a.N, a.batch, one_reduction);
    if (K == 0 || workspace == nullptr) return hipErrorInvalidValue;
    if (PersistGroup<0>::has(a.n)) return launch_pcg_persist_group<T, 0>(a, workspace, s, one_reduction, K);
    if (PersistGroup<1>::has(a.n)) return launch_pcg_persist_group<T, 1>(a, workspace, s, one_reduction, K);
    if (PersistGroup<2>::has(a.n)) return launch_pcg_persist_group<T, 2>(a, workspace, s, one_reduction, K);
    return hipErrorInvalidValue;
}

template uint32_t persist_knots_per_wg<float>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, bool);
template uint32_t persist_knots_per_wg<double>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, bool);
template size_t persist_workspace_bytes<float>(uint32_t, uint32_t, uint32_t);
template size_t persist_workspace_bytes<double>(uint32_t, uint32_t, uint32_t);
template size_t persist_rescue_bytes<float>(uint32_t, uint32_t, uint32_t);
template size_t persist_rescue_bytes<double>(uint32_t, uint32_t, uint32_t);
template hipError_t launch_pcg_persist<float>(const DeviceInfo &, const PcgArgs<float> &, void *, hipStream_t, bool);
template hipError_t launch_pcg_persist<double>(const DeviceInfo &, const PcgArgs<double> &, void *, hipStream_t, bool);
GBDPCG_PERSIST_GROUP(, 0)

}  // namespace gbdpcg
