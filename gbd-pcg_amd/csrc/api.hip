// api.hip -- the handle of libgbdpcg.so (include/gbdpcg.h): its lifetime, settings and buffers, status strings, the size and occupancy
// queries, gbdpcg_reserve, graph launch / destroy, the CSR converter.  The solve is in api_solve.hip, the KKT calls in api_kkt.hip.
#include <cstdio>
#include <cstring>

#include "api_context.hpp"

namespace gbdpcg {
namespace {

// Grow *buf to at least `need` bytes (at least doubling); the old buffer is retired, not freed (see
// gbdpcg_context::retired).  Never called while a stream of this handle is capturing.
gbdpcg_status grow_buffer(gbdpcg_handle_t h, void **buf, size_t *cap, size_t need)
{
    if (need <= *cap) return GBDPCG_OK;
    size_t want = need > 2 * *cap ? need : 2 * *cap;
    want = (want + 255) / 256 * 256;
    void *fresh = nullptr;
    hipError_t e = hipMalloc(&fresh, want);
    if (e != hipSuccess && want != (need + 255) / 256 * 256) {  // doubling was too much: exactly what is needed
        want = (need + 255) / 256 * 256;
        e = hipMalloc(&fresh, want);
    }
    if (e != hipSuccess) {
        h->last_err = e;
        return GBDPCG_ERR_ALLOC;
    }
    if (*buf) {
        try {
            h->retired.push_back(*buf);
        } catch (const std::bad_alloc &) {
            (void)hipFree(fresh);
            return GBDPCG_ERR_ALLOC;
        }
    }
    *buf = fresh;
    *cap = want;
    return GBDPCG_OK;
}

constexpr size_t kRejectRoom = 256;

// The query or the call for the element size the caller named: f(float{}) or f(double{}) (8: double, as ever; anything else: float).
template <typename F> auto by_elem_size(uint32_t elem_size, F &&f)
{
    if (elem_size == 8) return f(double{});
    return f(float{});
}

template <typename T>
gbdpcg_status csr_to_bt_impl(uint32_t n, uint32_t N, const uint32_t *row_ptr, const uint32_t *col_ind,
                             const T *val, T *h_M)
{
    if (!row_ptr || !col_ind || !val || !h_M || n == 0 || N == 0) return GBDPCG_ERR_INVALID;
    const size_t total = (size_t)3 * n * n * N;
    for (size_t i = 0; i < total; ++i) h_M[i] = T(0);
    const uint32_t rows = n * N;
    for (uint32_t row = 0; row < rows; ++row) {
        const uint32_t k = row / n, r = row - k * n;
        for (uint32_t q = row_ptr[row]; q < row_ptr[row + 1]; ++q) {
            const uint32_t col = col_ind[q];
            if (col >= rows) return GBDPCG_ERR_INVALID;
            const uint32_t kc = col / n, c = col - kc * n;
            if (kc + 1 < k || kc > k + 1) {
                if (val[q] != T(0)) return GBDPCG_ERR_INVALID;  // outside the block-tridiagonal pattern
                continue;
            }
            const uint32_t b = kc + 1 - k;  // 0: L, 1: D, 2: R
            h_M[(size_t)k * 3 * n * n + (size_t)b * n * n + (size_t)c * n + r] += val[q];
        }
    }
    return GBDPCG_OK;
}

}  // namespace

gbdpcg_status ensure_ws(gbdpcg_handle_t h, size_t bytes) { return grow_buffer(h, &h->ws, &h->ws_bytes, bytes); }

gbdpcg_status get_pws(gbdpcg_handle_t h, uint32_t elem, uint32_t n, uint32_t N, uint32_t batch, size_t bytes, bool may_allocate,
                      void **out)
{
    const uint64_t key = ((uint64_t)elem << 60) ^ ((uint64_t)n << 48) ^ ((uint64_t)N << 24) ^ (uint64_t)batch;
    for (const auto &e : h->pws)
        if (e.key == key) {
            *out = h->pws_last = e.buf;
            return GBDPCG_OK;
        }
    if (!may_allocate) return GBDPCG_ERR_ALLOC;
    void *buf = nullptr;
    hipError_t e = hipMalloc(&buf, bytes);
    if (e != hipSuccess) {
        h->last_err = e;
        return GBDPCG_ERR_ALLOC;
    }
    e = hipMemset(buf, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) {
        try {
            h->pws.push_back({key, buf});
        } catch (const std::bad_alloc &) {
            e = hipErrorOutOfMemory;
        }
    }
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return fail(h, e);
    }
    *out = h->pws_last = buf;
    return GBDPCG_OK;
}

uint32_t *reject_words(gbdpcg_handle_t h) { return reinterpret_cast<uint32_t *>(h->sym_flags + h->sym_cap); }
gbdpcg_status ensure_sym_flags(gbdpcg_handle_t h, size_t bytes)
{
    if (h->sym_flags && bytes <= h->sym_cap) return GBDPCG_OK;
    const gbdpcg_status st =
        grow_buffer(h, reinterpret_cast<void **>(&h->sym_flags), &h->sym_alloc, (bytes + 255) / 256 * 256 + kRejectRoom);
    if (st != GBDPCG_OK) return st;
    h->sym_cap = h->sym_alloc - kRejectRoom;   // (grow_buffer rounds to 256 bytes)
    // the count reads 0 wherever no verifying launch has counted: done before any stream of the caller can use the buffer
    hipError_t e = hipMemset(reject_words(h), 0, kRejectRoom);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? GBDPCG_OK : fail(h, e);
}

}  // namespace gbdpcg

using namespace gbdpcg;

extern "C" {

gbdpcg_status gbdpcg_create(gbdpcg_handle_t *out, int device)
{
    if (!out) return GBDPCG_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
        return GBDPCG_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GBDPCG_ERR_NO_DEVICE;
    // this library carries gfx950 code objects only
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return GBDPCG_ERR_NO_DEVICE;
    gbdpcg_context *h = new (std::nothrow) gbdpcg_context;
    if (!h) return GBDPCG_ERR_ALLOC;
    h->dev.device = device;
    h->dev.num_cus = prop.multiProcessorCount;
    // gfx950: 160 KiB of LDS per CU, and one workgroup may take all of it (hipDeviceProp_t reports the
    // 64 KiB default window; larger dynamic sizes are opted into per kernel with hipFuncSetAttribute)
    h->dev.lds_per_cu = 160 * 1024;
    h->dev.lds_per_wg_max = 160 * 1024;
    DeviceScope scope(device);
    hipError_t e = scope.err;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->d_iters), 256);
    if (e == hipSuccess) e = hipMalloc(&h->cluster_ws, cluster_workspace_bytes(h->dev));
    if (e == hipSuccess) e = hipMemset(h->cluster_ws, 0, cluster_workspace_bytes(h->dev));
    if (e == hipSuccess) e = hipMalloc(&h->cluster_rescue, cluster_rescue_bytes(h->dev));
    if (e == hipSuccess) e = hipDeviceSynchronize();   // the fill is done before any stream of the caller can use the handle
    if (e == hipSuccess) {
        h->d_exit = reinterpret_cast<uint8_t *>(h->d_iters) + 128;
        // coherent (fine-grained) mapping: the device-side bump of h_done must reach the host while the stream still runs
        e = hipHostMalloc(reinterpret_cast<void **>(&h->h_iters), 256, hipHostMallocCoherent | hipHostMallocMapped);
    }
    if (e != hipSuccess) {
        if (h->d_iters) (void)hipFree(h->d_iters);
        if (h->cluster_ws) (void)hipFree(h->cluster_ws);
        if (h->cluster_rescue) (void)hipFree(h->cluster_rescue);
        delete h;
        return GBDPCG_ERR_HIP;
    }
    h->h_exit = reinterpret_cast<uint8_t *>(h->h_iters) + 128;
    h->h_done = h->h_iters + 16;
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&h->h_done_dev), h->h_done, 0) != hipSuccess) h->h_done_dev = nullptr;
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&h->h_iters_dev), h->h_iters, 0) == hipSuccess)
        h->h_exit_dev = reinterpret_cast<uint8_t *>(h->h_iters_dev) + 128;
    else
        h->h_iters_dev = nullptr;
    *out = h;
    return GBDPCG_OK;
}

gbdpcg_status gbdpcg_destroy(gbdpcg_handle_t h)
{
    if (!h) return GBDPCG_ERR_INVALID;
    DeviceScope scope(h->dev.device);
    if (h->ws) (void)hipFree(h->ws);
    for (const auto &e : h->pws) (void)hipFree(e.buf);
    if (h->sym_flags) (void)hipFree(h->sym_flags);
    if (h->cluster_ws) (void)hipFree(h->cluster_ws);
    if (h->cluster_rescue) (void)hipFree(h->cluster_rescue);
    for (void *old : h->retired) (void)hipFree(old);
    if (h->d_iters) (void)hipFree(h->d_iters);
    if (h->h_iters) (void)hipHostFree(h->h_iters);
    delete h;
    return GBDPCG_OK;
}

const char *gbdpcg_status_string(gbdpcg_status s)
{
    switch (s) {
    case GBDPCG_OK: return "ok";
    case GBDPCG_ERR_INVALID: return "invalid argument";
    case GBDPCG_ERR_HIP: return "HIP runtime error";
    case GBDPCG_ERR_NO_DEVICE: return "no usable gfx950 device";
    case GBDPCG_ERR_UNSUPPORTED: return "unsupported shape";
    case GBDPCG_ERR_TOO_LARGE: return "problem does not fit on the device";
    case GBDPCG_ERR_ALLOC: return "allocation failed (or workspace growth requested during stream capture)";
    case GBDPCG_ERR_NOT_IMPLEMENTED: return "not implemented";
    }
    return "unknown status";
}

int gbdpcg_last_hip_error(gbdpcg_handle_t h) { return h ? (int)h->last_err : (int)hipErrorInvalidValue; }
const char *gbdpcg_last_hip_error_string(gbdpcg_handle_t h)
{
    return hipGetErrorString(h ? h->last_err : hipErrorInvalidValue);
}

gbdpcg_status gbdpcg_set_path(gbdpcg_handle_t h, gbdpcg_path path)
{
    if (!h || (int)path < 0 || (int)path > 4) return GBDPCG_ERR_INVALID;
    h->forced = path;
    return GBDPCG_OK;
}

gbdpcg_status gbdpcg_set_symmetric(gbdpcg_handle_t h, int mode)
{
    if (!h || mode < 0 || mode > 2) return GBDPCG_ERR_INVALID;
    h->symmetric = mode;
    return GBDPCG_OK;
}
gbdpcg_path gbdpcg_choose_path(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N, uint32_t batch)
{
    if (!h || !shape_ok(n, N, batch)) return GBDPCG_PATH_AUTO;
    return by_elem_size(elem_size, [&](auto t) { return pick_path<decltype(t)>(h, n, N, batch); });
}

uint32_t gbdpcg_cluster_members(uint32_t elem_size, uint32_t n, uint32_t N)
{
    if (!shape_ok(n, N, 1)) return 0;
    return by_elem_size(elem_size, [&](auto t) { return cluster_members<decltype(t)>(n, N); });
}

size_t gbdpcg_pcg_shared_mem_size(uint32_t elem_size, uint32_t n, uint32_t N)
{
    const size_t nn = (size_t)n * n, mx = n > N ? n : N;
    const size_t a = 6 * nn + 10 * (size_t)n + 2 * mx, b = 9 * nn;
    return elem_size * (a > b ? a : b);
}

gbdpcg_status gbdpcg_check_occupancy(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N, uint32_t batch)
{
    if (!h || (elem_size != 4 && elem_size != 8) || !shape_ok(n, N, batch)) return GBDPCG_ERR_INVALID;
    if (!by_elem_size(elem_size, [&](auto t) { return mappable<decltype(t)>(n); })) return GBDPCG_ERR_UNSUPPORTED;
    // FUSED needs one workgroup's LDS; SPLIT needs its workspace in HBM and one (rpw=1) window in LDS.
    if (by_elem_size(elem_size, [&](auto t) { return fused_fits<decltype(t)>(h->dev, n, N); })) return GBDPCG_OK;
    if ((size_t)3 * n * elem_size + 64 * elem_size > h->dev.lds_per_wg_max) return GBDPCG_ERR_TOO_LARGE;
    size_t free_b = 0, total_b = 0;
    DEVICE_SCOPE(h);
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    const size_t need = gbdpcg_workspace_bytes(h, elem_size, n, N, batch);
    return need <= h->ws_bytes || need <= free_b ? GBDPCG_OK : GBDPCG_ERR_TOO_LARGE;  // growth keeps the old buffer
}

size_t gbdpcg_workspace_bytes(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N, uint32_t batch)
{
    if (!h || !shape_ok(n, N, batch)) return 0;
    return by_elem_size(elem_size, [&](auto t) -> size_t {
        using T = decltype(t);
        const gbdpcg_path p = pick_path<T>(h, n, N, batch);
        if (p == GBDPCG_PATH_FUSED) return 0;
        return (p == GBDPCG_PATH_PERSISTENT || p == GBDPCG_PATH_PERSISTENT_1R) ? persist_total_bytes<T>(n, N, batch)
                                                                              : split_workspace_bytes<T>(n, N, batch);
    });
}

gbdpcg_status gbdpcg_reserve(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N, uint32_t batch)
{
    if (!h || (elem_size != 4 && elem_size != 8) || !shape_ok(n, N, batch)) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    return by_elem_size(elem_size, [&](auto t) {
        using T = decltype(t);
        // the verdict bytes of the device symmetry check (mode 2) must exist before a capture as well
        gbdpcg_status st = ensure_sym_flags(h, verdict_bytes<T>(n, N, batch));
        if (st != GBDPCG_OK) return st;
        const gbdpcg_path p = pick_path<T>(h, n, N, batch);
        void *pws = nullptr;
        if (p == GBDPCG_PATH_PERSISTENT || p == GBDPCG_PATH_PERSISTENT_1R)
            return get_pws(h, elem_size, n, N, batch, persist_total_bytes<T>(n, N, batch), true, &pws);
        // a batch that a later solve may cut into persistent launches (persist_slices: whether it does depends on that call's
        // max_iter): the slices' hand-off words as well as the split path's workspace
        if (const uint32_t per = persist_slices<T>(h, n, N, batch, 0x7fffffffu)) {
            for (uint32_t nb : {per, batch % per}) {
                if (nb == 0) continue;
                st = get_pws(h, elem_size, n, N, nb, persist_total_bytes<T>(n, N, nb), true, &pws);
                if (st != GBDPCG_OK) return st;
            }
        }
        return ensure_ws(h, p == GBDPCG_PATH_FUSED ? 0 : split_workspace_bytes<T>(n, N, batch));
    });
}

gbdpcg_status gbdpcg_graph_launch(gbdpcg_graph_t g, void *stream)
{
    if (!g || !g->exec) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(g->h);
    HIP_TRY(g->h, hipGraphLaunch(g->exec, (hipStream_t)stream));
    return GBDPCG_OK;
}

gbdpcg_status gbdpcg_graph_destroy(gbdpcg_graph_t g)
{
    if (!g) return GBDPCG_ERR_INVALID;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return GBDPCG_OK;
}
#define GBDPCG_CSR_TO_BT(SUF, TYPE)                                                                                                 \
    gbdpcg_status gbdpcg_csr_to_bt_##SUF(uint32_t n, uint32_t N, const uint32_t *row_ptr, const uint32_t *col_ind, const TYPE *val,  \
                                         TYPE *h_M)                                                                                 \
    {                                                                                                                               \
        return csr_to_bt_impl<TYPE>(n, N, row_ptr, col_ind, val, h_M);                                                              \
    }
GBDPCG_CSR_TO_BT(f32, float)
GBDPCG_CSR_TO_BT(f64, double)
#undef GBDPCG_CSR_TO_BT

const char *gbdpcg_version(void) { return "gbdpcg 0.1 gfx950"; }

// For the tests and tools of this repository only (not in gbdpcg.h, may change): where the handle keeps device state that no entry
// point returns.  which = 0: the verdict bytes of symmetric mode 2, 1: the reject words behind them (PcgArgs::reject_count),
// 2: the cluster path's workspace (u64 word 31 is the launch number).  nullptr: not allocated yet, or no such state.
void *gbdpcg_internal_state(gbdpcg_handle_t h, int which)
{
    if (!h) return nullptr;
    if (which == 0) return h->sym_flags;
    if (which == 1) return h->sym_flags ? reject_words(h) : nullptr;
    if (which == 2) return h->cluster_ws;
    return nullptr;
}

#if defined(GBDPCG_CL_STAMPS) || defined(GBDPCG_RS_STAMPS)
// diagnostic builds only (tools/cluster_stamps.py, tools/rs_stamps.py): the cluster path's workspace holds the stamps
void *gbdpcg_internal_cluster_ws(gbdpcg_handle_t h) { return h ? h->cluster_ws : nullptr; }
#endif

#ifdef GBDPCG_PERSIST_STAMPS
// diagnostic build only (tools/persist_stamps.py): where the persistent path keeps its stamps
void *gbdpcg_internal_persist_ws(gbdpcg_handle_t h) { return h ? h->pws_last : nullptr; }
#endif

}  // extern "C"
