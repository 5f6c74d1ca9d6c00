// api_context.hpp -- private to the host units of libgbdpcg.so (api.hip, api_solve.hip, api_kkt.hip), never installed: the handle,
// the graph object, the helpers every entry point uses, and the few functions that cross those units.  No device code.
#pragma once

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/gbdpcg.h"
#include "internal.hpp"

struct gbdpcg_context {
    gbdpcg::DeviceInfo dev;
    gbdpcg_path forced = GBDPCG_PATH_AUTO;
    int symmetric = 2;  // gbdpcg_set_symmetric: 0 never, 1 assume, 2 check on the device (default)
    uint8_t *sym_flags = nullptr;  // [sym_cap] per-problem result of the check
    size_t sym_cap = 0;
    // Behind the verdict bytes, at sym_flags + sym_cap (256-byte aligned: it shares no dword, and no cache line, with a verdict
    // byte): the two words of PcgArgs::reject_count.  Zeroed once when the buffer is allocated; a step leaves them zero.
    size_t sym_alloc = 0;          // bytes of the allocation: sym_cap + kRejectRoom
    hipError_t last_err = hipSuccess;
    // status words for the blocking entry points (replace the per-call cudaMalloc of interface.cuh:105-108)
    uint32_t *d_iters = nullptr;
    uint8_t *d_exit = nullptr;
    uint32_t *h_iters = nullptr;  // pinned
    uint8_t *h_exit = nullptr;    // pinned
    uint32_t *h_done = nullptr;   // pinned, device-visible: problems that reported convergence (blocking split solves)
    uint32_t *h_done_dev = nullptr;
    uint32_t *h_iters_dev = nullptr;  // device views of h_iters / h_exit: the blocking entry points let the kernels
    uint8_t *h_exit_dev = nullptr;    // write the two status words straight to the host (no copy-back)
    // split-path workspace, grown on demand outside capture
    void *ws = nullptr;
    size_t ws_bytes = 0;
    // persistent path: hand-off slots and epoch bases.  One zero-filled buffer PER SHAPE (element size, n, N, batch), made
    // outside capture on first use and kept until the handle goes: the slot layout depends on the shape, and a buffer
    // that only ever sees one layout can never show a launch a stale tag left by another (graphs captured for a shape
    // keep pointing at that shape's buffer).
    struct PersistWs {
        uint64_t key;
        void *buf;
    };
    std::vector<PersistWs> pws;
    // cluster path (pcg_cluster.hip): hand-off slots, one per CU and epoch parity.  Made with the handle (its size does not
    // depend on the shape) and zero-filled once; launches never clear it (a tag carries the launch number, and the word
    // that counts launches lives in it).
    void *cluster_ws = nullptr;
    void *cluster_rescue = nullptr;   // vectors of the cluster path's in-kernel rescue (cluster_rescue_bytes)
    void *pws_last = nullptr;   // diagnostic builds only (gbdpcg_internal_persist_ws)
    // Buffers replaced by a larger one.  Graphs built earlier (gbdpcg_graph_create_solve_*, or a caller's own
    // capture of gbdpcg_solve_*) hold the OLD pointers in their kernel nodes, so growth never frees: the old
    // buffer stays valid until the handle goes.  Sizes at least double, which bounds the total at 2x the largest.
    std::vector<void *> retired;
};

struct gbdpcg_graph {
    gbdpcg_handle_t h = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

namespace gbdpcg {

inline gbdpcg_status fail(gbdpcg_handle_t h, hipError_t e)
{
    if (h) h->last_err = e;
    return GBDPCG_ERR_HIP;
}

#define HIP_TRY(h, expr)                                \
    do {                                                \
        hipError_t e__ = (expr);                        \
        if (e__ != hipSuccess) return fail((h), e__);   \
    } while (0)

// Every entry point runs with the handle's device current and puts the caller's device back on return (a host
// thread that loops over the handles of several GPUs keeps whatever device it had selected).
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceScope()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};
#define DEVICE_SCOPE(h)                          \
    DeviceScope device_scope__((h)->dev.device); \
    if (device_scope__.err != hipSuccess) return fail((h), device_scope__.err)

inline bool shape_ok(uint32_t n, uint32_t N, uint32_t batch)
{
    if (n == 0 || N == 0 || batch == 0) return false;
    // index arithmetic inside the kernels is 32-bit within one problem
    if ((uint64_t)3 * n * n * N >= (1ull << 31)) return false;
    return true;
}

template <typename T> bool mappable(uint32_t n)
{
    const void *none[1] = {nullptr};
    return choose_vec<T>(n, none, 1) != 0;
}

// ---- api.hip: the handle's buffers.  None of these is called while a stream of the handle is capturing.
// The split path's workspace: at least `bytes` (growth at least doubles; the old buffer is retired, not freed).
gbdpcg_status ensure_ws(gbdpcg_handle_t h, size_t bytes);
// `bytes` verdict bytes and, behind them, the reject words (gbdpcg_context::sym_alloc).
gbdpcg_status ensure_sym_flags(gbdpcg_handle_t h, size_t bytes);
uint32_t *reject_words(gbdpcg_handle_t h);
// The persistent path's workspace of one shape (see gbdpcg_context::pws): found, or -- may_allocate -- allocated and zero-filled
// (epoch bases and tags must read zero where nothing was ever written); GBDPCG_ERR_ALLOC where it is neither.
gbdpcg_status get_pws(gbdpcg_handle_t h, uint32_t elem, uint32_t n, uint32_t N, uint32_t batch, size_t bytes, bool may_allocate,
                      void **out);

// Bytes of a shape's persistent-path buffer: the hand-off words, then (256-byte aligned) the vectors of the workgroup that
// solves a problem alone when its launch could not get its workgroups together (pcg_stream.hpp).
template <typename T> size_t persist_rescue_offset(uint32_t n, uint32_t N, uint32_t batch)
{
    return (persist_workspace_bytes<T>(n, N, batch) + 255) / 256 * 256;
}
template <typename T> size_t persist_total_bytes(uint32_t n, uint32_t N, uint32_t batch)
{
    return persist_rescue_offset<T>(n, N, batch) + persist_rescue_bytes<T>(n, N, batch);
}

// ---- api_solve.hip (instantiated there for float and double)
template <typename T> gbdpcg_path pick_path(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch);
// Problems per persistent launch where AUTO cuts a batch into several; 0: it does not.
template <typename T> uint32_t persist_slices(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, uint32_t max_iter);
// Verdict bytes a (n, N, batch) solve in symmetric mode 2 may need.
template <typename T> size_t verdict_bytes(uint32_t n, uint32_t N, uint32_t batch);

// How a solve is run, next to what it solves (PcgArgs).
struct SolveOpts {
    bool blocking = false;          // the caller synchronises before it returns (the split path may poll the host counter)
    uint32_t verdict_stride = 0;    // != 0: the verdict bytes are in the handle already, this many per problem: no test launch
    bool known_symmetric = false;   // the caller inside this library KNOWS every problem is symmetric in storage
    bool shared = false;            // gbdpcg_solve_shared_*: a.S, a.Pinv are ONE pair of matrices for the whole batch
};
// The solve: `a` as the entry point built it (pcg_args; the handle's own fields of PcgArgs are filled in here).
template <typename T> gbdpcg_status solve(gbdpcg_handle_t h, const PcgArgs<T> &a, hipStream_t stream, const SolveOpts &o = {});
// Phi^-1 from a.S into d_Pinv (== a.Pinv), then the solve, on one stream.
template <typename T>
gbdpcg_status form_pinv_solve(gbdpcg_handle_t h, const PcgArgs<T> &a, T *d_Pinv, gbdpcg_pinv_kind kind, hipStream_t stream);
// What a graph of a (a.n, a.N, a.batch) solve needs from the handle before its capture starts.
template <typename T> gbdpcg_status graph_reserve(gbdpcg_handle_t h, const PcgArgs<T> &a, bool shared);

// The solve is described once, at the ABI boundary: the arguments of the C entry points in their order.
template <typename T>
PcgArgs<T> pcg_args(uint32_t n, uint32_t N, uint32_t batch, const T *d_S, const T *d_Pinv, const T *d_gamma, T *d_lambda, T *d_r, T *d_p,
                    T tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_exit)
{
    return PcgArgs<T>{d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, tol, max_iter, n, N, batch, d_iters, d_exit};
}
// (in the entry points, whose parameters carry these names; NX: the name of the block size there)
#define PCG_ARGS(TYPE, NX) \
    gbdpcg::pcg_args<TYPE>(NX, N, batch, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, tol, max_iter, d_iters, d_max_iter_exit)

// A graph of whatever `body` puts on the stream it is given (hipStream_t -> gbdpcg_status; it contains the solve of `a`): the
// handle's workspaces for that solve are reserved first, then the body is captured and the graph instantiated.  The eager entry
// point of a pair calls the same body on the caller's stream.
template <typename T, typename Body>
gbdpcg_status graph_create(gbdpcg_handle_t h, const PcgArgs<T> &a, bool shared, gbdpcg_graph_t *out, Body &&body)
{
    if (!h || !out) return GBDPCG_ERR_INVALID;
    *out = nullptr;
    if (!shape_ok(a.n, a.N, a.batch)) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    gbdpcg_status st = graph_reserve<T>(h, a, shared);
    if (st != GBDPCG_OK) return st;
    resident_prepare<T>(a.n, a.N);
    hipStream_t cs = nullptr;
    HIP_TRY(h, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    gbdpcg_graph *g = new (std::nothrow) gbdpcg_graph;
    if (!g) {
        (void)hipStreamDestroy(cs);
        return GBDPCG_ERR_ALLOC;
    }
    g->h = h;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        st = body(cs);
        hipError_t e2 = hipStreamEndCapture(cs, &g->graph);
        if (st == GBDPCG_OK && e2 != hipSuccess) st = fail(h, e2);
    } else {
        st = fail(h, e);
    }
    if (st == GBDPCG_OK) {
        e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
        if (e != hipSuccess) st = fail(h, e);
    }
    (void)hipStreamDestroy(cs);
    if (st != GBDPCG_OK) {
        if (g->exec) (void)hipGraphExecDestroy(g->exec);
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        return st;
    }
    *out = g;
    return GBDPCG_OK;
}

}  // namespace gbdpcg
