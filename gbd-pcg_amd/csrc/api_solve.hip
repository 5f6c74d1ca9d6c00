// api_solve.hip -- the solve behind the C ABI (include/gbdpcg.h): which path a shape takes, the solve and its blocking and host
// forms, Phi^-1 + solve, SpMV and the symmetry check, and the graphs of the plain and the shared solve.  Host code only.
#include <cassert>
#include <cstdlib>

#include "api_context.hpp"

namespace gbdpcg {

template <typename T> int choose_vec(uint32_t n, const void *const *ptrs, int nptrs)
{
    const int cand[3] = {4, 2, 1};
    for (int V : cand) {
        if (V * sizeof(T) > 16 || n % V != 0 || n / V > 64) continue;
        bool ok = true;
        for (int i = 0; i < nptrs; ++i)
            if (ptrs[i] && reinterpret_cast<uintptr_t>(ptrs[i]) % (V * sizeof(T)) != 0) ok = false;
        if (ok) return V;
    }
    return 0;
}
template int choose_vec<float>(uint32_t, const void *const *, int);
template int choose_vec<double>(uint32_t, const void *const *, int);

template <typename T> gbdpcg_path pick_path(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch)
{
    const bool fits = fused_fits<T>(h->dev, n, N);
    const bool persist = persist_knots_per_wg<T>(h->dev, n, N, batch) != 0;
    if (h->forced == GBDPCG_PATH_PERSISTENT_1R && persist_knots_per_wg<T>(h->dev, n, N, batch, true) != 0)
        return GBDPCG_PATH_PERSISTENT_1R;
    if (h->forced == GBDPCG_PATH_PERSISTENT || h->forced == GBDPCG_PATH_PERSISTENT_1R)
        return persist ? GBDPCG_PATH_PERSISTENT : (fits ? GBDPCG_PATH_FUSED : GBDPCG_PATH_SPLIT);
    if (h->forced == GBDPCG_PATH_FUSED) return fits ? GBDPCG_PATH_FUSED : GBDPCG_PATH_SPLIT;
    if (h->forced == GBDPCG_PATH_SPLIT) return GBDPCG_PATH_SPLIT;
    // A problem too large for one workgroup: one persistent launch over many CUs when all of its workgroups can be
    // resident together (measured on config 4, n=36 N=256 fp64: see DESIGN.md), else two launches per iteration.
    if (!fits) return persist ? GBDPCG_PATH_PERSISTENT : GBDPCG_PATH_SPLIT;
    // Fits one workgroup but would stream both matrices through ONE CU's share of the fabric every iteration
    // (43 GB/s measured, below): the persistent launch keeps them in registers and pays ~5.7 us per iteration.
    const bool cluster = cluster_members<T>(n, N) != 0;   // general storage resident over 2-4 CUs (pcg_cluster.hip)
    if (persist && !cluster && !resident_shape<T>(n, N) && !(h->symmetric != 0 && resident_sym_shape<T>(n, N)) &&
        6.0 * n * n * N * sizeof(T) / 43e9 > 6e-6)
        return GBDPCG_PATH_PERSISTENT;
    // Shapes whose matrices stay on the CU for the whole solve: fused, whatever the batch.  (Symmetric mode 2
    // decides per problem on the device; the path is chosen for the problems that pass.)
    if (resident_shape<T>(n, N)) return GBDPCG_PATH_FUSED;
    if (h->symmetric != 0 && resident_sym_shape<T>(n, N)) return GBDPCG_PATH_FUSED;
    if (cluster) return GBDPCG_PATH_FUSED;
    if (batch >= (uint32_t)h->dev.num_cus) return GBDPCG_PATH_FUSED;  // every CU has a problem of its own to stream
    // Streaming, fewer problems than CUs.  FUSED: one workgroup per problem pulls both matrices through ONE CU's
    // share of the fabric every iteration (43 GB/s measured on the general kernel: 13.9 us per iteration for the
    // 602 KB of n=14, N=128 fp32, at any batch below the CU count).  SPLIT: the whole chip streams, at the price of
    // two dependent launches per iteration (measured on the same shape: 7.5 us at batch 1, 7.8 at 8, 11.8 at 32,
    // 13.9 at 64 = 7.4 us + batch x bytes at ~6 TB/s).
    const double bytes = 6.0 * n * n * N * sizeof(T);
    const double t_fused = bytes / 43e9, t_split = 7.4e-6 + batch * bytes / 6e12;
    return t_split < t_fused ? GBDPCG_PATH_SPLIT : GBDPCG_PATH_FUSED;
}
template gbdpcg_path pick_path<float>(gbdpcg_handle_t, uint32_t, uint32_t, uint32_t);
template gbdpcg_path pick_path<double>(gbdpcg_handle_t, uint32_t, uint32_t, uint32_t);

// A few problems too many for ONE persistent launch (stateSize 20 ... 36 beyond the on-chip kernels: one or two, at short horizons
// four or five, per launch) used to fall to the split path, whose hipGraph is 2 max_iter + 4 launches whatever the iteration count
// (8 problems of 24 x 128 under max_iter = 100: 370 us of launches for nine iterations).  They are solved by a few persistent
// launches in a row instead, `persist_slices` problems each, when that row is shorter than the split path's launches alone:
// 25 us of fixed cost per persistent launch against 1.8 us per launch of the split graph.  0: no slicing.
// (tests/test_gpu_footprint.py, slices(), restates this rule with these constants to know which launches a case reaches.)
template <typename T> uint32_t persist_slices(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, uint32_t max_iter)
{
    static const bool off = getenv("GBDPCG_NO_PERSIST_SLICES") != nullptr;   // tuning runs only
    if (off || h->forced != GBDPCG_PATH_AUTO || pick_path<T>(h, n, N, batch) != GBDPCG_PATH_SPLIT) return 0;
    uint32_t cap = 0;
    for (uint32_t b = 1; b <= 64 && b < batch && persist_knots_per_wg<T>(h->dev, n, N, b) != 0; ++b) cap = b;
    if (cap == 0) return 0;
    const uint32_t launches = (batch + cap - 1) / cap;
    if (launches > 16 || 25.0 * launches >= 1.8 * (2.0 * max_iter + 4.0)) return 0;
    return cap;
}
template uint32_t persist_slices<float>(gbdpcg_handle_t, uint32_t, uint32_t, uint32_t, uint32_t);
template uint32_t persist_slices<double>(gbdpcg_handle_t, uint32_t, uint32_t, uint32_t, uint32_t);

// Verdict bytes a (n, N, batch) solve in symmetric mode 2 may need: the larger of what the test kernel and the
// one-launch stair kernel write per problem.
// (never less than one byte per problem: the verifying resident launch writes that many; the words in which that launch counts
// the problems it rejects come on top, in ensure_sym_flags, through which every caller of this -- gbdpcg_reserve and the graph
// constructors -- allocates)
template <typename T> size_t verdict_bytes(uint32_t n, uint32_t N, uint32_t batch)
{
    const uint32_t a = check_pair_chunks<T>(n, N), b = pinv_verdict_chunks<T>(n, N, GBDPCG_PINV_STAIR);
    const uint32_t m = a > b ? a : b;
    const size_t bytes = (size_t)batch * (m ? m : 1);
    assert(bytes >= batch);
    return bytes;
}
template size_t verdict_bytes<float>(uint32_t, uint32_t, uint32_t);
template size_t verdict_bytes<double>(uint32_t, uint32_t, uint32_t);

namespace {

// Buffer X of the handle must hold what a launch needs.  If it already does (`enough`), fine; if the stream is capturing,
// GBDPCG_ERR_ALLOC: growing allocates and synchronises, the caller reserves first (gbdpcg_reserve, or the graph entry points, which
// do); otherwise grow() it.
template <typename Grow> gbdpcg_status hold(bool enough, hipStream_t stream, Grow &&grow)
{
    if (enough) return GBDPCG_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return GBDPCG_ERR_ALLOC;
    return grow();
}

}  // namespace

template <typename T> gbdpcg_status solve(gbdpcg_handle_t h, const PcgArgs<T> &in, hipStream_t stream, const SolveOpts &o)
{
    const uint32_t n = in.n, N = in.N, batch = in.batch, max_iter = in.max_iter;
    const T *const d_S = in.S, *const d_Pinv = in.Pinv;
    const bool shared = o.shared;
    if (!h || !d_S || !in.gamma || !in.lambda || !in.iters || !shape_ok(n, N, batch)) return GBDPCG_ERR_INVALID;
    if (!mappable<T>(n)) return GBDPCG_ERR_UNSUPPORTED;
    // a shared pair is solved by the fused family alone, whatever path the handle is set to: the persistent and split kernels
    // have no shared form
    if (shared && !fused_fits<T>(h->dev, n, N)) return GBDPCG_ERR_UNSUPPORTED;
    PcgArgs<T> a = in;
    a.cluster_ws = h->cluster_ws;
    a.rescue_vec = h->cluster_rescue;   // (the persistent path points it at its own buffer below)
    // problems the symmetry test of mode 2 looks at: the ONE pair of a shared batch is tested once, with the same kernels, and
    // every problem follows that verdict (the SHARED kernels read the verdict of problem 0 for all of them)
    const uint32_t vbatch = shared ? 1u : batch;
    DEVICE_SCOPE(h);
    if (const uint32_t per = shared ? 0u : persist_slices<T>(h, n, N, batch, max_iter)) {
        const size_t ms = (size_t)3 * n * n * N, vs = (size_t)n * N;
        for (uint32_t b0 = 0; b0 < batch; b0 += per) {
            PcgArgs<T> s = in;   // one slice: the same solve on the problems b0 ... b0 + s.batch - 1
            s.batch = batch - b0 < per ? batch - b0 : per;
            s.S += b0 * ms;
            if (s.Pinv) s.Pinv += b0 * ms;
            s.gamma += b0 * vs;
            s.lambda += b0 * vs;
            if (s.r) s.r += b0 * vs;
            if (s.p) s.p += b0 * vs;
            s.iters += b0;
            if (s.max_iter_exit) s.max_iter_exit += b0;
            const gbdpcg_status st = solve<T>(h, s, stream);
            if (st != GBDPCG_OK) return st;
        }
        return GBDPCG_OK;
    }
    const gbdpcg_path path = shared ? GBDPCG_PATH_FUSED : pick_path<T>(h, n, N, batch);
    if (path == GBDPCG_PATH_PERSISTENT || path == GBDPCG_PATH_PERSISTENT_1R) {
        // (capturing a shape this handle has not seen: gbdpcg_reserve first)
        void *pws = nullptr;
        const size_t bytes = persist_total_bytes<T>(n, N, batch);
        const gbdpcg_status st = hold(get_pws(h, sizeof(T), n, N, batch, bytes, false, &pws) == GBDPCG_OK, stream,
                                      [&] { return get_pws(h, sizeof(T), n, N, batch, bytes, true, &pws); });
        if (st != GBDPCG_OK) return st;
        // The workgroups of this launch wait for each other inside the kernel; if they cannot all get onto the device
        // (somebody else's kernel holds compute units) they give up, and the one that leaves last solves the problem alone
        // with these vectors (pcg_stream.hpp).  The reference refuses such a launch before it starts (pcg.cuh:23-49).
        a.rescue_vec = static_cast<unsigned char *>(pws) + persist_rescue_offset<T>(n, N, batch);
        HIP_TRY(h, launch_pcg_persist<T>(h->dev, a, pws, stream, path == GBDPCG_PATH_PERSISTENT_1R));
    } else if (path == GBDPCG_PATH_FUSED) {
        // shapes the cluster kernel keeps resident in general storage gain nothing from symmetric STREAMING: only the
        // CU-resident symmetric kernel (N <= 128) is worth a symmetry test there
        const bool cluster_only = cluster_members<T>(n, N) != 0 && !resident_sym_shape<T>(n, N);
        bool has_sym = h->symmetric != 0 && d_Pinv != nullptr && !cluster_only && fused_has_symmetric<T>(h->dev, n, N, batch);
        // A batch that one round of clusters holds (stateSize 14, N <= 128: up to 128 problems) is not worth the test either: the
        // cluster kernel solves it in general storage in one launch while the test, the symmetric launch and the general launch
        // that finds nothing to do would still be starting (measured, 1 / 16 / 64 / 128 problems to 1e-6: 50 / 46 / 47 / 53 us
        // against 52 / 61 / 65 / 74; from 160 problems on the two are level and the symmetric kernel then pulls away).
        const uint32_t members = cluster_members<T>(n, N);
        const bool one_cluster_round = members != 0 && (uint64_t)batch * members <= (uint64_t)h->dev.num_cus &&
                                       max_iter < (1u << 18) &&   // (its hand-off tags count 2 max_iter + 4 epochs per problem in 20 bits)
                                       !(reinterpret_cast<uintptr_t>(d_S) % 8) && !(d_Pinv && reinterpret_cast<uintptr_t>(d_Pinv) % 8);
        // (in every form of mode 2 -- also where the verdicts are already known and the two paths are level --, so that
        // gbdpcg_form_pinv_solve_* and gbdpcg_kkt_step_* stay bit-identical with the separate calls; mode 1, the caller's word, keeps
        // the symmetric kernel)
        if (h->symmetric == 2 && one_cluster_round) has_sym = false;
        if (has_sym && h->symmetric == 2 && o.known_symmetric) {
            // the caller inside this library KNOWS that every problem is symmetric in storage (gbdpcg_kkt_step_*: S written by
            // form_schur, Pinv by the stair kernel from that S): one launch, no test, no verdict bytes, no general launch
            a.symmetric = true;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
        } else if (has_sym && h->symmetric == 2 && o.verdict_stride) {
            // the verdict bytes are already in h->sym_flags, put there on this stream by the stair kernel that just
            // formed Pinv from S (gbdpcg_form_pinv_solve_*): no test launch
            a.sel_stride = o.verdict_stride;
            a.sel = h->sym_flags;
            a.symmetric = true;
            a.want = 1;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
            a.symmetric = false;
            a.want = 0;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
        } else if (has_sym && h->symmetric == 2 && !shared && resident_sym_verifies<T>(h->dev, n, N, d_S, d_Pinv)) {
            // AUTO on the CU-resident symmetric kernel: it takes EVERY problem and tests L_{k+1} == R_k^T itself, against the
            // tiles it holds anyway (no test launch, no second read of R); it writes one verdict byte per problem and leaves
            // the problems that fail untouched for the general launch, which takes exactly those.  One byte per problem:
            // verdict_bytes (what gbdpcg_reserve sizes) is never less.
            const gbdpcg_status st = hold(batch <= h->sym_cap, stream, [&] { return ensure_sym_flags(h, batch); });
            if (st != GBDPCG_OK) return st;
            a.symmetric = true;
            a.verdict_out = h->sym_flags;
            // the problems it rejects are counted on the device, and the general launch below returns at once when there are none
            // (whichever kernel launch_pcg_fused picks for it: the cluster kernel, or pcg_fused_kernel where that path is off or
            // refuses max_iter; the shapes of pcg_resident.hip never get here).  When there are some, that launch puts the count
            // back to 0 as it ends, so a step leaves the word as it found it: nothing to initialise, eager or captured.
            a.reject_count = reject_words(h);
            hipError_t rerr = hipSuccess;
            if (!launch_pcg_resident_sym_verify<T>(h->dev, a, stream, &rerr)) return GBDPCG_ERR_UNSUPPORTED;
            HIP_TRY(h, rerr);
            a.verdict_out = nullptr;
            a.symmetric = false;
            a.sel_stride = 1;
            a.sel = h->sym_flags;
            a.want = 0;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
            a.reject_count = nullptr;
        } else if (has_sym && h->symmetric == 2) {
            // AUTO: test L_{k+1} == R_k^T on the device (S, then Pinv and-ed in), then launch BOTH kernels:
            // the symmetric one takes the problems that passed, the general one the rest.  No host
            // round trip, so the whole thing stays asynchronous and graph-capturable.
            // one verdict byte per check workgroup when the pair kernel fits the shape (nothing to initialise),
            // else one flag per problem
            const uint32_t vpp = check_pair_chunks<T>(n, N);
            const bool aligned16 = !((reinterpret_cast<uintptr_t>(d_S) | reinterpret_cast<uintptr_t>(d_Pinv)) % 16);
            const size_t need_flags = (size_t)vbatch * (vpp && aligned16 ? vpp : 1);
            const gbdpcg_status st = hold(need_flags <= h->sym_cap, stream, [&] { return ensure_sym_flags(h, need_flags); });
            if (st != GBDPCG_OK) return st;
            hipError_t cerr = hipSuccess;
            uint32_t stride = 1;
            if (vpp && launch_check_symmetric_pair<T>(n, N, vbatch, d_S, d_Pinv, h->sym_flags, stream, &cerr, &stride)) {
                HIP_TRY(h, cerr);
            } else {
                stride = 1;
                HIP_TRY(h, launch_check_symmetric<T>(h->dev, n, N, vbatch, d_S, h->sym_flags, false, stream));
                HIP_TRY(h, launch_check_symmetric<T>(h->dev, n, N, vbatch, d_Pinv, h->sym_flags, true, stream));
            }
            a.sel_stride = stride;
            a.sel = h->sym_flags;
            a.symmetric = true;
            a.want = 1;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
            a.symmetric = false;
            a.want = 0;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
        } else {
            a.symmetric = has_sym && h->symmetric == 1;
            HIP_TRY(h, launch_pcg_fused<T>(h->dev, a, stream, shared));
        }
    } else {
        const size_t need = split_workspace_bytes<T>(n, N, batch);
        const gbdpcg_status st = hold(need <= h->ws_bytes, stream, [&] { return ensure_ws(h, need); });
        if (st != GBDPCG_OK) return st;
        const volatile uint32_t *poll = nullptr;
        if (o.blocking && h->h_done_dev) {  // the caller synchronises before returning: nobody else bumps the counter
            h->h_done[0] = 0;  // problems that converged
            h->h_done[1] = 0;  // iterations the device has started
            a.host_done = h->h_done_dev;
            poll = h->h_done;
        }
        HIP_TRY(h, launch_pcg_split<T>(h->dev, a, h->ws, stream, poll));
    }
    return GBDPCG_OK;
}
template gbdpcg_status solve<float>(gbdpcg_handle_t, const PcgArgs<float> &, hipStream_t, const SolveOpts &);
template gbdpcg_status solve<double>(gbdpcg_handle_t, const PcgArgs<double> &, hipStream_t, const SolveOpts &);

// Phi^-1 from S, then the solve, on one stream.  When the stair kernel can report, per problem, that S was exactly
// symmetric (then so is the Pinv it wrote), the solve takes those verdicts instead of launching its own test.
template <typename T>
gbdpcg_status form_pinv_solve(gbdpcg_handle_t h, const PcgArgs<T> &a, T *d_Pinv, gbdpcg_pinv_kind kind, hipStream_t stream)
{
    if (!h || !a.S || !d_Pinv || !a.gamma || !a.lambda || !a.iters || !shape_ok(a.n, a.N, a.batch) || (int)kind < 0 || (int)kind > 2)
        return GBDPCG_ERR_INVALID;
    if (!mappable<T>(a.n)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    SolveOpts o;
    if (h->symmetric == 2 && pick_path<T>(h, a.n, a.N, a.batch) == GBDPCG_PATH_FUSED && fused_has_symmetric<T>(h->dev, a.n, a.N, a.batch))
        o.verdict_stride = pinv_verdict_chunks<T>(a.n, a.N, (int)kind);
    if (o.verdict_stride) {
        const size_t need = verdict_bytes<T>(a.n, a.N, a.batch);
        const gbdpcg_status st = hold(need <= h->sym_cap, stream, [&] { return ensure_sym_flags(h, need); });
        if (st != GBDPCG_OK) return st;
    }
    HIP_TRY(h, launch_form_pinv<T>(h->dev, a.n, a.N, a.batch, a.S, d_Pinv, (int)kind, stream, o.verdict_stride ? h->sym_flags : nullptr));
    return solve<T>(h, a, stream, o);
}
template gbdpcg_status form_pinv_solve<float>(gbdpcg_handle_t, const PcgArgs<float> &, float *, gbdpcg_pinv_kind, hipStream_t);
template gbdpcg_status form_pinv_solve<double>(gbdpcg_handle_t, const PcgArgs<double> &, double *, gbdpcg_pinv_kind, hipStream_t);

// The handle's workspaces for a graph of this solve (the same choices as solve<T> makes, in its order).
template <typename T> gbdpcg_status graph_reserve(gbdpcg_handle_t h, const PcgArgs<T> &a, bool shared)
{
    const uint32_t n = a.n, N = a.N, batch = a.batch;
    void *pws = nullptr;
    if (shared) {   // the fused family whatever the handle's path: verdict bytes are all it may need
        if (mappable<T>(n) && !fused_fits<T>(h->dev, n, N)) return GBDPCG_ERR_UNSUPPORTED;
        return h->symmetric == 2 ? ensure_sym_flags(h, verdict_bytes<T>(n, N, batch)) : GBDPCG_OK;
    }
    if (const uint32_t per = persist_slices<T>(h, n, N, batch, a.max_iter)) {   // the hand-off words of the slices (solve<T>)
        gbdpcg_status st = get_pws(h, sizeof(T), n, N, per, persist_total_bytes<T>(n, N, per), true, &pws);
        if (st == GBDPCG_OK && batch % per) st = get_pws(h, sizeof(T), n, N, batch % per, persist_total_bytes<T>(n, N, batch % per), true, &pws);
        return st;
    }
    const gbdpcg_path path = pick_path<T>(h, n, N, batch);
    if (path == GBDPCG_PATH_PERSISTENT || path == GBDPCG_PATH_PERSISTENT_1R)
        return get_pws(h, sizeof(T), n, N, batch, persist_total_bytes<T>(n, N, batch), true, &pws);
    if (path == GBDPCG_PATH_SPLIT) return ensure_ws(h, split_workspace_bytes<T>(n, N, batch));
    return h->symmetric == 2 ? ensure_sym_flags(h, verdict_bytes<T>(n, N, batch)) : GBDPCG_OK;
}
template gbdpcg_status graph_reserve<float>(gbdpcg_handle_t, const PcgArgs<float> &, bool);
template gbdpcg_status graph_reserve<double>(gbdpcg_handle_t, const PcgArgs<double> &, bool);

namespace {

template <typename T>
gbdpcg_status spmv_impl(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const T *d_M, const T *d_x, T *d_y, hipStream_t stream)
{
    if (!h || !d_M || !d_x || !d_y || !shape_ok(n, N, batch)) return GBDPCG_ERR_INVALID;
    if (!mappable<T>(n)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    SpmvArgs<T> a{d_M, d_x, d_y, n, N, batch};
    a.symmetric = h->symmetric == 1;  // a check would cost as much as the product itself
    HIP_TRY(h, launch_spmv<T>(h->dev, a, stream));
    return GBDPCG_OK;
}

template <typename T>
gbdpcg_status check_symmetric_impl(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const T *d_M, uint8_t *d_flags,
                                   hipStream_t stream)
{
    if (!h || !d_M || !d_flags || !shape_ok(n, N, batch)) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    hipError_t cerr = hipSuccess;
    if (launch_check_symmetric_pair<T>(n, N, batch, d_M, nullptr, d_flags, stream, &cerr)) {
        HIP_TRY(h, cerr);
        return GBDPCG_OK;
    }
    HIP_TRY(h, launch_check_symmetric<T>(h->dev, n, N, batch, d_M, d_flags, false, stream));
    return GBDPCG_OK;
}

template <typename T>
gbdpcg_status form_pinv_impl(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const T *d_S, T *d_Pinv, gbdpcg_pinv_kind kind,
                             hipStream_t stream)
{
    if (!h || !d_S || !d_Pinv || !shape_ok(n, N, batch) || (int)kind < 0 || (int)kind > 2) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_form_pinv<T>(h->dev, n, N, batch, d_S, d_Pinv, (int)kind, stream));
    return GBDPCG_OK;
}

// `a` on the default stream (the reference launches there, interface.cuh:132), one problem, and its two status words on the host.
template <typename T> gbdpcg_status solve_blocking_impl(gbdpcg_handle_t h, PcgArgs<T> a, uint32_t *h_iters, uint8_t *h_exit)
{
    if (!h) return GBDPCG_ERR_INVALID;
    hipStream_t s = nullptr;
    // status words: written by the kernels straight into coherent pinned host memory when it is mapped
    // (saves the two copy-backs of interface.cuh:136,141), else into device words that are copied back
    const bool direct = h->h_iters_dev != nullptr;
    a.iters = direct ? h->h_iters_dev : h->d_iters;
    a.max_iter_exit = direct ? h->h_exit_dev : h->d_exit;
    SolveOpts o;
    o.blocking = true;
    gbdpcg_status st = solve<T>(h, a, s, o);
    if (st != GBDPCG_OK) return st;
    if (!direct) {
        HIP_TRY(h, hipMemcpyAsync(h->h_iters, h->d_iters, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(h->h_exit, h->d_exit, sizeof(uint8_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));  // interface.cuh:136 synchronises through its blocking copy
    if (h_iters) *h_iters = *h->h_iters;
    if (h_exit) *h_exit = *h->h_exit;
    return GBDPCG_OK;
}

template <typename T>
gbdpcg_status solve_host_impl(gbdpcg_handle_t h, uint32_t n, uint32_t N, const T *h_S, const T *h_Pinv, const T *h_gamma, T *h_lambda,
                              T tol, uint32_t max_iter, uint32_t *h_iters, uint8_t *h_exit)
{
    if (!h || !h_S || !h_gamma || !h_lambda || !shape_ok(n, N, 1)) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    const size_t mbytes = (size_t)3 * n * n * N * sizeof(T), vbytes = (size_t)n * N * sizeof(T);
    // one allocation: S | Pinv | gamma | lambda (256-byte aligned pieces)
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t total = 2 * up(mbytes) + 2 * up(vbytes);
    unsigned char *base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), total);
    if (e != hipSuccess) {
        h->last_err = e;
        return GBDPCG_ERR_ALLOC;
    }
    T *d_S = reinterpret_cast<T *>(base);
    T *d_P = reinterpret_cast<T *>(base + up(mbytes));
    T *d_g = reinterpret_cast<T *>(base + 2 * up(mbytes));
    T *d_l = reinterpret_cast<T *>(base + 2 * up(mbytes) + up(vbytes));
    gbdpcg_status st = GBDPCG_OK;
    auto chk = [&](hipError_t err) {
        if (err != hipSuccess && st == GBDPCG_OK) st = fail(h, err);
    };
    chk(hipMemcpy(d_S, h_S, mbytes, hipMemcpyHostToDevice));
    if (h_Pinv) chk(hipMemcpy(d_P, h_Pinv, mbytes, hipMemcpyHostToDevice));
    chk(hipMemcpy(d_g, h_gamma, vbytes, hipMemcpyHostToDevice));
    chk(hipMemcpy(d_l, h_lambda, vbytes, hipMemcpyHostToDevice));
    if (st == GBDPCG_OK)
        st = solve_blocking_impl<T>(h, pcg_args<T>(n, N, 1, d_S, h_Pinv ? d_P : nullptr, d_g, d_l, nullptr, nullptr, tol, max_iter, nullptr, nullptr),
                                    h_iters, h_exit);
    if (st == GBDPCG_OK) chk(hipMemcpy(h_lambda, d_l, vbytes, hipMemcpyDeviceToHost));
    (void)hipFree(base);
    return st;
}

}  // namespace
}  // namespace gbdpcg

using namespace gbdpcg;

extern "C" {

// One precision of the entry points of this unit.  An eager call and its graph_create twin build the solve's description once and
// define one body; the eager one runs it on the caller's stream, the other hands it to graph_create.
#define GBDPCG_SOLVE_ENTRIES(SUF, TYPE)                                                                                             \
    gbdpcg_status gbdpcg_check_symmetric_##SUF(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const TYPE *d_M,           \
                                               uint8_t *d_flags, void *stream)                                                      \
    {                                                                                                                               \
        return check_symmetric_impl<TYPE>(h, n, N, batch, d_M, d_flags, (hipStream_t)stream);                                       \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_spmv_##SUF(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const TYPE *d_M, const TYPE *d_x,     \
                                    TYPE *d_y, void *stream)                                                                        \
    {                                                                                                                               \
        return spmv_impl<TYPE>(h, n, N, batch, d_M, d_x, d_y, (hipStream_t)stream);                                                 \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_form_pinv_##SUF(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const TYPE *d_S, TYPE *d_Pinv,   \
                                         gbdpcg_pinv_kind kind, void *stream)                                                       \
    {                                                                                                                               \
        return form_pinv_impl<TYPE>(h, n, N, batch, d_S, d_Pinv, kind, (hipStream_t)stream);                                        \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_solve_blocking_##SUF(gbdpcg_handle_t h, uint32_t n, uint32_t N, const TYPE *d_S, const TYPE *d_Pinv,        \
                                              const TYPE *d_gamma, TYPE *d_lambda, TYPE *d_r, TYPE *d_p, TYPE tol,                  \
                                              uint32_t max_iter, uint32_t *h_iters, uint8_t *h_max_iter_exit)                       \
    {                                                                                                                               \
        return solve_blocking_impl<TYPE>(h, pcg_args<TYPE>(n, N, 1, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, tol, max_iter,        \
                                                            nullptr, nullptr), h_iters, h_max_iter_exit);                           \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_solve_host_##SUF(gbdpcg_handle_t h, uint32_t n, uint32_t N, const TYPE *h_S, const TYPE *h_Pinv,            \
                                          const TYPE *h_gamma, TYPE *h_lambda, TYPE tol, uint32_t max_iter, uint32_t *h_iters,      \
                                          uint8_t *h_max_iter_exit)                                                                 \
    {                                                                                                                               \
        return solve_host_impl<TYPE>(h, n, N, h_S, h_Pinv, h_gamma, h_lambda, tol, max_iter, h_iters, h_max_iter_exit);             \
    }                                                                                                                               \
    GBDPCG_SOLVE_PAIR(solve, SUF, TYPE, false)                                                                                      \
    GBDPCG_SOLVE_PAIR(solve_shared, SUF, TYPE, true)                                                                                \
    GBDPCG_FORM_PINV_SOLVE_PAIR(SUF, TYPE)

// (shared: one S, Phi^-1 for `batch` right-hand sides -- the single matrices are one problem's worth)
#define SOLVE_PARAMS(TYPE, PINV)                                                                                                    \
    gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const TYPE *d_S, PINV, const TYPE *d_gamma, TYPE *d_lambda,           \
        TYPE *d_r, TYPE *d_p, TYPE tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit
#define GBDPCG_SOLVE_PAIR(NAME, SUF, TYPE, SHARED)                                                                                  \
    gbdpcg_status gbdpcg_##NAME##_##SUF(SOLVE_PARAMS(TYPE, const TYPE *d_Pinv), void *stream)                                       \
    {                                                                                                                               \
        SolveOpts o;                                                                                                                \
        o.shared = SHARED;                                                                                                          \
        return solve<TYPE>(h, PCG_ARGS(TYPE, n), (hipStream_t)stream, o);                                                           \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_graph_create_##NAME##_##SUF(SOLVE_PARAMS(TYPE, const TYPE *d_Pinv), gbdpcg_graph_t *out)                   \
    {                                                                                                                               \
        SolveOpts o;                                                                                                                \
        o.shared = SHARED;                                                                                                          \
        const PcgArgs<TYPE> a = PCG_ARGS(TYPE, n);                                                                                  \
        return graph_create<TYPE>(h, a, SHARED, out, [&](hipStream_t s) { return solve<TYPE>(h, a, s, o); });                       \
    }
#define GBDPCG_FORM_PINV_SOLVE_PAIR(SUF, TYPE)                                                                                      \
    gbdpcg_status gbdpcg_form_pinv_solve_##SUF(SOLVE_PARAMS(TYPE, TYPE *d_Pinv COMMA gbdpcg_pinv_kind kind), void *stream)          \
    {                                                                                                                               \
        return form_pinv_solve<TYPE>(h, PCG_ARGS(TYPE, n), d_Pinv, kind, (hipStream_t)stream);                                      \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_graph_create_form_pinv_solve_##SUF(SOLVE_PARAMS(TYPE, TYPE *d_Pinv COMMA gbdpcg_pinv_kind kind),           \
                                                            gbdpcg_graph_t *out)                                                    \
    {                                                                                                                               \
        if (!d_Pinv || (int)kind < 0 || (int)kind > 2) return GBDPCG_ERR_INVALID;                                                   \
        const PcgArgs<TYPE> a = PCG_ARGS(TYPE, n);                                                                                  \
        return graph_create<TYPE>(h, a, false, out, [&](hipStream_t s) { return form_pinv_solve<TYPE>(h, a, d_Pinv, kind, s); });   \
    }
#define COMMA ,
GBDPCG_SOLVE_ENTRIES(f32, float)
GBDPCG_SOLVE_ENTRIES(f64, double)
#undef COMMA
#undef GBDPCG_FORM_PINV_SOLVE_PAIR
#undef GBDPCG_SOLVE_PAIR
#undef SOLVE_PARAMS
#undef GBDPCG_SOLVE_ENTRIES

}  // extern "C"
