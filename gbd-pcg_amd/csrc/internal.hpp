// internal.hpp -- launcher declarations shared by the translation units of libgbdpcg.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace gbdpcg {

// Device limits the launchers size against (filled once per handle).
struct DeviceInfo {
    int device = 0;
    int num_cus = 256;
    size_t lds_per_cu = 160 * 1024;   // MI355X: 160 KiB per CU, one workgroup may take all of it
    size_t lds_per_wg_max = 160 * 1024;
};

// What a kernel whose workgroups rendezvous in-kernel (pcg_cluster.hip, pcg_persist.hip) would leave in d_iters for a
// problem whose workgroups could not meet (with d_max_iter_exit = 2; lambda, r, p untouched).  Callers never see it: the
// workgroup of the problem that finishes last solves it alone inside the same launch (pcg_stream.hpp, stream_rescue);
// only variants/libgbdpcg_hooks.so can switch that off (GBDPCG_RESCUE_OFF) to show the mark to a test.
constexpr uint32_t kItersGaveUp = 0xffffffffu;

// Does this launch own problem `prob`?  (see PcgArgs::sel)
// SHARED (here and below): the instantiations of gbdpcg_solve_shared_* -- a.S and a.Pinv are ONE problem's matrices, used by every
// problem of the batch (the vectors stay per problem), and a.sel, where set, holds ONE verdict that every problem follows.  A
// compile-time switch throughout: the per-problem instantiations are what they were before the shared form existed.
template <bool SHARED = false, typename A> __device__ __forceinline__ bool pcg_takes(const A &a, uint32_t prob)
{
    if (!a.sel) return true;
    if constexpr (SHARED) prob = 0;
    bool sym = true;
    for (uint32_t c = 0; c < a.sel_stride; ++c) sym &= a.sel[(size_t)prob * a.sel_stride + c] == 1;
    return sym == (a.want == 1);
}

// The same verdicts for up to 64 problems at once: bit j of the result = this launch owns problem first + j * step
// (j < count <= 64).  Every lane of the calling wave fetches the verdict bytes of one problem, so a workgroup that walks
// over many problems pays one memory round trip for all of them instead of one per problem; every wave of a workgroup
// that calls it gets the same mask.  All 64 lanes must be active.
template <bool SHARED = false, typename A>
__device__ __forceinline__ unsigned long long pcg_takes_mask(const A &a, uint32_t first, uint32_t step, uint32_t count, uint32_t lane)
{
    if (!a.sel) return count >= 64 ? ~0ull : ((1ull << count) - 1ull);
    bool mine = false;
    if (lane < count) {
        const size_t prob = SHARED ? (size_t)0 : (size_t)first + (size_t)lane * step;
        bool sym = true;
        for (uint32_t c = 0; c < a.sel_stride; ++c) sym &= a.sel[prob * a.sel_stride + c] == 1;
        mine = sym == (a.want == 1);
    }
    return __ballot(mine);
}

// The general launch behind a verifying launch (PcgArgs::reject_count): true when the verifying launch rejected nothing, so that
// this launch owns nothing and the workgroup may return at once.  Called first thing by EVERY thread of the launch; the word is
// written by the launch before this one alone, so every workgroup reads the same value and all of them take the same branch --
// which is what makes leaving safe for kernels whose workgroups wait for each other (pcg_cluster.hip).
template <typename A> __device__ __forceinline__ bool pcg_reject_none(const A &a)
{
    return a.reject_count && __hip_atomic_load(a.reject_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
}
// ... and at the end of a launch that did not return there: the workgroup that leaves last puts the count (and the word that
// tells it that it is the last) back to 0 for the next verifying launch.  Every workgroup has read the count by then.
template <typename A> __device__ __forceinline__ void pcg_reject_leave(const A &a)
{
    if (!a.reject_count) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t before = __hip_atomic_fetch_add(a.reject_count + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == gridDim.x - 1u) {
            __hip_atomic_store(a.reject_count + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.reject_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <typename T> struct SpmvArgs {
    const T *M;
    const T *x;
    T *y;
    uint32_t n, N, batch;
    bool symmetric = false;
};

template <typename T> struct PcgArgs {
    const T *S;
    const T *Pinv;  // nullptr => identity
    const T *gamma;
    T *lambda;
    T *r;  // nullable
    T *p;  // nullable
    T tol;
    uint32_t max_iter;
    uint32_t n, N, batch;
    uint32_t *iters;         // [batch]
    uint8_t *max_iter_exit;  // [batch], nullable
    bool symmetric = false;  // stream [D|R] only: caller's assertion, or per problem where sel says so
    // Per-problem kernel selection (symmetric AUTO mode): a launch handles problem b only when
    // (sel[b] == 1) == (want == 1): flag 1 -> the symmetric launch, anything else -> the general one, so
    // every problem is taken by exactly one of the two launches whatever the flag holds.  sel == nullptr:
    // every problem.
    const uint8_t *sel = nullptr;
    uint8_t want = 0;
    uint32_t sel_stride = 1;  // verdict bytes per problem (one per workgroup of the check kernel); the flag is their AND
    // The verifying resident kernel (launch_pcg_resident_sym_verify) writes its symmetry verdict here, one byte per problem
    // (1 = symmetric, solved; 0 = left untouched for the general launch).  Read by no other kernel.
    uint8_t *verdict_out = nullptr;
    // Problems the verifying launch rejected, counted on the device: [0] the count, [1] workgroups of the general launch that
    // have left (gbdpcg_context::sym_flags holds both, behind the verdict bytes).  The verifying launch adds to [0]; the general
    // launch that follows it on the stream gets the same pointer, reads [0] before anything else and returns when it is 0
    // (pcg_reject_none); when it is not, the workgroup of that launch that leaves last puts both words back to 0
    // (pcg_reject_leave).  nullptr: a launch that does not follow a verifying launch -- nothing is read or written.
    uint32_t *reject_count = nullptr;
    // Split path, blocking entry points only: a counter in host-visible memory that a problem bumps when
    // it converges, so that the host can stop enqueueing iteration launches (nullptr: not used).
    uint32_t *host_done = nullptr;
    // Cluster path (pcg_cluster.hip): the handle's hand-off slots (cluster_workspace_bytes; zero-filled once when the
    // handle is made, never cleared afterwards: a tag carries the launch number); nullptr: the path is not offered.
    void *cluster_ws = nullptr;
    // In-kernel rescue (pcg_stream.hpp): device memory for the vectors of the workgroup that solves a problem alone when
    // the workgroups of its cluster / persistent launch could not meet -- rescue_vec_elems(n, N) elements per cluster
    // (pcg_cluster.hip) or per problem (pcg_persist.hip).  rescue_off: hooks build only (the mark stays visible).
    void *rescue_vec = nullptr;
    bool rescue_off = false;
};

// Widest per-lane vector (in elements) usable for this block size and these base pointers:
// V in {1,2,4}, n % V == 0, V*sizeof(T) <= 16, every pointer V*sizeof(T)-aligned, n/V <= 64.
// Returns 0 when no mapping exists (n/V > 64 for every V).
template <typename T> int choose_vec(uint32_t n, const void *const *ptrs, int nptrs);

// Block sizes with a compile-time specialised kernel (everything else runs the runtime-n pipeline).
// BASELINE shapes (14, 36), the reference's example (2) and common MPC state sizes.
#define GBDPCG_SPECIALIZED_N(X) X(2) X(4) X(6) X(8) X(10) X(12) X(13) X(14) X(16) X(18) X(20) X(24) X(36)

// Widest per-lane vector a specialised kernel of block size NCT is built with (the V choose_vec
// returns for aligned pointers); other V values of that n fall back to the runtime-n kernel.
template <typename T, int NCT> constexpr int best_v()
{
    for (int V : {4, 2, 1})
        if ((size_t)V * sizeof(T) <= 16 && NCT % V == 0 && NCT / V <= 64) return V;
    return 1;
}

// ---- spmv.hip
template <typename T> hipError_t launch_spmv(const DeviceInfo &dev, const SpmvArgs<T> &a, hipStream_t s);

// ---- pcg_fused.hip : one workgroup per problem
template <typename T> size_t fused_lds_bytes(uint32_t n, uint32_t N, uint32_t waves);
template <typename T> bool fused_fits(const DeviceInfo &dev, uint32_t n, uint32_t N);
// (shared, here and in the launchers below: the SHARED instantiations -- one pair of matrices for the whole batch)
template <typename T> hipError_t launch_pcg_fused(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, bool shared = false);

// ---- pcg_resident.hip : both matrices register-resident, one 8-wave workgroup per problem.
// Returns false when the shape is not eligible (then nothing was launched).
template <typename T> bool resident_shape(uint32_t n, uint32_t N);  // shape handled by the resident kernel
template <typename T> void resident_prepare(uint32_t n, uint32_t N);  // runtime queries of that kernel, outside any capture
template <typename T>
bool launch_pcg_resident(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool shared = false);
// Symmetric matrices resident on one CU (pcg_resident_sym.hip): n = 14, fp32, N <= 128, a.symmetric set.
template <typename T> bool resident_sym_shape(uint32_t n, uint32_t N);
template <typename T>
bool launch_pcg_resident_sym(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool shared = false);
// Its verifying form: every problem, L_{k+1} == R_k^T of S and Pinv tested inside the solve, verdicts into a.verdict_out
// (stride 1); a problem that fails is left untouched.  resident_sym_verifies: would that form take this solve (n = 14, fp32,
// N <= 128, S and Pinv 16-byte aligned)?
template <typename T> bool resident_sym_verifies(const DeviceInfo &dev, uint32_t n, uint32_t N, const T *S, const T *Pinv);
template <typename T>
bool launch_pcg_resident_sym_verify(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err);

// ---- pcg_cluster.hip : general-storage matrices register-resident, a problem over a cluster of up to eight (fp64: four) workgroups
// Workgroups per problem the cluster path would use; 0 = shape not handled (block size not built, a horizon one workgroup of
// pcg_resident.hip holds, or more members than a cluster has: at n = 14 in fp32 the path takes 72 < N <= 576).
template <typename T> uint32_t cluster_members(uint32_t n, uint32_t N);
size_t cluster_workspace_bytes(const DeviceInfo &dev);
size_t cluster_rescue_bytes(const DeviceInfo &dev);   // PcgArgs::rescue_vec of a cluster launch
// Returns false when the launch is not eligible (then nothing was launched).
template <typename T>
bool launch_pcg_cluster(const DeviceInfo &dev, const PcgArgs<T> &a, hipStream_t s, hipError_t *err, bool shared = false);

// ---- pcg_split.hip : many workgroups per problem, two launches per iteration
template <typename T> size_t split_workspace_bytes(uint32_t n, uint32_t N, uint32_t batch);
template <typename T>
hipError_t launch_pcg_split(const DeviceInfo &dev, const PcgArgs<T> &a, void *workspace, hipStream_t s,
                            const volatile uint32_t *host_done_poll = nullptr);

// ---- pcg_persist.hip : one large problem over many CUs in ONE persistent launch (matrices register-resident,
// in-kernel all-gather of {partial inner product, boundary knots} twice per iteration)
// Knots per workgroup the launch would use; 0 = the shape cannot run persistently on this device.
template <typename T>
uint32_t persist_knots_per_wg(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch, bool one_reduction = false);
template <typename T> size_t persist_workspace_bytes(uint32_t n, uint32_t N, uint32_t batch);
template <typename T> size_t persist_rescue_bytes(uint32_t n, uint32_t N, uint32_t batch);   // PcgArgs::rescue_vec of a persistent launch
// workspace: persist_workspace_bytes, ZERO-FILLED once when allocated (epoch bases live there), never cleared again
template <typename T>
hipError_t launch_pcg_persist(const DeviceInfo &dev, const PcgArgs<T> &a, void *workspace, hipStream_t s,
                              bool one_reduction = false);   // one_reduction: the Chronopoulos-Gear form (opt-in path 4)
// (the kernels compile in three units by block size -- pcg_persist.hip, pcg_persist_b.hip, pcg_persist_c.hip -- behind
// launch_pcg_persist_group<T, G> of pcg_persist_kernels.hpp)

// ---- symcheck.hip : flags[b] = 1 iff L_{k+1} == R_k^T bit for bit for every k of problem b
// and_into: flags[b] &= result instead of flags[b] = result (second matrix of a pair).
template <typename T>
hipError_t launch_check_symmetric(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch, const T *M,
                                  uint8_t *flags, bool and_into, hipStream_t s);
// Device fills as kernels (capturable, arguments travel with the graph node; see symcheck.hip).
hipError_t launch_fill_bytes(uint8_t *p, uint8_t v, size_t count, hipStream_t s);
hipError_t launch_fill_words(uint32_t *p, uint32_t v, size_t count, hipStream_t s);
// S and Pinv in one launch (flags = 1 where both are symmetric); false if the shape does not fit.
template <typename T>
bool launch_check_symmetric_pair(uint32_t n, uint32_t N, uint32_t batch, const T *A, const T *B, uint8_t *flags,
                                 hipStream_t s, hipError_t *err, uint32_t *verdicts_per_problem = nullptr);
// Verdict bytes per problem the pair kernel writes when asked for per-workgroup verdicts (0: shape not supported).
template <typename T> uint32_t check_pair_chunks(uint32_t n, uint32_t N);
// Does launch_pcg_fused have a symmetric-streaming kernel for this shape (and would it be used)?
template <typename T> bool fused_has_symmetric(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch);

// ---- pinv.hip
// verdicts (optional, only when pinv_verdict_chunks() != 0): pinv_verdict_chunks bytes per problem, 1 = every pair of
// that chunk was exactly symmetric in S and therefore is in Pinv (pcg_takes ANDs them).
template <typename T>
hipError_t launch_form_pinv(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch, const T *S,
                            T *Pinv, int kind, hipStream_t s, uint8_t *verdicts = nullptr, bool s_symmetric = false);
// (s_symmetric: the caller KNOWS L_{k+1} == R_k^T in S bit for bit -- the one-launch stair kernel then never reads L)
template <typename T> uint32_t pinv_verdict_chunks(uint32_t n, uint32_t N, int kind);

// ---- schur.hip: KKT blocks -> S, gamma, G^-1.  Layouts in include/gbdpcg.h.
// rho (device, [batch]; gbdpcg_form_schur_reg_*): problem b is formed from G_b + rho_b I -- the REG instantiations of the same
// kernels; nullptr: the kernels without the switch.
template <typename T>
hipError_t launch_form_schur(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *G, const T *C,
                             const T *g, const T *c, T *S, T *gamma, T *Ginv, hipStream_t s, const T *rho = nullptr);
template <typename T> bool schur_shape_ok(const DeviceInfo &dev, uint32_t nx, uint32_t nu);

// ---- schur_ginv.hip : the two steps that apply the stored G^-1.  lambda -> primal step z = -G^-1 (g + C' lambda)
template <typename T>
hipError_t launch_recover_primal(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *Ginv,
                                 const T *C, const T *g, const T *lambda, T *z, hipStream_t s, bool shared = false);
// gamma = -(c + C G^-1 g) alone, from the G^-1 launch_form_schur wrote: G and C unchanged, new g and c (S is not touched)
template <typename T>
hipError_t launch_form_gamma(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *Ginv, const T *C,
                             const T *g, const T *c, T *gamma, hipStream_t s, bool shared = false);
// (shared, the two launchers: Ginv and C are one problem's blocks, used by every problem of the batch)

// ---- schur_residual.hip
// res[2b] = ||G z + g + C' lambda||_inf, res[2b+1] = ||C z - c||_inf of problem b (G: the Hessians, not their inverses)
// rho (gbdpcg_kkt_residual_reg_*, not with shared): the stationarity of G_b + rho_b I
template <typename T>
hipError_t launch_kkt_residual(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *G, const T *C,
                               const T *g, const T *c, const T *z, const T *lambda, T *res, hipStream_t s, bool shared = false,
                               const T *rho = nullptr);
// (shared: G and C are one problem's blocks, used by every problem of the batch)

// ---- admm.hip : the splitting update of box-constrained ADMM on a kept factorisation, one launch, one workgroup per problem.
// Every array has the layout of g ((nx + nu) N - nu elements per problem), rho [batch], res [2 batch]:
//     w <- clip(z + y, lo, hi), y <- (z + y) - w, gt <- fma(-rho_b, w - y, g), res[2b] = ||z - w||_inf, res[2b+1] = rho_b ||w - w_old||_inf
// init: w <- clip(w, lo, hi), gt <- fma(-rho_b, w - y, g); y is not written, z and res are not looked at (may be null).
// kappa (the gbdpcg_admm_soft_* calls; null: the hard box): the layout of lo, the weight of the L1 penalty on leaving the bound --
// the kernel's SOFT instantiation, whose lines are in the head of admm.hip; kappa = +Inf everywhere gives the hard bits.
template <typename T>
hipError_t launch_admm_update(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *g, const T *lo, const T *hi, const T *rho,
                              const T *z, T *w, T *y, T *gt, T *res, hipStream_t s, bool init, const T *kappa = nullptr);

// (still admm.hip) The adjoint of that update, the backward pass of the hard box QP, same launch shape.  yf is the forward y, read
// only: the mask m = (yf != 0) stands where lo, hi stand in the update, which then projects onto {0} where m and onto the line elsewhere:
//     w <- m ? clip(az + y, 0, 0) : az + y, y <- (az + y) - w, gt <- fma(-rho_b, w - y, gz), res as in the update
// the bits of launch_admm_update on the explicit box lo = hi = +0 where m, -Inf / +Inf elsewhere.  init: as there (az, res may be null).
template <typename T>
hipError_t launch_admm_adjoint_update(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *gz, const T *yf, const T *rho,
                                      const T *az, T *w, T *y, T *gt, T *res, hipStream_t s, bool init);

// ---- admm_rebalance.hip : adaptive rho by residual balancing in powers of two, one launch, one workgroup per problem.  From
// r = res[2b], s = res[2b+1] and rho_b: rho_b <- rho_b 2^e with e in {+shift, -shift, 0} (the rule is in the head of the file and in
// include/gbdpcg.h), y <- y 2^-e over `len` elements per problem, expo[b] = e.  box: len is that of g and gt <- fma(-rho_b, w - y, g)
// is rebuilt in the same launch (w is read); otherwise g, w, gt are not looked at (may be null).  res is read only.
template <typename T>
hipError_t launch_admm_rebalance(uint64_t len, uint32_t batch, const T *g, const T *res, T *rho, const T *w, T *y, T *gt, T ratio,
                                 uint32_t shift, T rho_min, T rho_max, int32_t *expo, hipStream_t s, bool box);

// ---- admm_rows.hip : ADMM with stage-wise rows on E z, linear (lo <= E z <= hi) or in second-order cones; the layouts are in
// include/gbdpcg.h, the lines that define every bit in the head of the file.  Two kernels:
//     form:   Gt = G + rho_b E'E per diagonal block, one lane per entry (Gt may be G)
//     update: w <- projection of E z + y, y, gt, res; one workgroup per problem, the horizon in chunks of admm_rows_knot_chunk knots
// init: the update without z (w is projected itself), y is not written, z and res are not looked at (may be null).
// shared: E is one problem's blocks, used by every problem of the batch.
// cones (the gbdpcg_admm_soc_* calls; null: every row is linear): the rows behind the first lx / lu of a block are cones of
// dimension qx / qu, lo holds their offsets.  With cones the launch is the kernel's CONES instantiation, whatever the classes say.
// kappa (the gbdpcg_admm_lin_soft_* calls; null: hard rows): the layout of lo, the L1 weights -- the kernel's SOFT instantiation.
// Never with cones (refused): cone rows stay hard.
// adjoint (the gbdpcg_admm_lin_adjoint_* calls): lo is yf, the forward y, hi is not looked at (may be null), and the projection is
// yf != 0 ? clip(s, +0, +0) : s -- the bits of the hard linear launch on the explicit rows lo = hi = +0 where yf != 0, -Inf / +Inf
// elsewhere, with one array read less per row.  Never with cones, kappa or shared (refused).
struct RowClasses {
    uint32_t lx, qx, lu, qu;
};
template <typename T>
hipError_t launch_admm_lin_form(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *G, const T *E,
                                const T *rho, T *Gt, hipStream_t s);
template <typename T>
hipError_t launch_admm_rows_update(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *g,
                                   const T *E, const T *lo, const T *hi, const T *rho, const T *z, T *w, T *y, T *gt, T *res,
                                   hipStream_t s, bool init, bool shared = false, const RowClasses *cones = nullptr,
                                   const T *kappa = nullptr, bool adjoint = false);
// (mx, mu <= 64 and one knot's E blocks, z, t, d within the kernel's LDS)
template <typename T> bool admm_rows_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu);
uint32_t admm_rows_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu);
// (lx <= mx, lu <= mu; where a block has cone rows its q is not 0 and divides their number; q is ignored where it has none)
bool admm_rows_classes_ok(uint32_t mx, uint32_t mu, const RowClasses &c);

// ---- admm_infeas.hip : the primal infeasibility certificate of the hard ADMM paths from two iterates (lam0, y0), (lam1, y1) of the
// splitting, one launch, one workgroup per problem; the lines that define every bit are in the head of the file.  cert [3 batch]:
// the scale n, the residual r of C'dl + rho E'dy, the support value sigma; flag [batch] (may be null: not written):
// n > 0 && r <= eps n && sigma < -(eps n).  box: no E (not looked at), mx, mu are not looked at, lo, hi, y0, y1 have the layout of g.
// shared: C and E are one problem's blocks.  C may be null when N == 1.
// (a knot's [A | B], E blocks and vectors within the kernel's LDS; hipErrorInvalidValue otherwise)
template <typename T>
hipError_t launch_admm_infeas(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *C, const T *c,
                              const T *E, const T *lo, const T *hi, const T *rho, const T *lam0, const T *lam1, const T *y0,
                              const T *y1, T eps, T *cert, uint8_t *flag, hipStream_t s, bool box, bool shared);
template <typename T> bool admm_infeas_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box);
uint32_t admm_infeas_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box);

// ---- admm_optimality.hip : the optimality test of every ADMM family at (z, lambda, w, y), one launch, one workgroup per problem;
// the lines that define every bit are in the head of the file.  opt [6 batch]: r_s, r_e, r_r (stationarity with the row multiplier,
// dynamics, consensus) and their scales n_s, n_e, n_r; done [batch] (may be null: not written): r <= fma(eps_rel, n, eps_abs) for
// all three.  G is the Hessian.  box: no E (not looked at), mx, mu are not looked at, w, y have the layout of g.  shared: G, C and E
// are one problem's blocks.  C may be null when N == 1.
// (a knot's Q, R, [A | B], E blocks and vectors within the kernel's LDS; hipErrorInvalidValue otherwise)
template <typename T>
hipError_t launch_admm_optimality(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *G, const T *C,
                                  const T *g, const T *c, const T *E, const T *rho, const T *z, const T *lambda, const T *w, const T *y,
                                  T eps_abs, T eps_rel, T *opt, uint8_t *done, hipStream_t s, bool box, bool shared);
template <typename T> bool admm_optimality_shape_ok(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box);
uint32_t admm_optimality_knot_chunk(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, bool box);

// ---- kkt_grad.hip : the gradients of a scalar in the packed KKT blocks from the forward pair (z, lambda) and the adjoint pair
// (az, alam), one launch.  gG has the layout of G, gC that of C; either may be null (not written):
//     gQ_k = 1/2 (ax_k x_k' + x_k ax_k'), gR_k likewise with u;  [gA_k | gB_k] = -(alam_{k+1} z_k' + lam_{k+1} az_k')
// shared: gG, gC are ONE problem's worth, the sum over the batch in the order b = 0, 1, ...
template <typename T>
hipError_t launch_kkt_grad(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *z, const T *lam, const T *az, const T *alam,
                           T *gG, T *gC, hipStream_t s, bool shared = false);

// ---- admm_lin_grad.hip : the gradients of a scalar in the rows of the hard linear-row QP from the forward z and y (yf) and the
// adjoint's z and y (az, ya), one launch, one workgroup per problem.  glo, ghi have the layout of the rows (the bits of
// launch_admm_grad_bounds over that layout), gE that of E; each may be null (not written), not all three:
//     gE(r, j) = yf_r != 0 ? rho_b fma(yf_r, az_j, ya_r z_j) : +0
// (mx, mu <= 64 and a knot within the LDS, as admm_rows_shape_ok; hipErrorInvalidValue otherwise)
// kappa (the gbdpcg_admm_lin_soft_grad_* calls; null: the hard rows, E and gkappa not looked at): the kernel's SOFT instantiation --
// with sat = |yf_r| >= kappa_r / rho_b, glo and ghi are +0 on saturated rows, gE keeps the line above with the unmasked yf, and
//     gkappa_r = sat ? (yf_r > 0 ? v : -v) : +0,  v the chain of E(r, .) az in ascending j            (may be null like the others)
template <typename T>
hipError_t launch_admm_lin_grad(uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch, const T *z, const T *az,
                                const T *yf, const T *ya, const T *rho, T *glo, T *ghi, T *gE, hipStream_t s, const T *E = nullptr,
                                const T *kappa = nullptr, T *gkappa = nullptr);

// ---- admm_box_grad.hip : the elementwise launches of the backward passes around the adjoint loops, the launch shape of admm.hip.
//     grad_bounds: glo = yf < 0 ? -(rho_b ya) : +0, ghi = yf > 0 ? -(rho_b ya) : +0, over the layout of g (the hard box)
// The soft box and rows: theta = kappa / rho_b is the one division of the soft update, sat = |yf| >= theta (a NaN yf fails):
//     mask:             ym = sat ? +0 : yf over `len` elements per problem (nz: the box, nw: the rows); ym == yf is refused
//     soft_grad_bounds: glo = (yf < 0 && !sat) ? -(rho_b ya) : +0, ghi likewise with > 0, gkappa = sat ? (yf > 0 ? az : -az) : +0,
//                       over the layout of g; each output may be null (not written), not all three
// rho is the rho of the update that wrote yf.
template <typename T>
hipError_t launch_admm_grad_bounds(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *yf, const T *rho, const T *ya, T *glo,
                                   T *ghi, hipStream_t s);
template <typename T>
hipError_t launch_admm_soft_mask(uint64_t len, uint32_t batch, const T *yf, const T *kappa, const T *rho, T *ym, hipStream_t s);
template <typename T>
hipError_t launch_admm_soft_grad_bounds(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *yf, const T *kappa, const T *rho,
                                        const T *ya, const T *az, T *glo, T *ghi, T *gkappa, hipStream_t s);

// ---- kkt_refine.hip : mixed-precision refinement around an fp32 solve on a kept factorisation; the lines that define every bit
// are in the head of the file.  One workgroup per problem in the first two.
//     defect: rg = fl32(G z + g + C' lambda) 2^e_b, rc = fl32(-(C z - c)) 2^e_b, dlambda = 0 (may be null), expo[b] = e_b,
//             res[2b], res[2b+1] = the norms launch_kkt_residual<double> writes for the same point
//     apply:  z += (double)dz 2^-e_b, lambda += (double)dlambda 2^-e_b
//     demote: dst[i] = fl32(src[i]), i < count
// defect, shared: G and C are one problem's blocks (zero problem stride); rho != nullptr ([batch]): the defect of G_b + rho_b I,
// the diagonal entries as fl(d + rho_b); both as in launch_kkt_residual, and both together are hipErrorInvalidValue as there.
hipError_t launch_kkt_defect_mixed(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *G,
                                   const double *C, const double *g, const double *c, const double *z, const double *lambda, float *rg,
                                   float *rc, float *dlambda, int32_t *expo, double *res, hipStream_t s, bool shared = false,
                                   const double *rho = nullptr);
hipError_t launch_kkt_refine_apply(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *dz, const float *dlambda,
                                   const int32_t *expo, double *z, double *lambda, hipStream_t s);
hipError_t launch_demote(const DeviceInfo &dev, uint64_t count, const double *src, float *dst, hipStream_t s);

}  // namespace gbdpcg
