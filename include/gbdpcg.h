/*
 * gbdpcg.h -- C ABI of libgbdpcg.so: MI355X-native (gfx950) block-tridiagonal PCG.
 *
 * This is the drop-in boundary for the solve path of A2R-Lab/GBD-PCG.  Every entry
 * point cites the reference interface it replaces (paths relative to the reference
 * checkout).  Plain pointers and sizes only; no C++ or torch types cross it.  The
 * C++ surface the reference's callers see (solvePCG<T>, pcg_config<T>, ...) is the
 * header-only wrapper include/gbdpcg.hpp, which forwards here.
 *
 * DATA LAYOUT (include/pcg.cuh:104-110, include/utils.cuh:80)
 *   A block-tridiagonal matrix with N block-rows of n x n blocks is one array of
 *   3*n*n*N elements: for knot k the three column-major blocks [L_k | D_k | R_k]
 *   (block-row k, block-columns k-1, k, k+1); element (r,c) of block b lives at
 *   k*3n^2 + b*n^2 + c*n + r.  L_0 and R_{N-1} are present but never read.
 *   Vectors (gamma, lambda, r, p) have n*N elements.
 *   A batch of `batch` independent problems is the problem-major concatenation of
 *   the single-problem layout (matrix stride 3n^2N, vector stride nN).  The
 *   reference has no batch notion: batch = 1 is its case.
 *
 * ERRORS
 *   Every function returns a gbdpcg_status; nothing here prints or exits (the
 *   reference's gpuErrchk / exit(code) convention, include/gpuassert.cuh:5-14, is
 *   reproduced by the C++ wrapper).  Functions taking a stream are asynchronous and
 *   capturable into a hipGraph: they never allocate, free or synchronise.
 *
 * There is no CPU fallback: without a gfx950 device gbdpcg_create fails with
 * GBDPCG_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef GBDPCG_H
#define GBDPCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gbdpcg_status {
    GBDPCG_OK = 0,
    GBDPCG_ERR_INVALID = 1,       /* bad argument (null pointer, n == 0, N == 0, ...) */
    GBDPCG_ERR_HIP = 2,           /* a HIP runtime call failed; see gbdpcg_last_hip_error */
    GBDPCG_ERR_NO_DEVICE = 3,     /* no usable gfx950 device */
    GBDPCG_ERR_UNSUPPORTED = 4,   /* shape outside what this build supports */
    GBDPCG_ERR_TOO_LARGE = 5,     /* checkPcgOccupancy analogue: does not fit on the device */
    GBDPCG_ERR_ALLOC = 6,         /* workspace allocation failed */
    GBDPCG_ERR_NOT_IMPLEMENTED = 12 /* the reference's exit code for its CSR stub (interface.cuh:18-19) */
} gbdpcg_status;

typedef struct gbdpcg_context *gbdpcg_handle_t;
typedef struct gbdpcg_graph *gbdpcg_graph_t;

/* Which execution strategy a solve uses.  AUTO picks by shape. */
typedef enum gbdpcg_path {
    GBDPCG_PATH_AUTO = 0,
    GBDPCG_PATH_FUSED = 1, /* one workgroup per problem, vectors LDS-resident, one launch per solve */
    GBDPCG_PATH_SPLIT = 2, /* many workgroups per problem, two launches per iteration, vectors in L2/HBM */
    GBDPCG_PATH_PERSISTENT = 3, /* one large problem over many CUs in ONE launch: block-rows register-resident for the
                                  whole solve (the reference's layout, pcg.cuh:104-110), two in-kernel all-gathers of
                                  {partial inner product, boundary knots} per iteration instead of 4 grid.sync().  Wants
                                  every workgroup resident at once (ceil(N/K) * batch <= CU count, K = 2, 3 or 1).  The
                                  reference refuses a launch that cannot be co-resident before it starts
                                  (checkPcgOccupancy, pcg.cuh:23-49); here, if another kernel holds compute units for
                                  about two seconds (up to twice that when a workgroup arrives late, plus the streaming
                                  solve), the workgroups give up after a bounded spin WITHOUT having written
                                  anything, and the one that leaves last solves the problem alone inside the same launch
                                  (streaming kernel: slow, correct).  The caller always gets a solved problem; on a
                                  device shared with long-running kernels GBDPCG_PATH_SPLIT avoids the wait. */
    GBDPCG_PATH_PERSISTENT_1R = 4 /* OPT-IN, never chosen by AUTO: the persistent launch with the single-reduction
                                  (Chronopoulos-Gear style) recurrence -- u = Pinv r, w = S u, gamma = r.u, delta = u.w and
                                  chi = u.s + p.w in ONE all-gather per iteration (the halo knots of u are recomputed, not
                                  exchanged), p.Sp = delta + beta chi + beta^2 (p.Sp)_old, s = S p by recurrence.  Same
                                  iterates and the same exit test as pcg.cuh:154-206 in exact arithmetic, for ANY S and Pinv
                                  the storage holds, symmetric as matrices or not (chi is carried for that: the textbook form
                                  replaces it by an identity of symmetric operators); a different rounding sequence: equal
                                  iteration counts and fp64 lambda within 1e-10 of the oracle on the test shapes, but not
                                  the reference's recurrence. */
} gbdpcg_path;

/* Preconditioners gbdpcg_form_pinv can build from S. */
typedef enum gbdpcg_pinv_kind {
    GBDPCG_PINV_IDENTITY = 0,
    GBDPCG_PINV_BLOCK_JACOBI = 1, /* diag blocks D_k^-1 */
    GBDPCG_PINV_STAIR = 2         /* symmetric stair: D_k^-1, -D_k^-1 O_k D_{k+-1}^-1 */
} gbdpcg_pinv_kind;

/* ---- lifetime ------------------------------------------------------------------------ */

/* One handle per host thread AND per stream of concurrent work: a handle owns device scratch (status
 * words, the split path's workspace, the per-problem symmetry flags) that every solve and every graph
 * created through it uses, so two solves issued through the same handle must not overlap in time
 * (same stream, or otherwise ordered).  `device` is a HIP ordinal.  Replaces the per-call
 * cudaMalloc/cudaFree of interface.cuh:105-108,140-141.
 * A process may hold handles on several devices (one host thread per handle, or one thread looping over
 * them): every entry point makes the handle's device current for the duration of the call and restores the
 * caller's current device before it returns.  Streams and pointers passed in must belong to the handle's device. */
gbdpcg_status gbdpcg_create(gbdpcg_handle_t *out, int device);
gbdpcg_status gbdpcg_destroy(gbdpcg_handle_t h);

const char *gbdpcg_status_string(gbdpcg_status s);
/* hipError_t (as int) of the last failing HIP call on this handle, and its string. */
int gbdpcg_last_hip_error(gbdpcg_handle_t h);
const char *gbdpcg_last_hip_error_string(gbdpcg_handle_t h);

/* Force a path for subsequent solves on this handle (tests / benchmarks). */
gbdpcg_status gbdpcg_set_path(gbdpcg_handle_t h, gbdpcg_path path);
/* Path AUTO would take for this shape (elem_size 4 or 8).  One refinement is decided per solve, where max_iter is known: a
 * batch reported as GBDPCG_PATH_SPLIT that exceeds ONE persistent launch by a few problems (stateSize 14 ... 36) is cut into
 * persistent launches in a row when those cost less than the split path's 2 max_iter + 4 launches. */
gbdpcg_path gbdpcg_choose_path(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N,
                               uint32_t batch);
/* Compute units a GENERAL-storage problem of this shape is spread over inside the fused path (pcg_cluster.hip: both
 * matrices register-resident for the whole solve, 1-8 workgroups per problem (fp64: 1-4) exchanging inner-product partials and
 * boundary knots twice per iteration): built for stateSize 2 ... 16 and 18 in fp32, 2 ... 16 in fp64, horizons up to eight
 * (fp64: four) times what one workgroup holds (stateSize 14, fp32: 72 < knotPoints <= 576).  0 = the shape has no such form: the
 * single-workgroup resident kernel has it (short horizons of stateSize 2 ... 14), or general storage is streamed every
 * iteration (larger blocks, longer horizons). */
uint32_t gbdpcg_cluster_members(uint32_t elem_size, uint32_t n, uint32_t N);
/* The workgroups of one problem wait for each other inside the kernel (bounded spins), so they should get onto the device
 * together: the launch never has more workgroups than compute units and keeps the members of a problem next to each other
 * in dispatch order, which is enough as long as other kernels on the device finish within about a second.  A problem whose
 * workgroups could not meet within the bound is not lost: nothing of it has been written, and the workgroup of its cluster
 * that leaves last solves it (and the cluster's remaining problems) alone with the streaming kernel, inside the same
 * launch; the other problems of the batch are not affected.  d_max_iter_exit is therefore always 0 or 1.  Setting the
 * environment variable GBDPCG_NO_CLUSTER before the first solve of a process switches the form off (general storage is
 * then streamed every iteration, 3.4x slower at the config-3 shape). */

/* Symmetric storage.  S and Pinv of an MPC Schur system are symmetric block-tridiagonal, i.e. in
 * storage L_{k+1} == R_k^T for every knot (README.md:8; the symmetric-stair preconditioner of
 * gbdpcg_form_pinv_* satisfies it bit for bit whenever S does).  Batched solves can then read only
 * [D_k | R_k] of every block-row (2/3 of the bytes) and form L_{k+1} x_k as R_k^T x_k on the fly: with
 * exactly symmetric storage this multiplies the same numbers as the reference, which always reads L_k
 * (include/utils.cuh:77-83); only the summation order differs.  For stateSize 14, fp32, knotPoints <= 128
 * the halves of BOTH matrices (401 KB) then fit the registers + LDS of one compute unit and are read once
 * per solve instead of once per iteration.
 *   mode 2 (default): the relation is TESTED on the device, bit for bit, per problem, before every
 *           solve (one extra pass over L and R of both matrices: 74 us for 1024 problems of n=14, N=128);
 *           problems that pass run the symmetric kernel, the others the general one.  No host round trip.
 *   mode 1: the caller asserts it; no test.   mode 0: never; always read L.
 * Shapes without a symmetric kernel (and solves without a preconditioner) use the general kernels.
 * gbdpcg_check_symmetric_* exposes the test: d_flags[b] = 1 iff problem b satisfies the relation. */
gbdpcg_status gbdpcg_set_symmetric(gbdpcg_handle_t h, int mode);
gbdpcg_status gbdpcg_check_symmetric_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                         const float *d_M, uint8_t *d_flags, void *stream);
gbdpcg_status gbdpcg_check_symmetric_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                         const double *d_M, uint8_t *d_flags, void *stream);

/* ---- sizing helpers -------------------------------------------------------------------- */

/* pcgSharedMemSize<T> (include/pcg.cuh:13-20): elem_size * max(6n^2 + 10n + 2max(n,N), 9n^2).
 * Kept for callers that print / check it; this library sizes its own LDS. */
size_t gbdpcg_pcg_shared_mem_size(uint32_t elem_size, uint32_t n, uint32_t N);

/* checkPcgOccupancy<T> (include/pcg.cuh:23-49): GBDPCG_OK if a (n, N, batch) solve can run on
 * the handle's device, GBDPCG_ERR_TOO_LARGE otherwise (the reference exits 5/6 instead). */
gbdpcg_status gbdpcg_check_occupancy(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N,
                                     uint32_t batch);

/* Bytes of device workspace the SPLIT path needs for this shape (0 for FUSED).  The handle
 * grows its own workspace (and the verdict bytes of the device symmetry check) on demand outside
 * stream capture; call gbdpcg_reserve first when a solve will be captured into a caller-owned graph.
 * Growth never frees: graphs captured earlier keep the old buffers in their kernel nodes, so a replaced
 * buffer stays allocated until gbdpcg_destroy (sizes at least double, so at most 2x the largest is held).
 * The persistent path keeps one small zero-initialised hand-off workspace per shape it has run (element size, n, N,
 * batch), created on first use outside capture (or by gbdpcg_reserve) and kept until gbdpcg_destroy.
 * The split workspace is 6 vectors and 3 N partial sums per problem.  Largest batch it has been run at
 * (tests/test_gpu_large_batch.py): 57,100 problems of stateSize 14, 128 knots in fp32 -- 2,543,690,800 bytes, past 2^31 --
 * and 2,160 problems of stateSize 36, 256 knots in fp64. */
size_t gbdpcg_workspace_bytes(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N,
                              uint32_t batch);
gbdpcg_status gbdpcg_reserve(gbdpcg_handle_t h, uint32_t elem_size, uint32_t n, uint32_t N,
                             uint32_t batch);

/* ---- the hot path ---------------------------------------------------------------------- */

/* y = M x, block-tridiagonal, batched.  Replaces loadbdVec + bdmv (include/utils.cuh:9-85) as a
 * standalone operator; this is the kernel the HBM-roofline target is quoted on.
 * All pointers are device pointers; x and y must not alias. */
gbdpcg_status gbdpcg_spmv_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                              const float *d_M, const float *d_x, float *d_y, void *stream);
gbdpcg_status gbdpcg_spmv_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                              const double *d_M, const double *d_x, double *d_y, void *stream);

/* PCG solve of  Pinv S lambda = Pinv gamma  for `batch` independent problems.
 * Replaces the kernel pcg<T,n,N> (include/pcg.cuh:54-218) and its launch
 * (include/interface.cuh:110-133); same algorithm, same exit test (|eta_new| < tol, absolute),
 * same outputs:
 *   d_lambda  [batch*nN] in: initial guess, out: solution              (pcg.cuh:119,215)
 *   d_r, d_p  [batch*nN] out: final residual / direction, may be NULL  (pcg.cuh:125,175,139,205)
 *   d_iters   [batch]    out: iterations taken                         (pcg.cuh:212)
 *   d_max_iter_exit [batch] out: 1 if the loop ran out, 0 if converged (pcg.cuh:212), may be NULL
 * d_Pinv == NULL means the identity preconditioner.  The reference's scratch arguments
 * d_v_temp / d_eta_new_temp (interface.cuh:101-102) have no counterpart: dot products are
 * reduced on chip.  Asynchronous on `stream`; no host synchronisation.
 * A start from an exactly zero preconditioned residual (gamma == 0 with d_lambda == 0, or a warm start that solves the system
 * exactly) follows the reference's rule as well (pcg.cuh:169,195): the first alpha is 0/0, so lambda, r and p of THAT problem
 * come back NaN in every entry, |NaN| < tol is false, d_iters = max_iter and d_max_iter_exit = 1.  It is confined to its
 * problem: the other problems of the batch keep every bit, and nothing stays behind in the handle.  Detect it on the device
 * by d_max_iter_exit, or by the NaN norms gbdpcg_kkt_residual_* reports for such a point. */
gbdpcg_status gbdpcg_solve_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                               const float *d_S, const float *d_Pinv, const float *d_gamma,
                               float *d_lambda, float *d_r, float *d_p, float tol,
                               uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                               void *stream);
gbdpcg_status gbdpcg_solve_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                               const double *d_S, const double *d_Pinv, const double *d_gamma,
                               double *d_lambda, double *d_r, double *d_p, double tol,
                               uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                               void *stream);

/* Single-problem, blocking form of the device-pointer overload solvePCG<T>(state_size,
 * knot_points, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_v_temp, d_eta_new_temp, config)
 * (include/interface.cuh:92-144): launches on the null stream, waits, returns the iteration
 * count through *h_iters (what the reference returns at :143) and the max-iter flag the
 * reference computes but never copies back (:107-108,141). */
gbdpcg_status gbdpcg_solve_blocking_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N,
                                        const float *d_S, const float *d_Pinv,
                                        const float *d_gamma, float *d_lambda, float *d_r,
                                        float *d_p, float tol, uint32_t max_iter,
                                        uint32_t *h_iters, uint8_t *h_max_iter_exit);
gbdpcg_status gbdpcg_solve_blocking_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N,
                                        const double *d_S, const double *d_Pinv,
                                        const double *d_gamma, double *d_lambda, double *d_r,
                                        double *d_p, double tol, uint32_t max_iter,
                                        uint32_t *h_iters, uint8_t *h_max_iter_exit);

/* Host-pointer form of solvePCG<T>(h_S, h_gamma, h_lambda, stateSize, knotPoints, config)
 * (include/interface.cuh:24-89): allocates device buffers, copies S / gamma / lambda in,
 * solves, copies lambda out, frees.  Documented deviations from the reference, whose
 * behaviour here is undefined (it never initialises Pinv, :45-46,57-59, and returns the
 * constant 1, :88): h_Pinv == NULL means the identity preconditioner, and *h_iters receives
 * the real iteration count. */
gbdpcg_status gbdpcg_solve_host_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, const float *h_S,
                                    const float *h_Pinv, const float *h_gamma, float *h_lambda,
                                    float tol, uint32_t max_iter, uint32_t *h_iters,
                                    uint8_t *h_max_iter_exit);
gbdpcg_status gbdpcg_solve_host_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, const double *h_S,
                                    const double *h_Pinv, const double *h_gamma, double *h_lambda,
                                    double tol, uint32_t max_iter, uint32_t *h_iters,
                                    uint8_t *h_max_iter_exit);

/* ---- hipGraph-captured solves ---------------------------------------------------------- */

/* Captures gbdpcg_solve_* with these exact arguments into an executable hipGraph (the
 * "whole loop hipGraph-captured" of the north star).  MPC callers re-solve with the same
 * buffers every control step: build once, gbdpcg_graph_launch per step. */
gbdpcg_status gbdpcg_graph_create_solve_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N,
                                            uint32_t batch, const float *d_S, const float *d_Pinv,
                                            const float *d_gamma, float *d_lambda, float *d_r,
                                            float *d_p, float tol, uint32_t max_iter,
                                            uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                            gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_solve_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N,
                                            uint32_t batch, const double *d_S,
                                            const double *d_Pinv, const double *d_gamma,
                                            double *d_lambda, double *d_r, double *d_p, double tol,
                                            uint32_t max_iter, uint32_t *d_iters,
                                            uint8_t *d_max_iter_exit, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_launch(gbdpcg_graph_t g, void *stream);
gbdpcg_status gbdpcg_graph_destroy(gbdpcg_graph_t g);

/* ---- either side of the solve ---------------------------------- */

/* Builds Pinv from S on the device (f1): the step the reference's host overload lacks
 * (interface.cuh:33-34,45-46) and MPCGPU does with the block helpers of
 * include/utils.cuh:96-161.  d_Pinv gets the same [L|D|R] layout as d_S.
 * The D_k of S are taken to be symmetric: the kernels invert D_k and write the UPPER triangle of D_k^-1 into both
 * halves of the block (so that the stair comes out symmetric bit for bit whenever S is), which is D_k^-1 only for a
 * symmetric D_k.  L_{k+1} and R_k are independent: the left slot -D_{k+1}^-1 L_{k+1} D_k^-1 is evaluated from L_{k+1} itself
 * whenever it is not the mirror image of R_k, in every symmetric mode (tests/test_gpu_layout.py). */
gbdpcg_status gbdpcg_form_pinv_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                   const float *d_S, float *d_Pinv, gbdpcg_pinv_kind kind,
                                   void *stream);
gbdpcg_status gbdpcg_form_pinv_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                   const double *d_S, double *d_Pinv, gbdpcg_pinv_kind kind,
                                   void *stream);

/* gbdpcg_form_pinv_* followed by gbdpcg_solve_* on the same stream, as one call: what an SQP step does with a
 * freshly formed S (the host overload of the reference stops short of it, interface.cuh:33-34).  d_Pinv is an
 * OUTPUT here and stays valid afterwards.  In symmetric mode 2, for the shapes the one-launch stair kernel covers
 * (even stateSize <= 16), that kernel already compares L_{k+1} with R_k^T of S pair by pair -- it writes the pair
 * of Pinv as mirror images when they match -- so its per-problem verdict replaces the solve's own test launch
 * (74 us of a 0.30 ms converged solve of 1024 problems, n=14, N=128).  Same results as the two calls.
 * The graph form captures both steps for fixed buffers: replay it after rewriting S and gamma in place. */
gbdpcg_status gbdpcg_form_pinv_solve_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                         const float *d_S, float *d_Pinv, gbdpcg_pinv_kind kind,
                                         const float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                         float tol, uint32_t max_iter, uint32_t *d_iters,
                                         uint8_t *d_max_iter_exit, void *stream);
gbdpcg_status gbdpcg_form_pinv_solve_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                         const double *d_S, double *d_Pinv, gbdpcg_pinv_kind kind,
                                         const double *d_gamma, double *d_lambda, double *d_r, double *d_p,
                                         double tol, uint32_t max_iter, uint32_t *d_iters,
                                         uint8_t *d_max_iter_exit, void *stream);
gbdpcg_status gbdpcg_graph_create_form_pinv_solve_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N,
                                                      uint32_t batch, const float *d_S, float *d_Pinv,
                                                      gbdpcg_pinv_kind kind, const float *d_gamma,
                                                      float *d_lambda, float *d_r, float *d_p, float tol,
                                                      uint32_t max_iter, uint32_t *d_iters,
                                                      uint8_t *d_max_iter_exit, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_form_pinv_solve_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N,
                                                      uint32_t batch, const double *d_S, double *d_Pinv,
                                                      gbdpcg_pinv_kind kind, const double *d_gamma,
                                                      double *d_lambda, double *d_r, double *d_p,
                                                      double tol, uint32_t max_iter, uint32_t *d_iters,
                                                      uint8_t *d_max_iter_exit, gbdpcg_graph_t *out);

/* The MPCGPU steps either side of the solve (f4): forming S and gamma from the KKT blocks of a batch of linearised
 * MPC problems, and recovering the primal step from lambda.  The reference tree has no code for them (README.md:2-11
 * states the system that comes out, README.md:66-77 cites the paper), so the convention is fixed here:
 *
 *     minimise    sum_k  1/2 x_k' Q_k x_k + q_k' x_k  +  sum_{k<N-1} 1/2 u_k' R_k u_k + r_k' u_k
 *     subject to  x_0 = c_0,    x_{k+1} - A_k x_k - B_k u_k = c_{k+1}                       (k = 0 .. knotPoints-1)
 *
 * i.e. 1/2 z'Gz + g'z subject to Cz = c, z = (x_0, u_0, x_1, ..., x_{N-1}); Gz + g + C'lambda = 0 gives
 *     S lambda = gamma,  S = C G^-1 C',  gamma = -(c + C G^-1 g),      z = -G^-1 (g + C' lambda)
 * with D_0 = Q_0^-1, D_k = A_j Q_j^-1 A_j' + B_j R_j^-1 B_j' + Q_k^-1 (j = k-1), L_k = -A_j Q_j^-1, R_k = L_{k+1}'.
 * Packed device arrays, one problem after the other, every block column-major (nx = stateSize, nu = controlSize):
 *     d_G    [Q_0 R_0 Q_1 R_1 ... Q_{N-1}]   (nx^2+nu^2) N - nu^2     cost Hessians, symmetric; positive definite for the calls
 *                                                                     below, G + rho I positive definite for the _reg calls
 *     d_C    [A_0 B_0 A_1 B_1 ... B_{N-2}]   (nx^2+nx nu)(N-1)        dynamics Jacobians (A: nx x nx, B: nx x nu)
 *     d_g    [q_0 r_0 q_1 r_1 ... q_{N-1}]   (nx+nu) N - nu           cost gradients; d_z has this layout too
 *     d_c    [c_0 ... c_{N-1}]               nx N                     constraint residuals
 *     d_S, d_gamma                            3 nx^2 N, nx N           what gbdpcg_solve_* takes (n = nx)
 *     d_Ginv                                  as d_G                   every block inverted (may be NULL in form_schur)
 * The S written is exactly symmetric in storage (L_{k+1} == R_k' bit for bit), so the default symmetric mode of the solve
 * takes its resident kernels.  Shapes whose per-row working set exceeds one compute unit's LDS (7 nx^2 + 3 nu^2 elements
 * > 160 KB) give GBDPCG_ERR_UNSUPPORTED. */
gbdpcg_status gbdpcg_form_schur_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                    const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                    float *d_S, float *d_gamma, float *d_Ginv, void *stream);
gbdpcg_status gbdpcg_form_schur_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                    const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                    double *d_S, double *d_gamma, double *d_Ginv, void *stream);
gbdpcg_status gbdpcg_recover_primal_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                        const float *d_Ginv, const float *d_C, const float *d_g,
                                        const float *d_lambda, float *d_z, void *stream);
gbdpcg_status gbdpcg_recover_primal_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                        const double *d_Ginv, const double *d_C, const double *d_g,
                                        const double *d_lambda, double *d_z, void *stream);

/* One inner step of the SQP loop as ONE call (or one hipGraph for fixed buffers): gbdpcg_form_schur_* writes S, gamma and
 * G^-1, gbdpcg_form_pinv_solve_* forms Phi^-1 from that S (the S of form_schur is symmetric in storage, so in the default
 * symmetric mode the solve runs its resident symmetric kernels without a test launch of its own) and iterates from the
 * d_lambda it finds (warm start), gbdpcg_recover_primal_* writes the primal step z.  Same results as the three calls.
 * Every buffer is the caller's (layouts above); d_r, d_p may be NULL as in gbdpcg_solve_*.  Replay the graph after
 * rewriting G, C, g, c (and lambda, if no warm start is wanted) in place.
 * Exactly zero right-hand sides.  A problem with g = 0 and c = 0 (a regulator at its set-point), or any g, c whose
 * gamma = -(c + C G^-1 g) is exactly zero, started from lambda = 0 has the true answer z = 0, lambda = 0 -- and does NOT get it:
 * the gamma written is exactly zero, the solve starts from a zero residual and returns what the exit rule of gbdpcg_solve_*
 * above states (the reference's rule), so d_lambda and d_z of that problem are NaN in every entry, d_iters = max_iter and
 * d_max_iter_exit = 1.  The same holds for gbdpcg_kkt_step_reg_*, gbdpcg_kkt_resolve_* (also for a warm start that already solves
 * the system exactly), the _shared twins, every gbdpcg_admm_*_step_* whose shifted gradient and c are zero, the backward pass on a
 * zero cotangent pair (gbd_pcg_amd.autograd masks those problems), and every graph form.  The mixed-precision refinement at a point
 * whose fp64 defect is exactly zero writes d_res = (0, 0), e = 0 and a zero correction system, whose solve returns NaN;
 * gbdpcg_kkt_refine_apply then DESTROYS the point, which was exact: test d_res before applying.  In every case the damage is
 * confined to its problem: the other problems of the batch are bit-identical with a batch that has a regular problem in that
 * place, and nothing stays behind in the handle.  On the device the case shows as d_max_iter_exit = 1 and as NaN in both norms of
 * gbdpcg_kkt_residual_* for that problem (tests/test_gpu_kkt_degenerate.py). */
gbdpcg_status gbdpcg_kkt_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_G,
                                  const float *d_C, const float *d_g, const float *d_c, float *d_S, float *d_gamma,
                                  float *d_Ginv, float *d_Pinv, gbdpcg_pinv_kind kind, float *d_lambda, float *d_r, float *d_p,
                                  float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z,
                                  void *stream);
gbdpcg_status gbdpcg_kkt_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                  const double *d_C, const double *d_g, const double *d_c, double *d_S, double *d_gamma,
                                  double *d_Ginv, double *d_Pinv, gbdpcg_pinv_kind kind, double *d_lambda, double *d_r,
                                  double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                  double *d_z, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                               float *d_S, float *d_gamma, float *d_Ginv, float *d_Pinv, gbdpcg_pinv_kind kind,
                                               float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                               uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                               double *d_S, double *d_gamma, double *d_Ginv, double *d_Pinv,
                                               gbdpcg_pinv_kind kind, double *d_lambda, double *d_r, double *d_p, double tol,
                                               uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z,
                                               gbdpcg_graph_t *out);

/* A linearisation that is kept (linear and linear-time-varying MPC, real-time iterations, several inner steps on one set of
 * Jacobians): G and C are unchanged since the gbdpcg_form_schur_* or gbdpcg_kkt_step_* that wrote S, G^-1 (and Phi^-1), only the
 * gradients g and the residuals c are new (the measured state enters through c_0).  S, Phi^-1 and G^-1 stand, and
 *     gamma = -(c + C G^-1 g):   gamma_0 = -(c_0 + Q_0^-1 q_0),   gamma_k = -(c_k + Q_k^-1 q_k - A_j Q_j^-1 q_j - B_j R_j^-1 r_j)
 * is all that has to be formed before the solve.  gbdpcg_form_gamma_* does that from d_Ginv as form_schur wrote it (layouts
 * above): nothing is inverted, S is neither read nor written, d_gamma is the only output.  Asynchronous on `stream`,
 * capturable, never allocates.  d_C may be NULL when N == 1.  Null handle or required pointer, nx, nu, N or batch == 0:
 * GBDPCG_ERR_INVALID; a shape gbdpcg_form_schur_* refuses: GBDPCG_ERR_UNSUPPORTED. */
gbdpcg_status gbdpcg_form_gamma_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                    const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                    float *d_gamma, void *stream);
gbdpcg_status gbdpcg_form_gamma_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                    const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                    double *d_gamma, void *stream);

/* The whole step on a kept linearisation as ONE call (or one hipGraph for fixed buffers): gbdpcg_form_gamma_*, then
 * gbdpcg_solve_* on the caller's UNCHANGED d_S and d_Pinv (NULL: identity) from the d_lambda it finds (warm start), then
 * gbdpcg_recover_primal_*.  Same results as the three calls, bit for bit.  d_S, d_Pinv, d_Ginv, d_C, d_g, d_c are read only;
 * d_r, d_p, d_max_iter_exit may be NULL as in gbdpcg_solve_*.  The library cannot know that S was left alone since it was
 * formed, so the solve takes no shortcut on trust: it runs in the handle's symmetric mode like any gbdpcg_solve_* (the default
 * tests S and Pinv on the device).  A caller who keeps the S of form_schur untouched knows it to be symmetric in storage:
 * gbdpcg_set_symmetric(h, 1) is theirs to use.  Replay the graph after rewriting g and c (and lambda, if no warm start is
 * wanted) in place; like the other graph constructors it reserves what the solve needs. */
gbdpcg_status gbdpcg_kkt_resolve_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                     const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                     const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                     float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                     float *d_z, void *stream);
gbdpcg_status gbdpcg_kkt_resolve_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                     const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                     const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r,
                                     double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                     double *d_z, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_resolve_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                  const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                                  const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda,
                                                  float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                  uint8_t *d_max_iter_exit, float *d_z, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_resolve_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                  const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                                  const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda,
                                                  double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                  uint8_t *d_max_iter_exit, double *d_z, gbdpcg_graph_t *out);

/* Shared-matrix batches: ONE S and Phi^-1 (and ONE G^-1 and C) for `batch` right-hand sides -- one plant model against many
 * measured states or references: Monte-Carlo validation of a linear MPC, scenario MPC around one trajectory, a fleet of
 * identical robots.  Each entry point is the twin of the one named in it and takes the same arguments in the same order; the
 * difference is what the matrix pointers hold:
 *     gbdpcg_solve_shared_*, gbdpcg_graph_create_solve_shared_*              d_S, d_Pinv: 3 n^2 N elements each (d_Pinv NULL: identity)
 *     gbdpcg_form_gamma_shared_*, gbdpcg_recover_primal_shared_*             d_Ginv, d_C: one problem's blocks
 *     gbdpcg_kkt_resolve_shared_*, gbdpcg_graph_create_kkt_resolve_shared_*  d_Ginv, d_C, d_S, d_Pinv: one problem's each
 * Every vector (g, c, gamma, lambda, r, p, z) and d_iters / d_max_iter_exit stay per problem, problem-major, as in the twins.
 * No formation entry point is needed: the single matrices are what gbdpcg_form_schur_*, gbdpcg_form_pinv_* or
 * gbdpcg_kkt_step_* write with batch = 1.
 *  - Problem b gets exactly the bits its twin writes for problem b of a batch whose matrices are `batch` copies of the single
 *    ones, on the same handle in the same symmetric mode with the path set to GBDPCG_PATH_FUSED; batch = 1 is the twin.
 *  - A shared solve always runs on the fused family (one workgroup or one cluster of workgroups per problem), by the rules the
 *    twin applies to that n, N, batch and mode, whatever gbdpcg_set_path says.  A shape that does not fit one workgroup (36 x 256
 *    in fp64, say) gives GBDPCG_ERR_UNSUPPORTED and nothing is written: the persistent and split forms have no shared
 *    counterpart.  Where a kernel keeps a problem's matrices on chip (stateSize 14 in fp32, and the small blocks) a workgroup
 *    loads the one pair once and keeps it for all of its problems; elsewhere the pair is re-read from the caches.
 *  - Symmetric mode 2 tests the ONE pair once per call, on the device, and every problem follows that verdict; modes 1 and 0
 *    are as in gbdpcg_set_symmetric.
 *  - Exactly one problem's worth is read behind each single pointer: nothing past element 3 n^2 N of d_S / d_Pinv, nothing
 *    past one problem's extent of d_Ginv / d_C.
 *  - Everything else is as for the twins: asynchronous on `stream`, capturable, no allocation under capture (what
 *    gbdpcg_reserve sizes for (n, N, batch) suffices; the graph constructors reserve for themselves), warm start from
 *    d_lambda, d_r / d_p / d_max_iter_exit may be NULL, and the same error codes. */
gbdpcg_status gbdpcg_solve_shared_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const float *d_S,
                                      const float *d_Pinv, const float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                      float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, void *stream);
gbdpcg_status gbdpcg_solve_shared_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch, const double *d_S,
                                      const double *d_Pinv, const double *d_gamma, double *d_lambda, double *d_r, double *d_p,
                                      double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, void *stream);
gbdpcg_status gbdpcg_graph_create_solve_shared_f32(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                                   const float *d_S, const float *d_Pinv, const float *d_gamma, float *d_lambda,
                                                   float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                   uint8_t *d_max_iter_exit, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_solve_shared_f64(gbdpcg_handle_t h, uint32_t n, uint32_t N, uint32_t batch,
                                                   const double *d_S, const double *d_Pinv, const double *d_gamma, double *d_lambda,
                                                   double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                   uint8_t *d_max_iter_exit, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_form_gamma_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                           const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                           float *d_gamma, void *stream);
gbdpcg_status gbdpcg_form_gamma_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                           const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                           double *d_gamma, void *stream);
gbdpcg_status gbdpcg_recover_primal_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const float *d_Ginv, const float *d_C, const float *d_g, const float *d_lambda,
                                               float *d_z, void *stream);
gbdpcg_status gbdpcg_recover_primal_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const double *d_Ginv, const double *d_C, const double *d_g, const double *d_lambda,
                                               double *d_z, void *stream);
gbdpcg_status gbdpcg_kkt_resolve_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                            const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                            const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                            float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                            uint8_t *d_max_iter_exit, float *d_z, void *stream);
gbdpcg_status gbdpcg_kkt_resolve_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                            const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                            const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r,
                                            double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                            uint8_t *d_max_iter_exit, double *d_z, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_resolve_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N,
                                                         uint32_t batch, const float *d_Ginv, const float *d_C, const float *d_g,
                                                         const float *d_c, const float *d_S, const float *d_Pinv, float *d_gamma,
                                                         float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                                         uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z,
                                                         gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_resolve_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N,
                                                         uint32_t batch, const double *d_Ginv, const double *d_C, const double *d_g,
                                                         const double *d_c, const double *d_S, const double *d_Pinv, double *d_gamma,
                                                         double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                                         uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z,
                                                         gbdpcg_graph_t *out);

/* Does a point (z, lambda) solve the KKT system?  The two conditions an outer loop terminates on, per problem, on the device --
 * for the step gbdpcg_kkt_step_*, gbdpcg_kkt_resolve_* or gbdpcg_kkt_resolve_shared_* has just written, or for any other point:
 *     d_res[2b]   = || G z + g + C' lambda ||_inf     stationarity of problem b
 *     d_res[2b+1] = || C z - c ||_inf                 feasibility of problem b
 * in the call's precision, row by row of the convention above (d_G holds the HESSIANS, not d_Ginv; d_z has the layout of d_g;
 * d_lambda that of d_gamma; d_res has 2 batch elements):
 *     stationarity, x-part of knot k:   Q_k x_k + q_k + lambda_k - A_k' lambda_{k+1}
 *     stationarity, u-part of knot k:   R_k u_k + r_k - B_k' lambda_{k+1}          (the last knot has neither product and no u)
 *     feasibility of knot 0:            x_0 - c_0
 *     feasibility of knot k+1:          x_{k+1} - A_k x_k - B_k u_k - c_{k+1}
 * Every entry is one fma chain in a fixed order, so the result is bit-identical from call to call.  Both outputs are
 * overwritten whatever d_res held before and do not depend on it.  A NaN anywhere in a problem's residual makes that norm
 * NaN (the maximum is taken over bit patterns, it does not drop NaN as fmax does); Inf stays Inf; the other problems of the
 * batch are unaffected.
 * One launch, no handle state: asynchronous on `stream`, capturable (callers capture it on their stream behind the step; there
 * is no graph constructor of its own), never allocates, frees or synchronises, needs nothing from gbdpcg_reserve.  d_C may be
 * NULL when N == 1.  Null handle or required pointer, nx, nu, N or batch == 0: GBDPCG_ERR_INVALID; a shape gbdpcg_form_schur_*
 * refuses: GBDPCG_ERR_UNSUPPORTED (nothing is written).
 * gbdpcg_kkt_residual_shared_*: the shared-matrix twin -- d_G and d_C are ONE problem's blocks, every vector and d_res stay
 * per problem; problem b gets exactly the bits the per-problem call gives it on `batch` copies, batch = 1 is the twin, and
 * exactly one problem's extent is read behind d_G and d_C. */
gbdpcg_status gbdpcg_kkt_residual_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                      const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                      const float *d_z, const float *d_lambda, float *d_res, void *stream);
gbdpcg_status gbdpcg_kkt_residual_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                      const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                      const double *d_z, const double *d_lambda, double *d_res, void *stream);
gbdpcg_status gbdpcg_kkt_residual_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                             const float *d_z, const float *d_lambda, float *d_res, void *stream);
gbdpcg_status gbdpcg_kkt_residual_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                             const double *d_z, const double *d_lambda, double *d_res, void *stream);

/* Per-problem regularisation: problem b is solved with G_b + rho_b I in place of G_b -- costs that are only positive SEMI-definite
 * (a tracking cost on part of the state, an unpenalised input: the plain calls divide by a zero pivot and return Inf / NaN), the
 * damping of a rejected SQP step, decided per problem, and the matrix a splitting method on a frozen factorisation needs.
 * Each entry point takes the argument list of the one it extends with `d_rho` directly after `d_c`:
 *     d_rho  [batch] elements in the call's precision, on the device; read when the kernel RUNS, not when the call is made
 * Wherever a kernel picks up Q_k or R_k of problem b, every diagonal entry d is replaced by fl(d + rho_b) -- one rounding in the
 * call's precision, done on chip: d_G is not modified, no second buffer, no extra launch -- and everything downstream is the
 * arithmetic of the call without _reg.  So:
 *  - d_Ginv holds the blocks of (G + rho I)^-1, S = C (G + rho I)^-1 C', gamma = -(c + C (G + rho I)^-1 g).
 *  - gbdpcg_form_gamma_*, gbdpcg_recover_primal_*, gbdpcg_kkt_resolve_* and their shared twins need no _reg form: they work on
 *    that d_Ginv (and S, Phi^-1) as they are and give the regularised gamma and step.
 *  - rho_b is NOT validated on the device: negative values, NaN or Inf are added as they are, the outputs of that problem are
 *    whatever the arithmetic gives, and the other problems of the batch are unaffected.
 *  - with rho_b = 0 for every b each output is bit-identical with the entry point without _reg (d + 0 is exact).
 *  - S stays exactly symmetric in storage (L_{k+1} == R_k' bit for bit: both uses of a block see the same sum), so the default
 *    symmetric mode takes its resident kernels as it does behind gbdpcg_form_schur_*.
 * gbdpcg_kkt_step_reg_* is gbdpcg_form_schur_reg_* + gbdpcg_form_pinv_solve_* + gbdpcg_recover_primal_*, same results bit for bit.
 * The graph of gbdpcg_graph_create_kkt_step_reg_* keeps the POINTER d_rho: rewrite rho in place between replays, from the host or
 * from a kernel on the same stream (the outer loop's accept / reject decision) -- no re-capture.
 * gbdpcg_kkt_residual_reg_*: d_res[2b] = || (G + rho I) z + g + C' lambda ||_inf, the stationarity of the REGULARISED system
 * ("did the regularised step solve what it was asked to"; gbdpcg_kkt_residual_* answers the same for the original system), and
 * the unchanged feasibility norm in d_res[2b+1]; the same NaN-propagating maximum, the same determinism, one capturable launch.
 * There is no shared-matrix twin of it (the shared matrices themselves come from gbdpcg_form_schur_reg_* with batch = 1; the
 * regularised stationarity of a shared batch is gbdpcg_kkt_residual_shared_* on a G that holds G + rho I).
 * d_rho == NULL: GBDPCG_ERR_INVALID, nothing is written; every other error rule is the one of the function extended. */
gbdpcg_status gbdpcg_form_schur_reg_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                        const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                        const float *d_rho, float *d_S, float *d_gamma, float *d_Ginv, void *stream);
gbdpcg_status gbdpcg_form_schur_reg_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                        const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                        const double *d_rho, double *d_S, double *d_gamma, double *d_Ginv, void *stream);
gbdpcg_status gbdpcg_kkt_step_reg_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_G,
                                      const float *d_C, const float *d_g, const float *d_c, const float *d_rho, float *d_S,
                                      float *d_gamma, float *d_Ginv, float *d_Pinv, gbdpcg_pinv_kind kind, float *d_lambda,
                                      float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                      uint8_t *d_max_iter_exit, float *d_z, void *stream);
gbdpcg_status gbdpcg_kkt_step_reg_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                      const double *d_C, const double *d_g, const double *d_c, const double *d_rho, double *d_S,
                                      double *d_gamma, double *d_Ginv, double *d_Pinv, gbdpcg_pinv_kind kind, double *d_lambda,
                                      double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                      uint8_t *d_max_iter_exit, double *d_z, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_step_reg_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                   const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                                   const float *d_rho, float *d_S, float *d_gamma, float *d_Ginv, float *d_Pinv,
                                                   gbdpcg_pinv_kind kind, float *d_lambda, float *d_r, float *d_p, float tol,
                                                   uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z,
                                                   gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_step_reg_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                   const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                                   const double *d_rho, double *d_S, double *d_gamma, double *d_Ginv,
                                                   double *d_Pinv, gbdpcg_pinv_kind kind, double *d_lambda, double *d_r,
                                                   double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                   uint8_t *d_max_iter_exit, double *d_z, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_kkt_residual_reg_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                          const float *d_rho, const float *d_z, const float *d_lambda, float *d_res,
                                          void *stream);
gbdpcg_status gbdpcg_kkt_residual_reg_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                          const double *d_rho, const double *d_z, const double *d_lambda, double *d_res,
                                          void *stream);

/* Box constraints on a kept linearisation: ADMM iterations whose solve is gbdpcg_kkt_resolve_* on a frozen factorisation.  Problem b is
 *     minimise 1/2 z'Gz + g'z   subject to   Cz = c,   lo <= z <= hi
 * and is split into z (which satisfies the dynamics Cz = c) and a copy w (which lies in the box), held together by the scaled
 * multiplier y of z = w, with a per-problem penalty rho_b > 0.  The matrices come from gbdpcg_form_schur_reg_* or
 * gbdpcg_kkt_step_reg_* with that rho, so d_Ginv, d_S and d_Pinv belong to G + rho I and stay as they are for every iteration; only
 * the gradient of the solve changes.  d_lo, d_hi (per element; -Inf / +Inf: no bound), the state d_w, d_y and the shifted gradient
 * d_gt have the layout of d_g; d_rho has `batch` elements and d_res 2 batch, all on the device in the call's precision.
 * One iteration (gbdpcg_admm_step_*), per element of problem b:
 *     (z, lambda) = gbdpcg_kkt_resolve_* with d_gt in the place of d_g        warm start from d_lambda
 *     v   = fl(z + y)
 *     w+  = v < lo ? lo : (v > hi ? hi : v)                                   comparisons, not fmin / fmax: a NaN v stays NaN
 *     y+  = fl(v - w+)                                                        exactly 0 wherever nothing was clipped
 *     gt+ = fma(-rho_b, fl(w+ - y+), g)                                       one rounding
 *     d_res[2b]   = max_i |fl(z_i - w+_i)|                                    primal residual || z - w ||_inf
 *     d_res[2b+1] = max_i |fl(rho_b fl(w+_i - w_i))|                          dual residual rho || w+ - w ||_inf
 * Every line is a single IEEE operation or a comparison, so d_w, d_y, d_gt and d_res are defined to the bit; the two maxima are
 * those of gbdpcg_kkt_residual_* (over bit patterns: exact in any order, a NaN is that problem's norm, Inf stays Inf) and d_res is
 * overwritten whatever it held.  Which output is which: d_z satisfies the dynamics to the accuracy of the solve, d_w satisfies the
 * box exactly; they agree to d_res[2b], and at convergence either is the solution.  The multiplier of the bounds is mu = rho y:
 * y_i > 0 where the upper bound is active, y_i < 0 where the lower one is, and G z + g + C' lambda + rho y -> 0.
 *  - gbdpcg_admm_init_*: before the first iteration.  w <- clip(w, lo, hi) by the same comparisons, y is left as it is,
 *    gt <- fma(-rho_b, fl(w - y), g).  With w = y = 0 and 0 inside the box gt = g: the first solve is the equality-constrained one.
 *    A warm start passes the w and y of the previous control step.
 *  - gbdpcg_admm_update_*: everything behind the solve, one launch -- reads z, w, y, lo, hi, g, writes w, y, gt and d_res.
 *  - gbdpcg_admm_step_*: gbdpcg_kkt_resolve_* (with d_gt for d_g) followed by gbdpcg_admm_update_* on the same stream, same results
 *    bit for bit; d_g itself is read by the update only.  The solve runs in the handle's symmetric mode like any kkt_resolve.
 *  - gbdpcg_admm_step_shared_*: d_Ginv, d_C, d_S, d_Pinv are ONE problem's, as in gbdpcg_kkt_resolve_shared_*; every vector, d_lo,
 *    d_hi, d_rho [batch], d_w, d_y, d_gt and d_res stay per problem.  The caller fills d_rho with the rho the single matrices were
 *    formed with; nothing checks that.
 *  - the graphs keep the POINTER d_rho like gbdpcg_graph_create_kkt_step_reg_* (rewriting rho in place changes the update, not the
 *    matrices: a new rho needs gbdpcg_kkt_step_reg_* again, or gbdpcg_admm_restep_* below, which also rescales y); the constructors reserve what the solve needs, nothing allocates under
 *    capture.  Replay the graph once per iteration and read d_res every few replays to stop.
 *  - d_rho, d_lo, d_hi are NOT validated on the device: lo > hi, NaN or a negative rho give what the formulas give, inside their
 *    own problem only.
 * Null handle or required pointer, nx, nu, N or batch == 0: GBDPCG_ERR_INVALID, nothing is written (d_r, d_p, d_max_iter_exit and
 * d_Pinv may be NULL as in gbdpcg_kkt_resolve_*, d_C when N == 1).  init and update are elementwise and refuse no shape; step
 * inherits every refusal of gbdpcg_kkt_resolve_* or its shared twin and refuses before anything is written.  Every
 * gbdpcg_graph_create_admm*_step_* (box, admm_lin and admm_soc alike) sets *out to NULL before its first refusal: a refused
 * constructor never leaves a stale handle behind. */
gbdpcg_status gbdpcg_admm_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_g,
                                   const float *d_lo, const float *d_hi, const float *d_rho, float *d_w, float *d_y, float *d_gt,
                                   void *stream);
gbdpcg_status gbdpcg_admm_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_g,
                                   const double *d_lo, const double *d_hi, const double *d_rho, double *d_w, double *d_y,
                                   double *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_g,
                                     const float *d_lo, const float *d_hi, const float *d_rho, const float *d_z, float *d_w,
                                     float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_g,
                                     const double *d_lo, const double *d_hi, const double *d_rho, const double *d_z, double *d_w,
                                     double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_Ginv,
                                   const float *d_C, const float *d_g, const float *d_c, const float *d_lo, const float *d_hi,
                                   const float *d_rho, const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda,
                                   float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                   uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res,
                                   void *stream);
gbdpcg_status gbdpcg_admm_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_Ginv,
                                   const double *d_C, const double *d_g, const double *d_c, const double *d_lo,
                                   const double *d_hi, const double *d_rho, const double *d_S, const double *d_Pinv,
                                   double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                   uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                   double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                                const float *d_lo, const float *d_hi, const float *d_rho, const float *d_S,
                                                const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                                float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res,
                                                gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                                const double *d_lo, const double *d_hi, const double *d_rho, const double *d_S,
                                                const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r, double *d_p,
                                                double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res,
                                                gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                          const float *d_lo, const float *d_hi, const float *d_rho, const float *d_S,
                                          const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r, float *d_p, float tol,
                                          uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w,
                                          float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                          const double *d_lo, const double *d_hi, const double *d_rho, const double *d_S,
                                          const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r, double *d_p,
                                          double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z,
                                          double *d_w, double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                       const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                                       const float *d_lo, const float *d_hi, const float *d_rho, const float *d_S,
                                                       const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                                       float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                       uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                                       float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                       const double *d_Ginv, const double *d_C, const double *d_g,
                                                       const double *d_c, const double *d_lo, const double *d_hi,
                                                       const double *d_rho, const double *d_S, const double *d_Pinv,
                                                       double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol,
                                                       uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                       double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res,
                                                       gbdpcg_graph_t *out);

/* Stage-wise linear inequality rows on a kept linearisation: the ADMM iterations of the box section with a matrix in front of z.
 * Problem b is
 *     minimise 1/2 z'Gz + g'z   subject to   Cz = c,   lo <= E z <= hi
 * E is block-diagonal with the blocks of G: Ex_k (mx x nx) acts on x_k, Eu_k (mu x nu) on u_k, the row counts mx, mu are the
 * same for every knot (rows that mix x_k and u_k are out of scope: G has no x-u block for E'E to land in).  The box is E = I.
 * Layouts, one problem after the other, every block column-major, all on the device in the call's precision:
 *     d_E                    [Ex_0 Eu_0 Ex_1 Eu_1 ... Ex_{N-1}]        (mx nx + mu nu) N - mu nu elements per problem
 *     d_lo, d_hi, d_w, d_y   rows [mx | mu | mx | ... | mx]            (mx + mu) N - mu per problem; -Inf / +Inf: no bound
 *     d_Gt as d_G, d_gt as d_g, d_rho `batch` elements, d_res 2 batch.
 * E z is split into E z (z satisfies the dynamics) and a copy w between the bounds, held together by the scaled multiplier y of
 * E z = w with a per-problem penalty rho_b > 0; the matrices of the solve belong to Gt = G + rho E'E, which stays block-diagonal
 * in the layout of d_G.  Every line below is ONE IEEE operation or a comparison, so every output is defined to the bit whatever
 * the launch shape.  A "chain" is acc = +0; acc = fma(a_i, b_i, acc) over the stated index in ascending order.
 *  - gbdpcg_admm_lin_form_*: per diagonal block P(i,j) = chain over rows r of E(r,i) E(r,j), Gt(i,j) = fma(rho_b, P(i,j), G(i,j)).
 *    Gt is bit-symmetric when G is; a block with no rows gives fma(rho_b, +0, G).  Every element is written once by the lane that
 *    read it: d_Gt == d_G is allowed.  The caller then runs gbdpcg_kkt_step_* on d_Gt (or gbdpcg_kkt_step_reg_* for an additional
 *    sigma I); the d_Ginv, d_S, d_Pinv it writes are kept for every iteration.
 *  - gbdpcg_admm_lin_update_*: after the resolve with d_gt in the place of d_g has written z,
 *        v_r  = chain over columns j of E(r,j) z_j           (rows of the block that owns z's segment)
 *        s_r  = fl(v_r + y_r)
 *        w+_r = s_r < lo_r ? lo_r : (s_r > hi_r ? hi_r : s_r)                    comparisons: a NaN stays NaN
 *        y+_r = fl(s_r - w+_r)                                                   exactly 0 where nothing was clipped
 *        t_r  = fl(w+_r - y+_r);   d_r = fl(w+_r - w_r)
 *        u_j  = chain over rows r of E(r,j) t_r;   e_j = chain over rows r of E(r,j) d_r
 *        gt_j = fma(-rho_b, u_j, g_j)
 *        d_res[2b]   = max_r |fl(v_r - w+_r)|                                    primal residual || E z - w ||_inf
 *        d_res[2b+1] = max_j |fl(rho_b e_j)|                                     dual residual rho || E'(w+ - w) ||_inf
 *    The maxima are those of gbdpcg_kkt_residual_* (over bit patterns, a NaN on top); d_res is overwritten whatever it held.  The
 *    multiplier of the rows is mu = rho y: y_r > 0 where the upper bound is active, < 0 where the lower one is, and
 *    G z + g + C' lambda + rho E'y -> 0.  d_w satisfies the bounds exactly, E z agrees with it to d_res[2b].
 *  - gbdpcg_admm_lin_init_*: before the first iteration.  w <- clip(w) by the same comparisons, y is not written,
 *    t = fl(w - y), gt_j = fma(-rho_b, u_j, g_j); z and res are not touched.
 *  - gbdpcg_admm_lin_step_*: gbdpcg_kkt_resolve_* with d_gt for d_g, then the update on the same stream, the same bits as the two
 *    calls.  gbdpcg_graph_create_admm_lin_step_* is its graph form: it keeps the POINTER d_rho (rewriting rho in place changes the
 *    update, not the matrices), reserves what the solve needs, and nothing allocates under capture.
 *  - the _shared twins of step and graph take ONE problem's d_Ginv, d_C, d_S, d_Pinv AND d_E; the vectors, the bounds, d_rho,
 *    d_w, d_y, d_gt and d_res stay per problem.
 *  - d_lo, d_hi, d_rho and d_E are NOT validated on the device: bad values stay inside their own problem.
 * Refused before anything is written: null handle or required pointer, nx, nu, N or batch == 0, no row at all (mx = mu = 0, or
 * mx = 0 with N = 1): GBDPCG_ERR_INVALID.  mx or mu above 64, or a knot whose blocks of E with its x, u and two copies of its rows
 * exceed 60 KB (the update kernel stages them in LDS): GBDPCG_ERR_UNSUPPORTED.  Step and graph inherit every refusal of
 * gbdpcg_kkt_resolve_* or its shared twin (d_r, d_p, d_max_iter_exit and d_Pinv may be NULL, d_C when N == 1). */
gbdpcg_status gbdpcg_admm_lin_form_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const float *d_G, const float *d_E, const float *d_rho, float *d_Gt,
                                       void *stream);
gbdpcg_status gbdpcg_admm_lin_form_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const double *d_G, const double *d_E, const double *d_rho, double *d_Gt,
                                       void *stream);
gbdpcg_status gbdpcg_admm_lin_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const float *d_g, const float *d_E, const float *d_lo, const float *d_hi,
                                       const float *d_rho, float *d_w, float *d_y, float *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_lin_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const double *d_g, const double *d_E, const double *d_lo,
                                       const double *d_hi, const double *d_rho, double *d_w, double *d_y, double *d_gt,
                                       void *stream);
gbdpcg_status gbdpcg_admm_lin_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                         uint32_t batch, const float *d_g, const float *d_E, const float *d_lo, const float *d_hi,
                                         const float *d_rho, const float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res,
                                         void *stream);
gbdpcg_status gbdpcg_admm_lin_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                         uint32_t batch, const double *d_g, const double *d_E, const double *d_lo,
                                         const double *d_hi, const double *d_rho, const double *d_z, double *d_w, double *d_y,
                                         double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                       const float *d_E, const float *d_lo, const float *d_hi, const float *d_rho,
                                       const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                       float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                       float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const double *d_Ginv, const double *d_C, const double *d_g,
                                       const double *d_c, const double *d_E, const double *d_lo, const double *d_hi,
                                       const double *d_rho, const double *d_S, const double *d_Pinv, double *d_gamma,
                                       double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                       uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                       double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                    uint32_t N, uint32_t batch, const float *d_Ginv, const float *d_C,
                                                    const float *d_g, const float *d_c, const float *d_E, const float *d_lo,
                                                    const float *d_hi, const float *d_rho, const float *d_S, const float *d_Pinv,
                                                    float *d_gamma, float *d_lambda, float *d_r, float *d_p, float tol,
                                                    uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z,
                                                    float *d_w, float *d_y, float *d_gt, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                    uint32_t N, uint32_t batch, const double *d_Ginv, const double *d_C,
                                                    const double *d_g, const double *d_c, const double *d_E, const double *d_lo,
                                                    const double *d_hi, const double *d_rho, const double *d_S,
                                                    const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r,
                                                    double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                    uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                                    double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_lin_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                              uint32_t batch, const float *d_Ginv, const float *d_C, const float *d_g,
                                              const float *d_c, const float *d_E, const float *d_lo, const float *d_hi,
                                              const float *d_rho, const float *d_S, const float *d_Pinv, float *d_gamma,
                                              float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                              uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y,
                                              float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                              uint32_t batch, const double *d_Ginv, const double *d_C, const double *d_g,
                                              const double *d_c, const double *d_E, const double *d_lo, const double *d_hi,
                                              const double *d_rho, const double *d_S, const double *d_Pinv, double *d_gamma,
                                              double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                              uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                              double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                           uint32_t N, uint32_t batch, const float *d_Ginv, const float *d_C,
                                                           const float *d_g, const float *d_c, const float *d_E,
                                                           const float *d_lo, const float *d_hi, const float *d_rho,
                                                           const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda,
                                                           float *d_r, float *d_p, float tol, uint32_t max_iter,
                                                           uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w,
                                                           float *d_y, float *d_gt, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                           uint32_t N, uint32_t batch, const double *d_Ginv, const double *d_C,
                                                           const double *d_g, const double *d_c, const double *d_E,
                                                           const double *d_lo, const double *d_hi, const double *d_rho,
                                                           const double *d_S, const double *d_Pinv, double *d_gamma,
                                                           double *d_lambda, double *d_r, double *d_p, double tol,
                                                           uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                           double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res,
                                                           gbdpcg_graph_t *out);

/* Second-order cone rows next to the linear ones: norm bounds ||u_k||_2 <= r, friction cones ||(f_x, f_y)||_2 <= mu f_z, speed
 * limits.  Problem b is
 *     minimise 1/2 z'Gz + g'z   subject to   Cz = c,   lo <= (E z)_r <= hi on linear rows,   (E z + f)_cone in K_q on cone rows
 * with K_q = {(s_0, s_1 .. s_{q-1}) : ||(s_1 .. s_{q-1})||_2 <= s_0}.  d_E, its layout, the row packing [mx | mu | mx | ... | mx],
 * d_w, d_y, d_gt, d_rho and d_res are exactly those of gbdpcg_admm_lin_*, and Gt = G + rho E'E is formed by gbdpcg_admm_lin_form_*,
 * which does not depend on the set the rows are projected on.
 * ROW CLASSES, the four sizes directly behind mx, mu: in every x block the first lx rows are linear, the remaining mx - lx rows are
 * consecutive cones of dimension qx, head row (s_0) first; lu, qu do the same for the u blocks.  The split is the same for every
 * knot and every problem.  ON A CONE ROW d_lo[r] HOLDS THE OFFSET f_r AND d_hi[r] IS NOT READ (no further array, and less traffic
 * on a cone row than on a linear one).  A constant bound ||u||_2 <= r is a head row with a zero row of E and f = r.
 * Every line is one IEEE operation or a comparison, chains run in ascending index order, sqrt and / are correctly rounded:
 *  - gbdpcg_admm_soc_update_*: linear rows take the lines of gbdpcg_admm_lin_update_* unchanged.  Cone rows:
 *        v_r  = chain over columns j of E(r,j) z_j, SEEDED with f_r instead of +0    (acc = f_r; acc = fma(E(r,j), z_j, acc))
 *        s_r  = fl(v_r + y_r)
 *        per cone (its rows 0 .. q-1):
 *          n2 = chain over i = 1 .. q-1 of s_i s_i                                   (acc = +0; acc = fma(s_i, s_i, acc))
 *          a  = sqrt(n2)
 *          if      a <=  s_0 : w+ = s                                                (all rows of the cone)
 *          else if a <= -s_0 : w+ = +0                                               (all rows)
 *          else    h = fl(0.5 fl(s_0 + a));  c = fl(h / a);  w+_0 = h;  w+_i = fl(c s_i)
 *        y+_r = fl(s_r - w+_r)
 *        t_r  = fl(fl(w+_r - y+_r) - f_r);   d_r = fl(w+_r - w_r)
 *    then, as for the linear rows, u_j and e_j are the column chains of t and d, gt_j = fma(-rho_b, u_j, g_j),
 *    d_res[2b] = max_r |fl(v_r - w+_r)| and d_res[2b+1] = max_j |fl(rho_b e_j)|, the maxima over bit patterns with a NaN on top.
 *    A NaN fails both comparisons, takes the third branch and stays NaN.  q = 1 is the half-line s_0 >= 0: an empty chain, a = +0.
 *    The multiplier of a cone, mu = rho y, lies in -K (minus the cone), and G z + g + C' lambda + rho E'y -> 0.  Unlike the clip,
 *    d_w satisfies ||w_{1..}||_2 <= w_0 only to a few ulp: c s_i is rounded.  E z + f agrees with w to d_res[2b].
 *  - gbdpcg_admm_soc_init_*: before the first iteration.  w <- the projection of w by the same lines with s := w; y is not written,
 *    t = fl(fl(w_r - y_r) - f_r) on cone rows and fl(w_r - y_r) on linear ones, gt_j = fma(-rho_b, u_j, g_j); z and res are not
 *    touched.
 *  - gbdpcg_admm_soc_step_*: gbdpcg_kkt_resolve_* with d_gt for d_g, then the update on the same stream, the same bits as the two
 *    calls; gbdpcg_graph_create_admm_soc_step_* is its graph form (it keeps the POINTER d_rho).  The _shared twins of step and graph
 *    take ONE problem's d_Ginv, d_C, d_S, d_Pinv AND d_E; everything else stays per problem.
 *  - with lx = mx and lu = mu (no cone row) every output has the bits of the gbdpcg_admm_lin_* call, and qx, qu are ignored.
 * Refused before anything is written: everything gbdpcg_admm_lin_* refuses (d_hi is required even where no row reads it), and with
 * GBDPCG_ERR_INVALID lx > mx, lu > mu, qx == 0 with mx > lx or qu == 0 with mu > lu, (mx - lx) % qx != 0, (mu - lu) % qu != 0.
 * Every INVALID is reported before any UNSUPPORTED.  Rows that mix x_k and u_k, cones of differing dimension inside one block,
 * rotated cones and a backward pass through the cone rows are out of scope. */
gbdpcg_status gbdpcg_admm_soc_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                       uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const float *d_g,
                                       const float *d_E, const float *d_lo, const float *d_hi, const float *d_rho, float *d_w,
                                       float *d_y, float *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_soc_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                       uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const double *d_g,
                                       const double *d_E, const double *d_lo, const double *d_hi, const double *d_rho, double *d_w,
                                       double *d_y, double *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_soc_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                         uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const float *d_g,
                                         const float *d_E, const float *d_lo, const float *d_hi, const float *d_rho,
                                         const float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soc_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                         uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const double *d_g,
                                         const double *d_E, const double *d_lo, const double *d_hi, const double *d_rho,
                                         const double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soc_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                       uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const float *d_Ginv,
                                       const float *d_C, const float *d_g, const float *d_c, const float *d_E, const float *d_lo,
                                       const float *d_hi, const float *d_rho, const float *d_S, const float *d_Pinv, float *d_gamma,
                                       float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                       uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res,
                                       void *stream);
gbdpcg_status gbdpcg_admm_soc_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                       uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const double *d_Ginv,
                                       const double *d_C, const double *d_g, const double *d_c, const double *d_E,
                                       const double *d_lo, const double *d_hi, const double *d_rho, const double *d_S,
                                       const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol,
                                       uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w,
                                       double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_soc_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                    uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch,
                                                    const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                                    const float *d_E, const float *d_lo, const float *d_hi, const float *d_rho,
                                                    const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda,
                                                    float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                    uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                                    float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_soc_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                    uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch,
                                                    const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                                    const double *d_E, const double *d_lo, const double *d_hi, const double *d_rho,
                                                    const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda,
                                                    double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                    uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                                    double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_soc_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                              uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch,
                                              const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                              const float *d_E, const float *d_lo, const float *d_hi, const float *d_rho,
                                              const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                              float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                              uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                              float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soc_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                              uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch,
                                              const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                              const double *d_E, const double *d_lo, const double *d_hi, const double *d_rho,
                                              const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda,
                                              double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                              uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                              double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_soc_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                           uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N,
                                                           uint32_t batch, const float *d_Ginv, const float *d_C, const float *d_g,
                                                           const float *d_c, const float *d_E, const float *d_lo,
                                                           const float *d_hi, const float *d_rho, const float *d_S,
                                                           const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                                           float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                           uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y,
                                                           float *d_gt, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_soc_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                           uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N,
                                                           uint32_t batch, const double *d_Ginv, const double *d_C,
                                                           const double *d_g, const double *d_c, const double *d_E,
                                                           const double *d_lo, const double *d_hi, const double *d_rho,
                                                           const double *d_S, const double *d_Pinv, double *d_gamma,
                                                           double *d_lambda, double *d_r, double *d_p, double tol,
                                                           uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                           double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res,
                                                           gbdpcg_graph_t *out);

/* Adaptive rho for the three ADMM families: residual balancing in powers of two, decided and applied on the device, and the
 * iteration that refactors with the new rho.  The number of ADMM iterations depends on rho by orders of magnitude and the problems
 * of a batch do not share one good value; these calls move rho_b per problem without a host round trip.
 * THE RULE.  All quantities are of the call's type, every line is ONE IEEE operation or a comparison.  Per problem b the inputs are
 * r = d_res[2b], s = d_res[2b+1] as the last update launch wrote them and rho = d_rho[b]; the host passes `ratio` (>= 1), `shift`
 * (1 .. 16, tau = 2^shift) and the limits 0 < rho_min <= rho_max, both finite:
 *     up = fl(rho tau)          dn = fl(rho (1/tau))                           tau and 1/tau are exact constants
 *     if      r > fl(ratio s)  and  up <= rho_max :  rho' = up,  e = +shift
 *     else if s > fl(ratio r)  and  dn >= rho_min :  rho' = dn,  e = -shift
 *     else                                           rho' = rho, e = 0
 *     y'_i = fl(y_i 2^-e)                            one multiplication; y is not touched in bits when e = 0
 * The tests are comparisons, so a NaN in r, s or rho leaves the problem as it is (e = 0).  Scaling y keeps the multiplier
 * mu = rho y the iteration carries: a caller who rewrites rho and forgets y restarts from a wrong multiplier.  Outputs: d_rho[b] =
 * rho' in place (one lane writes it and d_expo[b] = e, int32, after the workgroup has read rho), d_y in place.  d_res is read, never
 * written.  The rule's arguments always come in the order ratio, shift, rho_min, rho_max, d_expo.
 *  - gbdpcg_admm_rebalance_* (box): ONE launch that additionally writes gt_i = fma(-rho', fl(w_i - y'_i), g_i), the line of
 *    gbdpcg_admm_init_*.  d_w is read only: it lies in the box already (it was written by an update or an init).  For such a w the
 *    bits of d_y, d_gt, d_rho and d_expo are those of the rows form (below) over the layout of g followed by gbdpcg_admm_init_*.
 *  - gbdpcg_admm_lin_rebalance_*: the same launch without w, g, gt over the (mx + mu) N - mu rows of a problem, then
 *    gbdpcg_admm_lin_init_* on the same stream, which rebuilds d_gt with the new rho and y.  With E = I its outputs have the bits of
 *    the box call.
 *  - gbdpcg_admm_soc_rebalance_*: the same through gbdpcg_admm_soc_init_*.  That init RE-PROJECTS an already projected w, as it
 *    documents: on cone rows c s_i is rounded, so d_w may move by ulps.
 *  - gbdpcg_admm_restep_*, gbdpcg_admm_lin_restep_*, gbdpcg_admm_soc_restep_*: one whole iteration with a new rho on one stream --
 *    the family's rebalance; the refactorisation and solve with d_gt in the place of d_g; the family's update launch.  The box
 *    refactors with gbdpcg_kkt_step_reg_* on d_G and d_rho; the families with rows form d_Gt from d_G with gbdpcg_admm_lin_form_* and
 *    run gbdpcg_kkt_step_* on d_Gt.  The arguments are those of the family's step with d_G (rows: d_G, d_Gt) in front of d_Ginv,
 *    `kind` (the Phi^-1 of the refactorisation) behind d_Pinv and the rule at the end; d_Ginv, d_S, d_Pinv and d_rho are written.
 *    The results are bit-identical with the constituent calls made one after another.  The families with rows refuse d_Gt == d_G
 *    with GBDPCG_ERR_INVALID: the next restep needs the original G.  EVERY restep refactors EVERY problem, whether its rho moved or
 *    not: it costs a gbdpcg_kkt_step_* where a step costs a gbdpcg_kkt_resolve_*, so it is made once per P plain steps.
 *  - gbdpcg_graph_create_admm*_restep_*: the graph forms.  They keep the POINTERS d_rho, d_res and d_expo: the decision is taken
 *    from what d_res holds at replay.  *out is set to NULL before the first refusal.  Intended use: replay the family's step graph P
 *    times, the restep graph once, and read d_res (and d_expo) as before.
 *  - no _shared twins: not provided.  A shared batch has one factorisation and hence one rho.
 * Refused with GBDPCG_ERR_INVALID before anything is written, reserved or captured: a null handle or pointer among those named
 * (d_r, d_p and d_max_iter_exit may be NULL, d_C when N == 1; a restep needs d_Pinv and d_gamma), nx, nu, N or batch == 0, shift
 * outside 1 .. 16, ratio < 1, rho_min <= 0, rho_max < rho_min, a limit that is not finite, a NaN among them; for the rows what
 * gbdpcg_admm_lin_* / gbdpcg_admm_soc_* refuse.  A restep refuses everything its constituent calls would, every INVALID before every
 * UNSUPPORTED. */
gbdpcg_status gbdpcg_admm_rebalance_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_g,
                                        const float *d_res, float *d_rho, const float *d_w, float *d_y, float *d_gt, float ratio,
                                        uint32_t shift, float rho_min, float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_rebalance_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_g,
                                        const double *d_res, double *d_rho, const double *d_w, double *d_y, double *d_gt,
                                        double ratio, uint32_t shift, double rho_min, double rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_lin_rebalance_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const float *d_g, const float *d_E, const float *d_lo, const float *d_hi,
                                            const float *d_res, float *d_rho, float *d_w, float *d_y, float *d_gt, float ratio,
                                            uint32_t shift, float rho_min, float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_lin_rebalance_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const double *d_g, const double *d_E, const double *d_lo,
                                            const double *d_hi, const double *d_res, double *d_rho, double *d_w, double *d_y,
                                            double *d_gt, double ratio, uint32_t shift, double rho_min, double rho_max,
                                            int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_soc_rebalance_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                            uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const float *d_g,
                                            const float *d_E, const float *d_lo, const float *d_hi, const float *d_res, float *d_rho,
                                            float *d_w, float *d_y, float *d_gt, float ratio, uint32_t shift, float rho_min,
                                            float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_soc_rebalance_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                            uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const double *d_g,
                                            const double *d_E, const double *d_lo, const double *d_hi, const double *d_res,
                                            double *d_rho, double *d_w, double *d_y, double *d_gt, double ratio, uint32_t shift,
                                            double rho_min, double rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_G,
                                     float *d_Ginv, const float *d_C, const float *d_g, const float *d_c, const float *d_lo,
                                     const float *d_hi, float *d_rho, float *d_S, float *d_Pinv, gbdpcg_pinv_kind kind,
                                     float *d_gamma, float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                     uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                     float *d_res, float ratio, uint32_t shift, float rho_min, float rho_max, int32_t *d_expo,
                                     void *stream);
gbdpcg_status gbdpcg_admm_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                     double *d_Ginv, const double *d_C, const double *d_g, const double *d_c, const double *d_lo,
                                     const double *d_hi, double *d_rho, double *d_S, double *d_Pinv, gbdpcg_pinv_kind kind,
                                     double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                     uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                     double *d_gt, double *d_res, double ratio, uint32_t shift, double rho_min, double rho_max,
                                     int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                  const float *d_G, float *d_Ginv, const float *d_C, const float *d_g,
                                                  const float *d_c, const float *d_lo, const float *d_hi, float *d_rho, float *d_S,
                                                  float *d_Pinv, gbdpcg_pinv_kind kind, float *d_gamma, float *d_lambda, float *d_r,
                                                  float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                  uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                                  float *d_res, float ratio, uint32_t shift, float rho_min, float rho_max,
                                                  int32_t *d_expo, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                  const double *d_G, double *d_Ginv, const double *d_C, const double *d_g,
                                                  const double *d_c, const double *d_lo, const double *d_hi, double *d_rho,
                                                  double *d_S, double *d_Pinv, gbdpcg_pinv_kind kind, double *d_gamma,
                                                  double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                                  uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                                  double *d_gt, double *d_res, double ratio, uint32_t shift, double rho_min,
                                                  double rho_max, int32_t *d_expo, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_lin_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                         uint32_t batch, const float *d_G, float *d_Gt, float *d_Ginv, const float *d_C,
                                         const float *d_g, const float *d_c, const float *d_E, const float *d_lo, const float *d_hi,
                                         float *d_rho, float *d_S, float *d_Pinv, gbdpcg_pinv_kind kind, float *d_gamma,
                                         float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                         uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res,
                                         float ratio, uint32_t shift, float rho_min, float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_lin_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                         uint32_t batch, const double *d_G, double *d_Gt, double *d_Ginv, const double *d_C,
                                         const double *d_g, const double *d_c, const double *d_E, const double *d_lo,
                                         const double *d_hi, double *d_rho, double *d_S, double *d_Pinv, gbdpcg_pinv_kind kind,
                                         double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                         uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                         double *d_gt, double *d_res, double ratio, uint32_t shift, double rho_min, double rho_max,
                                         int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                      uint32_t N, uint32_t batch, const float *d_G, float *d_Gt, float *d_Ginv,
                                                      const float *d_C, const float *d_g, const float *d_c, const float *d_E,
                                                      const float *d_lo, const float *d_hi, float *d_rho, float *d_S, float *d_Pinv,
                                                      gbdpcg_pinv_kind kind, float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                                      float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                      float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, float ratio,
                                                      uint32_t shift, float rho_min, float rho_max, int32_t *d_expo,
                                                      gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                      uint32_t N, uint32_t batch, const double *d_G, double *d_Gt, double *d_Ginv,
                                                      const double *d_C, const double *d_g, const double *d_c, const double *d_E,
                                                      const double *d_lo, const double *d_hi, double *d_rho, double *d_S,
                                                      double *d_Pinv, gbdpcg_pinv_kind kind, double *d_gamma, double *d_lambda,
                                                      double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                      uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                                      double *d_res, double ratio, uint32_t shift, double rho_min, double rho_max,
                                                      int32_t *d_expo, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_soc_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                         uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const float *d_G,
                                         float *d_Gt, float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                         const float *d_E, const float *d_lo, const float *d_hi, float *d_rho, float *d_S,
                                         float *d_Pinv, gbdpcg_pinv_kind kind, float *d_gamma, float *d_lambda, float *d_r,
                                         float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                         float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, float ratio, uint32_t shift,
                                         float rho_min, float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_soc_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx,
                                         uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N, uint32_t batch, const double *d_G,
                                         double *d_Gt, double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                         const double *d_E, const double *d_lo, const double *d_hi, double *d_rho, double *d_S,
                                         double *d_Pinv, gbdpcg_pinv_kind kind, double *d_gamma, double *d_lambda, double *d_r,
                                         double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                         double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res, double ratio,
                                         uint32_t shift, double rho_min, double rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_soc_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                      uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N,
                                                      uint32_t batch, const float *d_G, float *d_Gt, float *d_Ginv,
                                                      const float *d_C, const float *d_g, const float *d_c, const float *d_E,
                                                      const float *d_lo, const float *d_hi, float *d_rho, float *d_S, float *d_Pinv,
                                                      gbdpcg_pinv_kind kind, float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                                      float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                      float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, float ratio,
                                                      uint32_t shift, float rho_min, float rho_max, int32_t *d_expo,
                                                      gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_soc_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                      uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu, uint32_t N,
                                                      uint32_t batch, const double *d_G, double *d_Gt, double *d_Ginv,
                                                      const double *d_C, const double *d_g, const double *d_c, const double *d_E,
                                                      const double *d_lo, const double *d_hi, double *d_rho, double *d_S,
                                                      double *d_Pinv, gbdpcg_pinv_kind kind, double *d_gamma, double *d_lambda,
                                                      double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                      uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                                      double *d_res, double ratio, uint32_t shift, double rho_min, double rho_max,
                                                      int32_t *d_expo, gbdpcg_graph_t *out);

/* Soft (L1-penalised) bounds for the box and the linear-row families: gbdpcg_admm_soft_* and gbdpcg_admm_lin_soft_*.  Every bound of
 * the hard families is a constraint; after a disturbance a state bound can contradict Cz = c, the hard problem then has no feasible
 * point, d_res[2b] stalls at the distance between the affine set and the box and y grows without bound.  The soft families replace
 * the constraint on row r by the exact penalty kappa_r dist(v_r, [lo_r, hi_r]) in the cost, v = z (box) or v = E z (rows): always
 * feasible, and equal to the hard solution wherever kappa_r exceeds the hard multiplier |mu_r| = rho |y_r| of that row, which the
 * caller can read from d_y of a hard (or sufficiently weighted soft) run.  d_kappa has the layout of d_lo and d_hi and stands
 * directly behind d_hi in every argument list, which otherwise is the hard family's; kappa_r in [0, +Inf] per row and per problem
 * (also in the _shared twins), in the call's precision.  Only the projection line of the update changes; with s = fl(v + y), every
 * line one IEEE operation or a comparison, / correctly rounded:
 *     p     = s < lo ? lo : (s > hi ? hi : s)                    the clip of the hard update
 *     e     = fl(s - p)                                          exactly 0 inside the bounds
 *     theta = fl(kappa / rho_b)
 *     w+    = e > theta ? fl(s - theta) : (e < -theta ? fl(s + theta) : p)
 *     y+    = e > theta ? theta         : (e < -theta ? -theta        : e)
 * and gt+, d_res[2b], d_res[2b+1] follow from w+, y+ and the old w exactly as in the hard update.  So |y_r| <= fl(kappa_r / rho_b):
 * the multiplier mu = rho y is bounded by the weight.
 *  - kappa = +Inf: the third branch, whose operations w+ = p, y+ = fl(s - p) are those of the hard update -- with +Inf everywhere
 *    every output of every gbdpcg_admm_soft_* / gbdpcg_admm_lin_soft_* call has the bits of the hard call.  Inputs are kept hard
 *    this way (or with a large finite kappa), states get a finite kappa.
 *  - kappa = 0: the row is free (w+ = s, y+ = 0).  A tie e = +-theta takes the third branch.  A NaN s fails every comparison and
 *    stays NaN, inside its own problem.
 *  - init (gbdpcg_admm_soft_init_*, gbdpcg_admm_lin_soft_init_*): w <- (kappa == +Inf) ? clip(w, lo, hi) : w -- a soft row admits any
 *    w, so the init is idempotent and a restep does not move w; y is not written; gt is computed from w - y as in the hard init.
 *  - step, the _shared twins, the graphs: the hard family's composition with the soft update launch, the same bits as the calls they
 *    are made of.
 *  - adaptive rho.  gbdpcg_admm_rebalance_* IS the rebalance of the soft box family: it never looks at the bounds and does not clip
 *    w.  gbdpcg_admm_lin_soft_rebalance_* is the launch of gbdpcg_admm_lin_rebalance_* followed by gbdpcg_admm_lin_soft_init_*.
 *    gbdpcg_admm_soft_restep_* = gbdpcg_admm_rebalance_*, gbdpcg_kkt_step_reg_*, gbdpcg_admm_soft_update_*;
 *    gbdpcg_admm_lin_soft_restep_* = its rebalance, gbdpcg_admm_lin_form_*, gbdpcg_kkt_step_*, gbdpcg_admm_lin_soft_update_*.  The
 *    scaling of y is a power of two and so is that of theta: |y| <= fl(kappa / rho') holds after a rebalance (short of subnormals).
 *  - d_kappa, like d_rho, d_lo and d_hi, is NOT validated on the device: a negative or NaN kappa is the caller's error and gives
 *    what the formulas give, inside its own problem.
 *  - not provided: soft cone rows (the prox of a distance-to-cone penalty is another closed form; gbdpcg_admm_soc_* stay hard),
 *    quadratic penalties, per-side weights, a _shared restep.
 * Refused: a NULL d_kappa with GBDPCG_ERR_INVALID before anything is written; everything else as the hard family refuses it, in the
 * same order. */
gbdpcg_status gbdpcg_admm_soft_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_g,
                                        const float *d_lo, const float *d_hi, const float *d_kappa, const float *d_rho, float *d_w,
                                        float *d_y, float *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_soft_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_g,
                                        const double *d_lo, const double *d_hi, const double *d_kappa, const double *d_rho,
                                        double *d_w, double *d_y, double *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_soft_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_g,
                                          const float *d_lo, const float *d_hi, const float *d_kappa, const float *d_rho,
                                          const float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soft_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const double *d_g, const double *d_lo, const double *d_hi, const double *d_kappa,
                                          const double *d_rho, const double *d_z, double *d_w, double *d_y, double *d_gt,
                                          double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soft_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                        const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                        const float *d_lo, const float *d_hi, const float *d_kappa, const float *d_rho,
                                        const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                        float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                        float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soft_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                        const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                        const double *d_lo, const double *d_hi, const double *d_kappa, const double *d_rho,
                                        const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r,
                                        double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                        double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_soft_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                     const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                                     const float *d_lo, const float *d_hi, const float *d_kappa, const float *d_rho,
                                                     const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda,
                                                     float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                     uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                                     float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_soft_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                     const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                                     const double *d_lo, const double *d_hi, const double *d_kappa,
                                                     const double *d_rho, const double *d_S, const double *d_Pinv, double *d_gamma,
                                                     double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                                     uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w,
                                                     double *d_y, double *d_gt, double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_soft_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const float *d_Ginv, const float *d_C, const float *d_g, const float *d_c,
                                               const float *d_lo, const float *d_hi, const float *d_kappa, const float *d_rho,
                                               const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                               float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                               uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                               float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_soft_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                               const double *d_lo, const double *d_hi, const double *d_kappa, const double *d_rho,
                                               const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda,
                                               double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                               uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                               double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_soft_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                            const float *d_Ginv, const float *d_C, const float *d_g,
                                                            const float *d_c, const float *d_lo, const float *d_hi,
                                                            const float *d_kappa, const float *d_rho, const float *d_S,
                                                            const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                                            float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                            uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y,
                                                            float *d_gt, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_soft_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                            const double *d_Ginv, const double *d_C, const double *d_g,
                                                            const double *d_c, const double *d_lo, const double *d_hi,
                                                            const double *d_kappa, const double *d_rho, const double *d_S,
                                                            const double *d_Pinv, double *d_gamma, double *d_lambda, double *d_r,
                                                            double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                            uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                                            double *d_gt, double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_soft_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_G,
                                          float *d_Ginv, const float *d_C, const float *d_g, const float *d_c, const float *d_lo,
                                          const float *d_hi, const float *d_kappa, float *d_rho, float *d_S, float *d_Pinv,
                                          gbdpcg_pinv_kind kind, float *d_gamma, float *d_lambda, float *d_r, float *d_p, float tol,
                                          uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w,
                                          float *d_y, float *d_gt, float *d_res, float ratio, uint32_t shift, float rho_min,
                                          float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_soft_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const double *d_G, double *d_Ginv, const double *d_C, const double *d_g,
                                          const double *d_c, const double *d_lo, const double *d_hi, const double *d_kappa,
                                          double *d_rho, double *d_S, double *d_Pinv, gbdpcg_pinv_kind kind, double *d_gamma,
                                          double *d_lambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                          uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                          double *d_gt, double *d_res, double ratio, uint32_t shift, double rho_min, double rho_max,
                                          int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_soft_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                       const float *d_G, float *d_Ginv, const float *d_C, const float *d_g,
                                                       const float *d_c, const float *d_lo, const float *d_hi, const float *d_kappa,
                                                       float *d_rho, float *d_S, float *d_Pinv, gbdpcg_pinv_kind kind,
                                                       float *d_gamma, float *d_lambda, float *d_r, float *d_p, float tol,
                                                       uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z,
                                                       float *d_w, float *d_y, float *d_gt, float *d_res, float ratio,
                                                       uint32_t shift, float rho_min, float rho_max, int32_t *d_expo,
                                                       gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_soft_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                       const double *d_G, double *d_Ginv, const double *d_C, const double *d_g,
                                                       const double *d_c, const double *d_lo, const double *d_hi,
                                                       const double *d_kappa, double *d_rho, double *d_S, double *d_Pinv,
                                                       gbdpcg_pinv_kind kind, double *d_gamma, double *d_lambda, double *d_r,
                                                       double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                       uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                                       double *d_gt, double *d_res, double ratio, uint32_t shift, double rho_min,
                                                       double rho_max, int32_t *d_expo, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_lin_soft_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const float *d_g, const float *d_E, const float *d_lo,
                                            const float *d_hi, const float *d_kappa, const float *d_rho, float *d_w, float *d_y,
                                            float *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const double *d_g, const double *d_E, const double *d_lo,
                                            const double *d_hi, const double *d_kappa, const double *d_rho, double *d_w,
                                            double *d_y, double *d_gt, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                              uint32_t batch, const float *d_g, const float *d_E, const float *d_lo,
                                              const float *d_hi, const float *d_kappa, const float *d_rho, const float *d_z,
                                              float *d_w, float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                              uint32_t batch, const double *d_g, const double *d_E, const double *d_lo,
                                              const double *d_hi, const double *d_kappa, const double *d_rho, const double *d_z,
                                              double *d_w, double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const float *d_Ginv, const float *d_C, const float *d_g,
                                            const float *d_c, const float *d_E, const float *d_lo, const float *d_hi,
                                            const float *d_kappa, const float *d_rho, const float *d_S, const float *d_Pinv,
                                            float *d_gamma, float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                            uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y,
                                            float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const double *d_Ginv, const double *d_C, const double *d_g,
                                            const double *d_c, const double *d_E, const double *d_lo, const double *d_hi,
                                            const double *d_kappa, const double *d_rho, const double *d_S, const double *d_Pinv,
                                            double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol,
                                            uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z,
                                            double *d_w, double *d_y, double *d_gt, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_soft_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                         uint32_t N, uint32_t batch, const float *d_Ginv, const float *d_C,
                                                         const float *d_g, const float *d_c, const float *d_E, const float *d_lo,
                                                         const float *d_hi, const float *d_kappa, const float *d_rho,
                                                         const float *d_S, const float *d_Pinv, float *d_gamma, float *d_lambda,
                                                         float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                         uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y, float *d_gt,
                                                         float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_soft_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                         uint32_t N, uint32_t batch, const double *d_Ginv, const double *d_C,
                                                         const double *d_g, const double *d_c, const double *d_E,
                                                         const double *d_lo, const double *d_hi, const double *d_kappa,
                                                         const double *d_rho, const double *d_S, const double *d_Pinv,
                                                         double *d_gamma, double *d_lambda, double *d_r, double *d_p, double tol,
                                                         uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                         double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res,
                                                         gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_lin_soft_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                   uint32_t N, uint32_t batch, const float *d_Ginv, const float *d_C,
                                                   const float *d_g, const float *d_c, const float *d_E, const float *d_lo,
                                                   const float *d_hi, const float *d_kappa, const float *d_rho, const float *d_S,
                                                   const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                                   float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                   float *d_z, float *d_w, float *d_y, float *d_gt, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                   uint32_t N, uint32_t batch, const double *d_Ginv, const double *d_C,
                                                   const double *d_g, const double *d_c, const double *d_E, const double *d_lo,
                                                   const double *d_hi, const double *d_kappa, const double *d_rho,
                                                   const double *d_S, const double *d_Pinv, double *d_gamma, double *d_lambda,
                                                   double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                   uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y, double *d_gt,
                                                   double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_soft_step_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx,
                                                                uint32_t mu, uint32_t N, uint32_t batch, const float *d_Ginv,
                                                                const float *d_C, const float *d_g, const float *d_c,
                                                                const float *d_E, const float *d_lo, const float *d_hi,
                                                                const float *d_kappa, const float *d_rho, const float *d_S,
                                                                const float *d_Pinv, float *d_gamma, float *d_lambda, float *d_r,
                                                                float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                                uint8_t *d_max_iter_exit, float *d_z, float *d_w, float *d_y,
                                                                float *d_gt, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_soft_step_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx,
                                                                uint32_t mu, uint32_t N, uint32_t batch, const double *d_Ginv,
                                                                const double *d_C, const double *d_g, const double *d_c,
                                                                const double *d_E, const double *d_lo, const double *d_hi,
                                                                const double *d_kappa, const double *d_rho, const double *d_S,
                                                                const double *d_Pinv, double *d_gamma, double *d_lambda,
                                                                double *d_r, double *d_p, double tol, uint32_t max_iter,
                                                                uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_z,
                                                                double *d_w, double *d_y, double *d_gt, double *d_res,
                                                                gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_lin_soft_rebalance_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                 uint32_t batch, const float *d_g, const float *d_E, const float *d_lo,
                                                 const float *d_hi, const float *d_kappa, const float *d_res, float *d_rho,
                                                 float *d_w, float *d_y, float *d_gt, float ratio, uint32_t shift, float rho_min,
                                                 float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_rebalance_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                 uint32_t batch, const double *d_g, const double *d_E, const double *d_lo,
                                                 const double *d_hi, const double *d_kappa, const double *d_res, double *d_rho,
                                                 double *d_w, double *d_y, double *d_gt, double ratio, uint32_t shift,
                                                 double rho_min, double rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                              uint32_t batch, const float *d_G, float *d_Gt, float *d_Ginv, const float *d_C,
                                              const float *d_g, const float *d_c, const float *d_E, const float *d_lo,
                                              const float *d_hi, const float *d_kappa, float *d_rho, float *d_S, float *d_Pinv,
                                              gbdpcg_pinv_kind kind, float *d_gamma, float *d_lambda, float *d_r, float *d_p,
                                              float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z,
                                              float *d_w, float *d_y, float *d_gt, float *d_res, float ratio, uint32_t shift,
                                              float rho_min, float rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                              uint32_t batch, const double *d_G, double *d_Gt, double *d_Ginv, const double *d_C,
                                              const double *d_g, const double *d_c, const double *d_E, const double *d_lo,
                                              const double *d_hi, const double *d_kappa, double *d_rho, double *d_S, double *d_Pinv,
                                              gbdpcg_pinv_kind kind, double *d_gamma, double *d_lambda, double *d_r, double *d_p,
                                              double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                              double *d_z, double *d_w, double *d_y, double *d_gt, double *d_res, double ratio,
                                              uint32_t shift, double rho_min, double rho_max, int32_t *d_expo, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_soft_restep_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                           uint32_t N, uint32_t batch, const float *d_G, float *d_Gt, float *d_Ginv,
                                                           const float *d_C, const float *d_g, const float *d_c, const float *d_E,
                                                           const float *d_lo, const float *d_hi, const float *d_kappa, float *d_rho,
                                                           float *d_S, float *d_Pinv, gbdpcg_pinv_kind kind, float *d_gamma,
                                                           float *d_lambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                                           uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_z, float *d_w,
                                                           float *d_y, float *d_gt, float *d_res, float ratio, uint32_t shift,
                                                           float rho_min, float rho_max, int32_t *d_expo, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_soft_restep_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                           uint32_t N, uint32_t batch, const double *d_G, double *d_Gt,
                                                           double *d_Ginv, const double *d_C, const double *d_g, const double *d_c,
                                                           const double *d_E, const double *d_lo, const double *d_hi,
                                                           const double *d_kappa, double *d_rho, double *d_S, double *d_Pinv,
                                                           gbdpcg_pinv_kind kind, double *d_gamma, double *d_lambda, double *d_r,
                                                           double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                           uint8_t *d_max_iter_exit, double *d_z, double *d_w, double *d_y,
                                                           double *d_gt, double *d_res, double ratio, uint32_t shift,
                                                           double rho_min, double rho_max, int32_t *d_expo, gbdpcg_graph_t *out);

/* The backward pass: gradients of a scalar through (G, C, g, c) -> (z, lambda), on the device.  Forward convention as above:
 * G z + g + C' lambda = 0, C z = c.  For a scalar l with upstream gradients gz = dl/dz (layout of d_g) and glam = dl/dlambda (layout
 * of d_c) let (a_z, a_lambda) solve the SAME KKT matrix with the right-hand side (-gz, -glam).  The matrix is symmetric, so this
 * is exactly gbdpcg_kkt_resolve_* called with g := gz, c := -glam on the S, Phi^-1 and G^-1 the forward pass left behind: the
 * adjoint solve needs no kernel of its own.  Split a_z into ax_k, au_k and z into x_k, u_k; then (checked entry by entry against
 * fp64 autograd through a dense solve of the same system, tests/test_kkt_grad_reference.py):
 *     dl/dg = a_z                                   dl/dc = -a_lambda
 *     dl/dQ_k(i,j) = 1/2 (ax_k,i x_k,j + x_k,i ax_k,j)                        and dl/dR_k likewise with u
 *     dl/dA_k(i,j) = -(a_lambda,k+1,i x_k,j + lambda_k+1,i ax_k,j)
 *     dl/dB_k(i,j) = -(a_lambda,k+1,i u_k,j + lambda_k+1,i au_k,j)
 * The symmetrised form is the one for G because the library reads G as symmetric (the gradient with G entering as 1/2 (G + G')).
 * Row block 0 of C is the identity and has no parameter.  With the _reg calls dl/drho_b = a_z' z of problem b and the gradient in
 * G is unchanged; the backward pass works on whatever d_Ginv, d_S, d_Pinv the forward pass factored.  dl/dg, dl/dc and dl/drho
 * are the adjoint pair itself or one dot product of it: the caller's.
 *  - gbdpcg_kkt_grad_*: (d_z, d_lambda, d_az, d_alambda) -> d_gG (layout and size of d_G) and d_gC (layout and size of d_C), per
 *    problem, one launch.  Each entry is two rounded products and one rounded add in the call's precision, then an exact * 0.5 (G)
 *    or an exact negation (C), with the operands in the order written above: defined to the bit whatever the launch shape, and
 *    gQ_k, gR_k come out bit-symmetric.  Every output element is written exactly once and does not depend on what the buffer
 *    held: no atomics, no memset, no scratch.  A NaN in problem b's inputs stays in problem b's outputs.  Either output pointer
 *    may be NULL, which skips it (both NULL: GBDPCG_ERR_INVALID); d_gC is not touched when N == 1.  No handle state:
 *    asynchronous on `stream`, capturable, never allocates, needs nothing from gbdpcg_reserve.
 *  - gbdpcg_kkt_grad_shared_*: d_gG, d_gC are ONE problem's worth, the sum over the batch of the expressions above -- the gradient
 *    in the single G and C of a shared-matrix batch.  Problem b's term is the per-problem entry; the terms are added in the order
 *    b = 0, 1, ..., batch - 1 by one thread per entry, without atomics: bit-identical from call to call, and batch = 1 gives the
 *    bits of the per-problem call.
 *  - gbdpcg_kkt_backward_*: gbdpcg_kkt_resolve_* with g := d_gz, c := d_nglam, writing d_alambda (its lambda: read first as the warm
 *    start of the adjoint PCG, as d_lambda is for the forward pass) and d_az (its z), followed by gbdpcg_kkt_grad_* on (d_z,
 *    d_lambda, d_az, d_alambda) on the same stream; same results as the two calls, bit for bit.  d_nglam holds MINUS dl/dlambda;
 *    the caller passes zeros when l does not depend on lambda.  d_z, d_lambda are the forward point, read only.  d_gamma, d_r, d_p,
 *    d_iters, d_max_iter_exit are those of the adjoint solve (d_r, d_p, d_max_iter_exit, d_Pinv may be NULL as in
 *    gbdpcg_kkt_resolve_*, d_C when N == 1).  The solve runs in the handle's symmetric mode and path like any kkt_resolve.
 *  - gbdpcg_kkt_backward_shared_*: the same on ONE problem's d_Ginv, d_C, d_S, d_Pinv (gbdpcg_kkt_resolve_shared_*), with the
 *    summed d_gG, d_gC of gbdpcg_kkt_grad_shared_*; every vector stays per problem.
 *  - the graph constructors capture both steps for fixed buffers and reserve what the solve needs, like those of
 *    gbdpcg_kkt_resolve_*: replay after rewriting d_gz and d_nglam (and d_alambda, if no warm start is wanted) in place.
 * Null handle or required pointer, nx, nu, N or batch == 0: GBDPCG_ERR_INVALID; a shape gbdpcg_form_schur_* refuses:
 * GBDPCG_ERR_UNSUPPORTED; the backward calls also inherit every refusal of gbdpcg_kkt_resolve_* or its shared twin.  Refusals
 * come before anything is written. */
gbdpcg_status gbdpcg_kkt_grad_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_z,
                                  const float *d_lambda, const float *d_az, const float *d_alambda, float *d_gG, float *d_gC,
                                  void *stream);
gbdpcg_status gbdpcg_kkt_grad_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_z,
                                  const double *d_lambda, const double *d_az, const double *d_alambda, double *d_gG, double *d_gC,
                                  void *stream);
gbdpcg_status gbdpcg_kkt_grad_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_z,
                                         const float *d_lambda, const float *d_az, const float *d_alambda, float *d_gG,
                                         float *d_gC, void *stream);
gbdpcg_status gbdpcg_kkt_grad_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_z,
                                         const double *d_lambda, const double *d_az, const double *d_alambda, double *d_gG,
                                         double *d_gC, void *stream);
gbdpcg_status gbdpcg_kkt_backward_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_Ginv,
                                      const float *d_C, const float *d_gz, const float *d_nglam, const float *d_S,
                                      const float *d_Pinv, float *d_gamma, const float *d_z, const float *d_lambda, float *d_az,
                                      float *d_alambda, float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                      uint8_t *d_max_iter_exit, float *d_gG, float *d_gC, void *stream);
gbdpcg_status gbdpcg_kkt_backward_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_Ginv,
                                      const double *d_C, const double *d_gz, const double *d_nglam, const double *d_S,
                                      const double *d_Pinv, double *d_gamma, const double *d_z, const double *d_lambda, double *d_az,
                                      double *d_alambda, double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                      uint8_t *d_max_iter_exit, double *d_gG, double *d_gC, void *stream);
gbdpcg_status gbdpcg_kkt_backward_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const float *d_Ginv, const float *d_C, const float *d_gz, const float *d_nglam,
                                             const float *d_S, const float *d_Pinv, float *d_gamma, const float *d_z,
                                             const float *d_lambda, float *d_az, float *d_alambda, float *d_r, float *d_p,
                                             float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                             float *d_gG, float *d_gC, void *stream);
gbdpcg_status gbdpcg_kkt_backward_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const double *d_Ginv, const double *d_C, const double *d_gz, const double *d_nglam,
                                             const double *d_S, const double *d_Pinv, double *d_gamma, const double *d_z,
                                             const double *d_lambda, double *d_az, double *d_alambda, double *d_r, double *d_p,
                                             double tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                             double *d_gG, double *d_gC, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_backward_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                   const float *d_Ginv, const float *d_C, const float *d_gz, const float *d_nglam,
                                                   const float *d_S, const float *d_Pinv, float *d_gamma, const float *d_z,
                                                   const float *d_lambda, float *d_az, float *d_alambda, float *d_r, float *d_p,
                                                   float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                   float *d_gG, float *d_gC, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_backward_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                   const double *d_Ginv, const double *d_C, const double *d_gz,
                                                   const double *d_nglam, const double *d_S, const double *d_Pinv, double *d_gamma,
                                                   const double *d_z, const double *d_lambda, double *d_az, double *d_alambda,
                                                   double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                   uint8_t *d_max_iter_exit, double *d_gG, double *d_gC, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_backward_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                          const float *d_Ginv, const float *d_C, const float *d_gz,
                                                          const float *d_nglam, const float *d_S, const float *d_Pinv,
                                                          float *d_gamma, const float *d_z, const float *d_lambda, float *d_az,
                                                          float *d_alambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                                          uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_gG, float *d_gC,
                                                          gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_kkt_backward_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                          const double *d_Ginv, const double *d_C, const double *d_gz,
                                                          const double *d_nglam, const double *d_S, const double *d_Pinv,
                                                          double *d_gamma, const double *d_z, const double *d_lambda, double *d_az,
                                                          double *d_alambda, double *d_r, double *d_p, double tol,
                                                          uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                          double *d_gG, double *d_gC, gbdpcg_graph_t *out);

/* The backward pass of the hard box QP: gradients of a scalar through (G, C, g, c, lo, hi) -> (w, lambda) of the box section
 * (gbdpcg_admm_step_* run to convergence), on the device.  At a solution with the active set A (the entries held at a bound) the
 * adjoint pair (a_z, a_lambda) and a multiplier nu supported on A solve
 *     G a_z + gz + C' a_lambda + nu = 0,      C a_z = -glam,      (a_z)_A = 0              gz = dl/dz, glam = dl/dlambda
 * These are the optimality conditions of ANOTHER box QP with the same G and C: g := gz, c := -glam (the convention of
 * gbdpcg_kkt_backward_*: d_nglam holds MINUS dl/dlambda), and the degenerate box lo = hi = 0 on A, (-Inf, +Inf) elsewhere.  So the
 * adjoint is the ADMM iteration of the box section on the S, Phi^-1, G^-1 of G + rho I the forward pass kept, one
 * gbdpcg_kkt_resolve_* per adjoint iteration, and it is as converged as its loop is run.
 * The mask.  The forward pass leaves A defined to the bit: behind any hard update d_y (here d_yf, read only) is exactly 0 where
 * nothing was clipped, < 0 where w = lo and > 0 where w = hi.  Entry i is active iff yf_i != 0 -- no threshold, nothing to tune; a
 * NaN yf_i counts as active.  An entry that sits on its bound with yf_i = 0 (weakly active: the bound holds without force) counts
 * as FREE: the gradient is the one-sided derivative on the side where the bound stays inactive.  d_yf stands where d_lo, d_hi
 * stand in the box family; no adjoint bound arrays exist.  Per element of problem b, with m = (yf != 0):
 *     v   = fl(az + ya)
 *     wa+ = m ? (v < 0 ? 0 : (v > 0 ? 0 : v)) : v                             a NaN v stays NaN, v = -0 stays -0
 *     ya+ = fl(v - wa+)
 *     gta+ = fma(-rho_b, fl(wa+ - ya+), gz)                                   one rounding
 *     d_res[2b] = max_i |fl(az_i - wa+_i)|,   d_res[2b+1] = max_i |fl(rho_b fl(wa+_i - wa_i))|
 * d_wa, d_ya, d_gta and d_res are THE BITS of gbdpcg_admm_update_* / gbdpcg_admm_init_* called with the explicit box lo = hi = +0
 * where m and -Inf / +Inf elsewhere, signed zeros and NaN included.
 *  - gbdpcg_admm_adjoint_init_*: wa <- m ? clip(wa, 0, 0) : wa, ya is left as it is, gta <- fma(-rho_b, fl(wa - ya), gz).  Start from
 *    wa = ya = 0 (gta = gz), or warm from the adjoint state of the previous backward pass.
 *  - gbdpcg_admm_adjoint_update_*: everything behind the adjoint solve that wrote d_az, one launch.
 *  - gbdpcg_admm_adjoint_step_*: gbdpcg_kkt_resolve_* with g := d_gta, c := d_nglam (writing d_alambda, warm-started from it, and
 *    d_az) followed by gbdpcg_admm_adjoint_update_* on the same stream; same results as the two calls, bit for bit.
 *  - the graph constructor keeps the POINTER d_rho like the one of gbdpcg_admm_step_* and sets *out to NULL before its first refusal.
 *  - gbdpcg_admm_grad_bounds_*: from the converged adjoint y (nu = rho ya), one multiplication and one negation per element,
 *        glo_i = yf_i < 0 ? -fl(rho_b ya_i) : +0            ghi_i = yf_i > 0 ? -fl(rho_b ya_i) : +0
 * The gradients: dl/dg = a_z, reported as d_wa (EXACTLY zero on A: dl/dg_i = 0 for a clamped entry); dl/dc = -a_lambda; dl/dG and
 * dl/dC are gbdpcg_kkt_grad_* on (w, lambda, wa, alambda); dl/dlo = d_glo, dl/dhi = d_ghi; dl/drho = 0 (the solution does not depend
 * on rho).
 * NOT provided: _shared twins, cone rows (linear rows: gbdpcg_admm_lin_adjoint_* below; the soft box: gbdpcg_admm_soft_mask_* below), and the backward pass of a forward loop that has not
 * converged (the mask is then whatever d_y holds and the result is the gradient of no particular function).
 * Null handle or required pointer, nx, nu, N or batch == 0: GBDPCG_ERR_INVALID, nothing is written (d_r, d_p, d_max_iter_exit and
 * d_Pinv may be NULL as in gbdpcg_kkt_resolve_*, d_C when N == 1).  init, update and grad_bounds are elementwise and refuse no
 * shape; step inherits every refusal of gbdpcg_kkt_resolve_* and refuses before anything is written. */
gbdpcg_status gbdpcg_admm_adjoint_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_gz,
                                           const float *d_yf, const float *d_rho, float *d_wa, float *d_ya, float *d_gta,
                                           void *stream);
gbdpcg_status gbdpcg_admm_adjoint_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                           const double *d_gz, const double *d_yf, const double *d_rho, double *d_wa, double *d_ya,
                                           double *d_gta, void *stream);
gbdpcg_status gbdpcg_admm_adjoint_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const float *d_gz, const float *d_yf, const float *d_rho, const float *d_az,
                                             float *d_wa, float *d_ya, float *d_gta, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_adjoint_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const double *d_gz, const double *d_yf, const double *d_rho, const double *d_az,
                                             double *d_wa, double *d_ya, double *d_gta, double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_adjoint_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                           const float *d_Ginv, const float *d_C, const float *d_gz, const float *d_nglam,
                                           const float *d_yf, const float *d_rho, const float *d_S, const float *d_Pinv,
                                           float *d_gamma, float *d_alambda, float *d_r, float *d_p, float tol, uint32_t max_iter,
                                           uint32_t *d_iters, uint8_t *d_max_iter_exit, float *d_az, float *d_wa, float *d_ya,
                                           float *d_gta, float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_adjoint_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                           const double *d_Ginv, const double *d_C, const double *d_gz, const double *d_nglam,
                                           const double *d_yf, const double *d_rho, const double *d_S, const double *d_Pinv,
                                           double *d_gamma, double *d_alambda, double *d_r, double *d_p, double tol,
                                           uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_az,
                                           double *d_wa, double *d_ya, double *d_gta, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_adjoint_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                        const float *d_Ginv, const float *d_C, const float *d_gz,
                                                        const float *d_nglam, const float *d_yf, const float *d_rho,
                                                        const float *d_S, const float *d_Pinv, float *d_gamma, float *d_alambda,
                                                        float *d_r, float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                        uint8_t *d_max_iter_exit, float *d_az, float *d_wa, float *d_ya,
                                                        float *d_gta, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_adjoint_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                        const double *d_Ginv, const double *d_C, const double *d_gz,
                                                        const double *d_nglam, const double *d_yf, const double *d_rho,
                                                        const double *d_S, const double *d_Pinv, double *d_gamma,
                                                        double *d_alambda, double *d_r, double *d_p, double tol, uint32_t max_iter,
                                                        uint32_t *d_iters, uint8_t *d_max_iter_exit, double *d_az, double *d_wa,
                                                        double *d_ya, double *d_gta, double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_grad_bounds_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_yf,
                                          const float *d_rho, const float *d_ya, float *d_glo, float *d_ghi, void *stream);
gbdpcg_status gbdpcg_admm_grad_bounds_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const double *d_yf, const double *d_rho, const double *d_ya, double *d_glo, double *d_ghi,
                                          void *stream);

/* The backward pass of the hard linear-row QP: gradients of a scalar through (G, C, g, c, E, lo, hi) -> (z, lambda) of the rows
 * section (gbdpcg_admm_lin_step_* run to convergence), on the device.  At the solution G z + g + C' lambda + rho E' yf = 0, where yf
 * is the forward d_y (the multiplier of the rows is mu = rho yf).  Row r is ACTIVE iff yf_r != 0: yf_r < 0 where (E z)_r sits at
 * lo_r, yf_r > 0 where it sits at hi_r -- no threshold; a NaN yf_r counts as active; a row that sits on a bound with yf_r = 0
 * (weakly active) counts as FREE.  With A the active rows the adjoint triple (a_z, a_lambda, nu) solves
 *     G a_z + gz + C' a_lambda + E_A' nu = 0,      C a_z = -glam,      (E a_z)_A = 0         gz = dl/dz, glam = dl/dlambda
 * the optimality conditions of the SAME rows QP with g := gz, c := -glam (d_nglam holds MINUS dl/dlambda) and the degenerate rows
 * lo = hi = 0 on A, (-Inf, +Inf) elsewhere: the kept S, Phi^-1, G^-1 of Gt = G + rho E'E serve it unchanged, one gbdpcg_kkt_resolve_*
 * per adjoint iteration.  The calls take the arguments of the gbdpcg_admm_lin_* family with d_yf where d_lo, d_hi stand, d_gz where
 * d_g and d_nglam where d_c stand; d_wa, d_ya (layout of the rows), d_gta, d_az (layout of g) are the adjoint's splitting state.
 * Per row the update reads wa, ya, yf (3 arrays, the family's update reads 4) and its projection is
 *     wa+ = yf_r != 0 ? clip(s, +0, +0) : s              s = fl(v + ya), v the chain of E(r, .) az as in gbdpcg_admm_lin_update_*
 * every other line is that of gbdpcg_admm_lin_update_* / _init_*: d_wa, d_ya, d_gta, d_res are THE BITS of those calls on the explicit
 * rows lo = hi = +0 where yf != 0 and -Inf / +Inf elsewhere, signed zeros and NaN included.  From ya = 0 an inactive row's ya stays
 * exactly 0.
 *  - gbdpcg_admm_lin_adjoint_init_*: wa <- yf != 0 ? clip(wa, 0, 0) : wa, ya left alone, gta <- gz - rho E'(wa - ya) by the family's chain.
 *  - gbdpcg_admm_lin_adjoint_update_*: everything behind the adjoint solve that wrote d_az, one launch.
 *  - gbdpcg_admm_lin_adjoint_step_*: gbdpcg_kkt_resolve_* with g := d_gta, c := d_nglam (writing d_alambda, warm-started from it, and
 *    d_az) followed by the update on the same stream; the results of the two calls, bit for bit.
 *  - the graph constructor keeps the POINTER d_rho and sets *out to NULL before its first refusal.
 *  - gbdpcg_admm_lin_grad_*: from the forward d_z, d_yf and the converged adjoint d_az, d_ya (nu = rho ya), one launch; d_glo, d_ghi
 *    in the layout of the rows, d_gE in the layout of d_E; each may be NULL (not written), not all three:
 *        glo_r = yf_r < 0 ? -fl(rho_b ya_r) : +0        ghi_r = yf_r > 0 ? -fl(rho_b ya_r) : +0
 *        gE(r, j) = yf_r != 0 ? fl(rho_b fma(yf_r, az_j, fl(ya_r z_j))) : +0                  j over the columns of the row's block
 *    glo, ghi are the bits of gbdpcg_admm_grad_bounds_* called with (mx, mu, N) in the place of (nx, nu, N).
 * The gradients: dl/dg = d_az (the adjoint's z); dl/dc = -d_alambda; dl/dlo, dl/dhi, dl/dE from gbdpcg_admm_lin_grad_*; dl/dG and
 * dl/dC are gbdpcg_kkt_grad_* on (z, lambda, az, alambda) -- the gradient in G, not in Gt: nothing flows into E through rho E'E, and
 * dl/drho = 0, because the solution does not depend on rho.
 * NOT provided: _shared twins (and a gE summed over the batch for a shared E), cone rows (soft rows: gbdpcg_admm_lin_soft_mask_*
 * below), and the backward pass of a
 * forward loop that has not converged (the mask is then whatever d_y holds).
 * Refusals, before anything is written: those of the gbdpcg_admm_lin_* family.  Null handle or required pointer, nx, nu, N or batch
 * == 0, no rows at all: GBDPCG_ERR_INVALID; mx or mu > 64, a knot that does not fit the LDS: GBDPCG_ERR_UNSUPPORTED; a batch of
 * more than 2^31 - 1 problems: an error of the launch.  step inherits every refusal of gbdpcg_kkt_resolve_* (d_r, d_p,
 * d_max_iter_exit and d_Pinv may be NULL as there, d_C when N == 1). */
gbdpcg_status gbdpcg_admm_lin_adjoint_init_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                               uint32_t batch, const float *d_gz, const float *d_E, const float *d_yf,
                                               const float *d_rho, float *d_wa, float *d_ya, float *d_gta, void *stream);
gbdpcg_status gbdpcg_admm_lin_adjoint_init_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                               uint32_t batch, const double *d_gz, const double *d_E, const double *d_yf,
                                               const double *d_rho, double *d_wa, double *d_ya, double *d_gta, void *stream);
gbdpcg_status gbdpcg_admm_lin_adjoint_update_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                 uint32_t batch, const float *d_gz, const float *d_E, const float *d_yf,
                                                 const float *d_rho, const float *d_az, float *d_wa, float *d_ya, float *d_gta,
                                                 float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_adjoint_update_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                 uint32_t batch, const double *d_gz, const double *d_E, const double *d_yf,
                                                 const double *d_rho, const double *d_az, double *d_wa, double *d_ya, double *d_gta,
                                                 double *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_adjoint_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                               uint32_t batch, const float *d_Ginv, const float *d_C, const float *d_gz,
                                               const float *d_nglam, const float *d_E, const float *d_yf, const float *d_rho,
                                               const float *d_S, const float *d_Pinv, float *d_gamma, float *d_alambda, float *d_r,
                                               float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                               uint8_t *d_max_iter_exit, float *d_az, float *d_wa, float *d_ya, float *d_gta,
                                               float *d_res, void *stream);
gbdpcg_status gbdpcg_admm_lin_adjoint_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                               uint32_t batch, const double *d_Ginv, const double *d_C, const double *d_gz,
                                               const double *d_nglam, const double *d_E, const double *d_yf, const double *d_rho,
                                               const double *d_S, const double *d_Pinv, double *d_gamma, double *d_alambda,
                                               double *d_r, double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                               uint8_t *d_max_iter_exit, double *d_az, double *d_wa, double *d_ya, double *d_gta,
                                               double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_admm_lin_adjoint_step_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                            uint32_t N, uint32_t batch, const float *d_Ginv, const float *d_C,
                                                            const float *d_gz, const float *d_nglam, const float *d_E,
                                                            const float *d_yf, const float *d_rho, const float *d_S,
                                                            const float *d_Pinv, float *d_gamma, float *d_alambda, float *d_r,
                                                            float *d_p, float tol, uint32_t max_iter, uint32_t *d_iters,
                                                            uint8_t *d_max_iter_exit, float *d_az, float *d_wa, float *d_ya,
                                                            float *d_gta, float *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_graph_create_admm_lin_adjoint_step_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu,
                                                            uint32_t N, uint32_t batch, const double *d_Ginv, const double *d_C,
                                                            const double *d_gz, const double *d_nglam, const double *d_E,
                                                            const double *d_yf, const double *d_rho, const double *d_S,
                                                            const double *d_Pinv, double *d_gamma, double *d_alambda, double *d_r,
                                                            double *d_p, double tol, uint32_t max_iter, uint32_t *d_iters,
                                                            uint8_t *d_max_iter_exit, double *d_az, double *d_wa, double *d_ya,
                                                            double *d_gta, double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_admm_lin_grad_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const float *d_z, const float *d_az, const float *d_yf, const float *d_ya,
                                       const float *d_rho, float *d_glo, float *d_ghi, float *d_gE, void *stream);
gbdpcg_status gbdpcg_admm_lin_grad_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                       uint32_t batch, const double *d_z, const double *d_az, const double *d_yf,
                                       const double *d_ya, const double *d_rho, double *d_glo, double *d_ghi, double *d_gE,
                                       void *stream);

/* The backward pass of the SOFT box and rows QPs (gbdpcg_admm_soft_step_*, gbdpcg_admm_lin_soft_step_* run to convergence):
 * gradients of a scalar through (G, C, g, c, [E,] lo, hi, kappa) -> (w or z, lambda), on the device.  Behind a soft update the
 * forward d_y (here d_yf, read only) splits the rows of problem b into three sets, to the bit and with no threshold; theta_r =
 * fl(kappa_r / rho_b) is the one correctly rounded division of the update:
 *     free        yf_r == 0                          inside its bounds, mu_r = 0
 *     held        yf_r != 0 and |yf_r| < theta_r     on a bound with |mu_r| < kappa_r       (a NaN yf_r fails the comparison: held)
 *     saturated   |yf_r| >= theta_r                  beyond its bound, mu_r = +-kappa_r: the update wrote +-theta_r itself
 * A row whose excess ties with theta_r takes the third branch of the update with y = +-theta_r and counts as saturated.  The
 * multiplier of a saturated row is a constant, so in the adjoint problem the row is as free as an inactive one: the adjoint is the
 * HARD adjoint loop (gbdpcg_admm_adjoint_* / gbdpcg_admm_lin_adjoint_* above) on a MASKED copy of d_yf, and no soft adjoint update
 * exists.  A saturated row contributes through kappa and E instead:
 *     dl/dkappa_r = sign(yf_r) (E a_z)_r  on saturated rows, 0 elsewhere        dl/dE(r, j) keeps rho yf_r a_z,j on them
 *  - gbdpcg_admm_soft_mask_* (nz elements per problem, the layout of g) and gbdpcg_admm_lin_soft_mask_* (the layout of the rows):
 *        ym_r = |yf_r| >= theta_r ? +0 : yf_r
 *    kappa = +Inf gives d_ym the bits of d_yf, kappa = 0 gives +0 everywhere.  d_ym == d_yf is GBDPCG_ERR_INVALID whatever else the
 *    call would answer: the unmasked d_yf is needed by the gradient launch.  d_rho MUST be the rho of the update that wrote d_yf:
 *    take the mask directly behind an update (or a step), never behind a rebalance with no update after it, which rescales y away
 *    from +-theta.
 *  - gbdpcg_admm_soft_grad_bounds_*: from d_yf, d_kappa and the converged adjoint d_ya, d_az (the loop run on d_ym), with
 *    sat = |yf| >= theta, one launch, each output may be NULL (not written), not all three:
 *        glo_i = (yf_i < 0 && !sat) ? -fl(rho_b ya_i) : +0        ghi_i = (yf_i > 0 && !sat) ? -fl(rho_b ya_i) : +0
 *        gkappa_i = sat ? (yf_i > 0 ? az_i : -az_i) : +0
 *    glo, ghi are the bits of gbdpcg_admm_grad_bounds_* called with d_ym.
 *  - gbdpcg_admm_lin_soft_grad_*: the rows' launch with kappa, each output may be NULL, not all four:
 *        glo_r, ghi_r   the lines above over the rows
 *        gE(r, j)       the line of gbdpcg_admm_lin_grad_* with the UNMASKED yf: its bits on (z, az, yf, ya)
 *        gkappa_r = sat ? (yf_r > 0 ? v : -v) : +0,   v = the chain fma(E(r, j), az_j, acc) over the block's columns, ascending j, seed +0
 * Every line is one IEEE operation or a comparison: the outputs are defined to the bit whatever the alignment of the pointers.
 * The gradients: dl/dg, dl/dc, dl/dG, dl/dC as in the hard sections (gbdpcg_kkt_grad_* on the forward pair and the adjoint pair);
 * dl/dlo, dl/dhi, dl/dkappa[, dl/dE] from the launches here; dl/drho = 0.  Where kappa = +Inf dl/dkappa is exactly +0 and every
 * other gradient has the bits of the hard calls.
 * NOT provided: _shared twins, cone rows, the backward pass of a forward loop that has not converged, and gradients behind a
 * rebalance with no update after it.
 * Refusals, before anything is written: null handle or required pointer (every input; at least one output), nx, nu, N or batch
 * == 0, d_ym == d_yf, no rows at all: GBDPCG_ERR_INVALID; the rows calls: mx or mu > 64, a knot that does not fit the LDS:
 * GBDPCG_ERR_UNSUPPORTED; a batch of more than 2^31 - 1 problems: an error of the launch. */
gbdpcg_status gbdpcg_admm_soft_mask_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_yf,
                                        const float *d_kappa, const float *d_rho, float *d_ym, void *stream);
gbdpcg_status gbdpcg_admm_soft_mask_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_yf,
                                        const double *d_kappa, const double *d_rho, double *d_ym, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_mask_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const float *d_yf, const float *d_kappa, const float *d_rho, float *d_ym,
                                            void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_mask_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const double *d_yf, const double *d_kappa, const double *d_rho,
                                            double *d_ym, void *stream);
gbdpcg_status gbdpcg_admm_soft_grad_bounds_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const float *d_yf, const float *d_kappa, const float *d_rho, const float *d_ya,
                                               const float *d_az, float *d_glo, float *d_ghi, float *d_gkappa, void *stream);
gbdpcg_status gbdpcg_admm_soft_grad_bounds_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                               const double *d_yf, const double *d_kappa, const double *d_rho, const double *d_ya,
                                               const double *d_az, double *d_glo, double *d_ghi, double *d_gkappa, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_grad_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const float *d_z, const float *d_az, const float *d_E, const float *d_yf,
                                            const float *d_ya, const float *d_kappa, const float *d_rho, float *d_glo, float *d_ghi,
                                            float *d_gkappa, float *d_gE, void *stream);
gbdpcg_status gbdpcg_admm_lin_soft_grad_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                            uint32_t batch, const double *d_z, const double *d_az, const double *d_E,
                                            const double *d_yf, const double *d_ya, const double *d_kappa, const double *d_rho,
                                            double *d_glo, double *d_ghi, double *d_gkappa, double *d_gE, void *stream);

/* The primal infeasibility certificate of the HARD ADMM paths (gbdpcg_admm_step_*, gbdpcg_admm_lin_step_*), on the device.  A hard
 * iteration cannot tell an infeasible problem from a slow one: d_res[2b] stalls at the gap and y grows.  Problem b, min 1/2 z'Gz +
 * g'z subject to Cz = c and lo <= E z <= hi, is infeasible iff some (dl, dm) satisfies (Farkas)
 *     C'dl + E'dm = 0        and        c'dl + sum_r (dm_r > 0 ? hi_r dm_r : lo_r dm_r) < 0
 * Every z-step of the splitting satisfies Gt z + gt + C'lambda = 0, so on an infeasible problem, where z and w settle and E z - w
 * tends to the constant gap, the differences of two iterates dl = lambda1 - lambda0, dm = rho (y1 - y0) tend to such a pair.  The
 * two iterates may be any number of steps apart: a wider window scales the pair and does not change the test.  The caller copies
 * d_lambda and d_y aside with its own copy nodes (d_lambda0, d_y0), runs one or more steps, and hands both pairs to one launch,
 * which answers per problem how close the differences are to a certificate.  (G + rho E'E is factored, so positive definite: the
 * cost is never unbounded and there is no dual certificate to look for.)
 * d_C, d_c, d_E, d_lo, d_hi, d_rho and the layouts of d_lambda*, d_y* are those of the gbdpcg_admm_lin_* family; the box calls
 * (gbdpcg_admm_infeas_*) have no mx, mu, d_E, and d_lo, d_hi, d_y0, d_y1 have the layout of d_g.  d_C may be NULL when N == 1.
 * _shared: d_C and d_E are ONE problem's, as in gbdpcg_admm_lin_step_shared_*, read with a zero problem stride; everything else
 * stays per problem.
 * Per problem b, every line ONE IEEE operation or a comparison, a chain being acc = fma(a_i, b_i, acc) in ascending i:
 *     dl = fl(lambda1 - lambda0),   dy = fl(y1 - y0),   m_r = fl(rho_b dy_r)
 *     x-part of knot k, entry r:   s = dl_k[r];   s = fma(A_k(q,r), -dl_{k+1}[q], s), q < nx ascending (absent at the last knot)
 *     u-part of knot k, entry r:   s = +0;        s = fma(B_k(q,r), -dl_{k+1}[q], s), q < nx ascending
 *                                  (the signs and the order of the C' terms of gbdpcg_kkt_residual_*)
 *     u = chain over the rows i of Ex_k (Eu_k) of fma(E(i,r), dy_i, acc), seed +0;        q = fma(rho_b, u, s)
 *     d_cert[3b]   = n = max(max |dl|, max_r |m_r|)        the scale
 *     d_cert[3b+1] = r = max_j |q_j|                       the residual of the certificate
 *                    (both maxima over bit patterns as in gbdpcg_kkt_residual_*: NaN on top, exact in any order)
 *     t_k:  acc = +0;  over the knot's rows in storage order (x rows, then u rows):  dy_r > 0: acc = fma(hi_r, m_r, acc);
 *           dy_r < 0: acc = fma(lo_r, m_r, acc);  otherwise nothing -- a zero or NaN dy_r never multiplies an infinite bound;
 *           then acc = fma(c_k[i], dl_k[i], acc) for i < nx ascending
 *     d_cert[3b+2] = sigma:  acc = +0;  acc = fl(acc + t_k) for k ascending       the support value (the two levels are part of
 *                    the definition)
 *     d_flag[b] = (n > 0 && r <= fl(eps n) && sigma < -fl(eps n)) ? 1 : 0         a NaN anywhere gives 0
 * so the outputs are defined to the bit whatever the launch shape or the alignment of the pointers.  d_cert (3 batch elements of
 * the call's precision) and d_flag (batch bytes; may be NULL: not written) are overwritten whatever they held.  The box calls
 * take the single line u = fma(1, dy_r, +0) for the chain: THE BITS of the rows call with E = I, mx = nx, mu = nu on finite data,
 * signed zeros included.  (A NaN or Inf dy_r stays in its own entry of q there; through the zero entries of an explicit I it
 * reaches every entry of its block.)
 * eps is the caller's: r / n falls and sigma / n settles at minus the gap over the scale.  On the pinned infeasible fixture
 * (tests/admm_infeas_ref.py) eps = 0.1 flags every problem within 6 iterations in both precisions and never flags a feasible
 * one, close to convergence included (there n falls to rounding noise, r with it, and r / n stays of order 1).
 * One launch each, no handle state, asynchronous on `stream`, capturable inside a caller-owned capture; never allocates and needs
 * nothing from gbdpcg_reserve.  d_lo, d_hi, d_rho and eps are not validated: bad values stay inside their own problem.
 * NOT provided: cone rows (their certificate needs the dual cone); the soft families (always feasible in their soft rows); a
 * device-side count over the batch; any change to the step graphs -- the copies of lambda and y are the caller's.
 * Refusals, before anything is written: null handle or required pointer, nx, nu, N or batch == 0, no rows at all,
 * d_lambda0 == d_lambda1, d_y0 == d_y1: GBDPCG_ERR_INVALID; mx or mu > 64, a knot ([A_k | B_k], its E blocks and vectors) that
 * does not fit the LDS: GBDPCG_ERR_UNSUPPORTED; a batch of more than 2^31 - 1 problems: an error of the launch. */
gbdpcg_status gbdpcg_admm_infeas_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_C,
                                     const float *d_c, const float *d_lo, const float *d_hi, const float *d_rho,
                                     const float *d_lambda0, const float *d_lambda1, const float *d_y0, const float *d_y1, float eps,
                                     float *d_cert, uint8_t *d_flag, void *stream);
gbdpcg_status gbdpcg_admm_infeas_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_C,
                                     const double *d_c, const double *d_lo, const double *d_hi, const double *d_rho,
                                     const double *d_lambda0, const double *d_lambda1, const double *d_y0, const double *d_y1,
                                     double eps, double *d_cert, uint8_t *d_flag, void *stream);
gbdpcg_status gbdpcg_admm_infeas_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_C,
                                            const float *d_c, const float *d_lo, const float *d_hi, const float *d_rho,
                                            const float *d_lambda0, const float *d_lambda1, const float *d_y0, const float *d_y1,
                                            float eps, float *d_cert, uint8_t *d_flag, void *stream);
gbdpcg_status gbdpcg_admm_infeas_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                            const double *d_C, const double *d_c, const double *d_lo, const double *d_hi,
                                            const double *d_rho, const double *d_lambda0, const double *d_lambda1, const double *d_y0,
                                            const double *d_y1, double eps, double *d_cert, uint8_t *d_flag, void *stream);
gbdpcg_status gbdpcg_admm_lin_infeas_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                         uint32_t batch, const float *d_C, const float *d_c, const float *d_E, const float *d_lo,
                                         const float *d_hi, const float *d_rho, const float *d_lambda0, const float *d_lambda1,
                                         const float *d_y0, const float *d_y1, float eps, float *d_cert, uint8_t *d_flag, void *stream);
gbdpcg_status gbdpcg_admm_lin_infeas_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                         uint32_t batch, const double *d_C, const double *d_c, const double *d_E, const double *d_lo,
                                         const double *d_hi, const double *d_rho, const double *d_lambda0, const double *d_lambda1,
                                         const double *d_y0, const double *d_y1, double eps, double *d_cert, uint8_t *d_flag,
                                         void *stream);
gbdpcg_status gbdpcg_admm_lin_infeas_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                uint32_t batch, const float *d_C, const float *d_c, const float *d_E,
                                                const float *d_lo, const float *d_hi, const float *d_rho, const float *d_lambda0,
                                                const float *d_lambda1, const float *d_y0, const float *d_y1, float eps,
                                                float *d_cert, uint8_t *d_flag, void *stream);
gbdpcg_status gbdpcg_admm_lin_infeas_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                uint32_t batch, const double *d_C, const double *d_c, const double *d_E,
                                                const double *d_lo, const double *d_hi, const double *d_rho, const double *d_lambda0,
                                                const double *d_lambda1, const double *d_y0, const double *d_y1, double eps,
                                                double *d_cert, uint8_t *d_flag, void *stream);

/* The optimality test of the ADMM families, on the device: is (z, lambda, rho y) a solution of problem b,
 *     min 1/2 z'Gz + g'z   subject to   Cz = c   and   E z in the rows' set (the box: E = I)?
 * d_res of the updates cannot say: d_res[2b+1] = rho ||E'(w+ - w)|| is the stationarity residual only if the z-step solved
 * Gt z + gt + C'lambda = 0 EXACTLY, and a warm-started PCG with a small max_iter does not -- its error, and ||Cz - c||, show up
 * nowhere in d_res; and d_res is absolute, with no scale to build a relative test from.  Every update of every family (box, soft
 * box, linear rows, soft rows, cones) writes w+ = P(s), y+ = s - w+ with P the projection (prox) of its set, so w lies in the set
 * and rho y in the normal cone at w BY CONSTRUCTION: bounds, complementarity and the signs of the multipliers need no test, and
 * this call reads no bound and no kappa -- one pair of entry points serves all five families.  Three conditions remain, each
 * with the scale of the usual test r <= eps_abs + eps_rel * scale:
 *     stationarity  G z + g + C'lambda + rho E'y = 0,      dynamics  C z = c,      consensus  E z = w.
 * d_G holds the HESSIANS (not d_Ginv; for the rows families not d_Gt); every layout is that of gbdpcg_kkt_residual_* (d_G, d_C,
 * d_g, d_c, d_z, d_lambda) and of gbdpcg_admm_lin_update_* (d_E, d_rho, d_w, d_y); the box calls (gbdpcg_admm_optimality_*) have no
 * mx, mu, d_E, and d_w, d_y have the layout of d_g.  d_C may be NULL when N == 1.  _shared: d_G, d_C and d_E are ONE problem's,
 * read with a zero problem stride; everything else stays per problem.
 * Per problem b, rho = d_rho[b], every line ONE IEEE operation or a comparison, a chain being acc = fma(a_i, b_i, acc) in
 * ascending i:
 *     x-entry r of knot k:  s = fl(g + lambda_k[r]);  s = fma(Q_k(r,q), x_q, s), q < nx;  if k + 1 < N: s = fma(A_k(q,r),
 *                           -lambda_{k+1}[q], s), q < nx                                (the chain of gbdpcg_kkt_residual_*)
 *                           a = the same Q chain from +0;      t = lambda_k[r], then the same A' chain
 *     u-entry r of knot k:  the same with R_k, B_k and the seeds s = g, a = +0, t = +0   (the last knot has no C' terms and no u)
 *     u = chain over the rows i of Ex_k (Eu_k) of fma(E(i,r), y_i, acc), seed +0;      q = fma(rho, u, s);    p = fma(rho, u, t)
 *     knot 0, entry r:      f = fl(x_0[r] - c_0[r]);   h = x_0[r]
 *     knot k+1, entry r:    f = fl(x_{k+1}[r] - c_{k+1}[r]);  f = fma(A_k(r,q), -x_q, f), q < nx;  f = fma(B_k(r,q), -u_q, f), q < nu
 *                           h = the same chain seeded x_{k+1}[r]
 *     row r:                v_r = chain over the columns j of fma(E(r,j), z_j, acc), seed +0 (the update's);  d_r = fl(v_r - w_r)
 *     d_opt[6b+0] = r_s = max |q|        d_opt[6b+3] = n_s = max(max |a|, max |p|, max |g|)
 *     d_opt[6b+1] = r_e = max |f|        d_opt[6b+4] = n_e = max(max |h|, max |c|)
 *     d_opt[6b+2] = r_r = max |d|        d_opt[6b+5] = n_r = max(max |v|, max |w|)
 *                   (all maxima over bit patterns as in gbdpcg_kkt_residual_*: NaN on top, exact in any order)
 *     d_done[b] = (r_s <= fma(eps_rel, n_s, eps_abs) && r_e <= fma(eps_rel, n_e, eps_abs) && r_r <= fma(eps_rel, n_r, eps_abs))
 *                 ? 1 : 0                                                                     a NaN anywhere gives 0
 * so the outputs are defined to the bit whatever the launch shape or the alignment of the pointers.  d_opt (6 batch elements of
 * the call's precision) and d_done (batch bytes; may be NULL: not written) are overwritten whatever they held.  The box calls
 * take u = fma(1, y_r, +0) and v_r = z_r.  What follows from the lines:
 *   - with y = 0, r_s and r_e have THE BITS of gbdpcg_kkt_residual_* on (G, C, g, c, z, lambda);
 *   - called directly behind an update or step of ANY family, r_r has the bits of that update's d_res[2b] (soft and hard, box
 *     and rows; cone rows through the rows call, with zero offsets f -- the call knows of no offset);
 *   - on finite data the box calls give the bits of the rows calls with E = I, mx = nx, mu = nu;
 *   - _shared gives each problem the bits of the per-problem call on `batch` copies.
 * eps_abs, eps_rel are the caller's.  tests/admm_optimality_ref.py pins, on a feasible fixture, the window of iterations in which
 * the device's first d_done must fall.
 * One launch each, no handle state, asynchronous on `stream`, capturable inside a caller-owned capture; never allocates and needs
 * nothing from gbdpcg_reserve.  d_rho, eps_abs, eps_rel and the data are not validated: bad values stay inside their own problem.
 * NOT provided: a device-side count over the batch; any change to the step graphs (put the call behind the replay); a
 * dual-infeasibility test (Gt is factored, hence positive definite: the cost is never unbounded; primal infeasibility is
 * gbdpcg_admm_infeas_*).
 * Refusals, before anything is written: null handle or required pointer, nx, nu, N or batch == 0, rows forms with no row at all:
 * GBDPCG_ERR_INVALID; mx or mu > 64, a knot (Q_k, R_k, [A_k | B_k], its E blocks and vectors) that does not fit the LDS:
 * GBDPCG_ERR_UNSUPPORTED; a batch of more than 2^31 - 1 problems: an error of the launch. */
gbdpcg_status gbdpcg_admm_optimality_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_G,
                                         const float *d_C, const float *d_g, const float *d_c, const float *d_rho, const float *d_z,
                                         const float *d_lambda, const float *d_w, const float *d_y, float eps_abs, float eps_rel,
                                         float *d_opt, uint8_t *d_done, void *stream);
gbdpcg_status gbdpcg_admm_optimality_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                         const double *d_C, const double *d_g, const double *d_c, const double *d_rho,
                                         const double *d_z, const double *d_lambda, const double *d_w, const double *d_y,
                                         double eps_abs, double eps_rel, double *d_opt, uint8_t *d_done, void *stream);
gbdpcg_status gbdpcg_admm_optimality_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                                const float *d_rho, const float *d_z, const float *d_lambda, const float *d_w,
                                                const float *d_y, float eps_abs, float eps_rel, float *d_opt, uint8_t *d_done,
                                                void *stream);
gbdpcg_status gbdpcg_admm_optimality_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                                const double *d_rho, const double *d_z, const double *d_lambda, const double *d_w,
                                                const double *d_y, double eps_abs, double eps_rel, double *d_opt, uint8_t *d_done,
                                                void *stream);
gbdpcg_status gbdpcg_admm_lin_optimality_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                             uint32_t batch, const float *d_G, const float *d_C, const float *d_g, const float *d_c,
                                             const float *d_E, const float *d_rho, const float *d_z, const float *d_lambda,
                                             const float *d_w, const float *d_y, float eps_abs, float eps_rel, float *d_opt,
                                             uint8_t *d_done, void *stream);
gbdpcg_status gbdpcg_admm_lin_optimality_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                             uint32_t batch, const double *d_G, const double *d_C, const double *d_g,
                                             const double *d_c, const double *d_E, const double *d_rho, const double *d_z,
                                             const double *d_lambda, const double *d_w, const double *d_y, double eps_abs,
                                             double eps_rel, double *d_opt, uint8_t *d_done, void *stream);
gbdpcg_status gbdpcg_admm_lin_optimality_shared_f32(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                    uint32_t batch, const float *d_G, const float *d_C, const float *d_g,
                                                    const float *d_c, const float *d_E, const float *d_rho, const float *d_z,
                                                    const float *d_lambda, const float *d_w, const float *d_y, float eps_abs,
                                                    float eps_rel, float *d_opt, uint8_t *d_done, void *stream);
gbdpcg_status gbdpcg_admm_lin_optimality_shared_f64(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,
                                                    uint32_t batch, const double *d_G, const double *d_C, const double *d_g,
                                                    const double *d_c, const double *d_E, const double *d_rho, const double *d_z,
                                                    const double *d_lambda, const double *d_w, const double *d_y, double eps_abs,
                                                    double eps_rel, double *d_opt, uint8_t *d_done, void *stream);

/* Mixed-precision refinement of a KKT point: fp32 solves on a kept fp32 factorisation, the defect and the point in fp64.
 * For a caller who needs more digits in the step than fp32 carries (SQP close to convergence, an adjoint solve, ADMM on a
 * kept factorisation) without the price of the fp64 pipeline: factor once in fp32 (gbdpcg_demote_f32 of G and C, then
 * gbdpcg_kkt_step_f32, or gbdpcg_form_schur_f32 + gbdpcg_form_pinv_f32), then per step evaluate the defect of the current
 * fp64 point in fp64, solve for the correction with gbdpcg_kkt_resolve_f32, accumulate in fp64.  Conventions and layouts are
 * those of f4 above; the fp64 operands are d_G, d_C, d_g, d_c, d_z, d_lambda.
 *
 * gbdpcg_kkt_defect_mixed, per problem b (one launch):
 *     r_s = G z + g + C' lambda  (layout of d_g),   r_f = C z - c  (layout of d_c)
 *         every entry the fp64 fma chain of gbdpcg_kkt_residual_f64, in its order of terms
 *     m_s = max |r_s|,  m_f = max |r_f|     over bit patterns, NaN-propagating, as in gbdpcg_kkt_residual_*
 *     e_b = 0 where m = max(m_s, m_f) is 0, Inf or NaN; otherwise -ilogb(m) clamped to [-126, 127]  (m 2^e in [1, 2) unclamped)
 *     d_rg[i]      = fl32(r_s[i]) * 2^e_b       fp32: ONE rounding to fp32, then a product by the power of two in fp32, which is
 *     d_rc[i]      = fl32(-r_f[i]) * 2^e_b      exact unless it is subnormal or overflows
 *     d_dlambda[i] = 0                          fp32, nx N per problem, where the pointer is not NULL: the cold start of the
 *                                               correction solve, written in the same pass
 *     d_expo[b]    = e_b                        int32_t
 *     d_res[2b] = m_s, d_res[2b+1] = m_f        fp64: bit for bit what gbdpcg_kkt_residual_f64 writes for the same point
 * d_rg and d_rc are the g and the c of the correction system G dz + C' dlambda = -r_s, C dz = -r_f, scaled.
 * WHY THE SCALING: the exit test of gbdpcg_solve_* is ABSOLUTE (|eta| < tol).  From the second refinement step on the defect is
 * 1e-6 and smaller; an unscaled correction solve would leave after zero iterations and the refinement would stall at fp32
 * accuracy.  The exact power of two per problem makes every correction solve see a right-hand side whose max-norm is in [1, 2)
 * -- `tol` below applies to THAT system -- and costs no rounding.
 * Every output is overwritten whatever it held and depends on nothing it held; a problem with a NaN or an Inf in its defect gets
 * e_b = 0 and that norm, the other problems of the batch are unaffected.
 *
 * gbdpcg_kkt_refine_apply (one launch):  z[i] = z[i] + ldexp((double)dz[i], -e_b), lambda likewise from d_dlambda.  Widening
 * and scaling are exact, so each element is ONE IEEE addition; the bits do not depend on the alignment of the pointers.
 *
 * gbdpcg_demote_f32:  d_dst[i] = fl32(d_src[i]), round to nearest, i < count: the fp32 G and C the factorisation is formed from.
 *
 * gbdpcg_kkt_refine_step: the defect launch, gbdpcg_kkt_resolve_f32 with g := d_rg, c := d_rc from the zeroed d_dlambda on the
 * kept d_Ginv32, d_C32, d_S32, d_Pinv32 (correction d_dz, d_dlambda), the apply launch: bit-identical with those three calls.
 * d_res holds the norms of the point the step STARTED from.  gbdpcg_graph_create_kkt_refine_step takes the same arguments and
 * reserves like the other graph constructors: replay it K times from z = lambda = 0 for a whole solve, or after rewriting g, c
 * in place for the next tick of a kept linearisation.  d_rg, d_rc, d_gamma, d_dlambda, d_r, d_p, d_dz are fp32 work arrays
 * (layouts of g, c, c, c, c, c, g); d_Pinv32, d_r, d_p, d_max_iter_exit may be NULL as in gbdpcg_kkt_resolve_f32.
 *
 * All of them: asynchronous on `stream`, capturable, no allocation beyond what gbdpcg_reserve (or the graph constructor) sizes
 * for the fp32 solve.  Null handle or required pointer, nx, nu, N, batch or count == 0: GBDPCG_ERR_INVALID; a shape
 * gbdpcg_form_schur_* refuses (in either precision): GBDPCG_ERR_UNSUPPORTED; nothing is written in either case.  d_C and d_C32
 * may be NULL when N == 1.
 *
 * Regularised and shared-matrix forms.  Conventions, outputs, exponent rule and refusals are those above unless said here.
 * gbdpcg_kkt_defect_mixed_reg: the defect of the REGULARISED system, r_s = (G_b + rho_b I) z + g + C' lambda.  d_rho: [batch]
 *   fp64 on the device, directly behind d_c, required.  Every diagonal entry d of every Q_k and R_k enters its chain as
 *   fl(d + rho_b), ONE fp64 rounding, as gbdpcg_kkt_residual_reg_f64 takes it; the chains and r_f are unchanged.  d_G is
 *   untouched, no second buffer, no extra launch.  d_res is bit for bit what gbdpcg_kkt_residual_reg_f64 writes for the same
 *   point; with every rho_b == 0 every output has the bits of gbdpcg_kkt_defect_mixed.  rho is not validated: a NaN in rho_b
 *   costs problem b only (e_b = 0, NaN norm).
 * gbdpcg_kkt_refine_step_reg, gbdpcg_graph_create_kkt_refine_step_reg: the step with that defect.  The kept factorisation is
 *   what gbdpcg_kkt_step_reg_f32 (or gbdpcg_form_schur_reg_f32 + gbdpcg_form_pinv_f32) wrote from the demoted G and C with rho
 *   demoted by gbdpcg_demote_f32.  The refinement then converges to the solution of the fp64 system with G + rho I: the case of
 *   every ADMM z-update, of a damped SQP step, and of a cost that is only positive semi-definite, which has no plain
 *   factorisation at all.  The graph keeps the POINTER d_rho, as gbdpcg_graph_create_kkt_step_reg_* does: rewrite rho in place
 *   between replays (the kept fp32 factorisation should then be formed again, or the refinement slows down).
 * gbdpcg_kkt_defect_mixed_shared: d_G and d_C are ONE problem's blocks, read by every problem of the batch; exactly one
 *   problem's worth is read behind each.  g, c, z, lambda and every output stay per problem.  Problem b gets the bits of
 *   gbdpcg_kkt_defect_mixed on `batch` copies of the matrices; d_res is bit for bit gbdpcg_kkt_residual_shared_f64.
 * gbdpcg_kkt_refine_step_shared, gbdpcg_graph_create_kkt_refine_step_shared: d_G, d_C, d_Ginv32, d_C32, d_S32, d_Pinv32 are one
 *   problem's each; the correction solve is gbdpcg_kkt_resolve_shared_f32 and its rules hold as stated there (fused family only,
 *   one verdict for the one pair in symmetric mode 2, GBDPCG_ERR_UNSUPPORTED for a shape beyond one workgroup).  Problem b gets
 *   the bits of gbdpcg_kkt_refine_step on `batch` copies of the matrices, on the same handle with the path set to
 *   GBDPCG_PATH_FUSED.
 * Each step is bit-identical with its three calls (defect, gbdpcg_kkt_resolve[_shared]_f32, gbdpcg_kkt_refine_apply).
 * d_rho == NULL: GBDPCG_ERR_INVALID; every other refusal is that of the function extended; nothing is written on refusal.
 * Not provided: _shared and _reg TOGETHER.  A shared batch has one G, so rho could only be one number: the caller writes
 *   G + rho I into that one G (gbdpcg_admm_lin_form_f64 with E = I, batch 1, d_Gt == d_G allowed) and uses the _shared forms,
 *   as for gbdpcg_kkt_residual_shared_*.  Refinement behind the gbdpcg_admm_*_step_* entry points themselves is not provided
 *   either: an ADMM loop in mixed precision replays the refine_step_reg graph with g := the shifted gradient and calls
 *   gbdpcg_admm_update_f64 (examples/refine_box_mpc_loop.cpp).
 * A factorisation of G + rho I from gbdpcg_kkt_step_reg_f32 may still be passed as the kept one of the PLAIN step: the plain
 * defect does not contain rho, so the refinement then converges, more slowly, to the solution of the UNREGULARISED fp64 system. */
gbdpcg_status gbdpcg_demote_f32(gbdpcg_handle_t h, uint64_t count, const double *d_src, float *d_dst, void *stream);
gbdpcg_status gbdpcg_kkt_defect_mixed(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                      const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                      const double *d_z, const double *d_lambda, float *d_rg, float *d_rc, float *d_dlambda,
                                      int32_t *d_expo, double *d_res, void *stream);
gbdpcg_status gbdpcg_kkt_refine_apply(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                      const float *d_dz, const float *d_dlambda, const int32_t *d_expo, double *d_z,
                                      double *d_lambda, void *stream);
gbdpcg_status gbdpcg_kkt_refine_step(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                     const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                     const float *d_Ginv32, const float *d_C32, const float *d_S32, const float *d_Pinv32,
                                     float *d_rg, float *d_rc, float *d_gamma, float *d_dlambda, float *d_r, float *d_p,
                                     float *d_dz, float tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                     int32_t *d_expo, double *d_z, double *d_lambda, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_refine_step(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                  const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                                  const float *d_Ginv32, const float *d_C32, const float *d_S32,
                                                  const float *d_Pinv32, float *d_rg, float *d_rc, float *d_gamma,
                                                  float *d_dlambda, float *d_r, float *d_p, float *d_dz, float tol,
                                                  uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,
                                                  int32_t *d_expo, double *d_z, double *d_lambda, double *d_res,
                                                  gbdpcg_graph_t *out);

gbdpcg_status gbdpcg_kkt_defect_mixed_reg(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                          const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                          const double *d_rho, const double *d_z, const double *d_lambda, float *d_rg,
                                          float *d_rc, float *d_dlambda, int32_t *d_expo, double *d_res, void *stream);
gbdpcg_status gbdpcg_kkt_defect_mixed_shared(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                             const double *d_z, const double *d_lambda, float *d_rg, float *d_rc,
                                             float *d_dlambda, int32_t *d_expo, double *d_res, void *stream);
gbdpcg_status gbdpcg_kkt_refine_step_reg(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                         const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                         const double *d_rho, const float *d_Ginv32, const float *d_C32, const float *d_S32,
                                         const float *d_Pinv32, float *d_rg, float *d_rc, float *d_gamma, float *d_dlambda,
                                         float *d_r, float *d_p, float *d_dz, float tol, uint32_t max_iter, uint32_t *d_iters,
                                         uint8_t *d_max_iter_exit, int32_t *d_expo, double *d_z, double *d_lambda,
                                         double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_refine_step_reg(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                                      const double *d_G, const double *d_C, const double *d_g,
                                                      const double *d_c, const double *d_rho, const float *d_Ginv32,
                                                      const float *d_C32, const float *d_S32, const float *d_Pinv32,
                                                      float *d_rg, float *d_rc, float *d_gamma, float *d_dlambda, float *d_r,
                                                      float *d_p, float *d_dz, float tol, uint32_t max_iter,
                                                      uint32_t *d_iters, uint8_t *d_max_iter_exit, int32_t *d_expo,
                                                      double *d_z, double *d_lambda, double *d_res, gbdpcg_graph_t *out);
gbdpcg_status gbdpcg_kkt_refine_step_shared(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                            const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                            const float *d_Ginv32, const float *d_C32, const float *d_S32,
                                            const float *d_Pinv32, float *d_rg, float *d_rc, float *d_gamma, float *d_dlambda,
                                            float *d_r, float *d_p, float *d_dz, float tol, uint32_t max_iter,
                                            uint32_t *d_iters, uint8_t *d_max_iter_exit, int32_t *d_expo, double *d_z,
                                            double *d_lambda, double *d_res, void *stream);
gbdpcg_status gbdpcg_graph_create_kkt_refine_step_shared(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N,
                                                         uint32_t batch, const double *d_G, const double *d_C,
                                                         const double *d_g, const double *d_c, const float *d_Ginv32,
                                                         const float *d_C32, const float *d_S32, const float *d_Pinv32,
                                                         float *d_rg, float *d_rc, float *d_gamma, float *d_dlambda,
                                                         float *d_r, float *d_p, float *d_dz, float tol, uint32_t max_iter,
                                                         uint32_t *d_iters, uint8_t *d_max_iter_exit, int32_t *d_expo,
                                                         double *d_z, double *d_lambda, double *d_res, gbdpcg_graph_t *out);

/* CSR ingestion (f3): repacks a host CSR matrix (csr_t<T>, include/types.cuh:7-15) whose
 * sparsity lies inside the block-tridiagonal pattern into the [L|D|R] layout (host arrays).
 * Entries outside the pattern give GBDPCG_ERR_INVALID.  Implements what the stub overload
 * at include/interface.cuh:8-20 announces. */
gbdpcg_status gbdpcg_csr_to_bt_f32(uint32_t n, uint32_t N, const uint32_t *row_ptr,
                                   const uint32_t *col_ind, const float *val, float *h_M);
gbdpcg_status gbdpcg_csr_to_bt_f64(uint32_t n, uint32_t N, const uint32_t *row_ptr,
                                   const uint32_t *col_ind, const double *val, double *h_M);

/* Library / build identification ("gbdpcg <version> gfx950"). */
const char *gbdpcg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GBDPCG_H */
