// box_mpc_loop.cpp in mixed precision: box constraints lo <= z <= hi by ADMM in fp64, whose z-update is the REGULARISED refinement step
// on a kept fp32 factorisation (include/gbdpcg.h, "Regularised and shared-matrix forms" of the mixed-precision refinement).
//
//   once          : gbdpcg_demote_f32 of G, C, g, c, rho; gbdpcg_kkt_step_reg_f32 -- S, Phi^-1 and G^-1 of fl32(G) + fl32(rho) I, kept
//                   K0 replays of the refine_step_reg graph on the original g from z = lambda = 0: the fp64 solution WITHOUT the box,
//                   from which this example takes its bounds (inputs within half of the largest unconstrained input, states free)
//                   gbdpcg_admm_init_f64 with w = y = 0: writes the shifted gradient gt
//                   ONE executable graph of { fp64 defect of (G + rho I, gt) at (z, lambda) ; gamma ; PCG ; dz ; fp64 accumulation }
//   per iteration : K replays of that graph from the PREVIOUS (z, lambda) -- the warm start is free -- with g := gt, the fp64 shifted
//                   gradient gbdpcg_admm_update_f64 wrote; then gbdpcg_admm_update_f64.  Every CHECK iterations the ADMM norms and
//                   the _reg defect norms (of the point the last replay started from) are read back and printed.
// usage: refine_box_mpc_loop [batch=1024] [knotPoints=128] [max_iterations=400] [K=2]      (stateSize 14, controlSize 7)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "gbdpcg.h"
#include "synth_problem.hpp"

#define CK(x)                                                                                   \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)
#define GK(x)                                                                                        \
    do {                                                                                             \
        gbdpcg_status s_ = (x);                                                                      \
        if (s_ != GBDPCG_OK) {                                                                       \
            fprintf(stderr, "gbdpcg error %s at %s:%d\n", gbdpcg_status_string(s_), __FILE__, __LINE__); \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

namespace {
constexpr uint32_t nx = n, nu = 7;
constexpr uint32_t sg = nx * nx + nu * nu, sc = nx * nx + nx * nu, sv = nx + nu;
constexpr int CHECK = 10, K0 = 6;
constexpr double TOL = 1e-9, RHO = 2.0;   // (fp64 iterates: a tolerance fp32 ADMM cannot reach)

// M M' / m + I, column-major m x m
void spd(uint64_t &seed, uint32_t m, double *out)
{
    std::vector<double> a(m * m);
    for (auto &v : a) v = 1.7 * urand(seed);
    for (uint32_t c = 0; c < m; ++c)
        for (uint32_t r = 0; r < m; ++r) {
            double s = r == c ? 1.0 : 0.0;
            for (uint32_t q = 0; q < m; ++q) s += a[q * m + r] * a[q * m + c] / m;
            out[c * m + r] = s;
        }
}
}  // namespace

int main(int argc, char **argv)
{
    const uint32_t batch = argc > 1 ? (uint32_t)atoi(argv[1]) : 1024, N = argc > 2 ? (uint32_t)atoi(argv[2]) : 128;
    const int max_iterations = argc > 3 ? atoi(argv[3]) : 400, K = argc > 4 ? atoi(argv[4]) : 2;
    if (batch == 0 || N < 2 || max_iterations < 1 || K < 1) {
        fprintf(stderr, "usage: refine_box_mpc_loop [batch] [knotPoints >= 2] [max_iterations] [K >= 1]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N;

    // a few distinct problems, repeated over the batch (host generation only)
    const uint32_t distinct = batch < 8 ? batch : 8;
    std::vector<double> hG(szG * batch), hC(szC * batch), hg(szg * batch), hc(szc * batch), hrho(batch, RHO);
    uint64_t seed = 4321;
    for (uint32_t b = 0; b < distinct; ++b) {
        double *G = hG.data() + b * szG, *C = hC.data() + b * szC;
        for (uint32_t k = 0; k < N; ++k) {
            spd(seed, nx, G + (size_t)k * sg);
            if (k + 1 < N) {
                spd(seed, nu, G + (size_t)k * sg + nx * nx);
                double *A = C + (size_t)k * sc, *B = A + nx * nx;
                for (uint32_t i = 0; i < nx * nx; ++i) A[i] = 0.5 * urand(seed) / std::sqrt((double)nx) + (i / nx == i % nx ? 1.0 : 0.0);
                for (uint32_t i = 0; i < nx * nu; ++i) B[i] = 1.7 * urand(seed) / std::sqrt((double)nx);
            }
        }
        for (size_t i = 0; i < szg; ++i) hg[b * szg + i] = 1.7 * urand(seed);
        for (size_t i = 0; i < szc; ++i) hc[b * szc + i] = 0.17 * urand(seed);
    }
    for (uint32_t b = distinct; b < batch; ++b) {
        const uint32_t s = b % distinct;
        std::copy(hG.begin() + s * szG, hG.begin() + (s + 1) * szG, hG.begin() + b * szG);
        std::copy(hC.begin() + s * szC, hC.begin() + (s + 1) * szC, hC.begin() + b * szC);
        std::copy(hg.begin() + s * szg, hg.begin() + (s + 1) * szg, hg.begin() + b * szg);
        std::copy(hc.begin() + s * szc, hc.begin() + (s + 1) * szc, hc.begin() + b * szc);
    }

    // fp64: the problem, the point, the set and the splitting state; fp32: the kept factorisation and the work arrays of the step
    double *dG, *dC, *dg, *dc, *drho, *dz, *dl, *dlo, *dhi, *dw, *dy, *dgt, *dres, *dnorm;
    float *fG, *fC, *fg, *fc, *frho, *fS, *fgam, *fGi, *fP, *fl, *fz, *frg, *frc, *fdl, *fr, *fp, *fdz;
    uint32_t *d_iters;
    uint8_t *d_flags;
    int32_t *d_expo;
    CK(hipMalloc((void **)&dG, szG * batch * 8));
    CK(hipMalloc((void **)&dC, szC * batch * 8));
    CK(hipMalloc((void **)&dc, szc * batch * 8));
    CK(hipMalloc((void **)&dl, szc * batch * 8));
    CK(hipMalloc((void **)&drho, batch * 8));
    for (double **p : {&dg, &dz, &dlo, &dhi, &dw, &dy, &dgt}) CK(hipMalloc((void **)p, szg * batch * 8));
    CK(hipMalloc((void **)&dres, 2 * batch * 8));
    CK(hipMalloc((void **)&dnorm, 2 * batch * 8));
    CK(hipMalloc((void **)&fG, szG * batch * 4));
    CK(hipMalloc((void **)&fGi, szG * batch * 4));
    CK(hipMalloc((void **)&fC, szC * batch * 4));
    CK(hipMalloc((void **)&frho, batch * 4));
    for (float **p : {&fS, &fP}) CK(hipMalloc((void **)p, szS * batch * 4));
    for (float **p : {&fg, &fz, &frg, &fdz}) CK(hipMalloc((void **)p, szg * batch * 4));
    for (float **p : {&fc, &fgam, &fl, &frc, &fdl, &fr, &fp}) CK(hipMalloc((void **)p, szc * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMalloc((void **)&d_expo, batch * 4));
    CK(hipMemcpy(dG, hG.data(), szG * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dg, hg.data(), szg * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), szc * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(drho, hrho.data(), batch * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dz, 0, szg * batch * 8));
    CK(hipMemset(dl, 0, szc * batch * 8));
    CK(hipMemset(dw, 0, szg * batch * 8));
    CK(hipMemset(dy, 0, szg * batch * 8));
    CK(hipMemset(fl, 0, szc * batch * 4));
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    gbdpcg_handle_t h;
    GK(gbdpcg_create(&h, 0));

    // the fp32 factorisation of G + rho I, once
    const float pcg_tol = 1e-8f;   // (on a right-hand side of max-norm in [1, 2))
    const uint32_t pcg_max_iter = 200;
    GK(gbdpcg_demote_f32(h, szG * batch, dG, fG, stream));
    GK(gbdpcg_demote_f32(h, szC * batch, dC, fC, stream));
    GK(gbdpcg_demote_f32(h, szg * batch, dg, fg, stream));
    GK(gbdpcg_demote_f32(h, szc * batch, dc, fc, stream));
    GK(gbdpcg_demote_f32(h, batch, drho, frho, stream));
    GK(gbdpcg_kkt_step_reg_f32(h, nx, nu, N, batch, fG, fC, fg, fc, frho, fS, fgam, fGi, fP, GBDPCG_PINV_STAIR, fl, nullptr, nullptr, pcg_tol,
                               pcg_max_iter, d_iters, d_flags, fz, stream));
    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage

    // the fp64 solution without the box: K0 refinement steps on the original g
    for (int i = 0; i < K0; ++i)
        GK(gbdpcg_kkt_refine_step_reg(h, nx, nu, N, batch, dG, dC, dg, dc, drho, fGi, fC, fS, fP, frg, frc, fgam, fdl, fr, fp, fdz, pcg_tol,
                                      pcg_max_iter, d_iters, d_flags, d_expo, dz, dl, dnorm, stream));
    CK(hipStreamSynchronize(stream));
    std::vector<double> hz(szg * batch), hlo(szg * batch, -std::numeric_limits<double>::infinity()),
        hhi(szg * batch, std::numeric_limits<double>::infinity());
    CK(hipMemcpy(hz.data(), dz, szg * batch * 8, hipMemcpyDeviceToHost));
    size_t outside = 0;
    for (uint32_t b = 0; b < batch; ++b) {
        double umax = 0.0;
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) umax = std::max(umax, std::fabs(hz[b * szg + (size_t)k * sv + nx + i]));
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) {
                const size_t e = b * szg + (size_t)k * sv + nx + i;
                hlo[e] = -0.5 * umax;
                hhi[e] = 0.5 * umax;
                outside += std::fabs(hz[e]) > 0.5 * umax;
            }
    }
    CK(hipMemcpy(dlo, hlo.data(), szg * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhi, hhi.data(), szg * batch * 8, hipMemcpyHostToDevice));
    printf("%u problems, %u knots, K = %d: %zu inputs of the unconstrained solutions lie outside their bounds\n", batch, N, K, outside);

    GK(gbdpcg_admm_init_f64(h, nx, nu, N, batch, dg, dlo, dhi, drho, dw, dy, dgt, stream));
    gbdpcg_graph_t graph;   // g := dgt, which the update rewrites in place between the iterations
    GK(gbdpcg_graph_create_kkt_refine_step_reg(h, nx, nu, N, batch, dG, dC, dgt, dc, drho, fGi, fC, fS, fP, frg, frc, fgam, fdl, fr, fp, fdz,
                                               pcg_tol, pcg_max_iter, d_iters, d_flags, d_expo, dz, dl, dnorm, &graph));
    std::vector<double> hres(2 * batch), hnorm(2 * batch);
    bool converged = false, finite = true;
    int it = 0;
    while (it < max_iterations && !converged && finite) {
        for (int i = 0; i < CHECK && it < max_iterations; ++i, ++it) {
            for (int r = 0; r < K; ++r) GK(gbdpcg_graph_launch(graph, stream));
            GK(gbdpcg_admm_update_f64(h, nx, nu, N, batch, dg, dlo, dhi, drho, dz, dw, dy, dgt, dres, stream));
        }
        CK(hipMemcpyAsync(hres.data(), dres, 2 * batch * 8, hipMemcpyDeviceToHost, stream));
        CK(hipMemcpyAsync(hnorm.data(), dnorm, 2 * batch * 8, hipMemcpyDeviceToHost, stream));
        CK(hipStreamSynchronize(stream));
        double prim = 0.0, dual = 0.0, ms = 0.0, mf = 0.0;
        for (uint32_t b = 0; b < batch; ++b) {   // (a NaN in a problem is that problem's norm: this loop does not drop it either)
            finite = finite && std::isfinite(hres[2 * b]) && std::isfinite(hres[2 * b + 1]) && std::isfinite(hnorm[2 * b]);
            prim = std::fmax(prim, hres[2 * b]);
            dual = std::fmax(dual, hres[2 * b + 1]);
            ms = std::fmax(ms, hnorm[2 * b]);
            mf = std::fmax(mf, hnorm[2 * b + 1]);
        }
        printf("iteration %4d: max ||z - w||_inf %.3e, max rho ||w+ - w||_inf %.3e; z-update defect before its last step: stationarity "
               "%.3e, feasibility %.3e%s\n", it, prim, dual, ms, mf, finite ? "" : " (not finite)");
        converged = prim < TOL && dual < TOL;
    }

    // w lies in the box exactly
    std::vector<double> hw(szg * batch);
    CK(hipMemcpy(hw.data(), dw, szg * batch * 8, hipMemcpyDeviceToHost));
    size_t violations = 0;
    for (size_t e = 0; e < hw.size(); ++e) violations += !(hw[e] >= hlo[e] && hw[e] <= hhi[e]);
    const bool bad = !converged || violations != 0 || outside == 0;
    printf("%d iterations; w outside the box in %zu entries; %s\n", it, violations, converged ? "converged" : "NOT converged");

    gbdpcg_graph_destroy(graph);
    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)drho, (void *)dz, (void *)dl, (void *)dlo, (void *)dhi, (void *)dw,
                    (void *)dy, (void *)dgt, (void *)dres, (void *)dnorm, (void *)fG, (void *)fC, (void *)fg, (void *)fc, (void *)frho,
                    (void *)fS, (void *)fgam, (void *)fGi, (void *)fP, (void *)fl, (void *)fz, (void *)frg, (void *)frc, (void *)fdl,
                    (void *)fr, (void *)fp, (void *)fdz, (void *)d_iters, (void *)d_flags, (void *)d_expo})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
