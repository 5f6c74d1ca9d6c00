// Adaptive rho on top of box_mpc_loop.cpp: the same box-constrained batch, started from a penalty that is WRONG per problem (64 times
// too large for the even problems, 16 times too small for the odd ones), and brought back by residual balancing on the device
// (include/gbdpcg.h, "Adaptive rho for the three ADMM families").
//
//   once          : gbdpcg_kkt_step_reg_f32 on G + rho I with the starting rho, gbdpcg_admm_init_f32 with w = y = 0,
//                   the STEP graph    { gamma ; PCG on the kept S, Phi^-1 ; z ; the splitting update }
//                   the RESTEP graph  { rebalance: rho, y, gt, expo ; S, gamma, G^-1 of G + rho I ; Phi^-1 ; PCG ; z ; the update }
//   per period    : replay the step graph PERIOD times, the restep graph once, read the 2 batch residuals back and stop when
//                   max_b ||z - w||_inf and max_b rho ||w+ - w||_inf are both below TOL
// Nothing else changes for the caller: no host decision, no rewrite of rho, y or gt.  Every restep refactors EVERY problem, whether
// its rho moved or not: it costs a whole gbdpcg_kkt_step_reg where a step costs a gbdpcg_kkt_resolve, hence once per period.
// usage: adaptive_box_mpc_loop [batch=1024] [knotPoints=128] [max_replays=400]      (stateSize 14, controlSize 7, fp32)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
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
constexpr int PERIOD = 5;   // plain steps per restep
constexpr float TOL = 1e-3f, RHO = 2.0f;
// the rule: move rho by 2 when one residual is more than 10 times the other, inside [RHO / 1024, RHO * 1024]
constexpr float RATIO = 10.0f, RHO_MIN = RHO / 1024.0f, RHO_MAX = RHO * 1024.0f;
constexpr uint32_t SHIFT = 1;

// M M' / m + I, column-major m x m
void spd(uint64_t &seed, uint32_t m, float *out)
{
    std::vector<double> a(m * m);
    for (auto &v : a) v = 1.7 * urand(seed);
    for (uint32_t c = 0; c < m; ++c)
        for (uint32_t r = 0; r < m; ++r) {
            double s = r == c ? 1.0 : 0.0;
            for (uint32_t q = 0; q < m; ++q) s += a[q * m + r] * a[q * m + c] / m;
            out[c * m + r] = (float)s;
        }
}
}  // namespace

int main(int argc, char **argv)
{
    const uint32_t batch = argc > 1 ? (uint32_t)atoi(argv[1]) : 1024, N = argc > 2 ? (uint32_t)atoi(argv[2]) : 128;
    const int max_replays = argc > 3 ? atoi(argv[3]) : 400;
    if (batch == 0 || N < 2 || max_replays < 1) {
        fprintf(stderr, "usage: adaptive_box_mpc_loop [batch] [knotPoints >= 2] [max_replays]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N;

    // a few distinct problems, repeated over the batch (host generation only)
    const uint32_t distinct = batch < 8 ? batch : 8;
    std::vector<float> hG(szG * batch), hC(szC * batch), hg(szg * batch), hc(szc * batch), hrho(batch);
    for (uint32_t b = 0; b < batch; ++b) hrho[b] = b % 2 ? RHO / 16.0f : RHO * 64.0f;   // a deliberately bad start
    uint64_t seed = 4321;
    for (uint32_t b = 0; b < distinct; ++b) {
        float *G = hG.data() + b * szG, *C = hC.data() + b * szC;
        for (uint32_t k = 0; k < N; ++k) {
            spd(seed, nx, G + (size_t)k * sg);
            if (k + 1 < N) {
                spd(seed, nu, G + (size_t)k * sg + nx * nx);
                float *A = C + (size_t)k * sc, *B = A + nx * nx;
                for (uint32_t i = 0; i < nx * nx; ++i) A[i] = (float)(0.5 * urand(seed) / std::sqrt((double)nx)) + (i / nx == i % nx ? 1.f : 0.f);
                for (uint32_t i = 0; i < nx * nu; ++i) B[i] = (float)(1.7 * urand(seed) / std::sqrt((double)nx));
            }
        }
        for (size_t i = 0; i < szg; ++i) hg[b * szg + i] = 1.7f * (float)urand(seed);
        for (size_t i = 0; i < szc; ++i) hc[b * szc + i] = 0.17f * (float)urand(seed);
    }
    for (uint32_t b = distinct; b < batch; ++b) {
        const uint32_t s = b % distinct;
        std::copy(hG.begin() + s * szG, hG.begin() + (s + 1) * szG, hG.begin() + b * szG);
        std::copy(hC.begin() + s * szC, hC.begin() + (s + 1) * szC, hC.begin() + b * szC);
        std::copy(hg.begin() + s * szg, hg.begin() + (s + 1) * szg, hg.begin() + b * szg);
        std::copy(hc.begin() + s * szc, hc.begin() + (s + 1) * szc, hc.begin() + b * szc);
    }

    float *dG, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dz, *dlo, *dhi, *dw, *dy, *dgt, *dres;
    uint32_t *d_iters;
    int32_t *d_expo;
    uint8_t *d_flags;
    CK(hipMalloc((void **)&dG, szG * batch * 4));
    CK(hipMalloc((void **)&dC, szC * batch * 4));
    CK(hipMalloc((void **)&dg, szg * batch * 4));
    CK(hipMalloc((void **)&dc, szc * batch * 4));
    CK(hipMalloc((void **)&drho, batch * 4));
    CK(hipMalloc((void **)&dS, szS * batch * 4));
    CK(hipMalloc((void **)&dgam, szc * batch * 4));
    CK(hipMalloc((void **)&dGi, szG * batch * 4));
    CK(hipMalloc((void **)&dP, szS * batch * 4));
    CK(hipMalloc((void **)&dl, szc * batch * 4));
    for (float **p : {&dz, &dlo, &dhi, &dw, &dy, &dgt}) CK(hipMalloc((void **)p, szg * batch * 4));
    CK(hipMalloc((void **)&dres, 2 * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMalloc((void **)&d_expo, batch * 4));
    CK(hipMemcpy(dG, hG.data(), szG * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dg, hg.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), szc * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(drho, hrho.data(), batch * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dl, 0, szc * batch * 4));
    CK(hipMemset(dw, 0, szg * batch * 4));
    CK(hipMemset(dy, 0, szg * batch * 4));
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    gbdpcg_handle_t h;
    GK(gbdpcg_create(&h, 0));

    // the factorisation of G + rho I, once; its z is the solution without the box (of the regularised problem)
    const float pcg_tol = 1e-10f;
    const uint32_t pcg_max_iter = 200;
    GK(gbdpcg_kkt_step_reg_f32(h, nx, nu, N, batch, dG, dC, dg, dc, drho, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, dl, nullptr, nullptr,
                               pcg_tol, pcg_max_iter, d_iters, d_flags, dz, stream));
    CK(hipStreamSynchronize(stream));
    std::vector<float> hz(szg * batch), hlo(szg * batch, -std::numeric_limits<float>::infinity()),
        hhi(szg * batch, std::numeric_limits<float>::infinity());
    CK(hipMemcpy(hz.data(), dz, szg * batch * 4, hipMemcpyDeviceToHost));
    size_t outside = 0;
    for (uint32_t b = 0; b < batch; ++b) {
        float umax = 0.f;
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) umax = std::max(umax, std::fabs(hz[b * szg + (size_t)k * sv + nx + i]));
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) {
                const size_t e = b * szg + (size_t)k * sv + nx + i;
                hlo[e] = -0.5f * umax;
                hhi[e] = 0.5f * umax;
                outside += std::fabs(hz[e]) > 0.5f * umax;
            }
    }
    CK(hipMemcpy(dlo, hlo.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhi, hhi.data(), szg * batch * 4, hipMemcpyHostToDevice));
    printf("%u problems, %u knots: %zu inputs of the unconstrained solutions lie outside their bounds\n", batch, N, outside);

    GK(gbdpcg_admm_init_f32(h, nx, nu, N, batch, dg, dlo, dhi, drho, dw, dy, dgt, stream));
    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    gbdpcg_graph_t graph;
    GK(gbdpcg_graph_create_admm_step_f32(h, nx, nu, N, batch, dGi, dC, dg, dc, dlo, dhi, drho, dS, dP, dgam, dl, nullptr, nullptr, pcg_tol,
                                         pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, &graph));
    // the same iteration with a new rho: it writes dGi, dS, dP and drho, which the step graph reads through the same pointers
    gbdpcg_graph_t regraph;
    GK(gbdpcg_graph_create_admm_restep_f32(h, nx, nu, N, batch, dG, dGi, dC, dg, dc, dlo, dhi, drho, dS, dP, GBDPCG_PINV_STAIR, dgam, dl,
                                           nullptr, nullptr, pcg_tol, pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, RATIO, SHIFT,
                                           RHO_MIN, RHO_MAX, d_expo, &regraph));
    std::vector<float> hres(2 * batch);
    std::vector<int32_t> hexpo(batch);
    bool converged = false;
    int replays = 0;
    const auto t0 = std::chrono::steady_clock::now();
    while (replays < max_replays && !converged) {
        for (int i = 0; i < PERIOD && replays < max_replays; ++i, ++replays) GK(gbdpcg_graph_launch(graph, stream));
        if (replays < max_replays) {
            GK(gbdpcg_graph_launch(regraph, stream));
            ++replays;
        }
        CK(hipMemcpyAsync(hres.data(), dres, 2 * batch * 4, hipMemcpyDeviceToHost, stream));
        CK(hipMemcpyAsync(hexpo.data(), d_expo, batch * 4, hipMemcpyDeviceToHost, stream));   // (only to print it)
        CK(hipStreamSynchronize(stream));
        uint32_t raised = 0, lowered = 0;
        for (uint32_t b = 0; b < batch; ++b) raised += hexpo[b] > 0, lowered += hexpo[b] < 0;
        float prim = 0.f, dual = 0.f;
        bool finite = true;   // (a NaN in a problem is that problem's norm: the device does not drop it, neither does this loop)
        for (uint32_t b = 0; b < batch; ++b) {
            finite = finite && std::isfinite(hres[2 * b]) && std::isfinite(hres[2 * b + 1]);
            prim = std::fmax(prim, hres[2 * b]);
            dual = std::fmax(dual, hres[2 * b + 1]);
        }
        printf("replay %4d: max ||z - w||_inf %.3e, max rho ||w+ - w||_inf %.3e, rho raised in %u, lowered in %u problems%s\n", replays,
               prim, dual, raised, lowered, finite ? "" : " (not finite)");
        if (!finite) break;
        converged = prim < TOL && dual < TOL;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%d replays in %.3f ms (%.3f ms each, one in %d a restep, residual read-back every %d included)\n", replays, ms, ms / replays,
           PERIOD + 1, PERIOD + 1);

    // w lies in the box exactly
    std::vector<float> hw(szg * batch);
    CK(hipMemcpy(hw.data(), dw, szg * batch * 4, hipMemcpyDeviceToHost));
    size_t violations = 0;
    for (size_t e = 0; e < hw.size(); ++e) violations += !(hw[e] >= hlo[e] && hw[e] <= hhi[e]);
    const bool bad = !converged || violations != 0 || outside == 0;
    printf("w outside the box in %zu entries; %s\n", violations, converged ? "converged" : "NOT converged");

    gbdpcg_graph_destroy(graph);
    gbdpcg_graph_destroy(regraph);
    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)drho, (void *)dS, (void *)dgam, (void *)dGi, (void *)dP, (void *)dl,
                    (void *)dz, (void *)dlo, (void *)dhi, (void *)dw, (void *)dy, (void *)dgt, (void *)dres, (void *)d_iters, (void *)d_flags,
                    (void *)d_expo})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
