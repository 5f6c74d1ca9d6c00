// Soft (L1-penalised) state bounds on a kept linearisation (include/gbdpcg.h, "Soft (L1-penalised) bounds"): the loop of
// box_mpc_loop.cpp after a disturbance has pushed the initial state outside a state bound.  The first state of knot 0 is pinned by
// c (x_0 = c_0) and its upper bound lies GAP below that value, so NO point satisfies Cz = c and the box: the hard loop
// (gbdpcg_admm_step_*) never terminates here -- max ||z - w||_inf stalls at GAP and y grows at every replay.  The soft family pays
// kappa dist(x, [lo, hi]) on the states instead (finite KAPPA) and keeps the inputs hard (kappa = +Inf):
//
//   once          : gbdpcg_kkt_step_reg_f32 -- S, Phi^-1 and G^-1 of G + rho I; the bounds of box_mpc_loop.cpp on the inputs, every
//                   first state below its unconstrained maximum, and the bound on x_0 that c contradicts
//                   gbdpcg_admm_soft_init_f32 with w = y = 0
//                   ONE executable graph of { gamma ; PCG ; z ; the soft splitting update }
//   per iteration : replay the graph; every CHECK replays read the residuals back and stop when both are below TOL
// At the end the inputs lie in their box exactly, the state bounds are violated by what the dynamics force, and the multiplier
// mu = rho y of every soft row is at most its kappa.  Choice of kappa: above the multiplier a hard bound would carry (read rho |y|
// from a feasible run) the soft problem IS the hard one; below it the bound gives way.
// usage: soft_box_mpc_loop [batch=1024] [knotPoints=128] [max_replays=400]      (stateSize 14, controlSize 7, fp32)
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
constexpr int CHECK = 10;
constexpr float TOL = 1e-3f, RHO = 2.0f, GAP = 0.5f, KAPPA = 20.0f;

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
        fprintf(stderr, "usage: soft_box_mpc_loop [batch] [knotPoints >= 2] [max_replays]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N;

    // a few distinct problems, repeated over the batch (host generation only)
    const uint32_t distinct = batch < 8 ? batch : 8;
    std::vector<float> hG(szG * batch), hC(szC * batch), hg(szg * batch), hc(szc * batch), hrho(batch, RHO);
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

    float *dG, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dz, *dlo, *dhi, *dkap, *dw, *dy, *dgt, *dres;
    uint32_t *d_iters;
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
    for (float **p : {&dz, &dlo, &dhi, &dkap, &dw, &dy, &dgt}) CK(hipMalloc((void **)p, szg * batch * 4));
    CK(hipMalloc((void **)&dres, 2 * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
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
    // the states: the first state of every knot below its largest unconstrained value, and at knot 0 -- where c pins it -- GAP below
    // the pinned value: the disturbance.  Finite kappa on the states, +Inf on the inputs.
    std::vector<float> hkap(szg * batch, std::numeric_limits<float>::infinity());
    for (uint32_t b = 0; b < batch; ++b) {
        float xmax = 0.f;
        for (uint32_t k = 1; k < N; ++k) xmax = std::max(xmax, std::fabs(hz[b * szg + (size_t)k * sv]));
        for (uint32_t k = 0; k < N; ++k) {
            hhi[b * szg + (size_t)k * sv] = k == 0 ? hc[b * szc] - GAP : 0.5f * xmax;
            for (uint32_t i = 0; i < nx; ++i) hkap[b * szg + (size_t)k * sv + i] = KAPPA;
        }
    }
    CK(hipMemcpy(dlo, hlo.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhi, hhi.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dkap, hkap.data(), szg * batch * 4, hipMemcpyHostToDevice));
    printf("%u problems, %u knots: %zu inputs of the unconstrained solutions lie outside their bounds; x_0 is pinned %.2f above its bound\n",
           batch, N, outside, GAP);

    GK(gbdpcg_admm_soft_init_f32(h, nx, nu, N, batch, dg, dlo, dhi, dkap, drho, dw, dy, dgt, stream));
    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    gbdpcg_graph_t graph;
    GK(gbdpcg_graph_create_admm_soft_step_f32(h, nx, nu, N, batch, dGi, dC, dg, dc, dlo, dhi, dkap, drho, dS, dP, dgam, dl, nullptr, nullptr,
                                              pcg_tol, pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, &graph));
    std::vector<float> hres(2 * batch);
    bool converged = false;
    int replays = 0;
    const auto t0 = std::chrono::steady_clock::now();
    while (replays < max_replays && !converged) {
        for (int i = 0; i < CHECK && replays < max_replays; ++i, ++replays) GK(gbdpcg_graph_launch(graph, stream));
        CK(hipMemcpyAsync(hres.data(), dres, 2 * batch * 4, hipMemcpyDeviceToHost, stream));
        CK(hipStreamSynchronize(stream));
        float prim = 0.f, dual = 0.f;
        bool finite = true;   // (a NaN in a problem is that problem's norm: the device does not drop it, neither does this loop)
        for (uint32_t b = 0; b < batch; ++b) {
            finite = finite && std::isfinite(hres[2 * b]) && std::isfinite(hres[2 * b + 1]);
            prim = std::fmax(prim, hres[2 * b]);
            dual = std::fmax(dual, hres[2 * b + 1]);
        }
        printf("replay %4d: max ||z - w||_inf %.3e, max rho ||w+ - w||_inf %.3e%s\n", replays, prim, dual, finite ? "" : " (not finite)");
        if (!finite) break;
        converged = prim < TOL && dual < TOL;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%d replays in %.3f ms (%.3f ms each, residual read-back every %d included)\n", replays, ms, ms / replays, CHECK);

    // the hard rows (the inputs) lie in the box exactly; the soft rows give way where the dynamics force them to, and their
    // multiplier rho |y| never exceeds kappa
    std::vector<float> hw(szg * batch), hy(szg * batch);
    CK(hipMemcpy(hw.data(), dw, szg * batch * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hy.data(), dy, szg * batch * 4, hipMemcpyDeviceToHost));
    size_t violations = 0, soft_out = 0, over = 0;
    float worst = 0.f;
    for (size_t e = 0; e < hw.size(); ++e) {
        const bool in = hw[e] >= hlo[e] && hw[e] <= hhi[e];
        if (std::isinf(hkap[e])) {
            violations += !in;
        } else {
            soft_out += !in;
            worst = std::fmax(worst, std::fmax(hw[e] - hhi[e], hlo[e] - hw[e]));
            over += !(std::fabs(hy[e]) <= hkap[e] / RHO);
        }
    }
    const bool bad = !converged || violations != 0 || over != 0 || soft_out < batch || !(worst >= 0.99f * GAP);
    printf("hard rows outside the box: %zu; soft rows outside their bounds: %zu (worst by %.3f, the gap is %.2f); multipliers above "
           "kappa: %zu; %s\n", violations, soft_out, worst, GAP, over, converged ? "converged" : "NOT converged");

    gbdpcg_graph_destroy(graph);
    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)drho, (void *)dS, (void *)dgam, (void *)dGi, (void *)dP, (void *)dl,
                    (void *)dz, (void *)dlo, (void *)dhi, (void *)dkap, (void *)dw, (void *)dy, (void *)dgt, (void *)dres, (void *)d_iters, (void *)d_flags})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
