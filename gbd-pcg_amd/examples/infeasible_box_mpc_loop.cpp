// Telling the infeasible problems of a batch from the slow ones, on the device (include/gbdpcg.h, "The primal infeasibility
// certificate"): the loop of box_mpc_loop.cpp on a batch in which a disturbance has pushed the initial state of EVERY EIGHTH problem
// outside a state bound -- x_0 is pinned by c and its upper bound lies GAP below that value, so no point satisfies Cz = c and the
// box.  The hard loop (gbdpcg_admm_step_*) never terminates on those: max ||z - w||_inf stalls at GAP and y grows at every replay,
// which from the residuals alone looks like slow convergence.
//
//   once          : gbdpcg_kkt_step_reg_f32 -- S, Phi^-1 and G^-1 of G + rho I; the bounds; gbdpcg_admm_init_f32 with w = y = 0;
//                   ONE executable graph of { gamma ; PCG ; z ; the splitting update }
//   per iteration : replay the graph.  Every P-th replay is bracketed: lambda and y are copied aside in front of it (two copies on
//                   the stream) and gbdpcg_admm_infeas_f32 behind it turns (before, after) into a flag per problem; flags and
//                   residuals are read back, and the loop stops when every problem is flagged or converged
//   then          : the flagged problems are gathered (device-to-device copies of their blocks) and run again with the soft family,
//                   gbdpcg_admm_soft_*: finite KAPPA on the states, +Inf on the inputs -- the rest of the batch stayed hard
// The flag waits for z and w to settle: at 256 x 64 the feasible problems had converged by replay 60 and the 32 disturbed ones were
// flagged at replay 350 (all at once: with EVERY = 8 they are copies of one of the 8 distinct problems) -- hence the generous default.
// usage: infeasible_box_mpc_loop [batch=1024] [knotPoints=128] [max_replays=1000]      (stateSize 14, controlSize 7, fp32)
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
constexpr int P = 10;          // the certificate every P replays
constexpr uint32_t EVERY = 8;  // the disturbed problems
constexpr float TOL = 1e-3f, RHO = 2.0f, GAP = 0.5f, KAPPA = 20.0f, EPS = 0.1f;

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
    const int max_replays = argc > 3 ? atoi(argv[3]) : 1000;
    if (batch == 0 || N < 2 || max_replays < 1) {
        fprintf(stderr, "usage: infeasible_box_mpc_loop [batch] [knotPoints >= 2] [max_replays]\n");
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

    float *dG, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dl0, *dz, *dlo, *dhi, *dw, *dy, *dy0, *dgt, *dres, *dcert;
    uint32_t *d_iters;
    uint8_t *d_flags, *d_infeas;
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
    CK(hipMalloc((void **)&dl0, szc * batch * 4));
    for (float **p : {&dz, &dlo, &dhi, &dw, &dy, &dy0, &dgt}) CK(hipMalloc((void **)p, szg * batch * 4));
    CK(hipMalloc((void **)&dres, 2 * batch * 4));
    CK(hipMalloc((void **)&dcert, 3 * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMalloc((void **)&d_infeas, batch));
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
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> hz(szg * batch), hlo(szg * batch, -inf), hhi(szg * batch, inf);
    CK(hipMemcpy(hz.data(), dz, szg * batch * 4, hipMemcpyDeviceToHost));
    uint32_t disturbed = 0;
    for (uint32_t b = 0; b < batch; ++b) {
        float umax = 0.f, xmax = 0.f;
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) umax = std::max(umax, std::fabs(hz[b * szg + (size_t)k * sv + nx + i]));
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) hlo[b * szg + (size_t)k * sv + nx + i] = -0.5f * umax, hhi[b * szg + (size_t)k * sv + nx + i] = 0.5f * umax;
        for (uint32_t k = 1; k < N; ++k) xmax = std::max(xmax, std::fabs(hz[b * szg + (size_t)k * sv]));
        for (uint32_t k = 1; k < N; ++k) hhi[b * szg + (size_t)k * sv] = 0.5f * xmax;
        if (b % EVERY == 0) hhi[b * szg] = hc[b * szc] - GAP, ++disturbed;   // the disturbance: the bound on x_0 that c contradicts
    }
    CK(hipMemcpy(dlo, hlo.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhi, hhi.data(), szg * batch * 4, hipMemcpyHostToDevice));
    printf("%u problems, %u knots; in %u of them x_0 is pinned %.2f above its bound\n", batch, N, disturbed, GAP);

    GK(gbdpcg_admm_init_f32(h, nx, nu, N, batch, dg, dlo, dhi, drho, dw, dy, dgt, stream));
    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    gbdpcg_graph_t graph;
    GK(gbdpcg_graph_create_admm_step_f32(h, nx, nu, N, batch, dGi, dC, dg, dc, dlo, dhi, drho, dS, dP, dgam, dl, nullptr, nullptr, pcg_tol,
                                         pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, &graph));
    std::vector<float> hres(2 * batch);
    std::vector<uint8_t> hinf(batch);
    int replays = 0;
    uint32_t flagged = 0, converged = 0;
    while (replays < max_replays && flagged + converged < batch) {
        for (int i = 0; i + 1 < P && replays < max_replays; ++i, ++replays) GK(gbdpcg_graph_launch(graph, stream));
        // the bracketed replay: (lambda, y) aside, one step, the certificate of the pair
        CK(hipMemcpyAsync(dl0, dl, szc * batch * 4, hipMemcpyDeviceToDevice, stream));
        CK(hipMemcpyAsync(dy0, dy, szg * batch * 4, hipMemcpyDeviceToDevice, stream));
        GK(gbdpcg_graph_launch(graph, stream));
        ++replays;
        GK(gbdpcg_admm_infeas_f32(h, nx, nu, N, batch, dC, dc, dlo, dhi, drho, dl0, dl, dy0, dy, EPS, dcert, d_infeas, stream));
        CK(hipMemcpyAsync(hres.data(), dres, 2 * batch * 4, hipMemcpyDeviceToHost, stream));
        CK(hipMemcpyAsync(hinf.data(), d_infeas, batch, hipMemcpyDeviceToHost, stream));
        CK(hipStreamSynchronize(stream));
        flagged = converged = 0;
        for (uint32_t b = 0; b < batch; ++b) {
            flagged += hinf[b];
            converged += !hinf[b] && hres[2 * b] < TOL && hres[2 * b + 1] < TOL;
        }
        printf("replay %4d: %u flagged infeasible, %u converged, %u still iterating\n", replays, flagged, converged, batch - flagged - converged);
    }
    bool bad = flagged + converged != batch;
    for (uint32_t b = 0; b < batch; ++b) bad = bad || (hinf[b] != 0) != (b % EVERY == 0);   // exactly the disturbed problems
    gbdpcg_graph_destroy(graph);

    // the flagged problems again, soft: gather their blocks, kappa on the states, from w = y = 0
    std::vector<uint32_t> who;
    for (uint32_t b = 0; b < batch; ++b)
        if (hinf[b]) who.push_back(b);
    const uint32_t nf = (uint32_t)who.size();
    if (nf != 0) {
        float *sGi, *sC, *sg_, *sc_, *srho, *sS, *sP, *slo, *shi, *skap, *sw, *sy, *sgt, *sz, *sl, *sgam, *sres;
        CK(hipMalloc((void **)&sGi, szG * nf * 4));
        CK(hipMalloc((void **)&sC, szC * nf * 4));
        CK(hipMalloc((void **)&sc_, szc * nf * 4));
        CK(hipMalloc((void **)&srho, nf * 4));
        CK(hipMalloc((void **)&sS, szS * nf * 4));
        CK(hipMalloc((void **)&sP, szS * nf * 4));
        for (float **p : {&sg_, &slo, &shi, &skap, &sw, &sy, &sgt, &sz}) CK(hipMalloc((void **)p, szg * nf * 4));
        for (float **p : {&sl, &sgam}) CK(hipMalloc((void **)p, szc * nf * 4));
        CK(hipMalloc((void **)&sres, 2 * nf * 4));
        std::vector<float> hkap(szg * nf, inf);
        for (uint32_t f = 0; f < nf; ++f) {
            const uint32_t b = who[f];
            const struct { float *dst; const float *src; size_t len; } parts[] = {
                {sGi + f * szG, dGi + b * szG, szG}, {sC + f * szC, dC + b * szC, szC}, {sg_ + f * szg, dg + b * szg, szg},
                {sc_ + f * szc, dc + b * szc, szc}, {srho + f, drho + b, 1}, {sS + f * szS, dS + b * szS, szS},
                {sP + f * szS, dP + b * szS, szS}, {slo + f * szg, dlo + b * szg, szg}, {shi + f * szg, dhi + b * szg, szg}};
            for (const auto &p : parts) CK(hipMemcpyAsync(p.dst, p.src, p.len * 4, hipMemcpyDeviceToDevice, stream));
            for (uint32_t k = 0; k < N; ++k)
                for (uint32_t i = 0; i < nx; ++i) hkap[f * szg + (size_t)k * sv + i] = KAPPA;
        }
        CK(hipMemcpyAsync(skap, hkap.data(), szg * nf * 4, hipMemcpyHostToDevice, stream));
        CK(hipMemsetAsync(sw, 0, szg * nf * 4, stream));
        CK(hipMemsetAsync(sy, 0, szg * nf * 4, stream));
        CK(hipMemsetAsync(sl, 0, szc * nf * 4, stream));
        GK(gbdpcg_admm_soft_init_f32(h, nx, nu, N, nf, sg_, slo, shi, skap, srho, sw, sy, sgt, stream));
        gbdpcg_graph_t soft;
        GK(gbdpcg_graph_create_admm_soft_step_f32(h, nx, nu, N, nf, sGi, sC, sg_, sc_, slo, shi, skap, srho, sS, sP, sgam, sl, nullptr, nullptr,
                                                  pcg_tol, pcg_max_iter, d_iters, d_flags, sz, sw, sy, sgt, sres, &soft));
        bool done = false;
        int soft_replays = 0;
        while (soft_replays < max_replays && !done) {
            for (int i = 0; i < P && soft_replays < max_replays; ++i, ++soft_replays) GK(gbdpcg_graph_launch(soft, stream));
            CK(hipMemcpyAsync(hres.data(), sres, 2 * nf * 4, hipMemcpyDeviceToHost, stream));
            CK(hipStreamSynchronize(stream));
            float prim = 0.f, dual = 0.f;
            for (uint32_t f = 0; f < nf; ++f) prim = std::fmax(prim, hres[2 * f]), dual = std::fmax(dual, hres[2 * f + 1]);
            printf("soft replay %4d on %u problems: max ||z - w||_inf %.3e, max rho ||w+ - w||_inf %.3e\n", soft_replays, nf, prim, dual);
            done = prim < TOL && dual < TOL;
        }
        bad = bad || !done;
        gbdpcg_graph_destroy(soft);
        for (void *p : {(void *)sGi, (void *)sC, (void *)sg_, (void *)sc_, (void *)srho, (void *)sS, (void *)sP, (void *)slo, (void *)shi,
                        (void *)skap, (void *)sw, (void *)sy, (void *)sgt, (void *)sz, (void *)sl, (void *)sgam, (void *)sres})
            (void)hipFree(p);
    }

    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)drho, (void *)dS, (void *)dgam, (void *)dGi, (void *)dP, (void *)dl,
                    (void *)dl0, (void *)dz, (void *)dlo, (void *)dhi, (void *)dw, (void *)dy, (void *)dy0, (void *)dgt, (void *)dres,
                    (void *)dcert, (void *)d_iters, (void *)d_flags, (void *)d_infeas})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
