// Stopping every problem of a batch on its OWN optimality test, on the device (include/gbdpcg.h, "The optimality test of the ADMM
// families"): the loop of box_mpc_loop.cpp with gbdpcg_admm_optimality_f32 behind the step.  d_res of the update cannot say that
// (z, lambda, rho y) solves the QP -- it assumes an exact z-step and has no scale; the optimality launch evaluates stationarity with
// the row multiplier, the dynamics and consensus against eps_abs + eps_rel * scale and leaves ONE BYTE per problem.
//
//   once          : gbdpcg_kkt_step_reg_f32 -- S, Phi^-1 and G^-1 of G + rho I; the bounds; gbdpcg_admm_init_f32 with w = y = 0;
//                   a CALLER-OWNED capture of { gbdpcg_admm_step_f32 ; gbdpcg_admm_optimality_f32 } into one executable graph
//   per iteration : replay the graph, read back the `batch` bytes of d_done and nothing else.  A problem whose byte is set for the
//                   first time has its w copied aside (device to device): that is its answer, whatever the rest of the batch
//                   still does.  The loop ends when every problem has stopped.
// The PCG runs with a deliberately SMALL max_iter: the residuals of the update would not notice, the optimality test does -- it
// reads the Hessian G, not the factorisation.
// usage: optimality_box_mpc_loop [batch=1024] [knotPoints=128] [max_replays=400]      (stateSize 14, controlSize 7, fp32)
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
constexpr float RHO = 2.0f, EPS_ABS = 1e-4f, EPS_REL = 1e-4f;

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
        fprintf(stderr, "usage: optimality_box_mpc_loop [batch] [knotPoints >= 2] [max_replays]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N;

    // a few distinct problems, repeated over the batch (host generation only); the copies get their own g, so they stop apart
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
        for (size_t i = 0; i < szc; ++i) hc[b * szc + i] = 0.17f * (float)urand(seed);
    }
    for (uint32_t b = distinct; b < batch; ++b) {
        const uint32_t s = b % distinct;
        std::copy(hG.begin() + s * szG, hG.begin() + (s + 1) * szG, hG.begin() + b * szG);
        std::copy(hC.begin() + s * szC, hC.begin() + (s + 1) * szC, hC.begin() + b * szC);
        std::copy(hc.begin() + s * szc, hc.begin() + (s + 1) * szc, hc.begin() + b * szc);
    }
    for (size_t i = 0; i < szg * batch; ++i) hg[i] = 1.7f * (float)urand(seed);

    float *dG, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dr, *dp, *dz, *dlo, *dhi, *dw, *dy, *dgt, *dout, *dres, *dopt;
    uint32_t *d_iters;
    uint8_t *d_flags, *d_done;
    CK(hipMalloc((void **)&dG, szG * batch * 4));
    CK(hipMalloc((void **)&dC, szC * batch * 4));
    CK(hipMalloc((void **)&dc, szc * batch * 4));
    CK(hipMalloc((void **)&drho, batch * 4));
    CK(hipMalloc((void **)&dS, szS * batch * 4));
    CK(hipMalloc((void **)&dGi, szG * batch * 4));
    CK(hipMalloc((void **)&dP, szS * batch * 4));
    for (float **p : {&dgam, &dl, &dr, &dp}) CK(hipMalloc((void **)p, szc * batch * 4));
    for (float **p : {&dg, &dz, &dlo, &dhi, &dw, &dy, &dgt, &dout}) CK(hipMalloc((void **)p, szg * batch * 4));
    CK(hipMalloc((void **)&dres, 2 * batch * 4));
    CK(hipMalloc((void **)&dopt, 6 * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMalloc((void **)&d_done, batch));
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
    GK(gbdpcg_kkt_step_reg_f32(h, nx, nu, N, batch, dG, dC, dg, dc, drho, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, dl, dr, dp, 1e-10f, 200,
                               d_iters, d_flags, dz, stream));
    CK(hipStreamSynchronize(stream));
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> hz(szg * batch), hlo(szg * batch, -inf), hhi(szg * batch, inf);
    CK(hipMemcpy(hz.data(), dz, szg * batch * 4, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < batch; ++b) {
        float umax = 0.f;
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) umax = std::max(umax, std::fabs(hz[b * szg + (size_t)k * sv + nx + i]));
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) hlo[b * szg + (size_t)k * sv + nx + i] = -0.5f * umax, hhi[b * szg + (size_t)k * sv + nx + i] = 0.5f * umax;
    }
    CK(hipMemcpy(dlo, hlo.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhi, hhi.data(), szg * batch * 4, hipMemcpyHostToDevice));

    GK(gbdpcg_admm_init_f32(h, nx, nu, N, batch, dg, dlo, dhi, drho, dw, dy, dgt, stream));
    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    CK(hipStreamSynchronize(stream));

    // step -> optimality, captured by the caller into one graph.  max_iter = 4: the warm-started PCG is cut short on purpose.
    const float pcg_tol = 1e-10f;
    const uint32_t pcg_max_iter = 4;
    hipGraph_t captured;
    hipGraphExec_t exec;
    CK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    GK(gbdpcg_admm_step_f32(h, nx, nu, N, batch, dGi, dC, dg, dc, dlo, dhi, drho, dS, dP, dgam, dl, dr, dp, pcg_tol, pcg_max_iter, d_iters,
                            d_flags, dz, dw, dy, dgt, dres, stream));
    GK(gbdpcg_admm_optimality_f32(h, nx, nu, N, batch, dG, dC, dg, dc, drho, dz, dl, dw, dy, EPS_ABS, EPS_REL, dopt, d_done, stream));
    CK(hipStreamEndCapture(stream, &captured));
    CK(hipGraphInstantiate(&exec, captured, nullptr, nullptr, 0));

    std::vector<uint8_t> hdone(batch);
    std::vector<int> stopped_at(batch, 0);
    uint32_t stopped = 0;
    int replays = 0;
    while (replays < max_replays && stopped < batch) {
        CK(hipGraphLaunch(exec, stream));
        ++replays;
        CK(hipMemcpyAsync(hdone.data(), d_done, batch, hipMemcpyDeviceToHost, stream));   // the only read-back of the loop
        CK(hipStreamSynchronize(stream));
        uint32_t now = 0;
        for (uint32_t b = 0; b < batch; ++b)
            if (hdone[b] && !stopped_at[b]) {
                stopped_at[b] = replays, ++stopped, ++now;
                CK(hipMemcpyAsync(dout + b * szg, dw + b * szg, szg * 4, hipMemcpyDeviceToDevice, stream));   // this problem's answer
            }
        if (now || replays % 20 == 0) printf("replay %4d: %u stopped now, %u of %u in all\n", replays, now, stopped, batch);
    }
    CK(hipStreamSynchronize(stream));

    // what the last launch saw, for the record (not part of the loop)
    std::vector<float> hopt(6 * batch), hres(2 * batch);
    CK(hipMemcpy(hopt.data(), dopt, 6 * batch * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hres.data(), dres, 2 * batch * 4, hipMemcpyDeviceToHost));
    int first = max_replays + 1, last = 0;
    float worst = 0.f;
    for (uint32_t b = 0; b < batch; ++b) {
        if (stopped_at[b]) first = std::min(first, stopped_at[b]), last = std::max(last, stopped_at[b]);
        for (int i = 0; i < 3; ++i) worst = std::fmax(worst, hopt[6 * b + i] / (EPS_ABS + EPS_REL * hopt[6 * b + 3 + i]));
    }
    printf("%u of %u problems stopped between replay %d and %d; at the end the largest r / (eps_abs + eps_rel n) is %.3f\n", stopped, batch,
           first, last, worst);
    const bool bad = stopped != batch;

    CK(hipGraphExecDestroy(exec));
    CK(hipGraphDestroy(captured));
    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)drho, (void *)dS, (void *)dgam, (void *)dGi, (void *)dP, (void *)dl,
                    (void *)dr, (void *)dp, (void *)dz, (void *)dlo, (void *)dhi, (void *)dw, (void *)dy, (void *)dgt, (void *)dout,
                    (void *)dres, (void *)dopt, (void *)d_iters, (void *)d_flags, (void *)d_done})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
