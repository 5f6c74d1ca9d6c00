// Gradients through the box-constrained MPC solve (include/gbdpcg.h, "The backward pass of the hard box QP"): the loop of
// box_mpc_loop.cpp run to convergence, then the SAME iteration on the adjoint problem and two gradient launches.
//
//   forward  : gbdpcg_kkt_step_reg_f64 -- S, Phi^-1 and G^-1 of G + rho I --, gbdpcg_admm_init_f64 with w = y = 0, K replays of ONE graph of
//              { gamma ; PCG ; z ; splitting update }.  The sign pattern of y is the active set.
//   backward : for the loss l = gz' w, gbdpcg_admm_adjoint_init_f64 with wa = ya = 0, K replays of ONE graph of
//              { gamma ; PCG ; az ; adjoint update } on the kept factorisation (y stands where lo, hi stood),
//              gbdpcg_admm_grad_bounds_f64 (dl/dlo, dl/dhi) and gbdpcg_kkt_grad_f64 (dl/dG, dl/dC); dl/dg = wa, dl/dc = -alambda.
// The program prints dl/dg of a free input and dl/dhi of a clamped one of problem 0 next to central differences taken on the host:
// the forward loop is run again with that one number moved by +-H and the loss is differenced.  Both loops run a fixed count:
// the gradients are as converged as they are.
// usage: box_mpc_grad [batch=8] [knotPoints=16] [replays=400]      (stateSize 14, controlSize 7, fp64)
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
constexpr double RHO = 2.0, H = 1e-3;

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
    const uint32_t batch = argc > 1 ? (uint32_t)atoi(argv[1]) : 8, N = argc > 2 ? (uint32_t)atoi(argv[2]) : 16;
    const int K = argc > 3 ? atoi(argv[3]) : 400;
    if (batch == 0 || N < 2 || K < 1) {
        fprintf(stderr, "usage: box_mpc_grad [batch] [knotPoints >= 2] [replays]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N, D = sizeof(double);

    std::vector<double> hG(szG * batch), hC(szC * batch), hg(szg * batch), hc(szc * batch), hrho(batch, RHO), hgz(szg * batch);
    uint64_t seed = 4321;
    for (uint32_t b = 0; b < batch; ++b) {
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
        for (size_t i = 0; i < szg; ++i) hgz[b * szg + i] = urand(seed);
    }

    double *dG, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dz, *dlo, *dhi, *dw, *dy, *dgt, *dres;
    double *dgz, *dngl, *dgama, *dal, *daz, *dwa, *dya, *dgta, *dresa, *dglo, *dghi, *dgG, *dgC;
    uint32_t *d_iters;
    uint8_t *d_flags;
    for (double **p : {&dG, &dGi, &dgG}) CK(hipMalloc((void **)p, szG * batch * D));
    for (double **p : {&dC, &dgC}) CK(hipMalloc((void **)p, szC * batch * D));
    for (double **p : {&dS, &dP}) CK(hipMalloc((void **)p, szS * batch * D));
    for (double **p : {&dc, &dgam, &dl, &dngl, &dgama, &dal}) CK(hipMalloc((void **)p, szc * batch * D));
    for (double **p : {&dg, &dz, &dlo, &dhi, &dw, &dy, &dgt, &dgz, &daz, &dwa, &dya, &dgta, &dglo, &dghi}) CK(hipMalloc((void **)p, szg * batch * D));
    for (double **p : {&dres, &dresa}) CK(hipMalloc((void **)p, 2 * batch * D));
    CK(hipMalloc((void **)&drho, batch * D));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMemcpy(dG, hG.data(), szG * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), szc * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(drho, hrho.data(), batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dgz, hgz.data(), szg * batch * D, hipMemcpyHostToDevice));
    CK(hipMemset(dngl, 0, szc * batch * D));   // the loss does not depend on lambda
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    gbdpcg_handle_t h;
    GK(gbdpcg_create(&h, 0));
    const double pcg_tol = 1e-22;
    const uint32_t pcg_max_iter = 200;

    // the bounds: every input within half of the largest input of the solution without the box
    CK(hipMemcpy(dg, hg.data(), szg * batch * D, hipMemcpyHostToDevice));
    CK(hipMemset(dl, 0, szc * batch * D));
    GK(gbdpcg_kkt_step_reg_f64(h, nx, nu, N, batch, dG, dC, dg, dc, drho, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, dl, nullptr, nullptr, pcg_tol,
                               pcg_max_iter, d_iters, d_flags, dz, stream));
    CK(hipStreamSynchronize(stream));
    std::vector<double> hz(szg * batch), hlo(szg * batch, -std::numeric_limits<double>::infinity()),
        hhi(szg * batch, std::numeric_limits<double>::infinity());
    CK(hipMemcpy(hz.data(), dz, szg * batch * D, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < batch; ++b) {
        double umax = 0.0;
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) umax = std::max(umax, std::fabs(hz[b * szg + (size_t)k * sv + nx + i]));
        for (uint32_t k = 0; k + 1 < N; ++k)
            for (uint32_t i = 0; i < nu; ++i) {
                hlo[b * szg + (size_t)k * sv + nx + i] = -0.5 * umax;
                hhi[b * szg + (size_t)k * sv + nx + i] = 0.5 * umax;
            }
    }
    CK(hipMemcpy(dlo, hlo.data(), szg * batch * D, hipMemcpyHostToDevice));

    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    gbdpcg_graph_t fwd, adj;
    GK(gbdpcg_graph_create_admm_step_f64(h, nx, nu, N, batch, dGi, dC, dg, dc, dlo, dhi, drho, dS, dP, dgam, dl, nullptr, nullptr, pcg_tol,
                                         pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, &fwd));
    GK(gbdpcg_graph_create_admm_adjoint_step_f64(h, nx, nu, N, batch, dGi, dC, dgz, dngl, dy, drho, dS, dP, dgama, dal, nullptr, nullptr,
                                                 pcg_tol, pcg_max_iter, d_iters, d_flags, daz, dwa, dya, dgta, dresa, &adj));

    // the forward loop for the g and hi on the host: the graph reads the same device buffers every time
    std::vector<double> hw(szg * batch), hy(szg * batch);
    auto forward = [&](double &loss) -> int {
        CK(hipMemcpy(dg, hg.data(), szg * batch * D, hipMemcpyHostToDevice));
        CK(hipMemcpy(dhi, hhi.data(), szg * batch * D, hipMemcpyHostToDevice));
        CK(hipMemset(dl, 0, szc * batch * D));
        CK(hipMemset(dw, 0, szg * batch * D));
        CK(hipMemset(dy, 0, szg * batch * D));
        GK(gbdpcg_admm_init_f64(h, nx, nu, N, batch, dg, dlo, dhi, drho, dw, dy, dgt, stream));
        for (int i = 0; i < K; ++i) GK(gbdpcg_graph_launch(fwd, stream));
        CK(hipMemcpyAsync(hw.data(), dw, szg * batch * D, hipMemcpyDeviceToHost, stream));
        CK(hipMemcpyAsync(hy.data(), dy, szg * batch * D, hipMemcpyDeviceToHost, stream));
        CK(hipStreamSynchronize(stream));
        loss = 0.0;
        for (size_t e = 0; e < hw.size(); ++e) loss += hgz[e] * hw[e];
        return 0;
    };
    double loss = 0.0;
    if (forward(loss)) return 1;
    std::vector<double> hres(2 * batch);
    CK(hipMemcpy(hres.data(), dres, 2 * batch * D, hipMemcpyDeviceToHost));
    double prim = 0.0;
    size_t active = 0;
    for (uint32_t b = 0; b < batch; ++b) prim = std::fmax(prim, hres[2 * b]);
    for (double v : hy) active += v != 0.0;
    printf("%u problems, %u knots, %d forward replays: max ||z - w||_inf %.3e, %zu clamped inputs, loss %.12f\n", batch, N, K, prim, active, loss);
    // a free input and an input clamped at its upper bound, problem 0 (y == 0 / y > 0: the mask of the backward pass)
    size_t efree = szg, ehi = szg;
    for (uint32_t k = 0; k + 1 < N; ++k)
        for (uint32_t i = 0; i < nu; ++i) {
            const size_t e = (size_t)k * sv + nx + i;
            if (efree == szg && hy[e] == 0.0) efree = e;
            if (ehi == szg && hy[e] > 0.0) ehi = e;
        }

    // the backward pass
    CK(hipMemsetAsync(dal, 0, szc * batch * D, stream));
    CK(hipMemsetAsync(dwa, 0, szg * batch * D, stream));
    CK(hipMemsetAsync(dya, 0, szg * batch * D, stream));
    GK(gbdpcg_admm_adjoint_init_f64(h, nx, nu, N, batch, dgz, dy, drho, dwa, dya, dgta, stream));
    for (int i = 0; i < K; ++i) GK(gbdpcg_graph_launch(adj, stream));
    GK(gbdpcg_admm_grad_bounds_f64(h, nx, nu, N, batch, dy, drho, dya, dglo, dghi, stream));
    GK(gbdpcg_kkt_grad_f64(h, nx, nu, N, batch, dw, dl, dwa, dal, dgG, dgC, stream));
    std::vector<double> hwa(szg * batch), hghi(szg * batch), hgG(szG);
    CK(hipMemcpyAsync(hwa.data(), dwa, szg * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hghi.data(), dghi, szg * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hgG.data(), dgG, szG * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hres.data(), dresa, 2 * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    double aprim = 0.0;
    for (uint32_t b = 0; b < batch; ++b) aprim = std::fmax(aprim, hres[2 * b]);
    printf("%d adjoint replays: max ||az - wa||_inf %.3e; dl/dQ_0(0,0) of problem 0 = %.9f\n", K, aprim, hgG[0]);

    // central differences on the host: move one number, run the forward loop again, difference the loss
    bool bad = !(prim < 1e-6) || !(aprim < 1e-6);
    struct Probe {
        const char *what;
        std::vector<double> *arr;
        size_t e;
        double grad;
    };
    std::vector<Probe> probes;
    if (efree != szg) probes.push_back({"dl/dg  of a free input   ", &hg, efree, hwa[efree]});
    if (ehi != szg) probes.push_back({"dl/dhi of a clamped input", &hhi, ehi, hghi[ehi]});
    for (const Probe &p : probes) {
        const double keep = (*p.arr)[p.e];
        double lp, lm;
        (*p.arr)[p.e] = keep + H;
        if (forward(lp)) return 1;
        (*p.arr)[p.e] = keep - H;
        if (forward(lm)) return 1;
        (*p.arr)[p.e] = keep;
        const double fd = (lp - lm) / (2 * H);
        printf("%s (problem 0, entry %zu): device %.9f, central difference %.9f, difference %.2e\n", p.what, p.e, p.grad, fd, p.grad - fd);
        bad = bad || !(std::fabs(p.grad - fd) <= 1e-4 * std::fmax(1.0, std::fabs(fd)));
    }
    if (ehi != szg) printf("dl/dg of that clamped input: %.1f (exactly zero)\n", hwa[ehi]);
    bad = bad || probes.empty() || (ehi != szg && hwa[ehi] != 0.0);

    gbdpcg_graph_destroy(fwd);
    gbdpcg_graph_destroy(adj);
    gbdpcg_destroy(h);
    for (double *p : {dG, dC, dg, dc, drho, dS, dgam, dGi, dP, dl, dz, dlo, dhi, dw, dy, dgt, dres, dgz, dngl, dgama, dal, daz, dwa, dya, dgta,
                      dresa, dglo, dghi, dgG, dgC})
        (void)hipFree(p);
    (void)hipFree(d_iters);
    (void)hipFree(d_flags);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
