// Gradients through the MPC solve with stage-wise linear rows (include/gbdpcg.h, "The backward pass of the hard linear-row QP"):
// the loop of poly_mpc_loop.cpp run to convergence, then the SAME iteration on the adjoint problem and two gradient launches.
//
//   forward  : gbdpcg_admm_lin_form_f64 -- Gt = G + rho E'E --, gbdpcg_kkt_step_f64 on Gt -- S, Phi^-1 and G^-1 --,
//              gbdpcg_admm_lin_init_f64 with w = y = 0, K replays of ONE graph of { gamma ; PCG ; z ; rows update }.  The sign
//              pattern of y is the set of active rows.
//   backward : for the loss l = gz' z, gbdpcg_admm_lin_adjoint_init_f64 with wa = ya = 0, K replays of ONE graph of
//              { gamma ; PCG ; az ; adjoint rows update } on the kept factorisation (y stands where lo, hi stood),
//              gbdpcg_admm_lin_grad_f64 (dl/dlo, dl/dhi, dl/dE) and gbdpcg_kkt_grad_f64 (dl/dG, dl/dC); dl/dg = az, dl/dc = -alambda.
// The rows: x_0 + x_1 <= b on every state from knot 1 on, |u_0 + u_1| <= b and |u_2 - u_3| <= b on every input.
// The program prints dl/dg of an input, dl/dhi of a row held at its upper bound and dl/dE of one entry of that row, problem 0,
// next to central differences taken on the host: the forward pass is run again (E moves Gt, so it factors again) with that one
// number moved by +-H and the loss is differenced.  Both loops run a fixed count: the gradients are as converged as they are.
// usage: poly_mpc_grad [batch=8] [knotPoints=16] [replays=600]      (stateSize 14, controlSize 7, fp64)
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
constexpr uint32_t nx = n, nu = 7, mx = 1, mu = 2;
constexpr uint32_t sg = nx * nx + nu * nu, sc = nx * nx + nx * nu, sv = nx + nu, se = mx * nx + mu * nu, sw = mx + mu;
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
    const int K = argc > 3 ? atoi(argv[3]) : 600;
    if (batch == 0 || N < 2 || K < 1) {
        fprintf(stderr, "usage: poly_mpc_grad [batch] [knotPoints >= 2] [replays]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N, szE = (size_t)se * N - mu * nu, szw = (size_t)sw * N - mu, D = sizeof(double);
    const double inf = std::numeric_limits<double>::infinity();

    std::vector<double> hG(szG * batch), hC(szC * batch), hg(szg * batch), hc(szc * batch), hrho(batch, RHO), hgz(szg * batch);
    std::vector<double> hE(szE * batch, 0.0);
    uint64_t seed = 4321;
    for (uint32_t b = 0; b < batch; ++b) {
        double *G = hG.data() + b * szG, *C = hC.data() + b * szC;
        for (uint32_t k = 0; k < N; ++k) {
            spd(seed, nx, G + (size_t)k * sg);
            double *Ex = hE.data() + b * szE + (size_t)k * se, *Eu = Ex + mx * nx;
            Ex[0 + 0 * mx] = Ex[0 + 1 * mx] = 1.0;                                   // x_0 + x_1
            if (k + 1 < N) {
                Eu[0 + 0 * mu] = 1.0, Eu[0 + 1 * mu] = 1.0;                          // u_0 + u_1
                Eu[1 + 2 * mu] = 1.0, Eu[1 + 3 * mu] = -1.0;                         // u_2 - u_3
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

    double *dG, *dGt, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dz, *dE, *dlo, *dhi, *dw, *dy, *dgt, *dres;
    double *dgz, *dngl, *dgama, *dal, *daz, *dwa, *dya, *dgta, *dresa, *dglo, *dghi, *dgE, *dgG, *dgC;
    uint32_t *d_iters;
    uint8_t *d_flags;
    for (double **p : {&dG, &dGt, &dGi, &dgG}) CK(hipMalloc((void **)p, szG * batch * D));
    for (double **p : {&dC, &dgC}) CK(hipMalloc((void **)p, szC * batch * D));
    for (double **p : {&dS, &dP}) CK(hipMalloc((void **)p, szS * batch * D));
    for (double **p : {&dE, &dgE}) CK(hipMalloc((void **)p, szE * batch * D));
    for (double **p : {&dc, &dgam, &dl, &dngl, &dgama, &dal}) CK(hipMalloc((void **)p, szc * batch * D));
    for (double **p : {&dg, &dz, &dgt, &dgz, &daz, &dgta}) CK(hipMalloc((void **)p, szg * batch * D));
    for (double **p : {&dlo, &dhi, &dw, &dy, &dwa, &dya, &dglo, &dghi}) CK(hipMalloc((void **)p, szw * batch * D));
    for (double **p : {&dres, &dresa}) CK(hipMalloc((void **)p, 2 * batch * D));
    CK(hipMalloc((void **)&drho, batch * D));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMemcpy(dG, hG.data(), szG * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), szc * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dE, hE.data(), szE * batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(drho, hrho.data(), batch * D, hipMemcpyHostToDevice));
    CK(hipMemcpy(dgz, hgz.data(), szg * batch * D, hipMemcpyHostToDevice));
    CK(hipMemset(dngl, 0, szc * batch * D));   // the loss does not depend on lambda
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    gbdpcg_handle_t h;
    GK(gbdpcg_create(&h, 0));
    const double pcg_tol = 1e-22;
    const uint32_t pcg_max_iter = 200;

    // the rows of one problem's z on the host
    auto rows_of = [&](uint32_t b, const std::vector<double> &z, std::vector<double> &v) {
        for (uint32_t k = 0; k < N; ++k) {
            const double *Ex = hE.data() + b * szE + (size_t)k * se, *Eu = Ex + mx * nx, *zk = z.data() + b * szg + (size_t)k * sv;
            for (uint32_t r = 0; r < mx; ++r) {
                double a = 0.0;
                for (uint32_t j = 0; j < nx; ++j) a += Ex[r + j * mx] * zk[j];
                v[(size_t)k * sw + r] = a;
            }
            for (uint32_t r = 0; r < mu && k + 1 < N; ++r) {
                double a = 0.0;
                for (uint32_t j = 0; j < nu; ++j) a += Eu[r + j * mu] * zk[nx + j];
                v[(size_t)k * sw + mx + r] = a;
            }
        }
    };

    // the bounds: every row within half of the largest row of the solution without the rows (the state rows of knot 0 are free)
    CK(hipMemcpy(dg, hg.data(), szg * batch * D, hipMemcpyHostToDevice));
    CK(hipMemset(dl, 0, szc * batch * D));
    GK(gbdpcg_kkt_step_f64(h, nx, nu, N, batch, dG, dC, dg, dc, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, dl, nullptr, nullptr, pcg_tol,
                           pcg_max_iter, d_iters, d_flags, dz, stream));
    CK(hipStreamSynchronize(stream));
    std::vector<double> hz(szg * batch), hlo(szw * batch, -inf), hhi(szw * batch, inf), v(szw);
    CK(hipMemcpy(hz.data(), dz, szg * batch * D, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < batch; ++b) {
        rows_of(b, hz, v);
        double vmax = 0.0;
        for (size_t r = mx; r < szw; ++r) vmax = std::max(vmax, std::fabs(v[r]));
        for (size_t r = mx; r < szw; ++r) {
            hhi[b * szw + r] = 0.5 * vmax;
            if (r % sw >= mx) hlo[b * szw + r] = -0.5 * vmax;
        }
    }
    CK(hipMemcpy(dlo, hlo.data(), szw * batch * D, hipMemcpyHostToDevice));

    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    gbdpcg_graph_t fwd, adj;
    GK(gbdpcg_graph_create_admm_lin_step_f64(h, nx, nu, mx, mu, N, batch, dGi, dC, dg, dc, dE, dlo, dhi, drho, dS, dP, dgam, dl, nullptr,
                                             nullptr, pcg_tol, pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, &fwd));
    GK(gbdpcg_graph_create_admm_lin_adjoint_step_f64(h, nx, nu, mx, mu, N, batch, dGi, dC, dgz, dngl, dE, dy, drho, dS, dP, dgama, dal,
                                                     nullptr, nullptr, pcg_tol, pcg_max_iter, d_iters, d_flags, daz, dwa, dya, dgta,
                                                     dresa, &adj));

    // the forward pass for the g, hi and E on the host: the graph reads the same device buffers every time
    std::vector<double> hy(szw * batch);
    auto forward = [&](double &loss) -> int {
        CK(hipMemcpy(dg, hg.data(), szg * batch * D, hipMemcpyHostToDevice));
        CK(hipMemcpy(dhi, hhi.data(), szw * batch * D, hipMemcpyHostToDevice));
        CK(hipMemcpy(dE, hE.data(), szE * batch * D, hipMemcpyHostToDevice));
        CK(hipMemset(dl, 0, szc * batch * D));
        CK(hipMemset(dw, 0, szw * batch * D));
        CK(hipMemset(dy, 0, szw * batch * D));
        GK(gbdpcg_admm_lin_form_f64(h, nx, nu, mx, mu, N, batch, dG, dE, drho, dGt, stream));
        GK(gbdpcg_kkt_step_f64(h, nx, nu, N, batch, dGt, dC, dg, dc, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, dl, nullptr, nullptr, pcg_tol,
                               pcg_max_iter, d_iters, d_flags, dz, stream));
        GK(gbdpcg_admm_lin_init_f64(h, nx, nu, mx, mu, N, batch, dg, dE, dlo, dhi, drho, dw, dy, dgt, stream));
        for (int i = 0; i < K; ++i) GK(gbdpcg_graph_launch(fwd, stream));
        CK(hipMemcpyAsync(hz.data(), dz, szg * batch * D, hipMemcpyDeviceToHost, stream));
        CK(hipMemcpyAsync(hy.data(), dy, szw * batch * D, hipMemcpyDeviceToHost, stream));
        CK(hipStreamSynchronize(stream));
        loss = 0.0;
        for (size_t e = 0; e < hz.size(); ++e) loss += hgz[e] * hz[e];
        return 0;
    };
    double loss = 0.0;
    if (forward(loss)) return 1;
    std::vector<double> hres(2 * batch);
    CK(hipMemcpy(hres.data(), dres, 2 * batch * D, hipMemcpyDeviceToHost));
    double prim = 0.0;
    size_t active = 0;
    for (uint32_t b = 0; b < batch; ++b) prim = std::fmax(prim, hres[2 * b]);
    for (double y : hy) active += y != 0.0;
    printf("%u problems, %u knots, %d forward replays: max ||E z - w||_inf %.3e, %zu active rows, loss %.12f\n", batch, N, K, prim, active,
           loss);
    // a row of problem 0 held at its upper bound (y > 0: the mask of the backward pass), an input row if there is one
    size_t rhi = szw;
    for (size_t r = 0; r < szw; ++r)
        if (hy[r] > 0.0 && (rhi == szw || (rhi % sw < mx && r % sw >= mx))) rhi = r;

    // the backward pass
    CK(hipMemsetAsync(dal, 0, szc * batch * D, stream));
    CK(hipMemsetAsync(dwa, 0, szw * batch * D, stream));
    CK(hipMemsetAsync(dya, 0, szw * batch * D, stream));
    GK(gbdpcg_admm_lin_adjoint_init_f64(h, nx, nu, mx, mu, N, batch, dgz, dE, dy, drho, dwa, dya, dgta, stream));
    for (int i = 0; i < K; ++i) GK(gbdpcg_graph_launch(adj, stream));
    GK(gbdpcg_admm_lin_grad_f64(h, nx, nu, mx, mu, N, batch, dz, daz, dy, dya, drho, dglo, dghi, dgE, stream));
    GK(gbdpcg_kkt_grad_f64(h, nx, nu, N, batch, dz, dl, daz, dal, dgG, dgC, stream));
    std::vector<double> haz(szg * batch), hghi(szw * batch), hgE(szE * batch), hgG(szG);
    CK(hipMemcpyAsync(haz.data(), daz, szg * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hghi.data(), dghi, szw * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hgE.data(), dgE, szE * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hgG.data(), dgG, szG * D, hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(hres.data(), dresa, 2 * batch * D, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    double aprim = 0.0;
    for (uint32_t b = 0; b < batch; ++b) aprim = std::fmax(aprim, hres[2 * b]);
    printf("%d adjoint replays: max ||E az - wa||_inf %.3e; dl/dQ_0(0,0) of problem 0 = %.9f\n", K, aprim, hgG[0]);

    // central differences on the host: move one number, run the forward pass again, difference the loss
    bool bad = !(prim < 1e-6) || !(aprim < 1e-6);
    struct Probe {
        const char *what;
        std::vector<double> *arr;
        size_t e;
        double grad;
    };
    std::vector<Probe> probes;
    probes.push_back({"dl/dg  of u_0 of knot 0      ", &hg, (size_t)nx, haz[nx]});
    if (rhi != szw) {
        // the entry of E in the row's first column with a coefficient: row r of its block, column 0 (state) or 0 / 2 (input rows 0 / 1)
        const size_t k = rhi / sw, r = rhi % sw;
        const size_t e = r < mx ? k * se + r : k * se + mx * nx + (r - mx) + (r - mx == 0 ? 0 : 2) * mu;
        probes.push_back({"dl/dhi of a row at its bound ", &hhi, rhi, hghi[rhi]});
        probes.push_back({"dl/dE  of an entry of the row", &hE, e, hgE[e]});
    }
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
    bad = bad || probes.size() != 3;

    gbdpcg_graph_destroy(fwd);
    gbdpcg_graph_destroy(adj);
    gbdpcg_destroy(h);
    for (double *p : {dG, dGt, dC, dg, dc, drho, dS, dgam, dGi, dP, dl, dz, dE, dlo, dhi, dw, dy, dgt, dres, dgz, dngl, dgama, dal, daz, dwa,
                      dya, dgta, dresa, dglo, dghi, dgE, dgG, dgC})
        (void)hipFree(p);
    (void)hipFree(d_iters);
    (void)hipFree(d_flags);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
