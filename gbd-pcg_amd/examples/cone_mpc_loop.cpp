// Second-order cone rows on a kept linearisation: a thrust-norm bound ||(u_0, u_1, u_2)||_2 <= r per knot next to two linear state
// rows, by ADMM iterations whose solve is the frozen-factorisation step (include/gbdpcg.h, "Second-order cone rows next to the
// linear ones").  This is poly_mpc_loop.cpp with a cone in the place of the input polytope:
//   rows on u_k   : one q = 4 cone: a head row with a ZERO row of E and the offset f = r, then u_0, u_1, u_2; r is half of the
//                   largest norm the unconstrained solution reaches.  On cone rows d_lo holds the offsets, d_hi is not read.
//   rows on x_k   : x_0 + x_1 and x_2 + x_3, each below half of what the unconstrained solution reaches, from knot 1 on (x_0 is given)
//   once          : gbdpcg_admm_lin_form_f32 -- Gt = G + rho E'E (the formation does not depend on the set the rows are projected
//                   on); gbdpcg_kkt_step_f32 on Gt -- S, Phi^-1 and G^-1, and the solution WITHOUT the rows, from which this example
//                   takes its bounds; gbdpcg_admm_soc_init_f32 with w = y = 0;
//                   ONE executable graph of { gamma ; PCG on the unchanged S, Phi^-1 ; z ; the splitting update }
//   per iteration : replay the graph; every CHECK replays read the 2 batch residuals back and stop when
//                   max_b ||E z + f - w||_inf and max_b rho ||E'(w+ - w)||_inf are both below TOL
// At the end z satisfies the dynamics, w the bounds and (to a few ulp) the cones, and E z + f agrees with w to the primal residual.
// usage: cone_mpc_loop [batch=1024] [knotPoints=128] [max_replays=400]      (stateSize 14, controlSize 7, fp32)
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
constexpr uint32_t mx = 2, mu = 4;   // rows per state block, per input block
constexpr uint32_t lx = 2, qx = 0, lu = 0, qu = 4;   // x: both rows linear (qx is ignored); u: one cone of dimension 4
constexpr uint32_t sg = nx * nx + nu * nu, sc = nx * nx + nx * nu, sv = nx + nu, se = mx * nx + mu * nu, sw = mx + mu;
constexpr int CHECK = 10;
constexpr float TOL = 1e-3f, RHO = 2.0f;

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
        fprintf(stderr, "usage: cone_mpc_loop [batch] [knotPoints >= 2] [max_replays]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N, szE = (size_t)se * N - mu * nu, szw = (size_t)sw * N - mu;

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
    // the rows: the same blocks at every knot and in every problem (column-major: entry (r, j) of a block with m rows at r + j m)
    std::vector<float> hE(szE * batch, 0.f);
    for (uint32_t b = 0; b < batch; ++b)
        for (uint32_t k = 0; k < N; ++k) {
            float *Ex = hE.data() + b * szE + (size_t)k * se, *Eu = Ex + mx * nx;
            Ex[0 + 0 * mx] = Ex[0 + 1 * mx] = 1.f;                                   // x_0 + x_1
            Ex[1 + 2 * mx] = Ex[1 + 3 * mx] = 1.f;                                   // x_2 + x_3
            if (k + 1 < N)                                                           // row 0 stays zero: the head, s_0 = f = r
                Eu[1 + 0 * mu] = Eu[2 + 1 * mu] = Eu[3 + 2 * mu] = 1.f;              // u_0, u_1, u_2
        }
    for (uint32_t b = distinct; b < batch; ++b) {
        const uint32_t s = b % distinct;
        std::copy(hG.begin() + s * szG, hG.begin() + (s + 1) * szG, hG.begin() + b * szG);
        std::copy(hC.begin() + s * szC, hC.begin() + (s + 1) * szC, hC.begin() + b * szC);
        std::copy(hg.begin() + s * szg, hg.begin() + (s + 1) * szg, hg.begin() + b * szg);
        std::copy(hc.begin() + s * szc, hc.begin() + (s + 1) * szc, hc.begin() + b * szc);
    }

    float *dG, *dC, *dg, *dc, *drho, *dS, *dgam, *dGi, *dP, *dl, *dz, *dlo, *dhi, *dw, *dy, *dgt, *dres, *dE, *dGt;
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
    for (float **p : {&dz, &dgt}) CK(hipMalloc((void **)p, szg * batch * 4));
    for (float **p : {&dlo, &dhi, &dw, &dy}) CK(hipMalloc((void **)p, szw * batch * 4));
    CK(hipMalloc((void **)&dE, szE * batch * 4));
    CK(hipMalloc((void **)&dGt, szG * batch * 4));
    CK(hipMalloc((void **)&dres, 2 * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMemcpy(dG, hG.data(), szG * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dg, hg.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), szc * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(drho, hrho.data(), batch * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dl, 0, szc * batch * 4));
    CK(hipMemcpy(dE, hE.data(), szE * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dw, 0, szw * batch * 4));
    CK(hipMemset(dy, 0, szw * batch * 4));
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    gbdpcg_handle_t h;
    GK(gbdpcg_create(&h, 0));

    // Gt = G + rho E'E and its factorisation, once; its z is the solution without the rows (of the regularised problem)
    const float pcg_tol = 1e-10f;
    const uint32_t pcg_max_iter = 200;
    GK(gbdpcg_admm_lin_form_f32(h, nx, nu, mx, mu, N, batch, dG, dE, drho, dGt, stream));
    GK(gbdpcg_kkt_step_f32(h, nx, nu, N, batch, dGt, dC, dg, dc, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, dl, nullptr, nullptr, pcg_tol,
                           pcg_max_iter, d_iters, d_flags, dz, stream));
    CK(hipStreamSynchronize(stream));
    std::vector<float> hz(szg * batch), hlo(szw * batch, -std::numeric_limits<float>::infinity()),
        hhi(szw * batch, std::numeric_limits<float>::infinity());
    CK(hipMemcpy(hz.data(), dz, szg * batch * 4, hipMemcpyDeviceToHost));
    size_t outside = 0;
    std::vector<float> v(szw);
    for (uint32_t b = 0; b < batch; ++b) {
        // the solution without the rows: half of its largest state row and half of its largest thrust norm are the bounds
        float umax = 0.f, xmax = 0.f;
        for (uint32_t k = 0; k < N; ++k) {
            const float *Ex = hE.data() + b * szE + (size_t)k * se, *zk = hz.data() + b * szg + (size_t)k * sv;
            for (uint32_t r = 0; r < mx; ++r) {
                float a = 0.f;
                for (uint32_t j = 0; j < nx; ++j) a += Ex[r + j * mx] * zk[j];
                v[(size_t)k * sw + r] = a;
                if (k >= 1) xmax = std::max(xmax, a);
            }
            if (k + 1 < N) {
                const float *u = zk + nx;
                v[(size_t)k * sw + mx] = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
                umax = std::max(umax, v[(size_t)k * sw + mx]);
            }
        }
        for (uint32_t k = 0; k < N; ++k) {
            for (uint32_t r = 0; r < mx && k >= 1; ++r) {
                hhi[b * szw + (size_t)k * sw + r] = 0.5f * xmax;
                outside += v[(size_t)k * sw + r] > 0.5f * xmax;
            }
            if (k + 1 < N) {
                float *f = hlo.data() + b * szw + (size_t)k * sw + mx;
                f[0] = 0.5f * umax, f[1] = f[2] = f[3] = 0.f;     // the offsets of the cone; hhi on these rows is never read
                outside += v[(size_t)k * sw + mx] > 0.5f * umax;
            }
        }
    }
    CK(hipMemcpy(dlo, hlo.data(), szw * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhi, hhi.data(), szw * batch * 4, hipMemcpyHostToDevice));
    printf("%u problems, %u knots: %zu rows and cones of the unconstrained solutions lie outside their bounds\n", batch, N, outside);

    GK(gbdpcg_admm_soc_init_f32(h, nx, nu, mx, mu, lx, qx, lu, qu, N, batch, dg, dE, dlo, dhi, drho, dw, dy, dgt, stream));
    GK(gbdpcg_set_symmetric(h, 1));   // S and Phi^-1 stay as the device wrote them: symmetric in storage
    gbdpcg_graph_t graph;
    GK(gbdpcg_graph_create_admm_soc_step_f32(h, nx, nu, mx, mu, lx, qx, lu, qu, N, batch, dGi, dC, dg, dc, dE, dlo, dhi, drho, dS, dP, dgam,
                                             dl, nullptr, nullptr, pcg_tol, pcg_max_iter, d_iters, d_flags, dz, dw, dy, dgt, dres, &graph));
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
        printf("replay %4d: max ||E z + f - w||_inf %.3e, max rho ||E'(w+ - w)||_inf %.3e%s\n", replays, prim, dual, finite ? "" : " (not finite)");
        if (!finite) break;
        converged = prim < TOL && dual < TOL;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%d replays in %.3f ms (%.3f ms each, residual read-back every %d included)\n", replays, ms, ms / replays, CHECK);

    // w lies between the linear bounds exactly and in the cones to rounding (c s_i is rounded: a few ulp of the radius)
    std::vector<float> hw(szw * batch);
    CK(hipMemcpy(hw.data(), dw, szw * batch * 4, hipMemcpyDeviceToHost));
    size_t violations = 0, on_boundary = 0;
    for (uint32_t b = 0; b < batch; ++b)
        for (uint32_t k = 0; k < N; ++k) {
            const size_t e = b * szw + (size_t)k * sw;
            for (uint32_t r = 0; r < mx; ++r) violations += !(hw[e + r] >= hlo[e + r] && hw[e + r] <= hhi[e + r]);
            if (k + 1 < N) {
                const float *c = hw.data() + e + mx;
                const float norm = std::sqrt(c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
                violations += !(norm <= c[0] * (1.f + 8.f * std::numeric_limits<float>::epsilon()));
                on_boundary += norm >= c[0] * (1.f - 8.f * std::numeric_limits<float>::epsilon());
            }
        }
    const bool bad = !converged || violations != 0 || outside == 0 || on_boundary == 0;
    printf("w outside its bounds or cones in %zu places, %zu cones on their boundary; %s\n", violations, on_boundary,
           converged ? "converged" : "NOT converged");

    gbdpcg_graph_destroy(graph);
    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)drho, (void *)dS, (void *)dgam, (void *)dGi, (void *)dP, (void *)dl,
                    (void *)dz, (void *)dlo, (void *)dhi, (void *)dw, (void *)dy, (void *)dgt, (void *)dres, (void *)dE, (void *)dGt, (void *)d_iters, (void *)d_flags})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
