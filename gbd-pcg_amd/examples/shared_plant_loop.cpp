// One plant, many states: the shared-matrix form of the linear MPC loop (linear_mpc_loop.cpp).  The cost Hessians G and the
// dynamics Jacobians C of ONE plant model are fixed; `batch` copies of it (a fleet of identical robots, the scenarios of a
// sampling MPC, a Monte-Carlo run of one controller) each bring their own measured state (c_0) and gradients g every tick.
// S = C G^-1 C', Phi^-1, G^-1 and C exist ONCE on the device -- 0.9 MB at 14 / 7 / 128 in fp32 where `batch` copies would
// take 0.9 GB at batch 1024 -- and every kernel of the tick reads that one set (include/gbdpcg.h, shared-matrix batches):
//
//   once      : kktStep<float> at batch 1 on the plant -- forms S, G^-1, Phi^-1 (the factorisation)
//               ONE executable graph of { gamma = -(c + C G^-1 g) ; PCG on the one S, Phi^-1 ; z from lambda } for `batch` problems
//               (gbdpcg_graph_create_kkt_resolve_shared_f32; kktResolveShared<float> is the same step as a plain call)
//   per tick  : the caller rewrites g and c of every problem in place and replays the graph; lambda of the previous tick is
//               the warm start
//
// S is left exactly as form_schur wrote it, symmetric in storage, so the handle is told so (gbdpcg_set_symmetric(h, 1)).
// For the first and the last tick the two KKT residuals of a few problems are checked in double precision on the host:
// |G z + g + C'lambda| / |g|  and  |C z - c| / |c|; the exit status is non-zero if one of them, or a solve that ran out of
// iterations, fails.
// usage: shared_plant_loop [batch=1024] [knotPoints=128] [ticks=8]      (stateSize 14, controlSize 7, fp32)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gbdpcg.hpp"
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

struct Residuals {
    double stationarity, feasibility;
};

// KKT residuals of (z, lambda) for one problem, fp64 on the host, straight from the packed blocks.
Residuals kkt_residuals(uint32_t N, const float *G, const float *C, const float *g, const float *c, const float *z, const float *lam)
{
    double s2 = 0, g2 = 0, f2 = 0, c2 = 0;
    for (uint32_t k = 0; k < N; ++k) {
        const float *Q = G + (size_t)k * sg, *R = Q + nx * nx, *A = C + (size_t)k * sc, *B = A + nx * nx;
        const float *x = z + (size_t)k * sv, *u = x + nx, *q = g + (size_t)k * sv, *r = q + nx;
        const bool nxt = k + 1 < N;
        for (uint32_t i = 0; i < nx; ++i) {   // Q x + q + lambda_k - A' lambda_{k+1}
            double v = q[i] + lam[k * nx + i];
            for (uint32_t j = 0; j < nx; ++j) v += (double)Q[j * nx + i] * x[j];
            if (nxt)
                for (uint32_t j = 0; j < nx; ++j) v -= (double)A[i * nx + j] * lam[(k + 1) * nx + j];
            s2 += v * v;
            g2 += (double)q[i] * q[i];
        }
        if (nxt)
            for (uint32_t i = 0; i < nu; ++i) {   // R u + r - B' lambda_{k+1}
                double v = r[i];
                for (uint32_t j = 0; j < nu; ++j) v += (double)R[j * nu + i] * u[j];
                for (uint32_t j = 0; j < nx; ++j) v -= (double)B[i * nx + j] * lam[(k + 1) * nx + j];
                s2 += v * v;
                g2 += (double)r[i] * r[i];
            }
        for (uint32_t i = 0; i < nx; ++i) {   // x_k - A_{k-1} x_{k-1} - B_{k-1} u_{k-1} - c_k
            double v = (double)x[i] - c[k * nx + i];
            if (k > 0) {
                const float *Ap = C + (size_t)(k - 1) * sc, *Bp = Ap + nx * nx, *xp = z + (size_t)(k - 1) * sv, *up = xp + nx;
                for (uint32_t j = 0; j < nx; ++j) v -= (double)Ap[j * nx + i] * xp[j];
                for (uint32_t j = 0; j < nu; ++j) v -= (double)Bp[j * nx + i] * up[j];
            }
            f2 += v * v;
            c2 += (double)c[k * nx + i] * c[k * nx + i];
        }
    }
    return {std::sqrt(s2 / g2), std::sqrt(f2 / c2)};
}
}  // namespace

int main(int argc, char **argv)
{
    const uint32_t batch = argc > 1 ? (uint32_t)atoi(argv[1]) : 1024, N = argc > 2 ? (uint32_t)atoi(argv[2]) : 128;
    const int ticks = argc > 3 ? atoi(argv[3]) : 8;
    if (batch == 0 || N == 0 || ticks < 1) {
        fprintf(stderr, "usage: shared_plant_loop [batch] [knotPoints] [ticks]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N;

    // the one plant (host generation only)
    std::vector<float> hG(szG), hC(szC + 1), hg(szg * batch), hc(szc * batch);
    uint64_t seed = 1234;
    for (uint32_t k = 0; k < N; ++k) {
        spd(seed, nx, hG.data() + (size_t)k * sg);
        if (k + 1 < N) {
            spd(seed, nu, hG.data() + (size_t)k * sg + nx * nx);
            float *A = hC.data() + (size_t)k * sc, *B = A + nx * nx;
            for (uint32_t i = 0; i < nx * nx; ++i) A[i] = (float)(0.5 * urand(seed) / std::sqrt((double)nx)) + (i / nx == i % nx ? 1.f : 0.f);
            for (uint32_t i = 0; i < nx * nu; ++i) B[i] = (float)(1.7 * urand(seed) / std::sqrt((double)nx));
        }
    }
    // this tick's data, every problem its own: the tracking gradients drift, the measured state c_0 moves, the affine terms c_k (k > 0) stay
    auto new_tick = [&](bool first) {
        for (uint32_t b = 0; b < batch; ++b) {
            for (size_t i = 0; i < szg; ++i) hg[b * szg + i] = (first ? 0.f : 0.9f * hg[b * szg + i]) + (first ? 1.7f : 0.17f) * (float)urand(seed);
            for (size_t i = 0; i < szc; ++i)
                if (first) hc[b * szc + i] = 0.17f * (float)urand(seed);
                else if (i < nx) hc[b * szc + i] = 0.9f * hc[b * szc + i] + 0.05f * (float)urand(seed);
        }
    };

    // the plant's matrices once; the vectors per problem
    float *dG, *dC, *dg, *dc, *dS, *dgam, *dGi, *dP, *dl, *dz;
    uint32_t *d_iters;
    uint8_t *d_flags;
    CK(hipMalloc((void **)&dG, szG * 4));
    CK(hipMalloc((void **)&dC, (szC + 1) * 4));
    CK(hipMalloc((void **)&dS, szS * 4));
    CK(hipMalloc((void **)&dGi, szG * 4));
    CK(hipMalloc((void **)&dP, szS * 4));
    CK(hipMalloc((void **)&dg, szg * batch * 4));
    CK(hipMalloc((void **)&dc, szc * batch * 4));
    CK(hipMalloc((void **)&dgam, szc * batch * 4));
    CK(hipMalloc((void **)&dl, szc * batch * 4));
    CK(hipMalloc((void **)&dz, szg * batch * 4));
    CK(hipMalloc((void **)&d_iters, batch * 4));
    CK(hipMalloc((void **)&d_flags, batch));
    CK(hipMemcpy(dG, hG.data(), szG * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dl, 0, szc * batch * 4));
    hipStream_t stream;
    CK(hipStreamCreate(&stream));

    std::vector<float> hz(szg), hl(szc);
    std::vector<uint32_t> hi(batch);
    std::vector<uint8_t> hf(batch);
    bool bad = false;
    // counts and flags of every problem, the KKT residuals of problems first, first + step, ... (at most four)
    auto report = [&](const char *what, int tick, double ms, uint32_t count, uint32_t first) -> int {
        CK(hipMemcpy(hi.data(), d_iters, count * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hf.data(), d_flags, count, hipMemcpyDeviceToHost));
        double it = 0;
        uint32_t ran_out = 0;
        for (uint32_t i = 0; i < count; ++i) {
            it += hi[i];
            ran_out += hf[i] != 0;
        }
        printf("%s %d: %.3f ms for %u KKT systems on one plant, %.1f PCG iterations on average, %u ran out\n", what, tick, ms, count,
               it / count, ran_out);
        if (ran_out) bad = true;
        const uint32_t step = count / 4 ? count / 4 : 1;
        for (uint32_t b = first % count; b < count; b += step) {
            CK(hipMemcpy(hz.data(), dz + b * szg, szg * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hl.data(), dl + b * szc, szc * 4, hipMemcpyDeviceToHost));
            const Residuals r = kkt_residuals(N, hG.data(), hC.data(), hg.data() + b * szg, hc.data() + b * szc, hz.data(), hl.data());
            printf("    problem %u: stationarity %.2e, feasibility %.2e\n", b, r.stationarity, r.feasibility);
            if (!(r.stationarity < 1e-3) || !(r.feasibility < 1e-3)) bad = true;
        }
        return 0;
    };

    // the factorisation: kktStep at batch 1 on the plant and the first problem's vectors writes S, G^-1 and Phi^-1, never written again
    pcg_config<float> cfg;
    cfg.pcg_exit_tol = 1e-10f;
    cfg.pcg_max_iter = 200;
    new_tick(true);
    CK(hipMemcpy(dg, hg.data(), szg * batch * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), szc * batch * 4, hipMemcpyHostToDevice));
    auto t0 = std::chrono::steady_clock::now();
    kktStep<float>(nx, nu, N, 1, dG, dC, dg, dc, dS, dgam, dGi, dP, dl, dz, d_iters, d_flags, &cfg, stream);
    CK(hipStreamSynchronize(stream));
    double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (report("factor", 0, ms, 1, 0)) return 1;

    gbdpcg_handle_t h = gbdpcg_detail::handle();   // the handle kktStep<T> works on
    GK(gbdpcg_set_symmetric(h, 1));                // S and Phi^-1 stay as the device wrote them: symmetric in storage
    // tick 0 of the whole batch as a plain call ...
    CK(hipMemsetAsync(dl, 0, szc * batch * 4, stream));
    t0 = std::chrono::steady_clock::now();
    kktResolveShared<float>(nx, nu, N, batch, dGi, dC, dg, dc, dS, dP, dgam, dl, dz, d_iters, d_flags, &cfg, stream);
    CK(hipStreamSynchronize(stream));
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (report("tick", 0, ms, batch, 0)) return 1;
    // ... and the ticks after it as replays of one graph
    gbdpcg_graph_t graph;
    GK(gbdpcg_graph_create_kkt_resolve_shared_f32(h, nx, nu, N, batch, dGi, dC, dg, dc, dS, dP, dgam, dl, nullptr, nullptr,
                                                  cfg.pcg_exit_tol, cfg.pcg_max_iter, d_iters, d_flags, dz, &graph));
    for (int t = 1; t <= ticks; ++t) {
        new_tick(false);
        CK(hipMemcpyAsync(dg, hg.data(), szg * batch * 4, hipMemcpyHostToDevice, stream));
        CK(hipMemcpyAsync(dc, hc.data(), szc * batch * 4, hipMemcpyHostToDevice, stream));
        CK(hipStreamSynchronize(stream));
        t0 = std::chrono::steady_clock::now();
        GK(gbdpcg_graph_launch(graph, stream));
        CK(hipStreamSynchronize(stream));
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (t == ticks || t == 1) {
            if (report("tick", t, ms, batch, (uint32_t)t)) return 1;
        } else {
            printf("tick %d: %.3f ms\n", t, ms);
        }
    }
    gbdpcg_graph_destroy(graph);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)dS, (void *)dgam, (void *)dGi, (void *)dP, (void *)dl, (void *)dz,
                    (void *)d_iters, (void *)d_flags})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
