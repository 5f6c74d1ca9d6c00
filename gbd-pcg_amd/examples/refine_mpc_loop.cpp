// Linear MPC on a kept linearisation with fp64 answers from fp32 solves (include/gbdpcg.h, gbdpcg_kkt_refine_step):
//
//   once      : fp64 KKT blocks on the device; gbdpcg_demote_f32 of G, C (and one g, c); ONE gbdpcg_kkt_step_f32 factors the fp32
//               copy (S, G^-1, Phi^-1 are kept); ONE executable graph of
//               { fp64 defect of (z, lambda) -> scaled fp32 right-hand side ; gamma ; PCG ; primal step ; fp64 accumulation }
//   per tick  : new g and c in fp64 (the measured state enters through c_0), z and lambda of the previous tick stay as the
//               start, the graph is replayed until both norms of every problem are below the stop values; the norms the step
//               STARTED from come back with every replay and are printed
//
// usage: refine_mpc_loop [batch=1024] [knotPoints=128] [ticks=3] [maxSteps=8]      (stateSize 14, controlSize 7)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gbdpcg.h"

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
constexpr uint32_t nx = 14, nu = 7;
constexpr uint32_t sg = nx * nx + nu * nu, sc = nx * nx + nx * nu, sv = nx + nu;

// M M' / m + I, column-major m x m, in fp64 (not fp32-representable)
void spd(std::mt19937 &rng, uint32_t m, double *out)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::vector<double> a(m * m);
    for (auto &v : a) v = nd(rng);
    for (uint32_t c = 0; c < m; ++c)
        for (uint32_t r = 0; r < m; ++r) {
            double s = r == c ? 1.0 : 0.0;
            for (uint32_t q = 0; q < m; ++q) s += a[q * m + r] * a[q * m + c] / m;
            out[c * m + r] = s;
        }
}
template <typename T> hipError_t dev_alloc(T **p, size_t count) { return hipMalloc((void **)p, (count ? count : 1) * sizeof(T)); }
}  // namespace

int main(int argc, char **argv)
{
    const uint32_t batch = argc > 1 ? (uint32_t)atoi(argv[1]) : 1024, N = argc > 2 ? (uint32_t)atoi(argv[2]) : 128;
    const int ticks = argc > 3 ? atoi(argv[3]) : 3, max_steps = argc > 4 ? atoi(argv[4]) : 8;
    if (batch == 0 || N == 0 || ticks < 1 || max_steps < 1) {
        fprintf(stderr, "usage: refine_mpc_loop [batch] [knotPoints] [ticks] [maxSteps]\n");
        return 2;
    }
    const size_t szG = (size_t)sg * N - nu * nu, szC = (size_t)sc * (N - 1), szg = (size_t)sv * N - nu, szc = (size_t)nx * N;
    const size_t szS = (size_t)3 * nx * nx * N;
    const double stop_s = 1e-11, stop_f = 1e-11;   // absolute, on data of order 1: four digits past what fp32 carries

    const uint32_t distinct = std::min(batch, 8u);
    std::vector<double> hG(szG * batch), hC(szC * batch + 1), hg(szg * batch), hc(szc * batch);
    std::mt19937 rng(1234);
    std::normal_distribution<double> nd(0.0, 1.0);
    for (uint32_t b = 0; b < distinct; ++b) {
        double *G = hG.data() + b * szG, *C = hC.data() + b * szC;
        for (uint32_t k = 0; k < N; ++k) {
            spd(rng, nx, G + (size_t)k * sg);
            if (k + 1 < N) {
                spd(rng, nu, G + (size_t)k * sg + nx * nx);
                double *A = C + (size_t)k * sc, *B = A + nx * nx;
                for (uint32_t i = 0; i < nx * nx; ++i) A[i] = 0.3 * nd(rng) / std::sqrt((double)nx) + (i / nx == i % nx ? 1.0 : 0.0);
                for (uint32_t i = 0; i < nx * nu; ++i) B[i] = nd(rng) / std::sqrt((double)nx);
            }
        }
    }
    for (uint32_t b = distinct; b < batch; ++b) {
        std::copy(hG.begin() + (b % distinct) * szG, hG.begin() + (b % distinct + 1) * szG, hG.begin() + b * szG);
        std::copy(hC.begin() + (b % distinct) * szC, hC.begin() + (b % distinct + 1) * szC, hC.begin() + b * szC);
    }

    double *dG, *dC, *dg, *dc, *dz, *dl, *dres;
    float *dG32, *dC32, *dg32, *dc32, *dS, *dGi, *dP, *drg, *drc, *dgam, *ddl, *ddz;
    int32_t *dexpo;
    uint32_t *d_iters;
    uint8_t *d_flags;
    CK(dev_alloc(&dG, szG * batch));
    CK(dev_alloc(&dC, szC * batch));
    CK(dev_alloc(&dg, szg * batch));
    CK(dev_alloc(&dc, szc * batch));
    CK(dev_alloc(&dz, szg * batch));
    CK(dev_alloc(&dl, szc * batch));
    CK(dev_alloc(&dres, (size_t)2 * batch));
    CK(dev_alloc(&dG32, szG * batch));
    CK(dev_alloc(&dC32, szC * batch));
    CK(dev_alloc(&dg32, szg * batch));
    CK(dev_alloc(&dc32, szc * batch));
    CK(dev_alloc(&dS, szS * batch));
    CK(dev_alloc(&dGi, szG * batch));
    CK(dev_alloc(&dP, szS * batch));
    CK(dev_alloc(&drg, szg * batch));
    CK(dev_alloc(&drc, szc * batch));
    CK(dev_alloc(&dgam, szc * batch));
    CK(dev_alloc(&ddl, szc * batch));
    CK(dev_alloc(&ddz, szg * batch));
    CK(dev_alloc(&dexpo, batch));
    CK(dev_alloc(&d_iters, batch));
    CK(dev_alloc(&d_flags, batch));
    CK(hipMemcpy(dG, hG.data(), szG * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, hC.data(), szC * batch * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dg, 0, szg * batch * 8));
    CK(hipMemset(dc, 0, szc * batch * 8));
    CK(hipMemset(dz, 0, szg * batch * 8));
    CK(hipMemset(dl, 0, szc * batch * 8));
    CK(hipMemset(ddl, 0, szc * batch * 4));

    gbdpcg_handle_t h;
    GK(gbdpcg_create(&h, 0));
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    // the kept factorisation: fp32 copies, one fp32 step (its own solution, of g = c = 0, is not used)
    GK(gbdpcg_demote_f32(h, szG * batch, dG, dG32, stream));
    if (N > 1) GK(gbdpcg_demote_f32(h, szC * batch, dC, dC32, stream));
    GK(gbdpcg_demote_f32(h, szg * batch, dg, dg32, stream));
    GK(gbdpcg_demote_f32(h, szc * batch, dc, dc32, stream));
    GK(gbdpcg_kkt_step_f32(h, nx, nu, N, batch, dG32, dC32, dg32, dc32, dS, dgam, dGi, dP, GBDPCG_PINV_STAIR, ddl, nullptr, nullptr, 1e-6f, 1,
                           d_iters, d_flags, ddz, stream));
    CK(hipStreamSynchronize(stream));
    gbdpcg_graph_t graph;
    GK(gbdpcg_graph_create_kkt_refine_step(h, nx, nu, N, batch, dG, dC, dg, dc, dGi, dC32, dS, dP, drg, drc, dgam, ddl, nullptr, nullptr, ddz,
                                           1e-8f, 100, d_iters, d_flags, dexpo, dz, dl, dres, &graph));

    std::vector<double> hres((size_t)2 * batch);
    int bad = 0;
    for (int t = 0; t < ticks; ++t) {
        for (uint32_t b = 0; b < distinct; ++b) {
            for (size_t i = 0; i < szg; ++i) hg[b * szg + i] = (t == 0 ? 0.0 : 0.9 * hg[b * szg + i]) + (t == 0 ? 1.0 : 0.1) * nd(rng);
            for (size_t i = 0; i < szc; ++i) hc[b * szc + i] = (t == 0 ? 0.0 : 0.9 * hc[b * szc + i]) + (t == 0 ? 0.1 : 0.01) * nd(rng);
        }
        for (uint32_t b = distinct; b < batch; ++b) {
            std::copy(hg.begin() + (b % distinct) * szg, hg.begin() + (b % distinct + 1) * szg, hg.begin() + b * szg);
            std::copy(hc.begin() + (b % distinct) * szc, hc.begin() + (b % distinct + 1) * szc, hc.begin() + b * szc);
        }
        CK(hipMemcpyAsync(dg, hg.data(), szg * batch * 8, hipMemcpyHostToDevice, stream));
        CK(hipMemcpyAsync(dc, hc.data(), szc * batch * 8, hipMemcpyHostToDevice, stream));
        CK(hipStreamSynchronize(stream));
        bool done = false;
        const auto t0 = std::chrono::steady_clock::now();
        for (int s = 0; s <= max_steps && !done; ++s) {
            GK(gbdpcg_graph_launch(graph, stream));
            CK(hipMemcpyAsync(hres.data(), dres, hres.size() * 8, hipMemcpyDeviceToHost, stream));
            CK(hipStreamSynchronize(stream));
            double ms = 0, mf = 0;
            for (uint32_t b = 0; b < batch; ++b) {
                ms = hres[2 * b] > ms || std::isnan(hres[2 * b]) ? hres[2 * b] : ms;
                mf = hres[2 * b + 1] > mf || std::isnan(hres[2 * b + 1]) ? hres[2 * b + 1] : mf;
            }
            printf("tick %d, in front of step %d: stationarity %.3e, feasibility %.3e (max over %u problems)\n", t, s, ms, mf, batch);
            done = ms <= stop_s && mf <= stop_f;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("tick %d: %s in %.3f ms\n", t, done ? "converged" : "NOT converged", ms);
        if (!done) ++bad;
    }
    gbdpcg_graph_destroy(graph);
    gbdpcg_destroy(h);
    for (void *p : {(void *)dG, (void *)dC, (void *)dg, (void *)dc, (void *)dz, (void *)dl, (void *)dres, (void *)dG32, (void *)dC32,
                    (void *)dg32, (void *)dc32, (void *)dS, (void *)dGi, (void *)dP, (void *)drg, (void *)drc, (void *)dgam, (void *)ddl,
                    (void *)ddz, (void *)dexpo, (void *)d_iters, (void *)d_flags})
        (void)hipFree(p);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
