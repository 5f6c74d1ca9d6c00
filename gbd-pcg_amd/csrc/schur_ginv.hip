// schur_ginv.hip -- the two steps that apply the G^-1 form_schur stored (the conventions are those of
// schur.hip's head and include/gbdpcg.h):
//   recover_primal : lambda -> z = -G^-1 (g + C' lambda)
//   form_gamma     : G^-1, C and NEW g, c -> gamma alone, for a linearisation that is kept
// Each has an any-size kernel (one wavefront per row (problem, k), blocks staged in LDS) and a four-rows-per-wave kernel for the
// block sizes of GBDPCG_QUAD_SHAPES (schur_common.hpp); the two give the same bits.
#include "row16.hpp"
#include "schur_common.hpp"

namespace gbdpcg {

// z = -G^-1 (g + C' lambda): x_k = -Q_k^-1 (q_k + lambda_k - A_k' lambda_{k+1}),  u_k = -R_k^-1 (r_k - B_k' lambda_{k+1}).
// SHARED (here and in the three kernels below; gbdpcg_recover_primal_shared_*, gbdpcg_form_gamma_shared_*): Ginv and C are ONE
// problem's blocks, read with a zero problem stride by every problem of the batch -- the same fma chains, the same bits.
template <typename T, bool SHARED = false>
__global__ __launch_bounds__(256) void schur_recover_kernel(uint32_t nx, uint32_t nu, uint32_t N, uint64_t rows,
                                                           const T *__restrict__ Ginv, const T *__restrict__ C,
                                                           const T *__restrict__ g, const T *__restrict__ lambda, T *__restrict__ z)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (row >= rows) return;
    const KktDims d(nx, nu, N);
    const uint64_t prob = row / N;
    const uint32_t k = (uint32_t)(row - prob * N);
    const uint32_t nn = nx * nx, uu = nu * nu, xu = nx * nu;
    const bool has_next = k + 1 < N;

    T *Qi = reinterpret_cast<T *>(smem_raw) + (size_t)wave * recover_wave_elems(nx, nu);
    T *A = Qi + nn, *Ri = A + nn, *B = Ri + uu, *ln = B + xu, *tx = ln + nx, *tu = tx + 2 * nx;
    const uint64_t mprob = SHARED ? 0 : prob;   // the problem whose matrices this row reads
    const T *Gi = Ginv + mprob * d.szG + (size_t)k * d.sg, *Ck = C + mprob * d.szC + (size_t)k * d.sc;
    const T *gk = g + prob * d.szg + (size_t)k * d.sv;
    T *zk = z + prob * d.szg + (size_t)k * d.sv;

    for (uint32_t i = lane; i < nn; i += 64) Qi[i] = Gi[i];
    if (has_next) {
        for (uint32_t i = lane; i < nn; i += 64) A[i] = Ck[i];
        for (uint32_t i = lane; i < uu; i += 64) Ri[i] = Gi[nn + i];
        for (uint32_t i = lane; i < xu; i += 64) B[i] = Ck[nn + i];
        for (uint32_t i = lane; i < nx; i += 64) ln[i] = lambda[(size_t)(row + 1) * nx + i];
    }
    wave_sync();
    for (uint32_t r = lane; r < nx; r += 64) {
        T t = gk[r] + lambda[(size_t)row * nx + r];
        if (has_next) {
            T s = T(0);
            for (uint32_t q = 0; q < nx; ++q) s = fma_t(A[r * nx + q], ln[q], s);  // (A' lambda)_r = sum_q A(q, r) lambda_q
            t -= s;
        }
        tx[r] = t;
    }
    if (has_next)
        for (uint32_t r = lane; r < nu; r += 64) {
            T s = T(0);
            for (uint32_t q = 0; q < nx; ++q) s = fma_t(B[r * nx + q], ln[q], s);
            tu[r] = gk[nx + r] - s;
        }
    wave_sync();
    for (uint32_t r = lane; r < nx; r += 64) {
        T s = T(0);
        for (uint32_t q = 0; q < nx; ++q) s = fma_t(Qi[q * nx + r], tx[q], s);
        zk[r] = -s;
    }
    if (has_next)
        for (uint32_t r = lane; r < nu; r += 64) {
            T s = T(0);
            for (uint32_t q = 0; q < nu; ++q) s = fma_t(Ri[q * nu + r], tu[q], s);
            zk[nx + r] = -s;
        }
}

// ---- compile-time block sizes NX, NU <= 16: FOUR knots per wavefront, no LDS at all ----
// The kernel above stages every block in LDS and walks it with runtime indices (two LDS reads per fma): 172 us for the 131072
// rows of the BASELINE batch, 1.8 TB/s, on a step that moves 2.4 KB per row and has 0.5 flop per byte.  Here a 16-lane quarter
// owns one row (problem, k) and every operand goes from memory straight into the registers of the lane that multiplies it:
//   * lane l holds COLUMN l of A_k and B_k (14 contiguous elements each: (A' lambda+)_l and (B' lambda+)_l are dot products along
//     a column) and ROW l of Q_k^-1 and R_k^-1 (element q of it comes with the quarter's q-th load: 14 lanes x 4 bytes, contiguous);
//   * the vector a product multiplies sits one entry per lane (lambda_{k+1}; then t_x, t_u where they were computed) and reaches
//     the fma as a DPP row broadcast -- no LDS, no shuffles through the crossbar;
//   * every load of a row is requested before the first fma (53 registers of operands per lane), five or six waves per SIMD keep
//     ~200 KB per compute unit in flight.
// Same sums in the same order as the kernel above (q ascending, one fma chain per output entry): bit-identical results.
template <typename T, int NX, int NU, bool SHARED = false>
__global__ __launch_bounds__(256) void schur_recover_quad_kernel(uint32_t N, uint64_t rows, const T *__restrict__ Ginv,
                                                                const T *__restrict__ C, const T *__restrict__ g,
                                                                const T *__restrict__ lambda, T *__restrict__ z)
{
    static_assert(NX <= 16 && NU <= NX, "one row per 16-lane quarter");
    uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = lane & 15u;
    const uint64_t row = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const bool live = row < rows;
    const KktDims d(NX, NU, N);
    const uint64_t prob = live ? row / N : 0;
    const uint32_t k = live ? (uint32_t)(row - prob * N) : 0u;
    const bool has_next = live && k + 1 < N;
    const bool lx = live && l < NX, lu = has_next && l < NU;
    const uint32_t cx = l < NX ? l : 0u, cu = l < NU ? l : 0u;   // clamped: idle lanes read what a live lane reads
    const uint64_t mprob = SHARED ? 0 : prob;
    const T *Gi = Ginv + mprob * d.szG + (size_t)k * d.sg, *Ck = C + mprob * d.szC + (size_t)k * d.sc;
    const T *gk = g + prob * d.szg + (size_t)k * d.sv;
    const T *lk = lambda + (prob * N + k) * NX;

    T a[NX], b[NX], qi[NX], ri[NU];
    T lam_n = T(0), tx = T(0), tu = T(0);
    if (live) {
        tx = gk[cx] + lk[cx];
#pragma unroll
        for (int q = 0; q < NX; ++q) qi[q] = Gi[q * NX + cx];
    } else {
#pragma unroll
        for (int q = 0; q < NX; ++q) qi[q] = T(0);
    }
    if (has_next) {
        lam_n = lk[NX + cx];
        tu = gk[NX + cu];
#pragma unroll
        for (int q = 0; q < NX; ++q) {
            a[q] = Ck[cx * NX + q];
            b[q] = Ck[NX * NX + cu * NX + q];
        }
#pragma unroll
        for (int q = 0; q < NU; ++q) ri[q] = Gi[NX * NX + q * NU + cu];
    } else {
#pragma unroll
        for (int q = 0; q < NX; ++q) a[q] = b[q] = T(0);
#pragma unroll
        for (int q = 0; q < NU; ++q) ri[q] = T(0);
    }
    // t_x = q_k + lambda_k - A_k' lambda_{k+1},  t_u = r_k - B_k' lambda_{k+1}   (the rows of the last knot have neither product)
    T sa = T(0), sb = T(0);
    recover_dot<0, NX>(sa, a, lam_n);
    recover_dot<0, NX>(sb, b, lam_n);
    if (has_next) {
        tx -= sa;
        tu -= sb;
    }
    // x_k = -Q_k^-1 t_x,  u_k = -R_k^-1 t_u
    T sx = T(0), su = T(0);
    recover_dot<0, NX>(sx, qi, tx);
    recover_dot<0, NU>(su, ri, tu);
    T *zk = z + prob * d.szg + (size_t)k * d.sv;
    if (lx) zk[l] = -sx;
    if (lu) zk[NX + l] = -su;
}

// ---- gamma alone, for a frozen linearisation (G, C unchanged since the last form_schur: S, Phi^-1 and G^-1 stand, only g and c
// are new): gamma = -(c + C G^-1 g) from the stored G^-1, nothing inverted, S neither read nor written.
//     w_k = Q_k^-1 q_k,  v_k = R_k^-1 r_k,  t_k = A_k w_k + B_k v_k,      gamma_0 = -(c_0 + w_0),  gamma_k = -((c_k + w_k) - t_{k-1})
// Every entry is one fma chain from zero with q ascending (t: the columns of A, then those of B, in one chain), in both kernels
// below: their results are bit-identical, as those of the recovery pair are.
// Any block size: one wavefront per row (problem, k), blocks staged in LDS.
template <typename T, bool SHARED = false>
__global__ __launch_bounds__(256) void schur_gamma_kernel(uint32_t nx, uint32_t nu, uint32_t N, uint64_t rows,
                                                         const T *__restrict__ Ginv, const T *__restrict__ C,
                                                         const T *__restrict__ g, const T *__restrict__ c, T *__restrict__ gamma)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (row >= rows) return;  // whole wave
    const KktDims d(nx, nu, N);
    const uint64_t prob = row / N;
    const uint32_t k = (uint32_t)(row - prob * N);
    const uint32_t nn = nx * nx, uu = nu * nu, xu = nx * nu;
    const bool has_prev = k > 0;

    T *Qc = reinterpret_cast<T *>(smem_raw) + (size_t)wave * gamma_wave_elems(nx, nu);
    T *Qp = Qc + nn, *Ap = Qp + nn, *Rp = Ap + nn, *Bp = Rp + uu;
    T *qc = Bp + xu, *qp = qc + nx, *wp = qp + nx, *rp = wp + 2 * nx, *vp = rp + nu;
    const uint64_t mprob = SHARED ? 0 : prob;
    const T *Gp = Ginv + mprob * d.szG, *gp = g + prob * d.szg;

    for (uint32_t i = lane; i < nn; i += 64) Qc[i] = Gp[(size_t)k * d.sg + i];
    for (uint32_t i = lane; i < nx; i += 64) qc[i] = gp[(size_t)k * d.sv + i];
    if (has_prev) {
        const uint32_t j = k - 1;
        const T *Gj = Gp + (size_t)j * d.sg, *Cj = C + mprob * d.szC + (size_t)j * d.sc, *gj = gp + (size_t)j * d.sv;
        for (uint32_t i = lane; i < nn; i += 64) {
            Qp[i] = Gj[i];
            Ap[i] = Cj[i];
        }
        for (uint32_t i = lane; i < uu; i += 64) Rp[i] = Gj[nn + i];
        for (uint32_t i = lane; i < xu; i += 64) Bp[i] = Cj[nn + i];
        for (uint32_t i = lane; i < nx; i += 64) qp[i] = gj[i];
        for (uint32_t i = lane; i < nu; i += 64) rp[i] = gj[nx + i];
    }
    wave_sync();
    if (has_prev) {
        for (uint32_t r = lane; r < nx; r += 64) {
            T s = T(0);
            for (uint32_t q = 0; q < nx; ++q) s = fma_t(Qp[q * nx + r], qp[q], s);
            wp[r] = s;
        }
        for (uint32_t r = lane; r < nu; r += 64) {
            T s = T(0);
            for (uint32_t q = 0; q < nu; ++q) s = fma_t(Rp[q * nu + r], rp[q], s);
            vp[r] = s;
        }
    }
    wave_sync();
    for (uint32_t r = lane; r < nx; r += 64) {
        T w = T(0);
        for (uint32_t q = 0; q < nx; ++q) w = fma_t(Qc[q * nx + r], qc[q], w);
        T v = c[(size_t)row * nx + r] + w;
        if (has_prev) {
            T t = T(0);
            for (uint32_t q = 0; q < nx; ++q) t = fma_t(Ap[q * nx + r], wp[q], t);
            for (uint32_t q = 0; q < nu; ++q) t = fma_t(Bp[q * nx + r], vp[q], t);
            v -= t;
        }
        gamma[(size_t)row * nx + r] = -v;
    }
}

namespace {

// The value the same lane of the 16-lane quarter BEFORE this one holds (quarter 0 gets quarter 3's): a permute between vector
// registers through the LDS crossbar -- no LDS is allocated or addressed.  Every lane of the wave must be active.
__device__ __forceinline__ float prev_quarter(float v, uint32_t lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)(((lane + 48u) & 63u) * 4u), __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double prev_quarter(double v, uint32_t lane)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int a = (int)(((lane + 48u) & 63u) * 4u);
    const int lo = __builtin_amdgcn_ds_bpermute(a, (int)(b & 0xffffffffll));
    const int hi = __builtin_amdgcn_ds_bpermute(a, (int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// The operands of one knot in the lanes of one quarter, as schur_recover_quad_kernel holds them: lane l has ROW l of Q^-1, R^-1,
// A and B (element q of a row comes with the quarter's q-th load: contiguous across the lanes) and entry l of q and r.
// full: the knot has R^-1, r, A, B (every knot but a problem's last); on == false: nothing is read, everything is zero.
template <typename T, int NX, int NU>
__device__ __forceinline__ void gamma_knot_load(T (&qi)[NX], T (&a)[NX], T (&ri)[NU], T (&b)[NU], T &qv, T &rv, const T *__restrict__ Gi,
                                                const T *__restrict__ Ck, const T *__restrict__ gk, uint32_t cx, uint32_t cu, bool on,
                                                bool full)
{
    if (on) {
        qv = gk[cx];
#pragma unroll
        for (int q = 0; q < NX; ++q) qi[q] = Gi[q * NX + cx];
    } else {
        qv = T(0);
#pragma unroll
        for (int q = 0; q < NX; ++q) qi[q] = T(0);
    }
    if (on && full) {
        rv = gk[NX + cu];
#pragma unroll
        for (int q = 0; q < NX; ++q) a[q] = Ck[q * NX + cx];
#pragma unroll
        for (int q = 0; q < NU; ++q) ri[q] = Gi[NX * NX + q * NU + cu];
#pragma unroll
        for (int q = 0; q < NU; ++q) b[q] = Ck[NX * NX + q * NX + cx];
    } else {
        rv = T(0);
#pragma unroll
        for (int q = 0; q < NX; ++q) a[q] = T(0);
#pragma unroll
        for (int q = 0; q < NU; ++q) ri[q] = T(0);
#pragma unroll
        for (int q = 0; q < NU; ++q) b[q] = T(0);
    }
}
// w = Q^-1 q (entry l in lane l) and t = A w + B R^-1 r
template <typename T, int NX, int NU>
__device__ __forceinline__ void gamma_knot_products(const T (&qi)[NX], const T (&a)[NX], const T (&ri)[NU], const T (&b)[NU], T qv, T rv,
                                                    T &w, T &t)
{
    T v = T(0);
    w = T(0);
    t = T(0);
    recover_dot<0, NX>(w, qi, qv);
    recover_dot<0, NU>(v, ri, rv);
    recover_dot<0, NX>(t, a, w);
    recover_dot<0, NU>(t, b, v);
}

}  // namespace

// ---- compile-time block sizes: FOUR rows per wavefront, one per 16-lane quarter, no LDS (the form of schur_recover_quad_kernel).
// Every block of G^-1 and C is read ONCE: the quarter of row k forms w_k and t_k = A_k w_k + B_k v_k from the blocks of its own
// knot, and t_k goes to the quarter of row k+1 as a permute inside the wave.  The first quarter of a wave has no quarter before it:
// it reads the blocks of knot k-1 as well and forms t_{k-1} itself (the same chains on the same numbers as the wave before it) --
// 1.25 x the bytes of Q^-1, R^-1, A, B per wave instead of the 2 x of rows that each read both knots.  Every load of a row is
// requested before the first fma; the products of the second knot run in all quarters on zeros (the kernel waits on memory, and
// no DPP operand is read under a partial exec mask that way).
// 1024 x 128 rows at nx 14, nu 7: 87 us in fp32 (307 MB, 3.5 TB/s; 104 registers, four waves per SIMD), 135 us in fp64; 31 us at
// 12 / 4 (6.5 TB/s) -- profiles/r05_resolve.txt.
template <typename T, int NX, int NU, bool SHARED = false>
__global__ __launch_bounds__(256) void schur_gamma_quad_kernel(uint32_t N, uint64_t rows, const T *__restrict__ Ginv,
                                                              const T *__restrict__ C, const T *__restrict__ g,
                                                              const T *__restrict__ c, T *__restrict__ gamma)
{
    static_assert(NX <= 16 && NU <= NX, "one row per 16-lane quarter");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = lane & 15u, qd = lane >> 4;
    const uint64_t row = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4 + qd;
    const bool live = row < rows;
    const KktDims d(NX, NU, N);
    const uint64_t prob = live ? row / N : 0;
    const uint32_t k = live ? (uint32_t)(row - prob * N) : 0u;
    const bool has_next = live && k + 1 < N, has_prev = live && k > 0;
    const bool first = has_prev && qd == 0;                      // no quarter before this one holds t_{k-1}
    const uint32_t cx = l < NX ? l : 0u, cu = l < NU ? l : 0u;   // clamped: idle lanes read what a live lane reads
    const uint32_t j = first ? k - 1 : k;
    const uint64_t mprob = SHARED ? 0 : prob;
    const T *Gp = Ginv + mprob * d.szG, *Cp = C + mprob * d.szC, *gp = g + prob * d.szg;

    T qi[NX], a[NX], ri[NU], b[NU], qv, rv;       // this row's knot
    T qib[NX], ab[NX], rib[NU], bb[NU], qvb, rvb;  // the knot before it (first quarter only)
    gamma_knot_load<T, NX, NU>(qi, a, ri, b, qv, rv, Gp + (size_t)k * d.sg, Cp + (size_t)k * d.sc, gp + (size_t)k * d.sv, cx, cu, live, has_next);
    gamma_knot_load<T, NX, NU>(qib, ab, rib, bb, qvb, rvb, Gp + (size_t)j * d.sg, Cp + (size_t)j * d.sc, gp + (size_t)j * d.sv, cx, cu, first, true);
    const T ck = live ? c[(prob * N + k) * NX + cx] : T(0);

    T w, t, wb, tb;
    gamma_knot_products<T, NX, NU>(qi, a, ri, b, qv, rv, w, t);
    gamma_knot_products<T, NX, NU>(qib, ab, rib, bb, qvb, rvb, wb, tb);
    const T tp = prev_quarter(t, lane);
    T v = ck + w;
    if (has_prev) v -= first ? tb : tp;
    if (live && l < NX) gamma[(prob * N + k) * NX + l] = -v;
}

// (shared: the SHARED instantiations; the same launch geometry either way)
template <typename T>
hipError_t launch_recover_primal(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *Ginv,
                                 const T *C, const T *g, const T *lambda, T *z, hipStream_t s, bool shared)
{
    const uint64_t rows = (uint64_t)batch * N, quad_grid = (rows + 15) / 16;   // 4 waves x 4 rows per workgroup
    hipError_t st;
    if (quad_dispatch(nx, nu, quad_grid, st, [&](auto NX, auto NU) {
            auto kern = shared ? schur_recover_quad_kernel<T, NX(), NU(), true> : schur_recover_quad_kernel<T, NX(), NU()>;
            hipLaunchKernelGGL(kern, dim3((uint32_t)quad_grid), dim3(256), 0, s, N, rows, Ginv, C, g, lambda, z);
            return hipGetLastError();
        }))
        return st;
    return launch_lds_rows(dev, shared ? schur_recover_kernel<T, true> : schur_recover_kernel<T>,
                           (size_t)recover_wave_elems(nx, nu) * sizeof(T), [&](uint32_t waves) { return (rows + waves - 1) / waves; }, s,
                           nx, nu, N, rows, Ginv, C, g, lambda, z);
}

template <typename T>
hipError_t launch_form_gamma(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *Ginv, const T *C,
                             const T *g, const T *c, T *gamma, hipStream_t s, bool shared)
{
    const uint64_t rows = (uint64_t)batch * N, quad_grid = (rows + 15) / 16;   // 4 waves x 4 rows per workgroup
    hipError_t st;
    if (quad_dispatch(nx, nu, quad_grid, st, [&](auto NX, auto NU) {
            auto kern = shared ? schur_gamma_quad_kernel<T, NX(), NU(), true> : schur_gamma_quad_kernel<T, NX(), NU()>;
            hipLaunchKernelGGL(kern, dim3((uint32_t)quad_grid), dim3(256), 0, s, N, rows, Ginv, C, g, c, gamma);
            return hipGetLastError();
        }))
        return st;
    return launch_lds_rows(dev, shared ? schur_gamma_kernel<T, true> : schur_gamma_kernel<T>,
                           (size_t)gamma_wave_elems(nx, nu) * sizeof(T), [&](uint32_t waves) { return (rows + waves - 1) / waves; }, s,
                           nx, nu, N, rows, Ginv, C, g, c, gamma);
}

template hipError_t launch_recover_primal<float>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, uint32_t, const float *,
                                                 const float *, const float *, const float *, float *, hipStream_t, bool);
template hipError_t launch_recover_primal<double>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                  const double *, const double *, const double *, double *, hipStream_t, bool);
template hipError_t launch_form_gamma<float>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                             const float *, const float *, float *, hipStream_t, bool);
template hipError_t launch_form_gamma<double>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                              const double *, const double *, const double *, double *, hipStream_t, bool);

}  // namespace gbdpcg
