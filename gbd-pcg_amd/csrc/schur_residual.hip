// schur_residual.hip -- the KKT residual norms of a point (z, lambda) (the packed layout is that of
// schur.hip's head and include/gbdpcg.h):
//   kkt_residual : G, C, g, c and (z, lambda) -> ||G z + g + C' lambda||_inf and ||C z - c||_inf per problem
// An any-size kernel (blocks staged in LDS) and a four-rows-per-wave kernel for the block sizes of GBDPCG_QUAD_SHAPES
// (schur_common.hpp); the two give the same bits.
#include "norm_fold.hpp"
#include "row16.hpp"
#include "schur_common.hpp"

namespace gbdpcg {

// ---- KKT residual norms of a point (z, lambda), two numbers per problem: what an outer loop terminates on.
//     res[2b]   = || G z + g + C' lambda ||_inf     stationarity
//     res[2b+1] = || C z - c ||_inf                 feasibility
// Row (problem, k) evaluates the stationarity of knot k and the feasibility of knot k+1 (A_k and B_k serve both; row 0 also takes
// x_0 - c_0; the last knot has neither product and no u).  Every entry is ONE fma chain, q ascending, in this order of terms:
//     x-part, entry r:   s = q_k[r] + lambda_k[r];            s = fma(Q_k(r,q), x_k[q], s), q < nx;   s = fma(A_k(q,r), -lambda_{k+1}[q], s), q < nx
//     u-part, entry r:   s = r_k[r];                          s = fma(R_k(r,q), u_k[q], s), q < nu;   s = fma(B_k(q,r), -lambda_{k+1}[q], s), q < nx
//     knot 0, entry r:   f = x_0[r] - c_0[r]
//     knot k+1, entry r: f = x_{k+1}[r] - c_{k+1}[r];         f = fma(A_k(r,q), -x_k[q], f), q < nx;  f = fma(B_k(r,q), -u_k[q], f), q < nu
// in both kernels below (the negation of a vector entry is exact), so the entries agree bit for bit, and the maximum of their
// magnitudes is exact in any fold order: the two kernels give the same bits.
// REG (gbdpcg_kkt_residual_reg_*): Q_k(r,r) and R_k(r,r) enter their chains as fl(d + rho_b), as the formation kernels take them:
// the stationarity of the regularised system (G + rho I) z + g + C' lambda; the feasibility rows do not contain G.
// The maximum runs over the BIT PATTERN of |entry| as an unsigned integer: that orders the non-negative numbers as they are
// ordered, puts Inf above them and every NaN above Inf -- a NaN anywhere in a problem's residual is that problem's norm, where
// an fmax would drop it.  ONE WORKGROUP PER PROBLEM walks the problem's rows; every lane keeps two running maxima in registers,
// a wave folds them through DPP, the workgroup through one LDS slot per wave, and one lane writes the pair: one launch, nothing
// initialised beforehand, nothing read from res.  (A single problem with a long horizon runs on one compute unit.)
// (abs_bits / wave_umax / store_norms: norm_fold.hpp, shared with admm.hip)

// Any block size: one wavefront per row (problem, k), blocks staged in LDS; the waves of a workgroup share one problem's rows.
// SHARED (gbdpcg_kkt_residual_shared_*): G and C are ONE problem's blocks, read with a zero problem stride.
template <typename T, bool SHARED = false, bool REG = false>
__global__ __launch_bounds__(256) void schur_residual_kernel(uint32_t nx, uint32_t nu, uint32_t N, const T *__restrict__ G,
                                                             const T *__restrict__ C, const T *__restrict__ g, const T *__restrict__ c,
                                                             const T *__restrict__ z, const T *__restrict__ lambda, T *__restrict__ res,
                                                             const T *__restrict__ rho)   // [batch], REG only
{
    using U = decltype(abs_bits(T(0)));
    static_assert(sizeof(U) == sizeof(T), "the maxima live in the wave's own LDS block");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    const uint64_t prob = blockIdx.x;
    const KktDims d(nx, nu, N);
    const uint32_t nn = nx * nx, uu = nu * nu, xu = nx * nu, we = residual_wave_elems(nx, nu);
    T *base = reinterpret_cast<T *>(smem_raw);
    T *Q = base + (size_t)wave * we, *A = Q + nn, *R = A + nn, *B = R + uu, *xk = B + xu, *nl = xk + nx, *uk = nl + 2 * nx;
    const uint64_t mprob = SHARED ? 0 : prob;   // the problem whose matrices this workgroup reads
    const T *Gp = G + mprob * d.szG, *Cp = C + mprob * d.szC;
    const T *gp = g + prob * d.szg, *zp = z + prob * d.szg, *lp = lambda + prob * d.szc, *cp = c + prob * d.szc;

    T rb = T(0);
    if constexpr (REG) rb = rho[prob];   // (the workgroup's problem: a scalar load)

    U ms = 0, mf = 0;
    for (uint32_t k = wave; k < N; k += waves) {   // (whole waves)
        const bool has_next = k + 1 < N;
        const T *Gk = Gp + (size_t)k * d.sg, *Ck = Cp + (size_t)k * d.sc, *gk = gp + (size_t)k * d.sv, *zk = zp + (size_t)k * d.sv;
        const T *lk = lp + (size_t)k * nx, *ck = cp + (size_t)k * nx;
        wave_sync();   // the previous row has read its blocks
        if constexpr (REG) {   // (entry i of a column-major m x m block is on the diagonal where i is a multiple of m + 1)
            for (uint32_t i = lane; i < nn; i += 64) Q[i] = i % (nx + 1) == 0 ? Gk[i] + rb : Gk[i];
        } else {
            for (uint32_t i = lane; i < nn; i += 64) Q[i] = Gk[i];
        }
        for (uint32_t i = lane; i < nx; i += 64) xk[i] = zk[i];
        if (has_next) {
            for (uint32_t i = lane; i < nn; i += 64) A[i] = Ck[i];
            if constexpr (REG) {
                for (uint32_t i = lane; i < uu; i += 64) R[i] = i % (nu + 1) == 0 ? Gk[nn + i] + rb : Gk[nn + i];
            } else {
                for (uint32_t i = lane; i < uu; i += 64) R[i] = Gk[nn + i];
            }
            for (uint32_t i = lane; i < xu; i += 64) B[i] = Ck[nn + i];
            for (uint32_t i = lane; i < nx; i += 64) nl[i] = -lk[nx + i];
            for (uint32_t i = lane; i < nu; i += 64) uk[i] = zk[nx + i];
        }
        wave_sync();
        for (uint32_t r = lane; r < nx; r += 64) {
            T s = gk[r] + lk[r];
            for (uint32_t q = 0; q < nx; ++q) s = fma_t(Q[q * nx + r], xk[q], s);
            if (has_next)
                for (uint32_t q = 0; q < nx; ++q) s = fma_t(A[r * nx + q], nl[q], s);   // -(A' lambda+)_r = sum_q A(q, r) (-lambda+_q)
            ms = umax(ms, abs_bits(s));
            if (k == 0) mf = umax(mf, abs_bits(xk[r] - ck[r]));
            if (has_next) {
                T f = zk[d.sv + r] - ck[nx + r];
                for (uint32_t q = 0; q < nx; ++q) f = fma_t(A[q * nx + r], -xk[q], f);
                for (uint32_t q = 0; q < nu; ++q) f = fma_t(B[q * nx + r], -uk[q], f);
                mf = umax(mf, abs_bits(f));
            }
        }
        if (has_next)
            for (uint32_t r = lane; r < nu; r += 64) {
                T s = gk[nx + r];
                for (uint32_t q = 0; q < nu; ++q) s = fma_t(R[q * nu + r], uk[q], s);
                for (uint32_t q = 0; q < nx; ++q) s = fma_t(B[r * nx + q], nl[q], s);
                ms = umax(ms, abs_bits(s));
            }
    }
    store_norms(ms, mf, wave, lane, waves, [&](uint32_t w) { return reinterpret_cast<U *>(base + (size_t)(w + 1) * we - 2); }, res + 2 * prob);
}

// ---- compile-time block sizes: FOUR rows per wavefront, one per 16-lane quarter, operands from memory straight into registers
// (the form of schur_recover_quad_kernel); the 16 quarters of a workgroup take 16 consecutive knots of its problem per pass.
//   * lane l holds ROW l of Q_k and R_k (stationarity) and of A_k and B_k (feasibility of knot k+1: element q of a row comes with
//     the quarter's q-th load, contiguous across the lanes), and COLUMN l of A_k and B_k ((A' lambda+)_l, (B' lambda+)_l: 14
//     contiguous elements per lane) -- A_k and B_k are requested once per row; their second reading hits the cache;
//   * the vectors (x_k, u_k, -lambda_{k+1}) sit one entry per lane and reach the fma as a DPP row broadcast;
//   * every load of a pass is requested before its first fma, and nothing is computed under a partial exec mask: rows past
//     the horizon and the products the last knot does not have run on zeros and add 0 to the maxima.
// Lanes of a quarter that own no entry (l >= NX; l >= NU in the u-part) repeat lane 0's: a maximum does not mind.
// REG: the lane that holds row l adds rho_b to the l-th of its NX (NU) elements -- the index is the lane's, the registers are
// static, so the add is a select per element on a kernel that waits for memory.
template <typename T, int NX, int NU, bool SHARED = false, bool REG = false>
__global__ __launch_bounds__(256) void schur_residual_quad_kernel(uint32_t N, const T *__restrict__ G, const T *__restrict__ C,
                                                                  const T *__restrict__ g, const T *__restrict__ c,
                                                                  const T *__restrict__ z, const T *__restrict__ lambda,
                                                                  T *__restrict__ res, const T *__restrict__ rho)
{
    static_assert(NX <= 16 && NU <= NX, "one row per 16-lane quarter");
    using U = decltype(abs_bits(T(0)));
    __shared__ U slots[8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t l = lane & 15u, qd = lane >> 4;
    const uint64_t prob = blockIdx.x;
    const KktDims d(NX, NU, N);
    const uint32_t cx = l < NX ? l : 0u, cu = l < NU ? l : 0u;   // clamped: idle lanes read what a live lane reads
    const uint64_t mprob = SHARED ? 0 : prob;
    const T *Gp = G + mprob * d.szG, *Cp = C + mprob * d.szC;
    const T *gp = g + prob * d.szg, *zp = z + prob * d.szg, *lp = lambda + prob * d.szc, *cp = c + prob * d.szc;
    T rb = T(0);
    if constexpr (REG) rb = rho[prob];   // (the workgroup's problem: a scalar load)

    U ms = 0, mf = 0;
    for (uint32_t k0 = 0; k0 < N; k0 += 16) {   // (the whole workgroup)
        const uint32_t kr = k0 + wave * 4 + qd;
        const bool live = kr < N, has_next = kr + 1 < N;
        const uint32_t k = live ? kr : 0u;
        const T *Gk = Gp + (size_t)k * d.sg, *Ck = Cp + (size_t)k * d.sc, *gk = gp + (size_t)k * d.sv, *zk = zp + (size_t)k * d.sv;
        const T *lk = lp + (size_t)k * NX, *ck = cp + (size_t)k * NX;

        T qr[NX], ac[NX], ar[NX], bc[NX], rr[NU], br[NU];
        T xk = T(0), sx = T(0), f0 = T(0), uk = T(0), su = T(0), nl = T(0), f = T(0);
        if (live) {
            xk = zk[cx];
            sx = gk[cx] + lk[cx];
#pragma unroll
            for (int q = 0; q < NX; ++q) qr[q] = Gk[q * NX + cx];
            if constexpr (REG) {
#pragma unroll
                for (int q = 0; q < NX; ++q) qr[q] = (uint32_t)q == cx ? qr[q] + rb : qr[q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < NX; ++q) qr[q] = T(0);
        }
        if (live && k == 0) f0 = xk - ck[cx];
        if (has_next) {
            uk = zk[NX + cu];
            su = gk[NX + cu];
            nl = -lk[NX + cx];
            f = zk[NX + NU + cx] - ck[NX + cx];
#pragma unroll
            for (int q = 0; q < NX; ++q) {
                ac[q] = Ck[cx * NX + q];
                ar[q] = Ck[q * NX + cx];
                bc[q] = Ck[NX * NX + cu * NX + q];
            }
#pragma unroll
            for (int q = 0; q < NU; ++q) {
                rr[q] = Gk[NX * NX + q * NU + cu];
                br[q] = Ck[NX * NX + q * NX + cx];
            }
            if constexpr (REG) {
#pragma unroll
                for (int q = 0; q < NU; ++q) rr[q] = (uint32_t)q == cu ? rr[q] + rb : rr[q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < NX; ++q) ac[q] = ar[q] = bc[q] = T(0);
#pragma unroll
            for (int q = 0; q < NU; ++q) rr[q] = br[q] = T(0);
        }
        recover_dot<0, NX>(sx, qr, xk);
        recover_dot<0, NX>(sx, ac, nl);
        recover_dot<0, NU>(su, rr, uk);
        recover_dot<0, NX>(su, bc, nl);
        recover_dot<0, NX>(f, ar, -xk);
        recover_dot<0, NU>(f, br, -uk);
        ms = umax(umax(ms, abs_bits(sx)), abs_bits(su));
        mf = umax(umax(mf, abs_bits(f0)), abs_bits(f));
    }
    store_norms(ms, mf, wave, lane, 4u, [&](uint32_t w) { return slots + 2 * w; }, res + 2 * prob);
}

// rho != nullptr: the REG instantiations; shared: the SHARED ones; one workgroup per problem either way.
template <typename T>
hipError_t launch_kkt_residual(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *G, const T *C,
                               const T *g, const T *c, const T *z, const T *lambda, T *res, hipStream_t s, bool shared, const T *rho)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    if (shared && rho) return hipErrorInvalidValue;         // (there is no shared twin of the REG form)
    hipError_t st;
    if (quad_dispatch(nx, nu, 0, st, [&](auto NX, auto NU) {
            auto kern = rho      ? schur_residual_quad_kernel<T, NX(), NU(), false, true>
                        : shared ? schur_residual_quad_kernel<T, NX(), NU(), true>
                                 : schur_residual_quad_kernel<T, NX(), NU()>;
            hipLaunchKernelGGL(kern, dim3(batch), dim3(256), 0, s, N, G, C, g, c, z, lambda, res, rho);
            return hipGetLastError();
        }))
        return st;
    auto kern = rho ? schur_residual_kernel<T, false, true> : shared ? schur_residual_kernel<T, true> : schur_residual_kernel<T>;
    return launch_lds_rows(dev, kern, (size_t)residual_wave_elems(nx, nu) * sizeof(T), [&](uint32_t) { return (uint64_t)batch; }, s,
                           nx, nu, N, G, C, g, c, z, lambda, res, rho);
}

template hipError_t launch_kkt_residual<float>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *,
                                               const float *, const float *, const float *, const float *, float *, hipStream_t, bool,
                                               const float *);
template hipError_t launch_kkt_residual<double>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, uint32_t, const double *,
                                                const double *, const double *, const double *, const double *, const double *,
                                                double *, hipStream_t, bool, const double *);

}  // namespace gbdpcg
