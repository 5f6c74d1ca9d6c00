// kkt_refine.hip -- mixed-precision refinement of a KKT point (gbdpcg_kkt_defect_mixed, gbdpcg_kkt_refine_apply, gbdpcg_demote_f32,
// the first and the last launch of gbdpcg_kkt_refine_step): the defect of an fp64 point (z, lambda) in fp64, written out as the
// fp32 right-hand side of the correction system that a kept fp32 factorisation solves, and the fp64 accumulation of the correction.
//   defect :  r_s = G z + g + C' lambda (layout of g), r_f = C z - c (layout of c), every entry the fma chain at the head of
//             schur_residual.hip in fp64;  m_s = max |r_s|, m_f = max |r_f| over bit patterns (norm_fold.hpp);
//             e = 0 where m = max(m_s, m_f) is 0, Inf or NaN, else -ilogb(m) clamped to [-126, 127]  (m 2^e in [1, 2) unclamped);
//             rg = fl32(r_s) * 2^e,  rc = fl32(-r_f) * 2^e  (one rounding, then an fp32 product that is exact unless it is
//             subnormal or overflows),  dlambda = 0,  expo[b] = e,  res[2b] = m_s, res[2b+1] = m_f
//   apply  :  z += (double)dz * 2^-e,  lambda += (double)dlambda * 2^-e   (widening and scaling are exact: ONE IEEE addition)
//   demote :  fp64 -> fp32, round to nearest, over a flat array
// Why the scaling: the PCG exit test is absolute (|eta| < tol).  From the second refinement step on the defect is 1e-6 and
// smaller, an unscaled correction solve would leave after zero iterations and the refinement would stall at fp32 accuracy.  With
// the power of two the solve always sees a right-hand side of max-norm in [1, 2), and the power of two costs no rounding.
//
// Defect kernels: the two forms of schur_residual.hip with the vectors written out, ONE WORKGROUP PER PROBLEM, two phases.
//   A  walks the rows as the residual kernels do, stores fl32(r_s), fl32(-r_f) and the zeros of dlambda (the layout of rc, the
//      same pass: no memset node), keeps the running maxima;
//      the maxima are folded as in store_norms (DPP in the wave, one LDS slot per wave); behind the __syncthreads() every lane
//      reads the slots of all waves from LDS and so holds m_s, m_f and e; one lane writes expo[b] and the norm pair;
//   B  the same __syncthreads() is a workgroup-scope release / acquire and every value of phase A was written by a lane of this
//      workgroup: the workgroup reads its own (nx + nu) N - nu + nx N fp32 outputs again and scales them in place -- dense
//      16-byte accesses behind a scalar head, default cache policy (the lines were written a moment ago and the gamma kernel
//      reads them next).  8 bytes of traffic per element on top of the 4 of phase A, all of it expected to hit in L2.
// Nothing is initialised beforehand, nothing is read from an output before phase B; no atomics, no scratch, no workgroup waits
// for another.  Every entry is the same chain in both kernels, a maximum is exact in any order: the two give the same bits.
#include "norm_fold.hpp"
#include "row16.hpp"
#include "schur_common.hpp"

namespace gbdpcg {

namespace {

typedef float refine_f4 __attribute__((ext_vector_type(4)));
typedef double refine_d2 __attribute__((ext_vector_type(2)));

// The exponent of a problem from its two maxima (bit patterns of non-negative doubles, NaN on top).
__device__ __forceinline__ int32_t refine_exponent(uint64_t ms, uint64_t mf)
{
    const uint64_t m = umax(ms, mf);
    const int32_t field = (int32_t)(m >> 52);
    if (m == 0 || field == 0x7ff) return 0;   // nothing to scale / Inf, NaN: the problem is lost whatever the scale
    if (field == 0) return 127;               // subnormal: -ilogb(m) > 1022, clamped
    const int32_t e = 1023 - field;           // -ilogb(m) of a normal number
    return e < -126 ? -126 : (e > 127 ? 127 : e);
}
// 2^e, e in [-126, 127]: a normal number in either precision.
__device__ __forceinline__ float pow2_f32(int32_t e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }
__device__ __forceinline__ double pow2_f64(int32_t e) { return __builtin_bit_cast(double, (uint64_t)(e + 1023) << 52); }

// Phase B for one array of the problem: p[0 .. n) *= scale, by the whole workgroup.  The head runs up to the first 16-byte
// boundary of the ADDRESS (a float pointer is 4-byte aligned, so there always is one within three elements).
__device__ __forceinline__ void refine_scale(float *p, uint64_t n, float scale, uint32_t tid, uint32_t threads)
{
    uint64_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / 4u;
    if (head > n) head = n;
    const uint64_t body = (n - head) / 4;
    if (tid < head) p[tid] *= scale;
    for (uint64_t q = tid; q < body; q += threads) {
        refine_f4 *v = reinterpret_cast<refine_f4 *>(p + head + q * 4);
        *v = *v * scale;
    }
    for (uint64_t i = head + body * 4 + tid; i < n; i += threads) p[i] *= scale;
}

// Behind phase A: fold, publish, scale.  slot(w): two words of LDS that belong to wave w (as in store_norms).
template <typename F>
__device__ __forceinline__ void refine_finish(uint64_t ms, uint64_t mf, uint32_t wave, uint32_t lane, uint32_t waves, F &&slot,
                                              float *rg, uint64_t ng, float *rc, uint64_t nc, int32_t *expo, double *res)
{
    ms = wave_umax(ms);
    mf = wave_umax(mf);
    if (lane == 0) {
        uint64_t *s = slot(wave);
        s[0] = ms;
        s[1] = mf;
    }
    __syncthreads();   // the slots, and the fp32 vectors of phase A (workgroup-scope release / acquire)
    for (uint32_t w = 0; w < waves; ++w) {
        const uint64_t *s = slot(w);
        ms = umax(ms, s[0]);
        mf = umax(mf, s[1]);
    }
    const int32_t e = refine_exponent(ms, mf);
    if (threadIdx.x == 0) {
        *expo = e;
        res[0] = from_bits(ms);
        res[1] = from_bits(mf);
    }
    if (e == 0) return;   // (the whole workgroup: e is the same in every lane)
    const float scale = pow2_f32(e);
    refine_scale(rg, ng, scale, threadIdx.x, blockDim.x);
    refine_scale(rc, nc, scale, threadIdx.x, blockDim.x);
}

}  // namespace

// Any block size: schur_residual_kernel<double> with the vectors written out (one wavefront per row, blocks staged in LDS).
// SHARED (gbdpcg_kkt_defect_mixed_shared): G and C are ONE problem's blocks, read with a zero problem stride; everything else
// stays per problem.  REG (gbdpcg_kkt_defect_mixed_reg): Q_k(r,r) and R_k(r,r) are staged as fl(d + rho_b), rho [batch]: the
// defect of (G + rho I) z + g + C' lambda, every chain behind the staging unchanged (schur_residual.hip, REG).
template <bool SHARED = false, bool REG = false>
__global__ __launch_bounds__(256) void kkt_defect_kernel(uint32_t nx, uint32_t nu, uint32_t N, const double *__restrict__ G,
                                                         const double *__restrict__ C, const double *__restrict__ g,
                                                         const double *__restrict__ c, const double *__restrict__ z,
                                                         const double *__restrict__ lambda, float *rg, float *rc, float *dl,
                                                         int32_t *__restrict__ expo, double *__restrict__ res,
                                                         const double *__restrict__ rho)   // [batch], REG only
{
    using T = double;
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
    float *rgp = rg + prob * d.szg, *rcp = rc + prob * d.szc, *dlp = dl ? dl + prob * d.szc : nullptr;

    T rb = T(0);
    if constexpr (REG) rb = rho[prob];   // (the workgroup's problem: a scalar load)

    uint64_t ms = 0, mf = 0;
    for (uint32_t k = wave; k < N; k += waves) {   // (whole waves)
        const bool has_next = k + 1 < N;
        const T *Gk = Gp + (size_t)k * d.sg, *Ck = Cp + (size_t)k * d.sc, *gk = gp + (size_t)k * d.sv, *zk = zp + (size_t)k * d.sv;
        const T *lk = lp + (size_t)k * nx, *ck = cp + (size_t)k * nx;
        float *rgk = rgp + (size_t)k * d.sv, *rck = rcp + (size_t)k * nx;
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
                for (uint32_t q = 0; q < nx; ++q) s = fma_t(A[r * nx + q], nl[q], s);
            ms = umax(ms, abs_bits(s));
            rgk[r] = (float)s;
            if (k == 0) {
                const T f0 = xk[r] - ck[r];
                mf = umax(mf, abs_bits(f0));
                rck[r] = (float)-f0;
                if (dlp) dlp[r] = 0.0f;
            }
            if (has_next) {
                T f = zk[d.sv + r] - ck[nx + r];
                for (uint32_t q = 0; q < nx; ++q) f = fma_t(A[q * nx + r], -xk[q], f);
                for (uint32_t q = 0; q < nu; ++q) f = fma_t(B[q * nx + r], -uk[q], f);
                mf = umax(mf, abs_bits(f));
                rck[nx + r] = (float)-f;
                if (dlp) dlp[(size_t)(k + 1) * nx + r] = 0.0f;
            }
        }
        if (has_next)
            for (uint32_t r = lane; r < nu; r += 64) {
                T s = gk[nx + r];
                for (uint32_t q = 0; q < nu; ++q) s = fma_t(R[q * nu + r], uk[q], s);
                for (uint32_t q = 0; q < nx; ++q) s = fma_t(B[r * nx + q], nl[q], s);
                ms = umax(ms, abs_bits(s));
                rgk[nx + r] = (float)s;
            }
    }
    refine_finish(ms, mf, wave, lane, waves, [&](uint32_t w) { return reinterpret_cast<uint64_t *>(base + (size_t)(w + 1) * we - 2); },
                  rgp, d.szg, rcp, d.szc, expo + prob, res + 2 * prob);
}

// Compile-time block sizes: schur_residual_quad_kernel<double, NX, NU> with the vectors written out -- four rows per wavefront,
// one per 16-lane quarter, operands from memory straight into registers; lane l of a quarter owns entry l of its knot's vectors
// and stores it (the lanes past NX, past NU in the u-part, repeat lane 0's entry for the maxima and store nothing).
// SHARED, REG: as above; REG is the select per element of schur_residual_quad_kernel on the lane that holds the row.
template <int NX, int NU, bool SHARED = false, bool REG = false>
__global__ __launch_bounds__(256) void kkt_defect_quad_kernel(uint32_t N, const double *__restrict__ G, const double *__restrict__ C,
                                                              const double *__restrict__ g, const double *__restrict__ c,
                                                              const double *__restrict__ z, const double *__restrict__ lambda,
                                                              float *rg, float *rc, float *dl, int32_t *__restrict__ expo,
                                                              double *__restrict__ res, const double *__restrict__ rho)
{
    static_assert(NX <= 16 && NU <= NX, "one row per 16-lane quarter");
    using T = double;
    __shared__ uint64_t slots[8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t l = lane & 15u, qd = lane >> 4;
    const uint64_t prob = blockIdx.x;
    const KktDims d(NX, NU, N);
    const uint32_t cx = l < NX ? l : 0u, cu = l < NU ? l : 0u;   // clamped: idle lanes read what a live lane reads
    const uint64_t mprob = SHARED ? 0 : prob;
    const T *Gp = G + mprob * d.szG, *Cp = C + mprob * d.szC;
    const T *gp = g + prob * d.szg, *zp = z + prob * d.szg, *lp = lambda + prob * d.szc, *cp = c + prob * d.szc;
    float *rgp = rg + prob * d.szg, *rcp = rc + prob * d.szc, *dlp = dl ? dl + prob * d.szc : nullptr;
    T rb = T(0);
    if constexpr (REG) rb = rho[prob];   // (the workgroup's problem: a scalar load)

    uint64_t ms = 0, mf = 0;
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
        // the vectors (behind every fma: the products above run with the full exec mask)
        if (live && l < NX) {
            rgp[(size_t)k * d.sv + l] = (float)sx;
            if (k == 0) {
                rcp[l] = (float)-f0;
                if (dlp) dlp[l] = 0.0f;
            }
            if (has_next) {
                rcp[(size_t)(k + 1) * NX + l] = (float)-f;
                if (dlp) dlp[(size_t)(k + 1) * NX + l] = 0.0f;
            }
        }
        if (has_next && l < NU) rgp[(size_t)k * d.sv + NX + l] = (float)su;
    }
    refine_finish(ms, mf, wave, lane, 4u, [&](uint32_t w) { return slots + 2 * w; }, rgp, d.szg, rcp, d.szc, expo + prob, res + 2 * prob);
}

// z[i] += (double)dz[i] * 2^-e_b over the layout of g, lambda likewise over the layout of c: the shape of admm_update_kernel --
// one workgroup per problem, e_b a scalar load, a 16-byte body on the fp64 array behind a scalar head (the first 16-byte boundary
// of its address) and a scalar tail.  One product that is exact and one addition per element either way: the same bits whatever
// the alignment.
__global__ __launch_bounds__(256) void kkt_refine_apply_kernel(uint64_t nz, uint64_t nl, const float *__restrict__ dz,
                                                               const float *__restrict__ dlambda, const int32_t *__restrict__ expo,
                                                               double *__restrict__ z, double *__restrict__ lambda)
{
    const uint32_t prob = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    int32_t e = expo[prob];
    e = e < -126 ? -126 : (e > 127 ? 127 : e);   // (what the defect launch writes is inside already; never an invalid bit pattern below)
    const double scale = pow2_f64(-e);

    auto segment = [&](double *x, const float *dx, uint64_t n) {
        uint64_t head = (reinterpret_cast<uintptr_t>(x) & 15u) ? 1u : 0u;   // (a double pointer is 8-byte aligned)
        if (head > n) head = n;
        const uint64_t body = (n - head) / 2;
        if (tid < head) x[tid] = x[tid] + (double)dx[tid] * scale;
        for (uint64_t q = tid; q < body; q += threads) {
            const uint64_t i = head + q * 2;
            refine_d2 v = *reinterpret_cast<const refine_d2 *>(x + i);
            v[0] = v[0] + (double)dx[i] * scale;
            v[1] = v[1] + (double)dx[i + 1] * scale;
            *reinterpret_cast<refine_d2 *>(x + i) = v;
        }
        for (uint64_t i = head + body * 2 + tid; i < n; i += threads) x[i] = x[i] + (double)dx[i] * scale;
    };
    segment(z + (uint64_t)prob * nz, dz + (uint64_t)prob * nz, nz);
    segment(lambda + (uint64_t)prob * nl, dlambda + (uint64_t)prob * nl, nl);
}

// fp64 -> fp32, round to nearest: a grid-stride walk, four elements per lane (two 16-byte loads, one 16-byte store) where both
// base pointers are 16-byte aligned (vec, decided by the host), a scalar tail; every element through the scalar form otherwise.
__global__ __launch_bounds__(256) void demote_kernel(uint64_t count, uint32_t vec, const double *__restrict__ src, float *__restrict__ dst)
{
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, threads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t body = vec ? count / 4 : 0;
    for (uint64_t q = tid; q < body; q += threads) {
        const refine_d2 a = *reinterpret_cast<const refine_d2 *>(src + q * 4), b = *reinterpret_cast<const refine_d2 *>(src + q * 4 + 2);
        const refine_f4 v = {(float)a[0], (float)a[1], (float)b[0], (float)b[1]};
        *reinterpret_cast<refine_f4 *>(dst + q * 4) = v;
    }
    for (uint64_t i = body * 4 + tid; i < count; i += threads) dst[i] = (float)src[i];
}

// rho != nullptr: the REG instantiations; shared: the SHARED ones (as launch_kkt_residual); one workgroup per problem either way.
hipError_t launch_kkt_defect_mixed(const DeviceInfo &dev, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *G,
                                   const double *C, const double *g, const double *c, const double *z, const double *lambda, float *rg,
                                   float *rc, float *dlambda, int32_t *expo, double *res, hipStream_t s, bool shared, const double *rho)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    if (shared && rho) return hipErrorInvalidValue;         // (a shared batch has one G: the caller writes G + rho I into it)
    hipError_t st;
    if (quad_dispatch(nx, nu, 0, st, [&](auto NX, auto NU) {
            auto kern = rho      ? kkt_defect_quad_kernel<NX(), NU(), false, true>
                        : shared ? kkt_defect_quad_kernel<NX(), NU(), true>
                                 : kkt_defect_quad_kernel<NX(), NU()>;
            hipLaunchKernelGGL(kern, dim3(batch), dim3(256), 0, s, N, G, C, g, c, z, lambda, rg, rc, dlambda, expo, res, rho);
            return hipGetLastError();
        }))
        return st;
    auto kern = rho ? kkt_defect_kernel<false, true> : shared ? kkt_defect_kernel<true> : kkt_defect_kernel<>;
    return launch_lds_rows(dev, kern, (size_t)residual_wave_elems(nx, nu) * sizeof(double), [&](uint32_t) { return (uint64_t)batch; }, s,
                           nx, nu, N, G, C, g, c, z, lambda, rg, rc, dlambda, expo, res, rho);
}

hipError_t launch_kkt_refine_apply(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *dz, const float *dlambda,
                                   const int32_t *expo, double *z, double *lambda, hipStream_t s)
{
    if (batch > 0x7fffffffu) return hipErrorInvalidValue;   // one workgroup per problem
    const uint64_t nz = ((uint64_t)nx + nu) * N - nu, nl = (uint64_t)nx * N;
    const uint32_t threads = nz <= 512 ? 64 : 256;
    hipLaunchKernelGGL(kkt_refine_apply_kernel, dim3(batch), dim3(threads), 0, s, nz, nl, dz, dlambda, expo, z, lambda);
    return hipGetLastError();
}

hipError_t launch_demote(const DeviceInfo &dev, uint64_t count, const double *src, float *dst, hipStream_t s)
{
    const uint32_t vec = (reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0) ? 1u : 0u;
    const uint64_t want = (count / (vec ? 4 : 1) + 255) / 256, most = (uint64_t)dev.num_cus * 8;
    const uint32_t grid = (uint32_t)(want < 1 ? 1 : (want > most ? most : want));
    hipLaunchKernelGGL(demote_kernel, dim3(grid), dim3(256), 0, s, count, vec, src, dst);
    return hipGetLastError();
}

}  // namespace gbdpcg
