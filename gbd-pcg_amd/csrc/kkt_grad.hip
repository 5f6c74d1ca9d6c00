// kkt_grad.hip -- the device half of the KKT backward pass (gbdpcg_kkt_grad_*, gbdpcg_kkt_grad_shared_*, the last launch of
// gbdpcg_kkt_backward_*).  The forward map is G z + g + C' lambda = 0, C z = c; for a scalar l with upstream gradients gz = dl/dz,
// glam = dl/dlambda the adjoint pair (a_z, a_lambda) solves the SAME matrix with the right-hand side (-gz, -glam) -- one more
// gbdpcg_kkt_resolve_* -- and the gradients in the packed blocks are outer products of the two solutions.  With z = (x_k, u_k),
// a_z = (ax_k, au_k), l = lambda_{k+1}, al = a_lambda_{k+1}, blocks column-major as in d_G and d_C:
//     gQ_k(i,j) = 0.5 (ax_i x_j + x_i ax_j)        gR_k(i,j) = 0.5 (au_i u_j + u_i au_j)
//     gA_k(i,j) = -(al_i x_j + l_i ax_j)           gB_k(i,j) = -(al_i u_j + l_i au_j)
// Every entry: two rounded products, one rounded add (the build runs with -ffp-contract=off), then an exact scaling -- in that
// operand order, so the outputs are defined to the bit and gQ_k, gR_k are bit-symmetric (IEEE + and * commute).  [A_k | B_k] is one
// column-major nx x (nx + nu) matrix whose column index runs over (x_k, u_k): one formula serves both blocks.
//
// kkt_grad_kernel: purely write-bound ((nx^2 + nu^2 + nx^2 + nx nu) elements out per knot against 2 (nx + nu) + 2 nx in).  A
// workgroup owns `kch` consecutive knots of one problem: it stages their pieces of z, a_z, lambda, a_lambda in LDS (contiguous in
// memory, a few hundred bytes), then its lanes walk the knots' output elements in storage order -- the G range of the chunk, then
// the C range, each one contiguous piece of memory.  Knot strides such as 245 elements are not 16-byte aligned, so each range is
// written as a scalar head up to the first 16-byte boundary of the ADDRESS, 16-byte stores, a scalar tail (the shape of admm.hip).
// Every output element is written exactly once, by one lane: no atomics, no memset, no scratch, no handle state.
// The element -> (knot, column, row) maps divide by sg, sc, nx, nu: multiplications by reciprocals the host prepared (exact for
// the numerators of a chunk, see magic()), not divide sequences -- those would cost more than the stores.
//
// kkt_grad_shared_kernel: ONE problem's worth of gG, gC, the sum over the batch.  A thread owns one output element of one knot
// for the whole launch and adds the terms of b = 0, 1, ... batch-1 in that order (the accumulator STARTS as the term of b = 0, so
// batch == 1 gives the bits of the per-problem kernel, a -0 included); the workgroup stages the knot's vectors of `bb` problems
// per round.  No atomics: bit-identical from call to call.
#include "grad_store.hpp"
#include "internal.hpp"

namespace gbdpcg {

namespace {

struct GradShape {
    uint32_t nx, nu, N, batch;
    uint32_t kch, chunks;               // knots per workgroup, workgroups per problem
    uint32_t m_sg, m_sc, m_nx, m_nu;    // magic() of the four divisors
};

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void kkt_grad_kernel(GradShape s, const T *__restrict__ z, const T *__restrict__ lam,
                                                       const T *__restrict__ az, const T *__restrict__ alam, T *__restrict__ gG,
                                                       T *__restrict__ gC)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char grad_lds[];
    const uint32_t nx = s.nx, nu = s.nu, N = s.N, sv = nx + nu, sg = nx * nx + nu * nu, sc = nx * sv;
    T *sz = reinterpret_cast<T *>(grad_lds);   // z, a_z of the chunk's knots; lambda, a_lambda of the knots one further on
    T *sa = sz + s.kch * sv, *sl = sa + s.kch * sv, *sal = sl + s.kch * nx;
    const uint32_t prob = blockIdx.x / s.chunks, chunk = blockIdx.x - prob * s.chunks, tid = threadIdx.x, threads = blockDim.x;
    const uint32_t k0 = chunk * s.kch, kc = min(s.kch, N - k0);   // knots k0 .. k0 + kc - 1
    const uint32_t kcc = min(kc, N - 1 - k0);                      // ... of which the first kcc have an A_k, B_k (and a u_k)
    const uint64_t nz = (uint64_t)sv * N - nu, nl = (uint64_t)nx * N;

    const uint32_t zc = kc * sv - (kcc < kc ? nu : 0u);   // the last knot of the horizon has no u
    const T *zp = z + prob * nz + (uint64_t)k0 * sv, *ap = az + prob * nz + (uint64_t)k0 * sv;
    for (uint32_t i = tid; i < zc; i += threads) sz[i] = zp[i], sa[i] = ap[i];
    const T *lp = lam + prob * nl + (uint64_t)(k0 + 1) * nx, *alp = alam + prob * nl + (uint64_t)(k0 + 1) * nx;
    for (uint32_t i = tid; i < kcc * nx; i += threads) sl[i] = lp[i], sal[i] = alp[i];
    __syncthreads();

    if (gG) {
        const uint64_t LG = (uint64_t)sg * N - nu * nu;
        const uint32_t count = kc * sg - (kcc < kc ? nu * nu : 0u);
        store_range<T>(gG + prob * LG + (uint64_t)k0 * sg, count, tid, threads, [&](uint32_t f) {
            const uint32_t kk = fast_div(f, sg, s.m_sg);
            uint32_t e = f - kk * sg, d = nx, m = s.m_nx;
            const T *zz = sz + kk * sv, *aa = sa + kk * sv;
            if (e >= nx * nx) e -= nx * nx, d = nu, m = s.m_nu, zz += nx, aa += nx;
            const uint32_t j = fast_div(e, d, m), i = e - j * d;
            const T p1 = aa[i] * zz[j], p2 = zz[i] * aa[j];
            return T(0.5) * (p1 + p2);
        });
    }
    if (gC && kcc) {
        const uint64_t LC = (uint64_t)sc * (N - 1);
        store_range<T>(gC + prob * LC + (uint64_t)k0 * sc, kcc * sc, tid, threads, [&](uint32_t f) {
            const uint32_t kk = fast_div(f, sc, s.m_sc), e = f - kk * sc;
            const uint32_t j = fast_div(e, nx, s.m_nx), i = e - j * nx;
            const T p1 = sal[kk * nx + i] * sz[kk * sv + j], p2 = sl[kk * nx + i] * sa[kk * sv + j];
            return -(p1 + p2);
        });
    }
}

// grid (N, parts): workgroup (k, part) owns the elements part * 256 ... of knot k's [Q_k R_k | A_k B_k], one per thread.
template <typename T>
__global__ __launch_bounds__(256) void kkt_grad_shared_kernel(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, uint32_t bb,
                                                              const T *__restrict__ z, const T *__restrict__ lam,
                                                              const T *__restrict__ az, const T *__restrict__ alam,
                                                              T *__restrict__ gG, T *__restrict__ gC)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char grad_lds[];
    T *st = reinterpret_cast<T *>(grad_lds);   // per staged problem: [z_k (sv) | a_z,k (sv) | lambda_{k+1} (nx) | a_lambda,{k+1} (nx)]
    const uint32_t sv = nx + nu, sg = nx * nx + nu * nu, sc = nx * sv, per = 2 * sv + 2 * nx;
    const uint32_t k = blockIdx.x, tid = threadIdx.x, idx = blockIdx.y * 256u + tid;
    const bool last = k == N - 1;
    const uint32_t sgk = last ? nx * nx : sg, sck = last ? 0u : sc, svk = last ? nx : sv;
    const uint64_t nz = (uint64_t)sv * N - nu, nl = (uint64_t)nx * N;

    // the element's four operands inside one staged problem: term = (st[o1] * st[oz]) + (st[o2] * st[oa])
    const bool active = idx < sgk + sck, isC = idx >= sgk;
    uint32_t o1 = 0, o2 = 0, oz = 0, oa = 0;
    T *out = nullptr;
    if (active && !isC) {
        uint32_t e = idx, d = nx, off = 0;
        if (e >= nx * nx) e -= nx * nx, d = nu, off = nx;
        const uint32_t j = e / d, i = e - j * d;
        o1 = sv + off + i, oz = off + j, o2 = off + i, oa = sv + off + j;   // a_i z_j + z_i a_j
        if (gG) out = gG + (uint64_t)k * sg + idx;
    } else if (active) {
        const uint32_t e = idx - sgk, j = e / nx, i = e - j * nx;
        o1 = 2 * sv + nx + i, oz = j, o2 = 2 * sv + i, oa = sv + j;         // al_i z_j + l_i a_j
        if (gC) out = gC + (uint64_t)k * sc + e;
    }

    T acc = T(0);
    for (uint32_t b0 = 0; b0 < batch; b0 += bb) {
        const uint32_t nb = min(bb, batch - b0);
        for (uint32_t q = tid >> 6; q < nb; q += 4) {   // one wave per staged problem
            const uint64_t b = b0 + q;
            const T *zb = z + b * nz + (uint64_t)k * sv, *ab = az + b * nz + (uint64_t)k * sv;
            const T *lb = lam + b * nl + (uint64_t)(k + 1) * nx, *alb = alam + b * nl + (uint64_t)(k + 1) * nx;
            for (uint32_t t = tid & 63u; t < per; t += 64) {
                T v = T(0);
                if (t < sv) {
                    if (t < svk) v = zb[t];
                } else if (t < 2 * sv) {
                    if (t - sv < svk) v = ab[t - sv];
                } else if (!last) {
                    v = t < 2 * sv + nx ? lb[t - 2 * sv] : alb[t - 2 * sv - nx];
                }
                st[q * per + t] = v;
            }
        }
        __syncthreads();
        if (active) {
            for (uint32_t q = 0; q < nb; ++q) {
                const T *s = st + q * per;
                const T p1 = s[o1] * s[oz], p2 = s[o2] * s[oa];
                const T sum = p1 + p2;
                const T term = isC ? -sum : T(0.5) * sum;
                acc = (b0 == 0 && q == 0) ? term : acc + term;
            }
        }
        __syncthreads();
    }
    if (out) *out = acc;
}

template <typename T>
hipError_t launch_kkt_grad(uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *z, const T *lam, const T *az, const T *alam,
                           T *gG, T *gC, hipStream_t s, bool shared)
{
    const uint64_t sv = (uint64_t)nx + nu, sg = (uint64_t)nx * nx + (uint64_t)nu * nu, sc = (uint64_t)nx * sv;
    if (sg + sc >= (1ull << 24)) return hipErrorInvalidValue;   // element indices inside a chunk are 32-bit
    if (shared) {
        const uint32_t per = (uint32_t)(2 * sv + 2 * nx);
        const uint32_t parts = (uint32_t)((sg + sc + 255) / 256);
        if (parts > 65535u || N > 0x7fffffffu) return hipErrorInvalidValue;
        uint32_t bb = 4096u / per;   // problems staged per round: at most 32 KB of LDS
        bb = bb < 1u ? 1u : (bb > 32u ? 32u : bb);
        if (bb > batch) bb = batch;
        hipLaunchKernelGGL((kkt_grad_shared_kernel<T>), dim3(N, parts), dim3(256), (size_t)bb * per * sizeof(T), s, nx, nu, N, batch, bb, z,
                           lam, az, alam, gG, gC);
        return hipGetLastError();
    }
    // about 4096 output elements per workgroup (8 knots at nx = 14, nu = 7), at most 64 knots
    uint64_t kch = (4096 + sg + sc - 1) / (sg + sc);
    kch = kch > 64 ? 64 : kch;
    kch = kch > N ? N : kch;
    const uint64_t chunks = ((uint64_t)N + kch - 1) / kch;
    if (chunks * batch > 0x7fffffffull) return hipErrorInvalidValue;
    GradShape g;
    g.nx = nx, g.nu = nu, g.N = N, g.batch = batch, g.kch = (uint32_t)kch, g.chunks = (uint32_t)chunks;
    g.m_sg = magic((uint32_t)sg, kch * sg), g.m_sc = magic((uint32_t)sc, kch * sc);
    g.m_nx = magic(nx, sg > sc ? sg : sc), g.m_nu = magic(nu, sg);
    const size_t lds = (size_t)kch * (2 * sv + 2 * nx) * sizeof(T);
    hipLaunchKernelGGL((kkt_grad_kernel<T>), dim3((uint32_t)(chunks * batch)), dim3(256), lds, s, g, z, lam, az, alam, gG, gC);
    return hipGetLastError();
}

template hipError_t launch_kkt_grad<float>(uint32_t, uint32_t, uint32_t, uint32_t, const float *, const float *, const float *,
                                           const float *, float *, float *, hipStream_t, bool);
template hipError_t launch_kkt_grad<double>(uint32_t, uint32_t, uint32_t, uint32_t, const double *, const double *, const double *,
                                            const double *, double *, double *, hipStream_t, bool);

}  // namespace gbdpcg
