// pinv.hip -- build the preconditioner Pinv from S on the device.
//
// The reference never forms Pinv itself: its host overload leaves d_Pinv uninitialised
// (its include/interface.cuh:45-46,57-59) and MPCGPU builds it out of tree with the
// block helpers load_block_bd / store_block_bd (include/utils.cuh:96-161).  The pinv units supply the
// step so the host-pointer API is usable end to end:
//   IDENTITY     : D slot = I, L/R slots = 0
//   BLOCK_JACOBI : D slot = D_k^-1
//   STAIR        : D slot = D_k^-1, L slot = -D_k^-1 L_k D_{k-1}^-1, R slot = -D_k^-1 R_k D_{k+1}^-1
// (the symmetric-stair preconditioner of the MPCGPU paper the README cites, README.md:66-77).
//
// One thread GROUP per (problem, knot): a whole 256-thread workgroup for large blocks, ONE WAVEFRONT
// (four knots per workgroup) when n <= 24 -- these blocks are so small (n = 14: 196 elements) that a
// knot is pure latency, and a wave needs no workgroup barrier: LDS operations of one wave execute in
// program order, so a compiler-level fence between "everyone has read the old tableau" and "write the
// new one" is all the synchronisation there is.  Pass 1 inverts D_k by Gauss-Jordan on an LDS-resident
// [D | I] tableau (no pivoting: D_k is a definite diagonal block of a Schur complement); pass 2
// (STAIR only) does the two triple products with all three operands in LDS.  O(n^3) per knot on n^2
// data, once per control step; not the bandwidth-bound hot loop, but on the MPC critical path.
//
// This unit: the route (which kernels a shape takes, pinv_route), launch_form_pinv, and the any-size LDS kernels just
// described.  pinv_regs.hip: the two-pass kernels for the compile-time block sizes.  pinv_fused.hip: the stair in one launch.
#include "pinv_common.hpp"

namespace gbdpcg {

template <typename T, int GT, int EPT_MAX>
__global__ __launch_bounds__(kPinvThreads) void pinv_diag_kernel(uint32_t n, uint32_t N, uint64_t knots,
                                                                const T *__restrict__ S, T *__restrict__ Pinv, int kind)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr uint32_t GROUPS = kPinvThreads / GT;
    const uint32_t grp = threadIdx.x / GT, tid = threadIdx.x % GT;
    const uint64_t knot = (uint64_t)blockIdx.x * GROUPS + grp;  // (problem, knot) flattened: same stride
    const uint32_t w = 2 * n;
    T *tab = reinterpret_cast<T *>(smem_raw) + (size_t)grp * align16<T>(2 * n * n);  // [n][2n] row-major tableau
    if (GT == 64 && knot >= knots) return;  // whole wave idle (only the wave-per-knot form has spare groups)
    const size_t blk = (size_t)knot * 3 * n * n;
    const T *D = S + blk + (size_t)n * n;
    T *out = Pinv + blk;

    for (uint32_t i = tid; i < n * n; i += GT) {
        const uint32_t c = i / n, r = i - c * n;  // column-major source
        tab[r * w + c] = (kind == 0) ? (r == c ? T(1) : T(0)) : D[i];
        tab[r * w + n + c] = (r == c) ? T(1) : T(0);
    }
    group_sync<GT>();
    if (kind != 0) {
        for (uint32_t j = 0; j < n; ++j) {
            // every thread first READS what it needs of the old tableau (pivot, its column-j entries, the
            // pivot row), then all WRITE: the two halves are separated by group_sync
            const T piv = T(1) / tab[j * w + j];
            T upd[EPT_MAX];
            uint32_t cnt = 0;
            for (uint32_t i = tid; i < n * w && cnt < EPT_MAX; i += GT, ++cnt) {
                const uint32_t r = i / w, c = i - r * w;
                const T pr = tab[j * w + c] * piv;  // scaled pivot-row entry
                upd[cnt] = (r == j) ? pr : fma_t(-tab[r * w + j], pr, tab[r * w + c]);
            }
            group_sync<GT>();
            cnt = 0;
            for (uint32_t i = tid; i < n * w && cnt < EPT_MAX; i += GT, ++cnt) tab[i] = upd[cnt];
            group_sync<GT>();
        }
    }
    // D_k^-1 of a symmetric D_k is symmetric in exact arithmetic but not bit for bit after the
    // elimination; the upper triangle is mirrored so that the stair blocks built from it come out
    // exactly symmetric (L_{k+1} == R_k^T) whenever S is -- what gbdpcg_set_symmetric relies on.
    for (uint32_t i = tid; i < n * n; i += GT) {
        const uint32_t c = i / n, r = i - c * n;
        out[(size_t)n * n + i] = r <= c ? tab[r * w + n + c] : tab[c * w + n + r];
        out[i] = T(0);
        out[(size_t)2 * n * n + i] = T(0);
    }
}

// Off-diagonal slots of the stair preconditioner; reads the D slots pass 1 wrote.
template <typename T, int GT>
__global__ __launch_bounds__(kPinvThreads) void pinv_stair_kernel(uint32_t n, uint32_t N, uint64_t knots,
                                                                 const T *__restrict__ S, T *Pinv)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr uint32_t GROUPS = kPinvThreads / GT;
    const uint32_t grp = threadIdx.x / GT, tid = threadIdx.x % GT;
    const uint64_t knot = (uint64_t)blockIdx.x * GROUPS + grp;
    const uint32_t nn = n * n;
    T *A = reinterpret_cast<T *>(smem_raw) + (size_t)grp * align16<T>(4 * nn);  // first factor  (column-major)
    T *B = A + nn;                                                              // middle factor
    T *C = B + nn;                                                              // last factor
    T *W = C + nn;                                                              // A*B
    if (GT == 64 && knot >= knots) return;
    const uint32_t k = (uint32_t)(knot % N);
    const size_t blk = (size_t)knot * 3 * nn;

    // Right slot:  R'_k     = -(D_k^-1 R_k) D_{k+1}^-1.
    // Left slot :  L'_k     = -D_k^-1 L_k D_{k-1}^-1, evaluated as the TRANSPOSE of
    //              X = -(D_{k-1}^-1 L_k^T) D_k^-1  -- the same operation sequence the right slot of
    //              knot k-1 runs on (D_{k-1}^-1, R_{k-1}, D_k^-1).  With symmetric D^-1 blocks the two are
    //              equal as matrices for any S, and bit for bit each other's transpose when L_k == R_{k-1}^T.
    for (int side = 0; side < 2; ++side) {  // 0: left slot (needs k-1), 1: right slot (needs k+1)
        if ((side == 0 && k == 0) || (side == 1 && k == N - 1)) continue;  // uniform over the group
        const size_t nb = side == 0 ? blk - (size_t)3 * nn : blk + (size_t)3 * nn;
        for (uint32_t i = tid; i < nn; i += GT) {
            const uint32_t c = i / n, r = i - c * n;
            if (side == 1) {
                A[i] = Pinv[blk + nn + i];            // D_k^-1
                B[i] = S[blk + 2 * (size_t)nn + i];   // R_k
                C[i] = Pinv[nb + nn + i];             // D_{k+1}^-1
            } else {
                A[i] = Pinv[nb + nn + i];             // D_{k-1}^-1
                B[i] = S[blk + (size_t)r * n + c];    // L_k^T : element (r,c) = L_k(c,r)
                C[i] = Pinv[blk + nn + i];            // D_k^-1
            }
        }
        group_sync<GT>();
        for (uint32_t i = tid; i < nn; i += GT) {
            const uint32_t c = i / n, r = i - c * n;
            T acc = T(0);
            for (uint32_t q = 0; q < n; ++q) acc = fma_t(A[q * n + r], B[c * n + q], acc);
            W[i] = acc;
        }
        group_sync<GT>();
        for (uint32_t i = tid; i < nn; i += GT) {
            const uint32_t c = i / n, r = i - c * n;
            T acc = T(0);
            for (uint32_t q = 0; q < n; ++q) acc = fma_t(W[q * n + r], C[c * n + q], acc);
            if (side == 1) Pinv[blk + 2 * (size_t)nn + i] = -acc;                  // R'_k(r,c)
            else Pinv[blk + (size_t)r * n + c] = -acc;                             // L'_k(c,r) = X(r,c)
        }
        group_sync<GT>();
    }
}

template <typename T, int GT, int EPT_MAX>
static hipError_t launch_form_pinv_g(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch, const T *S, T *Pinv,
                                     int kind, hipStream_t s)
{
    constexpr uint32_t GROUPS = kPinvThreads / GT;
    const size_t lds1 = (size_t)GROUPS * align16<T>(2 * n * n) * sizeof(T);
    const size_t lds2 = (size_t)GROUPS * align16<T>(4 * n * n) * sizeof(T);
    if (lds1 > dev.lds_per_wg_max || lds2 > dev.lds_per_wg_max) return hipErrorInvalidValue;
    const uint64_t knots = (uint64_t)N * batch;
    const uint64_t blocks = (knots + GROUPS - 1) / GROUPS;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    auto k1 = pinv_diag_kernel<T, GT, EPT_MAX>;
    auto k2 = pinv_stair_kernel<T, GT>;
    if (lds1 > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)k1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
        if (e != hipSuccess) return e;
    }
    if (lds2 > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k1, dim3((uint32_t)blocks), dim3(kPinvThreads), lds1, s, n, N, knots, S, Pinv, kind);
    if (kind == 2) hipLaunchKernelGGL(k2, dim3((uint32_t)blocks), dim3(kPinvThreads), lds2, s, n, N, knots, S, Pinv);
    return hipGetLastError();
}

// The environment switches of the route, read once (tuning runs and tests only).
struct PinvSwitches {
    bool two_pass, no_mfma, pair, no_wide;
    int mfma_from;
};
static const PinvSwitches &pinv_switches()
{
    static const PinvSwitches sw = [] {
        const char *from = getenv("GBDPCG_PINV_MFMA_FROM");
        return PinvSwitches{getenv("GBDPCG_PINV_TWO_PASS") != nullptr, getenv("GBDPCG_PINV_NO_MFMA") != nullptr,
                            getenv("GBDPCG_PINV_PAIR") != nullptr, getenv("GBDPCG_PINV_NO_WIDE") != nullptr, from ? atoi(from) : 16};
    }();
    return sw;
}

// Which kernels a shape takes.  tests/pinv_ref.py restates this function line for line (pinv_route there), and
// tests/golden/pinv_routes.json holds what it returned before the two were written in this form.
PinvRoute pinv_route(size_t elem_size, uint32_t n, uint32_t N, int kind, bool s_aligned16, bool verdicts_wanted)
{
    const PinvSwitches &sw = pinv_switches();
    const bool listed = pinv_dispatch_n(n, false, [](auto) { return true; });
    bool specialised = false;
#define GBDPCG_X(NN) specialised |= n == NN;
    GBDPCG_SPECIALIZED_N(GBDPCG_X)
#undef GBDPCG_X
    PinvRoute r{PinvFamily::refused, 0};
    if (listed && 2 * n <= 64) {  // the tableau, or four blocks of n <= 16, in the registers of one wavefront
        if (n <= 16 && n % 2 == 0 && kind == 2 && N >= 2 && !sw.two_pass && specialised) {  // (GBDPCG_PINV_PAIR does not reach here)
            r.chunks = (N - 1 + 14) / 15;  // 15 pairs per workgroup
            // measured: -32 % at 16; a tie at 14 and 12 (profiles/r03_pinv_ab.txt).  LDS-DMA moves 16-byte pieces of S
            const bool mfma = elem_size == 4 && n >= 12 && !sw.no_mfma && (int)n >= sw.mfma_from && s_aligned16;
            r.family = mfma ? PinvFamily::mfma : PinvFamily::fused;
        } else if (2 * n <= 32) {
            r.family = kind == 2 && !sw.pair ? PinvFamily::quad : PinvFamily::pair;
        } else {
            r.family = PinvFamily::reg;
        }
    } else if (listed && n > 32 && n <= 64 && !sw.no_wide) {  // one column per lane
        r.family = PinvFamily::wide;
    } else if (2 * n * n <= 16 * 64) {
        // wave-per-knot needs the whole [D|I] tableau to fit 16 elements per lane: 2 n^2 <= 1024
        // (EPT_MAX tableau elements per thread are held in registers across the read / write halves of a pivot step)
        r.family = PinvFamily::lds64;
    } else if (2 * n * n <= 16 * 256) {
        r.family = PinvFamily::lds256;
    } else if (2 * n * n <= 64 * 256) {
        r.family = PinvFamily::lds256_long;
    }
    if (verdicts_wanted && r.chunks == 0) r.family = PinvFamily::refused;  // only the one-launch kernels report verdicts
    return r;
}

// Workgroups per problem of the one-launch stair kernel when launch_form_pinv will use it for this shape (it is
// the only form that can report symmetry verdicts), else 0.
template <typename T> uint32_t pinv_verdict_chunks(uint32_t n, uint32_t N, int kind)
{
    return pinv_route(sizeof(T), n, N, kind, true, false).chunks;
}

// Refused (hipErrorInvalidValue): a shape no family takes, verdicts asked of a shape without chunks (the caller asks
// pinv_verdict_chunks first), and what the family's launcher refuses: a grid of more than 0x7fffffff workgroups, and in
// the LDS tiers a knot whose factors exceed one compute unit's LDS.
template <typename T>
hipError_t launch_form_pinv(const DeviceInfo &dev, uint32_t n, uint32_t N, uint32_t batch, const T *S, T *Pinv,
                            int kind, hipStream_t s, uint8_t *verdicts, bool s_symmetric)
{
    const PinvRoute r = pinv_route(sizeof(T), n, N, kind, reinterpret_cast<uintptr_t>(S) % 16 == 0, verdicts != nullptr);
    switch (r.family) {
    case PinvFamily::mfma:
    case PinvFamily::fused: return launch_pinv_fused<T>(r, n, N, batch, S, Pinv, s, verdicts, s_symmetric);
    case PinvFamily::quad:
    case PinvFamily::pair:
    case PinvFamily::reg:
    case PinvFamily::wide: return launch_pinv_regs<T>(r.family, n, N, batch, S, Pinv, kind, s);
    case PinvFamily::lds64: return launch_form_pinv_g<T, 64, 16>(dev, n, N, batch, S, Pinv, kind, s);
    case PinvFamily::lds256: return launch_form_pinv_g<T, 256, 16>(dev, n, N, batch, S, Pinv, kind, s);
    case PinvFamily::lds256_long: return launch_form_pinv_g<T, 256, 64>(dev, n, N, batch, S, Pinv, kind, s);
    case PinvFamily::refused: break;
    }
    return hipErrorInvalidValue;
}

template hipError_t launch_form_pinv<float>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, const float *,
                                            float *, int, hipStream_t, uint8_t *, bool);
template hipError_t launch_form_pinv<double>(const DeviceInfo &, uint32_t, uint32_t, uint32_t, const double *,
                                             double *, int, hipStream_t, uint8_t *, bool);
template uint32_t pinv_verdict_chunks<float>(uint32_t, uint32_t, int);
template uint32_t pinv_verdict_chunks<double>(uint32_t, uint32_t, int);

}  // namespace gbdpcg
