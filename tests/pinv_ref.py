"""Reference, case table and route prediction for the tests of Phi^-1 formation (csrc/pinv*.hip); not a test module.

reference()       plain fp64 numpy on S already rounded to the case's precision: D slot inv(D_k), R slot -D_k^-1 R_k D_{k+1}^-1,
                  L slot -D_k^-1 L_k D_{k-1}^-1; Jacobi the D slots only; identity D slot = I.  The two never-read corner slots (L of
                  knot 0, R of knot N-1) are unspecified: corner_mask().
reference_ld()    the same in np.longdouble (x87 extended, eps 1.1e-19): inv(D_k) in fp64, then two Newton steps X <- X + X (I - D X)
                  in longdouble (the error squares: 1e-15 -> 1e-19 at these condition numbers), the products in longdouble.  It is the
                  reference of the fp64 cases, whose own-precision error an fp64 reference cannot measure; exact rationals
                  (reference_exact) check both at n = 3.
same_precision()  the formulas in the case's OWN precision with plain numpy (np.linalg.inv and @ in fp32 / fp64): the yardstick.  A
                  block's bound is max(TOL[dtype], 8 e_np(block)), e_np = the error of this evaluation against the reference, both
                  relative to the largest entry of the reference block: the project's tolerance, or a factor 8 for Gauss-Jordan
                  without pivoting over LAPACK's pivoted inverse at the same precision.
CASES             one table, each case naming the kernel family it is meant to reach; pinv_route() restates pinv_route of
                  csrc/pinv.hip line for line, route() names the kernels of its family, and tests/test_pinv_reference.py holds every case to it.
Everything is in the device layout: [B, N, 3, n * n], slot order L, D, R, element (r, c) of a block at c * n + r."""
import collections
import functools
from fractions import Fraction

import numpy as np

from gbd_pcg_amd import synth

F32, F64 = np.float32, np.float64
LD = np.longdouble
TOL = {F32: 2e-5, F64: 1e-12}   # tests/test_gpu_parity.py::test_form_pinv_shapes
MARGIN = 8.0
IDENTITY, JACOBI, STAIR = 0, 1, 2
LDS_PER_WG = 160 * 1024          # DeviceInfo::lds_per_wg_max

# internal.hpp GBDPCG_SPECIALIZED_N and pinv_common.hpp GBDPCG_PINV_N, restated: a change of either list must show up in route()
SPECIALIZED_N = (2, 4, 6, 8, 10, 12, 13, 14, 16, 18, 20, 24, 36)
PINV_N = SPECIALIZED_N + (3, 5, 7, 9, 11, 15, 22)

# every kernel template of the pinv units (tests/test_pinv_reference.py compares with a list of its own)
FUSED = ("pinv_stair_fused_kernel",)
MFMA = ("pinv_stair_mfma_kernel",)
QUAD = ("pinv_diag_quad_kernel", "pinv_stair_reg_kernel")
QUAD_ONLY = ("pinv_diag_quad_kernel",)
PAIR = ("pinv_diag_pair_kernel",)
PAIR_STAIR = ("pinv_diag_pair_kernel", "pinv_stair_reg_kernel")
REG = ("pinv_diag_reg_kernel",)
REG_STAIR = ("pinv_diag_reg_kernel", "pinv_stair_reg_kernel")
WIDE = ("pinv_diag_wide_kernel", "pinv_stair_wide_kernel")
G64 = ("pinv_diag_kernel<64,16>", "pinv_stair_kernel<64>")
G256 = ("pinv_diag_kernel<256,16>", "pinv_stair_kernel<256>")
G256L = ("pinv_diag_kernel<256,64>", "pinv_stair_kernel<256>")
REFUSED = ("refused",)
# PinvFamily of csrc/pinv_common.hpp, by name: the kernels of each family (the second one runs for the stair kind only)
FAMILY_KERNELS = {"mfma": MFMA, "fused": FUSED, "quad": QUAD, "pair": PAIR_STAIR, "reg": REG_STAIR, "wide": WIDE,
                  "lds64": G64, "lds256": G256, "lds256_long": G256L, "refused": REFUSED}
LDS_TIER = {"lds64": 64, "lds256": 256, "lds256_long": 256}   # threads per knot: launch_form_pinv_g<T, GT, .>

Case = collections.namedtuple("Case", "family dtype n N B kind perturbed s_off env")
PinvSwitches = collections.namedtuple("PinvSwitches", "two_pass no_mfma pair no_wide mfma_from")


def _align16(count, es):
    per = 16 // es
    return (count + per - 1) // per * per


def pinv_switches(env):
    env = dict(env)
    return PinvSwitches("GBDPCG_PINV_TWO_PASS" in env, "GBDPCG_PINV_NO_MFMA" in env, "GBDPCG_PINV_PAIR" in env,
                        "GBDPCG_PINV_NO_WIDE" in env, int(env.get("GBDPCG_PINV_MFMA_FROM", 16)))


def pinv_route(elem_size, n, N, kind, s_aligned16, verdicts_wanted, sw):
    """pinv_route of csrc/pinv.hip, line for line: (family, chunks)."""
    listed = n in PINV_N
    specialised = n in SPECIALIZED_N
    family, chunks = "refused", 0
    if listed and 2 * n <= 64:
        if n <= 16 and n % 2 == 0 and kind == 2 and N >= 2 and not sw.two_pass and specialised:
            chunks = (N - 1 + 14) // 15
            mfma = elem_size == 4 and n >= 12 and not sw.no_mfma and n >= sw.mfma_from and s_aligned16
            family = "mfma" if mfma else "fused"
        elif 2 * n <= 32:
            family = "quad" if kind == 2 and not sw.pair else "pair"
        else:
            family = "reg"
    elif listed and 32 < n <= 64 and not sw.no_wide:
        family = "wide"
    elif 2 * n * n <= 16 * 64:
        family = "lds64"
    elif 2 * n * n <= 16 * 256:
        family = "lds256"
    elif 2 * n * n <= 64 * 256:
        family = "lds256_long"
    if verdicts_wanted and chunks == 0:
        family = "refused"
    return family, chunks


def route(dtype, n, N, kind, s_aligned=True, env=()):
    """The kernels launch_form_pinv (verdicts == nullptr) starts for a shape, as names: the family pinv_route picks, refused where
    launch_form_pinv_g finds the four factors of a workgroup's knots over the LDS of a compute unit; kinds 0 and 1 return after
    the diagonal pass (and so does pinv_diag_wide_kernel at N = 1), so only the first name runs then."""
    es = np.dtype(dtype).itemsize
    family, _ = pinv_route(es, n, N, kind, s_aligned, False, pinv_switches(env))
    if family in LDS_TIER and 256 // LDS_TIER[family] * _align16(4 * n * n, es) * es > LDS_PER_WG:
        family = "refused"
    names = FAMILY_KERNELS[family]
    stair_pass = kind == STAIR and (family != "wide" or N >= 2)
    return names if stair_pass else names[:1]


def _cases():
    out = []

    def add(family, dtype, n, N, B, kind=STAIR, perturbed=False, s_off=0, env=()):
        out.append(Case(family, dtype, n, N, B, kind, perturbed, s_off, tuple(env)))

    both = (F32, F64)
    # one-launch stair, DPP elimination and register products
    for n in (2, 4, 6, 8, 10, 12, 14, 16):
        for dtype in both:
            if n == 16 and dtype == F32:
                continue
            for N in (2, 15, 16, 17, 31):
                add(FUSED, dtype, n, N, 2)
                add(FUSED, dtype, n, N, 3, perturbed=True)
    for N in (2, 15, 16, 17, 31):   # fp32 n = 16 with S one element past a 16-byte boundary
        add(FUSED, F32, 16, N, 2, s_off=1)
        add(FUSED, F32, 16, N, 3, perturbed=True, s_off=1)
    # the MFMA form of it (every case also runs with Pinv one element off: check_case in test_gpu_pinv_dispatch.py)
    for N in (2, 15, 16, 17, 31, 32):
        for B in (1, 3):
            add(MFMA, F32, 16, N, B)
            add(MFMA, F32, 16, N, B, perturbed=True)
    # quad elimination + register stair: even n at N = 1 (nothing for the stair pass to do), perturbed S at every odd n
    for dtype in both:
        for n in (2, 8, 16):
            add(QUAD, dtype, n, 1, 3)
        for n in (3, 5, 7, 9, 11, 13, 15):
            add(QUAD, dtype, n, 9, 3, perturbed=True)
    # kinds 0 and 1 at n <= 16: N B = 3, 27, no multiple of the 8 knots of a workgroup
    for dtype in both:
        for n in sorted(m for m in PINV_N if m <= 16):
            for kind in (IDENTITY, JACOBI):
                for N in (1, 9):
                    add(PAIR, dtype, n, N, 3, kind)
    # one column per lane in registers: N B = 15, no multiple of the 4 knots of a workgroup
    for dtype in both:
        for n in (18, 20, 22, 24):
            add(REG, dtype, n, 5, 3, IDENTITY)
            add(REG, dtype, n, 5, 3, JACOBI)
            add(REG_STAIR, dtype, n, 5, 3, perturbed=True)
    for dtype in both:
        add(WIDE, dtype, 36, 4, 1)
    # any-size tiers.  <64,16>: N B = 3, 6, 21, no multiple of 4
    for dtype in both:
        for n in (1, 17, 19, 21):
            for kind in (IDENTITY, JACOBI, STAIR):
                for N in (1, 2, 7):
                    add(G64, dtype, n, N, 3, kind)
            if n > 1:
                add(G64, dtype, n, 7, 3, perturbed=True)
        for n in (23, 33, 45):
            for kind in (IDENTITY, JACOBI, STAIR):
                add(G256, dtype, n, 3, 2, kind)
            add(G256, dtype, n, 3, 2, perturbed=True)
    for dtype, sizes in ((F32, (46, 64, 65, 90)), (F64, (46, 60, LARGEST[F64]))):
        for n in sizes:
            for kind in (IDENTITY, JACOBI, STAIR):
                add(G256L, dtype, n, 3, 2, kind)
            add(G256L, dtype, n, 3, 2, perturbed=True)
    # code only an environment switch reaches: one child process per switch set
    for n in (12, 14):
        for N in (2, 16, 17):
            add(MFMA, F32, n, N, 2, env=MFMA_FROM)
            add(MFMA, F32, n, N, 3, perturbed=True, env=MFMA_FROM)
    for N in (2, 17):
        add(FUSED, F32, 16, N, 2, env=NO_MFMA)
        add(FUSED, F32, 16, N, 3, perturbed=True, env=NO_MFMA)
    for dtype in both:
        for n in (2, 8, 14, 16):
            add(QUAD, dtype, n, 9, 3, env=TWO_PASS)
        add(QUAD, dtype, 14, 9, 3, perturbed=True, env=TWO_PASS)
        # GBDPCG_PINV_PAIR alone leaves an even n <= 16 with the one-launch stair (that branch returns first): the even sizes need
        # GBDPCG_PINV_TWO_PASS next to it for "the pair kernel followed by the stair"
        add(PAIR_STAIR, dtype, 3, 9, 3, env=PAIR_ON)
        for n in (8, 14, 16):
            add(PAIR_STAIR, dtype, n, 9, 3, env=PAIR_ON + TWO_PASS)
        add(PAIR_STAIR, dtype, 14, 9, 3, perturbed=True, env=PAIR_ON + TWO_PASS)
        for kind in (IDENTITY, JACOBI, STAIR):
            add(G256, dtype, 36, 3, 2, kind, env=NO_WIDE)
        add(G256, dtype, 36, 3, 2, perturbed=True, env=NO_WIDE)
    return tuple(out)


MFMA_FROM = (("GBDPCG_PINV_MFMA_FROM", "12"),)
NO_MFMA = (("GBDPCG_PINV_NO_MFMA", "1"),)
TWO_PASS = (("GBDPCG_PINV_TWO_PASS", "1"),)
PAIR_ON = (("GBDPCG_PINV_PAIR", "1"),)
NO_WIDE = (("GBDPCG_PINV_NO_WIDE", "1"),)
SWITCH_SETS = (MFMA_FROM, NO_MFMA, TWO_PASS, PAIR_ON, PAIR_ON + TWO_PASS, NO_WIDE)
# first refused block size per precision at N = 2, B = 1, and the largest accepted one (recorded: test_gpu_pinv_dispatch.py)
FIRST_REFUSED = {F32: 91, F64: 72}
LARGEST = {F32: 90, F64: 71}
CASES = _cases()


def case_id(c):
    env = ",".join(k.replace("GBDPCG_PINV_", "") + "=" + v for k, v in c.env)
    return (f"{'+'.join(c.family)} {np.dtype(c.dtype).name} n={c.n} N={c.N} B={c.B} kind={c.kind}"
            f"{' perturbed' if c.perturbed else ''}{' S+1' if c.s_off else ''}{' ' + env if env else ''}")


def perturbed_problems(c):
    """Problems whose L blocks make_S changes (every one but problem 0; the only one of a batch of 1)."""
    if not c.perturbed:
        return []
    return [0] if c.B == 1 else list(range(1, c.B))


def make_S(c):
    """The case's S in its precision, [B, 3 n^2 N]: synth.gen_numpy, and for non-symmetric storage the perturbation of
    test_gpu_parity.py::test_form_pinv_general_S (one L block scaled by 1.25 in odd problems, a ramp added to every L block of even
    ones), applied in fp64 before rounding."""
    d = synth.gen_numpy(c.n, c.N, seed=700 + 3 * c.n + c.N, batch=c.B, dtype=F64)
    S = d["S"]
    if c.perturbed:
        assert c.N >= 2
        L, D, R = (np.array(x) for x in synth.unpack_bt(c.n, c.N, S))
        for b in perturbed_problems(c):
            if b % 2 or c.B == 1:
                L[b, min(4, c.N - 1)] *= 1.25
            else:
                L[b, 1:] += 0.01 * np.arange(c.n)[None, :, None]
        S = synth.pack_bt(L, D, R)
    return np.ascontiguousarray(S.astype(c.dtype))


def unpack(n, N, S, dtype=F64):
    """[B, 3 n^2 N] -> L, D, R as [B, N, n, n] indexed (r, c), in `dtype`."""
    blk = np.asarray(S).reshape(-1, N, 3, n, n).astype(dtype)   # [.., c, r]
    blk = np.swapaxes(blk, -1, -2)
    return blk[:, :, 0], blk[:, :, 1], blk[:, :, 2]


def pack(L, D, R):
    """L, D, R [B, N, n, n] -> the device layout [B, N, 3, n n]."""
    blk = np.swapaxes(np.stack([L, D, R], axis=2), -1, -2)
    return np.ascontiguousarray(blk).reshape(*blk.shape[:3], -1)


def _slots(L, D, R, Dinv, kind):
    """The three slots from D^-1; the corner slots come out as zeros (L_0 and R_{N-1} meet a zero factor)."""
    Z = np.zeros_like(Dinv)
    if kind == IDENTITY:
        eye = np.zeros_like(Dinv)
        eye[...] = np.eye(Dinv.shape[-1], dtype=Dinv.dtype)
        return pack(Z, eye, Z)
    if kind == JACOBI:
        return pack(Z, Dinv, Z)
    Lp, Rp = Z.copy(), Z.copy()
    Rp[:, :-1] = -(Dinv[:, :-1] @ R[:, :-1] @ Dinv[:, 1:])
    Lp[:, 1:] = -(Dinv[:, 1:] @ L[:, 1:] @ Dinv[:, :-1])
    return pack(Lp, Dinv, Rp)


def reference(n, N, S, kind):
    L, D, R = unpack(n, N, S, F64)
    return _slots(L, D, R, np.linalg.inv(D), kind)


def reference_ld(n, N, S, kind):
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is no wider than fp64 here: the fp64 cases have no yardstick"
    L, D, R = unpack(n, N, S, LD)
    X = np.linalg.inv(D.astype(F64)).astype(LD)
    eye = np.eye(n, dtype=LD)
    for _ in range(2):
        X = X + X @ (eye - D @ X)
    return _slots(L, D, R, X, kind)


def same_precision(n, N, S, kind, dtype):
    L, D, R = unpack(n, N, S, dtype)
    out = _slots(L, D, R, np.linalg.inv(D), kind)
    assert out.dtype == np.dtype(dtype)
    return out


def _inv_exact(M):
    n = len(M)
    A = [[Fraction(M[r][c]) for c in range(n)] + [Fraction(int(r == c)) for c in range(n)] for r in range(n)]
    for j in range(n):
        p = next(r for r in range(j, n) if A[r][j] != 0)
        A[j], A[p] = A[p], A[j]
        A[j] = [v / A[j][j] for v in A[j]]
        for r in range(n):
            if r != j and A[r][j] != 0:
                A[r] = [a - A[r][j] * b for a, b in zip(A[r], A[j])]
    return [row[n:] for row in A]


def _mul_exact(A, B):
    return [[sum(A[r][q] * B[q][c] for q in range(len(B))) for c in range(len(B[0]))] for r in range(len(A))]


def reference_exact(n, N, S):
    """The stair of ONE problem in exact rationals (the inputs are binary fractions), rounded once to fp64: [N, 3, n n]."""
    L, D, R = (x[0] for x in unpack(n, N, S, F64))
    Dinv = [_inv_exact(D[k].tolist()) for k in range(N)]
    out = np.zeros((N, 3, n * n))
    for k in range(N):
        slots = [None, Dinv[k], None]
        if k > 0:
            slots[0] = _mul_exact(_mul_exact(Dinv[k], [[Fraction(v) for v in row] for row in L[k].tolist()]), Dinv[k - 1])
        if k < N - 1:
            slots[2] = _mul_exact(_mul_exact(Dinv[k], [[Fraction(v) for v in row] for row in R[k].tolist()]), Dinv[k + 1])
        for s, M in enumerate(slots):
            if M is not None:
                sign = 1 if s == 1 else -1
                out[k, s] = [float(sign * M[r][c]) for c in range(n) for r in range(n)]
    return out


def corner_mask(B, N):
    """True for every (problem, knot, slot) that is specified."""
    m = np.ones((B, N, 3), bool)
    m[:, 0, 0] = False
    m[:, -1, 2] = False
    return m


def block_error(got, ref):
    """Per (problem, knot, slot): max |got - ref| and max |ref|, as fp64."""
    ref = np.asarray(ref)
    diff = np.abs(np.asarray(got).astype(ref.dtype) - ref).max(axis=-1)
    return diff.astype(F64), np.abs(ref).max(axis=-1).astype(F64)


CaseData = collections.namedtuple("CaseData", "S ref scale e_np bound mask cond")


@functools.lru_cache(maxsize=None)
def case_data(c):
    """Input, reference, per-block yardstick and bound of a case; computed once, never written to."""
    S = make_S(c)
    ref = reference(c.n, c.N, S, c.kind) if c.dtype == F32 else reference_ld(c.n, c.N, S, c.kind)
    err, scale = block_error(same_precision(c.n, c.N, S, c.kind, c.dtype), ref)
    e_np = np.divide(err, scale, out=np.zeros_like(err), where=scale > 0)
    bound = np.maximum(TOL[c.dtype], MARGIN * e_np)
    D32 = unpack(c.n, c.N, S, F64)[1].astype(F32).astype(F64)
    for a in (S, ref, scale, e_np, bound):
        a.setflags(write=False)
    return CaseData(S, ref, scale, e_np, bound, corner_mask(c.B, c.N), float(np.linalg.cond(D32).max()))


def dense_from_blocks(n, N, M):
    """One problem's [N, 3, n n] blocks as the dense n N x n N matrix, in fp64."""
    blk = np.swapaxes(np.asarray(M, F64).reshape(N, 3, n, n), -1, -2)
    A = np.zeros((n * N, n * N))
    for k in range(N):
        A[k * n:(k + 1) * n, k * n:(k + 1) * n] = blk[k, 1]
        if k > 0:
            A[k * n:(k + 1) * n, (k - 1) * n:k * n] = blk[k, 0]
        if k < N - 1:
            A[k * n:(k + 1) * n, (k + 1) * n:(k + 2) * n] = blk[k, 2]
    return A
