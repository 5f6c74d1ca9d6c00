"""GPU: every SpMV, solve and stair kernel on NON-SYMMETRIC operators (tests/layout_ref.py), through the C ABI.

The rest of the suite feeds the kernels matrices that are symmetric as a whole up to rounding, so it pins the [L|D|R]
column-major layout only up to transposition.  Here D_k != D_k^T and L_{k+1} != R_k^T by 0.3 of a block's size: a kernel that
reads a D block row-major, takes L_{k+1} x_k from R_k^T, swaps its neighbours across a chunk or compute-unit seam or builds the
stair's left slot from the right one is off by 5 ... 100 per cent where the tolerances below are 1e-6 / 1e-10
(tests/test_layout_reference.py checks both ends of that on the CPU, for the same rows).

  a  SpMV on general matrices, component-wise  |y - yhat| <= 2 (3n + 2) u (|M| |x|)  against the dense fp64 product:
     (3n + 2) u is the a-priori bound of an inner product of length 3n in any order, with or without FMA; the factor 2 covers
     accumulation that is not one rounding per add.  NaN corner slots must not reach y.
  b  index probes: M is zero except one 1.5, x holds small integers, y is compared with ==.
  c  symmetric SpMV (mode 1, L slots NaN) on mirrored matrices whose D is not symmetric.
  d  fixed-count solves (tol = 0, 4 iterations, warm start), one row per kernel family: lambda against the oracle on the same
     storage within 1e-6 / 1e-10 norm-wise, r and p within 2e-5 / 1e-9 of max|gamma|, and the error against the plain fp64
     recurrence at most twice the worst of the oracle's four summation orders plus that tolerance.
  e  stair formation from independent L and R, every slot on its own.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import layout_ref as lr  # noqa: E402
from gbd_pcg_amd import binding, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SPECIALIZED_N = [2, 4, 6, 8, 10, 12, 13, 14, 16, 18, 20, 24, 36]   # GBDPCG_SPECIALIZED_N (csrc/internal.hpp)
RUNTIME_N = [3, 5, 7, 9, 15, 25, 37, 64]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_offset(a, off):
    """Device copy of a flat array that starts `off` elements past an allocation (narrower loads: V = 1, V = 2)."""
    a = np.ascontiguousarray(a).reshape(-1)
    buf = torch.zeros(a.size + off, dtype=torch.from_numpy(a[:1]).dtype, device="cuda")
    v = buf[off:]
    v.copy_(torch.from_numpy(a))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + off * a.dtype.itemsize
    return v


# ------------------------------------------------------------------------------------------------------------- a. SpMV
def _spmv_general(solver, n, N, B, dtype, seed, offsets):
    d = lr.gen_general(n, N, seed=seed, batch=B, dtype=dtype)
    x = np.stack([synth.normals(seed + 100 + b, 0, n * N) for b in range(B)]).astype(dtype)
    A = [lr.dense(n, N, d["S"][b]) for b in range(B)]
    want = np.stack([A[b] @ x[b].astype(np.float64) for b in range(B)])
    bound = 2 * (3 * n + 2) * lr.unit(dtype) * np.stack([np.abs(A[b]) @ np.abs(x[b].astype(np.float64)) for b in range(B)])
    dx = dev(x)
    for off in offsets:
        y = solver.spmv(n, N, B, dev_offset(d["S"], off), dx)
        torch.cuda.synchronize()
        y = y.cpu().numpy().astype(np.float64).reshape(B, -1)
        assert np.isfinite(y).all(), (N, off)                       # NaN in L_0 / R_{N-1} must not reach y
        ratio = (np.abs(y - want) / bound).max()
        print(f"spmv n={n} N={N} B={B} {np.dtype(dtype).name} off={off}: max |y - yhat| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (N, off, ratio)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SPECIALIZED_N + RUNTIME_N)
def test_spmv_general(solver, dtype, n):
    """Every specialised block size and the runtime-n kernel, N = 1, 2, 3, 9 (N = 9: chunk seams at knots 4 and 8), from an
    aligned pointer and from pointers one and two elements past one (V = 1 and V = 2 loads)."""
    for N in (1, 2, 3, 9):
        _spmv_general(solver, n, N, 3, dtype, seed=200 + n + N, offsets=(0, 1, 2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,N,B", [(14, 300, 2), (37, 41, 2)])
def test_spmv_general_many_chunks(solver, dtype, n, N, B):
    """One horizon per family that is cut into many workgroups."""
    _spmv_general(solver, n, N, B, dtype, seed=300 + n, offsets=(0, 1))


# ----------------------------------------------------------------------------------------------------- b. index probes
def _probes(n, N):
    rc = sorted({(0, 1), (1, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 2)})
    return [(s, k, r, c) for s in range(3) for k in range(N) for (r, c) in rc]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [2, 3, 13, 14, 16, 36, 37])
def test_spmv_index_probes(solver, dtype, n):
    """One non-zero per problem, at (slot s, knot k, row r, column c): y[k n + r] = 1.5 x[(k + s - 1) n + c] and nothing else,
    exactly.  Every knot of N = 9 (the first and last two and both sides of the chunk seams at 4 and 8); a probe in L_0 or
    R_{N-1} gives y == 0."""
    N = 9
    P = _probes(n, N)
    B = len(P)
    M = np.zeros((B, N, 3, n, n), dtype)          # [problem, knot, slot, column, row]: column-major blocks
    x = np.tile(np.arange(1, n * N + 1, dtype=dtype), (B, 1))
    want = np.zeros((B, n * N), dtype)
    for b, (s, k, r, c) in enumerate(P):
        M[b, k, s, c, r] = 1.5
        if 0 <= k + s - 1 < N:
            want[b, k * n + r] = 1.5 * x[b, (k + s - 1) * n + c]
    y = solver.spmv(n, N, B, dev(M.reshape(B, -1)), dev(x))
    torch.cuda.synchronize()
    y = y.cpu().numpy().reshape(B, -1)
    bad = [(P[b], np.flatnonzero(y[b] != want[b]).tolist()) for b in range(B) if not np.array_equal(y[b], want[b])]
    assert not bad, bad[:5]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 12, 14, 16])
def test_symmetric_spmv_index_probes(solver, dtype, n):
    """The same through gbdpcg_set_symmetric(1), probes in the D and R slots only and every L slot NaN: a D probe appears once
    (D is NOT assumed symmetric), an R_k probe at (r, c) appears at y[k n + r] and mirrored at y[(k + 1) n + c]."""
    N = 9
    P = [q for q in _probes(n, N) if q[0] != 0]
    B = len(P)
    M = np.zeros((B, N, 3, n, n), dtype)
    M[:, :, 0] = np.nan
    x = np.tile(np.arange(1, n * N + 1, dtype=dtype), (B, 1))
    want = np.zeros((B, n * N), dtype)
    for b, (s, k, r, c) in enumerate(P):
        M[b, k, s, c, r] = 1.5
        if s == 1:
            want[b, k * n + r] = 1.5 * x[b, k * n + c]
        elif k + 1 < N:
            want[b, k * n + r] = 1.5 * x[b, (k + 1) * n + c]
            want[b, (k + 1) * n + c] = 1.5 * x[b, k * n + r]
    solver.set_symmetric(1)
    try:
        y = solver.spmv(n, N, B, dev(M.reshape(B, -1)), dev(x))
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    y = y.cpu().numpy().reshape(B, -1)
    bad = [(P[b], np.flatnonzero(y[b] != want[b]).tolist()) for b in range(B) if not np.array_equal(y[b], want[b])]
    assert not bad, bad[:5]


# ------------------------------------------------------------------------------------ c. symmetric SpMV, mirrored storage
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,N,B", [(14, 128, 8), (14, 1, 3), (14, 2, 3), (14, 300, 2), (12, 40, 6), (16, 33, 5), (8, 50, 3)])
def test_symmetric_spmv_on_mirrored_storage(solver, dtype, n, N, B):
    """Mode 1, every L slot NaN, D_k != D_k^T: y against the dense product of (R^T mirrored, D, R), the bound of (a)."""
    d = lr.gen_mirrored(n, N, seed=400 + n + N, batch=B, dtype=dtype)
    x = np.stack([synth.normals(500 + b, 0, n * N) for b in range(B)]).astype(dtype)
    A = [lr.dense(n, N, d["S"][b]) for b in range(B)]
    want = np.stack([A[b] @ x[b].astype(np.float64) for b in range(B)])
    bound = 2 * (3 * n + 2) * lr.unit(dtype) * np.stack([np.abs(A[b]) @ np.abs(x[b].astype(np.float64)) for b in range(B)])
    Sp = d["S"].reshape(B, N, 3, n * n).copy()
    Sp[:, :, 0, :] = np.nan
    solver.set_symmetric(1)
    try:
        y = solver.spmv(n, N, B, dev(Sp.reshape(B, -1)), dev(x))
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    y = y.cpu().numpy().astype(np.float64)
    assert np.isfinite(y).all()
    ratio = (np.abs(y - want) / bound).max()
    print(f"symmetric spmv n={n} N={N} B={B} {np.dtype(dtype).name}: max |y - yhat| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------ d. fixed-count solves
FAMILY_PATH = {"resident": binding.PATH_AUTO, "cluster": binding.PATH_AUTO, "stream": binding.PATH_FUSED, "split": binding.PATH_SPLIT,
               "persist": binding.PATH_PERSISTENT, "persist1r": binding.PATH_PERSISTENT_1R, "sym": binding.PATH_FUSED,
               "mixed": binding.PATH_FUSED}
FAMILY_TAKES = {"resident": binding.PATH_FUSED, "cluster": binding.PATH_FUSED, "stream": binding.PATH_FUSED, "split": binding.PATH_SPLIT,
                "persist": binding.PATH_PERSISTENT, "persist1r": binding.PATH_PERSISTENT_1R, "sym": binding.PATH_FUSED,
                "mixed": binding.PATH_FUSED}
# workgroups per problem of the cluster kernel (gbdpcg_cluster_members).  The single-workgroup kernels of pcg_resident.hip are
# not built for stateSize 14 in fp64: there the "resident" row (14, 40) is a cluster of two.
MEMBERS = {(4, 14, 100): 2, (4, 14, 217): 4, (4, 14, 500): 7, (4, 12, 161): 3, (4, 16, 33): 1, (4, 18, 56): 1, (4, 14, 150): 3,
           (8, 14, 65): 3, (8, 13, 128): 4, (8, 16, 40): 2, (8, 14, 40): 2}


def _assert_family(solver, row):
    fam, n, N, B, dt, gen, mode = row
    es = np.dtype(dt).itemsize
    assert solver.choose_path(es, n, N, B) == FAMILY_TAKES[fam], (fam, solver.choose_path(es, n, N, B))
    if fam in ("resident", "cluster", "stream"):
        assert solver.cluster_members(es, n, N) == MEMBERS.get((es, n, N), 0)
    if fam == "cluster":
        assert solver.cluster_members(es, n, N) >= 1


def _solve(solver, row, c, shared=False, form=False):
    """The row's solve on the device: tol = 0, K_FIXED iterations from the warm start; r and p start as NaN."""
    fam, n, N, B, dt, gen, mode = row
    solver.set_symmetric(mode)
    solver.set_path(FAMILY_PATH.get(fam, binding.PATH_AUTO))
    try:
        if fam in FAMILY_TAKES:
            _assert_family(solver, row)
        dg, lam = dev(c["gamma"]), dev(c["lam0"])
        r, p = torch.full_like(dg, float("nan")), torch.full_like(dg, float("nan"))
        if shared:
            it, fl = solver.solve_shared(n, N, B, dev(c["S"][0]), dev(c["Pinv"][0]), dg, lam, r, p, tol=0.0, max_iter=lr.K_FIXED)
            Pd = None
        elif form:
            Pd = torch.full((B, 3 * n * n * N), float("nan"), dtype=dg.dtype, device="cuda")
            it, fl = solver.form_pinv_solve(n, N, B, dev(c["S"]), Pd, dg, lam, r=r, p=p, tol=0.0, max_iter=lr.K_FIXED)
        else:
            it, fl = solver.solve(n, N, B, dev(c["S"]), dev(c["Pinv"]), dg, lam, r, p, tol=0.0, max_iter=lr.K_FIXED)
            Pd = None
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
        solver.set_path(binding.PATH_AUTO)
    out = dict(lambda_=lam.cpu().numpy().reshape(B, -1), r=r.cpu().numpy().reshape(B, -1), p=p.cpu().numpy().reshape(B, -1),
               iters=it.cpu().numpy().astype(np.int64), flag=fl.cpu().numpy().astype(bool))
    if form:
        out["Pinv"] = Pd.cpu().numpy()
    return out


def _check(orc, row, c, out):
    """What every fixed-count case asserts (module docstring, d).  The figures are printed before they are asserted."""
    fam, n, N, B, dt, gen, mode = row
    tol, vt = lr.ltol(dt), lr.vtol(dt)
    ob = orc.pcg_batch(n, N, B, c["S"], c["Pinv"], c["gamma"], lambda0=c["lam0"], tol=0.0, max_iter=lr.K_FIXED, nthreads=8)
    gmax = np.abs(c["gamma"]).max(axis=1)
    e_lam = np.array([lr.relerr(out["lambda_"][b], ob["lambda_"][b]) for b in range(B)])
    e_r = np.abs(out["r"].astype(np.float64) - ob["r"]).max(axis=1) / gmax
    e_p = np.abs(out["p"].astype(np.float64) - ob["p"]).max(axis=1) / gmax
    print(f"{lr.row_id(row)}: against the oracle lambda {np.nanmax(e_lam):.2e} (tol {tol:.0e}), r {np.nanmax(e_r):.2e}, "
          f"p {np.nanmax(e_p):.2e} (tol {vt:.0e})")
    m = c["base"]
    var = lr.oracle_variants(orc, c, problems=m)
    figs = []
    for b in range(m):
        ref = dict(zip(("lambda_", "r", "p"), lr.fixed_reference(c, b)))
        for key, dist, slack in (("lambda_", lr.relerr, tol), ("r", lambda x, y: np.abs(x - y).max() / gmax[b], vt),
                                 ("p", lambda x, y: np.abs(x - y).max() / gmax[b], vt)):
            e_orc = max(dist(v[key][b].astype(np.float64), ref[key]) for v in var)
            figs.append((b, key, dist(out[key][b].astype(np.float64), ref[key]), 2 * e_orc + slack))
    worst = max(figs, key=lambda f: f[2] / f[3])
    print(f"    against the fp64 recurrence, worst of {m} problems: {worst[1]} of problem {worst[0]} {worst[2]:.2e} (allowed {worst[3]:.2e})")
    assert (out["iters"] == lr.K_FIXED).all(), out["iters"]
    assert np.array_equal(out["flag"], ob["max_iter_exit"].astype(bool))
    assert np.isfinite(out["lambda_"]).all() and np.isfinite(out["r"]).all() and np.isfinite(out["p"]).all()
    assert (e_lam < tol).all(), (int(e_lam.argmax()), e_lam.max())
    assert (e_r < vt).all(), (int(e_r.argmax()), e_r.max())
    assert (e_p < vt).all(), (int(e_p.argmax()), e_p.max())
    for b, key, e_gpu, allowed in figs:
        assert e_gpu <= allowed, (b, key, e_gpu, allowed)


@pytest.mark.parametrize("row", lr.SOLVE_ROWS, ids=lr.row_id)
def test_fixed_count_solve(solver, orc, row):
    """Mode 0 on general storage, one row per kernel family (single-workgroup resident, cluster of 1 / 2 / 3 / 4 / 7 workgroups and
    a batch beyond one round of clusters, streaming fused, split, persistent in both forms); modes 1 and 2 on mirrored storage
    whose D is not symmetric (CU-resident symmetric kernel, symmetric streaming kernels).

    The persist1r rows are what made the single-reduction kernel carry chi = u.s + p.w: with the textbook
    alpha = gamma / (delta - beta gamma / alpha_old), an identity of symmetric operators, lambda was off by 2.4 (36 x 37 fp64)
    norm-wise on these rows."""
    c = lr.row_case(row)
    _check(orc, row, c, _solve(solver, row, c))


@pytest.mark.parametrize("row", lr.MIXED_ROWS, ids=lr.row_id)
def test_mode2_on_an_interleaved_batch(solver, orc, row):
    """Even problems mirrored, odd problems general, default mode: each problem must match the reference for its OWN storage --
    the verdict is per problem, and whatever solves the general ones reads L."""
    fam, n, N, B, dt, gen, mode = row
    c = lr.row_case(row)
    ok = (solver.check_symmetric(n, N, B, dev(c["S"])) & solver.check_symmetric(n, N, B, dev(c["Pinv"]))).cpu().numpy()
    assert ok.tolist() == [1 - b % 2 for b in range(B)]
    _check(orc, row, c, _solve(solver, row, c))


@pytest.mark.parametrize("row", lr.SHARED_ROWS, ids=lr.row_id)
def test_shared_pair(solver, orc, row):
    """gbdpcg_solve_shared_*: one general pair, and one mirrored pair, for five right-hand sides, against the reference per
    right-hand side."""
    c = lr.row_case(row)
    _check(orc, row, c, _solve(solver, row, c, shared=True))


# ---------------------------------------------------------------------------------------------------- e. stair formation
STAIR_SHAPES = [(14, 2, 2), (14, 15, 1), (14, 16, 3), (14, 17, 2), (14, 31, 1), (14, 128, 2), (8, 20, 2), (12, 33, 1), (16, 47, 2),
                (6, 5, 2), (13, 18, 1), (36, 4, 1), (36, 1, 2), (36, 2, 1), (36, 21, 3), (3, 19, 3), (3, 2, 1), (5, 33, 2), (7, 18, 2),
                (9, 21, 1), (11, 17, 2), (15, 16, 2), (15, 1, 1), (20, 9, 2), (22, 13, 2), (22, 2, 1), (24, 7, 1), (18, 10, 2),
                (10, 40, 1), (4, 64, 2), (2, 30, 3)]   # the shapes of test_gpu_parity.py::test_form_pinv_shapes


def _slot_errors(got, want):
    """relerr of L', D' and R' separately over a set of problems ([B, N, 3, n, n] row/column-indexed; corners left out)."""
    return (lr.relerr(got[:, 1:, 0], want[:, 1:, 0]), lr.relerr(got[:, :, 1], want[:, :, 1]), lr.relerr(got[:, :-1, 2], want[:, :-1, 2]))


def _blocks(P, B, N, n):
    return np.swapaxes(np.asarray(P, np.float64).reshape(B, N, 3, n, n), -1, -2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,N,B", STAIR_SHAPES)
def test_stair_from_independent_L_and_R(solver, dtype, n, N, B):
    """L_{k+1} = R_k^T + 0.3 normal / sqrt(n) on every block, D the generator's symmetric D: the left slot -D_{k+1}^-1 L_{k+1}
    D_k^-1 has to come from L itself.  Modes 2 and 0; L', D' and R' each against the fp64 host construction on the cast S, so
    that a wrong left slot cannot hide behind the other two."""
    S, want, _ = lr.gen_stair_general(n, N, seed=600 + n + N, batch=B, dtype=dtype)
    bound = 1e-12 if dtype == np.float64 else 2e-5
    for mode in (2, 0):
        solver.set_symmetric(mode)
        try:
            P = solver.form_pinv(n, N, B, dev(S), binding.PINV_STAIR)
            torch.cuda.synchronize()
        finally:
            solver.set_symmetric(2)
        errs = _slot_errors(_blocks(P.cpu().numpy(), B, N, n), want)
        print(f"stair n={n} N={N} B={B} {np.dtype(dtype).name} mode {mode}: relerr L' {errs[0]:.2e} D' {errs[1]:.2e} R' {errs[2]:.2e}")
        for name, e in zip(("L'", "D'", "R'"), errs):
            assert e < bound, (mode, name, e)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,N", [(14, 31), (16, 17)])
def test_stair_and_solve_on_an_interleaved_batch(solver, orc, dtype, n, N):
    """Alternating symmetric and general problems in one batch: the symmetric ones still come out bit-symmetric, the general
    ones match the reference slot by slot; then gbdpcg_form_pinv_solve_* in mode 2, where the stair kernel's verdict replaces
    the test launch -- the general problems must be solved by a kernel that reads L: against the oracle run on the
    device-formed Pinv, as in (d)."""
    B = 4
    S, want, gamma = lr.gen_stair_general(n, N, seed=700 + n, batch=B, dtype=dtype, every=2)
    assert solver.check_symmetric(n, N, B, dev(S)).cpu().numpy().tolist() == [1, 0, 1, 0]
    P = solver.form_pinv(n, N, B, dev(S), binding.PINV_STAIR)
    torch.cuda.synchronize()
    assert solver.check_symmetric(n, N, B, P).cpu().numpy().tolist() == [1, 0, 1, 0]
    got = _blocks(P.cpu().numpy(), B, N, n)
    bound = 1e-12 if dtype == np.float64 else 2e-5
    for sel in (slice(0, B, 2), slice(1, B, 2)):
        for name, e in zip(("L'", "D'", "R'"), _slot_errors(got[sel], want[sel])):
            assert e < bound, (sel, name, e)
    row = ("form", n, N, B, dtype, "stair", 2)
    lam0 = np.stack([0.1 * synth.normals(800 + b, 0, n * N) for b in range(B)]).astype(dtype)
    c = dict(n=n, N=N, batch=B, base=B, S=S, gamma=gamma, lam0=lam0)
    out = _solve(solver, row, dict(c, Pinv=None), form=True)
    Pd, Ps = out["Pinv"].reshape(B, N, 3, n * n).copy(), P.cpu().numpy().reshape(B, N, 3, n * n).copy()
    for arr in (Pd, Ps):   # the corner slots are unspecified
        arr[:, 0, 0] = 0
        arr[:, -1, 2] = 0
    assert np.array_equal(Pd, Ps)      # same bits as the separate call
    _check(orc, row, dict(c, Pinv=Pd.reshape(B, -1)), out)
