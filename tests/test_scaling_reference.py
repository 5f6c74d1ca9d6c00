"""CPU half of the scaling tests (tests/scaling_ref.py; the GPU half is tests/test_gpu_scaling.py).

1  The helpers are right: the fp64 dense KKT residual (oracle/schur_oracle.py::dense_kkt) of the transformed pair in the
   transformed problem, scaled back, equals the residual of the base pair in the base problem bit for bit (every row summed
   in index order, so the order does not depend on the values).
2  The property the GPU half asserts of the kernels holds of the CPU implementations of the same operations, bit for bit, at
   every shape and exponent range the GPU half uses and in both precisions: the working-precision numpy formation
   (scaling_ref.form_twin: Gauss-Jordan without pivoting + the block formulas) and the oracle's PCG.
3  The range condition (every compared non-zero finite entry within 2^+-100 in fp32, 2^+-900 in fp64) holds for those inputs
   and outputs: it is asserted inside scaling_ref.solve_case / assert_equivariant / assert_solve_equivariant.
"""
import numpy as np
import pytest

import scaling_ref as sr
from gbd_pcg_amd import synth
from oracle import schur_oracle as so

KKT_ROWS = [(s, False) for s in sr.KKT_SHAPES] + [(s, True) for s in sr.UNIFORM_SHAPES]


def _kkt(nx, nu, N, dtype, uniform):
    """The base problem, exponents and copies tests/test_gpu_scaling.py::Kkt puts on the device."""
    d, _, ex, eu = sr.kkt_case(nx, nu, N, dtype, uniform)
    return d, ex, eu, sr.kkt_copies(d, nx, nu, N, ex, eu)


def test_draw_and_exponents():
    ex, eu = sr.draw(1, 14, 7, 9, 3, 12)
    assert not ex[0].any() and not eu[0].any() and np.abs(ex).max() == 12 and np.abs(eu).max() == 12
    assert (ex[2].max(axis=1) == 12).all() and (ex[2].min(axis=1) == -12).all()      # the worst copy: both ends in every block
    ex, eu = sr.draw(1, 5, 2, 9, 3, 40, uniform=True)
    assert [int(ex[k].min()) for k in range(3)] == [int(ex[k].max()) for k in range(3)] and abs(int(ex[2, 0, 0])) == 40
    sz = so.sizes(5, 2, 9)
    for kind in ("G", "C", "g", "c", "S", "gamma", "z", "Ginv"):
        assert sr.exps(kind, 5, 2, 9, ex, eu).shape == (3, sz[kind]), kind
    # uniform scaling 2^a: G by 2^2a, C unchanged, S by 2^-2a
    a = ex[:, 0, 0]
    assert (sr.exps("G", 5, 2, 9, ex, eu) == 2 * a[:, None]).all() and not sr.exps("C", 5, 2, 9, ex, eu).any()
    assert (sr.exps("S", 5, 2, 9, ex)[:, 3 * 25:-3 * 25] == -2 * a[:, None]).all()
    x = np.float32([1.5, -3.25, 0.0])
    assert sr.apply(x, [3, -2, 5]).tolist() == [12.0, -0.8125, 0.0] and sr.apply(x, [3, -2, 5]).dtype == np.float32
    assert sr.in_range(np.float32, np.float32([0.0, 2.0 ** -100, np.inf])) and not sr.in_range(np.float32, np.float32([2.0 ** -101]))


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape,uniform", KKT_ROWS, ids=str)
def test_helpers_against_the_dense_kkt_residual(shape, uniform, dtype):
    """(1): the problems and exponents of the GPU half in either precision, the arithmetic in fp64."""
    nx, nu, N = shape
    d, ex, eu, _ = _kkt(nx, nu, N, dtype, uniform)
    d = {k: v.astype(np.float64) for k, v in d.items()}
    dk = sr.kkt_copies(d, nx, nu, N, ex, eu)
    rng = np.random.default_rng(3)
    z = rng.standard_normal(d["g"].shape[1]).astype(np.float32).astype(np.float64)
    lam = rng.standard_normal(nx * N).astype(np.float32).astype(np.float64)
    zk, lk = sr.copies(z, "z", nx, nu, N, ex, eu), sr.copies(lam, "lam", nx, nu, N, ex, eu)
    st, fe = [], []
    for k in range(sr.K_COPIES):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, dk["G"][k], dk["C"][k], dk["g"][k], dk["c"][k])
        s, f = sr.residual_fixed_order(Gd, Cd, g, c, zk[k], lk[k])
        st.append(s)
        fe.append(f)
    assert np.abs(st[0]).max() > 0.1 and np.abs(fe[0]).max() > 0.1
    sr.assert_equivariant("stationarity", np.stack(st), sr.exps("g", nx, nu, N, ex, eu), np.float64)     # T (G z + g + C' lambda)
    sr.assert_equivariant("feasibility", np.stack(fe), sr.exps("c", nx, nu, N, ex, eu), np.float64)      # E (C z - c)


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape,uniform", KKT_ROWS, ids=str)
def test_working_precision_formation_is_equivariant(shape, uniform, dtype):
    """(2): Gauss-Jordan without pivoting and the block formulas in the test's precision, on cost blocks of condition up to
    2^48 x 30 (fp32) / 2^160 x 30 (fp64); the unscaled twin against the fp64 oracle at the formation tolerances of
    tests/test_gpu_schur.py."""
    nx, nu, N = shape
    d, ex, eu, dk = _kkt(nx, nu, N, dtype, uniform)
    assert sr.in_range(dtype, *dk.values())
    parts = [sr.form_twin(nx, nu, N, dk["G"][k], dk["C"][k], dk["g"][k], dk["c"][k]) for k in range(sr.K_COPIES)]
    oracle = so.form_schur(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0])
    tol = 2e-4 if np.dtype(dtype) == np.float32 else 1e-11
    for i, kind in enumerate(("S", "gamma", "Ginv")):
        back = sr.assert_equivariant(kind, np.stack([p[i] for p in parts]), sr.exps(kind, nx, nu, N, ex, eu), dtype)
        assert np.abs(back[-1].astype(np.float64) - oracle[i]).max() <= tol * np.abs(oracle[i]).max(), kind
    if not uniform and nx > 1:
        Q = dk["G"][-1][:nx * nx].reshape(nx, nx).astype(np.float64)
        assert np.linalg.cond(Q) > 2.0 ** (3 * sr.lim(dtype))       # the case is badly scaled


def _oracle_runs(orc, c, S, P, gamma, lam0, dtype, name, tol_scale=1.0):
    for run, tol, max_iter in sr.RUNS:
        ob = orc.pcg_batch(c["n"], c["N"], c["batch"], S, P, gamma, lambda0=lam0, tol=tol * tol_scale, max_iter=max_iter, nthreads=4)
        ob["flag"] = ob["max_iter_exit"]
        yield run, ob


@pytest.mark.parametrize("case", sr.SOLVE_CASES, ids=sr.solve_id)
def test_oracle_pcg_is_equivariant(orc, case):
    """(2): the C oracle on (S, Phi^-1, gamma) of every solve case of the GPU half: equal iteration counts, lambda, r and p
    bit-identical after unscaling, at tol 1e-6 and at the fixed count."""
    fam, n, N, dtype, mode, B, bases, warm = case
    c = sr.solve_case(n, N, dtype, B, bases, warm)
    for run, ob in _oracle_runs(orc, c, c["S"], c["Pinv"], c["gamma"], c["lam0"], dtype, sr.solve_id(case)):
        sr.assert_solve_equivariant(f"{sr.solve_id(case)} {run}", c, ob, dtype)
        assert (ob["iters"] == 6).all() if run == "fixed" else (ob["iters"] > 3).all() and not ob["flag"].any()


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
def test_oracle_pcg_without_preconditioner_and_scaled_right_hand_sides(orc, dtype):
    """The two solve cases that mix scales.  Phi^-1 = NULL: eta = r.r, so one exponent a for the whole batch and tol scaled by
    2^-2a, against the unscaled call.  Right-hand sides only (the shared-matrix case): S, Phi^-1 as they are, gamma and lambda_0
    by 2^a per problem -- eta scales by 2^2a, so the fixed count compares problems of one call, the run to a tolerance two
    calls with one a and tol scaled by 2^2a."""
    n, N, B = 14, 30, 3
    a = sr.lim(dtype)
    base = sr.solve_case(n, N, dtype, B, bases=B, warm=True, K=1)
    for sign in (1, -1):
        e = sign * a
        for run, tol, max_iter in sr.RUNS:
            want = orc.pcg_batch(n, N, B, base["S"], None, base["gamma"], lambda0=base["lam0"], tol=tol, max_iter=max_iter)
            got = orc.pcg_batch(n, N, B, np.ldexp(base["S"], -2 * e), None, np.ldexp(base["gamma"], -e), lambda0=np.ldexp(base["lam0"], e),
                                tol=float(np.ldexp(dtype(tol), -2 * e)), max_iter=max_iter)
            assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["max_iter_exit"], want["max_iter_exit"])
            for key, s in (("lambda_", -e), ("r", e), ("p", e)):       # p is r-like without a preconditioner
                assert sr.in_range(dtype, got[key]) and np.array_equal(np.ldexp(got[key], s), want[key]), (run, key)
            want = orc.pcg_batch(n, N, B, base["S"], base["Pinv"], base["gamma"], lambda0=base["lam0"], tol=tol, max_iter=max_iter)
            got = orc.pcg_batch(n, N, B, base["S"], base["Pinv"], np.ldexp(base["gamma"], e), lambda0=np.ldexp(base["lam0"], e),
                                tol=float(np.ldexp(dtype(tol), 2 * e)), max_iter=max_iter)
            assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["max_iter_exit"], want["max_iter_exit"])
            for key in ("lambda_", "r", "p"):
                assert sr.in_range(dtype, got[key]) and np.array_equal(np.ldexp(got[key], -e), want[key]), (run, key)


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,N", sr.PINV_SHAPES)
def test_oracle_spmv_is_equivariant(orc, n, N, dtype):
    """(2) for SpMV: the oracle's product is equivariant on S (x' = T x, y' = E y) and on Phi^-1 with T and E swapped; and (3)
    for the inputs of the Phi^-1 formation cases (asserted inside solve_case)."""
    c = sr.solve_case(n, N, dtype, sr.K_COPIES)
    x = np.stack([synth.normals(9, 0, n * N)] * sr.K_COPIES).astype(np.float32).astype(dtype)
    for M, xin, yout in (("S", "lam", "gamma"), ("Pinv", "gamma", "lam")):
        y = orc.spmv(n, N, c[M], sr.apply(x, c["E"][xin]), batch=sr.K_COPIES).reshape(sr.K_COPIES, -1)
        sr.assert_equivariant(f"spmv {M}", y, c["E"][yout], dtype)
