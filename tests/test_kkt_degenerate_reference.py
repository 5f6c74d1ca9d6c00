"""The constructions of tests/kkt_degenerate_ref.py on the host: gamma of the degenerate problems is EXACTLY zero in both precisions,
the CPU oracle (oracle/pcg_oracle.c, the reference's recurrence) runs such a problem to max_iter with the flag set and a non-finite
lambda, the regular problems have a finite dense solution, and exactly 2 of the 5 problems are degenerate."""
import numpy as np
import pytest

import kkt_degenerate_ref as kd
from oracle import oracle as orc
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
CASES = [(s, k) for s in kd.SHAPES for k in kd.KINDS[s]]


def test_kinds_and_masks():
    deg, reg = kd.expected_masks()
    assert deg.tolist() == [False, True, False, True, False] and reg.tolist() == [True, False, True, False, True]
    assert kd.B == 5 and all(set(kd.KINDS[s]) >= {"a", "c"} for s in kd.SHAPES)
    # kind b exists wherever there is a control to carry g: everywhere but N = 1, where gamma_0 = -Q_0^-1 q_0 = 0 means g = 0
    assert [s for s in kd.SHAPES if "b" not in kd.KINDS[s]] == [(3, 2, 1)]


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape,kind", CASES)
def test_gamma_is_exactly_zero_for_two_of_five(shape, kind, dtype):
    nx, nu, N = shape
    d, twin = kd.batch(nx, nu, N, kind)
    deg, _ = kd.expected_masks()
    zero = []
    for b in range(kd.B):
        gamma = kd.gamma_formula(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b], dtype)
        assert gamma.dtype == np.dtype(dtype) and gamma.shape == (nx * N,)
        zero.append(not gamma.any())
        if dtype == F64:    # the formula here is the oracle's
            assert np.allclose(gamma, so.form_schur(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])[1], rtol=1e-12, atol=1e-13)
        assert kd.gamma_formula(nx, nu, N, twin["G"][b], twin["C"][b], twin["g"][b], twin["c"][b], dtype).any()
    assert np.array_equal(np.array(zero), deg)
    for b in kd.DEGENERATE:
        assert not d["c"][b].any() and bool(d["g"][b].any()) == (kind == "b")
    for b in kd.REGULAR:
        assert all(np.array_equal(d[k][b], twin[k][b]) for k in "GCgc")
    for b in range(kd.B):
        assert np.array_equal(d["G"][b], twin["G"][b]) and np.array_equal(d["C"][b], twin["C"][b])


@pytest.mark.parametrize("dtype,tol", [(F32, 1e-10), (F64, 1e-22)])
@pytest.mark.parametrize("shape,kind", CASES)
def test_oracle_verdict_and_dense_solution(shape, kind, dtype, tol):
    """The oracle on S of the fp64 formation and the gamma of the batch, from lambda = 0, identity preconditioner, max_iter = 7."""
    nx, nu, N = shape
    d, _ = kd.batch(nx, nu, N, kind)
    deg, reg = kd.expected_masks()
    parts = [so.form_schur(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b]) for b in range(kd.B)]
    S = np.stack([p[0] for p in parts]).astype(dtype)
    gamma = np.stack([kd.gamma_formula(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b], dtype) for b in range(kd.B)])
    assert not gamma[deg].any() and gamma[reg].any(axis=1).all()
    out = orc.pcg_batch(nx, N, kd.B, S, None, gamma, tol=tol, max_iter=7)
    lam = np.asarray(out["lambda_"]).reshape(kd.B, -1)
    iters, flags = np.asarray(out["iters"]).reshape(-1), np.asarray(out["max_iter_exit"]).reshape(-1).astype(bool)
    assert (iters[deg] == 7).all() and flags[deg].all()
    assert not np.isfinite(lam[deg]).any()
    assert np.isfinite(lam[reg]).all()
    for b in kd.REGULAR:
        z, l = so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        assert np.isfinite(z).all() and np.isfinite(l).all() and z.any()


def test_add_rho_is_the_dense_shift():
    nx, nu, N = 5, 3, 4
    d, _ = kd.batch(5, 3, 10, "a")
    G = so.gen(nx, nu, N, seed=1)["G"][0]
    Gd = so.dense_kkt(nx, nu, N, G, np.zeros(so.sizes(nx, nu, N)["C"]), np.zeros(so.sizes(nx, nu, N)["g"]), np.zeros(nx * N))[0]
    Gr = so.dense_kkt(nx, nu, N, kd.add_rho(nx, nu, N, G, 0.75), np.zeros(so.sizes(nx, nu, N)["C"]), np.zeros(so.sizes(nx, nu, N)["g"]),
                      np.zeros(nx * N))[0]
    assert np.array_equal(Gr, Gd + 0.75 * np.eye(Gd.shape[0])) and d["G"].shape[0] == kd.B
