"""CPU pins of the soft-bound references (tests/admm_soft_ref.py): with kappa = +Inf they ARE the hard references, a finite kappa
gives a point that satisfies the optimality conditions of the L1-penalised problem, a kappa above the hard multiplier gives the hard
solution, and the infeasible-hard fixture is what it claims.  The figures the device tests read are pinned here; run with -s."""
import numpy as np
import pytest

import admm_lin_ref
import admm_ref
import admm_soft_ref as sr
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
KEYS = ("z", "lam", "w", "y", "gt", "r_prim", "r_dual", "gt0")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_infinite_kappa_is_the_hard_box_history():
    nx, nu, N, B = admm_ref.CONV_SHAPE
    d, lo, hi, _ = admm_ref.convergence_inputs()
    hard = admm_ref.convergence_reference(4000)
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        zero = np.zeros(g.size)
        h = sr.admm_soft(Gd, Cd, g, c, lo[b], hi[b], np.full(g.size, np.inf), admm_ref.CONV_RHO[b], 120, zero, zero)
        for k in KEYS:
            assert same(h[k], hard[b][k][:120] if k != "gt0" else hard[b][k]), (b, k)


def test_infinite_kappa_is_the_hard_rows_history():
    nx, nu, N, B = admm_lin_ref.CONV_SHAPE
    mx, mu = admm_lin_ref.CONV_ROWS
    d, E, lo, hi, _ = admm_lin_ref.convergence_inputs()
    hard = admm_lin_ref.convergence_reference(4000)
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = admm_lin_ref.dense_E(nx, nu, mx, mu, N, E[b])
        zero = np.zeros(lo[b].size)
        h = sr.admm_lin_soft(Gd, Cd, Ed, g, c, lo[b], hi[b], np.full(lo[b].size, np.inf), admm_lin_ref.CONV_RHO[b], 120, zero, zero)
        for k in KEYS:
            assert same(h[k], hard[b][k][:120] if k != "gt0" else hard[b][k]), (b, k)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_infinite_kappa_is_the_hard_update_ref(dtype):
    rng = np.random.default_rng(5)
    B, nz = 3, 41
    z, w, y, g = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    lo, hi = (-0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype), (0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype)
    lo[rng.random((B, nz)) < 0.3], hi[rng.random((B, nz)) < 0.3] = -np.inf, np.inf
    rho, inf = rng.uniform(0.5, 4.0, B).astype(dtype), np.full((B, nz), np.inf, dtype)
    for zz in (z, None):
        a, b = admm_ref.update_ref(dtype, g, lo, hi, rho, zz, w, y), sr.update_ref(dtype, g, lo, hi, inf, rho, zz, w, y)
        assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2]) and (a[3] == b[3]).all()
        assert zz is None or same(a[4], b[4])
    # rows: E = a random packed E
    nx, nu, mx, mu, N = 3, 2, 2, 1, 4
    nzl, nw, ne, _ = admm_lin_ref.sizes(nx, nu, mx, mu, N)
    E, g, z = (rng.standard_normal((B, n)).astype(dtype) for n in (ne, nzl, nzl))
    w, y = (rng.standard_normal((B, nw)).astype(dtype) for _ in range(2))
    lo, hi, inf = np.full((B, nw), -0.3, dtype), np.full((B, nw), 0.3, dtype), np.full((B, nw), np.inf, dtype)
    for zz in (z, None):
        a = admm_lin_ref.update_ref(dtype, nx, nu, mx, mu, N, g, E, lo, hi, rho, zz, w, y)
        b = sr.lin_update_ref(dtype, nx, nu, mx, mu, N, g, E, lo, hi, inf, rho, zz, w, y)
        assert all(same(p, q) for p, q in zip(a[:3], b[:3])) and (zz is None or same(a[3], b[3]))


def test_soft_update_lines():
    """kappa = 0 frees the row, a tie takes the hard branch, |y| <= theta, NaN stays NaN, init clips only the hard rows."""
    for dtype in (F32, F64):
        rho, hi, lo = dtype(2.0), dtype(1.0), dtype(-1.0)
        theta = dtype(dtype(0.75) / rho)
        s = np.array([hi + theta, lo - theta, 5.0, -5.0, 0.5, np.nan, 5.0, 5.0], dtype)     # two ties first
        kap = np.array([0.75, 0.75, 0.75, 0.75, 0.75, 0.75, 0.0, np.inf], dtype)
        assert s[0] - hi == theta and s[1] - lo == -theta
        w, y = sr.soft(s, lo, hi, kap, rho)
        assert same(w[:2], np.array([hi, lo], dtype)) and same(y[:2], np.array([theta, -theta], dtype))       # the third branch
        assert w[2] == dtype(5.0) - theta and y[2] == theta and w[3] == dtype(-5.0) + theta and y[3] == -theta
        assert w[4] == dtype(0.5) and y[4] == 0 and np.isnan(w[5]) and np.isnan(y[5])
        assert w[6] == dtype(5.0) and y[6] == 0 and w[7] == hi and y[7] == dtype(4.0)
        wi = sr.soft_init(np.array([3.0, 3.0], dtype), lo, hi, np.array([1.0, np.inf], dtype))
        assert same(wi, np.array([3.0, 1.0], dtype))


def test_finite_kappa_meets_the_soft_optimality_conditions():
    nx, nu, N, B = sr.CONV_SHAPE
    d, lo, hi, kappa = sr.soft_inputs()
    ref = sr.soft_reference(4000)
    tol = 1e-9
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        z, lam, mu = ref[b]["z"][-1], ref[b]["lam"][-1], sr.CONV_RHO[b] * ref[b]["y"][-1]
        assert ref[b]["r_prim"][-1] < 1e-12 and ref[b]["r_dual"][-1] < 1e-12
        stat = np.linalg.norm(Gd @ z + g + Cd.T @ lam + mu) / np.linalg.norm(g)
        feas = np.linalg.norm(Cd @ z - c) / max(np.linalg.norm(c), 1.0)
        assert stat < 1e-10 and feas < 1e-10, (b, stat, feas)
        assert (np.abs(mu) <= kappa[b] * (1 + 1e-12)).all()
        above, below = z - hi[b] > tol, lo[b] - z > tol
        inside = (z < hi[b] - tol) & (z > lo[b] + tol)
        assert np.allclose(mu[above], kappa[b][above], rtol=1e-9, atol=0) and np.allclose(mu[below], -kappa[b][below], rtol=1e-9, atol=0)
        assert not mu[inside].any()
        at_hi, at_lo = np.abs(z - hi[b]) <= tol, np.abs(z - lo[b]) <= tol
        assert (mu[at_hi] >= 0).all() and (mu[at_lo] <= 0).all()
        violated = int(above.sum() + below.sum())
        held = int((((at_hi | at_lo)) & (np.abs(mu) > tol) & (np.abs(mu) < kappa[b] * (1 - 1e-6))).sum())
        ratio = ref[b]["r_prim"][sr.SOFT_K - 1] / ref[b]["r_prim"][0]
        print(f"problem {b}: kappa {kappa[b, 0]:.4f}, {violated} rows violated, {held} at their bound with |mu| < kappa, stationarity "
              f"{stat:.1e}, r_prim({sr.SOFT_K})/r_prim(1) {ratio:.3e}")
        assert violated > 0 and held > 0
    worst = max(h["r_prim"][sr.SOFT_K - 1] / h["r_prim"][0] for h in ref)
    assert abs(worst - sr.SOFT_RATIO_REF) <= 0.01 * sr.SOFT_RATIO_REF, worst     # the figure the device test's bound is derived from


def test_exact_penalty():
    nx, nu, N, B = sr.CONV_SHAPE
    d, lo, hi, _ = admm_ref.convergence_inputs()
    hard, mu = admm_ref.convergence_reference(4000), sr.hard_multipliers()
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        zero = np.zeros(g.size)
        kap = np.full(g.size, 2.0 * np.abs(mu[b]).max())
        h = sr.admm_soft(Gd, Cd, g, c, lo[b], hi[b], kap, sr.CONV_RHO[b], 4000, zero, zero)
        err = np.linalg.norm(h["z"][-1] - hard[b]["z"][-1]) / np.linalg.norm(hard[b]["z"][-1])
        print(f"problem {b}: kappa = 2 max|mu_hard| = {kap[0]:.3f}: soft against hard {err:.2e}")
        assert err < 1e-10 and np.linalg.norm(sr.CONV_RHO[b] * h["y"][-1] - mu[b]) <= 1e-9 * np.linalg.norm(mu[b])


def test_infeasible_fixture():
    """Hard: r_prim never falls below the gap and ||y|| grows at every iteration.  Soft: converges.  Pins the two figures."""
    d, lo, hi, kappa = sr.infeasible_inputs()
    assert (hi[:, 0] < d["c"][:, 0] - 0.49).all()       # the bound excludes the x_0 that c pins
    hard, soft = sr.infeasible_reference(sr.INFEAS_K, False), sr.infeasible_reference(200, True)
    floor = min(float(h["r_prim"].min()) for h in hard)
    iters = tuple(sr.soft_converged_at(h) for h in soft)
    print(f"hard floor over {sr.INFEAS_K} iterations {floor:.9f}; soft converged (tol {sr.INFEAS_TOL:g}) at {iters}")
    for h in hard:
        assert h["r_prim"].min() >= sr.INFEAS_HARD_FLOOR
        assert (np.diff(np.abs(h["y"]).max(axis=1)) > 0).all() and (np.diff(np.linalg.norm(h["y"], axis=1)) > 0).all()
    assert iters == sr.INFEAS_SOFT_ITERS
    for h in soft:
        assert h["r_prim"][-1] < 1e-2 * sr.INFEAS_TOL and h["r_dual"][-1] < 1e-2 * sr.INFEAS_TOL      # and goes on falling
