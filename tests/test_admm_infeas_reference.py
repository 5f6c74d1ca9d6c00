"""CPU checks of the infeasibility certificate's references (tests/admm_infeas_ref.py): the mathematics on the pinned infeasible
fixture in fp64, the exact definition (box form against rows form at E = I, both dtypes, against the dense evaluation), detection
with the pinned iterations, no false alarm on any feasible fixture over every iterate, the choice of EPS, and the Farkas pair
recovered densely from the limiting iterates."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import admm_infeas_ref as ir  # noqa: E402
import admm_lin_ref as lr  # noqa: E402
import admm_ref  # noqa: E402
import admm_soft_ref as sr  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

NX, NU, N, B = admm_ref.CONV_SHAPE
DTYPES = [np.float64, np.float32]


def test_differences_of_the_hard_iterates_tend_to_a_certificate():
    """Through admm_ref.admm in fp64, before any device code: the gap sits in entry 0 of knot 0, dl_0[0] -> -rho dy_0 and the support
    value -> (hi_0 - c_0) rho dy_0 = -INFEAS_GAP rho dy_0."""
    d, lo, hi, _ = sr.infeasible_inputs()
    for b, h in enumerate(sr.infeasible_reference(sr.INFEAS_K, False)):
        rho = admm_ref.CONV_RHO[b]
        _, Cd, _, c = so.dense_kkt(NX, NU, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        dl, dy = h["lam"][-1] - h["lam"][-2], h["y"][-1] - h["y"][-2]
        assert abs(dy[0] - sr.INFEAS_GAP) < 5e-3 * sr.INFEAS_GAP            # E z - w has settled at the gap, in entry 0
        assert np.abs(np.delete(dy, 0)).max() < 5e-3 * sr.INFEAS_GAP
        assert abs(dl[0] / (-rho * dy[0]) - 1) < 5e-3
        n, r, sigma, _ = ir.cert_dense(np.float64, Cd, None, c, lo[b], hi[b], rho, h["lam"][-2], h["lam"][-1], h["y"][-2], h["y"][-1], ir.EPS)
        assert abs(sigma / (-sr.INFEAS_GAP * rho * dy[0]) - 1) < 5e-3
        assert abs(hi[b, 0] - c[0] + sr.INFEAS_GAP) < 1e-7                   # (hi is rounded to fp32)
        assert r < 5e-3 * n


@pytest.mark.parametrize("index", range(B))
def test_loop_in_fp64_gives_the_iterates_of_the_references(index):
    h = ir.history("infeasible", index, "float64", sr.INFEAS_K)
    ref = sr.infeasible_reference(sr.INFEAS_K, False)[index]
    for k in ("lam", "y", "r_prim", "r_dual"):
        assert np.array_equal(h[k], ref[k]), k
    name, Gd, Cd, Ed, g, c, lo, hi, rho = ir.feasible_problems()[B + index]
    assert name == "admm_lin_ref"
    ref = lr.convergence_reference(50)[index]
    h = ir.loop(np.float64, Gd, Cd, Ed, g, c, lo, hi, rho, 50)
    for k in ("lam", "y", "r_prim", "r_dual"):
        assert np.array_equal(h[k], ref[k]), k


small_inputs = ir.random_inputs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,Nk,Bk", [(3, 2, 4, 3), (2, 1, 1, 2)])
def test_box_form_is_the_rows_form_at_identity(nx, nu, Nk, Bk, dtype):
    a = small_inputs(nx, nu, 0, 0, Nk, Bk, 5, dtype, box=True)
    box = ir.cert_ref(dtype, nx, nu, 0, 0, Nk, a["C"], a["c"], None, a["lo"], a["hi"], a["rho"], a["lam0"], a["lam1"], a["y0"], a["y1"], 0.5)
    rows = ir.cert_ref(dtype, nx, nu, nx, nu, Nk, a["C"], a["c"], ir.box_as_rows(nx, nu, Nk, Bk, dtype), a["lo"], a["hi"], a["rho"],
                       a["lam0"], a["lam1"], a["y0"], a["y1"], 0.5)
    assert box[0].dtype == np.dtype(dtype)
    assert np.array_equal(box[0].view(np.uint8), rows[0].view(np.uint8)) and np.array_equal(box[1], rows[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,Nk,Bk,mx,mu", [(3, 2, 5, 2, 2, 1), (3, 2, 4, 2, 0, 2), (3, 2, 4, 2, 2, 0), (2, 1, 1, 2, 1, 1)])
def test_exact_definition_agrees_with_the_dense_evaluation(nx, nu, Nk, Bk, mx, mu, dtype):
    """cert_ref works on the packed layouts with one rounding per fma, cert_dense on dense matrices with numpy: the same numbers to
    rounding (the chains are at most nx + max(mx, mu) terms, the knot sums sw + nx, of numbers of order 1 to 10)."""
    a = small_inputs(nx, nu, mx, mu, Nk, Bk, 9, dtype)
    a["lo"][0], a["hi"][0] = np.maximum(a["lo"][0], -3), np.minimum(a["hi"][0], 3)      # problem 0: every bound finite
    cert, _ = ir.cert_ref(dtype, nx, nu, mx, mu, Nk, a["C"], a["c"], a["E"], a["lo"], a["hi"], a["rho"], a["lam0"], a["lam1"], a["y0"],
                          a["y1"], 0.5)
    tol = 64 * np.finfo(dtype).eps
    for b in range(Bk):
        zero = np.zeros(1)
        Cd = so.dense_kkt(nx, nu, Nk, np.zeros((nx * nx + nu * nu) * Nk - nu * nu), a["C"][b] if Nk > 1 else zero[:0],
                          np.zeros((nx + nu) * Nk - nu), a["c"][b])[1]
        Ed = lr.dense_E(nx, nu, mx, mu, Nk, a["E"][b])
        n, r, sigma, _ = ir.cert_dense(np.float64, Cd, Ed, a["c"][b], a["lo"][b], a["hi"][b], a["rho"][b], a["lam0"][b], a["lam1"][b],
                                       a["y0"][b], a["y1"][b], 0.5)
        scale = max(1.0, np.abs(a["lo"][b][np.isfinite(a["lo"][b])]).max(initial=0), np.abs(a["hi"][b][np.isfinite(a["hi"][b])]).max(initial=0))
        assert abs(cert[b, 0] - n) <= tol * n
        assert abs(cert[b, 1] - r) <= tol * 16 * n
        if np.isfinite(sigma):
            assert abs(cert[b, 2] - sigma) <= tol * 64 * n * scale
        else:                        # a row that moved towards an infinite bound: the same infinity in both
            assert cert[b, 2] == sigma


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_infinite_bounds_in_the_definition(dtype):
    nx, nu, Nk, Bk, mx, mu = 3, 2, 4, 3, 2, 1
    a = small_inputs(nx, nu, mx, mu, Nk, Bk, 13, dtype)
    args = lambda d: (dtype, nx, nu, mx, mu, Nk, d["C"], d["c"], d["E"], d["lo"], d["hi"], d["rho"], d["lam0"], d["lam1"], d["y0"], d["y1"], 0.5)  # noqa: E731
    clean = ir.cert_ref(*args(a))
    bad = {k: (None if v is None else v.copy()) for k, v in a.items()}
    bad["y1"][1, 2] = np.nan
    bad["hi"][1, :] = np.inf           # dy = 0 rows must not multiply them
    bad["y1"][1, 0] = bad["y0"][1, 0]
    cert, flag = ir.cert_ref(*args(bad))
    assert np.isnan(cert[1, 0]) and np.isnan(cert[1, 1]) and flag[1] == 0
    for b in (0, 2):
        assert np.array_equal(cert[b].view(np.uint8), clean[0][b].view(np.uint8)) and flag[b] == clean[1][b]


@pytest.mark.parametrize("dtype,pinned", [(np.float64, ir.FLAG_AT_F64), (np.float32, ir.FLAG_AT_F32)])
@pytest.mark.parametrize("index", range(B))
def test_detection_on_the_infeasible_fixture(index, dtype, pinned):
    """r / n falls, sigma / n settles at -INFEAS_GAP rho dy_0 / n = -0.5 n / n, and the flag is first set at the pinned iteration and
    stays set."""
    _, _, Cd, Ed, _, c, lo, hi, rho = ir.infeasible_problems()[index]
    h = ir.history("infeasible", index, np.dtype(dtype).name, sr.INFEAS_K)
    n, r, sigma, flag = ir.sweep(dtype, Cd, Ed, c, lo, hi, rho, h)
    ratio = r / n
    assert ratio[-1] < 2e-3 and ratio[-1] < 0.05 * ratio[2]
    assert np.all(ratio[10:] <= 1.001 * ratio[9:-1])                     # falls, iteration by iteration, from iteration 11 on
    assert np.all(sigma[1:] < 0) and abs(sigma[-1] / n[-1] + sr.INFEAS_GAP) < 5e-3
    assert ir.first_flag(flag) == pinned[index]
    assert flag[pinned[index] - 2:].all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(3 * B))
def test_no_false_alarm_on_the_feasible_fixtures(index, dtype):
    """Every iterate pair (k - 1, k) up to FEASIBLE_K, the iterations close to and past convergence included: never flagged, and where
    the support value is negative the residual stays a fixed fraction of the scale."""
    name, _, Cd, Ed, _, c, lo, hi, rho = ir.feasible_problems()[index]
    h = ir.history("feasible", index, np.dtype(dtype).name, ir.FEASIBLE_K)
    assert max(h["r_prim"][-1], h["r_dual"][-1]) < 64 * np.finfo(dtype).eps      # the sweep does reach convergence
    n, r, sigma, flag = ir.sweep(dtype, Cd, Ed, c, lo, hi, rho, h)
    assert not flag.any(), (name, ir.first_flag(flag))
    risky = (sigma < 0) & (n > 0)
    assert np.all(r[risky] >= ir.FEASIBLE_MIN_RATIO * n[risky])


def test_eps_is_the_largest_power_of_ten_that_separates():
    """0.1 holds both conditions (the two tests above); 1 cannot flag the infeasible fixture in either precision: sigma / n settles at
    -0.5 and never goes below -1."""
    for dtype in DTYPES:
        for index in range(B):
            _, _, Cd, Ed, _, c, lo, hi, rho = ir.infeasible_problems()[index]
            h = ir.history("infeasible", index, np.dtype(dtype).name, sr.INFEAS_K)
            assert not ir.sweep(dtype, Cd, Ed, c, lo, hi, rho, h, eps=1.0)[3].any()
            assert ir.sweep(dtype, Cd, Ed, c, lo, hi, rho, h, eps=ir.EPS)[3].any()
    assert ir.EPS == 0.1


@pytest.mark.parametrize("index", range(B))
def test_limiting_pair_is_a_farkas_pair(index):
    """Dense, from the last two iterates: C'dl + dm is small against the pair, the support of the box in direction dm plus c'dl is
    negative -- so the hyperplane dm separates the affine set {Cz = c} from the box: dm'z = -dl'c for every such z, above the
    largest dm'w over the box."""
    _, Gd, Cd, _, g, c, lo, hi, rho = ir.infeasible_problems()[index]
    h = ir.history("infeasible", index, "float64", sr.INFEAS_K)
    dl, dm = h["lam"][-1] - h["lam"][-2], rho * (h["y"][-1] - h["y"][-2])
    scale = max(np.abs(dl).max(), np.abs(dm).max())
    assert np.abs(Cd.T @ dl + dm).max() < 2e-3 * scale
    # the exact certificate behind it: project dm onto the range of -C' (least squares), which changes it by that residual
    dl_x = np.linalg.lstsq(Cd.T, -dm, rcond=None)[0]
    dm_x = -Cd.T @ dl_x
    assert np.abs(dm_x - dm).max() < 4e-3 * scale
    assert np.abs(dm_x[1:]).max() < 4e-3 * scale      # the infinite bounds meet (numerically) zero multipliers: leave them out
    support = hi[0] * dm_x[0] if dm_x[0] > 0 else lo[0] * dm_x[0]
    assert c @ dl_x + support < -0.4 * scale * sr.INFEAS_GAP
    z0 = np.linalg.lstsq(Cd, c, rcond=None)[0]          # a point of {Cz = c}
    assert np.abs(Cd @ z0 - c).max() < 1e-9
    assert dm_x[0] * z0[0] > support + 0.4 * scale * sr.INFEAS_GAP
