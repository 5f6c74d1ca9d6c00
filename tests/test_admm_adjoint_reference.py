"""CPU-only: the reference of the box QP's backward pass (tests/admm_adjoint_ref.py) against what it has to equal.

 1. The masked update, the init and grad_bounds equal, bit for bit, admm_ref.update_ref on the explicit degenerate box (lo = hi = +0
    where yf != 0, -Inf / +Inf elsewhere) resp. the formula evaluated entry by entry, on inputs with +-0, NaN, +-Inf and a NaN in yf.
 2. The pinned fixture is strictly complementary: in every problem at least one entry at lo, one at hi and one free, every active
    |y| and every free entry's distance to its bounds above admm_adjoint_ref.MARGIN.  A condition on the inputs; the fp64 forward
    reference alone has to meet it.
 3. The reference adjoint loop, run to convergence, gives the pair and the multiplier of the dense reduced KKT system with the rows
    and columns of the active set pinned, and through them the same gradients in G, C, g, c, lo, hi.
 4. Central differences of the dense active-set solve are a second witness for those gradients (the docstring of the test has the
    observed figures).
"""
import numpy as np
import pytest

import admm_adjoint_ref as ar
import admm_ref
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64


def same_bits(a, b):
    """Bit for bit; a NaN need only meet a NaN (both sides run the same numpy operations, but the payload is not part of the claim)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    ua = np.where(na, 0, a).astype(a.dtype).view(np.uint8)
    ub = np.where(nb, 0, b).astype(b.dtype).view(np.uint8)
    return np.array_equal(na, nb) and np.array_equal(ua, ub)


def special_data(dtype, B=3, nz=41, seed=5):
    """Order-1 data with every special value planted in every array: +-0, NaN, +-Inf; yf is 0 on about half of the entries, has both
    signs, -0 (free: -0 != 0 is false) and a NaN (active)."""
    rng = np.random.default_rng(seed)
    az, w, y, gz = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    yf = np.where(rng.random((B, nz)) < 0.5, 0.0, rng.standard_normal((B, nz))).astype(dtype)
    specials = [0.0, -0.0, np.nan, np.inf, -np.inf]
    for k, a in enumerate((az, w, y, gz)):
        for j, s in enumerate(specials):
            a[0, (7 * k + 5 * j) % nz] = s            # problem 0 takes them all; the masks below put each under both kinds of entry
            a[1, (3 * k + 11 * j + 1) % nz] = s
    yf[0, :12] = 0.0
    yf[0, 12:24] = rng.standard_normal(12).astype(dtype)
    yf[1, 3], yf[1, 4], yf[2, 5] = np.nan, -0.0, np.nan
    rho = np.array([0.5, 3.0, 2.25], dtype)
    return dict(az=az, w=w, y=y, gz=gz, yf=yf, rho=rho)


@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_masked_update_is_the_box_update_on_the_degenerate_box(dtype, init):
    d = special_data(dtype)
    lo, hi = ar.degenerate_box(d["yf"], dtype)
    assert np.isnan(d["yf"]).sum() == 2 and (lo[np.isnan(d["yf"])] == 0).all() and (hi[np.isnan(d["yf"])] == 0).all()
    assert np.isinf(lo[1, 4]) and not np.signbit(lo[d["yf"] != 0]).any() and not np.signbit(hi[d["yf"] != 0]).any()
    az = None if init else d["az"]
    got = ar.update_ref(dtype, d["gz"], d["yf"], d["rho"], az, d["w"], d["y"])
    want = admm_ref.update_ref(dtype, d["gz"], lo, hi, d["rho"], az, d["w"], d["y"])
    for name, a, b in zip(("w", "y", "t"), got[:3], want[:3]):
        assert same_bits(a, b), name
    assert (got[3] == want[3]).all(), "gt"       # exact rationals, None where not finite
    if init:
        assert got[4] is None and want[4] is None
    else:
        assert same_bits(got[4], want[4]), "res"
        assert np.isnan(got[4][0]).all() and np.isfinite(got[4][2]).all()      # NaN is its problem's norm, and stays there
    # the structure: pinned entries are 0 or NaN, free entries pass through with y+ = 0
    w, y = got[0], got[1]
    m = d["yf"] != 0
    v = d["w"] if init else d["az"] + d["y"]
    assert (np.isnan(w[m]) | (w[m] == 0)).all() and same_bits(w[~m], v[~m])
    if not init:
        fin = ~m & np.isfinite(v)
        assert not y[fin].any()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_grad_bounds_formula(dtype):
    d = special_data(dtype)
    glo, ghi = ar.grad_bounds_ref(dtype, d["yf"], d["rho"], d["y"])
    assert glo.dtype == np.dtype(dtype) and ghi.dtype == np.dtype(dtype)
    B, nz = d["yf"].shape
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for i in range(nz):
                n = -(d["rho"][b] * d["y"][b, i])
                assert isinstance(n, dtype)
                f = d["yf"][b, i]
                assert same_bits(glo[b, i], n if f < 0 else dtype(0.0)), (b, i)
                assert same_bits(ghi[b, i], n if f > 0 else dtype(0.0)), (b, i)
    nan = np.isnan(d["yf"])
    assert not glo[nan].view(np.uint8).any() and not ghi[nan].view(np.uint8).any()      # a NaN yf: +0 on both sides
    assert not (glo[d["yf"] >= 0].view(np.uint8).any() or ghi[d["yf"] <= 0].view(np.uint8).any())


@pytest.mark.parametrize("nx,nu,N,B", ar.FIXTURE_SHAPES)
def test_fixture_is_strictly_complementary(nx, nu, N, B):
    d, lo, hi, gz, glam = ar.fixture(nx, nu, N, B)
    for a in list(d.values()) + [lo, hi, gz, glam]:
        fin = np.isfinite(a)
        assert np.array_equal(a[fin].astype(F32).astype(F64), a[fin])       # fp32 numbers: both precisions get the same problem
    for b, r in enumerate(ar.reference(nx, nu, N, B)):
        A = r["at_lo"] | r["at_hi"]
        assert r["at_lo"].any() and r["at_hi"].any() and (~A).any(), b
        assert (r["w"][r["at_lo"]] == lo[b][r["at_lo"]]).all() and (r["w"][r["at_hi"]] == hi[b][r["at_hi"]]).all()
        active, free = np.abs(r["y"][A]).min(), np.minimum(r["w"] - lo[b], hi[b] - r["w"])[~A].min()
        print(f"({nx},{nu},{N}) problem {b}: {int(r['at_lo'].sum())} at lo, {int(r['at_hi'].sum())} at hi, {int((~A).sum())} free; "
              f"min active |y| {active:.3e}, min free distance {free:.3e} (margin {ar.MARGIN:.0e})")
        assert active > ar.MARGIN and free > ar.MARGIN
        # the loop's point is the KKT point of its own active set, with multipliers of the right sign
        z, lam, mu = ar.active_set_solve(r["Gd"], r["Cd"], r["g"], r["c"], lo[b], hi[b], r["at_lo"], r["at_hi"])
        assert np.abs(z - r["w"]).max() <= 1e-12 and np.abs(mu - ar.FIXTURE_RHO[b] * r["y"]).max() <= 1e-11
        assert (mu[r["at_lo"]] < 0).all() and (mu[r["at_hi"]] > 0).all()


# fp64 roundoff 1.1e-16 through the dense inverse of a KKT matrix whose condition number is below 1e4 for these problems (cost
# eigenvalues in [1, 30], dynamics of spectral radius about 1), with a factor 100 for the few thousand operations per entry
LOOP_TOL = 1e-10


@pytest.mark.parametrize("nx,nu,N,B", ar.FIXTURE_SHAPES)
def test_adjoint_loop_converges_to_the_pinned_dense_solve(nx, nu, N, B):
    d, lo, hi, gz, glam = ar.fixture(nx, nu, N, B)
    for b, r in enumerate(ar.reference(nx, nu, N, B)):
        rho = ar.FIXTURE_RHO[b]
        lp = ar.adjoint_loop(r["Gd"], r["Cd"], gz[b], -glam[b], r["y"], rho, 3000)
        wa, alam, ya = lp["wa"][-1], lp["alam"][-1], lp["ya"][-1]
        A = r["at_lo"] | r["at_hi"]
        assert not wa[A].view(np.uint64).any() and not r["az"][A].any()          # a_z is EXACTLY zero on the active set
        assert not ya[~A].any()
        glo, ghi = ar.grad_bounds_ref(F64, r["y"].reshape(1, -1), [rho], ya.reshape(1, -1))
        got = ar.gradients(nx, nu, N, r["w"], r["lam"], wa, alam, rho * ya, r["at_lo"], r["at_hi"])
        assert same_bits(got["lo"], glo[0] + 0.0) and same_bits(got["hi"], ghi[0] + 0.0)     # (+ 0.0: -0 and +0 are one gradient)
        for k, a, ref in [("az", wa, r["az"]), ("alam", alam, r["alam"]), ("nu", rho * ya, r["nu"])] + \
                [("d" + k, got[k], r["grads"][k]) for k in ("G", "C", "g", "c", "lo", "hi")]:
            err = np.abs(a - ref).max() / np.abs(ref).max()
            print(f"({nx},{nu},{N}) problem {b} {k}: {err:.2e}")
            assert err <= LOOP_TOL, (b, k, err)
        assert np.abs(r["grads"]["lo"]).max() > 0 and np.abs(r["grads"]["hi"]).max() > 0


def loss_along(nx, nu, N, d, lo, hi, gz, glam, b, r, direction, t):
    """l = gz' z + glam' lambda at the parameters moved by t along `direction`, through the dense solve on the reference's active set;
    G enters symmetrised, as the library reads it.  Returns (l, whether that set is still the optimal one)."""
    p = {k: d[k][b] + t * direction[k] for k in "GCgc"}
    lo_t, hi_t = lo[b].copy(), hi[b].copy()
    fin = np.isfinite(lo[b])
    lo_t[fin] += t * direction["lo"][fin]
    hi_t[fin] += t * direction["hi"][fin]
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, p["G"], p["C"], p["g"], p["c"])
    Gd = 0.5 * (Gd + Gd.T)
    z, lam, mu = ar.active_set_solve(Gd, Cd, g, c, lo_t, hi_t, r["at_lo"], r["at_hi"])
    A = r["at_lo"] | r["at_hi"]
    optimal = (mu[r["at_lo"]] < 0).all() and (mu[r["at_hi"]] > 0).all() and (z[~A] > lo_t[~A]).all() and (z[~A] < hi_t[~A]).all()
    return float(gz[b] @ z + glam[b] @ lam), bool(optimal)


@pytest.mark.parametrize("nx,nu,N,B", ar.FIXTURE_SHAPES)
def test_central_differences_are_a_second_witness(nx, nu, N, B):
    """Directional central differences of l = gz' w + glam' lambda through the dense active-set fp64 solve at the steps h = 2^-10 and
    2^-11, against <gradient, direction>: along one direction that moves all six parameter groups at once, and along one direction per
    group.  The active set must not change at any of the perturbed points.  No tolerance is fixed in advance; the yardstick is the
    reference's own curve.  l is a rational function of G and C, so along the joint direction the discrepancy is the h^2 term of the
    difference quotient and must fall by about 4 (asserted: between 3.5 and 4.5) when h halves.  A single group does the same, or
    its quotient is EXACT: for a fixed active set (w, lambda) is linear in g, c, lo and hi -- and in G too where every input is
    clamped, problem 1 of (3,2,4): the dynamics then fix w -- so the central difference has no h^2 term and what is left is
    roundoff, asserted as at least three orders below the joint direction's discrepancy at the smaller step.  g, c, lo and hi
    must be exact.
    Observed (relative to |<gradient, direction>| of the joint direction; h = 2^-10 -> 2^-11):
      (3,2,4)  problem 0: all 2.21e-05 -> 5.53e-06 (4.00), C 8.81e-08 -> 2.20e-08 (4.00), G 6.5e-12 -> 1.7e-12, g/c/lo/hi <= 2.5e-13
               problem 1: all 1.69e-06 -> 4.23e-07 (4.00), C 5.72e-07 -> 1.43e-07 (4.00), G <= 3.3e-13,        g/c/lo/hi <= 2.5e-14
      (14,7,3) problem 0: all 1.18e-05 -> 2.94e-06 (4.00), C 4.82e-06 -> 1.21e-06 (4.00), G 5.3e-11 -> 1.3e-11, g/c/lo/hi <= 4.9e-13
               problem 1: all 3.29e-05 -> 8.22e-06 (4.00), C 5.89e-06 -> 1.47e-06 (4.00), G 2.5e-10 -> 6.4e-11, g/c/lo/hi <= 6.2e-14
    (G alone leaves an h^2 term four orders below C's on these problems; it falls by 4 as well and counts as exact by the rule.)"""
    d, lo, hi, gz, glam = ar.fixture(nx, nu, N, B)
    rng = np.random.default_rng(77)
    steps = (2.0 ** -10, 2.0 ** -11)
    for b, r in enumerate(ar.reference(nx, nu, N, B)):
        full = {k: rng.standard_normal(r["grads"][k].shape) for k in ("G", "C", "g", "c", "lo", "hi")}
        zero = {k: np.zeros_like(v) for k, v in full.items()}
        fin = np.isfinite(lo[b])

        def discrepancy(direction):
            want = sum(float(r["grads"][k] @ direction[k]) for k in ("G", "C", "g", "c")) + \
                sum(float(r["grads"][k][fin] @ direction[k][fin]) for k in ("lo", "hi"))
            out = []
            for h in steps:
                (lp, okp), (lm, okm) = (loss_along(nx, nu, N, d, lo, hi, gz, glam, b, r, direction, s * h) for s in (1, -1))
                assert okp and okm, "the active set changed"
                out.append(abs((lp - lm) / (2 * h) - want))
            return want, out

        want, joint = discrepancy(full)
        scale = abs(want)
        print(f"({nx},{nu},{N}) problem {b}: all groups {joint[0] / scale:.2e} -> {joint[1] / scale:.2e} (ratio {joint[0] / joint[1]:.2f})")
        assert 3.5 <= joint[0] / joint[1] <= 4.5
        for k in ("G", "C", "g", "c", "lo", "hi"):
            _, e = discrepancy({**zero, k: full[k]})
            exact = max(e) <= 1e-3 * joint[1]
            print(f"    {k}: {e[0] / scale:.2e} -> {e[1] / scale:.2e}" + (" (exact)" if exact else f" (ratio {e[0] / e[1]:.2f})"))
            assert exact or 3.5 <= e[0] / e[1] <= 4.5, k
            assert exact or k in "GC", k
