"""CPU-only: the reference of the linear-row QP's backward pass (tests/admm_lin_adjoint_ref.py) against what it has to equal.

 1. The masked update and init equal, bit for bit, admm_lin_ref.update_ref on the explicit degenerate rows (lo = hi = +0 where
    yf != 0, -Inf / +Inf elsewhere), on inputs with +-0, NaN and a NaN in yf; with E = I they equal admm_adjoint_ref.update_ref.
 2. grad_ref: glo, ghi, gE entry by entry from the formula.
 3. The pinned fixture is strictly complementary: per problem an active row at lo and one at hi, an active state row and an active
    input row, every active |y| and every free row's distance to its bounds above MARGIN, [C; E_A] of full row rank.  The fp64
    forward reference alone has to meet it.
 4. The reference adjoint loop converges to the dense reduced KKT system with the rows of E_A appended to C, and the counts K_FWD,
    K_ADJ the device tests replay are counts at which the two loops have converged.
 5. Central differences of the dense active-set solve are a second witness for all seven gradients, E included.
"""
import numpy as np
import pytest

import admm_adjoint_ref as ar
import admm_lin_adjoint_ref as la
import admm_lin_ref as lr
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
SPECIAL_SHAPE = (3, 2, 2, 1, 4, 3)      # nx, nu, mx, mu, N, B


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    ua = np.where(na, 0, a).astype(a.dtype).view(np.uint8)
    ub = np.where(nb, 0, b).astype(b.dtype).view(np.uint8)
    return np.array_equal(na, nb) and np.array_equal(ua, ub)


def special_data(dtype, shape=SPECIAL_SHAPE, seed=9):
    """Order-1 data; yf is 0 on about half of the rows, has both signs, -0 (free) and a NaN (active); v and w hold NaN and -0."""
    nx, nu, mx, mu, N, B = shape
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(seed)
    az, gz = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(2))
    w, y = (rng.standard_normal((B, nw)).astype(dtype) for _ in range(2))
    E = rng.standard_normal((B, ne)).astype(dtype)
    yf = np.where(rng.random((B, nw)) < 0.5, 0.0, rng.standard_normal((B, nw))).astype(dtype)
    yf[0, 0], yf[0, 1], yf[1, 2], yf[1, 3], yf[2, 0] = 1.0, -0.0, np.nan, -2.0, 0.0
    az[0, :nx], y[0, 0] = 0.0, -0.0                 # row 0 of problem 0: v = +0 (an all-zero chain), s = +0 + -0 = +0, pinned
    az[1, nx + nu] = np.nan                         # a NaN in x_1 of problem 1: every state row of knot 1 has v = NaN
    w[2, 1], y[2, 3] = -0.0, np.nan
    rho = np.array([0.5, 3.0, 2.25], dtype)[:B]
    return dict(az=az, w=w, y=y, gz=gz, E=E, yf=yf, rho=rho)


@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_masked_update_is_the_rows_update_on_the_degenerate_rows(dtype, init):
    nx, nu, mx, mu, N, B = SPECIAL_SHAPE
    d = special_data(dtype)
    lo, hi = la.degenerate_rows(d["yf"], dtype)
    nan = np.isnan(d["yf"])
    assert nan.sum() == 1 and (lo[nan] == 0).all() and (hi[nan] == 0).all() and np.isinf(lo[0, 1])
    assert not np.signbit(lo[d["yf"] != 0]).any() and not np.signbit(hi[d["yf"] != 0]).any()
    az = None if init else d["az"]
    got = la.update_ref(dtype, nx, nu, mx, mu, N, d["gz"], d["E"], d["yf"], d["rho"], az, d["w"], d["y"])
    want = lr.update_ref(dtype, nx, nu, mx, mu, N, d["gz"], d["E"], lo, hi, d["rho"], az, d["w"], d["y"])
    for name, a, b in zip(("w", "y", "gt"), got[:3], want[:3]):
        assert same_bits(a, b), name
    if init:
        assert got[3] is None and want[3] is None
    else:
        assert same_bits(got[3], want[3]), "res"
        assert np.isnan(got[3][1]).all() and np.isfinite(got[3][0]).all()      # a NaN is its problem's norm, and stays there
    w = got[0]
    m = d["yf"] != 0
    assert (np.isnan(w[m]) | (w[m] == 0)).all()
    if not init:
        fin = ~m & np.isfinite(got[0])
        assert not got[1][fin].any()                # a free row's y+ is exactly 0: s - s


@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_identity_rows_give_the_box_adjoint(dtype, init):
    nx, nu, N, B = 3, 2, 3, 2
    nz = (nx + nu) * N - nu
    rng = np.random.default_rng(4)
    az, gz, w, y = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    yf = np.where(rng.random((B, nz)) < 0.5, 0.0, rng.standard_normal((B, nz))).astype(dtype)
    rho = np.array([0.75, 2.0], dtype)
    E = np.tile(lr.identity_E(nx, nu, N, dtype), (B, 1))
    got = la.update_ref(dtype, nx, nu, nx, nu, N, gz, E, yf, rho, None if init else az, w, y)
    wn, yn, t, gt, res = ar.update_ref(dtype, gz, yf, rho, None if init else az, w, y)
    assert same_bits(got[0], wn) and same_bits(got[1], yn)
    with np.errstate(invalid="ignore"):
        want_gt = np.array([[lr.fma_ref(-rho[b], t[b, i], gz[b, i], dtype) for i in range(nz)] for b in range(B)], dtype)
    assert same_bits(got[2], want_gt)
    if not init:
        assert same_bits(got[3], res)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_grad_formula(dtype):
    nx, nu, mx, mu, N, B = SPECIAL_SHAPE
    d = special_data(dtype)
    rng = np.random.default_rng(3)
    z = rng.standard_normal(d["az"].shape).astype(dtype)
    glo, ghi, gE = la.grad_ref(dtype, nx, nu, mx, mu, N, z, d["az"], d["yf"], d["y"], d["rho"])
    assert glo.dtype == ghi.dtype == gE.dtype == np.dtype(dtype)
    blo, bhi = ar.grad_bounds_ref(dtype, d["yf"], d["rho"], d["y"])
    assert same_bits(glo, blo) and same_bits(ghi, bhi)
    seen = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for m, n, eo, ro, co, _ in lr.blocks(nx, nu, mx, mu, N):
                for j in range(n):
                    for r in range(m):
                        f, a = d["yf"][b, ro + r], d["y"][b, ro + r]
                        p = a * z[b, co + j]
                        assert isinstance(p, dtype)
                        q = lr.fma_ref(f, d["az"][b, co + j], p, dtype)
                        want = d["rho"][b] * q if f != 0 else dtype(0.0)
                        assert same_bits(gE[b, eo + j * m + r], want), (b, eo, j, r)
                        seen += 1
    assert seen == gE.size
    free = d["yf"] == 0          # (-0 too)
    Ed_mask = np.stack([lr.dense_E(nx, nu, mx, mu, N, la.pack_E(nx, nu, mx, mu, N, np.broadcast_to(free[b][:, None], (free.shape[1], z.shape[1])).astype(dtype)))
                        for b in range(B)]) != 0
    dense = np.stack([lr.dense_E(nx, nu, mx, mu, N, gE[b]) for b in range(B)])
    assert not dense[Ed_mask].view(np.uint8).any()              # +0 on the free rows
    assert np.isnan(dense[1][np.isnan(d["yf"][1])]).any()       # a NaN yf is active: its row of gE is NaN through the fma


def fixture_parts(nx, nu, N, B):
    mx, mu = la.FIXTURE_ROWS[(nx, nu, N, B)]
    return (mx, mu) + la.fixture(nx, nu, N, B)


@pytest.mark.parametrize("nx,nu,N,B", la.FIXTURE_SHAPES)
def test_fixture_is_strictly_complementary(nx, nu, N, B):
    mx, mu, d, E, lo, hi, gz, glam = fixture_parts(nx, nu, N, B)
    for a in list(d.values()) + [E, lo, hi, gz, glam]:
        fin = np.isfinite(a)
        assert np.array_equal(a[fin].astype(F32).astype(F64), a[fin])       # fp32 numbers: both precisions get the same problem
    state = la.is_state_row(nx, nu, mx, mu, N)
    for b, r in enumerate(la.reference(nx, nu, N, B)):
        A = r["at_lo"] | r["at_hi"]
        assert r["at_lo"].any() and r["at_hi"].any() and (~A).any(), b
        assert (A & state).any() and (A & ~state).any(), b
        assert (r["w"][r["at_lo"]] == lo[b][r["at_lo"]]).all() and (r["w"][r["at_hi"]] == hi[b][r["at_hi"]]).all()
        v = r["Ed"] @ r["z"]
        active, free = np.abs(r["y"][A]).min(), np.minimum(v - lo[b], hi[b] - v)[~A].min()
        stacked = np.vstack([r["Cd"], r["Ed"][A]])
        print(f"({nx},{nu},{N}) rows ({mx},{mu}) problem {b}: {int(r['at_lo'].sum())} at lo, {int(r['at_hi'].sum())} at hi, "
              f"{int((A & state).sum())} state, {int((A & ~state).sum())} input, {int((~A).sum())} free; min active |y| {active:.3e}, "
              f"min free distance {free:.3e} (margin {la.MARGIN:.0e})")
        assert active >= la.MARGIN and free >= la.MARGIN
        assert np.linalg.matrix_rank(stacked) == stacked.shape[0]
        # the loop's point is the KKT point of its own active set, with multipliers of the right sign
        z, lam, mult = la.active_set_solve(r["Gd"], r["Cd"], r["Ed"], r["g"], r["c"], lo[b], hi[b], r["at_lo"], r["at_hi"])
        assert np.abs(z - r["z"]).max() <= 1e-10 and np.abs(mult - la.FIXTURE_RHO[b] * r["y"]).max() <= 1e-9
        assert (mult[r["at_lo"]] < 0).all() and (mult[r["at_hi"]] > 0).all()


# fp64 roundoff through the dense inverse of these KKT matrices (admm_adjoint_ref's problems, condition number below 1e4) with the
# rows appended: the bound of tests/test_admm_adjoint_reference.py
LOOP_TOL = 1e-10
# the pinned counts: what the loops still move by at K_FWD, K_ADJ relative to their limit.  The slowest problem, (3,2,4) problem 1,
# contracts by 0.9765 per iteration (1e-3 per 290): 7.4e-08 / 3.1e-07 at 600.  Below the fp32 STEP_TOL of the device tests by 1e3.
PINNED_TOL = 1e-6


@pytest.mark.parametrize("nx,nu,N,B", la.FIXTURE_SHAPES)
def test_adjoint_loop_converges_to_the_dense_solve_and_the_counts_are_pinned(nx, nu, N, B):
    mx, mu, d, E, lo, hi, gz, glam = fixture_parts(nx, nu, N, B)
    fwd = la.forward(nx, nu, N, B, la.K_REF)
    for b, r in enumerate(la.reference(nx, nu, N, B)):
        rho = la.FIXTURE_RHO[b]
        lp = la.adjoint_loop(r["Gd"], r["Cd"], r["Ed"], gz[b], -glam[b], r["y"], rho, la.K_REF)
        az, alam, ya = lp["az"][-1], lp["alam"][-1], lp["ya"][-1]
        A = r["at_lo"] | r["at_hi"]
        assert not ya[~A].view(np.uint64).any()                 # from ya = 0 an inactive row's ya stays exactly 0
        assert np.abs(r["Ed"][A] @ r["az"]).max() <= 1e-12
        got = la.gradients(nx, nu, mx, mu, N, r["z"], r["lam"], rho * r["y"], az, alam, rho * ya, r["at_lo"], r["at_hi"])
        for k, a, ref in [("az", az, r["az"]), ("alam", alam, r["alam"]), ("nu", rho * ya, r["nu"])] + \
                [("d" + k, got[k], r["grads"][k]) for k in ("G", "C", "g", "c", "E", "lo", "hi")]:
            err = np.abs(a - ref).max() / np.abs(ref).max()
            print(f"({nx},{nu},{N}) problem {b} {k}: {err:.2e}")
            assert err <= LOOP_TOL, (b, k, err)
        assert all(np.abs(r["grads"][k]).max() > 0 for k in ("E", "lo", "hi"))
        # the pinned counts
        h = fwd[b]
        assert np.array_equal(h["y"][la.K_FWD - 1] < 0, r["at_lo"]) and np.array_equal(h["y"][la.K_FWD - 1] > 0, r["at_hi"])
        ef = max(np.abs(h[k][la.K_FWD - 1] - r[k]).max() / np.abs(r[k]).max() for k in ("z", "lam", "y"))
        ea = max(np.abs(lp[k][la.K_ADJ - 1] - ref).max() / np.abs(ref).max() for k, ref in (("az", r["az"]), ("alam", r["alam"])))
        ea = max(ea, np.abs(rho * lp["ya"][la.K_ADJ - 1] - r["nu"]).max() / np.abs(r["nu"]).max())
        print(f"({nx},{nu},{N}) problem {b}: forward at {la.K_FWD}: {ef:.2e}, adjoint at {la.K_ADJ}: {ea:.2e}")
        assert ef <= PINNED_TOL and ea <= PINNED_TOL


GROUPS = ("G", "C", "g", "c", "E", "lo", "hi")


def loss_along(nx, nu, mx, mu, N, d, E, lo, hi, gz, glam, b, r, direction, t):
    """l = gz' z + glam' lambda at the parameters moved by t along `direction`, through the dense solve on the reference's active set;
    G enters symmetrised, as the library reads it.  Returns (l, whether that set is still the optimal one)."""
    p = {k: d[k][b] + t * direction[k] for k in "GCgc"}
    lo_t, hi_t = lo[b].copy(), hi[b].copy()
    fin = np.isfinite(lo[b])
    lo_t[fin] += t * direction["lo"][fin]
    hi_t[fin] += t * direction["hi"][fin]
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, p["G"], p["C"], p["g"], p["c"])
    Gd = 0.5 * (Gd + Gd.T)
    Ed = lr.dense_E(nx, nu, mx, mu, N, E[b] + t * direction["E"])
    z, lam, mult = la.active_set_solve(Gd, Cd, Ed, g, c, lo_t, hi_t, r["at_lo"], r["at_hi"])
    A = r["at_lo"] | r["at_hi"]
    v = Ed @ z
    optimal = (mult[r["at_lo"]] < 0).all() and (mult[r["at_hi"]] > 0).all() and (v[~A] > lo_t[~A]).all() and (v[~A] < hi_t[~A]).all()
    return float(gz[b] @ z + glam[b] @ lam), bool(optimal)


@pytest.mark.parametrize("nx,nu,N,B", la.FIXTURE_SHAPES)
def test_central_differences_are_a_second_witness(nx, nu, N, B):
    """Directional central differences of l = gz' z + glam' lambda through the dense active-set fp64 solve at the steps h = 2^-10 and
    2^-11, against <gradient, direction>: along one direction that moves all seven parameter groups at once, and along one direction
    per group.  The active set must not change at any of the perturbed points.  The yardstick is the reference's own curve, as in
    tests/test_admm_adjoint_reference.py: l is a rational function of G, C and E, so the discrepancy is the h^2 term of the
    difference quotient and must fall by about 4 (asserted: between 3.5 and 4.5) when h halves; for a fixed active set (z, lambda)
    is linear in g, c, lo, hi, whose quotients are exact -- asserted as at least three orders below the joint direction's
    discrepancy at the smaller step.  g, c, lo and hi must be exact; G, C, E either.
    Observed (relative to |<gradient, direction>| of the joint direction; h = 2^-10 -> 2^-11): see the -s output; every joint
    ratio and the ratios of C and E print as 4.00."""
    mx, mu, d, E, lo, hi, gz, glam = fixture_parts(nx, nu, N, B)
    rng = np.random.default_rng(78)
    steps = (2.0 ** -10, 2.0 ** -11)
    for b, r in enumerate(la.reference(nx, nu, N, B)):
        full = {k: rng.standard_normal(r["grads"][k].shape) for k in GROUPS}
        zero = {k: np.zeros_like(v) for k, v in full.items()}
        fin = np.isfinite(lo[b])

        def discrepancy(direction):
            want = sum(float(r["grads"][k] @ direction[k]) for k in ("G", "C", "g", "c", "E")) + \
                sum(float(r["grads"][k][fin] @ direction[k][fin]) for k in ("lo", "hi"))
            out = []
            for h in steps:
                (lp, okp), (lm, okm) = (loss_along(nx, nu, mx, mu, N, d, E, lo, hi, gz, glam, b, r, direction, s * h) for s in (1, -1))
                assert okp and okm, "the active set changed"
                out.append(abs((lp - lm) / (2 * h) - want))
            return want, out

        want, joint = discrepancy(full)
        scale = abs(want)
        print(f"({nx},{nu},{N}) problem {b}: all groups {joint[0] / scale:.2e} -> {joint[1] / scale:.2e} (ratio {joint[0] / joint[1]:.2f})")
        assert 3.5 <= joint[0] / joint[1] <= 4.5
        for k in GROUPS:
            _, e = discrepancy({**zero, k: full[k]})
            exact = max(e) <= 1e-3 * joint[1]
            print(f"    {k}: {e[0] / scale:.2e} -> {e[1] / scale:.2e}" + (" (exact)" if exact else f" (ratio {e[0] / e[1]:.2f})"))
            assert exact or 3.5 <= e[0] / e[1] <= 4.5, k
            assert exact or k in "GCE", k
