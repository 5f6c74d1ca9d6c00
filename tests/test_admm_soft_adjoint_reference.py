"""CPU-only: the reference of the soft QPs' backward pass (tests/admm_soft_adjoint_ref.py) against what it has to equal.

 1. mask_ref, grad_bounds_ref and lin_grad_ref element by element from their lines, on inputs with the tie |yf| = theta on both
    signs, +-0, NaN, kappa = 0 and kappa = +Inf; with kappa = +Inf everywhere the bits of the hard references; with E = I the rows
    reference gives the box one.
 2. The pinned fixtures (box and rows at nx, nu, N, batch = 5, 2, 3, 4; rows 3 + 2): after the fp64 loop EVERY problem has a free, a
    held and a saturated row, held and saturated rows on both the lo and the hi side, kappa finite, +Inf and 0; held rows have
    |rho y| <= 0.9 kappa and |y| >= MARGIN, saturated rows lie beyond their bound by at least MARGIN, free rows inside by as much;
    a numpy fp32 run of the same lines lands in the same sets.
 3. The mask followed by the HARD adjoint reference loop converges to the dense solve of the reduced KKT system with the held rows
    E_A appended to C, and the counts K_FWD, K_ADJ the device tests replay are counts at which both loops have converged.
 4. Central differences of the dense solve on the fixed sets are a second witness for all eight gradients, kappa included.
"""
import numpy as np
import pytest

import admm_adjoint_ref as ar
import admm_lin_adjoint_ref as la
import admm_lin_ref as lr
import admm_soft_adjoint_ref as sa
import admm_soft_ref as sr
from oracle import schur_oracle as so
from test_admm_lin_adjoint_reference import same_bits

F32, F64 = np.float32, np.float64
SPECIAL_SHAPE = (3, 2, 2, 1, 4, 3)      # nx, nu, mx, mu, N, B


def special_data(dtype, shape=SPECIAL_SHAPE, seed=17):
    """Order-1 data over the rows of `shape`.  yf is 0 on about a third of the rows; elsewhere about half sit exactly on +-theta
    (saturated), the others strictly inside it (held).  Planted: the tie on both signs, +-0 under a finite kappa, a NaN yf, kappa = 0
    under yf = +-0, kappa = +Inf next to finite kappa, a NaN in az."""
    nx, nu, mx, mu, N, B = shape
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(seed)
    z, az = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(2))
    ya = rng.standard_normal((B, nw)).astype(dtype)
    E = rng.standard_normal((B, ne)).astype(dtype)
    rho = np.array([0.75, 3.0, 2.25], dtype)[:B]
    kappa = rng.uniform(0.5, 2.0, (B, nw)).astype(dtype)
    kappa[rng.random((B, nw)) < 0.2] = np.inf
    theta = sa.theta_of(kappa, rho)
    u = rng.random((B, nw))
    sign = np.where(rng.random((B, nw)) < 0.5, -1.0, 1.0).astype(dtype)
    with np.errstate(invalid="ignore"):
        inside = (sign * np.where(np.isinf(theta), dtype(1.0), theta) * rng.uniform(0.1, 0.9, (B, nw)).astype(dtype)).astype(dtype)
        yf = np.where(u < 0.33, dtype(0.0), np.where((u < 0.66) & np.isfinite(theta), sign * theta, inside)).astype(dtype)
    kappa[0, 0] = kappa[0, 1] = 1.25
    tie = dtype(1.25) / rho[0]                                        # (5/3: not exact, the rounded quotient itself)
    yf[0, 0], yf[0, 1] = tie, -tie                                    # the tie, + and -
    yf[0, 2], yf[0, 3] = 0.0, -0.0                                    # free under whatever kappa stands there ...
    kappa[0, 2], kappa[0, 3] = 1.5, np.inf
    yf[1, 0], kappa[1, 0] = 0.0, 0.0                                  # kappa = 0: theta = 0, saturated with yf = +0 ...
    yf[1, 1], kappa[1, 1] = -0.0, 0.0                                 # ... and with yf = -0
    yf[1, 2] = np.nan                                                 # held, whatever kappa
    kappa[1, 3], kappa[1, 4] = np.inf, 0.25                           # +Inf next to a finite kappa
    yf[1, 3], yf[1, 4] = 0.5, np.nextafter(dtype(0.25) / rho[1], dtype(0))       # held under +Inf; one ulp inside theta: held
    az[2, 1] = np.nan
    return dict(z=z, az=az, ya=ya, E=E, yf=yf, kappa=kappa, rho=rho)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_mask_and_gradient_lines(dtype):
    nx, nu, mx, mu, N, B = SPECIAL_SHAPE
    d = special_data(dtype)
    yf, kappa, rho, ya, az, z, E = (d[k] for k in ("yf", "kappa", "rho", "ya", "az", "z", "E"))
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    ym = sa.mask_ref(dtype, yf, kappa, rho)
    glo, ghi, gk, gE = sa.lin_grad_ref(dtype, nx, nu, mx, mu, N, z, az, E, yf, ya, kappa, rho)
    assert all(a.dtype == np.dtype(dtype) for a in (ym, glo, ghi, gk, gE))
    Ed = [lr.dense_E(nx, nu, mx, mu, N, E[b]) for b in range(B)]
    cols = [[np.flatnonzero(Ed[b][r] != 0) for r in range(nw)] for b in range(B)]
    seen = {"sat+": 0, "sat-": 0, "held": 0, "free": 0}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            for r in range(nw):
                f, k = yf[b, r], kappa[b, r]
                theta = k / rho[b]
                assert isinstance(theta, dtype)
                sat = bool(np.abs(f) >= theta)
                assert same_bits(ym[b, r], dtype(0.0) if sat else f), (b, r)
                n = -(rho[b] * ya[b, r])
                assert same_bits(glo[b, r], n if (f < 0 and not sat) else dtype(0.0)), (b, r)
                assert same_bits(ghi[b, r], n if (f > 0 and not sat) else dtype(0.0)), (b, r)
                if sat:
                    v = dtype(0.0)
                    for j in cols[b][r]:           # ascending j over the row's block (random E: no zero entries)
                        v = lr.fma_ref(Ed[b][r, j], az[b, j], v, dtype)
                    assert same_bits(gk[b, r], v if f > 0 else -v), (b, r)
                else:
                    assert same_bits(gk[b, r], dtype(0.0)), (b, r)
                seen["sat+" if sat and f > 0 else "sat-" if sat else "held" if f != 0 else "free"] += 1
    assert min(seen.values()) >= 3, seen
    # the planted cases
    assert not ym[0, :2].view(np.uint8).any() and gk[0, 0] != 0 and gk[0, 1] != 0              # the ties are saturated, both signs
    assert same_bits(ym[0, 2:4], yf[0, 2:4]) and np.signbit(ym[0, 3]) and not gk[0, 2:4].any()    # +-0 under kappa > 0: free, bits kept
    assert not ym[1, :2].view(np.uint8).any()                                                    # kappa = 0: +0, also from -0
    assert np.isnan(ym[1, 2]) and gk[1, 2] == 0 and glo[1, 2] == 0 and ghi[1, 2] == 0           # a NaN yf passes: held, no side
    assert same_bits(ym[1, 3:5], yf[1, 3:5]) and ghi[1, 3] != 0 and ghi[1, 4] != 0               # +Inf, and one ulp inside theta
    # gE: the lines of the hard launch on the UNMASKED yf; glo, ghi: the hard lines on ym
    _, _, gE_hard = la.grad_ref(dtype, nx, nu, mx, mu, N, z, az, yf, ya, rho)
    assert same_bits(gE, gE_hard)
    blo, bhi = ar.grad_bounds_ref(dtype, ym, rho, ya)
    assert same_bits(glo, blo) and same_bits(ghi, bhi)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_infinite_kappa_gives_the_hard_bits_and_a_zero_kappa_frees_everything(dtype):
    nx, nu, mx, mu, N, B = SPECIAL_SHAPE
    d = special_data(dtype)
    inf, zero = np.full_like(d["kappa"], np.inf), np.zeros_like(d["kappa"])
    assert same_bits(sa.mask_ref(dtype, d["yf"], inf, d["rho"]), d["yf"])
    glo, ghi, gk, gE = sa.lin_grad_ref(dtype, nx, nu, mx, mu, N, d["z"], d["az"], d["E"], d["yf"], d["ya"], inf, d["rho"])
    hlo, hhi, hE = la.grad_ref(dtype, nx, nu, mx, mu, N, d["z"], d["az"], d["yf"], d["ya"], d["rho"])
    assert same_bits(glo, hlo) and same_bits(ghi, hhi) and same_bits(gE, hE) and not gk.view(np.uint8).any()
    ym = sa.mask_ref(dtype, d["yf"], zero, d["rho"])
    nan = np.isnan(d["yf"])
    assert nan.sum() == 1 and not ym[~nan].view(np.uint8).any() and np.isnan(ym[nan]).all()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_identity_rows_give_the_box_lines(dtype):
    nx, nu, N, B = 3, 2, 3, 2
    nz = (nx + nu) * N - nu
    rng = np.random.default_rng(5)
    z, az, ya = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(3))
    rho = np.array([0.75, 2.0], dtype)
    kappa = rng.uniform(0.5, 2.0, (B, nz)).astype(dtype)
    theta = sa.theta_of(kappa, rho)
    u = rng.random((B, nz))
    yf = np.where(u < 0.3, 0.0, np.where(u < 0.65, theta, -0.5 * theta)).astype(dtype)
    E = np.tile(lr.identity_E(nx, nu, N, dtype), (B, 1))
    glo, ghi, gk, _ = sa.lin_grad_ref(dtype, nx, nu, nx, nu, N, z, az, E, yf, ya, kappa, rho)
    blo, bhi, bk = sa.grad_bounds_ref(dtype, yf, kappa, rho, ya, az)
    assert same_bits(glo, blo) and same_bits(ghi, bhi) and same_bits(gk, bk) and gk.any()


# ---- 2. the fixtures
@pytest.mark.parametrize("kind", sa.KINDS)
def test_fixture_has_every_set_in_every_problem_with_margins(kind):
    nx, nu, mx, mu, N, B = sa.dims(kind)
    assert (nx, nu, N, B) == (5, 2, 3, 4) and (kind == "box" or (mx, mu) == (3, 2))
    d, E, lo, hi, kappa, gz, glam = sa.fixture(kind)
    for a in list(d.values()) + [lo, hi, kappa, gz, glam] + ([] if E is None else [E]):
        fin = np.isfinite(a)
        assert np.array_equal(a[fin].astype(F32).astype(F64), a[fin])       # fp32 numbers: both precisions get the same problem
    y32 = sa.forward_f32(kind)
    for b, r in enumerate(sa.reference(kind)):
        rho = sa.FIXTURE_RHO[kind][b]
        free, hl, hh, sl, sh = r["sets"]
        held, sat = hl | hh, sl | sh
        assert free.any() and hl.any() and hh.any() and sl.any() and sh.any(), b             # no problem is left out
        assert (free.astype(int) + held + sat == 1).all()
        k = kappa[b]
        assert (k == 0).any() and np.isinf(k).any() and ((k > 0) & np.isfinite(k)).any(), b
        assert (k[sat & (r["y"] != 0)] > 0).all() and np.isfinite(k[sat]).all() and np.isinf(k[held]).any() and np.isfinite(k[held]).any()
        v = sa._E(r["Ed"], r["z"].size) @ sa.forward(kind)[b]["z"][-1]
        fin = held & np.isfinite(k)
        ratio, hmin = (np.abs(rho * r["y"][fin]) / k[fin]).max(), np.abs(r["y"][held]).min()
        beyond = min((lo[b] - v)[sl].min(), (v - hi[b])[sh].min())
        inside = np.minimum(v - lo[b], hi[b] - v)[free].min()
        print(f"{kind} problem {b}: {int(free.sum())} free, {int(hl.sum())}+{int(hh.sum())} held, {int(sl.sum())}+{int(sh.sum())} saturated; "
              f"held |rho y| / kappa <= {ratio:.3f}, held |y| >= {hmin:.3e}, saturated beyond by {beyond:.3e}, free inside by {inside:.3e}")
        assert ratio <= sa.HELD_MAX and hmin >= sa.MARGIN and beyond >= sa.MARGIN and inside >= sa.MARGIN
        # a saturated y sits ON +-theta, to the bit, in both precisions
        theta = sa.theta_of(k, np.float64(rho))
        assert np.array_equal(np.abs(r["y"][sat]), theta[sat])
        stacked = np.vstack([r["Cd"], sa._E(r["Ed"], r["z"].size)[held]])
        assert np.linalg.matrix_rank(stacked) == stacked.shape[0]
        # the loop's point is the KKT point of its own sets
        z, lam, mult = sa.active_set_solve(r["Gd"], r["Cd"], r["Ed"], r["g"], r["c"], lo[b], hi[b], k, r["sets"])
        assert np.abs(z - sa.forward(kind)[b]["z"][-1]).max() <= 1e-10 and np.abs(mult - rho * r["y"]).max() <= 1e-9
        assert sa.sets_optimal(r["Ed"], z, mult, lo[b], hi[b], k, r["sets"])
        # the fp32 loop lands in the same sets
        s32 = sa.sets(y32[b], k.astype(F32), F32(rho))
        assert all(np.array_equal(a, c) for a, c in zip(r["sets"], s32)), b
        assert np.array_equal(np.abs(y32[b][sat]), sa.theta_of(k.astype(F32), F32(rho))[sat])


# fp64 roundoff through the dense inverse of these KKT matrices: the bound of tests/test_admm_lin_adjoint_reference.py
LOOP_TOL = 1e-10
# what the loops still move by at K_FWD, K_ADJ relative to their limit; the bound of tests/test_admm_lin_adjoint_reference.py
PINNED_TOL = 1e-6
GROUPS = {"box": ("G", "C", "g", "c", "lo", "hi", "kappa"), "rows": ("G", "C", "g", "c", "E", "lo", "hi", "kappa")}


@pytest.mark.parametrize("kind", sa.KINDS)
def test_mask_plus_hard_adjoint_loop_converges_to_the_dense_solve_and_the_counts_are_pinned(kind):
    nx, nu, mx, mu, N, B = sa.dims(kind)
    _, _, lo, hi, kappa, gz, glam = sa.fixture(kind)
    fwd = sa.forward(kind)
    for b, r in enumerate(sa.reference(kind)):
        rho = sa.FIXTURE_RHO[kind][b]
        free, hl, hh, sl, sh = r["sets"]
        held = hl | hh
        ym = sa.mask_ref(F64, r["y"], kappa[b], rho)
        assert np.array_equal(ym != 0, held) and not ym[~held].view(np.uint64).any() and np.array_equal(ym[held], r["y"][held])
        lp = sa.adjoint_loop(r["Gd"], r["Cd"], r["Ed"], gz[b], -glam[b], ym, rho, sa.K_REF)
        az = lp["wa" if kind == "box" else "az"][-1]
        alam, ya = lp["alam"][-1], lp["ya"][-1]
        assert not ya[~held].view(np.uint64).any()                 # a saturated row's ya stays exactly 0, like a free row's
        assert np.abs((sa._E(r["Ed"], az.size) @ r["az"])[held]).max() <= 1e-12
        got = sa.gradients(nx, nu, mx, mu, N, r["Ed"], r["z"], r["lam"], rho * r["y"], az, alam, rho * ya, r["sets"])
        for k, a, ref in [("az", az, r["az"]), ("alam", alam, r["alam"]), ("nu", rho * ya, r["nu"])] + \
                [("d" + k, got[k], r["grads"][k]) for k in GROUPS[kind]]:
            err = np.abs(a - ref).max() / np.abs(ref).max()
            print(f"{kind} problem {b} {k}: {err:.2e}")
            assert err <= LOOP_TOL, (b, k, err)
        assert all(np.abs(r["grads"][k]).max() > 0 for k in GROUPS[kind])
        gk = r["grads"]["kappa"]
        assert gk[sl | sh].all() and not gk[~(sl | sh)].any() and not gk[np.isinf(kappa[b])].any()
        # the pinned counts
        h = fwd[b]
        assert all(np.array_equal(a, c) for a, c in zip(sa.sets(h["y"][sa.K_FWD - 1], kappa[b], rho), r["sets"]))
        ef = max(np.abs(h[k][sa.K_FWD - 1] - h[k][-1]).max() / np.abs(h[k][-1]).max() for k in ("z", "w", "lam", "y"))
        ea = max(np.abs(lp[k][sa.K_ADJ - 1] - ref).max() / np.abs(ref).max() for k, ref in (("az", r["az"]), ("alam", r["alam"])))
        ea = max(ea, np.abs(rho * lp["ya"][sa.K_ADJ - 1] - r["nu"]).max() / np.abs(r["nu"]).max())
        print(f"{kind} problem {b}: forward at {sa.K_FWD}: {ef:.2e}, adjoint at {sa.K_ADJ}: {ea:.2e}")
        assert ef <= PINNED_TOL and ea <= PINNED_TOL


def loss_along(kind, b, r, direction, t):
    """l = gz' z + glam' lambda at the parameters moved by t along `direction`, through the dense solve on the reference's sets; G
    enters symmetrised, as the library reads it.  Returns (l, whether those sets are still the optimal ones)."""
    nx, nu, mx, mu, N, B = sa.dims(kind)
    d, E, lo, hi, kappa, gz, glam = sa.fixture(kind)
    p = {k: d[k][b] + t * direction[k] for k in "GCgc"}
    lo_t, hi_t, k_t = lo[b].copy(), hi[b].copy(), kappa[b].copy()
    fl, fh, fk = np.isfinite(lo[b]), np.isfinite(hi[b]), np.isfinite(kappa[b]) & (kappa[b] > 0)
    lo_t[fl] += t * direction["lo"][fl]
    hi_t[fh] += t * direction["hi"][fh]
    k_t[fk] += t * direction["kappa"][fk]
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, p["G"], p["C"], p["g"], p["c"])
    Gd = 0.5 * (Gd + Gd.T)
    Ed = None if E is None else lr.dense_E(nx, nu, mx, mu, N, E[b] + t * direction["E"])
    z, lam, mult = sa.active_set_solve(Gd, Cd, Ed, g, c, lo_t, hi_t, k_t, r["sets"])
    return float(gz[b] @ z + glam[b] @ lam), sa.sets_optimal(Ed, z, mult, lo_t, hi_t, k_t, r["sets"])


@pytest.mark.parametrize("kind", sa.KINDS)
def test_central_differences_are_a_second_witness(kind):
    """Directional central differences of l = gz' z + glam' lambda through the dense fixed-set fp64 solve at the steps h = 2^-10 and
    2^-11 (those of tests/test_admm_lin_adjoint_reference.py), against <gradient, direction>: along one direction that moves all
    eight parameter groups at once (seven for the box, which has no E), and along one direction per group.  The sets must not
    change at any of the perturbed points.  The discrepancy is the h^2 term of the difference quotient and must fall by about 4
    (asserted: between 3.5 and 4.5, the bound of the two existing adjoint reference tests) when h halves; for fixed sets (z, lambda)
    is linear in g, c, lo, hi and kappa, whose quotients are exact -- asserted as at least three orders below the joint direction's
    discrepancy at the smaller step.  lo, hi move where they are finite, kappa where it is finite and positive (at kappa = 0 only a
    one-sided derivative exists; at +Inf none).  Run with -s for the figures; every joint ratio prints as 4.00."""
    _, _, lo, hi, kappa, _, _ = sa.fixture(kind)
    groups = GROUPS[kind]
    rng = np.random.default_rng(79)
    steps = (2.0 ** -10, 2.0 ** -11)
    for b, r in enumerate(sa.reference(kind)):
        full = {k: rng.standard_normal(r["grads"][k].shape) for k in groups}
        if "E" not in full:
            full["E"] = None
        zero = {k: (None if v is None else np.zeros_like(v)) for k, v in full.items()}
        moves = {"lo": np.isfinite(lo[b]), "hi": np.isfinite(hi[b]), "kappa": np.isfinite(kappa[b]) & (kappa[b] > 0)}
        assert (moves["kappa"] & (r["sets"][3] | r["sets"][4])).sum() >= 2

        def discrepancy(direction):
            want = sum(float(r["grads"][k] @ direction[k]) for k in groups if k not in moves) + \
                sum(float(r["grads"][k][m] @ direction[k][m]) for k, m in moves.items())
            out = []
            for h in steps:
                (lp, okp), (lm, okm) = (loss_along(kind, b, r, direction, s * h) for s in (1, -1))
                assert okp and okm, "the sets changed"
                out.append(abs((lp - lm) / (2 * h) - want))
            return want, out

        want, joint = discrepancy(full)
        scale = abs(want)
        print(f"{kind} problem {b}: all groups {joint[0] / scale:.2e} -> {joint[1] / scale:.2e} (ratio {joint[0] / joint[1]:.2f})")
        assert 3.5 <= joint[0] / joint[1] <= 4.5
        for k in groups:
            _, e = discrepancy({**zero, k: full[k]})
            exact = max(e) <= 1e-3 * joint[1]
            print(f"    {k}: {e[0] / scale:.2e} -> {e[1] / scale:.2e}" + (" (exact)" if exact else f" (ratio {e[0] / e[1]:.2f})"))
            assert exact or 3.5 <= e[0] / e[1] <= 4.5, k
            assert exact or k in "GCE", k
