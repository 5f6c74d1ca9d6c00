"""References for the backward pass of the soft (L1-penalised) box and rows QPs (gbdpcg_admm_soft_mask_*, gbdpcg_admm_lin_soft_mask_*,
gbdpcg_admm_soft_grad_bounds_*, gbdpcg_admm_lin_soft_grad_*, gbd_pcg_amd.autograd.soft_box_qp_solve / soft_lin_qp_solve; not a test
module).

Forward (tests/admm_soft_ref.py): min 1/2 z'Gz + g'z + sum_r kappa_r dist((E z)_r, [lo_r, hi_r]) subject to Cz = c (the box: E = I),
with G z + g + C' lambda + rho E'y = 0 at the solution.  With theta_r = kappa_r / rho (the division of the update) the forward y
splits the rows, to the bit:
    free        y_r == 0                        inside its bounds
    held        y_r != 0, |y_r| < theta_r       on a bound, the multiplier mu_r = rho y_r moves with z
    saturated   |y_r| >= theta_r                beyond its bound, mu_r = +-kappa_r is a constant         (kappa_r = 0: y_r = 0, saturated)
A saturated row is free in the adjoint problem: with A the HELD rows the adjoint triple solves
    G a_z + gz + C' a_lambda + E_A' nu = 0,   C a_z = -glam,   (E a_z)_A = 0
which is the hard adjoint loop (admm_adjoint_ref / admm_lin_adjoint_ref) on the masked y, and
    dl/dg = a_z   dl/dc = -a_lambda   dl/dlo_r = -nu_r (held at lo)   dl/dhi_r = -nu_r (held at hi)
    dl/dkappa_r = sign(y_r) (E a_z)_r on saturated rows, 0 elsewhere                (sign(0) = -1: the line of the device)
    dl/dE(r, j) = mu_r a_z,j + nu_r z_j on held rows, mu_r a_z,j on saturated ones, 0 on free ones       dl/dG, dl/dC: kkt_grad_ref
The device's line for dl/dkappa reads a row with kappa_r = 0 (y_r = +-0) as saturated AT LO, which is the one-sided derivative of a
row that lies below lo; the fixture puts its kappa = 0 rows there.

saturated, mask_ref          the comparison and the masked copy ym, bit for bit
grad_bounds_ref, lin_grad_ref   the gradient launches as the device defines them, bit for bit
sets                         (free, held_lo, held_hi, sat_lo, sat_hi) of a forward y
dense_adjoint, active_set_solve, gradients   the dense reduced systems and every gradient they imply, box (E None) or rows
fixture, forward, reference, loop_reference, forward_f32   the pinned problems, their loops and the dense answers
"""
import functools

import numpy as np

import admm_adjoint_ref as ar
import admm_lin_adjoint_ref as la
import admm_lin_ref as lr
import admm_soft_ref as sr
import kkt_grad_ref
from admm_adjoint_ref import converged_bound  # noqa: F401
from oracle import schur_oracle as so


def theta_of(kappa, rho):
    """kappa / rho, one division per element in kappa's dtype; rho [B] against kappa [B, n]."""
    kappa = np.asarray(kappa)
    rho = np.asarray(rho, kappa.dtype)
    if rho.ndim == 1 and kappa.ndim == 2:
        rho = rho.reshape(-1, 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (kappa / rho).astype(kappa.dtype)


def saturated(dtype, yf, kappa, rho):
    """|yf| >= kappa / rho; a NaN yf (or a NaN theta) fails."""
    yf, kappa = np.asarray(yf, dtype), np.asarray(kappa, dtype)
    with np.errstate(invalid="ignore"):
        return np.abs(yf) >= theta_of(kappa, np.asarray(rho, dtype))


def mask_ref(dtype, yf, kappa, rho):
    """ym = sat ? +0 : yf -- the bits of yf where it passes (a NaN, -0 included)."""
    yf = np.asarray(yf, dtype)
    return np.where(saturated(dtype, yf, kappa, rho), dtype(0.0), yf).astype(dtype)


def grad_bounds_ref(dtype, yf, kappa, rho, ya, az):
    """(glo, ghi, gkappa) of the soft box: one multiplication and one negation, or one negation, per element in `dtype`."""
    yf, ya, az = (np.asarray(a, dtype) for a in (yf, ya, az))
    sat = saturated(dtype, yf, kappa, rho)
    r = np.asarray(rho, dtype).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        n = -(r * ya)
        zero = dtype(0.0)
        glo = np.where((yf < 0) & ~sat, n, zero).astype(dtype)
        ghi = np.where((yf > 0) & ~sat, n, zero).astype(dtype)
        gk = np.where(sat, np.where(yf > 0, az, -az), zero).astype(dtype)
    return glo, ghi, gk


def lin_grad_ref(dtype, nx, nu, mx, mu, N, z, az, E, yf, ya, kappa, rho):
    """(glo, ghi, gkappa [B, nw], gE [B, ne]) of the soft rows in `dtype`: glo, ghi the lines of grad_bounds_ref over the rows, gE the
    lines of admm_lin_adjoint_ref.grad_ref on the unmasked yf, gkappa_r = sat ? (yf_r > 0 ? v : -v) : +0 with v the chain of
    fma(E(r, j), az_j, acc) over the block's columns in ascending j from +0."""
    dtype = np.dtype(dtype)
    z, az, E, yf, ya, kappa, rho = (np.asarray(a, dtype) for a in (z, az, E, yf, ya, kappa, rho))
    B = z.shape[0]
    glo, ghi, _ = grad_bounds_ref(dtype.type, yf, kappa, rho, ya, np.zeros_like(yf))
    _, _, gE = la.grad_ref(dtype, nx, nu, mx, mu, N, z, az, yf, ya, rho)
    sat = saturated(dtype.type, yf, kappa, rho)
    gk = np.zeros_like(yf)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for m, n, eo, ro, co, _ in lr.blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for r in range(m):
                    if sat[b, ro + r]:
                        v = lr.chain(Eb[:, r], az[b, co:co + n], dtype)
                        gk[b, ro + r] = v if yf[b, ro + r] > 0 else -v
    return glo, ghi, gk, gE


def sets(y, kappa, rho):
    """(free, held_lo, held_hi, sat_lo, sat_hi) of one problem's forward y in fp64 (or in y's dtype); a saturated row with y = 0
    (kappa = 0) is at lo, as the device's line reads it."""
    y = np.asarray(y)
    sat = saturated(y.dtype.type, y, kappa, rho)
    return ~sat & (y == 0), ~sat & (y < 0), ~sat & (y > 0), sat & ~(y > 0), sat & (y > 0)


# ---- the dense systems.  Ed None: the box, E = I
def _E(Ed, nz):
    return np.eye(nz) if Ed is None else np.asarray(Ed, np.float64)


def dense_adjoint(Gd, Cd, Ed, gz, glam, held):
    """(a_z, a_lambda, nu): admm_lin_adjoint_ref.dense_adjoint with the HELD rows as the active ones."""
    return la.dense_adjoint(Gd, Cd, _E(Ed, Gd.shape[0]), gz, glam, held)


def active_set_solve(Gd, Cd, Ed, g, c, lo, hi, kappa, s):
    """(z, lambda, mu) for GIVEN sets s = (free, held_lo, held_hi, sat_lo, sat_hi): (E z)_r on its bound on the held rows, the
    constant multipliers -kappa / +kappa on the saturated ones in the stationarity.  mu is the full multiplier vector."""
    E = _E(Ed, Gd.shape[0])
    _, hl, hh, sl, sh = s
    const = np.where(sh, kappa, 0.0) - np.where(sl, kappa, 0.0)
    z, lam, mu = la.active_set_solve(Gd, Cd, E, g + E.T @ const, c, lo, hi, hl, hh)
    return z, lam, mu + const


def sets_optimal(Ed, z, mu, lo, hi, kappa, s):
    """Are the given sets those of the solution?  Held multipliers of the right sign and below kappa, saturated rows beyond their
    bound, free rows strictly inside."""
    free, hl, hh, sl, sh = s
    v = _E(Ed, z.size) @ z
    return bool((mu[hl] < 0).all() and (mu[hh] > 0).all() and (np.abs(mu[hl | hh]) < kappa[hl | hh]).all() and
                (v[sl] < lo[sl]).all() and (v[sh] > hi[sh]).all() and (v[free] > lo[free]).all() and (v[free] < hi[free]).all())


def gradients(nx, nu, mx, mu, N, Ed, z, lam, mu_rows, az, alam, nu_rows, s):
    """Every gradient the adjoint triple implies, packed as the device packs them (no "E" for the box).  mu_rows = rho y (all rows),
    nu_rows = rho ya (0 off the held rows)."""
    free, hl, hh, sl, sh = s
    gG, gC = kkt_grad_ref.block_grads(nx, nu, N, z, lam, az, alam)
    v = _E(Ed, z.size) @ az
    out = {"G": gG, "C": gC, "g": az.copy(), "c": -alam, "lo": np.where(hl, -nu_rows, 0.0), "hi": np.where(hh, -nu_rows, 0.0),
           "kappa": np.where(sh, v, 0.0) - np.where(sl, v, 0.0)}
    if Ed is not None:
        dE = np.where((~free)[:, None], np.outer(mu_rows, az), 0.0) + np.where((hl | hh)[:, None], np.outer(nu_rows, z), 0.0)
        out["E"] = la.pack_E(nx, nu, mx, mu, N, dE)
    return out


# ---- the pinned fixtures: fp64 arrays holding fp32 numbers.  One box and one rows fixture at nx, nu, N, batch = FIXTURE_SHAPE.
FIXTURE_SHAPE = (5, 2, 3, 4)
FIXTURE_ROWS = (3, 2)                   # mx, mu of the rows fixture
FIXTURE_RHO = {"box": (8.0, 16.0, 64.0, 4.0), "rows": (16.0, 16.0, 8.0, 4.0)}     # per problem, where its two loops contract fastest (powers of two)
FIXTURE_SEED = 523
HELD_FRACTION = 0.5                     # |mu| of a held row over its kappa by construction (the tests ask for <= HELD_MAX)
HELD_MAX = 0.9
GAP = 0.25                              # how far a saturated row lies beyond its bound by construction (the tests ask for >= MARGIN)
MARGIN = ar.MARGIN
MULT = 8.0                              # the scale of the multipliers: what keeps the sets through the central differences' steps
KINDS = ("box", "rows")


def _roles(kind, rng):
    """Per row of one problem a role: 'hl', 'hh' held (finite kappa), 'Hl' held at lo with kappa = +Inf, 'sl', 'sh' saturated,
    'z' kappa = 0 below lo, 'f' free with a finite kappa, 'F' free with kappa = +Inf, 'n' no bounds at all.  A row that only sees
    x_0 (which c pins) cannot be held: [C; E_A] would lose rank.  Three held rows per problem: the dynamics leave nu (N - 1) = 4
    free directions."""
    nx, nu, N, _ = FIXTURE_SHAPE
    mx, mu = (nx, nu) if kind == "box" else FIXTURE_ROWS
    nw = (mx + mu) * N - mu
    knot, in_block = np.arange(nw) // (mx + mu), np.arange(nw) % (mx + mu)
    movable = np.flatnonzero((knot > 0) | (in_block >= mx))
    pinned = np.flatnonzero((knot == 0) & (in_block < mx))
    roles = np.full(nw, "n", dtype=object)
    mv = rng.permutation(movable)
    for r, role in zip(mv, ("hl", "hh", "Hl", "sl", "sh", "z", "f", "F", "sl", "sh", "f")):
        roles[r] = role
    pv = rng.permutation(pinned)
    for r, role in zip(pv, ("sh", "z", "f")):
        roles[r] = role
    return roles


@functools.lru_cache(maxsize=None)
def fixture(kind):
    """(d, E [B, ne] or None, lo [B, nw], hi, kappa, gz [B, nz], glam [B, nx N]).  Built backwards from a solution: per problem the
    roles of _roles, multipliers of order 1 on the held and saturated rows, the equality-constrained solve with g + E'mu in the
    place of g, and then the bounds ON that point (held), GAP inside it (saturated, kappa = |mu|; kappa = 0) or around it (free);
    kappa of a held row is |mu| / HELD_FRACTION.  Everything is rounded to fp32, which moves the solution a little: the tests
    assert the sets and margins of the converged loop, not of the construction.  Read-only."""
    nx, nu, N, B = FIXTURE_SHAPE
    mx, mu = (nx, nu) if kind == "box" else FIXTURE_ROWS
    d = {k: v.astype(np.float32).astype(np.float64) for k, v in so.gen(nx, nu, N, seed=FIXTURE_SEED, batch=B, dtype=np.float64).items()}
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(FIXTURE_SEED + (1 if kind == "box" else 2))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    E = None if kind == "box" else f32(rng.standard_normal((B, ne)))
    lo, hi, kappa = np.full((B, nw), -np.inf), np.full((B, nw), np.inf), np.full((B, nw), np.inf)
    for b in range(B):
        roles = _roles(kind, rng)
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = np.eye(nz) if E is None else lr.dense_E(nx, nu, mx, mu, N, E[b])
        mult = np.zeros(nw)
        for r, role in enumerate(roles):
            if role in ("hl", "Hl", "sl"):
                mult[r] = -MULT * rng.uniform(0.5, 1.5)
            elif role in ("hh", "sh"):
                mult[r] = MULT * rng.uniform(0.5, 1.5)
        mult = f32(mult)
        K = np.zeros((nz + Cd.shape[0],) * 2)
        K[:nz, :nz], K[:nz, nz:], K[nz:, :nz] = Gd, Cd.T, Cd
        v = Ed @ np.linalg.solve(K, np.concatenate([-(g + Ed.T @ mult), c]))[:nz]
        for r, role in enumerate(roles):
            if role in ("hl", "Hl"):
                lo[b, r], kappa[b, r] = v[r], np.inf if role == "Hl" else abs(mult[r]) / HELD_FRACTION
            elif role == "hh":
                hi[b, r], kappa[b, r] = v[r], abs(mult[r]) / HELD_FRACTION
            elif role in ("sl", "z"):
                lo[b, r], kappa[b, r] = v[r] + GAP, abs(mult[r])
            elif role == "sh":
                hi[b, r], kappa[b, r] = v[r] - GAP, abs(mult[r])
            elif role in ("f", "F"):
                lo[b, r], hi[b, r], kappa[b, r] = v[r] - GAP, v[r] + GAP, np.inf if role == "F" else MULT
    lo, hi, kappa = f32(lo), f32(hi), f32(kappa)
    gz, glam = f32(rng.standard_normal((B, nz))), f32(rng.standard_normal((B, nx * N)))
    for a in list(d.values()) + [lo, hi, kappa, gz, glam] + ([] if E is None else [E]):
        a.setflags(write=False)
    return d, E, lo, hi, kappa, gz, glam


def dims(kind):
    nx, nu, N, B = FIXTURE_SHAPE
    mx, mu = (nx, nu) if kind == "box" else FIXTURE_ROWS
    return nx, nu, mx, mu, N, B


def dense_problem(kind, b):
    nx, nu, mx, mu, N, _ = dims(kind)
    d, E = fixture(kind)[:2]
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
    return Gd, Cd, (None if E is None else lr.dense_E(nx, nu, mx, mu, N, E[b])), g, c


K_REF = 4000                 # the forward loop of reference()
K_FWD, K_ADJ = 600, 600      # the counts the device tests replay (pinned by tests/test_admm_soft_adjoint_reference.py)


@functools.lru_cache(maxsize=None)
def forward(kind, K=K_REF):
    """admm_soft_ref's fp64 iteration on the fixture from w0 = y0 = 0, one history per problem."""
    _, _, lo, hi, kappa, _, _ = fixture(kind)
    out = []
    for b in range(FIXTURE_SHAPE[3]):
        Gd, Cd, Ed, g, c = dense_problem(kind, b)
        zero = np.zeros(lo.shape[1])
        run = sr.admm_soft(Gd, Cd, g, c, lo[b], hi[b], kappa[b], FIXTURE_RHO[kind][b], K, zero, zero) if Ed is None else \
            sr.admm_lin_soft(Gd, Cd, Ed, g, c, lo[b], hi[b], kappa[b], FIXTURE_RHO[kind][b], K, zero, zero)
        out.append(run)
    return out


def adjoint_loop(Gd, Cd, Ed, gz, nglam, ym, rho, K):
    """The HARD adjoint loop on the masked y: admm_adjoint_ref.adjoint_loop (box) or admm_lin_adjoint_ref.adjoint_loop (rows)."""
    if Ed is None:
        return ar.adjoint_loop(Gd, Cd, gz, nglam, ym, rho, K)
    return la.adjoint_loop(Gd, Cd, Ed, gz, nglam, ym, rho, K)


def primal(kind, h, k):
    """The primal output of iteration k: w for the box (box_qp_solve's convention), z for the rows."""
    return h["w" if kind == "box" else "z"][k]


@functools.lru_cache(maxsize=None)
def reference(kind):
    """Per problem: the converged forward point, its sets, the dense adjoint on the held rows and the gradients it implies."""
    nx, nu, mx, mu, N, B = dims(kind)
    _, _, lo, hi, kappa, gz, glam = fixture(kind)
    out = []
    for b, h in enumerate(forward(kind)):
        Gd, Cd, Ed, g, c = dense_problem(kind, b)
        rho = FIXTURE_RHO[kind][b]
        z, lam, y = primal(kind, h, -1), h["lam"][-1], h["y"][-1]
        s = sets(y, kappa[b], rho)
        az, alam, nu_rows = dense_adjoint(Gd, Cd, Ed, gz[b], glam[b], s[1] | s[2])
        out.append(dict(Gd=Gd, Cd=Cd, Ed=Ed, g=g, c=c, z=z, lam=lam, y=y, sets=s, az=az, alam=alam, nu=nu_rows,
                        grads=gradients(nx, nu, mx, mu, N, Ed, z, lam, rho * y, az, alam, nu_rows, s)))
    return out


@functools.lru_cache(maxsize=None)
def loop_reference(kind):
    """Per problem: what the two fp64 LOOPS give after K_FWD forward and K_ADJ adjoint iterations, next to reference()."""
    nx, nu, mx, mu, N, B = dims(kind)
    _, _, lo, hi, kappa, gz, glam = fixture(kind)
    out = []
    for b, (h, r) in enumerate(zip(forward(kind), reference(kind))):
        rho = FIXTURE_RHO[kind][b]
        z, lam, y = primal(kind, h, K_FWD - 1), h["lam"][K_FWD - 1], h["y"][K_FWD - 1]
        ym = mask_ref(np.float64, y, kappa[b], rho)
        lp = adjoint_loop(r["Gd"], r["Cd"], r["Ed"], gz[b], -glam[b], ym, rho, K_ADJ)
        az = lp["wa" if kind == "box" else "az"][-1]
        alam, ya = lp["alam"][-1], lp["ya"][-1]
        out.append(dict(z=z, lam=lam, y=y, az=az, alam=alam, ya=ya,
                        grads=gradients(nx, nu, mx, mu, N, r["Ed"], z, lam, rho * y, az, alam, rho * ya, sets(y, kappa[b], rho))))
    return out


@functools.lru_cache(maxsize=None)
def forward_f32(kind, K=K_FWD):
    """The forward loop with every vector operation in fp32 (the lines of admm_soft_ref.soft on fp32 arrays, the dense inverse
    rounded to fp32): y [B, nw] after K iterations, fp32."""
    _, _, lo, hi, kappa, _, _ = fixture(kind)
    F = np.float32
    ys = []
    for b in range(FIXTURE_SHAPE[3]):
        Gd, Cd, Ed, g, c = dense_problem(kind, b)
        rho, nz = F(FIXTURE_RHO[kind][b]), Gd.shape[0]
        E = np.eye(nz) if Ed is None else Ed
        K64 = np.zeros((nz + Cd.shape[0],) * 2)
        K64[:nz, :nz], K64[:nz, nz:], K64[nz:, :nz] = Gd + FIXTURE_RHO[kind][b] * (E.T @ E), Cd.T, Cd
        Kinv, E32 = np.linalg.inv(K64).astype(F), E.astype(F)
        l32, h32, k32, g32, c32 = (a.astype(F) for a in (lo[b], hi[b], kappa[b], g, c))
        w, y = sr.soft_init(np.zeros(l32.size, F), l32, h32, k32), np.zeros(l32.size, F)
        gt = g32 - rho * (E32.T @ (w - y))
        for _ in range(K):
            z = (Kinv @ np.concatenate([-gt, c32]))[:nz]
            w, y = sr.soft(E32 @ z + y, l32, h32, k32, rho)
            gt = g32 - rho * (E32.T @ (w - y))
            assert y.dtype == F
        ys.append(y)
    return np.array(ys)
