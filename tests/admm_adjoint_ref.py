"""References for the backward pass of the hard box QP (gbdpcg_admm_adjoint_*, gbdpcg_admm_grad_bounds_*,
gbd_pcg_amd.autograd.box_qp_solve; not a test module).

Forward (tests/admm_ref.py): min 1/2 z'Gz + g'z subject to Cz = c, lo <= z <= hi, with G z + g + C' lambda + rho y = 0 at the solution;
y_i < 0 where z_i = lo_i, y_i > 0 where z_i = hi_i, exactly 0 elsewhere.  For a scalar l with gz = dl/dz, glam = dl/dlambda and the
active set A = {i: y_i != 0} the adjoint pair solves
    G a_z + gz + C' a_lambda + nu = 0,   C a_z = -glam,   (a_z)_A = 0,   nu supported on A
-- the box QP with g := gz, c := -glam and the degenerate box lo = hi = 0 on A, (-Inf, +Inf) elsewhere -- and
    dl/dg = a_z   dl/dc = -a_lambda   dl/dlo_i = -nu_i (y_i < 0)   dl/dhi_i = -nu_i (y_i > 0)   dl/dG, dl/dC: kkt_grad_ref.block_grads
A weakly active entry (on its bound with y_i = 0) counts as free.

degenerate_box      the explicit bounds the mask stands for: +0, +0 where yf != 0 (a NaN yf too), -Inf, +Inf elsewhere
update_ref          the masked elementwise formulas in a given precision, one IEEE operation per line; gt in exact rationals
grad_bounds_ref     glo = yf < 0 ? -(rho ya) : +0, ghi = yf > 0 ? -(rho ya) : +0
adjoint_loop        the adjoint ADMM iteration in fp64 with the dense inverse of the regularised KKT matrix
dense_adjoint       the reduced KKT system with the rows and columns of A pinned, plain numpy
active_set_solve    the forward solution for a GIVEN active set, dense (what the central differences perturb)
gradients           every gradient the adjoint pair implies, packed as the device packs them
fixture, forward    the pinned problems and their converged forward loop
"""
import functools
from fractions import Fraction

import numpy as np

import admm_ref
import kkt_grad_ref
from oracle import schur_oracle as so


def degenerate_box(yf, dtype):
    yf = np.asarray(yf, dtype)
    m = yf != 0      # NaN != 0: active
    return np.where(m, dtype(0.0), dtype(-np.inf)).astype(dtype), np.where(m, dtype(0.0), dtype(np.inf)).astype(dtype)


def pin(v, yf):
    """m ? (v < 0 ? 0 : (v > 0 ? 0 : v)) : v by comparisons: a NaN v stays NaN, v = -0 stays -0."""
    v = np.asarray(v)
    zero = v.dtype.type(0.0)
    return np.where(yf != 0, np.where(v < 0, zero, np.where(v > 0, zero, v)), v).astype(v.dtype)


def update_ref(dtype, gz, yf, rho, az, w, y):
    """The masked formulas in `dtype` for arrays [B, nz] and rho [B]; az None: those of the init (y is returned unchanged, res is
    None).  Every numpy operation below is one IEEE operation per element in `dtype`.  Returns w+, y+, t = fl(w+ - y+), gt, res [B, 2]
    like admm_ref.update_ref: gt is an object array of fractions.Fraction, None where gz, rho or t is not finite."""
    gz, yf, w, y = (np.asarray(a, dtype) for a in (gz, yf, w, y))
    rho = np.asarray(rho, dtype).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if az is None:
            wn, yn, res = pin(w, yf), y, None
        else:
            az = np.asarray(az, dtype)
            v = az + y
            wn = pin(v, yf)
            yn = v - wn
            res = np.stack([admm_ref._norm(az - wn), admm_ref._norm(rho * (wn - w))], axis=1)
        t = wn - yn
    assert all(a.dtype == np.dtype(dtype) for a in (wn, yn, t))
    gt = np.empty(t.shape, dtype=object)
    for b in range(t.shape[0]):
        r = float(rho[b, 0])
        for i in range(t.shape[1]):
            if np.isfinite(t[b, i]) and np.isfinite(gz[b, i]) and np.isfinite(r):
                gt[b, i] = Fraction(float(gz[b, i])) - Fraction(r) * Fraction(float(t[b, i]))
            else:
                gt[b, i] = None
    return wn, yn, t, gt, res


def grad_bounds_ref(dtype, yf, rho, ya):
    """One multiplication and one negation per element in `dtype`; +0 where the comparison fails (a NaN yf fails both)."""
    yf, ya = np.asarray(yf, dtype), np.asarray(ya, dtype)
    rho = np.asarray(rho, dtype).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        n = -(rho * ya)
    zero = dtype(0.0)
    return np.where(yf < 0, n, zero).astype(dtype), np.where(yf > 0, n, zero).astype(dtype)


def kkt_inverse(Gd, Cd, rho):
    nz, nl = Gd.shape[0], Cd.shape[0]
    K = np.zeros((nz + nl, nz + nl))
    K[:nz, :nz], K[:nz, nz:], K[nz:, :nz] = Gd + rho * np.eye(nz), Cd.T, Cd
    return np.linalg.inv(K)


def adjoint_loop(Gd, Cd, gz, nglam, yf, rho, K):
    """K adjoint iterations for one problem in fp64 from wa = ya = 0.  Returns a dict of arrays indexed by iteration 1 .. K at position
    0 .. K-1: az, alam, wa, ya."""
    gz, nglam, yf = (np.asarray(a, np.float64) for a in (gz, nglam, yf))
    nz = Gd.shape[0]
    Kinv = kkt_inverse(np.asarray(Gd, np.float64), np.asarray(Cd, np.float64), rho)
    w, y = pin(np.zeros(nz), yf), np.zeros(nz)
    gt = gz - rho * (w - y)
    out = {k: [] for k in ("az", "alam", "wa", "ya")}
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, nglam])
        az, alam = sol[:nz], sol[nz:]
        v = az + y
        w = pin(v, yf)
        y = v - w
        gt = gz - rho * (w - y)
        for k, a in (("az", az), ("alam", alam), ("wa", w), ("ya", y)):
            out[k].append(a.copy())
    return {k: np.array(v) for k, v in out.items()}


def dense_adjoint(Gd, Cd, gz, glam, active):
    """(a_z, a_lambda, nu): the KKT system with the rows and columns of `active` (a boolean mask) pinned to a_z = 0, and the
    multiplier of the pins from the rows left out."""
    nz, nl = Gd.shape[0], Cd.shape[0]
    F = np.flatnonzero(~active)
    K = np.zeros((F.size + nl, F.size + nl))
    K[:F.size, :F.size], K[:F.size, F.size:], K[F.size:, :F.size] = Gd[np.ix_(F, F)], Cd[:, F].T, Cd[:, F]
    sol = np.linalg.solve(K, -np.concatenate([np.asarray(gz, np.float64)[F], np.asarray(glam, np.float64)]))
    az = np.zeros(nz)
    az[F] = sol[:F.size]
    alam = sol[F.size:]
    nu = -(Gd @ az + gz + Cd.T @ alam)
    nu[F] = 0.0
    return az, alam, nu


def active_set_solve(Gd, Cd, g, c, lo, hi, at_lo, at_hi):
    """(z, lambda, mu) with z = lo on at_lo, z = hi on at_hi and the KKT conditions on the rest; mu = -(G z + g + C' lambda) on the
    active entries, 0 elsewhere.  The set is optimal iff mu <= 0 on at_lo, mu >= 0 on at_hi and lo <= z <= hi."""
    nz, nl = Gd.shape[0], Cd.shape[0]
    A = at_lo | at_hi
    F = np.flatnonzero(~A)
    z = np.zeros(nz)
    z[at_lo], z[at_hi] = lo[at_lo], hi[at_hi]
    K = np.zeros((F.size + nl, F.size + nl))
    K[:F.size, :F.size], K[:F.size, F.size:], K[F.size:, :F.size] = Gd[np.ix_(F, F)], Cd[:, F].T, Cd[:, F]
    rhs = np.concatenate([-(g[F] + Gd[np.ix_(F, np.flatnonzero(A))] @ z[A]), c - Cd[:, A] @ z[A]])
    sol = np.linalg.solve(K, rhs)
    z[F] = sol[:F.size]
    lam = sol[F.size:]
    mu = -(Gd @ z + g + Cd.T @ lam)
    mu[F] = 0.0
    return z, lam, mu


def gradients(nx, nu, N, z, lam, az, alam, nu_pin, at_lo, at_hi):
    gG, gC = kkt_grad_ref.block_grads(nx, nu, N, z, lam, az, alam)
    return {"G": gG, "C": gC, "g": az.copy(), "c": -alam, "lo": np.where(at_lo, -nu_pin, 0.0), "hi": np.where(at_hi, -nu_pin, 0.0)}


# ---- the pinned fixture: fp64 arrays holding fp32 numbers, bounds on the inputs alone (the states follow the dynamics)
FIXTURE_SHAPES = [(3, 2, 4, 2), (14, 7, 3, 2)]     # nx, nu, N, batch
FIXTURE_RHO = (3.0, 4.0)
FIXTURE_SEED = 113
BOUND_FRACTION = 0.3     # every input within +-float32(0.3) max |u0|, u0 the inputs of the equality-constrained solution
MARGIN = 1e-2            # strict complementarity: every active |y|, every free entry's distance to its bounds


@functools.lru_cache(maxsize=None)
def fixture(nx, nu, N, B):
    """(d, lo [B, nz], hi, gz [B, nz], glam [B, nx N]): so.gen held in fp64 after a round trip through fp32, the bounds around the
    equality-constrained solutions, the cotangents of the loss l = gz' w + glam' lambda.  Read-only."""
    d = {k: v.astype(np.float32).astype(np.float64) for k, v in so.gen(nx, nu, N, seed=FIXTURE_SEED, batch=B, dtype=np.float64).items()}
    sv, nz = nx + nu, (nx + nu) * N - nu
    isu = np.zeros(nz, bool)
    for k in range(N - 1):
        isu[k * sv + nx:(k + 1) * sv] = True
    lo, hi = np.full((B, nz), -np.inf), np.full((B, nz), np.inf)
    for b in range(B):
        z0 = so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])[0]
        bound = float(np.float32(BOUND_FRACTION) * np.float32(np.abs(z0[isu]).max()))
        lo[b, isu], hi[b, isu] = -bound, bound
    rng = np.random.default_rng(FIXTURE_SEED + 1)
    gz = rng.standard_normal((B, nz)).astype(np.float32).astype(np.float64)
    glam = rng.standard_normal((B, nx * N)).astype(np.float32).astype(np.float64)
    for a in list(d.values()) + [lo, hi, gz, glam]:
        a.setflags(write=False)
    return d, lo, hi, gz, glam


@functools.lru_cache(maxsize=None)
def forward(nx, nu, N, B, K):
    """admm_ref.admm on the fixture from w0 = y0 = 0, K iterations, one history per problem."""
    d, lo, hi, _, _ = fixture(nx, nu, N, B)
    out = []
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        out.append(admm_ref.admm(Gd, Cd, g, c, lo[b], hi[b], FIXTURE_RHO[b], K, np.zeros(g.size), np.zeros(g.size)))
    return out


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, K=3000):
    """Per problem: the converged forward point (w, lam, y of iteration K), its active sets, the dense adjoint and the gradients it
    implies."""
    d, lo, hi, gz, glam = fixture(nx, nu, N, B)
    out = []
    for b, h in enumerate(forward(nx, nu, N, B, K)):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        w, lam, y = h["w"][-1], h["lam"][-1], h["y"][-1]
        at_lo, at_hi = y < 0, y > 0
        az, alam, nu_pin = dense_adjoint(Gd, Cd, gz[b], glam[b], at_lo | at_hi)
        out.append(dict(Gd=Gd, Cd=Cd, g=g, c=c, w=w, lam=lam, y=y, at_lo=at_lo, at_hi=at_hi, az=az, alam=alam, nu=nu_pin,
                        grads=gradients(nx, nu, N, w, lam, az, alam, nu_pin, at_lo, at_hi)))
    return out


K_FWD, K_ADJ = 320, 320      # the counts at which the fp64 loops above have converged on the fixture (tests/test_admm_adjoint_reference.py)


@functools.lru_cache(maxsize=None)
def loop_reference(nx, nu, N, B):
    """Per problem: what the two fp64 LOOPS give after K_FWD forward and K_ADJ adjoint iterations -- the point, the adjoint pair and
    the gradients -- next to reference(), the dense answer they converge to."""
    d, lo, hi, gz, glam = fixture(nx, nu, N, B)
    out = []
    for b, (h, r) in enumerate(zip(forward(nx, nu, N, B, 3000), reference(nx, nu, N, B))):
        w, lam, y = h["w"][K_FWD - 1], h["lam"][K_FWD - 1], h["y"][K_FWD - 1]
        lp = adjoint_loop(r["Gd"], r["Cd"], gz[b], -glam[b], y, FIXTURE_RHO[b], K_ADJ)
        wa, alam, ya = lp["wa"][-1], lp["alam"][-1], lp["ya"][-1]
        out.append(dict(w=w, lam=lam, y=y, wa=wa, alam=alam, ya=ya,
                        grads=gradients(nx, nu, N, w, lam, wa, alam, FIXTURE_RHO[b] * ya, y < 0, y > 0)))
    return out


def converged_bound(loop, dense, replays, step_tol):
    """The bound of tests/test_gpu_admm.py::test_eighty_replays_converge_like_the_reference for an array the device reaches by
    `replays` iterations: twice the reference loop's own distance at that count plus the per-step tolerance accumulated over them."""
    return 2 * np.abs(loop - dense).max() + replays * step_tol * np.abs(dense).max()
