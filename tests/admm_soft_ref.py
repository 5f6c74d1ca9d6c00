"""References for the soft (L1-penalised) ADMM calls (gbdpcg_admm_soft_*, gbdpcg_admm_lin_soft_*; not a test module).

Row r of problem b pays kappa_r dist(v_r, [lo_r, hi_r]) in the cost, v = z (box) or v = E z (rows), instead of being constrained.
Only the projection line of the hard update changes; with s = v + y, every line one IEEE operation or a comparison:
    p = s < lo ? lo : (s > hi ? hi : s);  e = s - p;  theta = kappa / rho
    w+ = e > theta ? s - theta : (e < -theta ? s + theta : p);   y+ = e > theta ? theta : (e < -theta ? -theta : e)
started by w <- (kappa == +Inf) ? clip(w) : w.  kappa = +Inf takes the third branch: the operations of the hard update.

soft, soft_init       the two lines above on arrays of one dtype
admm_soft, admm_lin_soft   the iterations in fp64, dense, after admm_ref.admm / admm_lin_ref.admm_lin (the same bits for kappa = +Inf)
update_ref, lin_update_ref   the update / the initialisation as the device defines them, after the update_ref of the two modules
soft_inputs, hard_multipliers, infeasible_inputs   the fixtures tests/test_admm_soft_reference.py pins and the device runs
"""
import functools
from fractions import Fraction

import numpy as np

import admm_lin_ref
import admm_ref
from admm_lin_ref import blocks, chain, fma_ref
from admm_ref import clip
from oracle import schur_oracle as so


def soft(s, lo, hi, kappa, rho):
    """(w+, y+) for arrays of one dtype; rho broadcasts.  One numpy operation per line of the definition."""
    s = np.asarray(s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = clip(s, lo, hi)
        e = s - p
        theta = (kappa / rho).astype(s.dtype)
        up, dn = e > theta, e < -theta
        w = np.where(up, s - theta, np.where(dn, s + theta, p)).astype(s.dtype)
        y = np.where(up, theta, np.where(dn, -theta, e)).astype(s.dtype)
    return w, y


def soft_init(w, lo, hi, kappa):
    w = np.asarray(w)
    return np.where(kappa == np.inf, clip(w, lo, hi), w).astype(w.dtype)


def _iterate(Gd, Cd, Ed, g, c, lo, hi, kappa, rho, K, w0, y0):
    """The common iteration; Ed None: the box (v = z, every product with E left out, as admm_ref.admm writes it)."""
    Gd, Cd = np.asarray(Gd, np.float64), np.asarray(Cd, np.float64)
    g, c, lo, hi, kappa = (np.asarray(a, np.float64) for a in (g, c, lo, hi, kappa))
    nz, nl = Gd.shape[0], Cd.shape[0]
    fwd = (lambda a: a) if Ed is None else (lambda a: Ed @ a)
    bwd = (lambda a: a) if Ed is None else (lambda a: Ed.T @ a)
    Kkt = np.zeros((nz + nl, nz + nl))
    Kkt[:nz, :nz] = Gd + rho * (np.eye(nz) if Ed is None else Ed.T @ Ed)
    Kkt[:nz, nz:] = Cd.T
    Kkt[nz:, :nz] = Cd
    Kinv = np.linalg.inv(Kkt)
    w, y = soft_init(np.asarray(w0, np.float64), lo, hi, kappa), np.array(y0, np.float64)
    gt = g - rho * bwd(w - y)
    out = {k: [] for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual")}
    out["gt0"] = gt.copy()
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, c])
        z, lam = sol[:nz], sol[nz:]
        v = fwd(z)
        s = v + y
        wn, y = soft(s, lo, hi, kappa, rho)
        gt = g - rho * bwd(wn - y)
        out["r_prim"].append(np.abs(v - wn).max())
        out["r_dual"].append(np.abs(rho * bwd(wn - w)).max())
        w = wn
        for k, a in (("z", z), ("lam", lam), ("w", w), ("y", y), ("gt", gt)):
            out[k].append(a.copy())
    for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual"):
        out[k] = np.array(out[k])
    return out


def admm_soft(Gd, Cd, g, c, lo, hi, kappa, rho, K, w0, y0):
    """K soft box iterations for one problem in fp64; what admm_ref.admm returns, and its bits for kappa = +Inf."""
    return _iterate(Gd, Cd, None, g, c, lo, hi, kappa, rho, K, w0, y0)


def admm_lin_soft(Gd, Cd, Ed, g, c, lo, hi, kappa, rho, K, w0, y0):
    """K soft iterations with rows; what admm_lin_ref.admm_lin returns, and its bits for kappa = +Inf."""
    return _iterate(Gd, Cd, np.asarray(Ed, np.float64), g, c, lo, hi, kappa, rho, K, w0, y0)


def update_ref(dtype, g, lo, hi, kappa, rho, z, w, y):
    """admm_ref.update_ref with the soft lines: arrays [B, nz], rho [B]; z None: the soft init.  Returns w+, y+, t, gt (exact
    Fractions, None where not finite), res [B, 2]."""
    g, lo, hi, kappa, w, y = (np.asarray(a, dtype) for a in (g, lo, hi, kappa, w, y))
    rho = np.asarray(rho, dtype).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if z is None:
            wn, yn, res = soft_init(w, lo, hi, kappa), y, None
        else:
            z = np.asarray(z, dtype)
            s = z + y
            wn, yn = soft(s, lo, hi, kappa, rho)
            res = np.stack([admm_ref._norm(z - wn), admm_ref._norm(rho * (wn - w))], axis=1)
        t = wn - yn
    assert all(a.dtype == np.dtype(dtype) for a in (wn, yn, t))
    gt = np.empty(t.shape, dtype=object)
    for b in range(t.shape[0]):
        r = float(rho[b, 0])
        for i in range(t.shape[1]):
            ok = np.isfinite(t[b, i]) and np.isfinite(g[b, i]) and np.isfinite(r)
            gt[b, i] = Fraction(float(g[b, i])) - Fraction(r) * Fraction(float(t[b, i])) if ok else None
    return wn, yn, t, gt, res


def lin_update_ref(dtype, nx, nu, mx, mu, N, g, E, lo, hi, kappa, rho, z, w, y):
    """admm_lin_ref.update_ref with the soft lines; returns w+, y+, gt, res [B, 2] of `dtype`, the bits the device must give."""
    dtype = np.dtype(dtype)
    g, E, lo, hi, kappa, w, y, rho = (np.asarray(a, dtype) for a in (g, E, lo, hi, kappa, w, y, rho))
    B = g.shape[0]
    wn, yn, gt = np.empty_like(w), y.copy(), np.empty_like(g)
    res = None if z is None else np.empty((B, 2), dtype)
    for b in range(B):
        v = np.zeros(w.shape[1], dtype)
        if z is not None:
            zb = np.asarray(z, dtype)[b]
            for m, n, eo, ro, co, _ in blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for r in range(m):
                    v[ro + r] = chain(Eb[:, r], zb[co:co + n], dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            if z is None:
                wn[b] = soft_init(w[b], lo[b], hi[b], kappa[b])
                t, d = wn[b] - y[b], None
            else:
                s = v + y[b]
                wn[b], yn[b] = soft(s, lo[b], hi[b], kappa[b], rho[b])
                t, d = wn[b] - yn[b], wn[b] - w[b]
            assert t.dtype == dtype
            ee = np.zeros(g.shape[1], dtype)
            for m, n, eo, ro, co, _ in blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for j in range(n):
                    gt[b, co + j] = fma_ref(-rho[b], chain(Eb[j], t[ro:ro + m], dtype), g[b, co + j], dtype)
                    if d is not None:
                        ee[co + j] = chain(Eb[j], d[ro:ro + m], dtype)
            if z is not None:
                res[b, 0], res[b, 1] = admm_lin_ref._norm(v - wn[b]), admm_lin_ref._norm(rho[b] * ee)
    return wn, yn, gt, res


# ---- the fixtures
CONV_SHAPE = admm_ref.CONV_SHAPE
CONV_RHO = admm_ref.CONV_RHO
KAPPA_FRACTION = 0.25     # of the largest hard multiplier of the problem: the rows above it give way, the others hold below kappa


# The device's convergence test: SOFT_K replays, where the reference's worst problem has reduced r_prim by SOFT_RATIO_REF (pinned by
# tests/test_admm_soft_reference.py) -- the regime of tests/test_gpu_admm.py (1.5e-3 at its 80 replays), above the fp32 floor of z.
# The bound on the device's ratio carries that test's headroom over its reference, 1e-2 against 1.5e-3.
SOFT_K = 40
SOFT_RATIO_REF = 1.24e-3
SOFT_RATIO_BOUND = SOFT_RATIO_REF * (1e-2 / 1.5e-3)


def _dense(b):
    nx, nu, N, _ = CONV_SHAPE
    d = admm_ref.convergence_inputs()[0]
    return so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])


def state_mask():
    """True on the state entries of z."""
    nx, nu, N, _ = CONV_SHAPE
    m = np.zeros((nx + nu) * N - nu, bool)
    for k in range(N):
        m[k * (nx + nu):k * (nx + nu) + nx] = True
    return m


@functools.lru_cache(maxsize=None)
def hard_multipliers():
    """mu = rho y [B, nz] of the converged hard reference (admm_ref.convergence_reference(4000))."""
    ref = admm_ref.convergence_reference(4000)
    mu = np.stack([CONV_RHO[b] * ref[b]["y"][-1] for b in range(CONV_SHAPE[3])])
    mu.setflags(write=False)
    return mu


@functools.lru_cache(maxsize=None)
def soft_inputs():
    """(d, lo, hi, kappa [B, nz]) on admm_ref.convergence_inputs(): on every row of problem b KAPPA_FRACTION of its largest hard
    multiplier, rounded to fp32 (fp64 arrays holding fp32 numbers).  (The state bounds of these problems do not bind, the input
    bounds do: the weight that decides is the one on the inputs.)  Read-only."""
    d, lo, hi, _ = admm_ref.convergence_inputs()
    mu = hard_multipliers()
    kappa = np.empty(lo.shape)
    for b in range(lo.shape[0]):
        kappa[b] = float(np.float32(KAPPA_FRACTION * np.abs(mu[b]).max()))
    kappa.setflags(write=False)
    return d, lo, hi, kappa


@functools.lru_cache(maxsize=None)
def soft_reference(iterations):
    """admm_soft() on soft_inputs() from w0 = y0 = 0, one history per problem."""
    d, lo, hi, kappa = soft_inputs()
    out = []
    for b in range(CONV_SHAPE[3]):
        Gd, Cd, g, c = _dense(b)
        out.append(admm_soft(Gd, Cd, g, c, lo[b], hi[b], kappa[b], CONV_RHO[b], iterations, np.zeros(g.size), np.zeros(g.size)))
    return out


# The infeasible-hard fixture: the first state of knot 0 is pinned by c (x_0 = c_0, oracle/schur_oracle.py) and its upper bound is put
# INFEAS_GAP below that value, so no point satisfies Cz = c and the box.  Soft: a finite kappa on the states.
INFEAS_GAP = 0.5
INFEAS_KAPPA = 50.0
INFEAS_K = 60             # iterations of the hard run that shows the stall
INFEAS_TOL = 1e-4         # the soft run counts as converged when r_prim and r_dual are both below it (fp64)
# pinned by tests/test_admm_soft_reference.py::test_infeasible_fixture, read by tests/test_gpu_admm_soft.py
INFEAS_HARD_FLOOR = 0.4999999   # min over problems and iterations of the hard r_prim: the gap itself, the distance of {Cz = c} from the box
INFEAS_SOFT_ITERS = (43, 66, 102)     # per problem: first iteration at which the soft reference meets INFEAS_TOL


@functools.lru_cache(maxsize=None)
def infeasible_inputs():
    """(d, lo, hi, kappa): convergence_inputs() with hi[b, 0] = c[b, 0] - INFEAS_GAP (fp32 numbers); kappa = INFEAS_KAPPA on the
    states, +Inf on the inputs."""
    d, lo, hi, _ = admm_ref.convergence_inputs()
    hi = hi.copy()
    hi[:, 0] = np.float32(d["c"][:, 0] - INFEAS_GAP).astype(np.float64)
    kappa = np.where(state_mask()[None, :], INFEAS_KAPPA, np.inf) * np.ones_like(lo)
    for a in (hi, kappa):
        a.setflags(write=False)
    return d, lo, hi, kappa


@functools.lru_cache(maxsize=None)
def infeasible_reference(iterations, soft_run):
    d, lo, hi, kappa = infeasible_inputs()
    out = []
    for b in range(CONV_SHAPE[3]):
        Gd, Cd, g, c = _dense(b)
        zero = np.zeros(g.size)
        if soft_run:
            out.append(admm_soft(Gd, Cd, g, c, lo[b], hi[b], kappa[b], CONV_RHO[b], iterations, zero, zero))
        else:
            out.append(admm_ref.admm(Gd, Cd, g, c, lo[b], hi[b], CONV_RHO[b], iterations, zero, zero))
    return out


def soft_converged_at(hist, tol=INFEAS_TOL):
    """The first iteration (1-based) at which both residuals are below tol, or None."""
    ok = (hist["r_prim"] < tol) & (hist["r_dual"] < tol)
    return int(np.argmax(ok)) + 1 if ok.any() else None
