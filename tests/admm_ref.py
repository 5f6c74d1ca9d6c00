"""References for the box-constrained ADMM calls (gbdpcg_admm_*; not a test module).

The method, per problem, with rho > 0, the box lo <= z <= hi, the box copy w and the scaled multiplier y (mu = rho y):
    (z, lambda) solves [[G + rho I, C'], [C, 0]] (z, lambda) = (-gt, c)
    v = z + y;  w+ = v < lo ? lo : (v > hi ? hi : v);  y+ = v - w+;  gt+ = g - rho (w+ - y+)
    r_prim = ||z - w+||_inf,  r_dual = rho ||w+ - w||_inf
started by w <- clip(w), gt = g - rho (w - y).

admm        the iteration in fp64 with the dense inverse of the regularised KKT matrix (oracle.schur_oracle.dense_kkt supplies Gd, Cd)
update_ref  the elementwise formulas in a given precision, one IEEE operation per line; gt in exact rational arithmetic
box         the bounds the convergence tests use
(convergence_inputs: the three problems tests/test_admm_reference.py pins and tests/test_gpu_admm.py runs on the device)
"""
import functools
from fractions import Fraction

import numpy as np

from oracle import schur_oracle as so


def clip(v, lo, hi):
    """The comparison rule of the kernels: a NaN v stays NaN (np.clip / fmin / fmax would not say so)."""
    v = np.asarray(v)
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(v.dtype)


def admm(Gd, Cd, g, c, lo, hi, rho, K, w0, y0):
    """K iterations for one problem in fp64.  Returns a dict of arrays indexed by iteration 1 .. K at position 0 .. K-1:
    z, lam, w, y, gt (the gradient the NEXT solve takes), r_prim, r_dual; and gt0, the gradient of the first solve."""
    Gd, Cd = np.asarray(Gd, np.float64), np.asarray(Cd, np.float64)
    g, c, lo, hi = (np.asarray(a, np.float64) for a in (g, c, lo, hi))
    nz, nl = Gd.shape[0], Cd.shape[0]
    Kkt = np.zeros((nz + nl, nz + nl))
    Kkt[:nz, :nz] = Gd + rho * np.eye(nz)
    Kkt[:nz, nz:] = Cd.T
    Kkt[nz:, :nz] = Cd
    Kinv = np.linalg.inv(Kkt)
    w, y = clip(np.asarray(w0, np.float64), lo, hi), np.array(y0, np.float64)
    gt = g - rho * (w - y)
    out = {k: [] for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual")}
    out["gt0"] = gt.copy()
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, c])
        z, lam = sol[:nz], sol[nz:]
        v = z + y
        wn = clip(v, lo, hi)
        y = v - wn
        gt = g - rho * (wn - y)
        out["r_prim"].append(np.abs(z - wn).max())
        out["r_dual"].append(np.abs(rho * (wn - w)).max())
        w = wn
        for k, a in (("z", z), ("lam", lam), ("w", w), ("y", y), ("gt", gt)):
            out[k].append(a.copy())
    for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual"):
        out[k] = np.array(out[k])
    return out


def _norm(a):
    """max |a| over the last axis with NaN on top, as the device takes it (over bit patterns)."""
    a = np.abs(a)
    return np.where(np.isnan(a).any(axis=-1), a.dtype.type(np.nan), np.where(np.isnan(a), 0, a).max(axis=-1)).astype(a.dtype)


def update_ref(dtype, g, lo, hi, rho, z, w, y):
    """The elementwise formulas in `dtype` for arrays [B, nz] and rho [B]; z None: the formulas of admm_init (y is returned unchanged,
    res is None).  Every numpy operation below is one IEEE operation per element in `dtype`.
    Returns w+, y+, t = fl(w+ - y+), gt, res [B, 2]: gt is an object array of fractions.Fraction, the EXACT value of
    g - rho t (numpy has no fma), None where g, rho or t is not finite."""
    g, lo, hi, w, y = (np.asarray(a, dtype) for a in (g, lo, hi, w, y))
    rho = np.asarray(rho, dtype).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if z is None:
            wn, yn, res = clip(w, lo, hi), y, None
        else:
            z = np.asarray(z, dtype)
            v = z + y
            wn = clip(v, lo, hi)
            yn = v - wn
            res = np.stack([_norm(z - wn), _norm(rho * (wn - w))], axis=1)
        t = wn - yn
    assert all(a.dtype == np.dtype(dtype) for a in (wn, yn, t))
    gt = np.empty(t.shape, dtype=object)
    for b in range(t.shape[0]):
        r = float(rho[b, 0])
        for i in range(t.shape[1]):
            if np.isfinite(t[b, i]) and np.isfinite(g[b, i]) and np.isfinite(r):
                gt[b, i] = Fraction(float(g[b, i])) - Fraction(r) * Fraction(float(t[b, i]))
            else:
                gt[b, i] = None
    return wn, yn, t, gt, res


def box(z0, nx, nu, N):
    """Bounds around the fp64 solution z0 of the equality-constrained problem, in the layout of z (fp64 arrays holding fp32 numbers):
    with m = float32(max |z0|), every input within +-float32(0.3) m, the even state entries of the knots >= 1 below float32(0.6) m,
    everything else unbounded."""
    z0 = np.asarray(z0, np.float64)
    m = np.float32(np.abs(z0).max())
    bu, bx = np.float32(0.3) * m, np.float32(0.6) * m
    assert bu.dtype == np.float32 and bx.dtype == np.float32
    lo, hi = np.full(z0.shape, -np.inf), np.full(z0.shape, np.inf)
    sv = nx + nu
    for k in range(N):
        o = k * sv
        if k >= 1:
            hi[o:o + nx:2] = float(bx)
        if k < N - 1:
            lo[o + nx:o + sv] = -float(bu)
            hi[o + nx:o + sv] = float(bu)
    return lo, hi


CONV_SHAPE = (14, 7, 24, 3)       # nx, nu, N, batch
CONV_RHO = (3.0, 4.0, 2.5)


@functools.lru_cache(maxsize=None)
def convergence_inputs():
    """(d, lo [B, nz], hi, z0): so.gen(14, 7, 24, seed=11, batch=3, float32) held in fp64, the bounds of box() around the fp64
    solutions z0 of the equality-constrained problems.  Read-only, computed once."""
    nx, nu, N, B = CONV_SHAPE
    d = {k: v.astype(np.float64) for k, v in so.gen(nx, nu, N, seed=11, batch=B, dtype=np.float32).items()}
    z0 = np.stack([so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])[0] for b in range(B)])
    bounds = [box(z0[b], nx, nu, N) for b in range(B)]
    lo, hi = np.stack([p[0] for p in bounds]), np.stack([p[1] for p in bounds])
    for a in list(d.values()) + [lo, hi, z0]:
        a.setflags(write=False)
    return d, lo, hi, z0


@functools.lru_cache(maxsize=None)
def convergence_reference(iterations):
    """admm() on convergence_inputs() from w0 = y0 = 0, one history per problem."""
    nx, nu, N, B = CONV_SHAPE
    d, lo, hi, _ = convergence_inputs()
    out = []
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        out.append(admm(Gd, Cd, g, c, lo[b], hi[b], CONV_RHO[b], iterations, np.zeros(g.size), np.zeros(g.size)))
    return out
