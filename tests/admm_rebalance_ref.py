"""References for adaptive rho (gbdpcg_admm*_rebalance_*, gbdpcg_admm*_restep_*; not a test module).

The rule, per problem, from r = res[2b], s = res[2b+1], rho = rho[b] and the host's ratio >= 1, tau = 2^shift, rho_min <= rho_max,
every line ONE IEEE operation of the call's type or a comparison (so numpy of that dtype gives the bits):
    up = rho tau;  dn = rho (1 / tau)
    if      r > ratio s and up <= rho_max: rho' = up, e = +shift
    else if s > ratio r and dn >= rho_min: rho' = dn, e = -shift
    else                                   rho' = rho, e = 0
    y' = y 2^-e                            (y is not touched when e = 0)
    box: gt = fma(-rho', w - y', g)        (numpy has no fma: the exact rational value, rounded once)

rule            rho', e
rebalance_ref   rho', y', e and, for the box, gt
fma_ref         a correctly rounded fused multiply-add of arrays in a given dtype
adaptive_admm   the dense fp64 ADMM loop for the box on the schedule "P plain steps, one restep", exact KKT solves
CONV_*          the convergence fixture tests/test_admm_rebalance_reference.py pins and tests/test_gpu_admm_rebalance.py runs
"""
import functools
from fractions import Fraction

import numpy as np

import admm_ref
from oracle import schur_oracle as so


def rule(dtype, res, rho, ratio, shift, rho_min, rho_max):
    """res [B, 2], rho [B] -> (rho' [B] of dtype, e [B] int32)."""
    T = np.dtype(dtype).type
    res, rho = np.asarray(res, dtype).reshape(-1, 2), np.asarray(rho, dtype).reshape(-1)
    ratio, rho_min, rho_max = T(ratio), T(rho_min), T(rho_max)
    tau, inv = T(2.0 ** shift), T(2.0 ** -shift)
    r, s = res[:, 0], res[:, 1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        up, dn = rho * tau, rho * inv
        raise_ = (r > ratio * s) & (up <= rho_max)
        lower = ~raise_ & (s > ratio * r) & (dn >= rho_min)
    new = np.where(raise_, up, np.where(lower, dn, rho)).astype(dtype)
    e = np.where(raise_, shift, np.where(lower, -shift, 0)).astype(np.int32)
    assert up.dtype == np.dtype(dtype) and dn.dtype == np.dtype(dtype)
    return new, e


def _round_fraction(fr, dtype):
    """fr (a Fraction) rounded to nearest-even in dtype."""
    if np.dtype(dtype) == np.dtype(np.float64):
        return np.float64(float(fr))          # Fraction.__float__ is correctly rounded
    c = np.float32(float(fr))                 # within one float32 step of the answer: pick among the neighbours exactly
    cands = {float(c), float(np.nextafter(c, np.float32(-np.inf))), float(np.nextafter(c, np.float32(np.inf)))}
    finite = [v for v in cands if np.isfinite(v)]
    best = min(finite, key=lambda v: (abs(Fraction(v) - fr), int(np.float32(v).view(np.uint32)) & 1))
    if np.isinf(c) and abs(fr) >= Fraction(float(np.finfo(np.float32).max)) + Fraction(2.0 ** 103):
        return c                              # beyond the rounding boundary of the largest finite number
    return np.float32(best)


def fma_ref(dtype, a, b, c):
    """fma(a, b, c) elementwise, one rounding, for arrays of dtype (broadcast).  Non-finite operands: the value numpy's fp64
    expression gives (an Inf or a NaN needs no rounding)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype), np.asarray(b, dtype), np.asarray(c, dtype))
    out = np.empty(a.shape, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in np.ndindex(a.shape):
            x, y, z = float(a[i]), float(b[i]), float(c[i])
            if np.isfinite(x) and np.isfinite(y) and np.isfinite(z):
                fr = Fraction(x) * Fraction(y) + Fraction(z)
                if fr == 0:        # an exact zero: the product is then exact in fp64 (it is -c or 0), whose sum has IEEE's sign
                    out[i] = np.dtype(dtype).type(np.float64(x) * np.float64(y) + np.float64(z))
                else:
                    out[i] = _round_fraction(fr, dtype)
            else:
                out[i] = np.dtype(dtype).type(np.float64(x) * np.float64(y) + np.float64(z))
    return out


def rebalance_ref(dtype, res, rho, y, ratio, shift, rho_min, rho_max, g=None, w=None):
    """y [B, n].  Returns (rho', y', e, gt): gt is None without g and w (the rows form)."""
    T = np.dtype(dtype).type
    y = np.asarray(y, dtype)
    new, e = rule(dtype, res, rho, ratio, shift, rho_min, rho_max)
    scale = np.where(e > 0, T(2.0 ** -shift), np.where(e < 0, T(2.0 ** shift), T(1))).astype(dtype).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        yn = np.where((e != 0).reshape(-1, 1), y * scale, y).astype(dtype)
    # (a row with e = 0 keeps the BITS of y, a signalling NaN included: np.where copies)
    keep = e == 0
    yn.view(np.uint32 if np.dtype(dtype) == np.dtype(np.float32) else np.uint64)[keep] = \
        y.view(np.uint32 if np.dtype(dtype) == np.dtype(np.float32) else np.uint64)[keep]
    gt = None
    if g is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.asarray(w, dtype) - yn).astype(dtype)
        gt = fma_ref(dtype, -new.reshape(-1, 1), t, np.asarray(g, dtype))
    return new, yn, e, gt


# ---- the dense fp64 loop with exact solves
def adaptive_admm(Gd, Cd, g, c, lo, hi, rho0, eps, cap, period=None, ratio=10.0, shift=1, rho_min=1e-6, rho_max=1e6):
    """ADMM for one box-constrained problem in fp64 from w = y = 0, the KKT systems solved by numpy.linalg.solve.  period None: rho
    stays rho0.  Otherwise the schedule of the device loop: `period` plain iterations, then one iteration that first applies the
    rule to the residuals of the last update, rescales y, rebuilds gt and refactors -- and so on.  Stops behind the first iteration
    whose residuals are both below eps, or at `cap`.  Returns (iterations made, reached, history of (r, s, rho, e))."""
    Gd, Cd = np.asarray(Gd, np.float64), np.asarray(Cd, np.float64)
    g, c, lo, hi = (np.asarray(a, np.float64) for a in (g, c, lo, hi))
    nz, nl = Gd.shape[0], Cd.shape[0]

    def factor(rho):
        K = np.zeros((nz + nl, nz + nl))
        K[:nz, :nz], K[:nz, nz:], K[nz:, :nz] = Gd + rho * np.eye(nz), Cd.T, Cd
        return np.linalg.inv(K)

    rho = np.float64(rho0)
    Kinv = factor(rho)
    w = admm_ref.clip(np.zeros(nz), lo, hi)
    y = np.zeros(nz)
    gt = g - rho * (w - y)
    hist, res = [], None
    for k in range(1, cap + 1):
        e = 0
        if period is not None and k % (period + 1) == 0:
            new, ee = rule(np.float64, res, [rho], ratio, shift, rho_min, rho_max)
            rho, e = new[0], int(ee[0])
            y = y * 2.0 ** -e
            gt = g - rho * (w - y)
            Kinv = factor(rho)
        z = (Kinv @ np.concatenate([-gt, c]))[:nz]
        v = z + y
        wn = admm_ref.clip(v, lo, hi)
        y = v - wn
        gt = g - rho * (wn - y)
        res = np.array([[np.abs(z - wn).max(), np.abs(rho * (wn - w)).max()]])
        w = wn
        hist.append((res[0, 0], res[0, 1], float(rho), e))
        if res.max() < eps:
            return k, True, hist
    return cap, False, hist


# The convergence fixture: the three problems of admm_ref.convergence_inputs() started from a deliberately bad rho -- 16 times
# smaller, 64 and 32 times larger than the values admm_ref pins for them: a batch does not share one direction either -- and
# brought below CONV_EPS in both residuals.
CONV_SHAPE = admm_ref.CONV_SHAPE
CONV_RHO0 = tuple(r * f for r, f in zip(admm_ref.CONV_RHO, (2.0 ** -4, 2.0 ** 6, 2.0 ** 5)))
CONV_EPS = 1e-6
CONV_PERIOD = 5
CONV_CAP = 2000
CONV_RULE = dict(ratio=10.0, shift=1, rho_min=1e-6, rho_max=1e6)


@functools.lru_cache(maxsize=None)
def convergence_counts():
    """(K_fixed, K_adapt): iterations until every problem of the batch is below CONV_EPS (the slowest problem's count), with rho kept
    and with the schedule; CONV_CAP where a problem did not get there."""
    nx, nu, N, B = CONV_SHAPE
    d, lo, hi, _ = admm_ref.convergence_inputs()
    fixed, adapt = [], []
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        fixed.append(adaptive_admm(Gd, Cd, g, c, lo[b], hi[b], CONV_RHO0[b], CONV_EPS, CONV_CAP)[:2])
        adapt.append(adaptive_admm(Gd, Cd, g, c, lo[b], hi[b], CONV_RHO0[b], CONV_EPS, CONV_CAP, CONV_PERIOD, **CONV_RULE)[:2])
    return fixed, adapt
