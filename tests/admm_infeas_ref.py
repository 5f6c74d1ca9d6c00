"""References for the primal infeasibility certificate of the hard ADMM paths (gbdpcg_admm_infeas_*, gbdpcg_admm_lin_infeas_* and
their _shared twins; not a test module).

Problem b, min 1/2 z'Gz + g'z subject to Cz = c and lo <= E z <= hi, is infeasible iff some (dl, dm) has (Farkas)
    C'dl + E'dm = 0    and    c'dl + sum_r (dm_r > 0 ? hi_r dm_r : lo_r dm_r) < 0
and the differences of two iterates of the hard loop, dl = lambda1 - lambda0 and dm = rho (y1 - y0), tend to such a pair.  Per
problem the device gives, every line one IEEE operation or a comparison (include/gbdpcg.h has the lines):
    n = max(max |dl|, max |rho dy|)   r = max |C'dl + rho E'dy|   sigma = the support value   flag = n > 0 and r <= eps n and sigma < -eps n

cert_ref      the definition, bit for bit, on the packed layouts: chains of admm_lin_ref.fma_ref (exact rational value, rounded once).
              E None: the box form, written on its own (u = fma(1, dy_r, +0)); it has to equal the rows form at E = I.
cert_dense    the same quantities with dense matrices and numpy's operations of one dtype (products and sums rounded one by one, not
              fused): what the sweeps over thousands of iterates use.  It agrees with cert_ref to rounding, not to the bit.
loop          the hard iteration of admm_ref.admm / admm_lin_ref.admm_lin with every array and operation of ONE dtype (the inverse of
              the KKT matrix is formed in fp64 and rounded): the fp32-arithmetic run of the same reference.  In fp64 it gives the
              iterates of those two functions.
EPS, FLAG_AT_F64, FLAG_AT_F32   what tests/test_admm_infeas_reference.py pins on admm_soft_ref.infeasible_inputs().

Choosing EPS (the caller's on the device; this is the tests' value).  It is the largest power of ten for which, in fp64 and in
fp32 arithmetic alike, every problem of the infeasible fixture is flagged within INFEAS_K iterations and no iterate of a feasible
fixture is ever flagged.  On the infeasible fixture sigma / n settles at -INFEAS_GAP rho dy_0 / (rho dy_0) = -0.5, so eps = 1 can
never flag; r / n falls below 0.1 at iteration 4 to 6.  On the feasible fixtures the smallest r / n met over 3000 iterations with
sigma < 0 is 0.39 (0.39 to 1.0 per problem), in both precisions and with n down to rounding noise: close to convergence dl and dy
are the last bits of lambda and y, and C'dl + rho E'dy is noise of the same size, so the ratio stays of order 1.  0.1 separates the
two with a factor of 4 on that side; the tightest margin on the other is problem 2, r / n = 0.0978 at its pinned iteration.
"""
import functools

import numpy as np

import admm_lin_ref as lr
import admm_ref
import admm_soft_ref as sr
from admm_lin_ref import blocks, fma_ref
from admm_ref import clip
from oracle import schur_oracle as so

EPS = 0.1
# per problem of admm_soft_ref.infeasible_inputs(): the first iteration k (1-based) at which the certificate of the iterates
# (k - 1, k) sets the flag at EPS
FLAG_AT_F64 = (5, 4, 6)
FLAG_AT_F32 = (5, 4, 6)
FEASIBLE_K = 3000          # iterations of the no-false-alarm sweeps: past convergence to the last bit in both precisions
FEASIBLE_MIN_RATIO = 0.39  # the smallest r / n over those sweeps where sigma < 0 and n > 0 (pinned, rounded down)


def _norm(vals, dtype):
    """max |.| over a list of numpy scalars with NaN on top; +0 for none."""
    a = np.abs(np.asarray(vals, dtype))
    if a.size == 0:
        return np.dtype(dtype).type(0)
    return np.dtype(dtype).type(np.nan) if np.isnan(a).any() else a.max()


def cert_ref(dtype, nx, nu, mx, mu, N, C, c, E, lo, hi, rho, lam0, lam1, y0, y1, eps):
    """(cert [B, 3], flag [B] uint8) of `dtype`: the bits the device must give.  C [B, nx (nx + nu) (N - 1)] packed [A_0 B_0 A_1 ...],
    column-major blocks; c, lam0, lam1 [B, nx N]; E [B, ne] or None (the box: mx, mu are ignored, the rows are the entries of z);
    lo, hi, y0, y1 [B, nw]; rho [B]."""
    dtype = np.dtype(dtype)
    T = dtype.type
    box = E is None
    if box:
        mx, mu = nx, nu
    C, c, lo, hi, rho, lam0, lam1, y0, y1 = (np.asarray(a, dtype) for a in (C, c, lo, hi, rho, lam0, lam1, y0, y1))
    if not box:
        E = np.asarray(E, dtype)
    B = c.shape[0]
    sv, sw, sc = nx + nu, mx + mu, nx * (nx + nu)
    cert, flag = np.empty((B, 3), dtype), np.zeros(B, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            dl, dy = lam1[b] - lam0[b], y1[b] - y0[b]
            m = rho[b] * dy
            assert dl.dtype == dtype and m.dtype == dtype
            q = []
            for k in range(N):
                last = k == N - 1
                A = None if last else C[b, k * sc:k * sc + nx * nx].reshape(nx, nx)          # A[r] is column r: A(q, r) = A[r][q]
                Bk = None if last else C[b, k * sc + nx * nx:(k + 1) * sc].reshape(nu, nx)   # Bk[r] is column r
                for part, cnt in ((0, nx),) + (() if last else ((1, nu),)):
                    for r in range(cnt):
                        s = T(0.0) if part else dl[k * nx + r]
                        if not last:
                            col = Bk[r] if part else A[r]
                            for i in range(nx):
                                s = fma_ref(col[i], -dl[(k + 1) * nx + i], s, dtype)
                        if box:
                            u = fma_ref(T(1.0), dy[k * sv + part * nx + r], T(0.0), dtype)
                        else:
                            rows, eo, ro = (mu, k * (mx * nx + mu * nu) + mx * nx, k * sw + mx) if part else (mx, k * (mx * nx + mu * nu), k * sw)
                            u = T(0.0)
                            for i in range(rows):
                                u = fma_ref(E[b, eo + r * rows + i], dy[ro + i], u, dtype)
                        q.append(fma_ref(rho[b], u, s, dtype))
            n = _norm(list(dl) + list(m), dtype)
            r = _norm(q, dtype)
            sigma = T(0.0)
            for k in range(N):
                acc = T(0.0)
                for i in range(k * sw, k * sw + (mx if k == N - 1 else sw)):
                    if dy[i] > 0:
                        acc = fma_ref(hi[b, i], m[i], acc, dtype)
                    elif dy[i] < 0:
                        acc = fma_ref(lo[b, i], m[i], acc, dtype)
                for i in range(k * nx, (k + 1) * nx):
                    acc = fma_ref(c[b, i], dl[i], acc, dtype)
                sigma = T(sigma + acc)
            cert[b] = n, r, sigma
            en = T(T(eps) * n)
            flag[b] = 1 if (n > 0 and r <= en and sigma < -en) else 0
    return cert, flag


def knot_chunk(nx, nu, mx, mu, box=False):
    """The knots the kernel stages at a time (admm_infeas_knot_chunk in csrc/admm_infeas.hip): what fits 4096 elements, 1 .. 64."""
    if box:
        mx, mu = nx, nu
    per = nx * (nx + nu) + (0 if box else mx * nx + mu * nu) + 2 * nx + 3 * (mx + mu) + 1
    return max(1, min(64, 4096 // per))


def random_inputs(nx, nu, mx, mu, N, B, seed, dtype, box=False):
    """Random fp32 numbers (held in `dtype`) in the packed layouts, some infinite bounds, some exactly repeated entries of y (dy = 0)
    with both signs of zero.  E is None for the box (mx, mu ignored)."""
    rng = np.random.default_rng(seed)
    if box:
        mx, mu = nx, nu
    _, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)

    def rnd(*shape):
        return rng.standard_normal(shape).astype(np.float32).astype(dtype)
    C, c, E = rnd(B, nx * (nx + nu) * (N - 1)), rnd(B, nx * N), rnd(B, ne)
    lo, hi = -np.abs(rnd(B, nw)) - 1, np.abs(rnd(B, nw)) + 1
    lo[rng.random((B, nw)) < 0.3] = -np.inf
    hi[rng.random((B, nw)) < 0.3] = np.inf
    lam0, lam1, y0, y1 = rnd(B, nx * N), rnd(B, nx * N), rnd(B, nw), rnd(B, nw)
    still = rng.random((B, nw)) < 0.25
    y1[still] = y0[still]
    y0[0, 0], y1[0, 0] = 0.0, -0.0
    rho = (np.abs(rnd(B)) + 0.5).astype(dtype)
    return dict(C=C, c=c, E=None if box else E, lo=lo, hi=hi, rho=rho, lam0=lam0, lam1=lam1, y0=y0, y1=y1)


def box_as_rows(nx, nu, N, B, dtype):
    """The packed identity E [B, ne] that makes the rows form the box form."""
    return np.tile(lr.identity_E(nx, nu, N, dtype), (B, 1))


def cert_dense(dtype, Cd, Ed, c, lo, hi, rho, lam0, lam1, y0, y1, eps):
    """(n, r, sigma, flag) for ONE problem with dense Cd [nl, nz], Ed [nw, nz] or None (the box), numpy operations of `dtype`."""
    dtype = np.dtype(dtype)
    Cd, c, lo, hi, lam0, lam1, y0, y1 = (np.asarray(a, dtype) for a in (Cd, c, lo, hi, lam0, lam1, y0, y1))
    rho, eps = dtype.type(rho), dtype.type(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        dl, dy = lam1 - lam0, y1 - y0
        m = rho * dy
        q = Cd.T @ dl + rho * (dy if Ed is None else np.asarray(Ed, dtype).T @ dy)
        n = max(np.abs(dl).max(), np.abs(m).max())
        r = np.abs(q).max()
        up, dn = dy > 0, dy < 0
        sigma = (np.where(up, hi, 0)[up] * m[up]).sum(dtype=dtype) + (np.where(dn, lo, 0)[dn] * m[dn]).sum(dtype=dtype) + c @ dl
        en = eps * n
        return n, r, sigma, bool(n > 0 and r <= en and sigma < -en)


def loop(dtype, Gd, Cd, Ed, g, c, lo, hi, rho, K):
    """K hard iterations for one problem from w0 = y0 = 0 with every array and operation of `dtype` (Ed None: the box).  Returns lam
    [K, nl], y [K, nw], r_prim [K], r_dual [K]; position k - 1 holds iteration k."""
    dtype = np.dtype(dtype)
    Gd, Cd = np.asarray(Gd, np.float64), np.asarray(Cd, np.float64)
    nz, nl = Gd.shape[0], Cd.shape[0]
    Kkt = np.zeros((nz + nl, nz + nl))
    Kkt[:nz, :nz] = Gd + rho * (np.eye(nz) if Ed is None else np.asarray(Ed, np.float64).T @ np.asarray(Ed, np.float64))
    Kkt[:nz, nz:], Kkt[nz:, :nz] = Cd.T, Cd
    Kinv = np.linalg.inv(Kkt).astype(dtype)
    E = None if Ed is None else np.asarray(Ed, dtype)
    fwd = (lambda a: a) if E is None else (lambda a: E @ a)
    bwd = (lambda a: a) if E is None else (lambda a: E.T @ a)
    g, c, lo, hi = (np.asarray(a, dtype) for a in (g, c, lo, hi))
    rho = dtype.type(rho)
    nw = nz if E is None else E.shape[0]
    w, y = clip(np.zeros(nw, dtype), lo, hi), np.zeros(nw, dtype)
    gt = g - rho * bwd(w - y)
    out = {k: [] for k in ("lam", "y", "r_prim", "r_dual")}
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, c])
        z, lam = sol[:nz], sol[nz:]
        v = fwd(z)
        s = v + y
        wn = clip(s, lo, hi)
        y = s - wn
        gt = g - rho * bwd(wn - y)
        out["r_prim"].append(np.abs(v - wn).max())
        out["r_dual"].append(np.abs(rho * bwd(wn - w)).max())
        w = wn
        out["lam"].append(lam.copy())
        out["y"].append(y.copy())
        assert lam.dtype == dtype and y.dtype == dtype
    return {k: np.array(v) for k, v in out.items()}


def sweep(dtype, Cd, Ed, c, lo, hi, rho, hist, eps=EPS):
    """cert_dense on the iterates (k - 1, k) for k = 2 .. K of a history: arrays n, r, sigma, flag at position k - 2."""
    rec = [cert_dense(dtype, Cd, Ed, c, lo, hi, rho, hist["lam"][k - 1], hist["lam"][k], hist["y"][k - 1], hist["y"][k], eps)
           for k in range(1, len(hist["lam"]))]
    n, r, sigma, flag = (np.array([x[i] for x in rec]) for i in range(4))
    return n.astype(np.float64), r.astype(np.float64), sigma.astype(np.float64), flag.astype(bool)


def first_flag(flag):
    """The iteration k (1-based) of the first set flag of a sweep, or None."""
    return int(np.argmax(flag)) + 2 if flag.any() else None


# ---- the fixtures: one dense problem per entry, (name, Gd, Cd, Ed or None, g, c, lo, hi, rho)
def _dense(d, b):
    nx, nu, N, _ = admm_ref.CONV_SHAPE
    return so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])


@functools.lru_cache(maxsize=None)
def infeasible_problems():
    d, lo, hi, _ = sr.infeasible_inputs()
    return [("infeasible", *_dense(d, b)[:2], None, *_dense(d, b)[2:], lo[b], hi[b], admm_ref.CONV_RHO[b])
            for b in range(admm_ref.CONV_SHAPE[3])]


@functools.lru_cache(maxsize=None)
def feasible_problems():
    """Every feasible fixture of admm_ref, admm_lin_ref and admm_soft_ref (whose soft_inputs() puts kappa on the problems and the
    box of admm_ref.convergence_inputs(): the hard loop on it is the hard loop on those -- it is listed, and costs nothing, so that
    a change of that fixture is met here)."""
    nx, nu, N, B = admm_ref.CONV_SHAPE
    out = []
    d, lo, hi, _ = admm_ref.convergence_inputs()
    out += [("admm_ref", *_dense(d, b)[:2], None, *_dense(d, b)[2:], lo[b], hi[b], admm_ref.CONV_RHO[b]) for b in range(B)]
    d, E, lo, hi, _ = lr.convergence_inputs()
    mx, mu = lr.CONV_ROWS
    out += [("admm_lin_ref", *_dense(d, b)[:2], lr.dense_E(nx, nu, mx, mu, N, E[b]), *_dense(d, b)[2:], lo[b], hi[b], lr.CONV_RHO[b])
            for b in range(B)]
    d, lo, hi, _ = sr.soft_inputs()
    out += [("admm_soft_ref", *_dense(d, b)[:2], None, *_dense(d, b)[2:], lo[b], hi[b], sr.CONV_RHO[b]) for b in range(B)]
    return out


@functools.lru_cache(maxsize=None)
def history(kind, index, dtype_name, K):
    """loop() on one fixture problem, cached: kind "infeasible" or "feasible"."""
    _, Gd, Cd, Ed, g, c, lo, hi, rho = (infeasible_problems() if kind == "infeasible" else feasible_problems())[index]
    return loop(np.dtype(dtype_name), Gd, Cd, Ed, g, c, lo, hi, rho, K)
