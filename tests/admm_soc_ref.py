"""References for ADMM with stage-wise linear AND second-order cone rows (gbdpcg_admm_soc_*; not a test module).  Builds on
tests/admm_lin_ref.py: E, its layout, the packing of the rows, w, y, gt, rho and res are the same.

Row classes, cones = (lx, qx, lu, qu): in every x block the first lx rows are linear (lo <= (E z)_r <= hi), the other mx - lx rows
are consecutive cones of dimension qx, head row first, (E z + f)_cone in K_q = {s : ||s_{1..}||_2 <= s_0}; lu, qu likewise for the u
blocks.  On a cone row lo holds the offset f and hi is not read.

layout            per row of one problem: the first row of its cone (-1: a linear row) and the cone's dimension
sqrt_ref          the correctly rounded square root of one number of a given precision, by integer isqrt
div_ref           the correctly rounded quotient (the exact rational value, rounded once)
project_ref       the projection of the rows as the device defines it, bit for bit; also the branch each cone took
update_ref        the update / the initialisation as the device defines them, bit for bit (chains of admm_lin_ref.fma_ref)
project, update_twin, admm_soc    the same lines in plain fp64 numpy: the twin that does the convergence runs
convergence_inputs, convergence_reference   the three problems tests/test_admm_soc_reference.py pins and the device runs
"""
import functools
import math
from fractions import Fraction

import numpy as np

import admm_lin_ref as lin
import admm_ref
from admm_ref import clip
from oracle import schur_oracle as so

INSIDE, POLAR, BOUNDARY = 0, 1, 2


def layout(nx, nu, mx, mu, cones, N):
    """(head, dim) per row of one problem: head[r] is the row index of the head of r's cone, -1 on a linear row; dim[r] its q."""
    lx, qx, lu, qu = cones
    assert lx <= mx and lu <= mu and (lx == mx or (qx > 0 and (mx - lx) % qx == 0)) and (lu == mu or (qu > 0 and (mu - lu) % qu == 0))
    nw = lin.sizes(nx, nu, mx, mu, N)[1]
    head, dim = np.full(nw, -1), np.zeros(nw, int)
    for i, (m, _, _, ro, _, _) in enumerate(lin.blocks(nx, nu, mx, mu, N)):
        l, q = (lx, qx) if i % 2 == 0 else (lu, qu)       # blocks alternate Ex_k, Eu_k
        for r in range(l, m):
            head[ro + r], dim[ro + r] = ro + l + (r - l) // q * q, q
    return head, dim


def heads(head):
    return np.unique(head[head >= 0])


# ---- exact arithmetic
def sqrt_ref(x, dtype):
    """sqrt(x) for x >= 0 of `dtype`, rounded to nearest: floor(sqrt(x 4^k)) by isqrt with more than p + 2 bits and a sticky half
    (the square root of a floating-point number is never half-way between two of them).  NaN, +Inf, zeros and negative numbers: what
    IEEE sqrt gives."""
    dtype = np.dtype(dtype)
    x = float(x)
    if not np.isfinite(x) or x <= 0:
        with np.errstate(invalid="ignore"):
            return dtype.type(np.sqrt(np.float64(x)))
    f = Fraction(x)
    k = 0
    while f.denominator > 1 or f.numerator.bit_length() < 2 * 53 + 8:
        f *= 4
        k += 1
    n = f.numerator
    r = math.isqrt(n)
    val = Fraction(r) if r * r == n else Fraction(2 * r + 1, 2)
    return lin.round_to(val / Fraction(2) ** k, dtype)


def div_ref(a, b, dtype):
    dtype = np.dtype(dtype)
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)) or a == 0 or b == 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            return dtype.type(np.float64(a) / np.float64(b))
    return lin.round_to(Fraction(a) / Fraction(b), dtype)


def chain_seeded(avec, bvec, seed, dtype):
    acc = np.dtype(dtype).type(seed)
    for a, b in zip(avec, bvec):
        acc = lin.fma_ref(a, b, acc, dtype)
    return acc


def project_ref(dtype, s, lo, hi, head, dim):
    """w+ for the rows s of ONE problem (all of `dtype`), and {head row: branch} for its cones."""
    dtype = np.dtype(dtype)
    T = dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        wn = clip(s, lo, hi)
        branch = {}
        for h0 in heads(head):
            q = int(dim[h0])
            n2 = T(0)
            for i in range(1, q):
                n2 = lin.fma_ref(s[h0 + i], s[h0 + i], n2, dtype)
            a, s0 = sqrt_ref(n2, dtype), s[h0]
            if a <= s0:
                wn[h0:h0 + q], branch[h0] = s[h0:h0 + q], INSIDE
            elif a <= -s0:
                wn[h0:h0 + q], branch[h0] = T(0), POLAR
            else:
                hh = T(0.5) * T(s0 + a)
                c = div_ref(hh, a, dtype)
                wn[h0], branch[h0] = hh, BOUNDARY
                for i in range(1, q):
                    wn[h0 + i] = T(c * s[h0 + i])
                assert hh.dtype == dtype and c.dtype == dtype
    return wn, branch


def update_ref(dtype, nx, nu, mx, mu, cones, N, g, E, lo, hi, rho, z, w, y):
    """The update in `dtype` for g, z [B, nz], E [B, ne], lo (offsets f on cone rows), hi, w, y [B, nw], rho [B]; z None: the
    initialisation (y is returned unchanged, res is None).  Returns w+, y+, gt, res [B, 2] -- arrays of `dtype` holding the bits the
    device must give -- and the list of {head row: branch} per problem."""
    dtype = np.dtype(dtype)
    g, E, lo, hi, w, y, rho = (np.asarray(a, dtype) for a in (g, E, lo, hi, w, y, rho))
    head, dim = layout(nx, nu, mx, mu, cones, N)
    cone = head >= 0
    B = g.shape[0]
    wn, yn, gt = np.empty_like(w), y.copy(), np.empty_like(g)
    res = None if z is None else np.empty((B, 2), dtype)
    branches = []
    for b in range(B):
        f = np.where(cone, lo[b], dtype.type(0))
        v = np.zeros(w.shape[1], dtype)
        if z is not None:
            zb = np.asarray(z, dtype)[b]
            for m, n, eo, ro, co, _ in lin.blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for r in range(m):
                    v[ro + r] = chain_seeded(Eb[:, r], zb[co:co + n], f[ro + r] if cone[ro + r] else 0.0, dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            s = w[b] if z is None else v + y[b]
            wn[b], br = project_ref(dtype, s, lo[b], hi[b], head, dim)
            branches.append(br)
            if z is None:
                t, d = wn[b] - y[b], None
            else:
                yn[b] = s - wn[b]
                t, d = wn[b] - yn[b], wn[b] - w[b]
            t = np.where(cone, t - f, t)
            assert t.dtype == dtype
            ee = np.zeros(g.shape[1], dtype)
            for m, n, eo, ro, co, _ in lin.blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for j in range(n):
                    u = lin.chain(Eb[j], t[ro:ro + m], dtype)
                    gt[b, co + j] = lin.fma_ref(-rho[b], u, g[b, co + j], dtype)
                    if d is not None:
                        ee[co + j] = lin.chain(Eb[j], d[ro:ro + m], dtype)
            if z is not None:
                res[b, 0], res[b, 1] = lin._norm(v - wn[b]), lin._norm(rho[b] * ee)
    return wn, yn, gt, res, branches


# ---- the fp64 twin
def project(s, lo, hi, head, dim):
    """The lines of project_ref in plain fp64."""
    s = np.asarray(s, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        wn = clip(s, lo, hi)
        branch = {}
        for h0 in heads(head):
            q = int(dim[h0])
            a, s0 = np.sqrt(np.sum(s[h0 + 1:h0 + q] ** 2)), s[h0]
            if a <= s0:
                wn[h0:h0 + q], branch[h0] = s[h0:h0 + q], INSIDE
            elif a <= -s0:
                wn[h0:h0 + q], branch[h0] = 0.0, POLAR
            else:
                hh = 0.5 * (s0 + a)
                wn[h0], branch[h0] = hh, BOUNDARY
                wn[h0 + 1:h0 + q] = (hh / a) * s[h0 + 1:h0 + q]
    return wn, branch


def update_twin(nx, nu, mx, mu, cones, N, g, E, lo, hi, rho, z, w, y):
    """update_ref's outputs in plain fp64 (dense products), per problem stacked."""
    head, dim = layout(nx, nu, mx, mu, cones, N)
    cone = head >= 0
    out = []
    for b in range(np.asarray(g).shape[0]):
        Ed = lin.dense_E(nx, nu, mx, mu, N, np.asarray(E[b], np.float64))
        f = np.where(cone, lo[b], 0.0)
        if z is None:
            wn, _ = project(w[b], lo[b], hi[b], head, dim)
            yn, t, res = np.array(y[b], np.float64), wn - y[b] - f, None
        else:
            v = Ed @ np.asarray(z[b], np.float64) + f
            s = v + y[b]
            wn, _ = project(s, lo[b], hi[b], head, dim)
            yn = s - wn
            t = wn - yn - f
            res = np.array([np.abs(v - wn).max(), np.abs(rho[b] * (Ed.T @ (wn - w[b]))).max()])
        out.append((wn, yn, np.asarray(g[b], np.float64) - rho[b] * (Ed.T @ t), res))
    return tuple(None if out[0][i] is None else np.stack([o[i] for o in out]) for i in range(4))


def admm_soc(Gd, Cd, Ed, g, c, lo, hi, head, dim, rho, K, w0, y0):
    """K iterations for one problem in fp64, dense, after admm_lin_ref.admm_lin.  Returns its dict, plus "branch": the branches of the
    first and of the last update."""
    Gd, Cd, Ed = (np.asarray(a, np.float64) for a in (Gd, Cd, Ed))
    g, c, lo, hi = (np.asarray(a, np.float64) for a in (g, c, lo, hi))
    f = np.where(head >= 0, lo, 0.0)
    nz, nl = Gd.shape[0], Cd.shape[0]
    Kkt = np.zeros((nz + nl, nz + nl))
    Kkt[:nz, :nz] = Gd + rho * (Ed.T @ Ed)
    Kkt[:nz, nz:] = Cd.T
    Kkt[nz:, :nz] = Cd
    Kinv = np.linalg.inv(Kkt)
    w, _ = project(np.asarray(w0, np.float64), lo, hi, head, dim)
    y = np.array(y0, np.float64)
    gt = g - rho * (Ed.T @ (w - y - f))
    out = {k: [] for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual")}
    out["gt0"], out["branch"] = gt.copy(), []
    for it in range(K):
        sol = Kinv @ np.concatenate([-gt, c])
        z, lam = sol[:nz], sol[nz:]
        v = Ed @ z + f
        s = v + y
        wn, br = project(s, lo, hi, head, dim)
        y = s - wn
        gt = g - rho * (Ed.T @ (wn - y - f))
        out["r_prim"].append(np.abs(v - wn).max())
        out["r_dual"].append(np.abs(rho * (Ed.T @ (wn - w))).max())
        w = wn
        if it in (0, K - 1):
            out["branch"].append(br)
        for k, a in (("z", z), ("lam", lam), ("w", w), ("y", y), ("gt", gt)):
            out[k].append(a.copy())
    for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual"):
        out[k] = np.array(out[k])
    return out


# ---- the convergence problems: a q = 4 thrust cone on u, 2 linear rows + a q = 3 cone on x
CONV_SHAPE = admm_ref.CONV_SHAPE      # nx, nu, N, batch
CONV_ROWS = (5, 4)                    # mx, mu
CONV_CONES = (2, 3, 0, 4)             # lx, qx, lu, qu
CONV_RHO = admm_ref.CONV_RHO
CONV_SLOPE, CONV_OFFSET, CONV_STATE, CONV_SLACK = 2.0, 0.1, 0.2, 64.0     # CONV_OFFSET .. CONV_SLACK: fractions of max |z0|, float32


def rows(z0, nx, nu, N):
    """(E, lo, hi) of one problem around the fp64 solution z0 of the equality-constrained problem, fp64 arrays holding fp32 numbers.
    With m = float32(max |z0|) and f = float32(CONV_OFFSET) m:
      u block   ||(u_0, u_1, u_2)||_2 <= CONV_SLOPE u_3 + f: a thrust whose norm is bounded by a throttle input (q = 4);
      x block   the two state rows of admm_lin_ref.rows (x_0 + x_2 and x_1 below float32(CONV_STATE) m from knot 1 on), then the
                friction-like cone ||(x_3, x_4)||_2 <= CONV_SLOPE x_5 + f (q = 3); at knot 0, whose x is given, the offset is
                float32(CONV_SLACK) m, which no x_0 of these problems comes near.
    A head row that depends on z lets all three branches of the projection occur (a constant bound is never in the polar cone).
    hi on the cone rows is NaN: nothing may read it."""
    mx, mu = CONV_ROWS
    _, nw, ne, _ = lin.sizes(nx, nu, mx, mu, N)
    m = np.float32(np.abs(np.asarray(z0, np.float64)).max())
    f, slack, bx = (float(np.float32(v) * m) for v in (CONV_OFFSET, CONV_SLACK, CONV_STATE))
    Ex, Eu = np.zeros((mx, nx)), np.zeros((mu, nu))
    Ex[0, 0] = Ex[0, 2] = Ex[1, 1] = 1.0
    Ex[2, 5], Ex[3, 3], Ex[4, 4] = CONV_SLOPE, 1.0, 1.0
    Eu[0, 3], Eu[1, 0], Eu[2, 1], Eu[3, 2] = CONV_SLOPE, 1.0, 1.0, 1.0
    E, lo, hi = np.zeros(ne), np.zeros(nw), np.full(nw, np.nan)
    for k, (r, n, eo, ro, _, _) in enumerate(lin.blocks(nx, nu, mx, mu, N)):
        state = k % 2 == 0
        E[eo:eo + r * n] = (Ex if state else Eu).T.reshape(-1)
        if state:
            lo[ro:ro + 2], hi[ro:ro + 2] = -np.inf, (bx if ro > 0 else np.inf)
            lo[ro + 2] = f if ro > 0 else slack
        else:
            lo[ro] = f
    return E, lo, hi


@functools.lru_cache(maxsize=None)
def convergence_inputs():
    """(d, E [B, ne], lo [B, nw], hi, z0): the problems of admm_ref.convergence_inputs() with the rows of rows().  Read-only."""
    nx, nu, N, B = CONV_SHAPE
    d, _, _, z0 = admm_ref.convergence_inputs()
    parts = [rows(z0[b], nx, nu, N) for b in range(B)]
    E, lo, hi = (np.stack([p[i] for p in parts]) for i in range(3))
    for a in (E, lo, hi):
        a.setflags(write=False)
    return d, E, lo, hi, z0


@functools.lru_cache(maxsize=None)
def convergence_reference(iterations):
    """admm_soc() on convergence_inputs() from w0 = y0 = 0, one history per problem."""
    nx, nu, N, B = CONV_SHAPE
    mx, mu = CONV_ROWS
    d, E, lo, hi, _ = convergence_inputs()
    head, dim = layout(nx, nu, mx, mu, CONV_CONES, N)
    out = []
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = lin.dense_E(nx, nu, mx, mu, N, E[b])
        out.append(admm_soc(Gd, Cd, Ed, g, c, lo[b], hi[b], head, dim, CONV_RHO[b], iterations, np.zeros(lo[b].size),
                            np.zeros(lo[b].size)))
    return out
