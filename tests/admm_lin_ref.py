"""References for ADMM with stage-wise linear inequality rows (gbdpcg_admm_lin_*; not a test module).

Per problem, with rho > 0, the rows lo <= E z <= hi, the copy w of E z and the scaled multiplier y (mu = rho y):
    (z, lambda) solves [[G + rho E'E, C'], [C, 0]] (z, lambda) = (-gt, c)
    v = E z;  s = v + y;  w+ = s < lo ? lo : (s > hi ? hi : s);  y+ = s - w+;  gt+ = g - rho E'(w+ - y+)
    r_prim = ||E z - w+||_inf,  r_dual = rho ||E'(w+ - w)||_inf
started by w <- clip(w), gt = g - rho E'(w - y).  E is block-diagonal with the blocks of G: Ex_k (mx x nx) on x_k, Eu_k (mu x nu) on
u_k, packed [Ex_0 Eu_0 Ex_1 ... Ex_{N-1}], every block column-major; the rows are packed [mx | mu | mx | ... | mx].

blocks, dense_E   the packed layout, and E as a dense [nw, nz] matrix
identity_E        the packed E of the box (mx = nx, mu = nu, every block the identity)
admm_lin          the iteration in fp64 with the dense inverse of the KKT matrix of G + rho E'E, after admm_ref.admm
fma_ref           ONE fused multiply-add in a given precision: the exact rational value (fractions.Fraction), rounded once
form_ref          Gt = G + rho E'E as the device defines it, bit for bit (chains of fma_ref)
update_ref        the update / the initialisation as the device defines them, bit for bit
convergence_inputs, convergence_reference   the three problems tests/test_admm_lin_reference.py pins and the device runs
"""
import functools
from fractions import Fraction

import numpy as np

import admm_ref
from admm_ref import clip
from oracle import schur_oracle as so


def sizes(nx, nu, mx, mu, N):
    """Elements per problem: nz (g), nw (rows), ne (E), ng (G)."""
    return (nx + nu) * N - nu, (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu, (nx * nx + nu * nu) * N - nu * nu


def blocks(nx, nu, mx, mu, N):
    """The diagonal blocks in storage order: (rows m, columns n, offset in E, first row, first column, offset of the block of G)."""
    out = []
    for k in range(N):
        eo, ro, co, go = k * (mx * nx + mu * nu), k * (mx + mu), k * (nx + nu), k * (nx * nx + nu * nu)
        out.append((mx, nx, eo, ro, co, go))
        if k < N - 1:
            out.append((mu, nu, eo + mx * nx, ro + mx, co + nx, go + nx * nx))
    return out


def dense_E(nx, nu, mx, mu, N, E):
    """One problem's packed E as a dense [nw, nz] matrix of E's dtype."""
    E = np.asarray(E)
    nz, nw, ne, _ = sizes(nx, nu, mx, mu, N)
    assert E.shape == (ne,)
    Ed = np.zeros((nw, nz), E.dtype)
    for m, n, eo, ro, co, _ in blocks(nx, nu, mx, mu, N):
        Ed[ro:ro + m, co:co + n] = E[eo:eo + m * n].reshape(n, m).T
    return Ed


def identity_E(nx, nu, N, dtype=np.float64):
    nz, nw, ne, _ = sizes(nx, nu, nx, nu, N)
    E = np.zeros(ne, dtype)
    for m, n, eo, _, _, _ in blocks(nx, nu, nx, nu, N):
        E[eo:eo + m * n] = np.eye(m, dtype=dtype).reshape(-1)
    return E


def admm_lin(Gd, Cd, Ed, g, c, lo, hi, rho, K, w0, y0):
    """K iterations for one problem in fp64, dense.  Returns what admm_ref.admm returns (w, y have the length of the rows); with
    Ed = I every operation below gives the bits of the one in admm_ref.admm."""
    Gd, Cd, Ed = (np.asarray(a, np.float64) for a in (Gd, Cd, Ed))
    g, c, lo, hi = (np.asarray(a, np.float64) for a in (g, c, lo, hi))
    nz, nl = Gd.shape[0], Cd.shape[0]
    Kkt = np.zeros((nz + nl, nz + nl))
    Kkt[:nz, :nz] = Gd + rho * (Ed.T @ Ed)
    Kkt[:nz, nz:] = Cd.T
    Kkt[nz:, :nz] = Cd
    Kinv = np.linalg.inv(Kkt)
    w, y = clip(np.asarray(w0, np.float64), lo, hi), np.array(y0, np.float64)
    gt = g - rho * (Ed.T @ (w - y))
    out = {k: [] for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual")}
    out["gt0"] = gt.copy()
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, c])
        z, lam = sol[:nz], sol[nz:]
        v = Ed @ z
        s = v + y
        wn = clip(s, lo, hi)
        y = s - wn
        gt = g - rho * (Ed.T @ (wn - y))
        out["r_prim"].append(np.abs(v - wn).max())
        out["r_dual"].append(np.abs(rho * (Ed.T @ (wn - w))).max())
        w = wn
        for k, a in (("z", z), ("lam", lam), ("w", w), ("y", y), ("gt", gt)):
            out[k].append(a.copy())
    for k in ("z", "lam", "w", "y", "gt", "r_prim", "r_dual"):
        out[k] = np.array(out[k])
    return out


# ---- exact arithmetic
_FMT = {np.dtype(np.float32): (24, -149, 128), np.dtype(np.float64): (53, -1074, 1024)}   # precision, log2 of the least subnormal, emax + 1


def round_to(x, dtype):
    """The Fraction x != 0 rounded to nearest, ties to even, in `dtype` (a numpy scalar)."""
    dtype = np.dtype(dtype)
    if dtype == np.dtype(np.float64):
        return np.float64(float(x))      # int / int true division: correctly rounded by the language
    p, emin, emax = _FMT[dtype]
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                      # 2^e <= a < 2^(e+1)
    q = max(e - (p - 1), emin)
    n = round(a / Fraction(2) ** q)                                 # Python rounds a Fraction half to even
    mag = float(n) * 2.0 ** q if n.bit_length() + q <= emax else float("inf")
    return dtype.type(-mag if x < 0 else mag)


def fma_ref(a, b, c, dtype):
    """fma(a, b, c) for finite numbers of `dtype`: the exact value, rounded once.  Non-finite operands: what a * b + c gives (Inf
    and NaN come out as the hardware gives them, apart from the payload)."""
    dtype = np.dtype(dtype)
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return dtype.type(np.float64(a) * np.float64(b) + np.float64(c))
    x = Fraction(a) * Fraction(b) + Fraction(c)
    if x:
        return round_to(x, dtype)
    if a * b != 0 or c != 0:
        return dtype.type(0.0)                       # exact cancellation: +0 in round-to-nearest
    neg = (np.signbit(a) != np.signbit(b)) and np.signbit(c)       # a zero product plus a zero: -0 only if both are
    return dtype.type(-0.0 if neg else 0.0)


def chain(avec, bvec, dtype):
    acc = np.dtype(dtype).type(0.0)
    for a, b in zip(avec, bvec):
        acc = fma_ref(a, b, acc, dtype)
    return acc


def form_ref(dtype, nx, nu, mx, mu, N, G, E, rho):
    """Gt [B, ng] of `dtype` for G [B, ng], E [B, ne], rho [B]: per block P(i,j) = chain over rows r of E(r,i) E(r,j),
    Gt(i,j) = fma(rho, P(i,j), G(i,j))."""
    G, E, rho = np.asarray(G, dtype), np.asarray(E, dtype), np.asarray(rho, dtype)
    Gt = np.empty_like(G)
    for b in range(G.shape[0]):
        for m, n, eo, _, _, go in blocks(nx, nu, mx, mu, N):
            Eb = E[b, eo:eo + m * n].reshape(n, m)       # Eb[j] is column j
            for j in range(n):
                for i in range(j + 1):
                    P = chain(Eb[i], Eb[j], dtype)      # = P(j,i): the same products (IEEE * commutes) in the same order
                    for at in {go + i + j * n, go + j + i * n}:
                        Gt[b, at] = fma_ref(rho[b], P, G[b, at], dtype)
    return Gt


def _norm(a):
    """max |a| over a 1-d array with NaN on top, as the device takes it (over bit patterns); 0 for no entry."""
    a = np.abs(a)
    if a.size == 0:
        return a.dtype.type(0)
    return a.dtype.type(np.nan) if np.isnan(a).any() else a.max()


def update_ref(dtype, nx, nu, mx, mu, N, g, E, lo, hi, rho, z, w, y):
    """The update in `dtype` for g, z [B, nz], E [B, ne], lo, hi, w, y [B, nw], rho [B]; z None: the initialisation (y is returned
    unchanged, res is None).  Returns w+, y+, gt, res [B, 2], every one an array of `dtype` holding the bits the device must give."""
    dtype = np.dtype(dtype)
    g, E, lo, hi, w, y, rho = (np.asarray(a, dtype) for a in (g, E, lo, hi, w, y, rho))
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
                wn[b] = clip(w[b], lo[b], hi[b])
                t = wn[b] - y[b]
                d = None
            else:
                s = v + y[b]
                wn[b] = clip(s, lo[b], hi[b])
                yn[b] = s - wn[b]
                t = wn[b] - yn[b]
                d = wn[b] - w[b]
            assert t.dtype == dtype
            ee = np.zeros(g.shape[1], dtype)
            for m, n, eo, ro, co, _ in blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for j in range(n):
                    u = chain(Eb[j], t[ro:ro + m], dtype)
                    gt[b, co + j] = fma_ref(-rho[b], u, g[b, co + j], dtype)
                    if d is not None:
                        ee[co + j] = chain(Eb[j], d[ro:ro + m], dtype)
            if z is not None:
                res[b, 0], res[b, 1] = _norm(v - wn[b]), _norm(rho[b] * ee)
    return wn, yn, gt, res


# ---- the convergence problems
CONV_SHAPE = admm_ref.CONV_SHAPE      # nx, nu, N, batch
CONV_ROWS = (2, 2)                    # mx, mu
CONV_RHO = admm_ref.CONV_RHO


def rows(z0, nx, nu, N):
    """(E, lo, hi) of one problem around the fp64 solution z0 of the equality-constrained problem, fp64 arrays holding fp32 numbers.
    With m = float32(max |z0|): the control rows u_0 + u_1 and u_2 - u_3 within +-float32(0.3) m, the state rows x_0 + x_2 and
    x_1 below float32(0.2) m from knot 1 on (no lower bound; the state rows of knot 0, whose x is given, have no bound at all).
    (0.2 and not the 0.6 of admm_ref.box: x_0 + x_2 and x_1 of the unconstrained solutions stay below 0.27 m / 0.47 m / 0.65 m, so
    at 0.6 m no state row binds in two of the three problems; at 0.2 m 2 / 4 / 7 of them do.)"""
    mx, mu = CONV_ROWS
    _, nw, ne, _ = sizes(nx, nu, mx, mu, N)
    m = np.float32(np.abs(np.asarray(z0, np.float64)).max())
    bu, bx = float(np.float32(0.3) * m), float(np.float32(0.2) * m)
    Ex, Eu = np.zeros((mx, nx)), np.zeros((mu, nu))
    Ex[0, 0] = Ex[0, 2] = Ex[1, 1] = 1.0
    Eu[0, 0] = Eu[0, 1] = Eu[1, 2] = 1.0
    Eu[1, 3] = -1.0
    E, lo, hi = np.zeros(ne), np.full(nw, -np.inf), np.full(nw, np.inf)
    for k, (r, n, eo, ro, _, _) in enumerate(blocks(nx, nu, mx, mu, N)):
        state = k % 2 == 0                 # blocks alternate Ex_k, Eu_k
        E[eo:eo + r * n] = (Ex if state else Eu).T.reshape(-1)
        if state and ro > 0:
            hi[ro:ro + r] = bx
        elif not state:
            lo[ro:ro + r], hi[ro:ro + r] = -bu, bu
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
    """admm_lin() on convergence_inputs() from w0 = y0 = 0, one history per problem."""
    nx, nu, N, B = CONV_SHAPE
    mx, mu = CONV_ROWS
    d, E, lo, hi, _ = convergence_inputs()
    out = []
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = dense_E(nx, nu, mx, mu, N, E[b])
        out.append(admm_lin(Gd, Cd, Ed, g, c, lo[b], hi[b], CONV_RHO[b], iterations, np.zeros(lo[b].size), np.zeros(lo[b].size)))
    return out
