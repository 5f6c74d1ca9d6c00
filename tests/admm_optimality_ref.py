"""References for the optimality test of the ADMM families (gbdpcg_admm_optimality_*, gbdpcg_admm_lin_optimality_* and their
_shared twins; not a test module).

Is (z, lambda, rho y) a solution of  min 1/2 z'Gz + g'z  s.t.  Cz = c,  E z in the rows' set?  Every update writes w+ = P(s),
y+ = s - w+, so w is in the set and rho y in its normal cone at w by construction; what the device evaluates per problem is
    r_s = max |G z + g + C'lambda + rho E'y|   r_e = max |C z - c|   r_r = max |E z - w|
    n_s = max(|G z|, |C'lambda + rho E'y|, |g|)   n_e = max(|C z|, |c|)   n_r = max(|E z|, |w|)
    done = r_s <= eps_abs + eps_rel n_s  and  r_e <= eps_abs + eps_rel n_e  and  r_r <= eps_abs + eps_rel n_r
every line one IEEE operation or a comparison (include/gbdpcg.h has the lines).

opt_ref       the definition, bit for bit, on the packed layouts: chains of admm_lin_ref.fma_ref (exact rational value, rounded once).
              E None: the box form, written on its own (u = fma(1, y_r, +0), v_r = z_r); it has to equal the rows form at E = I.
opt_dense     the same six quantities with dense matrices in numpy fp64, and the magnitudes sum |terms| the derived bound scales with.
chain_bound   (len + 2) u sum |terms|: the error of an fma chain of `len` terms behind one rounded seed, as kkt_refine_ref.floor.
loop          the hard iteration of admm_ref.admm / admm_lin_ref.admm_lin with every array and operation of ONE dtype (the inverse
              of the KKT matrix is formed in fp64 and rounded), recording the six quantities at every iterate (z, lambda, w+, y+).
windows       k_lo: the first iteration at which all three residuals are under 2 x their thresholds; k_hi: under 0.5 x.  A loop whose
              solves are good to well below eps must first report done inside [k_lo, k_hi].
EPS, K_LO, K_HI   what tests/test_admm_optimality_reference.py pins on admm_infeas_ref.feasible_problems().

Choosing EPS (the caller's eps_abs = eps_rel on the device; this is the tests' value): the smallest power of ten for which k_hi
exists within K_MAX = 300 iterations for every fixture problem in the fp32 emulation (loop with dtype float32): 1e-6.  At 1e-7 no
problem even reaches k_lo in fp32: r_s stalls at 2 to 4e-6, the rounding of the fp32 products behind it at n_s ~ 5, against a
threshold of 1e-7 (1 + n_s) = 6e-7.  At 1e-6 every problem reaches 0.5 x its thresholds (fp32 windows (72, 96), (112, 130),
(154, 175), (86, 100), (96, 138), (225, 271) on the first six problems), though not by much: r_s ends at 3.5e-6 on problem 0
against a threshold of 6.0e-6.  K_LO and K_HI are those of the fp64 loop at that EPS.
"""
import functools

import numpy as np

import admm_infeas_ref as ir
import admm_lin_ref as lr
from admm_lin_ref import fma_ref
from admm_ref import clip

F32, F64 = np.float32, np.float64
UNIT = {np.dtype(F32): 2.0 ** -24, np.dtype(F64): 2.0 ** -53}

EPS = 1e-6
K_MAX = 300
# per problem of admm_infeas_ref.feasible_problems(), the fp64 loop at EPS (pinned by tests/test_admm_optimality_reference.py)
K_LO = (72, 112, 154, 86, 96, 224, 72, 112, 154)
K_HI = (84, 130, 174, 100, 110, 257, 84, 130, 174)


def _norm(vals, dtype):
    """max |.| over a list of numpy scalars with NaN on top (the maximum over bit patterns); +0 for none."""
    a = np.abs(np.asarray(vals, dtype))
    if a.size == 0:
        return np.dtype(dtype).type(0)
    return np.dtype(dtype).type(np.nan) if np.isnan(a).any() else a.max()


def opt_ref(dtype, nx, nu, mx, mu, N, G, C, g, c, E, rho, z, lam, w, y, eps_abs, eps_rel):
    """(opt [B, 6], done [B] uint8) of `dtype`: the bits the device must give.  G [B, ng] packed [Q_0 R_0 Q_1 ... Q_{N-1}], C [B, nx
    (nx + nu) (N - 1)] packed [A_0 B_0 A_1 ...], column-major blocks; g, z [B, nz]; c, lam [B, nx N]; E [B, ne] or None (the box: mx,
    mu are ignored, the rows are the entries of z); w, y [B, nw]; rho [B].  G, C (and E) may have ONE row: the shared forms."""
    dtype = np.dtype(dtype)
    T = dtype.type
    box = E is None
    if box:
        mx, mu = nx, nu
    G, C, g, c, rho, z, lam, w, y = (np.asarray(a, dtype) for a in (G, C, g, c, rho, z, lam, w, y))
    if not box:
        E = np.asarray(E, dtype)
    B = g.shape[0]
    sv, sw, nn = nx + nu, mx + mu, nx * nx
    sg, sc, se = nn + nu * nu, nx * (nx + nu), mx * nx + mu * nu
    opt, done = np.empty((B, 6), dtype), np.zeros(B, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            Gb, Cb = G[b % G.shape[0]], C[b % C.shape[0]]
            Eb = None if box else E[b % E.shape[0]]
            gb, cb, zb, lb, wb, yb, r = g[b], c[b], z[b], lam[b], w[b], y[b], rho[b]
            q, a_, p, f, h, v = [], [], [], [], [], []
            for k in range(N):
                nxt = k + 1 < N
                Gk, Ck = Gb[k * sg:], Cb[k * sc:]
                x, lk = zb[k * sv:k * sv + nx], lb[k * nx:(k + 1) * nx]
                u = zb[k * sv + nx:(k + 1) * sv] if nxt else None
                nl = -lb[(k + 1) * nx:(k + 2) * nx] if nxt else None
                for part, cnt in ((0, nx),) + (((1, nu),) if nxt else ()):
                    for e in range(cnt):
                        if part == 0:
                            s, a, t = T(gb[k * sv + e] + lk[e]), T(0.0), lk[e]
                            for j in range(nx):
                                s = fma_ref(Gk[j * nx + e], x[j], s, dtype)
                                a = fma_ref(Gk[j * nx + e], x[j], a, dtype)
                            if nxt:
                                for j in range(nx):
                                    s = fma_ref(Ck[e * nx + j], nl[j], s, dtype)
                                    t = fma_ref(Ck[e * nx + j], nl[j], t, dtype)
                        else:
                            s, a, t = gb[k * sv + nx + e], T(0.0), T(0.0)
                            for j in range(nu):
                                s = fma_ref(Gk[nn + j * nu + e], u[j], s, dtype)
                                a = fma_ref(Gk[nn + j * nu + e], u[j], a, dtype)
                            for j in range(nx):
                                s = fma_ref(Ck[nn + e * nx + j], nl[j], s, dtype)
                                t = fma_ref(Ck[nn + e * nx + j], nl[j], t, dtype)
                        if box:
                            uu = fma_ref(T(1.0), yb[k * sv + part * nx + e], T(0.0), dtype)
                        else:
                            rows, eo, ro = (mu, k * se + mx * nx, k * sw + mx) if part else (mx, k * se, k * sw)
                            uu = T(0.0)
                            for i in range(rows):
                                uu = fma_ref(Eb[eo + e * rows + i], yb[ro + i], uu, dtype)
                        q.append(fma_ref(r, uu, s, dtype))
                        p.append(fma_ref(r, uu, t, dtype))
                        a_.append(a)
                # dynamics
                for e in range(nx):
                    if k == 0:
                        f.append(T(x[e] - cb[e]))
                        h.append(x[e])
                    if nxt:
                        xn = zb[(k + 1) * sv + e]
                        ff, hh = T(xn - cb[(k + 1) * nx + e]), xn
                        for j in range(nx):
                            ff = fma_ref(Ck[j * nx + e], -x[j], ff, dtype)
                            hh = fma_ref(Ck[j * nx + e], -x[j], hh, dtype)
                        for j in range(nu):
                            ff = fma_ref(Ck[nn + j * nx + e], -u[j], ff, dtype)
                            hh = fma_ref(Ck[nn + j * nx + e], -u[j], hh, dtype)
                        f.append(ff)
                        h.append(hh)
                # rows
                if box:
                    v += list(zb[k * sv:k * sv + (sv if nxt else nx)])
                else:
                    for part, rows, cols in ((0, mx, nx),) + (((1, mu, nu),) if nxt else ()):
                        eo, co = (k * se + mx * nx, k * sv + nx) if part else (k * se, k * sv)
                        for i in range(rows):
                            acc = T(0.0)
                            for j in range(cols):
                                acc = fma_ref(Eb[eo + j * rows + i], zb[co + j], acc, dtype)
                            v.append(acc)
            assert len(v) == wb.size and len(q) == gb.size and len(f) == cb.size
            v = np.asarray(v, dtype)
            d = v - wb
            assert d.dtype == dtype
            o = (_norm(q, dtype), _norm(f, dtype), _norm(d, dtype), _norm(a_ + p + list(gb), dtype), _norm(h + list(cb), dtype),
                 _norm(list(v) + list(wb), dtype))
            opt[b] = o
            thr = [fma_ref(T(eps_rel), o[3 + i], T(eps_abs), dtype) for i in range(3)]
            done[b] = 1 if (o[0] <= thr[0] and o[1] <= thr[1] and o[2] <= thr[2]) else 0
    return opt, done


def done_from_opt(opt, eps_abs, eps_rel):
    """The three comparisons recomputed from an opt array [B, 6] of the call's precision."""
    opt = np.asarray(opt)
    T = opt.dtype.type
    out = np.zeros(opt.shape[0], np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, o in enumerate(opt):
            out[b] = all(o[i] <= fma_ref(T(eps_rel), o[3 + i], T(eps_abs), opt.dtype) for i in range(3))
    return out


def knot_chunk(nx, nu, mx, mu, box=False):
    """The knots the kernel stages at a time (admm_optimality_knot_chunk in csrc/admm_optimality.hip): what fits 4096 elements,
    1 .. 64."""
    if box:
        mx, mu = nx, nu
    per = nx * nx + nu * nu + nx * (nx + nu) + (0 if box else mx * nx + mu * nu) + 2 * nx + nu + mx + mu
    return max(1, min(64, 4096 // per))


def random_inputs(nx, nu, mx, mu, N, B, seed, dtype, box=False):
    """Random fp32 numbers (held in `dtype`) in the packed layouts; some entries of y are zeros of both signs.  E is None for the
    box (mx, mu ignored).  Everything is of order 1, so every residual is about its scale: eps_abs = eps_rel = 1 gives flags of both
    values over a handful of problems."""
    rng = np.random.default_rng(seed)
    if box:
        mx, mu = nx, nu
    nz, nw, ne, ng = lr.sizes(nx, nu, mx, mu, N)

    def rnd(*shape):
        return rng.standard_normal(shape).astype(np.float32).astype(dtype)
    G, C, g, c, E = rnd(B, ng), rnd(B, nx * (nx + nu) * (N - 1)), rnd(B, nz), rnd(B, nx * N), rnd(B, ne)
    z, lam, w, y = rnd(B, nz), rnd(B, nx * N), rnd(B, nw), rnd(B, nw)
    y[rng.random((B, nw)) < 0.25] = 0.0
    y[0, 0] = -0.0
    rho = (np.abs(rnd(B)) + 0.5).astype(dtype)
    return dict(G=G, C=C, g=g, c=c, E=None if box else E, rho=rho, z=z, lam=lam, w=w, y=y)


def box_as_rows(nx, nu, N, B, dtype):
    """The packed identity E [B, ne] that makes the rows form the box form."""
    return np.tile(lr.identity_E(nx, nu, N, dtype), (B, 1))


def opt_dense(Gd, Cd, Ed, g, c, rho, z, lam, w, y, dtype=F64, want_mag=True):
    """((r_s, r_e, r_r, n_s, n_e, n_r), (mag_s, mag_e, mag_r)) for ONE problem with dense Gd [nz, nz], Cd [nl, nz], Ed [nw, nz] or
    None (the box), numpy operations of `dtype`.  mag: per quantity the largest sum of |terms| over its entries."""
    dtype = np.dtype(dtype)
    Gd, Cd, g, c, z, lam, w, y = (np.asarray(a, dtype) for a in (Gd, Cd, g, c, z, lam, w, y))
    Ed = np.eye(z.size, dtype=dtype) if Ed is None else np.asarray(Ed, dtype)
    rho = dtype.type(rho)
    with np.errstate(invalid="ignore", over="ignore"):
        a, p, h, v = Gd @ z, Cd.T @ lam + rho * (Ed.T @ y), Cd @ z, Ed @ z
        q, f, d = a + g + p, h - c, v - w
        six = (np.abs(q).max(), np.abs(f).max(), np.abs(d).max(), max(np.abs(a).max(), np.abs(p).max(), np.abs(g).max()),
               max(np.abs(h).max(), np.abs(c).max()), max(np.abs(v).max(), np.abs(w).max()))
        if not want_mag:
            return six, None
        mag = ((np.abs(Gd) @ np.abs(z) + np.abs(g) + np.abs(Cd).T @ np.abs(lam) + np.abs(rho) * (np.abs(Ed).T @ np.abs(y))).max(),
               (np.abs(Cd) @ np.abs(z) + np.abs(c)).max(), (np.abs(Ed) @ np.abs(z) + np.abs(w)).max())
    return six, mag


def chain_bound(length, dtype, mag):
    """(len + 2) u sum |terms|: what an fma chain of `length` terms behind a rounded seed can be off by in `dtype`."""
    return (length + 2) * UNIT[np.dtype(dtype)] * mag


def chain_lengths(nx, nu, mx, mu):
    """The longest chain behind each of the three residuals: Q (or R) + C' + E' + the line of q; [A | B]; a row of E + the line of d."""
    return 2 * nx + max(mx, mu) + 1, nx + nu, max(nx, nu) + 1


def loop(dtype, Gd, Cd, Ed, g, c, lo, hi, rho, K):
    """K hard iterations for one problem from w0 = y0 = 0 with every array and operation of `dtype` (Ed None: the box), as
    admm_infeas_ref.loop.  Returns [K, 6]: opt_dense in `dtype` at the iterate (z, lambda, w+, y+) of iteration k at position k - 1."""
    dtype = np.dtype(dtype)
    Gd64, Cd64 = np.asarray(Gd, F64), np.asarray(Cd, F64)
    nz, nl = Gd64.shape[0], Cd64.shape[0]
    Kkt = np.zeros((nz + nl, nz + nl))
    Kkt[:nz, :nz] = Gd64 + rho * (np.eye(nz) if Ed is None else np.asarray(Ed, F64).T @ np.asarray(Ed, F64))
    Kkt[:nz, nz:], Kkt[nz:, :nz] = Cd64.T, Cd64
    Kinv = np.linalg.inv(Kkt).astype(dtype)
    E = None if Ed is None else np.asarray(Ed, dtype)
    fwd = (lambda a: a) if E is None else (lambda a: E @ a)
    bwd = (lambda a: a) if E is None else (lambda a: E.T @ a)
    g, c, lo, hi = (np.asarray(a, dtype) for a in (g, c, lo, hi))
    r = dtype.type(rho)
    nw = nz if E is None else E.shape[0]
    w, y = clip(np.zeros(nw, dtype), lo, hi), np.zeros(nw, dtype)
    gt = g - r * bwd(w - y)
    out = []
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, c])
        z, lam = sol[:nz], sol[nz:]
        s = fwd(z) + y
        w = clip(s, lo, hi)
        y = s - w
        gt = g - r * bwd(w - y)
        assert z.dtype == dtype and y.dtype == dtype
        out.append(opt_dense(Gd, Cd, Ed, g, c, rho, z, lam, w, y, dtype, want_mag=False)[0])
    return np.array(out, F64)


def windows(hist, eps):
    """(k_lo, k_hi) of a history [K, 6] at eps_abs = eps_rel = eps, 1-based, None where the level is never reached: the first
    iteration at which all three residuals are under 2 x (k_lo) and under 0.5 x (k_hi) their thresholds eps + eps n."""
    thr = eps + eps * hist[:, 3:]
    out = []
    for factor in (2.0, 0.5):
        ok = (hist[:, :3] < factor * thr).all(axis=1)
        out.append(int(np.argmax(ok)) + 1 if ok.any() else None)
    return tuple(out)


def first_done(done):
    """The iteration (1-based) of the first set flag of a sequence, or None."""
    done = np.asarray(done).astype(bool)
    return int(np.argmax(done)) + 1 if done.any() else None


@functools.lru_cache(maxsize=None)
def history(index, dtype_name, K=K_MAX):
    """loop() on problem `index` of admm_infeas_ref.feasible_problems(), cached."""
    _, Gd, Cd, Ed, g, c, lo, hi, rho = ir.feasible_problems()[index]
    return loop(np.dtype(dtype_name), Gd, Cd, Ed, g, c, lo, hi, rho, K)
