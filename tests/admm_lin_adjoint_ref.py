"""References for the backward pass of the hard linear-row QP (gbdpcg_admm_lin_adjoint_*, gbdpcg_admm_lin_grad_*,
gbd_pcg_amd.autograd.lin_qp_solve; not a test module).

Forward (tests/admm_lin_ref.py): min 1/2 z'Gz + g'z subject to Cz = c, lo <= Ez <= hi, with G z + g + C' lambda + rho E'y = 0 at the
solution; y_r < 0 where (E z)_r = lo_r, y_r > 0 where (E z)_r = hi_r, exactly 0 elsewhere.  For a scalar l with gz = dl/dz,
glam = dl/dlambda and the active rows A = {r: y_r != 0} the adjoint triple solves
    G a_z + gz + C' a_lambda + E_A' nu = 0,   C a_z = -glam,   (E a_z)_A = 0
-- the rows QP with g := gz, c := -glam and the degenerate rows lo = hi = 0 on A, (-Inf, +Inf) elsewhere -- and with mu = rho y
    dl/dg = a_z   dl/dc = -a_lambda   dl/dlo_r = -nu_r (y_r < 0)   dl/dhi_r = -nu_r (y_r > 0)
    dl/dE(r, j) = mu_r a_z,j + nu_r z_j on A, 0 elsewhere            dl/dG, dl/dC: kkt_grad_ref.block_grads
A weakly active row (on its bound with y_r = 0) counts as free.

degenerate_rows     the explicit bounds the mask stands for (admm_adjoint_ref.degenerate_box over the layout of the rows)
update_ref          the masked update / init as the device defines them, bit for bit (admm_lin_ref.update_ref with the pin)
grad_ref            glo, ghi, gE as the device defines them, bit for bit
adjoint_loop        the adjoint ADMM iteration in fp64 with the dense inverse of the KKT matrix of G + rho E'E
dense_adjoint       the reduced KKT system with the rows of E_A appended to C, plain numpy
active_set_solve    the forward solution for a GIVEN active set, dense (what the central differences perturb)
gradients           every gradient the adjoint triple implies, packed as the device packs them
fixture, forward    the pinned problems and their converged forward loop
"""
import functools

import numpy as np

import admm_adjoint_ref as ar
import admm_lin_ref as lr
import kkt_grad_ref
from admm_adjoint_ref import MARGIN, converged_bound, degenerate_box as degenerate_rows, grad_bounds_ref, pin  # noqa: F401
from oracle import schur_oracle as so


def update_ref(dtype, nx, nu, mx, mu, N, gz, E, yf, rho, az, w, y):
    """The masked update in `dtype` for gz, az [B, nz], E [B, ne], yf, w, y [B, nw], rho [B]; az None: the initialisation (y is
    returned unchanged, res is None).  The lines of admm_lin_ref.update_ref with pin(., yf) where clip(., lo, hi) stands.  Returns
    w+, y+, gt, res [B, 2], every one an array of `dtype` holding the bits the device must give."""
    dtype = np.dtype(dtype)
    gz, E, yf, w, y, rho = (np.asarray(a, dtype) for a in (gz, E, yf, w, y, rho))
    B = gz.shape[0]
    wn, yn, gt = np.empty_like(w), y.copy(), np.empty_like(gz)
    res = None if az is None else np.empty((B, 2), dtype)
    for b in range(B):
        v = np.zeros(w.shape[1], dtype)
        if az is not None:
            zb = np.asarray(az, dtype)[b]
            for m, n, eo, ro, co, _ in lr.blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for r in range(m):
                    v[ro + r] = lr.chain(Eb[:, r], zb[co:co + n], dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            if az is None:
                wn[b] = pin(w[b], yf[b])
                t = wn[b] - y[b]
                d = None
            else:
                s = v + y[b]
                wn[b] = pin(s, yf[b])
                yn[b] = s - wn[b]
                t = wn[b] - yn[b]
                d = wn[b] - w[b]
            assert t.dtype == dtype
            ee = np.zeros(gz.shape[1], dtype)
            for m, n, eo, ro, co, _ in lr.blocks(nx, nu, mx, mu, N):
                Eb = E[b, eo:eo + m * n].reshape(n, m)
                for j in range(n):
                    u = lr.chain(Eb[j], t[ro:ro + m], dtype)
                    gt[b, co + j] = lr.fma_ref(-rho[b], u, gz[b, co + j], dtype)
                    if d is not None:
                        ee[co + j] = lr.chain(Eb[j], d[ro:ro + m], dtype)
            if az is not None:
                res[b, 0], res[b, 1] = lr._norm(v - wn[b]), lr._norm(rho[b] * ee)
    return wn, yn, gt, res


def grad_ref(dtype, nx, nu, mx, mu, N, z, az, yf, ya, rho):
    """(glo, ghi [B, nw], gE [B, ne]) in `dtype`: glo, ghi are grad_bounds_ref over the rows; per entry of a block
    p = ya_r z_j (one product), q = fma(yf_r, az_j, p), gE = yf_r != 0 ? rho q : +0."""
    dtype = np.dtype(dtype)
    z, az, yf, ya, rho = (np.asarray(a, dtype) for a in (z, az, yf, ya, rho))
    B = z.shape[0]
    _, _, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    glo, ghi = grad_bounds_ref(dtype.type, yf, rho, ya)
    gE = np.zeros((B, ne), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for m, n, eo, ro, co, _ in lr.blocks(nx, nu, mx, mu, N):
                for j in range(n):
                    for r in range(m):
                        f = yf[b, ro + r]
                        if f != 0:      # NaN != 0: active
                            p = ya[b, ro + r] * z[b, co + j]
                            q = lr.fma_ref(f, az[b, co + j], p, dtype)
                            gE[b, eo + j * m + r] = rho[b] * q
    return glo, ghi, gE


def kkt_inverse(Gd, Cd, Ed, rho):
    nz, nl = Gd.shape[0], Cd.shape[0]
    K = np.zeros((nz + nl, nz + nl))
    K[:nz, :nz], K[:nz, nz:], K[nz:, :nz] = Gd + rho * (Ed.T @ Ed), Cd.T, Cd
    return np.linalg.inv(K)


def adjoint_loop(Gd, Cd, Ed, gz, nglam, yf, rho, K):
    """K adjoint iterations for one problem in fp64 from wa = ya = 0.  Returns a dict of arrays indexed by iteration 1 .. K at position
    0 .. K-1: az, alam, wa, ya."""
    Gd, Cd, Ed, gz, nglam, yf = (np.asarray(a, np.float64) for a in (Gd, Cd, Ed, gz, nglam, yf))
    nz, nw = Gd.shape[0], Ed.shape[0]
    Kinv = kkt_inverse(Gd, Cd, Ed, rho)
    w, y = pin(np.zeros(nw), yf), np.zeros(nw)
    gt = gz - rho * (Ed.T @ (w - y))
    out = {k: [] for k in ("az", "alam", "wa", "ya")}
    for _ in range(K):
        sol = Kinv @ np.concatenate([-gt, nglam])
        az, alam = sol[:nz], sol[nz:]
        s = Ed @ az + y
        w = pin(s, yf)
        y = s - w
        gt = gz - rho * (Ed.T @ (w - y))
        for k, a in (("az", az), ("alam", alam), ("wa", w), ("ya", y)):
            out[k].append(a.copy())
    return {k: np.array(v) for k, v in out.items()}


def _bordered(Gd, Cd, EA):
    nz, nl, na = Gd.shape[0], Cd.shape[0], EA.shape[0]
    K = np.zeros((nz + nl + na, nz + nl + na))
    K[:nz, :nz], K[:nz, nz:nz + nl], K[nz:nz + nl, :nz] = Gd, Cd.T, Cd
    K[:nz, nz + nl:], K[nz + nl:, :nz] = EA.T, EA
    return K


def dense_adjoint(Gd, Cd, Ed, gz, glam, active):
    """(a_z, a_lambda, nu [nw]): the KKT system with the rows E_A appended to C and a zero right-hand side on them; nu is 0 off A."""
    nz, nl = Gd.shape[0], Cd.shape[0]
    A = np.flatnonzero(active)
    sol = np.linalg.solve(_bordered(Gd, Cd, Ed[A]), -np.concatenate([np.asarray(gz, np.float64), np.asarray(glam, np.float64),
                                                                     np.zeros(A.size)]))
    nu = np.zeros(Ed.shape[0])
    nu[A] = sol[nz + nl:]
    return sol[:nz], sol[nz:nz + nl], nu


def active_set_solve(Gd, Cd, Ed, g, c, lo, hi, at_lo, at_hi):
    """(z, lambda, mu [nw]) with (E z)_r = lo_r on at_lo, hi_r on at_hi and the KKT conditions G z + g + C' lambda + E' mu = 0; mu is
    0 off the set.  The set is optimal iff mu < 0 on at_lo, mu > 0 on at_hi and lo <= E z <= hi."""
    nz, nl = Gd.shape[0], Cd.shape[0]
    active = at_lo | at_hi
    A = np.flatnonzero(active)
    bound = np.where(at_lo, lo, hi)[A]
    sol = np.linalg.solve(_bordered(Gd, Cd, Ed[A]), np.concatenate([-g, c, bound]))
    mu = np.zeros(Ed.shape[0])
    mu[A] = sol[nz + nl:]
    return sol[:nz], sol[nz:nz + nl], mu


def pack_E(nx, nu, mx, mu, N, Ed):
    """A dense [nw, nz] matrix's diagonal blocks in the packed layout of E."""
    _, _, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    E = np.zeros(ne, Ed.dtype)
    for m, n, eo, ro, co, _ in lr.blocks(nx, nu, mx, mu, N):
        E[eo:eo + m * n] = Ed[ro:ro + m, co:co + n].T.reshape(-1)
    return E


def gradients(nx, nu, mx, mu, N, z, lam, mu_rows, az, alam, nu_rows, at_lo, at_hi):
    """mu_rows = rho yf, nu_rows = rho ya (both 0 off the active rows)."""
    gG, gC = kkt_grad_ref.block_grads(nx, nu, N, z, lam, az, alam)
    active = at_lo | at_hi
    dE = np.where(active[:, None], np.outer(mu_rows, az) + np.outer(nu_rows, z), 0.0)
    return {"G": gG, "C": gC, "g": az.copy(), "c": -alam, "E": pack_E(nx, nu, mx, mu, N, dE),
            "lo": np.where(at_lo, -nu_rows, 0.0), "hi": np.where(at_hi, -nu_rows, 0.0)}


# ---- the pinned fixture: the problems of admm_adjoint_ref.FIXTURE_SHAPES with a few rows per block, fp64 arrays holding fp32 numbers
FIXTURE_SHAPES = ar.FIXTURE_SHAPES                     # nx, nu, N, batch
FIXTURE_ROWS = {(3, 2, 4, 2): (1, 1), (14, 7, 3, 2): (3, 2)}     # mx, mu ((3,2,4) has 6 free directions behind its dynamics: 3 active rows fit)
FIXTURE_RHO = ar.FIXTURE_RHO
FIXTURE_SEED = 219
BOUND_FRACTION = 0.6     # the rows from knot 1 on (and every input row) within +-float32(0.6) max |E z0|, z0 the equality-constrained solution


@functools.lru_cache(maxsize=None)
def fixture(nx, nu, N, B):
    """(d, E [B, ne], lo [B, nw], hi, gz [B, nz], glam [B, nx N]): the problems of admm_adjoint_ref.fixture, random rows of fp32
    numbers, the bounds around E z0 of the equality-constrained solutions (the state rows of knot 0, whose x is given, have none),
    the cotangents of the loss l = gz' z + glam' lambda.  Read-only."""
    mx, mu = FIXTURE_ROWS[(nx, nu, N, B)]
    d = ar.fixture(nx, nu, N, B)[0]
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(FIXTURE_SEED)
    E = rng.standard_normal((B, ne)).astype(np.float32).astype(np.float64)
    lo, hi = np.full((B, nw), -np.inf), np.full((B, nw), np.inf)
    for b in range(B):
        z0 = so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])[0]
        v0 = lr.dense_E(nx, nu, mx, mu, N, E[b]) @ z0
        bound = float(np.float32(BOUND_FRACTION) * np.float32(np.abs(v0[mx:]).max()))
        lo[b, mx:], hi[b, mx:] = -bound, bound
    gz = rng.standard_normal((B, nz)).astype(np.float32).astype(np.float64)
    glam = rng.standard_normal((B, nx * N)).astype(np.float32).astype(np.float64)
    for a in (E, lo, hi, gz, glam):
        a.setflags(write=False)
    return d, E, lo, hi, gz, glam


def is_state_row(nx, nu, mx, mu, N):
    _, nw, _, _ = lr.sizes(nx, nu, mx, mu, N)
    return (np.arange(nw) % (mx + mu)) < mx


@functools.lru_cache(maxsize=None)
def forward(nx, nu, N, B, K):
    """admm_lin_ref.admm_lin on the fixture from w0 = y0 = 0, K iterations, one history per problem."""
    mx, mu = FIXTURE_ROWS[(nx, nu, N, B)]
    d, E, lo, hi, _, _ = fixture(nx, nu, N, B)
    out = []
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = lr.dense_E(nx, nu, mx, mu, N, E[b])
        nw = Ed.shape[0]
        out.append(lr.admm_lin(Gd, Cd, Ed, g, c, lo[b], hi[b], FIXTURE_RHO[b], K, np.zeros(nw), np.zeros(nw)))
    return out


K_REF = 4000                 # the forward loop of reference()
K_FWD, K_ADJ = 600, 600      # the counts at which the fp64 loops have converged on the fixture (tests/test_admm_lin_adjoint_reference.py)


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, K=K_REF):
    """Per problem: the converged forward point (z, lam, w, y of iteration K), its active rows, the dense adjoint and the gradients it
    implies."""
    mx, mu = FIXTURE_ROWS[(nx, nu, N, B)]
    d, E, lo, hi, gz, glam = fixture(nx, nu, N, B)
    out = []
    for b, h in enumerate(forward(nx, nu, N, B, K)):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = lr.dense_E(nx, nu, mx, mu, N, E[b])
        z, lam, w, y = h["z"][-1], h["lam"][-1], h["w"][-1], h["y"][-1]
        at_lo, at_hi = y < 0, y > 0
        az, alam, nu_rows = dense_adjoint(Gd, Cd, Ed, gz[b], glam[b], at_lo | at_hi)
        out.append(dict(Gd=Gd, Cd=Cd, Ed=Ed, g=g, c=c, z=z, lam=lam, w=w, y=y, at_lo=at_lo, at_hi=at_hi, az=az, alam=alam, nu=nu_rows,
                        grads=gradients(nx, nu, mx, mu, N, z, lam, FIXTURE_RHO[b] * y, az, alam, nu_rows, at_lo, at_hi)))
    return out


@functools.lru_cache(maxsize=None)
def loop_reference(nx, nu, N, B):
    """Per problem: what the two fp64 LOOPS give after K_FWD forward and K_ADJ adjoint iterations -- the point, the adjoint triple and
    the gradients -- next to reference(), the dense answer they converge to."""
    mx, mu = FIXTURE_ROWS[(nx, nu, N, B)]
    d, E, lo, hi, gz, glam = fixture(nx, nu, N, B)
    out = []
    for b, (h, r) in enumerate(zip(forward(nx, nu, N, B, K_REF), reference(nx, nu, N, B))):
        z, lam, y = h["z"][K_FWD - 1], h["lam"][K_FWD - 1], h["y"][K_FWD - 1]
        lp = adjoint_loop(r["Gd"], r["Cd"], r["Ed"], gz[b], -glam[b], y, FIXTURE_RHO[b], K_ADJ)
        az, alam, ya = lp["az"][-1], lp["alam"][-1], lp["ya"][-1]
        rho = FIXTURE_RHO[b]
        out.append(dict(z=z, lam=lam, y=y, az=az, alam=alam, ya=ya,
                        grads=gradients(nx, nu, mx, mu, N, z, lam, rho * y, az, alam, rho * ya, y < 0, y > 0)))
    return out
