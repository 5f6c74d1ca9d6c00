"""References for the mixed-precision KKT refinement (gbdpcg_kkt_defect_mixed, gbdpcg_kkt_refine_apply; not a test module).

defect_ref        r_s = G z + g + C' lambda and r_f = C z - c of one problem, every entry the fp64 fma chain the device defines
                  (the head of csrc/schur_residual.hip), each fma the exact rational value rounded once (admm_lin_ref.fma_ref)
max_bits          the NaN-propagating maximum of magnitudes: over the bit patterns of |entry|
exponent          e = 0 where m = max(m_s, m_f) is 0, Inf or NaN, else -ilogb(m) clamped to [-126, 127]
scaled_f32        fl32(v) * 2^e: one rounding to fp32 (admm_lin_ref.round_to), then an fp32 product
defect_mixed_ref  all outputs of the defect launch for one problem
apply_ref         z + ldexp((double)dz, -e)
magnitudes, floor the magnitudes the error of an fp64 residual scales with (evaluate() of tests/test_gpu_kkt_residual.py) and the
                  bounds built on them: a point inside them cannot be told from the exact solution by an fp64 residual
emulate           the refinement in numpy: fp32 G^-1 and S, fp32 dense solve of S, fp64 defect, fp64 accumulation from zero
"""
import math
from fractions import Fraction

import numpy as np

from admm_lin_ref import fma_ref, round_to
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53


def defect_ref(nx, nu, N, G, C, g, c, z, lam):
    """(r_s [nz], r_f [nx N]) of one problem in fp64, bit for bit what the device computes."""
    G, C, g, c, z, lam = (np.asarray(a, F64) for a in (G, C, g, c, z, lam))
    sg, sc, sv, nn = nx * nx + nu * nu, nx * nx + nx * nu, nx + nu, nx * nx
    rs, rf = np.zeros(sv * N - nu), np.zeros(nx * N)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(N):
            nxt = k + 1 < N
            Gk, Ck = G[k * sg:], C[k * sc:]
            x, lk = z[k * sv:k * sv + nx], lam[k * nx:(k + 1) * nx]
            u = z[k * sv + nx:(k + 1) * sv] if nxt else None
            nl = -lam[(k + 1) * nx:(k + 2) * nx] if nxt else None
            for r in range(nx):
                s = F64(g[k * sv + r] + lk[r])
                for q in range(nx):
                    s = fma_ref(Gk[q * nx + r], x[q], s, F64)
                if nxt:
                    for q in range(nx):
                        s = fma_ref(Ck[r * nx + q], nl[q], s, F64)
                rs[k * sv + r] = s
                if k == 0:
                    rf[r] = x[r] - c[r]
                if nxt:
                    f = F64(z[(k + 1) * sv + r] - c[(k + 1) * nx + r])
                    for q in range(nx):
                        f = fma_ref(Ck[q * nx + r], -x[q], f, F64)
                    for q in range(nu):
                        f = fma_ref(Ck[nn + q * nx + r], -u[q], f, F64)
                    rf[(k + 1) * nx + r] = f
            if nxt:
                for r in range(nu):
                    s = F64(g[k * sv + nx + r])
                    for q in range(nu):
                        s = fma_ref(Gk[nn + q * nu + r], u[q], s, F64)
                    for q in range(nx):
                        s = fma_ref(Ck[nn + r * nx + q], nl[q], s, F64)
                    rs[k * sv + nx + r] = s
    return rs, rf


def max_bits(v):
    """max |v| over bit patterns (an fp64 array, not empty): Inf above the finite numbers, every NaN above Inf."""
    b = np.ascontiguousarray(np.asarray(v, F64)).view(np.uint64) & np.uint64(0x7fffffffffffffff)
    return b.max().reshape(1).view(F64)[0]


def exponent(ms, mf):
    m = max_bits(np.array([ms, mf], F64))
    if m == 0 or not np.isfinite(m):
        return 0
    ilogb = math.frexp(float(m))[1] - 1          # m = f 2^x with f in [0.5, 1): ilogb = x - 1, subnormals included
    return int(min(127, max(-126, -ilogb)))


def scaled_f32(v, e):
    """fl32(v) * 2^e elementwise: the rounding by round_to, the product in fp32 (exact unless subnormal or overflowing)."""
    v = np.asarray(v, F64)
    out = np.empty(v.shape, F32)
    for i, x in enumerate(v.reshape(-1)):
        out.reshape(-1)[i] = round_to(Fraction(float(x)), F32) if np.isfinite(x) and x != 0 else F32(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return out * F32(2.0 ** e)


def defect_mixed_ref(nx, nu, N, G, C, g, c, z, lam):
    """(rg fp32, rc fp32, e, (m_s, m_f)) of one problem."""
    rs, rf = defect_ref(nx, nu, N, G, C, g, c, z, lam)
    ms, mf = max_bits(rs), max_bits(rf)
    e = exponent(ms, mf)
    return scaled_f32(rs, e), scaled_f32(-rf, e), e, (ms, mf)


def apply_ref(x, dx, e):
    return np.asarray(x, F64) + np.ldexp(np.asarray(dx, F32).astype(F64), -int(e))


def magnitudes(Gd, Cd, g, c, z, lam):
    aC = np.abs(Cd)
    return (np.abs(Gd) @ np.abs(z) + np.abs(g) + aC.T @ np.abs(lam)).max(), (aC @ np.abs(z) + np.abs(c)).max()


def floor(nx, nu, mag):
    """The derived error of evaluating the two norms in fp64 at all (the dot-product bound of tests/test_gpu_kkt_residual.py)."""
    return (2 * nx + 2) * U64 * mag[0], (nx + nu + 2) * U64 * mag[1]


def emulate(nx, nu, N, seed, steps, inner_error=0.0):
    """Refinement of one problem of so.gen(dtype=float64, cond=30) from z = lambda = 0.  Returns per step i = 0 .. steps the pair
    (m_s / bound_s, m_f / bound_f) of the point after i steps.  inner_error: relative perturbation of the multiplier correction,
    what a loose PCG tolerance leaves."""
    d = so.gen(nx, nu, N, seed=seed, batch=1, dtype=F64, cond=30.0)
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0])
    G32, C32 = Gd.astype(F32), Cd.astype(F32)
    Gi32 = np.linalg.inv(G32).astype(F32)
    S32 = (C32 @ Gi32 @ C32.T).astype(F32)
    rng = np.random.default_rng(seed + 7)
    z, lam = np.zeros(Gd.shape[0]), np.zeros(Cd.shape[0])
    out = []
    for i in range(steps + 1):
        rs, rf = Gd @ z + g + Cd.T @ lam, Cd @ z - c
        bs, bf = floor(nx, nu, magnitudes(Gd, Cd, g, c, z, lam))
        out.append((np.abs(rs).max() / bs, np.abs(rf).max() / bf))
        if i == steps:
            break
        e = exponent(np.abs(rs).max(), np.abs(rf).max())
        rg, rc = rs.astype(F32) * F32(2.0 ** e), (-rf).astype(F32) * F32(2.0 ** e)
        gamma = -(rc + C32 @ (Gi32 @ rg))
        dl = np.linalg.solve(S32, gamma).astype(F32)
        if inner_error:
            dl = (dl * (1 + inner_error * rng.standard_normal(dl.shape))).astype(F32)
        dz = -(Gi32 @ (rg + C32.T @ dl))
        z, lam = apply_ref(z, dz, e), apply_ref(lam, dl, e)
    return out
