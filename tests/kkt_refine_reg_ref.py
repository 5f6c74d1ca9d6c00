"""References for the regularised mixed-precision KKT refinement (gbdpcg_kkt_defect_mixed_reg, gbdpcg_kkt_refine_step_reg; not a
test module).  Built on tests/kkt_refine_ref.py.

regularised           the packed G with np.float64(d + rho) on the diagonal of every Q_k and R_k present in the layout: one fp64
                      addition in numpy is the device's fl(d + rho_b)
zero_inputs           the packed G with every R_k set to zero: a cost that is only positive semi-definite (unpenalised inputs)
defect_mixed_reg_ref  kkt_refine_ref.defect_mixed_ref on regularised(G): all outputs of the _reg defect launch for one problem
emulate_reg           kkt_refine_ref.emulate for the regularised system: the fp32 side is formed from fl32(G) + fl32(rho) (what
                      gbdpcg_kkt_step_reg_f32 sees behind gbdpcg_demote_f32), the fp64 defect is that of G + rho I, and the floor is
                      always that of the REGULARISED system.  plain_defect: the defect without rho (gbdpcg_kkt_refine_step on a
                      regularised factorisation), measured against the same floor -- the failure the _reg form removes.
"""
import numpy as np

import kkt_refine_ref as ref
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
# Steps of emulate_reg to the floor with inner_error = 1e-3 (tests/test_kkt_refine_reg_reference.py asserts it).  A step contracts
# the error by the accuracy of the correction, 1e-3 here (the fp32 factorisation is better: cond(G + rho I) u32 <= 241 * 6e-8);
# the start is 1 / ((2 nx + 2) u64) ~ 3e14 floors away: five contractions by 1e-3 and one for the noise in them.  The GPU test
# allows twice this, the rule of tests/test_gpu_kkt_refine.py.
N0 = 6
RHOS = (2.0 ** -3, 0.5, 1.0)


def _diagonals(nx, nu, N):
    """Indices into one problem's packed G of the diagonal entries of Q_0, R_0, Q_1, ..., Q_{N-1} (column-major blocks)."""
    sg, nn = nx * nx + nu * nu, nx * nx
    idx = []
    for k in range(N):
        idx += [k * sg + i * (nx + 1) for i in range(nx)]
        if k + 1 < N:
            idx += [k * sg + nn + i * (nu + 1) for i in range(nu)]
    return np.array(idx)


def regularised(nx, nu, N, G, rho):
    out = np.array(G, F64)
    idx = _diagonals(nx, nu, N)
    with np.errstate(invalid="ignore", over="ignore"):
        out[idx] = out[idx] + F64(rho)
    return out


def zero_inputs(nx, nu, N, G):
    out = np.array(G, F64)
    sg, nn = nx * nx + nu * nu, nx * nx
    for k in range(N - 1):
        out[k * sg + nn:(k + 1) * sg] = 0.0
    return out


def defect_mixed_reg_ref(nx, nu, N, G, C, g, c, rho, z, lam):
    """(rg fp32, rc fp32, e, (m_s, m_f)) of one problem of the regularised system."""
    return ref.defect_mixed_ref(nx, nu, N, regularised(nx, nu, N, G, rho), C, g, c, z, lam)


def emulate_reg(nx, nu, N, seed, steps, rho, inner_error=0.0, zero_R=False, plain_defect=False):
    """Refinement of one problem of so.gen(dtype=float64, cond=30) from z = lambda = 0 towards the solution of the system with
    G + rho I.  Returns per step i = 0 .. steps the pair (m_s / bound_s, m_f / bound_f) of the point after i steps, norms and bounds
    of the regularised system."""
    d = so.gen(nx, nu, N, seed=seed, batch=1, dtype=F64, cond=30.0)
    G = zero_inputs(nx, nu, N, d["G"][0]) if zero_R else d["G"][0]
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, G, d["C"][0], d["g"][0], d["c"][0])
    Gr = so.dense_kkt(nx, nu, N, regularised(nx, nu, N, G, rho), d["C"][0], d["g"][0], d["c"][0])[0]
    G32, C32 = Gd.astype(F32), Cd.astype(F32)
    G32[np.diag_indices_from(G32)] += F32(rho)            # fl32(fl32(d) + fl32(rho))
    Gi32 = np.linalg.inv(G32).astype(F32)
    S32 = (C32 @ Gi32 @ C32.T).astype(F32)
    Gdef = Gd if plain_defect else Gr
    rng = np.random.default_rng(seed + 7)
    z, lam = np.zeros(Gd.shape[0]), np.zeros(Cd.shape[0])
    out = []
    for i in range(steps + 1):
        rs, rf = Gr @ z + g + Cd.T @ lam, Cd @ z - c
        bs, bf = ref.floor(nx, nu, ref.magnitudes(Gr, Cd, g, c, z, lam))
        out.append((np.abs(rs).max() / bs, np.abs(rf).max() / bf))
        if i == steps:
            break
        ds = Gdef @ z + g + Cd.T @ lam                    # the defect the step is driven by
        e = ref.exponent(np.abs(ds).max(), np.abs(rf).max())
        rg, rc = ds.astype(F32) * F32(2.0 ** e), (-rf).astype(F32) * F32(2.0 ** e)
        gamma = -(rc + C32 @ (Gi32 @ rg))
        dl = np.linalg.solve(S32, gamma).astype(F32)
        if inner_error:
            dl = (dl * (1 + inner_error * rng.standard_normal(dl.shape))).astype(F32)
        dz = -(Gi32 @ (rg + C32.T @ dl))
        z, lam = ref.apply_ref(z, dz, e), ref.apply_ref(lam, dl, e)
    return out
