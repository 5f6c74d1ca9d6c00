"""References for the KKT backward pass (gbdpcg_kkt_grad_*, gbdpcg_kkt_backward_*, gbd_pcg_amd.autograd; not a test module).

Forward: G z + g + C' lambda = 0, C z = c.  For a scalar l with gz = dl/dz, glam = dl/dlambda the adjoint pair (a_z, a_lambda)
solves the same KKT matrix with the right-hand side (-gz, -glam), and with z = (x_k, u_k), a_z = (ax_k, au_k):
    dl/dg = a_z      dl/dc = -a_lambda      dl/drho = a_z' z
    dl/dQ_k(i,j) = 1/2 (ax_i x_j + x_i ax_j)                       dl/dR_k likewise with u
    dl/d[A_k | B_k](i,j) = -(a_lambda,k+1,i z_k,j + lambda_k+1,i a_z,k,j)      (j over (x_k, u_k))

block_grads   the outer-product formulas in a given precision, in the operation order of the kernels: two rounded products, one
              rounded add, an exact scaling -- what the device must reproduce bit for bit
block_bound   sum of |a_i||z_j| + |z_i||a_j| per entry (the magnitude the summation bound of the shared form is stated in)
adjoint       the dense fp64 adjoint solve through oracle.schur_oracle.dense_kkt
reference     everything for one problem in fp64: z, lam, az, alam and the gradients in G, C, g, c, rho
"""
import numpy as np

from oracle import schur_oracle as so

SHAPES = [(2, 1, 3, 2), (1, 1, 4, 1), (3, 3, 2, 1), (4, 6, 3, 2), (5, 2, 9, 2), (14, 7, 1, 2), (14, 7, 2, 1), (12, 4, 33, 2),
          (14, 7, 128, 3)]   # nx, nu, N, batch


def _blocks(nx, nu, N, z, lam, az, alam, dtype, combine):
    """Packed (gG, gC) of one problem; combine(p, q, r, s) gives the entry from the outer-product operands p_i q_j and r_i s_j."""
    z, lam, az, alam = (np.asarray(a, dtype) for a in (z, lam, az, alam))
    sv = nx + nu
    gG, gC = [], []
    for k in range(N):
        x, ax = z[k * sv:k * sv + nx], az[k * sv:k * sv + nx]
        gG.append(combine(ax, x, x, ax, "G").reshape(-1, order="F"))
        if k < N - 1:
            u, au = z[k * sv + nx:(k + 1) * sv], az[k * sv + nx:(k + 1) * sv]
            gG.append(combine(au, u, u, au, "G").reshape(-1, order="F"))
            zk, azk = z[k * sv:(k + 1) * sv], az[k * sv:(k + 1) * sv]
            l, al = lam[(k + 1) * nx:(k + 2) * nx], alam[(k + 1) * nx:(k + 2) * nx]
            gC.append(combine(al, zk, l, azk, "C").reshape(-1, order="F"))
    return np.concatenate(gG), (np.concatenate(gC) if gC else np.zeros(0, dtype))


def block_grads(nx, nu, N, z, lam, az, alam, dtype=np.float64):
    """Every numpy operation below is one IEEE operation per entry in `dtype`; * 0.5 and the negation are exact."""
    def combine(p, q, r, s, which):
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.multiply.outer(p, q) + np.multiply.outer(r, s)
            out = t * dtype(0.5) if which == "G" else -t
        assert out.dtype == np.dtype(dtype)
        return out
    return _blocks(nx, nu, N, z, lam, az, alam, dtype, combine)


def block_bound(nx, nu, N, z, lam, az, alam):
    """|p_i||q_j| + |r_i||s_j| per entry, fp64, in the layouts of gG and gC."""
    def combine(p, q, r, s, which):
        return np.multiply.outer(np.abs(p), np.abs(q)) + np.multiply.outer(np.abs(r), np.abs(s))
    return _blocks(nx, nu, N, z, lam, az, alam, np.float64, combine)


def kkt_matrix(nx, nu, N, G, C, rho=0.0):
    Gd, Cd, _, _ = so.dense_kkt(nx, nu, N, G, C, np.zeros(so.sizes(nx, nu, N)["g"]), np.zeros(nx * N))
    nz, nl = Gd.shape[0], Cd.shape[0]
    K = np.zeros((nz + nl, nz + nl))
    K[:nz, :nz] = Gd + rho * np.eye(nz)
    K[:nz, nz:] = Cd.T
    K[nz:, :nz] = Cd
    return K, nz


def adjoint(nx, nu, N, G, C, gz, glam, rho=0.0):
    """(a_z, a_lambda): [G + rho I, C'; C, 0] (a_z, a_lambda) = (-gz, -glam), dense, fp64."""
    K, nz = kkt_matrix(nx, nu, N, G, C, rho)
    sol = np.linalg.solve(K, -np.concatenate([np.asarray(gz, np.float64), np.asarray(glam, np.float64)]))
    return sol[:nz], sol[nz:]


def reference(nx, nu, N, G, C, g, c, gz, glam, rho=0.0, quad=0.0):
    """One problem, fp64: the forward point, the adjoint pair and every gradient of l = gz' z + glam' lambda + quad/2 ||z||^2."""
    from scipy.linalg import lu_factor, lu_solve
    K, nz = kkt_matrix(nx, nu, N, G, C, rho)
    lu = lu_factor(K)      # one factorisation for the forward and the adjoint right-hand side
    sol = lu_solve(lu, np.concatenate([-np.asarray(g, np.float64), np.asarray(c, np.float64)]))
    z, lam = sol[:nz], sol[nz:]
    sol = lu_solve(lu, -np.concatenate([np.asarray(gz, np.float64) + quad * z, np.asarray(glam, np.float64)]))
    az, alam = sol[:nz], sol[nz:]
    gG, gC = block_grads(nx, nu, N, z, lam, az, alam)
    return {"z": z, "lam": lam, "az": az, "alam": alam, "gG": gG, "gC": gC, "gg": az, "gc": -alam, "grho": float(az @ z)}
