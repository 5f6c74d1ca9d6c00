"""CPU: the gradient formulas of the KKT backward pass (tests/kkt_grad_ref.py, the twin the device tests compare with) against
torch.autograd through torch.linalg.solve of the same dense system in fp64.  The dense matrix is built in torch from the packed
blocks, G entering as 1/2 (G + G'), so autograd differentiates exactly the map the library implements; l is a random linear
functional of (z, lambda).  This is the test that pins signs and factors of dl/dG, dl/dC, dl/dg, dl/dc, dl/drho and of the batch
sum of the shared-matrix form.

Tolerance: relative max-norm per tensor.  Both sides are fp64 solves of the same system, so they differ by conditioning times
roundoff.  Measured over kkt_grad_ref.SHAPES with so.gen at its default conditioning, both cases, every problem and tensor, the
shared sums included: largest error 7.9e-15 (TOL is 100 x that, and may never exceed 1e-6).  A tensor whose exact value is
zero is measured against the scale of the pairs it is computed from (relerr, floors)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import schur_oracle as so  # noqa: E402
import kkt_grad_ref as kgr  # noqa: E402

MEASURED = 7.9e-15
TOL = 100 * MEASURED
assert TOL <= 1e-6


def index_maps(nx, nu, N):
    """Where each packed entry of G and C sits in the dense matrices: so.dense_kkt on arrays that hold their own indices."""
    sz = so.sizes(nx, nu, N)
    Gd, Cd, _, _ = so.dense_kkt(nx, nu, N, np.arange(1, sz["G"] + 1, dtype=np.float64), np.arange(2, sz["C"] + 2, dtype=np.float64),
                                np.zeros(sz["g"]), np.zeros(sz["c"]))
    gm, cm = Gd > 0, Cd < -1.5        # the identity blocks of C hold +1; the packed entries enter as -A_k, -B_k
    return (torch.from_numpy(gm), torch.from_numpy((Gd[gm] - 1).astype(np.int64)), torch.from_numpy(cm),
            torch.from_numpy((-Cd[cm] - 2).astype(np.int64)), torch.from_numpy(np.where(Cd > 0.5, 1.0, 0.0)))


def autograd_grads(nx, nu, N, maps, G, C, gs, cs, rhos, gzs, glams):
    """dl/d(G, C, g_b, c_b, rho_b) of l = sum_b gz_b' z_b + glam_b' lambda_b by torch.autograd; G and C are shared by the problems
    of the lists (one problem: the per-problem gradients)."""
    gm, gi, cm, ci, eye = maps
    G, C = torch.tensor(G, requires_grad=True), torch.tensor(C, requires_grad=True)
    gs, cs = [torch.tensor(a, requires_grad=True) for a in gs], [torch.tensor(a, requires_grad=True) for a in cs]
    rhos = [torch.tensor(float(r), dtype=torch.float64, requires_grad=True) for r in rhos]
    nz, nl = gs[0].numel(), cs[0].numel()
    Gd = torch.zeros(nz, nz, dtype=torch.float64)
    Gd[gm] = G[gi]
    Gd = 0.5 * (Gd + Gd.T)
    Cd = eye.clone()
    Cd[cm] = -C[ci]
    loss = 0.0
    for g, c, rho, gz, glam in zip(gs, cs, rhos, gzs, glams):
        K = torch.cat([torch.cat([Gd + rho * torch.eye(nz, dtype=torch.float64), Cd.T], 1),
                       torch.cat([Cd, torch.zeros(nl, nl, dtype=torch.float64)], 1)], 0)
        sol = torch.linalg.solve(K, torch.cat([-g, c]))
        loss = loss + torch.from_numpy(gz) @ sol[:nz] + torch.from_numpy(glam) @ sol[nz:]
    loss.backward()
    zero_c = torch.zeros_like(C)
    return (G.grad.numpy(), (C.grad if C.grad is not None else zero_c).numpy(), [g.grad.numpy() for g in gs],
            [c.grad.numpy() for c in cs], [float(r.grad) for r in rhos])


def relerr(a, b, floor=0.0):
    """Relative max-norm of a - b.  floor: the scale of the quantities the tensor is computed from, for a tensor whose exact value
    is zero (N = 1 with dl/dlambda = 0: x_0 = c_0 whatever g is, so a_z = 0 and both sides hold roundoff of the size of a_lambda)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-300))


def floors(ref):
    """(for dl/dg and dl/dc, for dl/dG, dl/dC and dl/drho): the largest entry of the adjoint pair, and that times the largest
    entry of the forward pair."""
    a = max(np.abs(ref["az"]).max(), np.abs(ref["alam"]).max())
    return a, a * max(np.abs(ref["z"]).max(), np.abs(ref["lam"]).max())


def upstream(rng, nz, nl, case):
    return rng.standard_normal(nz), (np.zeros(nl) if case == "glam0" else rng.standard_normal(nl))


@pytest.mark.parametrize("case", ["glam", "glam0"])
@pytest.mark.parametrize("nx,nu,N,B", kgr.SHAPES)
def test_formulas_against_autograd(nx, nu, N, B, case):
    """Per problem: every gradient of the twin against autograd.  "glam": random dl/dlambda and rho > 0; "glam0": l does not depend
    on lambda, rho = 0."""
    d = so.gen(nx, nu, N, seed=700 + nx + N, batch=B)
    rng = np.random.default_rng(nx * 1000 + N)
    maps = index_maps(nx, nu, N)
    worst = 0.0
    for b in range(B):
        gz, glam = upstream(rng, d["g"].shape[1], d["c"].shape[1], case)
        rho = 0.0 if case == "glam0" else float(rng.uniform(0.1, 1.0))
        ref = kgr.reference(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b], gz, glam, rho)
        aG, aC, ag, ac, arho = autograd_grads(nx, nu, N, maps, d["G"][b], d["C"][b], [d["g"][b]], [d["c"][b]], [rho], [gz], [glam])
        fa, faw = floors(ref)
        errs = {"G": relerr(ref["gG"], aG, faw), "C": relerr(ref["gC"], aC, faw), "g": relerr(ref["gg"], ag[0], fa),
                "c": relerr(ref["gc"], ac[0], fa), "rho": relerr([ref["grho"]], [arho[0]], faw)}
        print(f"({nx},{nu},{N}) problem {b} {case}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        worst = max(worst, *errs.values())
        assert all(v <= TOL for v in errs.values()), errs
    print(f"({nx},{nu},{N},{B}) {case}: worst {worst:.3e}")


@pytest.mark.parametrize("nx,nu,N,B", [s for s in kgr.SHAPES if s[2] <= 33] + [(2, 1, 3, 7), (5, 2, 9, 3)])
def test_shared_gradients_are_the_batch_sum(nx, nu, N, B):
    """One G and C for B problems: autograd's gradient in the single matrices is the sum over the batch of the per-problem
    formulas; the vector gradients stay per problem."""
    d = so.gen(nx, nu, N, seed=900 + nx + N, batch=B)
    rng = np.random.default_rng(N * 100 + B)
    ups = [upstream(rng, d["g"].shape[1], d["c"].shape[1], "glam") for _ in range(B)]
    refs = [kgr.reference(nx, nu, N, d["G"][0], d["C"][0], d["g"][b], d["c"][b], *ups[b]) for b in range(B)]
    aG, aC, ag, ac, _ = autograd_grads(nx, nu, N, index_maps(nx, nu, N), d["G"][0], d["C"][0], list(d["g"]), list(d["c"]), [0.0] * B,
                                       [u[0] for u in ups], [u[1] for u in ups])
    fl = [floors(r) for r in refs]
    faw = max(f[1] for f in fl)
    errs = [relerr(sum(r["gG"] for r in refs), aG, faw), relerr(sum(r["gC"] for r in refs), aC, faw)]
    errs += [relerr(refs[b]["gg"], ag[b], fl[b][0]) for b in range(B)] + [relerr(refs[b]["gc"], ac[b], fl[b][0]) for b in range(B)]
    print(f"shared ({nx},{nu},{N},{B}): worst {max(errs):.3e}")
    assert max(errs) <= TOL, errs


def test_twin_operation_order_and_symmetry():
    """block_grads in fp32 is two rounded products, one rounded add and an exact scaling, entry by entry, and gQ_k, gR_k are
    bit-symmetric."""
    nx, nu, N = 5, 2, 4
    rng = np.random.default_rng(5)
    sz = so.sizes(nx, nu, N)
    z, az = rng.standard_normal(sz["g"]).astype(np.float32), rng.standard_normal(sz["g"]).astype(np.float32)
    lam, alam = rng.standard_normal(sz["c"]).astype(np.float32), rng.standard_normal(sz["c"]).astype(np.float32)
    gG, gC = kgr.block_grads(nx, nu, N, z, lam, az, alam, np.float32)
    assert gG.dtype == np.float32 and gC.dtype == np.float32 and gG.size == sz["G"] and gC.size == sz["C"]
    sv, sg, sc = nx + nu, nx * nx + nu * nu, nx * nx + nx * nu
    k, i, j = 2, 3, 1
    x, ax = z[k * sv:k * sv + nx], az[k * sv:k * sv + nx]
    want = np.float32(0.5) * (np.float32(ax[i] * x[j]) + np.float32(x[i] * ax[j]))
    assert gG[k * sg + j * nx + i] == want
    j = nx + 1   # a column of B_k: u_k,1
    want = -(np.float32(alam[(k + 1) * nx + i] * z[k * sv + j]) + np.float32(lam[(k + 1) * nx + i] * az[k * sv + j]))
    assert gC[k * sc + j * nx + i] == want
    for k in range(N):
        Q = gG[k * sg:k * sg + nx * nx].reshape(nx, nx)
        assert np.array_equal(Q, Q.T)
        if k < N - 1:
            R = gG[k * sg + nx * nx:(k + 1) * sg].reshape(nu, nu)
            assert np.array_equal(R, R.T)
