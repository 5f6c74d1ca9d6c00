"""gbd_pcg_amd.autograd.soft_box_qp_solve and soft_lin_qp_solve on the device, on the pinned fixtures of tests/admm_soft_adjoint_ref.py:
 - against the composition of the calls they are made of (forward soft loop, mask, hard adjoint loop on the masked y, soft gradient
   launch, gbdpcg_kkt_grad_*), bit for bit;
 - torch.autograd.grad of a quadratic loss whose cotangents at the solution are the fixture's against the dense fp64 reference,
   within admm_adjoint_ref.converged_bound as in tests/test_gpu_admm_soft_adjoint.py;
 - problems with zero cotangents get exact zeros;
 - kappa = +Inf everywhere reproduces the hard functions' outputs and gradients bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_soft_adjoint_ref as sa  # noqa: E402
from admm_util import dev, same  # noqa: E402
from gbd_pcg_amd import autograd, binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_admm.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
MAX_ITER = 200
NAMES = {"box": ("G", "C", "g", "c", "lo", "hi", "kappa"), "rows": ("G", "C", "g", "c", "E", "lo", "hi", "kappa")}


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def inputs(kind, dtype, grad=True, kappa=None):
    d, E, lo, hi, kap, gz, glam = sa.fixture(kind)
    arrays = dict(G=d["G"], C=d["C"], g=d["g"], c=d["c"], lo=lo, hi=hi, kappa=kap if kappa is None else kappa)
    if E is not None:
        arrays["E"] = E
    t = {k: dev(arrays[k].astype(dtype).reshape(-1)).requires_grad_(grad) for k in NAMES[kind]}
    rho = dev(np.asarray(sa.FIXTURE_RHO[kind], dtype))
    return t, rho, dev(gz.astype(dtype).reshape(-1)), dev(glam.astype(dtype).reshape(-1))


def solve(solver, kind, dtype, t, rho, iters=sa.K_FWD, adj=sa.K_ADJ, hard=False):
    nx, nu, mx, mu, N, B = sa.dims(kind)
    kw = dict(tol=PCG_TOL[dtype], max_iter=MAX_ITER)
    if kind == "box":
        if hard:
            return autograd.box_qp_solve(solver, nx, nu, N, *(t[k] for k in NAMES[kind][:-1]), rho, iters, adj, **kw)
        return autograd.soft_box_qp_solve(solver, nx, nu, N, *(t[k] for k in NAMES[kind]), rho, iters, adj, **kw)
    if hard:
        return autograd.lin_qp_solve(solver, nx, nu, mx, mu, N, *(t[k] for k in NAMES[kind][:-1]), rho, iters, adj, **kw)
    return autograd.soft_lin_qp_solve(solver, nx, nu, mx, mu, N, *(t[k] for k in NAMES[kind]), rho, iters, adj, **kw)


def composition(solver, kind, dtype, t, rho, gz, glam, iters, adj):
    """The calls the autograd function is documented to make, in its order, on fresh buffers."""
    nx, nu, mx, mu, N, B = sa.dims(kind)
    kw = dict(tol=PCG_TOL[dtype], max_iter=MAX_ITER)
    G, C, g, c, lo, hi, kappa = (t[k].detach() for k in ("G", "C", "g", "c", "lo", "hi", "kappa"))
    E = t["E"].detach() if kind == "rows" else None
    S = torch.empty(B * 3 * nx * nx * N, dtype=g.dtype, device="cuda")
    Pinv, Ginv, gamma = torch.empty_like(S), torch.empty_like(G), torch.empty_like(c)
    lam, z = torch.zeros_like(c), torch.empty_like(g)
    w, y = torch.zeros_like(lo), torch.zeros_like(lo)
    res = torch.zeros(B, 2, dtype=g.dtype, device="cuda")
    if kind == "box":
        solver.kkt_step_reg(nx, nu, N, B, G, C, g, c, rho, S, gamma, Ginv, Pinv, lam, z, **kw)
        gt = solver.admm_soft_init(nx, nu, N, B, g, lo, hi, kappa, rho, w, y)
        for _ in range(iters):
            solver.admm_soft_step(nx, nu, N, B, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res=res, **kw)
    else:
        Gt = solver.admm_lin_form(nx, nu, mx, mu, N, B, G, E, rho)
        solver.kkt_step(nx, nu, N, B, Gt, C, g, c, S, gamma, Ginv, Pinv, lam, z, **kw)
        gt = solver.admm_lin_soft_init(nx, nu, mx, mu, N, B, g, E, lo, hi, kappa, rho, w, y)
        for _ in range(iters):
            solver.admm_lin_soft_step(nx, nu, mx, mu, N, B, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res=res,
                                      **kw)
    nglam = -glam
    gamma2, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(g)
    wa, ya = torch.zeros_like(y), torch.zeros_like(y)
    res2 = torch.empty(B, 2, dtype=g.dtype, device="cuda")
    if kind == "box":
        ym = solver.admm_soft_mask(nx, nu, N, B, y, kappa, rho)
        gta = solver.admm_adjoint_init(nx, nu, N, B, gz, ym, rho, wa, ya)
        for _ in range(adj):
            solver.admm_adjoint_step(nx, nu, N, B, Ginv, C, gz, nglam, ym, rho, S, Pinv, gamma2, alam, az, wa, ya, gta, res=res2, **kw)
        glo, ghi, gk = solver.admm_soft_grad_bounds(nx, nu, N, B, y, kappa, rho, ya, az)
        gG, gC = solver.kkt_grad(nx, nu, N, B, w, lam, wa, alam)
        return dict(out=w, lam=lam, res=res, G=gG, C=gC, g=wa, c=-alam, lo=glo, hi=ghi, kappa=gk)
    ym = solver.admm_lin_soft_mask(nx, nu, mx, mu, N, B, y, kappa, rho)
    gta = solver.admm_lin_adjoint_init(nx, nu, mx, mu, N, B, gz, E, ym, rho, wa, ya)
    for _ in range(adj):
        solver.admm_lin_adjoint_step(nx, nu, mx, mu, N, B, Ginv, C, gz, nglam, E, ym, rho, S, Pinv, gamma2, alam, az, wa, ya, gta, res=res2,
                                     **kw)
    glo, ghi, gk, gE = solver.admm_lin_soft_grad(nx, nu, mx, mu, N, B, z, az, E, y, ya, kappa, rho)
    gG, gC = solver.kkt_grad(nx, nu, N, B, z, lam, az, alam)
    return dict(out=z, lam=lam, res=res, G=gG, C=gC, g=az, c=-alam, E=gE, lo=glo, hi=ghi, kappa=gk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sa.KINDS)
def test_autograd_is_the_composition_bit_for_bit(solver, kind, dtype):
    K = 40       # (bits do not need convergence)
    t, rho, gz, glam = inputs(kind, dtype)
    out, lam, res = solve(solver, kind, dtype, t, rho, K, K)
    grads = torch.autograd.grad((out * gz).sum() + (lam * glam).sum(), [t[k] for k in NAMES[kind]])
    want = composition(solver, kind, dtype, t, rho, gz, glam, K, K)
    torch.cuda.synchronize()
    assert same(out, want["out"]) and same(lam, want["lam"]) and same(res, want["res"])
    for k, gr in zip(NAMES[kind], grads):
        assert same(gr, want[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sa.KINDS)
def test_gradients_of_a_quadratic_loss_match_the_dense_reference(solver, kind, dtype):
    """l = gz'(z - z*) + glam'(lambda - lambda*) + 1/2 |z - z*|^2 with (z*, lambda*) the detached outputs: a quadratic loss whose
    cotangents at the solution are the fixture's gz, glam.  Bound: admm_adjoint_ref.converged_bound, as in
    tests/test_gpu_admm_soft_adjoint.py."""
    nx, nu, mx, mu, N, B = sa.dims(kind)
    t, rho, gz, glam = inputs(kind, dtype)
    out, lam, res = solve(solver, kind, dtype, t, rho)
    loss = ((out - out.detach()) * gz).sum() + ((lam - lam.detach()) * glam).sum() + 0.5 * ((out - out.detach()) ** 2).sum()
    grads = torch.autograd.grad(loss, [t[k] for k in NAMES[kind]])
    torch.cuda.synchronize()
    ref, loop = sa.reference(kind), sa.loop_reference(kind)
    replays = sa.K_FWD + sa.K_ADJ
    for k, gr in zip(NAMES[kind], grads):
        got = gr.cpu().numpy().astype(F64).reshape(B, -1)
        for b in range(B):
            dense = ref[b]["grads"][k]
            err, bound = np.abs(got[b] - dense).max(), sa.converged_bound(loop[b]["grads"][k], dense, replays, STEP_TOL[dtype])
            print(f"{np.dtype(dtype).name} {kind} problem {b} d{k}: {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (b, k, err, bound)
    kap = sa.fixture(kind)[4]
    gk = grads[-1].cpu().numpy().reshape(B, -1)
    assert not gk[np.isinf(kap)].view(np.uint8).any()          # an exactly zero gradient where kappa = +Inf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sa.KINDS)
def test_problems_with_zero_cotangents_get_exact_zeros(solver, kind, dtype):
    nx, nu, mx, mu, N, B = sa.dims(kind)
    t, rho, gz, glam = inputs(kind, dtype)
    out, lam, res = solve(solver, kind, dtype, t, rho, 40, 40)
    live = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=out.dtype, device="cuda").view(B, 1)
    loss = ((out * gz).view(B, -1) * live).sum() + ((lam * glam).view(B, -1) * live).sum()
    grads = torch.autograd.grad(loss, [t[k] for k in NAMES[kind]])
    torch.cuda.synchronize()
    for k, gr in zip(NAMES[kind], grads):
        g2 = gr.view(B, -1)
        assert not bool(g2[1].view(torch.uint8).any()) and not bool(g2[3].view(torch.uint8).any()), k
        assert bool(torch.isfinite(g2).all()) and bool(g2[0].any()) and bool(g2[2].any()), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sa.KINDS)
def test_infinite_kappa_reproduces_the_hard_function(solver, kind, dtype):
    """On the fixture's bounds with every row hard (no convergence is needed for bits; where a hard row is infeasible the two
    functions stall alike)."""
    K = 40
    inf = np.full_like(sa.fixture(kind)[4], np.inf)
    t, rho, gz, glam = inputs(kind, dtype, kappa=inf)
    out, lam, res = solve(solver, kind, dtype, t, rho, K, K)
    grads = torch.autograd.grad((out * gz).sum() + (lam * glam).sum(), [t[k] for k in NAMES[kind]])
    h, _, _, _ = inputs(kind, dtype, kappa=inf)
    hout, hlam, hres = solve(solver, kind, dtype, h, rho, K, K, hard=True)
    hgrads = torch.autograd.grad((hout * gz).sum() + (hlam * glam).sum(), [h[k] for k in NAMES[kind][:-1]])
    torch.cuda.synchronize()
    assert same(out, hout) and same(lam, hlam) and same(res, hres)
    for k, a, b in zip(NAMES[kind][:-1], grads, hgrads):
        assert same(a, b), k
    assert not bool(grads[-1].view(torch.uint8).any())
