"""gbd_pcg_amd.autograd.lin_qp_solve on the device: torch.autograd through the ADMM solve with linear rows, (G, C, g, c, E, lo, hi) ->
(z, lambda), on the pinned fixture of tests/admm_lin_adjoint_ref.py.  All seven gradients of l = gz' z + glam' lambda after K_FWD
forward and K_ADJ adjoint iterations are held against the dense reference within admm_adjoint_ref.converged_bound (the bound of
tests/test_gpu_admm_lin_adjoint.py); rho gets no gradient; a problem with zero cotangents gets exactly zero gradients and leaves its
neighbours' bits alone; the arguments are validated as kkt_solve validates its own; outputs and gradients are, bit for bit, those of
the Solver calls the docstring names, in its order.  Run with -s for the figures."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_adjoint_ref as ar  # noqa: E402
import admm_soft_adjoint_ref as sa  # noqa: E402
from admm_util import dev, same  # noqa: E402
from gbd_pcg_amd import autograd, binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_admm.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
KEYS = ("G", "C", "g", "c", "E", "lo", "hi")


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def inputs(nx, nu, N, B, dtype):
    d, E, lo, hi, gz, glam = ar.fixture(nx, nu, N, B)
    t = {k: dev(d[k].astype(dtype).reshape(-1)).requires_grad_() for k in "GCgc"}
    t["E"] = dev(E.astype(dtype).reshape(-1)).requires_grad_()
    t["lo"], t["hi"] = dev(lo.astype(dtype).reshape(-1)).requires_grad_(), dev(hi.astype(dtype).reshape(-1)).requires_grad_()
    t["rho"] = dev(np.asarray(ar.FIXTURE_RHO[:B], dtype)).requires_grad_()
    return t, dev(gz.astype(dtype).reshape(-1)), dev(glam.astype(dtype).reshape(-1))


def solve(solver, shape, t, dtype):
    nx, nu, N, _ = shape
    mx, mu = ar.FIXTURE_ROWS[shape]
    return autograd.lin_qp_solve(solver, nx, nu, mx, mu, N, t["G"], t["C"], t["g"], t["c"], t["E"], t["lo"], t["hi"], t["rho"], ar.K_FWD,
                                 ar.K_ADJ, tol=PCG_TOL[dtype], max_iter=200)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", ar.FIXTURE_SHAPES)
def test_gradients_match_the_dense_reference(solver, nx, nu, N, B, dtype):
    shape = (nx, nu, N, B)
    ref, loop = ar.reference(*shape), ar.loop_reference(*shape)
    t, gz, glam = inputs(*shape, dtype)
    w, lam, res = solve(solver, shape, t, dtype)
    assert not res.requires_grad and w.requires_grad and lam.requires_grad
    loss = (gz * w).sum() + (glam * lam).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert t["rho"].grad is None
    what, replays = np.dtype(dtype).name, ar.K_FWD + ar.K_ADJ
    for k in KEYS:
        assert t[k].grad is not None and t[k].grad.shape == t[k].shape, k
        got = t[k].grad.cpu().numpy().astype(F64).reshape(B, -1)
        for b in range(B):
            dense = ref[b]["grads"][k]
            err, bound = np.abs(got[b] - dense).max(), ar.converged_bound(loop[b]["grads"][k], dense, replays, STEP_TOL[dtype])
            print(f"{what} ({nx},{nu},{N}) problem {b} d{k}: {err:.3e} (bound {bound:.3e}, scale {np.abs(dense).max():.3e})")
            assert err <= bound, (k, b, err, bound)
    mx, mu = ar.FIXTURE_ROWS[shape]
    for b in range(B):      # dl/dE, dl/dlo, dl/dhi are exactly zero off the active rows
        A = ref[b]["at_lo"] | ref[b]["at_hi"]
        gE = ar.lr.dense_E(nx, nu, mx, mu, N, t["E"].grad.view(B, -1)[b].cpu().numpy())
        assert not gE[~A].any() and gE[A].any()
        assert not t["lo"].grad.view(B, -1)[b].cpu().numpy()[~ref[b]["at_lo"]].any()
        assert not t["hi"].grad.view(B, -1)[b].cpu().numpy()[~ref[b]["at_hi"]].any()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_zero_cotangents_give_zero_gradients_and_leave_the_neighbours_alone(solver, dtype):
    shape = (14, 7, 3, 2)
    nx, nu, N, B = shape
    grads = []
    for masked in (False, True):
        t, gz, glam = inputs(*shape, dtype)
        w, lam, _ = solve(solver, shape, t, dtype)
        if masked:      # problem 1 does not enter the loss
            gz, glam = gz.clone(), glam.clone()
            gz.view(B, -1)[1].zero_()
            glam.view(B, -1)[1].zero_()
        ((gz * w).sum() + (glam * lam).sum()).backward()
        torch.cuda.synchronize()
        grads.append({k: t[k].grad.clone() for k in KEYS})
    for k in KEYS:
        full, part = grads[0][k].view(B, -1), grads[1][k].view(B, -1)
        assert not bool((part[1] != 0).any()), k
        assert bool(torch.isfinite(part).all()), k
        assert same(part[0], full[0]), k


@pytest.mark.parametrize("dtype", [F32, F64])
def test_autograd_is_the_composition_bit_for_bit(solver, dtype):
    """The shape (5, 2, 3, 4) with rows (3, 2) and the bounds of tests/admm_soft_adjoint_ref.py taken hard, 5 forward and 5 adjoint
    iterations (bits do not need convergence): z, lambda, res and the seven gradients against gbdpcg_admm_lin_form_*, gbdpcg_kkt_step_*,
    gbdpcg_admm_lin_init_*, gbdpcg_admm_lin_step_*, gbdpcg_admm_lin_adjoint_init_*, gbdpcg_admm_lin_adjoint_step_*,
    gbdpcg_admm_lin_grad_*, gbdpcg_kkt_grad_* on fresh buffers."""
    K = 5
    nx, nu, mx, mu, N, B = sa.dims("rows")
    d, E, lo, hi, _, gz, glam = sa.fixture("rows")
    arrays = dict(G=d["G"], C=d["C"], g=d["g"], c=d["c"], E=E, lo=lo, hi=hi)
    t = {k: dev(arrays[k].astype(dtype).reshape(-1)).requires_grad_() for k in KEYS}
    rho = dev(np.asarray(sa.FIXTURE_RHO["rows"], dtype))
    gz, glam = dev(gz.astype(dtype).reshape(-1)), dev(glam.astype(dtype).reshape(-1))
    kw = dict(tol=PCG_TOL[dtype], max_iter=200)
    out, lam, res = autograd.lin_qp_solve(solver, nx, nu, mx, mu, N, *(t[k] for k in KEYS), rho, K, K, **kw)
    grads = torch.autograd.grad((out * gz).sum() + (lam * glam).sum(), [t[k] for k in KEYS])

    G, C, g, c, E, lo, hi = (t[k].detach() for k in KEYS)
    S = torch.empty(B * 3 * nx * nx * N, dtype=g.dtype, device="cuda")
    Pinv, Ginv, gamma = torch.empty_like(S), torch.empty_like(G), torch.empty_like(c)
    lam2, z = torch.zeros_like(c), torch.empty_like(g)
    w, y = torch.zeros_like(lo), torch.zeros_like(lo)
    res2 = torch.zeros(B, 2, dtype=g.dtype, device="cuda")
    Gt = solver.admm_lin_form(nx, nu, mx, mu, N, B, G, E, rho)
    solver.kkt_step(nx, nu, N, B, Gt, C, g, c, S, gamma, Ginv, Pinv, lam2, z, **kw)
    gt = solver.admm_lin_init(nx, nu, mx, mu, N, B, g, E, lo, hi, rho, w, y)
    for _ in range(K):
        solver.admm_lin_step(nx, nu, mx, mu, N, B, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam2, z, w, y, gt, res=res2, **kw)
    nglam = -glam
    gamma2, alam, az = torch.empty_like(lam2), torch.zeros_like(lam2), torch.empty_like(g)
    wa, ya = torch.zeros_like(y), torch.zeros_like(y)
    res3 = torch.empty(B, 2, dtype=g.dtype, device="cuda")
    gta = solver.admm_lin_adjoint_init(nx, nu, mx, mu, N, B, gz, E, y, rho, wa, ya)
    for _ in range(K):
        solver.admm_lin_adjoint_step(nx, nu, mx, mu, N, B, Ginv, C, gz, nglam, E, y, rho, S, Pinv, gamma2, alam, az, wa, ya, gta,
                                     res=res3, **kw)
    glo, ghi, gE = solver.admm_lin_grad(nx, nu, mx, mu, N, B, z, az, y, ya, rho)
    gG, gC = solver.kkt_grad(nx, nu, N, B, z, lam2, az, alam)
    torch.cuda.synchronize()
    assert same(out, z) and same(lam, lam2) and same(res, res2)
    for k, gr, want in zip(KEYS, grads, (gG, gC, az, -alam, gE, glo, ghi)):
        assert same(gr, want), k


def test_arguments_are_validated(solver):
    shape = (3, 2, 4, 2)
    nx, nu, N, B = shape
    mx, mu = ar.FIXTURE_ROWS[shape]
    t, _, _ = inputs(*shape, F32)
    a = {k: v.detach() for k, v in t.items()}

    def call(iters=2, adj_iters=2, **over):
        v = {**a, **over}
        return autograd.lin_qp_solve(solver, nx, nu, mx, mu, N, v["G"], v["C"], v["g"], v["c"], v["E"], v["lo"], v["hi"], v["rho"], iters,
                                     adj_iters)

    with pytest.raises(TypeError):
        autograd.lin_qp_solve(None, nx, nu, mx, mu, N, a["G"], a["C"], a["g"], a["c"], a["E"], a["lo"], a["hi"], a["rho"], 2, 2)
    with pytest.raises(ValueError):
        call(E=a["E"][:-1].contiguous())                # size of E
    with pytest.raises(ValueError):
        call(iters=0)
    with pytest.raises(ValueError):
        call(adj_iters=0)
    with pytest.raises(ValueError):
        call(lo=a["lo"].double())                       # dtype
    with pytest.raises(ValueError):
        call(hi=a["hi"].cpu())                          # device
    with pytest.raises(ValueError):
        call(G=a["G"].repeat(2)[::2])                   # contiguity
    with pytest.raises(ValueError):
        call(lo=a["lo"][:-1].contiguous())              # size
    with pytest.raises(ValueError):
        call(rho=a["rho"][:1].contiguous())
    with pytest.raises(ValueError):
        call(g=a["g"][:-1].contiguous())                # not a whole number of problems
    with pytest.raises(TypeError):
        call(**{k: v.half() for k, v in a.items()})
    w, lam, res = call()
    torch.cuda.synchronize()
    assert w.shape == a["g"].shape and lam.shape == a["c"].shape and res.shape == (B, 2)
