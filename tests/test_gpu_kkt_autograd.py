"""torch.autograd through the device KKT solve (gbd_pcg_amd.autograd.kkt_solve): l = a random linear functional of (z, lambda)
plus 1/2 ||z||^2, .backward(), every gradient against the fp64 twin (tests/kkt_grad_ref.py) of the same inputs.

Tolerances from the project's own numbers: tests/test_gpu_resolve.py holds kkt_resolve to eps = 3e-4 (fp32) / 1e-9 (fp64) against
the dense solve at pcg_tol 1e-10 / 1e-22, max_iter 200 -- the settings used here.  The forward pair and the adjoint pair are both
such quantities, and every entry of dl/dG, dl/dC is a sum of two products of one of each, so per entry
    |dev - ref| <= (2 eps + eps^2) (||a||inf ||z||inf + ||lambda or z||inf ||a||inf)
with the factors the formula names (the 1/2 of dl/dG included), summed over the batch for the shared form; eps itself, relative to
the largest entry, for dl/dg = a_z and dl/dc = -a_lambda; dl/drho = a_z' z is a sum of nz such products: nz (2 eps + eps^2)
||a_z||inf ||z||inf.  The inputs are generated in fp32 and held in fp64 for the fp64 runs, so one twin serves both precisions.
Run with -s for the measured figures."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kkt_grad_ref as kgr  # noqa: E402
from gbd_pcg_amd import autograd, binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS = {F32: 3e-4, F64: 1e-9}          # tests/test_gpu_resolve.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
MAX_ITER = 200


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def problem(nx, nu, N, B, mode, seed=0):
    """Inputs (fp32 numbers held in fp64) and the fp64 twin, per problem.  mode: "plain", "shared" (problem 0's G and C for every
    problem) or "rho".  Read-only, computed once."""
    d = {k: v.astype(F64) for k, v in so.gen(nx, nu, N, seed=300 + nx + N + seed, batch=B, dtype=F32).items()}
    rng = np.random.default_rng(17 + N + seed)
    wz, wl = rng.standard_normal(d["g"].shape).astype(F32).astype(F64), rng.standard_normal(d["c"].shape).astype(F32).astype(F64)
    rho = rng.uniform(0.2, 1.0, B).astype(F32).astype(F64) if mode == "rho" else np.zeros(B)
    refs = [kgr.reference(nx, nu, N, d["G"][0 if mode == "shared" else b], d["C"][0 if mode == "shared" else b], d["g"][b], d["c"][b],
                          wz[b], wl[b], rho[b], quad=1.0) for b in range(B)]
    for a in list(d.values()) + [wz, wl, rho]:
        a.setflags(write=False)
    return d, wz, wl, rho, refs


def run(solver, nx, nu, N, B, dtype, mode, seed=0, live=None, with_lam=True):
    """kkt_solve and backward on the device; returns the gradients as numpy arrays and (z, lambda).  live: the problems that enter
    the loss (all of them when None); with_lam=False leaves lambda out of the loss."""
    d, wz, wl, rho, _ = problem(nx, nu, N, B, mode, seed)
    mats = 1 if mode == "shared" else B
    t = lambda a: torch.from_numpy(np.array(a, dtype=dtype).reshape(-1)).cuda().requires_grad_()   # noqa: E731
    G, C, g, c = t(d["G"][:mats]), t(d["C"][:mats]), t(d["g"]), t(d["c"])
    r = t(rho) if mode == "rho" else None
    z, lam = autograd.kkt_solve(solver, nx, nu, N, G, C, g, c, rho=r, shared=mode == "shared", tol=PCG_TOL[dtype], max_iter=MAX_ITER)
    if live is None and with_lam:
        loss = (t(wz).detach() * z).sum() + (t(wl).detach() * lam).sum() + 0.5 * (z * z).sum()
    else:
        idx = torch.tensor(list(range(B) if live is None else live), dtype=torch.long, device="cuda")
        zs, ls = z.view(B, -1)[idx], lam.view(B, -1)[idx]
        loss = (t(wz).detach().view(B, -1)[idx] * zs).sum() + 0.5 * (zs * zs).sum()
        if with_lam:
            loss = loss + (t(wl).detach().view(B, -1)[idx] * ls).sum()
    loss.backward()
    torch.cuda.synchronize()
    n = lambda x: None if x is None else x.detach().cpu().numpy().astype(F64)   # noqa: E731
    return {"G": n(G.grad), "C": n(C.grad), "g": n(g.grad), "c": n(c.grad), "rho": None if r is None else n(r.grad), "z": n(z), "lam": n(lam)}


def check(nx, nu, N, B, dtype, mode, got, refs, what):
    eps = EPS[dtype]
    e2 = 2 * eps + eps * eps
    inf = lambda a: float(np.abs(a).max())   # noqa: E731
    sz = so.sizes(nx, nu, N)
    bG = [0.5 * e2 * 2 * inf(r["az"]) * inf(r["z"]) for r in refs]
    bC = [e2 * (inf(r["alam"]) * inf(r["z"]) + inf(r["lam"]) * inf(r["az"])) for r in refs]
    figures = {}
    if mode == "shared":
        pairs = [("G", got["G"], sum(r["gG"] for r in refs), sum(bG)), ("C", got["C"], sum(r["gC"] for r in refs), sum(bC))]
    else:
        pairs = [("G", got["G"].reshape(B, -1)[b], refs[b]["gG"], bG[b]) for b in range(B)]
        pairs += [("C", got["C"].reshape(B, -1)[b], refs[b]["gC"], bC[b]) for b in range(B)]
    for b in range(B):
        pairs.append(("g", got["g"].reshape(B, -1)[b], refs[b]["gg"], eps * inf(refs[b]["gg"])))
        pairs.append(("c", got["c"].reshape(B, -1)[b], refs[b]["gc"], eps * inf(refs[b]["gc"])))
        if mode == "rho":
            pairs.append(("rho", got["rho"][b:b + 1], np.array([refs[b]["grho"]]), sz["g"] * e2 * inf(refs[b]["az"]) * inf(refs[b]["z"])))
    for name, dev, ref, bound in pairs:
        if ref.size:
            assert dev.shape == ref.shape and np.isfinite(dev).all(), name
            figures[name] = max(figures.get(name, 0.0), float(np.abs(dev - ref).max()) / bound)
    print(f"{what} ({nx},{nu},{N},{B}) {np.dtype(dtype).name} {mode}: worst error / bound " +
          " ".join(f"{k} {v:.3f}" for k, v in figures.items()))
    assert all(v <= 1.0 for v in figures.values()), figures


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", kgr.SHAPES)
def test_per_problem_gradients(solver, nx, nu, N, B, dtype):
    got = run(solver, nx, nu, N, B, dtype, "plain")
    check(nx, nu, N, B, dtype, "plain", got, problem(nx, nu, N, B, "plain")[4], "kkt_solve")
    if N == 1:
        assert not got["C"].size


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", [(2, 1, 3, 7), (5, 2, 9, 3), (12, 4, 33, 2), (14, 7, 24, 5)])
def test_shared_gradients_are_the_batch_sum(solver, nx, nu, N, B, dtype):
    got = run(solver, nx, nu, N, B, dtype, "shared")
    assert got["G"].size == so.sizes(nx, nu, N)["G"] and got["C"].size == so.sizes(nx, nu, N)["C"]
    check(nx, nu, N, B, dtype, "shared", got, problem(nx, nu, N, B, "shared")[4], "kkt_solve")


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", [(2, 1, 3, 2), (5, 2, 9, 2), (14, 7, 24, 3)])
def test_regularised_gradients_and_rho(solver, nx, nu, N, B, dtype):
    got = run(solver, nx, nu, N, B, dtype, "rho")
    check(nx, nu, N, B, dtype, "rho", got, problem(nx, nu, N, B, "rho")[4], "kkt_solve")


@pytest.mark.parametrize("dtype", [F32, F64])
def test_second_backward_on_the_same_solver(solver, dtype):
    """A fresh forward and backward on other inputs in between: right on its own, and the first computation repeated afterwards
    gives the bits it gave before -- the handle (symmetric mode, path, workspaces) is left as found."""
    nx, nu, N, B = 14, 7, 24, 3
    first = run(solver, nx, nu, N, B, dtype, "plain")
    check(nx, nu, N, B, dtype, "plain", first, problem(nx, nu, N, B, "plain")[4], "first")
    second = run(solver, nx, nu, N, B, dtype, "plain", seed=1)
    check(nx, nu, N, B, dtype, "plain", second, problem(nx, nu, N, B, "plain", 1)[4], "second")
    again = run(solver, nx, nu, N, B, dtype, "plain")
    for k in ("z", "lam", "G", "C", "g", "c"):
        assert np.array_equal(first[k], again[k]), k


# ---- problems that do not enter the loss: their adjoint right-hand side is exactly zero, and so are their gradients
MASK_SHAPES = [(2, 1, 3, 7), (5, 2, 9, 3), (14, 7, 24, 5)]
PER_PROBLEM = {"plain": ("G", "C", "g", "c"), "rho": ("G", "C", "g", "c", "rho"), "shared": ("g", "c")}


def rows(got, k, B):
    return got[k].reshape(B, -1)


def check_masked(nx, nu, N, B, dtype, mode, got, full, refs, live, what):
    """Masked problems: exact zeros.  Live problems: the bits of the run in which every problem enters the loss (per-problem
    gradients), and check()'s bound against the twin, summed over the live problems for the single G and C of the shared form."""
    dead = [b for b in range(B) if b not in live]
    for k in ("G", "C", "g", "c", "rho"):
        if got[k] is not None:
            assert np.isfinite(got[k]).all(), (what, k)
    for k in PER_PROBLEM[mode]:
        assert not rows(got, k, B)[dead].any(), (what, k)
        if full is not None:
            assert np.array_equal(rows(got, k, B)[live], rows(full, k, B)[live]), (what, k)
    for k in ("z", "lam"):
        assert full is None or np.array_equal(got[k], full[k]), (what, k)
    if not live:
        assert not got["G"].any() and not got["C"].any(), what
        return
    sub = {k: (None if got[k] is None else got[k] if mode == "shared" and k in "GC" else rows(got, k, B)[live].reshape(-1))
           for k in ("G", "C", "g", "c", "rho")}
    sub.update(z=got["z"], lam=got["lam"])
    check(nx, nu, N, len(live), dtype, mode, sub, [refs[b] for b in live], what)


@pytest.mark.parametrize("mode", ["plain", "rho", "shared"])
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", MASK_SHAPES)
def test_problems_outside_the_loss_get_zero_gradients(solver, nx, nu, N, B, dtype, mode):
    live = list(range(0, B, 2))
    full = run(solver, nx, nu, N, B, dtype, mode) if mode != "shared" else None
    got = run(solver, nx, nu, N, B, dtype, mode, live=live)
    if mode == "shared":     # the forward pass is that of the unmasked run; its per-problem gradients serve as `full`
        full = run(solver, nx, nu, N, B, dtype, mode)
    check_masked(nx, nu, N, B, dtype, mode, got, full, problem(nx, nu, N, B, mode)[4], live, "masked")


@pytest.mark.parametrize("mode", ["plain", "rho", "shared"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_every_problem_outside_the_loss(solver, dtype, mode):
    nx, nu, N, B = 5, 2, 9, 3
    got = run(solver, nx, nu, N, B, dtype, mode, live=[])
    check_masked(nx, nu, N, B, dtype, mode, got, None, None, [], "all masked")
    for k in ("G", "C", "g", "c") + (("rho",) if mode == "rho" else ()):
        assert got[k] is not None and not got[k].any(), k


@pytest.mark.parametrize("mode", ["plain", "shared"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_loss_without_lambda_and_masked_problems(solver, dtype, mode):
    """dl/dlambda is absent (None, or the zeros autograd materialises for an unused output): the mask is built from gz alone."""
    nx, nu, N, B = 5, 2, 9, 3
    live = [0, 2]
    d, wz, wl, rho, _ = problem(nx, nu, N, B, mode)
    refs = [kgr.reference(nx, nu, N, d["G"][0 if mode == "shared" else b], d["C"][0 if mode == "shared" else b], d["g"][b], d["c"][b],
                          wz[b], 0.0 * wl[b], 0.0, quad=1.0) for b in range(B)]
    full = run(solver, nx, nu, N, B, dtype, mode, with_lam=False)
    got = run(solver, nx, nu, N, B, dtype, mode, live=live, with_lam=False)
    check_masked(nx, nu, N, B, dtype, mode, got, full, refs, live, "no lambda in the loss")
