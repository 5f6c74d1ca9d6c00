"""The persistent single-launch path (csrc/pcg_persist.hip; BASELINE config 4: n = 36, N = 256, fp64, one problem)
against the CPU oracle, through the C ABI.  Tolerances as in test_gpu_parity.py: fp64 1e-10, fp32 1e-6 norm-wise,
equal iteration counts."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding, synth  # noqa: E402

pytestmark = pytest.mark.gpu
P = binding.PATH_PERSISTENT


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def relerr(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(solver, n, N, B, S, Pinv, gamma, lam0=None, tol=1e-6, max_iter=100, path=P):
    solver.set_path(path)
    try:
        es = S.dtype.itemsize
        assert solver.choose_path(es, n, N, B) == path, "shape not eligible for the persistent path"
        dS, dP, dg = dev(S), dev(Pinv), dev(gamma)
        lam = torch.zeros_like(dg) if lam0 is None else dev(lam0)
        r, p = torch.full_like(dg, float("nan")), torch.full_like(dg, float("nan"))
        it, fl = solver.solve(n, N, B, dS, dP, dg, lam, r, p, tol=tol, max_iter=max_iter)
        torch.cuda.synchronize()
    finally:
        solver.set_path(binding.PATH_AUTO)
    return dict(lambda_=lam.cpu().numpy().reshape(B, -1), r=r.cpu().numpy().reshape(B, -1),
                p=p.cpu().numpy().reshape(B, -1), iters=it.cpu().numpy().astype(np.int64),
                flag=fl.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N,B", [(256, 1), (255, 1), (129, 1), (100, 2), (37, 3), (5, 2), (3, 1), (2, 1), (1, 2)])
def test_persistent_vs_oracle(solver, orc, dtype, N, B):
    n = 36
    d = synth.gen_numpy(n, N, seed=300 + N, batch=B, dtype=dtype)
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=100)
    out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"])
    assert np.array_equal(out["iters"], ob["iters"].astype(np.int64)), (out["iters"], ob["iters"])
    assert not out["flag"].any()
    tol = 1e-10 if dtype == np.float64 else 1e-6
    for b in range(B):
        assert relerr(out["lambda_"][b], ob["lambda_"][b]) < tol
        scale = np.abs(d["gamma"][b]).max()
        assert np.abs(out["r"][b] - ob["r"].reshape(B, -1)[b]).max() < (1e-9 if dtype == np.float64 else 2e-5) * scale
        assert np.abs(out["p"][b] - ob["p"][b]).max() < (1e-9 if dtype == np.float64 else 2e-5) * scale


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_persistent_config4_against_golden(solver, golden_dir, dtype):
    """BASELINE config 4 (n = 36, N = 256): the committed fp64 golden vector (10 iterations with the stair
    preconditioner, 30 with the identity -- SURVEY.md section 8c)."""
    import os
    G = np.load(os.path.join(golden_dir, "gen_36x256.npz"))
    n, N = 36, 256
    d = synth.gen_numpy(n, N, seed=1234, batch=1, dtype=np.float64)
    S, Pi, g = d["S"].astype(dtype), d["Pinv"].astype(dtype), d["gamma"].astype(dtype)
    out = run(solver, n, N, 1, S, Pi, g, max_iter=25)
    assert out["iters"][0] == int(G["iters_f64_stair"]) == 10
    assert relerr(out["lambda_"][0], G["lambda_f64_stair"]) < (1e-10 if dtype == np.float64 else 2e-6)
    out = run(solver, n, N, 1, S, None, g, max_iter=100)      # identity preconditioner (d_Pinv == NULL)
    assert out["iters"][0] == int(G["iters_f64_ident"]) and relerr(out["lambda_"][0], G["lambda_f64_ident"]) < (1e-10 if dtype == np.float64 else 2e-5)


@pytest.mark.parametrize("tol,max_iter", [(1e-6, 0), (1e-6, 1), (1e30, 5), (0.0, 2), (0.0, 7)])
def test_persistent_iteration_edges(solver, orc, tol, max_iter):
    """max_iter = 0 (only r, p = Pinv r are produced), exit on the first test, and fixed iteration counts: lambda, r, p,
    iters and the max-iter flag all follow pcg.cuh:154-212."""
    n, N, B = 36, 70, 2
    d = synth.gen_numpy(n, N, seed=77, batch=B, dtype=np.float64)
    lam0 = np.stack([synth.normals(5 + b, 0, n * N) for b in range(B)]) * 0.1
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], lambda0=lam0, tol=tol, max_iter=max_iter)
    out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], lam0=lam0, tol=tol, max_iter=max_iter)
    assert np.array_equal(out["iters"], ob["iters"].astype(np.int64))
    assert np.array_equal(out["flag"], ob["max_iter_exit"].astype(np.int64))
    scale = np.abs(d["gamma"]).max()
    for key in ("lambda_", "r", "p"):
        assert np.abs(out[key] - ob[key]).max() < 1e-10 * max(scale, np.abs(ob[key]).max()), key


def test_persistent_replays_need_no_clearing(solver, orc):
    """Epochs continue from a base kept in the workspace: back-to-back solves, a graph replayed many times and a solve
    with a different max_iter in between all give the same answer (nothing is cleared between launches)."""
    n, N = 36, 256
    d = synth.gen_numpy(n, N, seed=1234, batch=1, dtype=np.float64)
    ob = orc.pcg_batch(n, N, 1, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=25)
    first = run(solver, n, N, 1, d["S"], d["Pinv"], d["gamma"], max_iter=25)
    assert first["iters"][0] == ob["iters"][0]
    run(solver, n, N, 1, d["S"], d["Pinv"], d["gamma"], tol=0.0, max_iter=3)
    solver.set_path(P)
    try:
        dS, dP, dg = dev(d["S"]), dev(d["Pinv"]), dev(d["gamma"])
        lam = torch.zeros_like(dg)
        r, p = torch.empty_like(dg), torch.empty_like(dg)
        it = torch.zeros(1, dtype=torch.int32, device="cuda")
        fl = torch.zeros(1, dtype=torch.uint8, device="cuda")
        gr = solver.graph_solve(n, N, 1, dS, dP, dg, lam, r, p, 1e-6, 25, it, fl)
        for _ in range(40):
            lam.zero_()
            gr.launch()
        torch.cuda.synchronize()
        gr.close()
    finally:
        solver.set_path(binding.PATH_AUTO)
    assert int(it[0]) == ob["iters"][0] and int(fl[0]) == 0
    assert np.array_equal(lam.cpu().numpy().reshape(1, -1), first["lambda_"])   # bit-identical run to run


# ---- the opt-in single-reduction (Chronopoulos-Gear) form: GBDPCG_PATH_PERSISTENT_1R -----------------------------------
P1R = binding.PATH_PERSISTENT_1R


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N,B,a", [(256, 1, 0.5), (255, 1, 0.5), (100, 2, 0.5), (37, 3, 0.5), (3, 1, 0.5), (1, 2, 0.5), (64, 1, 0.9)])
def test_single_reduction_form_vs_oracle(solver, orc, dtype, N, B, a):
    """One all-gather per iteration instead of two (u = Pinv r, w = S u, gamma and delta together; s = S p by
    recurrence).  Same iterates in exact arithmetic, another rounding sequence, so this is NOT what AUTO runs; the
    claim checked here is the one VERDICT r1 asked for: iteration counts equal to the oracle's (which restates the
    reference's recurrence) and lambda within 1e-10 (fp64) / 1e-6 (fp32, a = 0.5) of it.  On the a = 0.9 generator
    (kappa ~ 800, 50+ iterations) fp32 carries the order sensitivity SURVEY.md section 8c measured for the reference
    itself (1.4e-6 between two summation orders), so the fp32 bound there is 2e-5 and the count may move by one."""
    n = 36
    d = synth.gen_numpy(n, N, seed=500 + N, batch=B, dtype=dtype, a=a)
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=200)
    out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], max_iter=200, path=P1R)
    assert not out["flag"].any()
    hard32 = dtype == np.float32 and a > 0.5
    assert np.abs(out["iters"] - ob["iters"].astype(np.int64)).max() <= (1 if hard32 else 0), (out["iters"], ob["iters"])
    tol = 1e-10 if dtype == np.float64 else (2e-5 if hard32 else 1e-6)
    for b in range(B):
        assert relerr(out["lambda_"][b], ob["lambda_"][b]) < tol, (b, relerr(out["lambda_"][b], ob["lambda_"][b]))
    if not hard32:
        scale = np.abs(d["gamma"]).max()
        assert np.abs(out["r"] - ob["r"]).max() < (1e-9 if dtype == np.float64 else 5e-5) * scale
        assert np.abs(out["p"] - ob["p"]).max() < (1e-9 if dtype == np.float64 else 5e-5) * scale


@pytest.mark.parametrize("tol,max_iter", [(1e-6, 0), (1e-6, 1), (1e30, 5), (0.0, 2), (0.0, 7)])
def test_single_reduction_iteration_edges(solver, orc, tol, max_iter):
    n, N, B = 36, 70, 2
    d = synth.gen_numpy(n, N, seed=77, batch=B, dtype=np.float64)
    lam0 = np.stack([synth.normals(5 + b, 0, n * N) for b in range(B)]) * 0.1
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], lambda0=lam0, tol=tol, max_iter=max_iter)
    out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], lam0=lam0, tol=tol, max_iter=max_iter, path=P1R)
    assert np.array_equal(out["iters"], ob["iters"].astype(np.int64))
    assert np.array_equal(out["flag"], ob["max_iter_exit"].astype(np.int64))
    scale = np.abs(d["gamma"]).max()
    for key in ("lambda_", "r", "p"):
        assert np.abs(out[key] - ob[key]).max() < 1e-9 * max(scale, np.abs(ob[key]).max()), key


def test_auto_never_takes_the_single_reduction_form(solver):
    assert solver.choose_path(8, 36, 256, 1) == binding.PATH_PERSISTENT


# ---- other block sizes: n = 14 (rows of 56 bytes in fp32: the element-wise operand path) -------------------------------
@pytest.mark.parametrize("path", [P, P1R], ids=["two-reductions", "one-reduction"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N,B", [(256, 1), (200, 1), (129, 2), (33, 3), (2, 1)])
def test_persistent_state_size_14(solver, orc, path, dtype, N, B):
    """Long horizons of the iiwa shape (stateSize 14): one problem of N = 256 knots would stream 1.2 MB per iteration
    through one CU on the fused path; the persistent launch keeps it in the registers of 128 CUs."""
    n = 14
    d = synth.gen_numpy(n, N, seed=700 + N, batch=B, dtype=dtype)
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=100)
    out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], path=path)
    assert np.array_equal(out["iters"], ob["iters"].astype(np.int64)), (out["iters"], ob["iters"])
    assert not out["flag"].any()
    for b in range(B):
        assert relerr(out["lambda_"][b], ob["lambda_"][b]) < (1e-10 if dtype == np.float64 else 1e-6)


@pytest.mark.parametrize("path", [P, P1R], ids=["two-reductions", "one-reduction"])
@pytest.mark.parametrize("n,dtype,N,B", [(16, np.float32, 300, 1), (16, np.float64, 256, 1), (16, np.float32, 33, 3), (18, np.float32, 256, 1),
                                         (18, np.float64, 129, 2), (20, np.float32, 64, 1), (20, np.float32, 128, 2), (20, np.float64, 200, 1),
                                         (24, np.float32, 128, 1), (24, np.float32, 400, 1), (24, np.float64, 256, 1), (24, np.float64, 3, 2),
                                         (22, np.float32, 128, 1), (26, np.float32, 100, 1), (28, np.float64, 64, 1), (30, np.float32, 200, 1),
                                         (32, np.float32, 256, 1), (32, np.float64, 33, 2), (34, np.float32, 128, 1)])
def test_persistent_other_state_sizes(solver, orc, path, n, dtype, N, B):
    """The persistent kernels at the even block sizes between BASELINE's 14 and 36 (round 3): one problem of 24 x 128 took 369 us on the split path -- a
    graph of 2 max_iter + 4 launches whatever the iteration count -- and 60 us here.  Against the oracle to tolerance with equal
    iteration counts, in both forms; then (the reference's recurrence) a fixed count from a warm start with r and p."""
    d = synth.gen_numpy(n, N, seed=800 + N + n, batch=B, dtype=dtype)
    tol = 1e-10 if dtype == np.float64 else 1e-6
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=100)
    out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], path=path)
    assert np.array_equal(out["iters"], ob["iters"].astype(np.int64)), (out["iters"], ob["iters"])
    assert not out["flag"].any()
    for b in range(B):
        assert relerr(out["lambda_"][b], ob["lambda_"][b]) < tol
    if path == P:
        lam0 = (0.1 * np.random.default_rng(N).standard_normal((B, n * N))).astype(dtype)
        ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=0.0, max_iter=5, lambda0=lam0)
        out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], lam0=lam0, tol=0.0, max_iter=5, path=path)
        assert (out["iters"] == 5).all() and (out["flag"] == 1).all()
        for b in range(B):
            assert relerr(out["lambda_"][b], ob["lambda_"][b]) < 2 * tol
            scale = np.abs(d["gamma"][b]).max()
            assert np.abs(out["r"][b] - ob["r"].reshape(B, -1)[b]).max() < (1e-9 if dtype == np.float64 else 2e-5) * scale
            assert np.abs(out["p"][b] - ob["p"].reshape(B, -1)[b]).max() < (1e-9 if dtype == np.float64 else 2e-5) * scale


@pytest.mark.parametrize("n,dtype,N,B,max_iter", [(36, np.float64, 256, 3, 100), (36, np.float64, 256, 8, 100), (24, np.float32, 128, 8, 100),
                                                  (24, np.float32, 128, 11, 60), (20, np.float64, 200, 5, 100), (32, np.float32, 100, 9, 200),
                                                  (24, np.float32, 128, 8, 12)])
def test_small_batches_of_large_problems_go_persistent_in_slices(solver, orc, n, dtype, N, B, max_iter):
    """A few problems more than one persistent launch holds: AUTO cuts the batch into persistent launches in a row (api_solve.hip,
    persist_slices) instead of the split path's 2 max_iter + 4 launches -- unless max_iter is so small that the split graph is the
    shorter one (last case).  Every problem against the oracle, warm start, r and p included; then the same as a hipGraph."""
    es = np.dtype(dtype).itemsize
    assert solver.choose_path(es, n, N, B) == binding.PATH_SPLIT and solver.choose_path(es, n, N, 1) == binding.PATH_PERSISTENT
    d = synth.gen_numpy(n, N, seed=1500 + n + B, batch=B, dtype=dtype)
    tol = 1e-10 if dtype == np.float64 else 1e-6
    lam0 = (0.05 * np.random.default_rng(B).standard_normal((B, n * N))).astype(dtype)
    ob = orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=max_iter, lambda0=lam0, nthreads=8)
    dS, dP, dg = dev(d["S"]), dev(d["Pinv"]), dev(d["gamma"])
    lam = dev(lam0)
    r, p = torch.full_like(dg, float("nan")), torch.full_like(dg, float("nan"))
    it, fl = solver.solve(n, N, B, dS, dP, dg, lam, r, p, tol=1e-6, max_iter=max_iter)
    torch.cuda.synchronize()
    assert np.array_equal(it.cpu().numpy().astype(np.int64), ob["iters"].astype(np.int64))
    assert np.array_equal(fl.cpu().numpy().astype(bool), ob["max_iter_exit"].astype(bool))
    lam_h, r_h, p_h = (x.cpu().numpy().reshape(B, -1) for x in (lam, r, p))
    for b in range(B):
        assert relerr(lam_h[b], ob["lambda_"][b]) < tol, b
        scale = np.abs(d["gamma"][b]).max()
        assert np.abs(r_h[b] - ob["r"].reshape(B, -1)[b]).max() < (1e-9 if dtype == np.float64 else 2e-5) * scale
        assert np.abs(p_h[b] - ob["p"].reshape(B, -1)[b]).max() < (1e-9 if dtype == np.float64 else 2e-5) * scale
    # captured: the slices' hand-off words are reserved by the graph entry point before the capture starts
    lam2 = dev(lam0)
    it2 = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl2 = torch.zeros(B, dtype=torch.uint8, device="cuda")
    g = solver.graph_solve(n, N, B, dS, dP, dg, lam2, None, None, 1e-6, max_iter, it2, fl2)
    for _ in range(2):
        lam2.copy_(dev(lam0))
        g.launch()
    torch.cuda.synchronize()
    g.close()
    assert torch.equal(lam2, lam) and np.array_equal(it2.cpu().numpy(), it.cpu().numpy().astype(np.int32))


def test_auto_takes_the_persistent_path_for_one_long_horizon_problem(solver):
    # block sizes beyond the on-chip kernels: one problem goes persistent instead of through 2 max_iter + 4 launches of the split path
    assert solver.choose_path(4, 24, 128, 1) == binding.PATH_PERSISTENT and solver.choose_path(4, 20, 64, 1) == binding.PATH_PERSISTENT
    assert solver.choose_path(4, 16, 600, 1) == binding.PATH_PERSISTENT and solver.choose_path(4, 16, 128, 1) == binding.PATH_FUSED
    assert solver.choose_path(4, 22, 128, 1) == binding.PATH_PERSISTENT and solver.choose_path(8, 32, 64, 1) == binding.PATH_PERSISTENT
    assert solver.choose_path(4, 38, 128, 1) == binding.PATH_SPLIT           # no persistent kernel of that size
    assert solver.choose_path(8, 14, 256, 1) == binding.PATH_PERSISTENT      # 2.4 MB per iteration through one CU otherwise
    # fp32: four CUs keep it resident on the cluster path (3.7 us per iteration against 4.7 here, tools/ab_cluster.py 256 1)
    assert solver.choose_path(4, 14, 256, 1) == binding.PATH_FUSED and solver.cluster_members(4, 14, 256) == 4
    assert solver.choose_path(4, 14, 300, 1) == binding.PATH_FUSED and solver.cluster_members(4, 14, 300) == 5   # up to eight CUs in fp32
    assert solver.choose_path(4, 14, 600, 1) == binding.PATH_PERSISTENT      # beyond eight CUs' worth of knots
    assert solver.choose_path(4, 14, 128, 1) == binding.PATH_FUSED           # symmetric halves resident on one CU (default mode 2)
    assert solver.choose_path(4, 14, 64, 1) == binding.PATH_FUSED            # register-resident
    assert solver.choose_path(4, 14, 256, 64) == binding.PATH_FUSED or solver.choose_path(4, 14, 256, 64) == binding.PATH_SPLIT


_GIVE_UP = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gbd_pcg_amd import binding, synth
from oracle import oracle as orc
s = binding.Solver(0)
form, n, N, dt = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), (np.float64 if sys.argv[5] == "f64" else np.float32)
path = binding.PATH_PERSISTENT if form == "2r" else binding.PATH_PERSISTENT_1R
s.set_path(path)
assert s.choose_path(np.dtype(dt).itemsize, n, N, 1) == path
rescued = "GBDPCG_RESCUE_OFF" not in os.environ
tol = 1e-10 if dt == np.float64 else 1e-6
for rnd, seed in enumerate((5, 6, 5)):   # changed inputs in the second round: nothing of the first may leak into it
    d = synth.gen_numpy(n, N, seed=seed, batch=1, dtype=dt)
    S, P, g = (torch.from_numpy(d[k]).cuda() for k in ("S", "Pinv", "gamma"))
    lam = torch.full_like(g, 0.5)
    r, p = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    it, fl = s.solve(n, N, 1, S, P, g, lam, r, p, tol=1e-6, max_iter=30)
    torch.cuda.synchronize()
    it0, fl0 = int(it.cpu().numpy().astype(np.uint32)[0]), int(fl[0])
    if not rescued:
        assert it0 == 0xffffffff and fl0 == 2, (it0, fl0)
        assert bool((lam == 0.5).all()) and bool((r == 7.0).all()) and bool((p == 7.0).all())   # untouched
    else:
        ob = orc.pcg_batch(n, N, 1, d["S"], d["Pinv"], d["gamma"], lambda0=np.full((1, n * N), 0.5, dt), tol=1e-6, max_iter=30)
        err = np.linalg.norm(lam.cpu().numpy() - ob["lambda_"]) / np.linalg.norm(ob["lambda_"])
        assert it0 == int(ob["iters"][0]) and fl0 == 0 and err < tol, (rnd, it0, ob["iters"], fl0, err)
        assert np.abs(r.cpu().numpy() - ob["r"]).max() < 2e-5 * np.abs(d["gamma"]).max()
    # the late workgroup is late ONCE: the launches that follow are healthy ones, on the persistent kernel itself
    os.environ.pop("GBDPCG_PERSIST_HOLD_US", None)
print("RESULT", "seen" if not rescued else "solved")
"""

_HOOKS_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gbd-pcg_amd", "csrc", "variants",
                          "libgbdpcg_hooks.so")


def _hooked(form, n, N, dt, **hooks):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(_HOOKS_LIB), "make -C gbd-pcg_amd/csrc builds variants/libgbdpcg_hooks.so"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("GBDPCG_PERSIST_", "GBDPCG_RESCUE_"))}
    env.update(GBDPCG_LIB=_HOOKS_LIB, PYTHONPATH=root, **hooks)
    out = subprocess.run([sys.executable, "-c", _GIVE_UP, root, form, str(n), str(N), dt], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1].split()[1]


@pytest.mark.parametrize("form", ["2r", "1r"])
def test_persistent_launch_gives_up_instead_of_hanging(form):
    """A persistent launch whose workgroups are not all there (fault injection of variants/libgbdpcg_hooks.so: the last
    workgroup leaves at once, short spin bound; the shipped library has no such hook) must end by itself, mark the problem
    (d_iters = 0xffffffff, d_max_iter_exit = 2) and leave lambda, r, p as it found them.  Seen with the rescue launch
    switched off (GBDPCG_RESCUE_OFF, hooks build only)."""
    assert _hooked(form, 36, 64, "f64", GBDPCG_PERSIST_DROP_WG="1", GBDPCG_PERSIST_SPIN_LIMIT="2000", GBDPCG_RESCUE_OFF="1") == "seen"


@pytest.mark.parametrize("form,n,N,dt", [("2r", 36, 64, "f64"), ("1r", 36, 64, "f64"), ("2r", 14, 200, "f32"), ("2r", 36, 256, "f64"),
                                        ("2r", 24, 64, "f32"), ("1r", 20, 100, "f64")])
def test_persistent_give_up_is_rescued(form, n, N, dt):
    """The same fault with the library's default behaviour: the streaming launch queued behind the persistent one solves
    the marked problem from the untouched inputs -- vectors in LDS where one workgroup holds them (n = 14, N = 200), in
    device memory otherwise (n = 36: the GVEC form of pcg_fused.hip) -- and the caller gets the oracle's iteration count
    and lambda, three solves in a row on changed inputs.  (What the reference guarantees by refusing a launch that
    cannot be co-resident before it starts, /root/reference/include/pcg.cuh:23-49.)"""
    assert _hooked(form, n, N, dt, GBDPCG_PERSIST_DROP_WG="1", GBDPCG_PERSIST_SPIN_LIMIT="2000") == "solved"


@pytest.mark.parametrize("form", ["2r", "1r"])
def test_late_workgroup_does_not_poison_the_next_launch(form):
    """a workgroup that gets onto the device only after the others have given up (hook: it is held back for
    20 ms, the others' spin bound is ~2 ms) still publishes under the epochs of ITS launch; the epoch base of the next
    launch is stored by the workgroup that finishes last, so the next launch -- on changed inputs -- cannot take what the
    late one left for its own hand-offs.  Every round must equal the oracle (the first through the rescue launch)."""
    assert _hooked(form, 36, 64, "f64", GBDPCG_PERSIST_HOLD_US="20000", GBDPCG_PERSIST_SPIN_LIMIT="2000") == "solved"


def test_alternating_shapes_on_one_handle(solver, orc):
    """The persistent path keeps one zero-initialised hand-off workspace per shape (the slot layout depends on the
    shape): solves of different shapes interleaved on one handle, eager and from a graph captured earlier, all stay
    correct and bit-reproducible."""
    shapes = [(36, 256, 1, np.float64), (14, 200, 1, np.float32), (36, 100, 2, np.float64), (14, 140, 1, np.float64)]
    data, first = {}, {}
    for sh in shapes:
        n, N, B, dt = sh
        d = synth.gen_numpy(n, N, seed=900 + N, batch=B, dtype=dt)
        data[sh] = (d, orc.pcg_batch(n, N, B, d["S"], d["Pinv"], d["gamma"], tol=1e-6, max_iter=60))
    # a graph for the first shape, captured before the others are ever used
    n, N, B, dt = shapes[0]
    d0 = data[shapes[0]][0]
    solver.set_path(P)
    dS, dP, dg = dev(d0["S"]), dev(d0["Pinv"]), dev(d0["gamma"])
    glam = torch.zeros_like(dg)
    git = torch.zeros(B, dtype=torch.int32, device="cuda")
    gfl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    gr = solver.graph_solve(n, N, B, dS, dP, dg, glam, None, None, 1e-6, 60, git, gfl)
    solver.set_path(binding.PATH_AUTO)
    for rnd in range(3):
        for sh in shapes:
            n, N, B, dt = sh
            d, ob = data[sh]
            out = run(solver, n, N, B, d["S"], d["Pinv"], d["gamma"], max_iter=60)
            assert np.array_equal(out["iters"], ob["iters"].astype(np.int64)) and not out["flag"].any(), (sh, rnd)
            for b in range(B):
                assert relerr(out["lambda_"][b], ob["lambda_"][b]) < (1e-10 if dt == np.float64 else 1e-6)
            if sh in first:
                assert np.array_equal(out["lambda_"], first[sh]), (sh, rnd)     # bit-identical run to run
            first.setdefault(sh, out["lambda_"])
        glam.zero_()
        gr.launch()
        torch.cuda.synchronize()
        assert int(git[0]) == int(data[shapes[0]][1]["iters"][0]) and int(gfl[0]) == 0
        assert np.array_equal(glam.cpu().numpy().reshape(1, -1), first[shapes[0]])
    gr.close()
