"""SURVEY 8f-4 on the device (csrc/schur.hip and csrc/schur_ginv.hip, through the C ABI): KKT blocks -> S, gamma, G^-1 and lambda -> primal step,
against oracle/schur_oracle.py (fp64 block formulas, themselves pinned to a dense KKT solve in test_oracle_schur.py).
PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.  Tolerances: the device inverts the
cost blocks by Gauss-Jordan in working precision, so entries agree with the fp64 formulas to cond(Q) * eps -- 2e-4 of the
largest entry in fp32 (cost blocks of condition <= 30 here), 1e-11 in fp64."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


SHAPES = [(14, 7, 128, 3), (14, 7, 1, 2), (14, 7, 2, 1), (2, 1, 5, 4), (3, 3, 2, 1), (5, 2, 9, 2), (12, 4, 33, 2), (4, 6, 3, 2),
          (36, 18, 6, 1), (1, 1, 4, 1), (44, 3, 3, 1)]


@pytest.mark.parametrize("dtype,tol", [(np.float32, 2e-4), (np.float64, 1e-11)])
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_form_schur_and_recover_vs_oracle(solver, nx, nu, N, B, dtype, tol):
    d = so.gen(nx, nu, N, seed=100 + nx + N, batch=B, dtype=dtype)
    dG, dC, dg, dc = (dev(d[k].reshape(-1)) for k in "GCgc")
    S, gamma, Ginv = solver.form_schur(nx, nu, N, B, dG, dC, dg, dc)
    torch.cuda.synchronize()
    S, gamma, Ginv = S.cpu().numpy().reshape(B, -1), gamma.cpu().numpy().reshape(B, -1), Ginv.cpu().numpy().reshape(B, -1)
    rng = np.random.default_rng(1)
    lam = rng.standard_normal((B, nx * N)).astype(dtype)
    z = solver.recover_primal(nx, nu, N, B, dev(Ginv.reshape(-1)), dC, dg, dev(lam.reshape(-1)))
    torch.cuda.synchronize()
    z = z.cpu().numpy().reshape(B, -1)
    for b in range(B):
        oS, og, oGi = so.form_schur(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        assert close(S[b], oS, tol), "S"
        assert close(gamma[b], og, tol), "gamma"
        assert close(Ginv[b], oGi, tol), "Ginv"
        assert close(z[b], so.recover_primal(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], lam[b]), 10 * tol), "z"
        # storage symmetry, bit for bit: L_{k+1} == R_k', corner blocks zero
        Sb = S[b].reshape(N, 3, nx, nx)
        assert not Sb[0, 0].any() and not Sb[N - 1, 2].any()
        for k in range(N - 1):
            assert np.array_equal(Sb[k + 1, 0], Sb[k, 2].T)


def test_form_schur_blocks_wider_than_a_wavefront(solver):
    """nx = 66 > 64 lanes: every per-row loop of the kernels takes a second trip (fp32 only: the fp64 working set of this
    block size exceeds one compute unit's LDS and is refused)."""
    test_form_schur_and_recover_vs_oracle(solver, 66, 2, 3, 1, np.float32, 2e-4)


def test_general_kernel_where_the_four_knot_form_exists(solver, monkeypatch):
    """nx 14, nu 7 normally takes schur_form_quad_kernel; GBDPCG_SCHUR_GENERAL=1 keeps the any-size kernel on those shapes too.  Both against the oracle, and against each other to rounding."""
    nx, nu, N, B = 14, 7, 32, 5
    d = so.gen(nx, nu, N, seed=8, batch=B, dtype=np.float32)
    dG, dC, dg, dc = (dev(d[k].reshape(-1)) for k in "GCgc")
    fast = [t.cpu().numpy() for t in solver.form_schur(nx, nu, N, B, dG, dC, dg, dc)]
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    test_form_schur_and_recover_vs_oracle(solver, nx, nu, N, B, np.float32, 2e-4)
    gen = [t.cpu().numpy() for t in solver.form_schur(nx, nu, N, B, dG, dC, dg, dc)]
    monkeypatch.delenv("GBDPCG_SCHUR_GENERAL")
    for a, b in zip(fast, gen):
        assert close(a, b, 1e-4) and not np.array_equal(a, b)   # two kernels: other summation order, no mirrored inverses


@pytest.mark.parametrize("N,B", [(4, 1), (8, 3), (128, 2), (64, 40), (36, 7), (256, 1), (1, 3), (2, 2), (3, 5), (5, 3), (50, 3), (127, 2),
                                 (6, 300)])
def test_four_knot_form_runs_of_every_length(solver, N, B):
    """The walking kernel splits a problem into runs when the batch alone does not fill the device (each run starts with a silent
    step on the four knots before it): one problem of 256 knots is 64 runs of 4, 40 problems of 64 knots 2 runs each, ...
    Horizons that are not a multiple of 4 are one run whose last step has quarters without a knot (nothing of theirs may be
    stored: the arrays end with the last knot -- and the outputs behind them are checked for stray writes)."""
    if N % 4:
        nx, nu = 14, 7
        d = so.gen(nx, nu, N, seed=7, batch=B, dtype=np.float32)
        dG, dC, dg, dc = (dev(d[k].reshape(-1)) for k in "GCgc")
        nS, ng, nG = B * 3 * nx * nx * N, B * nx * N, dG.numel()
        big = [torch.full((m + 4096,), 777.0, dtype=torch.float32, device="cuda") for m in (nS, ng, nG)]
        solver.form_schur(nx, nu, N, B, dG, dC, dg, dc, S=big[0], gamma=big[1], Ginv=big[2])
        torch.cuda.synchronize()
        for t, m in zip(big, (nS, ng, nG)):
            assert bool((t[m:] == 777.0).all()) and bool(torch.isfinite(t[:m]).all())
    for dtype, tol in ((np.float32, 2e-4), (np.float64, 1e-11)):
        test_form_schur_and_recover_vs_oracle(solver, 14, 7, N, B, dtype, tol)


QUAD_SHAPES = [(2, 1), (4, 1), (4, 2), (6, 3), (8, 4), (10, 5), (12, 4), (12, 6), (13, 4), (3, 1), (5, 2), (6, 1), (6, 2), (7, 3), (8, 2), (9, 3),
               (10, 4), (11, 4), (12, 3), (14, 7)]   # GBDPCG_QUAD_SHAPES of csrc/schur_common.hpp (14 / 7 last: it has tests of its own)


@pytest.mark.parametrize("nx,nu", QUAD_SHAPES[:-1])
@pytest.mark.parametrize("N,B", [(1, 2), (3, 1), (4, 5), (16, 3), (50, 2), (64, 33), (128, 1), (7, 400)])
def test_four_knot_kernels_of_the_other_block_sizes(solver, monkeypatch, nx, nu, N, B):
    """The four-knots-per-wave formation kernel and the register recovery kernel are built for stateSize = 2 x controlSize in
    {4, 6, 8, 12, 14} and for the 2/1, 4/1, 12/4, 13/4 shapes: every size against the oracle (fp32 and fp64; whole runs, split runs, horizons that are not a multiple of
    4), the recovery bit for bit against the any-size kernel, and nothing written behind the outputs."""
    for dtype, tol in ((np.float32, 2e-4), (np.float64, 1e-11)):
        test_form_schur_and_recover_vs_oracle(solver, nx, nu, N, B, dtype, tol)
    d = so.gen(nx, nu, N, seed=9, batch=B, dtype=np.float32)
    dG, dC, dg, dc = (dev(d[k].reshape(-1)) for k in "GCgc")
    nS, ng, nG = B * 3 * nx * nx * N, B * nx * N, dG.numel()
    big = [torch.full((m + 4096,), 777.0, dtype=torch.float32, device="cuda") for m in (nS, ng, nG)]
    solver.form_schur(nx, nu, N, B, dG, dC, dg, dc, S=big[0], gamma=big[1], Ginv=big[2])
    lam = torch.randn(ng, device="cuda")
    zbig = torch.full((dg.numel() + 4096,), 777.0, dtype=torch.float32, device="cuda")
    solver.recover_primal(nx, nu, N, B, big[2], dC, dg, lam, z=zbig)
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    zg = solver.recover_primal(nx, nu, N, B, big[2], dC, dg, lam)
    monkeypatch.delenv("GBDPCG_SCHUR_GENERAL")
    torch.cuda.synchronize()
    for t, m in zip(big + [zbig], (nS, ng, nG, dg.numel())):
        assert bool((t[m:] == 777.0).all()) and bool(torch.isfinite(t[:m]).all())
    assert torch.equal(zbig[:dg.numel()], zg)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N,B", [(1, 1), (3, 1), (37, 3), (128, 5), (5, 13)])
def test_register_recover_kernel_is_bit_identical_with_the_general_one(solver, monkeypatch, N, B, dtype):
    """nx 14, nu 7 takes schur_recover_quad_kernel (four rows per wavefront, operands straight into registers): the same fma
    chains in the same order as the LDS kernel, so the two must agree bit for bit -- also on row counts that leave quarters,
    waves and workgroups partly empty (the last knot of a problem has no A, B, R^-1, r: what follows it in memory is the next
    problem's data, which the oracle comparison would expose)."""
    nx, nu = 14, 7
    d = so.gen(nx, nu, N, seed=50 + N, batch=B, dtype=dtype)
    rng = np.random.default_rng(2)
    lam = rng.standard_normal(B * nx * N).astype(dtype)
    _, _, Gi = zip(*(so.form_schur(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b]) for b in range(B)))
    dGi = dev(np.concatenate(Gi).astype(dtype))
    dC, dg, dl = dev(d["C"].reshape(-1)), dev(d["g"].reshape(-1)), dev(lam)
    zq = solver.recover_primal(nx, nu, N, B, dGi, dC, dg, dl)
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    zg = solver.recover_primal(nx, nu, N, B, dGi, dC, dg, dl)
    monkeypatch.delenv("GBDPCG_SCHUR_GENERAL")
    torch.cuda.synchronize()
    assert torch.equal(zq, zg) and bool(torch.isfinite(zq).all())
    zo = np.concatenate([so.recover_primal(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], lam.reshape(B, -1)[b]) for b in range(B)])
    assert close(zq.cpu().numpy(), zo, 2e-3 if dtype == np.float32 else 1e-10)


def test_form_schur_without_ginv_and_bad_arguments(solver):
    nx, nu, N, B = 14, 7, 8, 2
    d = so.gen(nx, nu, N, seed=3, batch=B, dtype=np.float32)
    dG, dC, dg, dc = (dev(d[k].reshape(-1)) for k in "GCgc")
    S1, g1, _ = solver.form_schur(nx, nu, N, B, dG, dC, dg, dc)
    S2, g2, none = solver.form_schur(nx, nu, N, B, dG, dC, dg, dc, want_ginv=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(S1, S2) and torch.equal(g1, g2)
    lib = solver.lib
    import ctypes
    u = ctypes.c_uint32
    assert lib.gbdpcg_form_schur_f32(solver.h, u(nx), u(0), u(N), u(B), *(ctypes.c_void_p(t.data_ptr()) for t in (dG, dC, dg, dc, S1, g1)),
                                     None, None) == 1
    assert lib.gbdpcg_form_schur_f32(solver.h, u(nx), u(nu), u(N), u(B), None, *(ctypes.c_void_p(t.data_ptr()) for t in (dC, dg, dc, S1, g1)),
                                     None, None) == 1
    # a block size whose working set does not fit one compute unit's LDS
    assert lib.gbdpcg_form_schur_f64(solver.h, u(80), u(40), u(N), u(1), *(ctypes.c_void_p(t.data_ptr()) for t in (dG, dC, dg, dc, S1, g1)),
                                     None, None) == 4


@pytest.mark.parametrize("dtype,tol", [(np.float32, 3e-4), (np.float64, 1e-9)])
def test_kkt_to_primal_step_end_to_end(solver, dtype, tol):
    """What one SQP iteration of MPCGPU does around the solve, all on the device: KKT blocks -> S, gamma -> stair Pinv ->
    PCG -> primal step; the step and the multipliers against numpy.linalg.solve of the whole KKT system (fp64).  The formed S
    passes the bit-for-bit symmetry test, so the default mode runs its symmetric kernels on it."""
    nx, nu, N, B = 14, 7, 64, 6
    d = so.gen(nx, nu, N, seed=21, batch=B, dtype=dtype)
    dG, dC, dg, dc = (dev(d[k].reshape(-1)) for k in "GCgc")
    S, gamma, Ginv = solver.form_schur(nx, nu, N, B, dG, dC, dg, dc)
    assert bool(solver.check_symmetric(nx, N, B, S).all())
    Pinv = torch.empty_like(S)
    lam = torch.zeros_like(gamma)
    it, fl = solver.form_pinv_solve(nx, N, B, S, Pinv, gamma, lam, kind=binding.PINV_STAIR,
                                    tol=1e-10 if dtype == np.float32 else 1e-22, max_iter=200)
    z = solver.recover_primal(nx, nu, N, B, Ginv, dC, dg, lam)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and (it.cpu().numpy() < 200).all()
    z, lam = z.cpu().numpy().reshape(B, -1), lam.cpu().numpy().reshape(B, -1)
    for b in range(B):
        oz, ol = so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        assert np.linalg.norm(lam[b] - ol) <= tol * np.linalg.norm(ol)
        assert np.linalg.norm(z[b] - oz) <= tol * np.linalg.norm(oz)


def test_form_schur_full_config3_batch(solver):
    """The BASELINE batch shape (1024 problems, stateSize 14, knotPoints 128): size-independent checks on every problem
    (storage symmetry via the device test) and the oracle on a sample."""
    nx, nu, N, B = 14, 7, 128, 1024
    base = so.gen(nx, nu, N, seed=77, batch=8, dtype=np.float32)
    reps = B // 8
    arr = {k: np.tile(base[k], (reps, 1)) for k in "GCgc"}
    arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=np.float32)[:, None] / B)   # gamma differs from problem to problem
    dG, dC, dg, dc = (dev(arr[k].reshape(-1)) for k in "GCgc")
    S, gamma, Ginv = solver.form_schur(nx, nu, N, B, dG, dC, dg, dc)
    assert bool(solver.check_symmetric(nx, N, B, S).all())
    Sh, gh = S.cpu().numpy().reshape(B, -1), gamma.cpu().numpy().reshape(B, -1)
    for b in (0, 9, 515, 1023):
        assert np.array_equal(Sh[b], Sh[b % 8])   # S depends on G and C only
        oS, og, _ = so.form_schur(nx, nu, N, arr["G"][b], arr["C"][b], arr["g"][b], arr["c"][b])
        assert close(Sh[b], oS, 2e-4) and close(gh[b], og, 2e-4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kkt_step_is_the_three_calls(solver, dtype):
    """gbdpcg_kkt_step_* and its graph form against form_schur + form_pinv_solve + recover_primal issued one by one: the same
    kernels on the same buffers, so every output must agree bit for bit -- cold start, a replay after the inputs were rewritten in
    place, and a replay that starts from the previous lambda (warm start: no more iterations than the cold one)."""
    nx, nu, N, B = 14, 7, 24, 9
    td = torch.float32 if dtype == np.float32 else torch.float64
    d = so.gen(nx, nu, N, seed=31, batch=B, dtype=dtype)
    d2 = so.gen(nx, nu, N, seed=32, batch=B, dtype=dtype)
    G, C, g, c = (dev(d[k].reshape(-1)) for k in "GCgc")

    def by_hand():
        S, gamma, Ginv = solver.form_schur(nx, nu, N, B, G, C, g, c)
        Pinv, lam = torch.empty_like(S), torch.zeros_like(gamma)
        it, fl = solver.form_pinv_solve(nx, N, B, S, Pinv, gamma, lam, tol=1e-8, max_iter=100)
        z = solver.recover_primal(nx, nu, N, B, Ginv, C, g, lam)
        torch.cuda.synchronize()
        return [t.clone() for t in (S, gamma, Ginv, Pinv, lam, z, it, fl)]

    want = by_hand()
    S, gamma, Ginv, Pinv = (torch.full_like(t, float("nan")) for t in want[:4])
    lam, z = torch.zeros_like(want[4]), torch.full_like(want[5], float("nan"))
    r, p = torch.empty_like(lam), torch.empty_like(lam)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    solver.kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, r=r, p=p, tol=1e-8, max_iter=100, iters=it, max_iter_exit=fl)
    torch.cuda.synchronize()
    for a, b in zip((S, gamma, Ginv, Pinv, lam, z, it, fl), want):
        assert torch.equal(a, b)
    assert int(fl.sum()) == 0
    # the graph: new inputs written in place, lambda reset -> the by-hand results for those inputs
    gr = solver.graph_kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, r, p, 1e-8, 100, it, fl, z)
    for t, k in zip((G, C, g, c), "GCgc"):
        t.copy_(dev(d2[k].reshape(-1)))
    lam.zero_()
    gr.launch()
    torch.cuda.synchronize()
    cold = it.clone()
    want2 = by_hand()
    for a, b in zip((S, gamma, Ginv, Pinv, lam, z, it, fl), want2):
        assert torch.equal(a, b)
    # warm start: the same system again from its own solution
    gr.launch()
    torch.cuda.synchronize()
    assert bool((it <= cold).all()) and float(it.float().mean()) < 0.5 * float(cold.float().mean())
    oz, _ = so.dense_kkt_solve(nx, nu, N, d2["G"][0], d2["C"][0], d2["g"][0], d2["c"][0])
    zz = z.cpu().numpy().reshape(B, -1)[0]
    assert np.linalg.norm(zz - oz) <= 3e-4 * np.linalg.norm(oz)   # exit test |eta| < 1e-8: a sanity bound, not the parity bar
    gr.close()
    assert td == z.dtype


def _random_kkt_shapes(count=28, seed=99):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        if rng.integers(2):
            nx, nu = QUAD_SHAPES[int(rng.integers(len(QUAD_SHAPES)))]                       # the four-knot kernels
        else:
            nx = int(rng.integers(1, 20))
            nu = int(rng.integers(1, nx + 3))                                               # the any-size kernels
        N = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 16, 21, 40, 64, 77]))
        B = int(rng.choice([1, 2, 3, 17, 120]))
        if nx * nx * N * B > 600000:
            B = max(1, 600000 // (nx * nx * N))
        out.append((nx, nu, N, B, [np.float32, np.float64][int(rng.integers(2))]))
    return out


@pytest.mark.parametrize("nx,nu,N,B,dtype", _random_kkt_shapes(), ids=lambda v: getattr(v, "__name__", str(v)))
def test_randomized_kkt_shapes(solver, nx, nu, N, B, dtype):
    """Random block sizes, horizons and batches through both kernel families (fixed seed): S, gamma, G^-1 and the recovered step
    against the fp64 block formulas, storage symmetry bit for bit."""
    test_form_schur_and_recover_vs_oracle(solver, nx, nu, N, B, dtype, 2e-4 if dtype == np.float32 else 1e-11)
