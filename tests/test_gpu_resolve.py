"""The frozen-linearisation step on the device (csrc/schur_ginv.hip schur_gamma_kernel / schur_gamma_quad_kernel, through the C ABI):
G and C are kept, g and c are new, so S, Phi^-1 and G^-1 stand and only gamma = -(c + C G^-1 g) is formed before the solve.
gamma against oracle/schur_oracle.py::form_schur (fp64 block formulas), the whole step against a dense fp64 solve of the KKT
system.  PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.  Tolerances are those
tests/test_gpu_schur.py applies to the same quantities: 2e-4 / 1e-11 of the largest entry for gamma, 3e-4 / 1e-9 norm-wise for
lambda and z after a tight solve."""
import ctypes

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


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


SHAPES = [(14, 7, 128, 3), (14, 7, 1, 2), (14, 7, 2, 1), (2, 1, 5, 4), (3, 3, 2, 1), (5, 2, 9, 2), (12, 4, 33, 2), (4, 6, 3, 2),
          (36, 18, 6, 1), (1, 1, 4, 1), (44, 3, 3, 1)]   # tests/test_gpu_schur.py
QUAD_SHAPES = [(2, 1), (4, 1), (4, 2), (6, 3), (8, 4), (10, 5), (12, 4), (12, 6), (13, 4), (3, 1), (5, 2), (6, 1), (6, 2), (7, 3), (8, 2), (9, 3),
               (10, 4), (11, 4), (12, 3), (14, 7)]   # GBDPCG_QUAD_SHAPES of csrc/schur_common.hpp
# rows = N * B of 2, 6, 3, 15, 77 and 80: quarters, waves and workgroups (16 rows) partly empty, problems that straddle waves
QUAD_NB = [(1, 2), (2, 3), (3, 1), (5, 3), (7, 11), (16, 5)]
GAMMA_CASES = SHAPES + [(nx, nu, N, B) for nx, nu in QUAD_SHAPES for N, B in QUAD_NB] + [(36, 12, 7, 3)]


def oracle_parts(nx, nu, N, d, dtype):
    """(gamma [B, nx N] in fp64, G^-1 packed and cast to dtype) of the fp64 oracle."""
    B = d["G"].shape[0]
    parts = [so.form_schur(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b]) for b in range(B)]
    return np.stack([p[1] for p in parts]), np.concatenate([np.asarray(p[2]).reshape(-1) for p in parts]).astype(dtype)


@pytest.mark.parametrize("dtype,tol", [(np.float32, 2e-4), (np.float64, 1e-11)])
@pytest.mark.parametrize("nx,nu,N,B", GAMMA_CASES)
def test_form_gamma_vs_oracle(solver, nx, nu, N, B, dtype, tol):
    """The kernel on its own: G^-1 is the fp64 oracle's, cast to the test's precision."""
    d = so.gen(nx, nu, N, seed=200 + nx + N, batch=B, dtype=dtype)
    og, Gi = oracle_parts(nx, nu, N, d, dtype)
    gamma = solver.form_gamma(nx, nu, N, B, dev(Gi), *(dev(d[k].reshape(-1)) for k in "Cgc"))
    torch.cuda.synchronize()
    gamma = gamma.cpu().numpy().reshape(B, -1)
    assert gamma.dtype == dtype and np.isfinite(gamma).all()
    for b in range(B):
        print(f"gamma ({nx},{nu},{N},{B}) {np.dtype(dtype).name} problem {b}: {relerr(gamma[b], og[b]):.3e}")
        assert close(gamma[b], og[b], tol)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,nu", [(14, 7), (13, 4), (2, 1), (9, 3)])
@pytest.mark.parametrize("N,B", [(1, 1), (3, 1), (37, 3), (128, 5), (5, 13)])
def test_register_gamma_kernel_is_bit_identical_with_the_general_one(solver, monkeypatch, nx, nu, N, B, dtype):
    """schur_gamma_quad_kernel (four rows per wavefront, t_{k-1} handed from quarter to quarter, the first quarter forming its
    own) runs the fma chains of schur_gamma_kernel in the same order: the two must agree bit for bit, also where rows, waves
    and workgroups are partly empty and where a problem starts in the middle of a wave."""
    d = so.gen(nx, nu, N, seed=60 + N, batch=B, dtype=dtype)
    og, Gi = oracle_parts(nx, nu, N, d, dtype)
    args = (dev(Gi), *(dev(d[k].reshape(-1)) for k in "Cgc"))
    gq = solver.form_gamma(nx, nu, N, B, *args)
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    gg = solver.form_gamma(nx, nu, N, B, *args)
    monkeypatch.delenv("GBDPCG_SCHUR_GENERAL")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gq).all())
    assert np.array_equal(gq.cpu().numpy(), gg.cpu().numpy())
    assert close(gq.cpu().numpy().reshape(B, -1), og, 2e-4 if dtype == np.float32 else 1e-11)


def factor(solver, nx, nu, N, B, d):
    """Device tensors G, C, g, c and the S, G^-1, Phi^-1 the device forms from them."""
    G, C, g, c = (dev(d[k].reshape(-1)) for k in "GCgc")
    S, _, Ginv = solver.form_schur(nx, nu, N, B, G, C, g, c)
    Pinv = solver.form_pinv(nx, N, B, S, binding.PINV_STAIR)
    return G, C, g, c, S, Ginv, Pinv


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 9), (5, 3, 10, 4)])
def test_kkt_resolve_is_the_three_calls(solver, nx, nu, N, B, dtype):
    """gbdpcg_kkt_resolve_* against form_gamma + solve + recover_primal issued one by one on the same buffers: bit for bit."""
    d = so.gen(nx, nu, N, seed=41, batch=B, dtype=dtype)
    d2 = so.gen(nx, nu, N, seed=42, batch=B, dtype=dtype)
    _, C, _, _, S, Ginv, Pinv = factor(solver, nx, nu, N, B, d)
    g, c = dev(d2["g"].reshape(-1)), dev(d2["c"].reshape(-1))
    gamma = solver.form_gamma(nx, nu, N, B, Ginv, C, g, c)
    lam = torch.zeros_like(gamma)
    r, p = torch.full_like(lam, float("nan")), torch.full_like(lam, float("nan"))
    it, fl = solver.solve(nx, N, B, S, Pinv, gamma, lam, r=r, p=p, tol=1e-8, max_iter=100)
    z = solver.recover_primal(nx, nu, N, B, Ginv, C, g, lam)
    torch.cuda.synchronize()
    want = [t.clone() for t in (gamma, lam, r, p, it, fl, z)]
    gamma2, z2 = torch.full_like(gamma, float("nan")), torch.full_like(z, float("nan"))
    lam2 = torch.zeros_like(lam)
    r2, p2 = torch.full_like(lam, float("nan")), torch.full_like(lam, float("nan"))
    it2 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    fl2 = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    solver.kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma2, lam2, z2, r=r2, p=p2, tol=1e-8, max_iter=100, iters=it2,
                       max_iter_exit=fl2)
    torch.cuda.synchronize()
    for name, a, b in zip("gamma lam r p iters flags z".split(), (gamma2, lam2, r2, p2, it2, fl2, z2), want):
        assert torch.equal(a, b), name
    assert int(fl2.sum()) == 0 and int(it2.min()) > 0


def check_against_dense(nx, nu, N, B, d, dnew, lam, z, tol, what):
    lam, z = lam.cpu().numpy().reshape(B, -1), z.cpu().numpy().reshape(B, -1)
    for b in range(B):
        oz, ol = so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], dnew["g"][b], dnew["c"][b])
        el, ez = np.linalg.norm(lam[b] - ol) / np.linalg.norm(ol), np.linalg.norm(z[b] - oz) / np.linalg.norm(oz)
        print(f"{what} problem {b}: lambda {el:.3e} z {ez:.3e}")
        assert el <= tol and ez <= tol, what


@pytest.mark.parametrize("dtype,tol", [(np.float32, 3e-4), (np.float64, 1e-9)])
def test_resolve_end_to_end(solver, dtype, tol):
    """kkt_step factors the system, then new gradients and residuals go through kkt_resolve from lambda = 0: multipliers and
    step against numpy.linalg.solve of the whole KKT system (fp64).  G^-1, S and Phi^-1 are the device's own."""
    nx, nu, N, B = 14, 7, 64, 6
    pcg_tol = 1e-10 if dtype == np.float32 else 1e-22
    d = so.gen(nx, nu, N, seed=21, batch=B, dtype=dtype)
    d2 = so.gen(nx, nu, N, seed=22, batch=B, dtype=dtype)
    G, C, g, c = (dev(d[k].reshape(-1)) for k in "GCgc")
    S = torch.empty(B * 3 * nx * nx * N, dtype=G.dtype, device="cuda")
    Pinv, Ginv = torch.empty_like(S), torch.empty_like(G)
    gamma = torch.empty(B * nx * N, dtype=G.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it, fl = solver.kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=pcg_tol, max_iter=200)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and (it.cpu().numpy() < 200).all()
    check_against_dense(nx, nu, N, B, d, d, lam, z, tol, "kkt_step")
    g.copy_(dev(d2["g"].reshape(-1)))
    c.copy_(dev(d2["c"].reshape(-1)))
    lam.zero_()
    it, fl = solver.kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, tol=pcg_tol, max_iter=200)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and (it.cpu().numpy() < 200).all()
    check_against_dense(nx, nu, N, B, d, d2, lam, z, tol, "kkt_resolve")


@pytest.mark.parametrize("dtype,tol", [(np.float32, 3e-4), (np.float64, 1e-9)])
def test_resolve_graph_replays(solver, dtype, tol):
    """One graph, three replays, g and c rewritten in place before each; lambda is zeroed before the first only, so the
    second and third start from the previous tick's multipliers.  Replays after that with g and c left alone start from their
    own solution and take at most one iteration."""
    nx, nu, N, B = 14, 7, 64, 6
    pcg_tol = 1e-10 if dtype == np.float32 else 1e-22
    d = so.gen(nx, nu, N, seed=23, batch=B, dtype=dtype)
    _, C, g, c, S, Ginv, Pinv = factor(solver, nx, nu, N, B, d)
    gamma = torch.empty(B * nx * N, dtype=g.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    r, p = torch.empty_like(lam), torch.empty_like(lam)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    gr = solver.graph_kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, pcg_tol, 200, it, fl, z)
    lam.zero_()
    for tick in range(3):
        dn = so.gen(nx, nu, N, seed=24 + tick, batch=B, dtype=dtype)
        g.copy_(dev(dn["g"].reshape(-1)))
        c.copy_(dev(dn["c"].reshape(-1)))
        gr.launch()
        torch.cuda.synchronize()
        print(f"tick {tick}: iters {it.cpu().numpy().tolist()}")
        assert int(fl.sum()) == 0 and int(it.max()) < 200
        check_against_dense(nx, nu, N, B, d, dn, lam, z, tol, f"replay {tick}")
    for again in range(2):
        gr.launch()
        torch.cuda.synchronize()
        print(f"unchanged g, c, replay {again}: iters {it.cpu().numpy().tolist()}")
        assert int(it.max()) <= 1 and int(fl.sum()) == 0
        check_against_dense(nx, nu, N, B, d, dn, lam, z, tol, f"unchanged replay {again}")
    gr.close()


GUARD = 4096


def guarded(n, dtype):
    """A tensor of n elements inside sentinel-filled guard regions; returns (whole, view)."""
    whole = torch.full((n + 2 * GUARD,), 777.0, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool((whole[:GUARD] == 777.0).all()) and bool((whole[GUARD + n:] == 777.0).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 9, 5), (14, 7, 2, 3), (5, 3, 6, 2), (12, 4, 7, 3)])
def test_resolve_footprint(solver, nx, nu, N, B, dtype):
    """kkt_resolve reads S, Pinv, G^-1, C, g, c and leaves them as they were; gamma and z are written inside their bounds."""
    d = so.gen(nx, nu, N, seed=51, batch=B, dtype=dtype)
    _, C, g, c, S, Ginv, Pinv = factor(solver, nx, nu, N, B, d)
    torch.cuda.synchronize()
    kept = [t.clone() for t in (S, Pinv, Ginv, C, g, c)]
    gw, gamma = guarded(B * nx * N, g.dtype)
    zw, z = guarded(g.numel(), g.dtype)
    lam = torch.zeros(B * nx * N, dtype=g.dtype, device="cuda")
    solver.kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, tol=1e-8, max_iter=100)
    torch.cuda.synchronize()
    for name, a, b in zip("S Pinv Ginv C g c".split(), (S, Pinv, Ginv, C, g, c), kept):
        assert torch.equal(a, b), name
    assert guards_intact(gw, gamma.numel()) and guards_intact(zw, z.numel())
    assert bool(torch.isfinite(gamma).all()) and bool(torch.isfinite(z).all()) and not bool((gamma == 777.0).any())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,nu,B", [(14, 7, 1), (14, 7, 6), (5, 3, 3), (36, 12, 2)])
def test_single_knot_writes_gamma_0_only(solver, monkeypatch, nx, nu, B, dtype):
    """N = 1: there is no C, no R, no r; gamma_0 = -(c_0 + Q_0^-1 q_0) per problem and nothing else is written, in either
    kernel."""
    d = so.gen(nx, nu, 1, seed=52, batch=B, dtype=dtype)
    og, Gi = oracle_parts(nx, nu, 1, d, dtype)
    Ginv, C, g, c = dev(Gi), dev(d["C"].reshape(-1)), dev(d["g"].reshape(-1)), dev(d["c"].reshape(-1))
    kept = [t.clone() for t in (Ginv, g, c)]
    for general in (False, True):
        if general:
            monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
        gw, gamma = guarded(B * nx, g.dtype)
        solver.form_gamma(nx, nu, 1, B, Ginv, C, g, c, gamma=gamma)
        torch.cuda.synchronize()
        assert guards_intact(gw, B * nx)
        assert close(gamma.cpu().numpy().reshape(B, -1), og, 2e-4 if dtype == np.float32 else 1e-11)
    monkeypatch.delenv("GBDPCG_SCHUR_GENERAL")
    for a, b in zip((Ginv, g, c), kept):
        assert torch.equal(a, b)


def test_resolve_bad_arguments(solver):
    nx, nu, N, B = 14, 7, 8, 2
    d = so.gen(nx, nu, N, seed=3, batch=B, dtype=np.float32)
    _, C, g, c, S, Ginv, Pinv = factor(solver, nx, nu, N, B, d)
    gamma = torch.empty(B * nx * N, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    lib, h = solver.lib, solver.h
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def calls(suf, ft, nx_, nu_, Gi):
        head = (h, nx_, nu_, N, B, p(Gi), p(C), p(g), p(c))
        solve = (p(S), p(Pinv), p(gamma), p(lam), None, None, ft(1e-6), 10, p(it), None, p(z))
        gr = ctypes.c_void_p()
        out = [getattr(lib, f"gbdpcg_form_gamma_{suf}")(*head, p(gamma), None),
               getattr(lib, f"gbdpcg_kkt_resolve_{suf}")(*head, *solve, None),
               getattr(lib, f"gbdpcg_graph_create_kkt_resolve_{suf}")(*head, *solve, ctypes.byref(gr))]
        assert not gr.value
        return out

    assert calls("f32", ctypes.c_float, nx, nu, None) == [1, 1, 1]      # null G^-1
    assert calls("f32", ctypes.c_float, nx, 0, Ginv) == [1, 1, 1]       # controlSize 0
    assert calls("f32", ctypes.c_float, 0, nu, Ginv) == [1, 1, 1]       # stateSize 0
    # a block size whose working set does not fit one compute unit's LDS: refused like form_schur refuses it
    # (the pointers are not looked at before the shape is)
    assert calls("f64", ctypes.c_double, 80, 40, Ginv) == [4, 4, 4]
    torch.cuda.synchronize()
