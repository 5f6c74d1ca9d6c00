"""GPU: every kernel on BADLY SCALED input, by exact power-of-two rescaling of the variables (tests/scaling_ref.py; the CPU half
is tests/test_scaling_reference.py).

A batch holds K >= 3 differently scaled copies of one base problem (problem 0 unscaled, the last copy with both ends of the
exponent range inside every block: cost blocks of condition up to 2^48 x 30 in fp32, 2^160 x 30 in fp64).  Every operation of the
library is equivariant under the rescaling and a power of two only moves exponents, so after exact unscaling every copy must
equal problem 0 BIT FOR BIT, with equal iteration counts and exit flags: no tolerance.  A hidden absolute threshold, an exit or
rescue test on an unpreconditioned norm, a reciprocal or flush that misbehaves away from 1 or an uninitialised read breaks it.
In the same test the unscaled output of the worst-scaled copy is held to the reference of the BASE problem at the tolerance the
existing test of that entry point uses (tests/test_gpu_schur.py, test_gpu_resolve.py, test_gpu_layout.py, test_gpu_parity.py,
test_gpu_kkt_residual.py); every compared array passes the range condition of scaling_ref.in_range.

Entry points that mix scales (residual norms, rho, the ADMM box, a solve without preconditioner, a shared pair with scaled
right-hand sides) get one exponent per problem: 2^a for the whole of problem b.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import layout_ref as lr  # noqa: E402
import scaling_ref as sr  # noqa: E402
from gbd_pcg_amd import binding, synth  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

K = sr.K_COPIES
IDS = {np.float32: "f32", np.float64: "f64"}


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t, rows=K):
    return t.cpu().numpy().reshape(rows, -1)


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


def normwise(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / np.linalg.norm(b)


class Kkt:
    """K copies of one problem of oracle/schur_oracle.py::gen (drawn in fp32, widened for fp64), and a second right-hand side."""

    def __init__(self, nx, nu, N, dtype, uniform=False, seed=700):
        self.nx, self.nu, self.N, self.dtype, self.shape = nx, nu, N, dtype, (nx, nu, N, K)
        self.d, self.d2, self.ex, self.eu = sr.kkt_case(nx, nu, N, dtype, uniform, seed)   # the CPU half checks these very inputs
        self.a = self.ex[:, 0, 0]                                    # the exponent of copy k where the scaling is uniform
        self.h = sr.kkt_copies(self.d, nx, nu, N, self.ex, self.eu)
        self.h2 = sr.kkt_copies(self.d2, nx, nu, N, self.ex, self.eu)
        assert sr.in_range(dtype, *self.h.values(), *self.h2.values()), "range condition (inputs)"
        self.G, self.C, self.g, self.c = (dev(self.h[k].reshape(-1)) for k in "GCgc")
        self.g2, self.c2 = dev(self.h2["g"].reshape(-1)), dev(self.h2["c"].reshape(-1))

    def e(self, kind):
        return sr.exps(kind, self.nx, self.nu, self.N, self.ex, self.eu)

    def copies(self, base, kind):
        out = sr.copies(np.asarray(base, self.dtype), kind, self.nx, self.nu, self.N, self.ex, self.eu)
        assert sr.in_range(self.dtype, out)
        return out

    def same(self, name, t, kind, corners=False):
        """The device tensor t holds K outputs of `kind`: bitwise equal after unscaling.  Returns the unscaled worst copy."""
        got = host(t)
        if corners:
            got = sr.mask_corners(got, self.N, self.nx)
        return sr.assert_equivariant(name, got, self.e(kind), self.dtype)[K - 1]

    def oracle(self, d=None):
        d = self.d if d is None else d
        return so.form_schur(self.nx, self.nu, self.N, self.d["G"][0], self.d["C"][0], d["g"][0], d["c"][0])

    def dense(self, d=None):
        d = self.d if d is None else d
        return so.dense_kkt_solve(self.nx, self.nu, self.N, self.d["G"][0], self.d["C"][0], d["g"][0], d["c"][0])


def general_kernels(monkeypatch, general):
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")     # the any-size kernels where a four-knot / register form exists
    else:
        monkeypatch.delenv("GBDPCG_SCHUR_GENERAL", raising=False)


KERNELS = pytest.mark.parametrize("general", [False, True], ids=["dispatch", "general"])
PRECISIONS = pytest.mark.parametrize("dtype,ftol,stol", [(np.float32, 2e-4, 3e-4), (np.float64, 1e-11, 1e-9)], ids=["f32", "f64"])


# ------------------------------------------------------------------------------------------ formation and its neighbours
@KERNELS
@PRECISIONS
@pytest.mark.parametrize("nx,nu,N", sr.KKT_SHAPES)
def test_formation(solver, monkeypatch, nx, nu, N, dtype, ftol, stol, general):
    """form_schur (S, gamma, G^-1), form_gamma on the G^-1 it wrote with a new g and c, recover_primal with a given lambda: one
    launch each over the K copies.  The worst copy against the fp64 block formulas of the base problem at the tolerances of
    tests/test_gpu_schur.py (2e-4 / 1e-11 of the largest entry; the recovered step 10 x that); S passes check_symmetric."""
    general_kernels(monkeypatch, general)
    p = Kkt(nx, nu, N, dtype)
    S, gamma, Ginv = solver.form_schur(nx, nu, N, K, p.G, p.C, p.g, p.c)
    gamma2 = solver.form_gamma(nx, nu, N, K, Ginv, p.C, p.g2, p.c2)
    lam = np.random.default_rng(5).standard_normal(nx * N).astype(np.float32)
    z = solver.recover_primal(nx, nu, N, K, Ginv, p.C, p.g, dev(p.copies(lam, "lam").reshape(-1)))
    sym = solver.check_symmetric(nx, N, K, S)
    torch.cuda.synchronize()
    assert sym.cpu().numpy().tolist() == [1] * K
    oS, og, oGi = p.oracle()
    assert close(p.same("S", S, "S"), oS, ftol), "S"
    assert close(p.same("gamma", gamma, "gamma"), og, ftol), "gamma"
    assert close(p.same("Ginv", Ginv, "Ginv"), oGi, ftol), "Ginv"
    assert close(p.same("gamma (form_gamma)", gamma2, "gamma"), p.oracle(p.d2)[1], ftol), "form_gamma"
    oz = so.recover_primal(nx, nu, N, p.d["G"][0], p.d["C"][0], p.d["g"][0], lam)
    assert close(p.same("z", z, "z"), oz, 10 * ftol), "z"


@KERNELS
@PRECISIONS
@pytest.mark.parametrize("nx,nu,N", sr.KKT_SHAPES)
def test_kkt_step_resolve_and_graph(solver, monkeypatch, nx, nu, N, dtype, ftol, stol, general):
    """kkt_step (formation, stair Phi^-1, PCG, recovery), kkt_resolve with a new g and c on what it wrote, and one replay of the
    kkt_step graph: every output of every copy, iteration counts and flags.  The worst copy's lambda and z against the dense
    fp64 solve of the base KKT system at the end-to-end tolerances of tests/test_gpu_resolve.py (3e-4 / 1e-9 norm-wise, PCG to
    1e-10 / 1e-22)."""
    general_kernels(monkeypatch, general)
    p = Kkt(nx, nu, N, dtype)
    td = p.G.dtype
    pcg_tol = 1e-10 if dtype == np.float32 else 1e-22
    S = torch.full((K * 3 * nx * nx * N,), float("nan"), dtype=td, device="cuda")
    Pinv, Ginv = torch.full_like(S, float("nan")), torch.full_like(p.G, float("nan"))
    gamma = torch.full((K * nx * N,), float("nan"), dtype=td, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.full_like(p.g, float("nan"))
    r, pp = torch.full_like(gamma, float("nan")), torch.full_like(gamma, float("nan"))
    it = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    fl = torch.full((K,), 9, dtype=torch.uint8, device="cuda")
    args = (nx, nu, N, K, p.G, p.C, p.g, p.c, S, gamma, Ginv, Pinv, lam)

    def check(what, d):
        torch.cuda.synchronize()
        its, fls = it.cpu().numpy(), fl.cpu().numpy()
        assert (its == its[0]).all() and not fls.any() and 0 < its[0] < 200, (what, its, fls)
        out = {}
        for name, t, kind, corners in (("S", S, "S", False), ("gamma", gamma, "gamma", False), ("Ginv", Ginv, "Ginv", False),
                                       ("Pinv", Pinv, "Pinv", True), ("lambda", lam, "lam", False), ("z", z, "z", False),
                                       ("r", r, "r", False), ("p", pp, "p", False)):
            out[name] = p.same(f"{what}: {name}", t, kind, corners)
        oz, ol = p.dense(d)
        el, ez = normwise(out["lambda"], ol), normwise(out["z"], oz)
        print(f"{what} ({nx},{nu},{N}) {IDS[dtype]}: iters {its.tolist()}, worst copy lambda {el:.3e} z {ez:.3e} (tol {stol:.0e})")
        assert el <= stol and ez <= stol, what
        return [host(t).copy() for t in (S, gamma, Ginv, Pinv, lam, z, r, pp)] + [its.copy()]

    solver.kkt_step(*args, z, r=r, p=pp, tol=pcg_tol, max_iter=200, iters=it, max_iter_exit=fl)
    eager = check("kkt_step", p.d)
    lam.zero_()
    solver.kkt_resolve(nx, nu, N, K, Ginv, p.C, p.g2, p.c2, S, Pinv, gamma, lam, z, r=r, p=pp, tol=pcg_tol, max_iter=200, iters=it,
                       max_iter_exit=fl)
    check("kkt_resolve", p.d2)
    gr = solver.graph_kkt_step(*args, r, pp, pcg_tol, 200, it, fl, z)
    try:
        for t in (S, gamma, Ginv, Pinv, z, r, pp):
            t.fill_(float("nan"))
        lam.zero_()
        gr.launch()
        replay = check("kkt_step graph replay", p.d)
    finally:
        gr.close()
    for i, (a, b) in enumerate(zip(eager, replay)):      # (index 3: Phi^-1, whose corner slots are unspecified)
        assert np.array_equal(sr.mask_corners(a, N, nx) if i == 3 else a, sr.mask_corners(b, N, nx) if i == 3 else b), i


# ------------------------------------------------------------------------------------------------- Phi^-1 formation
@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", [binding.PINV_STAIR, binding.PINV_BLOCK_JACOBI], ids=["stair", "jacobi"])
@pytest.mark.parametrize("n,N", sr.PINV_SHAPES)
def test_form_pinv(solver, n, N, kind, dtype):
    """form_pinv, stair and block-Jacobi, on E S E: T Phi^-1 T bit for bit (the never-read corner slots left out).  The worst
    copy slot by slot against the fp64 host construction on the base S at the bounds of tests/test_gpu_layout.py (2e-5 /
    1e-12); the block-Jacobi output as a whole at those of tests/test_gpu_parity.py (1e-5 / 1e-12)."""
    c = sr.solve_case(n, N, dtype, K)
    P = solver.form_pinv(n, N, K, dev(c["S"]), kind)
    torch.cuda.synchronize()
    back = sr.assert_equivariant("Pinv", sr.mask_corners(host(P), N, n), c["E"]["Pinv"], dtype)[K - 1]
    L, D, R = (np.asarray(b, np.float64) for b in synth.unpack_bt(n, N, c["S"][0]))
    if kind == binding.PINV_STAIR:
        want = np.stack(synth.stair_pinv_blocks(L, D, R), axis=1)[None]
        got = np.swapaxes(back.astype(np.float64).reshape(1, N, 3, n, n), -1, -2)
        errs = (lr.relerr(got[:, 1:, 0], want[:, 1:, 0]) if N > 1 else 0.0, lr.relerr(got[:, :, 1], want[:, :, 1]),
                lr.relerr(got[:, :-1, 2], want[:, :-1, 2]) if N > 1 else 0.0)
        print(f"stair n={n} N={N} {IDS[dtype]}: worst copy relerr L' {errs[0]:.2e} D' {errs[1]:.2e} R' {errs[2]:.2e}")
        assert max(errs) < (1e-12 if dtype == np.float64 else 2e-5), errs
    else:
        zero = np.zeros_like(D)
        want = synth.pack_bt(zero, np.linalg.inv(D), zero)
        assert lr.relerr(back, want) < (1e-12 if dtype == np.float64 else 1e-5)


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", [2, 0])
def test_stair_from_a_non_symmetric_S(solver, mode, dtype):
    """L_{k+1} != R_k^T (tests/layout_ref.py::gen_stair_general): the left slot -D_{k+1}^-1 L_{k+1} D_k^-1 is evaluated on its
    own, so it has to be equivariant on its own."""
    n, N = 14, 17
    S = lr.gen_stair_general(n, N, seed=640, batch=1, dtype=np.float32)[0].astype(dtype)
    want = np.stack(synth.stair_pinv_blocks(*(np.asarray(b, np.float64) for b in synth.unpack_bt(n, N, S[0]))), axis=1)[None]
    ex, _ = sr.draw(640, n, 1, N, K, sr.lim(dtype))
    E = sr.exps("S", n, 1, N, ex)
    Sk = sr.apply(np.broadcast_to(S, E.shape), E)
    assert sr.in_range(dtype, Sk)
    solver.set_symmetric(mode)
    try:
        assert solver.check_symmetric(n, N, K, dev(Sk)).cpu().numpy().tolist() == [0] * K
        P = solver.form_pinv(n, N, K, dev(Sk), binding.PINV_STAIR)
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    back = sr.assert_equivariant("Pinv", sr.mask_corners(host(P), N, n), sr.exps("Pinv", n, 1, N, ex), dtype)[K - 1]
    got = np.swapaxes(back.astype(np.float64).reshape(1, N, 3, n, n), -1, -2)
    errs = (lr.relerr(got[:, 1:, 0], want[:, 1:, 0]), lr.relerr(got[:, :, 1], want[:, :, 1]), lr.relerr(got[:, :-1, 2], want[:, :-1, 2]))
    assert max(errs) < (1e-12 if dtype == np.float64 else 2e-5), errs


# ---------------------------------------------------------------------------------------------------------------- SpMV
@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", [0, 1], ids=["general", "symmetric"])
@pytest.mark.parametrize("n", sr.SPMV_N)
def test_spmv(solver, n, mode, dtype):
    """y = M x on S (x' = T x, y' = E y) and on Phi^-1 (T and E swapped).  The worst copy component-wise against the dense fp64
    product of the base within 2 (3n + 2) u |M| |x|, the bound of tests/test_gpu_layout.py."""
    N = sr.SPMV_KNOTS
    c = sr.solve_case(n, N, dtype, K)
    x = synth.normals(77 + n, 0, n * N).astype(np.float32).astype(dtype)
    solver.set_symmetric(mode)
    try:
        for M, xin, yout in (("S", "lam", "gamma"), ("Pinv", "gamma", "lam")):
            L, D, R = (np.array(b) for b in synth.unpack_bt(n, N, c[M][0]))
            L[1:] = np.swapaxes(R[:-1], -1, -2)       # mirrored bit for bit (the host's stair blocks are mirrors up to rounding only)
            base = synth.pack_bt(L, D, R)
            Mk = sr.apply(np.broadcast_to(base, (K, base.size)), c["E"][M])
            xs = sr.apply(np.broadcast_to(x, (K, n * N)), c["E"][xin])
            assert sr.in_range(dtype, xs, Mk)
            y = solver.spmv(n, N, K, dev(Mk), dev(xs))
            torch.cuda.synchronize()
            back = sr.assert_equivariant(f"spmv {M}", host(y), c["E"][yout], dtype)[K - 1].astype(np.float64)
            A = lr.dense(n, N, base)
            bound = 2 * (3 * n + 2) * lr.unit(dtype) * (np.abs(A) @ np.abs(x.astype(np.float64)))
            assert (np.abs(back - A @ x.astype(np.float64)) <= bound).all(), M
    finally:
        solver.set_symmetric(2)


# -------------------------------------------------------------------------------------------------------------- solves
PATHS = {"sym": binding.PATH_FUSED, "resident": binding.PATH_AUTO, "cluster": binding.PATH_AUTO, "stream": binding.PATH_FUSED,
         "split": binding.PATH_SPLIT, "persist": binding.PATH_PERSISTENT, "persist1r": binding.PATH_PERSISTENT_1R,
         "symstream": binding.PATH_FUSED}
TAKES = {"sym": binding.PATH_FUSED, "resident": binding.PATH_FUSED, "cluster": binding.PATH_FUSED, "stream": binding.PATH_FUSED,
         "split": binding.PATH_SPLIT, "persist": binding.PATH_PERSISTENT, "persist1r": binding.PATH_PERSISTENT_1R,
         "symstream": binding.PATH_FUSED}
MEMBERS = {("cluster", 14, 145): 3, ("cluster", 14, 65): 3, ("cluster", 16, 33): 1, ("resident", 7, 9): 0, ("resident", 13, 5): 0,
           ("stream", 24, 20): 0}      # workgroups per problem of the cluster kernel (0: not a cluster)


def _launch(solver, n, N, B, S, P, gamma, lam0, tol, max_iter, shared=False):
    dg, lam = dev(gamma), dev(lam0)
    r, p = torch.full_like(dg, float("nan")), torch.full_like(dg, float("nan"))
    fn = solver.solve_shared if shared else solver.solve
    it, fl = fn(n, N, B, S, P, dg, lam, r, p, tol=tol, max_iter=max_iter)
    torch.cuda.synchronize()
    return dict(lambda_=host(lam, B), r=host(r, B), p=host(p, B), iters=it.cpu().numpy().astype(np.int64), flag=fl.cpu().numpy().astype(bool))


def _against_oracle(orc, name, n, N, c, P0, back, out, tol, max_iter, dtype, rows):
    """The unscaled worst copies (rows) against the oracle on the base storage, as tests/test_gpu_parity.py and
    tests/test_gpu_layout.py hold a solve: equal iteration counts, lambda norm-wise within 1e-6 / 1e-10, r and p within
    2e-5 / 1e-9 of max |gamma|."""
    for b in rows:
        f = c["first"][b]
        ob = orc.pcg(n, N, c["S"][f], P0[f], c["gamma"][f], lambda0=c["lam0"][f], tol=tol, max_iter=max_iter)
        gmax = np.abs(c["gamma"][f]).max()
        el = lr.relerr(back["lambda_"][b], ob["lambda_"])
        er, ep = (np.abs(back[k][b].astype(np.float64) - ob[k]).max() / gmax for k in ("r", "p"))
        print(f"{name} problem {b}: iters {out['iters'][b]} (oracle {ob['iters']}), lambda {el:.2e}, r {er:.2e}, p {ep:.2e}")
        assert out["iters"][b] == ob["iters"] and out["flag"][b] == ob["max_iter_exit"], name
        assert el < lr.ltol(dtype) and er < lr.vtol(dtype) and ep < lr.vtol(dtype), name


@pytest.mark.parametrize("case", sr.SOLVE_CASES, ids=sr.solve_id)
def test_solve(solver, orc, case):
    """One case per kernel family (scaling_ref.SOLVE_CASES), the stair Phi^-1 formed on the device from the scaled S, at tol 1e-6
    / 200 iterations and at the fixed count tol 0 / 6 iterations.  The persistent kernels take one problem per launch: the
    copies are launches of their own."""
    fam, n, N, dtype, mode, B, bases, warm = case
    name = sr.solve_id(case)
    c = sr.solve_case(n, N, dtype, B, bases, warm)
    es = np.dtype(dtype).itemsize
    per_launch = 1 if fam.startswith("persist") else B
    solver.set_symmetric(mode)
    solver.set_path(PATHS[fam])
    try:
        assert solver.choose_path(es, n, N, per_launch) == TAKES[fam], solver.choose_path(es, n, N, per_launch)
        if (fam, n, N) in MEMBERS:
            assert solver.cluster_members(es, n, N) == MEMBERS[(fam, n, N)]
        dS = dev(c["S"])
        dP = solver.form_pinv(n, N, B, dS, binding.PINV_STAIR)
        torch.cuda.synchronize()
        if mode:
            assert solver.check_symmetric(n, N, B, dS).min().item() == 1 and solver.check_symmetric(n, N, B, dP).min().item() == 1
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if fam == "sym":       # more than one round of clusters, or mode 2 solves the batch with the cluster kernel in general storage
            assert B * solver.cluster_members(es, n, N) > cus and N <= 128
        if fam == "symstream":  # past the resident (fp64 n = 12: 40 knots) and cluster horizons, one problem per compute unit or more
            assert solver.cluster_members(es, n, N) == 0 and N > 128 and B >= cus and n in (8, 10, 12, 14, 16)
        P = sr.mask_corners(host(dP, B), N, n)
        P0 = sr.undo(P, c["E"]["Pinv"])
        assert sr.in_range(dtype, P, P0), "range condition (Pinv)"
        for b in range(B):
            assert np.array_equal(P0[b], P0[c["first"][b]]), f"{name}: Pinv of problem {b} after unscaling"
        for run, tol, max_iter in sr.RUNS:
            if per_launch == B:
                out = _launch(solver, n, N, B, dS, dP, c["gamma"], c["lam0"], tol, max_iter)
            else:
                parts = [_launch(solver, n, N, 1, dS[b], dP[b], c["gamma"][b], c["lam0"][b], tol, max_iter) for b in range(B)]
                out = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
            back = sr.assert_solve_equivariant(f"{name} {run}", c, out, dtype)
            assert (out["iters"] == 6).all() and out["flag"].all() if run == "fixed" else (out["iters"] > 3).all() and not out["flag"].any()
            _against_oracle(orc, f"{name} {run}", n, N, c, P0, back, out, tol, max_iter, dtype, [bases * (K - 1) + j for j in range(bases)])
            if fam == "sym" and mode == 2:
                # the verifying kernel accepted every problem: what it leaves is what the caller's word (mode 1) gives, bit for bit
                solver.set_symmetric(1)
                other = _launch(solver, n, N, B, dS, dP, c["gamma"], c["lam0"], tol, max_iter)
                solver.set_symmetric(mode)
                for key in out:
                    assert np.array_equal(out[key], other[key]), (name, run, "mode 1", key)
            if fam == "symstream":
                # the symmetric streaming kernel forms L_{k+1} x_k from R_k: another summation order than the general kernel of
                # mode 0, so the two agree to rounding and not to the bit
                solver.set_symmetric(0)
                other = _launch(solver, n, N, B, dS, dP, c["gamma"], c["lam0"], tol, max_iter)
                solver.set_symmetric(mode)
                assert not np.array_equal(out["lambda_"], other["lambda_"]), "mode 2 ran the general kernel"
                assert max(lr.relerr(out["lambda_"][b], other["lambda_"][b]) for b in range(0, B, 37)) < lr.ltol(dtype)
    finally:
        solver.set_symmetric(2)
        solver.set_path(binding.PATH_AUTO)


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
def test_solve_shared_with_scaled_right_hand_sides(solver, orc, dtype):
    """gbdpcg_solve_shared_*: ONE S, Phi^-1; gamma and lambda_0 of problem b by 2^a_b.  eta = r.Phi^-1 r scales by 2^2a, so at the
    fixed count the problems of one call are compared, and to a tolerance two calls: one exponent for the batch and tol x 2^2a
    against the unscaled call."""
    n, N, B = 14, 100, 5
    a = sr.lim(dtype)
    base = sr.solve_case(n, N, dtype, 1, warm=True, K=1)
    dS = dev(base["S"][0])
    dP = solver.form_pinv(n, N, 1, dS, binding.PINV_STAIR)
    P0 = sr.mask_corners(host(dP, 1), N, n)
    e = np.array([0, a, -a, 3, -a])[:, None]
    c = dict(batch=B, first=np.zeros(B, int), copy=np.arange(B), E={k: np.broadcast_to(e, (B, n * N)) for k in ("lam", "r", "p")},
             S=base["S"], gamma=base["gamma"], lam0=base["lam0"])
    gam, lam0 = (sr.apply(np.broadcast_to(base[k], (B, n * N)), c["E"]["lam"]) for k in ("gamma", "lam0"))
    out = _launch(solver, n, N, B, dS, dP, gam, lam0, 0.0, 6, shared=True)
    back = sr.assert_solve_equivariant("shared fixed", c, out, dtype)
    _against_oracle(orc, "shared fixed", n, N, c, P0, back, out, 0.0, 6, dtype, [B - 1])
    want = _launch(solver, n, N, B, dS, dP, np.repeat(base["gamma"], B, 0), np.repeat(base["lam0"], B, 0), 1e-6, 200, shared=True)
    for s in (a, -a):
        got = _launch(solver, n, N, B, dS, dP, np.ldexp(np.repeat(base["gamma"], B, 0), s), np.ldexp(np.repeat(base["lam0"], B, 0), s),
                      float(np.ldexp(dtype(1e-6), 2 * s)), 200, shared=True)
        assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["flag"], want["flag"]) and not got["flag"].any()
        for key in ("lambda_", "r", "p"):
            assert sr.in_range(dtype, got[key], want[key]) and np.array_equal(np.ldexp(got[key], -s), want[key]), (s, key)
    c["E"] = {k: np.zeros((B, n * N), int) for k in ("lam", "r", "p")}
    _against_oracle(orc, "shared tol", n, N, c, P0, want, want, 1e-6, 200, dtype, [B - 1])


@pytest.mark.parametrize("dtype", sr.DTYPES, ids=["f32", "f64"])
def test_solve_without_preconditioner(solver, orc, dtype):
    """d_Pinv == NULL: eta = r.r is not invariant, so one exponent a for the whole batch (S by 2^-2a, gamma by 2^-a, lambda by
    2^a) and tol by 2^-2a, against the unscaled launch; p is r-like here.  The unscaled launch against the oracle as
    tests/test_gpu_parity.py holds this call: iteration counts within 3, lambda within 100 x the solve tolerance."""
    n, N, B = 14, 30, 3
    a = sr.lim(dtype)
    base = sr.solve_case(n, N, dtype, B, bases=B, warm=True, K=1)
    for run, tol, max_iter in sr.RUNS:
        want = _launch(solver, n, N, B, dev(base["S"]), None, base["gamma"], base["lam0"], tol, max_iter)
        for e in (a, -a):
            got = _launch(solver, n, N, B, dev(np.ldexp(base["S"], -2 * e)), None, np.ldexp(base["gamma"], -e), np.ldexp(base["lam0"], e),
                          float(np.ldexp(dtype(tol), -2 * e)), max_iter)
            assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["flag"], want["flag"]), (run, e)
            for key, s in (("lambda_", -e), ("r", e), ("p", e)):
                assert sr.in_range(dtype, got[key], want[key]) and np.array_equal(np.ldexp(got[key], s), want[key]), (run, e, key)
        ob = orc.pcg_batch(n, N, B, base["S"], None, base["gamma"], lambda0=base["lam0"], tol=tol, max_iter=max_iter)
        assert (np.abs(want["iters"] - ob["iters"].astype(np.int64)) <= 3).all()
        for b in range(B):
            assert lr.relerr(want["lambda_"][b], ob["lambda_"][b]) < 100 * lr.ltol(dtype), (run, b)


# ------------------------------------------------------------------------------------- entry points that mix scales
UNIFORM = pytest.mark.parametrize("nx,nu,N", sr.UNIFORM_SHAPES)
RHO = 3.0


def add_rho(G, nx, nu, N, rho):
    """Packed G (fp64 copy) with rho on the diagonal of every block."""
    G, sg = np.array(G, dtype=np.float64), nx * nx + nu * nu
    for k in range(N):
        G[k * sg:k * sg + nx * nx:nx + 1] += rho
        if k < N - 1:
            G[k * sg + nx * nx:(k + 1) * sg:nu + 1] += rho
    return G


def residual_within_bounds(p, Gpacked, d, z, lam, res, what):
    """The bounds of tests/test_gpu_kkt_residual.py: (2 nx + 2) u max(|G||z| + |g| + |C'||lambda|), (nx + nu + 2) u max(|C||z| + |c|)."""
    Gd, Cd, g, c = so.dense_kkt(p.nx, p.nu, p.N, Gpacked, p.d["C"][0], d["g"], d["c"])
    z, lam, aC = np.asarray(z, np.float64), np.asarray(lam, np.float64), np.abs(Cd)
    ref = np.array([np.abs(Gd @ z + g + Cd.T @ lam).max(), np.abs(Cd @ z - c).max()])
    mag = np.array([(np.abs(Gd) @ np.abs(z) + np.abs(g) + aC.T @ np.abs(lam)).max(), (aC @ np.abs(z) + np.abs(c)).max()])
    tol = np.array([2 * p.nx + 2, p.nx + p.nu + 2]) * lr.unit(p.dtype) * mag
    err = np.abs(np.asarray(res, np.float64) - ref)
    print(f"{what}: residual norms {res}, reference {ref}, err {err}, bound {tol}")
    assert (err <= tol).all(), what


@KERNELS
@PRECISIONS
@UNIFORM
def test_residual_norms(solver, monkeypatch, nx, nu, N, dtype, ftol, stol, general):
    """kkt_residual and kkt_residual_reg (rho' = 2^2a rho) on problems scaled by 2^a as a whole: stationarity x 2^a, feasibility
    x 2^-a.  kkt_residual_shared on ONE unscaled G, C with g, c, z, lambda of problem b all scaled by 2^s_b: both norms x 2^s."""
    general_kernels(monkeypatch, general)
    p = Kkt(nx, nu, N, dtype, uniform=True)
    rng = np.random.default_rng(11)
    z, lam = rng.standard_normal(p.h["g"].shape[1]).astype(np.float32), rng.standard_normal(nx * N).astype(np.float32)
    dz, dl = dev(p.copies(z, "z").reshape(-1)), dev(p.copies(lam, "lam").reshape(-1))
    rho = np.ldexp(np.full(K, RHO), 2 * p.a).astype(dtype)
    plain = solver.kkt_residual(nx, nu, N, K, p.G, p.C, p.g, p.c, dz, dl)
    reg = solver.kkt_residual_reg(nx, nu, N, K, p.G, p.C, p.g, p.c, dev(rho), dz, dl)
    s = np.array([0, sr.lim(dtype), -sr.lim(dtype)])[:, None]
    one = {k: np.broadcast_to(np.asarray(v, dtype), (K, np.size(v))) for k, v in (("g", p.d["g"][0]), ("c", p.d["c"][0]), ("z", z), ("l", lam))}
    sh = solver.kkt_residual_shared(nx, nu, N, K, p.G[:p.h["G"].shape[1]], p.C[:p.h["C"].shape[1]],
                                    *(dev(sr.apply(one[k], np.broadcast_to(s, one[k].shape)).reshape(-1)) for k in "gczl"))
    torch.cuda.synchronize()
    e = np.stack([p.a, -p.a], axis=1)
    base = {"g": p.d["g"][0], "c": p.d["c"][0]}
    G0 = p.d["G"][0].astype(np.float64)
    residual_within_bounds(p, G0, base, z, lam, sr.assert_equivariant("kkt_residual", host(plain), e, dtype)[K - 1], "kkt_residual")
    residual_within_bounds(p, add_rho(G0, nx, nu, N, RHO), base, z, lam, sr.assert_equivariant("kkt_residual_reg", host(reg), e, dtype)[K - 1],
                           "kkt_residual_reg")
    residual_within_bounds(p, G0, base, z, lam, sr.assert_equivariant("kkt_residual_shared", host(sh), np.broadcast_to(s, (K, 2)), dtype)[K - 1],
                           "kkt_residual_shared")


@KERNELS
@PRECISIONS
@UNIFORM
def test_regularised_step_and_admm(solver, monkeypatch, nx, nu, N, dtype, ftol, stol, general):
    """form_schur_reg and kkt_step_reg with rho' = 2^2a rho, then ADMM on the factorisation they wrote: admm_init, one
    admm_step and one admm_update behind a kkt_resolve, with lo, hi, w, y x 2^-a; ||z - w|| x 2^-a and rho ||w+ - w|| x 2^a.
    The worst copy: S, gamma, G^-1 of G + rho I at the formation tolerances, lambda and z of the step and of the first ADMM
    iteration norm-wise at 3e-4 / 1e-9 against dense fp64 (tests/test_gpu_reg.py, tests/test_gpu_admm.py)."""
    import admm_ref
    general_kernels(monkeypatch, general)
    p = Kkt(nx, nu, N, dtype, uniform=True)
    td, pcg_tol = p.G.dtype, (1e-10 if dtype == np.float32 else 1e-22)
    drho = dev(np.ldexp(np.full(K, RHO), 2 * p.a).astype(dtype))
    Gr = add_rho(p.d["G"][0], nx, nu, N, RHO)
    S, gamma, Ginv = solver.form_schur_reg(nx, nu, N, K, p.G, p.C, p.g, p.c, drho)
    torch.cuda.synchronize()
    for name, t, o in zip(("S", "gamma", "Ginv"), (S, gamma, Ginv), so.form_schur(nx, nu, N, Gr, p.d["C"][0], p.d["g"][0], p.d["c"][0])):
        assert close(p.same(f"form_schur_reg: {name}", t, name), o, ftol), name
    Pinv, lam, z = torch.full_like(S, float("nan")), torch.zeros_like(gamma), torch.full_like(p.g, float("nan"))
    r, pp = torch.full_like(gamma, float("nan")), torch.full_like(gamma, float("nan"))
    it, fl = solver.kkt_step_reg(nx, nu, N, K, p.G, p.C, p.g, p.c, drho, S, gamma, Ginv, Pinv, lam, z, r=r, p=pp, tol=pcg_tol, max_iter=200)

    def outputs(what, ts):
        torch.cuda.synchronize()
        its, fls = it.cpu().numpy(), fl.cpu().numpy()
        assert (its == its[0]).all() and not fls.any() and 0 < its[0] < 200, (what, its, fls)
        return {name: p.same(f"{what}: {name}", t, kind, kind == "Pinv") for name, t, kind in ts}

    out = outputs("kkt_step_reg", [("S", S, "S"), ("gamma", gamma, "gamma"), ("Ginv", Ginv, "Ginv"), ("Pinv", Pinv, "Pinv"),
                                   ("lambda", lam, "lam"), ("z", z, "z"), ("r", r, "r"), ("p", pp, "p")])
    oz, ol = so.dense_kkt_solve(nx, nu, N, Gr, p.d["C"][0], p.d["g"][0], p.d["c"][0])
    assert normwise(out["lambda"], ol) <= stol and normwise(out["z"], oz) <= stol
    # ADMM on the kept factorisation
    lo, hi = admm_ref.box(oz, nx, nu, N)
    rng = np.random.default_rng(13)
    w0 = (np.float32(np.abs(oz).max()) * rng.standard_normal(oz.size)).astype(np.float32)
    y0 = (np.float32(0.1 * np.abs(oz).max()) * rng.standard_normal(oz.size)).astype(np.float32)
    dlo, dhi, w, y = (dev(p.copies(a, "z").reshape(-1)) for a in (lo, hi, w0, y0))
    gt = solver.admm_init(nx, nu, N, K, p.g, dlo, dhi, drho, w, y)
    out = outputs("admm_init", [("w", w, "z"), ("y", y, "z"), ("gt", gt, "g")])
    assert np.array_equal(out["w"], admm_ref.clip(w0.astype(dtype), lo.astype(dtype), hi.astype(dtype)))
    prev = out

    def update_bits(what, now, res):
        """w, y and the two norms of the worst copy against the one-IEEE-operation-per-line formulas of tests/admm_ref.py on
        the z the device solved for: to the bit, as tests/test_gpu_admm.py holds the update."""
        wn, yn, _, _, rr = admm_ref.update_ref(dtype, p.d["g"][:1], lo[None], hi[None], np.array([RHO]), now["z"][None], prev["w"][None],
                                               prev["y"][None])
        assert np.array_equal(now["w"], wn[0]) and np.array_equal(now["y"], yn[0]), what
        assert np.array_equal(res, rr[0]), (what, res, rr[0])
    e_res = np.stack([-p.a, p.a], axis=1)
    it, fl, res = solver.admm_step(nx, nu, N, K, Ginv, p.C, p.g, p.c, dlo, dhi, drho, S, Pinv, gamma, lam, z, w, y, gt, r=r, p=pp,
                                   tol=pcg_tol, max_iter=200)
    state = [("lambda", lam, "lam"), ("z", z, "z"), ("w", w, "z"), ("y", y, "z"), ("gt", gt, "g"), ("gamma", gamma, "gamma"), ("r", r, "r"),
             ("p", pp, "p")]
    out = outputs("admm_step", state)
    update_bits("admm_step", out, sr.assert_equivariant("admm_step: res", host(res), e_res, dtype)[K - 1])
    Gd, Cd, g0, c0 = so.dense_kkt(nx, nu, N, p.d["G"][0], p.d["C"][0], p.d["g"][0], p.d["c"][0])
    ref = admm_ref.admm(Gd, Cd, g0, c0, lo, hi, RHO, 2, w0.astype(np.float64), y0.astype(np.float64))
    el, ez = normwise(out["lambda"], ref["lam"][0]), normwise(out["z"], ref["z"][0])
    print(f"admm_step ({nx},{nu},{N}) {IDS[dtype]}: worst copy lambda {el:.3e} z {ez:.3e} (tol {stol:.0e})")
    assert el <= stol and ez <= stol
    # a second iteration as its two calls: kkt_resolve with gt in the place of g, then admm_update
    it, fl = solver.kkt_resolve(nx, nu, N, K, Ginv, p.C, gt, p.c, S, Pinv, gamma, lam, z, r=r, p=pp, tol=pcg_tol, max_iter=200)
    res = solver.admm_update(nx, nu, N, K, p.g, dlo, dhi, drho, z, w, y, gt)
    prev, out = out, outputs("kkt_resolve + admm_update", state)
    update_bits("admm_update", out, sr.assert_equivariant("admm_update: res", host(res), e_res, dtype)[K - 1])
    el, ez = normwise(out["lambda"], ref["lam"][1]), normwise(out["z"], ref["z"][1])
    print(f"second iteration ({nx},{nu},{N}) {IDS[dtype]}: worst copy lambda {el:.3e} z {ez:.3e} (tol {stol:.0e})")
    assert el <= stol and ez <= stol
    assert td == res.dtype


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "per-entry"])
@PRECISIONS
@UNIFORM
def test_gradients(solver, nx, nu, N, dtype, ftol, stol, uniform):
    """kkt_grad (+ _shared) and kkt_backward (+ _shared): a_z as z, a_lambda as lambda, dl/dG as G^-1, dl/dC dual to C; kkt_grad is
    equivariant under the per-entry T as well.  The worst copy's gradients equal the working-precision outer-product formulas of
    tests/kkt_grad_ref.py bit for bit (what tests/test_gpu_kkt_grad.py holds the kernel to); a_z and a_lambda of kkt_backward
    norm-wise at 3e-4 / 1e-9 against the dense fp64 adjoint.  The shared calls take ONE set of matrices: there the right-hand
    sides of problem b are scaled by 2^s_b as a whole, and the batch sum is compared between a scaled and the unscaled call."""
    import kkt_grad_ref as kgr
    p = Kkt(nx, nu, N, dtype, uniform=uniform)
    rng = np.random.default_rng(17)
    sz = so.sizes(nx, nu, N)
    pts = [rng.standard_normal(sz[k]).astype(np.float32).astype(dtype) for k in ("g", "c", "g", "c")]          # z, lam, az, alam
    kinds = ("z", "lam", "z", "lam")
    gG, gC = solver.kkt_grad(nx, nu, N, K, *(dev(p.copies(a, k).reshape(-1)) for a, k in zip(pts, kinds)))
    torch.cuda.synchronize()
    tG, tC = kgr.block_grads(nx, nu, N, *pts, dtype=dtype)
    assert np.array_equal(p.same("kkt_grad: gG", gG, "gG"), tG) and np.array_equal(p.same("kkt_grad: gC", gC, "gC"), tC)
    if not uniform:
        return
    pcg_tol = 1e-10 if dtype == np.float32 else 1e-22
    S, gamma, Ginv = solver.form_schur(nx, nu, N, K, p.G, p.C, p.g, p.c)
    Pinv = solver.form_pinv(nx, N, K, S, binding.PINV_STAIR)
    lam, z = torch.zeros_like(gamma), torch.empty_like(p.g)
    solver.kkt_resolve(nx, nu, N, K, Ginv, p.C, p.g, p.c, S, Pinv, gamma, lam, z, tol=pcg_tol, max_iter=200)
    gz, nglam = pts[2], pts[3]                                                     # dl/dz (g-like), -dl/dlambda (c-like)
    az, alam = torch.full_like(z, float("nan")), torch.zeros_like(lam)
    gG, gC = torch.full_like(p.G, float("nan")), torch.full_like(p.C, float("nan"))
    it, fl = solver.kkt_backward(nx, nu, N, K, Ginv, p.C, dev(p.copies(gz, "g").reshape(-1)), dev(p.copies(nglam, "c").reshape(-1)), S, Pinv,
                                 gamma, z, lam, az, alam, gG, gC, tol=pcg_tol, max_iter=200)
    torch.cuda.synchronize()
    its = it.cpu().numpy()
    assert (its == its[0]).all() and not fl.cpu().numpy().any() and 0 < its[0] < 200
    back = {name: p.same(f"kkt_backward: {name}", t, kind) for name, t, kind in
            (("z", z, "z"), ("lam", lam, "lam"), ("az", az, "z"), ("alam", alam, "lam"), ("gG", gG, "gG"), ("gC", gC, "gC"))}
    tG, tC = kgr.block_grads(nx, nu, N, back["z"], back["lam"], back["az"], back["alam"], dtype=dtype)
    assert np.array_equal(back["gG"], tG) and np.array_equal(back["gC"], tC)
    oaz, oal = kgr.adjoint(nx, nu, N, p.d["G"][0], p.d["C"][0], gz, -nglam.astype(np.float64))
    assert normwise(back["az"], oaz) <= stol and normwise(back["alam"], oal) <= stol
    # shared matrices (problem 0's, unscaled): right-hand sides of problem b by 2^s_b, against the call with s = 0
    nG, nC, nS = p.h["G"].shape[1], p.h["C"].shape[1], 3 * nx * nx * N
    s = np.array([sr.lim(dtype), 0, -sr.lim(dtype)])[:, None]
    got = {}
    for tag, sh in (("unscaled", 0 * s), ("scaled", s)):
        rep = lambda a, f=1: dev(np.ldexp(np.broadcast_to(np.asarray(a, dtype), (K, np.size(a))), f * sh).astype(dtype).reshape(-1))  # noqa: E731
        zs, ls = rep(host(z)[0]), rep(host(lam)[0])
        azs, als = torch.full_like(zs, float("nan")), torch.zeros_like(ls)
        gGs, gCs = torch.full_like(p.G[:nG], float("nan")), torch.full_like(p.C[:nC], float("nan"))
        gam = torch.empty_like(ls)
        it, fl = solver.kkt_backward_shared(nx, nu, N, K, Ginv[:nG], p.C[:nC], rep(gz, -1), rep(nglam, -1), S[:nS], Pinv[:nS], gam, zs, ls, azs,
                                            als, gGs, gCs, tol=0.0, max_iter=4)      # (eta scales with s: a fixed count)
        gG2, gC2 = solver.kkt_grad_shared(nx, nu, N, K, zs, ls, azs, als)
        torch.cuda.synchronize()
        assert torch.equal(gG2, gGs) and torch.equal(gC2, gCs)
        got[tag] = [host(azs), host(als), host(gGs, 1), host(gCs, 1), it.cpu().numpy()]
    # z, lambda x 2^s and dl/dz, dl/dlambda x 2^-s: the adjoint pair x 2^-s, every outer product unchanged
    for i, f in ((0, 1), (1, 1)):
        assert sr.in_range(dtype, got["scaled"][i]) and np.array_equal(np.ldexp(got["scaled"][i], f * np.broadcast_to(s, got["scaled"][i].shape)),
                                                                       got["unscaled"][i])
    assert np.array_equal(got["scaled"][2], got["unscaled"][2]) and np.array_equal(got["scaled"][3], got["unscaled"][3])
    assert np.array_equal(got["scaled"][4], got["unscaled"][4])
    # the shared calls against fp64, run to the tolerance on the unscaled right-hand sides (K equal problems): the adjoint pair
    # at 3e-4 / 1e-9, the batch sums within K x the per-entry bound of tests/test_gpu_kkt_autograd.py
    sh = 0 * s
    zs, ls = rep(host(z)[0]), rep(host(lam)[0])
    azs, als, gam = torch.full_like(zs, float("nan")), torch.zeros_like(ls), torch.empty_like(ls)
    gGs, gCs = torch.full_like(p.G[:nG], float("nan")), torch.full_like(p.C[:nC], float("nan"))
    it, fl = solver.kkt_backward_shared(nx, nu, N, K, Ginv[:nG], p.C[:nC], rep(gz), rep(nglam), S[:nS], Pinv[:nS], gam, zs, ls, azs, als, gGs,
                                        gCs, tol=pcg_tol, max_iter=200)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and int(it.max()) < 200
    ref = kgr.reference(nx, nu, N, p.d["G"][0], p.d["C"][0], p.d["g"][0], p.d["c"][0], gz, -nglam.astype(np.float64))
    e2, inf = 2 * stol + stol * stol, lambda a: float(np.abs(a).max())   # noqa: E731
    for b in range(K):
        assert normwise(host(azs)[b], ref["az"]) <= stol and normwise(host(als)[b], ref["alam"]) <= stol
    assert np.abs(host(gGs, 1)[0] - K * ref["gG"]).max() <= K * 0.5 * e2 * 2 * inf(ref["az"]) * inf(ref["z"])
    assert np.abs(host(gCs, 1)[0] - K * ref["gC"]).max() <= K * e2 * (inf(ref["alam"]) * inf(ref["z"]) + inf(ref["lam"]) * inf(ref["az"]))


@PRECISIONS
@UNIFORM
def test_gradient_in_rho(solver, nx, nu, N, dtype, ftol, stol):
    """dl/drho_b = a_z' z, formed by gbd_pcg_amd.autograd.kkt_solve behind kkt_step_reg and the adjoint solve: x 2^-2a for problem b
    scaled by 2^a as a whole with rho' = 2^2a rho (every product of the sum has that one scale).  The sum is torch's, and
    its order depends on where a problem's row starts in memory (fp32, nz = 497: problem 1 differs from problem 0 in the last
    place on identical data), so each copy is compared with the UNSCALED problem at the same batch position, a second call, as
    the single-problem persistent solves are; z and lambda of the scaled call within the batch as everywhere.  The worst copy against the
    fp64 twin within nz (2 eps + eps^2) ||a_z|| ||z||, the bound of tests/test_gpu_kkt_autograd.py (eps = 3e-4 / 1e-9)."""
    import kkt_grad_ref as kgr
    from gbd_pcg_amd import autograd
    p = Kkt(nx, nu, N, dtype, uniform=True)
    rng = np.random.default_rng(19)
    wz = rng.standard_normal(p.h["g"].shape[1]).astype(np.float32)       # dl/dz: transforms as g
    wl = rng.standard_normal(nx * N).astype(np.float32)                  # dl/dlambda: transforms as c
    pcg_tol = 1e-10 if dtype == np.float32 else 1e-22

    def run(scaled):
        """(z, lambda, dl/drho) of the K copies; not scaled: K times the base problem, the same batch positions."""
        pick = (lambda a: a) if scaled else (lambda a: np.repeat(a[:1], K, axis=0))   # noqa: E731
        G, C, g, c = (dev(pick(p.h[k]).reshape(-1)) for k in "GCgc")
        rho = dev(pick(np.ldexp(np.full(K, RHO), 2 * p.a).astype(dtype))).requires_grad_()
        z, lam = autograd.kkt_solve(solver, nx, nu, N, G, C, g, c, rho=rho, tol=pcg_tol, max_iter=200)
        loss = (dev(pick(p.copies(wz, "g")).reshape(-1)) * z).sum() + (dev(pick(p.copies(wl, "c")).reshape(-1)) * lam).sum()
        loss.backward()
        torch.cuda.synchronize()
        return z.detach(), lam.detach(), host(rho.grad)

    z, lam, got = run(True)
    _, _, want = run(False)
    p.same("z", z, "z")
    p.same("lambda", lam, "lam")
    assert got.dtype == np.dtype(dtype) and np.isfinite(got).all() and sr.in_range(dtype, got, want)
    assert np.array_equal(np.ldexp(got, 2 * p.a[:, None].astype(np.int32)), want), (got, want)
    grho = want[K - 1, 0]
    ref = kgr.reference(nx, nu, N, p.d["G"][0], p.d["C"][0], p.d["g"][0], p.d["c"][0], wz, wl, RHO)
    bound = p.h["g"].shape[1] * (2 * stol + stol * stol) * np.abs(ref["az"]).max() * np.abs(ref["z"]).max()
    print(f"dl/drho ({nx},{nu},{N}) {IDS[dtype]}: {grho!r}, fp64 {ref['grho']!r}, bound {bound:.2e}")
    assert abs(float(grho) - ref["grho"]) <= bound
