"""Per-problem regularisation on the device (the REG instantiations of csrc/schur.hip and csrc/schur_residual.hip, through the C ABI): problem b is formed,
solved and judged with G_b + rho_b I in place of G_b -- gbdpcg_form_schur_reg_*, gbdpcg_kkt_step_reg_* and its graph,
gbdpcg_kkt_residual_reg_*.  PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.

Reference: fp64 numpy of oracle/schur_oracle.py, unchanged, on a COPY of the packed G with rho_b added to the diagonals in fp64
(rho_b and all data are fp32 numbers cast up, exact in either precision): so.form_schur for S, gamma, G^-1, so.dense_kkt_solve
for steps, so.dense_kkt for residuals.

Tolerances are the project's own: 2e-4 (fp32) / 1e-11 (fp64) of the largest entry for S, gamma, G^-1 (tests/test_gpu_schur.py:
entries agree to cond(Q) eps for cost blocks of condition <= 30, and adding rho >= 0 never raises the condition number); 3e-4 /
1e-9 norm-wise for lambda and z after a tight solve (test_gpu_schur.py, test_gpu_resolve.py); the derived row bounds of
tests/test_gpu_kkt_residual.py for the residual norms, the magnitude term taken with |G + rho I|.

rho_b = 0.5 (b + 1) wherever nothing else is said: distinct from problem to problem, so an indexing slip cannot pass.  Every
shape runs under the default dispatch and under GBDPCG_SCHUR_GENERAL=1 (the any-size kernels)."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
# four-knot form of 14 / 7: a run boundary (5), N = 1 without C, problems that straddle waves with empty quarters (3 x 5), three
# steps (9); the other four-knot sizes; then general kernel only: nu > nx, large blocks
SHAPES = [(14, 7, 5, 3), (14, 7, 1, 2), (14, 7, 3, 5), (14, 7, 9, 2), (12, 4, 33, 2), (2, 1, 5, 4), (3, 3, 2, 1), (4, 6, 3, 2),
          (36, 18, 6, 1)]
DTYPES = [F32, F64]
FORM_TOL = {F32: 2e-4, F64: 1e-11}
STEP_TOL = {F32: 3e-4, F64: 1e-9}
PCG_TOL = {F32: 1e-10, F64: 1e-22}
POINTS = ("solution", "solution + 1e-3 noise", "random")


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@pytest.fixture(params=[False, True], ids=["default", "general"])
def general(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    return request.param


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the cached references are read-only)


def tdt(dtype):
    return torch.float32 if dtype == F32 else torch.float64


def close(a, b, tol):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


def relerr(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def rho_default(B):
    return 0.5 * (np.arange(B, dtype=F64) + 1.0)


def diag_index(nx, nu, N):
    """Positions of the diagonal entries of Q_0, R_0, ..., Q_{N-1} in one problem's packed G."""
    sg, idx = nx * nx + nu * nu, []
    for k in range(N):
        idx += [k * sg + i * (nx + 1) for i in range(nx)]
        if k < N - 1:
            idx += [k * sg + nx * nx + i * (nu + 1) for i in range(nu)]
    return np.array(idx)


def add_rho(nx, nu, N, G, rho):
    """fp64 copy of the packed G [B, szG] with rho_b on every diagonal."""
    out = np.array(G, dtype=F64)
    out[:, diag_index(nx, nu, N)] += np.asarray(rho, F64)[:, None]
    return out


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def problem(nx, nu, N, B, seed=None, psd=False):
    """fp32 numbers held in fp64.  psd: the lower half of the eigenvalues of every cost block (at least one) set to zero."""
    seed = 700 + nx + N if seed is None else seed
    d = so.gen(nx, nu, N, seed=seed, batch=B, dtype=F64)
    if psd:
        sg = nx * nx + nu * nu
        for b in range(B):
            for k in range(N):
                for off, m in ((k * sg, nx),) + (((k * sg + nx * nx, nu),) if k < N - 1 else ()):
                    M = d["G"][b, off:off + m * m].reshape(m, m)
                    w, v = np.linalg.eigh(0.5 * (M + M.T))
                    w[:max(1, m // 2)] = 0.0
                    d["G"][b, off:off + m * m] = ((v * w) @ v.T).reshape(-1)
    d = {k: v.astype(F32).astype(F64) for k, v in d.items()}
    frozen(*d.values())
    return d


@functools.lru_cache(maxsize=None)
def form_reference(nx, nu, N, B, seed=None, psd=False, rho=None):
    """(rho [B], G + rho I [B, szG], [(S, gamma, Ginv)] per problem) in fp64, computed once and shared."""
    d = problem(nx, nu, N, B, seed, psd)
    rho = rho_default(B) if rho is None else np.full(B, rho, F64)
    Gr = add_rho(nx, nu, N, d["G"], rho)
    parts = [so.form_schur(nx, nu, N, Gr[b], d["C"][b], d["g"][b], d["c"][b]) for b in range(B)]
    frozen(rho, Gr, *(a for p in parts for a in p))
    return rho, Gr, parts


def device_data(d, dtype, N):
    G, C, g, c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
    return G, (None if N == 1 else C), g, c   # N == 1: there is no C


def check_form(S, gamma, Ginv, parts, nx, N, dtype, what):
    """S, gamma, G^-1 [B, -1] of the device against the fp64 parts; S symmetric in storage bit for bit."""
    tol = FORM_TOL[dtype]
    for b, (oS, og, oGi) in enumerate(parts):
        print(f"{what} problem {b}: S {relerr(S[b], oS):.3e} gamma {relerr(gamma[b], og):.3e} Ginv {relerr(Ginv[b], oGi):.3e} (tol {tol:.0e})")
        assert np.isfinite(S[b]).all() and np.isfinite(gamma[b]).all() and np.isfinite(Ginv[b]).all(), what
        assert close(S[b], oS, tol), f"{what}: S"
        assert close(gamma[b], og, tol), f"{what}: gamma"
        assert close(Ginv[b], oGi, tol), f"{what}: Ginv"
        Sb = S[b].reshape(N, 3, nx, nx)
        assert not Sb[0, 0].any() and not Sb[N - 1, 2].any()
        for k in range(N - 1):
            assert np.array_equal(Sb[k + 1, 0], Sb[k, 2].T), f"{what}: L_{k + 1} != R_{k}'"


def host(t, B):
    return t.cpu().numpy().reshape(B, -1)


# ---- 1. formation against fp64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_form_schur_reg_vs_fp64(solver, general, nx, nu, N, B, dtype):
    d = problem(nx, nu, N, B)
    rho, _, parts = form_reference(nx, nu, N, B)
    G, C, g, c = device_data(d, dtype, N)
    G0 = G.clone()
    S, gamma, Ginv = solver.form_schur_reg(nx, nu, N, B, G, C, g, c, dev(rho.astype(dtype)))
    torch.cuda.synchronize()
    assert torch.equal(G, G0)   # the add happens on chip: G is read only
    check_form(host(S, B), host(gamma, B), host(Ginv, B), parts, nx, N, dtype, f"({nx},{nu},{N},{B}) {np.dtype(dtype).name}")


# ---- 2. rho = 0: the bits of the entry points without _reg
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_rho_zero_is_bit_identical_with_the_plain_calls(solver, general, nx, nu, N, B, dtype):
    d = problem(nx, nu, N, B)
    G, C, g, c = device_data(d, dtype, N)
    zero = torch.zeros(B, dtype=G.dtype, device="cuda")
    plain = solver.form_schur(nx, nu, N, B, G, C, g, c)
    reg = solver.form_schur_reg(nx, nu, N, B, G, C, g, c, zero)
    rng = np.random.default_rng(5)
    z, lam = dev(rng.standard_normal(g.numel()).astype(dtype)), dev(rng.standard_normal(B * nx * N).astype(dtype))
    rp = solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam)
    rr = solver.kkt_residual_reg(nx, nu, N, B, G, C, g, c, zero, z, lam)
    torch.cuda.synchronize()
    for name, a, b in zip(("S", "gamma", "Ginv"), reg, plain):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name
    assert bool(torch.isfinite(rr).all()) and torch.equal(rr.view(torch.uint8), rp.view(torch.uint8))


# ---- 3. positive semi-definite costs
PSD_SHAPES = [(14, 7, 5, 3), (2, 1, 3, 4), (3, 3, 2, 2), (14, 7, 1, 2), (12, 4, 9, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", PSD_SHAPES)
def test_semidefinite_costs_with_rho_one(solver, general, nx, nu, N, B, dtype):
    """Every Q_k and R_k has the lower half of its eigenvalues at zero (to fp32 rounding): the plain formation has nothing to
    divide by.  With rho = 1 the blocks have condition <= 31: S, gamma, G^-1 at the formation tolerances, then the whole step
    (PCG to 1e-10 / 1e-22, at most 200 iterations) against the dense fp64 solve of the regularised KKT system at 3e-4 / 1e-9."""
    d = problem(nx, nu, N, B, 40 + nx + N, True)
    rho, Gr, parts = form_reference(nx, nu, N, B, 40 + nx + N, True, 1.0)
    conds = []
    for p in range(B):
        Q, R = so.unpack(nx, nu, N, Gr[p], d["C"][p], d["g"][p], d["c"][p])[:2]
        conds += [np.linalg.cond(m) for m in Q + R]
    assert max(conds) <= 31.0
    G, C, g, c = device_data(d, dtype, N)
    rt = dev(rho.astype(dtype))
    S, gamma, Ginv = solver.form_schur_reg(nx, nu, N, B, G, C, g, c, rt)
    torch.cuda.synchronize()
    what = f"psd ({nx},{nu},{N},{B}) {np.dtype(dtype).name}"
    check_form(host(S, B), host(gamma, B), host(Ginv, B), parts, nx, N, dtype, what)
    S, gamma, Ginv = (torch.full_like(t, float("nan")) for t in (S, gamma, Ginv))
    Pinv, lam, z = torch.empty_like(S), torch.zeros_like(gamma), torch.full_like(g, float("nan"))
    it, fl = solver.kkt_step_reg(nx, nu, N, B, G, C, g, c, rt, S, gamma, Ginv, Pinv, lam, z, tol=PCG_TOL[dtype], max_iter=200)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and (it.cpu().numpy() < 200).all()
    lam, z = host(lam, B), host(z, B)
    for b in range(B):
        oz, ol = so.dense_kkt_solve(nx, nu, N, Gr[b], d["C"][b], d["g"][b], d["c"][b])
        el, ez = np.linalg.norm(lam[b] - ol) / np.linalg.norm(ol), np.linalg.norm(z[b] - oz) / np.linalg.norm(oz)
        print(f"{what} problem {b}: lambda {el:.3e} z {ez:.3e} (tol {STEP_TOL[dtype]:.0e}), max cond {max(conds):.1f}")
        assert el <= STEP_TOL[dtype] and ez <= STEP_TOL[dtype], what


# ---- 4. / 5. the step is the three calls; the graph follows rho rewritten in place
def step_buffers(nx, N, B, G, g):
    S = torch.full((B * 3 * nx * nx * N,), float("nan"), dtype=G.dtype, device="cuda")
    gamma = torch.full((B * nx * N,), float("nan"), dtype=G.dtype, device="cuda")
    lam = torch.zeros_like(gamma)
    return dict(S=S, gamma=gamma, Ginv=torch.full_like(G, float("nan")), Pinv=torch.full_like(S, float("nan")), lam=lam,
                r=torch.full_like(lam, float("nan")), p=torch.full_like(lam, float("nan")), z=torch.full_like(g, float("nan")),
                it=torch.full((B,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))


ORDER = ("S", "gamma", "Ginv", "Pinv", "lam", "r", "p", "z", "it", "fl")


def eager_step(solver, nx, nu, N, B, G, C, g, c, rho, w):
    solver.kkt_step_reg(nx, nu, N, B, G, C, g, c, rho, w["S"], w["gamma"], w["Ginv"], w["Pinv"], w["lam"], w["z"], r=w["r"], p=w["p"],
                        tol=1e-8, max_iter=100, iters=w["it"], max_iter_exit=w["fl"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 9), (5, 3, 10, 4)])
def test_kkt_step_reg_is_the_three_calls(solver, general, nx, nu, N, B, dtype):
    """form_schur_reg -> form_pinv_solve -> recover_primal issued one by one: the same kernels on the same numbers."""
    d = problem(nx, nu, N, B, 31)
    G, C, g, c = device_data(d, dtype, N)
    rho = dev(rho_default(B).astype(dtype))
    a = step_buffers(nx, N, B, G, g)
    solver.form_schur_reg(nx, nu, N, B, G, C, g, c, rho, S=a["S"], gamma=a["gamma"], Ginv=a["Ginv"])
    solver.form_pinv_solve(nx, N, B, a["S"], a["Pinv"], a["gamma"], a["lam"], r=a["r"], p=a["p"], tol=1e-8, max_iter=100, iters=a["it"],
                           max_iter_exit=a["fl"])
    solver.recover_primal(nx, nu, N, B, a["Ginv"], C, g, a["lam"], z=a["z"])
    b = step_buffers(nx, N, B, G, g)
    eager_step(solver, nx, nu, N, B, G, C, g, c, rho, b)
    torch.cuda.synchronize()
    for k in ORDER:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert int(b["fl"].sum()) == 0 and int(b["it"].min()) > 0 and bool(torch.isfinite(b["z"]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_follows_rho_rewritten_in_place(solver, dtype):
    nx, nu, N, B = 14, 7, 24, 9
    d = problem(nx, nu, N, B, 31)
    G, C, g, c = device_data(d, dtype, N)
    rho = dev(rho_default(B).astype(dtype))
    rho2 = dev((3.0 - 0.25 * np.arange(B)).astype(dtype))
    w = step_buffers(nx, N, B, G, g)
    solver.reserve(G.element_size(), nx, N, B)
    gr = solver.graph_kkt_step_reg(nx, nu, N, B, G, C, g, c, rho, w["S"], w["gamma"], w["Ginv"], w["Pinv"], w["lam"], w["r"], w["p"],
                                   1e-8, 100, w["it"], w["fl"], w["z"])
    gr.launch()
    torch.cuda.synchronize()
    first = {k: w[k].clone() for k in ORDER}
    e = step_buffers(nx, N, B, G, g)
    eager_step(solver, nx, nu, N, B, G, C, g, c, rho, e)
    torch.cuda.synchronize()
    for k in ORDER:
        assert torch.equal(first[k].view(torch.uint8), e[k].view(torch.uint8)), k
    rho.copy_(rho2)          # in place: the graph holds the pointer
    w["lam"].zero_()
    gr.launch()
    torch.cuda.synchronize()
    e = step_buffers(nx, N, B, G, g)
    eager_step(solver, nx, nu, N, B, G, C, g, c, rho2, e)
    torch.cuda.synchronize()
    for k in ORDER:
        assert torch.equal(w[k].view(torch.uint8), e[k].view(torch.uint8)), k
    for k in ("S", "gamma", "Ginv", "Pinv", "lam", "z"):
        assert not torch.equal(w[k], first[k]), k
    gr.close()


# ---- 6. isolation between the problems of a batch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N", [(14, 7, 9), (14, 7, 3), (2, 1, 5), (5, 3, 4)])
def test_rho_of_one_problem_touches_that_problem_only(solver, general, nx, nu, N, dtype):
    B = 3
    d = problem(nx, nu, N, B)
    G, C, g, c = device_data(d, dtype, N)
    rho = dev(rho_default(B).astype(dtype))
    base = [host(t, B) for t in solver.form_schur_reg(nx, nu, N, B, G, C, g, c, rho)]
    for new in (7.25, float("nan")):
        r2 = rho.clone()
        r2[1] = new
        out = [host(t, B) for t in solver.form_schur_reg(nx, nu, N, B, G, C, g, c, r2)]
        for name, a, b in zip(("S", "gamma", "Ginv"), out, base):
            for p in (0, 2):
                assert np.array_equal(a[p].view(np.uint8), b[p].view(np.uint8)), (name, p, new)
            assert not np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8)), (name, new)
        if new != new:
            assert not np.isfinite(out[0][1]).all()


# ---- 7. the device's own symmetry test
@pytest.mark.parametrize("nx,nu,N,B,dtype", [(14, 7, 9, 2, F32), (12, 4, 33, 2, F64)])
def test_regularised_S_passes_check_symmetric(solver, nx, nu, N, B, dtype):
    d = problem(nx, nu, N, B)
    G, C, g, c = device_data(d, dtype, N)
    S, _, _ = solver.form_schur_reg(nx, nu, N, B, G, C, g, c, dev(rho_default(B).astype(dtype)))
    flags = solver.check_symmetric(nx, N, B, S)
    torch.cuda.synchronize()
    assert flags.cpu().numpy().tolist() == [1] * B


# ---- 8. the entry points that work on the G^-1, S and Pinv of a regularised step
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 4), (5, 3, 10, 4)])
def test_form_gamma_and_kkt_resolve_on_a_regularised_factorisation(solver, nx, nu, N, B, dtype):
    d, d2 = problem(nx, nu, N, B, 41), problem(nx, nu, N, B, 42)
    rho = rho_default(B)
    Gr = add_rho(nx, nu, N, d["G"], rho)
    G, C, g, c = device_data(d, dtype, N)
    w = step_buffers(nx, N, B, G, g)
    it, fl = solver.kkt_step_reg(nx, nu, N, B, G, C, g, c, dev(rho.astype(dtype)), w["S"], w["gamma"], w["Ginv"], w["Pinv"], w["lam"],
                                 w["z"], tol=PCG_TOL[dtype], max_iter=200)
    g2, c2 = dev(d2["g"].astype(dtype).reshape(-1)), dev(d2["c"].astype(dtype).reshape(-1))
    gam2 = solver.form_gamma(nx, nu, N, B, w["Ginv"], C, g2, c2)
    lam, z, gam3 = torch.zeros_like(w["lam"]), torch.full_like(w["z"], float("nan")), torch.full_like(gam2, float("nan"))
    it2, fl2 = solver.kkt_resolve(nx, nu, N, B, w["Ginv"], C, g2, c2, w["S"], w["Pinv"], gam3, lam, z, tol=PCG_TOL[dtype], max_iter=200)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and not fl2.cpu().numpy().any() and (it2.cpu().numpy() < 200).all()
    assert torch.equal(gam2, gam3)
    gam2, lam, z = host(gam2, B), host(lam, B), host(z, B)
    for b in range(B):
        og = so.form_schur(nx, nu, N, Gr[b], d["C"][b], d2["g"][b], d2["c"][b])[1]
        oz, ol = so.dense_kkt_solve(nx, nu, N, Gr[b], d["C"][b], d2["g"][b], d2["c"][b])
        el, ez = np.linalg.norm(lam[b] - ol) / np.linalg.norm(ol), np.linalg.norm(z[b] - oz) / np.linalg.norm(oz)
        print(f"downstream ({nx},{nu},{N},{B}) {np.dtype(dtype).name} problem {b}: gamma {relerr(gam2[b], og):.3e} lambda {el:.3e} z {ez:.3e}")
        assert close(gam2[b], og, FORM_TOL[dtype])
        assert el <= STEP_TOL[dtype] and ez <= STEP_TOL[dtype]


# ---- 9. the residual of the regularised system
def roundoff(dtype):
    return 2.0 ** -24 if dtype == F32 else 2.0 ** -53


def evaluate(nx, nu, N, d, Gpacked, z, lam):
    """fp64 norms [B, 2] of (Gpacked z + g + C' lambda, C z - c) and the magnitudes the bounds scale with [B, 2]."""
    B = z.shape[0]
    ref, mag = np.zeros((B, 2)), np.zeros((B, 2))
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, Gpacked[b], d["C"][b], d["g"][b], d["c"][b])
        zb, lb = np.asarray(z[b], F64), np.asarray(lam[b], F64)
        rs, rf = Gd @ zb + g + Cd.T @ lb, Cd @ zb - c
        ref[b] = np.abs(rs).max(), np.abs(rf).max()
        aC = np.abs(Cd)
        mag[b] = (np.abs(Gd) @ np.abs(zb) + np.abs(g) + aC.T @ np.abs(lb)).max(), (aC @ np.abs(zb) + np.abs(c)).max()
    return ref, mag


def bounds(mag, nx, nu, dtype):
    u = roundoff(dtype)
    return np.stack([(2 * nx + 2) * u * mag[:, 0], (nx + nu + 2) * u * mag[:, 1]], axis=1)


def within_bounds(res, ref, mag, nx, nu, dtype, what, lower):
    res = np.asarray(res, F64).reshape(-1, 2)
    tol = bounds(mag, nx, nu, dtype)
    for b in range(res.shape[0]):
        err = np.abs(res[b] - ref[b])
        print(f"{what} problem {b}: stationarity {res[b, 0]:.6e} (ref {ref[b, 0]:.6e}, err {err[0]:.2e}, bound {tol[b, 0]:.2e})  "
              f"feasibility {res[b, 1]:.6e} (ref {ref[b, 1]:.6e}, err {err[1]:.2e}, bound {tol[b, 1]:.2e})")
        assert np.isfinite(res[b]).all(), what
        assert err[0] <= tol[b, 0] and err[1] <= tol[b, 1], what
        if lower:
            assert res[b, 0] > 0.5 * ref[b, 0] and res[b, 1] > 0.5 * ref[b, 1], what


@functools.lru_cache(maxsize=None)
def residual_points(nx, nu, N, B):
    """The three fp64 points of tests/test_gpu_kkt_residual.py for the REGULARISED system."""
    d = problem(nx, nu, N, B)
    _, Gr, _ = form_reference(nx, nu, N, B)
    rng = np.random.default_rng(900 + nx + N)
    sol = [so.dense_kkt_solve(nx, nu, N, Gr[b], d["C"][b], d["g"][b], d["c"][b]) for b in range(B)]
    z0, l0 = np.stack([s[0] for s in sol]), np.stack([s[1] for s in sol])
    pts = [(z0, l0), (z0 + 1e-3 * rng.standard_normal(z0.shape), l0 + 1e-3 * rng.standard_normal(l0.shape)),
           (rng.standard_normal(z0.shape), rng.standard_normal(l0.shape))]
    frozen(*(v for p in pts for v in p))
    return pts


@functools.lru_cache(maxsize=None)
def residual_reference(nx, nu, N, B, dtype, kind):
    d = problem(nx, nu, N, B)
    _, Gr, _ = form_reference(nx, nu, N, B)
    z, lam = (np.ascontiguousarray(v.astype(dtype)) for v in residual_points(nx, nu, N, B)[kind])
    ref, mag = evaluate(nx, nu, N, d, Gr, z, lam)
    frozen(z, lam, ref, mag)
    return z, lam, ref, mag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_kkt_residual_reg_vs_fp64(solver, general, nx, nu, N, B, dtype):
    d = problem(nx, nu, N, B)
    G, C, g, c = device_data(d, dtype, N)
    rho = dev(rho_default(B).astype(dtype))
    for kind, name in enumerate(POINTS):
        z, lam, ref, mag = residual_reference(nx, nu, N, B, dtype, kind)
        res = solver.kkt_residual_reg(nx, nu, N, B, G, C, g, c, rho, dev(z.reshape(-1)), dev(lam.reshape(-1)))
        torch.cuda.synchronize()
        assert tuple(res.shape) == (B, 2) and res.dtype == G.dtype
        within_bounds(res.cpu().numpy(), ref, mag, nx, nu, dtype, f"({nx},{nu},{N},{B}) {np.dtype(dtype).name} {name}", lower=kind > 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 4), (4, 6, 3, 2)])
def test_residuals_of_the_step_kkt_step_reg_wrote(solver, general, nx, nu, N, B, dtype):
    """The regularised stationarity of the regularised step is at rounding level; the plain kkt_residual of the same point is
    about rho |z| -- at least half the fp64 value of ||rho z||_inf minus its bound, so the two calls are not one kernel."""
    d = problem(nx, nu, N, B, 41)
    rho = rho_default(B)
    Gr = add_rho(nx, nu, N, d["G"], rho)
    G, C, g, c = device_data(d, dtype, N)
    rt = dev(rho.astype(dtype))
    w = step_buffers(nx, N, B, G, g)
    it, fl = solver.kkt_step_reg(nx, nu, N, B, G, C, g, c, rt, w["S"], w["gamma"], w["Ginv"], w["Pinv"], w["lam"], w["z"],
                                 tol=PCG_TOL[dtype], max_iter=200)
    reg = solver.kkt_residual_reg(nx, nu, N, B, G, C, g, c, rt, w["z"], w["lam"])
    plain = solver.kkt_residual(nx, nu, N, B, G, C, g, c, w["z"], w["lam"])
    torch.cuda.synchronize()
    assert int(fl.sum()) == 0
    z, lam = host(w["z"], B), host(w["lam"], B)
    what = f"after kkt_step_reg ({nx},{nu},{N},{B}) {np.dtype(dtype).name}"
    ref, mag = evaluate(nx, nu, N, d, Gr, z, lam)
    within_bounds(reg.cpu().numpy(), ref, mag, nx, nu, dtype, what + " reg", lower=False)
    refp, magp = evaluate(nx, nu, N, d, d["G"], z, lam)
    within_bounds(plain.cpu().numpy(), refp, magp, nx, nu, dtype, what + " plain", lower=False)
    plain, tol = plain.cpu().numpy().astype(F64), bounds(magp, nx, nu, dtype)
    for b in range(B):
        rz = rho[b] * np.abs(z[b].astype(F64)).max()
        print(f"{what} problem {b}: plain stationarity {plain[b, 0]:.3e}, ||rho z||_inf {rz:.3e}, reg {float(reg[b, 0]):.3e}")
        assert plain[b, 0] > 0.5 * rz - tol[b, 0]


# ---- 10. arguments
@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
@pytest.mark.parametrize("name", ["form_schur_reg", "kkt_step_reg", "graph_create_kkt_step_reg", "kkt_residual_reg"])
def test_null_rho_and_refused_shapes(solver, name, suf, tt):
    nx, nu, N, B = 6, 3, 4, 3
    buf = torch.zeros(1 << 16, dtype=tt, device="cuda")
    buf[:B] = 1.0   # (rho, where it is read: zero Hessians + 1)
    outs = [torch.full((1 << 14,), 777.0, dtype=tt, device="cuda") for _ in range(8)]
    it = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    P = ctypes.c_void_p(buf.data_ptr())
    O = [ctypes.c_void_p(t.data_ptr()) for t in outs]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = getattr(solver.lib, f"gbdpcg_{name}_{suf}")
    graph = ctypes.c_void_p()

    def call(rho, nx=nx, nu=nu):
        head = (solver.h, nx, nu, N, B, P, P, P, P, rho)
        if name == "form_schur_reg":
            return fn(*head, O[0], O[1], O[2], s)
        if name == "kkt_residual_reg":
            return fn(*head, P, P, O[0], s)
        last = ctypes.byref(graph) if name.startswith("graph") else s
        return fn(*head, O[0], O[1], O[2], O[3], binding.PINV_STAIR, O[4], O[5], O[6], 1e-6, 10, ctypes.c_void_p(it.data_ptr()), None,
                  O[7], last)

    assert call(None) == 1
    # a block size whose working set does not fit one compute unit's LDS: refused like form_schur refuses it
    assert (call(P, nx=80, nu=40) if suf == "f64" else call(P, nx=120, nu=60)) == 4
    torch.cuda.synchronize()
    assert not graph.value
    assert all(bool((t == 777.0).all()) for t in outs) and bool((it == 777).all())
    for t in outs[4:7]:
        t.zero_()    # lambda, r, p of the step: a start the solve can use
    assert call(P) == 0
    if graph.value:
        assert solver.lib.gbdpcg_graph_launch(graph, s) == 0
    torch.cuda.synchronize()
    if graph.value:
        solver.lib.gbdpcg_graph_destroy(graph)
    n_out = {"form_schur_reg": B * 3 * nx * nx * N, "kkt_residual_reg": 2 * B}.get(name, B * 3 * nx * nx * N)
    assert bool(torch.isfinite(outs[0][:n_out]).all()) and not bool((outs[0][:n_out] == 777.0).any())
    assert bool((outs[0][n_out:] == 777.0).all())
