"""KKT residual norms on the device (csrc/schur_residual.hip schur_residual_kernel / schur_residual_quad_kernel, through the C ABI):
res[b] = (||G z + g + C' lambda||_inf, ||C z - c||_inf) per problem.  PARITY UNPINNED: the reference tree has no code, fixture or
output for this step.

Reference: fp64 numpy on oracle.schur_oracle.dense_kkt of the SAME inputs (the problem data are fp32 numbers, exact in either
precision; the point is the one the device gets, cast up): rs = Gd z + g + Cd' lambda, rf = Cd z - c, norms max|rs|, max|rf|.

Tolerance, derived and not tuned: with unit roundoff u (2^-24 / 2^-53)
    |dev - ref| <= (2 nx + 2) u max_i (|Gd||z| + |g| + |Cd'||lambda|)_i        stationarity
    |dev - ref| <= (nx + nu + 2) u max_i (|Cd||z| + |c|)_i                      feasibility
the dot-product bound for the number of terms in a row, valid for any order of summation (a row of the x-part has nx + 1 + 1 + nx
terms, a row of the dynamics 1 + nx + nu + 1).

Points: the fp64 solution of the KKT system cast down (both norms at rounding level), that point + 1e-3 noise, and a random
point of order 1; at the last two the device norm must also exceed half the reference, so zeros or a dropped term cannot pass."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [(14, 7, 128, 3), (14, 7, 1, 2), (14, 7, 2, 1), (2, 1, 5, 4), (3, 3, 2, 1), (5, 2, 9, 2), (12, 4, 33, 2), (4, 6, 3, 2),
          (36, 18, 6, 1), (1, 1, 4, 1), (44, 3, 3, 1)]   # SHAPES of tests/test_gpu_resolve.py
QUAD_SHAPES = [(2, 1), (4, 1), (4, 2), (6, 3), (8, 4), (10, 5), (12, 4), (12, 6), (13, 4), (3, 1), (5, 2), (6, 1), (6, 2), (7, 3), (8, 2), (9, 3),
               (10, 4), (11, 4), (12, 3), (14, 7)]   # GBDPCG_QUAD_SHAPES of csrc/schur_common.hpp
QUAD_NB = [(1, 2), (2, 3), (3, 1), (5, 3), (7, 11), (16, 5)]   # rows, waves and workgroups partly empty, problems that straddle waves
POINTS = ("solution", "solution + 1e-3 noise", "random")


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the cached references are read-only)


def roundoff(dtype):
    return 2.0 ** -24 if dtype == F32 else 2.0 ** -53


@functools.lru_cache(maxsize=None)
def problem(nx, nu, N, B, seed=None):
    """Problem data (fp32 numbers held in fp64: exact in both precisions) and the three fp64 points per problem, computed once."""
    seed = 300 + nx + N if seed is None else seed
    d = {k: v.astype(F64) for k, v in so.gen(nx, nu, N, seed=seed, batch=B, dtype=F32).items()}
    rng = np.random.default_rng(seed + 1)
    sol = [so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b]) for b in range(B)]
    z0, l0 = np.stack([s[0] for s in sol]), np.stack([s[1] for s in sol])
    pts = [(z0, l0),
           (z0 + 1e-3 * rng.standard_normal(z0.shape), l0 + 1e-3 * rng.standard_normal(l0.shape)),
           (rng.standard_normal(z0.shape), rng.standard_normal(l0.shape))]
    for v in d.values():
        v.setflags(write=False)
    for p in pts:
        for v in p:
            v.setflags(write=False)
    return d, pts


def evaluate(nx, nu, N, d, z, lam):
    """fp64 reference for points z [B, nz], lam [B, nx N]: (norms [B, 2], magnitudes the bounds scale with [B, 2])."""
    B = z.shape[0]
    ref, mag = np.zeros((B, 2)), np.zeros((B, 2))
    shared = d["G"].shape[0] == 1
    for b in range(B):
        m = 0 if shared else b
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][m], d["C"][m], d["g"][b], d["c"][b])
        zb, lb = np.asarray(z[b], F64), np.asarray(lam[b], F64)
        rs, rf = Gd @ zb + g + Cd.T @ lb, Cd @ zb - c
        ref[b] = np.abs(rs).max(), np.abs(rf).max()
        aC = np.abs(Cd)
        mag[b] = (np.abs(Gd) @ np.abs(zb) + np.abs(g) + aC.T @ np.abs(lb)).max(), (aC @ np.abs(zb) + np.abs(c)).max()
    return ref, mag


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, dtype, kind):
    """The point of this kind as the device gets it (cast to dtype) and its fp64 reference, computed once and shared."""
    d, pts = problem(nx, nu, N, B)
    z, lam = (np.ascontiguousarray(v.astype(dtype)) for v in pts[kind])
    ref, mag = evaluate(nx, nu, N, d, z, lam)
    for v in (z, lam, ref, mag):
        v.setflags(write=False)
    return z, lam, ref, mag


def device_data(nx, nu, N, B, dtype):
    d, _ = problem(nx, nu, N, B)
    G, C, g, c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
    return G, (None if N == 1 else C), g, c   # N == 1: there is no C


def within_bounds(res, ref, mag, nx, nu, dtype, what, lower):
    res = np.asarray(res, F64).reshape(-1, 2)
    u = roundoff(dtype)
    for b in range(res.shape[0]):
        err = np.abs(res[b] - ref[b])
        tol = np.array([(2 * nx + 2) * u * mag[b, 0], (nx + nu + 2) * u * mag[b, 1]])
        print(f"{what} problem {b}: stationarity {res[b, 0]:.6e} (ref {ref[b, 0]:.6e}, err {err[0]:.2e}, bound {tol[0]:.2e})  "
              f"feasibility {res[b, 1]:.6e} (ref {ref[b, 1]:.6e}, err {err[1]:.2e}, bound {tol[1]:.2e})")
        assert np.isfinite(res[b]).all(), what
        assert err[0] <= tol[0] and err[1] <= tol[1], what
        if lower:
            assert res[b, 0] > 0.5 * ref[b, 0] and res[b, 1] > 0.5 * ref[b, 1], what


def run_case(solver, nx, nu, N, B, dtype):
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    for kind, name in enumerate(POINTS):
        z, lam, ref, mag = reference(nx, nu, N, B, dtype, kind)
        res = solver.kkt_residual(nx, nu, N, B, G, C, g, c, dev(z.reshape(-1)), dev(lam.reshape(-1)))
        torch.cuda.synchronize()
        assert tuple(res.shape) == (B, 2) and res.dtype == G.dtype
        within_bounds(res.cpu().numpy(), ref, mag, nx, nu, dtype, f"({nx},{nu},{N},{B}) {np.dtype(dtype).name} {name}", lower=kind > 0)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_general_kernel_vs_fp64(solver, monkeypatch, nx, nu, N, B, dtype):
    """schur_residual_kernel at every shape (N = 1 without C, nu > nx, 36 / 18, 44 / 3 among them)."""
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    run_case(solver, nx, nu, N, B, dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_default_dispatch_vs_fp64(solver, nx, nu, N, B, dtype):
    """The same shapes through the kernel the launcher picks by itself."""
    run_case(solver, nx, nu, N, B, dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("N,B", QUAD_NB)
@pytest.mark.parametrize("nx,nu", QUAD_SHAPES)
def test_quad_kernel_vs_fp64(solver, nx, nu, N, B, dtype):
    """schur_residual_quad_kernel for every block size it is built for; quarters, waves and the workgroup partly empty."""
    run_case(solver, nx, nu, N, B, dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("N,B", [(1, 1), (3, 1), (37, 3), (5, 13)])
@pytest.mark.parametrize("nx,nu", [(14, 7), (13, 4), (2, 1), (9, 3)])
def test_quad_kernel_is_bit_identical_with_the_general_one(solver, monkeypatch, nx, nu, N, B, dtype):
    """Every residual entry is the same fma chain in both kernels and a maximum is exact: the same bits."""
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    for kind in range(3):
        z, lam, ref, mag = reference(nx, nu, N, B, dtype, kind)
        z, lam = dev(z.reshape(-1)), dev(lam.reshape(-1))
        rq = solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam)
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
        rg = solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam)
        monkeypatch.delenv("GBDPCG_SCHUR_GENERAL")
        torch.cuda.synchronize()
        assert np.array_equal(rq.cpu().numpy().view(np.uint8), rg.cpu().numpy().view(np.uint8)), POINTS[kind]
        within_bounds(rq.cpu().numpy(), ref, mag, nx, nu, dtype, f"quad ({nx},{nu},{N},{B}) {POINTS[kind]}", lower=kind > 0)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_overwrites_whatever_res_held(solver, monkeypatch, dtype, general):
    """No initialisation outside the launch and no dependence on the old contents: NaN-filled res, two calls, then 1e30."""
    nx, nu, N, B = 14, 7, 37, 3
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    z, lam, ref, mag = reference(nx, nu, N, B, dtype, 1)
    z, lam = dev(z.reshape(-1)), dev(lam.reshape(-1))
    res = torch.full((B, 2), float("nan"), dtype=G.dtype, device="cuda")
    out = []
    for fill in (None, None, 1e30):
        if fill is not None:
            res.fill_(fill)
        solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam, res=res)
        torch.cuda.synchronize()
        out.append(res.cpu().numpy().copy())
    within_bounds(out[0], ref, mag, nx, nu, dtype, "NaN-filled res", lower=True)
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
    assert np.array_equal(out[0].view(np.uint8), out[2].view(np.uint8))


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_where_the_maximum_sits(solver, monkeypatch, dtype, general):
    """10 added to one entry of z at the first knot, at the last knot and at a u entry in the middle: the norms follow the
    reference each time, so a kernel that skips row 0, the last row or the u-part fails."""
    nx, nu, N, B = 14, 7, 37, 3
    sv = nx + nu
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    d, _ = problem(nx, nu, N, B)
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    z0, lam0, _, _ = reference(nx, nu, N, B, dtype, 0)
    for where, (b, i) in (("first knot", (1, 3)), ("last knot", (2, (N - 1) * sv + 5)), ("middle u", (0, 18 * sv + nx + 2))):
        z = z0.copy()
        z[b, i] += 10
        ref, mag = evaluate(nx, nu, N, d, z, lam0)
        assert ref[b, 0] > 5   # the bump is the maximum of that problem (the cost blocks have eigenvalues >= 1)
        res = solver.kkt_residual(nx, nu, N, B, G, C, g, c, dev(z.reshape(-1)), dev(lam0.reshape(-1)))
        torch.cuda.synchronize()
        res = res.cpu().numpy()
        within_bounds(res, ref, mag, nx, nu, dtype, f"+10 at {where}", lower=False)
        assert res[b, 0] > 0.5 * ref[b, 0] and res[b, 1] > 0.5 * ref[b, 1]


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_nan_and_inf_propagate_inside_their_problem(solver, monkeypatch, dtype, general):
    """A NaN in one x entry of problem 1 at a middle knot makes both of its norms NaN (the maximum must not drop it); an Inf in
    g or c gives Inf in the norm it enters and leaves the other alone; problems 0 and 2 keep the bits of the clean run."""
    nx, nu, N, B = 14, 7, 37, 3
    sv = nx + nu
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    z, lam, _, _ = reference(nx, nu, N, B, dtype, 1)
    z, lam = dev(z.reshape(-1)), dev(lam.reshape(-1))
    clean = solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam).cpu().numpy()
    nz = z.numel() // B

    def same_elsewhere(r):
        for b in (0, 2):
            assert np.array_equal(r[b].view(np.uint8), clean[b].view(np.uint8)), b

    zn = z.clone()
    zn[nz + 18 * sv + 4] = float("nan")
    r = solver.kkt_residual(nx, nu, N, B, G, C, g, c, zn, lam).cpu().numpy()
    assert np.isnan(r[1]).all(), r
    same_elsewhere(r)
    gi = g.clone()
    gi[nz + 20 * sv + nx + 1] = float("inf")     # a u-part gradient: stationarity only
    r = solver.kkt_residual(nx, nu, N, B, G, C, gi, c, z, lam).cpu().numpy()
    assert np.isposinf(r[1, 0]) and np.array_equal(r[1, 1:].view(np.uint8), clean[1, 1:].view(np.uint8)), r
    same_elsewhere(r)
    ci = c.clone()
    ci[N * nx + 9 * nx + 2] = float("-inf")      # feasibility only
    r = solver.kkt_residual(nx, nu, N, B, G, C, g, ci, z, lam).cpu().numpy()
    assert np.isposinf(r[1, 1]) and np.array_equal(r[1, :1].view(np.uint8), clean[1, :1].view(np.uint8)), r
    same_elsewhere(r)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 9), (5, 3, 10, 4)])
def test_shared_twin(solver, monkeypatch, nx, nu, N, B, dtype, general):
    """One problem's G and C (exactly one problem's extent, NaN behind and in front of it) against the per-problem call on B
    copies: bit for bit, and finite -- nothing outside the single extent is read."""
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    d, pts = problem(nx, nu, N, B)
    g, c = dev(d["g"].astype(dtype).reshape(-1)), dev(d["c"].astype(dtype).reshape(-1))
    z, lam = (dev(v.astype(dtype).reshape(-1)) for v in pts[2])
    single = []
    for M in (d["G"][0], d["C"][0]):
        buf = torch.full((1024 + 3 * M.size,), float("nan"), dtype=g.dtype, device="cuda")
        buf[1024:1024 + M.size] = dev(M.astype(dtype))
        single.append((buf, buf[1024:1024 + M.size]))
    G1, C1 = single[0][1], single[1][1]
    rs = solver.kkt_residual_shared(nx, nu, N, B, G1, C1, g, c, z, lam)
    rr = solver.kkt_residual(nx, nu, N, B, G1.repeat(B), C1.repeat(B), g, c, z, lam)
    r1 = solver.kkt_residual_shared(nx, nu, N, 1, G1, C1, g, c, z, lam)     # batch = 1 is the twin
    torch.cuda.synchronize()
    rs, rr, r1 = rs.cpu().numpy(), rr.cpu().numpy(), r1.cpu().numpy()
    assert tuple(rs.shape) == (B, 2) and np.isfinite(rs).all()
    assert np.array_equal(rs.view(np.uint8), rr.view(np.uint8))
    assert np.array_equal(r1.view(np.uint8), rr[:1].view(np.uint8))
    dsh = {"G": d["G"][:1], "C": d["C"][:1], "g": d["g"], "c": d["c"]}
    ref, mag = evaluate(nx, nu, N, dsh, z.cpu().numpy().reshape(B, -1), lam.cpu().numpy().reshape(B, -1))
    within_bounds(rs, ref, mag, nx, nu, dtype, f"shared ({nx},{nu},{N},{B})", lower=True)


def factor(solver, nx, nu, N, B, dtype):
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    S, _, Ginv = solver.form_schur(nx, nu, N, B, G, C, g, c)
    Pinv = solver.form_pinv(nx, N, B, S, binding.PINV_STAIR)
    return G, C, g, c, S, Ginv, Pinv


@pytest.mark.parametrize("dtype", [F32, F64])
def test_under_a_graph_behind_kkt_resolve(solver, dtype):
    """Captured on the caller's stream behind gbdpcg_kkt_resolve_*: every replay gives the bits of the eager pair of calls,
    with the buffers the step writes (z, res) and the multipliers it starts from rewritten between replays."""
    nx, nu, N, B = 14, 7, 24, 9
    G, C, g, c, S, Ginv, Pinv = factor(solver, nx, nu, N, B, dtype)
    gamma = torch.empty(B * nx * N, dtype=G.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    res = torch.empty(B, 2, dtype=G.dtype, device="cuda")
    starts = [torch.zeros_like(lam), dev(0.1 * np.random.default_rng(8).standard_normal(lam.numel()).astype(dtype))]
    solver.reserve(S.element_size(), nx, N, B)

    def step():
        solver.kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, tol=1e-8, max_iter=100, iters=it, max_iter_exit=fl)
        solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam, res=res)

    want = []
    for start in starts:
        lam.copy_(start)
        step()
        torch.cuda.synchronize()
        want.append([t.clone() for t in (res, lam, z)])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):     # the capturing stream is torch's current one inside the block
        step()
    for start, (wres, wlam, wz) in zip(starts, want):
        lam.copy_(start)
        z.fill_(float("nan"))
        res.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lam, wlam) and torch.equal(z, wz)
        assert bool(torch.isfinite(res).all()) and torch.equal(res.view(torch.uint8), wres.view(torch.uint8))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_after_a_real_step(solver, dtype):
    """gbdpcg_kkt_step_* at tol 1e-8, then the norms of the step it wrote against the fp64 reference at that (z, lambda)."""
    nx, nu, N, B = 14, 7, 24, 9
    d, _ = problem(nx, nu, N, B)
    G, C, g, c = device_data(nx, nu, N, B, dtype)
    S = torch.empty(B * 3 * nx * nx * N, dtype=G.dtype, device="cuda")
    Pinv, Ginv = torch.empty_like(S), torch.empty_like(G)
    gamma = torch.empty(B * nx * N, dtype=G.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it, fl = solver.kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=1e-8, max_iter=100)
    res = solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam)
    torch.cuda.synchronize()
    assert int(fl.sum()) == 0
    ref, mag = evaluate(nx, nu, N, d, z.cpu().numpy().reshape(B, -1), lam.cpu().numpy().reshape(B, -1))
    within_bounds(res.cpu().numpy(), ref, mag, nx, nu, dtype, f"after kkt_step {np.dtype(dtype).name}", lower=False)


@pytest.mark.parametrize("name", ["kkt_residual", "kkt_residual_shared"])
@pytest.mark.parametrize("suf,tdt", [("f32", torch.float32), ("f64", torch.float64)])
def test_bad_arguments(solver, name, suf, tdt):
    nx, nu, N, B = 6, 3, 4, 3
    buf = torch.zeros(1 << 16, dtype=tdt, device="cuda")
    res = torch.full((2 * B,), 777.0, dtype=tdt, device="cuda")
    P, O = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = getattr(solver.lib, f"gbdpcg_{name}_{suf}")

    def args(**kw):
        a = dict(h=solver.h, nx=nx, nu=nu, N=N, batch=B, G=P, C=P, g=P, c=P, z=P, lam=P, res=O)
        a.update(kw)
        return tuple(a.values())

    for k in ("h", "G", "C", "g", "c", "z", "lam", "res"):
        assert fn(*args(**{k: None}), s) == 1, k
    for k in ("nx", "nu", "N", "batch"):
        assert fn(*args(**{k: 0}), s) == 1, k
    # a block size whose working set does not fit one compute unit's LDS: refused like form_schur refuses it
    assert fn(*args(nx=80, nu=40) if suf == "f64" else args(nx=120, nu=60), s) == 4
    torch.cuda.synchronize()
    assert bool((res == 777.0).all())
    assert fn(*args(N=1, C=None), s) == 0      # N == 1: there is no C
    assert fn(*args(), s) == 0
    torch.cuda.synchronize()
    assert bool((res == 0).all())              # all-zero inputs: both norms are 0, and they were written
