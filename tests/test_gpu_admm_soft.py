"""Soft (L1-penalised) box bounds on the device: gbdpcg_admm_soft_init_*, _update_*, _step_*, the shared twin, the graphs and
_restep_* (csrc/admm.hip's SOFT instantiations through the C ABI).  PARITY UNPINNED: the reference tree has nothing for these steps.

Reference: tests/admm_soft_ref.py.  The update is defined to the bit, so w, y and the norms are compared for EQUALITY with update_ref
in the call's precision and gt is held to the correctly rounded value of its exact fraction (admm_lin_ref.round_to).  With kappa =
+Inf every entry point must give the bits of its hard twin; the composite calls are compared bit for bit with their parts.
Convergence runs the fixtures tests/test_admm_soft_reference.py pins:
 (a) fp64: z of iterations 1, 2, 10, SOFT_K against the dense solve for the device's own gt, STEP_TOL of tests/test_gpu_admm.py;
 (b) res[2b](SOFT_K) <= SOFT_RATIO_BOUND res[2b](1): the reference's worst problem gives SOFT_RATIO_REF = 1.24e-3, the bound carries
     the headroom tests/test_gpu_admm.py gives over its reference (1e-2 against 1.5e-3) for the fp32 floor of z;
 (c) |rho y| <= kappa on every row, no solve ran out of iterations.
Run with -s for the measured figures."""
import functools
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_ref  # noqa: E402
import admm_soft_ref as sr  # noqa: E402
import test_gpu_admm as hard  # noqa: E402
from admm_lin_ref import round_to  # noqa: E402
from admm_util import dev, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_admm.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
SHAPES = [(3, 2, 4, 3),       # nz = 18: one wave, every problem base misaligned differently
          (14, 7, 24, 3)]     # nz = 497: four waves with head, body and tail


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def subnormal(dtype):
    return np.finfo(dtype).smallest_subnormal * dtype(3)


@functools.lru_cache(maxsize=None)
def soft_data(nx, nu, N, B, dtype):
    """The data of tests/test_gpu_admm.py with kappa drawn from {0, a subnormal, finite values, +Inf}, and in every problem two rows
    whose e is exactly +theta / -theta: s = +-2 theta against the bound +-theta (a doubling and its difference are exact), y = 0."""
    d = dict(hard.update_data(nx, nu, N, B, dtype))
    nz = d["z"].shape[1]
    rng = np.random.default_rng(77 + nz)
    pick = rng.integers(0, 6, (B, nz))
    kappa = np.select([pick == 0, pick == 1, pick == 2], [0.0, float(subnormal(dtype)), np.inf], rng.uniform(0.05, 1.5, (B, nz))).astype(dtype)
    z, y, lo, hi = (d[k].copy() for k in ("z", "y", "lo", "hi"))
    for b in range(B):
        for i, side in ((1, +1), (nz - 2, -1)):
            kappa[b, i] = dtype(0.75)
            theta = dtype(kappa[b, i] / d["rho"][b])
            bound = dtype(side * theta)
            lo[b, i], hi[b, i] = (-np.inf, bound) if side > 0 else (bound, np.inf)
            y[b, i] = dtype(0.0)
            z[b, i] = dtype(2.0) * bound
            assert dtype(dtype(z[b, i] + y[b, i]) - bound) == bound and abs(bound) == theta
    d.update(z=z, y=y, lo=lo, hi=hi, kappa=kappa)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def soft_reference(nx, nu, N, B, dtype, init):
    d = soft_data(nx, nu, N, B, dtype)
    return sr.update_ref(dtype, d["g"], d["lo"], d["hi"], d["kappa"], d["rho"], None if init else d["z"], d["w"], d["y"])


def run(solver, nx, nu, N, B, t, init, res=None):
    if init:
        solver.admm_soft_init(nx, nu, N, B, t["g"], t["lo"], t["hi"], t["kappa"], t["rho"], t["w"], t["y"], gt=t["gt"])
        return None
    return solver.admm_soft_update(nx, nu, N, B, t["g"], t["lo"], t["hi"], t["kappa"], t["rho"], t["z"], t["w"], t["y"], t["gt"], res=res)


def gt_rounded(gr, dtype):
    return np.array([[round_to(f, dtype) if f else dtype(0) for f in row] for row in gr], dtype)


# ---- 1. bits against update_ref, aligned and misaligned
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_update_and_init_bits(solver, nx, nu, N, B, dtype, init):
    d = soft_data(nx, nu, N, B, dtype)
    wr, yr, tr, gr, rr = soft_reference(nx, nu, N, B, dtype, init)
    outs = []
    for offset in (0, 1):
        t = hard.device_tensors(d, offset)
        assert all(t[k].data_ptr() % 16 == (0 if offset == 0 else t[k].element_size()) for k in ("g", "lo", "hi", "kappa", "z", "w", "y", "gt"))
        res = run(solver, nx, nu, N, B, t, init)
        torch.cuda.synchronize()
        w, y, gt = (t[k].cpu().numpy().reshape(B, -1) for k in ("w", "y", "gt"))
        assert np_same(w, wr), f"w (offset {offset})"
        assert np_same(y, yr), f"y (offset {offset})"
        if not init:
            assert np_same(res.cpu().numpy(), rr), f"res (offset {offset})"
        assert all(f is not None for f in gr.reshape(-1))
        assert np.array_equal(gt, gt_rounded(gr, dtype)), f"gt is not the correctly rounded fraction (offset {offset})"
        outs.append((w, y, gt))
    assert all(np_same(a, b) for a, b in zip(*outs))
    if init:
        hardrow = np.isinf(d["kappa"])
        assert np_same(wr[~hardrow], d["w"][~hardrow]) and ((wr[hardrow] >= d["lo"][hardrow]) & (wr[hardrow] <= d["hi"][hardrow])).all()
        return
    theta = (d["kappa"] / d["rho"].reshape(-1, 1)).astype(dtype)
    assert (np.abs(yr) <= theta).all()                      # the multiplier bound, by construction
    nz = wr.shape[1]
    for b in range(B):                                      # the ties took the hard branch: w on the bound, y = +-theta
        assert wr[b, 1] == d["hi"][b, 1] and yr[b, 1] == theta[b, 1] and wr[b, nz - 2] == d["lo"][b, nz - 2] and yr[b, nz - 2] == -theta[b, nz - 2]
    free = d["kappa"] == 0
    assert np_same(wr[free], (d["z"] + d["y"])[free]) and not yr[free].any()
    print(f"({nx},{nu},{N},{B}) {np.dtype(dtype).name}: {int((np.abs(yr) == theta)[~free].sum())} rows at their weight, "
          f"{int(free.sum())} free, {int(np.isinf(d['kappa']).sum())} hard")


# ---- 2. kappa = +Inf: the hard family's bits, entry point by entry point, 5 iterations
class SoftLoop(hard.Loop):
    """hard.Loop with the weights kappa (default +Inf everywhere) and the soft calls."""

    def __init__(self, *a, kappa=None, **k):
        super().__init__(*a, **k)
        self.kappa = torch.full_like(self.g, float("inf")) if kappa is None else dev(np.asarray(kappa).astype(a[5]).reshape(-1))

    def soft_start(self):
        """state() from w = y = 0 through the SOFT init (which clips only the rows with kappa = +Inf), as the references start."""
        o = self.state()
        o["w"].zero_(), o["y"].zero_(), o["lam"].zero_()
        self.s.admm_soft_init(*self.shape, self.g, self.lo, self.hi, self.kappa, self.rho, o["w"], o["y"], gt=o["gt"])
        return o

    def step_args(self, o, mats=None):
        Ginv, C, S, Pinv = mats or (self.Ginv, self.C, self.S, self.Pinv)
        return (*self.shape, Ginv, C, self.g, self.c, self.lo, self.hi, self.kappa, self.rho, S, Pinv, o["gamma"], o["lam"])

    def one_call(self, o, mats=None, shared=False):
        step = self.s.admm_soft_step_shared if shared else self.s.admm_soft_step
        step(*self.step_args(o, mats), o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=self.tol,
             max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])

    def two_calls(self, o, mats=None, shared=False):
        nx, nu, N, B = self.shape
        Ginv, C, S, Pinv = mats or (self.Ginv, self.C, self.S, self.Pinv)
        resolve = self.s.kkt_resolve_shared if shared else self.s.kkt_resolve
        resolve(nx, nu, N, B, Ginv, C, o["gt"], self.c, S, Pinv, o["gamma"], o["lam"], o["z"], r=o["r"], p=o["p"], tol=self.tol,
                max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        self.s.admm_soft_update(nx, nu, N, B, self.g, self.lo, self.hi, self.kappa, self.rho, o["z"], o["w"], o["y"], o["gt"], res=o["res"])

    def graph(self, o, mats=None, shared=False):
        make = self.s.graph_admm_soft_step_shared if shared else self.s.graph_admm_soft_step
        return make(*self.step_args(o, mats), o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])


RULE = dict(ratio=1.0, shift=1, rho_min=2.0 ** -10, rho_max=2.0 ** 10)     # ratio 1: rho moves whenever the residuals differ


def restep_buffers(L):
    """Matrices of their own (a restep rewrites Ginv, S, Pinv and rho)."""
    return dict(Ginv=L.Ginv.clone(), S=L.S.clone(), Pinv=L.Pinv.clone(), rho=L.rho.clone(),
                expo=torch.full((L.shape[3],), 99, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_kappa_gives_the_hard_bits(solver, dtype):
    nx, nu, N, B = 14, 7, 24, 3
    d = hard.step_problem(nx, nu, N, B)
    L = SoftLoop(solver, nx, nu, N, B, dtype, d, 0.5 * (np.arange(B) + 2.0))
    # init
    w = dev(hard.update_data(nx, nu, N, B, dtype)["w"].reshape(-1))
    wa, wb, ya = w.clone(), w.clone(), torch.zeros_like(w)
    ga = solver.admm_init(nx, nu, N, B, L.g, L.lo, L.hi, L.rho, wa, ya)
    gb = solver.admm_soft_init(nx, nu, N, B, L.g, L.lo, L.hi, L.kappa, L.rho, wb, ya.clone())
    assert same(wa, wb) and same(ga, gb)
    # update and step, 5 iterations each, fed by the hard loop's z
    a, b, c, e = L.state(), L.state(), L.state(), L.state()
    for _ in range(5):
        hard.one_call(L, a)
        L.one_call(b)
        c["z"].copy_(a["z"])
        solver.admm_soft_update(nx, nu, N, B, L.g, L.lo, L.hi, L.kappa, L.rho, c["z"], c["w"], c["y"], c["gt"], res=c["res"])
        solver.admm_update(nx, nu, N, B, L.g, L.lo, L.hi, L.rho, a["z"].clone(), e["w"], e["y"], e["gt"], res=e["res"])
    torch.cuda.synchronize()
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"step: {k}"
    for k in ("w", "y", "gt", "res"):
        assert same(c[k], e[k]), f"update: {k}"
    # the shared twin
    d1 = dict(d)
    d1["G"], d1["C"] = np.repeat(d["G"][:1], B, axis=0), np.repeat(d["C"][:1], B, axis=0)
    S = SoftLoop(solver, nx, nu, N, B, dtype, d1, np.full(B, 1.5))
    ng, nc, ns = S.G.numel() // B, S.C.numel() // B, S.S.numel() // B
    single = (S.Ginv[:ng].clone(), S.C[:nc].clone(), S.S[:ns].clone(), S.Pinv[:ns].clone())
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b = S.state(), S.state()
        for _ in range(5):
            hard.one_call(S, a, mats=single, shared=True)
            S.one_call(b, mats=single, shared=True)
        torch.cuda.synchronize()
    finally:
        solver.set_path(binding.PATH_AUTO)
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"shared step: {k}"
    # restep
    a, b, ma, mb = L.state(), L.state(), restep_buffers(L), restep_buffers(L)
    hard.one_call(L, a)
    L.one_call(b)
    for _ in range(5):
        solver.admm_restep(nx, nu, N, B, L.G, ma["Ginv"], L.C, L.g, L.c, L.lo, L.hi, ma["rho"], ma["S"], ma["Pinv"], a["gamma"], a["lam"],
                           a["z"], a["w"], a["y"], a["gt"], a["res"], ma["expo"], r=a["r"], p=a["p"], tol=L.tol, max_iter=L.max_iter,
                           iters=a["it"], max_iter_exit=a["fl"], **RULE)
        solver.admm_soft_restep(nx, nu, N, B, L.G, mb["Ginv"], L.C, L.g, L.c, L.lo, L.hi, L.kappa, mb["rho"], mb["S"], mb["Pinv"],
                                b["gamma"], b["lam"], b["z"], b["w"], b["y"], b["gt"], b["res"], mb["expo"], r=b["r"], p=b["p"], tol=L.tol,
                                max_iter=L.max_iter, iters=b["it"], max_iter_exit=b["fl"], **RULE)
    torch.cuda.synchronize()
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"restep: {k}"
    for k in ma:
        assert same(ma[k], mb[k]), f"restep: {k}"
    assert int(ma["expo"].abs().sum()) > 0


# ---- 4. step, graph, shared and restep identities with a finite kappa
def soft_loop(solver, dtype, shared=False):
    nx, nu, N, B = 14, 7, 24, 3
    d = dict(hard.step_problem(nx, nu, N, B))
    if shared:
        d["G"], d["C"] = np.repeat(d["G"][:1], B, axis=0), np.repeat(d["C"][:1], B, axis=0)
    L = SoftLoop(solver, nx, nu, N, B, dtype, d, np.full(B, 1.5) if shared else 0.5 * (np.arange(B) + 2.0))
    rng = np.random.default_rng(9)
    nz = L.g.numel() // B
    kap = np.where(rng.random((B, nz)) < 0.25, np.inf, rng.uniform(0.01, 0.5, (B, nz)))
    L.kappa = dev(kap.astype(dtype).reshape(-1))
    return L


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_graph_and_shared_identities(solver, dtype):
    L = soft_loop(solver, dtype)
    nx, nu, N, B = L.shape
    a, b, g = L.state(), L.state(), L.state()
    solver.reserve(L.g.element_size(), nx, N, B)
    gr = L.graph(g)
    for _ in range(3):
        L.two_calls(a)
        L.one_call(b)
        gr.launch()
    torch.cuda.synchronize()
    gr.close()
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"step vs resolve + soft update: {k}"
        assert same(b[k], g[k]), f"graph replay vs eager: {k}"
    y, theta = b["y"].view(B, -1), L.kappa.view(B, -1) / L.rho.view(B, 1)
    assert bool((y.abs() <= theta).all()) and int((y.abs() == theta).sum()) > 0, "some row must sit at its weight"
    assert int(b["fl"].sum()) == 0
    # shared: one plant, the twin against per-problem calls on tiled copies and against the graph of the twin
    S = soft_loop(solver, dtype, shared=True)
    ng, nc, ns = S.G.numel() // B, S.C.numel() // B, S.S.numel() // B
    single = (S.Ginv[:ng].clone(), S.C[:nc].clone(), S.S[:ns].clone(), S.Pinv[:ns].clone())
    copies = tuple(m.repeat(B) for m in single)
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b, c, g = S.state(), S.state(), S.state(), S.state()
        gr = S.graph(g, mats=single, shared=True)
        for _ in range(3):
            S.one_call(a, mats=copies)
            S.one_call(b, mats=single, shared=True)
            S.two_calls(c, mats=single, shared=True)
            gr.launch()
        torch.cuda.synchronize()
        gr.close()
    finally:
        solver.set_path(binding.PATH_AUTO)
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"shared vs copies: {k}"
        assert same(b[k], c[k]) and same(b[k], g[k]), f"shared step vs its parts / its graph: {k}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_restep_is_its_constituent_calls(solver, dtype):
    """gbdpcg_admm_rebalance_* (the soft box's rebalance), gbdpcg_kkt_step_reg_* on gt, gbdpcg_admm_soft_update_*; the graph form;
    |y| <= fl(kappa / rho_new) after a rebalance that moved rho."""
    L = soft_loop(solver, dtype)
    nx, nu, N, B = L.shape
    a, b, g = L.state(), L.state(), L.state()
    ma, mb, mg = restep_buffers(L), restep_buffers(L), restep_buffers(L)
    for o in (a, b, g):
        L.one_call(o)
    solver.reserve(L.g.element_size(), nx, N, B)
    gr = solver.graph_admm_soft_restep(nx, nu, N, B, L.G, mg["Ginv"], L.C, L.g, L.c, L.lo, L.hi, L.kappa, mg["rho"], mg["S"], mg["Pinv"],
                                       g["gamma"], g["lam"], g["r"], g["p"], L.tol, L.max_iter, g["it"], g["fl"], g["z"], g["w"], g["y"],
                                       g["gt"], g["res"], mg["expo"], **RULE)
    moved = 0
    for _ in range(3):
        solver.admm_rebalance(nx, nu, N, B, L.g, a["res"], ma["rho"], a["w"], a["y"], a["gt"], ma["expo"], **RULE)
        torch.cuda.synchronize()
        theta = L.kappa.view(B, -1) / ma["rho"].view(B, 1)
        assert bool((a["y"].view(B, -1).abs() <= theta).all()), "|y| <= fl(kappa / rho_new) after the rebalance"
        moved += int(ma["expo"].abs().sum())
        solver.kkt_step_reg(nx, nu, N, B, L.G, L.C, a["gt"], L.c, ma["rho"], ma["S"], a["gamma"], ma["Ginv"], ma["Pinv"], a["lam"], a["z"],
                            r=a["r"], p=a["p"], tol=L.tol, max_iter=L.max_iter, iters=a["it"], max_iter_exit=a["fl"])
        solver.admm_soft_update(nx, nu, N, B, L.g, L.lo, L.hi, L.kappa, ma["rho"], a["z"], a["w"], a["y"], a["gt"], res=a["res"])
        solver.admm_soft_restep(nx, nu, N, B, L.G, mb["Ginv"], L.C, L.g, L.c, L.lo, L.hi, L.kappa, mb["rho"], mb["S"], mb["Pinv"],
                                b["gamma"], b["lam"], b["z"], b["w"], b["y"], b["gt"], b["res"], mb["expo"], r=b["r"], p=b["p"], tol=L.tol,
                                max_iter=L.max_iter, iters=b["it"], max_iter_exit=b["fl"], **RULE)
        gr.launch()
    torch.cuda.synchronize()
    gr.close()
    assert moved > 0, "the rule must have moved some rho"
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"restep vs its parts: {k}"
        assert same(b[k], g[k]), f"restep graph vs eager: {k}"
    for k in ma:
        assert same(ma[k], mb[k]) and same(mb[k], mg[k]), k


# ---- 5. NaN and footprint
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_problem(solver, dtype):
    nx, nu, N, B = 14, 7, 24, 3
    d = soft_data(nx, nu, N, B, dtype)
    clean = hard.device_tensors(d)
    rc = run(solver, nx, nu, N, B, clean, False)
    t = hard.device_tensors(d)
    j = 131
    t["z"].view(B, -1)[1, j] = float("nan")
    res = run(solver, nx, nu, N, B, t, False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(res[1]).all())
    assert all(bool(torch.isnan(t[k].view(B, -1)[1, j])) for k in ("w", "y", "gt"))
    for p in (0, 2):
        for k in ("w", "y", "gt"):
            assert same(t[k].view(B, -1)[p], clean[k].view(B, -1)[p]), (k, p)
        assert same(res[p], rc[p]) and bool(torch.isfinite(res[p]).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_footprint(solver, nx, nu, N, B, dtype):
    d = soft_data(nx, nu, N, B, dtype)
    GUARD = 1024
    results = []
    for fill in (float("nan"), 1e30):
        bufs, t = {}, {}
        for k, a in list(d.items()) + [("gt", np.full_like(d["g"], np.nan)), ("res", np.full((B, 2), fill, dtype))]:
            n = a.size
            buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=hard.tdt(dtype), device="cuda")
            buf[GUARD:GUARD + n] = dev(a.reshape(-1))
            bufs[k], t[k] = buf, buf[GUARD:GUARD + n]
        before = {k: b.clone() for k, b in bufs.items()}
        run(solver, nx, nu, N, B, t, False, res=t["res"])
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert same(b[:GUARD], before[k][:GUARD]) and same(b[-GUARD:], before[k][-GUARD:]), f"guard of {k}"
        for k in ("z", "g", "lo", "hi", "kappa", "rho"):
            assert same(bufs[k], before[k]), f"{k} was written"
        for k in ("w", "y", "gt", "res"):
            assert bool(torch.isfinite(t[k]).all()), k
        results.append({k: t[k].clone() for k in ("w", "y", "gt", "res")})
    for k in results[0]:
        assert same(results[0][k], results[1][k]), k     # nothing is read from res


# ---- 6. convergence on the fixture of tests/test_admm_soft_reference.py
@pytest.mark.parametrize("dtype", DTYPES)
def test_replays_converge_like_the_reference(solver, dtype):
    nx, nu, N, B = sr.CONV_SHAPE
    rho = np.array(sr.CONV_RHO)
    d, lo, hi, kappa = sr.soft_inputs()
    ref = sr.soft_reference(4000)
    K, marks = sr.SOFT_K, (1, 2, 10, sr.SOFT_K)
    L = SoftLoop(solver, nx, nu, N, B, dtype, d, rho, lo=lo, hi=hi, kappa=kappa, tol=PCG_TOL[dtype], max_iter=200)
    o = L.soft_start()
    gr = L.graph(o)
    flags, snap = torch.zeros_like(o["fl"]), {}
    for k in range(1, K + 1):
        gt_in = o["gt"].clone() if k in marks else None
        gr.launch()
        flags |= o["fl"]
        if k in marks:
            snap[k] = (gt_in, o["z"].clone(), o["res"].clone())
    torch.cuda.synchronize()
    gr.close()
    what, tol = np.dtype(dtype).name, STEP_TOL[dtype]
    res1, resK = snap[1][2].cpu().numpy().astype(F64), snap[K][2].cpu().numpy().astype(F64)
    assert int(flags.sum()) == 0, "a solve ran out of iterations"
    y = o["y"].cpu().numpy().reshape(B, -1)
    assert (np.abs(y) <= (kappa.astype(dtype) / rho.astype(dtype).reshape(-1, 1)).astype(dtype)).all(), "(c) |rho y| <= kappa"
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        nz, nl = Gd.shape[0], Cd.shape[0]
        Kkt = np.zeros((nz + nl, nz + nl))
        Kkt[:nz, :nz], Kkt[:nz, nz:], Kkt[nz:, :nz] = Gd + rho[b] * np.eye(nz), Cd.T, Cd
        for k in marks:      # (a)
            gt_in, z = (snap[k][i].cpu().numpy().astype(F64).reshape(B, -1)[b] for i in (0, 1))
            zr = np.linalg.solve(Kkt, np.concatenate([-gt_in, c]))[:nz]
            err = np.linalg.norm(z - zr) / np.linalg.norm(zr)
            print(f"{what} problem {b} iteration {k}: z against the dense solve for the device's gt {err:.3e} (tol {tol:.0e})")
            assert err <= tol, (b, k, err)
        if dtype == F64:     # fp64 follows the reference history
            for k in marks:
                z = snap[k][1].cpu().numpy().reshape(B, -1)[b]
                err = np.linalg.norm(z - ref[b]["z"][k - 1]) / np.linalg.norm(ref[b]["z"][k - 1])
                assert err <= k * tol, (b, k, err)
        ratio = resK[b, 0] / res1[b, 0]
        print(f"{what} problem {b}: r_prim({K})/r_prim(1) {ratio:.3e} (reference {ref[b]['r_prim'][K - 1] / ref[b]['r_prim'][0]:.3e}, "
              f"bound {sr.SOFT_RATIO_BOUND:.3e})")
        assert resK[b, 0] <= sr.SOFT_RATIO_BOUND * res1[b, 0], (b, ratio)   # (b)


# ---- 7. the infeasible-hard fixture: the hard loop stalls at the gap, the soft loop converges in the pinned count
@pytest.mark.parametrize("dtype", DTYPES)
def test_infeasible_hard_problem_stalls_and_soft_converges(solver, dtype):
    nx, nu, N, B = sr.CONV_SHAPE
    d, lo, hi, kappa = sr.infeasible_inputs()
    L = SoftLoop(solver, nx, nu, N, B, dtype, d, np.array(sr.CONV_RHO), lo=lo, hi=hi, kappa=kappa, tol=PCG_TOL[dtype], max_iter=200)
    o = L.state()
    gr = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"], o["r"], o["p"],
                                L.tol, L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
    low = torch.full((B,), float("inf"), dtype=o["res"].dtype, device="cuda")
    for _ in range(sr.INFEAS_K):
        gr.launch()
        low = torch.minimum(low, o["res"][:, 0])
    torch.cuda.synchronize()
    gr.close()
    print(f"{np.dtype(dtype).name}: hard r_prim never below {low.cpu().numpy()} (pinned floor {sr.INFEAS_HARD_FLOOR})")
    assert bool((low >= 0.5 * sr.INFEAS_HARD_FLOOR).all())
    # the soft family on the same buffers, from the same start (the soft init of w = y = 0 is the start of the hard loop: gt = g)
    o2 = L.soft_start()
    gr = L.graph(o2)
    Kmax = int(1.1 * max(sr.INFEAS_SOFT_ITERS)) + 2
    hist = []
    for _ in range(Kmax):
        gr.launch()
        hist.append(o2["res"].clone())
    torch.cuda.synchronize()
    gr.close()
    hist = torch.stack(hist).cpu().numpy().astype(F64)      # [K, B, 2]
    for b in range(B):
        ok = (hist[:, b, 0] < sr.INFEAS_TOL) & (hist[:, b, 1] < sr.INFEAS_TOL)
        assert ok.any(), (b, hist[-1, b])
        at, want = int(np.argmax(ok)) + 1, sr.INFEAS_SOFT_ITERS[b]
        print(f"{np.dtype(dtype).name} problem {b}: soft converged at iteration {at} (reference {want})")
        assert at == want if dtype == F64 else abs(at - want) <= 0.1 * want, (b, at, want)


# ---- 8. refusals write nothing
@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_refusals_write_nothing(solver, suf, tt):
    import ctypes
    nx, nu, N, B = 6, 3, 4, 3
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = torch.zeros(1 << 16, dtype=tt, device="cuda")
    rho = torch.ones(B, dtype=tt, device="cuda")
    written = ("gamma", "lam", "r", "p", "z", "w", "y", "gt", "res", "Ginv", "S", "Pinv")
    outs = {k: torch.full((1 << 14,), 777.0, dtype=tt, device="cuda") for k in written}
    it = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
    expo = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    step_args = ("Ginv", "C", "g", "c", "lo", "hi", "kappa", "rho", "S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z",
                 "w", "y", "gt", "res")
    restep_args = ("G",) + step_args[:10] + ("kind",) + step_args[10:] + ("ratio", "shift", "rho_min", "rho_max", "expo")

    def untouched():
        torch.cuda.synchronize()
        return (all(bool((t == 777.0).all()) for t in outs.values()) and bool((it == 777).all()) and bool((fl == 77).all()) and
                bool((expo == 777).all()) and bool((rho == 1).all()))

    def values(null=(), **over):
        v = {k: P(ins) for k in ("G", "C", "g", "c", "lo", "hi", "kappa")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(it=P(it), fl=P(fl), expo=P(expo), tol=1e-6, max_iter=10, kind=2, ratio=10.0, shift=1, rho_min=1e-3, rho_max=1e3)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    graph = ctypes.c_void_p()
    head = (solver.h, nx, nu, N, B)
    calls = [(f"gbdpcg_admm_soft_step_{suf}", step_args, s), (f"gbdpcg_admm_soft_step_shared_{suf}", step_args, s),
             (f"gbdpcg_graph_create_admm_soft_step_{suf}", step_args, ctypes.byref(graph)),
             (f"gbdpcg_graph_create_admm_soft_step_shared_{suf}", step_args, ctypes.byref(graph)),
             (f"gbdpcg_admm_soft_restep_{suf}", restep_args, s), (f"gbdpcg_graph_create_admm_soft_restep_{suf}", restep_args, ctypes.byref(graph))]
    for name, names, last in calls:
        for k in ("kappa", "lo", "hi", "rho", "w", "y", "gt", "res", "z", "g"):
            v = values(null=(k,))
            assert getattr(lib, name)(*head, *(v[a] for a in names), last) == 1, (name, k)
        assert not graph.value
    for k in ("kappa", "lo", "hi", "w"):
        v = values(null=(k,))
        assert getattr(lib, f"gbdpcg_admm_soft_init_{suf}")(*head, v["g"], v["lo"], v["hi"], v["kappa"], v["rho"], v["w"], v["y"], v["gt"], s) == 1
        assert getattr(lib, f"gbdpcg_admm_soft_update_{suf}")(*head, v["g"], v["lo"], v["hi"], v["kappa"], v["rho"], v["z"], v["w"], v["y"],
                                                              v["gt"], v["res"], s) == 1
    # a block size the formation refuses: UNSUPPORTED from the composite calls, behind every INVALID
    big = (solver.h, 80, 40, N, B) if suf == "f64" else (solver.h, 120, 60, N, B)
    for name, names, last in calls:
        v = values()
        assert getattr(lib, name)(*big, *(v[a] for a in names), last) == 4, name
        v = values(null=("kappa",))
        assert getattr(lib, name)(*big, *(v[a] for a in names), last) == 1, name
    assert not graph.value and untouched()
