"""Soft (L1-penalised) stage-wise rows on the device: gbdpcg_admm_lin_soft_init_*, _update_*, _rebalance_*, _step_*, the shared twin,
the graphs and _restep_* (csrc/admm_rows.hip's SOFT instantiations through the C ABI).  PARITY UNPINNED: the reference tree has
nothing for these steps.

Reference: admm_soft_ref.lin_update_ref, which gives every output to the bit (chains of exactly rounded fmas).  With kappa = +Inf
every entry point must give the bits of its gbdpcg_admm_lin_* twin, with E = I those of gbdpcg_admm_soft_*, and the composite calls
the bits of the calls they are made of."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_ref as ref  # noqa: E402
import admm_soft_ref as sr  # noqa: E402
import test_gpu_admm_lin as hard  # noqa: E402
from admm_util import dev, host, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
SHAPES = hard.SHAPES          # with the N = 1 shape and the NC + 1 shape, whose horizon spans two staging chunks
assert (14, 7, hard.NC + 1, 2, 4, 2) in SHAPES and (3, 2, 1, 2, 2, 0) in SHAPES


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def soft_data(shape, dtype):
    """hard.lin_data with kappa drawn from {0, a subnormal, finite values, +Inf}."""
    d = dict(hard.lin_data(shape, dtype))
    B, nw = d["w"].shape
    rng = np.random.default_rng(31 + nw)
    pick = rng.integers(0, 6, (B, nw))
    sub = float(np.finfo(dtype).smallest_subnormal * dtype(3))
    d["kappa"] = np.select([pick == 0, pick == 1, pick == 2], [0.0, sub, np.inf], rng.uniform(0.05, 1.5, (B, nw))).astype(dtype)
    d["kappa"].setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def soft_reference(shape, dtype, init):
    nx, nu, N, B, mx, mu = shape
    d = soft_data(shape, dtype)
    return sr.lin_update_ref(dtype, nx, nu, mx, mu, N, d["g"], d["E"], d["lo"], d["hi"], d["kappa"], d["rho"], None if init else d["z"],
                             d["w"], d["y"])


def run(solver, shape, t, init):
    nx, nu, N, B, mx, mu = shape
    if init:
        solver.admm_lin_soft_init(nx, nu, mx, mu, N, B, t["g"], t["E"], t["lo"], t["hi"], t["kappa"], t["rho"], t["w"], t["y"], gt=t["gt"])
        return None
    return solver.admm_lin_soft_update(nx, nu, mx, mu, N, B, t["g"], t["E"], t["lo"], t["hi"], t["kappa"], t["rho"], t["z"], t["w"], t["y"],
                                       t["gt"], res=t["res"])


# ---- 1. bits against the exact reference; aligned and misaligned bases; guard elements around every array
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=hard.ids)
def test_update_and_init_bits(solver, shape, dtype, init):
    B = shape[3]
    d = soft_data(shape, dtype)
    wr, yr, gr, rr = soft_reference(shape, dtype, init)
    for offset in (0, 1):
        t = hard.device_tensors(d, offset, guard=64)
        before = {k: b.clone() for k, b in t["_bufs"].items()}
        run(solver, shape, t, init)
        torch.cuda.synchronize()
        assert np_same(host(t["w"], B), wr), f"w (offset {offset})"
        assert np_same(host(t["y"], B), yr), f"y (offset {offset})"
        assert np_same(host(t["gt"], B), gr), f"gt (offset {offset})"
        if not init:
            assert np_same(host(t["res"], B), rr), f"res (offset {offset})"
        written = ("w", "gt") if init else ("w", "y", "gt", "res")
        for k, b in t["_bufs"].items():
            lead = 64 + offset
            n = t[k].numel()
            assert same(b[:lead], before[k][:lead]) and same(b[lead + n:], before[k][lead + n:]), f"guard of {k}"
            if k not in written:
                assert same(b, before[k]), f"{k} was written"
    if not init:
        theta = (d["kappa"] / d["rho"].reshape(-1, 1)).astype(dtype)
        assert (np.abs(yr) <= theta).all()


# ---- 2. kappa = +Inf: the bits of the hard rows family, entry point by entry point
class SoftLinLoop(hard.LinLoop):
    def __init__(self, *a, kappa=None, **k):
        super().__init__(*a, **k)
        self.kappa = torch.full_like(self.lo, float("inf")) if kappa is None else dev(np.asarray(kappa).astype(a[2]).reshape(-1))

    def head(self, o, mats=None):
        nx, nu, N, B, mx, mu = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        return (nx, nu, mx, mu, N, B, Ginv, C, self.g, self.c, E, self.lo, self.hi, self.kappa, self.rho, S, Pinv, o["gamma"], o["lam"])

    def one_call(self, o, mats=None, shared=False):
        step = self.s.admm_lin_soft_step_shared if shared else self.s.admm_lin_soft_step
        step(*self.head(o, mats), o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter,
             iters=o["it"], max_iter_exit=o["fl"])

    def two_calls(self, o, mats=None, shared=False):
        nx, nu, N, B, mx, mu = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        resolve = self.s.kkt_resolve_shared if shared else self.s.kkt_resolve
        resolve(nx, nu, N, B, Ginv, C, o["gt"], self.c, S, Pinv, o["gamma"], o["lam"], o["z"], r=o["r"], p=o["p"], tol=self.tol,
                max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        self.s.admm_lin_soft_update(nx, nu, mx, mu, N, B, self.g, E.repeat(B) if shared else E, self.lo, self.hi, self.kappa, self.rho,
                                    o["z"], o["w"], o["y"], o["gt"], res=o["res"])

    def graph(self, o, mats=None, shared=False):
        make = self.s.graph_admm_lin_soft_step_shared if shared else self.s.graph_admm_lin_soft_step
        return make(*self.head(o, mats), o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])

    def restep_buffers(self):
        B = self.shape[3]
        return dict(Gt=self.Gt.clone(), Ginv=self.Ginv.clone(), S=self.S.clone(), Pinv=self.Pinv.clone(), rho=self.rho.clone(),
                    expo=torch.full((B,), 99, dtype=torch.int32, device="cuda"))

    def restep(self, o, m, soft=True, graph=False):
        nx, nu, N, B, mx, mu = self.shape
        kap = (self.kappa,) if soft else ()
        lead = (nx, nu, mx, mu, N, B, self.G, m["Gt"], m["Ginv"], self.C, self.g, self.c, self.E, self.lo, self.hi, *kap, m["rho"], m["S"],
                m["Pinv"], o["gamma"], o["lam"])
        if graph:
            return self.s.graph_admm_lin_soft_restep(*lead, o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"],
                                                     o["gt"], o["res"], m["expo"], **RULE)
        fn = self.s.admm_lin_soft_restep if soft else self.s.admm_lin_restep
        fn(*lead, o["z"], o["w"], o["y"], o["gt"], o["res"], m["expo"], r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter,
           iters=o["it"], max_iter_exit=o["fl"], **RULE)


RULE = dict(ratio=1.0, shift=1, rho_min=2.0 ** -10, rho_max=2.0 ** 10)     # ratio 1: rho moves whenever the residuals differ
STEP_SHAPE = (14, 7, 5, 3, 3, 2)


def loop(solver, dtype, finite, shared=False, shape=STEP_SHAPE):
    nx, nu, N, B, mx, mu = shape
    d = dict(hard.step_problem(nx, nu, N, B))
    E = hard.random_rows(shape)
    if shared:
        d["G"], d["C"] = np.repeat(d["G"][:1], B, axis=0), np.repeat(d["C"][:1], B, axis=0)
        E = np.repeat(np.asarray(E).reshape(B, -1)[:1], B, axis=0)
    L = SoftLinLoop(solver, shape, dtype, d, E, np.full(B, 1.5) if shared else 0.5 * (np.arange(B) + 2.0))
    if finite:
        rng = np.random.default_rng(9)
        nw = L.lo.numel() // B
        kap = np.where(rng.random((B, nw)) < 0.25, np.inf, rng.uniform(0.01, 0.5, (B, nw)))
        L.kappa = dev(kap.astype(dtype).reshape(-1))
    return L


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_kappa_gives_the_hard_bits(solver, dtype):
    shape = STEP_SHAPE
    nx, nu, N, B, mx, mu = shape
    # init and update on random data
    d = hard.lin_data(shape, dtype)
    for init in (True, False):
        a, b = hard.device_tensors(d), hard.device_tensors(d)
        b["kappa"] = torch.full_like(b["lo"], float("inf"))
        hard.run_update(solver, shape, a, init)
        run(solver, shape, b, init)
        torch.cuda.synchronize()
        for k in ("w", "y", "gt") + (() if init else ("res",)):
            assert same(a[k], b[k]), (init, k)
    # step over 5 iterations, the shared step, the rebalance and the restep
    L = loop(solver, dtype, finite=False)
    a, b = L.state(), L.state()
    for _ in range(5):
        hard.LinLoop.one_call(L, a)
        L.one_call(b)
    torch.cuda.synchronize()
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"step: {k}"
    ra, rb = L.rho.clone(), L.rho.clone()
    ea = solver.admm_lin_rebalance(nx, nu, mx, mu, N, B, L.g, L.E, L.lo, L.hi, a["res"], ra, a["w"], a["y"], a["gt"], **RULE)
    eb = solver.admm_lin_soft_rebalance(nx, nu, mx, mu, N, B, L.g, L.E, L.lo, L.hi, L.kappa, b["res"], rb, b["w"], b["y"], b["gt"], **RULE)
    torch.cuda.synchronize()
    assert same(ea, eb) and same(ra, rb) and all(same(a[k], b[k]) for k in ("w", "y", "gt")) and int(ea.abs().sum()) > 0
    a, b, ma, mb = L.state(), L.state(), L.restep_buffers(), L.restep_buffers()
    hard.LinLoop.one_call(L, a)
    L.one_call(b)
    for _ in range(5):
        L.restep(a, ma, soft=False)
        L.restep(b, mb)
    torch.cuda.synchronize()
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"restep: {k}"
    for k in ma:
        assert same(ma[k], mb[k]), f"restep: {k}"
    S = loop(solver, dtype, finite=False, shared=True)
    ne = S.E.numel() // B
    ng, nc, ns = S.G.numel() // B, S.C.numel() // B, S.S.numel() // B
    single = (S.Ginv[:ng].clone(), S.C[:nc].clone(), S.S[:ns].clone(), S.Pinv[:ns].clone(), S.E[:ne].clone())
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b = S.state(), S.state()
        for _ in range(5):
            hard.LinLoop.one_call(S, a, mats=single, shared=True)
            S.one_call(b, mats=single, shared=True)
        torch.cuda.synchronize()
    finally:
        solver.set_path(binding.PATH_AUTO)
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"shared step: {k}"


# ---- 3. E = I: the bits of the soft box calls
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(5, 2, 10, 4), (14, 7, 5, 3)])
def test_identity_rows_give_the_bits_of_the_soft_box_calls(solver, nx, nu, N, B, dtype):
    nz = (nx + nu) * N - nu
    rng = np.random.default_rng(5 + nz)
    E = dev(np.tile(ref.identity_E(nx, nu, N, dtype), B))
    rho = dev(rng.uniform(0.5, 4.0, B).astype(dtype))
    z, g, w, y = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    lo, hi = (-0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype), (0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype)
    lo[rng.random((B, nz)) < 1.0 / 3.0], hi[rng.random((B, nz)) < 1.0 / 3.0] = -np.inf, np.inf
    kap = np.where(rng.random((B, nz)) < 0.25, np.inf, rng.uniform(0.0, 0.8, (B, nz))).astype(dtype)
    t = {k: dev(v.reshape(-1)) for k, v in dict(z=z, g=g, lo=lo, hi=hi, kappa=kap).items()}
    for init in (True, False):
        a = {k: dev(v.reshape(-1)) for k, v in dict(w=w, y=y).items()}
        b = {k: v.clone() for k, v in a.items()}
        if init:
            a["gt"] = solver.admm_soft_init(nx, nu, N, B, t["g"], t["lo"], t["hi"], t["kappa"], rho, a["w"], a["y"])
            b["gt"] = solver.admm_lin_soft_init(nx, nu, nx, nu, N, B, t["g"], E, t["lo"], t["hi"], t["kappa"], rho, b["w"], b["y"])
        else:
            a["gt"], b["gt"] = torch.empty_like(t["g"]), torch.empty_like(t["g"])
            a["res"] = solver.admm_soft_update(nx, nu, N, B, t["g"], t["lo"], t["hi"], t["kappa"], rho, t["z"], a["w"], a["y"], a["gt"])
            b["res"] = solver.admm_lin_soft_update(nx, nu, nx, nu, N, B, t["g"], E, t["lo"], t["hi"], t["kappa"], rho, t["z"], b["w"], b["y"],
                                                   b["gt"])
        torch.cuda.synchronize()
        for k in a:
            assert same(a[k], b[k]), (init, k)


# ---- 4. step, graph, shared, rebalance and restep identities with finite weights
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [STEP_SHAPE, (14, 7, hard.NC + 1, 2, 4, 2)], ids=hard.ids)
def test_step_graph_and_restep_identities(solver, shape, dtype):
    nx, nu, N, B, mx, mu = shape
    L = loop(solver, dtype, finite=True, shape=shape)
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
    theta = L.kappa.view(B, -1) / L.rho.view(B, 1)
    assert bool((b["y"].view(B, -1).abs() <= theta).all()) and int(b["fl"].sum()) == 0
    # restep = soft rebalance (rebalance launch + SOFT init), formation, kkt_step on Gt, soft update; and its graph
    ma, mb, mg = L.restep_buffers(), L.restep_buffers(), L.restep_buffers()
    gr = L.restep(g, mg, graph=True)
    moved = 0
    for _ in range(3):
        w_before = a["w"].clone()
        solver.admm_lin_soft_rebalance(nx, nu, mx, mu, N, B, L.g, L.E, L.lo, L.hi, L.kappa, a["res"], ma["rho"], a["w"], a["y"], a["gt"],
                                       ma["expo"], **RULE)
        torch.cuda.synchronize()
        assert same(a["w"], w_before), "the soft init must not move a w the soft update wrote"
        theta = L.kappa.view(B, -1) / ma["rho"].view(B, 1)
        assert bool((a["y"].view(B, -1).abs() <= theta).all()), "|y| <= fl(kappa / rho_new) after the rebalance"
        moved += int(ma["expo"].abs().sum())
        solver.admm_lin_form(nx, nu, mx, mu, N, B, L.G, L.E, ma["rho"], Gt=ma["Gt"])
        solver.kkt_step(nx, nu, N, B, ma["Gt"], L.C, a["gt"], L.c, ma["S"], a["gamma"], ma["Ginv"], ma["Pinv"], a["lam"], a["z"], r=a["r"],
                        p=a["p"], tol=L.tol, max_iter=L.max_iter, iters=a["it"], max_iter_exit=a["fl"])
        solver.admm_lin_soft_update(nx, nu, mx, mu, N, B, L.g, L.E, L.lo, L.hi, L.kappa, ma["rho"], a["z"], a["w"], a["y"], a["gt"],
                                    res=a["res"])
        L.restep(b, mb)
        gr.launch()
    torch.cuda.synchronize()
    gr.close()
    assert moved > 0
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"restep vs its parts: {k}"
        assert same(b[k], g[k]), f"restep graph vs eager: {k}"
    for k in ma:
        assert same(ma[k], mb[k]) and same(mb[k], mg[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_twin(solver, dtype):
    B = STEP_SHAPE[3]
    S = loop(solver, dtype, finite=True, shared=True)
    ne, ng, nc, ns = S.E.numel() // B, S.G.numel() // B, S.C.numel() // B, S.S.numel() // B
    single = (S.Ginv[:ng].clone(), S.C[:nc].clone(), S.S[:ns].clone(), S.Pinv[:ns].clone(), S.E[:ne].clone())
    copies = tuple(m.repeat(B) for m in single)
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b, c = S.state(), S.state(), S.state()
        for _ in range(3):
            S.one_call(a, mats=copies)
            S.one_call(b, mats=single, shared=True)
            S.two_calls(c, mats=single, shared=True)
        torch.cuda.synchronize()
    finally:
        solver.set_path(binding.PATH_AUTO)
    for k in hard.ORDER:
        assert same(a[k], b[k]), f"shared vs copies: {k}"
        assert same(b[k], c[k]), f"shared step vs shared resolve + soft update: {k}"


@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_null_kappa_is_refused_and_nothing_is_written(solver, suf, tt):
    import ctypes
    nx, nu, mx, mu, N, B = 6, 3, 2, 2, 4, 3
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins, rho = torch.zeros(1 << 14, dtype=tt, device="cuda"), torch.ones(B, dtype=tt, device="cuda")
    out = torch.full((1 << 14,), 777.0, dtype=tt, device="cuda")
    expo = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    head = (solver.h, nx, nu, mx, mu, N, B)
    for kap, want in ((None, 1), (P(ins), 0)):
        st = getattr(lib, f"gbdpcg_admm_lin_soft_init_{suf}")(*head, P(ins), P(ins), P(ins), P(ins), kap, P(rho), P(out), P(out), P(out), s)
        if want:
            assert st == 1
            assert getattr(lib, f"gbdpcg_admm_lin_soft_update_{suf}")(*head, P(ins), P(ins), P(ins), P(ins), kap, P(rho), P(ins), P(out),
                                                                       P(out), P(out), P(out), s) == 1
            assert getattr(lib, f"gbdpcg_admm_lin_soft_rebalance_{suf}")(*head, P(ins), P(ins), P(ins), P(ins), kap, P(ins), P(rho), P(out),
                                                                          P(out), P(out), 10.0, 1, 1e-3, 1e3, P(expo), s) == 1
            torch.cuda.synchronize()
            assert bool((out == 777.0).all()) and bool((expo == 777).all()) and bool((rho == 1).all())
        else:
            assert st == 0      # the same call with kappa in place is taken
    torch.cuda.synchronize()
