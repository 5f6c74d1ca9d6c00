"""The backward pass of the hard box QP on the device (the adjoint entry of csrc/admm.hip, csrc/admm_box_grad.hip and their composite calls in csrc/api_kkt.hip, through the C
ABI): gbdpcg_admm_adjoint_init_*, gbdpcg_admm_adjoint_update_*, gbdpcg_admm_adjoint_step_* and its graph, gbdpcg_admm_grad_bounds_*.
PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.

Reference: tests/admm_adjoint_ref.py.  The update is defined to the bit, so w, y and the two norms are compared for EQUALITY with
update_ref in the call's precision AND with gbdpcg_admm_update_* / gbdpcg_admm_init_* on the explicit degenerate box (gt included: the
same fma); gt is also held against its exact rational value within u (|rho t| + |ref|), as in tests/test_gpu_admm.py.  The composite
calls are compared bit for bit with the calls they are made of.  Converged gradients: after K_FWD forward and K_ADJ adjoint replays
on the pinned fixture every gradient is within admm_adjoint_ref.converged_bound of the dense reference -- twice the fp64 loops' own
distance at those counts plus STEP_TOL (tests/test_gpu_admm.py, copied) accumulated over the replays.  Run with -s for the figures."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_adjoint_ref as ar  # noqa: E402
from admm_util import bits, dev, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_admm.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
SHAPES = [(2, 1, 1, 3),      # nz = 2
          (3, 2, 2, 3),      # nz = 8
          (14, 7, 3, 3),     # nz = 56
          (5, 3, 40, 2),     # nz = 317 > 256: four waves, odd problem stride
          (5, 2, 3, 4)]      # nz = 19: the four problems start 0, 3, 2, 1 elements behind a 16-byte boundary -- every head length
OFFSETS = [0, 1]             # 16-byte aligned bases (the vec path) / every base off by one element (the scalar path)


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.dtype(F32) else torch.float64


def nz_of(nx, nu, N):
    return (nx + nu) * N - nu


@functools.lru_cache(maxsize=None)
def data(nx, nu, N, B, dtype):
    """az, w, y, gz of order 1 with +0 and -0 planted (v = -0 under a pin stays -0), yf zero on about half of the entries with both
    signs elsewhere, rho_b in [0.5, 4]: arrays [B, nz] of `dtype`, read-only; lo, hi: the explicit degenerate box of yf."""
    nz = nz_of(nx, nu, N)
    rng = np.random.default_rng(2000 + nz)
    az, w, y, gz = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    yf = np.where(rng.random((B, nz)) < 0.5, 0.0, rng.standard_normal((B, nz))).astype(dtype)
    az[:, 0], y[:, 0], yf[:, 0] = -0.0, -0.0, 1.0          # v = -0, pinned
    az[:, nz - 1], y[:, nz - 1], yf[:, nz - 1] = 0.0, -0.0, -0.0     # v = +0, free (yf = -0 is not != 0)
    rho = rng.uniform(0.5, 4.0, B).astype(dtype)
    lo, hi = ar.degenerate_box(yf, dtype)
    d = dict(az=az, w=w, y=y, gz=gz, yf=yf, rho=rho, lo=lo, hi=hi)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, dtype, init):
    d = data(nx, nu, N, B, dtype)
    return ar.update_ref(dtype, d["gz"], d["yf"], d["rho"], None if init else d["az"], d["w"], d["y"])


def device_tensors(d, offset=0, guard=8, extra=()):
    """The arrays of data() on the device, flat, plus gt and res (NaN): every array starts `offset` elements into a buffer of its own
    whose base the allocator aligns.  Returns (views, buffers)."""
    t, bufs = {}, {}
    items = list(d.items()) + [("gt", np.full_like(d["gz"], np.nan)), ("res", np.full((d["rho"].size, 2), np.nan, d["gz"].dtype))] + list(extra)
    for k, a in items:
        flat = dev(a.reshape(-1))
        off = 0 if k in ("rho", "res") else offset
        buf = torch.full((flat.numel() + 2 * guard,), float("nan"), dtype=flat.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0 and (guard * flat.element_size()) % 16 == 0
        buf[guard + off:guard + off + flat.numel()] = flat
        t[k], bufs[k] = buf[guard + off:guard + off + flat.numel()], buf
    return t, bufs


def run_adjoint(solver, shape, t, init):
    nx, nu, N, B = shape
    if init:
        solver.admm_adjoint_init(nx, nu, N, B, t["gz"], t["yf"], t["rho"], t["w"], t["y"], gta=t["gt"])
    else:
        solver.admm_adjoint_update(nx, nu, N, B, t["gz"], t["yf"], t["rho"], t["az"], t["w"], t["y"], t["gt"], res=t["res"])


def run_box(solver, shape, t, init):
    nx, nu, N, B = shape
    if init:
        solver.admm_init(nx, nu, N, B, t["gz"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
    else:
        solver.admm_update(nx, nu, N, B, t["gz"], t["lo"], t["hi"], t["rho"], t["az"], t["w"], t["y"], t["gt"], res=t["res"])


def check_gt(gt, ref_gt, t, rho, dtype, what):
    u = Fraction(2.0 ** -24 if dtype == F32 else 2.0 ** -53)
    B, nz = t.shape
    for b in range(B):
        r = Fraction(float(rho[b]))
        for i in range(nz):
            ref = ref_gt[b, i]
            assert ref is not None and np.isfinite(gt[b, i]), (what, b, i)
            err, bound = abs(Fraction(float(gt[b, i])) - ref), u * (abs(r * Fraction(float(t[b, i]))) + abs(ref))
            assert err <= bound, (what, b, i, float(err), float(bound))


# ---- 1. bits: against the exact reference and against the box kernels on the explicit degenerate box, both alignments
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_bits_vs_reference_and_vs_box_update(solver, nx, nu, N, B, dtype, init):
    shape = (nx, nu, N, B)
    d = data(*shape, dtype)
    wr, yr, tr, gr, rr = reference(*shape, dtype, init)
    what = f"{shape} {np.dtype(dtype).name} {'init' if init else 'update'}"
    outs = []
    for offset in OFFSETS:
        t, _ = device_tensors(d, offset)
        want = 0 if offset == 0 else t["gz"].element_size()
        assert all(t[k].data_ptr() % 16 == want for k in ("gz", "yf", "az", "w", "y", "gt", "lo", "hi"))
        run_adjoint(solver, shape, t, init)
        tb, _ = device_tensors(d, offset)
        run_box(solver, shape, tb, init)
        torch.cuda.synchronize()
        keys = ("w", "y", "gt") + (() if init else ("res",))
        for k in keys:
            assert same(t[k], tb[k]), f"{what} offset {offset}: {k} differs from the box kernel on the degenerate box"
        w, y, gt = (t[k].cpu().numpy().reshape(B, -1) for k in ("w", "y", "gt"))
        assert np_same(w, wr), what + ": w"
        assert np_same(y, yr), what + ": y"
        if init:
            assert same(t["y"], dev(d["y"].reshape(-1)))
        else:
            assert np_same(t["res"].cpu().numpy().reshape(B, 2), rr), what + ": res"
        check_gt(gt, gr, tr, d["rho"], dtype, what)
        outs.append({k: t[k].clone() for k in keys})
    for k in outs[0]:
        assert same(outs[0][k], outs[1][k]), f"{what}: {k}, aligned vs misaligned"
    w = outs[0]["w"].cpu().numpy().reshape(B, -1)
    assert not w[d["yf"] != 0].any()                                     # pinned entries are zero
    if not init:
        assert np.signbit(w[:, 0]).all()                                 # v = -0 under a pin stays -0
        y = outs[0]["y"].cpu().numpy().reshape(B, -1)
        assert not y[d["yf"] == 0].any()                                 # free entries: the identity projection


# ---- 2. the bound gradients
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHAPES)
def test_grad_bounds_bits(solver, nx, nu, N, B, dtype):
    d = data(nx, nu, N, B, dtype)
    glo_r, ghi_r = ar.grad_bounds_ref(dtype, d["yf"], d["rho"], d["y"])
    outs = []
    for offset in OFFSETS:
        nan = np.full_like(d["gz"], np.nan)
        t, bufs = device_tensors(d, offset, extra=[("glo", nan), ("ghi", nan)])
        before = {k: b.clone() for k, b in bufs.items()}
        solver.admm_grad_bounds(nx, nu, N, B, t["yf"], t["rho"], t["y"], glo=t["glo"], ghi=t["ghi"])
        torch.cuda.synchronize()
        assert np_same(t["glo"].cpu().numpy().reshape(B, -1), glo_r) and np_same(t["ghi"].cpu().numpy().reshape(B, -1), ghi_r)
        for k in bufs:
            if k not in ("glo", "ghi"):
                assert same(bufs[k], before[k]), f"{k} was written"
        for k in ("glo", "ghi"):
            o, n = 8 + offset, t[k].numel()
            assert bool(torch.isnan(bufs[k][:o]).all()) and bool(torch.isnan(bufs[k][o + n:]).all()), f"guard of {k}"
        outs.append((t["glo"].clone(), t["ghi"].clone()))
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])
    glo, ghi = glo_r, ghi_r
    assert not glo[d["yf"] >= 0].view(np.uint8).any() and not ghi[d["yf"] <= 0].view(np.uint8).any()     # +0 off the side


# ---- 3. footprint: guard words around every output, inputs untouched, nothing read from res
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 3, 3), (5, 3, 40, 2)])
def test_footprint(solver, nx, nu, N, B, dtype, init):
    shape = (nx, nu, N, B)
    d = data(*shape, dtype)
    GUARD = 1024
    results = []
    for fill in (float("nan"), 1e30):
        t, bufs = device_tensors(d, 0, guard=GUARD)
        t["res"].fill_(fill)
        before = {k: b.clone() for k, b in bufs.items()}
        run_adjoint(solver, shape, t, init)
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert same(b[:GUARD], before[k][:GUARD]) and same(b[-GUARD:], before[k][-GUARD:]), f"guard of {k}"
            assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all())
        written = ("w", "gt") if init else ("w", "y", "gt", "res")
        for k in bufs:
            if k not in written:
                assert same(bufs[k], before[k]), f"{k} was written"
        for k in written:
            assert bool(torch.isfinite(t[k]).all()), k
        results.append({k: t[k].clone() for k in written})
    for k in results[0]:
        assert same(results[0][k], results[1][k]), k     # nothing is read from res


# ---- 4. isolation
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_problem_and_zero_yf_is_the_identity(solver, dtype):
    shape = (5, 3, 40, 3)
    nx, nu, N, B = shape
    d = data(*shape, dtype)
    clean, _ = device_tensors(d)
    run_adjoint(solver, shape, clean, False)
    t, _ = device_tensors(d)
    j = 131
    t["az"].view(B, -1)[1, j] = float("nan")
    run_adjoint(solver, shape, t, False)
    torch.cuda.synchronize()
    res, rc = t["res"].view(B, 2), clean["res"].view(B, 2)
    assert bool(torch.isnan(res[1]).all())
    assert bool(torch.isnan(t["w"].view(B, -1)[1, j])) and bool(torch.isnan(t["gt"].view(B, -1)[1, j]))
    for p in (0, 2):
        for k in ("w", "y", "gt"):
            assert same(t[k].view(B, -1)[p], clean[k].view(B, -1)[p]), (k, p)
        assert same(res[p], rc[p]) and bool(torch.isfinite(res[p]).all())
    # a NaN in yf pins its entry (NaN != 0) and touches nothing else
    t, _ = device_tensors(d)
    t["yf"].view(B, -1)[1, j] = float("nan")
    run_adjoint(solver, shape, t, False)
    torch.cuda.synchronize()
    assert float(t["w"].view(B, -1)[1, j]) == 0.0 and bool(torch.isfinite(t["res"]).all())
    keep = torch.ones(B, nz_of(nx, nu, N), dtype=torch.bool, device="cuda")
    keep[1, j] = False
    for k in ("w", "y", "gt"):
        assert same(t[k].view(B, -1)[keep], clean[k].view(B, -1)[keep]), k
    # yf == 0 everywhere: the identity projection -- w = v, y = 0
    t, _ = device_tensors(d)
    t["yf"].zero_()
    run_adjoint(solver, shape, t, False)
    torch.cuda.synchronize()
    v = d["az"] + d["y"]
    assert v.dtype == np.dtype(dtype)
    assert np_same(t["w"].cpu().numpy().reshape(B, -1), v)
    assert not bits(t["y"]).any()
    assert np_same(t["res"].view(B, 2)[:, 0].cpu().numpy(), np.abs(d["az"] - v).max(axis=1))


# ---- 5. composition: the kept factorisation of the pinned fixture, its converged forward y as the mask
class Kept:
    """kkt_step_reg on a fixture of admm_adjoint_ref, K_FWD replays of the forward graph, and the buffers of the adjoint iteration."""

    def __init__(self, solver, nx, nu, N, B, dtype, max_iter=200):
        self.s, self.shape, self.tol, self.max_iter, self.dtype = solver, (nx, nu, N, B), PCG_TOL[dtype], max_iter, dtype
        d, lo, hi, gz, glam = ar.fixture(nx, nu, N, B)
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        self.lo, self.hi = dev(lo.astype(dtype).reshape(-1)), dev(hi.astype(dtype).reshape(-1))
        self.gz, self.nglam = dev(gz.astype(dtype).reshape(-1)), dev((-glam).astype(dtype).reshape(-1))
        self.rho = dev(np.asarray(ar.FIXTURE_RHO[:B], dtype))
        nan = float("nan")
        self.S = torch.full((B * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        gamma = torch.full((B * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, z = torch.zeros_like(gamma), torch.full_like(self.g, nan)
        r, p = torch.full_like(gamma, nan), torch.full_like(gamma, nan)
        it, fl = solver.kkt_step_reg(nx, nu, N, B, self.G, self.C, self.g, self.c, self.rho, self.S, gamma, self.Ginv, self.Pinv,
                                     self.lam, z, tol=self.tol, max_iter=max_iter)
        self.w, self.y = torch.zeros_like(self.g), torch.zeros_like(self.g)
        gt = solver.admm_init(nx, nu, N, B, self.g, self.lo, self.hi, self.rho, self.w, self.y)
        res = torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda")
        solver.reserve(self.g.element_size(), nx, N, B)
        gr = solver.graph_admm_step(nx, nu, N, B, self.Ginv, self.C, self.g, self.c, self.lo, self.hi, self.rho, self.S, self.Pinv, gamma,
                                    self.lam, r, p, self.tol, max_iter, it, fl, z, self.w, self.y, gt, res)
        flags = torch.zeros_like(fl)
        for _ in range(ar.K_FWD):
            gr.launch()
            flags |= fl
        torch.cuda.synchronize()
        gr.close()
        assert int(flags.sum()) == 0

    def state(self):
        """Fresh buffers of the adjoint iteration, started by admm_adjoint_init from zeros."""
        nan, (nx, nu, N, B) = float("nan"), self.shape
        o = dict(alam=torch.zeros_like(self.lam), wa=torch.zeros_like(self.g), ya=torch.zeros_like(self.g))
        o.update(gamma=torch.full_like(self.lam, nan), r=torch.full_like(self.lam, nan), p=torch.full_like(self.lam, nan),
                 az=torch.full_like(self.g, nan), res=torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda"),
                 it=torch.full((B,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))
        o["gta"] = self.s.admm_adjoint_init(nx, nu, N, B, self.gz, self.y, self.rho, o["wa"], o["ya"])
        return o

    def two_calls(self, o, rho=None):
        nx, nu, N, B = self.shape
        self.s.kkt_resolve(nx, nu, N, B, self.Ginv, self.C, o["gta"], self.nglam, self.S, self.Pinv, o["gamma"], o["alam"], o["az"],
                           r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        self.s.admm_adjoint_update(nx, nu, N, B, self.gz, self.y, self.rho if rho is None else rho, o["az"], o["wa"], o["ya"], o["gta"],
                                   res=o["res"])

    def one_call(self, o, rho=None):
        nx, nu, N, B = self.shape
        self.s.admm_adjoint_step(nx, nu, N, B, self.Ginv, self.C, self.gz, self.nglam, self.y, self.rho if rho is None else rho, self.S,
                                 self.Pinv, o["gamma"], o["alam"], o["az"], o["wa"], o["ya"], o["gta"], res=o["res"], r=o["r"], p=o["p"],
                                 tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])

    def graph(self, o):
        nx, nu, N, B = self.shape
        return self.s.graph_admm_adjoint_step(nx, nu, N, B, self.Ginv, self.C, self.gz, self.nglam, self.y, self.rho, self.S, self.Pinv,
                                              o["gamma"], o["alam"], o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["az"],
                                              o["wa"], o["ya"], o["gta"], o["res"])


ORDER = ("gamma", "alam", "r", "p", "az", "it", "fl", "wa", "ya", "gta", "res")


@pytest.fixture(scope="module")
def kept(solver):
    cache = {}

    def get(nx, nu, N, B, dtype):
        key = (nx, nu, N, B, np.dtype(dtype).name)
        if key not in cache:
            cache[key] = Kept(solver, nx, nu, N, B, dtype)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", ar.FIXTURE_SHAPES)
def test_adjoint_step_is_kkt_resolve_plus_adjoint_update_and_the_graph_is_the_calls(kept, nx, nu, N, B, dtype):
    L = kept(nx, nu, N, B, dtype)
    a, b, g = L.state(), L.state(), L.state()
    gr = L.graph(g)
    for i in range(3):       # every iteration takes the one before's alambda, wa, ya, gta
        L.two_calls(a)
        L.one_call(b)
        gr.launch()
        torch.cuda.synchronize()
        for k in ORDER:
            assert same(a[k], b[k]), (i, k, "step vs resolve + update")
            assert same(g[k], b[k]), (i, k, "graph vs call")
    assert int(b["fl"].sum()) == 0 and all(bool(torch.isfinite(b[k]).all()) for k in ("az", "wa", "ya", "gta", "res"))
    # rho rewritten in place is seen at replay: the update follows the new values (the matrices are what they were, by design)
    rho1 = L.rho.clone()
    rho2 = rho1 + 0.75
    fresh = L.state()
    for k in ("alam", "wa", "ya", "gta"):
        g[k].copy_(fresh[k])
    try:
        L.rho.copy_(rho2)
        gr.launch()
        L.one_call(fresh, rho=rho2.clone())
        torch.cuda.synchronize()
    finally:
        L.rho.copy_(rho1)
        torch.cuda.synchronize()
    gr.close()
    for k in ORDER:
        assert same(g[k], fresh[k]), k
    c = L.state()
    L.one_call(c)
    torch.cuda.synchronize()
    assert same(c["az"], g["az"]) and same(c["wa"], g["wa"]) and not same(c["gta"], g["gta"])     # the solve is the old one, gta is not


# ---- 6. refusals: a NULL in each required slot is INVALID and nothing is written (no call here reaches the device)
@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_bad_arguments(solver, suf, tt):
    nx, nu, N, B = 6, 3, 4, 3
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = torch.zeros(1 << 14, dtype=tt, device="cuda")
    rho = torch.ones(B, dtype=tt, device="cuda")
    WRITTEN = ("gamma", "alam", "r", "p", "az", "wa", "ya", "gta", "res", "glo", "ghi")
    outs = {k: torch.full((1 << 12,), 777.0, dtype=tt, device="cuda") for k in WRITTEN}
    it = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def values(null=(), **over):
        v = {k: P(ins) for k in ("Ginv", "C", "gz", "nglam", "yf", "S", "Pinv")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(it=P(it), fl=P(fl), tol=1e-6, max_iter=10, nx=nx, nu=nu, N=N, batch=B)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    STEP = ("Ginv", "C", "gz", "nglam", "yf", "rho", "S", "Pinv", "gamma", "alam", "r", "p", "tol", "max_iter", "it", "fl", "az", "wa", "ya",
            "gta", "res")
    OPTIONAL = ("Pinv", "r", "p", "fl", "tol", "max_iter")
    graph = ctypes.c_void_p()

    def step(name, v, gr=None):
        last = ctypes.byref(gr) if gr is not None else s
        return getattr(lib, f"gbdpcg_{name}_{suf}")(solver.h, v["nx"], v["nu"], v["N"], v["batch"], *(v[k] for k in STEP), last)

    def single(name, keys, v):
        return getattr(lib, f"gbdpcg_{name}_{suf}")(solver.h, v["nx"], v["nu"], v["N"], v["batch"], *(v[k] for k in keys), s)

    singles = {"admm_adjoint_init": ("gz", "yf", "rho", "wa", "ya", "gta"),
               "admm_adjoint_update": ("gz", "yf", "rho", "az", "wa", "ya", "gta", "res"),
               "admm_grad_bounds": ("yf", "rho", "ya", "glo", "ghi")}
    for name, keys in singles.items():
        for k in keys:
            assert single(name, keys, values(null=(k,))) == 1, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert single(name, keys, values(**{k: 0})) == 1, (name, k)
    for name, gr in (("admm_adjoint_step", None), ("graph_create_admm_adjoint_step", graph)):
        for k in STEP:
            if k not in OPTIONAL:
                assert step(name, values(null=(k,)), gr) == 1, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert step(name, values(**{k: 0}), gr) == 1, (name, k)
        big = dict(nx=80, nu=40) if suf == "f64" else dict(nx=120, nu=60)       # a block size form_schur refuses
        assert step(name, values(**big), gr) == 4, name
    assert getattr(lib, f"gbdpcg_graph_create_admm_adjoint_step_{suf}")(solver.h, nx, nu, N, B, *(values()[k] for k in STEP), None) == 1
    torch.cuda.synchronize()
    assert not graph.value
    assert all(bool((t == 777.0).all()) for t in outs.values()) and bool((it == 777).all()) and bool((fl == 77).all())


# ---- 7. converged gradients on the pinned fixture
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", ar.FIXTURE_SHAPES)
def test_converged_gradients_match_the_dense_reference(solver, kept, nx, nu, N, B, dtype):
    L = kept(nx, nu, N, B, dtype)
    ref, loop = ar.reference(nx, nu, N, B), ar.loop_reference(nx, nu, N, B)
    o = L.state()
    gr = L.graph(o)
    flags = torch.zeros_like(o["fl"])
    for _ in range(ar.K_ADJ):
        gr.launch()
        flags |= o["fl"]
    glo, ghi = solver.admm_grad_bounds(nx, nu, N, B, L.y, L.rho, o["ya"])
    gG, gC = solver.kkt_grad(nx, nu, N, B, L.w, L.lam, o["wa"], o["alam"])
    torch.cuda.synchronize()
    gr.close()
    assert int(flags.sum()) == 0, "an adjoint solve ran out of iterations"
    got = {"G": gG, "C": gC, "g": o["wa"], "c": -o["alam"], "lo": glo, "hi": ghi, "w": L.w, "lam": L.lam}
    got = {k: v.cpu().numpy().astype(F64).reshape(B, -1) for k, v in got.items()}
    y = L.y.cpu().numpy().reshape(B, -1)
    what, replays = np.dtype(dtype).name, ar.K_FWD + ar.K_ADJ
    for b in range(B):
        assert np.array_equal(y[b] < 0, ref[b]["at_lo"]) and np.array_equal(y[b] > 0, ref[b]["at_hi"]), "the mask is not the active set"
        A = ref[b]["at_lo"] | ref[b]["at_hi"]
        assert not got["g"][b][A].any()              # dl/dg is EXACTLY zero on a clamped entry
        assert not got["lo"][b][~ref[b]["at_lo"]].any() and not got["hi"][b][~ref[b]["at_hi"]].any()
        for k in ("w", "lam"):
            err, bound = np.abs(got[k][b] - ref[b][k]).max(), ar.converged_bound(loop[b][k], ref[b][k], ar.K_FWD, STEP_TOL[dtype])
            print(f"{what} ({nx},{nu},{N}) problem {b} {k}: {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (b, k, err, bound)
        for k in ("G", "C", "g", "c", "lo", "hi"):
            dense = ref[b]["grads"][k]
            err, bound = np.abs(got[k][b] - dense).max(), ar.converged_bound(loop[b]["grads"][k], dense, replays, STEP_TOL[dtype])
            print(f"{what} ({nx},{nu},{N}) problem {b} d{k}: {err:.3e} (bound {bound:.3e}, scale {np.abs(dense).max():.3e})")
            assert err <= bound, (b, k, err, bound)
