"""The backward pass of the hard linear-row QP on the device (the adjoint instantiations of csrc/admm_rows.hip, csrc/admm_lin_grad.hip
and their composite calls in csrc/api_kkt.hip, through the C ABI): gbdpcg_admm_lin_adjoint_init_*, gbdpcg_admm_lin_adjoint_update_*,
gbdpcg_admm_lin_adjoint_step_* and its graph, gbdpcg_admm_lin_grad_*.
PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.

Reference: tests/admm_lin_adjoint_ref.py.  Every output is defined to the bit, so w, y, gt and the two norms are compared for
EQUALITY with update_ref in the call's precision AND with gbdpcg_admm_lin_update_* / _init_* on the explicit degenerate rows, and
with gbdpcg_admm_adjoint_* where E = I; glo, ghi, gE with grad_ref and gbdpcg_admm_grad_bounds_* on (mx, mu, N).  The composite
calls are compared bit for bit with the calls they are made of.  Converged gradients: after K_FWD forward and K_ADJ adjoint replays
on the pinned fixture every gradient is within admm_adjoint_ref.converged_bound of the dense reference -- twice the fp64 loops' own
distance at those counts plus STEP_TOL (tests/test_gpu_admm.py, copied) accumulated over the replays.  Run with -s for the figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_adjoint_ref as la  # noqa: E402
import admm_lin_ref as lr  # noqa: E402
from admm_util import dev, knot_chunk, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_admm.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
NC = knot_chunk(14, 7, 4, 2)
SHAPES = [(2, 1, 3, 2, 1, 1),          # smallest
          (3, 2, 1, 2, 2, 0),          # N = 1, no input block
          (2, 1, 4, 2, 5, 0),          # more rows than columns
          (4, 3, 3, 2, 0, 2),          # no state rows
          (14, 7, 5, 3, 3, 2),         # the workload's block size
          (14, 7, NC + 1, 2, 4, 2),    # one knot past a chunk of the update
          (14, 7, 3, 2, 64, 64),       # the row limit
          (5, 2, 3, 4, 3, 1)]          # ne = 49, nw = 11: across four problems every 16-byte head length, fp32 and fp64
GRAD_SHAPES = SHAPES + [(5, 2, 70, 2, 3, 1)]     # the grad launch stages at most 64 knots at a time: two chunks
OFFSETS = [0, 1]                       # 16-byte aligned bases / every base off by one element


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def data(nx, nu, N, B, mx, mu, dtype):
    """az, z, gz [B, nz], w, y [B, nw], E [B, ne] of order 1; yf zero on about half of the rows with both signs elsewhere and +-0, a
    NaN (active) planted; a NaN in az of the last problem makes v NaN on the rows of its first block; w_0 = -0 under a pin (the init
    keeps it -0; a chain seeded with +0 never ends in -0, so in the update s = -0 cannot occur: there y_0 = -0 gives s = v).
    Read-only; lo, hi: the explicit degenerate rows of yf."""
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(3000 + 7 * nz + nw)
    az, z, gz = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(3))
    w, y = (rng.standard_normal((B, nw)).astype(dtype) for _ in range(2))
    E = rng.standard_normal((B, ne)).astype(dtype)
    yf = np.where(rng.random((B, nw)) < 0.5, 0.0, rng.standard_normal((B, nw))).astype(dtype)
    w[0, 0], y[0, 0], yf[0, 0] = -0.0, -0.0, 1.0        # pinned
    yf[0, nw - 1] = -0.0                        # free: -0 != 0 is false
    yf[B - 1, nw // 2] = np.nan                 # active
    az[B - 1, 0 if mx else nx] = np.nan         # a column of the first block that has rows, in the last problem
    rho = rng.uniform(0.5, 4.0, B).astype(dtype)
    lo, hi = la.degenerate_rows(yf, dtype)
    d = dict(az=az, z=z, w=w, y=y, gz=gz, E=E, yf=yf, rho=rho, lo=lo, hi=hi)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, mx, mu, dtype, init):
    d = data(nx, nu, N, B, mx, mu, dtype)
    return la.update_ref(dtype, nx, nu, mx, mu, N, d["gz"], d["E"], d["yf"], d["rho"], None if init else d["az"], d["w"], d["y"])


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
    nx, nu, N, B, mx, mu = shape
    if init:
        solver.admm_lin_adjoint_init(nx, nu, mx, mu, N, B, t["gz"], t["E"], t["yf"], t["rho"], t["w"], t["y"], gta=t["gt"])
    else:
        solver.admm_lin_adjoint_update(nx, nu, mx, mu, N, B, t["gz"], t["E"], t["yf"], t["rho"], t["az"], t["w"], t["y"], t["gt"],
                                       res=t["res"])


def run_rows(solver, shape, t, init):
    nx, nu, N, B, mx, mu = shape
    if init:
        solver.admm_lin_init(nx, nu, mx, mu, N, B, t["gz"], t["E"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
    else:
        solver.admm_lin_update(nx, nu, mx, mu, N, B, t["gz"], t["E"], t["lo"], t["hi"], t["rho"], t["az"], t["w"], t["y"], t["gt"],
                               res=t["res"])


def outputs(init):
    return ("w", "gt") if init else ("w", "y", "gt", "res")


# ---- 1. bits: against the exact reference and against the rows kernel on the explicit degenerate rows, both alignments
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", SHAPES)
def test_bits_vs_reference_and_vs_rows_update(solver, nx, nu, N, B, mx, mu, dtype, init):
    shape = (nx, nu, N, B, mx, mu)
    d = data(*shape, dtype)
    wr, yr, gr, rr = reference(*shape, dtype, init)
    what = f"{shape} {np.dtype(dtype).name} {'init' if init else 'update'}"
    outs = []
    for offset in OFFSETS:
        t, _ = device_tensors(d, offset)
        run_adjoint(solver, shape, t, init)
        tb, _ = device_tensors(d, offset)
        run_rows(solver, shape, tb, init)
        torch.cuda.synchronize()
        for k in ("w", "y", "gt") + (() if init else ("res",)):
            assert same(t[k], tb[k]), f"{what} offset {offset}: {k} differs from the rows kernel on the degenerate rows"
        assert np_same(t["w"].cpu().numpy().reshape(B, -1), wr), what + ": w"
        assert np_same(t["y"].cpu().numpy().reshape(B, -1), yr), what + ": y"
        assert np_same(t["gt"].cpu().numpy().reshape(B, -1), gr), what + ": gt"
        if not init:
            assert np_same(t["res"].cpu().numpy().reshape(B, 2), rr), what + ": res"
        outs.append({k: t[k].clone() for k in ("w", "y", "gt", "res")})
    for k in outs[0]:
        assert same(outs[0][k], outs[1][k]), f"{what}: {k}, aligned vs misaligned"
    w = outs[0]["w"].cpu().numpy().reshape(B, -1)
    m = d["yf"] != 0
    assert (np.isnan(w[m]) | (w[m] == 0)).all()                          # pinned rows are zero (or the NaN that came in)
    if init:
        assert np.signbit(w[0, 0]) and w[0, 0] == 0                      # w = -0 under a pin stays -0
    else:
        y = outs[0]["y"].cpu().numpy().reshape(B, -1)
        assert not y[~m & np.isfinite(w)].any()                          # free rows: the identity projection, y+ = s - s
        assert bool(torch.isnan(outs[0]["res"].view(B, 2)[B - 1]).all())         # the planted NaN is its problem's norm ...
        assert bool(torch.isfinite(outs[0]["res"].view(B, 2)[:B - 1]).all())      # ... and stays there


# ---- 2. E = I: the bits of the box adjoint
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(3, 2, 4, 3), (14, 7, 3, 2)])
def test_identity_rows_give_the_bits_of_the_box_adjoint(solver, nx, nu, N, B, dtype, init):
    nz = (nx + nu) * N - nu
    rng = np.random.default_rng(11)
    az, gz, w, y = (dev(rng.standard_normal(B * nz).astype(dtype)) for _ in range(4))
    yf = dev(np.where(rng.random(B * nz) < 0.5, 0.0, rng.standard_normal(B * nz)).astype(dtype))
    rho = dev(rng.uniform(0.5, 4.0, B).astype(dtype))
    E = dev(np.tile(lr.identity_E(nx, nu, N, dtype), B))
    a, b = dict(w=w.clone(), y=y.clone()), dict(w=w.clone(), y=y.clone())
    if init:
        a["gt"] = solver.admm_lin_adjoint_init(nx, nu, nx, nu, N, B, gz, E, yf, rho, a["w"], a["y"])
        b["gt"] = solver.admm_adjoint_init(nx, nu, N, B, gz, yf, rho, b["w"], b["y"])
    else:
        a["gt"], b["gt"] = torch.empty_like(gz), torch.empty_like(gz)
        a["res"] = solver.admm_lin_adjoint_update(nx, nu, nx, nu, N, B, gz, E, yf, rho, az, a["w"], a["y"], a["gt"])
        b["res"] = solver.admm_adjoint_update(nx, nu, N, B, gz, yf, rho, az, b["w"], b["y"], b["gt"])
    torch.cuda.synchronize()
    for k in a:
        assert same(a[k], b[k]), k


# ---- 3. the grad launch
def run_grad(solver, shape, t, which="lhE"):
    nx, nu, N, B, mx, mu = shape
    solver.admm_lin_grad(nx, nu, mx, mu, N, B, t["z"], t["az"], t["yf"], t["y"], t["rho"], glo=t["glo"] if "l" in which else None,
                         ghi=t["ghi"] if "h" in which else None, gE=t["gE"] if "E" in which else None, want="")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", GRAD_SHAPES)
def test_grad_bits_subsets_alignment_and_footprint(solver, nx, nu, N, B, mx, mu, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = data(*shape, dtype)
    glo_r, ghi_r, gE_r = la.grad_ref(dtype, nx, nu, mx, mu, N, d["z"], d["az"], d["yf"], d["y"], d["rho"])
    ref = dict(glo=glo_r, ghi=ghi_r, gE=gE_r)
    extra = [("glo", np.full_like(d["yf"], np.nan)), ("ghi", np.full_like(d["yf"], np.nan)), ("gE", np.full_like(d["E"], np.nan))]
    full = []
    for offset in OFFSETS:
        t, bufs = device_tensors(d, offset, extra=extra)
        before = {k: b.clone() for k, b in bufs.items()}
        run_grad(solver, shape, t)
        torch.cuda.synchronize()
        for k in ("glo", "ghi", "gE"):
            assert np_same(t[k].cpu().numpy().reshape(B, -1), ref[k]), (k, offset)
            o, n = 8 + offset, t[k].numel()
            assert bool(torch.isnan(bufs[k][:o]).all()) and bool(torch.isnan(bufs[k][o + n:]).all()), f"guard of {k}"
        for k in bufs:
            if k not in ("glo", "ghi", "gE"):
                assert same(bufs[k], before[k]), f"{k} was written"
        full.append({k: t[k].clone() for k in ("glo", "ghi", "gE")})
        # glo, ghi: the bits of gbdpcg_admm_grad_bounds_* called with (mx, mu, N) in the place of (nx, nu, N)
        if mx and mu:
            blo, bhi = solver.admm_grad_bounds(mx, mu, N, B, t["yf"], t["rho"], t["y"])
            torch.cuda.synchronize()
            assert same(blo, t["glo"]) and same(bhi, t["ghi"])
        # every subset of NULL outputs: what is asked for has the same bits, what is not is not written
        for which in ("l", "h", "E", "lh", "lE", "hE"):
            s, sb = device_tensors(d, offset, extra=extra)
            run_grad(solver, shape, s, which)
            torch.cuda.synchronize()
            for c, k in (("l", "glo"), ("h", "ghi"), ("E", "gE")):
                if c in which:
                    assert same(s[k], t[k]), (which, k)
                else:
                    assert bool(torch.isnan(sb[k]).all()), (which, k)
    for k in full[0]:
        assert same(full[0][k], full[1][k]), f"{k}: aligned vs misaligned"
    dense = np.stack([lr.dense_E(nx, nu, mx, mu, N, gE_r[b]) for b in range(B)])
    free = d["yf"] == 0
    assert not dense[free].any()                # +0 on the free rows (-0 in yf is free)


# ---- 4. footprint of the update: guard words around every output, inputs untouched, nothing read from res
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", [(14, 7, 5, 3, 3, 2), (14, 7, NC + 1, 2, 4, 2)])
def test_footprint(solver, nx, nu, N, B, mx, mu, dtype, init):
    shape = (nx, nu, N, B, mx, mu)
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
        for k in bufs:
            if k not in outputs(init):
                assert same(bufs[k], before[k]), f"{k} was written"
        results.append({k: t[k].clone() for k in outputs(init)})
    for k in results[0]:
        assert same(results[0][k], results[1][k]), k     # nothing is read from res


# ---- 5. isolation
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_problem(solver, dtype):
    shape = (14, 7, 5, 3, 3, 2)
    nx, nu, N, B, mx, mu = shape
    d = data(*shape, dtype)
    extra = [("glo", np.full_like(d["yf"], np.nan)), ("ghi", np.full_like(d["yf"], np.nan)), ("gE", np.full_like(d["E"], np.nan))]
    clean, _ = device_tensors(d, extra=extra)
    run_adjoint(solver, shape, clean, False)
    run_grad(solver, shape, clean)
    t, _ = device_tensors(d, extra=extra)
    for k in ("az", "y", "z", "E"):
        t[k].view(B, -1)[1, 3] = float("nan")
    run_adjoint(solver, shape, t, False)
    run_grad(solver, shape, t)
    torch.cuda.synchronize()
    assert bool(torch.isnan(t["res"].view(B, 2)[1]).all())
    for p in (0,):          # (problem B - 1 carries the planted NaN of data() in both runs: equal bits all the same)
        for k in ("w", "y", "gt", "res", "glo", "ghi", "gE"):
            assert same(t[k].view(B, -1)[p], clean[k].view(B, -1)[p]), (k, p)
    for k in ("w", "y", "gt", "res", "glo", "ghi", "gE"):
        assert same(t[k].view(B, -1)[2], clean[k].view(B, -1)[2]), k
    assert bool(torch.isfinite(t["res"].view(B, 2)[0]).all())


# ---- 6. composition: the kept factorisation of the pinned fixture, its converged forward y as the mask
class Kept:
    """admm_lin_form + kkt_step on a fixture of admm_lin_adjoint_ref, K_FWD replays of the forward graph, and the buffers of the
    adjoint iteration."""

    def __init__(self, solver, nx, nu, N, B, dtype, max_iter=200):
        self.s, self.shape, self.tol, self.max_iter, self.dtype = solver, (nx, nu, N, B), PCG_TOL[dtype], max_iter, dtype
        self.mx, self.mu = mx, mu = la.FIXTURE_ROWS[(nx, nu, N, B)]
        d, E, lo, hi, gz, glam = la.fixture(nx, nu, N, B)
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        self.E, self.lo, self.hi = (dev(a.astype(dtype).reshape(-1)) for a in (E, lo, hi))
        self.gz, self.nglam = dev(gz.astype(dtype).reshape(-1)), dev((-glam).astype(dtype).reshape(-1))
        self.rho = dev(np.asarray(la.FIXTURE_RHO[:B], dtype))
        nan = float("nan")
        self.S = torch.full((B * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        gamma = torch.full((B * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, self.z = torch.zeros_like(gamma), torch.full_like(self.g, nan)
        r, p = torch.full_like(gamma, nan), torch.full_like(gamma, nan)
        Gt = solver.admm_lin_form(nx, nu, mx, mu, N, B, self.G, self.E, self.rho)
        it, fl = solver.kkt_step(nx, nu, N, B, Gt, self.C, self.g, self.c, self.S, gamma, self.Ginv, self.Pinv, self.lam, self.z,
                                 tol=self.tol, max_iter=max_iter)
        self.w, self.y = torch.zeros_like(self.lo), torch.zeros_like(self.lo)
        gt = solver.admm_lin_init(nx, nu, mx, mu, N, B, self.g, self.E, self.lo, self.hi, self.rho, self.w, self.y)
        res = torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda")
        solver.reserve(self.g.element_size(), nx, N, B)
        gr = solver.graph_admm_lin_step(nx, nu, mx, mu, N, B, self.Ginv, self.C, self.g, self.c, self.E, self.lo, self.hi, self.rho,
                                        self.S, self.Pinv, gamma, self.lam, r, p, self.tol, max_iter, it, fl, self.z, self.w, self.y, gt,
                                        res)
        flags = torch.zeros_like(fl)
        for _ in range(la.K_FWD):
            gr.launch()
            flags |= fl
        torch.cuda.synchronize()
        gr.close()
        assert int(flags.sum()) == 0

    def state(self):
        """Fresh buffers of the adjoint iteration, started by admm_lin_adjoint_init from zeros."""
        nan, (nx, nu, N, B) = float("nan"), self.shape
        o = dict(alam=torch.zeros_like(self.lam), wa=torch.zeros_like(self.y), ya=torch.zeros_like(self.y))
        o.update(gamma=torch.full_like(self.lam, nan), r=torch.full_like(self.lam, nan), p=torch.full_like(self.lam, nan),
                 az=torch.full_like(self.g, nan), res=torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda"),
                 it=torch.full((B,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))
        o["gta"] = self.s.admm_lin_adjoint_init(nx, nu, self.mx, self.mu, N, B, self.gz, self.E, self.y, self.rho, o["wa"], o["ya"])
        return o

    def two_calls(self, o):
        nx, nu, N, B = self.shape
        self.s.kkt_resolve(nx, nu, N, B, self.Ginv, self.C, o["gta"], self.nglam, self.S, self.Pinv, o["gamma"], o["alam"], o["az"],
                           r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        self.s.admm_lin_adjoint_update(nx, nu, self.mx, self.mu, N, B, self.gz, self.E, self.y, self.rho, o["az"], o["wa"], o["ya"],
                                       o["gta"], res=o["res"])

    def one_call(self, o):
        nx, nu, N, B = self.shape
        self.s.admm_lin_adjoint_step(nx, nu, self.mx, self.mu, N, B, self.Ginv, self.C, self.gz, self.nglam, self.E, self.y, self.rho,
                                     self.S, self.Pinv, o["gamma"], o["alam"], o["az"], o["wa"], o["ya"], o["gta"], res=o["res"],
                                     r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])

    def graph(self, o):
        nx, nu, N, B = self.shape
        return self.s.graph_admm_lin_adjoint_step(nx, nu, self.mx, self.mu, N, B, self.Ginv, self.C, self.gz, self.nglam, self.E, self.y,
                                                  self.rho, self.S, self.Pinv, o["gamma"], o["alam"], o["r"], o["p"], self.tol,
                                                  self.max_iter, o["it"], o["fl"], o["az"], o["wa"], o["ya"], o["gta"], o["res"])


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


@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", la.FIXTURE_SHAPES)
def test_adjoint_step_is_kkt_resolve_plus_update_and_the_graph_is_the_calls(solver, kept, nx, nu, N, B, dtype, mode):
    L = kept(nx, nu, N, B, dtype)
    solver.set_symmetric(mode)
    try:
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
        gr.close()
        assert int(b["fl"].sum()) == 0 and all(bool(torch.isfinite(b[k]).all()) for k in ("az", "wa", "ya", "gta", "res"))
    finally:
        solver.set_symmetric(2)


# ---- 7. refusals: nothing is written (no call here reaches the device)
@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_bad_arguments(solver, suf, tt):
    nx, nu, mx, mu, N, B = 6, 3, 3, 2, 4, 3
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = torch.zeros(1 << 14, dtype=tt, device="cuda")
    rho = torch.ones(B, dtype=tt, device="cuda")
    WRITTEN = ("gamma", "alam", "r", "p", "az", "wa", "ya", "gta", "res", "glo", "ghi", "gE")
    outs = {k: torch.full((1 << 12,), 777.0, dtype=tt, device="cuda") for k in WRITTEN}
    it = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def values(null=(), **over):
        v = {k: P(ins) for k in ("Ginv", "C", "gz", "nglam", "E", "yf", "S", "Pinv", "z")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(it=P(it), fl=P(fl), tol=1e-6, max_iter=10, nx=nx, nu=nu, mx=mx, mu=mu, N=N, batch=B)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    SIZES = ("nx", "nu", "mx", "mu", "N", "batch")
    STEP = ("Ginv", "C", "gz", "nglam", "E", "yf", "rho", "S", "Pinv", "gamma", "alam", "r", "p", "tol", "max_iter", "it", "fl", "az", "wa",
            "ya", "gta", "res")
    OPTIONAL = ("Pinv", "r", "p", "fl", "tol", "max_iter")
    graph = ctypes.c_void_p()

    def step(name, v, gr=None):
        last = ctypes.byref(gr) if gr is not None else s
        return getattr(lib, f"gbdpcg_{name}_{suf}")(solver.h, *(v[k] for k in SIZES), *(v[k] for k in STEP), last)

    def single(name, keys, v):
        return getattr(lib, f"gbdpcg_{name}_{suf}")(solver.h, *(v[k] for k in SIZES), *(v[k] for k in keys), s)

    singles = {"admm_lin_adjoint_init": ("gz", "E", "yf", "rho", "wa", "ya", "gta"),
               "admm_lin_adjoint_update": ("gz", "E", "yf", "rho", "az", "wa", "ya", "gta", "res"),
               "admm_lin_grad": ("z", "az", "yf", "ya", "rho", "glo", "ghi", "gE")}
    for name, keys in singles.items():
        for k in keys:
            if k not in ("glo", "ghi", "gE"):
                assert single(name, keys, values(null=(k,))) == 1, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert single(name, keys, values(**{k: 0})) == 1, (name, k)
        assert single(name, keys, values(mx=0, mu=0)) == 1, name                       # no rows at all
        assert single(name, keys, values(mx=65)) == 4 and single(name, keys, values(mu=65)) == 4, name     # past the row limit
        assert single(name, keys, values(nx=4000, nu=4000, mx=1, mu=1)) == 4, name     # a knot past the LDS
        assert single(name, keys, values(batch=1 << 31)) != 0, name                    # one workgroup per problem
    assert single("admm_lin_grad", singles["admm_lin_grad"], values(null=("glo", "ghi", "gE"))) == 1
    for name, gr in (("admm_lin_adjoint_step", None), ("graph_create_admm_lin_adjoint_step", graph)):
        for k in STEP:
            if k not in OPTIONAL:
                assert step(name, values(null=(k,)), gr) == 1, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert step(name, values(**{k: 0}), gr) == 1, (name, k)
        assert step(name, values(mx=0, mu=0), gr) == 1, name
        assert step(name, values(mx=65), gr) == 4, name
        big = dict(nx=80, nu=40) if suf == "f64" else dict(nx=120, nu=60)       # a block size form_schur refuses
        assert step(name, values(**big), gr) == 4, name
    assert getattr(lib, f"gbdpcg_graph_create_admm_lin_adjoint_step_{suf}")(solver.h, *(values()[k] for k in SIZES),
                                                                           *(values()[k] for k in STEP), None) == 1
    torch.cuda.synchronize()
    assert not graph.value
    assert all(bool((t == 777.0).all()) for t in outs.values()) and bool((it == 777).all()) and bool((fl == 77).all())


# ---- 8. converged gradients on the pinned fixture
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", la.FIXTURE_SHAPES)
def test_converged_gradients_match_the_dense_reference(solver, kept, nx, nu, N, B, dtype):
    L = kept(nx, nu, N, B, dtype)
    mx, mu = L.mx, L.mu
    ref, loop = la.reference(nx, nu, N, B), la.loop_reference(nx, nu, N, B)
    o = L.state()
    gr = L.graph(o)
    flags = torch.zeros_like(o["fl"])
    for _ in range(la.K_ADJ):
        gr.launch()
        flags |= o["fl"]
    glo, ghi, gE = solver.admm_lin_grad(nx, nu, mx, mu, N, B, L.z, o["az"], L.y, o["ya"], L.rho)
    gG, gC = solver.kkt_grad(nx, nu, N, B, L.z, L.lam, o["az"], o["alam"])
    torch.cuda.synchronize()
    gr.close()
    assert int(flags.sum()) == 0, "an adjoint solve ran out of iterations"
    got = {"G": gG, "C": gC, "g": o["az"], "c": -o["alam"], "E": gE, "lo": glo, "hi": ghi, "z": L.z, "lam": L.lam}
    got = {k: v.cpu().numpy().astype(F64).reshape(B, -1) for k, v in got.items()}
    y, ya = L.y.cpu().numpy().reshape(B, -1), o["ya"].cpu().numpy().reshape(B, -1)
    what, replays = np.dtype(dtype).name, la.K_FWD + la.K_ADJ
    for b in range(B):
        assert np.array_equal(y[b] < 0, ref[b]["at_lo"]) and np.array_equal(y[b] > 0, ref[b]["at_hi"]), "the mask is not the active set"
        A = ref[b]["at_lo"] | ref[b]["at_hi"]
        assert not ya[b][~A].any()                   # from ya = 0 an inactive row's ya stays exactly 0
        assert not got["lo"][b][~ref[b]["at_lo"]].any() and not got["hi"][b][~ref[b]["at_hi"]].any()
        assert not lr.dense_E(nx, nu, mx, mu, N, got["E"][b])[~A].any()
        for k in ("z", "lam"):
            err, bound = np.abs(got[k][b] - ref[b][k]).max(), la.converged_bound(loop[b][k], ref[b][k], la.K_FWD, STEP_TOL[dtype])
            print(f"{what} ({nx},{nu},{N}) problem {b} {k}: {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (b, k, err, bound)
        for k in ("G", "C", "g", "c", "E", "lo", "hi"):
            dense = ref[b]["grads"][k]
            err, bound = np.abs(got[k][b] - dense).max(), la.converged_bound(loop[b]["grads"][k], dense, replays, STEP_TOL[dtype])
            print(f"{what} ({nx},{nu},{N}) problem {b} d{k}: {err:.3e} (bound {bound:.3e}, scale {np.abs(dense).max():.3e})")
            assert err <= bound, (b, k, err, bound)
