"""The backward pass of the soft (L1-penalised) box and rows QPs on the device (csrc/admm_box_grad.hip, the SOFT instantiation of
csrc/admm_lin_grad.hip, through the C ABI): gbdpcg_admm_soft_mask_*, gbdpcg_admm_lin_soft_mask_*, gbdpcg_admm_soft_grad_bounds_*,
gbdpcg_admm_lin_soft_grad_*.
PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.

Reference: tests/admm_soft_adjoint_ref.py.  Every output is defined to the bit, so ym, glo, ghi, gkappa and gE are compared for
EQUALITY with the reference in the call's precision at aligned and misaligned bases, and with the existing calls they must agree
with: glo, ghi with gbdpcg_admm_grad_bounds_* on ym, gE with gbdpcg_admm_lin_grad_* on the unmasked yf, the rows calls with E = I
with the box calls, everything with the hard calls where kappa = +Inf.

Composition: the forward soft loop, the mask, the HARD adjoint loop on ym, the soft gradient launch and gbdpcg_kkt_grad_* on the
pinned fixtures.  The device's three sets equal the reference's for every problem, and every gradient is within
admm_adjoint_ref.converged_bound of the dense fp64 reference -- the bound of
tests/test_gpu_admm_lin_adjoint.py::test_converged_gradients_match_the_dense_reference, the same quantity on the hard fixture: twice
the fp64 loops' own distance at K_FWD, K_ADJ plus STEP_TOL accumulated over the replays.  Run with -s for the figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_ref as lr  # noqa: E402
import admm_soft_adjoint_ref as sa  # noqa: E402
from admm_util import dev, np_same, np_same_or_nan, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_admm.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
# nx, nu, N, B, mx, mu.  (14, 7, 3) and (5, 2, 3, 4) are the shapes of tests/test_gpu_admm_adjoint.py: nz = 56 and nz = 19, so that
# across four problems every 16-byte head length occurs; N = 1 has no u block; N = 70 crosses the 64-knot chunk of the grad launch and
# ends on a short one.
ROW_SHAPES = [(14, 7, 3, 3, 4, 2), (5, 2, 3, 4, 3, 1), (14, 7, 1, 2, 10, 3), (14, 7, 70, 3, 4, 2)]
BOX_SHAPES = [(14, 7, 3, 3), (5, 2, 3, 4), (14, 7, 1, 2)]
OFFSETS = [0, 1]                       # 16-byte aligned bases / every base off by one element
GUARD = 8


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def data(nx, nu, N, B, mx, mu, dtype, identity=False):
    """z, az [B, nz], ya, yf, kappa [B, nw], E [B, ne] (the identity blocks when asked), rho [B] of order 1.  kappa is finite on most rows,
    +Inf on a fifth, 0 on a tenth; yf is 0 on a third of the rows, exactly +-theta on a third (saturated), strictly inside theta on the
    rest (held).  Written into yf and kappa directly, in problem 0: the tie |yf| = theta on both signs, yf = +-0 under a finite kappa,
    a NaN yf, kappa = 0 under +-0 and under a finite yf, kappa = +Inf next to a finite kappa.  A NaN in az of the LAST problem.
    Read-only."""
    nz, nw, ne, _ = lr.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(4100 + 7 * nz + nw)
    z, az = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(2))
    ya = rng.standard_normal((B, nw)).astype(dtype)
    E = np.tile(lr.identity_E(nx, nu, N, dtype), (B, 1)) if identity else rng.standard_normal((B, ne)).astype(dtype)
    rho = rng.uniform(0.5, 4.0, B).astype(dtype)
    kappa = rng.uniform(0.5, 2.0, (B, nw)).astype(dtype)
    u = rng.random((B, nw))
    kappa[u < 0.2], kappa[u > 0.9] = np.inf, 0.0
    theta = sa.theta_of(kappa, rho)
    u = rng.random((B, nw))
    sign = np.where(rng.random((B, nw)) < 0.5, -1.0, 1.0).astype(dtype)
    scale = np.where(np.isfinite(theta) & (theta > 0), theta, dtype(1.0)).astype(dtype)
    inside = (sign * scale * rng.uniform(0.1, 0.9, (B, nw)).astype(dtype)).astype(dtype)
    yf = np.where(u < 0.33, dtype(0.0), np.where((u < 0.66) & np.isfinite(theta), sign * theta, inside)).astype(dtype)
    assert nw >= 9
    kappa[0, :9] = [1.25, 1.25, 1.5, 1.5, 0.75, 0.0, 0.0, 0.0, np.inf]
    tie = dtype(1.25) / rho[0]
    yf[0, :9] = [tie, -tie, 0.0, -0.0, np.nan, 0.0, -0.0, 0.5, 0.5]
    az[B - 1, 0 if mx else nx] = np.nan
    d = dict(z=z, az=az, ya=ya, E=E, yf=yf, kappa=kappa, rho=rho)
    for a in d.values():
        a.setflags(write=False)
    return d


OUTS = ("ym", "glo", "ghi", "gk", "gE")


def device_tensors(d, offset=0, guard=GUARD):
    """The arrays of data() on the device, flat, plus the outputs (NaN): every array starts `offset` elements into a buffer of its own
    whose base the allocator aligns.  Returns (views, buffers)."""
    t, bufs = {}, {}
    nanlike = lambda a: np.full_like(a, np.nan)  # noqa: E731
    items = list(d.items()) + [("ym", nanlike(d["yf"])), ("glo", nanlike(d["yf"])), ("ghi", nanlike(d["yf"])), ("gk", nanlike(d["yf"])),
                               ("gE", nanlike(d["E"]))]
    for k, a in items:
        flat = dev(a.reshape(-1))
        off = 0 if k == "rho" else offset
        buf = torch.full((flat.numel() + 2 * guard,), float("nan"), dtype=flat.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0 and (guard * flat.element_size()) % 16 == 0
        buf[guard + off:guard + off + flat.numel()] = flat
        t[k], bufs[k] = buf[guard + off:guard + off + flat.numel()], buf
    return t, bufs


def guards_intact(bufs, t, offset, keys):
    for k in keys:
        o, n = GUARD + offset, t[k].numel()
        if not (bool(torch.isnan(bufs[k][:o]).all()) and bool(torch.isnan(bufs[k][o + n:]).all())):
            return False
    return True


def run_lin_grad(solver, shape, t, which="lhkE"):
    nx, nu, N, B, mx, mu = shape
    pick = lambda c, k: t[k] if c in which else None  # noqa: E731
    solver.admm_lin_soft_grad(nx, nu, mx, mu, N, B, t["z"], t["az"], t["E"], t["yf"], t["ya"], t["kappa"], t["rho"], glo=pick("l", "glo"),
                              ghi=pick("h", "ghi"), gkappa=pick("k", "gk"), gE=pick("E", "gE"), want="")


def run_box_grad(solver, shape, t, which="lhk"):
    nx, nu, N, B = shape[:4]
    pick = lambda c, k: t[k] if c in which else None  # noqa: E731
    solver.admm_soft_grad_bounds(nx, nu, N, B, t["yf"], t["kappa"], t["rho"], t["ya"], t["az"], glo=pick("l", "glo"), ghi=pick("h", "ghi"),
                                 gkappa=pick("k", "gk"), want="")


# ---- 1. the mask: bits, both alignments, footprint, both forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", ROW_SHAPES + [(nx, nu, N, B, nx, nu) for nx, nu, N, B in BOX_SHAPES])
def test_mask_bits_alignment_and_footprint(solver, nx, nu, N, B, mx, mu, dtype):
    box = (mx, mu) == (nx, nu)
    d = data(nx, nu, N, B, mx, mu, dtype, identity=box)
    want = sa.mask_ref(dtype, d["yf"], d["kappa"], d["rho"])
    got = []
    for offset in OFFSETS:
        t, bufs = device_tensors(d, offset)
        before = {k: b.clone() for k, b in bufs.items()}
        solver.admm_lin_soft_mask(nx, nu, mx, mu, N, B, t["yf"], t["kappa"], t["rho"], ym=t["ym"])
        if box:      # the box form over the same nz elements: the same kernel, the same bits
            ymb = solver.admm_soft_mask(nx, nu, N, B, t["yf"], t["kappa"], t["rho"])
        torch.cuda.synchronize()
        assert np_same(t["ym"].cpu().numpy().reshape(B, -1), want), offset
        assert not box or same(ymb, t["ym"])
        assert guards_intact(bufs, t, offset, ("ym",))
        for k in bufs:
            if k != "ym":
                assert same(bufs[k], before[k]), f"{k} was written"
        got.append(t["ym"].clone())
    assert same(got[0], got[1])
    ym = want[0]
    assert not ym[:2].view(np.uint8).any()                                  # the ties, both signs: saturated, +0
    assert ym[2] == 0 and not np.signbit(ym[2]) and np.signbit(ym[3])       # +-0 under a finite kappa: the bits of yf
    assert np.isnan(ym[4])                                                  # a NaN passes: held
    assert not ym[5:8].view(np.uint8).any()                                 # kappa = 0: +0 whatever yf holds
    assert ym[8] == dtype(0.5)                                              # kappa = +Inf: yf


# ---- 2. the box gradients: bits, subsets, footprint, and the hard launch on ym
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", BOX_SHAPES)
def test_box_grad_bits_subsets_alignment_and_footprint(solver, nx, nu, N, B, dtype):
    shape = (nx, nu, N, B, nx, nu)
    d = data(*shape, dtype, identity=True)
    ref = dict(zip(("glo", "ghi", "gk"), sa.grad_bounds_ref(dtype, d["yf"], d["kappa"], d["rho"], d["ya"], d["az"])))
    full = []
    for offset in OFFSETS:
        t, bufs = device_tensors(d, offset)
        before = {k: b.clone() for k, b in bufs.items()}
        run_box_grad(solver, shape, t)
        ym = solver.admm_soft_mask(nx, nu, N, B, t["yf"], t["kappa"], t["rho"])
        blo, bhi = solver.admm_grad_bounds(nx, nu, N, B, ym, t["rho"], t["ya"])
        torch.cuda.synchronize()
        for k in ("glo", "ghi"):
            assert np_same(t[k].cpu().numpy().reshape(B, -1), ref[k]), (k, offset)
        assert np_same_or_nan(t["gk"].cpu().numpy().reshape(B, -1), ref["gk"]), offset
        assert same(blo, t["glo"]) and same(bhi, t["ghi"])                  # the bits of gbdpcg_admm_grad_bounds_* called with ym
        assert guards_intact(bufs, t, offset, ("glo", "ghi", "gk"))
        for k in bufs:
            if k not in ("glo", "ghi", "gk"):
                assert same(bufs[k], before[k]), f"{k} was written"
        full.append({k: t[k].clone() for k in ("glo", "ghi", "gk")})
        for which in ("l", "h", "k", "lh", "lk", "hk"):
            s, sb = device_tensors(d, offset)
            run_box_grad(solver, shape, s, which)
            torch.cuda.synchronize()
            for c, k in (("l", "glo"), ("h", "ghi"), ("k", "gk")):
                if c in which:
                    assert same(s[k], t[k]), (which, k)
                else:
                    assert bool(torch.isnan(sb[k]).all()), (which, k)
    for k in full[0]:
        assert same(full[0][k], full[1][k]), f"{k}: aligned vs misaligned"
    gk = ref["gk"][0]
    assert gk[0] == d["az"][0, 0] and gk[1] == -d["az"][0, 1]               # the ties: saturated at hi / at lo
    assert not gk[2:5].view(np.uint8).any() and not gk[8:9].view(np.uint8).any()        # free, held (NaN), hard: +0
    assert gk[5] == -d["az"][0, 5] and gk[7] == d["az"][0, 7]               # kappa = 0: saturated by the line, the side from yf > 0


# ---- 3. the rows gradients: bits, subsets, footprint, the hard launches, E = I
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", ROW_SHAPES)
def test_rows_grad_bits_subsets_alignment_and_footprint(solver, nx, nu, N, B, mx, mu, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = data(*shape, dtype)
    ref = dict(zip(("glo", "ghi", "gk", "gE"), sa.lin_grad_ref(dtype, nx, nu, mx, mu, N, d["z"], d["az"], d["E"], d["yf"], d["ya"], d["kappa"],
                                                               d["rho"])))
    full = []
    for offset in OFFSETS:
        t, bufs = device_tensors(d, offset)
        before = {k: b.clone() for k, b in bufs.items()}
        run_lin_grad(solver, shape, t)
        ym = solver.admm_lin_soft_mask(nx, nu, mx, mu, N, B, t["yf"], t["kappa"], t["rho"])
        hlo, hhi, _ = solver.admm_lin_grad(nx, nu, mx, mu, N, B, t["z"], t["az"], ym, t["ya"], t["rho"], want="lh")
        _, _, hE = solver.admm_lin_grad(nx, nu, mx, mu, N, B, t["z"], t["az"], t["yf"], t["ya"], t["rho"], want="E")
        torch.cuda.synchronize()
        for k in ("glo", "ghi", "gE"):
            assert np_same(t[k].cpu().numpy().reshape(B, -1), ref[k]), (k, offset)
        assert np_same_or_nan(t["gk"].cpu().numpy().reshape(B, -1), ref["gk"]), offset
        assert same(hlo, t["glo"]) and same(hhi, t["ghi"])                  # the existing bound gradients taken with ym
        assert same(hE, t["gE"])                                            # gbdpcg_admm_lin_grad_*'s gE taken with yf
        assert guards_intact(bufs, t, offset, ("glo", "ghi", "gk", "gE"))
        for k in bufs:
            if k not in ("glo", "ghi", "gk", "gE"):
                assert same(bufs[k], before[k]), f"{k} was written"
        full.append({k: t[k].clone() for k in ("glo", "ghi", "gk", "gE")})
        if N > 3:
            continue            # (the subsets at the small shapes)
        for which in ("l", "h", "k", "E", "lh", "kE", "lhk", "hkE"):
            s, sb = device_tensors(d, offset)
            run_lin_grad(solver, shape, s, which)
            torch.cuda.synchronize()
            for c, k in (("l", "glo"), ("h", "ghi"), ("k", "gk"), ("E", "gE")):
                if c in which:
                    assert same(s[k], t[k]), (which, k)
                else:
                    assert bool(torch.isnan(sb[k]).all()), (which, k)
    for k in full[0]:
        assert same(full[0][k], full[1][k]), f"{k}: aligned vs misaligned"
    sat = sa.saturated(dtype, d["yf"], d["kappa"], d["rho"])
    assert not ref["gk"][~sat].view(np.uint8).any() and sat.any() and ref["gk"][sat].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", BOX_SHAPES)
def test_identity_rows_give_the_bits_of_the_box_calls(solver, nx, nu, N, B, dtype):
    shape = (nx, nu, N, B, nx, nu)
    d = data(*shape, dtype, identity=True)
    a, _ = device_tensors(d)
    b, _ = device_tensors(d)
    clean = torch.nan_to_num(a["az"], nan=0.25)       # (the box negates az itself, the rows a chain: a NaN's sign may differ)
    a["az"].copy_(clean)
    b["az"].copy_(clean)
    run_lin_grad(solver, shape, a, "lhk")
    run_box_grad(solver, shape, b)
    solver.admm_lin_soft_mask(nx, nu, nx, nu, N, B, a["yf"], a["kappa"], a["rho"], ym=a["ym"])
    solver.admm_soft_mask(nx, nu, N, B, b["yf"], b["kappa"], b["rho"], ym=b["ym"])
    torch.cuda.synchronize()
    for k in ("ym", "glo", "ghi", "gk"):
        assert same(a[k], b[k]), k


# ---- 4. kappa = +Inf everywhere: the hard bits, gkappa = +0
@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_kappa_gives_the_bits_of_the_hard_calls(solver, dtype):
    shape = nx, nu, N, B, mx, mu = (5, 2, 3, 4, 3, 1)
    d = dict(data(*shape, dtype))
    d["kappa"] = np.full_like(d["kappa"], np.inf)
    t, _ = device_tensors(d, 1)
    run_lin_grad(solver, shape, t)
    solver.admm_lin_soft_mask(nx, nu, mx, mu, N, B, t["yf"], t["kappa"], t["rho"], ym=t["ym"])
    hlo, hhi, hE = solver.admm_lin_grad(nx, nu, mx, mu, N, B, t["z"], t["az"], t["yf"], t["ya"], t["rho"])
    torch.cuda.synchronize()
    assert same(t["ym"], t["yf"])
    assert same(t["glo"], hlo) and same(t["ghi"], hhi) and same(t["gE"], hE)
    assert not bool(t["gk"].view(torch.uint8).any())
    bshape = nx, nu, N, B, _, _ = (5, 2, 3, 4, 5, 2)
    d = dict(data(*bshape, dtype, identity=True))
    d["kappa"] = np.full_like(d["kappa"], np.inf)
    t, _ = device_tensors(d, 1)
    run_box_grad(solver, bshape, t)
    solver.admm_soft_mask(nx, nu, N, B, t["yf"], t["kappa"], t["rho"], ym=t["ym"])
    blo, bhi = solver.admm_grad_bounds(nx, nu, N, B, t["yf"], t["rho"], t["ya"])
    torch.cuda.synchronize()
    assert same(t["ym"], t["yf"]) and same(t["glo"], blo) and same(t["ghi"], bhi) and not bool(t["gk"].view(torch.uint8).any())


# ---- 5. isolation
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_problem(solver, dtype):
    shape = nx, nu, N, B, mx, mu = (14, 7, 3, 3, 4, 2)
    d = data(*shape, dtype)
    clean, _ = device_tensors(d)
    t, _ = device_tensors(d)
    for k in ("z", "az", "ya", "E", "yf", "kappa"):
        t[k].view(B, -1)[1, 3] = float("nan")
    for x in (clean, t):
        solver.admm_lin_soft_mask(nx, nu, mx, mu, N, B, x["yf"], x["kappa"], x["rho"], ym=x["ym"])
        run_lin_grad(solver, shape, x)
    torch.cuda.synchronize()
    assert bool(torch.isnan(t["gE"].view(B, -1)[1]).any())
    for k in OUTS:
        for p in (0, 2):
            assert same(t[k].view(B, -1)[p], clean[k].view(B, -1)[p]), (k, p)


# ---- 6. refusals: nothing is written (no call here reaches the device)
@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_bad_arguments(solver, suf, tt):
    nx, nu, mx, mu, N, B = 6, 3, 3, 2, 4, 3
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = torch.zeros(1 << 12, dtype=tt, device="cuda")
    rho = torch.ones(B, dtype=tt, device="cuda")
    outs = {k: torch.full((1 << 12,), 777.0, dtype=tt, device="cuda") for k in ("ym", "glo", "ghi", "gkappa", "gE")}
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def values(null=(), **over):
        v = {k: P(ins) for k in ("z", "az", "E", "yf", "ya", "kappa")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(nx=nx, nu=nu, mx=mx, mu=mu, N=N, batch=B)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    calls = {"admm_soft_mask": (False, ("yf", "kappa", "rho", "ym"), ()),
             "admm_lin_soft_mask": (True, ("yf", "kappa", "rho", "ym"), ()),
             "admm_soft_grad_bounds": (False, ("yf", "kappa", "rho", "ya", "az", "glo", "ghi", "gkappa"), ("glo", "ghi", "gkappa")),
             "admm_lin_soft_grad": (True, ("z", "az", "E", "yf", "ya", "kappa", "rho", "glo", "ghi", "gkappa", "gE"),
                                    ("glo", "ghi", "gkappa", "gE"))}

    def call(name, v):
        rows, keys, _ = calls[name]
        sizes = ("nx", "nu", "mx", "mu", "N", "batch") if rows else ("nx", "nu", "N", "batch")
        return getattr(lib, f"gbdpcg_{name}_{suf}")(solver.h, *(v[k] for k in sizes), *(v[k] for k in keys), s)

    for name, (rows, keys, optional) in calls.items():
        for k in keys:
            if k not in optional:
                assert call(name, values(null=(k,))) == 1, (name, k)            # a null required pointer
        if optional:
            assert call(name, values(null=optional)) == 1, name                 # every output null
        for k in ("nx", "nu", "N", "batch"):
            assert call(name, values(**{k: 0})) == 1, (name, k)
        assert call(name, values(batch=1 << 31)) != 0, name                     # one workgroup per problem
        if rows:
            assert call(name, values(mx=0, mu=0)) == 1, name                    # no rows at all
            assert call(name, values(mx=65)) == 4 and call(name, values(mu=65)) == 4, name      # past admm_rows_shape_ok
            assert call(name, values(nx=4000, nu=4000, mx=1, mu=1)) == 4, name  # a knot past the LDS
    # d_ym == d_yf is INVALID whatever the neighbouring refusals would answer
    for name in ("admm_soft_mask", "admm_lin_soft_mask"):
        assert call(name, values(ym=P(ins))) == 1, name
    assert call("admm_lin_soft_mask", values(ym=P(ins), mx=65)) == 1
    torch.cuda.synchronize()
    assert all(bool((t == 777.0).all()) for t in outs.values())


# ---- 7. composition on the pinned fixtures
class Kept:
    """The kept factorisation of a fixture of admm_soft_adjoint_ref, K_FWD replays of the forward SOFT step graph, and the buffers of
    the adjoint iteration on the masked y."""

    def __init__(self, solver, kind, dtype, max_iter=200):
        self.s, self.kind, self.tol, self.max_iter, self.dtype = solver, kind, PCG_TOL[dtype], max_iter, dtype
        self.dims = nx, nu, mx, mu, N, B = sa.dims(kind)
        d, E, lo, hi, kappa, gz, glam = sa.fixture(kind)
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        self.lo, self.hi, self.kappa = (dev(a.astype(dtype).reshape(-1)) for a in (lo, hi, kappa))
        self.E = None if E is None else dev(E.astype(dtype).reshape(-1))
        self.gz, self.nglam = dev(gz.astype(dtype).reshape(-1)), dev((-glam).astype(dtype).reshape(-1))
        self.rho = dev(np.asarray(sa.FIXTURE_RHO[kind], dtype))
        nan = float("nan")
        self.S = torch.full((B * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        gamma = torch.full((B * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, self.z = torch.zeros_like(gamma), torch.full_like(self.g, nan)
        r, p = torch.full_like(gamma, nan), torch.full_like(gamma, nan)
        self.w, self.y = torch.zeros_like(self.lo), torch.zeros_like(self.lo)
        res = torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda")
        solver.reserve(self.g.element_size(), nx, N, B)
        if kind == "box":
            it, fl = solver.kkt_step_reg(nx, nu, N, B, self.G, self.C, self.g, self.c, self.rho, self.S, gamma, self.Ginv, self.Pinv,
                                         self.lam, self.z, tol=self.tol, max_iter=max_iter)
            gt = solver.admm_soft_init(nx, nu, N, B, self.g, self.lo, self.hi, self.kappa, self.rho, self.w, self.y)
            gr = solver.graph_admm_soft_step(nx, nu, N, B, self.Ginv, self.C, self.g, self.c, self.lo, self.hi, self.kappa, self.rho,
                                             self.S, self.Pinv, gamma, self.lam, r, p, self.tol, max_iter, it, fl, self.z, self.w,
                                             self.y, gt, res)
        else:
            Gt = solver.admm_lin_form(nx, nu, mx, mu, N, B, self.G, self.E, self.rho)
            it, fl = solver.kkt_step(nx, nu, N, B, Gt, self.C, self.g, self.c, self.S, gamma, self.Ginv, self.Pinv, self.lam, self.z,
                                     tol=self.tol, max_iter=max_iter)
            gt = solver.admm_lin_soft_init(nx, nu, mx, mu, N, B, self.g, self.E, self.lo, self.hi, self.kappa, self.rho, self.w, self.y)
            gr = solver.graph_admm_lin_soft_step(nx, nu, mx, mu, N, B, self.Ginv, self.C, self.g, self.c, self.E, self.lo, self.hi,
                                                 self.kappa, self.rho, self.S, self.Pinv, gamma, self.lam, r, p, self.tol, max_iter, it,
                                                 fl, self.z, self.w, self.y, gt, res)
        flags = torch.zeros_like(fl)
        for _ in range(sa.K_FWD):
            gr.launch()
            flags |= fl
        torch.cuda.synchronize()
        gr.close()
        assert int(flags.sum()) == 0
        self.primal = self.w if kind == "box" else self.z

    def mask(self, ym=None):
        nx, nu, mx, mu, N, B = self.dims
        if self.kind == "box":
            return self.s.admm_soft_mask(nx, nu, N, B, self.y, self.kappa, self.rho, ym=ym)
        return self.s.admm_lin_soft_mask(nx, nu, mx, mu, N, B, self.y, self.kappa, self.rho, ym=ym)

    def state(self, ym):
        """Fresh buffers of the adjoint iteration, started by the HARD adjoint init on ym from zeros."""
        nan, (nx, nu, mx, mu, N, B) = float("nan"), self.dims
        o = dict(alam=torch.zeros_like(self.lam), wa=torch.zeros_like(self.y), ya=torch.zeros_like(self.y))
        o.update(gamma=torch.full_like(self.lam, nan), r=torch.full_like(self.lam, nan), p=torch.full_like(self.lam, nan),
                 az=torch.full_like(self.g, nan), res=torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda"),
                 it=torch.full((B,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))
        if self.kind == "box":
            o["gta"] = self.s.admm_adjoint_init(nx, nu, N, B, self.gz, ym, self.rho, o["wa"], o["ya"])
        else:
            o["gta"] = self.s.admm_lin_adjoint_init(nx, nu, mx, mu, N, B, self.gz, self.E, ym, self.rho, o["wa"], o["ya"])
        return o

    def step(self, o, ym):
        nx, nu, mx, mu, N, B = self.dims
        kw = dict(res=o["res"], r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        if self.kind == "box":
            self.s.admm_adjoint_step(nx, nu, N, B, self.Ginv, self.C, self.gz, self.nglam, ym, self.rho, self.S, self.Pinv, o["gamma"],
                                     o["alam"], o["az"], o["wa"], o["ya"], o["gta"], **kw)
        else:
            self.s.admm_lin_adjoint_step(nx, nu, mx, mu, N, B, self.Ginv, self.C, self.gz, self.nglam, self.E, ym, self.rho, self.S,
                                         self.Pinv, o["gamma"], o["alam"], o["az"], o["wa"], o["ya"], o["gta"], **kw)

    def graph(self, o, ym):
        nx, nu, mx, mu, N, B = self.dims
        tail = (self.S, self.Pinv, o["gamma"], o["alam"], o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["az"], o["wa"],
                o["ya"], o["gta"], o["res"])
        if self.kind == "box":
            return self.s.graph_admm_adjoint_step(nx, nu, N, B, self.Ginv, self.C, self.gz, self.nglam, ym, self.rho, *tail)
        return self.s.graph_admm_lin_adjoint_step(nx, nu, mx, mu, N, B, self.Ginv, self.C, self.gz, self.nglam, self.E, ym, self.rho, *tail)

    def grads(self, o, out=None):
        """(glo, ghi, gkappa, gE or None) from the UNMASKED y."""
        nx, nu, mx, mu, N, B = self.dims
        out = out or {}
        if self.kind == "box":
            return self.s.admm_soft_grad_bounds(nx, nu, N, B, self.y, self.kappa, self.rho, o["ya"], o["az"], glo=out.get("glo"),
                                                ghi=out.get("ghi"), gkappa=out.get("gk")) + (None,)
        return self.s.admm_lin_soft_grad(nx, nu, mx, mu, N, B, self.z, o["az"], self.E, self.y, o["ya"], self.kappa, self.rho,
                                         glo=out.get("glo"), ghi=out.get("ghi"), gkappa=out.get("gk"), gE=out.get("gE"))


@pytest.fixture(scope="module")
def kept(solver):
    cache = {}

    def get(kind, dtype):
        key = (kind, np.dtype(dtype).name)
        if key not in cache:
            cache[key] = Kept(solver, kind, dtype)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sa.KINDS)
def test_a_captured_mask_step_grad_replays_the_bits_of_the_calls(solver, kept, kind, dtype):
    L = kept(kind, dtype)
    nan = float("nan")

    def fresh():
        ym = torch.full_like(L.y, nan)
        outs = {k: torch.full_like(L.y, nan) for k in ("glo", "ghi", "gk")}
        if kind == "rows":
            outs["gE"] = torch.full_like(L.E, nan)
        return ym, outs

    ym_a, out_a = fresh()
    L.mask(ym_a)
    a = L.state(ym_a)
    for _ in range(2):
        L.step(a, ym_a)
    L.grads(a, out_a)
    torch.cuda.synchronize()
    ym_b, out_b = fresh()
    b = L.state(torch.zeros_like(L.y))          # (the init from zeros does not look at the mask's values: wa = 0 either way)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):     # the capturing stream is torch's current one inside the block
        L.mask(ym_b)
        L.step(b, ym_b)
        L.grads(b, out_b)
    for k in ("az", "gamma"):
        b[k].fill_(nan)
    for t in [ym_b] + list(out_b.values()):
        t.fill_(nan)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert same(ym_a, ym_b)
    for k in ("alam", "az", "wa", "ya", "gta", "res", "it", "fl"):
        assert same(a[k], b[k]), k
    for k in out_a:
        assert same(out_a[k], out_b[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sa.KINDS)
def test_converged_gradients_match_the_dense_reference(solver, kept, kind, dtype):
    """Bound: admm_adjoint_ref.converged_bound, as tests/test_gpu_admm_lin_adjoint.py applies it to the hard fixture."""
    L = kept(kind, dtype)
    nx, nu, mx, mu, N, B = L.dims
    ref, loop = sa.reference(kind), sa.loop_reference(kind)
    ym = L.mask()
    o = L.state(ym)
    gr = L.graph(o, ym)
    flags = torch.zeros_like(o["fl"])
    for _ in range(sa.K_ADJ):
        gr.launch()
        flags |= o["fl"]
    glo, ghi, gk, gE = L.grads(o)
    az = o["wa"] if kind == "box" else o["az"]           # dl/dg: the box reports wa, exactly zero on the held entries
    gG, gC = solver.kkt_grad(nx, nu, N, B, L.primal, L.lam, az, o["alam"])
    torch.cuda.synchronize()
    gr.close()
    assert int(flags.sum()) == 0, "an adjoint solve ran out of iterations"
    got = {"G": gG, "C": gC, "g": az, "c": -o["alam"], "lo": glo, "hi": ghi, "kappa": gk, "z": L.primal, "lam": L.lam}
    if kind == "rows":
        got["E"] = gE
    got = {k: v.cpu().numpy().astype(F64).reshape(B, -1) for k, v in got.items()}
    y, ya, ymh = (t.cpu().numpy().reshape(B, -1) for t in (L.y, o["ya"], ym))
    kappa, rho = L.kappa.cpu().numpy().reshape(B, -1), L.rho.cpu().numpy()
    what, replays = f"{np.dtype(dtype).name} {kind}", sa.K_FWD + sa.K_ADJ
    for b in range(B):
        mine = sa.sets(y[b], kappa[b], rho[b])
        assert all(np.array_equal(m, s) for m, s in zip(mine, ref[b]["sets"])), f"problem {b}: the device's sets are not the reference's"
        free, hl, hh, sl, sh = mine
        held, sat = hl | hh, sl | sh
        assert np.array_equal(ymh[b] != 0, held) and not ya[b][~held].any()       # a saturated row's ya stays exactly 0
        assert not got["lo"][b][~hl].any() and not got["hi"][b][~hh].any() and not got["kappa"][b][~sat].any()
        if kind == "rows":
            assert not lr.dense_E(nx, nu, mx, mu, N, got["E"][b])[free].any()
        for k in ("z", "lam"):
            err, bound = np.abs(got[k][b] - ref[b][k]).max(), sa.converged_bound(loop[b][k], ref[b][k], sa.K_FWD, STEP_TOL[dtype])
            print(f"{what} problem {b} {k}: {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (b, k, err, bound)
        for k in ("G", "C", "g", "c", "lo", "hi", "kappa") + (("E",) if kind == "rows" else ()):
            dense = ref[b]["grads"][k]
            err, bound = np.abs(got[k][b] - dense).max(), sa.converged_bound(loop[b]["grads"][k], dense, replays, STEP_TOL[dtype])
            print(f"{what} problem {b} d{k}: {err:.3e} (bound {bound:.3e}, scale {np.abs(dense).max():.3e})")
            assert err <= bound, (b, k, err, bound)
