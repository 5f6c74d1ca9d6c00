"""Adaptive rho on the device (csrc/admm_rebalance.hip and the composite calls of csrc/api_kkt.hip, through the C ABI):
gbdpcg_admm_rebalance_*, gbdpcg_admm_lin_rebalance_*, gbdpcg_admm_soc_rebalance_*, the three resteps and their graphs.  PARITY
UNPINNED: the reference tree has no code, fixture or output for these calls.

Reference: tests/admm_rebalance_ref.py.  The rule, the scaling of y and the box's gt are one IEEE operation per line, so d_rho, d_y,
d_expo and d_gt are compared for EQUALITY of bits (a NaN an operation makes need only meet a NaN: its sign and payload are the
platform's).  The composite calls are compared bit for bit with the calls they are made of.  Convergence runs the fixture
tests/test_admm_rebalance_reference.py pins (K_fixed = 1270, K_adapt = 104 in the dense fp64 reference): the device loop on the same
schedule must be below eps within K_adapt + P iterations -- the margin is one period, an inexact solve may tip a decision at the
threshold once -- and the loop without the rule must not be.  Run with -s for the measured figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_rebalance_ref as ar  # noqa: E402
import admm_ref  # noqa: E402
from admm_util import dev, np_same, np_same_or_nan, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
SHAPES = [(2, 1, 3),      # nz = 8
          (3, 2, 5),      # nz = 23: odd, the problems misalign, head and tail are peeled
          (14, 7, 16)]    # nz = 329: four waves
RULE = dict(ratio=10.0, rho_min=0.5, rho_max=8.0)
#            r      s      rho   the six branches
DECISIONS = [(100.0, 1.0, 1.0),            # raise
             (1.0, 100.0, 8.0),            # lower
             (5.0, 1.0, 1.0),              # unchanged inside the band
             (100.0, 1.0, 8.0),            # raise blocked by rho_max
             (1.0, 100.0, 0.5),            # lower blocked by rho_min
             (float("nan"), 1.0, 1.0)]     # NaN residual: unchanged
B6 = len(DECISIONS)
GUARD = 64


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
def box_data(nx, nu, N, dtype, special=True):
    """g, w, y [6, nz] of order 1, res and rho of DECISIONS; lo, hi around w with w on a bound here and there.  special: y holds 0,
    -0, +-Inf, NaN and numbers that become subnormal when halved.  Read-only."""
    nz = nz_of(nx, nu, N)
    rng = np.random.default_rng(700 + nz)
    g, w, y = (rng.standard_normal((B6, nz)).astype(dtype) for _ in range(3))
    if special:
        tiny = np.finfo(dtype).tiny
        y[:, 0], y[:, 1], y[:, 2], y[:, 3], y[:, 4] = 0.0, np.inf, -np.inf, np.nan, -0.0
        y[:, 5], y[:, 6] = tiny, 3 * np.finfo(dtype).smallest_subnormal
    lo = (w - 0.25 * (rng.random((B6, nz)) < 0.5)).astype(dtype)
    hi = (w + 0.25 * (rng.random((B6, nz)) < 0.5)).astype(dtype)
    d = dict(g=g, w=w, y=y, lo=lo, hi=hi, res=np.array([[r, s] for r, s, _ in DECISIONS], dtype),
             rho=np.array([p for _, _, p in DECISIONS], dtype))
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def box_reference(nx, nu, N, dtype, shift, special=True):
    d = box_data(nx, nu, N, dtype, special)
    return ar.rebalance_ref(dtype, d["res"], d["rho"], d["y"], RULE["ratio"], shift, RULE["rho_min"], RULE["rho_max"], g=d["g"], w=d["w"])


def guarded(d, dtype, offset, extra=()):
    """Every array of d (and NaN-filled `extra` outputs shaped like g) inside a buffer of its own with GUARD NaN elements on either
    side (+ offset elements in front: 0 -> 16-byte aligned, 1 -> off by one element).  Returns (buffers, views)."""
    bufs, t = {}, {}
    for k, a in list(d.items()) + [(k, np.full_like(d["g"], np.nan)) for k in extra]:
        n = a.size
        buf = torch.full((n + 2 * GUARD + 8,), float("nan"), dtype=tdt(dtype), device="cuda")
        assert buf.data_ptr() % 16 == 0
        lead = GUARD + (offset if k not in ("res", "rho") else 0)
        buf[lead:lead + n] = dev(a.reshape(-1))
        bufs[k], t[k] = (buf, lead, n), buf[lead:lead + n]
    t["expo"] = torch.full((B6 + 2 * GUARD,), -77, dtype=torch.int32, device="cuda")
    bufs["expo"] = (t["expo"], GUARD, B6)
    t["expo"] = t["expo"][GUARD:GUARD + B6]
    return bufs, t


def guards_intact(bufs):
    for k, (buf, lead, n) in bufs.items():
        for part in (buf[:lead], buf[lead + n:]):
            if k == "expo":
                assert bool((part == -77).all()), f"guard of {k}"
            else:
                assert bool(torch.isnan(part).all()), f"guard of {k}"


# ---- 1. the box launch against the reference: six branches, special y, aligned and misaligned bases, both shifts
@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N", SHAPES)
def test_box_rebalance_bits(solver, nx, nu, N, dtype, offset, shift):
    d = box_data(nx, nu, N, dtype)
    rho_r, y_r, e_r, gt_r = box_reference(nx, nu, N, dtype, shift)
    assert e_r.tolist() == [shift, -shift, 0, 0, 0, 0]
    bufs, t = guarded({k: d[k] for k in ("g", "w", "y", "res", "rho")}, dtype, offset, extra=("gt",))
    esz = t["g"].element_size()
    assert all(t[k].data_ptr() % 16 == (offset * esz) % 16 for k in ("g", "w", "y", "gt"))
    before = {k: t[k].clone() for k in ("g", "w", "res")}
    solver.admm_rebalance(nx, nu, N, B6, t["g"], t["res"], t["rho"], t["w"], t["y"], t["gt"], t["expo"], shift=shift, **RULE)
    torch.cuda.synchronize()
    what = f"({nx},{nu},{N}) {np.dtype(dtype).name} offset {offset} shift {shift}"
    assert np.array_equal(t["expo"].cpu().numpy(), e_r), what
    assert np_same(t["rho"].cpu().numpy(), rho_r), what + ": rho"
    y, gt = (t[k].cpu().numpy().reshape(B6, -1) for k in ("y", "gt"))
    assert np_same_or_nan(y, y_r), what + ": y"
    assert np_same(y[2:], d["y"][2:]), what + ": y of an unchanged problem keeps its bits"
    assert np_same_or_nan(gt, gt_r), what + ": gt"
    assert np.isfinite(gt[:, 7:]).all() and np.isnan(gt[:, 3]).all() and np.isinf(gt[:, 1]).all()
    assert (y[0, 5] != 0) and abs(float(y[0, 5])) < float(np.finfo(dtype).tiny), "subnormal after scaling"
    for k in before:
        assert same(t[k], before[k]), f"{k} was written"
    guards_intact(bufs)


# ---- 2. one launch for what the rows form and admm_init do in two; admm_lin_rebalance with E = I
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N", SHAPES[1:])
def test_box_call_is_rows_form_then_init_and_lin_with_identity(solver, nx, nu, N, dtype):
    """Finite y here: E = I multiplies every t_r by the zeros of its column, and 0 Inf is a NaN the box never makes."""
    d = box_data(nx, nu, N, dtype, special=False)
    rho_r, y_r, e_r, gt_r = box_reference(nx, nu, N, dtype, 1, special=False)
    nz = nz_of(nx, nu, N)
    eye = np.concatenate([np.eye(nx).reshape(-1), np.eye(nu).reshape(-1)] * N)[:(nx * nx + nu * nu) * N - nu * nu]
    E = dev(np.tile(eye.astype(dtype), B6))
    out = []
    for how in ("box", "lin", "lin+init"):
        t = {k: dev(d[k].reshape(-1)) for k in ("g", "w", "y", "lo", "hi", "res", "rho")}
        t["gt"] = torch.full_like(t["g"], float("nan"))
        if how == "box":
            t["expo"] = solver.admm_rebalance(nx, nu, N, B6, t["g"], t["res"], t["rho"], t["w"], t["y"], t["gt"], shift=1, **RULE)
        else:
            t["expo"] = solver.admm_lin_rebalance(nx, nu, nx, nu, N, B6, t["g"], E, t["lo"], t["hi"], t["res"], t["rho"], t["w"], t["y"],
                                                  t["gt"], shift=1, **RULE)
            if how == "lin+init":     # rho, y, expo of the rows form, gt of the box's own init
                t["gt"].fill_(float("nan"))
                solver.admm_init(nx, nu, N, B6, t["g"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
        torch.cuda.synchronize()
        out.append(t)
    assert np_same(out[0]["gt"].cpu().numpy().reshape(B6, nz), gt_r) and np_same(out[0]["y"].cpu().numpy().reshape(B6, nz), y_r)
    for k in ("rho", "y", "expo", "gt", "w"):
        assert same(out[0][k], out[2][k]), f"box vs rows form + admm_init: {k}"
        assert same(out[0][k], out[1][k]), f"box vs admm_lin_rebalance with E = I: {k}"
    assert np_same(out[0]["w"].cpu().numpy().reshape(B6, nz), d["w"])


# ---- 3. a restep is its constituent calls, eager and as a graph, for the three families
FAMILIES = {"box": None, "lin": (2, 1, None), "soc": (2, 4, (2, 1, 1, 3))}     # soc: 2 + (1 linear + one q = 3 cone) rows
STATE = ("rho", "expo", "Gt", "Ginv", "S", "Pinv", "gamma", "lam", "r", "p", "z", "it", "fl", "w", "y", "gt", "res")
RESTEP_RULE = dict(ratio=10.0, shift=1, rho_min=0.25, rho_max=64.0)


@functools.lru_cache(maxsize=None)
def step_problem(nx, nu, N, batch, seed=61):
    d = {k: v.astype(F32).astype(F64) for k, v in so.gen(nx, nu, N, seed=seed, batch=batch, dtype=F64).items()}
    for a in d.values():
        a.setflags(write=False)
    return d


class Family:
    """One of the three families on a small batch: the constant data, and a state (every buffer a restep writes) that has made two
    plain iterations from w = y = 0."""

    def __init__(self, solver, fam, dtype, nx=3, nu=2, N=5, batch=3, tol=1e-8, max_iter=100):
        self.s, self.fam, self.shape, self.batch, self.tol, self.max_iter = solver, fam, (nx, nu, N), batch, tol, max_iter
        d = step_problem(nx, nu, N, batch)
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        nz = nz_of(nx, nu, N)
        rng = np.random.default_rng(17)
        self.rows = FAMILIES[fam]
        if self.rows is None:
            lo, hi = np.full((batch, nz), -0.2), np.full((batch, nz), 0.2)
            self.E = None
        else:
            mx, mu, cones = self.rows
            _, nw, ne, _ = binding.Solver._lin_sizes(nx, nu, mx, mu, N)
            self.E = dev((0.5 * rng.standard_normal((batch, ne))).astype(F32).astype(dtype).reshape(-1))
            lo, hi = np.full((batch, nw), -0.2), np.full((batch, nw), 0.2)
            if cones is not None:      # the u blocks: row 0 linear, rows 1 .. 3 one cone with head offset 0.2
                for k in range(N - 1):
                    o = k * (mx + mu) + mx
                    lo[:, o + 1], lo[:, o + 2:o + 4], hi[:, o + 1:o + 4] = 0.2, 0.0, np.nan
        self.lo, self.hi = dev(lo.astype(dtype).reshape(-1)), dev(hi.astype(dtype).reshape(-1))
        nan, tt = float("nan"), self.G.dtype
        o = dict(rho=dev(np.array([0.5, 2.0, 1.0], dtype)), expo=torch.full((batch,), -77, dtype=torch.int32, device="cuda"),
                 Gt=torch.full_like(self.G, nan), Ginv=torch.full_like(self.G, nan),
                 S=torch.full((batch * 3 * nx * nx * N,), nan, dtype=tt, device="cuda"),
                 gamma=torch.full((batch * nx * N,), nan, dtype=tt, device="cuda"), z=torch.full_like(self.g, nan),
                 w=torch.zeros_like(self.lo), y=torch.zeros_like(self.lo), gt=torch.full_like(self.g, nan),
                 res=torch.full((batch, 2), nan, dtype=tt, device="cuda"), it=torch.full((batch,), -1, dtype=torch.int32, device="cuda"),
                 fl=torch.full((batch,), 9, dtype=torch.uint8, device="cuda"))
        o["Pinv"], o["lam"] = torch.full_like(o["S"], nan), torch.zeros_like(o["gamma"])
        o["r"], o["p"] = torch.full_like(o["gamma"], nan), torch.full_like(o["gamma"], nan)
        self.refactor(o, self.g)
        self.init(o)
        for _ in range(2):
            self.step(o)
        torch.cuda.synchronize()
        assert int(o["fl"].sum()) == 0 and bool(torch.isfinite(o["res"]).all()) and int((o["y"] != 0).sum()) > 0
        self.start = o

    def sizes(self):
        nx, nu, N = self.shape
        if self.rows is None:
            return (nx, nu, N, self.batch)
        mx, mu, cones = self.rows
        return (nx, nu, mx, mu) + ((cones,) if cones is not None else ()) + (N, self.batch)

    def set(self):
        return (self.lo, self.hi) if self.rows is None else (self.E, self.lo, self.hi)

    def call(self, name):
        return getattr(self.s, {"box": "admm", "lin": "admm_lin", "soc": "admm_soc"}[self.fam] + "_" + name)

    def state(self, res=None):
        o = {k: v.clone() for k, v in self.start.items()}
        if res is not None:
            o["res"].copy_(dev(np.asarray(res)).to(o["res"].dtype))
        return o

    def refactor(self, o, grad):
        nx, nu, N = self.shape
        kw = dict(r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        if self.rows is None:
            self.s.kkt_step_reg(nx, nu, N, self.batch, self.G, self.C, grad, self.c, o["rho"], o["S"], o["gamma"], o["Ginv"], o["Pinv"],
                                o["lam"], o["z"], **kw)
        else:
            self.s.admm_lin_form(nx, nu, self.rows[0], self.rows[1], N, self.batch, self.G, self.E, o["rho"], Gt=o["Gt"])
            self.s.kkt_step(nx, nu, N, self.batch, o["Gt"], self.C, grad, self.c, o["S"], o["gamma"], o["Ginv"], o["Pinv"], o["lam"], o["z"],
                            **kw)

    def init(self, o):
        self.call("init")(*self.sizes(), self.g, *self.set(), o["rho"], o["w"], o["y"], gt=o["gt"])

    def update(self, o):
        self.call("update")(*self.sizes(), self.g, *self.set(), o["rho"], o["z"], o["w"], o["y"], o["gt"], res=o["res"])

    def step(self, o):
        self.call("step")(*self.sizes(), o["Ginv"], self.C, self.g, self.c, *self.set(), o["rho"], o["S"], o["Pinv"], o["gamma"], o["lam"],
                          o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter,
                          iters=o["it"], max_iter_exit=o["fl"])

    def rebalance(self, o, **rule):
        if self.rows is None:
            self.s.admm_rebalance(*self.sizes(), self.g, o["res"], o["rho"], o["w"], o["y"], o["gt"], o["expo"], **rule)
        else:
            self.call("rebalance")(*self.sizes(), self.g, *self.set(), o["res"], o["rho"], o["w"], o["y"], o["gt"], o["expo"], **rule)

    def constituents(self, o, **rule):
        self.rebalance(o, **rule)
        self.refactor(o, o["gt"])
        self.update(o)

    def mats(self, o):
        return (self.G,) if self.rows is None else (self.G, o["Gt"])

    def restep(self, o, mats=None, expo="expo", **rule):
        self.call("restep")(*self.sizes(), *(mats or self.mats(o)), o["Ginv"], self.C, self.g, self.c, *self.set(), o["rho"], o["S"],
                            o["Pinv"], o["gamma"], o["lam"], o["z"], o["w"], o["y"], o["gt"], o["res"], o[expo] if expo else None,
                            r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"], **rule)

    def graph_args(self, o, **rule):
        return (*self.sizes(), *self.mats(o), o["Ginv"], self.C, self.g, self.c, *self.set(), o["rho"], o["S"], o["Pinv"], o["gamma"],
                o["lam"], o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"], o["expo"])

    def graph(self, o, **rule):
        return getattr(self.s, "graph_" + {"box": "admm", "lin": "admm_lin", "soc": "admm_soc"}[self.fam] + "_restep")(
            *self.graph_args(o), **rule)


def residuals(L, decisions):
    """res that makes problem b take decisions[b] (+1 raise, -1 lower, 0 keep), at the size of what the two iterations left."""
    base = L.start["res"].cpu().numpy().astype(F64).max()
    table = {1: (100.0, 1.0), -1: (1.0, 100.0), 0: (1.0, 1.0)}
    return np.array([table[v] for v in decisions]) * base


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_restep_is_its_constituent_calls_and_the_graph_keeps_pointers(solver, fam, dtype):
    L = Family(solver, fam, dtype)
    nx, nu, N = L.shape
    first, second = residuals(L, (1, -1, 0)), residuals(L, (0, 1, -1))
    a, b, g = L.state(first), L.state(first), L.state(first)
    solver.reserve(L.g.element_size(), nx, N, L.batch)
    gr = L.graph(g, **RESTEP_RULE)
    L.constituents(a, **RESTEP_RULE)
    L.restep(b, **RESTEP_RULE)
    gr.launch()
    torch.cuda.synchronize()
    keys = [k for k in STATE if not (k == "Gt" and fam == "box")]
    for k in keys:
        assert same(a[k], b[k]), f"{fam}: restep vs constituent calls: {k}"
        assert same(b[k], g[k]), f"{fam}: graph replay vs restep: {k}"
    assert b["expo"].tolist() == [1, -1, 0] and int(b["fl"].sum()) == 0
    assert all(bool(torch.isfinite(b[k]).all()) for k in ("z", "w", "y", "gt", "res", "S", "Ginv", "Pinv"))
    assert not same(b["S"], L.start["S"]) and not same(b["y"], L.start["y"])
    # the multiplier rho y is what it was in front of the solve: checked on the rebalance alone
    c = L.state(first)
    L.rebalance(c, **RESTEP_RULE)
    torch.cuda.synchronize()
    B = L.batch
    assert same(c["rho"].view(B, 1) * c["y"].view(B, -1), L.start["rho"].view(B, 1) * L.start["y"].view(B, -1))
    # d_res rewritten between two replays of ONE graph: the pointers are kept, the values are not baked in
    fresh = L.state(second)
    for k in keys:
        g[k].copy_(fresh[k])
    gr.launch()
    L.restep(fresh, **RESTEP_RULE)
    torch.cuda.synchronize()
    gr.close()
    for k in keys:
        assert same(g[k], fresh[k]), f"{fam}: second replay: {k}"
    assert g["expo"].tolist() == [0, 1, -1]


# ---- 4. refusals: INVALID, nothing written, *out == NULL
BAD_RULES = [dict(shift=0), dict(shift=17), dict(ratio=0.5), dict(ratio=float("nan")), dict(rho_min=0.0), dict(rho_min=-1.0),
             dict(rho_max=0.125), dict(rho_max=float("inf")), dict(rho_min=float("nan")), dict(rho_max=float("nan"))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_refusals_write_nothing(solver, fam, dtype):
    L = Family(solver, fam, dtype)
    o = L.state(residuals(L, (1, -1, 0)))
    before = {k: v.clone() for k, v in o.items()}
    name = {"box": "admm", "lin": "admm_lin", "soc": "admm_soc"}[fam] + "_restep"
    suf = "f32" if dtype == F32 else "f64"

    def invalid(fn):
        with pytest.raises(binding.GbdPcgError, match=r"status 1;"):
            fn()

    def graph_refused(o, mats=None, expo=True, **rule):
        """The raw constructor with a stale handle in *out: status 1 and *out == NULL."""
        _, args, _ = solver._admm_restep_args(*L.shape, L.batch, *((mats or L.mats(o)) + ((None,) if fam == "box" else ())), o["Ginv"], L.C,
                                              L.g, L.c, L.lo, L.hi, o["rho"], o["S"], o["Pinv"], binding.PINV_STAIR, o["gamma"], o["lam"],
                                              o["r"], o["p"], L.tol, L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"],
                                              o["expo"], rule["ratio"], rule["shift"], rule["rho_min"], rule["rho_max"],
                                              rows=None if fam == "box" else (L.rows[0], L.rows[1], L.E), cones=L.rows and L.rows[2])
        if not expo:
            args = args[:-1] + (None,)
        out = ctypes.c_void_p(0x1234)
        assert getattr(solver.lib, f"gbdpcg_graph_create_{name}_{suf}")(*args, ctypes.byref(out)) == 1
        assert not out.value

    for bad in BAD_RULES:
        rule = dict(RESTEP_RULE, **bad)
        invalid(lambda: L.rebalance(o, **rule))
        invalid(lambda: L.restep(o, **rule))
        graph_refused(o, **rule)
    # NULL d_expo (the binding would allocate one: the raw calls)
    graph_refused(o, expo=False, **RESTEP_RULE)
    _, args, _ = solver._admm_restep_args(*L.shape, L.batch, *(L.mats(o) + ((None,) if fam == "box" else ())), o["Ginv"], L.C, L.g, L.c, L.lo,
                                          L.hi, o["rho"], o["S"], o["Pinv"], binding.PINV_STAIR, o["gamma"], o["lam"], o["r"], o["p"], L.tol,
                                          L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"], o["expo"], 10.0, 1, 0.25, 64.0,
                                          rows=None if fam == "box" else (L.rows[0], L.rows[1], L.E), cones=L.rows and L.rows[2])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert getattr(solver.lib, f"gbdpcg_{name}_{suf}")(*args[:-1], None, stream) == 1
    reb = getattr(solver.lib, f"gbdpcg_{name.replace('restep', 'rebalance')}_{suf}")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    sizes = tuple(v for part in L.sizes() for v in (part if isinstance(part, tuple) else (part,)))
    rows = () if fam == "box" else (P(L.E), P(L.lo), P(L.hi))
    assert reb(solver.h, *sizes, P(L.g), *rows, P(o["res"]), P(o["rho"]), P(o["w"]), P(o["y"]), P(o["gt"]), 10.0, 1, 0.25, 64.0, None,
               stream) == 1
    assert reb(solver.h, *sizes[:-1], 0, P(L.g), *rows, P(o["res"]), P(o["rho"]), P(o["w"]), P(o["y"]), P(o["gt"]), 10.0, 1, 0.25, 64.0,
               P(o["expo"]), stream) == 1      # batch == 0
    if fam != "box":     # the next restep needs the original G
        invalid(lambda: L.restep(o, mats=(L.G, L.G), **RESTEP_RULE))
        graph_refused(o, mats=(L.G, L.G), **RESTEP_RULE)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert same(o[k], v), f"{fam}: {k} was written by a refused call"


# ---- 5. convergence on the fixture tests/test_admm_rebalance_reference.py pins
def test_adaptive_loop_converges_where_the_fixed_loop_does_not(solver):
    import test_gpu_admm as box
    nx, nu, N, B = ar.CONV_SHAPE
    P, eps = ar.CONV_PERIOD, ar.CONV_EPS
    fixed, adapt = ar.convergence_counts()
    k_adapt = max(k for k, _ in adapt)
    budget = k_adapt + P
    d, lo, hi, _ = admm_ref.convergence_inputs()
    rho0 = np.array(ar.CONV_RHO0)
    tol, max_iter = 1e-22, 400      # PCG_TOL of tests/test_gpu_admm.py: the solve is not the limit
    outcome = {}
    for adaptive in (True, False):
        L = box.Loop(solver, nx, nu, N, B, F64, d, rho0, lo=lo, hi=hi, tol=tol, max_iter=max_iter)
        o = L.state()
        expo = torch.zeros(B, dtype=torch.int32, device="cuda")
        step = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"], o["r"],
                                      o["p"], tol, max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
        restep = solver.graph_admm_restep(nx, nu, N, B, L.G, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"],
                                          o["r"], o["p"], tol, max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"], expo,
                                          **ar.CONV_RULE)
        flags, reached, history = torch.zeros_like(o["fl"]), None, []
        for k in range(1, budget + 1):
            w_prev, y_prev = o["w"].clone(), o["y"].clone()
            if adaptive and k % (P + 1) == 0:
                restep.launch()
                history.append(expo.tolist())
                y_prev = y_prev.view(B, -1) * torch.pow(2.0, -expo.double()).view(B, 1)
            else:
                step.launch()
            flags |= o["fl"]
            if float(o["res"].max()) < eps:
                reached = k
                break
        torch.cuda.synchronize()
        step.close()
        restep.close()
        res = o["res"].cpu().numpy()
        print(f"{'adaptive' if adaptive else 'fixed'}: reached {reached} (reference K_adapt {k_adapt}, K_fixed {max(k for k, _ in fixed)}, "
              f"budget {budget}); max res {res.max():.3e}; rho {L.rho.tolist()}; expo history {history}")
        assert int(flags.sum()) == 0, "a solve ran out of iterations"
        outcome[adaptive] = reached
        if not adaptive:
            continue
        assert reached is not None, f"max(d_res) {res.max():.3e} >= {eps} after {budget} iterations"
        z, w, y, rho = (t.cpu().numpy().reshape(B, -1) for t in (o["z"], o["w"], o["y"], L.rho))
        wp, yp = w_prev.cpu().numpy().reshape(B, -1), y_prev.cpu().numpy().reshape(B, -1)
        again = np.stack([np.abs(z - w).max(axis=1), np.abs(rho * (w - wp)).max(axis=1)], axis=1)
        assert np_same(res, again), "d_res recomputed from z, w, rho"
        assert np_same(y, (z + yp) - w), "y recomputed from z, w"
        assert ((w >= lo) & (w <= hi)).all(), "w outside the box"
        assert any(any(h) for h in history), "no rho moved"
    assert outcome[False] is None, "the loop without the rule reached eps too: the test would not notice a rebalance that does nothing"
