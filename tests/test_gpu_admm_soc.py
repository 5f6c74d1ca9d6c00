"""ADMM with stage-wise linear and second-order cone rows on a kept factorisation, on the device (csrc/admm_rows.hip and the composite
calls of csrc/api_kkt.hip, through the C ABI): gbdpcg_admm_soc_init_*, _update_*, _step_*, the shared twin and the two graphs.  PARITY
UNPINNED: the reference tree has no code, fixture or output for these steps.

Reference: tests/admm_soc_ref.py.  Initialisation and update are defined to the bit (every line one IEEE operation, chains in a fixed
order, sqrt and / correctly rounded), so w, y, gt and the two norms are compared for EQUALITY with update_ref, which evaluates every
line in exact rational arithmetic with one rounding per operation.  The composite calls are compared bit for bit with the calls they
are made of; without cone rows, and with q = 1 cones, everything is compared bit for bit with the gbdpcg_admm_lin_* calls.
Convergence (the last test) runs the three problems tests/test_admm_soc_reference.py pins, 80 graph replays from w = y = 0, against
the 80th iterate of the fp64 twin: see CLOSE and RATIO below.  Run with -s for the measured figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_ref as lin  # noqa: E402
import admm_soc_ref as ref  # noqa: E402
from admm_util import bits, dev, host, knot_chunk, np_same, np_same_or_nan, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
PCG_TOL = {F32: 1e-10, F64: 1e-22}      # tests/test_gpu_admm_lin.py
# The 80th iterate of the device against the 80th iterate of the fp64 twin, the worst of the three convergence problems, measured
# once on the MI355X (profiles/r12_admm_soc.txt); the test holds 4 times the measured figure, the margin tests/test_gpu_admm_lin.py
# uses for other PCG tolerances and fp32 rounding noise.
#   CLOSE  ||w_dev(80) - w_twin(80)||_inf: 2.064e-6 in fp32 (1.4e-6 / 1.5e-6 / 2.1e-6 per problem), 2.444e-12 in fp64 (8.5e-13 / 2.4e-12 /
#          1.2e-12)
#   RATIO  max over the two residuals of |res_dev(80)/res_dev(1) - res_twin(80)/res_twin(1)| / (res_twin(80)/res_twin(1)): 6.436e-2 in
#          fp32 (3.9e-4 / 6.4e-2 / 2.2e-4: the dual residual of problem 1 has fallen to 1.4e-7 of its first value, where fp32 rounding
#          shows), 1.472e-8 in fp64 (3.5e-12 / 1.5e-8 / 3.5e-11)
MEASURED_CLOSE = {F32: 2.064e-6, F64: 2.444e-12}
MEASURED_RATIO = {F32: 6.436e-2, F64: 1.472e-8}
CLOSE = {k: 4 * v for k, v in MEASURED_CLOSE.items()}
RATIO = {k: 4 * v for k, v in MEASURED_RATIO.items()}

B = 5
NAN_PROBLEM, INF_PROBLEM = 1, 2
TURN = (0, 0, 1, 1, 2)       # per problem, where its cones start in the cycle of the three branches: the clean ones differ
# nx, nu, N, mx, mu, (lx, qx, lu, qu)
SHAPES = [(4, 3, 5, 3, 4, (0, 3, 1, 3)),        # x one cone q = 3; u one linear row + one cone q = 3
          (3, 3, 1, 3, 3, (0, 3, 0, 3)),        # N = 1: no u block at all
          (2, 1, 3, 2, 1, (0, 1, 0, 1)),        # q = 1 cones: half-lines
          (14, 7, 40, 5, 4, (2, 3, 0, 4)),      # two chunks (29 knots fit 4096 staged elements), 261 rows in the first: two passes
          (6, 5, 3, 64, 64, (0, 8, 0, 64)),     # x 8 cones of 8, u one cone of 64: the row limit, 256-thread blocks
          (5, 3, 9, 6, 4, (0, 3, 0, 4))]        # 86 rows, 69 entries: the 64-thread launch, two passes, a cone across them


assert knot_chunk(14, 7, 5, 4) == 29 and 29 * 9 > 256 and (256 - 28 * 9) == 4      # row 256 is the last row of a q = 3 cone
assert knot_chunk(5, 3, 6, 4) >= 9 and 64 - 6 * 10 == 4                           # row 64 is the middle row of a q = 3 cone


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def ids(shape):
    return "-".join(str(v) for v in shape[:5]) + "-" + ".".join(str(v) for v in shape[5])


@functools.lru_cache(maxsize=None)
def soc_data(shape, dtype):
    """Random data of order 1 for B problems: arrays [B, .] of `dtype`, read-only.  Linear rows: bounds near +-0.3, a third of each
    side infinite.  Cone rows: lo holds an offset f of order 0.3, hi is NaN (not read).  y (for the update) and w (for the
    initialisation) are placed so that s = E z + f + y, respectively w, lies strictly inside the cone, inside its polar cone and
    outside both in turn over the cones (with q = 1 the third case does not exist).  Problem NAN_PROBLEM carries a NaN in z, problem
    INF_PROBLEM an infinity in the offset of its first cone."""
    nx, nu, N, mx, mu, cones = shape
    nz, nw, ne, _ = lin.sizes(nx, nu, mx, mu, N)
    head, dim = ref.layout(nx, nu, mx, mu, cones, N)
    rng = np.random.default_rng(9000 + 13 * nz + nw)
    d = dict(E=0.5 * rng.standard_normal((B, ne)), g=rng.standard_normal((B, nz)), z=rng.standard_normal((B, nz)),
             w=rng.standard_normal((B, nw)), y=0.3 * rng.standard_normal((B, nw)),
             lo=-0.3 + 0.05 * rng.standard_normal((B, nw)), hi=0.3 + 0.05 * rng.standard_normal((B, nw)), rho=rng.uniform(0.5, 4.0, B))
    d["lo"][rng.random((B, nw)) < 1.0 / 3.0] = -np.inf
    d["hi"][rng.random((B, nw)) < 1.0 / 3.0] = np.inf
    cone = head >= 0
    d["lo"][:, cone] = 0.3 * rng.standard_normal((B, int(cone.sum())))
    d["hi"][:, cone] = np.nan
    d = {k: v.astype(dtype).astype(F64) for k, v in d.items()}
    for b in range(B):
        v = lin.dense_E(nx, nu, mx, mu, N, d["E"][b]) @ d["z"][b] + np.where(cone, d["lo"][b], 0.0)
        for i, h0 in enumerate(ref.heads(head)):
            q = int(dim[h0])
            for key, turn in (("y", i + TURN[b]), ("w", i + TURN[b] + 1)):
                tail = rng.standard_normal(q - 1)
                s = np.concatenate([[(2.0, -2.0, 0.3)[turn % 3] * (np.linalg.norm(tail) if q > 1 else 1.0)], tail])
                d[key][b, h0:h0 + q] = s - v[h0:h0 + q] if key == "y" else s
    d["z"][NAN_PROBLEM, nz // 2] = np.nan
    d["lo"][INF_PROBLEM, ref.heads(head)[0] if cone.any() else 0] = np.inf
    d = {k: v.astype(dtype) for k, v in d.items()}
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def update_reference(shape, dtype, init):
    nx, nu, N, mx, mu, cones = shape
    d = soc_data(shape, dtype)
    return ref.update_ref(dtype, nx, nu, mx, mu, cones, N, d["g"], d["E"], d["lo"], d["hi"], d["rho"], None if init else d["z"], d["w"],
                          d["y"])


GUARD = 256


def device_tensors(d, batch=B):
    """The arrays on the device, flat, plus gt (NaN) and res (NaN), each with GUARD NaN elements either side (t["_bufs"])."""
    t, bufs = {}, {}
    extra = [("gt", np.full_like(d["g"], np.nan)), ("res", np.full((batch, 2), np.nan, d["g"].dtype))]
    for k, a in list(d.items()) + extra:
        flat = dev(a.reshape(-1))
        buf = torch.full((flat.numel() + 2 * GUARD,), float("nan"), dtype=flat.dtype, device="cuda")
        buf[GUARD:GUARD + flat.numel()] = flat
        bufs[k], t[k] = buf, buf[GUARD:GUARD + flat.numel()]
    t["_bufs"] = bufs
    return t


def guards_intact(t):
    return all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[b.numel() - GUARD:]).all()) for b in t["_bufs"].values())


def run_update(solver, shape, t, init, batch=B):
    nx, nu, N, mx, mu, cones = shape
    if init:
        solver.admm_soc_init(nx, nu, mx, mu, cones, N, batch, t["g"], t["E"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
        return None
    return solver.admm_soc_update(nx, nu, mx, mu, cones, N, batch, t["g"], t["E"], t["lo"], t["hi"], t["rho"], t["z"], t["w"], t["y"],
                                  t["gt"], res=t["res"])


# ---- 1. initialisation and update against the exact reference, bit for bit; NaN and Inf stay in their problem; guards
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_update_and_init_vs_reference(solver, shape, dtype, init):
    d = soc_data(shape, dtype)
    wr, yr, gr, rr, branches = update_reference(shape, dtype, init)
    t = device_tensors(d)
    before = {k: b.clone() for k, b in t["_bufs"].items()}
    res = run_update(solver, shape, t, init)
    torch.cuda.synchronize()
    w, y, gt = (host(t[k], B) for k in ("w", "y", "gt"))
    clean = [b for b in range(B) if b not in (NAN_PROBLEM, INF_PROBLEM)]
    for name, got, want in (("w", w, wr), ("y", y, yr), ("gt", gt, gr)):
        assert np_same(got[clean], want[clean]), name
        assert np_same_or_nan(got, want), name
    assert guards_intact(t)
    for k in ("g", "E", "lo", "hi", "rho", "z") + (("y", "res") if init else ()):
        assert same(t["_bufs"][k], before[k]), f"{k} was written"
    taken = {v for b in clean for v in branches[b].values()}
    want = {ref.INSIDE, ref.POLAR} | (set() if max(shape[5][1], shape[5][3]) == 1 else {ref.BOUNDARY})
    print(f"{ids(shape)} {np.dtype(dtype).name} {'init' if init else 'update'}: branches of the clean problems "
          f"{[sum(1 for b in clean for v in branches[b].values() if v == k) for k in range(3)]}")
    assert taken == want, taken
    for b in clean:
        assert np.isfinite(w[b]).all() and np.isfinite(gt[b]).all()
    if not init:
        assert np_same_or_nan(host(res, B), rr) and np_same(host(res, B)[clean], rr[clean]), "res"
        assert np.isnan(rr[NAN_PROBLEM]).any() and np.isfinite(rr[clean]).all()
        assert not np.isfinite(w[INF_PROBLEM]).all()


# ---- 2. no cone rows, and q = 1 cones: the bits of the admm_lin calls
def lin_calls(solver, shape, t, init, batch=B):
    nx, nu, N, mx, mu, _ = shape
    if init:
        solver.admm_lin_init(nx, nu, mx, mu, N, batch, t["g"], t["E"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
    else:
        solver.admm_lin_update(nx, nu, mx, mu, N, batch, t["g"], t["E"], t["lo"], t["hi"], t["rho"], t["z"], t["w"], t["y"], t["gt"],
                               res=t["res"])


@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(14, 7, 5, 3, 2), (14, 7, 40, 5, 4)], ids=lambda s: "-".join(map(str, s)))
def test_without_cone_rows_the_bits_of_admm_lin(solver, shape, dtype, init):
    """lx = mx, lu = mu; qx, qu are ignored (0 and a number that divides nothing).  Data with NaN, Inf and infinite bounds."""
    nx, nu, N, mx, mu = shape
    full = (nx, nu, N, mx, mu, (mx, 0, mu, 7))
    d = {k: v.copy() for k, v in soc_data((nx, nu, N, mx, mu, (mx, 1, mu, 1)), dtype).items()}
    a, b = device_tensors(d), device_tensors(d)
    lin_calls(solver, full, a, init)
    run_update(solver, full, b, init)
    torch.cuda.synchronize()
    for k in ("w", "y", "gt", "res"):
        assert same(a["_bufs"][k], b["_bufs"][k]), k


@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_lines_give_the_bits_of_admm_lin_with_zero_and_infinity(solver, dtype, init):
    """q = 1 cones with f = +0 against the rows 0 <= s <= +Inf, on input without NaN."""
    nx, nu, N, mx, mu = 5, 3, 9, 6, 4
    shape = (nx, nu, N, mx, mu, (0, 1, 0, 1))
    d = {k: v.copy() for k, v in soc_data(shape, dtype).items()}
    d["z"][NAN_PROBLEM] = d["z"][0]
    d["lo"][:] = 0.0
    a, b = device_tensors(dict(d, hi=np.full_like(d["hi"], np.inf))), device_tensors(d)
    assert bool(torch.isnan(b["hi"]).all())
    lin_calls(solver, shape, a, init)
    run_update(solver, shape, b, init)
    torch.cuda.synchronize()
    for k in ("w", "y", "gt", "res"):
        assert same(a[k], b[k]), k
    w = host(b["w"], B)
    assert (w >= 0).all() and (w == 0).mean() > 0.2 and (w > 0).mean() > 0.2


# ---- 3. batch isolation: another problem's rows change nothing
@pytest.mark.parametrize("dtype", DTYPES)
def test_changing_one_problems_rows_changes_no_other_problem(solver, dtype):
    shape = SHAPES[3]
    d = soc_data(shape, dtype)
    a = device_tensors(d)
    ra = run_update(solver, shape, a, False).clone()
    d2 = {k: v.copy() for k, v in d.items()}
    for k in ("E", "lo", "w", "y", "z", "g", "rho"):
        d2[k][3] = d2[k][3] * dtype(1.5) + dtype(0.25)
    b = device_tensors(d2)
    rb = run_update(solver, shape, b, False)
    torch.cuda.synchronize()
    for k in ("w", "y", "gt"):
        x, y = a[k].view(B, -1), b[k].view(B, -1)
        assert not same(x[3], y[3]), k
        for p in (0, 1, 2, 4):
            assert same(x[p], y[p]), (k, p)
    assert all(same(ra[p], rb[p]) for p in (0, 1, 2, 4)) and not same(ra[3], rb[3])
    assert guards_intact(a) and guards_intact(b)


# ---- 4. the composite calls
ORDER = ("gamma", "lam", "r", "p", "z", "it", "fl", "w", "y", "gt", "res")


@functools.lru_cache(maxsize=None)
def step_problem(nx, nu, N, batch, seed=61):
    d = {k: v.astype(F32).astype(F64) for k, v in so.gen(nx, nu, N, seed=seed, batch=batch, dtype=F64).items()}
    for a in d.values():
        a.setflags(write=False)
    return d


class SocLoop:
    """Gt = G + rho E'E (admm_lin_form), its factorisation (kkt_step on Gt), the rows, and the buffers of the iteration."""

    def __init__(self, solver, shape, batch, dtype, d, E, lo, hi, rho, tol=1e-8, max_iter=100):
        nx, nu, N, mx, mu, cones = shape
        self.s, self.shape, self.batch, self.tol, self.max_iter = solver, shape, batch, tol, max_iter
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        self.E, self.rho = dev(np.asarray(E, dtype).reshape(-1)), dev(np.asarray(rho, dtype))
        nan = float("nan")
        self.Gt = solver.admm_lin_form(nx, nu, mx, mu, N, batch, self.G, self.E, self.rho)
        self.S = torch.full((batch * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        self.gamma = torch.full((batch * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, self.z = torch.zeros_like(self.gamma), torch.full_like(self.g, nan)
        _, fl = solver.kkt_step(nx, nu, N, batch, self.Gt, self.C, self.g, self.c, self.S, self.gamma, self.Ginv, self.Pinv, self.lam,
                                self.z, tol=tol, max_iter=max_iter)
        torch.cuda.synchronize()
        assert int(fl.sum()) == 0
        self.lo, self.hi = dev(np.asarray(lo).astype(dtype).reshape(-1)), dev(np.asarray(hi).astype(dtype).reshape(-1))
        self.w, self.y = torch.zeros_like(self.lo), torch.zeros_like(self.lo)
        self.gt = solver.admm_soc_init(nx, nu, mx, mu, cones, N, batch, self.g, self.E, self.lo, self.hi, self.rho, self.w, self.y)
        torch.cuda.synchronize()
        self.start = {k: getattr(self, k).clone() for k in ("lam", "w", "y", "gt")}

    def state(self):
        nan, batch = float("nan"), self.batch
        o = {k: v.clone() for k, v in self.start.items()}
        o.update(gamma=torch.full_like(self.gamma, nan), r=torch.full_like(self.gamma, nan), p=torch.full_like(self.gamma, nan),
                 z=torch.full_like(self.g, nan), res=torch.full((batch, 2), nan, dtype=self.g.dtype, device="cuda"),
                 it=torch.full((batch,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((batch,), 9, dtype=torch.uint8, device="cuda"))
        return o

    def mats(self):
        return self.Ginv, self.C, self.S, self.Pinv, self.E

    def two_calls(self, o, mats=None, shared=False):
        nx, nu, N, mx, mu, cones = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        resolve = self.s.kkt_resolve_shared if shared else self.s.kkt_resolve
        resolve(nx, nu, N, self.batch, Ginv, C, o["gt"], self.c, S, Pinv, o["gamma"], o["lam"], o["z"], r=o["r"], p=o["p"], tol=self.tol,
                max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        if shared:     # the update has no shared form of its own: one problem's E, repeated
            E = E.repeat(self.batch)
        self.s.admm_soc_update(nx, nu, mx, mu, cones, N, self.batch, self.g, E, self.lo, self.hi, self.rho, o["z"], o["w"], o["y"], o["gt"],
                               res=o["res"])

    def one_call(self, o, mats=None, shared=False):
        nx, nu, N, mx, mu, cones = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        step = self.s.admm_soc_step_shared if shared else self.s.admm_soc_step
        step(nx, nu, mx, mu, cones, N, self.batch, Ginv, C, self.g, self.c, E, self.lo, self.hi, self.rho, S, Pinv, o["gamma"], o["lam"],
             o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter, iters=o["it"],
             max_iter_exit=o["fl"])

    def graph(self, o, mats=None, shared=False):
        nx, nu, N, mx, mu, cones = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        make = self.s.graph_admm_soc_step_shared if shared else self.s.graph_admm_soc_step
        return make(nx, nu, mx, mu, cones, N, self.batch, Ginv, C, self.g, self.c, E, self.lo, self.hi, self.rho, S, Pinv, o["gamma"],
                    o["lam"], o["r"], o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])


def random_rows(shape, batch, seed=3):
    """E of order 0.5; the linear rows within +-0.2, the cone offsets f = 0.2 on the head rows and 0 elsewhere; hi NaN on cone rows."""
    nx, nu, N, mx, mu, cones = shape
    _, nw, ne, _ = lin.sizes(nx, nu, mx, mu, N)
    head, _ = ref.layout(nx, nu, mx, mu, cones, N)
    E = (0.5 * np.random.default_rng(seed).standard_normal((batch, ne))).astype(F32).astype(F64)
    lo, hi = np.full((batch, nw), -0.2), np.full((batch, nw), 0.2)
    lo[:, head >= 0], hi[:, head >= 0] = 0.0, np.nan
    lo[:, ref.heads(head)] = 0.2
    return E, lo, hi


STEP_SHAPES = [(14, 7, 5, 5, 4, (2, 3, 0, 4)), (3, 3, 5, 3, 2, (0, 3, 1, 1))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids)
def test_step_is_resolve_plus_update_and_the_graph_replays_it(solver, shape, dtype):
    nx, nu, N = shape[:3]
    batch = 3
    E, lo, hi = random_rows(shape, batch)
    L = SocLoop(solver, shape, batch, dtype, step_problem(nx, nu, N, batch), E, lo, hi, 0.5 * (np.arange(batch) + 2.0))
    a, b, g, g2 = L.state(), L.state(), L.state(), L.state()
    solver.reserve(L.g.element_size(), nx, N, batch)
    gr, gr2 = L.graph(g), L.graph(g2)
    for _ in range(2):     # the second iteration takes the first one's lambda, w, y, gt
        L.two_calls(a)
        L.one_call(b)
        gr.launch()
        gr2.launch()
    torch.cuda.synchronize()
    gr.close()
    gr2.close()
    for k in ORDER:
        assert same(a[k], b[k]), f"step vs resolve + update: {k}"
        assert same(b[k], g[k]), f"graph vs step: {k}"
        assert same(g[k], g2[k]), f"two replays: {k}"
    assert int(b["fl"].sum()) == 0 and all(bool(torch.isfinite(b[k]).all()) for k in ("z", "w", "y", "gt", "res"))
    assert int((b["y"] != 0).sum()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_twin(solver, dtype):
    """One plant (problem 0's G, C and E, one rho), `batch` gradients and rows: the shared call against the per-problem call on copies
    of the single matrices (path FUSED, as include/gbdpcg.h states the equivalence for kkt_resolve), and its graph."""
    shape = STEP_SHAPES[0]
    nx, nu, N = shape[:3]
    batch = 3
    d = dict(step_problem(nx, nu, N, batch))
    d["G"], d["C"] = np.repeat(d["G"][:1], batch, axis=0), np.repeat(d["C"][:1], batch, axis=0)
    E, lo, hi = random_rows(shape, batch)
    E = np.repeat(E[:1], batch, axis=0)
    lo = lo * np.array([1.0, 0.5, 2.0])[:, None]
    L = SocLoop(solver, shape, batch, dtype, d, E, lo, hi, np.full(batch, 1.5))
    per = lambda t: None if t is None else t[:t.numel() // batch].clone()   # noqa: E731
    single = tuple(per(m) for m in L.mats())
    copies = tuple(None if m is None else m.repeat(batch) for m in single)
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b, c, g = L.state(), L.state(), L.state(), L.state()
        solver.reserve(L.g.element_size(), nx, N, batch)
        gr = L.graph(g, mats=single, shared=True)
        for _ in range(2):
            L.one_call(a, mats=copies)
            L.one_call(b, mats=single, shared=True)
            L.two_calls(c, mats=single, shared=True)
            gr.launch()
        torch.cuda.synchronize()
        gr.close()
    finally:
        solver.set_path(binding.PATH_AUTO)
    for k in ORDER:
        assert same(a[k], b[k]), f"shared vs copies: {k}"
        assert same(b[k], c[k]), f"shared step vs shared resolve + update: {k}"
        assert same(b[k], g[k]), f"shared graph: {k}"
    assert int(b["fl"].sum()) == 0 and bool(torch.isfinite(b["z"]).all()) and int((b["y"] != 0).sum()) > 0


# ---- 5. arguments: every refusal with a live handle, nothing written
STEP_ARGS = ("Ginv", "C", "g", "c", "E", "lo", "hi", "rho", "S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z", "w",
             "y", "gt", "res")
WRITTEN = ("gamma", "lam", "r", "p", "z", "w", "y", "gt", "res")


@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_refusals_write_nothing(solver, suf, tt):
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = torch.zeros(1 << 16, dtype=tt, device="cuda")
    rho = torch.ones(3, dtype=tt, device="cuda")
    outs = {k: torch.full((1 << 14,), 777.0, dtype=tt, device="cuda") for k in WRITTEN}
    it = torch.full((3,), 777, dtype=torch.int32, device="cuda")
    fl = torch.full((3,), 77, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def values(null=(), **over):
        v = {k: P(ins) for k in ("Ginv", "C", "g", "c", "E", "lo", "hi", "S", "Pinv")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(it=P(it), fl=P(fl), tol=1e-6, max_iter=10, nx=6, nu=3, mx=5, mu=4, lx=2, qx=3, lu=0, qu=4, N=4, batch=3)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    def sizes(v):
        return (solver.h,) + tuple(v[k] for k in ("nx", "nu", "mx", "mu", "lx", "qx", "lu", "qu", "N", "batch"))

    def step(name, v, graph=None):
        last = ctypes.byref(graph) if graph is not None else s
        return getattr(lib, f"gbdpcg_{name}_{suf}")(*sizes(v), *(v[k] for k in STEP_ARGS), last)

    def update(v, init=False):
        head = sizes(v) + (v["g"], v["E"], v["lo"], v["hi"], v["rho"])
        if init:
            return getattr(lib, f"gbdpcg_admm_soc_init_{suf}")(*head, v["w"], v["y"], v["gt"], s)
        return getattr(lib, f"gbdpcg_admm_soc_update_{suf}")(*head, v["z"], v["w"], v["y"], v["gt"], v["res"], s)

    graph = ctypes.c_void_p()
    steps = [("admm_soc_step", None), ("admm_soc_step_shared", None), ("graph_create_admm_soc_step", graph),
             ("graph_create_admm_soc_step_shared", graph)]
    calls = [("init", lambda v: update(v, True)), ("update", update)] + [(n, lambda v, n=n, g=g: step(n, v, g)) for n, g in steps]
    for k in ("g", "E", "lo", "hi", "rho", "w", "y", "gt"):
        assert update(values(null=(k,)), init=True) == 1, k
    for k in ("g", "E", "lo", "hi", "rho", "z", "w", "y", "gt", "res"):
        assert update(values(null=(k,))) == 1, k
    for name, gr in steps:
        for k in STEP_ARGS:
            if k in ("Pinv", "r", "p", "fl", "tol", "max_iter"):
                continue
            assert step(name, values(null=(k,)), gr) == 1, (name, k)
    for what, call in calls:
        for k in ("nx", "nu", "N", "batch"):
            assert call(values(**{k: 0})) == 1, (what, k)
        assert call(values(mx=0, mu=0, lx=0, lu=0)) == 1, what                  # no rows
        assert call(values(lx=6)) == 1 and call(values(lu=5)) == 1, what        # more linear rows than rows
        assert call(values(qx=0)) == 1 and call(values(qu=0)) == 1, what        # cone rows and q = 0
        assert call(values(qx=2)) == 1 and call(values(qu=3)) == 1, what        # not whole cones
        assert call(values(mx=65, lx=65)) == 4 and call(values(mu=68)) == 4, what      # above 64 rows per block
        assert call(values(mx=66, lx=67)) == 1, what                            # INVALID before UNSUPPORTED
        assert call(values(mx=64, mu=64, lx=0, qx=8, lu=0, qu=64, nx=200, nu=100)) == 4, what
    torch.cuda.synchronize()
    assert not graph.value
    assert all(bool((t == 777.0).all()) for t in outs.values()) and bool((it == 777).all()) and bool((fl == 77).all())
    # with no cone rows q is ignored; the limits themselves are taken
    assert update(values(lx=5, qx=0, lu=4, qu=0)) == 0 and update(values(lx=5, qx=0, lu=4, qu=0), init=True) == 0
    assert update(values(mx=64, mu=64, lx=0, qx=8, lu=0, qu=64)) == 0
    torch.cuda.synchronize()


# ---- 6. convergence on the problems tests/test_admm_soc_reference.py pins
@pytest.mark.parametrize("dtype", DTYPES)
def test_eighty_replays_follow_the_fp64_twin(solver, dtype):
    nx, nu, N, batch = ref.CONV_SHAPE
    mx, mu = ref.CONV_ROWS
    d, E, lo, hi, _ = ref.convergence_inputs()
    history = ref.convergence_reference(4000)
    K = 80
    L = SocLoop(solver, (nx, nu, N, mx, mu, ref.CONV_CONES), batch, dtype, d, E, lo, hi, np.array(ref.CONV_RHO), tol=PCG_TOL[dtype],
                max_iter=200)
    o = L.state()
    solver.reserve(L.g.element_size(), nx, N, batch)
    gr = L.graph(o)
    flags = torch.zeros_like(o["fl"])
    for k in range(1, K + 1):
        gr.launch()
        flags |= o["fl"]
        if k == 1:
            res1 = o["res"].clone()
    torch.cuda.synchronize()
    gr.close()
    what = np.dtype(dtype).name
    res1, res80 = res1.cpu().numpy().astype(F64), o["res"].cpu().numpy().astype(F64)
    w = host(o["w"], batch).astype(F64)
    assert int(flags.sum()) == 0, "a solve ran out of iterations"
    close = rel = 0.0
    for b in range(batch):
        h = history[b]
        dist = np.abs(w[b] - h["w"][K - 1]).max()
        twin = np.array([h["r_prim"][K - 1] / h["r_prim"][0], h["r_dual"][K - 1] / h["r_dual"][0]])
        ratio = res80[b] / res1[b]
        off = (np.abs(ratio - twin) / twin).max()
        close, rel = max(close, dist), max(rel, off)
        print(f"{what} problem {b}: ||w(80) - w_twin(80)||_inf {dist:.3e}  res(80)/res(1) {ratio[0]:.6e} {ratio[1]:.6e} "
              f"(twin {twin[0]:.6e} {twin[1]:.6e}, relative difference {off:.3e})  res(80) {res80[b, 0]:.3e} {res80[b, 1]:.3e}")
        assert (res80[b] < res1[b]).all(), (b, res1[b], res80[b])
    print(f"{what}: worst ||w(80) - w_twin(80)||_inf {close:.3e} (bound {CLOSE[dtype]}), worst relative difference of res(80)/res(1) "
          f"{rel:.3e} (bound {RATIO[dtype]})")
    assert close <= CLOSE[dtype], close
    assert rel <= RATIO[dtype], rel
