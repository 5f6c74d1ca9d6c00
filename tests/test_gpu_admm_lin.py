"""ADMM with stage-wise linear inequality rows lo <= E z <= hi on a kept factorisation, on the device (csrc/admm_rows.hip and the
composite calls of csrc/api_kkt.hip, through the C ABI): gbdpcg_admm_lin_form_*, _init_*, _update_*, _step_*, the shared twin and the two
graphs.  PARITY UNPINNED: the reference tree has no code, fixture or output for these steps.

Reference: tests/admm_lin_ref.py.  Formation, initialisation and update are defined to the bit (every line one IEEE operation, the
chains of fused multiply-adds in a fixed order), so Gt, w, y, gt and the two norms are compared for EQUALITY with form_ref / update_ref,
which evaluate the chains in exact rational arithmetic with one rounding per operation.  The composite calls are compared bit for bit
with the calls they are made of, and with E = I everything is compared bit for bit with the box calls (tests/test_gpu_admm.py).
Convergence (the last test) runs the three problems tests/test_admm_lin_reference.py pins, 80 graph replays from w = y = 0:
 (a) ||w_dev(80) - w*||_inf <= 2 ||w_ref(80) - w*||_inf + 80 STEP_TOL ||w*||_inf, the rule of test_gpu_admm.py (b) with STEP_TOL of
     tests/test_gpu_reg.py: a fixed-rho ADMM iteration is an averaged operator, per-step errors add and do not grow;
 (b) ||w_dev(80) - w_ref(80)||_inf <= CLOSE[dtype]: the closeness to the fp64 reference's 80th iterate, see CLOSE below;
 (c) res(80) <= 1e-2 res(1) for the primal residual (the reference's worst problem gives 4.0e-3) and both residuals decreased;
 (d) lo <= w <= hi exactly, no solve ran out of iterations.
Run with -s for the measured figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_ref as ref  # noqa: E402
import admm_ref  # noqa: E402
from admm_util import bits, dev, host, knot_chunk, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_reg.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
# ||w_dev(80) - w_ref(80)||_inf, the worst of the three convergence problems, measured once on the MI355X against the fp64
# reference (profiles/r11_admm_lin.txt): 2.781e-6 in fp32 (2.0e-6 / 2.2e-6 / 2.8e-6 per problem), 1.092e-12 in fp64 (1.1e-12 / 1.0e-12 /
# 6.7e-13); times 4 for other boxes and PCG tolerances
CLOSE = {F32: 1.12e-5, F64: 4.4e-12}


NC = knot_chunk(14, 7, 4, 2)
assert NC == 39 and knot_chunk(14, 7, 64, 64) == 2
# nx, nu, N, B, mx, mu
SHAPES = [(2, 1, 3, 2, 1, 1),
          (3, 2, 1, 2, 2, 0),          # N = 1: no control block at all
          (2, 1, 4, 2, 5, 0),          # more rows than columns, no control rows
          (4, 3, 3, 2, 0, 2),          # no state rows
          (14, 7, 5, 3, 3, 2),
          (14, 7, NC + 1, 2, 4, 2),    # one knot more than a chunk
          (14, 7, 3, 2, 64, 64)]       # the row limit: chunks of two knots


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


INPUTS = ("G", "E", "g", "z", "w", "y", "lo", "hi", "rho")


@functools.lru_cache(maxsize=None)
def lin_data(shape, dtype):
    """Random data of order 1: G with symmetric blocks, E, g, z, w, y, bounds near +-0.3 with a third of each side infinite, rho_b in
    [0.5, 4]: arrays [B, .] of `dtype`, read-only."""
    nx, nu, N, B, mx, mu = shape
    nz, nw, ne, ng = ref.sizes(nx, nu, mx, mu, N)
    rng = np.random.default_rng(7000 + 13 * nz + nw)
    G = rng.standard_normal((B, ng))
    for m, n, _, _, _, go in ref.blocks(nx, nu, 0, 0, N):
        blk = G[:, go:go + n * n].reshape(B, n, n)
        G[:, go:go + n * n] = (blk + blk.transpose(0, 2, 1)).reshape(B, -1)
    d = dict(G=G, E=0.5 * rng.standard_normal((B, ne)), g=rng.standard_normal((B, nz)), z=rng.standard_normal((B, nz)),
             w=rng.standard_normal((B, nw)), y=0.3 * rng.standard_normal((B, nw)),
             lo=-0.3 + 0.05 * rng.standard_normal((B, nw)), hi=0.3 + 0.05 * rng.standard_normal((B, nw)), rho=rng.uniform(0.5, 4.0, B))
    d["lo"][rng.random((B, nw)) < 1.0 / 3.0] = -np.inf
    d["hi"][rng.random((B, nw)) < 1.0 / 3.0] = np.inf
    d = {k: v.astype(dtype) for k, v in d.items()}
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def form_reference(shape, dtype):
    nx, nu, N, B, mx, mu = shape
    d = lin_data(shape, dtype)
    return ref.form_ref(dtype, nx, nu, mx, mu, N, d["G"], d["E"], d["rho"])


@functools.lru_cache(maxsize=None)
def update_reference(shape, dtype, init):
    nx, nu, N, B, mx, mu = shape
    d = lin_data(shape, dtype)
    return ref.update_ref(dtype, nx, nu, mx, mu, N, d["g"], d["E"], d["lo"], d["hi"], d["rho"], None if init else d["z"], d["w"], d["y"])


def device_tensors(d, offset=None, guard=0):
    """The arrays of lin_data on the device, flat, plus Gt, gt (NaN) and res.  offset: every array starts `offset` elements into a buffer
    of its own whose base the allocator aligns: 0 -> 16-byte aligned bases, 1 -> every base off by one element.  guard: that many NaN
    elements either side of every array; the buffers come back in t["_bufs"]."""
    t, bufs = {}, {}
    B = d["rho"].size
    extra = [("Gt", np.full_like(d["G"], np.nan)), ("gt", np.full_like(d["g"], np.nan)), ("res", np.full((B, 2), np.nan, d["g"].dtype))]
    for k, a in list(d.items()) + extra:
        flat = dev(a.reshape(-1))
        if offset is not None or guard:
            lead = guard + (offset or 0)
            buf = torch.full((flat.numel() + lead + guard + 8,), float("nan"), dtype=flat.dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[lead:lead + flat.numel()] = flat
            bufs[k], flat = buf, buf[lead:lead + flat.numel()]
        t[k] = flat
    t["_bufs"] = bufs
    return t


def run_form(solver, shape, t, out="Gt"):
    nx, nu, N, B, mx, mu = shape
    return solver.admm_lin_form(nx, nu, mx, mu, N, B, t["G"], t["E"], t["rho"], Gt=t[out])


def run_update(solver, shape, t, init):
    nx, nu, N, B, mx, mu = shape
    if init:
        solver.admm_lin_init(nx, nu, mx, mu, N, B, t["g"], t["E"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
        return None
    return solver.admm_lin_update(nx, nu, mx, mu, N, B, t["g"], t["E"], t["lo"], t["hi"], t["rho"], t["z"], t["w"], t["y"], t["gt"],
                                  res=t["res"])


def ids(shape):
    return "-".join(str(v) for v in shape)


# ---- 1. formation, initialisation and update against the exact references, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_form_vs_reference(solver, shape, dtype):
    nx, nu, N, B, mx, mu = shape
    d = lin_data(shape, dtype)
    t = device_tensors(d)
    run_form(solver, shape, t)
    inplace = t["G"].clone()
    t2 = dict(t, G=inplace, Gt=inplace)
    run_form(solver, shape, t2, out="G")
    torch.cuda.synchronize()
    Gt = host(t["Gt"], B)
    assert np_same(Gt, form_reference(shape, dtype)), "Gt"
    assert same(inplace, t["Gt"]), "d_Gt == d_G"
    assert same(t["G"], dev(d["G"].reshape(-1)))
    for _, n, _, _, _, go in ref.blocks(nx, nu, 0, 0, N):     # bit-symmetric, as G is
        blk = Gt[:, go:go + n * n].reshape(B, n, n)
        assert np_same(blk, np.ascontiguousarray(blk.transpose(0, 2, 1)))


@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_update_and_init_vs_reference(solver, shape, dtype, init):
    B = shape[3]
    d = lin_data(shape, dtype)
    wr, yr, gr, rr = update_reference(shape, dtype, init)
    t = device_tensors(d)
    res = run_update(solver, shape, t, init)
    torch.cuda.synchronize()
    w, y, gt = (host(t[k], B) for k in ("w", "y", "gt"))
    assert np_same(w, wr), "w"
    assert np_same(y, yr), "y"
    assert np_same(gt, gr), "gt"
    assert ((w >= d["lo"]) & (w <= d["hi"])).all()
    for k in ("g", "E", "lo", "hi", "rho", "z"):
        assert same(t[k], dev(d[k].reshape(-1))), f"{k} was written"
    if init:
        assert np_same(y, d["y"]) and bool(torch.isnan(t["res"]).all())
        return
    assert np_same(host(res, B), rr), "res"
    assert (w[y > 0] == d["hi"][y > 0]).all() and (w[y < 0] == d["lo"][y < 0]).all()
    low, high = float((y < 0).mean()), float((y > 0).mean())
    print(f"{shape} {np.dtype(dtype).name}: {low:.2f} of the rows clipped below, {high:.2f} above")
    if w.size >= 64:
        assert low > 0.1 and high > 0.1


# ---- 2. aligned and misaligned base pointers give the same bits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES[:1] + SHAPES[3:6], ids=ids)
def test_aligned_and_misaligned_bases_agree(solver, shape, dtype):
    B = shape[3]
    d = lin_data(shape, dtype)
    out = []
    for offset in (0, 1):
        got = {}
        for init in (True, False):
            t = device_tensors(d, offset)
            assert all(t[k].data_ptr() % 16 == (0 if offset == 0 else t[k].element_size()) for k in INPUTS + ("Gt", "gt", "res"))
            run_update(solver, shape, t, init)
            if not init:
                run_form(solver, shape, t)
            torch.cuda.synchronize()
            got.update({(init, k): t[k].clone() for k in ("w", "y", "gt") + (() if init else ("res", "Gt"))})
        out.append(got)
    for k in out[0]:
        assert same(out[0][k], out[1][k]), k
    assert np_same(host(out[1][(False, "Gt")], B), form_reference(shape, dtype))
    assert np_same(host(out[1][(False, "w")], B), update_reference(shape, dtype, False)[0])
    assert np_same(host(out[1][(True, "gt")], B), update_reference(shape, dtype, True)[2])


# ---- 3. E = I: the box calls, bit for bit
@functools.lru_cache(maxsize=None)
def step_problem(nx, nu, N, B, seed=61):
    d = {k: v.astype(F32).astype(F64) for k, v in so.gen(nx, nu, N, seed=seed, batch=B, dtype=F64).items()}
    for a in d.values():
        a.setflags(write=False)
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(5, 2, 10, 4), (14, 7, 5, 3)])
def test_identity_rows_give_the_bits_of_the_box_calls(solver, nx, nu, N, B, dtype):
    """Finite random data without negative zeros.  The last claim (kkt_step on Gt against kkt_step_reg on G) rests on the formation
    kernels rounding Q_ii + rho once."""
    nz, _, _, ng = ref.sizes(nx, nu, nx, nu, N)
    rng = np.random.default_rng(5 + nz)
    E = dev(np.tile(ref.identity_E(nx, nu, N, dtype), B))
    rho_h = rng.uniform(0.5, 4.0, B).astype(dtype)
    rho = dev(rho_h)
    z, g, w, y = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    lo, hi = (-0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype), (0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype)
    lo[rng.random((B, nz)) < 1.0 / 3.0], hi[rng.random((B, nz)) < 1.0 / 3.0] = -np.inf, np.inf
    t = {k: dev(v.reshape(-1)) for k, v in dict(z=z, g=g, lo=lo, hi=hi).items()}
    # formation
    d = step_problem(nx, nu, N, B)
    G = d["G"].astype(dtype)
    Gt = solver.admm_lin_form(nx, nu, nx, nu, N, B, dev(G.reshape(-1)), E, rho)
    want = G.copy()
    for m, _, _, _, _, go in ref.blocks(nx, nu, nx, nu, N):
        idx = go + np.arange(m) * (m + 1)
        want[:, idx] = G[:, idx] + rho_h[:, None]
    torch.cuda.synchronize()
    assert np_same(host(Gt, B), want), "Gt is not G with fl(diag + rho)"
    # init and update
    for init in (True, False):
        a = {k: dev(v.reshape(-1)) for k, v in dict(w=w, y=y).items()}
        b = {k: v.clone() for k, v in a.items()}
        if init:
            a["gt"] = solver.admm_init(nx, nu, N, B, t["g"], t["lo"], t["hi"], rho, a["w"], a["y"])
            b["gt"] = solver.admm_lin_init(nx, nu, nx, nu, N, B, t["g"], E, t["lo"], t["hi"], rho, b["w"], b["y"])
        else:
            a["gt"], b["gt"] = torch.empty_like(t["g"]), torch.empty_like(t["g"])
            a["res"] = solver.admm_update(nx, nu, N, B, t["g"], t["lo"], t["hi"], rho, t["z"], a["w"], a["y"], a["gt"])
            b["res"] = solver.admm_lin_update(nx, nu, nx, nu, N, B, t["g"], E, t["lo"], t["hi"], rho, t["z"], b["w"], b["y"], b["gt"])
        torch.cuda.synchronize()
        for k in a:
            assert same(a[k], b[k]), (init, k)
    # kkt_step on Gt + admm_lin_step against kkt_step_reg + admm_step
    box = BoxLoop(solver, nx, nu, N, B, dtype, d, rho_h)
    lin = LinLoop(solver, (nx, nu, N, B, nx, nu), dtype, d, np.tile(ref.identity_E(nx, nu, N), (B, 1)), rho_h,
                  lo=host(box.lo, B).astype(F64), hi=host(box.hi, B).astype(F64))
    for k in ("Ginv", "S", "Pinv", "lam", "z", "gt"):
        assert same(getattr(box, k), getattr(lin, k)), f"{k}: kkt_step on Gt against kkt_step_reg on G"
    a, b = box.state(), lin.state()
    for _ in range(2):
        box.one_call(a)
        lin.one_call(b)
    torch.cuda.synchronize()
    for k in ORDER:
        assert same(a[k], b[k]), k
    assert int((b["y"] != 0).sum()) > 0


# ---- the loops of the composite calls
ORDER = ("gamma", "lam", "r", "p", "z", "it", "fl", "w", "y", "gt", "res")


class LinLoop:
    """Gt = G + rho E'E (admm_lin_form), its factorisation (kkt_step on Gt), bounds on the rows, and the buffers of the iteration."""

    def __init__(self, solver, shape, dtype, d, E, rho, lo=None, hi=None, tol=1e-8, max_iter=100):
        nx, nu, N, B, mx, mu = shape
        self.s, self.shape, self.tol, self.max_iter = solver, shape, tol, max_iter
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        if N == 1:
            self.C = None
        self.E, self.rho = dev(np.asarray(E, dtype).reshape(-1)), dev(np.asarray(rho, dtype))
        nan = float("nan")
        self.Gt = solver.admm_lin_form(nx, nu, mx, mu, N, B, self.G, self.E, self.rho)
        self.S = torch.full((B * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        self.gamma = torch.full((B * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, self.z = torch.zeros_like(self.gamma), torch.full_like(self.g, nan)
        _, fl = solver.kkt_step(nx, nu, N, B, self.Gt, self.C, self.g, self.c, self.S, self.gamma, self.Ginv, self.Pinv, self.lam, self.z,
                                tol=tol, max_iter=max_iter)
        torch.cuda.synchronize()
        assert int(fl.sum()) == 0
        if lo is None:     # half of what the rows of the equality-constrained solution reach, both sides
            z0, Eh = host(self.z, B).astype(F64), np.asarray(E, F64).reshape(B, -1)
            v0 = np.stack([ref.dense_E(nx, nu, mx, mu, N, Eh[b]) @ z0[b] for b in range(B)])
            hi = np.repeat(np.float32(0.5 * np.abs(v0).max(axis=1)).astype(F64)[:, None], v0.shape[1], axis=1)
            lo = -hi
        self.lo, self.hi = dev(np.asarray(lo).astype(dtype).reshape(-1)), dev(np.asarray(hi).astype(dtype).reshape(-1))
        self.w, self.y = torch.zeros_like(self.lo), torch.zeros_like(self.lo)
        self.gt = solver.admm_lin_init(nx, nu, mx, mu, N, B, self.g, self.E, self.lo, self.hi, self.rho, self.w, self.y)
        torch.cuda.synchronize()
        self.start = {k: getattr(self, k).clone() for k in ("lam", "w", "y", "gt")}

    def state(self):
        """Fresh output buffers that start from the saved (lambda, w, y, gt)."""
        nan, B = float("nan"), self.shape[3]
        o = {k: v.clone() for k, v in self.start.items()}
        o.update(gamma=torch.full_like(self.gamma, nan), r=torch.full_like(self.gamma, nan), p=torch.full_like(self.gamma, nan),
                 z=torch.full_like(self.g, nan), res=torch.full((B, 2), nan, dtype=self.g.dtype, device="cuda"),
                 it=torch.full((B,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))
        return o

    def mats(self):
        return self.Ginv, self.C, self.S, self.Pinv, self.E

    def two_calls(self, o, mats=None, shared=False, rho=None):
        nx, nu, N, B, mx, mu = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        resolve = self.s.kkt_resolve_shared if shared else self.s.kkt_resolve
        resolve(nx, nu, N, B, Ginv, C, o["gt"], self.c, S, Pinv, o["gamma"], o["lam"], o["z"], r=o["r"], p=o["p"], tol=self.tol,
                max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])
        if shared:     # the update has no shared form of its own: one problem's E, repeated
            E = E.repeat(B)
        self.s.admm_lin_update(nx, nu, mx, mu, N, B, self.g, E, self.lo, self.hi, self.rho if rho is None else rho, o["z"], o["w"],
                               o["y"], o["gt"], res=o["res"])

    def one_call(self, o, mats=None, shared=False, rho=None):
        nx, nu, N, B, mx, mu = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        step = self.s.admm_lin_step_shared if shared else self.s.admm_lin_step
        step(nx, nu, mx, mu, N, B, Ginv, C, self.g, self.c, E, self.lo, self.hi, self.rho if rho is None else rho, S, Pinv, o["gamma"],
             o["lam"], o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=self.tol, max_iter=self.max_iter,
             iters=o["it"], max_iter_exit=o["fl"])

    def graph(self, o, mats=None, shared=False):
        nx, nu, N, B, mx, mu = self.shape
        Ginv, C, S, Pinv, E = mats or self.mats()
        make = self.s.graph_admm_lin_step_shared if shared else self.s.graph_admm_lin_step
        return make(nx, nu, mx, mu, N, B, Ginv, C, self.g, self.c, E, self.lo, self.hi, self.rho, S, Pinv, o["gamma"], o["lam"], o["r"],
                    o["p"], self.tol, self.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])


class BoxLoop:
    """The box counterpart (tests/test_gpu_admm.py): kkt_step_reg on G with rho, a box around its z, admm_init."""

    def __init__(self, solver, nx, nu, N, B, dtype, d, rho, tol=1e-8, max_iter=100):
        self.s, self.shape, self.tol, self.max_iter = solver, (nx, nu, N, B), tol, max_iter
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        self.rho = dev(np.asarray(rho, dtype))
        nan = float("nan")
        self.S = torch.full((B * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        self.gamma = torch.full((B * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, self.z = torch.zeros_like(self.gamma), torch.full_like(self.g, nan)
        _, fl = solver.kkt_step_reg(nx, nu, N, B, self.G, self.C, self.g, self.c, self.rho, self.S, self.gamma, self.Ginv, self.Pinv,
                                    self.lam, self.z, tol=tol, max_iter=max_iter)
        torch.cuda.synchronize()
        assert int(fl.sum()) == 0
        z0 = host(self.z, B).astype(F64)
        bounds = [admm_ref.box(z0[b], nx, nu, N) for b in range(B)]
        self.lo, self.hi = (dev(np.stack([p[i] for p in bounds]).astype(dtype).reshape(-1)) for i in range(2))
        self.w, self.y = torch.zeros_like(self.g), torch.zeros_like(self.g)
        self.gt = solver.admm_init(nx, nu, N, B, self.g, self.lo, self.hi, self.rho, self.w, self.y)
        torch.cuda.synchronize()
        self.start = {k: getattr(self, k).clone() for k in ("lam", "w", "y", "gt")}

    state = LinLoop.state

    def one_call(self, o):
        nx, nu, N, B = self.shape
        self.s.admm_step(nx, nu, N, B, self.Ginv, self.C, self.g, self.c, self.lo, self.hi, self.rho, self.S, self.Pinv, o["gamma"],
                         o["lam"], o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=self.tol,
                         max_iter=self.max_iter, iters=o["it"], max_iter_exit=o["fl"])


def random_rows(shape, seed=3):
    nx, nu, N, B, mx, mu = shape
    ne = ref.sizes(nx, nu, mx, mu, N)[2]
    return (0.5 * np.random.default_rng(seed).standard_normal((B, ne))).astype(F32).astype(F64)


STEP_SHAPES = [(14, 7, 5, 3, 3, 2), (3, 3, 5, 2, 2, 1), (14, 7, NC + 1, 2, 4, 2)]


# ---- 4. the composite calls
@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids)
def test_step_is_kkt_resolve_plus_update(solver, shape, dtype, mode):
    nx, nu, N, B, mx, mu = shape
    L = LinLoop(solver, shape, dtype, step_problem(nx, nu, N, B), random_rows(shape), 0.5 * (np.arange(B) + 2.0))
    solver.set_symmetric(mode)
    try:
        a, b = L.state(), L.state()
        for _ in range(2):     # the second iteration takes the first one's lambda, w, y, gt
            L.two_calls(a)
            L.one_call(b)
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    for k in ORDER:
        assert same(a[k], b[k]), k
    assert int(b["fl"].sum()) == 0 and all(bool(torch.isfinite(b[k]).all()) for k in ("z", "w", "y", "gt", "res"))
    active = int((b["y"] != 0).sum())
    print(f"{shape} {np.dtype(dtype).name} mode {mode}: {active} of {b['y'].numel()} rows active")
    assert active > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STEP_SHAPES[:2], ids=ids)
def test_shared_twin(solver, shape, dtype):
    """One plant (problem 0's G, C and E, one rho), B gradients and bounds: the shared call against the per-problem call on B copies of
    the single matrices (path FUSED, as include/gbdpcg.h states the equivalence for kkt_resolve), against the two calls it is made
    of, and its graph against itself."""
    nx, nu, N, B, mx, mu = shape
    d = dict(step_problem(nx, nu, N, B))
    d["G"], d["C"] = np.repeat(d["G"][:1], B, axis=0), np.repeat(d["C"][:1], B, axis=0)
    E = np.repeat(random_rows(shape)[:1], B, axis=0)
    L = LinLoop(solver, shape, dtype, d, E, np.full(B, 1.5))
    per = lambda t: None if t is None else t[:t.numel() // B].clone()   # noqa: E731
    single = tuple(per(m) for m in L.mats())
    copies = tuple(None if m is None else m.repeat(B) for m in single)
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b, c, g = L.state(), L.state(), L.state(), L.state()
        solver.reserve(L.g.element_size(), nx, N, B)
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_and_rho_rewritten_in_place(solver, dtype):
    shape = (14, 7, 5, 3, 3, 2)
    nx, nu, N, B, mx, mu = shape
    rho1 = 0.5 * (np.arange(B) + 2.0)
    L = LinLoop(solver, shape, dtype, step_problem(nx, nu, N, B), random_rows(shape), rho1)
    g = L.state()
    solver.reserve(L.g.element_size(), nx, N, B)
    gr = L.graph(g)
    e = L.state()
    for i in range(3):
        gr.launch()
        L.one_call(e)
        torch.cuda.synchronize()
        for k in ORDER:
            assert same(g[k], e[k]), (i, k)
        if i == 0:
            first = {k: g[k].clone() for k in ORDER}
    # rho rewritten in place: the matrices are what they were (by design), the update follows the new values
    rho2 = dev((rho1 + 0.75).astype(dtype))
    fresh = L.state()
    for k in ("lam", "w", "y", "gt"):
        g[k].copy_(fresh[k])
    L.rho.copy_(rho2)
    gr.launch()
    L.one_call(fresh, rho=rho2.clone())
    torch.cuda.synchronize()
    for k in ORDER:
        assert same(g[k], fresh[k]), k
    for k in ("gamma", "lam", "z", "w", "y", "res"):
        r0 = first[k][:, 0] if k == "res" else first[k]
        got = g[k][:, 0] if k == "res" else g[k]
        assert same(got, r0), f"{k} must not depend on rho rewritten after the formation"
    assert not bool((g["res"][:, 1] == first["res"][:, 1]).any()) and not same(g["gt"], first["gt"])
    gr.close()


# ---- 5. NaN, Inf, footprint
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_problem_and_infinite_bounds_clip_nothing(solver, dtype):
    shape = (14, 7, 5, 3, 3, 2)
    nx, nu, N, B, mx, mu = shape
    d = lin_data(shape, dtype)
    clean = device_tensors(d)
    rc = run_update(solver, shape, clean, False).clone()
    run_form(solver, shape, clean)
    for k, j in (("z", 30), ("E", 17), ("lo", 9), ("hi", 9)):
        t = device_tensors(d)
        t[k].view(B, -1)[1, j] = float("nan")
        res = run_update(solver, shape, t, False)
        run_form(solver, shape, t)
        torch.cuda.synchronize()
        if k in ("z", "E"):
            assert bool(torch.isnan(res[1]).any()), k
        for p in (0, 2):
            for o in ("w", "y", "gt", "Gt"):
                assert same(t[o].view(B, -1)[p], clean[o].view(B, -1)[p]), (k, o, p)
            assert same(res[p], rc[p]) and bool(torch.isfinite(res[p]).all())
    # every bound infinite: nothing clips
    t = device_tensors(d)
    t["lo"].fill_(float("-inf"))
    t["hi"].fill_(float("inf"))
    res = run_update(solver, shape, t, False)
    torch.cuda.synchronize()
    inf = dict(d, lo=np.full_like(d["lo"], -np.inf), hi=np.full_like(d["hi"], np.inf))
    wr, _, gr, rr = ref.update_ref(dtype, nx, nu, mx, mu, N, inf["g"], inf["E"], inf["lo"], inf["hi"], inf["rho"], inf["z"], inf["w"], inf["y"])
    assert not bits(t["y"]).any(), "y+ must be +0 everywhere"
    # w+ = s = fl(E z + y) and the dual residual is that of w+ - w alone: what update_ref gives for these bounds
    assert np_same(host(t["w"], B), wr) and np_same(host(t["gt"], B), gr) and np_same(host(res, B), rr)

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(14, 7, 5, 3, 3, 2), (14, 7, NC + 1, 2, 4, 2)], ids=ids)
def test_footprint(solver, shape, dtype):
    d = lin_data(shape, dtype)
    GUARD = 1024
    results = []
    for fill in (float("nan"), 1e30):
        t = device_tensors(d, guard=GUARD)
        bufs = t["_bufs"]
        t["res"].fill_(fill)
        before = {k: b.clone() for k, b in bufs.items()}
        run_update(solver, shape, t, True)
        torch.cuda.synchronize()
        assert same(bufs["y"], before["y"]), "init wrote y"
        assert same(bufs["res"], before["res"]), "init wrote res"
        t["w"].copy_(dev(d["w"].reshape(-1)))
        run_update(solver, shape, t, False)
        run_form(solver, shape, t)
        torch.cuda.synchronize()
        for k, b in bufs.items():
            n = t[k].numel()
            assert same(b[:GUARD], before[k][:GUARD]) and same(b[GUARD + n:], before[k][GUARD + n:]), f"guard of {k}"
            assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + n:]).all())
        for k in ("z", "g", "E", "G", "lo", "hi", "rho"):
            assert same(bufs[k], before[k]), f"{k} was written"
        for k in ("w", "y", "gt", "res", "Gt"):
            assert bool(torch.isfinite(t[k]).all()), k
        results.append({k: t[k].clone() for k in ("w", "y", "gt", "res", "Gt")})
    for k in results[0]:
        assert same(results[0][k], results[1][k]), k     # nothing is read from res


# ---- 6. arguments
STEP_ARGS = ("Ginv", "C", "g", "c", "E", "lo", "hi", "rho", "S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z", "w",
             "y", "gt", "res")
OPTIONAL = ("Pinv", "r", "p", "fl")
WRITTEN = ("gamma", "lam", "r", "p", "z", "w", "y", "gt", "res", "Gt")


@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_refusals_write_nothing(solver, suf, tt):
    nx, nu, N, B, mx, mu = 6, 3, 4, 3, 2, 1
    lib, s = solver.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = torch.zeros(1 << 16, dtype=tt, device="cuda")
    rho = torch.ones(B, dtype=tt, device="cuda")
    outs = {k: torch.full((1 << 14,), 777.0, dtype=tt, device="cuda") for k in WRITTEN}
    it = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 777.0).all()) for t in outs.values()) and bool((it == 777).all()) and bool((fl == 77).all())

    def values(null=(), **over):
        v = {k: P(ins) for k in ("Ginv", "C", "g", "c", "E", "G", "lo", "hi", "S", "Pinv")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(it=P(it), fl=P(fl), tol=1e-6, max_iter=10, nx=nx, nu=nu, mx=mx, mu=mu, N=N, batch=B)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    def sizes(v):
        return (solver.h, v["nx"], v["nu"], v["mx"], v["mu"], v["N"], v["batch"])

    def step(name, v, graph=None):
        last = ctypes.byref(graph) if graph is not None else s
        return getattr(lib, f"gbdpcg_{name}_{suf}")(*sizes(v), *(v[k] for k in STEP_ARGS), last)

    def form(v):
        return getattr(lib, f"gbdpcg_admm_lin_form_{suf}")(*sizes(v), v["G"], v["E"], v["rho"], v["Gt"], s)

    def update(v, init=False):
        head = sizes(v) + (v["g"], v["E"], v["lo"], v["hi"], v["rho"])
        if init:
            return getattr(lib, f"gbdpcg_admm_lin_init_{suf}")(*head, v["w"], v["y"], v["gt"], s)
        return getattr(lib, f"gbdpcg_admm_lin_update_{suf}")(*head, v["z"], v["w"], v["y"], v["gt"], v["res"], s)

    graph = ctypes.c_void_p()
    steps = [("admm_lin_step", None), ("admm_lin_step_shared", None), ("graph_create_admm_lin_step", graph),
             ("graph_create_admm_lin_step_shared", graph)]
    calls = [("form", form), ("init", lambda v: update(v, True)), ("update", update)] + [(n, lambda v, n=n, g=g: step(n, v, g)) for n, g in steps]
    # each required pointer NULL: GBDPCG_ERR_INVALID
    for k in ("G", "E", "rho", "Gt"):
        assert form(values(null=(k,))) == 1, k
    for k in ("g", "E", "lo", "hi", "rho", "w", "y", "gt"):
        assert update(values(null=(k,)), init=True) == 1, k
    for k in ("g", "E", "lo", "hi", "rho", "z", "w", "y", "gt", "res"):
        assert update(values(null=(k,))) == 1, k
    for name, gr in steps:
        for k in STEP_ARGS:
            if k in OPTIONAL or k in ("tol", "max_iter"):
                continue
            assert step(name, values(null=(k,)), gr) == 1, (name, k)
        if gr is not None:
            assert getattr(lib, f"gbdpcg_{name}_{suf}")(*sizes(values()), *(values()[k] for k in STEP_ARGS), None) == 1
    for what, call in calls:
        for k in ("nx", "nu", "N", "batch"):                          # a zero size: INVALID
            assert call(values(**{k: 0})) == 1, (what, k)
        assert call(values(mx=0, mu=0)) == 1, what                    # no rows: INVALID
        assert call(values(mx=0, mu=2, N=1, null=("C",))) == 1, what  # only control rows and no control: INVALID
        assert call(values(mx=65)) == 4 and call(values(mu=65)) == 4, what     # above 64 rows per block: UNSUPPORTED
        assert call(values(mx=64, mu=64, nx=200, nu=100)) == 4, what  # a knot beyond the staging (the steps: beyond form_schur)
    big = dict(nx=80, nu=40) if suf == "f64" else dict(nx=120, nu=60)
    for name, gr in steps:                                            # what kkt_resolve refuses
        assert step(name, values(**big), gr) == 4, name
    assert not graph.value and untouched()
    # the limits themselves are taken
    assert form(values(mx=64, mu=64)) == 0 and update(values(mx=64, mu=64)) == 0 and update(values(mx=64, mu=64), init=True) == 0
    assert update(values(mx=0, mu=2)) == 0 and update(values(mx=2, mu=0, N=1)) == 0
    torch.cuda.synchronize()


# ---- 7. convergence on the problems tests/test_admm_lin_reference.py pins
@pytest.mark.parametrize("dtype", DTYPES)
def test_eighty_replays_converge_like_the_reference(solver, dtype):
    nx, nu, N, B = ref.CONV_SHAPE
    mx, mu = ref.CONV_ROWS
    rho = np.array(ref.CONV_RHO)
    d, E, lo, hi, _ = ref.convergence_inputs()
    history = ref.convergence_reference(4000)
    K = 80
    L = LinLoop(solver, (nx, nu, N, B, mx, mu), dtype, d, E, rho, lo=lo, hi=hi, tol=PCG_TOL[dtype], max_iter=200)
    assert same(L.gt, L.g)      # w = y = 0 lies between the bounds: the first solve is the equality-constrained one
    o = L.state()
    solver.reserve(L.g.element_size(), nx, N, B)
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
    w = host(o["w"], B)
    assert int(flags.sum()) == 0, "(d) a solve ran out of iterations"
    assert ((w >= lo.astype(dtype)) & (w <= hi.astype(dtype))).all(), "(d) w outside the bounds"
    worst = 0.0
    for b in range(B):
        wstar, wref = history[b]["w"][-1], history[b]["w"][K - 1]
        dist, bound = np.abs(w[b].astype(F64) - wstar).max(), 2 * np.abs(wref - wstar).max() + K * STEP_TOL[dtype] * np.abs(wstar).max()
        close = np.abs(w[b].astype(F64) - wref).max()
        worst = max(worst, close)
        ratio = res80[b] / res1[b]
        print(f"{what} problem {b}: ||w(80) - w*||_inf {dist:.3e} (bound {bound:.3e})  ||w(80) - w_ref(80)||_inf {close:.3e}  "
              f"res(80)/res(1) {ratio[0]:.3e} {ratio[1]:.3e} (reference {history[b]['r_prim'][K - 1] / history[b]['r_prim'][0]:.3e} "
              f"{history[b]['r_dual'][K - 1] / history[b]['r_dual'][0]:.3e})  res(80) {res80[b, 0]:.3e} {res80[b, 1]:.3e} "
              f"(reference {history[b]['r_prim'][K - 1]:.3e} {history[b]['r_dual'][K - 1]:.3e})")
        assert dist <= bound, (b, dist, bound)                              # (a)
        assert res80[b, 0] <= 1e-2 * res1[b, 0], (b, ratio)                 # (c)
        assert (res80[b] < res1[b]).all(), (b, res1[b], res80[b])           # (c)
    print(f"{what}: worst ||w(80) - w_ref(80)||_inf {worst:.3e} (bound {CLOSE[dtype]})")
    assert worst <= CLOSE[dtype], worst        # (b)
