"""The optimality test of the ADMM families on the device (csrc/admm_optimality.hip through the C ABI): gbdpcg_admm_optimality_*,
gbdpcg_admm_lin_optimality_* and their _shared twins.
PARITY UNPINNED: the reference tree has no code, fixture or output for this launch.

Reference: tests/admm_optimality_ref.py.  Every output is defined to the bit, so d_opt and d_done are compared for EQUALITY with
opt_ref in the call's precision, with the bases 16-byte aligned and off by one element; the box form with the rows form at E = I,
the shared twins with the per-problem calls on tiled copies, r_s and r_e at y = 0 with Solver.kkt_residual, r_r behind the update of
every family with its d_res[2b], a caller-owned capture of step -> optimality with the calls it is made of.  End to end the device's
first d_done on the pinned feasible fixtures falls inside the window [K_LO, K_HI] of the fp64 reference loop.  Run with -s for the
figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_lin_ref as lr  # noqa: E402
import admm_optimality_ref as orf  # noqa: E402
import admm_ref  # noqa: E402
import admm_soc_ref as soc  # noqa: E402
import test_gpu_admm as hard  # noqa: E402
import test_gpu_admm_lin as lin  # noqa: E402
from admm_util import dev, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
SETUP_TOL = {F32: 1e-10, F64: 1e-22}   # the cold solve behind the factorisation (tests/test_gpu_admm.py): it has to converge
# The replays' PCG exit test is |eta| < tol with eta = r' Phi^-1 r, the SQUARE of a residual norm.  "At least 1e3 below eps" is
# therefore tol <= (1e-3 EPS)^2 = 1e-18: at 1e-10 the solve leaves a residual of 1e-5, ten times EPS, and the fp32 loops arrive
# 1 to 13 iterations late (measured: box 79, 125, 175, rows 113, 119, 252; at 1e-18 box 77, 121, 165, rows 92, 104, 237).
PCG_TOL = {F32: 1e-18, F64: 1e-22}
NC, NCB = orf.knot_chunk(14, 7, 4, 2), orf.knot_chunk(14, 7, 0, 0, box=True)
ROWS = [(2, 1, 1, 1, 1, 0),           # N = 1: no C, no u; one state row
        (2, 1, 2, 3, 0, 1),           # one input row, no state rows
        (3, 2, 5, 5, 4, 2),
        (3, 2, 3, 3, 64, 3),          # the most rows a block may have
        (14, 7, 3, 3, 4, 2),          # the workload's block size
        (14, 7, NC + 1, 1, 4, 2)]     # one knot past a chunk: two chunks, the last one partial
BOX = [(2, 1, 1, 1), (2, 1, 2, 3), (3, 2, 5, 5), (14, 7, 3, 3), (14, 7, NCB + 1, 1)]
OFFSETS = [0, 1]                      # 16-byte aligned bases / every base off by one element
EPS_BITS = 1.0                        # random data of order 1: flags of both values (test_reference_flags_both_ways)
INPUTS = ("G", "C", "g", "c", "E", "rho", "z", "lam", "w", "y")


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def data(nx, nu, N, B, mx, mu, dtype, box=False):
    d = orf.random_inputs(nx, nu, mx, mu, N, B, 5000 + 31 * nx + 7 * N + mx + (100 if box else 0), dtype, box=box)
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, mx, mu, dtype, box=False):
    d = data(nx, nu, N, B, mx, mu, dtype, box)
    return orf.opt_ref(dtype, nx, nu, mx, mu, N, *[d[k] for k in INPUTS], EPS_BITS, EPS_BITS)


def device_tensors(d, offset=0, guard=8):
    """The arrays of data() on the device, flat, plus opt (NaN) and done (7): every array starts `offset` elements into a buffer of
    its own whose base the allocator aligns, with `guard` elements of NaN (7) on either side.  Returns (views, buffers)."""
    B = d["rho"].size
    t, bufs = {}, {}
    items = [(k, d[k]) for k in INPUTS if d[k] is not None] + [("opt", np.full((B, 6), np.nan, d["c"].dtype)), ("done", np.full(B, 7, np.uint8))]
    for k, a in items:
        flat = dev(a.reshape(-1))
        fill = 7 if k == "done" else float("nan")
        buf = torch.full((flat.numel() + 2 * guard + 1,), fill, dtype=flat.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[guard + offset:guard + offset + flat.numel()] = flat
        t[k], bufs[k] = buf[guard + offset:guard + offset + flat.numel()], buf
    if d["E"] is None:
        t["E"] = None
    if t["C"].numel() == 0:
        t["C"] = None
    return t, bufs


def call(solver, shape, t, box=False, shared=False, done=True, eps=EPS_BITS):
    nx, nu, N, B, mx, mu = shape
    vec = (t["rho"], t["z"], t["lam"], t["w"], t["y"], eps, eps)
    kw = dict(opt=t["opt"], done=t["done"] if done else None, want_done=done)
    if box:
        (solver.admm_optimality_shared if shared else solver.admm_optimality)(nx, nu, N, B, t["G"], t["C"], t["g"], t["c"], *vec, **kw)
    else:
        (solver.admm_lin_optimality_shared if shared else solver.admm_lin_optimality)(nx, nu, mx, mu, N, B, t["G"], t["C"], t["g"], t["c"],
                                                                                      t["E"], *vec, **kw)
    torch.cuda.synchronize()


def guards_intact(t, bufs, guard=8):
    for k, buf in bufs.items():
        view = t[k] if t[k] is not None else buf[guard:guard]
        start = (view.data_ptr() - buf.data_ptr()) // buf.element_size() if view.numel() else guard
        head, tail = buf[:start], buf[start + view.numel():]
        ok = (lambda x: bool((x == 7).all())) if k == "done" else (lambda x: bool(torch.isnan(x).all()))
        if not (ok(head) and ok(tail)):
            return k
    return None


def check_bits(solver, shape, dtype, box):
    nx, nu, N, B, mx, mu = shape
    d = data(*shape, dtype, box)
    orr, dr = reference(*shape, dtype, box)
    for offset in OFFSETS:
        t, bufs = device_tensors(d, offset)
        call(solver, shape, t, box)
        opt, done = t["opt"].cpu().numpy().reshape(B, 6), t["done"].cpu().numpy()
        what = f"{shape} {np.dtype(dtype).name} box={box} offset {offset}"
        assert np_same(opt, orr), (what, opt, orr)
        assert np_same(done, dr), (what, done, dr)
        assert guards_intact(t, bufs) is None, what
        for k in INPUTS:                                   # inputs unchanged
            if d[k] is not None and d[k].size:
                assert np_same(t[k].cpu().numpy(), d[k].reshape(-1)), (what, k)
        # d_done = NULL: the same opt, and nothing else written
        t2, bufs2 = device_tensors(d, offset)
        call(solver, shape, t2, box, done=False)
        assert same(t2["opt"], t["opt"]) and bool((bufs2["done"] == 7).all()) and guards_intact(t2, bufs2) is None, what


# ---- 1. bits against the exact reference, both alignments; footprint; d_done = NULL
def test_reference_flags_both_ways():
    """(no device) the cases below give set and clear flags, so the three comparisons are exercised"""
    flags = np.concatenate([reference(*s, dt)[1] for s in ROWS for dt in DTYPES] +
                           [reference(nx, nu, N, B, 0, 0, dt, True)[1] for nx, nu, N, B in BOX for dt in DTYPES])
    assert flags.min() == 0 and flags.max() == 1 and 4 <= flags.sum() <= flags.size - 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", ROWS)
def test_rows_bits_footprint_and_null_done(solver, nx, nu, N, B, mx, mu, dtype):
    check_bits(solver, (nx, nu, N, B, mx, mu), dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", BOX)
def test_box_bits_and_box_is_rows_at_identity(solver, nx, nu, N, B, dtype):
    shape = (nx, nu, N, B, 0, 0)
    check_bits(solver, shape, dtype, True)
    d = dict(data(*shape, dtype, True))
    t, _ = device_tensors(d)
    call(solver, shape, t, True)
    d["E"] = orf.box_as_rows(nx, nu, N, B, dtype)
    tr, _ = device_tensors(d)
    call(solver, (nx, nu, N, B, nx, nu), tr, False)
    assert same(t["opt"], tr["opt"]) and same(t["done"], tr["done"])


# ---- 2. the shared twins against the per-problem calls on tiled copies
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", [(3, 2, 5, 5, 4, 2, False), (14, 7, NC + 1, 3, 4, 2, False), (2, 1, 1, 3, 1, 0, False),
                                                  (3, 2, 5, 5, 0, 0, True), (14, 7, 3, 3, 0, 0, True)])
def test_shared_twins(solver, nx, nu, N, B, mx, mu, box, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = dict(data(*shape, dtype, box))
    for k in ("G", "C", "E"):
        if d[k] is not None:
            d[k] = np.tile(d[k][1 % B:1 % B + 1], (B, 1))       # problem 1's matrices for everyone
    t, _ = device_tensors(d)
    call(solver, shape, t, box)
    one = dict(d)
    for k in ("G", "C", "E"):
        if d[k] is not None:
            one[k] = d[k][:1]
    ts, bufs = device_tensors(one)
    call(solver, shape, ts, box, shared=True)
    assert same(t["opt"], ts["opt"]) and same(t["done"], ts["done"]) and guards_intact(ts, bufs) is None


# ---- 3. with y = 0, r_s and r_e are Solver.kkt_residual
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", [(3, 2, 5, 5, 4, 2, False), (14, 7, NC + 1, 1, 4, 2, False), (14, 7, 3, 3, 0, 0, True),
                                                  (2, 1, 2, 3, 0, 0, True)])
def test_y_zero_gives_the_bits_of_kkt_residual(solver, nx, nu, N, B, mx, mu, box, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = dict(data(*shape, dtype, box))
    d["y"] = (np.where(np.arange(d["y"].shape[1]) % 2 == 0, 0.0, -0.0) * np.ones_like(d["y"])).astype(dtype)
    t, _ = device_tensors(d)
    call(solver, shape, t, box)
    res = solver.kkt_residual(nx, nu, N, B, t["G"].clone(), None if t["C"] is None else t["C"].clone(), t["g"].clone(), t["c"].clone(),
                              t["z"].clone(), t["lam"].clone())
    torch.cuda.synchronize()
    assert same(t["opt"].view(B, 6)[:, :2].contiguous(), res.contiguous())


# ---- 4. behind the update of every family, r_r is its d_res[2b]
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["box", "soft_box", "lin", "lin_soft", "soc"])
def test_behind_an_update_rr_is_res_primal(solver, family, dtype):
    nx, nu, N, B = 14, 7, NC + 1, 3
    box = "box" in family
    mx, mu = (0, 0) if box else ((5, 4) if family == "soc" else (4, 2))
    shape = (nx, nu, N, B, mx, mu)
    d = data(*shape, dtype, box)
    rng = np.random.default_rng(78)
    nw = d["w"].shape[1]
    lo = (-np.abs(rng.standard_normal((B, nw))) * 0.3).astype(F32).astype(dtype)
    hi = (np.abs(rng.standard_normal((B, nw))) * 0.3).astype(F32).astype(dtype)
    kappa = np.abs(rng.standard_normal((B, nw))).astype(F32).astype(dtype)
    kappa[:, ::3] = np.inf
    cones = soc.CONV_CONES
    if family == "soc":
        head, _ = soc.layout(nx, nu, mx, mu, cones, N)
        lo = np.where(head >= 0, 0.0, lo).astype(dtype)        # zero offsets f on the cone rows: the call knows of no offset
    t, _ = device_tensors(d)
    lo, hi, kappa = (dev(a.reshape(-1)) for a in (lo, hi, kappa))
    gt, res = torch.empty_like(t["g"]), torch.full((B, 2), float("nan"), dtype=t["g"].dtype, device="cuda")
    w, y = t["w"].clone(), t["y"].clone()
    if family == "box":
        solver.admm_update(nx, nu, N, B, t["g"], lo, hi, t["rho"], t["z"], w, y, gt, res=res)
    elif family == "soft_box":
        solver.admm_soft_update(nx, nu, N, B, t["g"], lo, hi, kappa, t["rho"], t["z"], w, y, gt, res=res)
    elif family == "lin":
        solver.admm_lin_update(nx, nu, mx, mu, N, B, t["g"], t["E"], lo, hi, t["rho"], t["z"], w, y, gt, res=res)
    elif family == "lin_soft":
        solver.admm_lin_soft_update(nx, nu, mx, mu, N, B, t["g"], t["E"], lo, hi, kappa, t["rho"], t["z"], w, y, gt, res=res)
    else:
        solver.admm_soc_update(nx, nu, mx, mu, cones, N, B, t["g"], t["E"], lo, hi, t["rho"], t["z"], w, y, gt, res=res)
    after = dict(t, w=w, y=y)
    call(solver, shape, after, box)
    opt = t["opt"].view(B, 6)
    assert same(opt[:, 2].contiguous(), res[:, 0].contiguous()), (opt[:, 2], res[:, 0])
    assert bool((opt[:, 2] > 0).all())


# ---- 5. a NaN stays inside its problem
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", [(3, 2, 5, 5, 4, 2, False), (3, 2, 5, 5, 0, 0, True)])
def test_nan_stays_in_its_problem(solver, nx, nu, N, B, mx, mu, box, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = data(*shape, dtype, box)
    orr, dr = reference(*shape, dtype, box)
    keep = [b for b in range(B) if b != 1]
    for key in ("z", "lam", "w", "y", "c", "rho", "G"):
        bad = {k: (None if v is None else v.copy()) for k, v in d.items()}
        if key == "rho":
            bad[key][1] = np.nan
        else:
            bad[key][1, 2] = np.nan
        t, _ = device_tensors(bad)
        call(solver, shape, t, box, eps=1e30)
        opt, done = t["opt"].cpu().numpy().reshape(B, 6), t["done"].cpu().numpy()
        assert np.isnan(opt[1]).any() and done[1] == 0, key
        assert np_same(opt[keep], orr[keep]) and bool((done[keep] == 1).all()), key


# ---- 6. every refusal, with nothing written
@pytest.mark.parametrize("suf,dtype", [("f32", F32), ("f64", F64)])
def test_refusals_write_nothing(solver, suf, dtype):
    shape = nx, nu, N, B, mx, mu = 3, 2, 5, 5, 4, 2
    t, bufs = device_tensors(data(*shape, dtype))
    before = {k: b.clone() for k, b in bufs.items()}
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ft = ctypes.c_float if suf == "f32" else ctypes.c_double
    p = {k: (None if v is None else ctypes.c_void_p(v.data_ptr())) for k, v in t.items()}
    INVALID, UNSUPPORTED = 1, 4

    def run(name, h=solver.h, null=(), **over):
        v = dict(nx=nx, nu=nu, mx=mx, mu=mu, N=N, batch=B, **p)
        v.update(over)
        for k in null:
            v[k] = None
        box = "lin" not in name
        head = [h, v["nx"], v["nu"]] + ([] if box else [v["mx"], v["mu"]]) + [v["N"], v["batch"], v["G"], v["C"], v["g"], v["c"]]
        return getattr(solver.lib, f"gbdpcg_{name}_{suf}")(*head, *([] if box else [v["E"]]), v["rho"], v["z"], v["lam"], v["w"], v["y"],
                                                           ft(0.1), ft(0.1), v["opt"], v["done"], s)

    for name in ("admm_optimality", "admm_optimality_shared", "admm_lin_optimality", "admm_lin_optimality_shared"):
        rows = "lin" in name
        assert run(name, h=None) == INVALID, name
        for k in ("G", "C", "g", "c", "rho", "z", "lam", "w", "y", "opt") + (("E",) if rows else ()):
            assert run(name, null=(k,)) == INVALID, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert run(name, **{k: 0}) == INVALID, (name, k)
        if rows:
            assert run(name, mx=0, mu=0) == INVALID and run(name, mx=0, N=1) == INVALID, name      # no rows at all
            assert run(name, mx=65) == UNSUPPORTED and run(name, mu=65) == UNSUPPORTED, name
            assert run(name, mx=0, mu=0, nx=200) == INVALID, name                                   # INVALID before UNSUPPORTED
        assert run(name, nx=200, nu=100) == UNSUPPORTED, name                                       # a knot that does not fit the LDS
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert same(b, before[k]), k
    # C may be NULL when N == 1
    shape1 = (2, 1, 1, 1, 1, 0)
    t1, _ = device_tensors(data(*shape1, dtype))
    assert t1["C"] is None
    call(solver, shape1, t1)
    assert np_same(t1["opt"].cpu().numpy().reshape(1, 6), reference(*shape1, dtype)[0])


# ---- 7. the loops: a captured step -> optimality, the pinned windows, lambda zeroed
def box_loop(solver, dtype):
    nx, nu, N, B = admm_ref.CONV_SHAPE
    d, lo, hi, _ = admm_ref.convergence_inputs()
    L = hard.Loop(solver, nx, nu, N, B, dtype, d, np.array(admm_ref.CONV_RHO), lo=lo, hi=hi, tol=SETUP_TOL[dtype], max_iter=200)
    L.tol = PCG_TOL[dtype]            # the warm-started solves of the iteration
    return L


def rows_loop(solver, dtype):
    nx, nu, N, B = admm_ref.CONV_SHAPE
    d, E, lo, hi, _ = lr.convergence_inputs()
    L = lin.LinLoop(solver, (nx, nu, N, B, *lr.CONV_ROWS), dtype, d, E, np.array(lr.CONV_RHO), lo=lo, hi=hi, tol=SETUP_TOL[dtype],
                    max_iter=200)
    L.tol = PCG_TOL[dtype]
    return L


def outputs(L):
    B = L.shape[3]
    return dict(opt=torch.full((B, 6), float("nan"), dtype=L.g.dtype, device="cuda"), done=torch.full((B,), 7, dtype=torch.uint8, device="cuda"))


def optimality(L, o, a, eps=orf.EPS):
    if len(L.shape) == 4:
        nx, nu, N, B = L.shape
        L.s.admm_optimality(nx, nu, N, B, L.G, L.C, L.g, L.c, L.rho, o["z"], o["lam"], o["w"], o["y"], eps, eps, opt=a["opt"], done=a["done"])
    else:
        nx, nu, N, B, mx, mu = L.shape
        L.s.admm_lin_optimality(nx, nu, mx, mu, N, B, L.G, L.C, L.g, L.c, L.E, L.rho, o["z"], o["lam"], o["w"], o["y"], eps, eps,
                                opt=a["opt"], done=a["done"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_captured_step_optimality_replays_the_bits_of_the_calls(solver, dtype):
    L = box_loop(solver, dtype)
    oa, ob = L.state(), L.state()
    aa, ab = outputs(L), outputs(L)
    for _ in range(3):
        hard.one_call(L, oa)
        optimality(L, oa, aa)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):     # the capturing stream is torch's current one inside the block
        hard.one_call(L, ob)
        optimality(L, ob, ab)
    for k, v in L.start.items():      # the capture ran nothing: start again from the saved state, outputs poisoned
        ob[k].copy_(v)
    ab["opt"].fill_(float("nan"))
    ab["done"].fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("lam", "z", "w", "y", "gt", "res"):
        assert same(oa[k], ob[k]), k
    for k in ("opt", "done"):
        assert same(aa[k], ab[k]), k
    assert not bool(torch.isnan(aa["opt"]).any()) and int(aa["done"].max()) <= 1


_RUNS = {}


def converged_run(solver, kind, dtype):
    """The step graph replayed max(K_HI) + 3 times with the optimality launch behind every replay, once per (kind, dtype):
    (L, o, a, done [K, B], opt [K, B, 6] as fp64)."""
    key = (kind, np.dtype(dtype).name)
    if key not in _RUNS:
        L = box_loop(solver, dtype) if kind == "box" else rows_loop(solver, dtype)
        first = 0 if kind == "box" else 3
        B = L.shape[3]
        o, a = L.state(), outputs(L)
        if kind == "box":
            nx, nu, N, _ = L.shape
            gr = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"], o["r"],
                                        o["p"], L.tol, L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
        else:
            gr = L.graph(o)
        K = max(orf.K_HI[first:first + B]) + 3
        dones, opts = torch.empty((K, B), dtype=torch.uint8, device="cuda"), torch.empty((K, B, 6), dtype=L.g.dtype, device="cuda")
        for k in range(K):
            gr.launch()
            optimality(L, o, a)
            dones[k].copy_(a["done"])
            opts[k].copy_(a["opt"])
        torch.cuda.synchronize()
        gr.close()
        _RUNS[key] = (L, o, a, dones.cpu().numpy(), opts.cpu().numpy().astype(F64))
    return _RUNS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["box", "rows"])
def test_first_done_falls_in_the_pinned_window(solver, kind, dtype):
    """The fixtures of admm_infeas_ref.feasible_problems(): problems 0 .. 2 (the box of admm_ref) and 3 .. 5 (the rows of
    admm_lin_ref).  The PCG exit tolerance of the replays is (1e-3 EPS)^2 on eta = r' Phi^-1 r (PCG_TOL above) at EPS = 1e-6.
    Measured on the MI355X: fp32 first done at 77, 121, 165 (box) and 92, 104, 237 (rows), fp64 at 78, 121, 164 and 93, 103, 240,
    against the windows [72, 84], [112, 130], [154, 174] and [86, 100], [96, 110], [224, 257]; the fp32 solves take 17 to 26 PCG
    iterations per replay at that tolerance."""
    assert max(PCG_TOL.values()) <= 1.0001 * (1e-3 * orf.EPS) ** 2       # eta is a squared norm
    L, o, a, dones, opts = converged_run(solver, kind, dtype)
    first = 0 if kind == "box" else 3
    B, K = L.shape[3], dones.shape[0]
    k_lo, k_hi = orf.K_LO[first:first + B], orf.K_HI[first:first + B]
    at = [orf.first_done(dones[:, b]) for b in range(B)]
    for b in range(B):
        i = (at[b] or K) - 1
        print(f"{kind} {np.dtype(dtype).name} problem {b}: first done at {at[b]} (window [{k_lo[b]}, {k_hi[b]}]); there r / threshold = "
              f"{(opts[i, b, :3] / (orf.EPS + orf.EPS * opts[i, b, 3:])).round(3)}; at {K}: {(opts[-1, b, :3] / (orf.EPS + orf.EPS * opts[-1, b, 3:])).round(3)}")
    for b in range(B):
        assert at[b] is not None and k_lo[b] <= at[b] <= k_hi[b], (b, at[b], k_lo[b], k_hi[b])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["box", "rows"])
def test_zeroing_lambda_clears_done_and_the_bits_hold(solver, kind, dtype):
    """Behind the run above the point passes at eps = 1e-3; with lambda zeroed it cannot: stationarity fails, the six numbers are
    the exact reference's, d_res has not moved."""
    L, o, a, _, _ = converged_run(solver, kind, dtype)
    B = L.shape[3]
    lam = o["lam"].clone()
    optimality(L, o, a, eps=1e-3)
    torch.cuda.synchronize()
    assert int(a["done"].min()) == 1
    res = o["res"].clone()
    o["lam"].zero_()
    optimality(L, o, a, eps=1e-3)
    torch.cuda.synchronize()
    assert int(a["done"].max()) == 0 and same(o["res"], res)
    # (problem 0 alone: the exact reference of a whole (14, 7, 24) batch would take several seconds)
    h = {k: v.cpu().numpy().reshape(B, -1)[:1] for k, v in dict(G=L.G, C=L.C, g=L.g, c=L.c, z=o["z"], lam=o["lam"], w=o["w"], y=o["y"]).items()}
    mx, mu = (0, 0) if kind == "box" else L.shape[4:]
    E = None if kind == "box" else L.E.cpu().numpy().reshape(B, -1)[:1]
    ref, rdone = orf.opt_ref(dtype, L.shape[0], L.shape[1], mx, mu, L.shape[2], h["G"], h["C"], h["g"], h["c"], E,
                             L.rho.cpu().numpy()[:1], h["z"], h["lam"], h["w"], h["y"], 1e-3, 1e-3)
    assert np_same(a["opt"].cpu().numpy()[:1], ref) and np_same(a["done"].cpu().numpy()[:1], rdone)
    o["lam"].copy_(lam)
