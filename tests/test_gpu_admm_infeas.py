"""The primal infeasibility certificate of the hard ADMM paths on the device (csrc/admm_infeas.hip through the C ABI):
gbdpcg_admm_infeas_*, gbdpcg_admm_lin_infeas_* and their _shared twins.
PARITY UNPINNED: the reference tree has no code, fixture or output for this launch.

Reference: tests/admm_infeas_ref.py.  Every output is defined to the bit, so d_cert and d_flag are compared for EQUALITY with
cert_ref in the call's precision, with the bases 16-byte aligned and off by one element; the box form with the rows form at E = I,
the shared twins with the per-problem calls on tiled copies, a caller-owned capture of copy -> step -> certificate with the calls it
is made of.  End to end the device flags every problem of admm_soft_ref.infeasible_inputs() at the iteration the reference of the
same precision pinned and never flags the feasible fixtures.  Run with -s for the figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_infeas_ref as ir  # noqa: E402
import admm_lin_ref as lr  # noqa: E402
import admm_ref  # noqa: E402
import admm_soft_ref as sr  # noqa: E402
import test_gpu_admm as hard  # noqa: E402
import test_gpu_admm_lin as lin  # noqa: E402
from admm_util import dev, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
PCG_TOL = {F32: 1e-10, F64: 1e-22}     # tests/test_gpu_admm.py
NC = ir.knot_chunk(14, 7, 4, 2)
ROWS = [(2, 1, 3, 2, 1, 1),           # smallest
        (3, 2, 5, 6, 2, 1),
        (3, 2, 4, 3, 0, 2),           # no state rows
        (3, 2, 4, 3, 2, 0),           # no input rows
        (14, 7, 3, 2, 4, 2),          # the workload's block size
        (3, 2, 1, 2, 2, 0),           # N = 1: no C, no u
        (14, 7, NC + 1, 2, 4, 2)]     # one knot past a chunk
BOX = [(3, 2, 4, 3), (14, 7, 3, 2), (3, 2, 1, 2), (14, 7, ir.knot_chunk(14, 7, 0, 0, box=True) + 1, 2)]
OFFSETS = [0, 1]                      # 16-byte aligned bases / every base off by one element
EPS_BITS = 4.0                        # with the planted bounds of data(): flags of both values (test_reference_flags_both_ways)
INPUTS = ("C", "c", "E", "lo", "hi", "rho", "lam0", "lam1", "y0", "y1")


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def data(nx, nu, N, B, mx, mu, dtype, box=False):
    """ir.random_inputs, with bounds planted in problem 0 that make its support value very negative (lo, hi are not validated).
    Read-only."""
    d = ir.random_inputs(nx, nu, mx, mu, N, B, 4000 + 31 * nx + 7 * N + mx + (100 if box else 0), dtype, box=box)
    dy = d["y1"][0] - d["y0"][0]
    d["hi"][0] = np.where(dy > 0, -100.0, d["hi"][0])
    d["lo"][0] = np.where(dy < 0, 100.0, d["lo"][0])
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, mx, mu, dtype, box=False):
    d = data(nx, nu, N, B, mx, mu, dtype, box)
    return ir.cert_ref(dtype, nx, nu, mx, mu, N, d["C"], d["c"], d["E"], d["lo"], d["hi"], d["rho"], d["lam0"], d["lam1"], d["y0"],
                       d["y1"], EPS_BITS)


def device_tensors(d, offset=0, guard=8):
    """The arrays of data() on the device, flat, plus cert (NaN) and flag (7): every array starts `offset` elements into a buffer of
    its own whose base the allocator aligns, with `guard` elements of NaN (7) on either side.  Returns (views, buffers)."""
    B = d["rho"].size
    t, bufs = {}, {}
    items = [(k, d[k]) for k in INPUTS if d[k] is not None] + [("cert", np.full((B, 3), np.nan, d["c"].dtype)), ("flag", np.full(B, 7, np.uint8))]
    for k, a in items:
        flat = dev(a.reshape(-1))
        fill = 7 if k == "flag" else float("nan")
        buf = torch.full((flat.numel() + 2 * guard + 1,), fill, dtype=flat.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[guard + offset:guard + offset + flat.numel()] = flat
        t[k], bufs[k] = buf[guard + offset:guard + offset + flat.numel()], buf
    if d["E"] is None:
        t["E"] = None
    if t["C"].numel() == 0:
        t["C"] = None
    return t, bufs


def call(solver, shape, t, box=False, shared=False, flag=True, eps=EPS_BITS):
    nx, nu, N, B, mx, mu = shape
    vec = (t["lo"], t["hi"], t["rho"], t["lam0"], t["lam1"], t["y0"], t["y1"], eps)
    kw = dict(cert=t["cert"], flag=t["flag"] if flag else None, want_flag=flag)
    if box:
        (solver.admm_infeas_shared if shared else solver.admm_infeas)(nx, nu, N, B, t["C"], t["c"], *vec, **kw)
    else:
        (solver.admm_lin_infeas_shared if shared else solver.admm_lin_infeas)(nx, nu, mx, mu, N, B, t["C"], t["c"], t["E"], *vec, **kw)
    torch.cuda.synchronize()


def guards_intact(t, bufs, guard=8):
    for k, buf in bufs.items():
        view = t[k] if t[k] is not None else buf[guard:guard]
        start = (view.data_ptr() - buf.data_ptr()) // buf.element_size() if view.numel() else guard
        head, tail = buf[:start], buf[start + view.numel():]
        ok = (lambda x: bool((x == 7).all())) if k == "flag" else (lambda x: bool(torch.isnan(x).all()))
        if not (ok(head) and ok(tail)):
            return k
    return None


def check_bits(solver, shape, dtype, box):
    nx, nu, N, B, mx, mu = shape
    d = data(*shape, dtype, box)
    cr, fr = reference(*shape, dtype, box)
    for offset in OFFSETS:
        t, bufs = device_tensors(d, offset)
        call(solver, shape, t, box)
        cert, flag = t["cert"].cpu().numpy().reshape(B, 3), t["flag"].cpu().numpy()
        what = f"{shape} {np.dtype(dtype).name} box={box} offset {offset}"
        assert np_same(cert, cr), (what, cert, cr)
        assert np_same(flag, fr), (what, flag, fr)
        assert guards_intact(t, bufs) is None, what
        for k in INPUTS:                                   # inputs unchanged
            if d[k] is not None and d[k].size:
                assert np_same(t[k].cpu().numpy(), d[k].reshape(-1)), (what, k)
        # d_flag = NULL: the same cert, and nothing else written
        t2, bufs2 = device_tensors(d, offset)
        call(solver, shape, t2, box, flag=False)
        assert same(t2["cert"], t["cert"]) and bool((bufs2["flag"] == 7).all()) and guards_intact(t2, bufs2) is None, what
    return cr, fr


# ---- 1. bits against the exact reference, both alignments; footprint; d_flag = NULL
def test_reference_flags_both_ways():
    """(no device) the planted bounds give set and clear flags in the cases below, so the flag's three comparisons are exercised"""
    flags = np.concatenate([reference(*s, dt)[1] for s in ROWS for dt in DTYPES] +
                           [reference(nx, nu, N, B, 0, 0, dt, True)[1] for nx, nu, N, B in BOX for dt in DTYPES])
    assert flags.min() == 0 and flags.max() == 1 and 4 <= flags.sum() <= flags.size - 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu", ROWS)
def test_rows_bits_footprint_and_null_flag(solver, nx, nu, N, B, mx, mu, dtype):
    check_bits(solver, (nx, nu, N, B, mx, mu), dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", BOX)
def test_box_bits_and_box_is_rows_at_identity(solver, nx, nu, N, B, dtype):
    shape = (nx, nu, N, B, 0, 0)
    check_bits(solver, shape, dtype, True)
    d = dict(data(*shape, dtype, True))
    t, _ = device_tensors(d)
    call(solver, shape, t, True)
    d["E"] = ir.box_as_rows(nx, nu, N, B, dtype)
    tr, _ = device_tensors(d)
    call(solver, (nx, nu, N, B, nx, nu), tr, False)
    assert same(t["cert"], tr["cert"]) and same(t["flag"], tr["flag"])


# ---- 2. the shared twins against the per-problem calls on tiled copies
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", [(3, 2, 5, 6, 2, 1, False), (14, 7, NC + 1, 2, 4, 2, False), (3, 2, 1, 2, 2, 0, False),
                                                  (3, 2, 4, 3, 0, 0, True), (14, 7, 3, 2, 0, 0, True)])
def test_shared_twins(solver, nx, nu, N, B, mx, mu, box, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = dict(data(*shape, dtype, box))
    for k in ("C", "E"):
        if d[k] is not None:
            d[k] = np.tile(d[k][1 % B:1 % B + 1], (B, 1))       # problem 1's matrices for everyone
    t, _ = device_tensors(d)
    call(solver, shape, t, box)
    one = dict(d)
    for k in ("C", "E"):
        if d[k] is not None:
            one[k] = d[k][:1]
    ts, bufs = device_tensors(one)
    call(solver, shape, ts, box, shared=True)
    assert same(t["cert"], ts["cert"]) and same(t["flag"], ts["flag"]) and guards_intact(ts, bufs) is None


# ---- 3. a NaN or an infinite bound stays inside its problem
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", [(3, 2, 5, 6, 2, 1, False), (3, 2, 4, 3, 0, 0, True)])
def test_nan_and_infinite_bounds_stay_in_their_problem(solver, nx, nu, N, B, mx, mu, box, dtype):
    shape = (nx, nu, N, B, mx, mu)
    d = data(*shape, dtype, box)
    cr, fr = reference(*shape, dtype, box)
    bad = {k: (None if v is None else v.copy()) for k, v in d.items()}
    bad["y1"][1, 2] = np.nan
    bad["lam0"][1, 0] = np.inf
    bad["hi"][1, :] = np.inf
    bad["rho"][1] = np.nan
    bad["y1"][1, 0] = bad["y0"][1, 0]              # dy = 0 under an infinite bound
    t, _ = device_tensors(bad)
    call(solver, shape, t, box)
    cert, flag = t["cert"].cpu().numpy().reshape(B, 3), t["flag"].cpu().numpy()
    assert np.isnan(cert[1, 0]) and np.isnan(cert[1, 1]) and flag[1] == 0
    keep = [b for b in range(B) if b != 1]
    assert np_same(cert[keep], cr[keep]) and np_same(flag[keep], fr[keep])


# ---- 4. every refusal, with nothing written
@pytest.mark.parametrize("suf,dtype", [("f32", F32), ("f64", F64)])
def test_refusals_write_nothing(solver, suf, dtype):
    shape = nx, nu, N, B, mx, mu = 3, 2, 4, 3, 2, 1
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
        head = [h, v["nx"], v["nu"]] + ([] if box else [v["mx"], v["mu"]]) + [v["N"], v["batch"], v["C"], v["c"]] + ([] if box else [v["E"]])
        return getattr(solver.lib, f"gbdpcg_{name}_{suf}")(*head, v["lo"], v["hi"], v["rho"], v["lam0"], v["lam1"], v["y0"], v["y1"],
                                                           ft(0.1), v["cert"], v["flag"], s)

    for name in ("admm_infeas", "admm_infeas_shared", "admm_lin_infeas", "admm_lin_infeas_shared"):
        rows = "lin" in name
        assert run(name, h=None) == INVALID, name
        for k in ("C", "c", "lo", "hi", "rho", "lam0", "lam1", "y0", "y1", "cert") + (("E",) if rows else ()):
            assert run(name, null=(k,)) == INVALID, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert run(name, **{k: 0}) == INVALID, (name, k)
        assert run(name, lam1=p["lam0"]) == INVALID and run(name, y1=p["y0"]) == INVALID, name
        if rows:
            assert run(name, mx=0, mu=0) == INVALID and run(name, mx=0, N=1) == INVALID, name      # no rows at all
            assert run(name, mx=65) == UNSUPPORTED and run(name, mu=65) == UNSUPPORTED, name
            assert run(name, mx=0, mu=0, nx=200) == INVALID, name                                   # INVALID before UNSUPPORTED
        assert run(name, nx=200, nu=100) == UNSUPPORTED, name                                       # a knot that does not fit the LDS
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert same(b, before[k]), k
    # C may be NULL when N == 1
    shape1 = (3, 2, 1, 2, 2, 0)
    t1, _ = device_tensors(data(*shape1, dtype))
    assert t1["C"] is None
    call(solver, shape1, t1)
    assert np_same(t1["cert"].cpu().numpy().reshape(2, 3), reference(*shape1, dtype)[0])


# ---- 5. a caller-owned capture of copy -> step -> certificate replays to the bits of the calls
def box_loop(solver, dtype, d, lo, hi):
    nx, nu, N, B = admm_ref.CONV_SHAPE
    return hard.Loop(solver, nx, nu, N, B, dtype, d, np.array(admm_ref.CONV_RHO), lo=lo, hi=hi, tol=PCG_TOL[dtype], max_iter=200)


def box_aside(L, o):
    B = L.shape[3]
    return dict(lam0=torch.full_like(o["lam"], float("nan")), y0=torch.full_like(o["y"], float("nan")),
                cert=torch.full((B, 3), float("nan"), dtype=L.g.dtype, device="cuda"), flag=torch.full((B,), 7, dtype=torch.uint8, device="cuda"))


def box_tick(L, o, a, step):
    """copy aside, one iteration, the certificate of (before, after)"""
    nx, nu, N, B = L.shape
    a["lam0"].copy_(o["lam"])
    a["y0"].copy_(o["y"])
    step()
    L.s.admm_infeas(nx, nu, N, B, L.C, L.c, L.lo, L.hi, L.rho, a["lam0"], o["lam"], a["y0"], o["y"], ir.EPS, cert=a["cert"], flag=a["flag"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_captured_copy_step_certificate_replays_the_bits_of_the_calls(solver, dtype):
    d, lo, hi, _ = sr.infeasible_inputs()
    L = box_loop(solver, dtype, d, lo, hi)
    oa, ob = L.state(), L.state()
    aa, ab = box_aside(L, oa), box_aside(L, ob)
    for _ in range(3):
        box_tick(L, oa, aa, lambda: hard.one_call(L, oa))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):     # the capturing stream is torch's current one inside the block
        box_tick(L, ob, ab, lambda: hard.one_call(L, ob))
    for k, v in L.start.items():      # the capture ran nothing: start again from the saved state, outputs poisoned
        ob[k].copy_(v)
    for k in ("cert", "lam0", "y0"):
        ab[k].fill_(float("nan"))
    ab["flag"].fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("lam", "z", "w", "y", "gt", "res"):
        assert same(oa[k], ob[k]), k
    for k in ("lam0", "y0", "cert", "flag"):
        assert same(aa[k], ab[k]), k


# ---- 6. end to end: the infeasible fixture is flagged at the pinned iteration, the feasible fixtures never
@pytest.mark.parametrize("dtype,pinned", [(F32, ir.FLAG_AT_F32), (F64, ir.FLAG_AT_F64)])
def test_infeasible_fixture_is_flagged_at_the_pinned_iteration(solver, dtype, pinned):
    d, lo, hi, _ = sr.infeasible_inputs()
    nx, nu, N, B = admm_ref.CONV_SHAPE
    L = box_loop(solver, dtype, d, lo, hi)
    o = L.state()
    a = box_aside(L, o)
    gr = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"], o["r"], o["p"],
                                L.tol, L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
    certs, flags = [], []
    for _ in range(sr.INFEAS_K):
        box_tick(L, o, a, gr.launch)
        certs.append(a["cert"].clone())
        flags.append(a["flag"].clone())
    torch.cuda.synchronize()
    gr.close()
    certs, flags = torch.stack(certs).cpu().numpy().astype(F64), torch.stack(flags).cpu().numpy()      # [K, B, 3], [K, B]
    for b in range(B):
        n, r, sigma = certs[:, b].T
        at = int(np.argmax(flags[1:, b])) + 2 if flags[1:, b].any() else None       # the pair (k - 1, k) from k = 2 on, as the reference counts
        print(f"{np.dtype(dtype).name} problem {b}: flagged at iteration {at} (pinned {pinned[b]}); there r/n = {r[pinned[b] - 1] / n[pinned[b] - 1]:.4f}, "
              f"sigma/n = {sigma[pinned[b] - 1] / n[pinned[b] - 1]:.4f}; at {sr.INFEAS_K}: r/n = {r[-1] / n[-1]:.2e}, sigma/n = {sigma[-1] / n[-1]:.4f}")
        assert at == pinned[b], (b, at, pinned[b])
        assert flags[at - 1:, b].all()
        assert r[-1] < 2e-3 * n[-1] and abs(sigma[-1] / n[-1] + sr.INFEAS_GAP) < 5e-3


FEASIBLE_K = 150      # replays: the box fixture's residuals are at the fp32 floor of z by 80 (tests/test_gpu_admm.py)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["box", "rows"])
def test_feasible_fixtures_are_never_flagged(solver, kind, dtype):
    nx, nu, N, B = admm_ref.CONV_SHAPE
    if kind == "box":
        d, lo, hi, _ = admm_ref.convergence_inputs()
        L = box_loop(solver, dtype, d, lo, hi)
        o = L.state()
        gr = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"], o["r"],
                                    o["p"], L.tol, L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
    else:
        mx, mu = lr.CONV_ROWS
        d, E, lo, hi, _ = lr.convergence_inputs()
        L = lin.LinLoop(solver, (nx, nu, N, B, mx, mu), dtype, d, E, np.array(lr.CONV_RHO), lo=lo, hi=hi, tol=PCG_TOL[dtype], max_iter=200)
        o = L.state()
        gr = L.graph(o)
    a = box_aside(L, o)
    any_flag = torch.zeros(B, dtype=torch.uint8, device="cuda")
    low = torch.full((B,), float("inf"), dtype=L.g.dtype, device="cuda")
    for k in range(FEASIBLE_K):
        a["lam0"].copy_(o["lam"])
        a["y0"].copy_(o["y"])
        gr.launch()
        if kind == "box":
            solver.admm_infeas(nx, nu, N, B, L.C, L.c, L.lo, L.hi, L.rho, a["lam0"], o["lam"], a["y0"], o["y"], ir.EPS, cert=a["cert"], flag=a["flag"])
        else:
            solver.admm_lin_infeas(nx, nu, mx, mu, N, B, L.C, L.c, L.E, L.lo, L.hi, L.rho, a["lam0"], o["lam"], a["y0"], o["y"], ir.EPS,
                                   cert=a["cert"], flag=a["flag"])
        if k >= 1:
            any_flag |= a["flag"]
            risky = (a["cert"][:, 2] < 0) & (a["cert"][:, 0] > 0)
            low = torch.minimum(low, torch.where(risky, a["cert"][:, 1] / a["cert"][:, 0], torch.full_like(low, float("inf"))))
    torch.cuda.synchronize()
    gr.close()
    print(f"{kind} {np.dtype(dtype).name}: smallest r/n with sigma < 0 over {FEASIBLE_K} replays {low.cpu().numpy()} (reference {ir.FEASIBLE_MIN_RATIO}, eps {ir.EPS}); "
          f"final res {o['res'].cpu().numpy().max(axis=0)}")
    assert int(any_flag.sum()) == 0
