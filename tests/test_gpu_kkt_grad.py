"""The device half of the KKT backward pass (csrc/kkt_grad.hip through the C ABI): gbdpcg_kkt_grad_*, gbdpcg_kkt_grad_shared_*,
gbdpcg_kkt_backward_* and its shared and graph forms.

Reference: tests/kkt_grad_ref.py (pinned against fp64 autograd by tests/test_kkt_grad_reference.py).  The per-problem kernel is
defined to the bit -- two rounded products, one rounded add, an exact scaling -- so its outputs must EQUAL the twin evaluated in
the call's precision.  The shared form is a sum over the batch in a fixed order: any-order summation bound against the fp64 twin,
identical bits from call to call, and the per-problem bits at batch 1.  The composite calls are bit for bit the calls they are
made of.  Run with -s for the measured figures."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kkt_grad_ref as kgr  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
UNIT = {F32: 2.0 ** -24, F64: 2.0 ** -53}
SMALL = [s for s in kgr.SHAPES if s[2] <= 33]
GUARD = 1024
SENTINEL = 777.0


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


TORCH = {F32: torch.float32, F64: torch.float64}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def guarded(n, dtype):
    """n elements of NaN between sentinel guards; (whole, view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    whole[GUARD:GUARD + n] = float("nan")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def points(nx, nu, N, B, dtype, seed=0):
    """Random (z, lam, az, alam) of order 1, [B, .] in `dtype`; read-only."""
    rng = np.random.default_rng(1000 * nx + 10 * N + B + seed)
    sz = so.sizes(nx, nu, N)
    out = tuple(rng.standard_normal((B, sz[k])).astype(dtype) for k in ("g", "c", "g", "c"))
    for a in out:
        a.setflags(write=False)
    return out


def twin(nx, nu, N, pts, dtype):
    parts = [kgr.block_grads(nx, nu, N, *(a[b] for a in pts), dtype=dtype) for b in range(pts[0].shape[0])]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def run_grad(solver, nx, nu, N, B, pts, shared=False, want="GC"):
    """The launch into guarded NaN-filled outputs; checks the guards and that every element was written."""
    dt = TORCH[pts[0].dtype.type]
    sz, mats = so.sizes(nx, nu, N), 1 if shared else B
    want = want if N > 1 else want.replace("C", "")
    Gw, gG = guarded(mats * sz["G"], dt) if "G" in want else (None, None)
    Cw, gC = guarded(mats * sz["C"], dt) if "C" in want else (None, None)
    fn = solver.kkt_grad_shared if shared else solver.kkt_grad
    fn(nx, nu, N, B, *(dev(a.reshape(-1)) for a in pts), gG=gG, gC=gC, want="")
    torch.cuda.synchronize()
    for whole, view in ((Gw, gG), (Cw, gC)):
        if view is not None:
            assert guards_intact(whole, view.numel())
            if all(np.isfinite(a).all() for a in pts):
                assert not bool(torch.isnan(view).any()), "an output element was not written"
    return (None if gG is None else gG.cpu().numpy()), (None if gC is None else gC.cpu().numpy())


# ---- 1. the per-problem kernel, to the bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", kgr.SHAPES)
def test_grad_bits(solver, nx, nu, N, B, dtype):
    pts = points(nx, nu, N, B, dtype)
    tG, tC = twin(nx, nu, N, pts, dtype)
    gG, gC = run_grad(solver, nx, nu, N, B, pts)
    assert gG.dtype == dtype and same_bits(gG, tG)
    if N > 1:
        assert same_bits(gC, tC)
    # gQ_k, gR_k bit-symmetric
    sg, LG = nx * nx + nu * nu, so.sizes(nx, nu, N)["G"]
    for b in range(B):
        for k in range(N):
            Q = bits(gG[b * LG + k * sg:b * LG + k * sg + nx * nx]).reshape(nx, nx)
            assert np.array_equal(Q, Q.T)
            if k < N - 1:
                R = bits(gG[b * LG + k * sg + nx * nx:b * LG + (k + 1) * sg]).reshape(nu, nu)
                assert np.array_equal(R, R.T)
    # either output alone: the other's bits are what they were
    oG, none = run_grad(solver, nx, nu, N, B, pts, want="G")
    assert none is None and same_bits(oG, gG)
    if N > 1:
        none, oC = run_grad(solver, nx, nu, N, B, pts, want="C")
        assert none is None and same_bits(oC, gC)


def test_grad_unaligned_outputs(solver):
    """Output pointers that are element- but not 16-byte aligned: the scalar head follows the address, same bits."""
    nx, nu, N, B = 5, 2, 9, 2
    for dtype in DTYPES:
        pts = points(nx, nu, N, B, dtype)
        tG, tC = twin(nx, nu, N, pts, dtype)
        dt = TORCH[dtype]
        for shift in (1, 2, 3):
            Gw, Cw = (torch.full((n + 8,), SENTINEL, dtype=dt, device="cuda") for n in (tG.size, tC.size))
            gG, gC = Gw[shift:shift + tG.size], Cw[shift:shift + tC.size]
            assert gG.data_ptr() % 16 != 0 or dtype == F64 and shift == 2
            solver.kkt_grad(nx, nu, N, B, *(dev(a.reshape(-1)) for a in pts), gG=gG, gC=gC)
            torch.cuda.synchronize()
            assert same_bits(gG, tG) and same_bits(gC, tC)
            for whole, n in ((Gw, tG.size), (Cw, tC.size)):
                assert bool((whole[:shift] == SENTINEL).all()) and bool((whole[shift + n:] == SENTINEL).all())


# ---- 2. the shared sum
# batches 1, 2, 3, 7, 64 at the small shapes; the bench shape at 1 and at its own 3
SHARED_CASES = [s[:3] + (B,) for s in SMALL for B in (1, 2, 3, 7, 64)] + [(14, 7, 128, 1), (14, 7, 128, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", SHARED_CASES)
def test_shared_sum(solver, nx, nu, N, B, dtype):
    pts = points(nx, nu, N, B, dtype, seed=1)
    sG, sC = run_grad(solver, nx, nu, N, B, pts, shared=True)
    again = run_grad(solver, nx, nu, N, B, pts, shared=True)
    assert same_bits(sG, again[0]) and (N == 1 or same_bits(sC, again[1]))
    p64 = [a.astype(F64) for a in pts]
    ref = [sum(t) for t in zip(*(kgr.block_grads(nx, nu, N, *(a[b] for a in p64)) for b in range(B)))]
    mag = [sum(t) for t in zip(*(kgr.block_bound(nx, nu, N, *(a[b] for a in p64)) for b in range(B)))]
    for name, got, want, m in zip("GC", (sG, sC), ref, mag):
        if got is None:
            continue
        err, bound = np.abs(got.astype(F64) - want), (B + 2) * UNIT[dtype] * m
        print(f"shared g{name} ({nx},{nu},{N}) B={B} {np.dtype(dtype).name}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), name
    if B == 1:
        gG, gC = run_grad(solver, nx, nu, N, 1, pts)
        assert same_bits(sG, gG) and (N == 1 or same_bits(sC, gC))


# ---- 3. isolation between problems
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(5, 2, 9, 3), (12, 4, 33, 3), (14, 7, 128, 3)])
def test_nan_stays_in_its_problem(solver, nx, nu, N, B, dtype):
    pts = points(nx, nu, N, B, dtype)
    gG, gC = run_grad(solver, nx, nu, N, B, pts)
    bad = [a.copy() for a in pts]
    bad[2][1, :] = np.nan       # a_z of problem 1
    bG, bC = run_grad(solver, nx, nu, N, B, tuple(bad))
    sz = so.sizes(nx, nu, N)
    for got, clean, n in ((bG, gG, sz["G"]), (bC, gC, sz["C"])):
        got, clean = got.reshape(B, n), clean.reshape(B, n)
        assert np.isnan(got[1]).all()
        assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[2])


# ---- 4. the composite calls
PCG_TOL = {F32: 1e-10, F64: 1e-22}


def setting(solver, nx, nu, N, B, dtype, shared):
    """A factorisation (one problem's when shared), a forward point and upstream gradients on the device."""
    mats = 1 if shared else B
    d = so.gen(nx, nu, N, seed=31, batch=mats, dtype=dtype)
    v = so.gen(nx, nu, N, seed=32, batch=B, dtype=dtype)
    G, C = dev(d["G"].reshape(-1)), dev(d["C"].reshape(-1))
    g, c = dev(v["g"].reshape(-1)), dev(v["c"].reshape(-1))
    S, _, Ginv = solver.form_schur(nx, nu, N, mats, G, C, g[:mats * g.numel() // B], c[:mats * c.numel() // B])
    Pinv = solver.form_pinv(nx, N, mats, S, binding.PINV_STAIR)
    gamma = torch.empty(B * nx * N, dtype=g.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    resolve = solver.kkt_resolve_shared if shared else solver.kkt_resolve
    resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, tol=PCG_TOL[dtype], max_iter=200)
    rng = np.random.default_rng(7)
    gz = dev(rng.standard_normal(z.numel()).astype(dtype))
    nglam = dev(rng.standard_normal(lam.numel()).astype(dtype))
    torch.cuda.synchronize()
    return Ginv, C, S, Pinv, z, lam, gz, nglam


def adjoint_buffers(nx, nu, N, B, z, lam, shared):
    sz, mats = so.sizes(nx, nu, N), 1 if shared else B
    nan = lambda n: torch.full((n,), float("nan"), dtype=z.dtype, device="cuda")   # noqa: E731
    return {"gamma": nan(lam.numel()), "az": nan(z.numel()), "alam": torch.zeros_like(lam), "r": nan(lam.numel()), "p": nan(lam.numel()),
            "it": torch.full((B,), -1, dtype=torch.int32, device="cuda"), "fl": torch.full((B,), 9, dtype=torch.uint8, device="cuda"),
            "gG": nan(mats * sz["G"]), "gC": nan(mats * sz["C"])}


def two_calls(solver, nx, nu, N, B, st, shared, dtype):
    Ginv, C, S, Pinv, z, lam, gz, nglam = st
    o = adjoint_buffers(nx, nu, N, B, z, lam, shared)
    resolve = solver.kkt_resolve_shared if shared else solver.kkt_resolve
    grad = solver.kkt_grad_shared if shared else solver.kkt_grad
    resolve(nx, nu, N, B, Ginv, C, gz, nglam, S, Pinv, o["gamma"], o["alam"], o["az"], r=o["r"], p=o["p"], tol=PCG_TOL[dtype],
            max_iter=200, iters=o["it"], max_iter_exit=o["fl"])
    grad(nx, nu, N, B, z, lam, o["az"], o["alam"], gG=o["gG"], gC=o["gC"])
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 5), (5, 3, 10, 4)])
def test_backward_is_the_two_calls(solver, nx, nu, N, B, dtype, shared):
    st = setting(solver, nx, nu, N, B, dtype, shared)
    Ginv, C, S, Pinv, z, lam, gz, nglam = st
    want = two_calls(solver, nx, nu, N, B, st, shared, dtype)
    assert int(want["fl"].sum()) == 0 and int(want["it"].min()) > 0 and bool(torch.isfinite(want["gG"]).all())
    o = adjoint_buffers(nx, nu, N, B, z, lam, shared)
    back = solver.kkt_backward_shared if shared else solver.kkt_backward
    back(nx, nu, N, B, Ginv, C, gz, nglam, S, Pinv, o["gamma"], z, lam, o["az"], o["alam"], o["gG"], o["gC"], r=o["r"], p=o["p"],
         tol=PCG_TOL[dtype], max_iter=200, iters=o["it"], max_iter_exit=o["fl"])
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(o[k].view(torch.uint8), want[k].view(torch.uint8)), k
    # the graph: the same bits, and again after gz is rewritten in place
    o = adjoint_buffers(nx, nu, N, B, z, lam, shared)
    make = solver.graph_kkt_backward_shared if shared else solver.graph_kkt_backward
    gr = make(nx, nu, N, B, Ginv, C, gz, nglam, S, Pinv, o["gamma"], z, lam, o["az"], o["alam"], o["r"], o["p"], PCG_TOL[dtype], 200,
              o["it"], o["fl"], o["gG"], o["gC"])
    gr.launch()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(o[k].view(torch.uint8), want[k].view(torch.uint8)), "graph " + k
    gz.copy_(dev(np.random.default_rng(8).standard_normal(gz.numel()).astype(dtype)))
    want2 = two_calls(solver, nx, nu, N, B, st, shared, dtype)
    assert not torch.equal(want2["gG"], want["gG"])
    o["alam"].zero_()
    gr.launch()
    torch.cuda.synchronize()
    for k in want2:
        assert torch.equal(o[k].view(torch.uint8), want2[k].view(torch.uint8)), "replay " + k
    gr.close()


# ---- 5. refusals write nothing
def test_bad_arguments_write_nothing(solver):
    nx, nu, N, B = 14, 7, 8, 2
    st = setting(solver, nx, nu, N, B, F32, False)
    Ginv, C, S, Pinv, z, lam, gz, nglam = st
    sz = so.sizes(nx, nu, N)
    outs = {k: torch.full((n,), SENTINEL, device="cuda") for k, n in (("gamma", lam.numel()), ("az", z.numel()), ("alam", lam.numel()),
                                                                     ("gG", B * sz["G"]), ("gC", B * sz["C"]))}
    it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    lib, h = solver.lib, solver.h
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def calls(suf, ft, nx_, nu_, z_, gG_=outs["gG"], gC_=outs["gC"]):
        head = (h, nx_, nu_, N, B)
        grad = (p(z_), p(lam), p(outs["az"]), p(outs["alam"]), p(gG_), p(gC_))
        back = (p(Ginv), p(C), p(gz), p(nglam), p(S), p(Pinv), p(outs["gamma"]), p(z_), p(lam), p(outs["az"]), p(outs["alam"]), None, None,
                ft(1e-6), 10, p(it), None, p(gG_), p(gC_))
        res = []
        for tw in ("", "_shared"):
            gr = ctypes.c_void_p()
            res += [getattr(lib, f"gbdpcg_kkt_grad{tw}_{suf}")(*head, *grad, None),
                    getattr(lib, f"gbdpcg_kkt_backward{tw}_{suf}")(*head, *back, None),
                    getattr(lib, f"gbdpcg_graph_create_kkt_backward{tw}_{suf}")(*head, *back, ctypes.byref(gr))]
            assert not gr.value
        return res

    assert calls("f32", ctypes.c_float, nx, nu, None) == [1] * 6                      # null forward point
    assert calls("f32", ctypes.c_float, nx, 0, z) == [1] * 6                          # controlSize 0
    assert calls("f32", ctypes.c_float, 0, nu, z) == [1] * 6                          # stateSize 0
    assert calls("f32", ctypes.c_float, nx, nu, z, None, None) == [1] * 6             # nothing to write
    assert calls("f64", ctypes.c_double, 80, 40, z) == [4] * 6                        # a shape form_schur refuses
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), k
    assert bool((it == -1).all())
