"""Box-constrained ADMM on a kept factorisation, on the device (csrc/admm.hip and the composite calls of csrc/api_kkt.hip, through the C
ABI): gbdpcg_admm_init_*, gbdpcg_admm_update_*, gbdpcg_admm_step_*, the shared twin and the two graphs.  PARITY UNPINNED: the
reference tree has no code, fixture or output for these steps.

Reference: tests/admm_ref.py.  The update is defined to the bit (every line one IEEE operation or a comparison), so w, y and the two
norms are compared for EQUALITY with update_ref in the call's precision; gt, the one fused multiply-add, is held against its exact
rational value within u (|rho t| + |ref|), u = 2^-24 / 2^-53: the bound of one or two roundings.  The composite calls are compared
bit for bit with the calls they are made of.  Convergence (test 7) runs the three problems tests/test_admm_reference.py pins:
 (a) z of iterations 1, 2, 10, 80 against the fp64 dense solve of the regularised KKT system for the device's own gt of that
     iteration, 3e-4 / 1e-9 norm-wise (STEP_TOL of tests/test_gpu_reg.py, copied);
 (b) ||z_dev(80) - z*||_inf <= 2 ||z_ref(80) - z*||_inf + 80 STEP_TOL ||z*||_inf: a fixed-rho ADMM iteration is an averaged operator,
     per-step errors add and do not grow; in fp32 the right side is about 1e-2 against a first-iteration distance of at least 0.15;
 (c) res[2b](80) <= 1e-2 res[2b](1): the reference's worst problem gives 1.5e-3, the margin is for the fp32 floor of z;
 (d) lo <= w <= hi exactly, no solve ran out of iterations.
Run with -s for the measured figures."""
import copy
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_ref  # noqa: E402
from admm_util import bits, dev, np_same, same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
STEP_TOL = {F32: 3e-4, F64: 1e-9}     # tests/test_gpu_reg.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
UPDATE_SHAPES = [(1, 1, 1, 1),     # nz = 1
                 (2, 1, 2, 3),     # nz = 5
                 (3, 3, 5, 2),     # nz = 27: less than a wave
                 (5, 2, 10, 4),    # nz = 68: a second pass of a one-wave workgroup, odd problem stride
                 (12, 4, 17, 3),   # nz = 268: four waves, ragged last pass
                 (14, 7, 37, 3)]   # nz = 770


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


def roundoff(dtype):
    return 2.0 ** -24 if dtype == F32 else 2.0 ** -53


@functools.lru_cache(maxsize=None)
def update_data(nx, nu, N, B, dtype):
    """z, w, y, g of order 1, bounds near +-0.3 with a third of each side infinite (so about 0.28 of v = z + y clip at either
    side), rho_b in [0.5, 4]: arrays [B, nz] of `dtype`, read-only."""
    rng = np.random.default_rng(1000 + nz_of(nx, nu, N))
    nz = nz_of(nx, nu, N)
    z, w, y, g = (rng.standard_normal((B, nz)).astype(dtype) for _ in range(4))
    lo = (-0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype)
    hi = (0.3 + 0.05 * rng.standard_normal((B, nz))).astype(dtype)
    lo[rng.random((B, nz)) < 1.0 / 3.0] = -np.inf
    hi[rng.random((B, nz)) < 1.0 / 3.0] = np.inf
    rho = rng.uniform(0.5, 4.0, B).astype(dtype)
    d = dict(z=z, w=w, y=y, g=g, lo=lo, hi=hi, rho=rho)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def update_reference(nx, nu, N, B, dtype, init):
    d = update_data(nx, nu, N, B, dtype)
    return admm_ref.update_ref(dtype, d["g"], d["lo"], d["hi"], d["rho"], None if init else d["z"], d["w"], d["y"])


def run_update(solver, nx, nu, N, B, t, init, res=None):
    """t: dict of device tensors (flat); w, y are updated in place, gt is written.  Returns res ([B, 2]) or None."""
    if init:
        solver.admm_init(nx, nu, N, B, t["g"], t["lo"], t["hi"], t["rho"], t["w"], t["y"], gt=t["gt"])
        return None
    return solver.admm_update(nx, nu, N, B, t["g"], t["lo"], t["hi"], t["rho"], t["z"], t["w"], t["y"], t["gt"], res=res)


def device_tensors(d, offset=None):
    """The arrays of update_data on the device, flat, plus gt (NaN).  offset: every array starts `offset` elements into a buffer of its
    own whose base the allocator aligns (to 512 bytes): 0 -> 16-byte aligned bases, 1 -> every base off by one element."""
    t = {}
    for k, a in list(d.items()) + [("gt", np.full_like(d["g"], np.nan))]:
        flat = dev(a.reshape(-1))
        if offset is not None and k != "rho":
            buf = torch.full((flat.numel() + 8,), float("nan"), dtype=flat.dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[offset:offset + flat.numel()] = flat
            flat = buf[offset:offset + flat.numel()]
        t[k] = flat
    return t


def check_gt(gt, ref_gt, t, rho, dtype, what):
    u = Fraction(roundoff(dtype))
    B, nz = t.shape
    worst = Fraction(0)
    for b in range(B):
        r = Fraction(float(rho[b]))
        for i in range(nz):
            ref = ref_gt[b, i]
            assert ref is not None and np.isfinite(gt[b, i]), (what, b, i)
            err, bound = abs(Fraction(float(gt[b, i])) - ref), u * (abs(r * Fraction(float(t[b, i]))) + abs(ref))
            assert err <= bound, (what, b, i, float(err), float(bound))
            if bound:
                worst = max(worst, err / bound)
    print(f"{what}: gt worst error / bound {float(worst):.3f}")


# ---- 1. the update and the initialisation against update_ref
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", UPDATE_SHAPES)
def test_update_and_init_vs_reference(solver, nx, nu, N, B, dtype, init):
    d = update_data(nx, nu, N, B, dtype)
    wr, yr, tr, gr, rr = update_reference(nx, nu, N, B, dtype, init)
    t = device_tensors(d)
    res = run_update(solver, nx, nu, N, B, t, init)
    torch.cuda.synchronize()
    w, y, gt = (t[k].cpu().numpy().reshape(B, -1) for k in ("w", "y", "gt"))
    what = f"({nx},{nu},{N},{B}) {np.dtype(dtype).name} {'init' if init else 'update'}"
    assert np_same(w, wr), what + ": w"
    assert np_same(y, yr), what + ": y"
    if not init:
        assert np_same(res.cpu().numpy(), rr), what + ": res"
    check_gt(gt, gr, tr, d["rho"], dtype, what)
    if init:
        assert ((w >= d["lo"]) & (w <= d["hi"])).all()
        return
    # y != 0 only where w sits on the bound of that sign; exactly 0 wherever v lies strictly inside
    v = d["z"] + d["y"]
    assert v.dtype == np.dtype(dtype)
    assert (w[y > 0] == d["hi"][y > 0]).all() and (w[y < 0] == d["lo"][y < 0]).all()
    inside = (d["lo"] < v) & (v < d["hi"])
    assert not y[inside].any() and np_same(w[inside], v[inside])
    low, high = float((v < d["lo"]).mean()), float((v > d["hi"]).mean())
    print(f"{what}: {low:.2f} of v clipped below, {high:.2f} above")
    if w.size >= 64:
        assert 0.15 < low < 0.45 and 0.15 < high < 0.45


# ---- 2. the 16-byte form and the all-scalar form give the same bits
@pytest.mark.parametrize("init", [False, True], ids=["update", "init"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", UPDATE_SHAPES[1:])
def test_aligned_and_misaligned_bases_agree(solver, nx, nu, N, B, dtype, init):
    d = update_data(nx, nu, N, B, dtype)
    wr, yr, _, _, rr = update_reference(nx, nu, N, B, dtype, init)
    out = []
    for offset in (0, 1):
        t = device_tensors(d, offset)
        assert all(t[k].data_ptr() % 16 == (0 if offset == 0 else t[k].element_size()) for k in ("g", "lo", "hi", "z", "w", "y", "gt"))
        res = run_update(solver, nx, nu, N, B, t, init)
        torch.cuda.synchronize()
        out.append({k: t[k].clone() for k in ("w", "y", "gt")})
        if not init:
            out[-1]["res"] = res.clone()
    for k in out[0]:
        assert same(out[0][k], out[1][k]), k
    assert np_same(out[1]["w"].cpu().numpy().reshape(B, -1), wr) and np_same(out[1]["y"].cpu().numpy().reshape(B, -1), yr)
    if not init:
        assert np_same(out[1]["res"].cpu().numpy(), rr)


# ---- 3. footprint
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(5, 2, 10, 4), (12, 4, 17, 3)])
def test_footprint(solver, nx, nu, N, B, dtype):
    d = update_data(nx, nu, N, B, dtype)
    GUARD = 1024
    results = []
    for fill in (float("nan"), 1e30):
        bufs, t = {}, {}
        for k, a in list(d.items()) + [("gt", np.full_like(d["g"], np.nan)), ("res", np.full((B, 2), fill, dtype))]:
            n = a.size
            buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=tdt(dtype), device="cuda")
            buf[GUARD:GUARD + n] = dev(a.reshape(-1))
            bufs[k], t[k] = buf, buf[GUARD:GUARD + n]
        before = {k: b.clone() for k, b in bufs.items()}
        run_update(solver, nx, nu, N, B, t, False, res=t["res"])
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert same(b[:GUARD], before[k][:GUARD]) and same(b[-GUARD:], before[k][-GUARD:]), f"guard of {k}"
            assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all())
        for k in ("z", "g", "lo", "hi", "rho"):
            assert same(bufs[k], before[k]), f"{k} was written"
        for k in ("w", "y", "gt", "res"):
            assert bool(torch.isfinite(t[k]).all()), k
        results.append({k: t[k].clone() for k in ("w", "y", "gt", "res")})
    for k in results[0]:
        assert same(results[0][k], results[1][k]), k     # nothing is read from res


# ---- 4. NaN and Inf
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_problem_and_infinite_box_is_identity(solver, dtype):
    nx, nu, N, B = 12, 4, 17, 3
    d = update_data(nx, nu, N, B, dtype)
    clean = device_tensors(d)
    rc = run_update(solver, nx, nu, N, B, clean, False)
    t = device_tensors(d)
    j = 131
    t["z"].view(B, -1)[1, j] = float("nan")
    res = run_update(solver, nx, nu, N, B, t, False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(res[1]).all())
    assert bool(torch.isnan(t["w"].view(B, -1)[1, j])) and bool(torch.isnan(t["gt"].view(B, -1)[1, j]))
    for p in (0, 2):
        for k in ("w", "y", "gt"):
            assert same(t[k].view(B, -1)[p], clean[k].view(B, -1)[p]), (k, p)
        assert same(res[p], rc[p]) and bool(torch.isfinite(res[p]).all())
    # every bound infinite: nothing clips
    t = device_tensors(d)
    t["lo"].fill_(float("-inf"))
    t["hi"].fill_(float("inf"))
    res = run_update(solver, nx, nu, N, B, t, False)
    torch.cuda.synchronize()
    v = d["z"] + d["y"]
    assert np_same(t["w"].cpu().numpy().reshape(B, -1), v)
    assert not bits(t["y"]).any()
    assert np_same(res[:, 0].cpu().numpy(), np.abs(d["z"] - v).max(axis=1))


# ---- 5. / 6. the composite calls
@functools.lru_cache(maxsize=None)
def step_problem(nx, nu, N, B, seed=61):
    d = {k: v.astype(F32).astype(F64) for k, v in so.gen(nx, nu, N, seed=seed, batch=B, dtype=F64).items()}
    for a in d.values():
        a.setflags(write=False)
    return d


class Loop:
    """A factorisation of G + rho I (kkt_step_reg) with a box around its z, and the buffers of the iteration."""

    def __init__(self, solver, nx, nu, N, B, dtype, d, rho, lo=None, hi=None, tol=1e-8, max_iter=100):
        self.s, self.shape, self.tol, self.max_iter = solver, (nx, nu, N, B), tol, max_iter
        self.G, self.C, self.g, self.c = (dev(d[k].astype(dtype).reshape(-1)) for k in "GCgc")
        if N == 1:
            self.C = None
        self.rho = dev(np.asarray(rho, dtype))
        nan = float("nan")
        self.S = torch.full((B * 3 * nx * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.Pinv, self.Ginv = torch.full_like(self.S, nan), torch.full_like(self.G, nan)
        self.gamma = torch.full((B * nx * N,), nan, dtype=self.G.dtype, device="cuda")
        self.lam, self.z = torch.zeros_like(self.gamma), torch.full_like(self.g, nan)
        it, fl = solver.kkt_step_reg(nx, nu, N, B, self.G, self.C, self.g, self.c, self.rho, self.S, self.gamma, self.Ginv, self.Pinv,
                                     self.lam, self.z, tol=tol, max_iter=max_iter)
        torch.cuda.synchronize()
        assert int(fl.sum()) == 0
        if lo is None:
            z0 = self.z.cpu().numpy().astype(F64).reshape(B, -1)
            bounds = [admm_ref.box(z0[b], nx, nu, N) for b in range(B)]
            lo, hi = np.stack([p[0] for p in bounds]), np.stack([p[1] for p in bounds])
        self.lo, self.hi = dev(lo.astype(dtype).reshape(-1)), dev(hi.astype(dtype).reshape(-1))
        self.w, self.y = torch.zeros_like(self.g), torch.zeros_like(self.g)
        self.gt = solver.admm_init(nx, nu, N, B, self.g, self.lo, self.hi, self.rho, self.w, self.y)
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


    def first(self, o):
        """(L1, o1): problem 0 alone -- the loop with batch = 1 and views of the leading problem of every buffer of o."""
        nx, nu, N, B = self.shape
        L1 = copy.copy(self)
        L1.shape = (nx, nu, N, 1)
        for k in ("g", "c", "lo", "hi", "rho"):
            t = getattr(self, k)
            setattr(L1, k, t[:t.numel() // B])
        return L1, {k: v[:v.shape[0] // B] for k, v in o.items()}


ORDER = ("gamma", "lam", "r", "p", "z", "it", "fl", "w", "y", "gt", "res")


def two_calls(L, o, mats=None, shared=False, rho=None):
    nx, nu, N, B = L.shape
    Ginv, C, S, Pinv = mats or (L.Ginv, L.C, L.S, L.Pinv)
    resolve = L.s.kkt_resolve_shared if shared else L.s.kkt_resolve
    resolve(nx, nu, N, B, Ginv, C, o["gt"], L.c, S, Pinv, o["gamma"], o["lam"], o["z"], r=o["r"], p=o["p"], tol=L.tol,
            max_iter=L.max_iter, iters=o["it"], max_iter_exit=o["fl"])
    L.s.admm_update(nx, nu, N, B, L.g, L.lo, L.hi, L.rho if rho is None else rho, o["z"], o["w"], o["y"], o["gt"], res=o["res"])


def one_call(L, o, mats=None, shared=False, rho=None):
    nx, nu, N, B = L.shape
    Ginv, C, S, Pinv = mats or (L.Ginv, L.C, L.S, L.Pinv)
    step = L.s.admm_step_shared if shared else L.s.admm_step
    step(nx, nu, N, B, Ginv, C, L.g, L.c, L.lo, L.hi, L.rho if rho is None else rho, S, Pinv, o["gamma"],
         o["lam"], o["z"], o["w"], o["y"], o["gt"], res=o["res"], r=o["r"], p=o["p"], tol=L.tol, max_iter=L.max_iter, iters=o["it"],
         max_iter_exit=o["fl"])


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 3), (3, 3, 5, 2), (12, 4, 33, 2)])
def test_admm_step_is_kkt_resolve_plus_admm_update(solver, nx, nu, N, B, dtype, mode):
    L = Loop(solver, nx, nu, N, B, dtype, step_problem(nx, nu, N, B), 0.5 * (np.arange(B) + 2.0))
    solver.set_symmetric(mode)
    try:
        a, b = L.state(), L.state()
        for _ in range(2):     # the second iteration takes the first one's lambda, w, y, gt
            two_calls(L, a)
            one_call(L, b)
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    for k in ORDER:
        assert same(a[k], b[k]), k
    assert int(b["fl"].sum()) == 0 and int(b["it"].min()) >= 0 and all(bool(torch.isfinite(b[k]).all()) for k in ("z", "w", "y", "gt", "res"))
    print(f"({nx},{nu},{N},{B}) {np.dtype(dtype).name} mode {mode}: {int((b['y'] != 0).sum())} of {b['y'].numel()} bounds active")


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 24, 3), (3, 3, 5, 2), (12, 4, 33, 2)])
def test_shared_twin(solver, nx, nu, N, B, dtype, mode):
    """One plant (problem 0's G and C, one rho), B gradients and residuals: the shared call against the per-problem call on B copies
    of the single matrices (path FUSED, as include/gbdpcg.h states the equivalence), against the two shared calls it is made of, and
    with batch = 1 against the per-problem call."""
    d = dict(step_problem(nx, nu, N, B))
    d["G"], d["C"] = np.repeat(d["G"][:1], B, axis=0), np.repeat(d["C"][:1], B, axis=0)
    L = Loop(solver, nx, nu, N, B, dtype, d, np.full(B, 1.5))
    ng, nc, ns = L.G.numel() // B, (L.C.numel() // B if L.C is not None else 0), L.S.numel() // B
    single = (L.Ginv[:ng].clone(), None if L.C is None else L.C[:nc].clone(), L.S[:ns].clone(), L.Pinv[:ns].clone())
    copies = tuple(None if m is None else m.repeat(B) for m in single)
    solver.set_symmetric(mode)
    solver.set_path(binding.PATH_FUSED)
    try:
        a, b, c = L.state(), L.state(), L.state()
        for _ in range(2):
            one_call(L, a, mats=copies)
            one_call(L, b, mats=single, shared=True)
            two_calls(L, c, mats=single, shared=True)
        # batch = 1: the shared call is the twin (problem 0's vectors lead every array)
        e, f = L.state(), L.state()
        L1, e1 = L.first(e)
        one_call(L1, e1, mats=single)
        L1, f1 = L.first(f)
        one_call(L1, f1, mats=single, shared=True)
        torch.cuda.synchronize()
    finally:
        solver.set_path(binding.PATH_AUTO)
        solver.set_symmetric(2)
    for k in ORDER:
        assert same(a[k], b[k]), f"shared vs copies: {k}"
        assert same(b[k], c[k]), f"shared step vs shared resolve + update: {k}"
        assert same(e[k], f[k]), f"batch 1: {k}"
    assert int(b["fl"].sum()) == 0 and bool(torch.isfinite(b["z"]).all())
    nz = nz_of(nx, nu, N)
    assert bool(torch.isfinite(f["z"][:nz]).all()) and bool(torch.isnan(f["z"][nz:]).all())     # batch = 1 wrote one problem


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_and_rho_rewritten_in_place(solver, dtype):
    nx, nu, N, B = 14, 7, 24, 3
    rho1 = 0.5 * (np.arange(B) + 2.0)
    L = Loop(solver, nx, nu, N, B, dtype, step_problem(nx, nu, N, B), rho1)
    g = L.state()
    solver.reserve(L.g.element_size(), nx, N, B)
    gr = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, g["gamma"], g["lam"], g["r"], g["p"],
                                L.tol, L.max_iter, g["it"], g["fl"], g["z"], g["w"], g["y"], g["gt"], g["res"])
    e = L.state()
    for i in range(3):
        gr.launch()
        one_call(L, e)
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
    one_call(L, fresh, rho=rho2.clone())
    torch.cuda.synchronize()
    for k in ORDER:
        assert same(g[k], fresh[k]), k
    for k in ("gamma", "lam", "z", "w", "y", "res"):
        ref = first[k][:, 0] if k == "res" else first[k]
        got = g[k][:, 0] if k == "res" else g[k]
        assert same(got, ref), f"{k} must not depend on rho rewritten after the formation"
    assert not bool((g["res"][:, 1] == first["res"][:, 1]).any()) and not same(g["gt"], first["gt"])
    ratio = g["res"][:, 1].cpu().numpy().astype(F64) / first["res"][:, 1].cpu().numpy().astype(F64)
    assert np.allclose(ratio, (rho1 + 0.75) / rho1, rtol=4 * roundoff(dtype))     # rho ||w+ - w||: the same w, the new rho
    gr.close()


# ---- 7. convergence on the problems tests/test_admm_reference.py pins
@pytest.mark.parametrize("dtype", DTYPES)
def test_eighty_replays_converge_like_the_reference(solver, dtype):
    nx, nu, N, B = admm_ref.CONV_SHAPE
    rho = np.array(admm_ref.CONV_RHO)
    d, lo, hi, _ = admm_ref.convergence_inputs()
    ref = admm_ref.convergence_reference(4000)
    K, marks = 80, (1, 2, 10, 80)
    L = Loop(solver, nx, nu, N, B, dtype, d, rho, lo=lo, hi=hi, tol=PCG_TOL[dtype], max_iter=200)
    assert same(L.gt, L.g)      # w = y = 0 and 0 lies in the box: the first solve is the equality-constrained one
    o = L.state()
    gr = solver.graph_admm_step(nx, nu, N, B, L.Ginv, L.C, L.g, L.c, L.lo, L.hi, L.rho, L.S, L.Pinv, o["gamma"], o["lam"], o["r"], o["p"],
                                L.tol, L.max_iter, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
    flags = torch.zeros_like(o["fl"])
    snap = {}
    for k in range(1, K + 1):
        gt_in = o["gt"].clone() if k in marks else None
        gr.launch()
        flags |= o["fl"]
        if k in marks:
            snap[k] = (gt_in, o["z"].clone(), o["res"].clone())
    torch.cuda.synchronize()
    gr.close()
    what = np.dtype(dtype).name
    tol = STEP_TOL[dtype]
    res1, res80 = snap[1][2].cpu().numpy().astype(F64), snap[K][2].cpu().numpy().astype(F64)
    w = o["w"].cpu().numpy().reshape(B, -1)
    assert int(flags.sum()) == 0, "(d) a solve ran out of iterations"
    assert ((w >= lo.astype(dtype)) & (w <= hi.astype(dtype))).all(), "(d) w outside the box"
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        nz, nl = Gd.shape[0], Cd.shape[0]
        Kkt = np.zeros((nz + nl, nz + nl))
        Kkt[:nz, :nz], Kkt[:nz, nz:], Kkt[nz:, :nz] = Gd + rho[b] * np.eye(nz), Cd.T, Cd
        for k in marks:      # (a)
            gt_in, z = (snap[k][i].cpu().numpy().astype(F64).reshape(B, -1)[b] for i in (0, 1))
            zr = np.linalg.solve(Kkt, np.concatenate([-gt_in, c]))[:nz]
            err = np.linalg.norm(z - zr) / np.linalg.norm(zr)
            print(f"{what} problem {b} iteration {k}: z against the dense solve for the device's gt {err:.3e} (tol {tol:.0e})")
            assert err <= tol, (b, k, err)
        zstar, zref = ref[b]["z"][-1], ref[b]["z"][K - 1]
        z = snap[K][1].cpu().numpy().astype(F64).reshape(B, -1)[b]
        dist, bound = np.abs(z - zstar).max(), 2 * np.abs(zref - zstar).max() + K * tol * np.abs(zstar).max()
        first = np.abs(snap[1][1].cpu().numpy().astype(F64).reshape(B, -1)[b] - zstar).max()
        ratio = res80[b, 0] / res1[b, 0]
        print(f"{what} problem {b}: ||z(80) - z*||_inf {dist:.3e} (bound {bound:.3e}, first iteration {first:.3e})  "
              f"r_prim(80)/r_prim(1) {ratio:.3e} (reference {ref[b]['r_prim'][K - 1] / ref[b]['r_prim'][0]:.3e}, bound 1e-2)")
        assert dist <= bound, (b, dist, bound)            # (b)
        assert res80[b, 0] <= 1e-2 * res1[b, 0], (b, ratio)   # (c)


# ---- 8. arguments
STEP_ARGS = ("Ginv", "C", "g", "c", "lo", "hi", "rho", "S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z", "w", "y",
             "gt", "res")
OPTIONAL = ("Pinv", "r", "p", "fl")
WRITTEN = ("gamma", "lam", "r", "p", "z", "w", "y", "gt", "res")


@pytest.mark.parametrize("suf,tt", [("f32", torch.float32), ("f64", torch.float64)])
def test_bad_arguments(solver, suf, tt):
    nx, nu, N, B = 6, 3, 4, 3
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
        v = {k: P(ins) for k in ("Ginv", "C", "g", "c", "lo", "hi", "S", "Pinv")}
        v["rho"] = P(rho)
        v.update({k: P(t) for k, t in outs.items()})
        v.update(it=P(it), fl=P(fl), tol=1e-6, max_iter=10, nx=nx, nu=nu, N=N, batch=B)
        v.update(over)
        for k in null:
            v[k] = None
        return v

    def step(name, v, graph=None):
        fn = getattr(lib, f"gbdpcg_{name}_{suf}")
        last = ctypes.byref(graph) if graph is not None else s
        return fn(solver.h, v["nx"], v["nu"], v["N"], v["batch"], *(v[k] for k in STEP_ARGS), last)

    def update(v, init=False):
        head = (solver.h, v["nx"], v["nu"], v["N"], v["batch"], v["g"], v["lo"], v["hi"], v["rho"])
        if init:
            return getattr(lib, f"gbdpcg_admm_init_{suf}")(*head, v["w"], v["y"], v["gt"], s)
        return getattr(lib, f"gbdpcg_admm_update_{suf}")(*head, v["z"], v["w"], v["y"], v["gt"], v["res"], s)

    graph = ctypes.c_void_p()
    steps = [("admm_step", None), ("admm_step_shared", None), ("graph_create_admm_step", graph), ("graph_create_admm_step_shared", graph)]
    # each required pointer NULL, each zero size: GBDPCG_ERR_INVALID
    for k in ("g", "lo", "hi", "rho", "w", "y", "gt"):
        assert update(values(null=(k,)), init=True) == 1, k
    for k in ("g", "lo", "hi", "rho", "z", "w", "y", "gt", "res"):
        assert update(values(null=(k,))) == 1, k
    for k in ("nx", "nu", "N", "batch"):
        assert update(values(**{k: 0})) == 1 and update(values(**{k: 0}), init=True) == 1, k
    for name, gr in steps:
        for k in STEP_ARGS:
            if k in OPTIONAL or k in ("tol", "max_iter"):
                continue
            assert step(name, values(null=(k,)), gr) == 1, (name, k)
        for k in ("nx", "nu", "N", "batch"):
            assert step(name, values(**{k: 0}), gr) == 1, (name, k)
        if gr is not None:
            assert getattr(lib, f"gbdpcg_{name}_{suf}")(solver.h, nx, nu, N, B, *(values()[k] for k in STEP_ARGS), None) == 1
    assert not graph.value and untouched()
    # a block size form_schur refuses: UNSUPPORTED from the step, nothing written; the update is elementwise and takes it
    big = dict(nx=80, nu=40) if suf == "f64" else dict(nx=120, nu=60)
    for name, gr in steps:
        assert step(name, values(**big), gr) == 4, name
    assert not graph.value and untouched()
    assert update(values(**big)) == 0
    torch.cuda.synchronize()
    nz = nz_of(big["nx"], big["nu"], N) * B
    for k in ("w", "y", "gt"):
        assert bool(torch.isfinite(outs[k][:nz]).all()) and bool((outs[k][nz:] == 777.0).all()), k
    assert bool(torch.isfinite(outs["res"][:2 * B]).all()) and bool((outs["res"][2 * B:] == 777.0).all())
    # N == 1 needs no C; Pinv, r, p, max_iter_exit may be NULL.  G + rho I = 2 I, so G^-1 = S = I / 2; c = 0 and the box is [0, 0]:
    # lambda = -g, z = 0 whatever g is
    eye = torch.zeros(3 * nx * nx, dtype=tt, device="cuda")
    eye[nx * nx:2 * nx * nx] = 0.5 * torch.eye(nx, dtype=tt, device="cuda").reshape(-1)
    Ginv, S = eye[nx * nx:2 * nx * nx].repeat(B), eye.repeat(B)
    grad = torch.linspace(-1.0, 2.0, B * nx, dtype=tt, device="cuda")
    for name, gr in steps:
        for t in outs.values():
            t.zero_()
        outs["gt"][:B * nx] = grad      # what admm_init leaves for w = y = 0
        v = values(null=("C",) + OPTIONAL, N=1, Ginv=P(Ginv), S=P(S), g=P(grad))
        assert step(name, v, gr) == 0, name
        if gr is not None:
            assert graph.value and lib.gbdpcg_graph_launch(graph, s) == 0
        torch.cuda.synchronize()
        if gr is not None:
            lib.gbdpcg_graph_destroy(graph)
            graph.value = None
        assert all(bool(torch.isfinite(outs[k]).all()) for k in WRITTEN), name
        assert float(outs["z"].abs().max()) <= 1e-5 and not bool(outs["w"].any()), name
        assert bool((outs["lam"][:B * nx] + grad).abs().max() <= 1e-5), name
    assert update(values(null=("C",), N=1)) == 0
    torch.cuda.synchronize()
