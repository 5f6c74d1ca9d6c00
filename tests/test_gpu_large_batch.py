"""Every kernel on batches whose arrays pass 4 GiB and 2^32 elements (64-bit strides between problems).

Method (tests/large_batch_ref.py holds the arithmetic, tests/test_large_batch_reference.py checks it on the CPU):
  1. the batch is 7-periodic: 7 base problems from the generator of the kernel's own test, problem b = base problem b mod 7, built on
     the device in chunks of fewer than 2^30 elements (copy_ from an expanded view) and verified against the base with torch.equal;
  2. after the call every output must be 7-periodic bit for bit over the WHOLE batch (integer views, chunk by chunk): a wrapped offset
     lands in a problem of another residue.  Every entry point here passes this comparison exactly at the full batch (the deviation
     between a problem and its twin is 0 everywhere), so no entry point needed a tolerance in its place;
  3. the first 7 and last 7 problems, and every problem that contains a boundary (byte offsets 2^31 .. 2^34, element offsets 2^31,
     2^32) of any array of the call with its two neighbours, go to the host and against the kernel's existing reference at the
     tolerance of its existing test (named where it is copied);
  4. outputs start as NaN and must end finite (the corner blocks L_0, R_{N-1} of Phi^-1 excepted, as everywhere); a 4096-element
     sentinel tail behind every output must survive;
  5. a test computes its memory up front (at most 48 GB), skips only when mem_get_info reports less, frees in `finally`.

Not covered here: admm_lin_* and admm_soc_*; kkt_grad and kkt_backward; the _shared twins (their matrices have stride 0); the graph
forms; the refusal paths (grids above 0x7fffffff, 3 n^2 N >= 2^31), which are read in api_context.hpp and the launchers, not run.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import admm_ref  # noqa: E402
import kkt_refine_ref  # noqa: E402
import large_batch_ref as lb  # noqa: E402
import pinv_ref  # noqa: E402
from gbd_pcg_amd import binding, synth  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
K = lb.K
SENT = 1234.5           # the tail's value


@pytest.fixture
def solver():
    """A handle per test: the split path's workspace (gigabytes here) lives until the handle goes."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def tt(dt):
    return {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.uint8): torch.uint8}[np.dtype(dt)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relerr(a, b):
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def need_memory(nbytes):
    nbytes += lb.SCRATCH_BYTES
    assert nbytes <= lb.CAP_BYTES, f"the case plans {nbytes} bytes, over the cap of {lb.CAP_BYTES}"
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes} bytes of device memory, {free} are free")
    torch.cuda.reset_peak_memory_stats()


def ints(t):
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Arr:
    """One array of the batch: B problems of `stride` elements, for outputs a sentinel tail behind them."""

    def __init__(self, name, B, stride, dt, tail=False):
        self.name, self.B, self.stride, self.es, self.tail = name, B, stride, np.dtype(dt).itemsize, tail
        self.full = torch.empty(B * stride + (lb.TAIL if tail else 0), dtype=tt(dt), device="cuda")
        self.t = self.full[:B * stride]
        if tail:
            self.full[B * stride:] = self.sentinel()
        assert self.t.data_ptr() % 16 == 0

    def sentinel(self):
        return SENT if self.full.is_floating_point() else 0x5a

    def rows(self, lo, hi):
        return self.t[lo * self.stride:hi * self.stride]

    def set(self, value):
        """Every element of the body, in chunks of fewer than 2^30 elements."""
        for lo in range(0, self.t.numel(), lb.CHUNK_ELEMS):
            self.t[lo:lo + lb.CHUNK_ELEMS].fill_(value)
        return self

    def tile(self, base, sample):
        """Problem b <- base[b % 7] (base: device tensor [7, stride]), then the fill is verified on `sample`."""
        assert tuple(base.shape) == (K, self.stride) and base.dtype == self.t.dtype
        for lo, hi in lb.chunks(self.stride, self.B):
            m, rem = divmod(hi - lo, K)
            if m:
                self.rows(lo, lo + m * K).view(m, K, self.stride).copy_(base.unsqueeze(0).expand(m, K, self.stride))
            if rem:
                self.rows(lo + m * K, hi).view(rem, self.stride).copy_(base[:rem])
        for b in sample:
            assert torch.equal(self.rows(b, b + 1), base[b % K]), \
                f"the periodic FILL of {self.name} is wrong at problem {b} (torch copy_, not the kernel under test)"
        return self

    def gather(self, sample):
        return torch.stack([self.rows(b, b + 1) for b in sample]).cpu().numpy()

    def crossed(self):
        return [n for n, _ in lb.crossed(self.stride, self.es, self.B)]

    def where(self, b):
        name = lb.behind(b, self.stride, self.es, self.B)
        if name == "no boundary":
            return f"{self.name}: no boundary"
        return f"{self.name}: {name} (first problem wholly behind it: {lb.first_behind(self.stride, self.es, self.B)[name]})"

    def check_tail(self):
        assert self.tail
        tail = self.full[self.B * self.stride:]
        assert bool((tail == self.sentinel()).all()), f"{self.name}: the {lb.TAIL} elements behind the array were written"

    def check_twins(self, what, arrays=None):
        """out[b] == out[b - 7] bit for bit for every b >= 7.  arrays: every array of the call (the failure message names the boundary
        of each that the first wrong problem lies behind: the wrapped offset may be an input's)."""
        for lo, hi in lb.chunks(self.stride, self.B, first=K):
            a, b = ints(self.rows(lo, hi)), ints(self.rows(lo - K, hi - K))
            if not torch.equal(a, b):
                bad = (a.view(hi - lo, -1) != b.view(hi - lo, -1)).any(dim=1).nonzero()
                first = lo + int(bad[0])
                raise AssertionError(
                    f"{what}: {self.name} of problem {first} differs from problem {first - K} (same inputs); {len(bad)} problems of "
                    f"this chunk differ; problem {first} lies behind: " + "; ".join(
                        x.where(first) for x in [self] + [v for v in (arrays or {}).values() if isinstance(v, Arr) and v is not self]))

    def check_finite(self, what, pinv_shape=None):
        """Every element finite; pinv_shape = (n, N): all but the corner blocks L_0 and R_{N-1}."""
        per = max(lb.FINITE_ELEMS // self.stride, 1)      # (isfinite makes temporaries of the size of its argument)
        for lo in range(0, self.B, per):
            hi = min(lo + per, self.B)
            c = self.rows(lo, hi)
            if pinv_shape:
                n, N = pinv_shape
                c = c.view(hi - lo, N, 3, n * n)
                ok = bool(torch.isfinite(c[:, :, 1]).all()) and bool(torch.isfinite(c[:, 1:, 0]).all()) and \
                    bool(torch.isfinite(c[:, :-1, 2]).all())
            else:
                ok = bool(torch.isfinite(c).all())
            if not ok:
                per = ~torch.isfinite(c.reshape(hi - lo, -1)).all(dim=1) if not pinv_shape else None
                first = lo + int(per.nonzero()[0]) if per is not None else lo
                raise AssertionError(f"{what}: {self.name} holds a non-finite value (not written?) in problem {first} "
                                     f"(chunk {lo}..{hi}), behind {lb.behind(first, self.stride, self.es, self.B)}")


def free(*groups):
    for g in groups:
        if isinstance(g, dict):
            g.clear()
    torch.cuda.empty_cache()


def report(what, t0, **figures):
    torch.cuda.synchronize()
    fig = "  ".join(f"{k} {v}" for k, v in figures.items())
    print(f"[large batch] {what}: peak {torch.cuda.max_memory_allocated() / 1e9:.1f} GB, {time.time() - t0:.1f} s  {fig}")


# ------------------------------------------------------------------------------------------------ solves, SpMV, symmetry test, Phi^-1
def symmetrize(n, N, P):
    """L_{k+1} <- R_k' in storage (tests/test_gpu_shared.py, symmetrize): the host-formula stair is symmetric to rounding only."""
    L, D, R = synth.unpack_bt(n, N, P)
    L = L.copy()
    L[..., 1:, :, :] = np.swapaxes(R[..., :-1, :, :], -1, -2)
    return synth.pack_bt(L, D, R)


def base_problems(n, N, dt, all_symmetric):
    """7 problems of synth.gen_numpy (a = 0.5), Pinv symmetric in storage, a 7-periodic warm start; base problem 3 with one L entry of
    S one ulp off unless all_symmetric."""
    d = synth.gen_numpy(n, N, seed=4100 + 13 * n + N, batch=K, dtype=dt, a=0.5)
    S, P, g = d["S"].copy(), symmetrize(n, N, d["Pinv"]).astype(dt), d["gamma"]
    if not all_symmetric:
        S[3] = lb.unsymmetrize_one(S[3], n, N)
    lam0 = (0.1 * np.random.default_rng(N + n).standard_normal((K, n * N))).astype(dt)
    return dict(S=S, Pinv=P, gamma=g, lam0=lam0)


def solve_tols(dt):
    # test_gpu_cluster.py, test_cluster_one_row_per_lane and check(): relerr(lambda) 1e-6 (fp64 1e-10), r and p within vtol 2e-5
    # (fp64 1e-9) of max |gamma|, equal iteration counts and exit flags
    return (1e-6, 2e-5) if np.dtype(dt) == np.dtype(F32) else (1e-10, 1e-9)


def check_solve(what, out, ob, gamma, sample, ltol, vtol):
    """test_gpu_cluster.check on the sampled problems: problem b against the oracle's solve of base problem b % 7."""
    worst_l = worst_v = 0.0
    for i, b in enumerate(sample):
        q = b % K
        assert out["iters"][i] == int(ob["iters"][q]), (what, "iterations", b, out["iters"][i], int(ob["iters"][q]))
        assert out["flags"][i] == int(ob["max_iter_exit"][q]), (what, "max_iter_exit", b)
        scale = np.abs(gamma[q]).max()
        el = relerr(out["lambda"][i], ob["lambda_"][q])
        ev = max(np.abs(out["r"][i] - ob["r"][q]).max(), np.abs(out["p"][i] - ob["p"][q]).max()) / scale
        worst_l, worst_v = max(worst_l, el), max(worst_v, ev)
        assert el < ltol, (what, "lambda", b, el, ltol)
        assert ev < vtol, (what, "r / p", b, ev, vtol)
    return f"relerr(lambda) {worst_l:.2e} (tol {ltol:.0e}), r/p {worst_v:.2e} (tol {vtol:.0e})"


SOLVES = [
    # id, case of large_batch_ref, n, N, dtype, symmetric mode, forced path, family, identity-preconditioner solve too
    ("resident_sym-verify", "resident_sym-14x128-f32", 14, 128, F32, 2, binding.PATH_AUTO, "resident_sym", True),
    ("resident_sym-plain", "resident_sym-14x128-f32", 14, 128, F32, 1, binding.PATH_AUTO, "resident_sym", False),
    ("cluster2", "resident_sym-14x128-f32", 14, 128, F32, 0, binding.PATH_AUTO, "cluster", False),
    ("resident", "resident-14x64-f32", 14, 64, F32, 2, binding.PATH_AUTO, "resident", False),
    ("fused-n20", "fused-20x64-f32", 20, 64, F32, 2, binding.PATH_AUTO, "fused", False),
    ("fused-runtime-n37", "fused-runtime-37x16-f32", 37, 16, F32, 2, binding.PATH_FUSED, "fused", False),
    ("split", "split-14x128-f32", 14, 128, F32, 2, binding.PATH_SPLIT, "split", False),
    ("cluster4-f64", "cluster4-14x128-f64", 14, 128, F64, 2, binding.PATH_AUTO, "cluster", True),
    ("auto-36x256-f64", "auto-36x256-f64", 36, 256, F64, 2, binding.PATH_AUTO, "auto", False),
]


def confirm_family(solver, n, N, dt, B, mode, path, family):
    """What the API tells (choose_path, cluster_members); elsewhere the rule of tests/test_gpu_shared.py, family()."""
    es = np.dtype(dt).itemsize
    chosen = solver.choose_path(es, n, N, B)
    members = solver.cluster_members(es, n, N)
    if family == "split":
        assert chosen == binding.PATH_SPLIT
    elif family == "auto":
        assert chosen in (binding.PATH_SPLIT, binding.PATH_PERSISTENT), chosen
        print(f"[large batch] AUTO at ({n}, {N}) fp64, batch {B}: path {chosen} (2 = split; the batch is far beyond persistent slices)")
    else:
        assert chosen == binding.PATH_FUSED
        if family == "cluster":
            assert members == (2 if es == 4 else 4)
        elif family == "resident_sym":
            # test_gpu_shared.family: (14, fp32), N <= 128, Pinv given, 8-byte aligned, mode 1 or (mode 2 and more than one cluster round)
            assert (n, es) == (14, 4) and N <= 128 and mode in (1, 2) and B * members > torch.cuda.get_device_properties(0).multi_processor_count
        elif family == "resident":
            assert members == 0 and n <= 15       # pcg_resident.hip holds the horizon in one workgroup
        else:
            assert members == 0 and n > 15        # general or symmetric streaming (pcg_fused.hip)
    return chosen


@pytest.mark.parametrize("sid,cname,n,N,dt,mode,path,family,identity", SOLVES, ids=[s[0] for s in SOLVES])
def test_solve(solver, orc, sid, cname, n, N, dt, mode, path, family, identity):
    """To tol 1e-6 from lambda = 0, five iterations from a 7-periodic warm start, (two rows) four iterations without Phi^-1; r and p
    requested everywhere.  In mode 2 every seventh problem fails the symmetry test and takes the general route.
    AUTO at (36, 256) fp64, batch 2160: the split path (choose_path says so; 1080 persistent slices are no option)."""
    c = lb.case(cname)
    B, es, stride, vlen = c.B, np.dtype(dt).itemsize, lb.bt(n, N), n * N
    assert B * stride > (1 << 32 if es == 4 else 1 << 31) and B * stride * es > 1 << 34
    base = base_problems(n, N, dt, all_symmetric=(mode == 1))
    ltol, vtol = solve_tols(dt)
    sample = lb.sample_union([(stride, es), (vlen, es)], B)
    t0, a = time.time(), {}
    solver.set_path(path)
    solver.set_symmetric(mode)
    try:
        chosen = confirm_family(solver, n, N, dt, B, mode, path, family)
        ws = solver.lib.gbdpcg_workspace_bytes(solver.h, es, n, N, B) if chosen == binding.PATH_SPLIT else 0
        if family == "split":
            # 6 vectors and 3 N partials per problem (csrc/pcg_split.hip, SplitWs): 2.5 GB here -- past 2^31 bytes, short of 2^32
            assert ws > 1 << 31, ws
            print(f"[large batch] split workspace of the handle: {ws} bytes")
        assert ws <= c.extra_bytes, (ws, c.extra_bytes)
        need_memory(lb.case_bytes(c))
        a["S"] = Arr("S", B, stride, dt).tile(dev(base["S"]), sample)
        a["P"] = Arr("Pinv", B, stride, dt).tile(dev(base["Pinv"]), sample)
        a["g"] = Arr("gamma", B, vlen, dt).tile(dev(base["gamma"]), sample)
        a["l0"] = Arr("lambda0", B, vlen, dt).tile(dev(base["lam0"]), sample)
        for k in ("lam", "r", "p"):
            a[k] = Arr({"lam": "lambda"}.get(k, k), B, vlen, dt, tail=True)
        a["it"], a["fl"] = Arr("iters", B, 1, np.int32, tail=True), Arr("max_iter_exit", B, 1, np.uint8, tail=True)
        assert a["S"].crossed() == c.claims["S"] and a["P"].crossed() == c.claims["Pinv"]
        runs = [("tol 1e-6", True, None, 1e-6, 100, ltol, vtol),
                # (the warm start: test_cluster_one_row_per_lane allows 2 ltol; the bound here is the tighter one)
                ("5 iterations, warm", True, base["lam0"], 0.0, 5, ltol, vtol)]
        if identity:
            runs.append(("4 iterations, no Pinv", False, base["lam0"], 0.0, 4, ltol, vtol))
        figures = {}
        for name, with_p, lam0, tol, max_iter, lt, vt in runs:
            what = f"{sid} {name}"
            ob = orc.pcg_batch(n, N, K, base["S"], base["Pinv"] if with_p else None, base["gamma"], lambda0=lam0, tol=tol,
                               max_iter=max_iter, nthreads=8)
            if lam0 is None:
                a["lam"].set(0.0)
            else:
                a["lam"].t.copy_(a["l0"].t)
            a["r"].set(float("nan")), a["p"].set(float("nan")), a["it"].set(0x7f7f7f7f), a["fl"].set(0x7f)
            solver.solve(n, N, B, a["S"].t, a["P"].t if with_p else None, a["g"].t, a["lam"].t, a["r"].t, a["p"].t, tol=tol,
                         max_iter=max_iter, iters=a["it"].t, max_iter_exit=a["fl"].t)
            torch.cuda.synchronize()
            for k in ("lam", "r", "p", "it", "fl"):
                a[k].check_tail()
                a[k].check_twins(what, a)
            for k in ("lam", "r", "p"):
                a[k].check_finite(what)
            assert bool((a["it"].t != 0x7f7f7f7f).all()) and bool((a["fl"].t <= 1).all()), f"{what}: iters / max_iter_exit not written"
            out = dict(iters=a["it"].gather(sample).ravel(), flags=a["fl"].gather(sample).ravel(), r=a["r"].gather(sample),
                       p=a["p"].gather(sample), **{"lambda": a["lam"].gather(sample)})
            figures[name] = check_solve(what, out, ob, base["gamma"], sample, lt, vt)
        report(f"solve {sid} B {B} path {chosen} S crosses {a['S'].crossed()}", t0, **figures)
    finally:
        solver.set_path(binding.PATH_AUTO)
        solver.set_symmetric(2)
        free(a)


SHAPES = [("14x128-f32", "resident_sym-14x128-f32", 14, 128, F32), ("14x128-f64", "cluster4-14x128-f64", 14, 128, F64)]
shapes = pytest.mark.parametrize("cname,n,N,dt", [s[1:] for s in SHAPES], ids=[s[0] for s in SHAPES])


@shapes
@pytest.mark.parametrize("sym", [0, 1], ids=["general", "symmetric"])
def test_spmv(solver, orc, cname, n, N, dt, sym):
    """y = S x in general storage (set_symmetric(0)) and from [D|R] alone (set_symmetric(1), an all-symmetric base)."""
    c = lb.case(cname)
    B, es, stride, vlen = c.B, np.dtype(dt).itemsize, lb.bt(n, N), n * N
    base = base_problems(n, N, dt, all_symmetric=bool(sym))
    x = np.stack([synth.normals(60 + q, 0, vlen) for q in range(K)]).astype(dt)
    want = orc.spmv(n, N, base["S"], x, batch=K, nthreads=8).reshape(K, -1)
    sample = lb.sample_union([(stride, es), (vlen, es)], B)
    t0, a = time.time(), {}
    solver.set_symmetric(sym)
    try:
        need_memory((B * stride + 2 * B * vlen + lb.TAIL) * es)
        a["S"] = Arr("S", B, stride, dt).tile(dev(base["S"]), sample)
        a["x"] = Arr("x", B, vlen, dt).tile(dev(x), sample)
        a["y"] = Arr("y", B, vlen, dt, tail=True).set(float("nan"))
        assert a["S"].crossed() == c.claims["S"]
        what = f"spmv {'symmetric' if sym else 'general'} {cname}"
        solver.spmv(n, N, B, a["S"].t, a["x"].t, a["y"].t)
        torch.cuda.synchronize()
        a["y"].check_tail(), a["y"].check_twins(what, a), a["y"].check_finite(what)
        y = a["y"].gather(sample)
        tol = 1e-13 if es == 8 else 1e-6     # test_gpu_parity.py, test_spmv_vs_oracle_and_dense / test_symmetric_spmv (F32_TOL)
        worst = max(relerr(y[i], want[b % K]) for i, b in enumerate(sample))
        assert worst < tol, (what, worst, tol)
        report(f"{what} B {B} S crosses {a['S'].crossed()}", t0, relerr=f"{worst:.2e} (tol {tol:.0e})")
    finally:
        solver.set_symmetric(2)
        free(a)


@shapes
def test_check_symmetric(solver, cname, n, N, dt):
    """Flags exact: 0 where b mod 7 == 3 (one L entry one ulp off), 1 elsewhere."""
    c = lb.case(cname)
    B, es, stride = c.B, np.dtype(dt).itemsize, lb.bt(n, N)
    base = base_problems(n, N, dt, all_symmetric=False)
    sample = lb.boundary_problems(stride, es, B)
    t0, a = time.time(), {}
    try:
        need_memory(B * stride * es + B + lb.TAIL)
        a["S"] = Arr("S", B, stride, dt).tile(dev(base["S"]), sample)
        a["f"] = Arr("flags", B, 1, np.uint8, tail=True).set(0x7f)
        solver.check_symmetric(n, N, B, a["S"].t, flags=a["f"].t)
        torch.cuda.synchronize()
        a["f"].check_tail()
        want = (torch.arange(B, device="cuda") % K != 3).to(torch.uint8)
        if not torch.equal(a["f"].t, want):
            first = int((a["f"].t != want).nonzero()[0])
            raise AssertionError(f"check_symmetric {cname}: flag of problem {first} is {int(a['f'].t[first])}, behind "
                                 f"{lb.behind(first, stride, es, B)} of S")
        report(f"check_symmetric {cname} B {B} S crosses {a['S'].crossed()}", t0, flags="exact")
    finally:
        free(a)


KINDS = [("stair", binding.PINV_STAIR, pinv_ref.STAIR), ("jacobi", binding.PINV_BLOCK_JACOBI, pinv_ref.JACOBI),
         ("identity", binding.PINV_IDENTITY, pinv_ref.IDENTITY)]


@shapes
def test_form_pinv_and_form_pinv_solve(solver, cname, n, N, dt):
    """The three kinds against tests/pinv_ref.py (fp64 formulas), then form_pinv_solve against the two calls bit for bit on the whole
    batch: Phi^-1 of the two calls is 7-periodic (checked), so its first 7 problems stand for all of it."""
    c = lb.case(cname)
    B, es, stride, vlen = c.B, np.dtype(dt).itemsize, lb.bt(n, N), n * N
    base = base_problems(n, N, dt, all_symmetric=False)
    sample = lb.sample_union([(stride, es), (vlen, es)], B)
    tol = 1e-12 if es == 8 else 1e-5        # test_gpu_parity.py, test_form_pinv
    t0, a, figures = time.time(), {}, {}
    try:
        need_memory(lb.case_bytes(c))
        a["S"] = Arr("S", B, stride, dt).tile(dev(base["S"]), sample)
        a["P"] = Arr("Pinv", B, stride, dt, tail=True)
        assert a["P"].crossed() == c.claims["Pinv"]
        for name, code, rkind in KINDS:
            what = f"form_pinv {name} {cname}"
            a["P"].set(float("nan"))
            solver.form_pinv(n, N, B, a["S"].t, code, Pinv=a["P"].t)
            torch.cuda.synchronize()
            a["P"].check_tail(), a["P"].check_twins(what, a), a["P"].check_finite(what, pinv_shape=(n, N))
            want = pinv_ref.reference(n, N, base["S"], rkind).reshape(K, N, 3, n * n)
            got = a["P"].gather(sample).reshape(len(sample), N, 3, n * n).copy()
            got[:, 0, 0], got[:, -1, 2] = 0, 0          # the never-read corner slots are unspecified (test_form_pinv)
            worst = max(relerr(got[i], want[b % K]) for i, b in enumerate(sample))
            assert worst < tol, (what, worst, tol)
            figures[name] = f"{worst:.2e} (tol {tol:.0e})"
        # form_pinv_solve == form_pinv, then solve
        a["g"] = Arr("gamma", B, vlen, dt).tile(dev(base["gamma"]), sample)
        for k in ("lam", "lam2"):
            a[k] = Arr("lambda", B, vlen, dt, tail=True).set(0.0)
        for k in ("it", "it2"):
            a[k] = Arr("iters", B, 1, np.int32, tail=True).set(0x7f7f7f7f)
        a["P"].set(float("nan"))
        solver.form_pinv(n, N, B, a["S"].t, binding.PINV_STAIR, Pinv=a["P"].t)
        solver.solve(n, N, B, a["S"].t, a["P"].t, a["g"].t, a["lam"].t, tol=1e-6, max_iter=100, iters=a["it"].t)
        torch.cuda.synchronize()
        a["P"].check_twins("form_pinv before the solve")
        period = a["P"].rows(0, K).view(K, stride).clone()
        a["P"].set(float("nan"))
        solver.form_pinv_solve(n, N, B, a["S"].t, a["P"].t, a["g"].t, a["lam2"].t, kind=binding.PINV_STAIR, tol=1e-6, max_iter=100,
                               iters=a["it2"].t)
        torch.cuda.synchronize()
        what = f"form_pinv_solve {cname}"
        for lo, hi in lb.chunks(stride, B):
            m, rem = divmod(hi - lo, K)
            ok = torch.equal(ints(a["P"].rows(lo, lo + m * K)).view(m, K, -1), ints(period).unsqueeze(0).expand(m, K, -1)) and \
                (not rem or torch.equal(ints(a["P"].rows(lo + m * K, hi)).view(rem, -1), ints(period)[:rem]))
            assert ok, f"{what}: Pinv differs from form_pinv's in problems {lo}..{hi}, behind {lb.behind(hi - 1, stride, es, B)}"
        for k in ("P", "lam2", "it2"):
            a[k].check_tail()
        assert torch.equal(ints(a["lam2"].t), ints(a["lam"].t)), f"{what}: lambda differs from the two calls"
        assert torch.equal(a["it2"].t, a["it"].t) and bool((a["it"].t != 0x7f7f7f7f).all()), f"{what}: iters differ from the two calls"
        a["lam2"].check_twins(what, a), a["lam2"].check_finite(what)
        report(f"form_pinv + form_pinv_solve {cname} B {B} Pinv crosses {a['P'].crossed()}", t0, **figures)
    finally:
        free(a)


# ------------------------------------------------------------------------------------------------------------------- the KKT side
NX, NU, NK = 14, 7, 128


def close_err(a, b):
    """The figure of tests/test_gpu_schur.py, close(): max |a - b| / max |b|."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def kkt_base(dt):
    d = so.gen(NX, NU, NK, seed=100 + NX + NK, batch=K, dtype=dt)
    rng = np.random.default_rng(5)
    d["lam"] = rng.standard_normal((K, NX * NK)).astype(dt)
    d["z"] = rng.standard_normal((K, lb.NZ)).astype(dt)
    d["rho"] = (0.5 * (np.arange(K) + 1.0)).astype(dt)          # tests/test_gpu_reg.py, rho_default
    return d


def residual_reference(d):
    """tests/test_gpu_kkt_residual.py, evaluate(): the two norms in fp64 and the magnitudes their bounds scale with."""
    ref, mag = np.zeros((K, 2)), np.zeros((K, 2))
    for q in range(K):
        Gd, Cd, g, c = so.dense_kkt(NX, NU, NK, d["G"][q], d["C"][q], d["g"][q], d["c"][q])
        zb, lb_ = np.asarray(d["z"][q], F64), np.asarray(d["lam"][q], F64)
        ref[q] = np.abs(Gd @ zb + g + Cd.T @ lb_).max(), np.abs(Cd @ zb - c).max()
        aC = np.abs(Cd)
        mag[q] = (np.abs(Gd) @ np.abs(zb) + np.abs(g) + aC.T @ np.abs(lb_)).max(), (aC @ np.abs(zb) + np.abs(c)).max()
    return ref, mag


def check_residual(what, res, sample, ref, mag, dt):
    """tests/test_gpu_kkt_residual.py, within_bounds(): (2 nx + 2) u and (nx + nu + 2) u times the magnitudes."""
    u = 2.0 ** -24 if np.dtype(dt) == np.dtype(F32) else 2.0 ** -53
    worst = 0.0
    for i, b in enumerate(sample):
        q = b % K
        err = np.abs(np.asarray(res[i], F64) - ref[q])
        tol = np.array([(2 * NX + 2) * u * mag[q, 0], (NX + NU + 2) * u * mag[q, 1]])
        assert np.isfinite(res[i]).all() and (err <= tol).all(), (what, b, err, tol)
        worst = max(worst, (err / tol).max())
    return f"worst error / bound {worst:.3f}"


def test_kkt_side_fp32(solver, monkeypatch):
    """form_schur, form_schur_reg (7-periodic rho), recover_primal, form_gamma, kkt_residual at B 57100: S passes 2^32 elements; G, G^-1
    (7.2 GB) and C (8.5 GB) pass 2^32 bytes and stay below 2^33 bytes = 2^31 elements.  Then the any-size kernels
    (GBDPCG_SCHUR_GENERAL=1) on the same batch."""
    dt, c = F32, lb.case("kkt-14x7x128-f32")
    B, z = c.B, lb.kkt_sizes(NX, NU, NK)
    d = kkt_base(dt)
    tol = 2e-4                              # tests/test_gpu_schur.py, test_form_schur_and_recover_vs_oracle (fp32); z: 10 tol
    parts = [so.form_schur(NX, NU, NK, d["G"][q], d["C"][q], d["g"][q], d["c"][q]) for q in range(K)]
    Gr = np.array(d["G"], F64)
    sg = NX * NX + NU * NU
    diag = np.array([k * sg + i * (NX + 1) for k in range(NK) for i in range(NX)] +
                    [k * sg + NX * NX + i * (NU + 1) for k in range(NK - 1) for i in range(NU)])
    Gr[:, diag] += d["rho"].astype(F64)[:, None]                # tests/test_gpu_reg.py, add_rho
    parts_reg = [so.form_schur(NX, NU, NK, Gr[q], d["C"][q], d["g"][q], d["c"][q]) for q in range(K)]
    zref = [so.recover_primal(NX, NU, NK, d["G"][q], d["C"][q], d["g"][q], d["lam"][q]) for q in range(K)]
    rref, rmag = residual_reference(d)
    sample = lb.sample_union([(z[k], 4) for k in ("S", "G", "C", "g", "c")], B)
    t0, a, figures = time.time(), {}, {}
    try:
        need_memory(lb.case_bytes(c))
        for k, name in (("G", "G"), ("C", "C"), ("g", "g"), ("c", "c")):
            a[k] = Arr(name, B, z[name], dt).tile(dev(d[name]), sample)
        a["lam"] = Arr("lambda", B, z["c"], dt).tile(dev(d["lam"]), sample)
        a["zin"] = Arr("z", B, z["g"], dt).tile(dev(d["z"]), sample)
        a["rho"] = Arr("rho", B, 1, dt).tile(dev(d["rho"].reshape(K, 1)), sample)
        a["Gi"] = Arr("Ginv", B, z["G"], dt, tail=True)
        a["gam"] = Arr("gamma", B, z["c"], dt, tail=True)
        a["zout"] = Arr("z", B, z["g"], dt, tail=True)
        a["res"] = Arr("res", B, 2, dt, tail=True)
        for k in ("G", "C", "Gi"):
            assert a[k].crossed() == c.claims[a[k].name], (k, a[k].crossed())
        for general in (False, True):
            if general:
                monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
            tag = "general" if general else "default"
            a["S"] = Arr("S", B, z["S"], dt, tail=True)
            assert a["S"].crossed() == c.claims["S"]
            for reg, pp in ((True, parts_reg), (False, parts)):      # (the plain form last: its G^-1 and gamma are used below)
                what = f"form_schur{'_reg' if reg else ''} {tag}"
                for k in ("S", "gam", "Gi"):
                    a[k].set(float("nan"))
                if reg:
                    solver.form_schur_reg(NX, NU, NK, B, a["G"].t, a["C"].t, a["g"].t, a["c"].t, a["rho"].t, S=a["S"].t, gamma=a["gam"].t,
                                          Ginv=a["Gi"].t)
                else:
                    solver.form_schur(NX, NU, NK, B, a["G"].t, a["C"].t, a["g"].t, a["c"].t, S=a["S"].t, gamma=a["gam"].t, Ginv=a["Gi"].t)
                torch.cuda.synchronize()
                worst = 0.0
                for k, j in (("S", 0), ("gam", 1), ("Gi", 2)):
                    a[k].check_tail(), a[k].check_twins(what, a), a[k].check_finite(what)
                    got = a[k].gather(sample)
                    worst = max(worst, max(close_err(got[i], pp[b % K][j]) for i, b in enumerate(sample)))
                assert worst <= tol, (what, worst, tol)
                figures[what] = f"{worst:.2e} (tol {tol:.0e})"
            a.pop("S")                      # the calls below do not read S: stay under the cap
            torch.cuda.empty_cache()
            what = f"recover_primal {tag}"
            a["zout"].set(float("nan"))
            solver.recover_primal(NX, NU, NK, B, a["Gi"].t, a["C"].t, a["g"].t, a["lam"].t, z=a["zout"].t)
            torch.cuda.synchronize()
            a["zout"].check_tail(), a["zout"].check_twins(what, a), a["zout"].check_finite(what)
            got = a["zout"].gather(sample)
            worst = max(close_err(got[i], zref[b % K]) for i, b in enumerate(sample))
            assert worst <= 10 * tol, (what, worst)
            figures[what] = f"{worst:.2e} (tol {10 * tol:.0e})"
            what = f"form_gamma {tag}"
            a["gam"].set(float("nan"))
            solver.form_gamma(NX, NU, NK, B, a["Gi"].t, a["C"].t, a["g"].t, a["c"].t, gamma=a["gam"].t)
            torch.cuda.synchronize()
            a["gam"].check_tail(), a["gam"].check_twins(what, a), a["gam"].check_finite(what)
            got = a["gam"].gather(sample)
            worst = max(close_err(got[i], parts[b % K][1]) for i, b in enumerate(sample))
            assert worst <= tol, (what, worst)       # tests/test_gpu_resolve.py holds form_gamma to the formation tolerance
            figures[what] = f"{worst:.2e} (tol {tol:.0e})"
            what = f"kkt_residual {tag}"
            a["res"].set(float("nan"))
            solver.kkt_residual(NX, NU, NK, B, a["G"].t, a["C"].t, a["g"].t, a["c"].t, a["zin"].t, a["lam"].t, res=a["res"].t)
            torch.cuda.synchronize()
            a["res"].check_tail(), a["res"].check_twins(what, a), a["res"].check_finite(what)
            figures[what] = check_residual(what, a["res"].gather(sample), sample, rref, rmag, dt)
        report(f"KKT side fp32 B {B} S crosses {c.claims['S']}, G / C / Ginv cross {c.claims['G']}", t0, **figures)
    finally:
        free(a)


def test_kkt_side_fp64(solver, monkeypatch):
    """kkt_residual and kkt_defect_mixed in fp64 at B 28600 (G 7.2 GB, C 8.5 GB: past 2^32 bytes), default and any-size kernels."""
    dt, c = F64, lb.case("kkt-14x7x128-f64")
    B, z = c.B, lb.kkt_sizes(NX, NU, NK)
    d = kkt_base(dt)
    rref, rmag = residual_reference(d)
    dref = [kkt_refine_ref.defect_mixed_ref(NX, NU, NK, d["G"][q], d["C"][q], d["g"][q], d["c"][q], d["z"][q], d["lam"][q]) for q in range(K)]
    sample = lb.sample_union([(z[k], 8) for k in ("G", "C", "g", "c")], B)
    t0, a, figures = time.time(), {}, {}
    try:
        need_memory(lb.case_bytes(c))
        for k in ("G", "C", "g", "c"):
            a[k] = Arr(k, B, z[k], dt).tile(dev(d[k]), sample)
            if k in c.claims:
                assert a[k].crossed() == c.claims[k], (k, a[k].crossed())
        a["lam"] = Arr("lambda", B, z["c"], dt).tile(dev(d["lam"]), sample)
        a["z"] = Arr("z", B, z["g"], dt).tile(dev(d["z"]), sample)
        a["res"], a["res2"] = Arr("res", B, 2, dt, tail=True), Arr("res", B, 2, dt, tail=True)
        a["rg"], a["rc"], a["dl"] = (Arr(n_, B, z[s_], F32, tail=True) for n_, s_ in (("rg", "g"), ("rc", "c"), ("dlambda", "c")))
        a["expo"] = Arr("expo", B, 1, np.int32, tail=True)
        for general in (False, True):
            if general:
                monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
            tag = "general" if general else "default"
            what = f"kkt_residual fp64 {tag}"
            a["res"].set(float("nan"))
            solver.kkt_residual(NX, NU, NK, B, a["G"].t, a["C"].t, a["g"].t, a["c"].t, a["z"].t, a["lam"].t, res=a["res"].t)
            torch.cuda.synchronize()
            a["res"].check_tail(), a["res"].check_twins(what, a), a["res"].check_finite(what)
            figures[what] = check_residual(what, a["res"].gather(sample), sample, rref, rmag, dt)
            what = f"kkt_defect_mixed {tag}"
            for k in ("res2", "rg", "rc", "dl"):
                a[k].set(float("nan"))
            a["expo"].set(12345)
            solver.kkt_defect_mixed(NX, NU, NK, B, a["G"].t, a["C"].t, a["g"].t, a["c"].t, a["z"].t, a["lam"].t, rg=a["rg"].t, rc=a["rc"].t,
                                    dlam=a["dl"].t, expo=a["expo"].t, res=a["res2"].t)
            torch.cuda.synchronize()
            for k in ("res2", "rg", "rc", "dl", "expo"):
                a[k].check_tail(), a[k].check_twins(what, a)
            for k in ("res2", "rg", "rc"):
                a[k].check_finite(what)
            assert not bool(ints(a["dl"].t).any()), f"{what}: dlambda is not +0 everywhere"
            # tests/test_gpu_kkt_refine.py, test_defect_bits: res is gbdpcg_kkt_residual_f64's bit for bit; rg, rc, expo are the reference's bits
            assert torch.equal(ints(a["res2"].t), ints(a["res"].t)), f"{what}: res differs from kkt_residual's"
            rg, rc, ex = a["rg"].gather(sample), a["rc"].gather(sample), a["expo"].gather(sample).ravel()
            for i, b in enumerate(sample):
                wrg, wrc, we, _ = dref[b % K]
                assert ex[i] == we and np.array_equal(rg[i].view(np.uint32), np.asarray(wrg, F32).view(np.uint32)) and \
                    np.array_equal(rc[i].view(np.uint32), np.asarray(wrc, F32).view(np.uint32)), (what, b)
            figures[what] = "bits equal"
        report(f"KKT side fp64 B {B} G / C cross {c.claims['G']}", t0, **figures)
    finally:
        free(a)


# ------------------------------------------------------------------------------------------------------------ element-wise kernels
def test_admm_update_and_init(solver):
    """fp64, (14, 7, 128), B 200400: each of the seven arrays passes 2^32 bytes.  w, y, res bit for bit against tests/admm_ref.py, gt
    within one rounding of the exact g - rho t (tests/test_gpu_admm.py, test_update_and_init_vs_reference and check_gt)."""
    from fractions import Fraction
    dt, c = F64, lb.ADMM_CASE
    B, nz = c.B, lb.NZ
    rng = np.random.default_rng(1000 + nz)                       # tests/test_gpu_admm.py, update_data
    zz, w, y, g = (rng.standard_normal((K, nz)).astype(dt) for _ in range(4))
    lo = (-0.3 + 0.05 * rng.standard_normal((K, nz))).astype(dt)
    hi = (0.3 + 0.05 * rng.standard_normal((K, nz))).astype(dt)
    lo[rng.random((K, nz)) < 1.0 / 3.0] = -np.inf
    hi[rng.random((K, nz)) < 1.0 / 3.0] = np.inf
    rho = rng.uniform(0.5, 4.0, K).astype(dt)
    sample = lb.boundary_problems(nz, 8, B)
    t0, a = time.time(), {}
    try:
        need_memory(lb.case_bytes(c) + 40 * B)
        for k, v in (("g", g), ("lo", lo), ("hi", hi), ("z", zz)):
            a[k] = Arr(k, B, nz, dt).tile(dev(v), sample)
            assert a[k].crossed() == c.claims[k]
        a["rho"] = Arr("rho", B, 1, dt).tile(dev(rho.reshape(K, 1)), sample)
        for k in ("w", "y", "gt"):
            a[k] = Arr(k, B, nz, dt, tail=True)
        a["res"] = Arr("res", B, 2, dt, tail=True)
        for init in (False, True):
            what = "admm_init" if init else "admm_update"
            wr, yr, tr, gr, rr = admm_ref.update_ref(dt, g, lo, hi, rho, None if init else zz, w, y)
            a["w"].tile(dev(w), sample), a["y"].tile(dev(y), sample), a["gt"].set(float("nan")), a["res"].set(float("nan"))
            if init:
                solver.admm_init(NX, NU, NK, B, a["g"].t, a["lo"].t, a["hi"].t, a["rho"].t, a["w"].t, a["y"].t, gt=a["gt"].t)
            else:
                solver.admm_update(NX, NU, NK, B, a["g"].t, a["lo"].t, a["hi"].t, a["rho"].t, a["z"].t, a["w"].t, a["y"].t, a["gt"].t,
                                   res=a["res"].t)
            torch.cuda.synchronize()
            for k in ("w", "y", "gt") + (() if init else ("res",)):
                a[k].check_tail(), a[k].check_twins(what, a), a[k].check_finite(what)
            gw, gy, ggt, gres = (a[k].gather(sample) for k in ("w", "y", "gt", "res"))
            u = Fraction(2.0 ** -53)
            for i, b in enumerate(sample):
                q = b % K
                assert np.array_equal(gw[i].view(np.uint64), wr[q].view(np.uint64)), (what, "w", b)
                assert np.array_equal(gy[i].view(np.uint64), yr[q].view(np.uint64)), (what, "y", b)
                if not init:
                    assert np.array_equal(gres[i].view(np.uint64), rr[q].view(np.uint64)), (what, "res", b)
                if i < K:       # (exact rationals: the first period; the twins of these problems are compared bit for bit above)
                    r = Fraction(float(rho[q]))
                    for j in range(nz):
                        ref = gr[q, j]
                        err, bound = abs(Fraction(float(ggt[i, j])) - ref), u * (abs(r * Fraction(float(tr[q, j]))) + abs(ref))
                        assert err <= bound, (what, "gt", b, j)
        report(f"admm_update + admm_init B {B}, every array crosses {c.claims['g']}", t0, result="bits equal")
    finally:
        free(a)


def test_kkt_refine_apply(solver):
    """z += ldexp(dz, -e_b), lambda += ldexp(dlambda, -e_b) at B 200400 (z passes 2^32 bytes): the bits of tests/kkt_refine_ref.py,
    apply_ref (tests/test_gpu_kkt_refine.py, test_apply_bits)."""
    c = lb.APPLY_CASE
    B, nz, nl = c.B, lb.NZ, NX * NK
    rng = np.random.default_rng(77)
    z0, l0 = rng.standard_normal((K, nz)), rng.standard_normal((K, nl))
    dz, dl = rng.standard_normal((K, nz)).astype(F32), rng.standard_normal((K, nl)).astype(F32)
    expo = np.array([0, 3, -2, 17, 40, -9, 1], np.int32)
    sample = lb.sample_union([(nz, 8), (nl, 8)], B)
    t0, a = time.time(), {}
    try:
        need_memory(lb.case_bytes(c))
        a["z"] = Arr("z", B, nz, F64, tail=True).tile(dev(z0), sample)
        a["l"] = Arr("lambda", B, nl, F64, tail=True).tile(dev(l0), sample)
        a["dz"] = Arr("dz", B, nz, F32).tile(dev(dz), sample)
        a["dl"] = Arr("dlambda", B, nl, F32).tile(dev(dl), sample)
        a["e"] = Arr("expo", B, 1, np.int32).tile(dev(expo.reshape(K, 1)), sample)
        assert a["z"].crossed() == c.claims["z"]
        solver.kkt_refine_apply(NX, NU, NK, B, a["dz"].t, a["dl"].t, a["e"].t, a["z"].t, a["l"].t)
        torch.cuda.synchronize()
        for k in ("z", "l"):
            a[k].check_tail(), a[k].check_twins("kkt_refine_apply", a), a[k].check_finite("kkt_refine_apply")
        gz, gl = a["z"].gather(sample), a["l"].gather(sample)
        for i, b in enumerate(sample):
            q = b % K
            assert np.array_equal(gz[i].view(np.uint64), kkt_refine_ref.apply_ref(z0[q], dz[q], expo[q]).view(np.uint64)), ("z", b)
            assert np.array_equal(gl[i].view(np.uint64), kkt_refine_ref.apply_ref(l0[q], dl[q], expo[q]).view(np.uint64)), ("lambda", b)
        report(f"kkt_refine_apply B {B} z crosses {a['z'].crossed()}", t0, result="bits equal")
    finally:
        free(a)


def test_demote(solver):
    """count = 2^31 + 2^30 + 12345: the source passes 2^31 elements and 2^34 bytes; the destination equals torch's rounding."""
    count = lb.DEMOTE_COUNT
    t0, a = time.time(), {}
    try:
        need_memory(lb.case_bytes(lb.DEMOTE_CASE) + 4 * lb.CHUNK_ELEMS)     # (the rounded chunk torch makes for the comparison)
        a["src"] = torch.empty(count, dtype=torch.float64, device="cuda")
        a["dst"] = torch.empty(count + lb.TAIL, dtype=torch.float32, device="cuda")
        a["dst"][count:] = SENT
        gen = torch.Generator(device="cuda").manual_seed(5)
        for lo in range(0, count, lb.CHUNK_ELEMS):
            hi = min(lo + lb.CHUNK_ELEMS, count)
            part = a["src"][lo:hi]
            part.normal_(generator=gen)
            part.mul_(1.0 + 1e-9 * (lo // lb.CHUNK_ELEMS))         # no two chunks alike
            a["dst"][lo:hi].fill_(float("nan"))
        solver.demote(a["src"], a["dst"][:count])
        torch.cuda.synchronize()
        assert bool((a["dst"][count:] == SENT).all()), "demote wrote behind its destination"
        for lo in range(0, count, lb.CHUNK_ELEMS):
            hi = min(lo + lb.CHUNK_ELEMS, count)
            want = a["src"][lo:hi].to(torch.float32)
            got = a["dst"][lo:hi]
            if not torch.equal(ints(got), ints(want)):
                first = lo + int((ints(got) != ints(want)).nonzero()[0])
                raise AssertionError(f"demote: element {first} (byte {8 * first} of the source) is {float(got[first - lo])}, "
                                     f"want {float(want[first - lo])}")
            del want
        report(f"demote count {count}", t0, result="bits equal")
    finally:
        free(a)
