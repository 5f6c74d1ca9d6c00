"""Shared-matrix batches on the device: ONE S, Phi^-1 (G^-1, C) for `batch` right-hand sides, through the C ABI
(gbdpcg_solve_shared_*, gbdpcg_form_gamma_shared_*, gbdpcg_recover_primal_shared_*, gbdpcg_kkt_resolve_shared_* and the graph forms).

The reference of every bit-identity check is the per-problem twin on `batch` copies of the single matrices, same handle, same
symmetric mode, path set to GBDPCG_PATH_FUSED (include/gbdpcg.h).  The oracle comparisons hand the same single matrix to
oracle/ once per problem, at the project's tolerances: fp32 1e-6 / fp64 1e-10 norm-wise at equal iteration counts for the
solve (tests/test_gpu_parity.py), 2e-4 / 1e-11 of the largest entry for gamma and 3e-4 / 1e-9 norm-wise for the whole step
against the dense KKT solve (tests/test_gpu_resolve.py).  Which kernel family a case reaches is asserted, never skipped, from
what the C ABI tells (gbdpcg_cluster_members, the mode, the batch against the CU count, the alignment), as
tests/test_gpu_footprint.py does.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding, synth  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    s.set_path(binding.PATH_FUSED)
    yield s
    s.set_symmetric(2)
    s.set_path(binding.PATH_AUTO)
    s.close()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tt(dt):
    return torch.float32 if np.dtype(dt) == F32 else torch.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def symmetrize(n, N, P):
    L, D, R = synth.unpack_bt(n, N, P)
    L = L.copy()
    L[..., 1:, :, :] = np.swapaxes(R[..., :-1, :, :], -1, -2)
    return synth.pack_bt(L, D, R)


class Case:
    def __init__(self, name, reach, n, N, dt, mode=2, sym=True, pinv=True, shift=0):
        self.name, self.reach, self.n, self.N, self.dt = name, set(reach), n, N, np.dtype(dt)
        self.mode, self.sym, self.pinv, self.shift, self.es = mode, sym, pinv, shift, np.dtype(dt).itemsize

    def __repr__(self):
        return self.name


# reach: the families the case must reach over the batches below (a batch that one round of clusters holds goes to the cluster
# kernel in mode 2, api_solve.hip one_cluster_round)
CASES = [
    Case("14x128-m2", {"resident_sym", "cluster"}, 14, 128, F32, mode=2),
    Case("14x128-m1", {"resident_sym"}, 14, 128, F32, mode=1),
    Case("14x128-m0", {"cluster"}, 14, 128, F32, mode=0),
    Case("14x64", {"resident"}, 14, 64, F32),
    Case("12x128", {"cluster"}, 12, 128, F32),
    Case("14x128-f64", {"cluster"}, 14, 128, F64),
    Case("20x128", {"fused"}, 20, 128, F32),
    Case("24x64", {"fused"}, 24, 64, F32),
    Case("7x64", {"resident"}, 7, 64, F32),
    Case("7x64-f64", {"resident"}, 7, 64, F64),
    Case("14x128-m2-nonsym", {"cluster"}, 14, 128, F32, mode=2, sym=False),
    Case("14x128-ident", {"cluster"}, 14, 128, F32, pinv=False),
    Case("14x128-off4", {"fused"}, 14, 128, F32, shift=4),
    Case("14x128-m1-off8", {"resident_sym"}, 14, 128, F32, mode=1, shift=8),
]


def batches():
    return [1, 5, 100, 300, 4 * cus() + 37]


def resident_horizon(solver, es, n):
    """Longest horizon pcg_resident.hip takes at this block size: the cluster kernel takes over one knot later."""
    if n > 15:
        return 0
    for N in range(1, 2049):
        if solver.cluster_members(es, n, N) != 0:
            return N - 1
    raise AssertionError("no cluster horizon found")


def family(solver, c, B):
    """The kernel family the fused branch of solve reaches for this case and batch (csrc/api_solve.hip, csrc/pcg_fused.hip)."""
    assert solver.choose_path(c.es, c.n, c.N, B) == binding.PATH_FUSED
    members = solver.cluster_members(c.es, c.n, c.N)
    al8 = c.shift % 8 == 0
    if members == 0 and c.n <= 15:
        assert c.N <= resident_horizon(solver, c.es, c.n)
        if c.shift % (4 if c.es == 4 and c.n % 2 else 8) == 0:
            return "resident"
    one_round = members != 0 and B * members <= cus() and al8
    if (c.n, c.dt) == (14, F32) and c.N <= 128 and c.pinv and al8 and ((c.mode == 2 and c.sym and not one_round) or c.mode == 1):
        return "resident_sym"
    if members != 0 and al8:
        return "cluster"
    assert members == 0 or not al8
    return "fused"


class Data:
    """One pair of matrices and B sets of vectors on the host."""

    def __init__(self, c, B, seed=0):
        n, N = c.n, c.N
        d = synth.gen_numpy(n, N, seed=900 + 17 * n + N + seed, batch=1, dtype=c.dt)
        self.S = d["S"][0].copy()
        self.P = symmetrize(n, N, d["Pinv"])[0].copy() if c.mode else d["Pinv"][0].copy()
        if not c.sym:   # one ulp in one element of an L block: the pair fails the bit test, the numbers hardly move
            i = 3 * n * n + 2 * n + 1
            self.S[i] = np.nextafter(self.S[i], c.dt.type(np.inf))
        rng = np.random.default_rng(1000 * n + N + B + seed)
        self.gamma = (d["gamma"][0][None, :] * (1.0 + 0.003 * np.arange(B))[:, None] + 0.05 * rng.standard_normal((B, n * N))).astype(c.dt)
        self.lam0 = np.zeros_like(self.gamma)
        self.warm0 = (0.1 * rng.standard_normal(self.gamma.shape)).astype(c.dt)


def shifted(flat, shift_bytes):
    """A device copy of `flat` whose address is 16-byte aligned plus shift_bytes."""
    es = flat.element_size()
    buf = torch.empty(flat.numel() + 16 // es, dtype=flat.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[shift_bytes // es:shift_bytes // es + flat.numel()]
    v.copy_(flat)
    assert v.data_ptr() % 16 == shift_bytes
    return v


def outputs(c, B):
    lam = torch.empty(B * c.n * c.N, dtype=tt(c.dt), device="cuda")
    return dict(lam=lam, r=torch.full_like(lam, float("nan")), p=torch.full_like(lam, float("nan")),
                it=torch.full((B,), -1, dtype=torch.int32, device="cuda"), fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))


def solve_both(solver, c, B, S1, P1, gamma, lam0, tol, mi):
    """(replicated, shared) outputs of one solve; S1, P1: the single matrices on the device."""
    solver.set_symmetric(c.mode)
    solver.set_path(binding.PATH_FUSED)
    try:
        Sr = shifted(S1.repeat(B), c.shift)
        Pr = shifted(P1.repeat(B), c.shift) if c.pinv else None
        a = outputs(c, B)
        a["lam"].copy_(lam0)
        solver.solve(c.n, c.N, B, Sr, Pr, gamma, a["lam"], r=a["r"], p=a["p"], tol=tol, max_iter=mi, iters=a["it"], max_iter_exit=a["fl"])
        torch.cuda.synchronize()
        del Sr, Pr
        b = outputs(c, B)
        b["lam"].copy_(lam0)
        solver.solve_shared(c.n, c.N, B, S1, P1 if c.pinv else None, gamma, b["lam"], r=b["r"], p=b["p"], tol=tol, max_iter=mi,
                            iters=b["it"], max_iter_exit=b["fl"])
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    return a, b


def assert_same(a, b, what):
    for k in ("lam", "r", "p", "it", "fl"):
        x, y = a[k], b[k]
        if x.is_floating_point():
            x, y = x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)
        assert torch.equal(x, y), (what, k)


# ------------------------------------------------------------------------------------------- 1. bit identity with the twin
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_solve_shared_is_the_replicated_solve(solver, c):
    """Every output of gbdpcg_solve_shared_* against gbdpcg_solve_* on `batch` copies, to tolerance from lambda = 0 and at a
    fixed count from a warm start, over batches of 1, 5, one round of clusters, 300 and more than 4 x CUs problems."""
    reached = set()
    for B in batches():
        fam = family(solver, c, B)
        reached.add(fam)
        d = Data(c, B)
        S1, P1 = shifted(dev(d.S), c.shift), shifted(dev(d.P), c.shift)
        gamma = dev(d.gamma.reshape(-1))
        tol = 1e-6 if c.dt == F32 else 1e-10
        a, b = solve_both(solver, c, B, S1, P1, gamma, dev(d.lam0.reshape(-1)), tol, 60)
        it = a["it"].cpu().numpy()
        print(f"{c} B={B} {fam}: iters {it.min()}..{it.max()}")
        assert int(a["fl"].sum()) == 0 and it.min() >= 1 and it.max() < 60, (c, B)
        assert bool(torch.isfinite(b["lam"]).all())
        assert_same(a, b, (c, B, "to tolerance"))
        a, b = solve_both(solver, c, B, S1, P1, gamma, dev(d.warm0.reshape(-1)), 0.0, 6)
        assert (a["it"].cpu().numpy() == 6).all() and (a["fl"].cpu().numpy() == 1).all()
        assert_same(a, b, (c, B, "fixed count, warm start"))
    assert reached == c.reach, (c, reached)


def test_batch_one_is_the_twin(solver):
    """batch = 1: the shared call and the twin see the same arguments."""
    c = CASES[0]
    d = Data(c, 1, seed=3)
    a, b = solve_both(solver, c, 1, dev(d.S), dev(d.P), dev(d.gamma.reshape(-1)), dev(d.lam0.reshape(-1)), 1e-6, 60)
    assert_same(a, b, "batch 1")


_OFF8_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_shared as t
s = t.binding.Solver(0)
for N in (3, 128):
    c = t.Case(f"14x{N}-m1-off8", {"resident_sym"}, 14, N, t.F32, mode=1, shift=8)
    d = t.Data(c, 3)
    S1, P1, gamma = t.shifted(t.dev(d.S), 8), t.shifted(t.dev(d.P), 8), t.dev(d.gamma.reshape(-1))
    for lam0, tol, mi in ((d.lam0, 1e-6, 60), (d.warm0, 0.0, 6)):
        a, b = t.solve_both(s, c, 3, S1, P1, gamma, t.dev(lam0.reshape(-1)), tol, mi)
        it, fl = a["it"].cpu().numpy(), a["fl"].cpu().numpy()
        assert ((it >= 1).all() and (it < 60).all() and not fl.any()) if tol else ((it == 6).all() and (fl == 1).all()), (N, it, fl)
        assert bool(t.torch.isfinite(b["lam"]).all())
        t.assert_same(a, b, (N, tol))
print("off8 ok")
"""


def test_shared_pair_at_8_byte_offset_is_the_plain_kernel():
    """pcg_resident_sym.hip's shared instantiation with direct tile loads (the one pair only 8-byte aligned) at N = 3 and N = 128,
    batch 3: the checks of test_solve_shared_is_the_replicated_solve, whose case 14x128-m1-off8 asserts that the family is reached
    at N = 128.  In a child process, because N = 3 gets past pcg_resident.hip only with GBDPCG_NO_RESIDENT, read once per process
    (csrc/pcg_fused.hip, launch_pcg_fused: pcg_resident.hip first, then pcg_resident_sym.hip when the caller asserts symmetry)."""
    env = dict(os.environ, GBDPCG_NO_RESIDENT="1")
    res = subprocess.run([sys.executable, "-c", _OFF8_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "off8 ok" in res.stdout, res.stderr[-3000:]


SCHUR_SHAPES = [(14, 7, 128, 3), (14, 7, 1, 2), (14, 7, 2, 1), (2, 1, 5, 4), (3, 3, 2, 1), (5, 2, 9, 2), (12, 4, 33, 2), (4, 6, 3, 2),
                (36, 18, 6, 1), (1, 1, 4, 1), (44, 3, 3, 1)]
QUAD_SHAPES = [(2, 1), (4, 1), (4, 2), (6, 3), (8, 4), (10, 5), (12, 4), (12, 6), (13, 4), (3, 1), (5, 2), (6, 1), (6, 2), (7, 3), (8, 2), (9, 3),
               (10, 4), (11, 4), (12, 3), (14, 7)]
QUAD_NB = [(1, 2), (2, 3), (3, 1), (5, 3), (7, 11), (16, 5)]
GAMMA_CASES = SCHUR_SHAPES + [(nx, nu, N, B) for nx, nu in QUAD_SHAPES for N, B in QUAD_NB] + [(36, 12, 7, 3)]   # tests/test_gpu_resolve.py


def one_plant(nx, nu, N, B, dtype, seed):
    """One problem's KKT blocks with the fp64 oracle's G^-1 (cast), and B sets of g, c."""
    d1 = so.gen(nx, nu, N, seed=seed, batch=1, dtype=dtype)
    dv = so.gen(nx, nu, N, seed=seed + 1, batch=B, dtype=dtype)
    _, _, Gi = so.form_schur(nx, nu, N, d1["G"][0], d1["C"][0], d1["g"][0], d1["c"][0])
    Gi = np.asarray(Gi).reshape(-1).astype(dtype)
    return d1, dv, Gi


@pytest.mark.parametrize("general", [False, True], ids=["register", "any-size"])
@pytest.mark.parametrize("dtype,tol", [(F32, 2e-4), (F64, 1e-11)])
@pytest.mark.parametrize("nx,nu,N,B", GAMMA_CASES)
def test_gamma_and_recovery_shared_are_their_twins(solver, monkeypatch, nx, nu, N, B, dtype, tol, general):
    """gbdpcg_form_gamma_shared_* / gbdpcg_recover_primal_shared_* against the twins on B copies of G^-1 and C, bit for bit,
    with the four-rows-per-wave kernels and with the any-size ones; gamma also against the fp64 oracle given the same single
    blocks once per problem."""
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    d1, dv, Gi = one_plant(nx, nu, N, B, dtype, 300 + nx + N)
    Gi1, C1 = dev(Gi), dev(d1["C"][0].reshape(-1))
    g, c = dev(dv["g"].reshape(-1)), dev(dv["c"].reshape(-1))
    lam = dev(np.random.default_rng(nx * N).standard_normal(B * nx * N).astype(dtype))
    gs = solver.form_gamma_shared(nx, nu, N, B, Gi1, C1, g, c)
    gr = solver.form_gamma(nx, nu, N, B, Gi1.repeat(B), C1.repeat(B), g, c)
    zs = solver.recover_primal_shared(nx, nu, N, B, Gi1, C1, g, lam)
    zr = solver.recover_primal(nx, nu, N, B, Gi1.repeat(B), C1.repeat(B), g, lam)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(zs).all())
    assert np.array_equal(gs.cpu().numpy(), gr.cpu().numpy())
    assert np.array_equal(zs.cpu().numpy(), zr.cpu().numpy())
    gs = gs.cpu().numpy().reshape(B, -1).astype(np.float64)
    for b in range(B):
        og = np.asarray(so.form_schur(nx, nu, N, d1["G"][0], d1["C"][0], dv["g"][b], dv["c"][b])[1], np.float64).reshape(-1)
        assert np.abs(gs[b] - og).max() <= tol * max(np.abs(og).max(), 1e-300), (b, np.abs(gs[b] - og).max() / np.abs(og).max())


# ------------------------------------------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("c", [CASES[0], CASES[1], CASES[2], CASES[3], CASES[5], CASES[6], CASES[9]], ids=repr)
def test_solve_shared_vs_oracle(solver, orc, c):
    B = 300 if c.n == 14 and c.N == 128 and c.dt == F32 else 6
    tol = 1e-6 if c.dt == F32 else 1e-10
    d = Data(c, B, seed=5)
    solver.set_symmetric(c.mode)
    try:
        o = outputs(c, B)
        o["lam"].zero_()
        solver.solve_shared(c.n, c.N, B, dev(d.S), dev(d.P), dev(d.gamma.reshape(-1)), o["lam"], r=o["r"], p=o["p"], tol=tol,
                            max_iter=60, iters=o["it"], max_iter_exit=o["fl"])
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    idx = list(range(0, B, max(1, B // 6)))[:6]
    ob = orc.pcg_batch(c.n, c.N, len(idx), np.stack([d.S] * len(idx)), np.stack([d.P] * len(idx)), d.gamma[idx], tol=tol, max_iter=60)
    lam = o["lam"].cpu().numpy().reshape(B, -1).astype(np.float64)[idx]
    it = o["it"].cpu().numpy()[idx]
    err = np.linalg.norm(lam - ob["lambda_"], axis=1) / np.linalg.norm(ob["lambda_"], axis=1)
    print(f"{c} {family(solver, c, B)}: iters {it.tolist()} oracle {ob['iters'].tolist()} lambda err {err.max():.3e}")
    assert np.array_equal(it, ob["iters"].astype(np.int32)) and int(o["fl"].sum()) == 0
    assert err.max() < tol, err.max()


@pytest.mark.parametrize("dtype,tol", [(F32, 3e-4), (F64, 1e-9)])
def test_resolve_shared_end_to_end(solver, dtype, tol):
    """kkt_step at batch 1 factors the one plant; new gradients and residuals of B problems go through kkt_resolve_shared from
    lambda = 0: multipliers and step of every problem against numpy.linalg.solve of its whole KKT system (fp64)."""
    nx, nu, N, B = 14, 7, 64, 6
    pcg_tol = 1e-10 if dtype == F32 else 1e-22
    d1 = so.gen(nx, nu, N, seed=31, batch=1, dtype=dtype)
    dv = so.gen(nx, nu, N, seed=32, batch=B, dtype=dtype)
    G, C, g1, c1 = (dev(d1[k].reshape(-1)) for k in "GCgc")
    S = torch.empty(3 * nx * nx * N, dtype=G.dtype, device="cuda")
    Pinv, Ginv = torch.empty_like(S), torch.empty_like(G)
    gamma1 = torch.empty(nx * N, dtype=G.dtype, device="cuda")
    lam1, z1 = torch.zeros_like(gamma1), torch.empty_like(g1)
    solver.kkt_step(nx, nu, N, 1, G, C, g1, c1, S, gamma1, Ginv, Pinv, lam1, z1, tol=pcg_tol, max_iter=200)
    g, c = dev(dv["g"].reshape(-1)), dev(dv["c"].reshape(-1))
    gamma = torch.empty(B * nx * N, dtype=G.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it, fl = solver.kkt_resolve_shared(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, tol=pcg_tol, max_iter=200)
    torch.cuda.synchronize()
    assert not fl.cpu().numpy().any() and (it.cpu().numpy() < 200).all()
    lam, z = lam.cpu().numpy().reshape(B, -1), z.cpu().numpy().reshape(B, -1)
    for b in range(B):
        oz, ol = so.dense_kkt_solve(nx, nu, N, d1["G"][0], d1["C"][0], dv["g"][b], dv["c"][b])
        el, ez = np.linalg.norm(lam[b] - ol) / np.linalg.norm(ol), np.linalg.norm(z[b] - oz) / np.linalg.norm(oz)
        print(f"kkt_resolve_shared {np.dtype(dtype).name} problem {b}: lambda {el:.3e} z {ez:.3e}")
        assert el <= tol and ez <= tol


# ------------------------------------------------------------------------------------- 3. one matrix is all that is read
def arena_matrix(M, n, N, no_L=False):
    """M behind 4 KiB of NaN and in front of two further matrices' worth of NaN, L_0 and R_{N-1} (and, no_L, every L) NaN."""
    ms = M.numel()
    pre = 4096 // M.element_size()
    buf = torch.full((pre + 3 * ms,), float("nan"), dtype=M.dtype, device="cuda")
    v = buf[pre:pre + ms]
    v.copy_(M)
    v[:n * n] = float("nan")
    v[ms - n * n:] = float("nan")
    if no_L:
        v.view(N, 3, n * n)[:, 0, :] = float("nan")
    return buf, v


@pytest.mark.parametrize("c", [CASES[0], CASES[1], CASES[2], CASES[3], CASES[5], CASES[6], CASES[8]], ids=repr)
def test_one_matrix_is_all_that_is_read(solver, c):
    B = 4 * cus() + 37 if c.n <= 14 and c.dt == F32 else 40
    d = Data(c, B, seed=7)
    S1, P1, gamma, lam0 = dev(d.S), dev(d.P), dev(d.gamma.reshape(-1)), dev(d.warm0.reshape(-1))
    fam = family(solver, c, B)
    no_L = c.mode == 1 and fam == "resident_sym"      # the [D|R] kernel never reads an L block: proves that it ran
    bufS, aS = arena_matrix(S1, c.n, c.N, no_L)
    bufP, aP = arena_matrix(P1, c.n, c.N, no_L)
    keepS, keepP, keepg = bufS.clone(), bufP.clone(), gamma.clone()
    solver.set_symmetric(c.mode)
    try:
        free, tight = outputs(c, B), outputs(c, B)
        for o, (s, p) in ((free, (S1, P1)), (tight, (aS, aP))):
            o["lam"].copy_(lam0)
            solver.solve_shared(c.n, c.N, B, s, p, gamma, o["lam"], r=o["r"], p=o["p"], tol=1e-6 if c.dt == F32 else 1e-10, max_iter=60,
                                iters=o["it"], max_iter_exit=o["fl"])
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    assert bool(torch.isfinite(tight["lam"]).all()) and int(tight["fl"].sum()) == 0, fam
    assert_same(free, tight, (c, fam))
    for kept, now in ((keepS, bufS), (keepP, bufP), (keepg, gamma)):
        assert torch.equal(kept.view(torch.uint8), now.view(torch.uint8))


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 128, 300), (9, 3, 7, 11), (36, 12, 7, 3)])
def test_gamma_and_recovery_read_one_problems_blocks(solver, nx, nu, N, B, dtype):
    d1, dv, Gi = one_plant(nx, nu, N, B, dtype, 77)
    g, c = dev(dv["g"].reshape(-1)), dev(dv["c"].reshape(-1))
    lam = dev(np.random.default_rng(5).standard_normal(B * nx * N).astype(dtype))
    outs = []
    for guarded in (False, True):
        mats = []
        for M in (dev(Gi), dev(d1["C"][0].reshape(-1))):
            if guarded:   # NaN in front, and at least one further problem's worth of NaN behind
                buf = torch.full((1024 + 3 * M.numel(),), float("nan"), dtype=M.dtype, device="cuda")
                buf[1024:1024 + M.numel()] = M
                M = buf[1024:1024 + M.numel()]
                mats.append(buf)
            mats.append(M)
        Gd, Cd = (mats[1], mats[3]) if guarded else (mats[0], mats[1])
        outs.append((solver.form_gamma_shared(nx, nu, N, B, Gd, Cd, g, c), solver.recover_primal_shared(nx, nu, N, B, Gd, Cd, g, lam)))
        torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert bool(torch.isfinite(b).all()) and np.array_equal(a.cpu().numpy(), b.cpu().numpy())


# ----------------------------------------------------------------------------------------------------------- 4. isolation
@pytest.mark.parametrize("c", [CASES[0], CASES[2], CASES[3], CASES[6]], ids=repr)
def test_isolation_and_permutation(solver, c):
    B = 4 * cus() + 37 if c.n <= 14 else 300
    d = Data(c, B, seed=9)
    S1, P1 = dev(d.S), dev(d.P)
    mi, tol = 30, 1e-6
    bad = B // 2 + 1

    def run(gamma):
        o = outputs(c, B)
        o["lam"].zero_()
        solver.set_symmetric(c.mode)
        try:
            solver.solve_shared(c.n, c.N, B, S1, P1, dev(gamma.reshape(-1)), o["lam"], r=o["r"], p=o["p"], tol=tol, max_iter=mi,
                                iters=o["it"], max_iter_exit=o["fl"])
            torch.cuda.synchronize()
        finally:
            solver.set_symmetric(2)
        return o

    clean = run(d.gamma)
    g2 = d.gamma.copy()
    g2[bad, 3] = np.nan
    broken = run(g2)
    others = torch.as_tensor([b for b in range(B) if b != bad], device="cuda")
    for k in ("lam", "r", "p"):
        x, y = clean[k].view(B, -1)[others], broken[k].view(B, -1)[others]
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k
    assert torch.equal(clean["it"][others], broken["it"][others]) and torch.equal(clean["fl"][others], broken["fl"][others])
    assert int(broken["it"][bad]) == mi and int(broken["fl"][bad]) == 1
    assert not bool(torch.isfinite(broken["lam"].view(B, -1)[bad]).any())
    perm = np.random.default_rng(4).permutation(B)
    moved = run(d.gamma[perm])
    tp = torch.as_tensor(perm, device="cuda")
    for k in ("lam", "r", "p"):
        assert torch.equal(moved[k].view(B, -1).view(torch.uint8), clean[k].view(B, -1)[tp].view(torch.uint8)), k
    assert torch.equal(moved["it"], clean["it"][tp]) and torch.equal(moved["fl"], clean["fl"][tp])


# ------------------------------------------------------------------- 5. a batch that replication could not hold comfortably
def test_8192_problems_on_one_pair(solver, orc):
    """8192 problems of 14 x 128 on one pair (replicated: 2 x 2.5 GB of matrices), exit_tol 0 and 25 iterations as bench.py times
    its configurations: count and flag of every problem, lambda / r / p of 64 against the oracle, the true residual of all."""
    n, N, B, MI = 14, 128, 8192, 25
    c = Case("8192", {"resident_sym"}, n, N, F32)
    assert family(solver, c, B) == "resident_sym"
    d = Data(c, B, seed=11)
    S1, P1, gamma = dev(d.S), dev(d.P), dev(d.gamma.reshape(-1))
    o = outputs(c, B)
    o["lam"].zero_()
    gr = solver.graph_solve_shared(n, N, B, S1, P1, gamma, o["lam"], o["r"], o["p"], 0.0, MI, o["it"], o["fl"])
    for _ in range(2):
        o["lam"].zero_()
        gr.launch()
    torch.cuda.synchronize()
    gr.close()
    assert (o["it"].cpu().numpy() == MI).all() and (o["fl"].cpu().numpy() == 1).all()
    assert all(bool(torch.isfinite(o[k]).all()) for k in ("lam", "r", "p"))
    idx = list(range(77, B, 128))
    assert len(idx) == 64
    ob = orc.pcg_batch(n, N, 64, np.stack([d.S] * 64), np.stack([d.P] * 64), d.gamma[idx], tol=0.0, max_iter=MI, nthreads=8)
    sel = torch.as_tensor(idx, device="cuda")
    hl, hr, hp = (o[k].view(B, -1)[sel].cpu().numpy().astype(np.float64) for k in ("lam", "r", "p"))
    for j in range(64):
        err = np.linalg.norm(hl[j] - ob["lambda_"][j]) / np.linalg.norm(ob["lambda_"][j])
        assert err < 1e-6, (idx[j], err)
        scale = np.abs(d.gamma[idx[j]]).max()
        assert np.abs(hr[j] - ob["r"][j]).max() < 2e-5 * scale and np.abs(hp[j] - ob["p"][j]).max() < 2e-5 * scale, idx[j]
    chunk = 256
    Sr = S1.repeat(chunk)
    worst = 0.0
    for b0 in range(0, B, chunk):
        lam = o["lam"].view(B, -1)[b0:b0 + chunk].reshape(-1)
        y = solver.spmv(n, N, chunk, Sr, lam)
        torch.cuda.synchronize()
        gm = gamma.view(B, -1)[b0:b0 + chunk].double()
        res = (gm - y.view(chunk, -1).double()).norm(dim=1) / gm.norm(dim=1)
        worst = max(worst, float(res.max()))
    print(f"8192 on one pair: worst true residual {worst:.3e}")
    assert worst < 2e-6, worst          # the fp32 rounding floor tests/test_gpu_timed_configs.py states for this shape


# ------------------------------------------------------------------------- 6. kkt_resolve_shared is the three shared calls
def factor_one(solver, nx, nu, N, dtype, seed):
    d1 = so.gen(nx, nu, N, seed=seed, batch=1, dtype=dtype)
    G, C, g1, c1 = (dev(d1[k].reshape(-1)) for k in "GCgc")
    S, _, Ginv = solver.form_schur(nx, nu, N, 1, G, C, g1, c1)
    Pinv = solver.form_pinv(nx, N, 1, S, binding.PINV_STAIR)
    return d1, C, S, Ginv, Pinv


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 128, 300), (14, 7, 24, 9), (5, 3, 10, 4)])
def test_kkt_resolve_shared_is_the_three_shared_calls(solver, nx, nu, N, B, dtype):
    _, C, S, Ginv, Pinv = factor_one(solver, nx, nu, N, dtype, 41)
    dv = so.gen(nx, nu, N, seed=42, batch=B, dtype=dtype)
    g, c = dev(dv["g"].reshape(-1)), dev(dv["c"].reshape(-1))
    gamma = solver.form_gamma_shared(nx, nu, N, B, Ginv, C, g, c)
    lam = torch.zeros_like(gamma)
    r, p = torch.full_like(lam, float("nan")), torch.full_like(lam, float("nan"))
    it, fl = solver.solve_shared(nx, N, B, S, Pinv, gamma, lam, r=r, p=p, tol=1e-8, max_iter=100)
    z = solver.recover_primal_shared(nx, nu, N, B, Ginv, C, g, lam)
    torch.cuda.synchronize()
    want = [t.clone() for t in (gamma, lam, r, p, it, fl, z)]
    gamma2, z2, lam2 = torch.full_like(gamma, float("nan")), torch.full_like(z, float("nan")), torch.zeros_like(lam)
    r2, p2 = torch.full_like(lam, float("nan")), torch.full_like(lam, float("nan"))
    it2 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    fl2 = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    solver.kkt_resolve_shared(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma2, lam2, z2, r=r2, p=p2, tol=1e-8, max_iter=100, iters=it2,
                              max_iter_exit=fl2)
    torch.cuda.synchronize()
    for name, a, b in zip("gamma lam r p iters flags z".split(), (gamma2, lam2, r2, p2, it2, fl2, z2), want):
        assert torch.equal(a, b), name
    assert int(fl2.sum()) == 0 and int(it2.min()) > 0


@pytest.mark.parametrize("dtype,tol", [(F32, 3e-4), (F64, 1e-9)])
def test_resolve_shared_graph_replays_and_caller_capture(solver, dtype, tol):
    """One graph of the shared resolve replayed after g and c are rewritten in place (against the dense KKT solve of every
    problem), then the same call captured into a caller-owned stream after gbdpcg_reserve: same bits as the direct call."""
    nx, nu, N, B = 14, 7, 64, 6
    pcg_tol = 1e-10 if dtype == F32 else 1e-22
    d1, C, S, Ginv, Pinv = factor_one(solver, nx, nu, N, dtype, 51)
    g = torch.empty(B * so.sizes(nx, nu, N)["g"], dtype=S.dtype, device="cuda")
    c = torch.empty(B * nx * N, dtype=S.dtype, device="cuda")
    gamma = torch.empty(B * nx * N, dtype=S.dtype, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    r, p = torch.empty_like(lam), torch.empty_like(lam)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    gr = solver.graph_kkt_resolve_shared(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, pcg_tol, 200, it, fl, z)
    for tick in range(3):
        dn = so.gen(nx, nu, N, seed=60 + tick, batch=B, dtype=dtype)
        assert dn["g"].reshape(-1).size == g.numel()
        g.copy_(dev(dn["g"].reshape(-1)))
        c.copy_(dev(dn["c"].reshape(-1)))
        gr.launch()
        torch.cuda.synchronize()
        assert int(fl.sum()) == 0 and int(it.max()) < 200
        hl, hz = lam.cpu().numpy().reshape(B, -1), z.cpu().numpy().reshape(B, -1)
        for b in range(B):
            oz, ol = so.dense_kkt_solve(nx, nu, N, d1["G"][0], d1["C"][0], dn["g"][b], dn["c"][b])
            assert np.linalg.norm(hl[b] - ol) / np.linalg.norm(ol) <= tol and np.linalg.norm(hz[b] - oz) / np.linalg.norm(oz) <= tol
    gr.close()
    # the caller's own capture
    solver.reserve(S.element_size(), nx, N, B)
    lam.zero_()
    solver.kkt_resolve_shared(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, r=r, p=p, tol=pcg_tol, max_iter=200, iters=it,
                              max_iter_exit=fl)
    torch.cuda.synchronize()
    want = [t.clone() for t in (gamma, lam, r, p, it, fl, z)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):     # the capturing stream is torch's current one inside the block
        solver.kkt_resolve_shared(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, z, r=r, p=p, tol=pcg_tol, max_iter=200, iters=it,
                                  max_iter_exit=fl)
    for t in (gamma, r, p, z):
        t.fill_(float("nan"))
    lam.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip("gamma lam r p iters flags z".split(), (gamma, lam, r, p, it, fl, z), want):
        assert torch.equal(a, b), name


# -------------------------------------------------------------------------------------------------------- 7. bad arguments
@pytest.mark.parametrize("suf,ft,tdt", [("f32", ctypes.c_float, torch.float32), ("f64", ctypes.c_double, torch.float64)])
def test_bad_arguments(solver, suf, ft, tdt):
    lib, h = solver.lib, solver.h
    nx, nu, N, B = 6, 3, 4, 3
    buf, obuf = torch.zeros(4096, dtype=tdt, device="cuda"), torch.zeros(4096, dtype=tdt, device="cuda")
    P, O = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(obuf.data_ptr())   # inputs (zeros), outputs
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def solve_args(**kw):
        a = dict(h=h, n=nx, N=N, batch=B, S=P, Pinv=P, gamma=P, lam=O, r=None, p=None, tol=ft(1e-6), mi=5, it=O, fl=None)
        a.update(kw)
        return tuple(a.values())

    fn = getattr(lib, f"gbdpcg_solve_shared_{suf}")
    assert fn(*solve_args(), s) == 0
    for k in ("S", "gamma", "lam", "it"):
        assert fn(*solve_args(**{k: None}), s) == INVALID, k
    for k in ("n", "N", "batch"):
        assert fn(*solve_args(**{k: 0}), s) == INVALID, k
    out = ctypes.c_void_p()
    gfn = getattr(lib, f"gbdpcg_graph_create_solve_shared_{suf}")
    for k in ("S", "gamma", "lam", "it"):
        assert gfn(*solve_args(**{k: None}), ctypes.byref(out)) == INVALID and not out.value, k
    assert gfn(*solve_args(batch=0), ctypes.byref(out)) == INVALID
    assert gfn(*solve_args(), None) == INVALID

    def head(**kw):
        a = dict(h=h, nx=nx, nu=nu, N=N, batch=B, Ginv=P, C=P, g=P, x=P)
        a.update(kw)
        return tuple(a.values())

    for name in ("form_gamma_shared", "recover_primal_shared"):
        f = getattr(lib, f"gbdpcg_{name}_{suf}")
        assert f(*head(), O, s) == 0
        for k in ("Ginv", "C", "g", "x"):
            assert f(*head(**{k: None}), O, s) == INVALID, (name, k)
        assert f(*head(), None, s) == INVALID, name
        for k in ("nx", "nu", "N", "batch"):
            assert f(*head(**{k: 0}), O, s) == INVALID, (name, k)

    def tail(**kw):
        a = dict(S=P, Pinv=P, gamma=O, lam=O, r=None, p=None, tol=ft(1e-6), mi=5, it=O, fl=None, z=O)
        a.update(kw)
        return tuple(a.values())

    f = getattr(lib, f"gbdpcg_kkt_resolve_shared_{suf}")
    gf = getattr(lib, f"gbdpcg_graph_create_kkt_resolve_shared_{suf}")
    for k in ("Ginv", "C", "g", "x"):
        assert f(*head(**{k: None}), *tail(), s) == INVALID, k
        assert gf(*head(**{k: None}), *tail(), ctypes.byref(out)) == INVALID, k
    for k in ("S", "gamma", "lam", "it", "z"):
        assert f(*head(), *tail(**{k: None}), s) == INVALID, k
        assert gf(*head(), *tail(**{k: None}), ctypes.byref(out)) == INVALID, k
    for k in ("nx", "nu", "N", "batch"):
        assert f(*head(**{k: 0}), *tail(), s) == INVALID, k
        assert gf(*head(**{k: 0}), *tail(), ctypes.byref(out)) == INVALID, k
    torch.cuda.synchronize()


def test_a_shape_beyond_one_workgroup_is_unsupported(solver):
    """36 x 256 in fp64 does not fit one workgroup: the shared persistent and split forms do not exist, d_lambda is untouched."""
    n, N, B = 36, 256, 2
    S = torch.zeros(3 * n * n * N, dtype=torch.float64, device="cuda")
    gamma = torch.ones(B * n * N, dtype=torch.float64, device="cuda")
    lam = torch.full_like(gamma, 3.25)
    it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    args = (solver.h, n, N, B, ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(gamma.data_ptr()),
            ctypes.c_void_p(lam.data_ptr()), None, None, ctypes.c_double(1e-6), 5, ctypes.c_void_p(it.data_ptr()), None)
    st = solver.lib.gbdpcg_solve_shared_f64(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = ctypes.c_void_p()
    st2 = solver.lib.gbdpcg_graph_create_solve_shared_f64(*args, ctypes.byref(out))
    torch.cuda.synchronize()
    assert st == UNSUPPORTED and st2 == UNSUPPORTED and not out.value
    assert bool((lam == 3.25).all()) and bool((it == -1).all())


# ----------------------------------------------------------------------------------------------------------- 8. the example
def test_shared_plant_loop_example_runs():
    ex = os.path.join(ROOT, "gbd-pcg_amd", "examples")
    subprocess.check_call(["make", "-C", ex, "shared_plant_loop"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ex, "shared_plant_loop")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
