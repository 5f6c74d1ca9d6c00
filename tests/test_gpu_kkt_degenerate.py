"""Exactly zero right-hand sides at the KKT level, on the device: what gbdpcg_kkt_step_*, gbdpcg_kkt_step_reg_*, gbdpcg_kkt_resolve_*,
gbdpcg_kkt_resolve_shared_*, gbdpcg_admm_step_*, one graph form of each, and the mixed-precision refinement do with a problem whose
gamma (or fp64 defect) is exactly zero, and that they do it to that problem alone.

The solve follows the reference's recurrence (pcg.cuh:169,195): from a zero preconditioned residual the first alpha is 0/0, lambda,
r and p become NaN, |NaN| < tol is false, and the problem runs to max_iter and leaves with max_iter_exit = 1.
tests/test_gpu_footprint.py part B pins that for the solve entry points; oracle/pcg_oracle.c reproduces it
(tests/test_kkt_degenerate_reference.py).  This file pins what the layers above the solve hand back (include/gbdpcg.h states it):

  degenerate problems (1 and 3 of 5; constructions a, b, c of tests/kkt_degenerate_ref.py)
      iters == max_iter, max_iter_exit == 1, lambda and z non-finite in EVERY entry, the gamma written exactly zero, and
      gbdpcg_kkt_residual_* behind the call NaN in both norms -- which, with the flag, is how a caller sees the case on the device;
  regular problems (0, 2, 4)
      every output bit-identical with the same call on the twin batch (regular vectors in problems 1 and 3 as well), and within
      3e-4 (fp32) / 1e-9 (fp64) norm-wise of the fp64 dense solve -- the tolerances of tests/test_gpu_resolve.py at its PCG settings
      (tol 1e-10 / 1e-22, max_iter 200);
  history
      the twin call on the same handle AFTER the degenerate one gives, in every output, the bits it gives on a fresh handle.

The dense bound presupposes a converged solve (tests/test_gpu_resolve.py asserts the flags before it compares).  At max_iter 200 every
regular problem has to converge; in the rows at max_iter 7, there so that the run to the limit is short, a regular problem that runs
out is held to the bit-identity with its twin alone, one that converges to the dense bound as well.

Refinement: a problem at an exactly solved point (z = lambda = 0, g = c = 0) has the fp64 defect zero: d_res = (0, 0), e = 0 (the
rule of tests/kkt_refine_ref.py for m = 0), a zero right-hand side, and the correction solve returns NaN like any other solve;
gbdpcg_kkt_refine_apply adds it: THE POINT IS DESTROYED (NaN in every entry of z and lambda), in the three calls and in the
gbdpcg_kkt_refine_step graph alike.  A caller tests d_res before applying.  The neighbours keep every bit.
Run with -s for the observed (iters, flag, finiteness) per entry point."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kkt_degenerate_ref as kd  # noqa: E402
import kkt_refine_ref as rref  # noqa: E402
from admm_util import np_same  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
B = kd.B
EPS = {F32: 3e-4, F64: 1e-9}            # tests/test_gpu_resolve.py
PCG_TOL = {F32: 1e-10, F64: 1e-22}
RHO = np.array([0.5, 0.125, 1.5, 0.125, 0.75])   # (1/8 in the degenerate problems: kind b of the regularised step, Scenario)
ROWS = ([(s, dt, general, mode, 200) for s in kd.SHAPES for dt in (F32, F64) for general in (False, True) for mode in (2, 1)] +
        [(s, dt, False, 2, 7) for s in kd.SHAPES for dt in (F32, F64)])
ENTRIES = {"kkt_step": "ab", "kkt_step_reg": "ab", "kkt_resolve": "abc", "kkt_resolve_shared": "ac", "admm_step": "ac"}
STEP_OUT = ("S", "gamma", "Ginv", "Pinv", "lam", "z", "it", "fl")
RESOLVE_OUT = ("gamma", "lam", "z", "it", "fl")
ADMM_OUT = RESOLVE_OUT + ("w", "y", "gt", "res")
DENSE = {}


def row_id(r):
    (nx, nu, N), dt, general, mode, mi = r
    return f"{nx}-{nu}-{N}-{np.dtype(dt).name}-{'general' if general else 'default'}-mode{mode}-mi{mi}"


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.set_symmetric(2)
    s.close()


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype).reshape(-1))).cuda()


def host(o, keys):
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy().reshape(B, -1) for k in keys}


class Scenario:
    """One entry point on one handle: the kept factorisation (where the entry has one), the two sets of vectors (degenerate batch
    and twin) and the multipliers each starts from."""

    def __init__(self, s, entry, kind, shape, dtype, tol, mi):
        nx, nu, N = shape
        self.s, self.entry, self.kind, self.shape, self.dtype, self.tol, self.mi = s, entry, kind, shape, dtype, tol, mi
        self.td = torch.float32 if dtype == F32 else torch.float64
        d, twin = kd.batch(nx, nu, N, "b" if kind == "b" else "a")
        self.shared, self.reg = entry == "kkt_resolve_shared", entry in ("kkt_step_reg", "admm_step")
        self.step = entry in ("kkt_step", "kkt_step_reg")
        mats = slice(0, 1) if self.shared else slice(0, B)
        if self.reg and kind == "b":
            # the regularised step inverts G + rho I: the matrices of kind b are what it must find there, so G is handed over with
            # rho = 1/8 taken off its diagonal (1/8, 7/8, 31/8: exact in fp32, and the sum with rho is exact again)
            twin = dict(twin, G=np.stack([kd.add_rho(nx, nu, N, twin["G"][b], -RHO[b]) if b in kd.DEGENERATE else twin["G"][b]
                                          for b in range(B)]))
        self.Gh = np.stack([twin["G"][0 if self.shared else b] for b in range(B)])      # per problem, for the dense reference
        self.Ch = np.stack([twin["C"][0 if self.shared else b] for b in range(B)])
        self.G, self.C = dev(twin["G"][mats], dtype), (None if N == 1 else dev(twin["C"][mats], dtype))
        self.rho = dev(RHO, dtype) if self.reg else None
        if self.reg:
            self.Gh = np.stack([kd.add_rho(nx, nu, N, self.Gh[b], RHO[b]) for b in range(B)])
        sz = so.sizes(nx, nu, N)
        nm = 1 if self.shared else B
        self.nl, self.nz = sz["c"], sz["g"]
        if self.step:
            self.vec = {"deg": (d["g"], d["c"]), "twin": (twin["g"], twin["c"])}
            self.lam0 = {"deg": np.zeros((B, self.nl)), "twin": np.zeros((B, self.nl))}
            return
        # the factorisation: one regular step on the twin (at batch 1 on problem 0 for the shared form)
        self.S = torch.empty(nm * sz["S"], dtype=self.td, device="cuda")
        self.Pinv, self.Ginv = torch.empty_like(self.S), torch.empty_like(self.G)
        gamma = torch.empty(nm * self.nl, dtype=self.td, device="cuda")
        lam, z = torch.zeros_like(gamma), torch.empty(nm * self.nz, dtype=self.td, device="cuda")
        g, c = dev(twin["g"][mats], dtype), dev(twin["c"][mats], dtype)
        if self.reg:
            it, fl = s.kkt_step_reg(nx, nu, N, nm, self.G, self.C, g, c, self.rho, self.S, gamma, self.Ginv, self.Pinv, lam, z, tol=tol,
                                    max_iter=200)
        else:
            it, fl = s.kkt_step(nx, nu, N, nm, self.G, self.C, g, c, self.S, gamma, self.Ginv, self.Pinv, lam, z, tol=tol, max_iter=200)
        if self.shared:     # every problem's multipliers of the twin vectors, on the single matrices
            g, c = dev(twin["g"], dtype), dev(twin["c"], dtype)
            gamma, lam, z = gamma.repeat(B), torch.zeros(B * self.nl, dtype=self.td, device="cuda"), z.repeat(B)
            it, fl = s.kkt_resolve_shared(nx, nu, N, B, self.Ginv, self.C, g, c, self.S, self.Pinv, gamma, lam, z, tol=tol, max_iter=200)
        torch.cuda.synchronize()
        assert int(fl.sum()) == 0 and bool(torch.isfinite(lam).all())
        ng, nc = kd.new_vectors(nx, nu, N)
        g2, c2 = ng.copy(), nc.copy()
        for b in kd.DEGENERATE:
            g2[b], c2[b] = d["g"][b], 0.0
        self.vec = {"deg": (g2, c2), "twin": (ng, nc)}
        warm = lam.cpu().numpy().astype(F64).reshape(B, -1) if kind == "c" else np.zeros((B, self.nl))
        cold = warm.copy()
        cold[list(kd.DEGENERATE)] = 0.0
        self.lam0 = {"deg": cold, "twin": warm}

    def run(self, which, graph=False):
        """The entry point on fresh NaN-filled outputs; returns (host arrays [B, -1] by name, the residual norms behind the call)."""
        s, (nx, nu, N), td, nan = self.s, self.shape, self.td, float("nan")
        gh, ch = self.vec[which]
        g, c = dev(gh, self.dtype), dev(ch, self.dtype)
        nm = 1 if self.shared else B
        o = dict(gamma=torch.full((B * self.nl,), nan, dtype=td, device="cuda"), z=torch.full((B * self.nz,), nan, dtype=td, device="cuda"),
                 lam=dev(self.lam0[which], self.dtype), it=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                 fl=torch.full((B,), 9, dtype=torch.uint8, device="cuda"))
        tol, mi = self.tol, self.mi
        gr = None
        if self.step:
            o.update(S=torch.full((B * 3 * nx * nx * N,), nan, dtype=td, device="cuda"), Ginv=torch.full_like(self.G, nan))
            o["Pinv"] = torch.full_like(o["S"], nan)
            if self.reg:
                head = (nx, nu, N, B, self.G, self.C, g, c, self.rho, o["S"], o["gamma"], o["Ginv"], o["Pinv"], o["lam"])
                eager, capture = s.kkt_step_reg, s.graph_kkt_step_reg
            else:
                head = (nx, nu, N, B, self.G, self.C, g, c, o["S"], o["gamma"], o["Ginv"], o["Pinv"], o["lam"])
                eager, capture = s.kkt_step, s.graph_kkt_step
            if graph:
                gr = capture(*head, None, None, tol, mi, o["it"], o["fl"], o["z"])
            else:
                eager(*head, o["z"], tol=tol, max_iter=mi, iters=o["it"], max_iter_exit=o["fl"])
            keys = STEP_OUT
        elif self.entry == "admm_step":
            lo, hi = torch.full_like(g, -0.5), torch.full_like(g, 0.5)
            o.update(w=torch.zeros_like(g), y=torch.zeros_like(g), res=torch.full((B, 2), nan, dtype=td, device="cuda"))
            o["gt"] = s.admm_init(nx, nu, N, B, g, lo, hi, self.rho, o["w"], o["y"])     # w = y = 0: gt = g
            gt_in = o["gt"].clone()
            head = (nx, nu, N, B, self.Ginv, self.C, g, c, lo, hi, self.rho, self.S, self.Pinv, o["gamma"], o["lam"])
            if graph:
                s.reserve(g.element_size(), nx, N, B)
                gr = s.graph_admm_step(*head, None, None, tol, mi, o["it"], o["fl"], o["z"], o["w"], o["y"], o["gt"], o["res"])
            else:
                s.admm_step(*head, o["z"], o["w"], o["y"], o["gt"], res=o["res"], tol=tol, max_iter=mi, iters=o["it"], max_iter_exit=o["fl"])
            keys = ADMM_OUT
        else:
            head = (nx, nu, N, B, self.Ginv, self.C, g, c, self.S, self.Pinv, o["gamma"], o["lam"])
            eager, capture = ((s.kkt_resolve_shared, s.graph_kkt_resolve_shared) if self.shared else (s.kkt_resolve, s.graph_kkt_resolve))
            if graph:
                gr = capture(*head, None, None, tol, mi, o["it"], o["fl"], o["z"])
            else:
                eager(*head, o["z"], tol=tol, max_iter=mi, iters=o["it"], max_iter_exit=o["fl"])
            keys = RESOLVE_OUT
        if gr is not None:
            gr.launch()
        if self.entry == "admm_step":
            norms = s.kkt_residual_reg(nx, nu, N, B, self.G, self.C, gt_in, c, self.rho, o["z"], o["lam"])
        elif self.reg:
            norms = s.kkt_residual_reg(nx, nu, N, B, self.G, self.C, g, c, self.rho, o["z"], o["lam"])
        elif self.shared:
            norms = s.kkt_residual_shared(nx, nu, N, B, self.G, self.C, g, c, o["z"], o["lam"])
        else:
            norms = s.kkt_residual(nx, nu, N, B, self.G, self.C, g, c, o["z"], o["lam"])
        out = host(o, keys)
        if gr is not None:
            gr.close()
        return out, norms.cpu().numpy()


def check_case(sc, fresh, what):
    """sc: the scenario on the module's handle, fresh: the same on a handle nothing else ran on."""
    nx, nu, N = sc.shape
    deg, reg = kd.expected_masks()
    want, want_norms = fresh.run("twin")
    assert all(np.isfinite(want[k]).all() for k in ("gamma", "lam", "z")) and np.isfinite(want_norms).all(), what
    if sc.mi == 200:
        assert not want["fl"].any() and (want["it"] < 200).all(), what
    for graph in (False, True):
        got, norms = sc.run("deg", graph)
        tag = f"{what} {'graph' if graph else 'eager'}"
        finite = {k: bool(np.isfinite(got[k][deg]).any()) for k in ("lam", "z")}
        print(f"{tag}: degenerate iters {got['it'][deg].ravel().tolist()} flags {got['fl'][deg].ravel().tolist()} "
              f"finite entries in lambda {finite['lam']} in z {finite['z']} gamma all zero {not got['gamma'][deg].any()}; "
              f"regular iters {got['it'][reg].ravel().tolist()} flags {got['fl'][reg].ravel().tolist()}")
        assert not got["gamma"][deg].any(), tag                      # exactly zero, before anything is concluded from it
        assert (got["it"][deg] == sc.mi).all() and (got["fl"][deg] == 1).all(), tag
        assert not np.isfinite(got["lam"][deg]).any() and not np.isfinite(got["z"][deg]).any(), tag
        assert np.isnan(norms[deg]).all() and np.isfinite(norms[reg]).all(), (tag, norms)
        for k, v in got.items():
            assert np_same(v[reg], want[k][reg]), (tag, k)
        gh, ch = sc.vec["deg"]
        for b in kd.REGULAR:
            if got["fl"][b, 0]:
                assert sc.mi == 7, tag
                continue
            key = (sc.shape, sc.entry, sc.kind, b)      # (the same numbers in every precision, dispatch and mode)
            if key not in DENSE:
                DENSE[key] = so.dense_kkt_solve(nx, nu, N, sc.Gh[b], sc.Ch[b], gh[b], ch[b])
            oz, ol = DENSE[key]
            el = np.linalg.norm(got["lam"][b] - ol) / np.linalg.norm(ol)
            ez = np.linalg.norm(got["z"][b] - oz) / np.linalg.norm(oz)
            assert el <= EPS[sc.dtype] and ez <= EPS[sc.dtype], (tag, b, el, ez)
    after, _ = sc.run("twin")
    for k, v in after.items():
        assert np_same(v, want[k]), (what, "history", k)


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_zero_gamma_stays_in_its_problem(solver, monkeypatch, row):
    shape, dtype, general, mode, mi = row
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    fresh = binding.Solver(0)
    try:
        for s in (solver, fresh):
            s.set_symmetric(mode)
        for entry, kinds in ENTRIES.items():
            for kind in kinds:
                if kind not in kd.KINDS[shape]:
                    continue
                a, b = (Scenario(s, entry, kind, shape, dtype, PCG_TOL[dtype], mi) for s in (solver, fresh))
                check_case(a, b, f"{row_id(row)} {entry} kind {kind}")
    finally:
        solver.set_symmetric(2)
        fresh.close()


# ---- refinement at an exactly solved point
REFINE_TOL, REFINE_MAX_ITER = 1e-8, 100     # tests/test_gpu_kkt_refine.py


def refine_data(nx, nu, N, degenerate):
    d = so.gen(nx, nu, N, seed=700 + nx + N, batch=3, dtype=F64)
    if degenerate:
        d["g"][1], d["c"][1] = 0.0, 0.0
    return d


def refine_run(solver, nx, nu, N, d, graph):
    Bn = 3
    G, C, g, c = (dev(d[k], F64) for k in "GCgc")
    G32, C32 = solver.demote(G), solver.demote(C)
    S32, _, Ginv32 = solver.form_schur(nx, nu, N, Bn, G32, C32, solver.demote(g), solver.demote(c))
    Pinv32 = solver.form_pinv(nx, N, Bn, S32, binding.PINV_STAIR)
    w = solver.refine_work(nx, nu, N, Bn)
    for k in ("rg", "rc", "gamma", "dlam", "r", "p", "dz", "res"):
        w[k].fill_(float("nan"))
    z = torch.zeros(Bn * so.sizes(nx, nu, N)["g"], dtype=torch.float64, device="cuda")
    lam = torch.zeros(Bn * nx * N, dtype=torch.float64, device="cuda")
    if graph:
        gr = solver.graph_kkt_refine_step(nx, nu, N, Bn, G, C, g, c, Ginv32, C32, S32, Pinv32, z, lam, tol=REFINE_TOL,
                                          max_iter=REFINE_MAX_ITER, **w)
        gr.launch()
        torch.cuda.synchronize()
        gr.close()
    else:
        solver.kkt_defect_mixed(nx, nu, N, Bn, G, C, g, c, z, lam, rg=w["rg"], rc=w["rc"], dlam=w["dlam"], expo=w["expo"], res=w["res"])
        solver.kkt_resolve(nx, nu, N, Bn, Ginv32, C32, w["rg"], w["rc"], S32, Pinv32, w["gamma"], w["dlam"], w["dz"], r=w["r"], p=w["p"],
                           tol=REFINE_TOL, max_iter=REFINE_MAX_ITER, iters=w["iters"], max_iter_exit=w["max_iter_exit"])
        solver.kkt_refine_apply(nx, nu, N, Bn, w["dz"], w["dlam"], w["expo"], z, lam)
    torch.cuda.synchronize()
    out = {k: w[k].cpu().numpy().reshape(Bn, -1) for k in ("rg", "rc", "gamma", "dlam", "dz", "expo", "res", "iters", "max_iter_exit")}
    out.update(z=z.cpu().numpy().reshape(Bn, -1), lam=lam.cpu().numpy().reshape(Bn, -1))
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["three-calls", "graph"])
@pytest.mark.parametrize("nx,nu,N", [(14, 7, 24), (5, 3, 10)])
def test_refinement_at_an_exactly_solved_point(solver, nx, nu, N, graph):
    got = refine_run(solver, nx, nu, N, refine_data(nx, nu, N, True), graph)
    want = refine_run(solver, nx, nu, N, refine_data(nx, nu, N, False), graph)
    print(f"refine ({nx},{nu},{N}) {'graph' if graph else 'three calls'}: problem 1 res {got['res'][1].tolist()} expo {got['expo'][1].tolist()} "
          f"iters {got['iters'][1].tolist()} flag {got['max_iter_exit'][1].tolist()}; finite entries left in z {int(np.isfinite(got['z'][1]).sum())} "
          f"of {got['z'][1].size}, in lambda {int(np.isfinite(got['lam'][1]).sum())} of {got['lam'][1].size}")
    assert (got["res"][1] == 0).all() and got["expo"][1, 0] == rref.exponent(0.0, 0.0) == 0
    assert not got["rg"][1].any() and not got["rc"][1].any() and not got["gamma"][1].any()
    assert got["iters"][1, 0] == REFINE_MAX_ITER and got["max_iter_exit"][1, 0] == 1
    assert not np.isfinite(got["dlam"][1]).any() and not np.isfinite(got["dz"][1]).any()
    # as found: the apply adds the NaN correction, the exactly solved point is lost
    assert np.isnan(got["z"][1]).all() and np.isnan(got["lam"][1]).all()
    for k, v in got.items():
        for b in (0, 2):
            assert np_same(v[b], want[k][b]), (k, b)
        assert np.isfinite(want[k][[0, 2]]).all(), k
    assert not want["max_iter_exit"].any()


def test_three_calls_and_graph_agree_on_the_lost_point(solver):
    nx, nu, N = 5, 3, 10
    a = refine_run(solver, nx, nu, N, refine_data(nx, nu, N, True), False)
    b = refine_run(solver, nx, nu, N, refine_data(nx, nu, N, True), True)
    for k in a:
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])) and np_same(np.nan_to_num(a[k]), np.nan_to_num(b[k])), k
