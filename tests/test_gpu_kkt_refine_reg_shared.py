"""The regularised and the shared-matrix forms of the mixed-precision KKT refinement on the device (csrc/kkt_refine.hip, REG and
SHARED, through the C ABI).  PARITY UNPINNED: the reference tree has no code, fixture or output for this.

Bits: tests/kkt_refine_reg_ref.py restates the _reg defect (kkt_refine_ref.defect_mixed_ref on G with np.float64(d + rho) on the
diagonals); d_rg, d_rc, d_expo equal it exactly, d_res equals gbdpcg_kkt_residual_reg_f64 of the same point.  The _shared forms
equal the plain calls on `batch` tiled copies of the matrices, and each step equals its three calls.

Convergence of the _reg step: data whose R_k are all zero (the plain formation divides by a zero pivot there), rho in {2^-3, 0.5,
1}, from z = lambda = 0 until for every problem
    m_s <= (2 nx + 2) u64 mag_s   and   m_f <= (nx + nu + 2) u64 mag_f
with the norms of gbdpcg_kkt_residual_reg_f64 and the magnitudes of the dense G + rho I: inside within 2 N0 = 12 steps (N0: what
the numpy emulation of tests/test_kkt_refine_reg_reference.py needs with an inner solve that is only 1e-3 accurate), the point
after step 1 outside by at least 2^20, no growth beyond 2x once below 1e-12 -- and the plain step on the same regularised
factorisation is NOT inside after the same number of steps.  Correction solve: tol = 1e-8, max_iter = 100, as in
tests/test_gpu_kkt_refine.py."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kkt_refine_ref as ref  # noqa: E402
import kkt_refine_reg_ref as reg  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
QUAD = [(14, 7, 1, 2), (14, 7, 17, 3), (14, 7, 33, 2), (5, 2, 9, 2)]   # N = 1: no C; 17, 33 straddle the 16-knot pass
ANY = [(3, 3, 2, 1), (4, 6, 3, 2), (1, 1, 4, 1)]
CASES = [(s, False) for s in QUAD + ANY] + [(s, True) for s in QUAD]     # (shape, GBDPCG_SCHUR_GENERAL=1)
STEPS = [(14, 7, 17, 3), (4, 6, 3, 2)]
TOL, MAX_ITER = 1e-8, 100
N0 = reg.N0


def case_id(c):
    return "-".join(map(str, c[0])) + ("-general" if c[1] else "")


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the cached references are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def rho_of(B):
    """Distinct per problem and no power of two: d + rho rounds."""
    return np.array([0.3 + 0.41 * b for b in range(B)], F64)


@functools.lru_cache(maxsize=None)
def problem(nx, nu, N, B):
    """Genuine fp64 data and one random fp64 point per problem, computed once.  The seed is that of tests/test_gpu_kkt_refine.py:
    the same matrices as the plain tests there."""
    seed = 700 + nx + N
    d = so.gen(nx, nu, N, seed=seed, batch=B, dtype=F64)
    rng = np.random.default_rng(seed + 1)
    z, lam = rng.standard_normal(d["g"].shape), rng.standard_normal(d["c"].shape)
    for v in list(d.values()) + [z, lam]:
        v.setflags(write=False)
    return d, z, lam


@functools.lru_cache(maxsize=None)
def reg_reference(nx, nu, N, B):
    """(rg [B, nz], rc [B, nl], expo [B], norms [B, 2]) of the Fraction reference of the _reg defect, computed once."""
    d, z, lam = problem(nx, nu, N, B)
    rho = rho_of(B)
    out = [reg.defect_mixed_reg_ref(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b], rho[b], z[b], lam[b]) for b in range(B)]
    res = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
           np.array([o[3] for o in out], F64))
    for v in res:
        v.setflags(write=False)
    return res


def device_data(d, N):
    G, C, g, c = (dev(d[k].reshape(-1)) for k in "GCgc")
    return G, (None if N == 1 else C), g, c   # N == 1: there is no C


def run_defect(solver, nx, nu, N, B, data, z, lam, fill, rho=None, shared=False):
    """One defect launch (plain, _reg with rho, or _shared) on outputs pre-filled with `fill`; everything back on the host."""
    nz, nl = (nx + nu) * N - nu, nx * N
    rg = torch.full((B * nz,), fill, dtype=torch.float32, device="cuda")
    rc, dl = (torch.full((B * nl,), fill, dtype=torch.float32, device="cuda") for _ in range(2))
    expo = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
    res = torch.full((B, 2), fill, dtype=torch.float64, device="cuda")
    out = dict(rg=rg, rc=rc, dlam=dl, expo=expo, res=res)
    if rho is not None:
        solver.kkt_defect_mixed_reg(nx, nu, N, B, *data, rho, z, lam, **out)
    elif shared:
        solver.kkt_defect_mixed_shared(nx, nu, N, B, *data, z, lam, **out)
    else:
        solver.kkt_defect_mixed(nx, nu, N, B, *data, z, lam, **out)
    torch.cuda.synchronize()
    return (rg.cpu().numpy().reshape(B, nz), rc.cpu().numpy().reshape(B, nl), dl.cpu().numpy(), expo.cpu().numpy(),
            res.cpu().numpy())


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---- 1. the _reg defect
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reg_defect_bits(solver, monkeypatch, case):
    """rg, rc, expo against the Fraction reference, res against gbdpcg_kkt_residual_reg_f64, the zeros of dlambda; NaN-filled and
    1e30-filled outputs give the same bits; rho = 0 gives the plain call."""
    (nx, nu, N, B), general = case
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    d, zh, lh = problem(nx, nu, N, B)
    data = device_data(d, N)
    z, lam, rho = dev(zh.reshape(-1)), dev(lh.reshape(-1)), dev(rho_of(B))
    wrg, wrc, wexpo, wres = reg_reference(nx, nu, N, B)
    norms = solver.kkt_residual_reg(nx, nu, N, B, *data, rho, z, lam).cpu().numpy()
    first = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"), rho=rho)
    rg, rc, dl, expo, res = first
    print(f"({nx},{nu},{N},{B}) general {general}: expo {expo.tolist()} norms {res.tolist()}")
    assert np.array_equal(bits(res), bits(norms))
    assert np.array_equal(bits(res), bits(wres))
    assert np.array_equal(expo, wexpo)
    assert np.array_equal(bits(rg), bits(wrg)) and np.array_equal(bits(rc), bits(wrc))
    assert not dl.any() and not np.signbit(dl).any()
    assert same(first, run_defect(solver, nx, nu, N, B, data, z, lam, 1e30, rho=rho))
    plain = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"))
    assert not np.array_equal(bits(plain[0]), bits(rg))                  # rho is in it
    zero = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"), rho=torch.zeros_like(rho))
    assert same(zero, plain)


@pytest.mark.parametrize("nx,nu,N,B", QUAD)
def test_reg_quad_and_any_size_kernels_agree(solver, monkeypatch, nx, nu, N, B):
    d, zh, lh = problem(nx, nu, N, B)
    data = device_data(d, N)
    z, lam, rho = dev(zh.reshape(-1)), dev(lh.reshape(-1)), dev(rho_of(B))
    quad = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"), rho=rho)
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    assert same(quad, run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"), rho=rho))


@pytest.mark.parametrize("general", [False, True])
def test_nan_in_rho_stays_inside_its_problem(solver, monkeypatch, general):
    """NaN in rho_1: e_1 = 0 and a NaN stationarity norm there, problems 0 and 2 keep every bit of the clean run."""
    nx, nu, N, B = 14, 7, 17, 3
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    d, zh, lh = problem(nx, nu, N, B)
    data = device_data(d, N)
    z, lam, rho = dev(zh.reshape(-1)), dev(lh.reshape(-1)), dev(rho_of(B))
    clean = run_defect(solver, nx, nu, N, B, data, z, lam, 7.0, rho=rho)
    bad = rho.clone()
    bad[1] = float("nan")
    rg, rc, dl, expo, res = run_defect(solver, nx, nu, N, B, data, z, lam, 7.0, rho=bad)
    assert expo[1] == 0 and np.isnan(res[1, 0]), (expo, res)
    assert np.array_equal(bits(res[1, 1]), bits(clean[4][1, 1]))         # the feasibility rows do not contain G
    assert np.isnan(rg[1]).any() and not dl.any()
    for b in (0, 2):
        for a, w in zip((rg, rc, expo, res), (clean[0], clean[1], clean[3], clean[4])):
            assert np.array_equal(bits(a[b]), bits(w[b])), b


# ---- 2. the _shared defect
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shared_defect_bits(solver, monkeypatch, case):
    """Every output equals the plain call on `batch` tiled copies of G and C; res equals gbdpcg_kkt_residual_shared_f64.  The one
    G and C are tensors of exactly one problem's size, and in a second run the head of buffers whose "problem 1 .." is NaN: a read
    past one problem's extent would change bits."""
    (nx, nu, N, B), general = case
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    d, zh, lh = problem(nx, nu, N, B)
    z, lam, g, c = dev(zh.reshape(-1)), dev(lh.reshape(-1)), dev(d["g"].reshape(-1)), dev(d["c"].reshape(-1))
    G1, C1 = dev(d["G"][0]), (None if N == 1 else dev(d["C"][0]))
    tiled = (dev(np.tile(d["G"][0], B)), None if N == 1 else dev(np.tile(d["C"][0], B)), g, c)
    want = run_defect(solver, nx, nu, N, B, tiled, z, lam, float("nan"))
    got = run_defect(solver, nx, nu, N, B, (G1, C1, g, c), z, lam, float("nan"), shared=True)
    assert same(got, want)
    assert same(got, run_defect(solver, nx, nu, N, B, (G1, C1, g, c), z, lam, 1e30, shared=True))
    norms = solver.kkt_residual_shared(nx, nu, N, B, G1, C1, g, c, z, lam).cpu().numpy()
    assert np.array_equal(bits(got[4]), bits(norms))
    assert not got[2].any() and not np.signbit(got[2]).any()

    def poisoned(a):
        buf = torch.full((2 * a.numel(),), float("nan"), dtype=torch.float64, device="cuda")
        buf[:a.numel()] = a
        return buf
    Gn, Cn = poisoned(G1), (None if C1 is None else poisoned(C1))
    assert same(got, run_defect(solver, nx, nu, N, B, (Gn, Cn, g, c), z, lam, float("nan"), shared=True))


# ---- 3. the steps are their three calls
def demote_opt(solver, t):
    return None if t is None else solver.demote(t)


def kept_reg(solver, nx, nu, N, B, data, rho):
    """The kept fp32 factorisation of the demoted G + rho I: what gbdpcg_kkt_step_reg_f32 forms (formation, then Phi^-1)."""
    G, C, g, c = data
    C32 = demote_opt(solver, C)
    S32, _, Ginv32 = solver.form_schur_reg(nx, nu, N, B, solver.demote(G), C32, solver.demote(g), solver.demote(c), solver.demote(rho))
    return Ginv32, C32, S32, solver.form_pinv(nx, N, B, S32, binding.PINV_STAIR)


def kept_plain(solver, nx, nu, N, B, data):
    G, C, g, c = data
    C32 = demote_opt(solver, C)
    S32, _, Ginv32 = solver.form_schur(nx, nu, N, B, solver.demote(G), C32, solver.demote(g), solver.demote(c))
    return Ginv32, C32, S32, solver.form_pinv(nx, N, B, S32, binding.PINV_STAIR)


def fresh_state(solver, nx, nu, N, B):
    w = solver.refine_work(nx, nu, N, B)
    for k in ("rg", "rc", "gamma", "dlam", "r", "p", "dz", "res"):
        w[k].fill_(float("nan"))
    nz, nl = B * ((nx + nu) * N - nu), B * nx * N
    return torch.zeros(nz, dtype=torch.float64, device="cuda"), torch.zeros(nl, dtype=torch.float64, device="cuda"), w


def snapshot(z, lam, w):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (z, lam, w["rg"], w["rc"], w["dz"], w["dlam"], w["expo"], w["res"], w["iters"])]


@pytest.mark.parametrize("nx,nu,N,B", STEPS)
def test_reg_step_is_the_three_calls(solver, nx, nu, N, B):
    """gbdpcg_kkt_refine_step_reg against defect_reg + kkt_resolve_f32 + apply, two steps from zero: eager, and as one graph
    replayed twice; then rho is rewritten IN PLACE and the next replay equals a fresh eager step with the new rho."""
    d, _, _ = problem(nx, nu, N, B)
    data = device_data(d, N)
    rho = dev(rho_of(B))
    fac = kept_reg(solver, nx, nu, N, B, data, rho)
    opts = dict(tol=TOL, max_iter=MAX_ITER)

    z, lam, w = fresh_state(solver, nx, nu, N, B)
    want = []
    for _ in range(2):
        solver.kkt_defect_mixed_reg(nx, nu, N, B, *data, rho, z, lam, rg=w["rg"], rc=w["rc"], dlam=w["dlam"], expo=w["expo"], res=w["res"])
        solver.kkt_resolve(nx, nu, N, B, fac[0], fac[1], w["rg"], w["rc"], fac[2], fac[3], w["gamma"], w["dlam"], w["dz"], r=w["r"],
                           p=w["p"], iters=w["iters"], max_iter_exit=w["max_iter_exit"], **opts)
        solver.kkt_refine_apply(nx, nu, N, B, w["dz"], w["dlam"], w["expo"], z, lam)
        want.append(snapshot(z, lam, w))
    assert np.abs(want[1][7]).max() < 1e-3 * np.abs(want[0][7]).max()       # the second step started from a refined point

    z, lam, w = fresh_state(solver, nx, nu, N, B)
    for i in range(2):
        solver.kkt_refine_step_reg(nx, nu, N, B, *data, rho, *fac, z, lam, **opts, **w)
        assert same(snapshot(z, lam, w), want[i]), ("eager", i)

    z, lam, w = fresh_state(solver, nx, nu, N, B)
    grho = rho.clone()
    graph = solver.graph_kkt_refine_step_reg(nx, nu, N, B, *data, grho, *fac, z, lam, **opts, **w)
    for i in range(2):
        graph.launch()
        assert same(snapshot(z, lam, w), want[i]), ("graph", i)
    # the pointer is kept: new values behind it, the same kept factorisation, against an eager step from the same point
    new = dev(rho_of(B)[::-1] * 1.7)
    ze, le, we = fresh_state(solver, nx, nu, N, B)
    ze.copy_(z), le.copy_(lam)
    solver.kkt_refine_step_reg(nx, nu, N, B, *data, new, *fac, ze, le, **opts, **we)
    fresh = snapshot(ze, le, we)
    grho.copy_(new)
    graph.launch()
    got = snapshot(z, lam, w)
    graph.close()
    assert same(got, fresh)
    assert not np.array_equal(bits(got[7]), bits(want[1][7]))


@pytest.mark.parametrize("nx,nu,N,B", STEPS)
def test_shared_step_is_the_three_calls_and_the_plain_step_on_copies(solver, nx, nu, N, B):
    """gbdpcg_kkt_refine_step_shared against defect_shared + kkt_resolve_shared_f32 + apply, eager and as a graph; and against the
    plain step on `batch` copies of the matrices with the path set to GBDPCG_PATH_FUSED, as the shared solve defines it."""
    d, _, _ = problem(nx, nu, N, B)
    g, c = dev(d["g"].reshape(-1)), dev(d["c"].reshape(-1))
    one = (dev(d["G"][0]), dev(d["C"][0]), g[:g.numel() // B].clone(), c[:c.numel() // B].clone())
    fac = kept_plain(solver, nx, nu, N, 1, one)
    data = (one[0], one[1], g, c)
    opts = dict(tol=TOL, max_iter=MAX_ITER)

    z, lam, w = fresh_state(solver, nx, nu, N, B)
    want = []
    for _ in range(2):
        solver.kkt_defect_mixed_shared(nx, nu, N, B, *data, z, lam, rg=w["rg"], rc=w["rc"], dlam=w["dlam"], expo=w["expo"], res=w["res"])
        solver.kkt_resolve_shared(nx, nu, N, B, fac[0], fac[1], w["rg"], w["rc"], fac[2], fac[3], w["gamma"], w["dlam"], w["dz"],
                                  r=w["r"], p=w["p"], iters=w["iters"], max_iter_exit=w["max_iter_exit"], **opts)
        solver.kkt_refine_apply(nx, nu, N, B, w["dz"], w["dlam"], w["expo"], z, lam)
        want.append(snapshot(z, lam, w))
    assert np.abs(want[1][7]).max() < 1e-3 * np.abs(want[0][7]).max()

    z, lam, w = fresh_state(solver, nx, nu, N, B)
    for i in range(2):
        solver.kkt_refine_step_shared(nx, nu, N, B, *data, *fac, z, lam, **opts, **w)
        assert same(snapshot(z, lam, w), want[i]), ("eager", i)

    z, lam, w = fresh_state(solver, nx, nu, N, B)
    graph = solver.graph_kkt_refine_step_shared(nx, nu, N, B, *data, *fac, z, lam, **opts, **w)
    for i in range(2):
        graph.launch()
        assert same(snapshot(z, lam, w), want[i]), ("graph", i)
    graph.close()

    tiled = (dev(np.tile(d["G"][0], B)), dev(np.tile(d["C"][0], B)), g, c)
    tfac = tuple(t.repeat(B) for t in fac)
    z, lam, w = fresh_state(solver, nx, nu, N, B)
    solver.set_path(binding.PATH_FUSED)
    try:
        for i in range(2):
            solver.kkt_refine_step(nx, nu, N, B, *tiled, *tfac, z, lam, **opts, **w)
            assert same(snapshot(z, lam, w), want[i]), ("plain on copies", i)
    finally:
        solver.set_path(binding.PATH_AUTO)


# ---- 4., 5. convergence
def ratios(nx, nu, N, B, dense, z, lam, norms):
    """Per problem: (norm / mag [2], norm / bound [2]) at the point (z, lam) with the device's norms; dense(b) -> Gd, Cd, g, c."""
    rel, out = np.zeros((B, 2)), np.zeros((B, 2))
    for b in range(B):
        Gd, Cd, g, c = dense(b)
        mag = ref.magnitudes(Gd, Cd, g, c, z[b], lam[b])
        rel[b] = norms[b] / np.array(mag)
        out[b] = norms[b] / np.array(ref.floor(nx, nu, mag))
    return rel, out


def refine_loop(label, B, launch, norms_of, ratios_of, steps, z, lam, w):
    """`steps` launches at the most; stops two steps behind the first point inside the bounds.  Returns (reached, history)."""
    history, reached = [], None
    for step in range(1, steps + 1):
        launch()
        norms = norms_of()
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            rel, over = ratios_of(z.cpu().numpy().reshape(B, -1), lam.cpu().numpy().reshape(B, -1), norms.cpu().numpy())
        history.append((rel.max(axis=1), over.max(axis=1)))
        print(f"{label} after step {step}: norm / bound per problem {over.max(axis=1)}  PCG iterations {w['iters'].cpu().tolist()}")
        if reached is None and (over <= 1.0).all():
            reached = step
        if reached is not None and step >= reached + 2:      # two more steps: the point has to stay where it is
            break
    return reached, history


def check_history(reached, history, steps):
    assert reached is not None, f"not inside the bounds within {steps} steps"
    assert all(np.isfinite(o).all() for _, o in history)
    assert (history[0][1] >= 2.0 ** 20).all(), history[0][1]            # fp32 alone does not pass
    for (r0, _), (r1, _) in zip(history, history[1:]):
        settled = r0 < 1e-12
        assert (r1[settled] <= 2.0 * r0[settled]).all(), (r0, r1)


@functools.lru_cache(maxsize=None)
def semidefinite(nx, nu, N, B):
    """The data of problem() with every R_k = 0, and rho_b from {2^-3, 0.5, 1}."""
    d, _, _ = problem(nx, nu, N, B)
    d = dict(d, G=np.stack([reg.zero_inputs(nx, nu, N, d["G"][b]) for b in range(B)]))
    rho = np.array([reg.RHOS[b % 3] for b in range(B)], F64)
    d["G"].setflags(write=False)
    return d, rho


def test_the_plain_formation_fails_on_semidefinite_data(solver):
    """The reason for _reg: R_k = 0 has no inverse, the plain fp32 formation writes non-finite blocks; the _reg one does not."""
    nx, nu, N, B = 5, 2, 9, 2
    d, rho = semidefinite(nx, nu, N, B)
    G, C, g, c = (solver.demote(t) for t in device_data(d, N))
    S, _, Ginv = solver.form_schur(nx, nu, N, B, G, C, g, c)
    Sr, _, Gr = solver.form_schur_reg(nx, nu, N, B, G, C, g, c, solver.demote(dev(rho)))
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(S).all()) and not bool(torch.isfinite(Ginv).all())
    assert bool(torch.isfinite(Sr).all()) and bool(torch.isfinite(Gr).all())


@pytest.mark.parametrize("nx,nu,N,B", QUAD + ANY)
def test_reg_refinement_reaches_the_regularised_fp64_floor(solver, nx, nu, N, B):
    d, rhoh = semidefinite(nx, nu, N, B)
    data, rho = device_data(d, N), dev(rhoh)
    fac = kept_reg(solver, nx, nu, N, B, data, rho)
    steps = 2 * N0

    @functools.lru_cache(maxsize=None)
    def dense(b):
        return so.dense_kkt(nx, nu, N, reg.regularised(nx, nu, N, d["G"][b], rhoh[b]), d["C"][b], d["g"][b], d["c"][b])

    def run(label, make):
        z, lam, w = fresh_state(solver, nx, nu, N, B)
        graph = make(z, lam, w)
        out = refine_loop(f"({nx},{nu},{N},{B}) {label}", B, graph.launch,
                          lambda: solver.kkt_residual_reg(nx, nu, N, B, *data, rho, z, lam),      # the point this step wrote
                          lambda zz, ll, nn: ratios(nx, nu, N, B, dense, zz, ll, nn), steps, z, lam, w)
        graph.close()
        return out

    reached, history = run("_reg", lambda z, lam, w: solver.graph_kkt_refine_step_reg(nx, nu, N, B, *data, rho, *fac, z, lam, tol=TOL,
                                                                                     max_iter=MAX_ITER, **w))
    print(f"({nx},{nu},{N},{B}): the regularised floor is reached after {reached} steps (allowed {steps})")
    check_history(reached, history, steps)
    # the plain step on the same regularised factorisation: rho only in the factorisation, never inside in the same number of steps
    preached, phistory = run("plain defect", lambda z, lam, w: solver.graph_kkt_refine_step(nx, nu, N, B, *data, *fac, z, lam, tol=TOL,
                                                                                            max_iter=MAX_ITER, **w))
    print(f"({nx},{nu},{N},{B}): plain defect on the regularised factorisation, norm / bound at the end {phistory[-1][1]}")
    assert preached is None and len(phistory) == steps
    assert not (phistory[-1][1] <= 2.0 ** 20).any()


@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 17, 3), (5, 2, 9, 2)])
def test_shared_refinement_reaches_the_fp64_floor(solver, nx, nu, N, B):
    """One plant, `batch` states: the rule of test_refinement_reaches_the_fp64_floor (12 steps)."""
    d, _, _ = problem(nx, nu, N, B)
    g, c = dev(d["g"].reshape(-1)), dev(d["c"].reshape(-1))
    one = (dev(d["G"][0]), dev(d["C"][0]), g[:g.numel() // B].clone(), c[:c.numel() // B].clone())
    fac = kept_plain(solver, nx, nu, N, 1, one)
    data = (one[0], one[1], g, c)
    z, lam, w = fresh_state(solver, nx, nu, N, B)
    graph = solver.graph_kkt_refine_step_shared(nx, nu, N, B, *data, *fac, z, lam, tol=TOL, max_iter=MAX_ITER, **w)
    reached, history = refine_loop(f"({nx},{nu},{N},{B}) _shared", B, graph.launch,
                                   lambda: solver.kkt_residual_shared(nx, nu, N, B, *data, z, lam),
                                   lambda zz, ll, nn: ratios(nx, nu, N, B, lambda b: so.dense_kkt(nx, nu, N, d["G"][0], d["C"][0],
                                                                                                  d["g"][b], d["c"][b]), zz, ll, nn),
                                   12, z, lam, w)
    graph.close()
    print(f"({nx},{nu},{N},{B}): the floor is reached after {reached} steps")
    check_history(reached, history, 12)


def test_kkt_solve_refined_takes_rho_and_shared(solver):
    nx, nu, N, B = 5, 2, 9, 2
    d, rhoh = semidefinite(nx, nu, N, B)
    data, rho = device_data(d, N), dev(rhoh)
    fac = kept_reg(solver, nx, nu, N, B, data, rho)
    z, lam, history = solver.kkt_solve_refined(nx, nu, N, B, *data, *fac, max_steps=12, stop_s=1e-12, stop_f=1e-12, tol=TOL,
                                               max_iter=MAX_ITER, rho=rho)
    assert 2 <= len(history) < 12 and (history[-1] <= 1e-12).all()
    assert (solver.kkt_residual_reg(nx, nu, N, B, *data, rho, z, lam).cpu().numpy() <= 1e-12).all()
    p, _, _ = problem(nx, nu, N, B)
    g, c = dev(p["g"].reshape(-1)), dev(p["c"].reshape(-1))
    one = (dev(p["G"][0]), dev(p["C"][0]), g[:g.numel() // B].clone(), c[:c.numel() // B].clone())
    sfac = kept_plain(solver, nx, nu, N, 1, one)
    z, lam, history = solver.kkt_solve_refined(nx, nu, N, B, one[0], one[1], g, c, *sfac, max_steps=12, stop_s=1e-12, stop_f=1e-12,
                                               tol=TOL, max_iter=MAX_ITER, shared=True)
    assert 2 <= len(history) < 12
    assert (solver.kkt_residual_shared(nx, nu, N, B, one[0], one[1], g, c, z, lam).cpu().numpy() <= 1e-12).all()
    with pytest.raises(ValueError):
        solver.kkt_solve_refined(nx, nu, N, B, one[0], one[1], g, c, *sfac, rho=rho, shared=True)


# ---- 6. refusals
def test_bad_arguments(solver):
    """All six: null d_rho, null required pointers, zero sizes: INVALID (1); a block size form_schur refuses: UNSUPPORTED (4); a
    null `out` of the graph forms: INVALID; nothing written.  N == 1 with d_C == NULL is accepted."""
    nx, nu, N, B = 6, 3, 4, 3
    lib = solver.lib
    buf64 = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    buf32 = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    out = {k: torch.full((1 << 12,), 777.0, dtype=dt, device="cuda")
           for k, dt in (("rg", torch.float32), ("rc", torch.float32), ("dlam", torch.float32), ("gamma", torch.float32),
                         ("dz", torch.float32), ("z", torch.float64), ("lam", torch.float64), ("res", torch.float64))}
    out["expo"] = torch.full((64,), 777, dtype=torch.int32, device="cuda")
    out["iters"] = torch.full((64,), 777, dtype=torch.int32, device="cuda")
    P64, P32 = ctypes.c_void_p(buf64.data_ptr()), ctypes.c_void_p(buf32.data_ptr())
    O = {k: ctypes.c_void_p(v.data_ptr()) for k, v in out.items()}
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((v == 777).all()) for v in out.values())

    def check(fn, base, nullable, tail):
        for k in base:
            if k in nullable:
                continue
            if k in ("nx", "nu", "N", "batch"):
                assert fn(*dict(base, **{k: 0}).values(), *tail) == 1, k
            elif k not in ("tol", "max_iter"):
                assert fn(*dict(base, **{k: None}).values(), *tail) == 1, k
        assert fn(*dict(base, nx=80, nu=40).values(), *tail) == 4
        assert untouched()

    sizes = dict(h=solver.h, nx=nx, nu=nu, N=N, batch=B)
    for suffix, extra in (("reg", dict(rho=P64)), ("shared", {})):
        head = dict(sizes, G=P64, C=P64, g=P64, c=P64, **extra)         # rho directly behind c
        defect = dict(head, z=P64, lam=P64, rg=O["rg"], rc=O["rc"], dlam=O["dlam"], expo=O["expo"], res=O["res"])
        fn = getattr(lib, f"gbdpcg_kkt_defect_mixed_{suffix}")
        check(fn, defect, {"dlam"}, (s,))
        step = dict(head, Ginv=P32, C32=P32, S=P32, Pinv=P32, rg=O["rg"], rc=O["rc"], gamma=O["gamma"], dlam=O["dlam"], r=None, p=None,
                    dz=O["dz"], tol=1e-6, max_iter=10, iters=O["iters"], flags=None, expo=O["expo"], z=O["z"], lam=O["lam"],
                    res=O["res"])
        check(getattr(lib, f"gbdpcg_kkt_refine_step_{suffix}"), step, {"Pinv", "r", "p", "flags"}, (s,))
        graph = ctypes.c_void_p()
        create = getattr(lib, f"gbdpcg_graph_create_kkt_refine_step_{suffix}")
        check(create, step, {"Pinv", "r", "p", "flags"}, (ctypes.byref(graph),))
        assert not graph.value
        assert create(*step.values(), None) == 1
        assert untouched()
        if suffix == "reg":
            assert "rho" in defect and list(defect).index("rho") == list(defect).index("c") + 1
    # N == 1: there is no C; dlambda may be NULL
    for suffix, extra in (("shared", {}), ("reg", dict(rho=P64))):
        head = dict(sizes, G=P64, C=P64, g=P64, c=P64, **extra)
        defect = dict(head, z=P64, lam=P64, rg=O["rg"], rc=O["rc"], dlam=O["dlam"], expo=O["expo"], res=O["res"])
        fn = getattr(lib, f"gbdpcg_kkt_defect_mixed_{suffix}")
        for v in out.values():
            v.fill_(777)
        assert fn(*dict(defect, N=1, C=None, dlam=None).values(), s) == 0
        torch.cuda.synchronize()
        assert bool((out["dlam"] == 777.0).all()) and bool((out["rg"][:B * nx] == 0).all()) and bool((out["expo"][:B] == 0).all())
