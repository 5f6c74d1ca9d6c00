"""Mixed-precision KKT refinement on the device (csrc/kkt_refine.hip through the C ABI): the fp64 defect as a scaled fp32 right-hand
side, the fp64 accumulation, the step composed of them and gbdpcg_kkt_resolve_f32, and the convergence of that step to the fp64
rounding floor.  PARITY UNPINNED: the reference tree has no code, fixture or output for this.

Bits: tests/kkt_refine_ref.py restates the defect as exact rational fma chains rounded once, the exponent rule, the scaling and
the apply line; d_rg, d_rc, d_expo must equal it exactly, d_res must equal gbdpcg_kkt_residual_f64 of the same point.

Convergence: from z = lambda = 0 on the factorisation of the demoted G and C, until for every problem
    m_s <= (2 nx + 2) u64 mag_s   and   m_f <= (nx + nu + 2) u64 mag_f
(mag as in evaluate() of tests/test_gpu_kkt_residual.py) -- the derived error of evaluating the residual at all, so a point inside
the bounds cannot be told from the exact solution by an fp64 residual.  Required: inside within 12 steps (twice what the numpy
emulation of tests/test_kkt_refine_reference.py needs with an inner solve that is only 1e-3 accurate), the point after step 1
OUTSIDE by at least 2^20 (fp32 alone does not pass), and no growth by more than 2x between steps once below 1e-12.
Correction solve: tol = 1e-8 on a right-hand side of max-norm in [1, 2), max_iter = 100 -- the setting tests/test_gpu_kkt_residual.py
uses for an fp32 step on data of order 1."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kkt_refine_ref as ref  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
QUAD = [(14, 7, 1, 2), (14, 7, 2, 1), (14, 7, 17, 3), (14, 7, 33, 2), (12, 4, 33, 2), (5, 2, 9, 2)]   # N = 17, 33 straddle the 16-row pass
ANY = [(3, 3, 2, 1), (4, 6, 3, 2), (1, 1, 4, 1)]
CASES = [(s, False) for s in QUAD + ANY] + [(s, True) for s in QUAD]     # (shape, GBDPCG_SCHUR_GENERAL=1)
POINTS = ("solution", "solution + 1e-3 noise", "random")
TOL, MAX_ITER = 1e-8, 100


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


@functools.lru_cache(maxsize=None)
def problem(nx, nu, N, B):
    """Genuine fp64 data (not fp32-representable) and the three fp64 points per problem, computed once."""
    seed = 700 + nx + N
    d = so.gen(nx, nu, N, seed=seed, batch=B, dtype=F64)
    rng = np.random.default_rng(seed + 1)
    sol = [so.dense_kkt_solve(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b]) for b in range(B)]
    z0, l0 = np.stack([s[0] for s in sol]), np.stack([s[1] for s in sol])
    pts = [(z0, l0),
           (z0 + 1e-3 * rng.standard_normal(z0.shape), l0 + 1e-3 * rng.standard_normal(l0.shape)),
           (rng.standard_normal(z0.shape), rng.standard_normal(l0.shape))]
    for v in list(d.values()) + [v for p in pts for v in p]:
        v.setflags(write=False)
    assert not np.array_equal(d["G"], d["G"].astype(F32).astype(F64))
    return d, pts


@functools.lru_cache(maxsize=None)
def reference(nx, nu, N, B, kind):
    """(rg [B, nz], rc [B, nl], expo [B], norms [B, 2]) of the Fraction reference at the point of this kind, computed once."""
    d, pts = problem(nx, nu, N, B)
    z, lam = pts[kind]
    out = [ref.defect_mixed_ref(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b], z[b], lam[b]) for b in range(B)]
    res = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
           np.array([o[3] for o in out], F64))
    for v in res:
        v.setflags(write=False)
    return res


def device_data(nx, nu, N, B):
    d, _ = problem(nx, nu, N, B)
    G, C, g, c = (dev(d[k].reshape(-1)) for k in "GCgc")
    return G, (None if N == 1 else C), g, c   # N == 1: there is no C


def run_defect(solver, nx, nu, N, B, data, z, lam, fill):
    """One defect launch on outputs pre-filled with `fill`; everything back on the host."""
    nz, nl = (nx + nu) * N - nu, nx * N
    rg = torch.full((B * nz,), fill, dtype=torch.float32, device="cuda")
    rc, dl = (torch.full((B * nl,), fill, dtype=torch.float32, device="cuda") for _ in range(2))
    expo = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
    res = torch.full((B, 2), fill, dtype=torch.float64, device="cuda")
    solver.kkt_defect_mixed(nx, nu, N, B, *data, z, lam, rg=rg, rc=rc, dlam=dl, expo=expo, res=res)
    torch.cuda.synchronize()
    return (rg.cpu().numpy().reshape(B, nz), rc.cpu().numpy().reshape(B, nl), dl.cpu().numpy(), expo.cpu().numpy(),
            res.cpu().numpy())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_defect_bits(solver, monkeypatch, case):
    """rg, rc, expo against the Fraction reference, res against gbdpcg_kkt_residual_f64, the zeros of dlambda; NaN-filled and
    1e30-filled outputs give the same bits."""
    (nx, nu, N, B), general = case
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    data = device_data(nx, nu, N, B)
    _, pts = problem(nx, nu, N, B)
    for kind, name in enumerate(POINTS):
        z, lam = dev(pts[kind][0].reshape(-1)), dev(pts[kind][1].reshape(-1))
        wrg, wrc, wexpo, wres = reference(nx, nu, N, B, kind)
        norms = solver.kkt_residual(nx, nu, N, B, *data, z, lam).cpu().numpy()
        first = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"))
        rg, rc, dl, expo, res = first
        print(f"({nx},{nu},{N},{B}) {name}: expo {expo.tolist()} norms {res.tolist()}")
        assert np.array_equal(bits(res), bits(norms)), name
        assert np.array_equal(bits(res), bits(wres)), name
        assert np.array_equal(expo, wexpo), name
        assert np.array_equal(bits(rg), bits(wrg)) and np.array_equal(bits(rc), bits(wrc)), name
        assert not dl.any() and not np.signbit(dl).any(), name
        top = np.maximum(np.abs(rg).max(axis=1), np.abs(rc).max(axis=1))
        assert ((top >= 1) & (top <= 2)).all(), (name, top)     # (2 itself: where fl32 rounds the maximum up to the power of two)
        again = run_defect(solver, nx, nu, N, B, data, z, lam, 1e30)
        for a, b in zip(first, again):
            assert np.array_equal(bits(a), bits(b)), name


@pytest.mark.parametrize("nx,nu,N,B", QUAD)
def test_quad_and_any_size_kernels_agree(solver, monkeypatch, nx, nu, N, B):
    data = device_data(nx, nu, N, B)
    _, pts = problem(nx, nu, N, B)
    z, lam = dev(pts[2][0].reshape(-1)), dev(pts[2][1].reshape(-1))
    quad = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"))
    monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    gen = run_defect(solver, nx, nu, N, B, data, z, lam, float("nan"))
    for a, b in zip(quad, gen):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("general", [False, True])
def test_nan_stays_inside_its_problem(solver, monkeypatch, general):
    """A NaN in z of problem 1: e = 0 and NaN norms there, problems 0 and 2 keep every bit of the clean run."""
    nx, nu, N, B = 14, 7, 17, 3
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    data = device_data(nx, nu, N, B)
    _, pts = problem(nx, nu, N, B)
    z, lam = dev(pts[1][0].reshape(-1)), dev(pts[1][1].reshape(-1))
    clean = run_defect(solver, nx, nu, N, B, data, z, lam, 7.0)
    nz = z.numel() // B
    zn = z.clone()
    zn[nz + 8 * (nx + nu) + 4] = float("nan")
    rg, rc, dl, expo, res = run_defect(solver, nx, nu, N, B, data, zn, lam, 7.0)
    assert expo[1] == 0 and np.isnan(res[1]).all(), (expo, res)
    assert np.isnan(rg[1]).any() and not dl.any()
    for b in (0, 2):
        for a, w in zip((rg, rc, expo, res), (clean[0], clean[1], clean[3], clean[4])):
            assert np.array_equal(bits(a[b]), bits(w[b])), b


@pytest.mark.parametrize("general", [False, True])
def test_a_tiny_defect_is_scaled_up(solver, monkeypatch, general):
    """Problem 1 with g, c and the point multiplied by 2^-70 (exact): its defect is that of the unscaled problem times 2^-70, so
    m < 2^-60, and the right-hand side still has max-norm in [1, 2) -- the mantissas of the unscaled run, e larger by 70."""
    nx, nu, N, B = 5, 2, 9, 2
    if general:
        monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
    G, C, g, c = device_data(nx, nu, N, B)
    _, pts = problem(nx, nu, N, B)
    z, lam = dev(pts[2][0].reshape(-1)), dev(pts[2][1].reshape(-1))
    plain = run_defect(solver, nx, nu, N, B, (G, C, g, c), z, lam, float("nan"))
    s = 2.0 ** -70
    for t in (g, c, z, lam):
        t.view(B, -1)[1] *= s
    rg, rc, dl, expo, res = run_defect(solver, nx, nu, N, B, (G, C, g, c), z, lam, float("nan"))
    assert res[1].max() < 2.0 ** -60 and np.array_equal(res[1], plain[4][1] * s)
    assert expo[1] == plain[3][1] + 70 and expo[0] == plain[3][0]
    assert np.array_equal(bits(rg), bits(plain[0])) and np.array_equal(bits(rc), bits(plain[1]))
    top = max(np.abs(rg[1]).max(), np.abs(rc[1]).max())
    assert 1 <= top < 2, top
    d, _ = problem(nx, nu, N, B)
    wrg, wrc, we, _ = ref.defect_mixed_ref(nx, nu, N, d["G"][1], d["C"][1], d["g"][1] * s, d["c"][1] * s, pts[2][0][1] * s, pts[2][1][1] * s)
    assert we == expo[1] and np.array_equal(bits(wrg), bits(rg[1])) and np.array_equal(bits(wrc), bits(rc[1]))


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("nx,nu,N,B", [(5, 2, 9, 3), (14, 7, 33, 2), (1, 1, 1, 4)])
def test_apply_bits(solver, nx, nu, N, B, offset):
    """z + ldexp((double)dz, -e) exactly, with every array starting `offset` elements behind a 16-byte boundary (fp64: 0 or 8 bytes
    off, fp32: 0, 4 or 12); nothing outside the arrays is touched."""
    nz, nl = (nx + nu) * N - nu, nx * N
    rng = np.random.default_rng(nx + N + offset)
    z, lam = rng.standard_normal((B, nz)), rng.standard_normal((B, nl)) * 1e-3
    dz, dl = (rng.standard_normal((B, n)).astype(F32) * F32(1.5) for n in (nz, nl))
    expo = np.array([23, -3, 0, 61][:B], np.int32)

    def place(a):
        buf = torch.full((a.size + 8,), 777.0, dtype=torch.from_numpy(a).dtype, device="cuda")
        view = buf[offset:offset + a.size]
        view.copy_(dev(a.reshape(-1)))
        return buf, view

    (zb, zv), (lb, lv), (_, dzv), (_, dlv) = (place(a) for a in (z, lam, dz, dl))
    solver.kkt_refine_apply(nx, nu, N, B, dzv, dlv, dev(expo), zv, lv)
    torch.cuda.synchronize()
    wz = np.stack([ref.apply_ref(z[b], dz[b], expo[b]) for b in range(B)])
    wl = np.stack([ref.apply_ref(lam[b], dl[b], expo[b]) for b in range(B)])
    assert np.array_equal(bits(zv.cpu().numpy().reshape(B, nz)), bits(wz))
    assert np.array_equal(bits(lv.cpu().numpy().reshape(B, nl)), bits(wl))
    for buf, n in ((zb, z.size), (lb, lam.size)):
        assert bool((buf[:offset] == 777.0).all()) and bool((buf[offset + n:] == 777.0).all())


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("count", [1, 3, 4, 1027, 70001])
def test_demote_rounds_to_nearest(solver, count, offset):
    rng = np.random.default_rng(count)
    a = rng.standard_normal(count) * np.exp(rng.uniform(-40, 40, count))
    a[0] = 1.0 + 2.0 ** -24            # a tie: to even
    if count > 3:
        a[1], a[2], a[3] = 1e300, -1e-300, 1.0 + 2.0 ** -24 + 2.0 ** -50
    src = torch.zeros(count + 4, dtype=torch.float64, device="cuda")
    dst = torch.full((count + 4,), 777.0, dtype=torch.float32, device="cuda")
    src[offset:offset + count] = dev(a)
    solver.demote(src[offset:offset + count], dst[offset:offset + count])
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        want = a.astype(F32)
    assert np.array_equal(bits(dst[offset:offset + count].cpu().numpy()), bits(want))
    assert bool((dst[:offset] == 777.0).all()) and bool((dst[offset + count:] == 777.0).all())


def kept(solver, nx, nu, N, B, data):
    """The kept fp32 factorisation of the demoted problem: Ginv32, C32, S32, Pinv32."""
    G, C, g, c = data
    G32, g32, c32 = solver.demote(G), solver.demote(g), solver.demote(c)
    C32 = None if C is None else solver.demote(C)
    S32, _, Ginv32 = solver.form_schur(nx, nu, N, B, G32, C32, g32, c32)
    Pinv32 = solver.form_pinv(nx, N, B, S32, binding.PINV_STAIR)
    return Ginv32, C32, S32, Pinv32


@pytest.mark.parametrize("nx,nu,N,B", [(14, 7, 17, 3), (4, 6, 3, 2)])
def test_step_is_the_three_calls(solver, nx, nu, N, B):
    """gbdpcg_kkt_refine_step against defect + kkt_resolve_f32 + apply, two steps from zero: eager, and as one graph replayed
    twice -- every output bit for bit."""
    data = device_data(nx, nu, N, B)
    fac = kept(solver, nx, nu, N, B, data)
    nz, nl = B * ((nx + nu) * N - nu), B * nx * N

    def state():
        w = solver.refine_work(nx, nu, N, B)
        for k in ("rg", "rc", "gamma", "dlam", "r", "p", "dz", "res"):
            w[k].fill_(float("nan"))
        return torch.zeros(nz, dtype=torch.float64, device="cuda"), torch.zeros(nl, dtype=torch.float64, device="cuda"), w

    def snapshot(z, lam, w):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (z, lam, w["rg"], w["rc"], w["dz"], w["dlam"], w["expo"], w["res"], w["iters"])]

    z, lam, w = state()
    want = []
    for _ in range(2):
        solver.kkt_defect_mixed(nx, nu, N, B, *data, z, lam, rg=w["rg"], rc=w["rc"], dlam=w["dlam"], expo=w["expo"], res=w["res"])
        solver.kkt_resolve(nx, nu, N, B, fac[0], fac[1], w["rg"], w["rc"], fac[2], fac[3], w["gamma"], w["dlam"], w["dz"], r=w["r"],
                           p=w["p"], tol=TOL, max_iter=MAX_ITER, iters=w["iters"], max_iter_exit=w["max_iter_exit"])
        solver.kkt_refine_apply(nx, nu, N, B, w["dz"], w["dlam"], w["expo"], z, lam)
        want.append(snapshot(z, lam, w))
    assert np.abs(want[1][7]).max() < 1e-3 * np.abs(want[0][7]).max()       # the second step started from a refined point

    z, lam, w = state()
    for i in range(2):
        solver.kkt_refine_step(nx, nu, N, B, *data, *fac, z, lam, tol=TOL, max_iter=MAX_ITER, **w)
        for a, b in zip(snapshot(z, lam, w), want[i]):
            assert np.array_equal(bits(a), bits(b)), ("eager", i)

    z, lam, w = state()
    graph = solver.graph_kkt_refine_step(nx, nu, N, B, *data, *fac, z, lam, tol=TOL, max_iter=MAX_ITER, **w)
    for i in range(2):
        graph.launch()
        for a, b in zip(snapshot(z, lam, w), want[i]):
            assert np.array_equal(bits(a), bits(b)), ("graph", i)
    graph.close()


def ratios(nx, nu, N, B, d, z, lam, norms):
    """Per problem: (norm / mag [2], norm / bound [2]) at the point (z, lam) with the device's norms."""
    rel, out = np.zeros((B, 2)), np.zeros((B, 2))
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        mag = ref.magnitudes(Gd, Cd, g, c, z[b], lam[b])
        rel[b] = norms[b] / np.array(mag)
        out[b] = norms[b] / np.array(ref.floor(nx, nu, mag))
    return rel, out


@pytest.mark.parametrize("nx,nu,N,B", QUAD + ANY)
def test_refinement_reaches_the_fp64_floor(solver, nx, nu, N, B):
    d, _ = problem(nx, nu, N, B)
    data = device_data(nx, nu, N, B)
    fac = kept(solver, nx, nu, N, B, data)
    w = solver.refine_work(nx, nu, N, B)
    z = torch.zeros(B * ((nx + nu) * N - nu), dtype=torch.float64, device="cuda")
    lam = torch.zeros(B * nx * N, dtype=torch.float64, device="cuda")
    graph = solver.graph_kkt_refine_step(nx, nu, N, B, *data, *fac, z, lam, tol=TOL, max_iter=MAX_ITER, **w)
    history, reached = [], None
    for step in range(1, 13):
        graph.launch()
        norms = solver.kkt_residual(nx, nu, N, B, *data, z, lam)     # the point this step wrote
        torch.cuda.synchronize()
        rel, over = ratios(nx, nu, N, B, d, z.cpu().numpy().reshape(B, -1), lam.cpu().numpy().reshape(B, -1), norms.cpu().numpy())
        history.append((rel.max(axis=1), over.max(axis=1)))
        print(f"({nx},{nu},{N},{B}) after step {step}: norm / bound per problem {over.max(axis=1)}  PCG iterations {w['iters'].cpu().tolist()}")
        assert np.isfinite(over).all()
        if reached is None and (over <= 1.0).all():
            reached = step
        if reached is not None and step >= reached + 2:      # two more steps: the point has to stay where it is
            break
    graph.close()
    print(f"({nx},{nu},{N},{B}): the floor is reached after {reached} steps")
    assert reached is not None, "not inside the bounds within 12 steps"
    assert (history[0][1] >= 2.0 ** 20).all(), history[0][1]            # fp32 alone does not pass
    for (r0, _), (r1, _) in zip(history, history[1:]):
        settled = r0 < 1e-12
        assert (r1[settled] <= 2.0 * r0[settled]).all(), (r0, r1)


def test_kkt_solve_refined_stops_on_the_norms(solver):
    nx, nu, N, B = 5, 2, 9, 2
    data = device_data(nx, nu, N, B)
    fac = kept(solver, nx, nu, N, B, data)
    z, lam, history = solver.kkt_solve_refined(nx, nu, N, B, *data, *fac, max_steps=12, stop_s=1e-12, stop_f=1e-12, tol=TOL,
                                               max_iter=MAX_ITER)
    assert 2 <= len(history) < 12 and (history[-1] <= 1e-12).all() and (history[0] > 1e-3).any()
    final = solver.kkt_residual(nx, nu, N, B, *data, z, lam).cpu().numpy()
    assert (final <= 1e-12).all()


def test_bad_arguments(solver):
    """Null required pointers and zero sizes: INVALID (1); a block size form_schur refuses: UNSUPPORTED (4); nothing written."""
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
            if k in ("nx", "nu", "N", "batch", "count"):
                assert fn(*dict(base, **{k: 0}).values(), *tail) == 1, k
            elif k not in ("tol", "max_iter"):
                assert fn(*dict(base, **{k: None}).values(), *tail) == 1, k
        if "nx" in base:
            assert fn(*dict(base, nx=80, nu=40).values(), *tail) == 4
        assert untouched()

    sizes = dict(h=solver.h, nx=nx, nu=nu, N=N, batch=B)
    defect = dict(sizes, G=P64, C=P64, g=P64, c=P64, z=P64, lam=P64, rg=O["rg"], rc=O["rc"], dlam=O["dlam"], expo=O["expo"], res=O["res"])
    check(lib.gbdpcg_kkt_defect_mixed, defect, {"dlam"}, (s,))
    apply_ = dict(sizes, dz=P32, dlam=P32, expo=ctypes.c_void_p(out["iters"].data_ptr()), z=O["z"], lam=O["lam"])
    check(lib.gbdpcg_kkt_refine_apply, apply_, set(), (s,))
    step = dict(sizes, G=P64, C=P64, g=P64, c=P64, Ginv=P32, C32=P32, S=P32, Pinv=P32, rg=O["rg"], rc=O["rc"], gamma=O["gamma"],
                dlam=O["dlam"], r=None, p=None, dz=O["dz"], tol=1e-6, max_iter=10, iters=O["iters"], flags=None, expo=O["expo"],
                z=O["z"], lam=O["lam"], res=O["res"])
    check(lib.gbdpcg_kkt_refine_step, step, {"Pinv", "r", "p", "flags"}, (s,))
    graph = ctypes.c_void_p()
    check(lib.gbdpcg_graph_create_kkt_refine_step, step, {"Pinv", "r", "p", "flags"}, (ctypes.byref(graph),))
    assert not graph.value
    assert lib.gbdpcg_graph_create_kkt_refine_step(*step.values(), None) == 1
    demote = dict(h=solver.h, count=100, src=P64, dst=O["rg"])
    check(lib.gbdpcg_demote_f32, demote, set(), (s,))
    # N == 1: there is no C, in either precision; dlambda may be NULL
    assert lib.gbdpcg_kkt_defect_mixed(*dict(defect, N=1, C=None, dlam=None).values(), s) == 0
    torch.cuda.synchronize()
    assert bool((out["dlam"] == 777.0).all()) and bool((out["rg"][:B * nx] == 0).all()) and bool((out["expo"][:B] == 0).all())
    assert lib.gbdpcg_kkt_defect_mixed(*defect.values(), s) == 0
    torch.cuda.synchronize()
    assert bool((out["dlam"][:B * nx * N] == 0).all()) and bool((out["res"][:2 * B] == 0).all())
