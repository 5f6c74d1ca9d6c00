"""CPU checks of the references of the optimality test (tests/admm_optimality_ref.py): the exact definition against a dense fp64
evaluation within the derived fma-chain bound, the four identities the header states (against kkt_refine_ref.defect_ref and the row
residual of the four update references), NaN isolation, the flag against its three comparisons, and the pinned windows and EPS."""
import numpy as np
import pytest

import admm_infeas_ref as ir
import admm_lin_ref as lr
import admm_optimality_ref as orf
import admm_ref
import admm_soc_ref as soc
import admm_soft_ref as sr
import kkt_refine_ref as kr
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
ARGS = ("G", "C", "g", "c", "E", "rho", "z", "lam", "w", "y")
EPS_BITS = 1.0            # with random data of order 1: flags of both values
SHAPES = [(2, 1, 1, 2, 1, 0, False), (3, 2, 4, 3, 2, 1, False), (3, 2, 3, 2, 0, 2, False), (5, 3, 3, 2, 4, 2, False),
          (3, 2, 4, 3, 0, 0, True), (2, 1, 1, 2, 0, 0, True)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def inputs(nx, nu, N, B, mx, mu, box, dtype, seed=0):
    return orf.random_inputs(nx, nu, mx, mu, N, B, 900 + seed + 13 * nx + N + mx, dtype, box=box)


def ref(dtype, nx, nu, mx, mu, N, d, eps=EPS_BITS):
    return orf.opt_ref(dtype, nx, nu, mx, mu, N, *[d[k] for k in ARGS], eps, eps)


# ---- 1. the exact definition against the dense evaluation, within the derived bound
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", SHAPES)
def test_exact_reference_agrees_with_the_dense_evaluation_within_the_chain_bound(nx, nu, N, B, mx, mu, box, dtype):
    """Per residual the bound is (len + 2) u sum |terms| of the longest chain behind it, once for the reference's precision and once
    for the fp64 of the dense evaluation.  The scales are maxima of PARTS of those sums: the same bound holds for them."""
    d = inputs(nx, nu, N, B, mx, mu, box, dtype)
    opt, _ = ref(dtype, nx, nu, mx, mu, N, d)
    rows = (nx, nu) if box else (mx, mu)
    lens = orf.chain_lengths(nx, nu, *rows)
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = None if box else lr.dense_E(nx, nu, mx, mu, N, d["E"][b].astype(F64))
        six, mag = orf.opt_dense(Gd, Cd, Ed, g, c, float(d["rho"][b]), d["z"][b], d["lam"][b], d["w"][b], d["y"][b])
        for i in range(6):
            bound = orf.chain_bound(lens[i % 3], dtype, mag[i % 3]) + orf.chain_bound(lens[i % 3], F64, mag[i % 3])
            assert abs(float(opt[b, i]) - six[i]) <= bound, (b, i, opt[b, i], six[i], bound)


# ---- 2. the identities
@pytest.mark.parametrize("nx,nu,N,B,mx,mu,box", SHAPES)
def test_with_y_zero_rs_and_re_are_the_kkt_residual(nx, nu, N, B, mx, mu, box):
    d = dict(inputs(nx, nu, N, B, mx, mu, box, F64))
    d["y"] = np.where(np.arange(d["y"].shape[1]) % 2 == 0, 0.0, -0.0) * np.ones_like(d["y"])
    opt, _ = ref(F64, nx, nu, mx, mu, N, d)
    for b in range(B):
        rs, rf = kr.defect_ref(nx, nu, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b], d["z"][b], d["lam"][b])
        assert same(opt[b, 0], kr.max_bits(rs)) and same(opt[b, 1], kr.max_bits(rf))


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("family", ["box", "soft_box", "lin", "lin_soft", "soc"])
def test_behind_an_update_rr_is_its_primal_residual(family, dtype):
    nx, nu, N, B = 3, 2, 4, 3
    mx, mu = (nx, nu) if "box" in family else ((4, 3) if family == "soc" else (2, 1))
    d = inputs(nx, nu, N, B, mx, mu, "box" in family, dtype, seed=5)
    rng = np.random.default_rng(77)
    nw = d["w"].shape[1]
    lo = (-np.abs(rng.standard_normal((B, nw))) * 0.3).astype(np.float32).astype(dtype)
    hi = (np.abs(rng.standard_normal((B, nw))) * 0.3).astype(np.float32).astype(dtype)
    kappa = np.abs(rng.standard_normal((B, nw))).astype(np.float32).astype(dtype)
    kappa[:, ::3] = np.inf
    g, E, rho, z, w, y = d["g"], d["E"], d["rho"], d["z"], d["w"], d["y"]
    if family == "box":
        wn, yn, _, _, res = admm_ref.update_ref(dtype, g, lo, hi, rho, z, w, y)
    elif family == "soft_box":
        wn, yn, _, _, res = sr.update_ref(dtype, g, lo, hi, kappa, rho, z, w, y)
    elif family == "lin":
        wn, yn, _, res = lr.update_ref(dtype, nx, nu, mx, mu, N, g, E, lo, hi, rho, z, w, y)
    elif family == "lin_soft":
        wn, yn, _, res = sr.lin_update_ref(dtype, nx, nu, mx, mu, N, g, E, lo, hi, kappa, rho, z, w, y)
    else:
        cones = (1, 3, 1, 2)                                   # x block: 1 linear row + one cone of 3; u block: 1 linear + one of 2
        head, _ = soc.layout(nx, nu, mx, mu, cones, N)
        lo = np.where(head >= 0, 0.0, lo).astype(dtype)        # zero offsets f on the cone rows
        wn, yn, _, res, _ = soc.update_ref(dtype, nx, nu, mx, mu, cones, N, g, E, lo, hi, rho, z, w, y)
    after = dict(d, w=wn, y=yn)
    opt, _ = ref(dtype, nx, nu, mx, mu, N, after)
    assert same(opt[:, 2], np.asarray(res[:, 0], dtype)), (opt[:, 2], res[:, 0])
    assert (opt[:, 2] > 0).all()


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nx,nu,N,B", [(3, 2, 4, 3), (2, 1, 1, 2)])
def test_box_is_rows_at_identity(nx, nu, N, B, dtype):
    d = dict(inputs(nx, nu, N, B, 0, 0, True, dtype))
    box = ref(dtype, nx, nu, 0, 0, N, d)
    d["E"] = orf.box_as_rows(nx, nu, N, B, dtype)
    rows = ref(dtype, nx, nu, nx, nu, N, d)
    assert same(box[0], rows[0]) and same(box[1], rows[1])


@pytest.mark.parametrize("box", [False, True])
def test_shared_is_the_per_problem_call_on_copies(box):
    nx, nu, N, B, mx, mu = 3, 2, 3, 3, 2, 1
    d = dict(inputs(nx, nu, N, B, mx, mu, box, F32))
    one = dict(d)
    for k in ("G", "C", "E"):
        if d[k] is not None:
            one[k] = d[k][1:2]
            d[k] = np.tile(d[k][1:2], (B, 1))
    a, b = ref(F32, nx, nu, mx, mu, N, d), ref(F32, nx, nu, mx, mu, N, one)
    assert same(a[0], b[0]) and same(a[1], b[1])


# ---- 3. NaN isolation, the flag
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("box", [False, True])
def test_a_nan_stays_in_its_problem_and_clears_its_flag(box, dtype):
    nx, nu, N, B, mx, mu = 3, 2, 4, 3, 2, 1
    d = inputs(nx, nu, N, B, mx, mu, box, dtype)
    good = ref(dtype, nx, nu, mx, mu, N, d, eps=1e6)
    assert good[1].all()                                       # everything passes at a huge eps ...
    for key in ("z", "lam", "w", "y", "g", "c", "rho", "G"):
        bad = {k: (None if v is None else v.copy()) for k, v in d.items()}
        if key == "rho":
            bad[key][1] = np.nan
        else:
            bad[key][1, 0] = np.nan
        opt, done = ref(dtype, nx, nu, mx, mu, N, bad, eps=1e6)
        assert done[1] == 0 and np.isnan(opt[1]).any(), key    # ... except the problem with the NaN
        keep = [0, 2]
        assert same(opt[keep], good[0][keep]) and same(done[keep], good[1][keep]), key


@pytest.mark.parametrize("dtype", [F32, F64])
def test_done_is_the_three_comparisons_and_takes_both_values(dtype):
    flags = []
    for nx, nu, N, B, mx, mu, box in SHAPES:
        d = inputs(nx, nu, N, B, mx, mu, box, dtype)
        opt, done = ref(dtype, nx, nu, mx, mu, N, d)
        assert same(done, orf.done_from_opt(opt, EPS_BITS, EPS_BITS))
        flags.append(done)
        for i in range(3):                                      # each comparison alone can clear the flag
            o = opt.copy()
            o[:, :3] = 0
            o[:, i] = np.inf
            assert not orf.done_from_opt(o, EPS_BITS, EPS_BITS).any()
    flags = np.concatenate(flags)
    assert flags.min() == 0 and flags.max() == 1


def test_knot_chunk_is_the_kernels():
    assert orf.knot_chunk(14, 7, 4, 2) == 4096 // 650 and orf.knot_chunk(14, 7, 0, 0, box=True) == 4096 // (245 + 294 + 35 + 21)
    assert orf.knot_chunk(2, 1, 1, 0) == 64 and orf.knot_chunk(60, 30, 4, 2) == 1


# ---- 4. the pinned fixture: windows of the fp64 loop, EPS by the stated rule
def test_windows_are_pinned_and_eps_is_the_smallest_power_of_ten_the_fp32_loop_reaches():
    P = ir.feasible_problems()
    assert len(P) == len(orf.K_LO) == len(orf.K_HI)
    # problems 6 .. 8 (admm_soft_ref's box) are the hard loop on the box of admm_ref: the histories of 0 .. 2, not run again
    for i in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(P[i][1:3] + P[i][4:], P[i + 6][1:3] + P[i + 6][4:])) and P[i + 6][3] is None
    idx = range(6)
    w64 = [orf.windows(orf.history(i, "float64"), orf.EPS) for i in idx]
    assert tuple(w[0] for w in w64) == orf.K_LO[:6] and tuple(w[1] for w in w64) == orf.K_HI[:6], w64
    assert orf.K_LO[6:] == orf.K_LO[:3] and orf.K_HI[6:] == orf.K_HI[:3]
    assert all(lo < hi <= orf.K_MAX for lo, hi in w64)
    w32 = [orf.windows(orf.history(i, "float32"), orf.EPS) for i in idx]
    assert all(hi is not None for _, hi in w32), w32                               # EPS: every problem reaches 0.5 x in fp32
    w32s = [orf.windows(orf.history(i, "float32"), orf.EPS / 10) for i in idx]
    assert any(hi is None for _, hi in w32s), w32s                                 # EPS / 10: not every one does
    # in fp64 the residuals fall well below: the loop, not the arithmetic, sets the windows
    assert all(orf.history(i, "float64")[-1, :3].max() < 0.05 * orf.EPS for i in idx if i != 5)
