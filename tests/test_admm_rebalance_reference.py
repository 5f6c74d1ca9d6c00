"""CPU checks of tests/admm_rebalance_ref.py, the reference tests/test_gpu_admm_rebalance.py holds the device to: the rule's corner
cases, the scaling of y, the rounding of the reference fma, and the convergence fixture -- the reference ALONE must show that
adapting rho pays on it, or the device test would prove nothing."""
import math

import numpy as np
import pytest

import admm_rebalance_ref as ar

F32, F64 = np.float32, np.float64
RULE = dict(ratio=10.0, shift=1, rho_min=0.5, rho_max=8.0)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shift", [1, 3])
def test_rule_branches(dtype, shift):
    tau = 2.0 ** shift
    nan = float("nan")
    #            r     s     rho
    rows = [(100.0, 1.0, 1.0),          # raise
            (1.0, 100.0, 8.0),          # lower
            (5.0, 1.0, 1.0),            # inside the band
            (100.0, 1.0, 8.0),          # raise blocked by rho_max (8 tau > 8)
            (1.0, 100.0, 0.5),          # lower blocked by rho_min
            (nan, 1.0, 1.0),            # NaN residual
            (1.0, nan, 1.0),
            (100.0, 1.0, nan),          # NaN rho
            (10.0, 1.0, 1.0),           # r == ratio s: a strict comparison, unchanged
            (100.0, 1.0, 8.0 / tau),    # up == rho_max: allowed
            (1.0, 100.0, 0.5 * tau)]    # dn == rho_min: allowed
    res = np.array([[r, s] for r, s, _ in rows], dtype)
    rho = np.array([p for _, _, p in rows], dtype)
    new, e = ar.rule(dtype, res, rho, RULE["ratio"], shift, RULE["rho_min"], RULE["rho_max"])
    assert new.dtype == np.dtype(dtype) and e.dtype == np.int32
    assert e.tolist() == [shift, -shift, 0, 0, 0, 0, 0, 0, 0, shift, -shift]
    want = [tau, 8.0 / tau, 1.0, 8.0, 0.5, 1.0, 1.0, nan, 1.0, 8.0, 0.5]
    for got, w in zip(new.tolist(), want):
        assert (math.isnan(got) and math.isnan(w)) or got == w


@pytest.mark.parametrize("dtype", [F32, F64])
def test_scaling_keeps_the_multiplier_and_untouched_rows_keep_their_bits(dtype):
    T = np.dtype(dtype).type
    tiny = np.finfo(dtype).tiny
    y = np.array([[1.5, -0.0, np.inf, -np.inf, np.nan, tiny, 3.0 * np.finfo(dtype).smallest_subnormal]] * 3, dtype)
    res = np.array([[100.0, 1.0], [1.0, 100.0], [1.0, 1.0]], dtype)
    rho = np.array([1.0, 4.0, 2.0], dtype)
    new, yn, e, gt = ar.rebalance_ref(dtype, res, rho, y, 10.0, 1, 0.5, 8.0)
    assert gt is None and e.tolist() == [1, -1, 0] and new.tolist() == [2.0, 2.0, 2.0]
    assert yn[0, 0] == T(0.75) and yn[1, 0] == T(3.0)
    assert np.signbit(yn[0, 1]) and yn[0, 1] == 0 and np.isposinf(yn[0, 2]) and np.isneginf(yn[0, 3]) and np.isnan(yn[0, 4])
    assert 0 < yn[0, 5] < tiny and yn[0, 5] == tiny / 2                      # lands in the subnormals, still exact
    assert yn[0, 6] == T(2.0) * np.finfo(dtype).smallest_subnormal           # 1.5 steps: rounded to even
    assert yn[2].tobytes() == y[2].tobytes()
    finite = np.isfinite(y[0]) & (np.abs(y[0]) >= tiny * 2)
    assert np.array_equal(new[0] * yn[0][finite], rho[0] * y[0][finite])     # rho y is what it was


def test_reference_fma_rounds_once():
    # fp32: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie, c = 2^-40 lifts it just above: one rounding goes up, a product rounded
    # first goes to even and the sum then loses c
    a, b, c = F32(1.0 + 2.0 ** -12), F32(1.0 + 2.0 ** -12), F32(2.0 ** -40)
    got = ar.fma_ref(F32, [a], [b], [c])[0]
    twice = F32(F32(a * b) + c)
    assert got.dtype == np.float32 and float(got) == 1.0 + 2.0 ** -11 + 2.0 ** -23 and float(twice) == 1.0 + 2.0 ** -11
    # fp64 against math.fma where the interpreter has one, else against an exactly representable case
    x, y, z = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -31, -1.0
    got = float(ar.fma_ref(F64, [x], [y], [z])[0])
    assert got == 2.0 ** -30 + 2.0 ** -31 + 2.0 ** -61
    if hasattr(math, "fma"):
        rng = np.random.default_rng(5)
        v = rng.standard_normal((3, 200))
        assert all(float(ar.fma_ref(F64, [p], [q], [r])[0]) == math.fma(p, q, r) for p, q, r in v.T)
    assert np.isnan(ar.fma_ref(F32, [np.inf], [0.0], [1.0])[0]) and np.isneginf(ar.fma_ref(F64, [-2.0], [np.inf], [1.0])[0])
    assert np.signbit(ar.fma_ref(F32, [-0.0], [1.0], [-0.0])[0]) and not np.signbit(ar.fma_ref(F32, [1.0], [1.0], [-1.0])[0])


def test_box_gradient_is_the_init_line():
    rng = np.random.default_rng(9)
    B, n = 3, 11
    g, w, y = (rng.standard_normal((B, n)) for _ in range(3))
    res = np.array([[100.0, 1.0], [1.0, 100.0], [1.0, 1.0]])
    rho = np.array([1.0, 4.0, 2.0])
    new, yn, e, gt = ar.rebalance_ref(F64, res, rho, y, 10.0, 1, 0.5, 8.0, g=g, w=w)
    assert np.allclose(gt, g - new[:, None] * (w - yn), rtol=1e-15, atol=1e-15)
    assert np.array_equal(yn[2], y[2]) and np.array_equal(yn[0], y[0] / 2) and np.array_equal(yn[1], y[1] * 2)


def test_convergence_fixture_shows_that_adapting_pays():
    """The fixture of the device test, in the dense fp64 reference with exact solves: three (14, 7, 24) problems from rho 16 times too
    small, 64 and 32 times too large, eps = 1e-6 on both residuals, 5 plain iterations per restep, ratio 10, shift 1.
    K_fixed = 1270 (per problem 1270, 1195, 408), K_adapt = 104 (per problem 104, 67, 58): K_adapt <= K_fixed / 2, both below the
    cap of 2000."""
    fixed, adapt = ar.convergence_counts()
    assert all(ok for _, ok in fixed) and all(ok for _, ok in adapt)
    k_fixed, k_adapt = max(k for k, _ in fixed), max(k for k, _ in adapt)
    print(f"K_fixed {k_fixed} {[k for k, _ in fixed]}  K_adapt {k_adapt} {[k for k, _ in adapt]}")
    assert k_fixed < ar.CONV_CAP and k_adapt < ar.CONV_CAP
    assert k_adapt <= k_fixed / 2
    assert (k_fixed, k_adapt) == (1270, 104)      # what the docstring and the device test quote
    # the device test's last claim: with the rule disabled the loop is nowhere near eps after K_adapt + P iterations
    assert min(k for k, _ in fixed) > 2 * (k_adapt + ar.CONV_PERIOD)
