"""CPU checks of the references of the mixed-precision refinement (tests/kkt_refine_ref.py), which the GPU tests compare bits with:
the Fraction defect against plain fp64 numpy within the dot-product bound of tests/test_gpu_kkt_residual.py, the exponent rule at
its corners, the scaling and the apply line, and the refinement emulated in numpy -- fp32 G^-1 and S, an exact (dense) fp32
solve of S, fp64 defect, fp64 accumulation from zero -- reaching the fp64 rounding floor in 3 steps and not before step 2."""
import numpy as np
import pytest

import kkt_refine_ref as ref
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
EMULATED = [(14, 7, 33), (12, 4, 16), (5, 2, 17), (3, 3, 2)]   # the shapes of the emulation the feature was specified with


@pytest.mark.parametrize("nx,nu,N", [(5, 2, 4), (3, 3, 2), (4, 6, 3), (1, 1, 4), (14, 7, 1), (6, 3, 2)])
def test_fraction_defect_against_numpy(nx, nu, N):
    d = so.gen(nx, nu, N, seed=40 + nx + N, batch=1, dtype=F64)
    rng = np.random.default_rng(5)
    z, lam = rng.standard_normal(d["g"].shape[1]), rng.standard_normal(d["c"].shape[1])
    rs, rf = ref.defect_ref(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0], z, lam)
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0])
    ws, wf = Gd @ z + g + Cd.T @ lam, Cd @ z - c
    bs, bf = ref.floor(nx, nu, ref.magnitudes(Gd, Cd, g, c, z, lam))
    assert np.abs(rs - ws).max() <= bs and np.abs(rf - wf).max() <= bf
    assert np.abs(rs).max() > 0.5 * np.abs(ws).max() and np.abs(rf).max() > 0.5 * np.abs(wf).max()


def test_exponent_rule():
    below = np.nextafter(4.0, 0.0)
    assert ref.exponent(0.0, 0.0) == 0
    assert ref.exponent(4.0, 1.0) == -2 and ref.exponent(1.0, 4.0) == -2          # a power of two: m 2^e = 1
    assert ref.exponent(below, 0.0) == -1 and 1.0 <= below * 2.0 ** -1 < 2.0      # just below it
    assert ref.exponent(1.0, 0.5) == 0 and ref.exponent(0.75, 0.0) == 1
    assert ref.exponent(np.inf, 1.0) == 0 and ref.exponent(1.0, np.nan) == 0 and ref.exponent(np.nan, np.inf) == 0
    assert ref.exponent(2.0 ** -60, 2.0 ** -70) == 60
    assert ref.exponent(2.0 ** -300, 0.0) == 127 and ref.exponent(5e-324, 0.0) == 127 and ref.exponent(2.0 ** 200, 0.0) == -126
    for m in (3.7e-9, 0.11, 1.0, 1.999, 6.02e23):
        assert 1.0 <= m * 2.0 ** ref.exponent(m, m / 3) < 2.0


def test_max_bits_propagates_nan_and_orders_inf():
    assert ref.max_bits(np.array([1.0, -3.0, 2.0])) == 3.0
    assert np.isposinf(ref.max_bits(np.array([1.0, -np.inf])))
    assert np.isnan(ref.max_bits(np.array([np.inf, np.nan, 1.0])))


def test_scaling_and_apply_lines():
    v = np.array([1.0 + 2.0 ** -30, -2.0 ** -61 * (1 + 2.0 ** -24 + 2.0 ** -40), 0.0, 3.0e-50, np.inf])
    s = ref.scaled_f32(v, 3)
    assert s.dtype == F32
    assert s[0] == F32(8.0) and s[2] == 0 and np.isposinf(s[4])
    assert s[1] == -F32(2.0 ** -58) * (F32(1) + F32(2.0 ** -23))      # a tie broken upwards by the sticky bit, then an exact product
    assert s[3] == F32(0)                                            # below half the smallest fp32 subnormal
    assert np.array_equal(ref.scaled_f32(v[:3], 61), v[:3].astype(F32) * F32(2.0 ** 61))
    z, dz = np.array([1.0, -2.0 ** -3]), np.array([1.5, 2.0 ** -20], F32)
    assert np.array_equal(ref.apply_ref(z, dz, 30), z + dz.astype(F64) * 2.0 ** -30)
    assert np.array_equal(ref.apply_ref(z, dz, -4), z + dz.astype(F64) * 16.0)


@pytest.mark.parametrize("nx,nu,N", EMULATED)
def test_emulated_refinement_reaches_the_floor_in_three_steps(nx, nu, N):
    """Ratios norm / bound per step (1 = the floor): above it by orders of magnitude after one step -- fp32 alone does not pass --
    and inside it after three."""
    out = ref.emulate(nx, nu, N, seed=900 + nx + N, steps=4)
    for i, (s, f) in enumerate(out):
        print(f"({nx},{nu},{N}) after {i} steps: stationarity / bound {s:.3e}  feasibility / bound {f:.3e}")
    assert max(out[1]) > 2.0 ** 20
    assert max(out[3]) <= 1.0 and max(out[4]) <= 1.0


def test_a_loose_inner_solve_contracts_by_its_accuracy():
    """With a correction that is only 1e-3 accurate the floor is reached at step 6: the bound of 12 steps the GPU test allows is
    twice that."""
    out = ref.emulate(14, 7, 33, seed=947, steps=8, inner_error=1e-3)
    for i, (s, f) in enumerate(out):
        print(f"after {i} steps: {s:.3e} {f:.3e}")
    assert max(out[2]) > 1.0 and max(out[6]) <= 1.0 and max(out[8]) <= 1.0
