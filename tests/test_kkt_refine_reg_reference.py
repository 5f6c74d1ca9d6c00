"""CPU checks of the references of the regularised mixed-precision refinement (tests/kkt_refine_reg_ref.py), which the GPU tests of
gbdpcg_kkt_defect_mixed_reg and gbdpcg_kkt_refine_step_reg compare bits and step counts with: rho = 0 is the plain reference, the
Fraction defect agrees with dense numpy (G + rho I) z + g + C' lambda within the dot-product bound, and the refinement emulated in
numpy on SEMI-DEFINITE data (every R_k = 0, where the unregularised cost has no factorisation) reaches the fp64 floor of the
regularised system in N0 steps with an inner solve that is only 1e-3 accurate -- while the same loop driven by the plain defect
(rho only in the factorisation) stays orders of magnitude outside it."""
from fractions import Fraction

import numpy as np
import pytest

import kkt_refine_ref as ref
import kkt_refine_reg_ref as reg
from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
RHOS, N0 = list(reg.RHOS), reg.N0
EMULATED = [(14, 7, 33), (14, 7, 17), (5, 2, 9), (4, 6, 3), (3, 3, 2), (1, 1, 4), (14, 7, 1)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def data(nx, nu, N):
    d = so.gen(nx, nu, N, seed=60 + nx + N, batch=1, dtype=F64)
    rng = np.random.default_rng(11)
    return d, rng.standard_normal(d["g"].shape[1]), rng.standard_normal(d["c"].shape[1])


@pytest.mark.parametrize("nx,nu,N", [(5, 2, 4), (4, 6, 3), (1, 1, 4), (14, 7, 1)])
def test_regularised_touches_the_diagonals_only(nx, nu, N):
    d, _, _ = data(nx, nu, N)
    rho = 0.3
    Gd = so.dense_kkt(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0])[0]
    Gr = so.dense_kkt(nx, nu, N, reg.regularised(nx, nu, N, d["G"][0], rho), d["C"][0], d["g"][0], d["c"][0])[0]
    want = Gd.copy()
    want[np.diag_indices_from(want)] = np.diag(Gd) + F64(rho)
    assert np.array_equal(bits(Gr), bits(want))
    Z = so.dense_kkt(nx, nu, N, reg.zero_inputs(nx, nu, N, d["G"][0]), d["C"][0], d["g"][0], d["c"][0])[0]
    sv = nx + nu
    for k in range(N):
        assert np.array_equal(Z[k * sv:k * sv + nx, k * sv:k * sv + nx], Gd[k * sv:k * sv + nx, k * sv:k * sv + nx])
        if k + 1 < N:
            assert not Z[k * sv + nx:(k + 1) * sv].any()


@pytest.mark.parametrize("nx,nu,N", [(5, 2, 4), (3, 3, 2), (4, 6, 3), (1, 1, 4), (14, 7, 1)])
def test_rho_zero_is_the_plain_reference(nx, nu, N):
    d, z, lam = data(nx, nu, N)
    a = ref.defect_mixed_ref(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0], z, lam)
    b = reg.defect_mixed_reg_ref(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0], 0.0, z, lam)
    assert a[2] == b[2] and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(bits(np.array(a[3])), bits(np.array(b[3])))


@pytest.mark.parametrize("rho", [0.3, 1.7e-3, 41.0 / 3.0])
@pytest.mark.parametrize("nx,nu,N", [(5, 2, 4), (3, 3, 2), (4, 6, 3), (1, 1, 4), (14, 7, 1), (6, 3, 2)])
def test_fraction_defect_against_numpy(nx, nu, N, rho):
    """The reference against (G + rho I) z + g + C' lambda in plain numpy, within the dot-product bound of kkt_refine_ref.floor on
    the magnitudes of the regularised system; and rho is in it: the plain defect differs by about rho |z|."""
    d, z, lam = data(nx, nu, N)
    rg, rc, e, (ms, mf) = reg.defect_mixed_reg_ref(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0], rho, z, lam)
    rs, rf = ref.defect_ref(nx, nu, N, reg.regularised(nx, nu, N, d["G"][0], rho), d["C"][0], d["g"][0], d["c"][0], z, lam)
    Gd, Cd, g, c = so.dense_kkt(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0])
    Gr = Gd + rho * np.eye(Gd.shape[0])
    ws, wf = Gr @ z + g + Cd.T @ lam, Cd @ z - c
    bs, bf = ref.floor(nx, nu, ref.magnitudes(Gr, Cd, g, c, z, lam))
    assert np.abs(rs - ws).max() <= bs and np.abs(rf - wf).max() <= bf
    assert ms == np.abs(rs).max() and mf == np.abs(rf).max()
    assert np.array_equal(bits(rg), bits(ref.scaled_f32(rs, e))) and np.array_equal(bits(rc), bits(ref.scaled_f32(-rf, e)))
    plain, _ = ref.defect_ref(nx, nu, N, d["G"][0], d["C"][0], d["g"][0], d["c"][0], z, lam)
    assert np.abs((rs - plain) - rho * z).max() <= 2 * bs
    # d + rho rounds for this data: the one fp64 addition is part of what the device is held to
    assert any(Fraction(float(x)) + Fraction(float(rho)) != Fraction(float(F64(x) + F64(rho))) for x in np.diag(Gd))


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("nx,nu,N", EMULATED)
def test_emulated_refinement_reaches_the_regularised_floor(nx, nu, N, rho):
    """Semi-definite data: inside the floor of the regularised system after N0 steps and from there on; fp32 alone (one step)
    does not pass."""
    out = reg.emulate_reg(nx, nu, N, seed=900 + nx + N, steps=N0 + 2, rho=rho, inner_error=1e-3, zero_R=True)
    n0 = next(i for i in range(len(out)) if all(max(p) <= 1.0 for p in out[i:]))
    for i, (s, f) in enumerate(out):
        print(f"({nx},{nu},{N}) rho {rho} after {i} steps: stationarity / bound {s:.3e}  feasibility / bound {f:.3e}")
    print(f"({nx},{nu},{N}) rho {rho}: n0 = {n0} (N0 = {N0})")
    assert n0 <= N0
    assert max(out[1]) > 2.0 ** 20
    assert all(max(p) <= 1.0 for p in out[N0:])


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("nx,nu,N", EMULATED)
def test_the_plain_defect_does_not_reach_the_regularised_floor(nx, nu, N, rho):
    """The same loop with rho in the factorisation only: what gbdpcg_kkt_refine_step does with a kept factorisation of G + rho I.
    It heads for the unregularised system (singular in the inputs where N > 1) and is not inside the floor of the regularised one
    after N0 steps, nor after 2 N0."""
    with np.errstate(all="ignore"):
        out = reg.emulate_reg(nx, nu, N, seed=900 + nx + N, steps=2 * N0, rho=rho, inner_error=1e-3, zero_R=True, plain_defect=True)
    print(f"({nx},{nu},{N}) rho {rho}: plain defect, norm / bound after {N0} steps {max(out[N0]):.3e}, after {2 * N0} {max(out[-1]):.3e}")
    for i in (N0, 2 * N0):
        assert not max(out[i]) <= 1.0
        assert not max(out[i]) <= 2.0 ** 20     # not near it either
