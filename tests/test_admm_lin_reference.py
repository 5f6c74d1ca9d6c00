"""CPU: the references of ADMM with stage-wise linear inequality rows (tests/admm_lin_ref.py) on the inputs of the device's convergence
test (tests/test_gpu_admm_lin.py): the three problems of admm_ref.convergence_inputs() with mx = mu = 2 rows per block (admm_lin_ref.rows),
rho = (3, 4, 2.5), w0 = y0 = 0.

 - after 4000 iterations the fp64 reference satisfies the KKT conditions of the inequality QP.  Measured once with this code, per
   problem: stationarity ||G z + g + C'lambda + rho E'y||_inf 7.6e-15 / 9.8e-15 / 1.1e-14, ||C z - c||_inf 1.5e-15 / 3.8e-15 / 1.8e-15,
   row violation 5.6e-17 / 4.2e-17 / 1.1e-16, distance of an active row from its bound 5.6e-17 / 5.6e-17 / 1.1e-16; each is held to
   1e-12, two orders above the worst, as tests/test_admm_reference.py holds the box;
 - rows of each kind bind: 2 / 4 / 7 state rows and 13 / 27 / 18 control rows are active at the solution, and the unconstrained
   solution violates 17 / 33 / 27 rows (pinned: if the generator ever differs this fails here, not on the device);
 - after 80 iterations the reference has come as far as TABLE says (measured r_prim(80) / r_prim(1) 2.3e-5 / 6.2e-5 / 4.0e-3,
   ||w(80) - w*||_inf 2.9e-6 / 8.7e-6 / 1.6e-3, ||w(1) - w*||_inf 0.12 / 0.12 / 0.16), so that "80 replays" asks something;
 - with E = I admm_lin is admm_ref.admm to the last fp64 bit, and form_ref gives G with fl(diag + rho), off-diagonals untouched."""
import numpy as np

import admm_lin_ref
import admm_ref
from oracle import schur_oracle as so

NX, NU, N, B = admm_lin_ref.CONV_SHAPE
MX, MU = admm_lin_ref.CONV_ROWS
RHO = admm_lin_ref.CONV_RHO
assert (NX, NU, N, B, MX, MU) == (14, 7, 24, 3, 2, 2) and RHO == (3.0, 4.0, 2.5)
K = 80
KKT_TOL = 1e-12
# problem: r_prim(80) / r_prim(1) at most, ||w(80) - w*||_inf at most, ||w(1) - w*||_inf at least
TABLE = {0: (5e-5, 6e-6, 0.1), 1: (2e-4, 2e-5, 0.1), 2: (8e-3, 4e-3, 0.1)}
ACTIVE_STATE, ACTIVE_CONTROL, VIOLATED = (2, 4, 7), (13, 27, 18), (17, 33, 27)

inputs, run = admm_lin_ref.convergence_inputs, admm_lin_ref.convergence_reference


def kinds():
    """0 for a state row, 1 for a control row, in the layout of the rows."""
    k = np.zeros(admm_lin_ref.sizes(NX, NU, MX, MU, N)[1], int)
    for i, (m, _, _, ro, _, _) in enumerate(admm_lin_ref.blocks(NX, NU, MX, MU, N)):
        k[ro:ro + m] = i % 2
    return k


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_reference_reaches_the_kkt_point_of_the_inequality_qp():
    d, E, lo, hi, _ = inputs()
    for b, h in enumerate(run(4000)):
        Gd, Cd, g, c = so.dense_kkt(NX, NU, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = admm_lin_ref.dense_E(NX, NU, MX, MU, N, E[b])
        z, lam, y = h["z"][-1], h["lam"][-1], h["y"][-1]
        v = Ed @ z
        stat = np.abs(Gd @ z + g + Cd.T @ lam + RHO[b] * (Ed.T @ y)).max()
        feas = np.abs(Cd @ z - c).max()
        viol = max(np.maximum(lo[b] - v, 0).max(), np.maximum(v - hi[b], 0).max())
        comp = max(np.abs(v[y > 0] - hi[b][y > 0]).max(initial=0), np.abs(v[y < 0] - lo[b][y < 0]).max(initial=0))
        print(f"problem {b}: stationarity {stat:.2e} feasibility {feas:.2e} row violation {viol:.2e} complementarity {comp:.2e}")
        assert stat <= KKT_TOL and feas <= KKT_TOL and viol <= KKT_TOL and comp <= KKT_TOL
        # the sign of the multiplier: y > 0 only at an upper bound, y < 0 only at a lower one, y = 0 strictly inside
        assert np.isfinite(hi[b][y > 0]).all() and np.isfinite(lo[b][y < 0]).all()
        inside = (v > lo[b] + KKT_TOL) & (v < hi[b] - KKT_TOL)
        assert not y[inside].any()


def test_rows_of_each_kind_bind():
    _, E, lo, hi, z0 = inputs()
    kind = kinds()
    for b, h in enumerate(run(4000)):
        v0 = admm_lin_ref.dense_E(NX, NU, MX, MU, N, E[b]) @ z0[b]
        y = h["y"][-1]
        state, control = int((y[kind == 0] != 0).sum()), int((y[kind == 1] != 0).sum())
        violated = int(((v0 < lo[b]) | (v0 > hi[b])).sum())
        print(f"problem {b}: {state} state rows and {control} control rows active, {violated} rows violated by the unconstrained solution")
        assert state >= 1 and control >= 1
        assert (state, control, violated) == (ACTIVE_STATE[b], ACTIVE_CONTROL[b], VIOLATED[b])


def test_eighty_iterations_come_this_far():
    for b, h in enumerate(run(4000)):   # (the first 80 iterations of the same run)
        wstar = h["w"][-1]
        ratio = h["r_prim"][K - 1] / h["r_prim"][0]
        dist, first = np.abs(h["w"][K - 1] - wstar).max(), np.abs(h["w"][0] - wstar).max()
        print(f"problem {b}: r_prim(80)/r_prim(1) {ratio:.2e}  ||w(80) - w*|| {dist:.2e}  ||w(1) - w*|| {first:.2e}")
        assert ratio <= TABLE[b][0] and dist <= TABLE[b][1] and first >= TABLE[b][2]


def test_identity_rows_are_the_box_to_the_last_bit():
    d, lo, hi, _ = admm_ref.convergence_inputs()
    Ed = admm_lin_ref.dense_E(NX, NU, NX, NU, N, admm_lin_ref.identity_E(NX, NU, N))
    assert np.array_equal(Ed, np.eye(Ed.shape[0]))
    for b in range(B):
        Gd, Cd, g, c = so.dense_kkt(NX, NU, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        zero = np.zeros(g.size)
        box = admm_ref.admm(Gd, Cd, g, c, lo[b], hi[b], RHO[b], 40, zero, zero)
        lin = admm_lin_ref.admm_lin(Gd, Cd, Ed, g, c, lo[b], hi[b], RHO[b], 40, zero, zero)
        assert set(box) == set(lin)
        for k in box:
            assert same_bits(box[k], lin[k]), (b, k)


def test_form_ref_with_identity_rows_adds_rho_to_the_diagonal():
    nx, nu, n = 3, 2, 3
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        ng = admm_lin_ref.sizes(nx, nu, nx, nu, n)[3]
        G = rng.standard_normal((2, ng)).astype(dtype)
        rho = np.array([0.7, 3.1], dtype)
        Gt = admm_lin_ref.form_ref(dtype, nx, nu, nx, nu, n, G, np.stack([admm_lin_ref.identity_E(nx, nu, n, dtype)] * 2), rho)
        want = G.copy()
        for m, _, _, _, _, go in admm_lin_ref.blocks(nx, nu, nx, nu, n):
            idx = go + np.arange(m) * (m + 1)
            want[:, idx] = G[:, idx] + rho[:, None]        # one rounding in dtype
        assert want.dtype == np.dtype(dtype) and same_bits(Gt, want)


def test_fma_ref_rounds_once():
    """Cases where a rounded product followed by a rounded sum differs from the fused operation, and the ties."""
    f32, f64 = np.float32, np.float64
    a = f32(1 + 2.0 ** -12)
    assert admm_lin_ref.fma_ref(a, a, f32(-1), f32) == f32(2.0 ** -11 + 2.0 ** -24)       # a * a alone rounds the 2^-24 away
    assert f32(a * a) + f32(-1) == f32(2.0 ** -11)
    a = f64(1 + 2.0 ** -27)
    assert admm_lin_ref.fma_ref(a, a, f64(-1), f64) == f64(2.0 ** -26 + 2.0 ** -54)
    assert admm_lin_ref.round_to(admm_lin_ref.Fraction(1) + admm_lin_ref.Fraction(1, 2 ** 24), f32) == f32(1)            # tie to even
    assert admm_lin_ref.round_to(admm_lin_ref.Fraction(1) + admm_lin_ref.Fraction(3, 2 ** 24), f32) == f32(1 + 2.0 ** -22)
    assert admm_lin_ref.round_to(admm_lin_ref.Fraction(1, 2 ** 150), f32) == f32(0) and admm_lin_ref.round_to(admm_lin_ref.Fraction(3, 2 ** 150), f32) == f32(2.0 ** -148)
    z = admm_lin_ref.fma_ref(f32(-0.0), f32(2), f32(-0.0), f32)
    assert z == 0 and np.signbit(z) and not np.signbit(admm_lin_ref.fma_ref(f32(-0.0), f32(2), f32(0.0), f32))
    assert not np.signbit(admm_lin_ref.fma_ref(f32(3), f32(2), f32(-6), f32))
