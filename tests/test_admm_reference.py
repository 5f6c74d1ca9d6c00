"""CPU: the fp64 reference of the box-constrained ADMM iteration (tests/admm_ref.py) on the inputs of the device's convergence test
(tests/test_gpu_admm.py): so.gen(14, 7, 24, seed=11, batch=3, float32) held in fp64, rho = (3, 4, 2.5), the bounds of admm_ref.box,
w0 = y0 = 0.

 - after 4000 iterations the reference satisfies the KKT conditions of the box-constrained QP in fp64 (1e-12);
 - after 80 iterations it has come as far as the table below says, per problem -- so that "80 replays" asks something of the device;
 - the box is not decoration: the unconstrained solution violates it in 24 / 43 / 37 entries and 21 / 38 / 35 are active at z*.
The figures were measured with this code (ratios 5.6e-6 / 2.3e-4 / 1.5e-3, distances 1.1e-6 / 3.3e-5 / 4.4e-4, first-iteration
distances 0.19 / 0.16 / 0.29); the test pins the generator: if its output ever differs this fails here, not on the device."""
import numpy as np

import admm_ref
from oracle import schur_oracle as so

NX, NU, N, B = admm_ref.CONV_SHAPE
RHO = admm_ref.CONV_RHO
assert (NX, NU, N, B) == (14, 7, 24, 3) and RHO == (3.0, 4.0, 2.5)
K = 80
# problem: r_prim(80) / r_prim(1) at most, ||z(80) - z*||_inf at most, ||z(1) - z*||_inf at least
TABLE = {0: (1e-5, 2e-6, 0.15), 1: (5e-4, 5e-5, 0.15), 2: (3e-3, 6e-4, 0.15)}
VIOLATED, ACTIVE = (24, 43, 37), (21, 38, 35)


inputs, run = admm_ref.convergence_inputs, admm_ref.convergence_reference


def test_reference_reaches_the_kkt_point_of_the_box_qp():
    d, lo, hi, _ = inputs()
    for b, h in enumerate(run(4000)):
        Gd, Cd, g, c = so.dense_kkt(NX, NU, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        z, lam, y = h["z"][-1], h["lam"][-1], h["y"][-1]
        stat = np.abs(Gd @ z + g + Cd.T @ lam + RHO[b] * y).max()
        feas = np.abs(Cd @ z - c).max()
        viol = max(np.maximum(lo[b] - z, 0).max(), np.maximum(z - hi[b], 0).max())
        print(f"problem {b}: stationarity {stat:.2e} feasibility {feas:.2e} box violation {viol:.2e}")
        assert stat <= 1e-12 and feas <= 1e-12 and viol <= 1e-12
        assert (np.abs(z[y > 0] - hi[b][y > 0]) <= 1e-12).all()
        assert (np.abs(z[y < 0] - lo[b][y < 0]) <= 1e-12).all()


def test_eighty_iterations_come_this_far():
    zstar = [h["z"][-1] for h in run(4000)]
    for b, h in enumerate(run(4000)):   # (the first 80 iterations of the same run)
        ratio = h["r_prim"][K - 1] / h["r_prim"][0]
        dist, first = np.abs(h["z"][K - 1] - zstar[b]).max(), np.abs(h["z"][0] - zstar[b]).max()
        print(f"problem {b}: r_prim(80)/r_prim(1) {ratio:.2e}  ||z(80) - z*|| {dist:.2e}  ||z(1) - z*|| {first:.2e}")
        assert ratio <= TABLE[b][0] and dist <= TABLE[b][1] and first >= TABLE[b][2]


def test_the_box_binds():
    _, lo, hi, z0 = inputs()
    for b, h in enumerate(run(4000)):
        violated = int(((z0[b] < lo[b]) | (z0[b] > hi[b])).sum())
        active = int((h["y"][-1] != 0).sum())
        print(f"problem {b}: {violated} entries of the unconstrained solution outside the box, {active} active at z*")
        assert violated == VIOLATED[b] and active == ACTIVE[b]
