"""CPU: the references of ADMM with linear and second-order cone rows (tests/admm_soc_ref.py).

 - update_ref / the initialisation in exact rational arithmetic (one rounding per operation, sqrt by integer isqrt) agree with the
   plain fp64 twin to a few ulp on random input, and sqrt_ref / div_ref round correctly on cases where the neighbours are known;
 - with no cone rows update_ref gives the bits of admm_lin_ref.update_ref; q = 1 cones with f = +0 give the bits of the rows
   0 <= s < +Inf;
 - on the inputs of the device's convergence test (tests/test_gpu_admm_soc.py: three 14 / 7 / 24 problems, a q = 4 thrust cone on u,
   2 linear rows + a q = 3 cone on x, rho = (3, 4, 2.5), w0 = y0 = 0) the twin's iterate after 4000 iterations satisfies the conic KKT
   conditions: stationarity with rho E'y, C z = c, the linear rows as in tests/test_admm_lin_reference.py, w in K, -y in K, y'w = 0,
   each held to the KKT_TOL = 1e-12 of that test (the cone conditions relative to 1 + ||w||, ||y||: w is only a few ulp from K);
 - the cap that keeps the device test honest: in the FIRST update each of the three projection branches (inside, polar, boundary) is
   taken by at least 10 % of the 47 cones of every problem; at the final iterate at least a quarter of the cones are on the boundary
   and at least one is strictly inside."""
import numpy as np

import admm_lin_ref
import admm_soc_ref as ref
from oracle import schur_oracle as so

NX, NU, N, B = ref.CONV_SHAPE
MX, MU = ref.CONV_ROWS
CONES = ref.CONV_CONES
RHO = ref.CONV_RHO
assert (NX, NU, N, B, MX, MU, CONES) == (14, 7, 24, 3, 5, 4, (2, 3, 0, 4)) and RHO == (3.0, 4.0, 2.5)
KKT_TOL = 1e-12     # tests/test_admm_lin_reference.py
ITER = 4000
F32, F64 = np.float32, np.float64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def random_case(seed, nx, nu, mx, mu, n, batch):
    rng = np.random.default_rng(seed)
    nz, nw, ne, _ = admm_lin_ref.sizes(nx, nu, mx, mu, n)
    d = dict(g=rng.standard_normal((batch, nz)), E=0.5 * rng.standard_normal((batch, ne)), z=rng.standard_normal((batch, nz)),
             w=rng.standard_normal((batch, nw)), y=0.3 * rng.standard_normal((batch, nw)),
             lo=-0.3 + 0.05 * rng.standard_normal((batch, nw)), hi=0.3 + 0.05 * rng.standard_normal((batch, nw)),
             rho=rng.uniform(0.5, 4.0, batch))
    return d


def test_sqrt_and_division_round_once():
    for dtype in (F32, F64):
        eps = np.finfo(dtype).eps
        one = dtype(1)
        assert ref.sqrt_ref(dtype(4), dtype) == dtype(2) and ref.sqrt_ref(dtype(0), dtype) == 0 and np.isnan(ref.sqrt_ref(dtype(np.nan), dtype))
        assert ref.sqrt_ref(dtype(np.inf), dtype) == np.inf
        # sqrt(1 + 2 eps) = 1 + eps - eps^2/2 + ...: rounds to 1 + eps;  sqrt(1 - eps) = 1 - eps/2 - ...: the neighbour below 1
        assert ref.sqrt_ref(one + 2 * eps, dtype) == one + eps
        assert ref.sqrt_ref(one - eps, dtype) == one - eps / 2
        tiny = np.finfo(dtype).smallest_subnormal
        assert float(ref.sqrt_ref(tiny, dtype)) ** 2 == float(tiny) or abs(float(ref.sqrt_ref(tiny, dtype)) ** 2 / float(tiny) - 1) < 4 * eps
        assert ref.div_ref(one, dtype(3), dtype) == one / dtype(3) and ref.div_ref(dtype(-0.0), dtype(3), dtype) == 0
        assert np.signbit(ref.div_ref(dtype(-0.0), dtype(3), dtype))
    rng = np.random.default_rng(1)
    for x in rng.uniform(0, 10, 200):                       # the platform's fp64 sqrt and / are IEEE: the same bits
        assert ref.sqrt_ref(F64(x), F64) == np.sqrt(F64(x))
        assert ref.sqrt_ref(F32(x), F32) == np.sqrt(F32(x))
        assert ref.div_ref(F64(x), F64(x + 0.37), F64) == F64(x) / F64(x + 0.37)


def test_rational_reference_agrees_with_the_fp64_twin():
    nx, nu, mx, mu, n, batch = 4, 3, 5, 4, 4, 2
    cones = (2, 3, 1, 3)
    d = random_case(3, nx, nu, mx, mu, n, batch)
    eps = np.finfo(F64).eps
    for init in (False, True):
        z = None if init else d["z"]
        wr, yr, gr, rr, br = ref.update_ref(F64, nx, nu, mx, mu, cones, n, d["g"], d["E"], d["lo"], d["hi"], d["rho"], z, d["w"], d["y"])
        wt, yt, gt_, rt = ref.update_twin(nx, nu, mx, mu, cones, n, d["g"], d["E"], d["lo"], d["hi"], d["rho"], z, d["w"], d["y"])
        scale = 1 + max(np.abs(a).max() for a in (wr, yr, gr))
        worst = max(np.abs(wr - wt).max(), np.abs(yr - yt).max(), np.abs(gr - gt_).max())
        print(f"init {init}: worst difference {worst / eps:.1f} eps at scale {scale:.1f}")
        assert worst <= 16 * eps * scale        # sums of at most 5 products of numbers of order 1: a few ulp of the scale
        if not init:
            assert np.abs(rr - rt).max() <= 16 * eps * scale
            taken = {v for b in br for v in b.values()}
            assert taken == {ref.INSIDE, ref.POLAR, ref.BOUNDARY}


def test_no_cones_and_half_lines_are_the_linear_rows_to_the_bit():
    nx, nu, mx, mu, n, batch = 3, 2, 3, 2, 3, 2
    d = random_case(4, nx, nu, mx, mu, n, batch)
    for dtype in (F32, F64):
        for init in (False, True):
            z = None if init else d["z"]
            a = admm_lin_ref.update_ref(dtype, nx, nu, mx, mu, n, d["g"], d["E"], d["lo"], d["hi"], d["rho"], z, d["w"], d["y"])
            b = ref.update_ref(dtype, nx, nu, mx, mu, (mx, 0, mu, 7), n, d["g"], d["E"], d["lo"], d["hi"], d["rho"], z, d["w"], d["y"])
            for x, y in zip(a, b[:4]):
                assert (x is None and y is None) or same_bits(x, y)
            zero, inf = np.zeros_like(d["lo"]), np.full_like(d["hi"], np.inf)
            a = admm_lin_ref.update_ref(dtype, nx, nu, mx, mu, n, d["g"], d["E"], zero, inf, d["rho"], z, d["w"], d["y"])
            b = ref.update_ref(dtype, nx, nu, mx, mu, (0, 1, 0, 1), n, d["g"], d["E"], zero, np.full_like(inf, np.nan), d["rho"], z, d["w"], d["y"])
            for x, y in zip(a, b[:4]):
                assert (x is None and y is None) or same_bits(x, y)


def counts(branch):
    return [sum(1 for v in branch.values() if v == k) for k in (ref.INSIDE, ref.POLAR, ref.BOUNDARY)]


def test_twin_reaches_the_conic_kkt_point_and_every_branch_is_taken():
    d, E, lo, hi, _ = ref.convergence_inputs()
    head, dim = ref.layout(NX, NU, MX, MU, CONES, N)
    linear = head < 0
    for b, h in enumerate(ref.convergence_reference(ITER)):
        Gd, Cd, g, c = so.dense_kkt(NX, NU, N, d["G"][b], d["C"][b], d["g"][b], d["c"][b])
        Ed = admm_lin_ref.dense_E(NX, NU, MX, MU, N, E[b])
        z, lam, y, w = h["z"][-1], h["lam"][-1], h["y"][-1], h["w"][-1]
        f = np.where(linear, 0.0, lo[b])
        v = Ed @ z + f
        stat = np.abs(Gd @ z + g + Cd.T @ lam + RHO[b] * (Ed.T @ y)).max()
        feas = np.abs(Cd @ z - c).max()
        split = np.abs(v - w).max()
        vl, yl, lol, hil = v[linear], y[linear], lo[b][linear], hi[b][linear]
        viol = max(np.maximum(lol - vl, 0).max(), np.maximum(vl - hil, 0).max())
        comp = max(np.abs(vl[yl > 0] - hil[yl > 0]).max(initial=0), np.abs(vl[yl < 0] - lol[yl < 0]).max(initial=0))
        in_k = in_polar = gap = 0.0
        strictly_inside = 0
        for h0 in ref.heads(head):
            q = int(dim[h0])
            wc, yc = w[h0:h0 + q], y[h0:h0 + q]
            in_k = max(in_k, (np.linalg.norm(wc[1:]) - wc[0]) / (1 + np.linalg.norm(wc)))
            in_polar = max(in_polar, (np.linalg.norm(yc[1:]) + yc[0]) / (1 + np.linalg.norm(yc)))      # -y in K
            gap = max(gap, abs(yc @ wc) / (1 + np.linalg.norm(wc) * np.linalg.norm(yc)))
            strictly_inside += bool(np.linalg.norm(wc[1:]) < wc[0] - KKT_TOL and not yc.any())
        first, last = (counts(br) for br in h["branch"])
        print(f"problem {b}: stationarity {stat:.2e} feasibility {feas:.2e} ||E z + f - w|| {split:.2e} row violation {viol:.2e} "
              f"complementarity {comp:.2e} w in K {in_k:.2e} -y in K {in_polar:.2e} y'w {gap:.2e}; first update "
              f"inside/polar/boundary {first}, last {last}, strictly inside {strictly_inside}")
        assert max(stat, feas, split, viol, comp, in_k, in_polar, gap) <= KKT_TOL
        total = sum(first)
        assert total == 2 * N - 1 == 47
        assert min(first) >= 0.1 * total, first                  # every branch in the first update
        assert last[2] >= 0.25 * total and strictly_inside >= 1, (last, strictly_inside)


def test_eighty_iterations_have_not_converged_yet_but_decrease():
    """What the device is compared with after 80 replays is an iterate on its way, not the fixed point: r_prim(80) / r_prim(1) lies
    between 1e-5 and 0.5 in every problem (measured 4.2e-2 / 1.8e-4 / 1.4e-1)."""
    for b, h in enumerate(ref.convergence_reference(ITER)):
        ratio = h["r_prim"][79] / h["r_prim"][0]
        print(f"problem {b}: r_prim(80)/r_prim(1) {ratio:.2e}  r_dual(80)/r_dual(1) {h['r_dual'][79] / h['r_dual'][0]:.2e}")
        assert 1e-5 < ratio < 0.5
