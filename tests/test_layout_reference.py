"""CPU: the oracle on NON-SYMMETRIC operators against plain numpy fp64 (tests/layout_ref.py), and the two conditions that
give the tolerances of tests/test_gpu_layout.py their meaning, for every row of its fixed-count solve table:

  (i)  the oracle's four summation orders agree on lambda within HALF the tolerance the GPU test uses (1e-6 fp32 / 1e-10 fp64
       norm-wise), and on r and p within half of theirs (2e-5 / 1e-9 of max|gamma|): a kernel that does the same arithmetic
       in yet another order has room to pass;
  (ii) each index mistake -- D read transposed, L_{k+1} taken from R_k^T, R_k taken from L_{k+1}^T, the L and R slots swapped
       -- applied to the READING of S alone and of Pinv alone moves lambda by at least 100 x that tolerance: a kernel that makes
       one cannot pass.  On mirrored storage only the D mistake changes the matrix.

`python -m pytest tests/test_layout_reference.py -q -s` prints the table of (ii): the smallest shift per mistake and row.
"""
import numpy as np
import pytest

import layout_ref as lr
from gbd_pcg_amd import synth

ALL_ROWS = lr.SOLVE_ROWS + lr.MIXED_ROWS + lr.SHARED_ROWS
# one entry per distinct (shape, dtype, generator): the symmetric mode and the forced path do not change the inputs
ROWS = list({lr.row_key(r): r for r in ALL_ROWS}.values())


# ----------------------------------------------------------------------------------------- dense assembly and the product
@pytest.mark.parametrize("n,N", [(2, 3), (3, 5), (7, 2), (14, 1), (14, 9), (13, 18), (36, 4), (37, 6)])
def test_oracle_dense_and_spmv_on_general_storage(orc, n, N):
    """orc.dense_from_bt and orc.spmv (all four summation orders) on a matrix whose blocks are all different and whose corner
    slots are NaN, against dense() built from synth.unpack_bt: fp64, component-wise
    |y - yhat| <= 2 (3n + 2) u (|M| |x|), the bound tests/test_gpu_layout.py holds the kernels to."""
    B = 2
    d = lr.gen_general(n, N, seed=40 + n + N, batch=B, dtype=np.float64)
    x = np.stack([synth.normals(50 + b, 0, n * N) for b in range(B)])
    for b in range(B):
        A = lr.dense(n, N, d["S"][b])
        assert np.isfinite(A).all()
        assert np.array_equal(orc.dense_from_bt(n, N, d["S"][b]), A)
        # not symmetric anywhere a kernel could mix the two sides up
        assert not np.allclose(A, A.T, atol=1e-3)
        want, bound = A @ x[b], 2 * (3 * n + 2) * lr.unit(np.float64) * (np.abs(A) @ np.abs(x[b]))
        for flags in range(4):
            y = orc.spmv(n, N, d["S"][b], x[b], flags=flags)
            assert np.isfinite(y).all()
            assert (np.abs(y - want) <= bound).all(), (flags, np.abs(y - want).max())


def test_generators():
    """What the two generators promise: general storage differs on both sides of every seam and has NaN corners; mirrored
    storage has L_{k+1} == R_k^T bit for bit after the cast while no D block is symmetric; the symmetric part of every D of S
    stays positive definite."""
    n, N, B = 6, 5, 2
    for dt in (np.float32, np.float64):
        g = lr.gen_general(n, N, seed=3, batch=B, dtype=dt)
        m = lr.gen_mirrored(n, N, seed=3, batch=B, dtype=dt)
        for key in ("S", "Pinv"):
            L, D, R = synth.unpack_bt(n, N, g[key])
            assert np.isnan(L[:, 0]).all() and np.isnan(R[:, N - 1]).all()
            assert np.isfinite(L[:, 1:]).all() and np.isfinite(R[:, :-1]).all() and np.isfinite(D).all()
            assert (np.abs(L[:, 1:] - np.swapaxes(R[:, :-1], -1, -2)).max(axis=(-1, -2)) > 0.05).all()
            L, D, R = synth.unpack_bt(n, N, m[key])
            assert np.array_equal(L[:, 1:], np.swapaxes(R[:, :-1], -1, -2))
            assert (np.abs(D - np.swapaxes(D, -1, -2)).max(axis=(-1, -2)) > 0.05).all()
        for d in (g, m):
            D = np.asarray(synth.unpack_bt(n, N, d["S"])[1], np.float64)
            assert np.linalg.eigvalsh(0.5 * (D + np.swapaxes(D, -1, -2))).min() > 0.5


# --------------------------------------------------------------------------------------- the recurrence and the conditions
def _spread(vals, scale):
    """Largest pairwise distance of the four variants (norm-wise relative to `scale`, or max-norm over it)."""
    return max(scale(vals[i], vals[j]) for i in range(4) for j in range(i))


@pytest.fixture(scope="module")
def mutant_table():
    rows = []
    yield rows
    if rows:
        names = [f"{m} {w}" for w in ("S", "Pinv") for m in lr.MUTANTS]
        print("\nsmallest relative shift of lambda per index mistake (required: >= 100 x tol)")
        print(f"{'row':44s} {'tol':>7s} " + " ".join(f"{x:>12s}" for x in names))
        for rid, tol, shifts in rows:
            print(f"{rid:44s} {tol:7.0e} " + " ".join(f"{shifts[x]:12.2e}" if x in shifts else f"{'-':>12s}" for x in names))


@pytest.mark.parametrize("row", ROWS, ids=lr.row_id)
def test_fixed_count_rows(orc, mutant_table, row):
    fam, n, N, B, dt, gen, mode = row
    c = lr.row_case(row)
    m = c["base"]                      # every other problem of the batch is a scaled copy of one of these
    tol, vt = lr.ltol(dt), lr.vtol(dt)
    var = lr.oracle_variants(orc, c, problems=m)
    for o in var:
        assert (o["iters"] == lr.K_FIXED).all() and o["max_iter_exit"].all()
    # the same storage in fp64: oracle (default order) against the plain recurrence on dense matrices, <= 1e-12
    o64 = orc.pcg_batch(n, N, m, c["S"][:m].astype(np.float64), c["Pinv"][:m].astype(np.float64), c["gamma"][:m].astype(np.float64),
                        lambda0=c["lam0"][:m].astype(np.float64), tol=0.0, max_iter=lr.K_FIXED)
    shifts = {}
    for b in range(m):
        Sd, Pd = lr.dense(n, N, c["S"][b]), lr.dense(n, N, c["Pinv"][b])
        lam, r, p = lr.pcg_fixed(Sd, Pd, c["gamma"][b], c["lam0"][b], lr.K_FIXED)
        assert np.isfinite(lam).all() and np.isfinite(r).all() and np.isfinite(p).all()
        for key, want in (("lambda_", lam), ("r", r), ("p", p)):
            assert lr.relerr(o64[key][b], want) <= 1e-12, (key, b, lr.relerr(o64[key][b], want))
        # (i) the four summation orders
        gmax = np.abs(c["gamma"][b]).max()
        s_lam = _spread([o["lambda_"][b] for o in var], lr.relerr)
        assert s_lam <= 0.5 * tol, ("lambda", b, s_lam)
        for key in ("r", "p"):
            s = _spread([o[key][b].astype(np.float64) for o in var], lambda x, y: np.abs(x - y).max() / gmax)
            assert s <= 0.5 * vt, (key, b, s)
        # (ii) the index mistakes, in S alone and in Pinv alone
        for which in lr.MUTANTS:
            if (gen == "mirrored" or (gen == "mixed" and b % 2 == 0)) and which != "D->D^T":
                continue               # L_{k+1} == R_k^T: the other three read the same matrix
            for name, mats in (("S", (lr.dense_blocks(*lr.mutant_blocks(n, N, c["S"][b], which)), Pd)),
                               ("Pinv", (Sd, lr.dense_blocks(*lr.mutant_blocks(n, N, c["Pinv"][b], which))))):
                lam_m, _, _ = lr.pcg_fixed(mats[0], mats[1], c["gamma"][b], c["lam0"][b], lr.K_FIXED)
                shift = lr.relerr(lam_m, lam) if np.isfinite(lam_m).all() else np.inf
                key = f"{which} {name}"
                shifts[key] = min(shifts.get(key, np.inf), shift)
                assert shift >= 100 * tol, (which, name, b, shift)
    mutant_table.append((lr.row_id(row)[len(fam) + 1:-3], tol, shifts))
