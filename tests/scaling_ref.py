"""Exact power-of-two rescaling of the variables, for tests/test_scaling_reference.py (CPU) and tests/test_gpu_scaling.py (GPU);
not a test module.

With z = T z', T = diag(t) and every t an integer power of two, every operation of this library is equivariant, and because a
power of two only moves the exponent every floating-point operation commutes with the scaling: the property holds BIT FOR BIT,
whatever the summation order, the FMA contraction or the reciprocal method, as long as nothing overflows or goes subnormal
(every sum the algorithms form adds terms of one common scale).  The identity blocks of C stay identities, so constraint row
block k is scaled by E_k = (T^x_k)^-1.

Everything here works on EXPONENTS: `exps(kind, ...)` is the integer array e with  transformed = base * 2^e  in the packed layout
of `kind`, `apply` / `undo` are numpy.ldexp with +e / -e (exact inside the range `in_range` asserts).

    kind     transformed                       kind     transformed
    G        T G T                             S        E S E    (block (k, l): E_k left, E_l right)
    Ginv     T^-1 G^-1 T^-1                    Pinv     T^x Phi^-1 T^x
    C        A_k: E_k+1 A_k T^x_k              gamma r  E gamma
             B_k: E_k+1 B_k T^u_k              lam p    T^x lambda
    g        T g                               gG       as Ginv
    z        T^-1 z                            gC       the dual of C: 1 / (the factor of C)
    c        E c

`form_twin` is the formation in WORKING precision in numpy: Gauss-Jordan without pivoting and the block formulas of
oracle/schur_oracle.py::form_schur, every sum in an order that does not depend on the values.
"""
import numpy as np

F32_LIM, F64_LIM = 12, 40            # exponents are integers in [-lim, lim]
F32_RANGE, F64_RANGE = 100, 900      # every compared non-zero finite entry has magnitude in [2^-range, 2^range]


def lim(dtype):
    return F64_LIM if np.dtype(dtype) == np.float64 else F32_LIM


def draw(seed, nx, nu, N, K, lim, uniform=False):
    """Exponents of K copies of one problem: (ex [K, N, nx], eu [K, max(N-1, 0), nu]) integers in [-lim, lim].  Copy 0 is unscaled.
    The last copy is the worst scaled: both ends of the range sit inside every block that has two entries.  uniform: one
    exponent per copy (0, then +lim, -lim, then drawn)."""
    rng = np.random.default_rng(seed)
    M = max(N - 1, 0)
    if uniform:
        a = np.array(([0, lim, -lim] + list(rng.integers(-lim, lim + 1, max(K - 3, 0))))[:K], dtype=np.int64)
        if K >= 2:
            a[[1, K - 1]] = a[[K - 1, 1]]          # the last copy is the one furthest from 1
        return np.broadcast_to(a[:, None, None], (K, N, nx)).copy(), np.broadcast_to(a[:, None, None], (K, M, nu)).copy()
    ex = rng.integers(-lim, lim + 1, (K, N, nx))
    eu = rng.integers(-lim, lim + 1, (K, M, nu))
    ex[0], eu[0] = 0, 0
    if K > 1:
        ex[K - 1, :, 0] = lim
        ex[K - 1, :, -1] = -lim if nx > 1 else lim
        eu[K - 1, :, 0] = -lim
        eu[K - 1, :, -1] = lim if nu > 1 else -lim
    return ex, eu


def exps(kind, nx, nu, N, ex, eu=None):
    """Exponent array [K, size of kind] (see the module docstring); ex [K, N, nx], eu [K, N-1, nu]."""
    ex = np.asarray(ex, dtype=np.int64)
    K = ex.shape[0]
    if kind in ("lam", "p"):
        return ex.reshape(K, -1)
    if kind in ("c", "gamma", "r"):
        return -ex.reshape(K, -1)
    if kind in ("S", "Pinv"):
        s = -1 if kind == "S" else 1
        e = np.zeros((K, N, 3, nx, nx), dtype=np.int64)               # [copy, knot, slot, column, row]
        for slot in range(3):
            for k in range(N):
                kc = k + slot - 1
                if 0 <= kc < N:                                         # (the corner slots are never read: factor 1)
                    e[:, k, slot] = s * (ex[:, kc, :, None] + ex[:, k, None, :])
        return e.reshape(K, -1)
    eu = np.asarray(eu, dtype=np.int64)
    out = []
    for k in range(N):
        last = k == N - 1
        if kind in ("g", "z"):
            part = [ex[:, k]] + ([] if last else [eu[:, k]])
        elif kind in ("G", "Ginv", "gG"):
            part = [(ex[:, k, :, None] + ex[:, k, None, :]).reshape(K, -1)]
            if not last:
                part.append((eu[:, k, :, None] + eu[:, k, None, :]).reshape(K, -1))
        elif kind in ("C", "gC"):
            if last:
                continue
            part = [(ex[:, k, :, None] - ex[:, k + 1, None, :]).reshape(K, -1),     # A_k, stored [column, row]
                    (eu[:, k, :, None] - ex[:, k + 1, None, :]).reshape(K, -1)]     # B_k
        else:
            raise ValueError(kind)
        out += part
    e = np.concatenate(out, axis=1) if out else np.zeros((K, 0), dtype=np.int64)
    return -e if kind in ("z", "Ginv", "gG", "gC") else e


def apply(a, e):
    """base -> transformed (exact: ldexp in the array's own precision)."""
    a = np.asarray(a)
    return np.ldexp(a, np.asarray(e).reshape(a.shape).astype(np.int32)).astype(a.dtype)


def undo(a, e):
    """transformed -> base."""
    return apply(a, -np.asarray(e))


def copies(base, kind, nx, nu, N, ex, eu=None):
    """One problem's array of `kind` -> its K transformed copies [K, size]."""
    e = exps(kind, nx, nu, N, ex, eu)
    return apply(np.broadcast_to(np.asarray(base).reshape(1, -1), e.shape), e)


def kkt_copies(d, nx, nu, N, ex, eu, b=0):
    """Problem b of a dict of packed G, C, g, c -> dict of the K transformed copies."""
    return {k: copies(d[k][b], k, nx, nu, N, ex, eu) for k in "GCgc"}


def in_range(dtype, *arrays):
    """The range condition: every non-zero finite entry has magnitude in [2^-R, 2^R], R = 100 (fp32) / 900 (fp64)."""
    R = F64_RANGE if np.dtype(dtype) == np.float64 else F32_RANGE
    for a in arrays:
        m = np.abs(np.asarray(a, dtype=np.float64))
        m = m[np.isfinite(m) & (m != 0)]
        if m.size and not (m.min() >= 2.0 ** -R and m.max() <= 2.0 ** R):
            return False
    return True


def assert_equivariant(name, got, e, dtype):
    """got [K, m] holds the K copies' outputs, e their exponents: after exact unscaling every copy equals copy 0 bit for bit;
    both sides of the comparison satisfy the range condition.  Returns the unscaled array."""
    got = np.asarray(got).reshape(np.shape(e))
    assert got.dtype == np.dtype(dtype), (name, got.dtype)
    back = undo(got, e)
    assert in_range(dtype, got, back), f"{name}: range condition"
    assert np.isfinite(got).all(), f"{name}: an output is not finite (or was never written)"
    for k in range(1, got.shape[0]):
        if not np.array_equal(back[k], back[0]):
            bad = np.flatnonzero(back[k] != back[0])
            raise AssertionError(f"{name}: copy {k} differs from copy 0 after unscaling in {bad.size} of {back[0].size} entries, "
                                 f"first at {bad[0]}: {back[k][bad[0]]!r} against {back[0][bad[0]]!r}")
    return back


# ------------------------------------------------------------------------------------------- the cases, both test files
f32, f64 = np.float32, np.float64
DTYPES = [f32, f64]
KKT_SHAPES = [(14, 7, 9), (14, 7, 1), (3, 3, 2), (2, 1, 5), (13, 4, 5), (12, 4, 33), (4, 6, 3), (36, 12, 3)]     # nx, nu, N
UNIFORM_SHAPES = [(14, 7, 24), (5, 2, 9)]                                                                       # three copies each
PINV_SHAPES = [(14, 2), (14, 17), (14, 128), (8, 20), (16, 33), (36, 17), (7, 9)]                               # n, N
SPMV_N, SPMV_KNOTS = [3, 14, 16, 37], 5
K_COPIES = 3
RUNS = [("tol", 1e-6, 200), ("fixed", 0.0, 6)]            # the two runs of every solve case: (name, tol, max_iter)
# (family, n, N, dtype, symmetric mode, B, distinct base problems, warm start); the GPU half forces the dispatch and asserts what
# the C ABI lets it see of it (path, workgroups per cluster, batch against the number of compute units).
# "sym": B = 132 = 44 x 3 copies, more than one round of two-workgroup clusters on 256 compute units: below that, mode 2 hands
# the batch to the cluster kernel in general storage (csrc/api_solve.hip, one_cluster_round) and never runs the verifying kernel.
# "symstream": symmetric streaming exists for even n in 8 ... 16 beyond the horizons of the resident and cluster kernels and for
# batches of at least one problem per compute unit: fp64 12 x 161 (resident up to 40 knots, clusters up to 160).  In fp32 the
# cluster kernel holds n = 12 up to 640 knots (n = 16: 512, n = 8: 1024), so the smallest fp32 case is 256 x (12, 641): 284 MB
# per matrix, 1.1 GB of host arrays to scale and compare -- too heavy for this suite, and left out.
SOLVE_CASES = (
    [("sym", 14, N, f32, mode, 132, 1, (N, mode) == (73, 2)) for N in (73, 128) for mode in (1, 2)]
    + [("resident", n, N, dt, 0, 3, 1, False) for (n, N) in ((7, 9), (13, 5)) for dt in DTYPES]
    + [("cluster", 14, 145, f32, 0, 3, 1, False), ("cluster", 14, 65, f64, 0, 3, 1, True), ("cluster", 16, 33, f32, 0, 3, 1, False)]
    + [("stream", 24, 20, dt, 0, 3, 1, False) for dt in DTYPES]
    + [("split", 14, 40, dt, 0, 3, 1, False) for dt in DTYPES]
    + [(fam, n, N, dt, 0, 3, 1, False) for fam in ("persist", "persist1r") for (n, N, dt) in ((36, 64, f64), (14, 200, f32))]
    + [("symstream", 12, 161, f64, 2, 256, 3, False)]
)


def kkt_case(nx, nu, N, dtype, uniform=False, seed=700):
    """The KKT inputs of both halves: two problems of oracle/schur_oracle.py::gen (drawn in fp32, widened for fp64; the second
    supplies a new g and c) and the exponents of the K copies.  Returns d, d2, ex, eu."""
    from oracle import schur_oracle as so
    d = {k: v.astype(dtype) for k, v in so.gen(nx, nu, N, seed=seed + nx + N, batch=1, dtype=np.float32).items()}
    d2 = {k: v.astype(dtype) for k, v in so.gen(nx, nu, N, seed=seed + 1 + nx + N, batch=1, dtype=np.float32).items()}
    ex, eu = draw(seed + nx + N, nx, nu, N, K_COPIES, lim(dtype), uniform)
    return d, d2, ex, eu


def solve_id(case):
    fam, n, N, dt, mode, B, bases, warm = case
    return f"{fam}-{n}x{N}x{B}-{np.dtype(dt).name}-m{mode}" + ("-warm" if warm else "")


def solve_case(n, N, dtype, B, bases=1, warm=False, uniform=False, seed=None, K=K_COPIES):
    """B problems: problem b is copy (b // bases) % K of base problem b % bases (synth.gen_numpy in fp32, widened for fp64), so
    the first `bases` problems are unscaled.  Returns S [B, 3n^2N], Pinv (the host's stair, transformed), gamma, lam0 [B, nN]
    in dtype, the exponents E[kind] [B, ...] and `first` [B]: the unscaled problem every problem must equal after unscaling."""
    from gbd_pcg_amd import synth
    seed = 3000 + 41 * n + N if seed is None else seed
    d = synth.gen_numpy(n, N, seed=seed, batch=bases, dtype=np.float32)
    ex, _ = draw(seed, n, 1, N, K, lim(dtype), uniform)
    bi, ci = np.arange(B) % bases, (np.arange(B) // bases) % K
    E = {kind: exps(kind, n, 1, N, ex).astype(np.int32)[ci] for kind in ("S", "Pinv", "gamma", "lam", "r", "p")}
    lam0 = np.stack([0.1 * synth.normals(seed + j, 30, n * N) if warm else np.zeros(n * N) for j in range(bases)]).astype(np.float32)
    out = dict(n=n, N=N, batch=B, E=E, first=bi, copy=ci,
               S=apply(d["S"].astype(dtype)[bi], E["S"]), Pinv=apply(d["Pinv"].astype(dtype)[bi], E["Pinv"]),
               gamma=apply(d["gamma"].astype(dtype)[bi], E["gamma"]), lam0=apply(lam0.astype(dtype)[bi], E["lam"]))
    assert in_range(dtype, out["S"], out["Pinv"], out["gamma"], out["lam0"]), "range condition (inputs)"
    return out


def assert_solve_equivariant(name, c, out, dtype):
    """lambda, r, p of every problem equal those of its unscaled first copy after unscaling; iteration counts and exit flags
    are equal as they are.  out: dict of lambda_, r, p [B, nN], iters, flag [B].  Returns the unscaled lambda, r, p."""
    back = {}
    for key, kind in (("lambda_", "lam"), ("r", "r"), ("p", "p")):
        got = np.asarray(out[key]).reshape(c["batch"], -1)
        assert got.dtype == np.dtype(dtype)
        back[key] = undo(got, c["E"][kind])
        assert in_range(dtype, got, back[key]), f"{name}: range condition ({key})"
    it, fl = np.asarray(out["iters"]).astype(np.int64), np.asarray(out["flag"]).astype(bool)
    for b in range(c["batch"]):
        f = c["first"][b]
        assert it[b] == it[f] and fl[b] == fl[f], (name, b, it[b], it[f], fl[b], fl[f])
        for key in back:
            assert np.array_equal(back[key][b], back[key][f]), f"{name}: {key} of problem {b} (copy {c['copy'][b]}) after unscaling"
    return back


def mask_corners(P, N, n):
    """A copy of [B, 3n^2N] storage with the never-read corner slots (L_0, R_{N-1}) zeroed: their contents are unspecified."""
    P = np.array(P).reshape(-1, N, 3, n * n)
    P[:, 0, 0] = 0
    P[:, N - 1, 2] = 0
    return P.reshape(P.shape[0], -1)


# ---------------------------------------------------------------------------------- the formation in working precision
def mm(a, b):
    """a @ b in the operands' precision, the inner index accumulated in order (no BLAS: the order is fixed by the shapes)."""
    out = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
    for m in range(a.shape[1]):
        out += np.multiply.outer(a[:, m], b[m, :])
    return out


def gauss_jordan(a):
    """Inverse by Gauss-Jordan WITHOUT pivoting, in a's precision."""
    n = a.shape[0]
    w = np.concatenate([a.copy(), np.eye(n, dtype=a.dtype)], axis=1)
    for k in range(n):
        w[k] = w[k] * (a.dtype.type(1) / w[k, k])
        for i in range(n):
            if i != k:
                w[i] = w[i] - w[i, k] * w[k]
    return np.ascontiguousarray(w[:, n:])


def form_twin(nx, nu, N, G, C, g, c):
    """oracle/schur_oracle.py::form_schur in the precision of G.  Returns S, gamma, Ginv, packed."""
    dt = np.asarray(G).dtype
    sg, sc, sv = nx * nx + nu * nu, nx * nx + nx * nu, nx + nu
    G, C, g, c = (np.asarray(a, dtype=dt) for a in (G, C, g, c))
    Q = [G[k * sg:k * sg + nx * nx].reshape(nx, nx).T for k in range(N)]
    R = [G[k * sg + nx * nx:(k + 1) * sg].reshape(nu, nu).T for k in range(N - 1)]
    A = [C[k * sc:k * sc + nx * nx].reshape(nx, nx).T for k in range(N - 1)]
    B = [C[k * sc + nx * nx:(k + 1) * sc].reshape(nu, nx).T for k in range(N - 1)]
    q = [g[k * sv:k * sv + nx].reshape(-1, 1) for k in range(N)]
    r = [g[k * sv + nx:(k + 1) * sv].reshape(-1, 1) for k in range(N - 1)]
    Qi, Ri = [gauss_jordan(m) for m in Q], [gauss_jordan(m) for m in R]
    S = np.zeros((N, 3, nx * nx), dtype=dt)
    gamma = np.zeros((N, nx), dtype=dt)
    for k in range(N):
        D = Qi[k].copy()
        v = c[k * nx:(k + 1) * nx].reshape(-1, 1) + mm(Qi[k], q[k])
        if k > 0:
            j = k - 1
            W, V = mm(A[j], Qi[j]), mm(B[j], Ri[j])
            D = D + (mm(W, A[j].T) + mm(V, B[j].T))
            v = v - (mm(W, q[j]) + mm(V, r[j]))
            S[k, 0] = (-W).T.reshape(-1)
        if k < N - 1:
            S[k, 2] = (-mm(Qi[k], A[k].T)).T.reshape(-1)
        S[k, 1] = D.T.reshape(-1)
        gamma[k] = -v[:, 0]
    Ginv = []
    for k in range(N):
        Ginv.append(Qi[k].T.reshape(-1))
        if k < N - 1:
            Ginv.append(Ri[k].T.reshape(-1))
    out = S.reshape(-1), gamma.reshape(-1), np.concatenate(Ginv)
    assert all(a.dtype == dt for a in out)
    return out


def residual_fixed_order(Gd, Cd, g, c, z, lam):
    """(G z + g + C' lambda, C z - c) in fp64, every row summed column by column in index order (zeros included)."""
    st, fe = np.array(g, dtype=np.float64), -np.array(c, dtype=np.float64)
    acc_s, acc_f = np.zeros_like(st), np.zeros_like(fe)
    for j in range(Gd.shape[1]):
        acc_s += Gd[:, j] * z[j]
        acc_f += Cd[:, j] * z[j]
    for j in range(Cd.shape[0]):
        acc_s += Cd[j, :] * lam[j]
    return acc_s + st, acc_f + fe
