"""Plain numpy fp64 references and NON-SYMMETRIC test operators for the [L|D|R] column-major layout (not a test module).

Everything the rest of the suite feeds a kernel is symmetric as a whole matrix up to rounding, which pins the layout only up
to transposition.  The operators built here differ on the two sides of every seam: a kernel that reads a D block row-major,
takes L_{k+1} x_k from R_k^T, swaps its neighbours or builds a left slot from the right one gives a visibly different answer.
The references do not go through the oracle: `dense` assembles the matrix from synth.unpack_bt alone and `pcg_fixed` is the
recurrence of pcg.cuh:118-206 on dense fp64 matrices.

tests/test_layout_reference.py (CPU) checks, for every row of SOLVE_ROWS, that the oracle agrees with these references, that
its four summation orders agree within half of what the GPU tests allow, and that each transposition mistake moves lambda by
at least a hundred times that; tests/test_gpu_layout.py (GPU) then holds the kernels to the same rows.
"""
import numpy as np

from gbd_pcg_amd import synth

F32_TOL, F64_TOL = 1e-6, 1e-10          # lambda, norm-wise against the oracle (tests/test_gpu_parity.py)
F32_VTOL, F64_VTOL = 2e-5, 1e-9         # r and p, max-norm on the scale of max|gamma| (tests/test_gpu_cluster.py check())
K_FIXED = 4                             # iterations of every fixed-count solve
DELTA = 0.3                             # size of the non-symmetric part


def ltol(dtype):
    return F64_TOL if np.dtype(dtype) == np.float64 else F32_TOL


def vtol(dtype):
    return F64_VTOL if np.dtype(dtype) == np.float64 else F32_VTOL


def unit(dtype):
    """Unit roundoff of the format."""
    return 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24


def relerr(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# --------------------------------------------------------------------------------------------------------- references
def dense_blocks(L, D, R):
    """Dense nN x nN fp64 matrix from [N, n, n] row/column-indexed blocks; L_0 and R_{N-1} are left out."""
    N, n = D.shape[0], D.shape[-1]
    A = np.zeros((n * N, n * N))
    for k in range(N):
        A[k * n:(k + 1) * n, k * n:(k + 1) * n] = D[k]
        if k > 0:
            A[k * n:(k + 1) * n, (k - 1) * n:k * n] = L[k]
        if k + 1 < N:
            A[k * n:(k + 1) * n, (k + 1) * n:(k + 2) * n] = R[k]
    return A


def dense(n, N, M):
    """Dense fp64 matrix of ONE problem in the [L|D|R] column-major layout, from synth.unpack_bt alone."""
    L, D, R = (np.asarray(b, dtype=np.float64) for b in synth.unpack_bt(n, N, np.asarray(M).reshape(-1)))
    return dense_blocks(L, D, R)


def pcg_fixed(S, P, g, lam0, k):
    """k iterations of the reference recurrence (pcg.cuh:118-206, no exit test) in fp64 on dense S and P.  Returns (lam, r, p)."""
    S, P = np.asarray(S, np.float64), np.asarray(P, np.float64)
    lam = np.array(lam0, dtype=np.float64)
    r = np.asarray(g, np.float64) - S @ lam
    z = P @ r
    p = z.copy()
    eta = r @ z
    for _ in range(k):
        Sp = S @ p
        alpha = eta / (p @ Sp)
        lam += alpha * p
        r -= alpha * Sp
        z = P @ r
        eta_new = r @ z
        p = z + (eta_new / eta) * p
        eta = eta_new
    return lam, r, p


# ---------------------------------------------------------------------------------------------------------- generators
def _perturb(n, N, M, seed, stream, delta, mirrored):
    """One problem's flat fp64 matrix -> the same with a non-symmetric part of size delta (see gen_general / gen_mirrored)."""
    L, D, R = (np.array(b, dtype=np.float64) for b in synth.unpack_bt(n, N, M))
    K = synth.normals(seed, stream, N * n * n).reshape(N, n, n) / np.sqrt(n)
    D += delta * (K - np.swapaxes(K, -1, -2))          # skew: the symmetric part of D_k stays positive definite
    if mirrored:
        L[1:] = np.swapaxes(R[:-1], -1, -2)            # bit for bit (the stair blocks of numpy are mirrors only up to rounding)
    else:
        L += delta * synth.normals(seed, stream + 1, N * n * n).reshape(N, n, n) / np.sqrt(n)
        R += delta * synth.normals(seed, stream + 2, N * n * n).reshape(N, n, n) / np.sqrt(n)
        L[0] = np.nan                                  # the never-read corner slots
        R[N - 1] = np.nan
    return synth.pack_bt(L, D, R)


def _gen(n, N, seed, batch, dtype, delta, mirrored):
    d = synth.gen_numpy(n, N, seed=seed, batch=batch, dtype=np.float64)
    S = np.stack([_perturb(n, N, d["S"][b], seed + b, 10, delta, mirrored) for b in range(batch)])
    P = np.stack([_perturb(n, N, d["Pinv"][b], seed + b, 20, delta, mirrored) for b in range(batch)])
    return dict(n=n, N=N, batch=batch, S=S.astype(dtype), Pinv=P.astype(dtype), gamma=d["gamma"].astype(dtype))


def gen_general(n, N, seed=1, batch=1, dtype=np.float64, delta=DELTA):
    """synth.gen_numpy with an independent perturbation on every block a kernel reads, in S and in Pinv: D_k += delta (K - K^T),
    L_k (k >= 1) and R_k (k < N-1) += delta normal / sqrt(n); L_0 and R_{N-1} are NaN.  Built in fp64, cast last.  Pinv is
    just a second non-symmetric block-tridiagonal matrix: at a fixed iteration count the solve is arithmetic, not a method."""
    return _gen(n, N, seed, batch, dtype, delta, False)


def gen_mirrored(n, N, seed=1, batch=1, dtype=np.float64, delta=DELTA):
    """D_k += delta (K - K^T) only, L_{k+1} = R_k^T bit for bit, in S and in Pinv: storage that passes the device symmetry test
    (modes 1 and 2 take the symmetric kernels) while no D block is symmetric."""
    return _gen(n, N, seed, batch, dtype, delta, True)


# ------------------------------------------------------------------------------------- mistakes in READING the storage
def _no_nan(M):
    return np.nan_to_num(np.asarray(M, np.float64), nan=0.0)   # corners: a mutant may move them into a slot that is read


def mutant_blocks(n, N, M, which):
    """Blocks (L, D, R) of one problem as a kernel with the index mistake `which` would read them."""
    L, D, R = (np.array(b) for b in synth.unpack_bt(n, N, _no_nan(M)))
    T = lambda X: np.swapaxes(X, -1, -2)   # noqa: E731
    if which == "D->D^T":
        D = T(D)
    elif which == "L<-R^T":
        L[1:] = T(R[:-1])
    elif which == "R<-L^T":
        R[:-1] = T(L[1:])
    elif which == "L<->R":
        L, R = R, L
    else:
        raise ValueError(which)
    return L, D, R


MUTANTS = ("D->D^T", "L<-R^T", "R<-L^T", "L<->R")


# ------------------------------------------------------------------------------- the fixed-count solve cases, both files
f32, f64 = np.float32, np.float64
# (family, n, N, B, dtype, generator, symmetric mode); family names the dispatch the GPU test forces and asserts
_GENERAL = (
    [("resident", n, N, B, dt, "general", 0) for (n, N, B) in ((3, 19, 2), (7, 20, 3), (13, 18, 2), (14, 40, 3)) for dt in (f32, f64)]
    + [("cluster", n, N, B, f32, "general", 0) for (n, N, B) in ((14, 100, 3), (14, 217, 2), (14, 500, 1), (12, 161, 3), (16, 33, 1),
                                                                  (18, 56, 2), (14, 150, 100))]
    + [("cluster", n, N, B, f64, "general", 0) for (n, N, B) in ((14, 65, 2), (13, 128, 2), (16, 40, 1))]
    + [("stream", n, N, B, dt, "general", 0) for (n, N, B) in ((20, 9, 2), (24, 7, 1), (37, 6, 2), (48, 5, 1)) for dt in (f32, f64)]
    + [("split", n, N, B, dt, "general", 0) for (n, N, B) in ((5, 9, 4), (14, 64, 1), (36, 21, 2)) for dt in (f32, f64)]
    + [(fam, n, N, B, dt, "general", 0) for fam in ("persist", "persist1r")
       for (n, N, B, dt) in ((36, 37, 1, f64), (36, 2, 1, f64), (14, 200, 1, f32), (24, 33, 3, f32))]
)
_MIRRORED = (
    [("sym", 14, N, B, f32, "mirrored", mode) for (N, B) in ((128, 5), (127, 3), (73, 2), (2, 3), (1, 2)) for mode in (1, 2)]
    + [("sym", n, N, B, dt, "mirrored", mode) for (n, N, B, dt) in ((14, 20, 300, f32), (12, 40, 260, f64)) for mode in (1, 2)]
)
SOLVE_ROWS = _GENERAL + _MIRRORED
# interleaved batches of mode 2 (even problems mirrored, odd problems general) and the shared pairs
MIXED_ROWS = [("mixed", 14, 128, 6, f32, "mixed", 2), ("mixed", 14, 100, 6, f32, "mixed", 2)]
SHARED_ROWS = [("shared", 14, 100, 5, f32, "general", 2), ("shared", 14, 128, 5, f32, "mirrored", 2)]
BASE = 4   # distinct systems of a batch; problem b repeats system b % BASE with gamma and lambda_0 scaled by 1 + (b // BASE) / 100


def row_id(row):
    fam, n, N, B, dt, gen, mode = row
    return f"{fam}-{n}x{N}x{B}-{np.dtype(dt).name}-{gen}-m{mode}"


def row_key(row):
    """What decides a row's inputs: the symmetric mode and the forced path do not."""
    fam, n, N, B, dt, gen, mode = row
    return (n, N, B, np.dtype(dt).name, gen, fam == "shared")


def row_case(row):
    """Inputs of a row: dict with S, Pinv [B, 3n^2N], gamma, lam0 [B, nN] in the row's dtype and `base`, the number of distinct
    systems.  A batch beyond BASE problems repeats them with gamma and the warm start scaled together, so every problem of the
    batch is a scaled copy of one the CPU conditions were checked on.  A shared row is ONE pair of matrices (every problem
    holds a copy of it) with B different right-hand sides and warm starts."""
    fam, n, N, B, dt, gen, mode = row
    shared = fam == "shared"
    base = B if shared else min(B, BASE)
    seed = 1000 + 37 * n + N
    delta = DELTA
    if gen == "mixed":
        dm, dg = gen_mirrored(n, N, seed, base, dt, delta), gen_general(n, N, seed, base, dt, delta)
        d = {k: np.where((np.arange(base) % 2 == 0)[:, None], dm[k], dg[k]) for k in ("S", "Pinv", "gamma")}
    else:
        d = (gen_mirrored if gen == "mirrored" else gen_general)(n, N, seed, base, dt, delta)
    if shared:
        d["S"], d["Pinv"] = np.repeat(d["S"][:1], base, axis=0), np.repeat(d["Pinv"][:1], base, axis=0)
    lam0 = np.stack([0.1 * synth.normals(seed + b, 30, n * N) for b in range(base)]).astype(dt)
    idx = np.arange(B) % base
    scale = (1.0 + 0.01 * (np.arange(B) // base))[:, None]
    return dict(n=n, N=N, batch=B, base=base, S=np.ascontiguousarray(d["S"][idx]), Pinv=np.ascontiguousarray(d["Pinv"][idx]),
                gamma=(d["gamma"][idx] * scale).astype(dt), lam0=(lam0[idx] * scale).astype(dt))


def oracle_variants(orc, c, k=K_FIXED, problems=None):
    """The oracle's four summation orders (FMA on / off x tree / sequential reduce) on problems [0, problems) of a case:
    list of dicts as orc.pcg_batch returns them, index = flags."""
    m = c["batch"] if problems is None else problems
    return [orc.pcg_batch(c["n"], c["N"], m, c["S"][:m], c["Pinv"][:m], c["gamma"][:m], lambda0=c["lam0"][:m], tol=0.0,
                          max_iter=k, flags=f) for f in range(4)]


def fixed_reference(c, b, k=K_FIXED):
    """pcg_fixed of problem b of a case on dense() of its storage."""
    n, N = c["n"], c["N"]
    return pcg_fixed(dense(n, N, c["S"][b]), dense(n, N, c["Pinv"][b]), c["gamma"][b], c["lam0"][b], k)


# ------------------------------------------------------------------------------------------------ stair formation input
def gen_stair_general(n, N, seed=1, batch=1, dtype=np.float64, every=1):
    """S for the stair formation with INDEPENDENT left and right blocks: D is the generator's symmetric positive definite D
    (formation mirrors the upper triangle of D^-1 by design), L_{k+1} = R_k^T + 0.3 normal / sqrt(n) on every block of every
    `every`-th problem counted from problem `every - 1` (every = 2: even problems keep symmetric storage).  Returns the cast S
    [batch, 3n^2N] and the fp64 stair blocks of that cast S as [batch, N, 3, n, n] row/column-indexed (L', D', R')."""
    d = synth.gen_numpy(n, N, seed=seed, batch=batch, dtype=np.float64)
    L, D, R = (np.array(b) for b in synth.unpack_bt(n, N, d["S"]))
    for b in range(every - 1, batch, every):
        L[b, 1:] += DELTA * synth.normals(seed + b, 40, (N - 1) * n * n).reshape(N - 1, n, n) / np.sqrt(n)
    S = synth.pack_bt(L, D, R).astype(dtype)
    Lq, Dq, Rq = (np.array(b, dtype=np.float64) for b in synth.unpack_bt(n, N, S))
    want = np.stack(synth.stair_pinv_blocks(Lq, Dq, Rq), axis=2)
    return S, want, d["gamma"].astype(dtype)
