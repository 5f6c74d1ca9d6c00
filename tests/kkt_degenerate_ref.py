"""Batches with exactly zero right-hand sides at the KKT level (not a test module): the constructions tests/test_gpu_kkt_degenerate.py
runs on the device and tests/test_kkt_degenerate_reference.py checks on the host.

Every batch has B = 5 problems.  Problems 1 and 3 are degenerate: their gamma = -(c + C G^-1 g) is EXACTLY zero, so a solve that starts
from lambda = 0 starts from a zero residual.  Problems 0, 2 and 4 are regular data of oracle/schur_oracle.py::gen, fp32 numbers held
in fp64 (one array serves both precisions).  The `twin` of a batch is the same batch with regular vectors g, c in problems 1 and 3
as well (same matrices): what the regular problems' outputs are compared with bit for bit.

kinds
  a  g = 0 and c = 0 (a regulator at its set-point): every product of the formation has a zero factor.
  b  c = 0 and g != 0 with gamma == 0 all the same.  Problems 1 and 3 get matrices on which every product is exact: Q_k, R_k
     diagonal with entries 1/4, 1, 4 (their square roots, inverses and every multiple are exact), A_k a signed permutation, B_k
     with entries 0, +-1.  With t_k = Q_k^-1 q_k the rows of gamma read  gamma_0 = -t_0,  gamma_k = -(t_k - A_j t_j - B_j s_j),
     s_j = R_j^-1 r_j, j = k - 1: so t_0 = 0, s_j a vector of +-1, t_k = A_j t_j + B_j s_j, q_k = Q_k t_k, r_j = R_j s_j.
     |t_k|_inf <= k nu: small integers, sums of them exact in any order and with or without fused multiply-adds, in fp32 as in fp64.
     There is no such problem at N = 1: gamma_0 = -Q_0^-1 q_0 is zero only for q_0 = 0 = g.  KINDS[shape] leaves it out there.
  c  a warm start: the factorisation stands (a regular step ran on the twin), the regular problems start from that step's
     multipliers with new g, c, and problems 1 and 3 start from lambda = 0 with g = c = 0 -- a start that solves their system
     exactly.  The vectors are those of kind a; what differs is lambda_0 of the neighbours, which the device test supplies.
"""
import functools

import numpy as np

from oracle import schur_oracle as so

F32, F64 = np.float32, np.float64
B = 5
DEGENERATE, REGULAR = (1, 3), (0, 2, 4)
SHAPES = [(14, 7, 24), (5, 3, 10), (2, 1, 3), (3, 2, 1)]     # a quad-list shape, an any-size shape, the smallest, N = 1 (no C)
KINDS = {s: ("a", "c") if s[2] == 1 else ("a", "b", "c") for s in SHAPES}


def exact_matrices(nx, nu, N, rng):
    """One problem's packed G and C on which the formation is exact (kind b)."""
    G, C = [], []
    for k in range(N):
        G.append(np.diag(4.0 ** rng.integers(-1, 2, nx)).T.reshape(-1))
        if k < N - 1:
            G.append(np.diag(4.0 ** rng.integers(-1, 2, nu)).T.reshape(-1))
            A = np.zeros((nx, nx))
            A[np.arange(nx), rng.permutation(nx)] = rng.choice([-1.0, 1.0], nx)
            Bk = rng.integers(-1, 2, (nx, nu)).astype(F64)
            C += [A.T.reshape(-1), Bk.T.reshape(-1)]
    return np.concatenate(G), (np.concatenate(C) if C else np.zeros(0))


def zero_gamma_g(nx, nu, N, G, C, rng):
    """g != 0 with gamma == 0 at c = 0 on exact_matrices (the recursion of the module docstring)."""
    Q, R, A, Bm, _, _, _ = so.unpack(nx, nu, N, G, C, np.zeros((nx + nu) * N - nu), np.zeros(nx * N))
    t, g = np.zeros(nx), []
    for k in range(N):
        g.append(Q[k] @ t)
        if k < N - 1:
            s = rng.choice([-1.0, 1.0], nu)
            g.append(R[k] @ s)
            t = A[k] @ t + Bm[k] @ s
    return np.concatenate(g)


def gamma_formula(nx, nu, N, G, C, g, c, dtype):
    """gamma = -(c + C G^-1 g) by the block formulas of oracle/schur_oracle.py, every operation in `dtype`."""
    Q, R, A, Bm, q, r, cc = (([m.astype(dtype) for m in part]) for part in so.unpack(nx, nu, N, G, C, g, c))
    Qi = [np.linalg.inv(m).astype(dtype) for m in Q]
    Ri = [np.linalg.inv(m).astype(dtype) for m in R]
    out = []
    for k in range(N):
        v = cc[k] + Qi[k] @ q[k]
        if k > 0:
            j = k - 1
            v = v - (A[j] @ (Qi[j] @ q[j]) + Bm[j] @ (Ri[j] @ r[j]))
        assert v.dtype == np.dtype(dtype)
        out.append(-v)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def batch(nx, nu, N, kind, seed=0):
    """(d, twin): dicts of G, C, g, c as [B, size] fp64 arrays holding fp32 numbers, read-only.  d is the degenerate batch."""
    assert kind in KINDS[(nx, nu, N)]
    base = 900 + 10 * (nx + N) + seed
    twin = {k: v.astype(F64) for k, v in so.gen(nx, nu, N, seed=base, batch=B, dtype=F32).items()}
    rng = np.random.default_rng(base + 1)
    if kind == "b":
        for b in DEGENERATE:
            twin["G"][b], twin["C"][b] = exact_matrices(nx, nu, N, rng)
    d = {k: v.copy() for k, v in twin.items()}
    for b in DEGENERATE:
        d["c"][b] = 0.0
        d["g"][b] = zero_gamma_g(nx, nu, N, d["G"][b], d["C"][b], rng) if kind == "b" else 0.0
    for a in list(d.values()) + list(twin.values()):
        assert np.array_equal(a, a.astype(F32).astype(F64))
        a.setflags(write=False)
    return d, twin


@functools.lru_cache(maxsize=None)
def new_vectors(nx, nu, N, seed=0):
    """(g, c) of another draw, [B, size] each: the new gradients and residuals of a frozen-linearisation tick."""
    d = so.gen(nx, nu, N, seed=950 + 10 * (nx + N) + seed, batch=B, dtype=F32)
    g, c = d["g"].astype(F64), d["c"].astype(F64)
    g.setflags(write=False)
    c.setflags(write=False)
    return g, c


def add_rho(nx, nu, N, G, rho):
    """One problem's packed G with rho on the diagonal of every block."""
    G = np.array(G, F64)
    sg = nx * nx + nu * nu
    for k in range(N):
        G[k * sg:k * sg + nx * nx:nx + 1] += rho
        if k < N - 1:
            G[k * sg + nx * nx:(k + 1) * sg:nu + 1] += rho
    return G


def expected_masks():
    """(degenerate [B] bool, regular [B] bool)."""
    deg = np.zeros(B, bool)
    deg[list(DEGENERATE)] = True
    return deg, ~deg
