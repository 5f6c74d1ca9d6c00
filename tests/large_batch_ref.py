"""Arithmetic of the large-batch tests (tests/test_gpu_large_batch.py): which offsets a batch crosses, which problems to look at,
how much device memory a case holds.  Pure Python and numpy, no device.

A batch is problem-major: problem b of an array with `stride` elements per problem starts at element b * stride, byte
b * stride * elem_size.  The offsets at which 32-bit arithmetic goes wrong -- the BOUNDARIES -- are the byte offsets 2^31, 2^32,
2^33, 2^34 and the element offsets 2^31, 2^32.  An array CROSSES a boundary when it ends behind it.

The batches are 7-periodic (problem b is base problem b mod 7).  7 is odd and every boundary is a power of two, so no boundary is
a multiple of 7 strides of any array used here (checked by tests/test_large_batch_reference.py): an offset that wrapped at a
boundary lands in a problem of another residue, never on the twin of the problem it was meant for.
"""
from collections import namedtuple

import numpy as np

K = 7                                      # base problems; problem b of a batch is base problem b % K
BYTE_BOUNDARIES = tuple(1 << s for s in (31, 32, 33, 34))
ELEM_BOUNDARIES = tuple(1 << s for s in (31, 32))
CAP_BYTES = 48 * 10 ** 9                   # no case holds more device memory than this
TAIL = 4096                                # sentinel elements behind every output
CHUNK_ELEMS = (1 << 30) - 1                # fills and comparisons touch fewer than 2^30 elements per torch call
FINITE_ELEMS = 1 << 27                     # ... and the finiteness checks, whose temporaries are as large as their argument, 2^27
SCRATCH_BYTES = 2 * 10 ** 9                # room for those temporaries, the base problems and the sampled copies, in every plan


def boundaries(elem_size):
    """Every boundary as (name, element offset) for arrays of this element size, ascending, without duplicates by offset
    (in fp32 the byte offset 2^33 IS the element offset 2^31: both names are kept, joined)."""
    by_off = {}
    for b in BYTE_BOUNDARIES:
        by_off.setdefault(b // elem_size, []).append(f"2^{b.bit_length() - 1} bytes")
    for e in ELEM_BOUNDARIES:
        by_off.setdefault(e, []).append(f"2^{e.bit_length() - 1} elements")
    return [(" = ".join(names), off) for off, names in sorted(by_off.items())]


def crossed(stride_elems, elem_size, B):
    """The boundaries an array of B problems ends behind: [(name, element offset)]."""
    return [(name, off) for name, off in boundaries(elem_size) if B * stride_elems > off]


def boundary_problems(stride_elems, elem_size, B):
    """The problems worth a reference check, sorted: the first K, the last K, and for every boundary the array crosses the problem
    that contains it (the one the boundary's element lies in) with its two neighbours."""
    assert stride_elems > 0 and B > 0
    out = set(range(min(K, B))) | set(range(max(B - K, 0), B))
    for _, off in crossed(stride_elems, elem_size, B):
        p = off // stride_elems
        out |= {q for q in (p - 1, p, p + 1) if 0 <= q < B}
    return sorted(out)


def first_behind(stride_elems, elem_size, B):
    """{boundary name: first problem that lies wholly behind it} for the boundaries the array crosses."""
    return {name: -(-off // stride_elems) for name, off in crossed(stride_elems, elem_size, B)}


def min_batch(stride_elems, boundary_elems):
    """The smallest B whose array crosses the element offset `boundary_elems` by at least K whole problems."""
    return -(-boundary_elems // stride_elems) + K


def behind(b, stride_elems, elem_size, B):
    """For a failure message: the last boundary problem b lies (at least partly) behind, or 'no boundary'."""
    names = [name for name, off in crossed(stride_elems, elem_size, B) if (b + 1) * stride_elems > off]
    return names[-1] if names else "no boundary"


def chunks(stride_elems, B, first=0):
    """[first, B) in runs of whole groups of K problems, each run of fewer than 2^30 elements: [(lo, hi)], (hi - lo) % K == 0
    except in the last run."""
    per = max(CHUNK_ELEMS // (K * stride_elems), 1) * K
    assert per * stride_elems <= CHUNK_ELEMS, "one group of K problems is 2^30 elements or more"
    return [(lo, min(lo + per, B)) for lo in range(first, B, per)]


def sample_union(arrays, B):
    """boundary_problems over several arrays of one call: arrays = [(stride_elems, elem_size)]."""
    out = set()
    for stride, es in arrays:
        out |= set(boundary_problems(stride, es, B))
    return sorted(out)


# ---- the cases.  arrays: {name: (elements per problem, element size)} of everything the case holds on the device at once; claims:
# {array: names of boundaries it must cross}.  extra_bytes: device memory next to the arrays (the handle's workspace).
Case = namedtuple("Case", "name B arrays claims extra_bytes")


def bt(n, N):
    return 3 * n * n * N


def kkt_sizes(nx, nu, N):
    """Elements per problem of the packed KKT arrays (include/gbdpcg.h)."""
    return {"G": (nx * nx + nu * nu) * N - nu * nu, "C": (nx * nx + nx * nu) * (N - 1), "g": (nx + nu) * N - nu, "c": nx * N,
            "S": bt(nx, N), "gamma": nx * N}


ALL_F32 = ["2^31 bytes", "2^32 bytes", "2^33 bytes = 2^31 elements", "2^34 bytes = 2^32 elements"]
ALL_F64 = ["2^31 bytes", "2^32 bytes", "2^33 bytes", "2^34 bytes = 2^31 elements"]


def solve_case(name, n, N, es, B, split_ws_elems=0):
    """S, Pinv and the vectors of one solve: gamma, lambda, r, p, the warm start, and the reference copy of lambda, r, p the
    bit-for-bit comparisons keep (form_pinv_solve against the two calls)."""
    arrays = {"S": (bt(n, N), es), "Pinv": (bt(n, N), es)}
    for v in ("gamma", "lambda", "r", "p", "lambda0", "lambda_keep"):
        arrays[v] = (n * N, es)
    arrays["iters"], arrays["flags"] = (1, 4), (1, 1)
    every = ALL_F32 if es == 4 else ALL_F64
    return Case(name, B, arrays, {"S": every, "Pinv": every}, split_ws_elems * es * B)


# per problem, the split path keeps 6 vectors and 3 N partial sums (csrc/pcg_split.hip, SplitWs): the test takes the true figure from
# gbdpcg_workspace_bytes, this one is the room the memory plan leaves for it
SPLIT_WS_VECTORS = 12

SOLVE_CASES = [
    solve_case("resident_sym-14x128-f32", 14, 128, 4, 57100),
    solve_case("resident-14x64-f32", 14, 64, 4, 114200),
    solve_case("fused-20x64-f32", 20, 64, 4, 55950),
    solve_case("fused-runtime-37x16-f32", 37, 16, 4, 65400),
    solve_case("split-14x128-f32", 14, 128, 4, 57100, split_ws_elems=SPLIT_WS_VECTORS * 14 * 128),
    solve_case("cluster4-14x128-f64", 14, 128, 8, 28600),
    solve_case("auto-36x256-f64", 36, 256, 8, 2160, split_ws_elems=SPLIT_WS_VECTORS * 36 * 256),
]


def kkt_case(name, es, B, with_S):
    z = kkt_sizes(14, 7, 128)
    arrays = {"G": (z["G"], es), "C": (z["C"], es), "Ginv": (z["G"], es)}
    for v in ("g", "c", "z", "lambda", "gamma", "rg", "rc"):
        arrays[v] = (z["g"] if v in ("g", "z", "rg") else z["c"], es)
    arrays["res"] = (2, es)
    claims = {"G": ["2^31 bytes", "2^32 bytes"], "C": ["2^31 bytes", "2^32 bytes"], "Ginv": ["2^31 bytes", "2^32 bytes"]}
    if with_S:
        arrays["S"] = (z["S"], es)
        claims["S"] = ALL_F32
    else:
        del arrays["Ginv"], claims["Ginv"]
    return Case(name, B, arrays, claims, 0)


KKT_CASES = [kkt_case("kkt-14x7x128-f32", 4, 57100, True), kkt_case("kkt-14x7x128-f64", 8, 28600, False)]

NZ = kkt_sizes(14, 7, 128)["g"]
ADMM_CASE = Case("admm-14x7x128-f64", 200400, {k: (NZ, 8) for k in ("g", "lo", "hi", "z", "w", "y", "gt")},
                 {k: ["2^31 bytes", "2^32 bytes"] for k in ("g", "lo", "hi", "z", "w", "y", "gt")}, 0)
APPLY_CASE = Case("refine_apply-14x7x128", 200400, {"z": (NZ, 8), "z0": (NZ, 8), "lambda": (14 * 128, 8), "lambda0": (14 * 128, 8),
                                                      "dz": (NZ, 4), "dlambda": (14 * 128, 4)},
                  {"z": ["2^31 bytes", "2^32 bytes"], "z0": ["2^31 bytes", "2^32 bytes"]}, 0)
DEMOTE_COUNT = (1 << 31) + (1 << 30) + 12345
DEMOTE_CASE = Case("demote", 1, {"src": (DEMOTE_COUNT, 8), "dst": (DEMOTE_COUNT, 4)},
                   {"src": ALL_F64, "dst": ["2^31 bytes", "2^32 bytes", "2^33 bytes = 2^31 elements"]}, 0)

CASES = SOLVE_CASES + KKT_CASES + [ADMM_CASE, APPLY_CASE, DEMOTE_CASE]


def case(name):
    return next(c for c in CASES if c.name == name)


def case_bytes(c):
    """Device memory the case holds at once: the arrays, a sentinel tail behind each, the workspace."""
    return sum((stride * c.B + TAIL) * es for stride, es in c.arrays.values()) + c.extra_bytes


def planned_bytes(c):
    """... and with the room every plan leaves for temporaries: what the test asks mem_get_info for."""
    return case_bytes(c) + SCRATCH_BYTES


def unsymmetrize_one(M, n, N):
    """One problem's [L|D|R] storage with one L entry moved by one ulp (tests/test_gpu_cluster.py, unsymmetrize, b = 3): the
    storage fails the bit-for-bit symmetry test, the matrix hardly moves."""
    M = np.array(M).reshape(N, 3, n, n)
    k = 1 + (7 * 3) % (N - 1)
    M[k, 0, 3, 5] = np.nextafter(M[k, 0, 3, 5], M.dtype.type(np.inf))
    return M.reshape(-1)
