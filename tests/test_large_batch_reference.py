"""The arithmetic of tests/large_batch_ref.py, on the CPU: every case of tests/test_gpu_large_batch.py crosses the boundaries it
names, its sample holds the problems that straddle them, its fills stay below 2^30 elements, and it fits the memory cap."""
import numpy as np
import pytest

import large_batch_ref as lb


def test_boundaries_by_element_size():
    assert [off for _, off in lb.boundaries(4)] == [1 << 29, 1 << 30, 1 << 31, 1 << 32]
    assert [off for _, off in lb.boundaries(8)] == [1 << 28, 1 << 29, 1 << 30, 1 << 31, 1 << 32]
    assert [off for _, off in lb.boundaries(1)] == [1 << 31, 1 << 32, 1 << 33, 1 << 34]
    assert dict((off, n) for n, off in lb.boundaries(4))[1 << 31] == "2^33 bytes = 2^31 elements"
    assert dict((off, n) for n, off in lb.boundaries(8))[1 << 31] == "2^34 bytes = 2^31 elements"


@pytest.mark.parametrize("stride,es,B", [(75264, 4, 57100), (75264, 8, 28600), (995328, 8, 2160), (2681, 8, 200400), (1, 4, 100), (5, 4, 3),
                                         (1 << 20, 4, 5000), (3, 8, (1 << 32) // 3 + 50)])
def test_boundary_problems(stride, es, B):
    s = lb.boundary_problems(stride, es, B)
    assert s == sorted(set(s)) and all(0 <= b < B for b in s)
    assert set(range(min(lb.K, B))) <= set(s) and set(range(max(B - lb.K, 0), B)) <= set(s)
    crossed = lb.crossed(stride, es, B)
    for name, off in lb.boundaries(es):
        is_crossed = B * stride > off
        assert ((name, off) in crossed) == is_crossed
        if not is_crossed:
            continue
        p = off // stride                       # the problem the boundary's element lies in
        assert p * stride <= off < (p + 1) * stride
        for q in (p - 1, p, p + 1):
            assert q in s or not 0 <= q < B
        first = lb.first_behind(stride, es, B)[name]
        assert first * stride >= off > (first - 1) * stride
        assert name in lb.behind(B - 1, stride, es, B) or lb.behind(B - 1, stride, es, B) == crossed[-1][0]
    assert len(s) <= 2 * lb.K + 3 * len(crossed)
    assert lb.behind(0, stride, es, B) == "no boundary" or stride * es > 1 << 31


def test_boundary_problems_by_hand():
    # 10 problems of 2^29 fp32 elements (2 GiB each): boundaries at elements 2^29, 2^30, 2^31, 2^32 = problems 1, 2, 4, 8
    assert lb.boundary_problems(1 << 29, 4, 10) == list(range(10))
    assert lb.boundary_problems(1 << 29, 4, 40) == list(range(0, 10)) + list(range(33, 40))
    # nothing crossed: the two ends only
    assert lb.boundary_problems(100, 4, 30) == list(range(7)) + list(range(23, 30))
    assert lb.boundary_problems(100, 4, 5) == [0, 1, 2, 3, 4]
    assert lb.sample_union([(100, 4), (1 << 29, 4)], 40) == lb.boundary_problems(1 << 29, 4, 40)


@pytest.mark.parametrize("stride", [1, 3, 1792, 75264, 37632, 76800, 65712, 995328, 31311])
@pytest.mark.parametrize("boundary", [1 << 28, 1 << 31, 1 << 32, (1 << 32) + 1])
def test_min_batch(stride, boundary):
    B = lb.min_batch(stride, boundary)
    assert (B - lb.K) * stride >= boundary          # the last 7 problems lie wholly behind it
    assert (B - 1 - lb.K) * stride < boundary       # one problem fewer: they do not


def test_chunks_cover_the_batch_in_whole_periods():
    for stride, B, first in ((75264, 57100, 0), (75264, 57100, 7), (995328, 2160, 7), (1, 200400, 0), (2681, 200400, 7), (2, 10, 0)):
        ch = lb.chunks(stride, B, first)
        assert ch[0][0] == first and ch[-1][1] == B and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all((hi - lo) * stride < 1 << 30 for lo, hi in ch)
        assert all((hi - lo) % lb.K == 0 for lo, hi in ch[:-1]) and all((lo - first) % lb.K == 0 for lo, _ in ch)


def test_no_boundary_is_a_multiple_of_seven_strides():
    """... so an offset that wrapped at a boundary never lands on the twin of the problem it was meant for."""
    for c in lb.CASES:
        for stride, es in c.arrays.values():
            for _, off in lb.boundaries(es):
                assert off % (lb.K * stride) != 0 or stride == 1, (c.name, stride)


@pytest.mark.parametrize("c", lb.CASES, ids=[c.name for c in lb.CASES])
def test_case_crosses_what_it_claims_and_fits(c):
    for name, want in c.claims.items():
        stride, es = c.arrays[name]
        got = [n for n, _ in lb.crossed(stride, es, c.B)]
        assert got == want, (c.name, name, got)
        for n, off in lb.crossed(stride, es, c.B):
            assert c.B * stride > off and c.B * stride * es > off * es
    assert lb.planned_bytes(c) <= lb.CAP_BYTES, (c.name, lb.planned_bytes(c))


def test_the_tables_of_the_issue():
    """The arithmetic behind each row, spelled out."""
    for c in lb.SOLVE_CASES:
        stride, es = c.arrays["S"]
        assert c.B * stride * es > 1 << 34, c.name                             # every byte boundary
        assert c.B * stride > (1 << 32 if es == 4 else 1 << 31), c.name        # fp32: 2^32 elements; fp64: 2^31 elements
        assert 17.1e9 < c.B * stride * es < 17.4e9                             # "each matrix is 17.2 GB"
        # the last problems lie wholly behind the top boundary: 7 of them everywhere but at (36, 256) fp64, where B = 2160 leaves 2
        top = 1 << 32 if es == 4 else 1 << 31
        whole = c.B - -(-top // stride)
        assert whole >= (2 if c.name == "auto-36x256-f64" else lb.K), (c.name, whole)
        assert (c.B >= lb.min_batch(stride, top)) == (c.name != "auto-36x256-f64")
    z = lb.kkt_sizes(14, 7, 128)
    assert (z["G"], z["C"], z["g"], z["c"], z["S"]) == (31311, 37338, 2681, 1792, 75264)
    B = 57100
    assert B * z["S"] > 1 << 32
    # G, G^-1 (7.2 GB) and C (8.5 GB) pass 2^32 bytes; 2^31 ELEMENTS would be 8.59 GB in fp32, which neither reaches
    assert 1 << 32 < 4 * B * z["G"] < 1 << 33 and 1 << 32 < 4 * B * z["C"] < 1 << 33
    assert B * z["G"] < 1 << 31 and B * z["C"] < 1 << 31
    assert 1 << 32 < 8 * 28600 * z["G"] < 1 << 33 and 1 << 32 < 8 * 28600 * z["C"] < 1 << 33
    assert 8 * 200400 * z["g"] > 1 << 32 and 7 * 8 * 200400 * z["g"] < 31e9
    assert lb.DEMOTE_COUNT > 1 << 31 and 8 * lb.DEMOTE_COUNT > 1 << 34 and 4 * lb.DEMOTE_COUNT > 1 << 33


def test_unsymmetrize_one_moves_one_entry_by_one_ulp():
    n, N = 14, 128
    M = np.random.default_rng(0).standard_normal(3 * n * n * N).astype(np.float32)
    U = lb.unsymmetrize_one(M, n, N)
    diff = np.flatnonzero(U != M)
    assert len(diff) == 1 and U[diff[0]] == np.nextafter(M[diff[0]], np.float32(np.inf))
    k, slot = divmod(diff[0], 3 * n * n)
    assert 1 <= k < N and slot < n * n            # an L block that is read
