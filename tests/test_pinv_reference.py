"""CPU half of tests/test_gpu_pinv_dispatch.py: the reference of tests/pinv_ref.py against the product-side host formula and
against exact rationals, the conditioning of the inputs, the yardstick against the project's tolerance, and the case table against
a restatement of launch_form_pinv's conditions."""
import json
import os

import numpy as np
import pytest

import pinv_ref as pr
from gbd_pcg_amd import synth

F32, F64 = pr.F32, pr.F64

# every kernel template of csrc/pinv.hip, pinv_regs.hip and pinv_fused.hip, written here (not read from the binary or from pinv_ref.py)
KERNEL_TEMPLATES = ["pinv_diag_kernel", "pinv_stair_kernel", "pinv_diag_reg_kernel", "pinv_diag_pair_kernel", "pinv_diag_quad_kernel",
                    "pinv_diag_wide_kernel", "pinv_stair_reg_kernel", "pinv_stair_fused_kernel", "pinv_stair_mfma_kernel",
                    "pinv_stair_wide_kernel"]
# the instantiations of the two any-size templates the three tiers of launch_form_pinv use
TIER_INSTANCES = ["pinv_diag_kernel<64,16>", "pinv_diag_kernel<256,16>", "pinv_diag_kernel<256,64>", "pinv_stair_kernel<64>",
                  "pinv_stair_kernel<256>"]


def rel(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / np.abs(np.asarray(b, F64)).max())


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("n,N,B", [(3, 3, 2), (14, 9, 3), (36, 4, 2)])
def test_reference_agrees_with_the_host_formula(n, N, B, perturbed):
    c = pr.Case(pr.QUAD, F64, n, N, B, pr.STAIR, perturbed, 0, ())
    S = pr.make_S(c)
    L, D, R = (np.array(x, dtype=F64) for x in synth.unpack_bt(n, N, S))
    want = synth.pack_bt(*synth.stair_pinv_blocks(L, D, R)).reshape(B, N, 3, n * n)
    mask = pr.corner_mask(B, N)
    for ref in (pr.reference(n, N, S, pr.STAIR), pr.reference_ld(n, N, S, pr.STAIR)):
        assert rel(ref[mask], want[mask]) < 1e-12
        assert not ref[~mask].any()
    if perturbed:   # the generator did make the storage non-symmetric, in every problem but the first
        Lq, _, Rq = pr.unpack(n, N, S)
        sym = [np.array_equal(Lq[b, 1:], np.swapaxes(Rq[b, :-1], -1, -2)) for b in range(B)]
        assert sym == [b not in pr.perturbed_problems(c) for b in range(B)]
    jac = pr.reference(n, N, S, pr.JACOBI)
    assert np.array_equal(jac[:, :, 1], pr.reference(n, N, S, pr.STAIR)[:, :, 1]) and not jac[:, :, (0, 2)].any()
    ident = pr.reference(n, N, S, pr.IDENTITY)
    assert np.array_equal(ident[0, 0, 1].reshape(n, n), np.eye(n)) and not ident[:, :, (0, 2)].any()


@pytest.mark.parametrize("perturbed", [False, True])
def test_reference_against_exact_rationals(perturbed):
    """n = 3, N = 3: the fp64 reference to a few units in the last place of fp64, the longdouble one to the rounding of the
    comparison itself."""
    n, N = 3, 3
    for dtype in (F32, F64):
        c = pr.Case(pr.QUAD, dtype, n, N, 2, pr.STAIR, perturbed, 0, ())
        S = pr.make_S(c)
        for b in range(2):
            exact = pr.reference_exact(n, N, S[b:b + 1])
            e64 = rel(pr.reference(n, N, S, pr.STAIR)[b], exact)
            eld = rel(pr.reference_ld(n, N, S, pr.STAIR)[b], exact)
            print(f"{np.dtype(dtype).name} problem {b}: fp64 reference {e64:.2e}, longdouble reference {eld:.2e} off the exact stair")
            assert e64 < 32 * np.finfo(F64).eps and eld <= np.finfo(F64).eps


def test_table_inputs_are_well_conditioned_and_the_yardstick_meets_the_tolerance():
    """Every D block of every case has condition number <= 100 after rounding to fp32 (else the project's tolerance means
    nothing), and up to n = 36 the same-precision numpy evaluation is within TOL[dtype] per block: the reference alone
    satisfies the bound."""
    worst_cond, worst = 0.0, {F32: 0.0, F64: 0.0}
    for c in pr.CASES:
        d = pr.case_data(c)
        worst_cond = max(worst_cond, d.cond)
        assert d.cond <= 100, (pr.case_id(c), d.cond)
        assert np.isfinite(d.e_np).all()
        if c.n <= 36:
            worst[c.dtype] = max(worst[c.dtype], float(d.e_np[d.mask].max()))
            assert d.e_np[d.mask].max() <= pr.TOL[c.dtype], (pr.case_id(c), d.e_np[d.mask].max())
    print(f"largest condition number of a D block: {worst_cond:.1f}; largest e_np up to n = 36: fp32 {worst[F32]:.2e}, "
          f"fp64 {worst[F64]:.2e}")


def test_table_names_every_kernel_template():
    named = {k for c in pr.CASES for k in c.family}
    for t in KERNEL_TEMPLATES:
        assert any(k == t or k.startswith(t + "<") for k in named), t
    for t in TIER_INSTANCES:
        assert t in named, t
    for k in named:
        assert k.split("<")[0] in KERNEL_TEMPLATES, k


def test_every_case_takes_the_route_the_table_claims():
    for c in pr.CASES:
        want = c.family if c.kind == pr.STAIR else c.family[:1]
        assert pr.route(c.dtype, c.n, c.N, c.kind, c.s_off == 0, c.env) == want, pr.case_id(c)
        assert c.N <= 33 and (c.n <= 36 or (c.N <= 5 and c.B <= 2)), pr.case_id(c)
        assert tuple(c.env) in ((),) + pr.SWITCH_SETS
    # what the alignment runs of the GPU half rely on: only fp32 n = 16 looks at the address of S
    for dt in (F32, F64):
        for n in range(1, 92):
            for kind in (0, 1, 2):
                for N in (1, 2):
                    differs = pr.route(dt, n, N, kind, True) != pr.route(dt, n, N, kind, False)
                    assert differs == (dt == F32 and n == 16 and kind == 2 and N >= 2)
    # the refusals, from the code: 2 n^2 > 16384 in fp32, four n x n factors over 160 KiB of LDS in fp64
    for dt in (F32, F64):
        assert pr.route(dt, pr.FIRST_REFUSED[dt], 2, pr.STAIR) == pr.REFUSED
        assert pr.route(dt, pr.LARGEST[dt], 2, pr.STAIR) == pr.G256L and pr.LARGEST[dt] + 1 == pr.FIRST_REFUSED[dt]


def test_route_agrees_with_the_table_recorded_before_the_rewrite():
    """tests/golden/pinv_routes.json: what route() returned for every (dtype, n <= 91, N in {1, 2}, kind, S aligned) when it still
    restated the launcher's macro bodies, before it and the launcher were rewritten around one pinv_route: kernel names only."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pinv_routes.json")) as fh:
        recorded = json.load(fh)
    seen = 0
    for dt in (F32, F64):
        for n in range(1, 92):
            for N in (1, 2):
                for kind in (0, 1, 2):
                    for aligned in (True, False):
                        key = "%s,%d,%d,%d,%d" % (np.dtype(dt).name, n, N, kind, aligned)
                        assert "+".join(pr.route(dt, n, N, kind, aligned)) == recorded[key], key
                        seen += 1
    assert seen == len(recorded)
    # every family name of the route is one of the documented ones, and each names kernels of the template list
    for family, names in pr.FAMILY_KERNELS.items():
        assert family == "refused" or all(k.split("<")[0] in KERNEL_TEMPLATES for k in names), family


def test_cases_are_unique():
    assert len(set(pr.CASES)) == len(pr.CASES)
