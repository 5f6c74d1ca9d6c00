"""CPU-only checks of the entry points of the optimality test (gbdpcg_admm_optimality_*, gbdpcg_admm_lin_optimality_* and their
_shared twins), after tests/test_admm_infeas_abi.py: declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built
library, their argument lists related to gbdpcg_admm_lin_update_* and to each other as the header states, refusing a null handle
and a NULL in every required slot before anything is looked at or written, reachable through binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_optimality", "admm_optimality_shared", "admm_lin_optimality", "admm_lin_optimality_shared")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def declaration(name):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def key(arg):
    return arg.split()[-1].lstrip("*")


def test_new_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", hdr))
    assert len(set(NEW)) == 8
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name
    # not provided: a count over the batch, a dual-infeasibility test
    assert not any("optimality" in n and ("count" in n or "dual" in n) for n in declared)


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("shared", ["", "_shared"])
def test_rows_argument_list_follows_the_lin_update(shared, suf):
    """The sizes of gbdpcg_admm_lin_update_*, then the matrices and vectors (d_G, d_C, d_g, d_c, d_E) with its d_g and d_E among them,
    then its d_rho, the point (its d_z, d_w, d_y with d_lambda behind d_z), the tolerances, the outputs, the stream."""
    ty = "float" if suf == "f32" else "double"
    a, u = declaration(f"gbdpcg_admm_lin_optimality{shared}_{suf}"), declaration(f"gbdpcg_admm_lin_update_{suf}")
    uk = [key(x) for x in u]
    ig = uk.index("d_g")
    assert uk[:ig] == ["h", "nx", "nu", "mx", "mu", "N", "batch"]
    byname = dict(zip(uk, u))
    want = (u[:ig] + [f"const {ty} *d_G", f"const {ty} *d_C", byname["d_g"], f"const {ty} *d_c", byname["d_E"], byname["d_rho"],
                      byname["d_z"], f"const {ty} *d_lambda", f"const {ty} *d_w", f"const {ty} *d_y", f"{ty} eps_abs", f"{ty} eps_rel",
                      f"{ty} *d_opt", "uint8_t *d_done", "void *stream"])
    assert a == want
    # the point is read only: the update's d_w, d_y are its outputs, here they are const
    assert byname["d_w"] == f"{ty} *d_w" and byname["d_y"] == f"{ty} *d_y"


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("shared", ["", "_shared"])
def test_box_argument_list_is_the_rows_one_without_mx_mu_and_E(shared, suf):
    rows = declaration(f"gbdpcg_admm_lin_optimality{shared}_{suf}")
    box = declaration(f"gbdpcg_admm_optimality{shared}_{suf}")
    assert box == [x for x in rows if key(x) not in ("mx", "mu", "d_E")]
    assert declaration(f"gbdpcg_admm_lin_optimality_{suf}") == declaration(f"gbdpcg_admm_lin_optimality_shared_{suf}")


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_order_follows_the_infeasibility_calls(suf):
    """sizes, then matrices and vectors, then d_rho, the point, the tolerances, two outputs, stream -- as gbdpcg_admm_lin_infeas_*."""
    a = [key(x) for x in declaration(f"gbdpcg_admm_lin_optimality_{suf}")]
    i = [key(x) for x in declaration(f"gbdpcg_admm_lin_infeas_{suf}")]
    assert a[:a.index("batch") + 1] == i[:i.index("batch") + 1]
    assert a.index("d_E") < a.index("d_rho") < a.index("d_z") < a.index("eps_abs") < a.index("d_opt") < a.index("stream")
    assert i.index("d_E") < i.index("d_rho") < i.index("d_lambda0") < i.index("eps") < i.index("d_cert") < i.index("stream")
    assert a[-3:] == ["d_opt", "d_done", "stream"] and i[-3:] == ["d_cert", "d_flag", "stream"]


@pytest.mark.parametrize("name", NEW)
def test_argtypes_match_the_declaration(lib, name):
    args = declaration(name)
    at = getattr(lib, name).argtypes
    assert at is not None and len(at) == len(args), name
    for a, t in zip(args, at):
        if "*" in a or a.startswith("gbdpcg_handle_t"):
            assert t is ctypes.c_void_p, (name, a)
        elif a.startswith("uint32_t"):
            assert t is ctypes.c_uint32, (name, a)
        else:
            assert key(a) in ("eps_abs", "eps_rel") and t is (ctypes.c_float if name.endswith("f32") else ctypes.c_double), (name, a)


@pytest.mark.parametrize("name", NEW)
def test_null_handle_and_null_pointers_are_invalid(lib, name):
    """No call here reaches a device: a null handle is refused first, alone and with a NULL in any one slot (d_done, which may be
    NULL, included), and the words passed for d_opt and d_done keep what they held."""
    args = declaration(name)
    words = {key(a): (ctypes.c_double * 6)(*[7.0] * 6) for a in args if "*" in a}

    def value(a, null):
        if "*" in a:
            return None if key(a) == null else ctypes.cast(words[key(a)], ctypes.c_void_p)
        return 2 if a.startswith("uint32_t") else 0.1
    for null in [None] + [key(a) for a in args[1:] if "*" in a]:
        assert getattr(lib, name)(None, *[value(a, null) for a in args[1:]]) == 1, null      # GBDPCG_ERR_INVALID
    assert all(list(w) == [7.0] * 6 for w in words.values())


def test_reachable_from_python():
    for m in NAMES:
        assert callable(getattr(binding.Solver, m)), m
