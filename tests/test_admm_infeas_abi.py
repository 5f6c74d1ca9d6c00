"""CPU-only checks of the entry points of the infeasibility certificate (gbdpcg_admm_infeas_*, gbdpcg_admm_lin_infeas_* and their
_shared twins), after tests/test_admm_lin_adjoint_abi.py: declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the
built library, their argument lists related to gbdpcg_admm_lin_update_* as the header states, refusing a null handle and a NULL in
every slot before anything is looked at or written, reachable through binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_infeas", "admm_infeas_shared", "admm_lin_infeas", "admm_lin_infeas_shared")
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
    # not provided: cone rows, the soft families, a count over the batch
    assert not any("infeas" in n and ("soc" in n or "soft" in n or "count" in n) for n in declared)


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("shared", ["", "_shared"])
def test_rows_argument_list_follows_the_lin_update(shared, suf):
    """The sizes and (d_E, d_lo, d_hi, d_rho) of gbdpcg_admm_lin_update_*, with (d_C, d_c) where its d_g stands and the two iterates,
    eps and the outputs where its state stands."""
    ty = "float" if suf == "f32" else "double"
    a, u = declaration(f"gbdpcg_admm_lin_infeas{shared}_{suf}"), declaration(f"gbdpcg_admm_lin_update_{suf}")
    ig, ie, ir = (([key(x) for x in u]).index(k) for k in ("d_g", "d_E", "d_rho"))
    assert ie == ig + 1 and [key(x) for x in u[ie:ir + 1]] == ["d_E", "d_lo", "d_hi", "d_rho"]
    want = (u[:ig] + [f"const {ty} *d_C", f"const {ty} *d_c"] + u[ie:ir + 1] +
            [f"const {ty} *d_lambda0", f"const {ty} *d_lambda1", f"const {ty} *d_y0", f"const {ty} *d_y1", f"{ty} eps",
             f"{ty} *d_cert", "uint8_t *d_flag", "void *stream"])
    assert a == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("shared", ["", "_shared"])
def test_box_argument_list_is_the_rows_one_without_mx_mu_and_E(shared, suf):
    rows = declaration(f"gbdpcg_admm_lin_infeas{shared}_{suf}")
    box = declaration(f"gbdpcg_admm_infeas{shared}_{suf}")
    assert box == [x for x in rows if key(x) not in ("mx", "mu", "d_E")]
    assert declaration(f"gbdpcg_admm_lin_infeas_{suf}") == declaration(f"gbdpcg_admm_lin_infeas_shared_{suf}")


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
            assert key(a) == "eps" and t is (ctypes.c_float if name.endswith("f32") else ctypes.c_double), (name, a)


@pytest.mark.parametrize("name", NEW)
def test_null_handle_and_null_pointers_are_invalid(lib, name):
    """No call here reaches a device: a null handle is refused first, alone and with a NULL in any one slot, and the words passed
    for d_cert and d_flag keep what they held."""
    args = declaration(name)
    words = {key(a): (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0) for a in args if "*" in a}

    def value(a, null):
        if "*" in a:
            return None if key(a) == null else ctypes.cast(words[key(a)], ctypes.c_void_p)
        return 2 if a.startswith("uint32_t") else 0.1
    for null in [None] + [key(a) for a in args[1:] if "*" in a]:
        assert getattr(lib, name)(None, *[value(a, null) for a in args[1:]]) == 1, null      # GBDPCG_ERR_INVALID
    assert all(list(w) == [7.0] * 4 for w in words.values())


def test_reachable_from_python():
    for m in NAMES:
        assert callable(getattr(binding.Solver, m)), m
