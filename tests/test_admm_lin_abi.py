"""CPU-only checks of the entry points for stage-wise linear inequality rows (gbdpcg_admm_lin_form_*, gbdpcg_admm_lin_init_*,
gbdpcg_admm_lin_update_*, gbdpcg_admm_lin_step_*, gbdpcg_admm_lin_step_shared_* and the two graph constructors): declared in
include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, bound with argument lists that match the declarations,
refusing a null handle, reachable through binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_lin_form", "admm_lin_init", "admm_lin_update", "admm_lin_step", "graph_create_admm_lin_step", "admm_lin_step_shared",
         "graph_create_admm_lin_step_shared")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
HEAD = ["h", "nx", "nu", "mx", "mu", "N", "batch"]
ROWS = ["d_g", "d_E", "d_lo", "d_hi", "d_rho"]
STEP = HEAD + ["d_Ginv", "d_C", "d_g", "d_c", "d_E", "d_lo", "d_hi", "d_rho", "d_S", "d_Pinv", "d_gamma", "d_lambda", "d_r", "d_p", "tol",
               "max_iter", "d_iters", "d_max_iter_exit", "d_z", "d_w", "d_y", "d_gt", "d_res"]
ARGS = {"admm_lin_form": HEAD + ["d_G", "d_E", "d_rho", "d_Gt", "stream"],
        "admm_lin_init": HEAD + ROWS + ["d_w", "d_y", "d_gt", "stream"],
        "admm_lin_update": HEAD + ROWS + ["d_z", "d_w", "d_y", "d_gt", "d_res", "stream"],
        "admm_lin_step": STEP + ["stream"], "admm_lin_step_shared": STEP + ["stream"],
        "graph_create_admm_lin_step": STEP + ["out"], "graph_create_admm_lin_step_shared": STEP + ["out"]}


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def declaration(name):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", hdr))
    assert len(NEW) == 14
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", NEW)
def test_declared_argument_lists(name):
    """mx, mu directly behind nu, d_E directly in front of d_lo; the step takes the list of gbdpcg_admm_step_* with those three more,
    and with them and the box's own operands taken out it is the list of gbdpcg_kkt_resolve_* (the shared twins likewise)."""
    base = name[len("gbdpcg_"):-4]
    args = declaration(name)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS[base], (name, args)
    if "step" in base:
        rest = [a for a in args if a.split()[-1].lstrip("*") not in ("mx", "mu", "d_E")]
        assert rest == declaration(name.replace("admm_lin_step", "admm_step")), name
        rest = [a for a in rest if a.split()[-1].lstrip("*") not in ("d_lo", "d_hi", "d_rho", "d_w", "d_y", "d_gt", "d_res")]
        assert rest == declaration(name.replace("admm_lin_step", "kkt_resolve")), name


@pytest.mark.parametrize("name", NEW)
def test_bound_argtypes_match_the_declaration(lib, name):
    ft = ctypes.c_float if name.endswith("f32") else ctypes.c_double
    want = []
    for a in declaration(name):
        if "*" in a or a.startswith("gbdpcg_handle_t"):
            want.append(ctypes.POINTER(ctypes.c_void_p) if a.startswith("gbdpcg_graph_t") else ctypes.c_void_p)
        elif a.startswith("uint32_t"):
            want.append(ctypes.c_uint32)
        else:
            assert a.split()[0] in ("float", "double"), a
            want.append(ft)
    assert list(getattr(lib, name).argtypes) == want, name


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    fn = getattr(lib, name)
    base = name[len("gbdpcg_"):-4]
    out = ctypes.c_void_p()
    args = []
    for a in ARGS[base]:
        args.append({"nx": 14, "nu": 7, "mx": 4, "mu": 2, "N": 8, "batch": 1, "tol": 1e-6, "max_iter": 10, "out": ctypes.byref(out)}.get(a))
    assert fn(*args) == 1
    assert not out.value


def test_solver_has_the_methods():
    for name in ("admm_lin_form", "admm_lin_init", "admm_lin_update", "admm_lin_step", "admm_lin_step_shared", "graph_admm_lin_step",
                 "graph_admm_lin_step_shared"):
        assert callable(getattr(binding.Solver, name, None)), name
