"""CPU-only checks of the adaptive-rho entry points (gbdpcg_admm_rebalance_*, gbdpcg_admm_lin_rebalance_*, gbdpcg_admm_soc_rebalance_*,
the three gbdpcg_admm*_restep_* and their graph constructors): declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by
the built library, bound with argument lists that match the declarations, refusing a null handle, reachable through
binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = {"admm": [], "admm_lin": ["mx", "mu"], "admm_soc": ["mx", "mu", "lx", "qx", "lu", "qu"]}
RULE = ["ratio", "shift", "rho_min", "rho_max", "d_expo"]
SOLVE = ["d_gamma", "d_lambda", "d_r", "d_p", "tol", "max_iter", "d_iters", "d_max_iter_exit", "d_z"]
STATE = ["d_w", "d_y", "d_gt"]
ARGS = {}
for fam, extra in FAMILIES.items():
    head = ["h", "nx", "nu"] + extra + ["N", "batch"]
    rows = ["d_E"] if extra else []
    ARGS[f"{fam}_rebalance"] = head + ["d_g"] + (rows + ["d_lo", "d_hi"] if extra else []) + ["d_res", "d_rho"] + STATE + RULE + ["stream"]
    restep = (head + ["d_G"] + (["d_Gt"] if extra else []) + ["d_Ginv", "d_C", "d_g", "d_c"] + rows + ["d_lo", "d_hi", "d_rho", "d_S", "d_Pinv",
              "kind"] + SOLVE + STATE + ["d_res"] + RULE)
    ARGS[f"{fam}_restep"] = restep + ["stream"]
    ARGS[f"graph_create_{fam}_restep"] = restep + ["out"]
NEW = [f"gbdpcg_{name}_{suf}" for name in ARGS for suf in ("f32", "f64")]
METHODS = ("admm_rebalance", "admm_lin_rebalance", "admm_soc_rebalance", "admm_restep", "admm_lin_restep", "admm_soc_restep",
           "graph_admm_restep", "graph_admm_lin_restep", "graph_admm_soc_restep")


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
    assert len(NEW) == 18
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name
    assert not [n for n in declared if "rebalance_shared" in n or "restep_shared" in n]     # no shared twins: one matrix, one rho


@pytest.mark.parametrize("name", NEW)
def test_declared_argument_lists(name):
    """The names and the order: the rule always as ratio, shift, rho_min, rho_max, d_expo at the end; a restep takes the list of the
    family's step with d_G (rows: d_G, d_Gt) in front of d_Ginv and the kind behind d_Pinv."""
    base = name[len("gbdpcg_"):-4]
    args = declaration(name)
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ARGS[base], (name, names)
    assert names[-6:-1] == RULE
    if "restep" in base:
        step = [a.split()[-1].lstrip("*") for a in declaration(name.replace("restep", "step"))]
        rest = [a for a in names if a not in ("d_G", "d_Gt", "kind") + tuple(RULE)]
        assert rest == step, name
        # what the refactorisation and the rule write is not const
        for a in args:
            if a.split()[-1].lstrip("*") in ("d_Ginv", "d_S", "d_Pinv", "d_rho", "d_Gt", "d_expo"):
                assert not a.startswith("const"), (name, a)
    by_name = {a.split()[-1].lstrip("*"): a for a in args}
    assert by_name["d_res"].startswith("const") == ("rebalance" in base)
    assert by_name["d_expo"].startswith("int32_t") and by_name["shift"].startswith("uint32_t")


@pytest.mark.parametrize("name", NEW)
def test_bound_argtypes_match_the_declaration(lib, name):
    ft = ctypes.c_float if name.endswith("f32") else ctypes.c_double
    want = []
    for a in declaration(name):
        if "*" in a or a.startswith("gbdpcg_handle_t"):
            want.append(ctypes.POINTER(ctypes.c_void_p) if a.startswith("gbdpcg_graph_t") else ctypes.c_void_p)
        elif a.startswith("uint32_t"):
            want.append(ctypes.c_uint32)
        elif a.startswith("gbdpcg_pinv_kind"):
            want.append(ctypes.c_int)
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
    sizes = {"nx": 14, "nu": 7, "mx": 2, "mu": 1, "lx": 2, "qx": 1, "lu": 1, "qu": 1, "N": 8, "batch": 1, "tol": 1e-6, "max_iter": 10,
             "kind": 2, "ratio": 10.0, "shift": 1, "rho_min": 1e-3, "rho_max": 1e3, "out": ctypes.byref(out)}
    assert fn(*[sizes.get(a) for a in ARGS[base]]) == 1
    assert not out.value


def test_solver_has_the_methods():
    for name in METHODS:
        assert callable(getattr(binding.Solver, name, None)), name
