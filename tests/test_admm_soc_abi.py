"""CPU-only checks of the entry points for second-order cone rows (gbdpcg_admm_soc_init_*, gbdpcg_admm_soc_update_*,
gbdpcg_admm_soc_step_*, gbdpcg_admm_soc_step_shared_* and the two graph constructors): declared in include/gbdpcg.h, listed in
binding.SYMBOLS, exported by the built library, bound with argument lists that match the declarations, refusing a null handle and
every bad split of the rows, reachable through binding.Solver.

The refusals of the row classes are decided from the sizes alone, before the handle or any pointer is looked into; so they are
checked here without a device, with a handle and pointers that are not null and point at nothing the library may use (a zeroed
buffer): a call that got past its refusal would not return the status asserted."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_soc_init", "admm_soc_update", "admm_soc_step", "graph_create_admm_soc_step", "admm_soc_step_shared",
         "graph_create_admm_soc_step_shared")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
HEAD = ["h", "nx", "nu", "mx", "mu", "lx", "qx", "lu", "qu", "N", "batch"]
ROWS = ["d_g", "d_E", "d_lo", "d_hi", "d_rho"]
STEP = HEAD + ["d_Ginv", "d_C", "d_g", "d_c", "d_E", "d_lo", "d_hi", "d_rho", "d_S", "d_Pinv", "d_gamma", "d_lambda", "d_r", "d_p", "tol",
               "max_iter", "d_iters", "d_max_iter_exit", "d_z", "d_w", "d_y", "d_gt", "d_res"]
ARGS = {"admm_soc_init": HEAD + ROWS + ["d_w", "d_y", "d_gt", "stream"],
        "admm_soc_update": HEAD + ROWS + ["d_z", "d_w", "d_y", "d_gt", "d_res", "stream"],
        "admm_soc_step": STEP + ["stream"], "admm_soc_step_shared": STEP + ["stream"],
        "graph_create_admm_soc_step": STEP + ["out"], "graph_create_admm_soc_step_shared": STEP + ["out"]}
INVALID, UNSUPPORTED = 1, 4


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
    assert len(NEW) == 12
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", NEW)
def test_declared_argument_lists(name):
    """lx, qx, lu, qu directly behind mx, mu; with them taken out every list is that of the gbdpcg_admm_lin_* call."""
    base = name[len("gbdpcg_"):-4]
    args = declaration(name)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS[base], (name, args)
    rest = [a for a in args if a.split()[-1] not in ("lx", "qx", "lu", "qu")]
    assert rest == declaration(name.replace("admm_soc", "admm_lin")), name


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


GOOD = {"nx": 14, "nu": 7, "mx": 5, "mu": 4, "lx": 2, "qx": 3, "lu": 0, "qu": 4, "N": 8, "batch": 1, "tol": 1e-6, "max_iter": 10}


def call(lib, name, handle, pointer, **over):
    base = name[len("gbdpcg_"):-4]
    out = ctypes.c_void_p()
    v = dict(GOOD, **over)
    args = []
    for a in ARGS[base]:
        if a == "h":
            args.append(handle)
        elif a == "out":
            args.append(ctypes.byref(out))
        elif a == "stream":
            args.append(None)
        else:
            args.append(v[a] if a in v else pointer)
    st = getattr(lib, name)(*args)
    assert not out.value
    return st


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID before anything else is looked at, as for the older entry points; with good and with bad row classes."""
    assert call(lib, name, None, None) == INVALID
    assert call(lib, name, None, None, lx=6) == INVALID


# the splits of the rows that are refused, with the status the header gives
BAD = [(dict(lx=6), INVALID), (dict(lu=5), INVALID),                              # more linear rows than rows
       (dict(qx=0), INVALID), (dict(qu=0), INVALID),                              # cone rows and no dimension
       (dict(qx=2), INVALID), (dict(qu=3), INVALID), (dict(lx=1, qx=3), INVALID),  # not a whole number of cones
       (dict(mx=0, mu=0, lx=0, lu=0), INVALID),                                   # what admm_lin refuses: no rows at all
       (dict(nx=0), INVALID), (dict(nu=0), INVALID), (dict(N=0), INVALID), (dict(batch=0), INVALID),
       (dict(mx=65, lx=65), UNSUPPORTED), (dict(mu=68), UNSUPPORTED),   # above 64 rows per block
       (dict(mx=66, lx=67), INVALID)]                                             # INVALID comes before UNSUPPORTED


@pytest.mark.parametrize("name", NEW)
def test_bad_row_classes_are_refused_before_anything_is_looked_into(lib, name):
    zeros = ctypes.create_string_buffer(1 << 16)
    handle = pointer = ctypes.c_void_p(ctypes.addressof(zeros))
    for over, status in BAD:
        if status == UNSUPPORTED and "step" in name:
            continue    # (the steps ask the device of the handle about the solve first: tests/test_gpu_admm_soc.py)
        assert call(lib, name, handle, pointer, **over) == status, (name, over)
    assert not any(zeros.raw), "a refused call wrote through a pointer"


def test_solver_has_the_methods():
    for name in ("admm_soc_init", "admm_soc_update", "admm_soc_step", "admm_soc_step_shared", "graph_admm_soc_step",
                 "graph_admm_soc_step_shared"):
        assert callable(getattr(binding.Solver, name, None)), name
