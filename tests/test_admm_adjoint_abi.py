"""CPU-only checks of the entry points of the box QP's backward pass (gbdpcg_admm_adjoint_*, gbdpcg_admm_grad_bounds_*), after
tests/test_admm_soft_abi.py: declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, taking the box
family's argument list with d_yf where d_lo, d_hi stand, bound with matching argtypes, refusing a null handle and a NULL in every
required slot before anything is looked at, reachable through binding.Solver and gbd_pcg_amd.autograd."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_adjoint_init", "admm_adjoint_update", "admm_adjoint_step", "graph_create_admm_adjoint_step", "admm_grad_bounds")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
# adjoint name -> the box entry it mirrors, and the adjoint's names for the box's arguments
BOX = {"admm_adjoint_init": "admm_init", "admm_adjoint_update": "admm_update", "admm_adjoint_step": "admm_step",
       "graph_create_admm_adjoint_step": "graph_create_admm_step"}
RENAMED = {"d_g": "d_gz", "d_c": "d_nglam", "d_z": "d_az", "d_lambda": "d_alambda", "d_w": "d_wa", "d_y": "d_ya", "d_gt": "d_gta"}
OPTIONAL = ("d_Pinv", "d_r", "d_p", "d_max_iter_exit")


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
    assert len(set(NEW)) == 10
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name
    assert not any("adjoint" in n and "shared" in n for n in declared)      # no _shared twins


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(BOX))
def test_argument_list_is_the_box_one_with_yf_for_lo_and_hi(name, suf):
    a, h = declaration(f"gbdpcg_{name}_{suf}"), declaration(f"gbdpcg_{BOX[name]}_{suf}")
    ty = "float" if suf == "f32" else "double"
    i = [key(x) for x in h].index("d_lo")
    assert key(h[i + 1]) == "d_hi"
    want = h[:i] + [f"const {ty} *d_yf"] + h[i + 2:]
    want = [re.sub(r"\b(d_[A-Za-z_]+)$", lambda m: RENAMED.get(m.group(1), m.group(1)), x) for x in want]
    assert a == want, name


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_grad_bounds_declaration(suf):
    ty = "float" if suf == "f32" else "double"
    assert declaration(f"gbdpcg_admm_grad_bounds_{suf}") == [
        "gbdpcg_handle_t h", "uint32_t nx", "uint32_t nu", "uint32_t N", "uint32_t batch", f"const {ty} *d_yf", f"const {ty} *d_rho",
        f"const {ty} *d_ya", f"{ty} *d_glo", f"{ty} *d_ghi", "void *stream"]


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


def call_args(name, null=(), **over):
    """Every pointer a distinct non-null dummy (nothing is dereferenced before the refusal), sizes valid; `null`: the arguments
    passed as NULL."""
    out = ctypes.c_void_p(0x77)
    scalars = {"nx": 14, "nu": 7, "N": 8, "batch": 1, "tol": 1e-6, "max_iter": 10}
    scalars.update(over)
    args = []
    for i, a in enumerate(declaration(name)):
        k = key(a)
        if k in null:
            args.append(None)
        elif k in scalars:
            args.append(scalars[k])
        elif k == "out":
            args.append(ctypes.byref(out))
        else:
            args.append(ctypes.c_void_p(0x1000 * (i + 1)))
    return args, out


@pytest.mark.parametrize("name", NEW)
def test_null_in_a_required_slot_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID with every other argument in place: the refusal comes before the handle or any array is looked at (the
    handle and the pointers here are dummies no call could use)."""
    fn = getattr(lib, name)
    required = [key(a) for a in declaration(name) if ("*" in a or a.startswith("gbdpcg_handle_t")) and key(a) not in OPTIONAL + ("stream",)]
    assert "h" in required and "d_yf" in required and "d_rho" in required
    for k in required:
        args, out = call_args(name, null=(k,))
        assert fn(*args) == 1, (name, k)
        assert k == "out" or not out.value or "graph_create" not in name, (name, k)      # a refused constructor leaves NULL
    for k in ("nx", "nu", "N", "batch"):
        args, out = call_args(name, **{k: 0})
        assert fn(*args) == 1, (name, k)


def test_solver_and_autograd_have_the_entries():
    for name in ("admm_adjoint_init", "admm_adjoint_update", "admm_adjoint_step", "graph_admm_adjoint_step", "admm_grad_bounds"):
        assert callable(getattr(binding.Solver, name, None)), name
    from gbd_pcg_amd import autograd
    assert callable(autograd.box_qp_solve)
    with pytest.raises(TypeError):
        autograd.box_qp_solve(None, 3, 2, 4, *([None] * 7), 10, 10)
