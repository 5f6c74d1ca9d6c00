"""CPU-only checks of the entry points of the linear-row QP's backward pass (gbdpcg_admm_lin_adjoint_*, gbdpcg_admm_lin_grad_*),
after tests/test_admm_adjoint_abi.py: declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, taking
the admm_lin family's argument list with d_yf where d_lo, d_hi stand, refusing a null handle and a NULL in every required slot
before anything is looked at, reachable through binding.Solver and gbd_pcg_amd.autograd."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_lin_adjoint_init", "admm_lin_adjoint_update", "admm_lin_adjoint_step", "graph_create_admm_lin_adjoint_step",
         "admm_lin_grad")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
LIN = {"admm_lin_adjoint_init": "admm_lin_init", "admm_lin_adjoint_update": "admm_lin_update",
       "admm_lin_adjoint_step": "admm_lin_step", "graph_create_admm_lin_adjoint_step": "graph_create_admm_lin_step"}
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
    assert not any("lin_grad_shared" in n or "soc_adjoint" in n or "soft_adjoint" in n for n in declared)


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(LIN))
def test_argument_list_is_the_lin_one_with_yf_for_lo_and_hi(name, suf):
    a, h = declaration(f"gbdpcg_{name}_{suf}"), declaration(f"gbdpcg_{LIN[name]}_{suf}")
    ty = "float" if suf == "f32" else "double"
    i = [key(x) for x in h].index("d_lo")
    assert key(h[i + 1]) == "d_hi" and key(h[i - 1]) == "d_E"
    want = h[:i] + [f"const {ty} *d_yf"] + h[i + 2:]
    want = [re.sub(r"\b(d_[A-Za-z_]+)$", lambda m: RENAMED.get(m.group(1), m.group(1)), x) for x in want]
    assert a == want, name


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_grad_declaration(suf):
    ty = "float" if suf == "f32" else "double"
    assert declaration(f"gbdpcg_admm_lin_grad_{suf}") == [
        "gbdpcg_handle_t h", "uint32_t nx", "uint32_t nu", "uint32_t mx", "uint32_t mu", "uint32_t N", "uint32_t batch",
        f"const {ty} *d_z", f"const {ty} *d_az", f"const {ty} *d_yf", f"const {ty} *d_ya", f"const {ty} *d_rho", f"{ty} *d_glo",
        f"{ty} *d_ghi", f"{ty} *d_gE", "void *stream"]


@pytest.mark.parametrize("name", NEW)
def test_argtypes_match_the_declaration(lib, name):
    args = declaration(name)
    at = getattr(lib, name).argtypes
    assert at is not None and len(at) == len(args), name
    for a, t in zip(args, at):
        if "*" in a or a.startswith("gbdpcg_handle_t") or a.startswith("gbdpcg_graph_t"):
            assert t in (ctypes.c_void_p,) or issubclass(t, ctypes._Pointer), (name, a)
        elif a.startswith("uint32_t"):
            assert t is ctypes.c_uint32, (name, a)
        else:
            assert t is (ctypes.c_float if name.endswith("f32") else ctypes.c_double), (name, a)


@pytest.mark.parametrize("name", NEW)
def test_null_handle_and_null_pointers_are_invalid(lib, name):
    """No call here reaches a device: a null handle, or a handle-less NULL in a required slot, is refused first.  The scratch word
    passed for every pointer is never dereferenced."""
    args = declaration(name)
    word = (ctypes.c_double * 4)()
    out = ctypes.c_void_p()

    def value(a, null=False):
        if a.startswith("gbdpcg_graph_t"):
            return ctypes.byref(out)
        if "*" in a:
            return None if null else ctypes.cast(word, ctypes.c_void_p)
        if a.startswith("uint32_t"):
            return 8 if key(a) == "max_iter" else 2
        return 1e-6
    assert getattr(lib, name)(None, *[value(a) for a in args[1:]]) == 1      # GBDPCG_ERR_INVALID
    assert not out.value


def test_reachable_from_python():
    from gbd_pcg_amd import autograd
    for m in ("admm_lin_adjoint_init", "admm_lin_adjoint_update", "admm_lin_adjoint_step", "graph_admm_lin_adjoint_step",
              "admm_lin_grad"):
        assert callable(getattr(binding.Solver, m)), m
    assert callable(autograd.lin_qp_solve)
    with pytest.raises(TypeError):
        autograd.lin_qp_solve(object(), 2, 1, 1, 1, 3, *[None] * 8, 5, 5)
