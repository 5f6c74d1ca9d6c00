"""CPU-only checks of the entry points of the soft QPs' backward pass (gbdpcg_admm_soft_mask_*, gbdpcg_admm_lin_soft_mask_*,
gbdpcg_admm_soft_grad_bounds_*, gbdpcg_admm_lin_soft_grad_*), after tests/test_admm_lin_adjoint_abi.py: declared in
include/gbdpcg.h with the argument lists the contract gives, listed in binding.SYMBOLS, exported by the built library, refusing a
null handle before anything is looked at, reachable through binding.Solver and gbd_pcg_amd.autograd."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("admm_soft_mask", "admm_lin_soft_mask", "admm_soft_grad_bounds", "admm_lin_soft_grad")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
BOX = ["gbdpcg_handle_t h", "uint32_t nx", "uint32_t nu", "uint32_t N", "uint32_t batch"]
ROWS = ["gbdpcg_handle_t h", "uint32_t nx", "uint32_t nu", "uint32_t mx", "uint32_t mu", "uint32_t N", "uint32_t batch"]
# inputs (const), outputs
LISTS = {"admm_soft_mask": (BOX, ("d_yf", "d_kappa", "d_rho"), ("d_ym",)),
         "admm_lin_soft_mask": (ROWS, ("d_yf", "d_kappa", "d_rho"), ("d_ym",)),
         "admm_soft_grad_bounds": (BOX, ("d_yf", "d_kappa", "d_rho", "d_ya", "d_az"), ("d_glo", "d_ghi", "d_gkappa")),
         "admm_lin_soft_grad": (ROWS, ("d_z", "d_az", "d_E", "d_yf", "d_ya", "d_kappa", "d_rho"), ("d_glo", "d_ghi", "d_gkappa", "d_gE"))}


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
    assert len(set(NEW)) == 8
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name
    assert not any(("soft_mask" in n or "soft_grad" in n) and "shared" in n for n in declared)      # no _shared twins


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_declaration(name, suf):
    ty = "float" if suf == "f32" else "double"
    sizes, ins, outs = LISTS[name]
    want = sizes + [f"const {ty} *{a}" for a in ins] + [f"{ty} *{a}" for a in outs] + ["void *stream"]
    assert declaration(f"gbdpcg_{name}_{suf}") == want


@pytest.mark.parametrize("name", NEW)
def test_argtypes_match_the_declaration(lib, name):
    args = declaration(name)
    at = getattr(lib, name).argtypes
    assert at is not None and len(at) == len(args), name
    for a, t in zip(args, at):
        if "*" in a or a.startswith("gbdpcg_handle_t"):
            assert t is ctypes.c_void_p, (name, a)
        else:
            assert a.startswith("uint32_t") and t is ctypes.c_uint32, (name, a)


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """No call here reaches a device: a null handle is refused first.  The scratch words are never dereferenced."""
    args = declaration(name)
    words = [(ctypes.c_double * 4)() for _ in args]
    values = [ctypes.cast(w, ctypes.c_void_p) if "*" in a else 2 for a, w in zip(args[1:], words)]
    assert getattr(lib, name)(None, *values) == 1      # GBDPCG_ERR_INVALID


def test_reachable_from_python():
    from gbd_pcg_amd import autograd
    for m in ("admm_soft_mask", "admm_lin_soft_mask", "admm_soft_grad_bounds", "admm_lin_soft_grad"):
        assert callable(getattr(binding.Solver, m)), m
    with pytest.raises(TypeError):
        autograd.soft_box_qp_solve(object(), 2, 1, 3, *[None] * 8, 5, 5)
    with pytest.raises(TypeError):
        autograd.soft_lin_qp_solve(object(), 2, 1, 1, 1, 3, *[None] * 9, 5, 5)
