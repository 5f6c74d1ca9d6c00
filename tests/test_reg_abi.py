"""CPU-only checks of the per-problem regularisation entry points (gbdpcg_form_schur_reg_*, gbdpcg_kkt_step_reg_*,
gbdpcg_graph_create_kkt_step_reg_*, gbdpcg_kkt_residual_reg_*): declared in include/gbdpcg.h, listed in binding.SYMBOLS,
exported by the built library, refusing a null handle, and reachable through binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("form_schur_reg", "kkt_step_reg", "graph_create_kkt_step_reg", "kkt_residual_reg")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
# pointer arguments behind (h, nx, nu, N, batch): G, C, g, c, rho, then ...
TAIL = {"form_schur_reg": 4,               # S, gamma, Ginv, stream
        "kkt_residual_reg": 4}             # z, lambda, res, stream


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def test_new_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", hdr))
    assert len(NEW) == 8
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


def test_rho_follows_c_in_every_declaration():
    """Each entry point takes the argument list of the one it extends with d_rho directly after d_c."""
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    for name in NEW:
        m = re.search(name + r"\s*\(([^;]*)\);", hdr)
        assert m, name
        args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert args[:10] == ["h", "nx", "nu", "N", "batch", "d_G", "d_C", "d_g", "d_c", "d_rho"], (name, args)
        plain = re.search(name.replace("_reg", "") + r"\s*\(([^;]*)\);", hdr)
        assert [a.split()[-1].lstrip("*") for a in plain.group(1).split(",")] == args[:9] + args[10:], name


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    fn = getattr(lib, name)
    base = name[len("gbdpcg_"):-4]
    ft = ctypes.c_float if name.endswith("f32") else ctypes.c_double
    head = (None, 14, 7, 8, 1, None, None, None, None, None)    # h, nx, nu, N, batch, G, C, g, c, rho
    if base in TAIL:
        assert fn(*head, *([None] * TAIL[base])) == 1
    else:   # S, gamma, Ginv, Pinv, kind, lambda, r, p, tol, max_iter, iters, flags, z, stream / graph out
        out = ctypes.c_void_p()
        last = ctypes.byref(out) if base.startswith("graph") else None
        assert fn(*head, None, None, None, None, 2, None, None, None, ft(1e-6), 10, None, None, None, last) == 1
        assert not out.value


def test_solver_has_the_methods():
    for name in ("form_schur_reg", "kkt_step_reg", "graph_kkt_step_reg", "kkt_residual_reg"):
        assert callable(getattr(binding.Solver, name, None)), name
