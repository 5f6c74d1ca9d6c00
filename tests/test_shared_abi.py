"""CPU-only checks of the shared-matrix entry points (one S, Phi^-1, G^-1, C for a whole batch: gbdpcg_solve_shared_*,
gbdpcg_form_gamma_shared_*, gbdpcg_recover_primal_shared_*, gbdpcg_kkt_resolve_shared_* and the two graph forms): declared in
include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, refusing a null handle, and reachable through
binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("solve_shared", "graph_create_solve_shared", "form_gamma_shared", "recover_primal_shared", "kkt_resolve_shared",
         "graph_create_kkt_resolve_shared")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def test_twelve_symbols_declared_listed_and_exported(lib):
    assert len(NEW) == 12
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("suf,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_null_handle_is_invalid(lib, suf, ft):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the twins."""
    plain = (None, 14, 8, 3, None, None, None, None, None, None, ft(0), 1, None, None)   # h, n, N, batch, S .. flags
    head = (None, 14, 7, 8, 3, None, None, None, None)              # h, nx, nu, N, batch, Ginv, C, g, c
    solve = (None, None, None, None, None, None, ft(0), 1, None, None, None)   # S, Pinv, gamma, lambda, r, p, tol, max_iter, iters, flags, z
    g = ctypes.c_void_p(1)
    assert getattr(lib, f"gbdpcg_solve_shared_{suf}")(*plain, None) == 1
    assert getattr(lib, f"gbdpcg_graph_create_solve_shared_{suf}")(*plain, ctypes.byref(g)) == 1
    assert getattr(lib, f"gbdpcg_form_gamma_shared_{suf}")(*head, None, None) == 1
    assert getattr(lib, f"gbdpcg_recover_primal_shared_{suf}")(*head, None, None) == 1
    assert getattr(lib, f"gbdpcg_kkt_resolve_shared_{suf}")(*head, *solve, None) == 1
    assert getattr(lib, f"gbdpcg_graph_create_kkt_resolve_shared_{suf}")(*head, *solve, ctypes.byref(g)) == 1


def test_solver_has_the_methods():
    for name in ("solve_shared", "graph_solve_shared", "form_gamma_shared", "recover_primal_shared", "kkt_resolve_shared",
                 "graph_kkt_resolve_shared"):
        assert callable(getattr(binding.Solver, name, None)), name
