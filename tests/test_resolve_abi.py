"""CPU-only checks of the frozen-linearisation entry points (gbdpcg_form_gamma_*, gbdpcg_kkt_resolve_* and the graph form):
declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, refusing a null handle, and reachable
through binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = [f"gbdpcg_{name}_{suf}" for name in ("form_gamma", "kkt_resolve", "graph_create_kkt_resolve") for suf in ("f32", "f64")]


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def test_new_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("suf,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_null_handle_is_invalid(lib, suf, ft):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    head = (None, 14, 7, 8, 1, None, None, None, None)              # h, nx, nu, N, batch, Ginv, C, g, c
    solve = (None, None, None, None, None, None, ft(0), 1, None, None, None)   # S, Pinv, gamma, lambda, r, p, tol, max_iter, iters, flags, z
    assert getattr(lib, f"gbdpcg_form_gamma_{suf}")(*head, None, None) == 1
    assert getattr(lib, f"gbdpcg_kkt_resolve_{suf}")(*head, *solve, None) == 1
    g = ctypes.c_void_p(1)
    assert getattr(lib, f"gbdpcg_graph_create_kkt_resolve_{suf}")(*head, *solve, ctypes.byref(g)) == 1


def test_solver_has_the_methods():
    for name in ("form_gamma", "kkt_resolve", "graph_kkt_resolve"):
        assert callable(getattr(binding.Solver, name, None)), name
