"""CPU-only checks of the regularised and shared-matrix refinement entry points: declared in include/gbdpcg.h, listed in
binding.SYMBOLS, exported by the built library, with the ctypes signatures of the header, refusing a null handle, reachable
through binding.Solver.  The header no longer calls them "not provided"."""
import ctypes
import inspect
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VP, U32 = ctypes.c_void_p, ctypes.c_uint32
HEAD = [VP, U32, U32, U32, U32, VP, VP, VP, VP]                                     # h, nx, nu, N, batch, G, C, g, c
DEFECT = [VP] * 8                                                                   # z, lambda | rg, rc, dlambda, expo, res | stream
STEP = [VP] * 4 + [VP] * 7 + [ctypes.c_float, U32, VP, VP] + [VP] * 4               # kept | work | tol, max_iter, iters, flags | expo, z, lambda, res
ARGTYPES = {
    "gbdpcg_kkt_defect_mixed_reg": HEAD + [VP] + DEFECT,                            # rho directly behind c
    "gbdpcg_kkt_defect_mixed_shared": HEAD + DEFECT,
    "gbdpcg_kkt_refine_step_reg": HEAD + [VP] + STEP + [VP],
    "gbdpcg_graph_create_kkt_refine_step_reg": HEAD + [VP] + STEP + [ctypes.POINTER(VP)],
    "gbdpcg_kkt_refine_step_shared": HEAD + STEP + [VP],
    "gbdpcg_graph_create_kkt_refine_step_shared": HEAD + STEP + [ctypes.POINTER(VP)],
}
NEW = list(ARGTYPES)
C_TYPES = {"uint32_t": U32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def header():
    return open(os.path.join(ROOT, "include", "gbdpcg.h")).read()


def test_new_symbols_declared_listed_and_exported(lib):
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", header()))
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", NEW)
def test_ctypes_signature_is_the_header_s(lib, name):
    m = re.search(r"gbdpcg_status\s+" + name + r"\s*\(([^;]*)\)\s*;", header())
    assert m, name
    want, names = [], []
    for prm in m.group(1).split(","):
        prm = " ".join(prm.split())
        names.append(prm.split()[-1].lstrip("*"))
        if "*" in prm:
            want.append(ctypes.POINTER(VP) if prm.startswith("gbdpcg_graph_t *") else VP)
        elif prm.startswith("gbdpcg_handle_t"):
            want.append(VP)
        else:
            want.append(C_TYPES[prm.split()[0]])
    assert want == ARGTYPES[name]
    assert list(getattr(lib, name).argtypes) == ARGTYPES[name]
    # d_rho stands directly behind d_c in the _reg forms and nowhere in the others
    assert ("d_rho" in names) == name.endswith("_reg")
    if name.endswith("_reg"):
        assert names[names.index("d_c") + 1] == "d_rho"


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    args = [None if t is VP or t == ctypes.POINTER(VP) else 3 for t in ARGTYPES[name]]
    assert getattr(lib, name)(*args) == 1


def test_solver_has_the_methods():
    for name in ("kkt_defect_mixed_reg", "kkt_defect_mixed_shared", "kkt_refine_step_reg", "kkt_refine_step_shared",
                 "graph_kkt_refine_step_reg", "graph_kkt_refine_step_shared"):
        assert callable(getattr(binding.Solver, name, None)), name
    prm = inspect.signature(binding.Solver.kkt_solve_refined).parameters
    assert prm["rho"].default is None and prm["shared"].default is False


def test_the_header_says_what_is_provided():
    hdr = header()
    assert "Not provided: _shared twins, and a _reg form" not in hdr
    assert "Not provided: _shared and _reg TOGETHER" in hdr
    assert "UNREGULARISED fp64 system" in hdr      # what a regularised factorisation behind the plain defect converges to
