"""CPU-only checks of the mixed-precision refinement entry points: declared in include/gbdpcg.h, listed in binding.SYMBOLS,
exported by the built library, with the ctypes signatures of the header, refusing a null handle, reachable through
binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["gbdpcg_demote_f32", "gbdpcg_kkt_defect_mixed", "gbdpcg_kkt_refine_apply", "gbdpcg_kkt_refine_step",
       "gbdpcg_graph_create_kkt_refine_step"]
VP, U32 = ctypes.c_void_p, ctypes.c_uint32
HEAD = [VP, U32, U32, U32, U32, VP, VP, VP, VP]                                     # h, nx, nu, N, batch, G, C, g, c
STEP = HEAD + [VP] * 4 + [VP] * 7 + [ctypes.c_float, U32, VP, VP] + [VP] * 4        # kept | work | tol, max_iter, iters, flags | expo, z, lambda, res
ARGTYPES = {
    "gbdpcg_demote_f32": [VP, ctypes.c_uint64, VP, VP, VP],
    "gbdpcg_kkt_defect_mixed": HEAD + [VP] * 8,
    "gbdpcg_kkt_refine_apply": [VP, U32, U32, U32, U32] + [VP] * 6,
    "gbdpcg_kkt_refine_step": STEP + [VP],
    "gbdpcg_graph_create_kkt_refine_step": STEP + [ctypes.POINTER(VP)],
}
# the parameter types of the header, in the order of ARGTYPES' classes: pointer -> VP, uint32_t -> U32, ...
C_TYPES = {"uint32_t": U32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}


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


@pytest.mark.parametrize("name", NEW)
def test_ctypes_signature_is_the_header_s(lib, name):
    hdr = open(os.path.join(ROOT, "include", "gbdpcg.h")).read()
    m = re.search(r"gbdpcg_status\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, name
    want = []
    for prm in m.group(1).split(","):
        prm = " ".join(prm.split())
        if "*" in prm:
            want.append(ctypes.POINTER(VP) if prm.startswith("gbdpcg_graph_t *") else VP)
        elif prm.startswith("gbdpcg_handle_t"):
            want.append(VP)
        else:
            want.append(C_TYPES[prm.split()[0]])
    assert want == ARGTYPES[name]
    assert list(getattr(lib, name).argtypes) == ARGTYPES[name]


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    args = [None if t is VP or t == ctypes.POINTER(VP) else 3 for t in ARGTYPES[name]]
    assert getattr(lib, name)(*args) == 1


def test_solver_has_the_methods():
    for name in ("demote", "kkt_defect_mixed", "kkt_refine_apply", "kkt_refine_step", "graph_kkt_refine_step", "kkt_solve_refined"):
        assert callable(getattr(binding.Solver, name, None)), name
