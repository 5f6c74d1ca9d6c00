"""CPU-only checks of the KKT residual entry points (gbdpcg_kkt_residual_* and gbdpcg_kkt_residual_shared_*): declared in
include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, refusing a null handle, and reachable through
binding.Solver."""
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = [f"gbdpcg_{name}_{suf}" for name in ("kkt_residual", "kkt_residual_shared") for suf in ("f32", "f64")]


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
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    # h, nx, nu, N, batch, G, C, g, c, z, lambda, res, stream
    assert getattr(lib, name)(None, 14, 7, 8, 1, None, None, None, None, None, None, None, None) == 1


def test_solver_has_the_methods():
    for name in ("kkt_residual", "kkt_residual_shared"):
        assert callable(getattr(binding.Solver, name, None)), name
