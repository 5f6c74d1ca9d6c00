"""CPU-only checks of the soft-bound ADMM entry points (gbdpcg_admm_soft_*, gbdpcg_admm_lin_soft_*), after tests/test_admm_abi.py:
declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the built library, taking the hard family's argument list with
d_kappa directly behind d_hi, bound with matching argtypes, refusing a null handle and a NULL d_kappa, reachable through
binding.Solver."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPS = ("init", "update", "step", "graph_create:step", "step_shared", "graph_create:step_shared", "restep", "graph_create:restep")


def name_of(fam, op, suf):
    pre, _, op = op.rpartition(":")
    return f"gbdpcg_{pre + '_' if pre else ''}{fam}_{op}_{suf}"


PAIRS = [(name_of(soft, op, suf), name_of(hard, op, suf)) for soft, hard in (("admm_soft", "admm"), ("admm_lin_soft", "admm_lin"))
         for op in OPS + (("rebalance",) if hard == "admm_lin" else ()) for suf in ("f32", "f64")]
NEW = [p[0] for p in PAIRS]


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
    assert len(NEW) == 34 and len(set(NEW)) == 34
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "gbdpcg_admm_soft_rebalance_f32" not in declared      # gbdpcg_admm_rebalance_* is the soft box's rebalance


@pytest.mark.parametrize("soft,hard", PAIRS)
def test_argument_list_is_the_hard_one_with_kappa_behind_hi(soft, hard):
    a, h = declaration(soft), declaration(hard)
    i = [x.split()[-1].lstrip("*") for x in h].index("d_hi")
    ty = "float" if soft.endswith("f32") else "double"
    assert a == h[:i + 1] + [f"const {ty} *d_kappa"] + h[i + 1:], soft
    assert len(a) == len(h) + 1


@pytest.mark.parametrize("name", NEW)
def test_bound_argtypes_match_the_declaration(lib, name):
    ft = ctypes.c_float if name.endswith("f32") else ctypes.c_double
    want = []
    for a in declaration(name):
        if "*" in a or a.startswith("gbdpcg_handle_t"):
            want.append(ctypes.POINTER(ctypes.c_void_p) if a.startswith("gbdpcg_graph_t") else ctypes.c_void_p)
        elif a.startswith("uint32_t"):
            want.append(ctypes.c_uint32)
        elif a.startswith("gbdpcg_pinv_kind"):
            want.append(ctypes.c_int)
        else:
            assert a.split()[0] in ("float", "double"), a
            want.append(ft)
    assert list(getattr(lib, name).argtypes) == want, name


def call_args(name, null):
    """Every pointer a distinct non-null dummy (nothing is dereferenced before the refusal), sizes and the rule valid; `null`: the
    arguments passed as NULL."""
    out = ctypes.c_void_p()
    scalars = {"nx": 14, "nu": 7, "mx": 2, "mu": 2, "N": 8, "batch": 1, "tol": 1e-6, "max_iter": 10, "kind": 2, "ratio": 10.0, "shift": 1,
               "rho_min": 1e-3, "rho_max": 1e3}
    args = []
    for i, a in enumerate(declaration(name)):
        key = a.split()[-1].lstrip("*")
        if key in null:
            args.append(None)
        elif key in scalars:
            args.append(scalars[key])
        elif key == "out":
            args.append(ctypes.byref(out))
        else:
            args.append(ctypes.c_void_p(0x1000 * (i + 1)))
    return args, out


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    args, out = call_args(name, null=("h",))
    assert getattr(lib, name)(*args) == 1
    assert not out.value


@pytest.mark.parametrize("name", NEW)
def test_null_kappa_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID with every other argument in place: the refusal comes before the handle or any array is looked at (the
    handle here is a dummy no call could use)."""
    args, out = call_args(name, null=("d_kappa",))
    assert getattr(lib, name)(*args) == 1
    assert not out.value


def test_solver_has_the_methods():
    for fam in ("admm_soft", "admm_lin_soft"):
        for name in (f"{fam}_init", f"{fam}_update", f"{fam}_step", f"graph_{fam}_step", f"{fam}_step_shared", f"graph_{fam}_step_shared",
                     f"{fam}_restep", f"graph_{fam}_restep"):
            assert callable(getattr(binding.Solver, name, None)), name
    assert callable(getattr(binding.Solver, "admm_lin_soft_rebalance", None))
