"""CPU-only checks of the backward-pass entry points (gbdpcg_kkt_grad_*, gbdpcg_kkt_grad_shared_*, gbdpcg_kkt_backward_*,
gbdpcg_kkt_backward_shared_* and the two graph constructors): declared in include/gbdpcg.h, listed in binding.SYMBOLS, exported by the
built library, bound with argument lists that match the declarations, refusing a null handle, reachable through binding.Solver and
gbd_pcg_amd.autograd; the header states the definitions the kernels implement."""
import ctypes
import os
import re

import pytest

from gbd_pcg_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("kkt_grad", "kkt_grad_shared", "kkt_backward", "kkt_backward_shared", "graph_create_kkt_backward",
         "graph_create_kkt_backward_shared")
NEW = [f"gbdpcg_{name}_{suf}" for name in NAMES for suf in ("f32", "f64")]
HEAD = ["h", "nx", "nu", "N", "batch"]
GRAD = HEAD + ["d_z", "d_lambda", "d_az", "d_alambda", "d_gG", "d_gC", "stream"]
BACK = HEAD + ["d_Ginv", "d_C", "d_gz", "d_nglam", "d_S", "d_Pinv", "d_gamma", "d_z", "d_lambda", "d_az", "d_alambda", "d_r", "d_p", "tol",
               "max_iter", "d_iters", "d_max_iter_exit", "d_gG", "d_gC"]
ARGS = {"kkt_grad": GRAD, "kkt_grad_shared": GRAD, "kkt_backward": BACK + ["stream"], "kkt_backward_shared": BACK + ["stream"],
        "graph_create_kkt_backward": BACK + ["out"], "graph_create_kkt_backward_shared": BACK + ["out"]}


@pytest.fixture(scope="module")
def lib():
    binding.build()
    return binding.load()


def header():
    return open(os.path.join(ROOT, "include", "gbdpcg.h")).read()


def declaration(name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_declared_listed_and_exported(lib):
    declared = set(re.findall(r"\b(gbdpcg_[a-z0-9_]+)\s*\(", header()))
    assert len(NEW) == 12
    for name in NEW:
        assert name in declared, name
        assert name in binding.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", NEW)
def test_declared_argument_lists(name):
    """The names and the order of the issue's argument lists.  The backward calls take the list of gbdpcg_kkt_resolve_* with d_gz,
    d_nglam for d_g, d_c, the forward point d_z, d_lambda (read only) in front of the adjoint pair d_az, d_alambda that stands for
    the resolve's d_lambda, d_z, and d_gG, d_gC behind d_max_iter_exit; the shared twins and the graph constructors take the same
    operands."""
    base = name[len("gbdpcg_"):-4]
    args = declaration(name)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS[base], (name, args)
    if "backward" in base:
        twin = declaration(name.replace("kkt_backward", "kkt_resolve"))
        rename = {"d_gz": "d_g", "d_nglam": "d_c", "d_alambda": "d_lambda", "d_az": "d_z"}
        rest = [a for a in args if a.split()[-1].lstrip("*") not in ("d_z", "d_lambda", "d_gG", "d_gC")]
        rest = [re.sub(r"(\w+)$", lambda m: rename.get(m.group(1), m.group(1)), a) for a in rest]
        assert sorted(rest) == sorted(twin), name      # (the resolve has d_z last, here d_az stands next to d_alambda)
        names = [a.split()[-1].lstrip("*") for a in args]
        for const_in in ("d_z", "d_lambda", "d_gz", "d_nglam"):
            assert args[names.index(const_in)].startswith("const "), (name, const_in)


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


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_invalid(lib, name):
    """GBDPCG_ERR_INVALID (1) before anything else is looked at, as for the older entry points."""
    fn = getattr(lib, name)
    base = name[len("gbdpcg_"):-4]
    out = ctypes.c_void_p()
    args = []
    for a in ARGS[base]:
        args.append({"nx": 14, "nu": 7, "N": 8, "batch": 1, "tol": 1e-6, "max_iter": 10, "out": ctypes.byref(out)}.get(a))
    assert fn(*args) == 1
    assert not out.value


def test_header_states_the_definitions():
    """The comment in front of the declarations carries the formulas in the binding's operand names and order."""
    hdr = " ".join(header().split())
    for text in ("dl/dg = a_z", "dl/dc = -a_lambda", "dl/dQ_k(i,j) = 1/2 (ax_k,i x_k,j + x_k,i ax_k,j)",
                 "dl/dA_k(i,j) = -(a_lambda,k+1,i x_k,j + lambda_k+1,i ax_k,j)",
                 "dl/dB_k(i,j) = -(a_lambda,k+1,i u_k,j + lambda_k+1,i au_k,j)", "dl/drho_b = a_z' z",
                 "g := d_gz, c := d_nglam", "d_nglam holds MINUS dl/dlambda", "(d_z, d_lambda, d_az, d_alambda)"):
        assert text in hdr, text


def test_solver_and_autograd_have_the_entry_points():
    for name in ("kkt_grad", "kkt_grad_shared", "kkt_backward", "kkt_backward_shared", "graph_kkt_backward", "graph_kkt_backward_shared"):
        assert callable(getattr(binding.Solver, name, None)), name
    pytest.importorskip("torch")
    from gbd_pcg_amd import autograd
    assert callable(autograd.kkt_solve)


def test_autograd_refuses_host_and_strided_tensors():
    """Non-contiguous or CPU tensors raise, as elsewhere in Solver: nothing is copied or moved behind the caller's back."""
    torch = pytest.importorskip("torch")
    from gbd_pcg_amd import autograd
    solver = object.__new__(binding.Solver)      # the argument checks come before the handle is touched
    solver.h = ctypes.c_void_p()
    nx, nu, N = 2, 1, 3
    G, C, g, c = torch.ones(13), torch.ones(12), torch.ones(8), torch.ones(6)
    with pytest.raises(ValueError):
        autograd.kkt_solve(solver, nx, nu, N, G, C, g, c)
    with pytest.raises(TypeError):
        autograd.kkt_solve(None, nx, nu, N, G, C, g, c)
