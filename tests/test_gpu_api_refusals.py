"""The refusals of the solve and KKT entry points, one table: gbdpcg_solve_*, gbdpcg_form_pinv_solve_*, gbdpcg_kkt_step_*,
gbdpcg_kkt_step_reg_*, gbdpcg_kkt_resolve_*, gbdpcg_kkt_backward_*, the _shared twins of the solve, the resolve and the backward
pass, each next to its graph_create twin and in both precisions.  For every bad argument set the direct call and the graph-create
call return a recorded status, no graph comes back, and exactly the recorded output arrays were written: the composite calls run
their parts in order, so a part may have written before a later one refuses (gbdpcg_kkt_step_* forms S, gamma and G^-1 before the
solve looks at d_lambda) -- that order is behaviour.  A graph-create call writes nothing: what it captures never runs.  Its *out
comes back null where the call got as far as the common graph constructor, and is left as the caller had it where the entry point
refused before that (recorded per case; DESIGN.md lists it with the other unevennesses the table showed).

EXPECTED was recorded ONCE, by running this table against the build of the commit before the host layer was split into units
(one api.hip of 1731 lines); it is not derived from the code under test.  Per (entry, case): the status of the direct call, the
status of graph_create, the outputs the direct call wrote, what became of *out.  Where f32 and f64 differ the value is a dict by
precision (block size 65 passes the Schur formation's limit in f32 and not in f64).

The good shape is that of tests/test_gpu_admm_refusals.py.  The shapes of the bad cases are refused for what they are, but every
buffer is large enough for them, so that a call that wrongly went ahead would show as a wrong status and not as a fault."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, 1, 4
NX, NU, N, BATCH = 4, 3, 5, 2
# the Schur formation's smallest refused nx with nu = nx // 2 (tests/test_gpu_schur_dispatch.py, REFUSED_NX)
SCHUR_LIMIT = {"f32": 71, "f64": 50}
# a shape beyond one workgroup: that of tests/test_gpu_shared.py::test_a_shape_beyond_one_workgroup_is_unsupported in f64; its four
# LDS vectors of n N elements are 295 KB there and only 147 KB in f32, which fits, so f32 takes twice the horizon (295 KB again)
BEYOND_ONE_WG = {"f32": (36, 512, 2), "f64": (36, 256, 2)}

SOLVE = ("S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl")
RESOLVE = ("Ginv", "C", "g", "c", "S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z")
BACKWARD = ("Ginv", "C", "gz", "nglam", "S", "Pinv", "gamma", "z", "lam", "az", "alam", "r", "p", "tol", "max_iter", "it", "fl", "gG",
            "gC")
# entry -> (arguments behind the sizes, required pointers, outputs, has nu)
ENTRIES = {
    "solve": (SOLVE, ("S", "gamma", "lam", "it"), ("lam", "r", "p", "it", "fl"), False),
    "solve_shared": (SOLVE, ("S", "gamma", "lam", "it"), ("lam", "r", "p", "it", "fl"), False),
    "form_pinv_solve": (("S", "Pinv", "kind", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl"),
                        ("S", "Pinv", "gamma", "lam", "it"), ("Pinv", "lam", "r", "p", "it", "fl"), False),
    "kkt_step": (("G", "C", "g", "c", "S", "gamma", "Ginv", "Pinv", "kind", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z"),
                 ("G", "C", "g", "c", "S", "gamma", "Ginv", "Pinv", "lam", "it", "z"),
                 ("S", "gamma", "Ginv", "Pinv", "lam", "r", "p", "it", "fl", "z"), True),
    "kkt_step_reg": (("G", "C", "g", "c", "rho", "S", "gamma", "Ginv", "Pinv", "kind", "lam", "r", "p", "tol", "max_iter", "it", "fl",
                      "z"),
                     ("G", "C", "g", "c", "rho", "S", "gamma", "Ginv", "Pinv", "lam", "it", "z"),
                     ("S", "gamma", "Ginv", "Pinv", "lam", "r", "p", "it", "fl", "z"), True),
    "kkt_resolve": (RESOLVE, ("Ginv", "C", "g", "c", "S", "gamma", "lam", "it", "z"), ("gamma", "lam", "r", "p", "it", "fl", "z"), True),
    "kkt_resolve_shared": (RESOLVE, ("Ginv", "C", "g", "c", "S", "gamma", "lam", "it", "z"),
                           ("gamma", "lam", "r", "p", "it", "fl", "z"), True),
    "kkt_backward": (BACKWARD, ("Ginv", "C", "gz", "nglam", "S", "gamma", "z", "lam", "az", "alam", "it"),
                     ("gamma", "az", "alam", "r", "p", "it", "fl", "gG", "gC"), True),
    "kkt_backward_shared": (BACKWARD, ("Ginv", "C", "gz", "nglam", "S", "gamma", "z", "lam", "az", "alam", "it"),
                            ("gamma", "az", "alam", "r", "p", "it", "fl", "gG", "gC"), True),
}
LARGE = ("S", "Pinv", "Ginv", "gG", "gC")   # outputs of matrix size; the others are vectors
LARGE_ELEMS, SMALL_ELEMS = 1 << 21, 1 << 16


def cases(entry):
    args, required, _, has_nu = ENTRIES[entry]
    out = ["null-h"] + [f"null-{k}" for k in required] + ["N0", "batch0", "n65"]
    if "gG" in args:
        out.append("null-gG+gC")
    if "kind" in args:
        out.append("kind3")
    if has_nu:
        out += ["nu0", "schur-limit"]
    if entry.endswith("_shared"):
        out.append("beyond-one-wg")
    return out


# what graph_create left in *out: a null handle, or whatever the caller had there (the entries that refuse before they reach the
# common graph constructor return without touching it)
NULLED, KEPT = "nulled", "kept"
EXPECTED = {
    "solve": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', NULLED),
        "null-gamma": (INVALID, INVALID, '', NULLED),
        "null-lam": (INVALID, INVALID, '', NULLED),
        "null-it": (INVALID, INVALID, '', NULLED),
        "N0": (INVALID, INVALID, '', NULLED),
        "batch0": (INVALID, INVALID, '', NULLED),
        "n65": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
    },
    "solve_shared": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', NULLED),
        "null-gamma": (INVALID, INVALID, '', NULLED),
        "null-lam": (INVALID, INVALID, '', NULLED),
        "null-it": (INVALID, INVALID, '', NULLED),
        "N0": (INVALID, INVALID, '', NULLED),
        "batch0": (INVALID, INVALID, '', NULLED),
        "n65": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
        "beyond-one-wg": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
    },
    "form_pinv_solve": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', NULLED),
        "null-Pinv": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', NULLED),
        "null-lam": (INVALID, INVALID, '', NULLED),
        "null-it": (INVALID, INVALID, '', NULLED),
        "N0": (INVALID, INVALID, '', NULLED),
        "batch0": (INVALID, INVALID, '', NULLED),
        "n65": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
        "kind3": (INVALID, INVALID, '', KEPT),
    },
    "kkt_step": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-G": (INVALID, INVALID, '', NULLED),
        "null-C": (INVALID, INVALID, '', NULLED),
        "null-g": (INVALID, INVALID, '', NULLED),
        "null-c": (INVALID, INVALID, '', NULLED),
        "null-S": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', KEPT),
        "null-Ginv": (INVALID, INVALID, '', KEPT),
        "null-Pinv": (INVALID, INVALID, 'S gamma Ginv', KEPT),
        "null-lam": (INVALID, INVALID, 'S gamma Ginv', NULLED),
        "null-it": (INVALID, INVALID, 'S gamma Ginv', NULLED),
        "null-z": (INVALID, INVALID, '', KEPT),
        "N0": (INVALID, INVALID, '', NULLED),
        "batch0": (INVALID, INVALID, '', NULLED),
        "n65": {"f32": (UNSUPPORTED, UNSUPPORTED, 'S gamma Ginv', NULLED), "f64": (UNSUPPORTED, UNSUPPORTED, '', NULLED)},
        "kind3": (INVALID, INVALID, 'S gamma Ginv', KEPT),
        "nu0": (INVALID, INVALID, '', NULLED),
        "schur-limit": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
    },
    "kkt_step_reg": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-G": (INVALID, INVALID, '', NULLED),
        "null-C": (INVALID, INVALID, '', NULLED),
        "null-g": (INVALID, INVALID, '', NULLED),
        "null-c": (INVALID, INVALID, '', NULLED),
        "null-rho": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', KEPT),
        "null-Ginv": (INVALID, INVALID, '', KEPT),
        "null-Pinv": (INVALID, INVALID, 'S gamma Ginv', KEPT),
        "null-lam": (INVALID, INVALID, 'S gamma Ginv', NULLED),
        "null-it": (INVALID, INVALID, 'S gamma Ginv', NULLED),
        "null-z": (INVALID, INVALID, '', KEPT),
        "N0": (INVALID, INVALID, '', NULLED),
        "batch0": (INVALID, INVALID, '', NULLED),
        "n65": {"f32": (UNSUPPORTED, UNSUPPORTED, 'S gamma Ginv', NULLED), "f64": (UNSUPPORTED, UNSUPPORTED, '', NULLED)},
        "kind3": (INVALID, INVALID, 'S gamma Ginv', KEPT),
        "nu0": (INVALID, INVALID, '', NULLED),
        "schur-limit": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
    },
    "kkt_resolve": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-Ginv": (INVALID, INVALID, '', KEPT),
        "null-C": (INVALID, INVALID, '', KEPT),
        "null-g": (INVALID, INVALID, '', KEPT),
        "null-c": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', KEPT),
        "null-lam": (INVALID, INVALID, '', KEPT),
        "null-it": (INVALID, INVALID, '', KEPT),
        "null-z": (INVALID, INVALID, '', KEPT),
        "N0": (INVALID, INVALID, '', KEPT),
        "batch0": (INVALID, INVALID, '', KEPT),
        "n65": {"f32": (UNSUPPORTED, UNSUPPORTED, 'gamma', NULLED), "f64": (UNSUPPORTED, UNSUPPORTED, '', KEPT)},
        "nu0": (INVALID, INVALID, '', KEPT),
        "schur-limit": (UNSUPPORTED, UNSUPPORTED, '', KEPT),
    },
    "kkt_resolve_shared": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-Ginv": (INVALID, INVALID, '', KEPT),
        "null-C": (INVALID, INVALID, '', KEPT),
        "null-g": (INVALID, INVALID, '', KEPT),
        "null-c": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', KEPT),
        "null-lam": (INVALID, INVALID, '', KEPT),
        "null-it": (INVALID, INVALID, '', KEPT),
        "null-z": (INVALID, INVALID, '', KEPT),
        "N0": (INVALID, INVALID, '', KEPT),
        "batch0": (INVALID, INVALID, '', KEPT),
        "n65": {"f32": (UNSUPPORTED, UNSUPPORTED, 'gamma', NULLED), "f64": (UNSUPPORTED, UNSUPPORTED, '', KEPT)},
        "nu0": (INVALID, INVALID, '', KEPT),
        "schur-limit": (UNSUPPORTED, UNSUPPORTED, '', KEPT),
        "beyond-one-wg": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
    },
    "kkt_backward": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-Ginv": (INVALID, INVALID, '', KEPT),
        "null-C": (INVALID, INVALID, '', KEPT),
        "null-gz": (INVALID, INVALID, '', KEPT),
        "null-nglam": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', KEPT),
        "null-z": (INVALID, INVALID, '', KEPT),
        "null-lam": (INVALID, INVALID, '', KEPT),
        "null-az": (INVALID, INVALID, '', KEPT),
        "null-alam": (INVALID, INVALID, '', KEPT),
        "null-it": (INVALID, INVALID, '', KEPT),
        "N0": (INVALID, INVALID, '', KEPT),
        "batch0": (INVALID, INVALID, '', KEPT),
        "n65": {"f32": (UNSUPPORTED, UNSUPPORTED, '', NULLED), "f64": (UNSUPPORTED, UNSUPPORTED, '', KEPT)},
        "null-gG+gC": (INVALID, INVALID, '', KEPT),
        "nu0": (INVALID, INVALID, '', KEPT),
        "schur-limit": (UNSUPPORTED, UNSUPPORTED, '', KEPT),
    },
    "kkt_backward_shared": {
        "null-h": (INVALID, INVALID, '', KEPT),
        "null-Ginv": (INVALID, INVALID, '', KEPT),
        "null-C": (INVALID, INVALID, '', KEPT),
        "null-gz": (INVALID, INVALID, '', KEPT),
        "null-nglam": (INVALID, INVALID, '', KEPT),
        "null-S": (INVALID, INVALID, '', KEPT),
        "null-gamma": (INVALID, INVALID, '', KEPT),
        "null-z": (INVALID, INVALID, '', KEPT),
        "null-lam": (INVALID, INVALID, '', KEPT),
        "null-az": (INVALID, INVALID, '', KEPT),
        "null-alam": (INVALID, INVALID, '', KEPT),
        "null-it": (INVALID, INVALID, '', KEPT),
        "N0": (INVALID, INVALID, '', KEPT),
        "batch0": (INVALID, INVALID, '', KEPT),
        "n65": {"f32": (UNSUPPORTED, UNSUPPORTED, '', NULLED), "f64": (UNSUPPORTED, UNSUPPORTED, '', KEPT)},
        "null-gG+gC": (INVALID, INVALID, '', KEPT),
        "nu0": (INVALID, INVALID, '', KEPT),
        "schur-limit": (UNSUPPORTED, UNSUPPORTED, '', KEPT),
        "beyond-one-wg": (UNSUPPORTED, UNSUPPORTED, '', NULLED),
    },
}


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def make_buffers():
    """Per precision: what the calls read (zeros, and well-posed blocks of the good shape for G, so that a formation that does run
    before a refusal inverts something), and one sentinel-filled array per output."""
    out = {}
    for suf, tt in (("f32", torch.float32), ("f64", torch.float64)):
        ins = torch.zeros(LARGE_ELEMS, dtype=tt, device="cuda")
        G = torch.zeros(1 << 12, dtype=tt, device="cuda")
        knot = torch.cat([torch.eye(NX, dtype=tt).flatten(), torch.eye(NU, dtype=tt).flatten()]).cuda()
        G[:knot.numel() * N * BATCH] = knot.repeat(N * BATCH)
        rho = torch.ones(64, dtype=tt, device="cuda")
        outs = {k: torch.full((LARGE_ELEMS if k in LARGE else SMALL_ELEMS,), 777.0, dtype=tt, device="cuda")
                for k in ("S", "Pinv", "Ginv", "gG", "gC", "gamma", "lam", "r", "p", "z", "az", "alam")}
        outs["it"] = torch.full((64,), 777, dtype=torch.int32, device="cuda")
        outs["fl"] = torch.full((64,), 77, dtype=torch.uint8, device="cuda")
        out[suf] = ins, G, rho, outs
    return out


@pytest.fixture(scope="module")
def buffers():
    return make_buffers()


def written(outs, names):
    """The names of the outputs that no longer hold their sentinel, which is put back."""
    torch.cuda.synchronize()
    flags = torch.stack([(outs[k] != (77 if k == "fl" else 777)).any() for k in names]).tolist()
    hit = [k for k, f in zip(names, flags) if f]
    for k in hit:
        outs[k].fill_(77 if k == "fl" else 777)
    return " ".join(hit)


def observe(lib, h, suf, entry, case, bufs):
    """(status of the direct call, what it wrote, status of graph_create, the graph handle afterwards, what graph_create wrote)."""
    ins, G, rho, outs = bufs
    args, _, outputs, has_nu = ENTRIES[entry]
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    v = {k: P(outs[k]) if k in outputs else P(ins) for k in args if k not in ("tol", "max_iter", "kind")}
    v.update(tol=1e-6, max_iter=10, kind=binding.PINV_STAIR, h=h, n=NX, nu=NU, N=N, batch=BATCH, rho=P(rho))
    if "G" in args:
        v["G"] = P(G)
    if case == "null-gG+gC":
        v["gG"] = v["gC"] = None
    elif case.startswith("null-"):
        v[case[5:]] = None
    elif case == "N0":
        v["N"] = 0
    elif case == "batch0":
        v["batch"] = 0
    elif case == "n65":
        v["n"], v["G"] = 65, P(ins)
    elif case == "kind3":
        v["kind"] = 3
    elif case == "nu0":
        v["nu"] = 0
    elif case == "schur-limit":
        v["n"], v["nu"], v["G"] = SCHUR_LIMIT[suf], SCHUR_LIMIT[suf] // 2, P(ins)
    elif case == "beyond-one-wg":
        v["n"], v["N"], v["batch"] = BEYOND_ONE_WG[suf]
    else:
        raise KeyError(case)
    # (not every entry has argtypes in binding.py: the scalars are converted here)
    u32, real = ctypes.c_uint32, ctypes.c_float if suf == "f32" else ctypes.c_double
    v.update(tol=real(v["tol"]), max_iter=u32(v["max_iter"]), kind=ctypes.c_int(v["kind"]))
    head = (v["h"], u32(v["n"])) + ((u32(v["nu"]),) if has_nu else ()) + (u32(v["N"]), u32(v["batch"]))
    call = head + tuple(v[k] for k in args)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    direct = getattr(lib, f"gbdpcg_{entry}_{suf}")(*call, stream)
    wrote = written(outs, outputs)
    graph = ctypes.c_void_p(0xdead0)
    create = getattr(lib, f"gbdpcg_graph_create_{entry}_{suf}")(*call, ctypes.byref(graph))
    return direct, wrote, create, graph.value, written(outs, outputs)


PARAMS = [pytest.param(e, c, id=f"{e}-{c}") for e in ENTRIES for c in cases(e)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry,case", PARAMS)
def test_call_and_graph_create_refuse_as_recorded(solver, buffers, entry, case, suf):
    direct, wrote, create, graph, wrote_by_create = observe(solver.lib, solver.h, suf, entry, case, buffers[suf])
    print(f"{entry} {case} {suf}: call {direct} wrote [{wrote}], graph_create {create} wrote [{wrote_by_create}], handle {graph}")
    want = EXPECTED[entry][case]
    if isinstance(want, dict):
        want = want[suf]
    assert direct != OK and create != OK, "every case of this table is a refusal"
    assert graph in (None, 0xdead0), "no graph comes back"
    assert (direct, create, wrote, NULLED if graph is None else KEPT) == want
    assert wrote_by_create == "", "a refused graph_create has run nothing"
