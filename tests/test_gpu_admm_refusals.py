"""The refusals of the ADMM iteration, one table for the three families (gbdpcg_admm_step_*, gbdpcg_admm_lin_step_*,
gbdpcg_admm_soc_step_*), their _shared twins and both precisions: for every bad argument set the direct step and its graph-create
twin return a recorded status, the graph handle comes back null and no output array is touched.  Nothing is launched: every call
ends at its refusal.

EXPECTED was recorded ONCE, by running this table against the build of the commit before the three families were given one host
path; it is not derived from the code under test.  It came out the same for the plain and the shared entries and for f32 and f64,
so it is keyed by (family, case) alone and holds (status of the step, status of graph_create)."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
NX, NU, N, BATCH = 4, 3, 5, 2
# the sizes between nu and N, and the good values of a family
SIZES = {"admm": (), "admm_lin": ("mx", "mu"), "admm_soc": ("mx", "mu", "lx", "qx", "lu", "qu")}
GOOD = {"admm": {}, "admm_lin": dict(mx=3, mu=2), "admm_soc": dict(mx=5, mu=4, lx=2, qx=3, lu=0, qu=4)}
STEP_ARGS = ("Ginv", "C", "g", "c", "E", "lo", "hi", "rho", "S", "Pinv", "gamma", "lam", "r", "p", "tol", "max_iter", "it", "fl", "z", "w",
             "y", "gt", "res")
REQUIRED = ("h", "Ginv", "C", "g", "c", "E", "lo", "hi", "rho", "S", "gamma", "lam", "it", "z", "w", "y", "gt", "res")
WRITTEN = ("gamma", "lam", "r", "p", "z", "w", "y", "gt", "res")
# the bad sizes: what is set over the good values
BAD_SIZES = {"nu0": dict(nu=0),
             "no-rows": dict(mx=0, mu=0, lx=0, lu=0),
             "mx65": dict(mx=65, lx=65),           # (no cone rows in the x blocks: the classes fit)
             "lx>mx": dict(lx=6),
             "qx0-with-cone-rows": dict(qx=0),
             "part-cone": dict(qx=2)}


def cases(family):
    out = [f"null-{k}" for k in REQUIRED if k != "E" or family != "admm"] + ["nu0"]
    if family != "admm":
        out += ["no-rows", "mx65"]
    if family == "admm_soc":
        out += ["lx>mx", "qx0-with-cone-rows", "part-cone"]
    return out


EXPECTED = {
    ("admm", "null-h"): (INVALID, INVALID), ("admm", "null-Ginv"): (INVALID, INVALID), ("admm", "null-C"): (INVALID, INVALID),
    ("admm", "null-g"): (INVALID, INVALID), ("admm", "null-c"): (INVALID, INVALID), ("admm", "null-lo"): (INVALID, INVALID),
    ("admm", "null-hi"): (INVALID, INVALID), ("admm", "null-rho"): (INVALID, INVALID), ("admm", "null-S"): (INVALID, INVALID),
    ("admm", "null-gamma"): (INVALID, INVALID), ("admm", "null-lam"): (INVALID, INVALID), ("admm", "null-it"): (INVALID, INVALID),
    ("admm", "null-z"): (INVALID, INVALID), ("admm", "null-w"): (INVALID, INVALID), ("admm", "null-y"): (INVALID, INVALID),
    ("admm", "null-gt"): (INVALID, INVALID), ("admm", "null-res"): (INVALID, INVALID), ("admm", "nu0"): (INVALID, INVALID),
    ("admm_lin", "null-h"): (INVALID, INVALID), ("admm_lin", "null-Ginv"): (INVALID, INVALID),
    ("admm_lin", "null-C"): (INVALID, INVALID), ("admm_lin", "null-g"): (INVALID, INVALID), ("admm_lin", "null-c"): (INVALID, INVALID),
    ("admm_lin", "null-E"): (INVALID, INVALID), ("admm_lin", "null-lo"): (INVALID, INVALID),
    ("admm_lin", "null-hi"): (INVALID, INVALID), ("admm_lin", "null-rho"): (INVALID, INVALID),
    ("admm_lin", "null-S"): (INVALID, INVALID), ("admm_lin", "null-gamma"): (INVALID, INVALID),
    ("admm_lin", "null-lam"): (INVALID, INVALID), ("admm_lin", "null-it"): (INVALID, INVALID),
    ("admm_lin", "null-z"): (INVALID, INVALID), ("admm_lin", "null-w"): (INVALID, INVALID), ("admm_lin", "null-y"): (INVALID, INVALID),
    ("admm_lin", "null-gt"): (INVALID, INVALID), ("admm_lin", "null-res"): (INVALID, INVALID), ("admm_lin", "nu0"): (INVALID, INVALID),
    ("admm_lin", "no-rows"): (INVALID, INVALID), ("admm_lin", "mx65"): (UNSUPPORTED, UNSUPPORTED),
    ("admm_soc", "null-h"): (INVALID, INVALID), ("admm_soc", "null-Ginv"): (INVALID, INVALID),
    ("admm_soc", "null-C"): (INVALID, INVALID), ("admm_soc", "null-g"): (INVALID, INVALID), ("admm_soc", "null-c"): (INVALID, INVALID),
    ("admm_soc", "null-E"): (INVALID, INVALID), ("admm_soc", "null-lo"): (INVALID, INVALID),
    ("admm_soc", "null-hi"): (INVALID, INVALID), ("admm_soc", "null-rho"): (INVALID, INVALID),
    ("admm_soc", "null-S"): (INVALID, INVALID), ("admm_soc", "null-gamma"): (INVALID, INVALID),
    ("admm_soc", "null-lam"): (INVALID, INVALID), ("admm_soc", "null-it"): (INVALID, INVALID),
    ("admm_soc", "null-z"): (INVALID, INVALID), ("admm_soc", "null-w"): (INVALID, INVALID), ("admm_soc", "null-y"): (INVALID, INVALID),
    ("admm_soc", "null-gt"): (INVALID, INVALID), ("admm_soc", "null-res"): (INVALID, INVALID), ("admm_soc", "nu0"): (INVALID, INVALID),
    ("admm_soc", "no-rows"): (INVALID, INVALID), ("admm_soc", "mx65"): (UNSUPPORTED, UNSUPPORTED),
    ("admm_soc", "lx>mx"): (INVALID, INVALID), ("admm_soc", "qx0-with-cone-rows"): (INVALID, INVALID),
    ("admm_soc", "part-cone"): (INVALID, INVALID),
}


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def arrays():
    """Per precision: zeros to read, and one guarded block that every output points into."""
    out = {}
    for suf, tt in (("f32", torch.float32), ("f64", torch.float64)):
        ins = torch.zeros(1 << 12, dtype=tt, device="cuda")
        rho = torch.ones(BATCH, dtype=tt, device="cuda")
        guard = torch.full((len(WRITTEN) << 12,), 777.0, dtype=tt, device="cuda")
        it = torch.full((BATCH,), 777, dtype=torch.int32, device="cuda")
        fl = torch.full((BATCH,), 77, dtype=torch.uint8, device="cuda")
        out[suf] = ins, rho, guard, it, fl
    return out


def run_case(lib, h, suf, family, shared, case, arrays):
    """(status of the step, status of graph_create, the graph handle afterwards)."""
    ins, rho, guard, it, fl = arrays
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    v = {k: P(ins) for k in ("Ginv", "C", "g", "c", "E", "lo", "hi", "S", "Pinv")}
    v.update({k: P(guard[i << 12:]) for i, k in enumerate(WRITTEN)})
    v.update(rho=P(rho), it=P(it), fl=P(fl), tol=1e-6, max_iter=10, h=h, nx=NX, nu=NU, N=N, batch=BATCH, **GOOD[family])
    if case.startswith("null-"):
        v[case[5:]] = None
    else:
        v.update({k: x for k, x in BAD_SIZES[case].items() if k in v})
    head = (v["h"], v["nx"], v["nu"]) + tuple(v[k] for k in SIZES[family]) + (v["N"], v["batch"])
    args = head + tuple(v[k] for k in STEP_ARGS if k != "E" or family != "admm")
    name = f"{family}_step" + ("_shared" if shared else "")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    graph = ctypes.c_void_p(0xdead0)
    direct = getattr(lib, f"gbdpcg_{name}_{suf}")(*args, stream)
    create = getattr(lib, f"gbdpcg_graph_create_{name}_{suf}")(*args, ctypes.byref(graph))
    return direct, create, graph.value


PARAMS = [pytest.param(f, c, id=f"{f}-{c}") for f in SIZES for c in cases(f)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
@pytest.mark.parametrize("family,case", PARAMS)
def test_step_and_graph_create_refuse_alike_and_write_nothing(solver, arrays, family, case, shared, suf):
    direct, create, graph = run_case(solver.lib, solver.h, suf, family, shared, case, arrays[suf])
    print(f"{family} {case} {'shared' if shared else 'plain'} {suf}: step {direct}, graph_create {create}, handle {graph}")
    assert (direct, create) == EXPECTED[family, case]
    assert not graph, "the graph handle comes back null"
    torch.cuda.synchronize()
    _, _, guard, it, fl = arrays[suf]
    assert bool((guard == 777.0).all()) and bool((it == 777).all()) and bool((fl == 77).all())
