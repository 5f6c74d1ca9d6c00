"""The reject count of the verifying resident solve and the early way out of the general launch behind it (symmetric mode 2,
n = 14, fp32).

The verifying launch counts the problems it rejects in a device word behind the handle's verdict bytes; the general launch that
follows reads the word first and returns at once when it is 0, and otherwise solves the rejected problems and puts the word back
to 0 as it ends.  Checked here, eager and as a captured graph replayed three times (a stale count would show from the second
replay on), for N = 2 (one pair of block-rows), 5 (an odd count, one dead slot) and 128 (the full geometry):

  * every problem against the CPU oracle on the same storage (tolerances of test_gpu_parity.py: lambda to 1e-6 norm-wise,
    equal iteration counts),
  * a problem whose Phi^-1 is asymmetric in ONE element of L_1 bit for bit what a mode-0 solve gives it (lambda, r, p, iters, flag),
  * the verdict bytes against the planted pattern, and both reject words back at 0 after every solve and every replay,
  * the cluster path's hand-off state: a launch that leaves early takes no launch number, and a mode-0 cluster solve right
    after it on the same handle matches the oracle.

Which launches a case reaches follows from the shape alone (api_solve.hip): the verifying launch exists where the general kernel is
the cluster kernel (N > 72 at this block size) and the batch is more than one round of clusters (2 CUs per problem at N = 128).
The other cases (N = 2, 5; three problems at N = 128) are solved by one general launch in mode 2: no verdict byte is written for
them, which is asserted as such, and everything else is checked all the same.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding, synth  # noqa: E402

pytestmark = pytest.mark.gpu

n = 14
NN = n * n
F32_TOL = 1e-6          # test_gpu_parity.py
TOL, MAX_ITER = 1e-6, 60
SENTINEL = 7            # what a verdict byte holds here when no launch wrote it

# (batch, problems made asymmetric): no reject; the middle one of three; more than one round of 256 workgroups, a partial last
# round and both ends
BATCHES = [(3, ()), (3, (1,)), (300, (0, 255, 256, 299))]
HORIZONS = [2, 5, 128]


class Dev:
    """Device words the handle keeps to itself, read and written with the HIP runtime directly."""

    def __init__(self, solver):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.fn = solver.lib.gbdpcg_internal_state
        self.fn.restype = ctypes.c_void_p
        self.fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.h = solver.h

    def ptr(self, which):
        p = self.fn(self.h, which)
        assert p, f"the handle has no state {which} yet"
        return p

    def read(self, which, offset, dtype, count):
        torch.cuda.synchronize()
        out = np.zeros(count, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr(which) + offset),
                                  ctypes.c_size_t(out.nbytes), 2) == 0
        return out

    def fill_verdicts(self, count):
        torch.cuda.synchronize()
        assert self.hip.hipMemset(ctypes.c_void_p(self.ptr(0)), SENTINEL, ctypes.c_size_t(count)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def verdicts(self, count):
        return self.read(0, 0, np.uint8, count)

    def reject_words(self):
        return self.read(1, 0, np.uint32, 2).tolist()

    def launch_number(self):
        return int(self.read(2, 31 * 8, np.uint64, 1)[0])


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.set_symmetric(2)
    s.close()


@pytest.fixture(scope="module")
def dev(solver):
    return Dev(solver)


def host_symmetric(M, N):
    """Per problem: L_{k+1} == R_k^T bit for bit for every k <= N - 2."""
    m = M.view(torch.int32).reshape(M.shape[0], N, 3, n, n)   # [b, k, block, col, row]
    return (m[:, :N - 1, 2] == m[:, 1:, 0].transpose(-1, -2)).flatten(1).all(dim=1)


_cases = {}


def case(solver, orc, N, B, rejects):
    """The batch (on the device) and its oracle solution, made once per case and left unchanged."""
    key = (N, B, rejects)
    if key not in _cases:
        pool = min(B, 8)
        g = synth.gen_torch_seeded(n, N, 0, pool, "cuda", torch.float32, seed=5100 + N)
        idx = torch.arange(B, device="cuda") % pool
        S = g["S"][idx].contiguous()
        gamma = (g["gamma"][idx] * (1.0 + 0.003 * torch.arange(B, device="cuda", dtype=torch.float32))[:, None]).contiguous()
        P = solver.form_pinv(n, N, B, S, binding.PINV_STAIR)
        for b in rejects:   # one element of L_1 of Phi^-1, last mantissa bit: L_1(c, r) at 3 n^2 + r n + c
            P[b, 3 * NN + 5 * n + 3:3 * NN + 5 * n + 4].view(torch.int32).bitwise_xor_(1)
        torch.cuda.synchronize()
        sym = (host_symmetric(S, N) & host_symmetric(P, N)).cpu().numpy()
        expect = np.ones(B, dtype=bool)
        expect[list(rejects)] = False
        assert np.array_equal(sym, expect), "the planted asymmetries are not what the storage shows"
        ob = orc.pcg_batch(n, N, B, S.cpu().numpy(), P.cpu().numpy(), gamma.cpu().numpy(), tol=TOL, max_iter=MAX_ITER)
        _cases[key] = (S, P, gamma, ob)
    return _cases[key]


def buffers(gamma):
    B = gamma.shape[0]
    return {"lam": torch.zeros_like(gamma), "r": torch.full_like(gamma, float("nan")), "p": torch.full_like(gamma, float("nan")),
            "it": torch.full((B,), -1, dtype=torch.int32, device="cuda"), "fl": torch.full((B,), 7, dtype=torch.uint8, device="cuda")}


def eager(solver, mode, N, S, P, gamma):
    o = buffers(gamma)
    solver.set_symmetric(mode)
    try:
        solver.solve(n, N, gamma.shape[0], S, P, gamma, o["lam"], o["r"], o["p"], tol=TOL, max_iter=MAX_ITER, iters=o["it"],
                     max_iter_exit=o["fl"])
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    return o


def same_rows(a, b):
    eq = torch.ones(a["it"].shape[0], dtype=torch.bool, device="cuda")
    for k in ("lam", "r", "p"):
        eq &= (a[k].view(torch.int32) == b[k].view(torch.int32)).all(dim=1)
    return (eq & (a["it"] == b["it"]) & (a["fl"] == b["fl"])).cpu().numpy()


def check_oracle(o, ob, what):
    lam = o["lam"].cpu().numpy().astype(np.float64)
    err = np.linalg.norm(lam - ob["lambda_"], axis=1) / np.linalg.norm(ob["lambda_"], axis=1)
    print(f"{what}: max relative error of lambda {err.max():.3e}, iterations {o['it'].min().item()}..{o['it'].max().item()}")
    assert np.array_equal(o["it"].cpu().numpy(), ob["iters"].astype(np.int32)), what
    assert o["fl"].sum().item() == 0 and err.max() < F32_TOL, (what, err.max())


def verifies(solver, N, B):
    """Does the default mode reach the verifying launch?  (module docstring)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    members = solver.cluster_members(4, n, N)
    return N > 72 and members != 0 and B * members > cus


def check_verdicts(dev, solver, N, B, rejects, what):
    v = dev.verdicts(B)
    if verifies(solver, N, B):
        expect = np.ones(B, dtype=np.uint8)
        expect[list(rejects)] = 0
        assert np.array_equal(v, expect), (what, np.nonzero(v != expect)[0][:10].tolist())
    else:
        assert (v == SENTINEL).all(), (what, "a verdict was written where no verifying launch is expected")
    assert dev.reject_words() == [0, 0], (what, "the reject words are not back at 0")


@pytest.mark.parametrize("B,rejects", BATCHES, ids=["3-none", "3-middle", "300-ends"])
@pytest.mark.parametrize("N", HORIZONS)
def test_rejects_eager_and_replayed(solver, dev, orc, N, B, rejects):
    S, P, gamma, ob = case(solver, orc, N, B, rejects)
    solver.reserve(4, n, N, B)
    m0 = eager(solver, 0, N, S, P, gamma)
    dev.fill_verdicts(B)
    m2 = eager(solver, 2, N, S, P, gamma)
    check_verdicts(dev, solver, N, B, rejects, "eager")
    check_oracle(m2, ob, f"N={N} B={B} eager")
    if rejects:
        assert same_rows(m2, m0)[list(rejects)].all(), "a rejected problem is not what mode 0 gives it"
    o = buffers(gamma)
    gr = solver.graph_solve(n, N, B, S, P, gamma, o["lam"], o["r"], o["p"], TOL, MAX_ITER, o["it"], o["fl"])
    try:
        for rep in range(3):
            o["lam"].zero_()
            o["r"].fill_(float("nan"))
            o["p"].fill_(float("nan"))
            o["it"].fill_(-1)
            o["fl"].fill_(7)
            dev.fill_verdicts(B)
            gr.launch()
            torch.cuda.synchronize()
            check_verdicts(dev, solver, N, B, rejects, f"replay {rep}")
            bad = np.nonzero(~same_rows(o, m2))[0]
            assert bad.size == 0, f"replay {rep}: problems {bad[:10].tolist()} differ from the eager solve"
        check_oracle(o, ob, f"N={N} B={B} replayed")
    finally:
        gr.close()


def test_cluster_solve_right_after_an_early_exit(solver, dev, orc):
    """A general launch that leaves early takes no launch number and leaves the hand-off slots alone; the next launch that owns
    problems -- a plain mode-0 cluster solve on the same handle -- gets its number and matches the oracle."""
    N, B = 128, 300
    assert solver.cluster_members(4, n, N) == 2 and verifies(solver, N, B)
    S, P, gamma, ob = case(solver, orc, N, B, ())
    solver.reserve(4, n, N, B)
    before = dev.launch_number()
    for _ in range(2):
        m2 = eager(solver, 2, N, S, P, gamma)
    assert dev.launch_number() == before, "a launch that owned nothing and left early took a launch number"
    assert dev.reject_words() == [0, 0]
    check_oracle(m2, ob, "mode 2, nothing rejected")
    m0 = eager(solver, 0, N, S, P, gamma)
    assert dev.launch_number() == before + 1
    check_oracle(m0, ob, "mode 0 right after the early exit")
    # ... and a general launch that does own problems, behind a verifying launch, takes a number as ever
    Sr, Pr, gr_, obr = case(solver, orc, N, B, (0, 255, 256, 299))
    mr = eager(solver, 2, N, Sr, Pr, gr_)
    assert dev.launch_number() == before + 2 and dev.reject_words() == [0, 0]
    check_oracle(mr, obr, "mode 2 with rejects after that")
