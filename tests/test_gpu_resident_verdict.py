"""Symmetric mode 2 with the symmetry test inside the CU-resident solve (pcg_resident_sym.hip, VERIFY = true).

At n = 14 fp32 with 16-byte aligned matrices the default mode no longer launches a test kernel: the resident kernel takes
every problem, compares its resident R_k rows with L_{k+1} of S and Phi^-1 bit for bit, and writes a problem only when
it passes; the general launch that follows takes the rest from the caller's warm start.  So, bit for bit:

    a problem that is symmetric in storage (L_{k+1} == R_k^T for every k <= N-2, both matrices) == mode 1 on it,
    any other problem                                                                       == mode 0 on it,

lambda, r, p, iters and max_iter_exit alike.  Which problems are symmetric is decided here on the host, from the bits.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding, synth  # noqa: E402

pytestmark = pytest.mark.gpu

n = 14
NN = n * n


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.set_symmetric(2)
    s.close()


def batch_of(solver, N, B, pool=8, seed=4100):
    """B problems from a pool of Gen(14, N, seed + i): S and gamma on the device, stair Phi^-1 formed there (exactly
    symmetric in storage); gamma scaled per problem so that no two problems are the same."""
    g = synth.gen_torch_seeded(n, N, 0, pool, "cuda", torch.float32, seed=seed)
    idx = torch.arange(B, device="cuda") % pool
    S = g["S"][idx].contiguous()
    gamma = (g["gamma"][idx] * (1.0 + 0.003 * torch.arange(B, device="cuda", dtype=torch.float32))[:, None]).contiguous()
    P = solver.form_pinv(n, N, B, S, binding.PINV_STAIR)
    return S, P, gamma


def l_index(N, k, r, c):
    """Flat index of L_{k+1}(c, r) (column-major blocks), the transpose partner of R_k(r, c)."""
    return (k + 1) * 3 * NN + r * n + c


def r_index(N, k, r, c):
    return k * 3 * NN + 2 * NN + c * n + r


def to_i32(bits):
    return int(np.array([bits], dtype=np.uint32).view(np.int32)[0])


def flip_bit(M, b, i, bit=0):
    v = M[b, i:i + 1].view(torch.int32)
    v ^= to_i32(1 << bit)


def set_bits(M, b, i, bits):
    M[b, i:i + 1].view(torch.int32).fill_(to_i32(bits))


def host_symmetric(M, N):
    """Per problem: L_{k+1} == R_k^T bit for bit for every k <= N - 2 (what check_symmetric_pair_kernel decides)."""
    m = M.view(torch.int32).reshape(M.shape[0], N, 3, n, n)   # [b, k, block, col, row] (column-major blocks)
    if N < 2:
        return torch.ones(M.shape[0], dtype=torch.bool, device=M.device)
    R = m[:, :N - 1, 2]                      # R_k[col c][row r]
    L = m[:, 1:, 0]                          # L_{k+1}[col][row]
    return (R == L.transpose(-1, -2)).flatten(1).all(dim=1)


def solve(solver, mode, N, B, S, P, gamma, lam0=None, tol=0.0, max_iter=25):
    solver.set_symmetric(mode)
    try:
        lam = torch.zeros_like(gamma) if lam0 is None else lam0.clone()
        r = torch.full_like(gamma, float("nan"))
        p = torch.full_like(gamma, float("nan"))
        it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        fl = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
        solver.solve(n, N, B, S, P, gamma, lam, r, p, tol=tol, max_iter=max_iter, iters=it, max_iter_exit=fl)
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    return {"lam": lam, "r": r, "p": p, "it": it, "fl": fl}


def same_rows(a, b):
    """Per problem: every output bit-identical."""
    eq = torch.ones(a["it"].shape[0], dtype=torch.bool, device="cuda")
    for k in ("lam", "r", "p"):
        eq &= (a[k].view(torch.int32) == b[k].view(torch.int32)).all(dim=1)
    return eq & (a["it"] == b["it"]) & (a["fl"] == b["fl"])


def check_against_modes(solver, N, B, S, P, gamma, expect_sym=None, **kw):
    sym = host_symmetric(S, N) & host_symmetric(P, N)
    if expect_sym is not None:
        assert torch.equal(sym.cpu(), torch.as_tensor(expect_sym)), "the corruptions do not do what the test meant"
    m2 = solve(solver, 2, N, B, S, P, gamma, **kw)
    m1 = solve(solver, 1, N, B, S, P, gamma, **kw)
    m0 = solve(solver, 0, N, B, S, P, gamma, **kw)
    ok1, ok0 = same_rows(m2, m1), same_rows(m2, m0)
    bad = torch.nonzero(~torch.where(sym, ok1, ok0)).flatten().tolist()
    assert not bad, f"N={N} B={B}: problems {bad[:10]} (symmetric: {sym[bad[:10]].tolist()})"
    return sym, m0, m1, m2


def corrupt_cases(S, P, N):
    """One problem per case (problem index = 3 * case + 1); returns the expected verdicts' False entries."""
    cases = [
        (S, 0, 0, 0, 0), (P, 0, 0, 3, 5),                 # k = 0, both matrices
        (S, N - 2, 6, 13, 23), (P, N - 2, 5, 2, 9),       # k = N - 2
        (S, 10, 3, 7, 4), (S, 11, 2, 6, 30),              # even k, odd k
        (P, 10, 4, 8, 1), (P, 11, 1, 0, 17),              # Phi^-1 k0 tile (registers), k1 tile (LDS)
        (S, 41, 13, 5, 22), (P, 57, 13, 12, 0),           # column 2rp + 1 at rp = 6
        (P, 2 * 12 + 1, 6, 11, 31),                       # an LDS-resident (k1) Phi^-1 piece, sign bit
    ]
    bad = []
    for j, (M, k, r, c, bit) in enumerate(cases):
        b = 3 * j + 1
        flip_bit(M, b, l_index(N, k, r, c), bit)
        bad.append(b)
    b = 3 * len(cases) + 1                                # +0.0 in R, -0.0 in L
    S[b, r_index(N, 20, 4, 9)] = 0.0
    set_bits(S, b, l_index(N, 20, 4, 9), 0x80000000)
    bad.append(b)
    b += 3                                                # two NaNs with different payloads (Phi^-1)
    set_bits(P, b, r_index(N, 33, 9, 3), 0x7fc00001)
    set_bits(P, b, l_index(N, 33, 9, 3), 0x7fc00002)
    bad.append(b)
    b += 3                                                # the same NaN on both sides: symmetric in storage
    set_bits(P, b, r_index(N, 34, 9, 3), 0x7fc00005)
    set_bits(P, b, l_index(N, 34, 9, 3), 0x7fc00005)
    b += 3                                                # R_{N-1} and L_0 are not part of the relation
    flip_bit(S, b, (N - 1) * 3 * NN + 2 * NN + 17, 3)
    flip_bit(P, b, (N - 1) * 3 * NN + 2 * NN + 100, 0)
    b += 3
    flip_bit(S, b, 5, 2)
    flip_bit(P, b, NN - 1, 0)
    return bad


@pytest.mark.parametrize("lam_seed,tol,max_iter", [(None, 0.0, 25), (3, 1e-6, 60)])
def test_single_bit_corruptions(solver, lam_seed, tol, max_iter):
    N, B = 128, 300
    S, P, gamma = batch_of(solver, N, B)
    bad = corrupt_cases(S, P, N)
    expect = np.ones(B, dtype=bool)
    expect[bad] = False
    lam0 = None
    if lam_seed is not None:
        gen = torch.Generator(device="cuda").manual_seed(lam_seed)
        lam0 = 0.1 * torch.randn(gamma.shape, device="cuda", generator=gen)
    sym, m0, m1, m2 = check_against_modes(solver, N, B, S, P, gamma, expect_sym=expect, lam0=lam0, tol=tol, max_iter=max_iter)
    # the rejected problems really did take the other kernel (mode 1 on them differs from mode 0)
    assert not same_rows(m1, m0)[bad[:-2]].any()


@pytest.mark.parametrize("N", [1, 2, 3, 64, 127, 128])
def test_shapes_and_batches(solver, N):
    for B in (200, 257, 1024, 1300):
        S, P, gamma = batch_of(solver, N, B, seed=4200 + N)
        if N >= 2:
            for j, b in enumerate(range(3, B, 97)):          # every 97th problem: one bit of one L block
                M = S if j % 2 else P
                k = (7 * j) % (N - 1)
                flip_bit(M, b, l_index(N, k, (3 * j) % n, (5 * j) % n), j % 23)
        check_against_modes(solver, N, B, S, P, gamma, max_iter=25)


@pytest.mark.parametrize("tol,max_iter", [(0.0, 0), (0.0, 1), (0.0, 3), (1e30, 25)])
def test_early_exit(solver, tol, max_iter):
    """The verdict is complete whatever the iteration count: no iteration, one, three, and an exit at the first test."""
    N, B = 128, 300
    S, P, gamma = batch_of(solver, N, B, seed=4300)
    bad = corrupt_cases(S, P, N)
    expect = np.ones(B, dtype=bool)
    expect[bad] = False
    check_against_modes(solver, N, B, S, P, gamma, expect_sym=expect, tol=tol, max_iter=max_iter)


def test_graph_follows_the_data(solver):
    """A captured mode-2 solve, replayed while one problem's storage flips between symmetric and not on the device: every
    replay takes the verdict of the data it finds."""
    N, B = 128, 300
    S, P, gamma = batch_of(solver, N, B, seed=4400)
    b, i = 77, l_index(N, 45, 6, 13)
    clean = S[b, i].clone()
    ref_sym = solve(solver, 2, N, B, S, P, gamma)
    flip_bit(S, b, i, 4)
    ref_bad = solve(solver, 2, N, B, S, P, gamma)
    ref_bad0 = solve(solver, 0, N, B, S, P, gamma)
    assert same_rows(ref_bad, ref_bad0)[b] and not same_rows(ref_bad, ref_sym)[b]
    S[b, i] = clean
    lam = torch.zeros_like(gamma)
    r, p = torch.empty_like(gamma), torch.empty_like(gamma)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    solver.reserve(4, n, N, B)
    gr = solver.graph_solve(n, N, B, S, P, gamma, lam, r, p, 0.0, 25, it, fl)
    try:
        for rep in range(6):
            corrupt = rep % 2 == 1
            if corrupt:
                flip_bit(S, b, i, 4)
            else:
                S[b, i] = clean
            lam.zero_()
            r.fill_(float("nan"))
            gr.launch()
            torch.cuda.synchronize()
            ref = ref_bad if corrupt else ref_sym
            assert same_rows({"lam": lam, "r": r, "p": p, "it": it, "fl": fl}, ref).all(), rep
    finally:
        gr.close()


def test_eight_byte_aligned_fallback(solver):
    """Matrices 8- but not 16-byte aligned keep the test launch and the direct-load kernel: same bit-identities."""
    N, B = 128, 300
    S0, P0, gamma = batch_of(solver, N, B, seed=4500)
    size = S0.numel()
    bufS = torch.empty(size + 4, dtype=torch.float32, device="cuda")
    bufP = torch.empty(size + 4, dtype=torch.float32, device="cuda")
    S = bufS[2:2 + size].view(B, -1)
    P = bufP[2:2 + size].view(B, -1)
    assert S.data_ptr() % 16 == 8 and P.data_ptr() % 16 == 8
    S.copy_(S0)
    P.copy_(P0)
    bad = corrupt_cases(S, P, N)
    expect = np.ones(B, dtype=bool)
    expect[bad] = False
    check_against_modes(solver, N, B, S, P, gamma, expect_sym=expect)
