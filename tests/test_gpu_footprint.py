"""What a solve touches, and what can reach it from outside its own problem.

The other GPU files ask whether a kernel, given well-formed inputs in tensors of their own, reproduces the CPU oracle.  This
one compares every kernel family WITH ITSELF, same data in other surroundings, and demands bit-identity:

  A  the same problems once in tensors of their own (corner blocks L_0 / R_{N-1} zero, as the generator leaves them) and once
     as views into one arena filled with NaN (float arrays) or a byte pattern (iters, max_iter_exit), a guard of at least one
     whole problem and 4 KiB on both sides of every array, NaN in L_0 and R_{N-1} of S and Phi^-1 of every problem.  Same
     outputs bit for bit, no guard byte changed, S / Phi^-1 / gamma untouched, and the tight run equal to the oracle.
     Where the caller asserts symmetry (mode 1) every L block is NaN: the [D|R] kernels never read one, which also proves
     that such a kernel ran.
  B  a degenerate problem (gamma = 0; NaN / +Inf in gamma; NaN in a D block of S and, in the symmetric modes, in a
     mirrored pair of Phi^-1) changes no bit of its neighbours, runs to max_iter with the flag set and lambda non-finite
     everywhere (pcg.cuh:169,195: alpha = 0/0, |NaN| < tol is false), and leaves nothing behind in the handle.
  C  a permutation of the batch permutes the outputs.

Which kernel a case reaches is asserted (never skipped) from what the C ABI tells -- gbdpcg_choose_path,
gbdpcg_cluster_members, the symmetric mode, the batch against the CU count, the alignment -- and, between the resident
symmetric kernel and the cluster kernel, from the bits.  The horizons of the single-workgroup kernel (pcg_resident.hip) are
pinned through gbdpcg_cluster_members at the first horizon the cluster kernel takes.  Note that stateSize 14, fp32 with
N <= 72 (N = 1, 2 here) is solved by pcg_resident.hip in every symmetric mode, and that pcg_resident_sym.hip needs a
Phi^-1 (without one the problem goes to the cluster kernel): those cases are listed under the family they reach.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding, synth  # noqa: E402

pytestmark = pytest.mark.gpu

AUTO, FUSED, SPLIT, PERSIST, PERSIST_1R = (binding.PATH_AUTO, binding.PATH_FUSED, binding.PATH_SPLIT,
                                           binding.PATH_PERSISTENT, binding.PATH_PERSISTENT_1R)
F32, F64 = np.float32, np.float64
# horizon of pcg_resident.hip per (element size, stateSize): the cluster kernel takes over one knot later (test_cluster_shapes)
RESIDENT_HORIZON = {(4, 14): 72, (4, 8): 128, (4, 13): 32, (8, 12): 40}


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.set_symmetric(2)
    s.set_path(AUTO)
    s.close()


class Case:
    def __init__(self, name, fam, n, N, dt, B, mode=0, path=AUTO, shift=0, pinv=True, tol=1e-6, mi=50, run="ABC", zero=False):
        self.name, self.fam, self.n, self.N, self.dt, self.B = name, fam, n, N, np.dtype(dt), B
        self.mode, self.path, self.shift, self.pinv, self.tol, self.mi, self.run, self.zero = mode, path, shift, pinv, tol, mi, run, zero
        self.es = self.dt.itemsize
        # mode 1 on a kernel that reads [D|R] only: the tight run poisons every L block
        self.no_L = mode == 1 and fam in ("resident_sym", "fused_sym")

    def __repr__(self):
        return self.name


FIX = dict(tol=0.0, mi=6)      # fixed count (warm start in A)
IDENT = dict(pinv=False, tol=0.0, mi=4)
CASES = [
    # pcg_resident_sym.hip, verifying (mode 2, 16-byte aligned, more problems than one round of clusters)
    Case("rsv-128x1300", "resident_sym_verify", 14, 128, F32, 1300, mode=2, zero=True),
    Case("rsv-127x1300-fix", "resident_sym_verify", 14, 127, F32, 1300, mode=2, **FIX),
    # ... plain: the caller's word (mode 1), or mode 2 at 8-byte alignment behind the test launch
    Case("rs-128x1300-m1", "resident_sym", 14, 128, F32, 1300, mode=1, **FIX),
    Case("rs-127x3-m1", "resident_sym", 14, 127, F32, 3, mode=1),
    Case("rs-128x3-m1", "resident_sym", 14, 128, F32, 3, mode=1, zero=True),
    Case("rs-127x3-m1-al8", "resident_sym", 14, 127, F32, 3, mode=1, shift=8, **FIX),
    Case("rs-128x1300-m2-al8", "resident_sym", 14, 128, F32, 1300, mode=2, shift=8),
    # pcg_resident.hip (one workgroup holds the problem); N = 1, 2 of the symmetric table land here.  Up to four workgroups share
    # a compute unit (all but the staged 14 x fp32 form, which has one): the large batches are beyond 4 x CUs
    # (N = 1 always to tolerance: the stair of a single block is its inverse, and a fixed count beyond the exact solve is 0/0)
    Case("res-14x2x1300-m2", "resident", 14, 2, F32, 1300, mode=2, **FIX),
    Case("res-14x1x1300-m2", "resident", 14, 1, F32, 1300, mode=2),
    Case("res-14x2x3-m1", "resident", 14, 2, F32, 3, mode=1, **FIX),
    Case("res-14x1x3-m1", "resident", 14, 1, F32, 3, mode=1),
    Case("res-14x64x1300", "resident", 14, 64, F32, 1300, zero=True),
    Case("res-14x64x1300-al8", "resident", 14, 64, F32, 1300, shift=8, **FIX),
    Case("res-14x63x3-ident", "resident", 14, 63, F32, 3, **IDENT),
    Case("res-8x100x1300", "resident", 8, 100, F32, 1300, **FIX),
    Case("res-13x31x5", "resident", 13, 31, F32, 5),
    Case("res-12x40x1300-f64", "resident", 12, 40, F64, 1300),
    # pcg_cluster.hip
    Case("cl-14x128x5", "cluster", 14, 128, F32, 5, zero=True),
    Case("cl-14x128x3-m2", "cluster", 14, 128, F32, 3, mode=2),          # mode 2, one round of clusters: no symmetry test
    Case("cl-14x127x140-fix", "cluster", 14, 127, F32, 140, **FIX),
    Case("cl-14x128x140", "cluster", 14, 128, F32, 140),
    Case("cl-14x128x5-al8", "cluster", 14, 128, F32, 5, shift=8),
    Case("cl-14x128x4-ident", "cluster", 14, 128, F32, 4, **IDENT),
    Case("cl-16x64x300-one", "cluster", 16, 64, F32, 300),
    Case("cl-16x2x3-one", "cluster", 16, 2, F32, 3, **FIX),
    Case("cl-18x128x100", "cluster", 18, 128, F32, 100, **FIX),
    Case("cl-14x64x5-f64", "cluster", 14, 64, F64, 5),
    Case("cl-14x300x60", "cluster", 14, 300, F32, 60),
    # pcg_persist.hip: both forms, and the sliced launches
    Case("ps-36x256x1-f64", "persist", 36, 256, F64, 1, zero=True),
    Case("ps-36x256x2-f64", "persist", 36, 256, F64, 2, **FIX),
    Case("ps-36x256x5-f64-sliced", "persist_sliced", 36, 256, F64, 5, mi=100),
    Case("ps-36x256x1-f64-1r", "persist", 36, 256, F64, 1, path=PERSIST_1R),
    Case("ps-36x37x3-f64-1r", "persist", 36, 37, F64, 3, path=PERSIST_1R, **FIX),
    Case("ps-14x200x1", "persist", 14, 200, F32, 1, path=PERSIST),
    Case("ps-36x2x1-f64", "persist", 36, 2, F64, 1, path=PERSIST, **FIX),
    Case("ps-36x1x2-f64", "persist", 36, 1, F64, 2, path=PERSIST),
    Case("ps-36x64x1-f64-ident", "persist", 36, 64, F64, 1, **IDENT),
    # pcg_fused.hip, general streaming: specialised (20, 24) and runtime (25, 37) block sizes.  The launch puts up to four
    # workgroups on a compute unit (32 / 8 waves): a workgroup takes a second problem only beyond 4 x CUs problems
    Case("fu-20x64x1300", "fused", 20, 64, F32, 1300, zero=True),
    Case("fu-24x33x1300-fix", "fused", 24, 33, F32, 1300, **FIX),
    Case("fu-25x40x1300", "fused", 25, 40, F32, 1300),
    Case("fu-37x21x1300-fix", "fused", 37, 21, F32, 1300, **FIX),
    Case("fu-20x1x1300", "fused", 20, 1, F32, 1300),
    Case("fu-24x2x1300-ident", "fused", 24, 2, F32, 1300, **IDENT),
    # (the cluster kernel declines what its tags cannot count, test_cluster_declines_...: the streaming kernel at 14 x 128)
    # (not in B: a degenerate problem runs to max_iter, 600000 iterations here; the family is in B through the cases above)
    Case("fu-14x128x1300-forced", "fused", 14, 128, F32, 1300, path=FUSED, mi=600000, run="AC"),
    # ... symmetric streaming ([D|R] only), beyond the horizons of the resident and cluster kernels
    Case("fs-8x300x520-f64", "fused_sym", 8, 300, F64, 520, mode=1),
    Case("fs-12x171x520-f64", "fused_sym", 12, 171, F64, 520, mode=1, **FIX),
    Case("fs-16x130x520-f64", "fused_sym", 16, 130, F64, 520, mode=1),
    # pcg_split.hip
    Case("sp-36x256x16-f64", "split", 36, 256, F64, 16, **FIX),
    Case("sp-14x16x5-forced", "split", 14, 16, F32, 5, path=SPLIT, zero=True),
    Case("sp-14x1x3-forced", "split", 14, 1, F32, 3, path=SPLIT),
    Case("sp-7x3x3-f64-forced-ident", "split", 7, 3, F64, 3, path=SPLIT, **IDENT),
]


def cases(letter):
    return [c for c in CASES if letter in c.run]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def slices(solver, c):
    """Problems per persistent launch when AUTO cuts a batch into several (api_solve.hip, persist_slices); 0: it does not."""
    if c.path != AUTO or solver.choose_path(c.es, c.n, c.N, c.B) != SPLIT:
        return 0
    cap = 0
    for b in range(1, min(c.B, 65)):
        if solver.choose_path(c.es, c.n, c.N, b) != PERSIST:
            break
        cap = b
    if cap == 0:
        return 0
    launches = -(-c.B // cap)
    return 0 if launches > 16 or 25.0 * launches >= 1.8 * (2.0 * c.mi + 4.0) else cap


def assert_family(solver, c):
    """The shape, batch, mode and alignment of the case reach the kernel family it was written for."""
    solver.set_symmetric(c.mode)
    solver.set_path(c.path)
    try:
        path = solver.choose_path(c.es, c.n, c.N, c.B)
        members = solver.cluster_members(c.es, c.n, c.N)
        one_round = members != 0 and c.B * members <= cus()
        if c.fam in ("resident_sym_verify", "resident_sym"):
            assert (c.n, c.dt, members) == (14, F32, 2) and c.N <= 128 and c.pinv and path == FUSED, (path, members)
            if c.fam == "resident_sym_verify":
                assert c.mode == 2 and c.shift == 0 and not one_round
            else:
                assert c.mode == 1 or (c.mode == 2 and c.shift == 8 and not one_round)
        elif c.fam == "resident":
            H = RESIDENT_HORIZON[(c.es, c.n)]
            assert path == FUSED and c.N <= H and members == 0 and solver.cluster_members(c.es, c.n, H + 1) == 2, (path, members)
            assert solver.cluster_members(c.es, c.n, H) == 0
            assert c.B <= 5 or c.B > 4 * cus(), "no workgroup takes a second problem"
        elif c.fam == "cluster":
            assert path == FUSED and members >= 1, (path, members)
            assert c.mode == 0 or (c.mode == 2 and one_round)
        elif c.fam == "persist":
            assert path == (c.path if c.path != AUTO else PERSIST), path
        elif c.fam == "persist_sliced":
            assert path == SPLIT and slices(solver, c) >= 1, (path, slices(solver, c))
        elif c.fam == "fused":
            # no resident and no cluster kernel at the block size, or an iteration limit the cluster kernel's tags cannot count
            assert path == FUSED and c.mode == 0 and ((members == 0 and c.n > 15) or c.mi >= (1 << 19)), (path, members)
            assert c.B > 4 * cus(), "no workgroup takes a second problem"
        elif c.fam == "fused_sym":
            # beyond the cluster kernel's (so also the resident kernel's) horizon, a batch that is worth the [D|R] kernel
            assert path == FUSED and members == 0 and c.mode == 1 and c.pinv and c.B >= cus() and c.n % 2 == 0 and c.N > 128, (path, members)
        elif c.fam == "split":
            assert path == SPLIT and slices(solver, c) == 0, (path, slices(solver, c))
        else:
            raise AssertionError(c.fam)
    finally:
        solver.set_symmetric(2)
        solver.set_path(AUTO)


# ----------------------------------------------------------------------------------------------------------- the arena
class Arena:
    """Arrays as views into one device buffer: float arrays lie in NaN (all-ones bytes), the integer ones in 0xA5, each with a
    guard of max(4 KiB, one problem of that array) on both sides; the start of a view keeps the wanted address modulo 16."""

    def __init__(self, specs):
        self.at = {}
        off = 0
        for name, nbytes, per_problem, mod16, fill in specs:
            g = -(-max(4096, per_problem) // 16) * 16
            start = off + g + mod16
            self.at[name] = (start, start + nbytes, g, fill)
            off = -(-(start + nbytes + g) // 16) * 16
        self.buf = torch.full((off,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        for start, end, g, fill in self.at.values():
            if fill != 0xFF:
                self.buf[start - g:end + g] = fill

    def view(self, name, dtype):
        start, end = self.at[name][:2]
        return self.buf[start:end].view(dtype)

    def snapshot(self):
        return self.buf.clone()

    def assert_only_changed(self, before, written):
        """Every byte outside the arrays named in `written` is what the snapshot holds (guards and inputs alike)."""
        after = self.buf.clone()
        for name in written:
            start, end = self.at[name][:2]
            after[start:end] = before[start:end]
        if not torch.equal(after, before):
            i = int(torch.nonzero(after != before)[0])
            where = [f"{nm}{'-guard-before' if i < s else '-guard-behind' if i >= e else ''} at byte {i - s}"
                     for nm, (s, e, g, _) in self.at.items() if s - g <= i < e + g]
            raise AssertionError(f"bytes outside the outputs changed, first: {where or i}")


def tt(dt):
    return torch.float32 if np.dtype(dt) == F32 else torch.float64


def ibits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _symmetrize(n, N, P):
    L, D, R = synth.unpack_bt(n, N, P)
    L = L.copy()
    L[..., 1:, :, :] = np.swapaxes(R[..., :-1, :, :], -1, -2)
    return synth.pack_bt(L, D, R)


class Problem:
    """The data of one case on the host: a pool of generated problems, repeated with gamma scaled per problem."""

    def __init__(self, c, seed=0, asym_every=0):
        n, N, B = c.n, c.N, c.B
        pool = min(B, 8)
        d = synth.gen_numpy(n, N, seed=7000 + 13 * n + N + seed, batch=pool, dtype=c.dt)
        self.S, self.P = d["S"], (_symmetrize(n, N, d["Pinv"]) if c.mode else d["Pinv"])
        if asym_every and N >= 2:     # mode 2: some problems fail the symmetry test (one ulp in one element of an L block)
            pool = min(B, 8 * asym_every)
            rep = np.arange(pool) % self.S.shape[0]
            self.S, self.P = self.S[rep].copy(), self.P[rep].copy()
            i = 3 * n * n + 2 * n + 1                    # L_1(1, 2)
            for b in range(0, pool, asym_every):
                self.S[b, i] = np.nextafter(self.S[b, i], c.dt.type(np.inf))
        self.idx = np.arange(B) % pool
        base = d["gamma"][np.arange(B) % d["gamma"].shape[0]]
        self.gamma = (base * (1.0 + 0.003 * np.arange(B))[:, None]).astype(c.dt)
        self.lam0 = np.zeros_like(self.gamma)
        self.c = c

    def warm(self):
        rng = np.random.default_rng(self.c.N)
        self.lam0 = (0.1 * rng.standard_normal(self.gamma.shape)).astype(self.c.dt)
        return self

    def host(self, sub):
        return self.S[self.idx[sub]], (self.P[self.idx[sub]] if self.c.pinv else None), self.gamma[sub], self.lam0[sub]


NAMES = ("S", "P", "gamma", "lam", "r", "p", "it", "fl")
OUT = ("lam", "r", "p", "it", "fl")


def upload(c, pr, tight, perm=None):
    """Device tensors of the case: of their own, or (tight) inside an arena with NaN corner blocks."""
    n, N, B, es = c.n, c.N, c.B, c.es
    ms, vs = 3 * n * n * N, n * N
    idx = pr.idx if perm is None else pr.idx[perm]
    sel = np.arange(B) if perm is None else perm
    dS = torch.from_numpy(pr.S).cuda()[torch.from_numpy(idx).cuda()]
    dP = torch.from_numpy(pr.P).cuda()[torch.from_numpy(idx).cuda()] if c.pinv else None
    src = {"S": dS, "P": dP, "gamma": torch.from_numpy(pr.gamma[sel]).cuda(), "lam": torch.from_numpy(pr.lam0[sel]).cuda()}
    if tight:
        for M in (dS, dP):
            if M is None:
                continue
            M[:, :n * n] = float("nan")                  # L_0
            M[:, ms - n * n:] = float("nan")             # R_{N-1}
            if c.no_L:
                M.view(B, N, 3, n * n)[:, :, 0, :] = float("nan")
    specs = [("S", B * ms * es, ms * es, c.shift, 0xFF), ("P", B * ms * es, ms * es, c.shift, 0xFF)]
    specs += [(k, B * vs * es, vs * es, 0, 0xFF) for k in ("gamma", "lam", "r", "p")]
    specs += [("it", 4 * B, 4, 0, 0xA5), ("fl", B, 1, 0, 0xA5)]
    T = {}
    if tight:
        ar = Arena(specs)
        T["arena"] = ar
        for name, *_ in specs:
            T[name] = ar.view(name, torch.int32 if name == "it" else torch.uint8 if name == "fl" else tt(c.dt))
    else:
        for name, nbytes, _, mod16, _ in specs:
            if name in ("it", "fl"):
                T[name] = torch.empty(B, dtype=torch.int32 if name == "it" else torch.uint8, device="cuda")
            else:
                buf = torch.empty(nbytes // es + 16 // es, dtype=tt(c.dt), device="cuda")
                assert buf.data_ptr() % 16 == 0
                T[name] = buf[mod16 // es:mod16 // es + nbytes // es]
                T["_keep_" + name] = buf
    for k in ("S", "P", "gamma", "lam"):
        if src[k] is not None:
            T[k].copy_(src[k].reshape(-1))
    if not c.pinv:
        T["P_arg"] = None
    reset_outputs(T)
    for k in ("S", "P"):
        assert T[k].data_ptr() % 16 == c.shift
    for k in ("gamma", "lam", "r", "p", "it", "fl"):
        assert T[k].data_ptr() % 16 == 0
    return T


def reset_outputs(T, lam0=None):
    if lam0 is not None:
        T["lam"].copy_(lam0)
    T["r"].fill_(float("nan"))
    T["p"].fill_(float("nan"))
    T["it"].fill_(-1)
    T["fl"].fill_(7)


def run(solver, c, T, mode=None, mi=None):
    solver.set_symmetric(c.mode if mode is None else mode)
    solver.set_path(c.path)
    try:
        solver.solve(c.n, c.N, c.B, T["S"], T["P"] if c.pinv else None, T["gamma"], T["lam"], T["r"], T["p"], tol=c.tol,
                     max_iter=c.mi if mi is None else mi, iters=T["it"], max_iter_exit=T["fl"])
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
        solver.set_path(AUTO)
    return {k: T[k].clone().reshape(c.B, -1) for k in OUT}


def same_rows(a, b):
    """Per problem: lambda, r, p, iters and the flag bit-identical."""
    eq = torch.ones(a["it"].shape[0], dtype=torch.bool, device="cuda")
    for k in ("lam", "r", "p"):
        eq &= (ibits(a[k]) == ibits(b[k])).all(dim=1)
    return eq & (a["it"] == b["it"]).all(dim=1) & (a["fl"] == b["fl"]).all(dim=1)


def relerr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def check_oracle(orc, c, pr, out):
    """The rule of the per-family files: equal iteration counts and flags; lambda 1e-6 (fp32) / 1e-10 (fp64) norm-wise, twice
    that for the cluster kernel's fixed-count warm starts; r and p to 2e-5 / 1e-9 of max |gamma|; without a preconditioner
    (fixed count) 20 x and 10 x that (test_gpu_cluster.py)."""
    sub = np.unique(np.linspace(0, c.B - 1, min(c.B, 10)).astype(np.int64))
    S, P, g, l0 = pr.host(sub)
    ob = orc.pcg_batch(c.n, c.N, len(sub), S, P, g, lambda0=l0, tol=c.tol, max_iter=c.mi, nthreads=8)
    ltol = 1e-10 if c.dt == F64 else 1e-6
    vtol = 1e-9 if c.dt == F64 else 2e-5
    if not c.pinv:
        ltol, vtol = 20 * ltol, 10 * vtol
    elif c.tol == 0.0 and c.fam == "cluster":
        ltol *= 2
    ts = torch.from_numpy(sub).cuda()
    h = {k: out[k][ts].cpu().numpy() for k in OUT}
    assert np.array_equal(h["it"].ravel().astype(np.int64), ob["iters"].astype(np.int64)), (h["it"].ravel(), ob["iters"])
    assert np.array_equal(h["fl"].ravel().astype(bool), ob["max_iter_exit"])
    for j in range(len(sub)):
        scale = np.abs(g[j]).max()
        assert relerr(h["lam"][j], ob["lambda_"][j]) < ltol, (sub[j], relerr(h["lam"][j], ob["lambda_"][j]))
        assert np.abs(h["r"][j] - ob["r"][j]).max() < vtol * scale, sub[j]
        assert np.abs(h["p"][j] - ob["p"][j]).max() < vtol * scale, sub[j]


# ------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("c", cases("A"), ids=repr)
def test_same_answer_whatever_lies_around_the_data(solver, orc, c):
    assert_family(solver, c)
    pr = Problem(c)
    if c.tol == 0.0:
        pr.warm()
    plain = upload(c, pr, tight=False)
    out_plain = run(solver, c, plain)
    tight = upload(c, pr, tight=True)
    before = tight["arena"].snapshot()
    out_tight = run(solver, c, tight)
    bad = torch.nonzero(~same_rows(out_plain, out_tight)).flatten().tolist()
    assert not bad, f"problems {bad[:10]} of {c.B} differ between tensors of their own and the arena"
    tight["arena"].assert_only_changed(before, OUT)
    check_oracle(orc, c, pr, out_tight)
    if c.fam in ("resident_sym_verify", "resident_sym"):
        # NaN corners do not change the verdict (they are outside the symmetry relation): mode 2 == mode 1 bit for bit, and both
        # are the resident symmetric kernel, whose bits are not the cluster kernel's
        if c.mode == 2:
            reset_outputs(tight, torch.from_numpy(pr.lam0).cuda().reshape(-1))
            assert same_rows(run(solver, c, tight, mode=1), out_tight).all()
        reset_outputs(plain, torch.from_numpy(pr.lam0).cuda().reshape(-1))
        assert not same_rows(run(solver, c, plain, mode=0), out_plain).all(), "mode 0 gives the same bits: which kernel ran?"


# ------------------------------------------------------------------------------------------------------------------- B
def break_problems(c, T):
    """One kind each at the first, the last and two adjacent middle positions (fewer where the batch is smaller)."""
    n, N, B = c.n, c.N, c.B
    ms, vs = 3 * n * n * N, n * N
    pos = list(dict.fromkeys([0, B - 1, B // 2, min(B // 2 + 1, B - 1)]))
    S, g = T["S"].view(B, ms), T["gamma"].view(B, vs)
    k = N // 2
    kinds = ["zero", "nan", "inf", "matrix"]
    for b, kind in zip(pos, kinds):
        if kind == "zero":
            g[b] = 0.0
        elif kind == "nan":
            g[b, (vs * 2) // 5] = float("nan")
        elif kind == "inf":
            g[b, vs // 3] = float("inf")
        else:
            S[b, k * 3 * n * n + n * n + (n // 2) * n + 1] = float("nan")          # D_k(1, n/2)
            if c.mode and c.pinv and N >= 2:      # the same NaN bits in R_kk and L_{kk+1} of Phi^-1: storage stays symmetric
                P, kk = T["P"].view(B, ms), min(k, N - 2)
                P[b, kk * 3 * n * n + 2 * n * n + 3 * n + 2] = float("nan")          # R_kk(2, 3)
                P[b, (kk + 1) * 3 * n * n + 2 * n + 3] = float("nan")                # L_kk+1(3, 2)
    return pos


@pytest.mark.parametrize("c", cases("B"), ids=repr)
def test_a_broken_problem_stays_in_its_own_row(solver, orc, c):
    assert_family(solver, c)
    pr = Problem(c)
    T = upload(c, pr, tight=False)
    lam0 = T["lam"].clone()
    clean_in = {k: T[k].clone() for k in ("S", "P", "gamma")}
    for mi in ([c.mi, 0] if c.zero else [c.mi]):
        reset_outputs(T, lam0)
        clean = run(solver, c, T, mi=mi)
        pos = break_problems(c, T)
        reset_outputs(T, lam0)
        broken = run(solver, c, T, mi=mi)            # (a GbdPcgError here: the call did not return success)
        healthy = torch.ones(c.B, dtype=torch.bool, device="cuda")
        healthy[pos] = False
        bad = torch.nonzero(healthy & ~same_rows(clean, broken)).flatten().tolist()
        assert not bad, f"healthy problems {bad[:10]} changed next to the broken ones {pos}"
        if c.mode == 2 and c.fam in ("resident_sym_verify", "resident_sym"):
            # the mirrored NaN pair keeps the storage symmetric: the broken problems stay on the resident kernel, bit for bit
            # what the caller's word (mode 1) gives -- not what the general launch would make of them
            reset_outputs(T, lam0)
            assert same_rows(run(solver, c, T, mode=1, mi=mi), broken).all(), "a broken problem left the resident symmetric kernel"
        it, fl = broken["it"].flatten().cpu().numpy(), broken["fl"].flatten().cpu().numpy()
        if mi >= 1:
            assert (it[pos] == mi).all() and (fl[pos] == 1).all(), (pos, it[pos], fl[pos])
            assert not torch.isfinite(broken["lam"][pos]).any(), "finite entries of lambda in a degenerate problem"
        else:
            assert (it[pos] == 0).all() and (fl[pos] == 1).all(), (pos, it[pos], fl[pos])
            assert torch.equal(ibits(broken["lam"][pos]), ibits(lam0.view(c.B, -1)[pos]))
            tp = torch.tensor(pos, device="cuda")
            hS, hg = T["S"].view(c.B, -1)[tp].cpu().numpy(), T["gamma"].view(c.B, -1)[tp].cpu().numpy()
            hP = T["P"].view(c.B, -1)[tp].cpu().numpy() if c.pinv else None
            ob = orc.pcg_batch(c.n, c.N, len(pos), hS, hP, hg, tol=c.tol, max_iter=0)
            assert not ob["iters"].any() and ob["max_iter_exit"].all()
            for key in ("r", "p"):
                assert np.array_equal(np.isfinite(broken[key][tp].cpu().numpy()), np.isfinite(ob[key])), key
        # nothing of it stays in the handle: the clean batch again, bit for bit
        for k in ("S", "P", "gamma"):
            T[k].copy_(clean_in[k])
        reset_outputs(T, lam0)
        assert same_rows(run(solver, c, T, mi=mi), clean).all(), "the clean batch after the broken one differs from the first"


# ------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("c", [c for c in cases("C") if c.B >= 3], ids=repr)
def test_position_in_the_batch_does_not_matter(solver, c):
    assert_family(solver, c)
    # mode 2: every fifth problem fails the symmetry test, so that the verdict bytes differ from slot to slot
    pr = Problem(c, seed=1, asym_every=5 if c.mode == 2 and c.fam != "cluster" else 0)
    T = upload(c, pr, tight=False)
    first = run(solver, c, T)
    perm = np.random.default_rng(20261016 + c.B).permutation(c.B)
    T2 = upload(c, pr, tight=False, perm=perm)
    for k in ("S", "P", "gamma", "lam"):
        T[k].copy_(T2[k])
    reset_outputs(T)
    second = run(solver, c, T)
    tp = torch.from_numpy(perm).cuda()
    bad = torch.nonzero(~same_rows({k: v[tp] for k, v in first.items()}, second)).flatten().tolist()
    assert not bad, f"slots {bad[:10]}: the answer depends on the position in the batch"


# ------------------------------------------------------------------------------------- the other kernels, same arena
AUX_SHAPES = [(14, 128, 5, F32), (14, 1, 3, F32), (14, 2, 3, F64), (16, 33, 4, F32), (36, 17, 2, F64), (14, 300, 2, F32)]


def aux_data(n, N, B, dt):
    d = synth.gen_numpy(n, N, seed=8100 + n + N, batch=B, dtype=dt)
    x = np.stack([synth.normals(8200 + b, 0, n * N) for b in range(B)]).astype(dt)
    return d["S"], x


def poison(M, n, N, B, all_L=False):
    ms = 3 * n * n * N
    M = M.view(B, ms)
    M[:, :n * n] = float("nan")
    M[:, ms - n * n:] = float("nan")
    if all_L:
        M.view(B, N, 3, n * n)[:, :, 0, :] = float("nan")


@pytest.mark.parametrize("n,N,B,dt", AUX_SHAPES)
@pytest.mark.parametrize("sym", [0, 1], ids=["general", "symmetric"])
def test_spmv_in_the_arena(solver, n, N, B, dt, sym):
    S, x = aux_data(n, N, B, dt)
    es, ms, vs = np.dtype(dt).itemsize, 3 * n * n * N, n * N
    solver.set_symmetric(sym)
    try:
        y0 = solver.spmv(n, N, B, torch.from_numpy(S).cuda(), torch.from_numpy(x).cuda())
        ar = Arena([("M", B * ms * es, ms * es, 0, 0xFF), ("x", B * vs * es, vs * es, 0, 0xFF), ("y", B * vs * es, vs * es, 0, 0xFF)])
        M, dx, y = (ar.view(k, tt(dt)) for k in ("M", "x", "y"))
        M.copy_(torch.from_numpy(S).cuda().reshape(-1))
        dx.copy_(torch.from_numpy(x).cuda().reshape(-1))
        poison(M, n, N, B, all_L=bool(sym) and n in (8, 12, 14, 16))     # the block sizes with a [D|R] product (test_symmetric_spmv)
        before = ar.snapshot()
        solver.spmv(n, N, B, M, dx, y)
        torch.cuda.synchronize()
    finally:
        solver.set_symmetric(2)
    ar.assert_only_changed(before, ("y",))
    assert torch.equal(ibits(y), ibits(y0.reshape(-1)))


@pytest.mark.parametrize("n,N,B,dt", AUX_SHAPES)
def test_check_symmetric_in_the_arena(solver, n, N, B, dt):
    S, _ = aux_data(n, N, B, dt)
    S = S.copy()
    if N >= 2:
        S[B - 1, 3 * n * n + 1] = np.nextafter(S[B - 1, 3 * n * n + 1], np.dtype(dt).type(np.inf))    # L_1 of the last problem
    es, ms = np.dtype(dt).itemsize, 3 * n * n * N
    f0 = solver.check_symmetric(n, N, B, torch.from_numpy(S).cuda())
    assert f0.cpu().tolist() == [1] * (B - 1) + [0 if N >= 2 else 1]
    ar = Arena([("M", B * ms * es, ms * es, 0, 0xFF), ("flags", B, 1, 0, 0xA5)])
    M, fl = ar.view("M", tt(dt)), ar.view("flags", torch.uint8)
    M.copy_(torch.from_numpy(S).cuda().reshape(-1))
    poison(M, n, N, B)
    before = ar.snapshot()
    solver.check_symmetric(n, N, B, M, flags=fl)
    torch.cuda.synchronize()
    ar.assert_only_changed(before, ("flags",))
    assert torch.equal(fl, f0)


@pytest.mark.parametrize("kind", [binding.PINV_STAIR, binding.PINV_BLOCK_JACOBI, binding.PINV_IDENTITY], ids=["stair", "jacobi", "identity"])
@pytest.mark.parametrize("n,N,B,dt", [(14, 128, 5, F32), (14, 1, 3, F32), (14, 2, 3, F64), (16, 33, 4, F32), (16, 17, 3, F64), (36, 17, 2, F64),
                                      (36, 5, 3, F32)])
def test_form_pinv_in_the_arena(solver, n, N, B, dt, kind):
    S, _ = aux_data(n, N, B, dt)
    es, ms = np.dtype(dt).itemsize, 3 * n * n * N
    P0 = solver.form_pinv(n, N, B, torch.from_numpy(S).cuda().reshape(-1), kind)
    ar = Arena([("S", B * ms * es, ms * es, 0, 0xFF), ("P", B * ms * es, ms * es, 0, 0xFF)])
    dS, dP = ar.view("S", tt(dt)), ar.view("P", tt(dt))
    dS.copy_(torch.from_numpy(S).cuda().reshape(-1))
    poison(dS, n, N, B)
    before = ar.snapshot()
    solver.form_pinv(n, N, B, dS, kind, Pinv=dP)
    torch.cuda.synchronize()
    ar.assert_only_changed(before, ("P",))
    a, b = ibits(dP).view(B, ms).clone(), ibits(P0).view(B, ms).clone()
    for M in (a, b):      # the corner slots of the output are unspecified
        M[:, :n * n] = 0
        M[:, ms - n * n:] = 0
    assert torch.equal(a, b)
