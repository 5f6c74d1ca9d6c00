"""Phi^-1 formation kernel by kernel: every family launch_form_pinv (csrc/pinv.hip) can pick, at the block sizes, kinds, horizons,
precisions and pointer alignments that pick it, against the plain numpy reference of tests/pinv_ref.py (CPU half:
tests/test_pinv_reference.py, which also holds every case to a restatement of the dispatch).

Per case (check_case): the output buffer is NaN-filled and every slot but the two never-read corner slots must come back
finite; every (problem, knot, slot) block is within max(TOL, 8 e_np) of the reference relative to the block's largest entry
(e_np: the same formulas in the case's own precision with plain numpy; pinv_ref.py); kinds 0 and 1 write exact zeros, exact
identities and exactly symmetric inverses; gbdpcg_check_symmetric_* answers 1 for every problem whose S was symmetric in storage;
and the same input with S and Pinv one element past a 16-byte boundary gives the same bits wherever the dispatch does not look at
the address (fp32 n = 16 runs two different kernels and is held to the reference twice).

Kernels only an environment switch reaches run in one fresh child process per switch set (the switches are read once per
process), one child at a time, through the same check_case.

RECORDED on the build before this module (N = 2, B = 1, stepping n up from 88 / 68): fp32 accepts 90 and refuses 91, fp64 accepts
71 and refuses 72; a refusal answers GBDPCG_ERR_HIP (2) with "invalid argument" as the last HIP error -- NOT the
GBDPCG_ERR_UNSUPPORTED (4) the Schur launchers answer through schur_shape_ok.  The ABI is left as it is.

gbdpcg_form_pinv_solve_* at the largest sizes: fp32 n = 90 solves; fp64 n = 71 forms Phi^-1 but the solve side has no lane map
for an odd n > 64 and the call answers GBDPCG_ERR_UNSUPPORTED before anything runs, so the fp64 end-to-end case is n = 70 and
the refusal at 71 is asserted as recorded.

OBSERVED on the MI355X: largest kernel error / e_np over the blocks of a family (fp32, fp64), D blocks of condition number <= 6.1
throughout.  The quotient is a maximum over blocks, so it is set by the blocks where numpy's own error happens to be smallest;
in fp32 it exceeds the margin of 8 in most families while every block stays under the project's 2e-5 (the first term of the
bound, which is the one that holds there); in fp64 it stays under 8 everywhere.
    pinv_stair_fused_kernel                      14.80   6.66      pinv_stair_mfma_kernel<16>                11.19   --
    pinv_diag_quad_kernel + pinv_stair_reg        8.81   3.83      pinv_diag_pair_kernel (kinds 0, 1)         9.59   3.83
    pinv_diag_reg_kernel (+ pinv_stair_reg)      11.24   3.58      pinv_diag_wide + pinv_stair_wide          10.28   1.91
    any-size <64,16>                             12.69   4.32      any-size <256,16>                         12.68   3.31
    any-size <256,64>                            22.53   2.43
    children: MFMA_FROM=12 9.44, NO_MFMA 7.74, TWO_PASS 9.59, PAIR 8.81, PAIR + TWO_PASS 9.59, NO_WIDE 11.22 (36 in fp64: 2.22)
    form + solve against the dense fp64 solve: fp32 at most 5.0e-6 (n = 2), fp64 at most 1.2e-11 (n = 8); at the largest sizes
    2.4e-5 (fp32 n = 90, 6 iterations, bound 5.8e-4) and 4.1e-7 (fp64 n = 70, 8 iterations, bound 5.6e-6)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pinv_ref as pr  # noqa: E402
from gbd_pcg_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = pr.F32, pr.F64
OK, ERR_HIP, UNSUPPORTED = 0, 2, 4
TDT = {F32: torch.float32, F64: torch.float64}
# tests/test_gpu_parity.py against a dense fp64 solve: test_readme_system_fp32 (5e-5), test_readme_system_fp64 (1e-10)
LAMBDA_TOL = {F32: 5e-5, F64: 1e-10}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def placed(host, off, fill=None):
    """A device tensor of host's size that starts `off` elements past a 16-byte boundary: host's values, or `fill`."""
    host = np.array(host).reshape(-1)   # (a copy: the cached inputs are read-only)
    buf = torch.empty(host.size + 4, dtype=TDT[host.dtype.type], device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + host.size]
    if fill is None:
        t.copy_(torch.from_numpy(host))
    else:
        t.fill_(fill)
    return t


def form(solver, c, S_host, s_off, p_off):
    S = placed(S_host, s_off)
    P = placed(S_host, p_off, fill=float("nan"))
    solver.form_pinv(c.n, c.N, c.B, S, c.kind, Pinv=P)
    torch.cuda.synchronize()
    flags = solver.check_symmetric(c.n, c.N, c.B, P.clone()).cpu().numpy()
    return P.cpu().numpy().reshape(c.B, c.N, 3, c.n * c.n), flags


def check_output(c, d, got, flags, what):
    """One output of a case against its reference; returns the worst kernel error / e_np over the blocks with e_np > 0."""
    n, m = c.n, d.mask
    assert np.isfinite(got[m]).all(), (what, "a specified slot is not finite")
    err, _ = pr.block_error(got, d.ref)
    over = (err > d.bound * d.scale) & m
    assert not over.any(), (what, "blocks (problem, knot, slot) over the bound", np.argwhere(over)[:4].tolist(),
                            (err[over] / np.maximum(d.scale[over], 1e-300))[:4].tolist(), d.bound[over][:4].tolist())
    if c.kind != pr.STAIR:
        off = got[:, :, (0, 2)][m[:, :, (0, 2)]]
        assert not off.any(), (what, "L / R slots are not exactly zero")
        D = got[:, :, 1].reshape(c.B, c.N, n, n)
        if c.kind == pr.IDENTITY:
            assert np.array_equal(D, np.broadcast_to(np.eye(n, dtype=got.dtype), D.shape)), (what, "D slot is not exactly I")
        else:
            assert np.array_equal(D, np.swapaxes(D, -1, -2)), (what, "D slot is not exactly symmetric")
    keep = [b for b in range(c.B) if b not in pr.perturbed_problems(c)]
    assert flags[keep].tolist() == [1] * len(keep), (what, "symmetric S, but Phi^-1 is not symmetric in storage", flags.tolist())
    pos = m & (d.e_np > 0)
    return float((err[pos] / (d.e_np[pos] * d.scale[pos])).max()) if pos.any() else 0.0


def check_case(solver, c):
    """Every assertion of the module docstring on one case; returns (worst error ratio, condition number)."""
    d, what = pr.case_data(c), pr.case_id(c)
    worst, outs = 0.0, {}
    for s_off, p_off in ((c.s_off, 0), (c.s_off, 1)) + (((1, 1),) if c.s_off == 0 else ()):
        got, flags = form(solver, c, d.S, s_off, p_off)
        worst = max(worst, check_output(c, d, got, flags, (what, f"S+{s_off}", f"Pinv+{p_off}")))
        outs[s_off, p_off] = got
    first = outs[c.s_off, 0]
    for (s_off, p_off), got in outs.items():
        same_kernels = pr.route(c.dtype, c.n, c.N, c.kind, s_off == 0, c.env) == pr.route(c.dtype, c.n, c.N, c.kind, c.s_off == 0, c.env)
        if same_kernels:
            assert np.array_equal(got[d.mask], first[d.mask]), (what, f"S+{s_off} Pinv+{p_off} differs in bits from Pinv+0")
    return worst, d.cond


def run_cases(solver, cases, label):
    assert cases
    worst, cond = 0.0, 0.0
    for c in cases:
        w, k = check_case(solver, c)
        worst, cond = max(worst, w), max(cond, k)
    print(f"{label}: {len(cases)} cases, worst kernel error / e_np {worst:.2f}, worst condition number {cond:.1f}")
    return worst


FAMILIES = sorted({c.family for c in pr.CASES if not c.env})


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", FAMILIES, ids=["+".join(f) for f in FAMILIES])
def test_family(solver, family, dtype):
    cases = [c for c in pr.CASES if c.family == family and c.dtype == dtype and not c.env]
    if not cases:
        assert family == pr.MFMA and dtype == F64   # the MFMA stair is fp32 only
        return
    run_cases(solver, cases, f"{'+'.join(family)} {np.dtype(dtype).name}")


# ---------------------------------------------------------------------- kernels behind environment switches: child processes
def child_main(names):
    """Runs in the child: the cases of one switch set, one line per case."""
    env = tuple((k, os.environ[k]) for k in names.split(","))
    solver = binding.Solver(0)
    for c in pr.CASES:
        if c.env == env:
            w, k = check_case(solver, c)
            print(f"CASE ok ratio={w:.3f} cond={k:.1f} {pr.case_id(c)}", flush=True)
    solver.close()


@pytest.mark.parametrize("switches", pr.SWITCH_SETS, ids=["+".join(k.replace("GBDPCG_PINV_", "") for k, _ in s) for s in pr.SWITCH_SETS])
def test_switch_only_kernels(switches):
    cases = [c for c in pr.CASES if c.env == switches]
    assert cases
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("GBDPCG_PINV_"):
            del env[k]
    env.update(dict(switches))
    names = ",".join(k for k, _ in switches)
    code = (f"import sys; sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {ROOT!r}]; "
            f"import test_gpu_pinv_dispatch as t; t.child_main({names!r})")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=120, capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ok ")]
    assert len(done) == len(cases), (len(done), len(cases))
    ratios = [float(re.search(r"ratio=([0-9.]+)", ln).group(1)) for ln in done]
    print(f"{names}: {len(cases)} cases, worst kernel error / e_np {max(ratios):.2f}")


# ---------------------------------------------------------------------------------------------------------------- refusals
def try_form(solver, dtype, n, N=2, B=1, kind=pr.STAIR):
    """(status, Pinv on the host, S on the host) of one gbdpcg_form_pinv_* call into a NaN-filled buffer."""
    c = pr.Case(pr.REFUSED, dtype, n, N, B, kind, False, 0, ())
    S_host = pr.make_S(c)
    S, P = placed(S_host, 0), placed(S_host, 0, fill=float("nan"))
    try:
        solver.form_pinv(n, N, B, S, kind, Pinv=P)
        status = OK
    except binding.GbdPcgError as e:
        status = int(re.search(r"status (\d+)", str(e)).group(1))
    torch.cuda.synchronize()
    return status, P.cpu().numpy(), c


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_refusals_as_recorded(solver, dtype):
    seen = {}
    for n in range(88 if dtype == F32 else 68, pr.FIRST_REFUSED[dtype] + 2):
        status, P, c = try_form(solver, dtype, n)
        seen[n] = status
        print(f"{np.dtype(dtype).name} n = {n}: status {status}")
        if status != OK:
            assert np.isnan(P).all(), "a refused call wrote into Pinv"
            hip = solver.lib.gbdpcg_last_hip_error_string(solver.h).decode()
            print(f"    last HIP error: {hip}")
            assert hip == "invalid argument"
        else:
            d = pr.case_data(pr.Case(pr.G256L, dtype, n, 2, 1, pr.STAIR, False, 0, ()))
            err, _ = pr.block_error(P.reshape(1, 2, 3, n * n), d.ref)
            assert np.isfinite(P.reshape(1, 2, 3, -1)[d.mask]).all() and (err <= d.bound * d.scale)[d.mask].all(), n
    first = min(n for n, s in seen.items() if s != OK)
    assert first == pr.FIRST_REFUSED[dtype] and all(s == ERR_HIP for n, s in seen.items() if n >= first), seen
    # the next accepted call on the same handle succeeds
    status, P, _ = try_form(solver, dtype, 14, N=3, B=2)
    assert status == OK and np.isfinite(P.reshape(2, 3, 3, -1)[pr.corner_mask(2, 3)]).all()


# ------------------------------------------------------------------------------------------------- form + solve in one call
def dense_lambda(n, N, S_host, gamma):
    return np.stack([np.linalg.solve(pr.dense_from_blocks(n, N, S_host[b].reshape(N, 3, n * n)), gamma[b].astype(F64))
                     for b in range(S_host.shape[0])])


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a, F64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("dtype,n", [(F32, 2), (F32, 4), (F32, 8), (F32, 10), (F32, 16), (F64, 8), (F64, 14), (F64, 16)])
def test_form_pinv_solve_with_some_asymmetric_problems(solver, dtype, n):
    """tests/test_gpu_robustness.py::test_form_pinv_solve_with_some_asymmetric_problems at the other block sizes, N = 20.  The stair
    kernel reports verdicts only where the solve would pick a symmetric kernel (api_solve.hip: FUSED path, fused_has_symmetric): at N = 20
    that needs a block size the register-resident kernel does not take (16; 14 in fp64) and a batch of at least the device's 256
    compute units, so those sizes run 258 problems; the solve then takes them as clusters of one and ignores the bytes, so no size of
    this list has the two-kernel dispatch, and the others run 6 problems."""
    N, base = 20, 6
    B = 258 if n == 16 or (n == 14 and dtype == F64) else 6
    c = pr.Case(pr.FUSED, dtype, n, N, base, pr.STAIR, False, 0, ())
    idx = np.arange(B) % base
    S_h = pr.make_S(c)[idx].reshape(B, N, 3, n, n).copy()
    from gbd_pcg_amd import synth
    g0 = synth.gen_numpy(n, N, seed=31337, batch=base, dtype=dtype)["gamma"]
    gamma = (g0[idx] * (1.0 + 0.001 * (np.arange(B) // base))[:, None]).astype(dtype)
    S_h[1, 12, 0, 1, 0] *= 1.0 + 2.0 ** (-16 if dtype == F32 else -40)   # L_12 of problem 1: last-bits perturbation
    S_h[4, N - 1, 0, 0, 0] += 1e-3                                        # L_{N-1} of problem 4
    S_h = S_h.reshape(B, -1)
    tol = 1e-9 if dtype == F32 else 1e-20
    S, g = placed(S_h, 0), placed(gamma, 0)
    P = torch.full_like(S, float("nan"))
    lam = torch.zeros_like(g)
    it, fl = solver.form_pinv_solve(n, N, B, S, P, g, lam, tol=tol, max_iter=100)
    torch.cuda.synchronize()
    P2 = solver.form_pinv(n, N, B, S, pr.STAIR)
    lam2 = torch.zeros_like(g)
    it2, fl2 = solver.solve(n, N, B, S, P2, g, lam2, tol=tol, max_iter=100)
    torch.cuda.synchronize()
    m = torch.from_numpy(np.repeat(pr.corner_mask(B, N), n * n, axis=None).reshape(-1)).cuda()
    assert torch.equal(P[m].view(torch.uint8), P2[m].view(torch.uint8))
    assert torch.equal(lam, lam2) and torch.equal(it, it2) and torch.equal(fl, fl2)
    flags = solver.check_symmetric(n, N, B, P).cpu().numpy()
    assert flags[:6].tolist() == [1, 0, 1, 1, 0, 1] and flags[6:].all()   # Phi^-1 is exactly symmetric exactly where S was
    want = dense_lambda(n, N, S_h, gamma)
    worst = max(relerr(lam.cpu().numpy().reshape(B, -1)[b], want[b]) for b in range(B))
    print(f"{np.dtype(dtype).name} n = {n}, {B} problems: worst lambda error against the dense solve {worst:.2e}, "
          f"iterations {int(it.min())} .. {int(it.max())}")
    assert worst < LAMBDA_TOL[dtype]


@pytest.mark.parametrize("dtype,n", [(F32, 90), (F64, 70)], ids=["f32-90", "f64-70"])
def test_form_pinv_solve_at_the_largest_sizes(solver, dtype, n):
    """One gbdpcg_form_pinv_solve_* call on the last any-size tier against the dense fp64 solve (N = 3, B = 2, tol 1e-6 / 1e-10,
    max_iter 200).  fp64: the largest n formation accepts is 71, which the solve refuses (odd and over 64: no lane map) -- asserted
    below as recorded -- so the case is 70.  The iteration stops on |r . Phi^-1 r| < tol, hence
    ||lambda - lambda*|| <= ||S^-1|| ||r|| <= ||S^-1|| sqrt(tol / lambda_min(Phi^-1)); on top of that the rounding floor of
    LAMBDA_TOL."""
    N, B = 3, 2
    tol = 1e-6 if dtype == F32 else 1e-10
    c = pr.Case(pr.G256L, dtype, n, N, B, pr.STAIR, False, 0, ())
    d = pr.case_data(c)
    from gbd_pcg_amd import synth
    gamma = synth.gen_numpy(n, N, seed=4242, batch=B, dtype=dtype)["gamma"]
    S, g = placed(d.S, 0), placed(gamma, 0)
    P = torch.full_like(S, float("nan"))
    lam = torch.zeros_like(g)
    it, fl = solver.form_pinv_solve(n, N, B, S, P, g, lam, tol=tol, max_iter=200)
    torch.cuda.synchronize()
    assert fl.sum().item() == 0
    err, _ = pr.block_error(P.cpu().numpy().reshape(B, N, 3, n * n), d.ref)
    assert (err <= d.bound * d.scale)[d.mask].all()
    want = dense_lambda(n, N, d.S, gamma)
    for b in range(B):
        Sd = pr.dense_from_blocks(n, N, d.S[b].reshape(N, 3, n * n))
        ref_b = np.where(d.mask[b][:, :, None], np.asarray(d.ref[b], F64), 0.0)
        Pd = pr.dense_from_blocks(n, N, ref_b)
        lmin = np.linalg.eigvalsh(0.5 * (Pd + Pd.T)).min()
        bound = np.linalg.norm(np.linalg.inv(Sd), 2) * np.sqrt(tol / lmin) / np.linalg.norm(want[b]) + LAMBDA_TOL[dtype]
        e = relerr(lam.cpu().numpy().reshape(B, -1)[b], want[b])
        print(f"{np.dtype(dtype).name} n = {n} problem {b}: {int(it[b])} iterations, lambda error {e:.2e} (bound {bound:.2e})")
        assert e <= bound
    if dtype == F64:
        n1 = pr.LARGEST[F64]
        z = torch.zeros(B * 3 * n1 * n1 * N, dtype=torch.float64, device="cuda")
        v = torch.zeros(B * n1 * N, dtype=torch.float64, device="cuda")
        with pytest.raises(binding.GbdPcgError, match=f"status {UNSUPPORTED}"):
            solver.form_pinv_solve(n1, N, B, z, torch.full_like(z, float("nan")), v, v.clone(), tol=tol, max_iter=200)
