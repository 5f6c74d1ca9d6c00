"""Which kernel -- or which refusal -- every launcher either side of the solve answers a shape with (csrc/schur.hip,
schur_ginv.hip, schur_residual.hip: quad_dispatch and launch_lds_rows of schur_common.hpp, through the C ABI).

The statuses below were RECORDED on the build before the four launchers were folded onto one dispatch, at N = 5 (not a
multiple of 4), batch = 2, and are asserted here as they were: per entry point and precision, once under the default dispatch
and once under GBDPCG_SCHUR_GENERAL=1,
    (14, 7)   a block size of GBDPCG_QUAD_SHAPES,
    (3, 1)    an odd one of that list,
    (5, 3)    a size outside the list: the any-size LDS kernels either way,
    REFUSED   the smallest nx (nu = nx // 2) the build refuses for LDS, found by stepping nx: 71 in fp32, 50 in fp64 -- and
              the nx before it, the largest it accepts.
Through the C ABI the threshold is the same for every entry point: each call first asks schur_shape_ok, the LDS need of the
FORMATION kernel (the largest of the four), and answers GBDPCG_ERR_UNSUPPORTED; the smaller needs of the other launchers
(recover_wave_elems, gamma_wave_elems, residual_wave_elems) are never the ones that refuse.  The residual launcher's refusal of
`shared` together with `rho` has no entry point that reaches it (there is no gbdpcg_kkt_residual_shared_reg_*), so it has no
case here.

An accepted call is also held to the fp64 formulas of oracle/schur_oracle.py with the tolerances of tests/test_gpu_schur.py
(2e-4 / 1e-11 of the largest entry; 10 x for the recovered step; the residual norms 10 x as well: at most 2 nx + 2 terms of order
one per row) -- an accepted launch that wrote nothing cannot pass.  At the largest accepted size every any-size kernel runs one
wavefront per workgroup on more than 48 KB of LDS: the branch of launch_lds_rows that raises the dynamic-LDS limit."""
import functools
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
N, B = 5, 2
OK, UNSUPPORTED = 0, 4
REFUSED_NX = {F32: 71, F64: 50}
ENTRIES = ("form_schur", "form_schur_reg", "recover_primal", "recover_primal_shared", "form_gamma", "form_gamma_shared",
           "kkt_residual", "kkt_residual_shared", "kkt_residual_reg")
TOL = {F32: 2e-4, F64: 1e-11}


def shapes(dtype):
    r = REFUSED_NX[dtype]
    return [(14, 7), (3, 1), (5, 3), (r - 1, (r - 1) // 2), (r, r // 2)]


# The recording: status by (precision, shape); every entry point gave it, under the default dispatch and under
# GBDPCG_SCHUR_GENERAL=1 alike (2 x 9 x 5 x 2 = 180 calls).
RECORDED = {(F32, (14, 7)): OK, (F32, (3, 1)): OK, (F32, (5, 3)): OK, (F32, (70, 35)): OK, (F32, (71, 35)): UNSUPPORTED,
            (F64, (14, 7)): OK, (F64, (3, 1)): OK, (F64, (5, 3)): OK, (F64, (49, 24)): OK, (F64, (50, 25)): UNSUPPORTED}


def recorded_status(entry, dtype, nx, nu, general):
    return RECORDED[dtype, (nx, nu)]


@pytest.fixture(scope="module")
def solver():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    s = binding.Solver(0)
    yield s
    s.close()


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype).reshape(-1))).cuda()


def close(a, b, tol):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.isfinite(a).all() and np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def case(nx, nu):
    """Problem data (fp32 numbers held in fp64: exact in both precisions), rho, a point, and every fp64 reference: computed once."""
    d = {k: v.astype(F64) for k, v in so.gen(nx, nu, N, seed=500 + nx, batch=B, dtype=F32).items()}
    rng = np.random.default_rng(nx)
    rho = np.array([0.5, 1.0])
    lam = rng.standard_normal((B, nx * N)).astype(F32).astype(F64)
    z = rng.standard_normal((B, d["g"].shape[1])).astype(F32).astype(F64)
    sg, didx = nx * nx + nu * nu, []
    for k in range(N):   # the diagonal entries of Q_0, R_0, ..., Q_{N-1} in one problem's packed G
        didx += [k * sg + i * (nx + 1) for i in range(nx)] + ([k * sg + nx * nx + i * (nu + 1) for i in range(nu)] if k < N - 1 else [])
    Gr = d["G"].copy()
    Gr[:, didx] += rho[:, None]

    def norms(G, C, gb, cb, zb, lb):
        Gd, Cd, gv, cv = so.dense_kkt(nx, nu, N, G, C, gb, cb)
        return [np.abs(Gd @ zb + gv + Cd.T @ lb).max(), np.abs(Cd @ zb - cv).max()]

    ref = {"d": d, "rho": rho, "lam": lam, "z": z}
    for name, G, shared in (("plain", d["G"], False), ("reg", Gr, False), ("shared", d["G"], True)):
        m = [0 if shared else b for b in range(B)]
        ref[name] = {
            "form": [so.form_schur(nx, nu, N, G[m[b]], d["C"][m[b]], d["g"][b], d["c"][b]) for b in range(B)],
            "z": [so.recover_primal(nx, nu, N, G[m[b]], d["C"][m[b]], d["g"][b], lam[b]) for b in range(B)],
            "res": [norms(G[m[b]], d["C"][m[b]], d["g"][b], d["c"][b], z[b], lam[b]) for b in range(B)],
        }
    return ref


def call(solver, entry, nx, nu, dtype, r):
    """The entry point on the case's data: (status, outputs as host arrays [B, .])."""
    d = r["d"]
    G, C, g, c = (dev(d[k], dtype) for k in "GCgc")
    G1, C1 = dev(d["G"][0], dtype), dev(d["C"][0], dtype)
    kind = "reg" if entry.endswith("_reg") else "shared" if entry.endswith("_shared") else "plain"
    Ginv = dev(np.stack([f[2] for f in r[kind]["form"]])[:1 if kind == "shared" else B], dtype)   # the reference's G^-1, cast
    rho, lam, z = dev(r["rho"], dtype), dev(r["lam"], dtype), dev(r["z"], dtype)
    try:
        if entry == "form_schur":
            out = solver.form_schur(nx, nu, N, B, G, C, g, c)
        elif entry == "form_schur_reg":
            out = solver.form_schur_reg(nx, nu, N, B, G, C, g, c, rho)
        elif entry == "recover_primal":
            out = (solver.recover_primal(nx, nu, N, B, Ginv, C, g, lam),)
        elif entry == "recover_primal_shared":
            out = (solver.recover_primal_shared(nx, nu, N, B, Ginv, C1, g, lam),)
        elif entry == "form_gamma":
            out = (solver.form_gamma(nx, nu, N, B, Ginv, C, g, c),)
        elif entry == "form_gamma_shared":
            out = (solver.form_gamma_shared(nx, nu, N, B, Ginv, C1, g, c),)
        elif entry == "kkt_residual":
            out = (solver.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam),)
        elif entry == "kkt_residual_shared":
            out = (solver.kkt_residual_shared(nx, nu, N, B, G1, C1, g, c, z, lam),)
        else:
            out = (solver.kkt_residual_reg(nx, nu, N, B, G, C, g, c, rho, z, lam),)
    except binding.GbdPcgError as e:
        return int(re.search(r"status (\d+)", str(e)).group(1)), None
    torch.cuda.synchronize()
    return OK, [t.cpu().numpy().reshape(B, -1) for t in out]


def check_outputs(entry, out, r, dtype, what):
    kind = "reg" if entry.endswith("_reg") else "shared" if entry.endswith("_shared") else "plain"
    ref, tol = r[kind], TOL[dtype]
    for b in range(B):
        if entry.startswith("form_schur"):
            for got, want, name in zip(out, ref["form"][b], ("S", "gamma", "Ginv")):
                assert close(got[b], want, tol), (what, name, b)
        elif entry.startswith("recover_primal"):
            assert close(out[0][b], ref["z"][b], 10 * tol), (what, "z", b)
        elif entry.startswith("form_gamma"):
            assert close(out[0][b], ref["form"][b][1], tol), (what, "gamma", b)
        else:
            assert close(out[0][b], ref["res"][b], 10 * tol), (what, "norms", b)


def run(solver, monkeypatch, entry, dtype, nx, nu):
    """Both dispatch modes of one entry point at one shape: [(general, status)], the outputs of accepted calls checked."""
    r = case(nx, nu)
    seen = []
    for general in (False, True):
        if general:
            monkeypatch.setenv("GBDPCG_SCHUR_GENERAL", "1")
        else:
            monkeypatch.delenv("GBDPCG_SCHUR_GENERAL", raising=False)
        status, out = call(solver, entry, nx, nu, dtype, r)
        print(f"{entry} {np.dtype(dtype).name} ({nx}, {nu}) general={int(general)}: status {status}")
        if status == OK:
            check_outputs(entry, out, r, dtype, (entry, np.dtype(dtype).name, nx, nu, general))
        seen.append((general, status))
    monkeypatch.delenv("GBDPCG_SCHUR_GENERAL", raising=False)
    return seen


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("entry", ENTRIES)
def test_status_of_every_launcher_and_shape(solver, monkeypatch, entry, dtype):
    for nx, nu in shapes(dtype):
        for general, status in run(solver, monkeypatch, entry, dtype, nx, nu):
            assert status == recorded_status(entry, dtype, nx, nu, general), (entry, np.dtype(dtype).name, nx, nu, general, status)
