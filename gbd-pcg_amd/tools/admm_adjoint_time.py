#!/usr/bin/env python3
"""What the adjoint update of the box QP's backward pass costs next to the box update it mirrors, in ONE process on one device:
    python gbd-pcg_amd/tools/admm_adjoint_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm_adjoint.txt

Per shape: the forward loop (kkt_step_reg, rho = 2, every input within half of the largest unconstrained one, 60 replays of the
admm_step graph) leaves the mask y; then the gbdpcg_admm_update_* and gbdpcg_admm_adjoint_update_* launches alone (K launches between
two device events each) and windows of K graph replays of admm_step / admm_adjoint_step, alternating, R rounds; median and range over
the rounds.  Every replay starts from lambda = 0 (the zero fill is inside every window alike).  Algorithmic bytes: 9 accesses per
element for the box update, 8 for the adjoint one, rho and the two norms per problem, against the 8 TB/s HBM peak."""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s


def window(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count   # ms per call


def stat(v):
    return f"{statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def one_shape(s, nx, nu, N, B, dtype, a):
    td = torch.float32 if dtype == np.float32 else torch.float64
    base = so.gen(nx, nu, N, seed=77, batch=8, dtype=dtype)
    arr = {k: np.tile(base[k], ((B + 7) // 8, 1))[:B] for k in "GCgc"}
    arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=dtype)[:, None] / B)
    G, C, g, c = (torch.from_numpy(np.ascontiguousarray(arr[k].reshape(-1))).cuda() for k in "GCgc")
    rho = torch.full((B,), 2.0, dtype=td, device="cuda")
    S = torch.empty(B * 3 * nx * nx * N, dtype=td, device="cuda")
    Pinv, Ginv = torch.empty_like(S), torch.empty_like(G)
    gamma = torch.empty(B * nx * N, dtype=td, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    res = torch.empty(B, 2, dtype=td, device="cuda")
    s.kkt_step_reg(nx, nu, N, B, G, C, g, c, rho, S, gamma, Ginv, Pinv, lam, z, tol=a.tol, max_iter=a.max_iter, iters=it, max_iter_exit=fl)
    torch.cuda.synchronize()
    sv, nz = nx + nu, (nx + nu) * N - nu
    is_u = torch.zeros(nz, dtype=torch.bool, device="cuda")
    for k in range(N - 1):
        is_u[k * sv + nx:(k + 1) * sv] = True
    bound = 0.5 * z.view(B, nz)[:, is_u].abs().amax(dim=1, keepdim=True)
    lo, hi = torch.full((B, nz), float("-inf"), dtype=td, device="cuda"), torch.full((B, nz), float("inf"), dtype=td, device="cuda")
    lo[:, is_u], hi[:, is_u] = (-bound).expand(B, int(is_u.sum())), bound.expand(B, int(is_u.sum()))
    lo, hi = lo.reshape(-1).contiguous(), hi.reshape(-1).contiguous()
    w, y = torch.zeros_like(g), torch.zeros_like(g)
    gt = s.admm_init(nx, nu, N, B, g, lo, hi, rho, w, y)
    g_admm = s.graph_admm_step(nx, nu, N, B, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z,
                               w, y, gt, res)
    for _ in range(60):
        g_admm.launch()
    torch.cuda.synchronize()
    print(f"  after 60 forward iterations: max ||z - w||_inf {float(res[:, 0].max()):.2e}, {int((y != 0).sum())} of "
          f"{int(is_u.sum()) * B} bounded entries active")
    # the adjoint on a state of its own; the mask is a copy of the forward y, which the forward windows below go on updating
    yf = y.clone()
    gz, nglam = torch.randn_like(g), torch.zeros_like(gamma)
    gamma_a, alam, az = torch.empty_like(gamma), torch.zeros_like(gamma), torch.empty_like(g)
    wa, ya, res_a = torch.zeros_like(g), torch.zeros_like(g), torch.empty_like(res)
    it_a, fl_a = torch.zeros_like(it), torch.zeros_like(fl)
    gta = s.admm_adjoint_init(nx, nu, N, B, gz, yf, rho, wa, ya)
    g_adj = s.graph_admm_adjoint_step(nx, nu, N, B, Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma_a, alam, None, None, a.tol, a.max_iter, it_a,
                                      fl_a, az, wa, ya, gta, res_a)
    for _ in range(60):
        g_adj.launch()
    torch.cuda.synchronize()
    print(f"  after 60 adjoint iterations: max ||az - wa||_inf {float(res_a[:, 0].max()):.2e}, PCG iterations mean "
          f"{float(it_a.float().mean()):.2f}, ran out {int(fl_a.sum())}")

    def replay(gr, start):
        start.zero_()
        gr.launch()

    def update_only():
        s.admm_update(nx, nu, N, B, g, lo, hi, rho, z, w, y, gt, res=res)

    def adjoint_update_only():
        s.admm_adjoint_update(nx, nu, N, B, gz, yf, rho, az, wa, ya, gta, res=res_a)

    runs = {"update": update_only, "adjoint_update": adjoint_update_only, "admm": lambda: replay(g_admm, lam),
            "adjoint": lambda: replay(g_adj, alam)}
    for _ in range(2):
        for fn in runs.values():
            window(fn, a.warmup)
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(window(fn, a.steps))
    es = np.dtype(dtype).itemsize
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, acc, label in (("update", 9, "admm_update launch alone        "), ("adjoint_update", 8, "admm_adjoint_update launch alone")):
        must = (acc * nz * es + 3 * es) * B
        print(f"  {label} {stat(t[k])}; algorithmic bytes {must / 1e6:.1f} MB -> {must / (med[k] * 1e-3) / 1e12:.2f} TB/s, "
              f"{100.0 * must / (med[k] * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    print(f"  adjoint update / box update: {med['adjoint_update'] / med['update']:.3f} (bytes: 8/9 = 0.889)")
    print(f"  admm_step graph replay           {stat(t['admm'])}")
    print(f"  admm_adjoint_step graph replay   {stat(t['adjoint'])}; {med['adjoint'] / med['admm']:.3f} of the forward step replay")
    g_admm.close()
    g_adj.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    print(f"# admm_adjoint_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}) {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
