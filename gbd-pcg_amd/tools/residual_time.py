#!/usr/bin/env python3
"""What the device-side KKT residual norms (gbdpcg_kkt_residual_*) cost next to the step whose result they judge, in ONE process
on one device:  python gbd-pcg_amd/tools/residual_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_residual.txt

Per shape: windows of K launches between two device events -- the kkt_residual launch alone, the recover_primal launch alone
(the same class of data movement) and the kkt_step graph replay (every replay from lambda = 0) -- alternating, R rounds; median
and range over the rounds.  Before timing, the norms of the step's (z, lambda) are printed, and checked against a torch fp64
evaluation of one problem.  Must-move bytes of the residual launch: G, C, g, c, z, lambda read once and two numbers per problem
written, from the shapes; the share of the 8 TB/s HBM peak is that over the launch time."""
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
    S = torch.empty(B * 3 * nx * nx * N, dtype=td, device="cuda")
    Pinv, Ginv = torch.empty_like(S), torch.empty_like(G)
    gamma = torch.empty(B * nx * N, dtype=td, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    res = torch.empty(B, 2, dtype=td, device="cuda")
    g_step = s.graph_kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, None, None, a.tol, a.max_iter, it, fl, z)

    def step():
        lam.zero_()
        g_step.launch()

    def residual():
        s.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam, res=res)

    def recover():
        s.recover_primal(nx, nu, N, B, Ginv, C, g, lam, z=z)

    # what the step left behind, and the device norms against fp64 for the last problem
    step()
    residual()
    torch.cuda.synchronize()
    r = res.cpu().numpy().astype(np.float64)
    b = B - 1
    Gd, Cd, gv, cv = so.dense_kkt(nx, nu, N, arr["G"][b], arr["C"][b], arr["g"][b], arr["c"][b])
    zb, lb = z.view(B, -1)[b].cpu().numpy().astype(np.float64), lam.view(B, -1)[b].cpu().numpy().astype(np.float64)
    ref = np.array([np.abs(Gd @ zb + gv + Cd.T @ lb).max(), np.abs(Cd @ zb - cv).max()])
    print(f"  after kkt_step (tol {a.tol}, iterations mean {float(it.float().mean()):.2f}, ran out {int(fl.sum())}): stationarity max "
          f"{r[:, 0].max():.3e}, feasibility max {r[:, 1].max():.3e} over the batch; problem {b}: device {r[b, 0]:.3e} / {r[b, 1]:.3e}, "
          f"fp64 {ref[0]:.3e} / {ref[1]:.3e}")
    ok = bool(np.isfinite(r).all())

    fns = {"res": residual, "rec": recover, "step": step}
    for _ in range(2):
        for fn in fns.values():
            window(fn, a.warmup)
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, a.steps))
    es = np.dtype(dtype).itemsize
    sz = so.sizes(nx, nu, N)
    must = (sz["G"] + sz["C"] + 2 * sz["g"] + 2 * sz["c"] + 2) * es * B
    must_rec = (sz["Ginv"] + sz["C"] + 2 * sz["g"] + sz["c"]) * es * B
    tr, tc = statistics.median(t["res"]) * 1e-3, statistics.median(t["rec"]) * 1e-3
    print(f"  kkt_residual launch alone      {stat(t['res'])}; must-move {must / 1e6:.1f} MB -> {must / tr / 1e12:.2f} TB/s, "
          f"{100.0 * must / tr / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    print(f"  recover_primal launch alone    {stat(t['rec'])}; must-move {must_rec / 1e6:.1f} MB -> {must_rec / tc / 1e12:.2f} TB/s, "
          f"{100.0 * must_rec / tc / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    print(f"  kkt_step graph replay          {stat(t['step'])}")
    print(f"  residual launch / kkt_step replay: {statistics.median(t['res']) / statistics.median(t['step']):.3f}")
    g_step.close()
    return ok


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
    print(f"# residual_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    ok = True
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64), (12, 4, 128, 1024, np.float32)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}) {np.dtype(dtype).name}")
        ok = one_shape(s, nx, nu, N, B, dtype, a) and ok
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
