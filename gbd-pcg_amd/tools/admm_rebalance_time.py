#!/usr/bin/env python3
"""What adaptive rho costs next to the calls it replaces, in ONE process on one device:
    python gbd-pcg_amd/tools/admm_rebalance_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm_rebalance.txt

Per shape, windows of K calls between two device events, the candidates alternating, R rounds; median and range over the rounds:
  - the box rebalance launch (rho, y, gt, expo) next to the gbdpcg_admm_init_* launch, which rebuilds gt alone;
  - the restep graph replay next to what a caller would replay by hand: the kkt_step_reg graph plus the admm_step graph.
The factorisation is that of G + rho I (rho = 2), the bounds hold every input within half of the largest unconstrained one, and every
replay starts from lambda = 0 (the zero fill is inside every window alike).  The residuals are rewritten in front of every window so
that a third of the problems raise rho, a third lower it and a third keep it; the limits are rho itself times / over 4, so rho stays
within a factor 4 of its start however many replays a window makes.  The launch's algorithmic bytes -- y read and written, w and g
read, gt written, rho, the two norms and expo per problem: (5 nz s + 4 s + 4) batch -- are held against the 8 TB/s HBM peak."""
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
    expo = torch.zeros(B, dtype=torch.int32, device="cuda")
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
    rule = dict(ratio=10.0, shift=1, rho_min=0.5, rho_max=8.0)
    g_step = s.graph_admm_step(nx, nu, N, B, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z,
                               w, y, gt, res)
    g_reg = s.graph_kkt_step_reg(nx, nu, N, B, G, C, gt, c, rho, S, gamma, Ginv, Pinv, lam, None, None, a.tol, a.max_iter, it, fl, z)
    g_restep = s.graph_admm_restep(nx, nu, N, B, G, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl,
                                   z, w, y, gt, res, expo, **rule)
    for _ in range(30):
        g_step.launch()
    torch.cuda.synchronize()
    print(f"  after 30 iterations: max ||z - w||_inf {float(res[:, 0].max()):.2e}, max rho ||w+ - w||_inf {float(res[:, 1].max()):.2e}, "
          f"PCG iterations mean {float(it.float().mean()):.2f}, ran out {int(fl.sum())}")
    forced = torch.ones(B, 2, dtype=td, device="cuda")
    forced[0::3, 0], forced[1::3, 1] = 100.0, 100.0

    def rebalance_only():
        s.admm_rebalance(nx, nu, N, B, g, forced, rho, w, y, gt, expo, **rule)

    def init_only():
        s.admm_init(nx, nu, N, B, g, lo, hi, rho, w, y, gt=gt)

    def restep():
        lam.zero_()
        res.copy_(forced)
        g_restep.launch()

    def by_hand():
        lam.zero_()
        res.copy_(forced)
        g_reg.launch()
        g_step.launch()

    cands = (("rebalance", rebalance_only), ("init", init_only), ("restep", restep), ("by_hand", by_hand))
    for _ in range(2):
        for _, fn in cands:
            window(fn, a.warmup)
    t = {k: [] for k, _ in cands}
    for _ in range(a.rounds):
        for k, fn in cands:
            rho.fill_(2.0)
            t[k].append(window(fn, a.steps))
    es = np.dtype(dtype).itemsize
    must = (5 * nz * es + 4 * es + 4) * B
    tb, ti, tr, th = (statistics.median(t[k]) for k, _ in cands)
    print(f"  admm_rebalance launch alone    {stat(t['rebalance'])}; algorithmic bytes {must / 1e6:.1f} MB -> {must / (tb * 1e-3) / 1e12:.2f} TB/s, "
          f"{100.0 * must / (tb * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    print(f"  admm_init launch alone         {stat(t['init'])}")
    print(f"  admm_restep graph replay       {stat(t['restep'])}")
    print(f"  kkt_step_reg + admm_step replays {stat(t['by_hand'])}   (two graphs; by hand the rescaling of y and gt would come on top)")
    print(f"  rebalance / init: {tb / ti:.2f};  restep replay - the two replays: {1e3 * (tr - th):.1f} us ({100.0 * (tr - th) / th:.1f} %)")
    for gr in (g_step, g_reg, g_restep):
        gr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    print(f"# admm_rebalance_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}) {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
