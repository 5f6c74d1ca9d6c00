#!/usr/bin/env python3
"""What the splitting update of box-constrained ADMM costs next to the solve it follows, in ONE process on one device:
    python gbd-pcg_amd/tools/admm_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm.txt

Per shape: the gbdpcg_admm_update_* launch alone (K launches between two device events), then windows of K graph replays between
two device events, kkt_resolve / admm_step alternating, R rounds; median and range over the rounds.  The factorisation is that of
G + rho I (kkt_step_reg, rho = 2), the bounds hold every input within half of the largest unconstrained one, and every replay
starts from lambda = 0 (the zero fill is inside every window alike) so both graphs solve systems of the same kind.  The update is
reported as a fraction of the resolve replay of the same run, and its algorithmic bytes -- 9 accesses per element of z, rho and the
two norms per problem: (9 nz s + 3 s) batch -- against the 8 TB/s HBM peak."""
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
    # inputs within half of the largest input of the solution without the box
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
    g_res = s.graph_kkt_resolve(nx, nu, N, B, Ginv, C, gt, c, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z)
    g_admm = s.graph_admm_step(nx, nu, N, B, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z,
                               w, y, gt, res)

    # the soft twin on a state of its own: the same bounds, kappa = +Inf for the first half of the batch and a quarter of the bound
    # for the second, so every branch of the soft line is taken
    kappa = torch.full((B, nz), float("inf"), dtype=td, device="cuda")
    kappa[B // 2:] = (0.25 * bound[B // 2:]).expand(B - B // 2, nz)
    kappa = kappa.reshape(-1).contiguous()
    ws, ys, res_s = torch.zeros_like(g), torch.zeros_like(g), torch.empty_like(res)
    gts = s.admm_soft_init(nx, nu, N, B, g, lo, hi, kappa, rho, ws, ys)
    g_soft = s.graph_admm_soft_step(nx, nu, N, B, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it,
                                    fl, z, ws, ys, gts, res_s)

    def replay(gr):
        lam.zero_()
        gr.launch()

    def update_only():
        s.admm_update(nx, nu, N, B, g, lo, hi, rho, z, w, y, gt, res=res)

    def soft_update_only():
        s.admm_soft_update(nx, nu, N, B, g, lo, hi, kappa, rho, z, ws, ys, gts, res=res_s)

    # a few iterations first: the loop does what it is for
    for _ in range(30):
        g_admm.launch()
    torch.cuda.synchronize()
    print(f"  after 30 iterations: max ||z - w||_inf {float(res[:, 0].max()):.2e}, max rho ||w+ - w||_inf {float(res[:, 1].max()):.2e}, "
          f"{int((y != 0).sum())} of {int(is_u.sum()) * B} bounded entries active, PCG iterations mean {float(it.float().mean()):.2f}, "
          f"ran out {int(fl.sum())}")
    for _ in range(30):
        g_soft.launch()
    torch.cuda.synchronize()
    for _ in range(2):
        window(update_only, a.warmup)
        window(soft_update_only, a.warmup)
        for gr in (g_res, g_admm, g_soft):
            window(lambda: replay(gr), a.warmup)
    t = {"update": [], "resolve": [], "admm": [], "soft_update": [], "soft": []}
    for _ in range(a.rounds):
        t["update"].append(window(update_only, a.steps))
        t["soft_update"].append(window(soft_update_only, a.steps))
        t["resolve"].append(window(lambda: replay(g_res), a.steps))
        t["admm"].append(window(lambda: replay(g_admm), a.steps))
        t["soft"].append(window(lambda: replay(g_soft), a.steps))
    es = np.dtype(dtype).itemsize
    must = (9 * nz * es + 3 * es) * B
    tu, tr, ta = (statistics.median(t[k]) for k in ("update", "resolve", "admm"))
    print(f"  admm_update launch alone       {stat(t['update'])}; algorithmic bytes {must / 1e6:.1f} MB -> {must / (tu * 1e-3) / 1e12:.2f} TB/s, "
          f"{100.0 * must / (tu * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    print(f"  kkt_resolve graph replay       {stat(t['resolve'])}")
    print(f"  admm_step graph replay         {stat(t['admm'])}")
    print(f"  update alone / resolve replay: {100.0 * tu / tr:.1f} %;  admm_step replay - resolve replay: {1e3 * (ta - tr):.1f} us "
          f"({100.0 * (ta - tr) / tr:.1f} % of the resolve replay)")
    # the soft twin of the same run: 10 accesses per element against 9, and one division per element
    tsu, tsa = statistics.median(t["soft_update"]), statistics.median(t["soft"])
    print(f"  admm_soft_update launch alone  {stat(t['soft_update'])}; {tsu / tu:.3f} of the hard update launch (bytes: 10/9 = 1.111)")
    print(f"  admm_soft_step graph replay    {stat(t['soft'])}; {tsa / ta:.3f} of the hard step replay")
    for gr in (g_res, g_admm, g_soft):
        gr.close()


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
    print(f"# admm_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64), (12, 4, 128, 1024, np.float32)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}) {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
