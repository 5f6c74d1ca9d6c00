#!/usr/bin/env python3
"""What a control tick costs on a frozen linearisation (gbdpcg_kkt_resolve_*) next to a full inner step (gbdpcg_kkt_step_*), in
ONE process on one device:  python gbd-pcg_amd/tools/resolve_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_resolve.txt

Per shape: the form_gamma launch alone (K launches between two device events), then windows of K graph replays between two
device events, kkt_step / kkt_resolve (handle's default symmetric mode: S and Phi^-1 tested on every tick) / kkt_resolve with
gbdpcg_set_symmetric(h, 1) alternating, R rounds; median and range over the rounds.  Every replay starts from lambda = 0 (the
zero fill is inside every window alike), so all three solve the same systems with the same iteration counts.  Before timing,
the resolve's lambda and z are compared with the step's on the same data.  Must-move bytes of the gamma launch: G^-1, C, g, c
read once and gamma written, from the shapes; the share of the 8 TB/s HBM peak is that over the launch time."""
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
    s.set_symmetric(2)
    g_step = s.graph_kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, None, None, a.tol, a.max_iter, it, fl, z)
    g_res2 = s.graph_kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z)
    s.set_symmetric(1)
    g_res1 = s.graph_kkt_resolve(nx, nu, N, B, Ginv, C, g, c, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z)
    s.set_symmetric(2)

    def replay(gr):
        lam.zero_()
        gr.launch()

    # same answers first: the step factors, the resolves reproduce its lambda and z from the kept S, Phi^-1, G^-1
    replay(g_step)
    torch.cuda.synchronize()
    want = (lam.clone(), z.clone(), it.clone())
    for name, gr in (("mode 2", g_res2), ("mode 1", g_res1)):
        z.fill_(float("nan"))
        replay(gr)
        torch.cuda.synchronize()
        dl = float((lam - want[0]).abs().max() / want[0].abs().max())
        dz = float((z - want[1]).abs().max() / want[1].abs().max())
        print(f"  kkt_resolve ({name}) vs kkt_step on the same data: max |dlambda| / max |lambda| {dl:.2e}, max |dz| / max |z| {dz:.2e}, "
              f"iterations mean {float(it.float().mean()):.2f} (step {float(want[2].float().mean()):.2f}), ran out {int(fl.sum())}")

    def gamma_only():
        s.form_gamma(nx, nu, N, B, Ginv, C, g, c, gamma=gamma)

    for _ in range(2):
        window(gamma_only, a.warmup)
        for gr in (g_step, g_res2, g_res1):
            window(lambda: replay(gr), a.warmup)
    t = {"gamma": [], "step": [], "res2": [], "res1": []}
    for _ in range(a.rounds):
        t["gamma"].append(window(gamma_only, a.steps))
        t["step"].append(window(lambda: replay(g_step), a.steps))
        t["res2"].append(window(lambda: replay(g_res2), a.steps))
        t["res1"].append(window(lambda: replay(g_res1), a.steps))
    es = np.dtype(dtype).itemsize
    sz = so.sizes(nx, nu, N)
    must = (sz["Ginv"] + sz["C"] + sz["g"] + sz["c"] + sz["gamma"]) * es * B
    tg = statistics.median(t["gamma"]) * 1e-3
    print(f"  form_gamma launch alone        {stat(t['gamma'])}; must-move {must / 1e6:.1f} MB -> {must / tg / 1e12:.2f} TB/s, "
          f"{100.0 * must / tg / HBM_PEAK:.0f} % of the 8 TB/s HBM peak (memory-bound: 0.5 flop per byte)")
    print(f"  kkt_step graph replay          {stat(t['step'])}")
    print(f"  kkt_resolve graph replay       {stat(t['res2'])}   (symmetric mode 2, the default: S and Phi^-1 tested every tick)")
    print(f"  kkt_resolve graph replay       {stat(t['res1'])}   (symmetric mode 1: the caller vouches for the kept S)")
    faster = statistics.median(t["res2"]) < statistics.median(t["step"]) and statistics.median(t["res1"]) < statistics.median(t["step"])
    print(f"  resolve faster than step in this run: {faster}")
    for gr in (g_step, g_res2, g_res1):
        gr.close()
    return faster


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
    print(f"# resolve_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    ok = True
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64), (12, 4, 128, 1024, np.float32)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}) {np.dtype(dtype).name}")
        ok = one_shape(s, nx, nu, N, B, dtype, a) and ok
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
