#!/usr/bin/env python3
"""What the optimality test costs next to the launches it stands beside in a loop, in ONE process on one device:
    python gbd-pcg_amd/tools/admm_optimality_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm_optimality.txt

Per precision at 1024 x (14, 7, 128) with 4 + 2 random rows per knot, on random operands (every launch here waits for memory; none
takes a data-dependent path), alternating over R rounds of K calls between two device events each:
  - gbdpcg_admm_lin_optimality_* and gbdpcg_admm_optimality_* (the box form) next to gbdpcg_kkt_residual_* -- the yardstick: the
    new calls move that launch's bytes plus E, w and y -- and next to gbdpcg_admm_lin_update_* and gbdpcg_admm_lin_infeas_*.
Median and range over the rounds, the algorithmic bytes of every launch, and the repeat-to-repeat spread (max - min) / median of
every launch's rounds as the yardstick of what a difference between two launches of this run means."""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

MX, MU = 4, 2


def window(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count   # ms per call


def stat(v):
    return f"{1e3 * statistics.median(v):7.1f} us (min {1e3 * min(v):.1f}, max {1e3 * max(v):.1f})"


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def one_shape(s, nx, nu, N, B, dtype, a):
    td = torch.float32 if dtype == np.float32 else torch.float64
    kw = dict(dtype=td, device="cuda")
    mx, mu = MX, MU
    base = so.gen(nx, nu, N, seed=77, batch=8, dtype=dtype)
    arr = {k: np.tile(base[k], ((B + 7) // 8, 1))[:B] for k in "GCgc"}
    G, C, g, c = (torch.from_numpy(np.ascontiguousarray(arr[k].reshape(-1))).cuda() for k in "GCgc")
    nz, nw, ne = (nx + nu) * N - nu, (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu
    nl = nx * N
    gen = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda n: torch.randn(n, generator=gen, **kw)     # noqa: E731
    E, rho = rnd(B * ne), torch.full((B,), 2.0, **kw)
    z, lam0, lam1 = rnd(B * nz), rnd(B * nl), rnd(B * nl)
    rows = dict(lo=-rnd(B * nw).abs(), hi=rnd(B * nw).abs(), y0=rnd(B * nw), y1=rnd(B * nw), w=rnd(B * nw), y=rnd(B * nw))
    box = dict(w=rnd(B * nz), y=rnd(B * nz))
    gt, res, res2 = torch.empty_like(g), torch.empty(B, 2, **kw), torch.empty(B, 2, **kw)
    cert, flag = torch.empty(B, 3, **kw), torch.empty(B, dtype=torch.uint8, device="cuda")
    opt, done = torch.empty(B, 6, **kw), torch.empty(B, dtype=torch.uint8, device="cuda")
    runs = {
        "kkt_residual": lambda: s.kkt_residual(nx, nu, N, B, G, C, g, c, z, lam1, res=res),
        "lin_update": lambda: s.admm_lin_update(nx, nu, mx, mu, N, B, g, E, rows["lo"], rows["hi"], rho, z, rows["w"], rows["y"], gt, res=res2),
        "lin_infeas": lambda: s.admm_lin_infeas(nx, nu, mx, mu, N, B, C, c, E, rows["lo"], rows["hi"], rho, lam0, lam1, rows["y0"], rows["y1"],
                                                0.1, cert=cert, flag=flag),
        "lin_optimality": lambda: s.admm_lin_optimality(nx, nu, mx, mu, N, B, G, C, g, c, E, rho, z, lam1, rows["y0"], rows["y1"], 1e-4, 1e-4,
                                                        opt=opt, done=done),
        "optimality": lambda: s.admm_optimality(nx, nu, N, B, G, C, g, c, rho, z, lam1, box["w"], box["y"], 1e-4, 1e-4, opt=opt, done=done),
    }
    for _ in range(2):
        for fn in runs.values():
            window(fn, a.warmup)
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(window(fn, a.steps))
    es = np.dtype(dtype).itemsize
    med = {k: statistics.median(v) for k, v in t.items()}
    nc, ng = nx * (nx + nu) * (N - 1), (nx * nx + nu * nu) * N - nu * nu
    bytes_ = {   # per problem, in elements: what each launch has to read and write once
        "kkt_residual": ng + nc + 2 * nz + 2 * nl + 2,
        "lin_update": 6 * nw + 3 * nz + ne + 3,
        "lin_infeas": nc + ne + 3 * nl + 3 * nw + 4,
        "lin_optimality": ng + nc + 2 * nz + 2 * nl + ne + 2 * nw + 7,      # kkt_residual's, plus E, w, y
        "optimality": ng + nc + 2 * nz + 2 * nl + 2 * nz + 7,
    }
    names = {"kkt_residual": "kkt_residual", "lin_update": "admm_lin_update", "lin_infeas": "admm_lin_infeas",
             "lin_optimality": "admm_lin_optimality", "optimality": "admm_optimality"}
    for k in runs:
        mb = bytes_[k] * es * B / 1e6
        print(f"  {names[k]:20s} {stat(t[k])}; algorithmic bytes {mb:6.1f} MB -> {mb * 1e6 / (med[k] * 1e-3) / 1e12:.2f} TB/s; "
              f"spread {100 * spread(t[k]):.1f} %")
    print(f"  admm_lin_optimality / kkt_residual: {med['lin_optimality'] / med['kkt_residual']:.3f} in time, "
          f"{bytes_['lin_optimality'] / bytes_['kkt_residual']:.3f} in bytes; / admm_lin_update: {med['lin_optimality'] / med['lin_update']:.3f}; "
          f"/ admm_lin_infeas: {med['lin_optimality'] / med['lin_infeas']:.3f}; admm_optimality / kkt_residual: "
          f"{med['optimality'] / med['kkt_residual']:.3f} in time, {bytes_['optimality'] / bytes_['kkt_residual']:.3f} in bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    print(f"# admm_optimality_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds}; {torch.cuda.get_device_name(0)}; "
          f"{s.lib.gbdpcg_version().decode()}")
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}), {MX} + {MU} rows, {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
