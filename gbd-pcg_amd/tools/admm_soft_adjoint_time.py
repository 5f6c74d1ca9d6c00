#!/usr/bin/env python3
"""What the backward pass of the soft linear-row QP costs next to the hard calls it sits beside, in ONE process on one device:
    python gbd-pcg_amd/tools/admm_soft_adjoint_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm_soft_adjoint.txt

Per shape (4 + 2 random rows per knot, rho = 2, every bounded row within half of the largest |E z| of the equality-constrained solve,
kappa a quarter of the largest hard multiplier of the problem so that rows of all three kinds occur): the forward soft loop
(admm_lin_form, kkt_step, 60 replays of the admm_lin_soft_step graph) leaves y; then, alternating over R rounds of K calls between two
device events each,
  - gbdpcg_admm_lin_soft_mask_* (3 element accesses per row) next to gbdpcg_admm_grad_bounds_* over the same rows (4),
  - gbdpcg_admm_lin_soft_grad_* next to gbdpcg_admm_lin_grad_*, with the byte ratio from what each reads and writes,
  - the whole backward pass (mask, adjoint init, A replays of the admm_lin_adjoint_step graph, grad launch, kkt_grad) with the soft
    launches next to the same pass with the hard ones: the adjoint step graph is the same graph on another mask.
Median and range over the rounds; the spread (max - min) / median of every series is printed as the yardstick of what a difference
between two launches of this run means."""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

MX, MU = 4, 2
ADJ = 20       # adjoint replays of the whole backward pass


def window(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count   # ms per call


def stat(v):
    return f"{statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f}, spread {100 * (max(v) - min(v)) / statistics.median(v):.1f} %)"


def one_shape(s, nx, nu, N, B, dtype, a):
    td = torch.float32 if dtype == np.float32 else torch.float64
    kw = dict(dtype=td, device="cuda")
    mx, mu = MX, MU
    base = so.gen(nx, nu, N, seed=77, batch=8, dtype=dtype)
    arr = {k: np.tile(base[k], ((B + 7) // 8, 1))[:B] for k in "GCgc"}
    arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=dtype)[:, None] / B)
    G, C, g, c = (torch.from_numpy(np.ascontiguousarray(arr[k].reshape(-1))).cuda() for k in "GCgc")
    nz, nw, ne = (nx + nu) * N - nu, (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu
    gen = torch.Generator(device="cuda").manual_seed(5)
    E = torch.randn(B * ne, generator=gen, **kw)
    rho = torch.full((B,), 2.0, **kw)
    S = torch.empty(B * 3 * nx * nx * N, **kw)
    Pinv, Ginv = torch.empty_like(S), torch.empty_like(G)
    gamma = torch.empty(B * nx * N, **kw)
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it, fl = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    res = torch.empty(B, 2, **kw)
    solve = dict(tol=a.tol, max_iter=a.max_iter, iters=it, max_iter_exit=fl)
    s.kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, **solve)     # the equality-constrained solve places the bounds
    w, y = torch.zeros(B * nw, **kw), torch.zeros(B * nw, **kw)
    free = torch.full((B * nw,), float("inf"), **kw)
    s.admm_lin_update(nx, nu, mx, mu, N, B, g, E, -free, free, rho, z, w, y, torch.empty_like(g), res=res)     # w = E z
    bound = 0.5 * w.view(B, nw)[:, mx:].abs().amax(dim=1, keepdim=True)
    lo, hi = -free.view(B, nw).clone(), free.view(B, nw).clone()
    lo[:, mx:], hi[:, mx:] = (-bound).expand(B, nw - mx), bound.expand(B, nw - mx)
    lo, hi = lo.reshape(-1).contiguous(), hi.reshape(-1).contiguous()
    Gt = s.admm_lin_form(nx, nu, mx, mu, N, B, G, E, rho)

    def forward(kappa):
        lam.zero_(), w.zero_(), y.zero_()
        s.kkt_step(nx, nu, N, B, Gt, C, g, c, S, gamma, Ginv, Pinv, lam, z, **solve)
        gt = s.admm_lin_soft_init(nx, nu, mx, mu, N, B, g, E, lo, hi, kappa, rho, w, y)
        gr = s.graph_admm_lin_soft_step(nx, nu, mx, mu, N, B, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, None, None, a.tol,
                                        a.max_iter, it, fl, z, w, y, gt, res)
        for _ in range(60):
            gr.launch()
        torch.cuda.synchronize()
        gr.close()

    forward(free)                                                          # hard rows: the multipliers that size kappa
    kap = 0.25 * (2.0 * y.view(B, nw).abs().amax(dim=1, keepdim=True))
    kappa = kap.expand(B, nw).reshape(-1).contiguous()
    forward(kappa)
    yf, zf = y.clone(), z.clone()
    theta = kappa / 2.0
    sat, held = yf.abs() >= theta, (yf != 0) & (yf.abs() < theta)
    print(f"  after 60 forward soft iterations: max ||E z - w||_inf {float(res[:, 0].max()):.2e}; of {B * nw} rows {int(sat.sum())} "
          f"saturated, {int(held.sum())} held")
    gz, nglam = torch.randn(B * nz, generator=gen, **kw), torch.zeros_like(gamma)
    gamma_a, alam, az = torch.empty_like(gamma), torch.zeros_like(gamma), torch.empty_like(g)
    wa, ya, res_a = torch.zeros_like(yf), torch.zeros_like(yf), torch.empty_like(res)
    it_a, fl_a = torch.zeros_like(it), torch.zeros_like(fl)
    ym = s.admm_lin_soft_mask(nx, nu, mx, mu, N, B, yf, kappa, rho)
    gta = torch.empty_like(gz)
    graphs = {}
    for name, mask in (("soft", ym), ("hard", yf)):       # the same graph on the two masks
        graphs[name] = s.graph_admm_lin_adjoint_step(nx, nu, mx, mu, N, B, Ginv, C, gz, nglam, E, mask, rho, S, Pinv, gamma_a, alam, None,
                                                     None, a.tol, a.max_iter, it_a, fl_a, az, wa, ya, gta, res_a)
    glo, ghi, gk, gE = torch.empty_like(yf), torch.empty_like(yf), torch.empty_like(yf), torch.empty_like(E)
    gG, gC = torch.empty_like(G), torch.empty_like(C)

    def backward(soft):
        mask = ym if soft else yf
        if soft:
            s.admm_lin_soft_mask(nx, nu, mx, mu, N, B, yf, kappa, rho, ym=ym)
        wa.zero_(), ya.zero_(), alam.zero_()
        s.admm_lin_adjoint_init(nx, nu, mx, mu, N, B, gz, E, mask, rho, wa, ya, gta=gta)
        for _ in range(ADJ):
            graphs["soft" if soft else "hard"].launch()
        if soft:
            s.admm_lin_soft_grad(nx, nu, mx, mu, N, B, zf, az, E, yf, ya, kappa, rho, glo=glo, ghi=ghi, gkappa=gk, gE=gE)
        else:
            s.admm_lin_grad(nx, nu, mx, mu, N, B, zf, az, yf, ya, rho, glo=glo, ghi=ghi, gE=gE)
        s.kkt_grad(nx, nu, N, B, zf, lam, az, alam, gG=gG, gC=gC)

    backward(True)
    torch.cuda.synchronize()
    runs = {
        "mask": lambda: s.admm_lin_soft_mask(nx, nu, mx, mu, N, B, yf, kappa, rho, ym=ym),
        "bounds": lambda: s.admm_grad_bounds(mx, mu, N, B, yf, rho, ya, glo=glo, ghi=ghi),
        "soft_grad": lambda: s.admm_lin_soft_grad(nx, nu, mx, mu, N, B, zf, az, E, yf, ya, kappa, rho, glo=glo, ghi=ghi, gkappa=gk, gE=gE),
        "hard_grad": lambda: s.admm_lin_grad(nx, nu, mx, mu, N, B, zf, az, yf, ya, rho, glo=glo, ghi=ghi, gE=gE),
        "soft_back": lambda: backward(True),
        "hard_back": lambda: backward(False),
    }
    count = {k: (max(1, a.steps // ADJ) if k.endswith("back") else a.steps) for k in runs}
    for _ in range(2):
        for k, fn in runs.items():
            window(fn, max(1, a.warmup // (ADJ if k.endswith("back") else 1)))
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(window(fn, count[k]))
    es = np.dtype(dtype).itemsize
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"  admm_lin_soft_mask            {stat(t['mask'])}; {3 * nw * es * B / 1e6:.1f} MB")
    print(f"  admm_grad_bounds on the rows  {stat(t['bounds'])}; {4 * nw * es * B / 1e6:.1f} MB")
    print(f"  mask / grad_bounds: {med['mask'] / med['bounds']:.3f} (bytes: 0.750)")
    hard_b, soft_b = 2 * nz + 2 * nw + ne + 2 * nw, 2 * nz + 3 * nw + int(sat.sum()) / B * nx + ne + 3 * nw
    print(f"  admm_lin_soft_grad            {stat(t['soft_grad'])}; {soft_b * es * B / 1e6:.1f} MB (z, az, yf, ya, kappa, the saturated rows "
          f"of E in; gE, glo, ghi, gkappa out)")
    print(f"  admm_lin_grad                 {stat(t['hard_grad'])}; {hard_b * es * B / 1e6:.1f} MB")
    print(f"  soft grad / hard grad: {med['soft_grad'] / med['hard_grad']:.3f} (bytes: {soft_b / hard_b:.3f})")
    print(f"  backward pass, {ADJ} adjoint replays, soft launches {stat(t['soft_back'])}")
    print(f"  backward pass, {ADJ} adjoint replays, hard launches {stat(t['hard_back'])}")
    print(f"  soft - hard: {1e3 * (med['soft_back'] - med['hard_back']):.1f} us; mask + (soft grad - hard grad): "
          f"{1e3 * (med['mask'] + med['soft_grad'] - med['hard_grad']):.1f} us")
    for gr in graphs.values():
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
    print(f"# admm_soft_adjoint_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}), {MX} + {MU} rows, {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
