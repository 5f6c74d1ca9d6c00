#!/usr/bin/env python3
"""What the backward pass of the linear-row QP costs next to the calls it mirrors, in ONE process on one device:
    python gbd-pcg_amd/tools/admm_lin_adjoint_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm_lin_adjoint.txt

Per shape (4 + 2 random rows per knot, rho = 2, every row within half of the largest |E z| of the equality-constrained solve): the
forward loop (admm_lin_form, kkt_step, 60 replays of the admm_lin_step graph) leaves the mask y; then, alternating over R rounds
of K calls between two device events each,
  - gbdpcg_admm_lin_adjoint_update_* next to gbdpcg_admm_lin_update_* ON THE EXPLICIT DEGENERATE ROWS of the same mask (what a
    caller had to do without the adjoint calls: same bits, one array read more per row),
  - the admm_lin_adjoint_step graph replay next to the admm_lin_step replay,
  - gbdpcg_admm_lin_grad_* (bytes written over time against the 6.3 TB/s a copy achieves) next to gbdpcg_kkt_grad_*.
Median and range over the rounds; the spread (max - min) / median of the admm_lin_update rounds is printed as the yardstick of what
a difference between two launches of this run means."""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

ACHIEVABLE = 6.3e12   # bytes / s
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
    return f"{statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


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
    # the equality-constrained solve places the bounds
    s.kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=a.tol, max_iter=a.max_iter, iters=it, max_iter_exit=fl)
    w, y = torch.zeros(B * nw, **kw), torch.zeros(B * nw, **kw)
    free = torch.full((B * nw,), float("inf"), **kw)
    s.admm_lin_update(nx, nu, mx, mu, N, B, g, E, -free, free, rho, z, w, y, torch.empty_like(g), res=res)     # w = E z
    bound = 0.5 * w.view(B, nw)[:, mx:].abs().amax(dim=1, keepdim=True)
    lo, hi = -free.view(B, nw).clone(), free.view(B, nw).clone()
    lo[:, mx:], hi[:, mx:] = (-bound).expand(B, nw - mx), bound.expand(B, nw - mx)
    lo, hi = lo.reshape(-1).contiguous(), hi.reshape(-1).contiguous()
    Gt = s.admm_lin_form(nx, nu, mx, mu, N, B, G, E, rho)
    lam.zero_()
    s.kkt_step(nx, nu, N, B, Gt, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=a.tol, max_iter=a.max_iter, iters=it, max_iter_exit=fl)
    w.zero_()
    y.zero_()
    gt = s.admm_lin_init(nx, nu, mx, mu, N, B, g, E, lo, hi, rho, w, y)
    g_fwd = s.graph_admm_lin_step(nx, nu, mx, mu, N, B, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter,
                                  it, fl, z, w, y, gt, res)
    for _ in range(60):
        g_fwd.launch()
    torch.cuda.synchronize()
    print(f"  after 60 forward iterations: max ||E z - w||_inf {float(res[:, 0].max()):.2e}, {int((y != 0).sum())} of {B * (nw - mx)} "
          f"bounded rows active")
    yf, zf = y.clone(), z.clone()
    dlo = torch.where(yf != 0, torch.zeros_like(yf), -free)
    dhi = torch.where(yf != 0, torch.zeros_like(yf), free)
    gz, nglam = torch.randn(B * nz, generator=gen, **kw), torch.zeros_like(gamma)
    gamma_a, alam, az = torch.empty_like(gamma), torch.zeros_like(gamma), torch.empty_like(g)
    wa, ya, res_a = torch.zeros_like(yf), torch.zeros_like(yf), torch.empty_like(res)
    it_a, fl_a = torch.zeros_like(it), torch.zeros_like(fl)
    gta = s.admm_lin_adjoint_init(nx, nu, mx, mu, N, B, gz, E, yf, rho, wa, ya)
    g_adj = s.graph_admm_lin_adjoint_step(nx, nu, mx, mu, N, B, Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma_a, alam, None, None, a.tol,
                                          a.max_iter, it_a, fl_a, az, wa, ya, gta, res_a)
    for _ in range(60):
        g_adj.launch()
    torch.cuda.synchronize()
    print(f"  after 60 adjoint iterations: max ||E az - wa||_inf {float(res_a[:, 0].max()):.2e}, PCG iterations mean "
          f"{float(it_a.float().mean()):.2f}, ran out {int(fl_a.sum())}")
    # the explicit form on a state of its own, and the gradient outputs
    wd, yd, gtd, resd = wa.clone(), ya.clone(), gta.clone(), torch.empty_like(res)
    glo, ghi, gE = torch.empty_like(yf), torch.empty_like(yf), torch.empty_like(E)
    gG, gC = torch.empty_like(G), torch.empty_like(C)

    def replay(gr, start):
        start.zero_()
        gr.launch()

    runs = {
        "explicit": lambda: s.admm_lin_update(nx, nu, mx, mu, N, B, gz, E, dlo, dhi, rho, az, wd, yd, gtd, res=resd),
        "adjoint": lambda: s.admm_lin_adjoint_update(nx, nu, mx, mu, N, B, gz, E, yf, rho, az, wa, ya, gta, res=res_a),
        "fwd_step": lambda: replay(g_fwd, lam),
        "adj_step": lambda: replay(g_adj, alam),
        "lin_grad": lambda: s.admm_lin_grad(nx, nu, mx, mu, N, B, zf, az, yf, ya, rho, glo=glo, ghi=ghi, gE=gE),
        "kkt_grad": lambda: s.kkt_grad(nx, nu, N, B, zf, lam, az, alam, gG=gG, gC=gC),
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
    rows_bytes = lambda reads: ((reads + 2) * nw + 3 * nz + ne + 3) * es * B     # noqa: E731  (rows, z | g | gt, E, rho and the norms)
    print(f"  admm_lin_update on explicit degenerate rows {stat(t['explicit'])}; algorithmic bytes {rows_bytes(4) / 1e6:.1f} MB")
    print(f"  admm_lin_adjoint_update                     {stat(t['adjoint'])}; algorithmic bytes {rows_bytes(3) / 1e6:.1f} MB")
    print(f"  adjoint update / explicit update: {med['adjoint'] / med['explicit']:.3f} (bytes: {rows_bytes(3) / rows_bytes(4):.3f}); "
          f"repeat-to-repeat spread of the explicit update {100 * spread(t['explicit']):.1f} %, of the adjoint update "
          f"{100 * spread(t['adjoint']):.1f} %")
    print(f"  admm_lin_step graph replay                  {stat(t['fwd_step'])}")
    print(f"  admm_lin_adjoint_step graph replay          {stat(t['adj_step'])}; {med['adj_step'] / med['fwd_step']:.3f} of the forward "
          f"step replay")
    out = (ne + 2 * nw) * es * B
    print(f"  admm_lin_grad launch                        {stat(t['lin_grad'])}; {out / 1e6:.1f} MB written -> "
          f"{out / (med['lin_grad'] * 1e-3) / 1e12:.2f} TB/s, {100.0 * out / (med['lin_grad'] * 1e-3) / ACHIEVABLE:.0f} % of the "
          f"6.3 TB/s achievable rate")
    outk = (G.numel() + C.numel()) * es
    print(f"  kkt_grad launch                             {stat(t['kkt_grad'])}; {outk / 1e6:.1f} MB written -> "
          f"{outk / (med['kkt_grad'] * 1e-3) / 1e12:.2f} TB/s")
    g_fwd.close()
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
    print(f"# admm_lin_adjoint_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for nx, nu, N, B, dtype in ((14, 7, 128, 1024, np.float32), (14, 7, 128, 1024, np.float64)):
        print(f"{B} x (nx {nx}, nu {nu}, N {N}), {MX} + {MU} rows, {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
