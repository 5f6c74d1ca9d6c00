#!/usr/bin/env python3
"""What the KKT backward pass costs, in ONE process on one device:
    python gbd-pcg_amd/tools/grad_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_grad.txt

Per precision at 1024 x (nx 14, nu 7, N 128): windows of K calls between two device events, R rounds, median and range --
    the gbdpcg_kkt_grad_* launch alone                   (purely write-bound: (nx^2 + nu^2 + nx^2 + nx nu) elements per knot)
    the gbdpcg_kkt_grad_shared_* launch alone            (one problem's worth out, the whole batch of vectors in)
    the kkt_backward graph replay next to the kkt_resolve graph replay of the same run, alternating (both from lambda = 0)
    the same gradients in plain torch: what a caller writes today from the (z, lambda, a_z, a_lambda) the solves return -- batched
    outer products per block, packed into the layouts of G and C
    loss.backward() through gbd_pcg_amd.autograd.kkt_solve (l = 1/2 ||z||^2; a fresh forward pass outside the timed span each
    time), and, with --against FILE, the same through another version of autograd.py (the parent commit's, say:
    git show HEAD~1:gbd-pcg_amd/autograd.py > FILE), the two alternating in one run
The grad launch is reported against the bytes it must write (reads are 0.5 % of that) as a fraction of the 8 TB/s HBM peak."""
import argparse
import importlib.util
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import autograd, binding  # noqa: E402
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


def torch_grads(nx, nu, N, B, z, lam, az, alam):
    """The formulas of include/gbdpcg.h in strided torch: (gG, gC) packed like G and C."""
    sv, sg, sc = nx + nu, nx * nx + nu * nu, nx * (nx + nu)
    zp = torch.nn.functional.pad(z.view(B, -1), (0, nu)).view(B, N, sv)
    ap = torch.nn.functional.pad(az.view(B, -1), (0, nu)).view(B, N, sv)
    x, u, ax, au = zp[..., :nx], zp[..., nx:], ap[..., :nx], ap[..., nx:]
    # column-major blocks: entry (i, j) at j * rows + i, i.e. the [j, i] element of a row-major array
    gQ = 0.5 * (x.unsqueeze(-1) * ax.unsqueeze(-2) + ax.unsqueeze(-1) * x.unsqueeze(-2))
    gR = 0.5 * (u.unsqueeze(-1) * au.unsqueeze(-2) + au.unsqueeze(-1) * u.unsqueeze(-2))
    gG = torch.cat([gQ.reshape(B, N, nx * nx), gR.reshape(B, N, nu * nu)], 2).reshape(B, N * sg)[:, :N * sg - nu * nu]
    l, al = lam.view(B, N, nx)[:, 1:], alam.view(B, N, nx)[:, 1:]
    gC = -(zp[:, :-1].unsqueeze(-1) * al.unsqueeze(-2) + ap[:, :-1].unsqueeze(-1) * l.unsqueeze(-2))
    return gG.reshape(-1).contiguous(), gC.reshape(B, (N - 1) * sc).reshape(-1).contiguous()


def backward_window(mod, s, nx, nu, N, G, C, g, c, a, count):
    """ms per loss.backward() of mod.kkt_solve: device time between an event in front of the call and one behind it."""
    total = 0.0
    for _ in range(count):
        z, _ = mod.kkt_solve(s, nx, nu, N, G, C, g, c, tol=a.tol, max_iter=a.max_iter)
        loss = 0.5 * (z * z).sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
        for t in (G, C, g, c):
            t.grad = None
    return total / count


def autograd_backward(s, nx, nu, N, G, C, g, c, a, against):
    mods = {"this tree": autograd}
    if against is not None:
        mods[a.against] = against
    leaves = [t.clone().requires_grad_() for t in (G, C, g, c)]
    t = {k: [] for k in mods}
    for m in mods.values():
        backward_window(m, s, nx, nu, N, *leaves, a, a.warmup)
    for _ in range(a.rounds):
        for k, m in mods.items():
            t[k].append(backward_window(m, s, nx, nu, N, *leaves, a, a.steps))
    for k, v in t.items():
        print(f"  autograd loss.backward(), {k:<12} {stat(v)}")
    if against is not None:
        m0, m1 = statistics.median(t["this tree"]), statistics.median(t[a.against])
        print(f"  this tree - {a.against}: {1e3 * (m0 - m1):.1f} us ({100.0 * (m0 - m1) / m1:.1f} %)")


def one_precision(s, nx, nu, N, B, dtype, a, against=None):
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
    s.kkt_step(nx, nu, N, B, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=a.tol, max_iter=a.max_iter, iters=it, max_iter_exit=fl)
    gz, nglam = z.clone(), torch.zeros_like(lam)        # l = 1/2 ||z||^2
    az, alam, agamma = torch.empty_like(z), torch.zeros_like(lam), torch.empty_like(gamma)
    gG, gC = torch.empty_like(G), torch.empty_like(C)
    sG, sC = torch.empty(G.numel() // B, dtype=td, device="cuda"), torch.empty(C.numel() // B, dtype=td, device="cuda")
    g_res = s.graph_kkt_resolve(nx, nu, N, B, Ginv, C, gz, nglam, S, Pinv, agamma, alam, None, None, a.tol, a.max_iter, it, fl, az)
    g_back = s.graph_kkt_backward(nx, nu, N, B, Ginv, C, gz, nglam, S, Pinv, agamma, z, lam, az, alam, None, None, a.tol, a.max_iter,
                                  it, fl, gG, gC)
    g_back.launch()
    torch.cuda.synchronize()
    tG, tC = torch_grads(nx, nu, N, B, z, lam, az, alam)
    scale = float(gG.abs().max())
    print(f"  adjoint PCG iterations mean {float(it.float().mean()):.2f}, ran out {int(fl.sum())}; plain torch against the kernel: "
          f"max |difference| / max |gG| {float((tG - gG).abs().max()) / scale:.1e} (G), {float((tC - gC).abs().max()) / scale:.1e} (C)")

    def replay(gr):
        alam.zero_()
        gr.launch()

    fns = {"grad": lambda: s.kkt_grad(nx, nu, N, B, z, lam, az, alam, gG=gG, gC=gC),
           "shared": lambda: s.kkt_grad_shared(nx, nu, N, B, z, lam, az, alam, gG=sG, gC=sC),
           "resolve": lambda: replay(g_res), "backward": lambda: replay(g_back),
           "torch": lambda: torch_grads(nx, nu, N, B, z, lam, az, alam)}
    for _ in range(2):
        for fn in fns.values():
            window(fn, a.warmup)
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, a.steps))
    es = np.dtype(dtype).itemsize
    must = (G.numel() + C.numel()) * es
    m = {k: statistics.median(v) for k, v in t.items()}
    print(f"  kkt_grad launch alone          {stat(t['grad'])}; writes {must / 1e6:.1f} MB -> {must / (m['grad'] * 1e-3) / 1e12:.2f} TB/s, "
          f"{100.0 * must / (m['grad'] * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    print(f"  kkt_grad_shared launch alone   {stat(t['shared'])}")
    print(f"  kkt_resolve graph replay       {stat(t['resolve'])}")
    print(f"  kkt_backward graph replay      {stat(t['backward'])}; backward - resolve: {1e3 * (m['backward'] - m['resolve']):.1f} us "
          f"({100.0 * (m['backward'] - m['resolve']) / m['resolve']:.1f} % of the resolve replay)")
    print(f"  the same gradients in torch    {stat(t['torch'])}; {m['torch'] / m['grad']:.1f} x the kkt_grad launch")
    for gr in (g_res, g_back):
        gr.close()
    autograd_backward(s, nx, nu, N, G, C, g, c, a, against)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=25)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--against", default=None, help="another version of autograd.py to time loss.backward() against")
    a = ap.parse_args()
    against = None
    if a.against:
        spec = importlib.util.spec_from_file_location("gbd_pcg_amd.autograd_against", a.against)
        against = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(against)
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    print(f"# grad_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter} "
          f"--batch {a.batch}; {torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for dtype in (np.float32, np.float64):
        print(f"{a.batch} x (nx 14, nu 7, N 128) {np.dtype(dtype).name}")
        one_precision(s, 14, 7, 128, a.batch, dtype, a, against)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
