#!/usr/bin/env python3
"""What the fused per-problem regularisation (gbdpcg_form_schur_reg_*, gbdpcg_kkt_step_reg_*) costs next to the plain calls and
next to adding rho outside the library, in ONE process on one device, interleaved:
    python gbd-pcg_amd/tools/reg_time.py [--warmup W] [--steps K] [--rounds R] [--baseline-lib PATH] > profiles/r08_reg.txt

Per shape and precision, windows of K graph replays between two device events, the five candidates alternating, R rounds;
median and range (the run-to-run spread) over the rounds:
  (a) form_schur                                        (captured on the stream, one launch)
  (b) form_schur_reg, rho_b = 0.5 + b / batch           (one launch)
  (c) the do-it-outside alternative: G copied into a second buffer, rho_b added to its diagonals (two torch kernels: 2 x |G| of
      traffic and a buffer the fused form does not need), then form_schur on the copy
  (d) kkt_step graph replay
  (e) kkt_step_reg graph replay
--baseline-lib: another build of the library (the commit before the feature) loaded beside this one; its kkt_step graph is timed
in the same rounds as (d'), so that "the existing step did not move" is measured on one box in one run.
Every step replay starts from lambda = 0 (the zero fill is inside every window alike).  Before timing, (b) is compared with (c)
(the same numbers: fl(d + rho) either way, so the same bits) and (e)'s lambda with a step on the copy."""
import argparse
import ctypes
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402


def window(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count   # ms per call


def stat(v):
    return f"{statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f}, spread {max(v) - min(v):.4f})"


def capture(fn):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):   # the capturing stream is torch's current one inside the block
        fn()
    return gr


def solver_on(path):
    """A Solver on another build of the library (only entry points that exist in both are used)."""
    lib = ctypes.CDLL(path)
    lib.gbdpcg_status_string.restype = ctypes.c_char_p
    lib.gbdpcg_last_hip_error_string.restype = ctypes.c_char_p
    lib.gbdpcg_version.restype = ctypes.c_char_p
    s = binding.Solver.__new__(binding.Solver)
    s.lib, s.h, s.device = lib, ctypes.c_void_p(), 0
    st = lib.gbdpcg_create(ctypes.byref(s.h), ctypes.c_int(0))
    assert st == binding.OK, st
    return s


def diag_index(nx, nu, N):
    sg, idx = nx * nx + nu * nu, []
    for k in range(N):
        idx += [k * sg + i * (nx + 1) for i in range(nx)]
        if k < N - 1:
            idx += [k * sg + nx * nx + i * (nu + 1) for i in range(nu)]
    return torch.tensor(idx, dtype=torch.int64, device="cuda")


def one_shape(s, base, nx, nu, N, B, dtype, a):
    td = torch.float32 if dtype == np.float32 else torch.float64
    src = so.gen(nx, nu, N, seed=77, batch=8, dtype=dtype)
    arr = {k: np.tile(src[k], ((B + 7) // 8, 1))[:B] for k in "GCgc"}
    arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=dtype)[:, None] / B)
    G, C, g, c = (torch.from_numpy(np.ascontiguousarray(arr[k].reshape(-1))).cuda() for k in "GCgc")
    rho = (0.5 + torch.arange(B, device="cuda") / B).to(td)
    G2, idx = torch.empty_like(G), diag_index(nx, nu, N)
    rho_cols = rho[:, None].expand(B, idx.numel())

    def bufs():
        S = torch.empty(B * 3 * nx * nx * N, dtype=td, device="cuda")
        gamma = torch.empty(B * nx * N, dtype=td, device="cuda")
        return dict(S=S, gamma=gamma, Ginv=torch.empty_like(G), Pinv=torch.empty_like(S), lam=torch.zeros_like(gamma), z=torch.empty_like(g),
                    it=torch.zeros(B, dtype=torch.int32, device="cuda"), fl=torch.zeros(B, dtype=torch.uint8, device="cuda"))

    f, r, o = bufs(), bufs(), bufs()

    def outside():
        G2.copy_(G)
        G2.view(B, -1).index_add_(1, idx, rho_cols)
        s.form_schur(nx, nu, N, B, G2, C, g, c, S=o["S"], gamma=o["gamma"], Ginv=o["Ginv"])

    g_a = capture(lambda: s.form_schur(nx, nu, N, B, G, C, g, c, S=f["S"], gamma=f["gamma"], Ginv=f["Ginv"]))
    g_b = capture(lambda: s.form_schur_reg(nx, nu, N, B, G, C, g, c, rho, S=r["S"], gamma=r["gamma"], Ginv=r["Ginv"]))
    g_c = capture(outside)
    s.reserve(G.element_size(), nx, N, B)
    g_d = s.graph_kkt_step(nx, nu, N, B, G, C, g, c, f["S"], f["gamma"], f["Ginv"], f["Pinv"], f["lam"], None, None, a.tol, a.max_iter,
                           f["it"], f["fl"], f["z"])
    g_e = s.graph_kkt_step_reg(nx, nu, N, B, G, C, g, c, rho, r["S"], r["gamma"], r["Ginv"], r["Pinv"], r["lam"], None, None, a.tol,
                               a.max_iter, r["it"], r["fl"], r["z"])
    g_o = s.graph_kkt_step(nx, nu, N, B, G2, C, g, c, o["S"], o["gamma"], o["Ginv"], o["Pinv"], o["lam"], None, None, a.tol, a.max_iter,
                           o["it"], o["fl"], o["z"])
    cand = {"a": g_a.replay, "b": g_b.replay, "c": g_c.replay}

    def step(gr, w):
        def go():
            w["lam"].zero_()
            gr.launch()
        return go

    cand["d"], cand["e"] = step(g_d, f), step(g_e, r)
    graphs = [g_d, g_e, g_o]
    if base is not None:
        p = bufs()
        base.reserve(G.element_size(), nx, N, B)
        g_p = base.graph_kkt_step(nx, nu, N, B, G, C, g, c, p["S"], p["gamma"], p["Ginv"], p["Pinv"], p["lam"], None, None, a.tol,
                                  a.max_iter, p["it"], p["fl"], p["z"])
        cand["d'"] = step(g_p, p)
        graphs.append(g_p)

    # the same answers first
    g_b.replay()
    g_c.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(r[k], o[k]) for k in ("S", "gamma", "Ginv"))
    cand["e"]()
    step(g_o, o)()
    torch.cuda.synchronize()
    print(f"  form_schur_reg vs form_schur on the copy G + rho I: bit-identical {same}; kkt_step_reg vs kkt_step on the copy: lambda "
          f"bit-identical {torch.equal(r['lam'], o['lam'])}, iterations mean {float(r['it'].float().mean()):.2f}, ran out {int(r['fl'].sum())}")

    for _ in range(2):
        for fn in cand.values():
            window(fn, a.warmup)
    t = {k: [] for k in cand}
    for _ in range(a.rounds):
        for k, fn in cand.items():
            t[k].append(window(fn, a.steps))
    names = {"a": "(a) form_schur", "b": "(b) form_schur_reg", "c": "(c) copy + diagonal add + form_schur", "d": "(d) kkt_step graph replay",
             "e": "(e) kkt_step_reg graph replay", "d'": "(d') kkt_step graph replay, baseline library"}
    for k in cand:
        print(f"  {names[k]:46s} {stat(t[k])}")
    med, prime = {k: statistics.median(v) for k, v in t.items()}, "d'"
    spread = max(max(t[k]) - min(t[k]) for k in ("a", "b"))
    es = np.dtype(dtype).itemsize
    print(f"  (b) - (a) = {1e3 * (med['b'] - med['a']):+.1f} us (larger spread of the two in this run: {1e3 * spread:.1f} us); "
          f"(c) - (b) = {1e3 * (med['c'] - med['b']):+.1f} us for 2 x {G.numel() * es / 1e6:.0f} MB of extra traffic; "
          f"(e) - (d) = {1e3 * (med['e'] - med['d']):+.1f} us" + (f"; (d) - (d') = {1e3 * (med['d'] - med[prime]):+.1f} us" if prime in med else ""))
    for gr in graphs:
        gr.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=25)
    ap.add_argument("--baseline-lib", default=None, help="another build of libgbdpcg.so whose kkt_step graph is timed in the same rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    base = solver_on(a.baseline_lib) if a.baseline_lib else None
    print(f"# reg_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}"
          f"{' --baseline-lib (the parent commit)' if base else ''}; {torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    ok = True
    for dtype in (np.float32, np.float64):
        nx, nu, N, B = 14, 7, 128, 1024
        print(f"{B} x (nx {nx}, nu {nu}, N {N}) {np.dtype(dtype).name}")
        ok = one_shape(s, base, nx, nu, N, B, dtype, a) and ok
    s.close()
    if base is not None:
        base.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
