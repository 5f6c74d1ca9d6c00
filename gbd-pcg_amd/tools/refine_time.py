#!/usr/bin/env python3
"""What mixed-precision KKT refinement (gbdpcg_kkt_refine_step) costs next to the fp64 pipeline, in ONE process on one device:
    python gbd-pcg_amd/tools/refine_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_refine.txt

At 1024 x (14, 7, 128), fp64 data: windows of K launches between two device events, alternating, R rounds, median and range --
  * the defect launch next to the kkt_residual_f64 launch (the same reads; the defect writes and re-reads the fp32 vectors),
  * the apply launch,
  * the refine-step graph replay next to the kkt_resolve_f32 and kkt_resolve_f64 graph replays (each resolve from lambda = 0),
  * the refinement from z = lambda = 0 to the fp64 floor -- every problem with m_s <= (2 nx + 2) u mag_s, m_f <= (nx + nu + 2) u mag_f,
    the bounds of tests/test_gpu_kkt_refine.py -- in steps and in time, next to ONE fp64 kkt_step + kkt_residual_f64 at --tol64,
  * the _reg and the _shared defect launch and step replay next to the plain ones, in the same windows: the ratio reg / plain and
    shared / plain is what they report (rho_b = 0.3 on the same data; the shared batch is problem 0's plant under every state).
The magnitudes come from the device: kkt_residual_f64 of (|G|, -|C|, |g|, -|c|, |z|, |lambda|) is max(|G||z| + |g| + |C'||lambda|) and
max(|C||z| + |c|) row by row.  Small shapes of the GPU test follow with their step counts."""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

U64 = 2.0 ** -53


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


class Problem:
    def __init__(self, s, nx, nu, N, B, seed=77):
        self.s, self.dims = s, (nx, nu, N, B)
        base = so.gen(nx, nu, N, seed=seed, batch=min(B, 8), dtype=np.float64)
        arr = {k: np.tile(base[k], ((B + 7) // 8, 1))[:B] for k in "GCgc"}
        arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=np.float64)[:, None] / B)
        self.G, C, self.g, self.c = (torch.from_numpy(np.ascontiguousarray(arr[k].reshape(-1))).cuda() for k in "GCgc")
        self.C = None if N == 1 else C
        self.G32, self.g32, self.c32 = s.demote(self.G), s.demote(self.g), s.demote(self.c)
        self.C32 = None if N == 1 else s.demote(self.C)
        self.S32, _, self.Ginv32 = s.form_schur(nx, nu, N, B, self.G32, self.C32, self.g32, self.c32)
        self.Pinv32 = s.form_pinv(nx, N, B, self.S32, binding.PINV_STAIR)
        self.z = torch.zeros_like(self.g)
        self.lam = torch.zeros_like(self.c)
        self.work = s.refine_work(nx, nu, N, B)
        self.absd = (self.G.abs(), None if self.C is None else -self.C.abs(), self.g.abs(), -self.c.abs())

    def data(self):
        return self.G, self.C, self.g, self.c

    def kept(self):
        return self.Ginv32, self.C32, self.S32, self.Pinv32

    def over_floor(self, z, lam):
        """[B] : max(m_s / bound_s, m_f / bound_f) of the point, norms and magnitudes from the device."""
        nx, nu, N, B = self.dims
        norms = self.s.kkt_residual(nx, nu, N, B, *self.data(), z, lam)
        mag = self.s.kkt_residual(nx, nu, N, B, *self.absd, z.abs(), lam.abs())
        bound = mag * torch.tensor([(2 * nx + 2) * U64, (nx + nu + 2) * U64], dtype=torch.float64, device="cuda")
        return (norms / bound).max(dim=1).values


def steps_to_floor(p, a, limit=12):
    nx, nu, N, B = p.dims
    s = p.s
    p.z.zero_()
    p.lam.zero_()
    graph = s.graph_kkt_refine_step(nx, nu, N, B, *p.data(), *p.kept(), p.z, p.lam, tol=a.tol, max_iter=a.max_iter, **p.work)
    reached, lines = None, []
    for step in range(1, limit + 1):
        graph.launch()
        over = p.over_floor(p.z, p.lam)
        torch.cuda.synchronize()
        it = p.work["iters"].float()
        lines.append(f"    after step {step}: norm / bound max {float(over.max()):.3e} median {float(over.median()):.3e}; PCG iterations mean "
                     f"{float(it.mean()):.1f} max {int(it.max())}, ran out {int(p.work['max_iter_exit'].sum())}")
        if bool((over <= 1.0).all()):
            reached = step
            break
    return graph, reached, lines


def flagship(s, a):
    nx, nu, N, B = 14, 7, 128, 1024
    print(f"{B} x (nx {nx}, nu {nu}, N {N}), fp64 data; correction solve: tol {a.tol} on a right-hand side of max-norm in [1, 2), max_iter {a.max_iter}")
    p = Problem(s, nx, nu, N, B)
    w = p.work
    graph, reached, lines = steps_to_floor(p, a)
    print("\n".join(lines))
    print(f"  steps from z = lambda = 0 to the fp64 floor: {reached if reached else 'NOT within 12'}")
    K = reached or 12

    # the fp32 and fp64 resolves the step is measured against, and the fp64 step + residual the whole solve is measured against
    t64 = dict(dtype=torch.float64, device="cuda")
    S64 = torch.empty(B * 3 * nx * nx * N, **t64)
    Pinv64, Ginv64 = torch.empty_like(S64), torch.empty_like(p.G)
    gamma64 = torch.empty(B * nx * N, **t64)
    lam64, z64, r64, p64 = torch.zeros_like(gamma64), torch.empty_like(p.g), torch.empty_like(gamma64), torch.empty_like(gamma64)
    it64 = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl64 = torch.zeros(B, dtype=torch.uint8, device="cuda")
    res64 = torch.empty(B, 2, **t64)
    g_step64 = s.graph_kkt_step(nx, nu, N, B, *p.data(), S64, gamma64, Ginv64, Pinv64, lam64, r64, p64, a.tol64, a.max_iter64, it64, fl64, z64)
    lam64.zero_()
    g_step64.launch()
    over = p.over_floor(z64, lam64)
    torch.cuda.synchronize()
    print(f"  fp64 kkt_step (tol {a.tol64}, max_iter {a.max_iter64}) from lambda = 0: PCG iterations mean {float(it64.float().mean()):.1f} max "
          f"{int(it64.max())}, ran out {int(fl64.sum())}; norm / bound max {float(over.max()):.3e} median {float(over.median()):.3e}")
    g_res64 = s.graph_kkt_resolve(nx, nu, N, B, Ginv64, p.C, p.g, p.c, S64, Pinv64, gamma64, lam64, r64, p64, a.tol64, a.max_iter64, it64,
                                  fl64, z64)
    lam32, z32 = torch.zeros_like(w["gamma"]), torch.empty_like(p.g32)
    g_res32 = s.graph_kkt_resolve(nx, nu, N, B, p.Ginv32, p.C32, p.g32, p.c32, p.S32, p.Pinv32, w["gamma"], lam32, w["r"], w["p"], a.tol,
                                  a.max_iter, w["iters"], w["max_iter_exit"], z32)

    def solve_refined():
        p.z.zero_()
        p.lam.zero_()
        for _ in range(K):
            graph.launch()

    def solve64():
        lam64.zero_()
        g_step64.launch()
        s.kkt_residual(nx, nu, N, B, *p.data(), z64, lam64, res=res64)

    def resolve64():
        lam64.zero_()
        g_res64.launch()

    def resolve32():
        lam32.zero_()
        g_res32.launch()

    fns = {
        "defect": lambda: s.kkt_defect_mixed(nx, nu, N, B, *p.data(), p.z, p.lam, rg=w["rg"], rc=w["rc"], dlam=w["dlam"], expo=w["expo"],
                                             res=w["res"]),
        "residual64": lambda: s.kkt_residual(nx, nu, N, B, *p.data(), p.z, p.lam, res=res64),
        "apply": lambda: s.kkt_refine_apply(nx, nu, N, B, w["dz"], w["dlam"], w["expo"], p.z, p.lam),
        "step": graph.launch, "resolve32": resolve32, "resolve64": resolve64, "refined": solve_refined, "solve64": solve64,
    }
    extra = variants(s, a, p, K)
    fns.update({k: v[0] for k, v in extra.items() if v[0]})
    solve_refined()     # (the single launches are timed at a converged point: dz, dlam, expo are those of the last step)
    w["dz"].zero_()     # ... with a zero correction, so that K applications leave the point where it is
    w["dlam"].zero_()
    order = ("defect", "defect_reg", "defect_shared", "residual64", "apply", "resolve32", "resolve64", "solve64", "step", "step_reg",
             "step_shared", "refined")
    order = tuple(k for k in order if k in fns)
    for _ in range(2):
        for k in order:
            window(fns[k], max(1, a.warmup // (K if k == "refined" else 1)))
    t = {k: [] for k in order}
    for _ in range(a.rounds):
        for k in order:
            t[k].append(window(fns[k], max(1, a.steps // (K if k == "refined" else 1))))
    sz = so.sizes(nx, nu, N)
    rd = (sz["G"] + sz["C"] + 2 * sz["g"] + 2 * sz["c"]) * 8 * B
    vec = (sz["g"] + sz["c"]) * B
    md = statistics.median
    print(f"  kkt_defect_mixed launch        {stat(t['defect'])}; reads {rd / 1e6:.1f} MB, phase A writes {(vec + sz['c'] * B) * 4 / 1e6:.1f} MB, "
          f"phase B re-reads and writes {2 * vec * 4 / 1e6:.1f} MB")
    print(f"  kkt_residual_f64 launch        {stat(t['residual64'])}; defect / residual {md(t['defect']) / md(t['residual64']):.3f}")
    print(f"  kkt_refine_apply launch        {stat(t['apply'])}; moves {vec * (4 + 16) / 1e6:.1f} MB -> {vec * 20 / (md(t['apply']) * 1e-3) / 1e12:.2f} TB/s")
    print(f"  kkt_resolve_f32 graph replay   {stat(t['resolve32'])}")
    print(f"  kkt_resolve_f64 graph replay   {stat(t['resolve64'])}   (tol {a.tol64}, max_iter {a.max_iter64})")
    print(f"  kkt_refine_step graph replay   {stat(t['step'])}   (at the converged point; step / resolve_f32 {md(t['step']) / md(t['resolve32']):.3f}, "
          f"step / resolve_f64 {md(t['step']) / md(t['resolve64']):.3f})")
    print(f"  {K} refinement steps from zero   {stat(t['refined'])}   (kept fp32 factorisation; its formation is not in this figure)")
    print(f"  fp64 kkt_step + kkt_residual   {stat(t['solve64'])}   (forms S, Phi^-1 in fp64 every time)")
    print(f"  refined / fp64: {md(t['refined']) / md(t['solve64']):.3f}")
    for k, label, base in (("defect_reg", "kkt_defect_mixed_reg launch   ", "defect"), ("defect_shared", "kkt_defect_mixed_shared launch", "defect"),
                           ("step_reg", "refine_step_reg graph replay  ", "step"), ("step_shared", "refine_step_shared graph replay", "step")):
        if k in t:
            print(f"  {label} {stat(t[k])}   ({k.split('_')[1]} / plain {md(t[k]) / md(t[base]):.3f}; {extra[k][1]})")
        else:
            print(f"  {label} not timed: {extra[k][1]}")
    for g in [graph, g_step64, g_res64, g_res32] + [v[2] for v in extra.values() if v[2]]:
        g.close()
    return reached is not None


def variants(s, a, p, K):
    """The _reg and _shared rows: name -> (callable or None, note, graph or None).  Each step has its own point and work arrays and
    is replayed K times from zero first, so that it is timed at ITS converged point, as the plain step is."""
    nx, nu, N, B = p.dims
    out = {}
    rho = torch.full((B,), 0.3, dtype=torch.float64, device="cuda")
    wr = s.refine_work(nx, nu, N, B)
    out["defect_reg"] = (lambda: s.kkt_defect_mixed_reg(nx, nu, N, B, *p.data(), rho, p.z, p.lam, rg=wr["rg"], rc=wr["rc"], dlam=wr["dlam"],
                                                        expo=wr["expo"], res=wr["res"]), "rho_b = 0.3", None)
    G1, C1 = p.G[:p.G.numel() // B].clone(), None if p.C is None else p.C[:p.C.numel() // B].clone()
    ws = s.refine_work(nx, nu, N, B)
    out["defect_shared"] = (lambda: s.kkt_defect_mixed_shared(nx, nu, N, B, G1, C1, p.g, p.c, p.z, p.lam, rg=ws["rg"], rc=ws["rc"],
                                                              dlam=ws["dlam"], expo=ws["expo"], res=ws["res"]), "one G, C", None)

    def converged(make, note):
        z, lam = torch.zeros_like(p.g), torch.zeros_like(p.c)
        try:
            graph = make(z, lam)
        except Exception as e:   # (a shape the shared solve does not take: reported, not timed)
            return None, f"refused ({e})", None
        for _ in range(K):
            graph.launch()
        torch.cuda.synchronize()
        return graph.launch, note, graph

    S32, _, Ginv32 = s.form_schur_reg(nx, nu, N, B, p.G32, p.C32, p.g32, p.c32, s.demote(rho))
    Pinv32 = s.form_pinv(nx, N, B, S32, binding.PINV_STAIR)
    out["step_reg"] = converged(lambda z, lam: s.graph_kkt_refine_step_reg(nx, nu, N, B, *p.data(), rho, Ginv32, p.C32, S32, Pinv32, z, lam,
                                                                           tol=a.tol, max_iter=a.max_iter, **wr),
                                f"after {K} steps on the factorisation of fl32(G) + fl32(rho)")
    n1 = lambda t: None if t is None else t[:t.numel() // B].clone()   # noqa: E731
    S1, _, Gi1 = s.form_schur(nx, nu, N, 1, n1(p.G32), n1(p.C32), n1(p.g32), n1(p.c32))
    P1 = s.form_pinv(nx, N, 1, S1, binding.PINV_STAIR)
    out["step_shared"] = converged(lambda z, lam: s.graph_kkt_refine_step_shared(nx, nu, N, B, G1, C1, p.g, p.c, Gi1, n1(p.C32), S1, P1, z,
                                                                                 lam, tol=a.tol, max_iter=a.max_iter, **ws),
                                   f"after {K} steps; one G, C, Ginv32, C32, S32, Pinv32")
    return out


def small_shapes(s, a):
    print("steps to the fp64 floor at the shapes of tests/test_gpu_kkt_refine.py (same tol, max_iter)")
    ok = True
    for nx, nu, N, B in ((14, 7, 1, 2), (14, 7, 2, 1), (14, 7, 17, 3), (14, 7, 33, 2), (12, 4, 33, 2), (5, 2, 9, 2), (3, 3, 2, 1), (4, 6, 3, 2),
                         (1, 1, 4, 1)):
        p = Problem(s, nx, nu, N, B, seed=700 + nx + N)
        graph, reached, lines = steps_to_floor(p, a)
        graph.close()
        print(f"  {B} x ({nx}, {nu}, {N}): {reached if reached else 'NOT within 12'} steps;{lines[-1].split(':', 1)[1]}")
        ok = ok and reached is not None
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tol64", type=float, default=1e-24)
    ap.add_argument("--max-iter64", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    print(f"# refine_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter} --tol64 {a.tol64} "
          f"--max-iter64 {a.max_iter64}; {torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    ok = flagship(s, a)
    ok = small_shapes(s, a) and ok
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
