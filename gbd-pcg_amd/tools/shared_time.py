#!/usr/bin/env python3
"""What a batch on ONE pair of matrices costs next to the same batch on `batch` copies of them, in ONE process on one device:
python gbd-pcg_amd/tools/shared_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_shared.txt

1024 x (nx 14, nu 7, N 128) fp32 to 1e-6: one plant is factored at batch 1 (gbdpcg_kkt_step_*), its S, Phi^-1, G^-1 and C are
copied `batch` times for the per-problem calls.  Windows of K graph replays between two device events, R rounds, median and
range over the rounds, in the symmetric modes 2 and 1:  kkt_resolve (replicated) / kkt_resolve_shared,  solve (replicated) /
solve_shared;  then the form_gamma and recover_primal launches alone, replicated / shared.  Every replicated timing is taken
TWICE per round (before and after the shared one): the spread between the two is the run's own noise, and the reference of a
shared number is the replicated call of this same run.  Every replay starts from lambda = 0 (the zero fill is inside every
window alike).  Before timing, the shared outputs are compared bit for bit with the replicated ones."""
import argparse
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
    return f"{statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def compare(name, rep_a, rep_b, shared):
    """One line per comparison: replicated (first timing), replicated (second timing), shared; is shared slower than the
    replicated median by more than the spread between the two replicated timings?"""
    ma, mb, ms = statistics.median(rep_a), statistics.median(rep_b), statistics.median(shared)
    ref, spread = 0.5 * (ma + mb), abs(ma - mb)
    print(f"  {name}")
    print(f"      replicated, first timing    {stat(rep_a)}")
    print(f"      replicated, second timing   {stat(rep_b)}")
    print(f"      shared                      {stat(shared)}")
    slower = ms > ref + spread
    print(f"      shared / replicated {ms / ref:.3f}; spread of the replicated timings {spread:.4f} ms; shared slower beyond it: {slower}")
    return not slower


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=25)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path"
    s = binding.Solver(0)
    nx, nu, N, B, dtype = 14, 7, 128, a.batch, np.float32
    print(f"# shared_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter} --batch {B}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    print(f"{B} x (nx {nx}, nu {nu}, N {N}) float32, one plant")
    d1 = so.gen(nx, nu, N, seed=77, batch=1, dtype=dtype)
    dv = so.gen(nx, nu, N, seed=78, batch=8, dtype=dtype)
    arr = {k: np.tile(dv[k], ((B + 7) // 8, 1))[:B] for k in "gc"}
    arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=dtype)[:, None] / B)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).cuda()   # noqa: E731
    G1, C1, g1, c1 = (dev(d1[k]) for k in "GCgc")
    g, c = dev(arr["g"]), dev(arr["c"])
    S1 = torch.empty(3 * nx * nx * N, dtype=torch.float32, device="cuda")
    P1, Gi1 = torch.empty_like(S1), torch.empty_like(G1)
    gam1 = torch.empty(nx * N, dtype=torch.float32, device="cuda")
    s.kkt_step(nx, nu, N, 1, G1, C1, g1, c1, S1, gam1, Gi1, P1, torch.zeros_like(gam1), torch.empty_like(g1), tol=a.tol, max_iter=a.max_iter)
    torch.cuda.synchronize()
    Sr, Pr, Gir, Cr = S1.repeat(B), P1.repeat(B), Gi1.repeat(B), C1.repeat(B)
    print(f"  matrices on the device: shared {(2 * S1.numel() + Gi1.numel() + C1.numel()) * 4 / 1e6:.2f} MB, "
          f"replicated {(2 * Sr.numel() + Gir.numel() + Cr.numel()) * 4 / 1e6:.1f} MB")
    gamma = torch.empty(B * nx * N, dtype=torch.float32, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    r, p = torch.empty_like(lam), torch.empty_like(lam)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")

    def replay(gr):
        lam.zero_()
        gr.launch()

    ok = True
    for mode in (2, 1):
        s.set_symmetric(mode)
        graphs = {
            "res_rep": s.graph_kkt_resolve(nx, nu, N, B, Gir, Cr, g, c, Sr, Pr, gamma, lam, r, p, a.tol, a.max_iter, it, fl, z),
            "res_sh": s.graph_kkt_resolve_shared(nx, nu, N, B, Gi1, C1, g, c, S1, P1, gamma, lam, r, p, a.tol, a.max_iter, it, fl, z),
            "sol_rep": s.graph_solve(nx, N, B, Sr, Pr, gamma, lam, r, p, a.tol, a.max_iter, it, fl),
            "sol_sh": s.graph_solve_shared(nx, N, B, S1, P1, gamma, lam, r, p, a.tol, a.max_iter, it, fl),
        }
        s.set_symmetric(2)
        # same bits first
        for rep, sh in (("res_rep", "res_sh"), ("sol_rep", "sol_sh")):
            replay(graphs[rep])
            torch.cuda.synchronize()
            want = [t.clone() for t in (gamma, lam, r, p, it, fl, z)]
            replay(graphs[sh])
            torch.cuda.synchronize()
            same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip((gamma, lam, r, p, it, fl, z), want))
            print(f"  mode {mode} {sh} vs {rep}: bit-identical {same}; iterations mean {float(it.float().mean()):.2f}, ran out {int(fl.sum())}")
            ok = ok and same
        for _ in range(2):
            for gr in graphs.values():
                window(lambda: replay(gr), a.warmup)
        t = {k: [] for k in ("res_rep_a", "res_sh", "res_rep_b", "sol_rep_a", "sol_sh", "sol_rep_b")}
        for _ in range(a.rounds):
            t["res_rep_a"].append(window(lambda: replay(graphs["res_rep"]), a.steps))
            t["res_sh"].append(window(lambda: replay(graphs["res_sh"]), a.steps))
            t["res_rep_b"].append(window(lambda: replay(graphs["res_rep"]), a.steps))
            t["sol_rep_a"].append(window(lambda: replay(graphs["sol_rep"]), a.steps))
            t["sol_sh"].append(window(lambda: replay(graphs["sol_sh"]), a.steps))
            t["sol_rep_b"].append(window(lambda: replay(graphs["sol_rep"]), a.steps))
        ok = compare(f"kkt_resolve graph replay, symmetric mode {mode}", t["res_rep_a"], t["res_rep_b"], t["res_sh"]) and ok
        ok = compare(f"solve graph replay, symmetric mode {mode}", t["sol_rep_a"], t["sol_rep_b"], t["sol_sh"]) and ok
        for gr in graphs.values():
            gr.close()

    launches = {
        "gam_rep": lambda: s.form_gamma(nx, nu, N, B, Gir, Cr, g, c, gamma=gamma),
        "gam_sh": lambda: s.form_gamma_shared(nx, nu, N, B, Gi1, C1, g, c, gamma=gamma),
        "rec_rep": lambda: s.recover_primal(nx, nu, N, B, Gir, Cr, g, lam, z=z),
        "rec_sh": lambda: s.recover_primal_shared(nx, nu, N, B, Gi1, C1, g, lam, z=z),
    }
    for _ in range(2):
        for fn in launches.values():
            window(fn, a.warmup)
    t = {k: [] for k in ("gam_rep_a", "gam_sh", "gam_rep_b", "rec_rep_a", "rec_sh", "rec_rep_b")}
    for _ in range(a.rounds):
        for key, fn in (("gam_rep_a", "gam_rep"), ("gam_sh", "gam_sh"), ("gam_rep_b", "gam_rep"), ("rec_rep_a", "rec_rep"),
                        ("rec_sh", "rec_sh"), ("rec_rep_b", "rec_rep")):
            t[key].append(window(launches[fn], a.steps))
    ok = compare("form_gamma launch alone", t["gam_rep_a"], t["gam_rep_b"], t["gam_sh"]) and ok
    ok = compare("recover_primal launch alone", t["rec_rep_a"], t["rec_rep_b"], t["rec_sh"]) and ok
    print(f"bit-identical and no shared line slower than its replicated line beyond the run's spread: {ok}")
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
