#!/usr/bin/env python3
"""What the ADMM updates with stage-wise rows cost next to each other, next to the box update and next to the solve, in ONE process
on one device:
    python gbd-pcg_amd/tools/admm_rows_time.py [--warmup W] [--steps K] [--rounds R] > profiles/rNN_admm_rows.txt

At 1024 x (nx 14, nu 7, N 128) with mx = 2 linear rows on x and mu = 5 rows on u (1 linear + one q = 4 cone: the norm of three
inputs bounded by a fourth), random E, fp32 and fp64: the gbdpcg_admm_soc_update_* launch alone and the gbdpcg_admm_lin_update_*
launch alone on the same E and row counts, the gbdpcg_admm_lin_form_* launch alone and the gbdpcg_admm_update_* (box) launch alone
on buffers of its own (K launches between two device events each), then windows of K graph replays, kkt_resolve / admm_lin_step /
admm_soc_step alternating, R rounds; median and range over the rounds.  The factorisation is that of G + rho E'E (admm_lin_form,
kkt_step; rho = 2); the linear bounds hold every row within half of the largest row of the solution without them, the cone rows
have the offset 0 (admm_lin: the same bounds on all rows); every replay starts from lambda = 0 (the zero fill is inside every
window alike).  Algorithmic bytes, s = element size:
    lin update  (6 nw + 3 nz + ne) s + 3 s per problem     w, y, lo, hi in, w, y out; z, g in, gt out; E once; rho and two norms
                (a cone row reads no hi: one element less; the soc update is rated with the lin update's bytes)
    lin form    (2 ng + ne) s + s per problem              G in, Gt out; E once (its re-reads are the caches'); rho
    box update  9 nz s + 3 s per problem                   (tools/admm_time.py)
each over its time, against the HBM rates: 8 TB/s peak, about 6.3 TB/s achievable."""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/gbd-pcg_amd/", 1)[0])
from gbd_pcg_amd import binding  # noqa: E402
from oracle import schur_oracle as so  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12   # bytes / s


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


def rate(nbytes, ms):
    r = nbytes / (ms * 1e-3)
    return f"{nbytes / 1e6:.1f} MB -> {r / 1e12:.2f} TB/s, {100.0 * r / HBM_PEAK:.0f} % of peak, {100.0 * r / HBM_ACHIEVABLE:.0f} % of achievable"


def one_shape(s, nx, nu, N, B, mx, mu, cones, dtype, a):
    td = torch.float32 if dtype == np.float32 else torch.float64
    base = so.gen(nx, nu, N, seed=77, batch=8, dtype=dtype)
    arr = {k: np.tile(base[k], ((B + 7) // 8, 1))[:B] for k in "GCgc"}
    arr["g"] = arr["g"] * (1.0 + np.arange(B, dtype=dtype)[:, None] / B)
    G, C, g, c = (torch.from_numpy(np.ascontiguousarray(arr[k].reshape(-1))).cuda() for k in "GCgc")
    sv, sw = nx + nu, mx + mu
    nz, nw, ne, ng = sv * N - nu, sw * N - mu, (mx * nx + mu * nu) * N - mu * nu, (nx * nx + nu * nu) * N - nu * nu
    E = torch.from_numpy(np.tile((0.5 * np.random.default_rng(3).standard_normal(ne)).astype(dtype), B)).cuda()
    rho = torch.full((B,), 2.0, dtype=td, device="cuda")
    S = torch.empty(B * 3 * nx * nx * N, dtype=td, device="cuda")
    Pinv, Ginv, Gt = torch.empty_like(S), torch.empty_like(G), torch.empty_like(G)
    gamma = torch.empty(B * nx * N, dtype=td, device="cuda")
    lam, z = torch.zeros_like(gamma), torch.empty_like(g)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.uint8, device="cuda")
    s.admm_lin_form(nx, nu, mx, mu, N, B, G, E, rho, Gt=Gt)
    s.kkt_step(nx, nu, N, B, Gt, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=a.tol, max_iter=a.max_iter, iters=it, max_iter_exit=fl)
    torch.cuda.synchronize()
    Ed = torch.zeros(nw, nz, dtype=td, device="cuda")
    Eh = E[:ne]
    cone = torch.zeros(nw, dtype=torch.bool, device="cuda")
    lx, _, lu, _ = cones
    for k in range(N):
        eo, ro, co = k * (mx * nx + mu * nu), k * sw, k * sv
        Ed[ro:ro + mx, co:co + nx] = Eh[eo:eo + mx * nx].view(nx, mx).T
        cone[ro + lx:ro + mx] = True
        if k < N - 1:
            Ed[ro + mx:ro + sw, co + nx:co + sv] = Eh[eo + mx * nx:eo + mx * nx + mu * nu].view(nu, mu).T
            cone[ro + mx + lu:ro + sw] = True
    bound = 0.5 * (z.view(B, nz) @ Ed.T).abs().amax(dim=1, keepdim=True)
    lo, hi = (-bound).expand(B, nw).reshape(-1).contiguous(), bound.expand(B, nw).reshape(-1).contiguous()
    slo = lo.view(B, nw).clone()
    slo[:, cone] = 0.0
    slo = slo.reshape(-1).contiguous()
    st = {}
    for kind in ("lin", "soc"):
        st[kind] = dict(w=torch.zeros_like(lo), y=torch.zeros_like(lo), res=torch.empty(B, 2, dtype=td, device="cuda"))
    st["lin"]["gt"] = s.admm_lin_init(nx, nu, mx, mu, N, B, g, E, lo, hi, rho, st["lin"]["w"], st["lin"]["y"])
    st["soc"]["gt"] = s.admm_soc_init(nx, nu, mx, mu, cones, N, B, g, E, slo, hi, rho, st["soc"]["w"], st["soc"]["y"])
    L, Q = st["lin"], st["soc"]
    g_res = s.graph_kkt_resolve(nx, nu, N, B, Ginv, C, L["gt"], c, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter, it, fl, z)
    g_lin = s.graph_admm_lin_step(nx, nu, mx, mu, N, B, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol, a.max_iter,
                                  it, fl, z, L["w"], L["y"], L["gt"], L["res"])
    g_soc = s.graph_admm_soc_step(nx, nu, mx, mu, cones, N, B, Ginv, C, g, c, E, slo, hi, rho, S, Pinv, gamma, lam, None, None, a.tol,
                                  a.max_iter, it, fl, z, Q["w"], Q["y"], Q["gt"], Q["res"])
    # the soft twin of the linear rows on a state of its own: kappa = +Inf for the first half of the batch, 0.1 for the second
    kappa = torch.full((B, nw), float("inf"), dtype=td, device="cuda")
    kappa[B // 2:] = 0.1
    kappa = kappa.reshape(-1).contiguous()
    F = dict(w=torch.zeros_like(lo), y=torch.zeros_like(lo), res=torch.empty(B, 2, dtype=td, device="cuda"))
    F["gt"] = s.admm_lin_soft_init(nx, nu, mx, mu, N, B, g, E, lo, hi, kappa, rho, F["w"], F["y"])
    g_soft = s.graph_admm_lin_soft_step(nx, nu, mx, mu, N, B, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, None, None, a.tol,
                                        a.max_iter, it, fl, z, F["w"], F["y"], F["gt"], F["res"])
    # the box update of the same run, on buffers of its own in the layout of z
    blo, bhi = torch.full_like(g, -1.0), torch.full_like(g, 1.0)
    bw, by, bgt, bres = torch.zeros_like(g), torch.zeros_like(g), torch.empty_like(g), torch.empty(B, 2, dtype=td, device="cuda")

    def replay(gr):
        lam.zero_()
        gr.launch()

    calls = {"soc update": lambda: s.admm_soc_update(nx, nu, mx, mu, cones, N, B, g, E, slo, hi, rho, z, Q["w"], Q["y"], Q["gt"], res=Q["res"]),
             "lin update": lambda: s.admm_lin_update(nx, nu, mx, mu, N, B, g, E, lo, hi, rho, z, L["w"], L["y"], L["gt"], res=L["res"]),
             "lin form": lambda: s.admm_lin_form(nx, nu, mx, mu, N, B, G, E, rho, Gt=Gt),
             "box update": lambda: s.admm_update(nx, nu, N, B, g, blo, bhi, rho, z, bw, by, bgt, res=bres),
             "resolve replay": lambda: replay(g_res), "lin step replay": lambda: replay(g_lin), "soc step replay": lambda: replay(g_soc),
             "lin soft update": lambda: s.admm_lin_soft_update(nx, nu, mx, mu, N, B, g, E, lo, hi, kappa, rho, z, F["w"], F["y"], F["gt"],
                                                               res=F["res"]),
             "lin soft step replay": lambda: replay(g_soft)}
    for _ in range(30):      # a few iterations first: the loops do what they are for
        g_lin.launch()
        g_soc.launch()
        g_soft.launch()
    torch.cuda.synchronize()
    for kind, d in st.items():
        print(f"  {kind} after 30 iterations: max primal residual {float(d['res'][:, 0].max()):.2e}, max dual residual "
              f"{float(d['res'][:, 1].max()):.2e}, {int((d['y'] != 0).sum())} of {nw * B} rows active, ran out {int(fl.sum())}")
    for _ in range(2):
        for fn in calls.values():
            window(fn, a.warmup)
    t = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t[k].append(window(fn, a.steps))
    med = {k: statistics.median(v) for k, v in t.items()}
    es = np.dtype(dtype).itemsize
    must = {"soc update": ((6 * nw + 3 * nz + ne) * es + 3 * es) * B, "lin form": ((2 * ng + ne) * es + es) * B,
            "box update": (9 * nz * es + 3 * es) * B}
    must["lin update"] = must["soc update"]
    for k in ("soc update", "lin update", "lin form", "box update"):
        print(f"  {k + ' launch alone':30s} {stat(t[k])}; algorithmic bytes {rate(must[k], med[k])}")
    for k, name in (("resolve replay", "kkt_resolve"), ("lin step replay", "admm_lin_step"), ("soc step replay", "admm_soc_step")):
        print(f"  {name + ' graph replay':30s} {stat(t[k])}")
    print(f"  soc update / lin update: {med['soc update'] / med['lin update']:.2f} x ({1e3 * (med['soc update'] - med['lin update']):+.1f} us);  "
          f"soc step replay - resolve replay {1e3 * (med['soc step replay'] - med['resolve replay']):.1f} us, "
          f"lin step replay - resolve replay {1e3 * (med['lin step replay'] - med['resolve replay']):.1f} us")
    bl, bb = must["lin update"] / med["lin update"], must["box update"] / med["box update"]
    print(f"  lin update / box update: time {med['lin update'] / med['box update']:.2f} x, bytes {must['lin update'] / must['box update']:.2f} x, "
          f"bytes over time {bl / bb:.2f} x;  lin update alone / resolve replay {100.0 * med['lin update'] / med['resolve replay']:.1f} %")
    # the soft twin of the same run: one more read per row ((5 + 2) / (4 + 2) of the per-row traffic) and one division per row
    must["lin soft update"] = must["lin update"] + nw * es * B
    print(f"  {'lin soft update launch alone':30s} {stat(t['lin soft update'])}; algorithmic bytes {rate(must['lin soft update'], med['lin soft update'])}; "
          f"{med['lin soft update'] / med['lin update']:.3f} of the hard update launch (bytes {must['lin soft update'] / must['lin update']:.3f})")
    print(f"  {'admm_lin_soft_step graph replay':30s} {stat(t['lin soft step replay'])}; "
          f"{med['lin soft step replay'] / med['lin step replay']:.3f} of the hard step replay")
    for gr in (g_res, g_lin, g_soc, g_soft):
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
    print(f"# admm_rows_time.py --warmup {a.warmup} --steps {a.steps} --rounds {a.rounds} --tol {a.tol} --max-iter {a.max_iter}; "
          f"{torch.cuda.get_device_name(0)}; {s.lib.gbdpcg_version().decode()}")
    for dtype in (np.float32, np.float64):
        nx, nu, N, B, mx, mu, cones = 14, 7, 128, 1024, 2, 5, (2, 1, 1, 4)
        print(f"{B} x (nx {nx}, nu {nu}, N {N}), mx {mx} (linear), mu {mu} (1 linear + one q = 4 cone), {np.dtype(dtype).name}")
        one_shape(s, nx, nu, N, B, mx, mu, cones, dtype, a)
    s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
