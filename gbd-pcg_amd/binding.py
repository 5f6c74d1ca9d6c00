"""ctypes view of libgbdpcg.so (the C ABI of include/gbdpcg.h) over torch device tensors.

Plumbing for tests and bench.py only: torch supplies device memory and streams, every
computation goes through the C ABI into the hand-written HIP kernels.  There is NO fallback:
a missing library raises at load(), and Solver() raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# GBDPCG_LIB: alternative build of the same library (A/B tuning runs on one device)
LIB_PATH = os.environ.get("GBDPCG_LIB") or os.path.join(CSRC, "libgbdpcg.so")

OK = 0
PATH_AUTO, PATH_FUSED, PATH_SPLIT, PATH_PERSISTENT, PATH_PERSISTENT_1R = 0, 1, 2, 3, 4
PINV_IDENTITY, PINV_BLOCK_JACOBI, PINV_STAIR = 0, 1, 2

# every symbol include/gbdpcg.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "gbdpcg_create", "gbdpcg_destroy", "gbdpcg_status_string", "gbdpcg_last_hip_error",
    "gbdpcg_last_hip_error_string", "gbdpcg_set_path", "gbdpcg_choose_path", "gbdpcg_cluster_members", "gbdpcg_set_symmetric",
    "gbdpcg_check_symmetric_f32", "gbdpcg_check_symmetric_f64",
    "gbdpcg_pcg_shared_mem_size", "gbdpcg_check_occupancy", "gbdpcg_workspace_bytes",
    "gbdpcg_reserve", "gbdpcg_spmv_f32", "gbdpcg_spmv_f64", "gbdpcg_solve_f32", "gbdpcg_solve_f64",
    "gbdpcg_solve_blocking_f32", "gbdpcg_solve_blocking_f64", "gbdpcg_solve_host_f32",
    "gbdpcg_solve_host_f64", "gbdpcg_graph_create_solve_f32", "gbdpcg_graph_create_solve_f64",
    "gbdpcg_graph_launch", "gbdpcg_graph_destroy", "gbdpcg_form_pinv_f32", "gbdpcg_form_pinv_f64",
    "gbdpcg_form_pinv_solve_f32", "gbdpcg_form_pinv_solve_f64",
    "gbdpcg_graph_create_form_pinv_solve_f32", "gbdpcg_graph_create_form_pinv_solve_f64",
    "gbdpcg_form_schur_f32", "gbdpcg_form_schur_f64", "gbdpcg_recover_primal_f32", "gbdpcg_recover_primal_f64",
    "gbdpcg_kkt_step_f32", "gbdpcg_kkt_step_f64", "gbdpcg_graph_create_kkt_step_f32", "gbdpcg_graph_create_kkt_step_f64",
    "gbdpcg_form_gamma_f32", "gbdpcg_form_gamma_f64", "gbdpcg_kkt_resolve_f32", "gbdpcg_kkt_resolve_f64",
    "gbdpcg_graph_create_kkt_resolve_f32", "gbdpcg_graph_create_kkt_resolve_f64",
    "gbdpcg_solve_shared_f32", "gbdpcg_solve_shared_f64", "gbdpcg_graph_create_solve_shared_f32", "gbdpcg_graph_create_solve_shared_f64",
    "gbdpcg_form_gamma_shared_f32", "gbdpcg_form_gamma_shared_f64", "gbdpcg_recover_primal_shared_f32", "gbdpcg_recover_primal_shared_f64",
    "gbdpcg_kkt_resolve_shared_f32", "gbdpcg_kkt_resolve_shared_f64",
    "gbdpcg_graph_create_kkt_resolve_shared_f32", "gbdpcg_graph_create_kkt_resolve_shared_f64",
    "gbdpcg_kkt_residual_f32", "gbdpcg_kkt_residual_f64", "gbdpcg_kkt_residual_shared_f32", "gbdpcg_kkt_residual_shared_f64",
    "gbdpcg_form_schur_reg_f32", "gbdpcg_form_schur_reg_f64", "gbdpcg_kkt_step_reg_f32", "gbdpcg_kkt_step_reg_f64",
    "gbdpcg_graph_create_kkt_step_reg_f32", "gbdpcg_graph_create_kkt_step_reg_f64",
    "gbdpcg_kkt_residual_reg_f32", "gbdpcg_kkt_residual_reg_f64",
    "gbdpcg_admm_init_f32", "gbdpcg_admm_init_f64", "gbdpcg_admm_update_f32", "gbdpcg_admm_update_f64",
    "gbdpcg_admm_step_f32", "gbdpcg_admm_step_f64", "gbdpcg_graph_create_admm_step_f32", "gbdpcg_graph_create_admm_step_f64",
    "gbdpcg_admm_step_shared_f32", "gbdpcg_admm_step_shared_f64",
    "gbdpcg_graph_create_admm_step_shared_f32", "gbdpcg_graph_create_admm_step_shared_f64",
    "gbdpcg_admm_lin_form_f32", "gbdpcg_admm_lin_form_f64", "gbdpcg_admm_lin_init_f32", "gbdpcg_admm_lin_init_f64",
    "gbdpcg_admm_lin_update_f32", "gbdpcg_admm_lin_update_f64", "gbdpcg_admm_lin_step_f32", "gbdpcg_admm_lin_step_f64",
    "gbdpcg_graph_create_admm_lin_step_f32", "gbdpcg_graph_create_admm_lin_step_f64",
    "gbdpcg_admm_lin_step_shared_f32", "gbdpcg_admm_lin_step_shared_f64",
    "gbdpcg_graph_create_admm_lin_step_shared_f32", "gbdpcg_graph_create_admm_lin_step_shared_f64",
    "gbdpcg_admm_soc_init_f32", "gbdpcg_admm_soc_init_f64", "gbdpcg_admm_soc_update_f32", "gbdpcg_admm_soc_update_f64",
    "gbdpcg_admm_soc_step_f32", "gbdpcg_admm_soc_step_f64",
    "gbdpcg_graph_create_admm_soc_step_f32", "gbdpcg_graph_create_admm_soc_step_f64",
    "gbdpcg_admm_soc_step_shared_f32", "gbdpcg_admm_soc_step_shared_f64",
    "gbdpcg_graph_create_admm_soc_step_shared_f32", "gbdpcg_graph_create_admm_soc_step_shared_f64",
    "gbdpcg_admm_rebalance_f32", "gbdpcg_admm_rebalance_f64", "gbdpcg_admm_lin_rebalance_f32", "gbdpcg_admm_lin_rebalance_f64",
    "gbdpcg_admm_soc_rebalance_f32", "gbdpcg_admm_soc_rebalance_f64",
    "gbdpcg_admm_restep_f32", "gbdpcg_admm_restep_f64", "gbdpcg_graph_create_admm_restep_f32", "gbdpcg_graph_create_admm_restep_f64",
    "gbdpcg_admm_lin_restep_f32", "gbdpcg_admm_lin_restep_f64",
    "gbdpcg_graph_create_admm_lin_restep_f32", "gbdpcg_graph_create_admm_lin_restep_f64",
    "gbdpcg_admm_soc_restep_f32", "gbdpcg_admm_soc_restep_f64",
    "gbdpcg_graph_create_admm_soc_restep_f32", "gbdpcg_graph_create_admm_soc_restep_f64",
    # soft (L1-penalised) bounds: the box and the linear rows with kappa behind hi
    *[f"gbdpcg_{pre}{fam}_{op}_{suf}" for fam in ("admm_soft", "admm_lin_soft")
      for pre, op in (("", "init"), ("", "update"), ("", "step"), ("graph_create_", "step"), ("", "step_shared"),
                      ("graph_create_", "step_shared"), ("", "restep"), ("graph_create_", "restep")) for suf in ("f32", "f64")],
    "gbdpcg_admm_lin_soft_rebalance_f32", "gbdpcg_admm_lin_soft_rebalance_f64",
    "gbdpcg_kkt_grad_f32", "gbdpcg_kkt_grad_f64", "gbdpcg_kkt_grad_shared_f32", "gbdpcg_kkt_grad_shared_f64",
    "gbdpcg_kkt_backward_f32", "gbdpcg_kkt_backward_f64", "gbdpcg_kkt_backward_shared_f32", "gbdpcg_kkt_backward_shared_f64",
    "gbdpcg_graph_create_kkt_backward_f32", "gbdpcg_graph_create_kkt_backward_f64",
    "gbdpcg_graph_create_kkt_backward_shared_f32", "gbdpcg_graph_create_kkt_backward_shared_f64",
    # the backward pass of the hard box QP: the forward y where lo, hi stand
    *[f"gbdpcg_{name}_{suf}" for name in ("admm_adjoint_init", "admm_adjoint_update", "admm_adjoint_step",
                                          "graph_create_admm_adjoint_step", "admm_grad_bounds") for suf in ("f32", "f64")],
    # the backward pass of the hard linear-row QP: the admm_lin family with yf where lo, hi stand, and the gradients in the rows
    *[f"gbdpcg_{name}_{suf}" for name in ("admm_lin_adjoint_init", "admm_lin_adjoint_update", "admm_lin_adjoint_step",
                                          "graph_create_admm_lin_adjoint_step", "admm_lin_grad") for suf in ("f32", "f64")],
    # the backward pass of the soft box and rows QPs: the mask in front of the hard adjoint calls, the gradients with kappa
    *[f"gbdpcg_{name}_{suf}" for name in ("admm_soft_mask", "admm_lin_soft_mask", "admm_soft_grad_bounds", "admm_lin_soft_grad")
      for suf in ("f32", "f64")],
    # the primal infeasibility certificate of the hard box and rows paths, from two iterates of the splitting
    *[f"gbdpcg_{name}_{suf}" for name in ("admm_infeas", "admm_infeas_shared", "admm_lin_infeas", "admm_lin_infeas_shared")
      for suf in ("f32", "f64")],
    # the optimality test of every ADMM family: stationarity with the row multiplier, dynamics, consensus, each with its scale
    *[f"gbdpcg_{name}_{suf}" for name in ("admm_optimality", "admm_optimality_shared", "admm_lin_optimality",
                                           "admm_lin_optimality_shared") for suf in ("f32", "f64")],
    "gbdpcg_demote_f32", "gbdpcg_kkt_defect_mixed", "gbdpcg_kkt_refine_apply", "gbdpcg_kkt_refine_step",
    "gbdpcg_graph_create_kkt_refine_step",
    "gbdpcg_kkt_defect_mixed_reg", "gbdpcg_kkt_defect_mixed_shared", "gbdpcg_kkt_refine_step_reg", "gbdpcg_kkt_refine_step_shared",
    "gbdpcg_graph_create_kkt_refine_step_reg", "gbdpcg_graph_create_kkt_refine_step_shared",
    "gbdpcg_csr_to_bt_f32", "gbdpcg_csr_to_bt_f64", "gbdpcg_version",
]


def _resolve_argtypes(lib):
    """argtypes of the frozen-linearisation entry points (gbdpcg_form_gamma_*, gbdpcg_kkt_resolve_* and its graph form)."""
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    for suf, ft in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        head = [vp, u32, u32, u32, u32, vp, vp, vp, vp]            # h, nx, nu, N, batch, Ginv, C, g, c
        solve = [vp, vp, vp, vp, vp, vp, ft, u32, vp, vp, vp]      # S, Pinv, gamma, lambda, r, p, tol, max_iter, iters, flags, z
        getattr(lib, f"gbdpcg_form_gamma_{suf}").argtypes = head + [vp, vp]
        getattr(lib, f"gbdpcg_kkt_resolve_{suf}").argtypes = head + solve + [vp]
        getattr(lib, f"gbdpcg_graph_create_kkt_resolve_{suf}").argtypes = head + solve + [ctypes.POINTER(vp)]
        # the shared-matrix twins: the same argument lists
        plain = [vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, ft, u32, vp, vp]   # h, n, N, batch, S, Pinv, gamma, lambda, r, p, tol, max_iter, iters, flags
        getattr(lib, f"gbdpcg_solve_shared_{suf}").argtypes = plain + [vp]
        getattr(lib, f"gbdpcg_graph_create_solve_shared_{suf}").argtypes = plain + [ctypes.POINTER(vp)]
        getattr(lib, f"gbdpcg_form_gamma_shared_{suf}").argtypes = head + [vp, vp]
        getattr(lib, f"gbdpcg_recover_primal_shared_{suf}").argtypes = head + [vp, vp]      # (lambda in the place of c, z, stream)
        getattr(lib, f"gbdpcg_kkt_resolve_shared_{suf}").argtypes = head + solve + [vp]
        getattr(lib, f"gbdpcg_graph_create_kkt_resolve_shared_{suf}").argtypes = head + solve + [ctypes.POINTER(vp)]
        # the residual norms: h, nx, nu, N, batch, G, C, g, c | z, lambda, res, stream
        getattr(lib, f"gbdpcg_kkt_residual_{suf}").argtypes = head + [vp, vp, vp, vp]
        getattr(lib, f"gbdpcg_kkt_residual_shared_{suf}").argtypes = head + [vp, vp, vp, vp]
        # per-problem regularisation: d_rho directly behind c
        step = [vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, ft, u32, vp, vp, vp]   # S, gamma, Ginv, Pinv, kind, lambda, r, p, tol, max_iter, iters, flags, z
        getattr(lib, f"gbdpcg_form_schur_reg_{suf}").argtypes = head + [vp] + [vp, vp, vp, vp]     # rho | S, gamma, Ginv, stream
        getattr(lib, f"gbdpcg_kkt_step_reg_{suf}").argtypes = head + [vp] + step + [vp]
        getattr(lib, f"gbdpcg_graph_create_kkt_step_reg_{suf}").argtypes = head + [vp] + step + [ctypes.POINTER(vp)]
        getattr(lib, f"gbdpcg_kkt_residual_reg_{suf}").argtypes = head + [vp] + [vp, vp, vp, vp]   # rho | z, lambda, res, stream
        # ADMM on a kept factorisation, three families: box (lo <= z <= hi), stage-wise linear rows (lo <= E z <= hi), second-order
        # cone rows next to them.  A family is the sizes it puts between nu and N and whether E stands in front of lo, hi:
        #   init    h, nx, nu, [sizes], N, batch | g | [E], lo, hi, rho | w, y, gt | stream
        #   update  ...                          | g | [E], lo, hi, rho | z, w, y, gt, res | stream
        #   step    ...             | Ginv, C, g, c | [E], lo, hi, rho | the solve's arguments | w, y, gt, res | stream / graph out
        # The soft twins (admm_soft, admm_lin_soft) put kappa directly behind hi, everywhere; the soft box has no rebalance of its
        # own (gbdpcg_admm_rebalance_* is it).
        sizes = [vp, u32, u32, u32, u32]
        for fam, extra, soft in (("admm", [], False), ("admm_lin", [u32, u32], False), ("admm_soc", [u32] * 6, False),   # mx, mu | lx, qx, lu, qu
                                 ("admm_soft", [], True), ("admm_lin_soft", [u32, u32], True)):
            fsizes = [vp, u32, u32] + extra + [u32, u32]
            fset = ([vp] if extra else []) + [vp, vp] + ([vp] if soft else []) + [vp]
            getattr(lib, f"gbdpcg_{fam}_init_{suf}").argtypes = fsizes + [vp] + fset + [vp, vp, vp] + [vp]
            getattr(lib, f"gbdpcg_{fam}_update_{suf}").argtypes = fsizes + [vp] + fset + [vp, vp, vp, vp, vp] + [vp]
            for name in (f"{fam}_step", f"{fam}_step_shared"):
                step_args = fsizes + [vp, vp, vp, vp] + fset + solve + [vp, vp, vp, vp]
                getattr(lib, f"gbdpcg_{name}_{suf}").argtypes = step_args + [vp]
                getattr(lib, f"gbdpcg_graph_create_{name}_{suf}").argtypes = step_args + [ctypes.POINTER(vp)]
            # adaptive rho.  The rule: ratio, shift, rho_min, rho_max, expo
            #   rebalance  ...                   | g | [E, lo, hi], res, rho | w, y, gt | rule | stream
            #   restep     ...   | G, [Gt], Ginv, C, g, c | [E], lo, hi, rho | S, Pinv, kind, the rest of the solve | w, y, gt, res | rule |
            rule = [ft, u32, ft, ft, vp]
            if extra or not soft:
                getattr(lib, f"gbdpcg_{fam}_rebalance_{suf}").argtypes = (fsizes + [vp] + (fset[:-1] if extra else []) + [vp, vp] +
                                                                         [vp, vp, vp] + rule + [vp])
            restep_args = (fsizes + [vp] + ([vp] if extra else []) + [vp, vp, vp, vp] + fset + [vp, vp, ctypes.c_int] + solve[2:] +
                           [vp, vp, vp, vp] + rule)
            getattr(lib, f"gbdpcg_{fam}_restep_{suf}").argtypes = restep_args + [vp]
            getattr(lib, f"gbdpcg_graph_create_{fam}_restep_{suf}").argtypes = restep_args + [ctypes.POINTER(vp)]
        getattr(lib, f"gbdpcg_admm_lin_form_{suf}").argtypes = sizes + [u32, u32] + [vp, vp, vp, vp, vp]   # (mx, mu) G, E, rho, Gt, stream
        # the backward pass: z, lambda, az, alambda | gG, gC, stream
        for name in ("kkt_grad", "kkt_grad_shared"):
            getattr(lib, f"gbdpcg_{name}_{suf}").argtypes = sizes + [vp, vp, vp, vp] + [vp, vp, vp]
        # Ginv, C, gz, nglam | S, Pinv, gamma | z, lambda, az, alambda | r, p, tol, max_iter, iters, flags | gG, gC | stream / graph out
        back = head + [vp, vp, vp] + [vp, vp, vp, vp] + [vp, vp, ft, u32, vp, vp] + [vp, vp]
        for name in ("kkt_backward", "kkt_backward_shared"):
            getattr(lib, f"gbdpcg_{name}_{suf}").argtypes = back + [vp]
            getattr(lib, f"gbdpcg_graph_create_{name}_{suf}").argtypes = back + [ctypes.POINTER(vp)]
        # the backward pass of the hard box QP: the box family with yf where lo, hi stand
        #   init    h, nx, nu, N, batch | gz | yf, rho | wa, ya, gta | stream
        #   update  ...                 | gz | yf, rho | az, wa, ya, gta, res | stream
        #   step    ...   | Ginv, C, gz, nglam | yf, rho | the solve's arguments (lambda := alambda, z := az) | wa, ya, gta, res |
        #   grad_bounds ...             | yf, rho, ya | glo, ghi | stream
        getattr(lib, f"gbdpcg_admm_adjoint_init_{suf}").argtypes = sizes + [vp] + [vp, vp] + [vp, vp, vp] + [vp]
        getattr(lib, f"gbdpcg_admm_adjoint_update_{suf}").argtypes = sizes + [vp] + [vp, vp] + [vp, vp, vp, vp, vp] + [vp]
        adj = sizes + [vp, vp, vp, vp] + [vp, vp] + solve + [vp, vp, vp, vp]
        getattr(lib, f"gbdpcg_admm_adjoint_step_{suf}").argtypes = adj + [vp]
        getattr(lib, f"gbdpcg_graph_create_admm_adjoint_step_{suf}").argtypes = adj + [ctypes.POINTER(vp)]
        getattr(lib, f"gbdpcg_admm_grad_bounds_{suf}").argtypes = sizes + [vp, vp, vp] + [vp, vp] + [vp]
        # the backward pass of the hard linear-row QP: the admm_lin family with yf where lo, hi stand
        #   init    h, nx, nu, mx, mu, N, batch | gz | E, yf, rho | wa, ya, gta | stream
        #   update  ...                         | gz | E, yf, rho | az, wa, ya, gta, res | stream
        #   step    ...   | Ginv, C, gz, nglam | E, yf, rho | the solve's arguments (lambda := alambda, z := az) | wa, ya, gta, res |
        #   grad    ...                         | z, az, yf, ya, rho | glo, ghi, gE | stream
        lsizes = [vp, u32, u32, u32, u32, u32, u32]
        getattr(lib, f"gbdpcg_admm_lin_adjoint_init_{suf}").argtypes = lsizes + [vp] + [vp, vp, vp] + [vp, vp, vp] + [vp]
        getattr(lib, f"gbdpcg_admm_lin_adjoint_update_{suf}").argtypes = lsizes + [vp] + [vp, vp, vp] + [vp, vp, vp, vp, vp] + [vp]
        ladj = lsizes + [vp, vp, vp, vp] + [vp, vp, vp] + solve + [vp, vp, vp, vp]
        getattr(lib, f"gbdpcg_admm_lin_adjoint_step_{suf}").argtypes = ladj + [vp]
        getattr(lib, f"gbdpcg_graph_create_admm_lin_adjoint_step_{suf}").argtypes = ladj + [ctypes.POINTER(vp)]
        getattr(lib, f"gbdpcg_admm_lin_grad_{suf}").argtypes = lsizes + [vp, vp, vp, vp, vp] + [vp, vp, vp] + [vp]
        # the backward pass of the soft QPs
        #   mask         h, nx, nu, [mx, mu], N, batch | yf, kappa, rho | ym | stream
        #   grad_bounds  h, nx, nu, N, batch           | yf, kappa, rho, ya, az | glo, ghi, gkappa | stream
        #   lin grad     h, nx, nu, mx, mu, N, batch   | z, az, E, yf, ya, kappa, rho | glo, ghi, gkappa, gE | stream
        getattr(lib, f"gbdpcg_admm_soft_mask_{suf}").argtypes = sizes + [vp, vp, vp] + [vp] + [vp]
        getattr(lib, f"gbdpcg_admm_lin_soft_mask_{suf}").argtypes = lsizes + [vp, vp, vp] + [vp] + [vp]
        getattr(lib, f"gbdpcg_admm_soft_grad_bounds_{suf}").argtypes = sizes + [vp, vp, vp, vp, vp] + [vp, vp, vp] + [vp]
        getattr(lib, f"gbdpcg_admm_lin_soft_grad_{suf}").argtypes = lsizes + [vp] * 7 + [vp] * 4 + [vp]
        # the infeasibility certificate
        #   h, nx, nu, [mx, mu], N, batch | C, c, [E], lo, hi, rho | lambda0, lambda1, y0, y1 | eps | cert, flag | stream
        for name in ("infeas", "infeas_shared"):
            getattr(lib, f"gbdpcg_admm_{name}_{suf}").argtypes = sizes + [vp] * 5 + [vp] * 4 + [ft] + [vp, vp] + [vp]
            getattr(lib, f"gbdpcg_admm_lin_{name}_{suf}").argtypes = lsizes + [vp] * 6 + [vp] * 4 + [ft] + [vp, vp] + [vp]
        # the optimality test
        #   h, nx, nu, [mx, mu], N, batch | G, C, g, c, [E], rho | z, lambda, w, y | eps_abs, eps_rel | opt, done | stream
        for name in ("optimality", "optimality_shared"):
            getattr(lib, f"gbdpcg_admm_{name}_{suf}").argtypes = sizes + [vp] * 5 + [vp] * 4 + [ft, ft] + [vp, vp] + [vp]
            getattr(lib, f"gbdpcg_admm_lin_{name}_{suf}").argtypes = lsizes + [vp] * 6 + [vp] * 4 + [ft, ft] + [vp, vp] + [vp]

    # mixed-precision refinement (no suffix: fp64 data and point, fp32 solve)
    head = [vp, u32, u32, u32, u32, vp, vp, vp, vp]                # h, nx, nu, N, batch, G, C, g, c (fp64)
    lib.gbdpcg_demote_f32.argtypes = [vp, ctypes.c_uint64, vp, vp, vp]                    # h, count, src, dst, stream
    # the defect: head | z, lambda | rg, rc, dlambda, expo, res | stream
    lib.gbdpcg_kkt_refine_apply.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]   # dz, dlambda, expo | z, lambda | stream
    # Ginv32, C32, S32, Pinv32 | rg, rc, gamma, dlambda, r, p, dz | tol, max_iter, iters, flags | expo, z, lambda, res
    tail = [vp] * 4 + [vp] * 7 + [ctypes.c_float, u32, vp, vp] + [vp] * 4
    # the _shared forms: the same argument lists; the _reg forms: rho (fp64, [batch]) directly behind c
    for name, hd in (("", head), ("_shared", head), ("_reg", head + [vp])):
        getattr(lib, f"gbdpcg_kkt_defect_mixed{name}").argtypes = hd + [vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(lib, f"gbdpcg_kkt_refine_step{name}").argtypes = hd + tail + [vp]
        getattr(lib, f"gbdpcg_graph_create_kkt_refine_step{name}").argtypes = hd + tail + [ctypes.POINTER(vp)]


_lib = None


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of csrc/ (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j8"] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `make -C gbd-pcg_amd/csrc` "
                               "(there is no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        lib.gbdpcg_status_string.restype = ctypes.c_char_p
        lib.gbdpcg_last_hip_error_string.restype = ctypes.c_char_p
        lib.gbdpcg_version.restype = ctypes.c_char_p
        lib.gbdpcg_pcg_shared_mem_size.restype = ctypes.c_size_t
        lib.gbdpcg_workspace_bytes.restype = ctypes.c_size_t
        _resolve_argtypes(lib)
        _lib = lib
    return _lib


class GbdPcgError(RuntimeError):
    pass


def _suffix(t):
    import torch
    if t.dtype == torch.float32:
        return "f32", ctypes.c_float
    if t.dtype == torch.float64:
        return "f64", ctypes.c_double
    raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Solver:
    """One gbdpcg handle on one device."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.h = ctypes.c_void_p()
        st = self.lib.gbdpcg_create(ctypes.byref(self.h), ctypes.c_int(device))
        if st != OK:
            raise GbdPcgError(f"gbdpcg_create: {self.lib.gbdpcg_status_string(st).decode()}")
        self.device = device

    def close(self):
        if self.h:
            self.lib.gbdpcg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, what):
        if st != OK:
            msg = self.lib.gbdpcg_status_string(st).decode()
            hip = self.lib.gbdpcg_last_hip_error_string(self.h).decode()
            raise GbdPcgError(f"{what}: {msg} (status {st}; last HIP error: {hip})")

    @staticmethod
    def _stream(stream):
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        return ctypes.c_void_p(s.cuda_stream)

    def set_path(self, path: int):
        self._check(self.lib.gbdpcg_set_path(self.h, ctypes.c_int(path)), "set_path")

    def set_symmetric(self, mode):
        """0 / False: never, 1 / True: assume, 2: test on the device before every solve (the default)."""
        self._check(self.lib.gbdpcg_set_symmetric(self.h, ctypes.c_int(int(mode))), "set_symmetric")

    def check_symmetric(self, n, N, batch, M, stream=None, flags=None):
        """uint8 tensor [batch]: 1 where L_{k+1} == R_k^T bit for bit for every knot."""
        import torch
        suf, _ = _suffix(M)
        if flags is None:
            flags = torch.empty(batch, dtype=torch.uint8, device=M.device)
        assert flags.dtype == torch.uint8 and flags.numel() == batch and flags.is_contiguous()
        fn = getattr(self.lib, f"gbdpcg_check_symmetric_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(n), ctypes.c_uint32(N), ctypes.c_uint32(batch), _p(M), _p(flags),
                       self._stream(stream)), "check_symmetric")
        return flags

    def choose_path(self, elem_size, n, N, batch) -> int:
        return self.lib.gbdpcg_choose_path(self.h, ctypes.c_uint32(elem_size), ctypes.c_uint32(n),
                                           ctypes.c_uint32(N), ctypes.c_uint32(batch))

    def cluster_members(self, elem_size, n, N) -> int:
        return self.lib.gbdpcg_cluster_members(ctypes.c_uint32(elem_size), ctypes.c_uint32(n), ctypes.c_uint32(N))

    def reserve(self, elem_size, n, N, batch):
        self._check(self.lib.gbdpcg_reserve(self.h, ctypes.c_uint32(elem_size), ctypes.c_uint32(n),
                                            ctypes.c_uint32(N), ctypes.c_uint32(batch)), "reserve")

    def spmv(self, n, N, batch, M, x, y=None, stream=None):
        import torch
        suf, _ = _suffix(M)
        assert M.is_cuda and M.is_contiguous() and x.is_contiguous()
        assert M.numel() == batch * 3 * n * n * N and x.numel() == batch * n * N
        if y is None:
            y = torch.empty_like(x)
        fn = getattr(self.lib, f"gbdpcg_spmv_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(n), ctypes.c_uint32(N), ctypes.c_uint32(batch),
                       _p(M), _p(x), _p(y), self._stream(stream)), "spmv")
        return y

    def solve_args(self, n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, mie):
        suf, cty = _suffix(S)
        for t, cnt in ((S, 3 * n * n * N), (Pinv, 3 * n * n * N), (gamma, n * N), (lam, n * N),
                       (r, n * N), (p, n * N)):
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.numel() == batch * cnt and t.dtype == S.dtype
        assert iters.numel() == batch and mie is None or mie.numel() == batch
        return suf, (self.h, ctypes.c_uint32(n), ctypes.c_uint32(N), ctypes.c_uint32(batch), _p(S),
                     _p(Pinv), _p(gamma), _p(lam), _p(r), _p(p), cty(tol), ctypes.c_uint32(max_iter),
                     _p(iters), _p(mie))

    def solve(self, n, N, batch, S, Pinv, gamma, lam, r=None, p=None, tol=1e-6, max_iter=25,
              iters=None, max_iter_exit=None, stream=None):
        """Asynchronous batched solve (gbdpcg_solve_*).  lam is in/out.  Returns (iters, flags)."""
        import torch
        if iters is None:
            iters = torch.empty(batch, dtype=torch.int32, device=S.device)
        if max_iter_exit is None:
            max_iter_exit = torch.empty(batch, dtype=torch.uint8, device=S.device)
        suf, args = self.solve_args(n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                                    max_iter_exit)
        fn = getattr(self.lib, f"gbdpcg_solve_{suf}")
        self._check(fn(*args, self._stream(stream)), "solve")
        return iters, max_iter_exit

    def solve_blocking(self, n, N, S, Pinv, gamma, lam, r=None, p=None, tol=1e-6, max_iter=25):
        """gbdpcg_solve_blocking_* : the reference's device-pointer overload. Returns (iters, flag)."""
        suf, cty = _suffix(S)
        it = ctypes.c_uint32(0)
        fl = ctypes.c_uint8(0)
        fn = getattr(self.lib, f"gbdpcg_solve_blocking_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(n), ctypes.c_uint32(N), _p(S), _p(Pinv), _p(gamma),
                       _p(lam), _p(r), _p(p), cty(tol), ctypes.c_uint32(max_iter), ctypes.byref(it),
                       ctypes.byref(fl)), "solve_blocking")
        return int(it.value), bool(fl.value)

    def solve_host(self, n, N, S, Pinv, gamma, lam, tol=1e-6, max_iter=25):
        """gbdpcg_solve_host_* on numpy arrays (lam in/out). Returns (iters, flag)."""
        import numpy as np
        suf, cty = {np.dtype(np.float32): ("f32", ctypes.c_float),
                    np.dtype(np.float64): ("f64", ctypes.c_double)}[S.dtype]
        it = ctypes.c_uint32(0)
        fl = ctypes.c_uint8(0)

        def hp(a):
            return None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        fn = getattr(self.lib, f"gbdpcg_solve_host_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(n), ctypes.c_uint32(N), hp(S), hp(Pinv), hp(gamma),
                       hp(lam), cty(tol), ctypes.c_uint32(max_iter), ctypes.byref(it),
                       ctypes.byref(fl)), "solve_host")
        return int(it.value), bool(fl.value)

    def graph_solve(self, n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit):
        """Capture a solve into a hipGraph; returns a Graph whose launch() replays it."""
        suf, args = self.solve_args(n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                                    max_iter_exit)
        g = ctypes.c_void_p()
        fn = getattr(self.lib, f"gbdpcg_graph_create_solve_{suf}")
        self._check(fn(*args, ctypes.byref(g)), "graph_create_solve")
        return Graph(self, g, keep=(S, Pinv, gamma, lam, r, p, iters, max_iter_exit))

    def _form_solve_args(self, n, N, batch, S, Pinv, kind, gamma, lam, r, p, tol, max_iter, iters, mie):
        suf, a = self.solve_args(n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, mie)
        # (h, n, N, batch, S, Pinv, | kind, | gamma, lam, r, p, tol, max_iter, iters, mie)
        return suf, a[:6] + (ctypes.c_int(kind),) + a[6:]

    def form_pinv_solve(self, n, N, batch, S, Pinv, gamma, lam, kind=PINV_STAIR, r=None, p=None, tol=1e-6,
                        max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_form_pinv_solve_*: Pinv (output) formed from S, then the solve, one call.  Returns (iters, flags)."""
        import torch
        if iters is None:
            iters = torch.empty(batch, dtype=torch.int32, device=S.device)
        if max_iter_exit is None:
            max_iter_exit = torch.empty(batch, dtype=torch.uint8, device=S.device)
        suf, args = self._form_solve_args(n, N, batch, S, Pinv, kind, gamma, lam, r, p, tol, max_iter, iters,
                                          max_iter_exit)
        fn = getattr(self.lib, f"gbdpcg_form_pinv_solve_{suf}")
        self._check(fn(*args, self._stream(stream)), "form_pinv_solve")
        return iters, max_iter_exit

    def graph_form_pinv_solve(self, n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit,
                              kind=PINV_STAIR):
        """Capture Pinv formation + solve into one hipGraph (gbdpcg_graph_create_form_pinv_solve_*)."""
        suf, args = self._form_solve_args(n, N, batch, S, Pinv, kind, gamma, lam, r, p, tol, max_iter, iters,
                                          max_iter_exit)
        g = ctypes.c_void_p()
        fn = getattr(self.lib, f"gbdpcg_graph_create_form_pinv_solve_{suf}")
        self._check(fn(*args, ctypes.byref(g)), "graph_create_form_pinv_solve")
        return Graph(self, g, keep=(S, Pinv, gamma, lam, r, p, iters, max_iter_exit))

    def form_pinv(self, n, N, batch, S, kind=PINV_STAIR, Pinv=None, stream=None):
        import torch
        suf, _ = _suffix(S)
        if Pinv is None:
            Pinv = torch.empty_like(S)
        fn = getattr(self.lib, f"gbdpcg_form_pinv_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(n), ctypes.c_uint32(N), ctypes.c_uint32(batch), _p(S),
                       _p(Pinv), ctypes.c_int(kind), self._stream(stream)), "form_pinv")
        return Pinv

    def form_schur(self, nx, nu, N, batch, G, C, g, c, S=None, gamma=None, Ginv=None, want_ginv=True, stream=None):
        """gbdpcg_form_schur_*: packed KKT blocks (layouts in include/gbdpcg.h) -> S, gamma and (optionally) G^-1."""
        import torch
        suf, _ = _suffix(G)
        if S is None:
            S = torch.empty(batch * 3 * nx * nx * N, dtype=G.dtype, device=G.device)
        if gamma is None:
            gamma = torch.empty(batch * nx * N, dtype=G.dtype, device=G.device)
        if Ginv is None and want_ginv:
            Ginv = torch.empty_like(G)
        fn = getattr(self.lib, f"gbdpcg_form_schur_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(nx), ctypes.c_uint32(nu), ctypes.c_uint32(N), ctypes.c_uint32(batch), _p(G),
                       _p(C), _p(g), _p(c), _p(S), _p(gamma), _p(Ginv), self._stream(stream)), "form_schur")
        return S, gamma, Ginv

    def recover_primal(self, nx, nu, N, batch, Ginv, C, g, lam, z=None, stream=None):
        """gbdpcg_recover_primal_*: z = -G^-1 (g + C' lambda), the layout of g."""
        import torch
        suf, _ = _suffix(Ginv)
        if z is None:
            z = torch.empty_like(g)
        fn = getattr(self.lib, f"gbdpcg_recover_primal_{suf}")
        self._check(fn(self.h, ctypes.c_uint32(nx), ctypes.c_uint32(nu), ctypes.c_uint32(N), ctypes.c_uint32(batch), _p(Ginv),
                       _p(C), _p(g), _p(lam), _p(z), self._stream(stream)), "recover_primal")
        return z

    def form_gamma(self, nx, nu, N, batch, Ginv, C, g, c, gamma=None, stream=None):
        """gbdpcg_form_gamma_*: gamma = -(c + C G^-1 g) from the G^-1 form_schur wrote -- G, C unchanged, new g and c."""
        import torch
        suf, _ = _suffix(Ginv)
        if gamma is None:
            gamma = torch.empty(batch * nx * N, dtype=Ginv.dtype, device=Ginv.device)
        fn = getattr(self.lib, f"gbdpcg_form_gamma_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(Ginv), _p(C), _p(g), _p(c), _p(gamma), self._stream(stream)), "form_gamma")
        return gamma

    def _resolve_args(self, nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, mie, z):
        suf, _ = _suffix(Ginv)
        return suf, (self.h, nx, nu, N, batch, _p(Ginv), _p(C), _p(g), _p(c), _p(S), _p(Pinv), _p(gamma), _p(lam), _p(r), _p(p),
                     tol, max_iter, _p(iters), _p(mie), _p(z))

    def kkt_resolve(self, nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, z, r=None, p=None, tol=1e-6, max_iter=25,
                    iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_kkt_resolve_*: new g, c on unchanged S, Pinv, G^-1 -> gamma -> PCG (warm start from lam) -> primal step z."""
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=Ginv.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=Ginv.device)
        suf, args = self._resolve_args(nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                                       max_iter_exit, z)
        fn = getattr(self.lib, f"gbdpcg_kkt_resolve_{suf}")
        self._check(fn(*args, self._stream(stream)), "kkt_resolve")
        return iters, max_iter_exit

    def graph_kkt_resolve(self, nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit, z):
        """Capture gamma + solve + recovery into one hipGraph (gbdpcg_graph_create_kkt_resolve_*)."""
        suf, args = self._resolve_args(nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                                       max_iter_exit, z)
        gr = ctypes.c_void_p()
        fn = getattr(self.lib, f"gbdpcg_graph_create_kkt_resolve_{suf}")
        self._check(fn(*args, ctypes.byref(gr)), "graph_create_kkt_resolve")
        return Graph(self, gr, keep=(Ginv, C, g, c, S, Pinv, gamma, lam, r, p, iters, max_iter_exit, z))

    # ---- shared-matrix batches: ONE S, Pinv, Ginv, C (one problem's worth each) for `batch` sets of vectors (include/gbdpcg.h)
    def _solve_shared_args(self, n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, mie):
        for t, cnt in ((S, 3 * n * n * N), (Pinv, 3 * n * n * N), (gamma, batch * n * N), (lam, batch * n * N), (r, batch * n * N),
                       (p, batch * n * N)):
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.numel() == cnt and t.dtype == S.dtype
        suf, _ = _suffix(S)
        return suf, (self.h, n, N, batch, _p(S), _p(Pinv), _p(gamma), _p(lam), _p(r), _p(p), tol, max_iter, _p(iters), _p(mie))

    def solve_shared(self, n, N, batch, S, Pinv, gamma, lam, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None,
                     stream=None):
        """gbdpcg_solve_shared_*: one S and Pinv (3 n^2 N elements each) for `batch` gamma / lambda.  Returns (iters, flags)."""
        import torch
        if iters is None:
            iters = torch.empty(batch, dtype=torch.int32, device=S.device)
        if max_iter_exit is None:
            max_iter_exit = torch.empty(batch, dtype=torch.uint8, device=S.device)
        suf, args = self._solve_shared_args(n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit)
        self._check(getattr(self.lib, f"gbdpcg_solve_shared_{suf}")(*args, self._stream(stream)), "solve_shared")
        return iters, max_iter_exit

    def graph_solve_shared(self, n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit):
        """Capture a shared-matrix solve into a hipGraph (gbdpcg_graph_create_solve_shared_*)."""
        suf, args = self._solve_shared_args(n, N, batch, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit)
        g = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_solve_shared_{suf}")(*args, ctypes.byref(g)), "graph_create_solve_shared")
        return Graph(self, g, keep=(S, Pinv, gamma, lam, r, p, iters, max_iter_exit))

    def form_gamma_shared(self, nx, nu, N, batch, Ginv, C, g, c, gamma=None, stream=None):
        """gbdpcg_form_gamma_shared_*: one problem's Ginv and C, `batch` g and c."""
        import torch
        suf, _ = _suffix(Ginv)
        if gamma is None:
            gamma = torch.empty(batch * nx * N, dtype=Ginv.dtype, device=Ginv.device)
        fn = getattr(self.lib, f"gbdpcg_form_gamma_shared_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(Ginv), _p(C), _p(g), _p(c), _p(gamma), self._stream(stream)), "form_gamma_shared")
        return gamma

    def recover_primal_shared(self, nx, nu, N, batch, Ginv, C, g, lam, z=None, stream=None):
        """gbdpcg_recover_primal_shared_*: one problem's Ginv and C, `batch` g and lambda."""
        import torch
        suf, _ = _suffix(Ginv)
        if z is None:
            z = torch.empty_like(g)
        fn = getattr(self.lib, f"gbdpcg_recover_primal_shared_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(Ginv), _p(C), _p(g), _p(lam), _p(z), self._stream(stream)), "recover_primal_shared")
        return z

    def kkt_resolve_shared(self, nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, z, r=None, p=None, tol=1e-6, max_iter=25,
                           iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_kkt_resolve_shared_*: gamma -> PCG -> primal step on ONE Ginv, C, S, Pinv for `batch` g, c, lambda."""
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=Ginv.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=Ginv.device)
        suf, args = self._resolve_args(nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                                       max_iter_exit, z)
        self._check(getattr(self.lib, f"gbdpcg_kkt_resolve_shared_{suf}")(*args, self._stream(stream)), "kkt_resolve_shared")
        return iters, max_iter_exit

    def graph_kkt_resolve_shared(self, nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, max_iter_exit,
                                 z):
        """Capture the shared-matrix resolve into one hipGraph (gbdpcg_graph_create_kkt_resolve_shared_*)."""
        suf, args = self._resolve_args(nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                                       max_iter_exit, z)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_kkt_resolve_shared_{suf}")(*args, ctypes.byref(gr)),
                    "graph_create_kkt_resolve_shared")
        return Graph(self, gr, keep=(Ginv, C, g, c, S, Pinv, gamma, lam, r, p, iters, max_iter_exit, z))

    def _kkt_residual(self, name, nx, nu, N, batch, G, C, g, c, z, lam, res, stream):
        import torch
        suf, _ = _suffix(G)
        if res is None:
            res = torch.empty(batch, 2, dtype=G.dtype, device=G.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == G.dtype
        fn = getattr(self.lib, f"gbdpcg_{name}_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(G), _p(C), _p(g), _p(c), _p(z), _p(lam), _p(res), self._stream(stream)), name)
        return res.view(batch, 2)

    def kkt_residual(self, nx, nu, N, batch, G, C, g, c, z, lam, res=None, stream=None):
        """gbdpcg_kkt_residual_*: [batch, 2] tensor of (||G z + g + C' lambda||_inf, ||C z - c||_inf) per problem.  G holds the
        Hessians (not G^-1); z has the layout of g."""
        return self._kkt_residual("kkt_residual", nx, nu, N, batch, G, C, g, c, z, lam, res, stream)

    def kkt_residual_shared(self, nx, nu, N, batch, G, C, g, c, z, lam, res=None, stream=None):
        """gbdpcg_kkt_residual_shared_*: one problem's G and C, `batch` g, c, z and lambda."""
        return self._kkt_residual("kkt_residual_shared", nx, nu, N, batch, G, C, g, c, z, lam, res, stream)

    def _kkt_args(self, nx, nu, N, batch, G, C, g, c, S, gamma, Ginv, Pinv, kind, lam, r, p, tol, max_iter, iters, mie, z):
        suf, ft = _suffix(G)
        return suf, (self.h, ctypes.c_uint32(nx), ctypes.c_uint32(nu), ctypes.c_uint32(N), ctypes.c_uint32(batch), _p(G), _p(C),
                     _p(g), _p(c), _p(S), _p(gamma), _p(Ginv), _p(Pinv), ctypes.c_int(kind), _p(lam), _p(r), _p(p), ft(tol),
                     ctypes.c_uint32(max_iter), _p(iters), _p(mie), _p(z))

    def kkt_step(self, nx, nu, N, batch, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, kind=PINV_STAIR, r=None, p=None, tol=1e-6,
                 max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_kkt_step_*: KKT blocks -> S, gamma, G^-1 -> Pinv -> PCG (warm start from lam) -> primal step z, one call."""
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=G.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=G.device)
        suf, args = self._kkt_args(nx, nu, N, batch, G, C, g, c, S, gamma, Ginv, Pinv, kind, lam, r, p, tol, max_iter, iters,
                                   max_iter_exit, z)
        fn = getattr(self.lib, f"gbdpcg_kkt_step_{suf}")
        self._check(fn(*args, self._stream(stream)), "kkt_step")
        return iters, max_iter_exit

    def graph_kkt_step(self, nx, nu, N, batch, G, C, g, c, S, gamma, Ginv, Pinv, lam, r, p, tol, max_iter, iters, max_iter_exit, z,
                       kind=PINV_STAIR):
        """Capture the whole step into one hipGraph (gbdpcg_graph_create_kkt_step_*)."""
        suf, args = self._kkt_args(nx, nu, N, batch, G, C, g, c, S, gamma, Ginv, Pinv, kind, lam, r, p, tol, max_iter, iters,
                                   max_iter_exit, z)
        gr = ctypes.c_void_p()
        fn = getattr(self.lib, f"gbdpcg_graph_create_kkt_step_{suf}")
        self._check(fn(*args, ctypes.byref(gr)), "graph_create_kkt_step")
        return Graph(self, gr, keep=(G, C, g, c, S, gamma, Ginv, Pinv, lam, r, p, iters, max_iter_exit, z))

    # ---- per-problem regularisation: problem b on G_b + rho_b I, rho a device tensor [batch] of G's dtype (include/gbdpcg.h)
    @staticmethod
    def _rho(rho, batch, G):
        assert rho is not None and rho.is_cuda and rho.is_contiguous() and rho.numel() == batch and rho.dtype == G.dtype
        return rho

    def form_schur_reg(self, nx, nu, N, batch, G, C, g, c, rho, S=None, gamma=None, Ginv=None, want_ginv=True, stream=None):
        """gbdpcg_form_schur_reg_*: S, gamma and (optionally) the inverse blocks of G + rho I, the add fused into the formation."""
        import torch
        suf, _ = _suffix(G)
        if S is None:
            S = torch.empty(batch * 3 * nx * nx * N, dtype=G.dtype, device=G.device)
        if gamma is None:
            gamma = torch.empty(batch * nx * N, dtype=G.dtype, device=G.device)
        if Ginv is None and want_ginv:
            Ginv = torch.empty_like(G)
        fn = getattr(self.lib, f"gbdpcg_form_schur_reg_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(G), _p(C), _p(g), _p(c), _p(self._rho(rho, batch, G)), _p(S), _p(gamma), _p(Ginv),
                       self._stream(stream)), "form_schur_reg")
        return S, gamma, Ginv

    def _kkt_reg_args(self, nx, nu, N, batch, G, C, g, c, rho, S, gamma, Ginv, Pinv, kind, lam, r, p, tol, max_iter, iters, mie, z):
        suf, _ = _suffix(G)
        return suf, (self.h, nx, nu, N, batch, _p(G), _p(C), _p(g), _p(c), _p(self._rho(rho, batch, G)), _p(S), _p(gamma), _p(Ginv),
                     _p(Pinv), kind, _p(lam), _p(r), _p(p), tol, max_iter, _p(iters), _p(mie), _p(z))

    def kkt_step_reg(self, nx, nu, N, batch, G, C, g, c, rho, S, gamma, Ginv, Pinv, lam, z, kind=PINV_STAIR, r=None, p=None, tol=1e-6,
                     max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_kkt_step_reg_*: the whole step of kkt_step on G + rho I, one call."""
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=G.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=G.device)
        suf, args = self._kkt_reg_args(nx, nu, N, batch, G, C, g, c, rho, S, gamma, Ginv, Pinv, kind, lam, r, p, tol, max_iter, iters,
                                       max_iter_exit, z)
        self._check(getattr(self.lib, f"gbdpcg_kkt_step_reg_{suf}")(*args, self._stream(stream)), "kkt_step_reg")
        return iters, max_iter_exit

    def graph_kkt_step_reg(self, nx, nu, N, batch, G, C, g, c, rho, S, gamma, Ginv, Pinv, lam, r, p, tol, max_iter, iters,
                           max_iter_exit, z, kind=PINV_STAIR):
        """Capture the regularised step into one hipGraph (gbdpcg_graph_create_kkt_step_reg_*): the graph keeps rho's pointer,
        rewrite the tensor in place between replays."""
        suf, args = self._kkt_reg_args(nx, nu, N, batch, G, C, g, c, rho, S, gamma, Ginv, Pinv, kind, lam, r, p, tol, max_iter, iters,
                                       max_iter_exit, z)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_kkt_step_reg_{suf}")(*args, ctypes.byref(gr)), "graph_create_kkt_step_reg")
        return Graph(self, gr, keep=(G, C, g, c, rho, S, gamma, Ginv, Pinv, lam, r, p, iters, max_iter_exit, z))

    def kkt_residual_reg(self, nx, nu, N, batch, G, C, g, c, rho, z, lam, res=None, stream=None):
        """gbdpcg_kkt_residual_reg_*: [batch, 2] tensor of (||(G + rho I) z + g + C' lambda||_inf, ||C z - c||_inf) per problem."""
        import torch
        suf, _ = _suffix(G)
        if res is None:
            res = torch.empty(batch, 2, dtype=G.dtype, device=G.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == G.dtype
        fn = getattr(self.lib, f"gbdpcg_kkt_residual_reg_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(G), _p(C), _p(g), _p(c), _p(self._rho(rho, batch, G)), _p(z), _p(lam), _p(res),
                       self._stream(stream)), "kkt_residual_reg")
        return res.view(batch, 2)

    # ---- box constraints on a kept factorisation: ADMM iterations around kkt_resolve (include/gbdpcg.h).  lo, hi, w, y, gt have the
    # layout of g; rho is a device tensor [batch]; the matrices are those kkt_step_reg / form_schur_reg wrote with that rho
    def _box(self, g, batch, *tensors):
        for t in tensors:
            assert t is not None and t.is_cuda and t.is_contiguous() and t.numel() == g.numel() and t.dtype == g.dtype
        return tensors

    def admm_init(self, nx, nu, N, batch, g, lo, hi, rho, w, y, gt=None, stream=None):
        """gbdpcg_admm_init_*: w <- clip(w, lo, hi), gt <- g - rho (w - y); y is left alone.  Returns gt."""
        import torch
        suf, _ = _suffix(g)
        if gt is None:
            gt = torch.empty_like(g)
        self._box(g, batch, lo, hi, w, y, gt)
        fn = getattr(self.lib, f"gbdpcg_admm_init_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(g), _p(lo), _p(hi), _p(self._rho(rho, batch, g)), _p(w), _p(y), _p(gt),
                       self._stream(stream)), "admm_init")
        return gt

    def admm_update(self, nx, nu, N, batch, g, lo, hi, rho, z, w, y, gt, res=None, stream=None):
        """gbdpcg_admm_update_*: the update behind a solve that wrote z -- w, y, gt in place; returns the [batch, 2] tensor of
        (||z - w||_inf, rho ||w - w_old||_inf) per problem."""
        import torch
        suf, _ = _suffix(g)
        if res is None:
            res = torch.empty(batch, 2, dtype=g.dtype, device=g.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == g.dtype
        self._box(g, batch, lo, hi, z, w, y, gt)
        fn = getattr(self.lib, f"gbdpcg_admm_update_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(g), _p(lo), _p(hi), _p(self._rho(rho, batch, g)), _p(z), _p(w), _p(y), _p(gt),
                       _p(res), self._stream(stream)), "admm_update")
        return res.view(batch, 2)

    # One set of helpers for the three families.  rows = (mx, mu, E) for the calls with stage-wise rows (lo, hi, w, y then have the
    # layout of the rows), cones = (lx, qx, lu, qu) next to rows for the calls with cone rows; `name` ends in "shared" for the twins.
    def _admm_step_args(self, name, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters, mie,
                        z, w, y, gt, res, rows=None, cones=None, kappa=None):
        """(suffix, the argument tuple up to d_res, the tensors a graph has to keep alive).  kappa: the soft families, behind hi."""
        suf, _ = _suffix(g)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == g.dtype
        sizes, E = (), ()
        soft = () if kappa is None else (kappa,)
        if rows is None:
            assert cones is None
            self._box(g, batch, lo, hi, z, w, y, gt, *soft)
        else:
            mx, mu, E = rows
            self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y) + soft, (g, z, gt), mats=1 if name.endswith("shared") else None)
            sizes, E = (mx, mu), (E,)
            if cones is not None:
                assert len(cones) == 4
                sizes += tuple(int(v) for v in cones)
        args = ((self.h, nx, nu) + sizes + (N, batch, _p(Ginv), _p(C), _p(g), _p(c)) + tuple(_p(t) for t in E) +
                (_p(lo), _p(hi)) + tuple(_p(t) for t in soft) +
                (_p(self._rho(rho, batch, g)), _p(S), _p(Pinv), _p(gamma), _p(lam), _p(r), _p(p), tol, max_iter,
                 _p(iters), _p(mie), _p(z), _p(w), _p(y), _p(gt), _p(res)))
        return suf, args, (Ginv, C, g, c) + E + (lo, hi) + soft + (rho, S, Pinv, gamma, lam, r, p, iters, mie, z, w, y, gt, res)

    def _admm_step(self, name, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, r, p, tol,
                   max_iter, iters, max_iter_exit, stream, rows=None, cones=None, kappa=None):
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=g.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=g.device)
        if res is None:
            res = torch.empty(batch, 2, dtype=g.dtype, device=g.device)
        suf, args, _ = self._admm_step_args(name, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter,
                                            iters, max_iter_exit, z, w, y, gt, res, rows, cones, kappa)
        self._check(getattr(self.lib, f"gbdpcg_{name}_{suf}")(*args, self._stream(stream)), name)
        return iters, max_iter_exit, res.view(batch, 2)

    def _graph_admm_step(self, name, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                         max_iter_exit, z, w, y, gt, res, rows=None, cones=None, kappa=None):
        suf, args, keep = self._admm_step_args(name, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                               max_iter, iters, max_iter_exit, z, w, y, gt, res, rows, cones, kappa)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_{name}_{suf}")(*args, ctypes.byref(gr)), f"graph_create_{name}")
        return Graph(self, gr, keep=keep)

    def admm_step(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None, r=None, p=None,
                  tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_step_*: kkt_resolve with gt in the place of g (warm start from lam), then admm_update, one call.
        Returns (iters, flags, res [batch, 2])."""
        return self._admm_step("admm_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, r, p,
                               tol, max_iter, iters, max_iter_exit, stream)

    def graph_admm_step(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                        max_iter_exit, z, w, y, gt, res):
        """Capture one ADMM iteration into a hipGraph (gbdpcg_graph_create_admm_step_*): replay it once per iteration; the graph
        keeps rho's pointer."""
        return self._graph_admm_step("admm_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res)

    def admm_step_shared(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None, r=None,
                         p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_step_shared_*: ONE Ginv, C, S, Pinv for `batch` problems; box, rho and the state stay per problem."""
        return self._admm_step("admm_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                               r, p, tol, max_iter, iters, max_iter_exit, stream)

    def graph_admm_step_shared(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                               max_iter_exit, z, w, y, gt, res):
        """Capture the shared-matrix iteration into a hipGraph (gbdpcg_graph_create_admm_step_shared_*)."""
        return self._graph_admm_step("admm_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res)

    # ---- stage-wise linear rows lo <= E z <= hi on a kept factorisation of G + rho E'E (include/gbdpcg.h).  E: [Ex_0 Eu_0 ... Ex_{N-1}]
    # column-major blocks (one problem's in the shared calls); lo, hi, w, y have the layout of the rows; gt that of g
    @staticmethod
    def _lin_sizes(nx, nu, mx, mu, N):
        """(nz, nw, ne, ng): elements per problem of g / the rows / E / G."""
        return (nx + nu) * N - nu, (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu, (nx * nx + nu * nu) * N - nu * nu

    def _lin(self, g, batch, nx, nu, mx, mu, N, E, rows, vectors, mats=None):
        """The sizes of E (`mats` problems' worth, default batch), of the row arrays and of the arrays laid out like g."""
        nz, nw, ne, _ = self._lin_sizes(nx, nu, mx, mu, N)
        for t, cnt in [(E, (batch if mats is None else mats) * ne)] + [(t, batch * nw) for t in rows] + [(t, batch * nz) for t in vectors]:
            assert t is not None and t.is_cuda and t.is_contiguous() and t.numel() == cnt and t.dtype == g.dtype

    def admm_lin_form(self, nx, nu, mx, mu, N, batch, G, E, rho, Gt=None, stream=None):
        """gbdpcg_admm_lin_form_*: Gt = G + rho E'E in the layout of G (Gt may be G).  Returns Gt."""
        import torch
        suf, _ = _suffix(G)
        if Gt is None:
            Gt = torch.empty_like(G)
        _, _, ne, ng = self._lin_sizes(nx, nu, mx, mu, N)
        for t, cnt in ((G, batch * ng), (Gt, batch * ng), (E, batch * ne)):
            assert t is not None and t.is_cuda and t.is_contiguous() and t.numel() == cnt and t.dtype == G.dtype
        fn = getattr(self.lib, f"gbdpcg_admm_lin_form_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(G), _p(E), _p(self._rho(rho, batch, G)), _p(Gt), self._stream(stream)),
                    "admm_lin_form")
        return Gt

    def admm_lin_init(self, nx, nu, mx, mu, N, batch, g, E, lo, hi, rho, w, y, gt=None, stream=None):
        """gbdpcg_admm_lin_init_*: w <- clip(w, lo, hi), gt <- g - rho E'(w - y); y is left alone.  Returns gt."""
        import torch
        suf, _ = _suffix(g)
        if gt is None:
            gt = torch.empty_like(g)
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y), (g, gt))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_init_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(g), _p(E), _p(lo), _p(hi), _p(self._rho(rho, batch, g)), _p(w), _p(y),
                       _p(gt), self._stream(stream)), "admm_lin_init")
        return gt

    def admm_lin_update(self, nx, nu, mx, mu, N, batch, g, E, lo, hi, rho, z, w, y, gt, res=None, stream=None):
        """gbdpcg_admm_lin_update_*: the update behind a solve that wrote z -- w, y, gt in place; returns the [batch, 2] tensor of
        (||E z - w||_inf, rho ||E'(w - w_old)||_inf) per problem."""
        import torch
        suf, _ = _suffix(g)
        if res is None:
            res = torch.empty(batch, 2, dtype=g.dtype, device=g.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == g.dtype
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y), (g, z, gt))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_update_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(g), _p(E), _p(lo), _p(hi), _p(self._rho(rho, batch, g)), _p(z), _p(w),
                       _p(y), _p(gt), _p(res), self._stream(stream)), "admm_lin_update")
        return res.view(batch, 2)

    def admm_lin_step(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None, r=None,
                      p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_lin_step_*: kkt_resolve with gt in the place of g (warm start from lam), then admm_lin_update, one call.
        Returns (iters, flags, res [batch, 2])."""
        return self._admm_step("admm_lin_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, r, p,
                               tol, max_iter, iters, max_iter_exit, stream, rows=(mx, mu, E))

    def graph_admm_lin_step(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                            max_iter_exit, z, w, y, gt, res):
        """Capture one iteration into a hipGraph (gbdpcg_graph_create_admm_lin_step_*): replay it once per iteration; the graph
        keeps rho's pointer."""
        return self._graph_admm_step("admm_lin_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, rows=(mx, mu, E))

    def admm_lin_step_shared(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None,
                             r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_lin_step_shared_*: ONE Ginv, C, S, Pinv and E for `batch` problems; bounds, rho and the state stay per
        problem."""
        return self._admm_step("admm_lin_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                               r, p, tol, max_iter, iters, max_iter_exit, stream, rows=(mx, mu, E))

    def graph_admm_lin_step_shared(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                   max_iter, iters, max_iter_exit, z, w, y, gt, res):
        """Capture the shared-matrix iteration into a hipGraph (gbdpcg_graph_create_admm_lin_step_shared_*)."""
        return self._graph_admm_step("admm_lin_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, rows=(mx, mu, E))

    # ---- second-order cone rows next to the linear ones (include/gbdpcg.h): cones = (lx, qx, lu, qu) -- the first lx rows of an x
    # block are linear, the rest cones of dimension qx, head row first; on a cone row lo holds the offset f and hi is not read.  The
    # formation is admm_lin_form.
    def admm_soc_init(self, nx, nu, mx, mu, cones, N, batch, g, E, lo, hi, rho, w, y, gt=None, stream=None):
        """gbdpcg_admm_soc_init_*: w <- its projection on the bounds / cones, gt <- g - rho E'(w - f - y); y is left alone.  Returns gt."""
        import torch
        suf, _ = _suffix(g)
        if gt is None:
            gt = torch.empty_like(g)
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y), (g, gt))
        fn = getattr(self.lib, f"gbdpcg_admm_soc_init_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, *cones, N, batch, _p(g), _p(E), _p(lo), _p(hi), _p(self._rho(rho, batch, g)), _p(w), _p(y),
                       _p(gt), self._stream(stream)), "admm_soc_init")
        return gt

    def admm_soc_update(self, nx, nu, mx, mu, cones, N, batch, g, E, lo, hi, rho, z, w, y, gt, res=None, stream=None):
        """gbdpcg_admm_soc_update_*: the update behind a solve that wrote z -- w, y, gt in place; returns the [batch, 2] tensor of
        (||E z + f - w||_inf, rho ||E'(w - w_old)||_inf) per problem."""
        import torch
        suf, _ = _suffix(g)
        if res is None:
            res = torch.empty(batch, 2, dtype=g.dtype, device=g.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == g.dtype
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y), (g, z, gt))
        fn = getattr(self.lib, f"gbdpcg_admm_soc_update_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, *cones, N, batch, _p(g), _p(E), _p(lo), _p(hi), _p(self._rho(rho, batch, g)), _p(z), _p(w),
                       _p(y), _p(gt), _p(res), self._stream(stream)), "admm_soc_update")
        return res.view(batch, 2)

    def admm_soc_step(self, nx, nu, mx, mu, cones, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None,
                      r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_soc_step_*: kkt_resolve with gt in the place of g (warm start from lam), then admm_soc_update, one call.
        Returns (iters, flags, res [batch, 2])."""
        return self._admm_step("admm_soc_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, r, p,
                               tol, max_iter, iters, max_iter_exit, stream, rows=(mx, mu, E), cones=cones)

    def graph_admm_soc_step(self, nx, nu, mx, mu, cones, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter,
                            iters, max_iter_exit, z, w, y, gt, res):
        """Capture one iteration into a hipGraph (gbdpcg_graph_create_admm_soc_step_*); the graph keeps rho's pointer."""
        return self._graph_admm_step("admm_soc_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, rows=(mx, mu, E), cones=cones)

    def admm_soc_step_shared(self, nx, nu, mx, mu, cones, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt,
                             res=None, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_soc_step_shared_*: ONE Ginv, C, S, Pinv and E for `batch` problems; bounds, offsets, rho and the state stay per
        problem."""
        return self._admm_step("admm_soc_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                               r, p, tol, max_iter, iters, max_iter_exit, stream, rows=(mx, mu, E), cones=cones)

    def graph_admm_soc_step_shared(self, nx, nu, mx, mu, cones, N, batch, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                   max_iter, iters, max_iter_exit, z, w, y, gt, res):
        """Capture the shared-matrix iteration into a hipGraph (gbdpcg_graph_create_admm_soc_step_shared_*)."""
        return self._graph_admm_step("admm_soc_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, rows=(mx, mu, E), cones=cones)

    # ---- adaptive rho (include/gbdpcg.h): residual balancing in powers of two on the device.  rho is rewritten in place, y rescaled so
    # that rho y stays, expo [batch] int32 receives the exponent applied to rho (+shift, -shift or 0)
    @staticmethod
    def _expo(expo, batch, like):
        import torch
        if expo is None:
            expo = torch.zeros(batch, dtype=torch.int32, device=like.device)
        assert expo.is_cuda and expo.is_contiguous() and expo.numel() == batch and expo.dtype == torch.int32
        return expo

    @staticmethod
    def _res(res, batch, g):
        assert res is not None and res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == g.dtype
        return res

    def admm_rebalance(self, nx, nu, N, batch, g, res, rho, w, y, gt, expo=None, *, ratio=10.0, shift=1, rho_min, rho_max, stream=None):
        """gbdpcg_admm_rebalance_*: rho and y in place from the residuals in res, gt rebuilt as admm_init would, one launch.
        Returns expo."""
        suf, _ = _suffix(g)
        self._box(g, batch, w, y, gt)
        expo = self._expo(expo, batch, g)
        fn = getattr(self.lib, f"gbdpcg_admm_rebalance_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(g), _p(self._res(res, batch, g)), _p(self._rho(rho, batch, g)), _p(w), _p(y), _p(gt),
                       ratio, shift, rho_min, rho_max, _p(expo), self._stream(stream)), "admm_rebalance")
        return expo

    def _rows_rebalance(self, name, sizes, nx, nu, mx, mu, N, batch, g, E, lo, hi, res, rho, w, y, gt, expo, ratio, shift, rho_min, rho_max,
                        stream, kappa=None):
        suf, _ = _suffix(g)
        soft = () if kappa is None else (kappa,)
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y) + soft, (g, gt))
        expo = self._expo(expo, batch, g)
        fn = getattr(self.lib, f"gbdpcg_{name}_{suf}")
        self._check(fn(self.h, nx, nu, *sizes, N, batch, _p(g), _p(E), _p(lo), _p(hi), *(_p(t) for t in soft), _p(self._res(res, batch, g)),
                       _p(self._rho(rho, batch, g)), _p(w), _p(y), _p(gt), ratio, shift, rho_min, rho_max, _p(expo), self._stream(stream)),
                    name)
        return expo

    def admm_lin_rebalance(self, nx, nu, mx, mu, N, batch, g, E, lo, hi, res, rho, w, y, gt, expo=None, *, ratio=10.0, shift=1, rho_min,
                           rho_max, stream=None):
        """gbdpcg_admm_lin_rebalance_*: rho and y (layout of the rows) in place, then admm_lin_init rebuilds gt.  Returns expo."""
        return self._rows_rebalance("admm_lin_rebalance", (mx, mu), nx, nu, mx, mu, N, batch, g, E, lo, hi, res, rho, w, y, gt, expo, ratio,
                                    shift, rho_min, rho_max, stream)

    def admm_soc_rebalance(self, nx, nu, mx, mu, cones, N, batch, g, E, lo, hi, res, rho, w, y, gt, expo=None, *, ratio=10.0, shift=1,
                           rho_min, rho_max, stream=None):
        """gbdpcg_admm_soc_rebalance_*: the same through admm_soc_init, which re-projects w (cone rows may move by ulps).  Returns expo."""
        assert len(cones) == 4
        return self._rows_rebalance("admm_soc_rebalance", (mx, mu) + tuple(int(v) for v in cones), nx, nu, mx, mu, N, batch, g, E, lo, hi,
                                    res, rho, w, y, gt, expo, ratio, shift, rho_min, rho_max, stream)

    def _admm_restep_args(self, nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, kind, gamma, lam, r, p, tol, max_iter, iters,
                          mie, z, w, y, gt, res, expo, ratio, shift, rho_min, rho_max, rows=None, cones=None, kappa=None):
        """(suffix, the argument tuple up to d_expo, the tensors a graph has to keep alive); Gt is None for the box."""
        suf, _ = _suffix(g)
        self._res(res, batch, g)
        sizes, E, mats = (), (), (G,)
        soft = () if kappa is None else (kappa,)
        if rows is None:
            assert cones is None and Gt is None
            self._box(g, batch, lo, hi, z, w, y, gt, *soft)
        else:
            mx, mu, E = rows
            self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, w, y) + soft, (g, z, gt))
            assert Gt is not None and Gt.numel() == G.numel() and Gt.dtype == G.dtype and Gt.is_cuda and Gt.is_contiguous()
            sizes, E, mats = (mx, mu), (E,), (G, Gt)
            if cones is not None:
                assert len(cones) == 4
                sizes += tuple(int(v) for v in cones)
        args = ((self.h, nx, nu) + sizes + (N, batch) + tuple(_p(t) for t in mats) + (_p(Ginv), _p(C), _p(g), _p(c)) +
                tuple(_p(t) for t in E) + (_p(lo), _p(hi)) + tuple(_p(t) for t in soft) +
                (_p(self._rho(rho, batch, g)), _p(S), _p(Pinv), kind, _p(gamma), _p(lam), _p(r), _p(p), tol, max_iter, _p(iters), _p(mie),
                 _p(z), _p(w), _p(y), _p(gt), _p(res), ratio, shift, rho_min, rho_max, _p(expo)))
        return suf, args, mats + (Ginv, C, g, c) + E + (lo, hi) + soft + (rho, S, Pinv, gamma, lam, r, p, iters, mie, z, w, y, gt, res, expo)

    def _admm_restep(self, name, nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, expo, kind, r, p,
                     tol, max_iter, iters, max_iter_exit, ratio, shift, rho_min, rho_max, stream, rows=None, cones=None, kappa=None):
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=g.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=g.device)
        expo = self._expo(expo, batch, g)
        suf, args, _ = self._admm_restep_args(nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, kind, gamma, lam, r, p, tol,
                                              max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, ratio, shift, rho_min, rho_max,
                                              rows, cones, kappa)
        self._check(getattr(self.lib, f"gbdpcg_{name}_{suf}")(*args, self._stream(stream)), name)
        return iters, max_iter_exit, res.view(batch, 2), expo

    def _graph_admm_restep(self, name, nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                           max_iter_exit, z, w, y, gt, res, expo, kind, ratio, shift, rho_min, rho_max, rows=None, cones=None, kappa=None):
        suf, args, keep = self._admm_restep_args(nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, kind, gamma, lam, r, p, tol,
                                                 max_iter, iters, max_iter_exit, z, w, y, gt, res, self._expo(expo, batch, g), ratio,
                                                 shift, rho_min, rho_max, rows, cones, kappa)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_{name}_{suf}")(*args, ctypes.byref(gr)), f"graph_create_{name}")
        return Graph(self, gr, keep=keep)

    def admm_restep(self, nx, nu, N, batch, G, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, expo=None, kind=PINV_STAIR,
                    r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, *, ratio=10.0, shift=1, rho_min, rho_max,
                    stream=None):
        """gbdpcg_admm_restep_*: one iteration with a new rho -- admm_rebalance, kkt_step_reg on G and rho with gt in the place of g,
        admm_update.  Every problem is refactored.  Returns (iters, flags, res [batch, 2], expo)."""
        return self._admm_restep("admm_restep", nx, nu, N, batch, G, None, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                                 expo, kind, r, p, tol, max_iter, iters, max_iter_exit, ratio, shift, rho_min, rho_max, stream)

    def graph_admm_restep(self, nx, nu, N, batch, G, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                          max_iter_exit, z, w, y, gt, res, expo, kind=PINV_STAIR, *, ratio=10.0, shift=1, rho_min, rho_max):
        """Capture the iteration with a new rho into a hipGraph (gbdpcg_graph_create_admm_restep_*): replay it once per P replays of the
        step graph; it keeps the pointers of rho, res and expo."""
        return self._graph_admm_restep("admm_restep", nx, nu, N, batch, G, None, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                       max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind, ratio, shift, rho_min, rho_max)

    def admm_lin_restep(self, nx, nu, mx, mu, N, batch, G, Gt, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, expo=None,
                        kind=PINV_STAIR, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, *, ratio=10.0, shift=1,
                        rho_min, rho_max, stream=None):
        """gbdpcg_admm_lin_restep_*: admm_lin_rebalance, admm_lin_form from G into Gt (not G itself), kkt_step on Gt with gt in the
        place of g, admm_lin_update.  Returns (iters, flags, res [batch, 2], expo)."""
        return self._admm_restep("admm_lin_restep", nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                                 expo, kind, r, p, tol, max_iter, iters, max_iter_exit, ratio, shift, rho_min, rho_max, stream,
                                 rows=(mx, mu, E))

    def graph_admm_lin_restep(self, nx, nu, mx, mu, N, batch, G, Gt, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol, max_iter,
                              iters, max_iter_exit, z, w, y, gt, res, expo, kind=PINV_STAIR, *, ratio=10.0, shift=1, rho_min, rho_max):
        """Capture gbdpcg_admm_lin_restep_* into a hipGraph; it keeps the pointers of rho, res and expo."""
        return self._graph_admm_restep("admm_lin_restep", nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                       max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind, ratio, shift, rho_min, rho_max,
                                       rows=(mx, mu, E))

    def admm_soc_restep(self, nx, nu, mx, mu, cones, N, batch, G, Gt, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                        expo=None, kind=PINV_STAIR, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, *, ratio=10.0,
                        shift=1, rho_min, rho_max, stream=None):
        """gbdpcg_admm_soc_restep_*: the same with cone rows (admm_soc_rebalance, admm_soc_update).  Returns (iters, flags, res, expo)."""
        return self._admm_restep("admm_soc_restep", nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res,
                                 expo, kind, r, p, tol, max_iter, iters, max_iter_exit, ratio, shift, rho_min, rho_max, stream,
                                 rows=(mx, mu, E), cones=cones)

    def graph_admm_soc_restep(self, nx, nu, mx, mu, cones, N, batch, G, Gt, Ginv, C, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                              max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind=PINV_STAIR, *, ratio=10.0, shift=1, rho_min,
                              rho_max):
        """Capture gbdpcg_admm_soc_restep_* into a hipGraph; it keeps the pointers of rho, res and expo."""
        return self._graph_admm_restep("admm_soc_restep", nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                       max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind, ratio, shift, rho_min, rho_max,
                                       rows=(mx, mu, E), cones=cones)

    # ---- soft (L1-penalised) bounds (include/gbdpcg.h): the box and the linear rows with the weights kappa, laid out like lo and hi
    # and passed directly behind hi; +Inf keeps a row hard, 0 frees it.  Everything else mirrors the hard methods.  The rebalance of
    # the soft box is admm_rebalance.
    def admm_soft_init(self, nx, nu, N, batch, g, lo, hi, kappa, rho, w, y, gt=None, stream=None):
        """gbdpcg_admm_soft_init_*: w <- clip(w, lo, hi) where kappa = +Inf only, gt <- g - rho (w - y); y is left alone.  Returns gt."""
        import torch
        suf, _ = _suffix(g)
        if gt is None:
            gt = torch.empty_like(g)
        self._box(g, batch, lo, hi, kappa, w, y, gt)
        fn = getattr(self.lib, f"gbdpcg_admm_soft_init_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(g), _p(lo), _p(hi), _p(kappa), _p(self._rho(rho, batch, g)), _p(w), _p(y), _p(gt),
                       self._stream(stream)), "admm_soft_init")
        return gt

    def admm_soft_update(self, nx, nu, N, batch, g, lo, hi, kappa, rho, z, w, y, gt, res=None, stream=None):
        """gbdpcg_admm_soft_update_*: the soft update behind a solve that wrote z; returns the [batch, 2] tensor of residual norms."""
        import torch
        suf, _ = _suffix(g)
        if res is None:
            res = torch.empty(batch, 2, dtype=g.dtype, device=g.device)
        self._res(res, batch, g)
        self._box(g, batch, lo, hi, kappa, z, w, y, gt)
        fn = getattr(self.lib, f"gbdpcg_admm_soft_update_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(g), _p(lo), _p(hi), _p(kappa), _p(self._rho(rho, batch, g)), _p(z), _p(w), _p(y),
                       _p(gt), _p(res), self._stream(stream)), "admm_soft_update")
        return res.view(batch, 2)

    def admm_soft_step(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None, r=None, p=None,
                       tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_soft_step_*: kkt_resolve with gt in the place of g, then admm_soft_update.  Returns (iters, flags, res)."""
        return self._admm_step("admm_soft_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, r, p,
                               tol, max_iter, iters, max_iter_exit, stream, kappa=kappa)

    def graph_admm_soft_step(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                             max_iter_exit, z, w, y, gt, res):
        """Capture one soft iteration into a hipGraph (gbdpcg_graph_create_admm_soft_step_*)."""
        return self._graph_admm_step("admm_soft_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, kappa=kappa)

    def admm_soft_step_shared(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None, r=None,
                              p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_soft_step_shared_*: ONE Ginv, C, S, Pinv; bounds, kappa, rho and the state stay per problem."""
        return self._admm_step("admm_soft_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt,
                               res, r, p, tol, max_iter, iters, max_iter_exit, stream, kappa=kappa)

    def graph_admm_soft_step_shared(self, nx, nu, N, batch, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, r, p, tol, max_iter,
                                    iters, max_iter_exit, z, w, y, gt, res):
        """Capture the shared-matrix soft iteration into a hipGraph (gbdpcg_graph_create_admm_soft_step_shared_*)."""
        return self._graph_admm_step("admm_soft_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, kappa=kappa)

    def admm_soft_restep(self, nx, nu, N, batch, G, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res, expo=None,
                         kind=PINV_STAIR, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, *, ratio=10.0, shift=1,
                         rho_min, rho_max, stream=None):
        """gbdpcg_admm_soft_restep_*: admm_rebalance, kkt_step_reg with gt in the place of g, admm_soft_update.
        Returns (iters, flags, res [batch, 2], expo)."""
        return self._admm_restep("admm_soft_restep", nx, nu, N, batch, G, None, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt,
                                 res, expo, kind, r, p, tol, max_iter, iters, max_iter_exit, ratio, shift, rho_min, rho_max, stream,
                                 kappa=kappa)

    def graph_admm_soft_restep(self, nx, nu, N, batch, G, Ginv, C, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, r, p, tol, max_iter, iters,
                               max_iter_exit, z, w, y, gt, res, expo, kind=PINV_STAIR, *, ratio=10.0, shift=1, rho_min, rho_max):
        """Capture gbdpcg_admm_soft_restep_* into a hipGraph; it keeps the pointers of rho, res and expo."""
        return self._graph_admm_restep("admm_soft_restep", nx, nu, N, batch, G, None, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p,
                                       tol, max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind, ratio, shift, rho_min, rho_max,
                                       kappa=kappa)

    def admm_lin_soft_init(self, nx, nu, mx, mu, N, batch, g, E, lo, hi, kappa, rho, w, y, gt=None, stream=None):
        """gbdpcg_admm_lin_soft_init_*: w <- clip(w) where kappa = +Inf only, gt <- g - rho E'(w - y); y is left alone.  Returns gt."""
        import torch
        suf, _ = _suffix(g)
        if gt is None:
            gt = torch.empty_like(g)
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, kappa, w, y), (g, gt))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_soft_init_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(g), _p(E), _p(lo), _p(hi), _p(kappa), _p(self._rho(rho, batch, g)), _p(w),
                       _p(y), _p(gt), self._stream(stream)), "admm_lin_soft_init")
        return gt

    def admm_lin_soft_update(self, nx, nu, mx, mu, N, batch, g, E, lo, hi, kappa, rho, z, w, y, gt, res=None, stream=None):
        """gbdpcg_admm_lin_soft_update_*: the soft update of the rows behind a solve that wrote z; returns res [batch, 2]."""
        import torch
        suf, _ = _suffix(g)
        if res is None:
            res = torch.empty(batch, 2, dtype=g.dtype, device=g.device)
        self._res(res, batch, g)
        self._lin(g, batch, nx, nu, mx, mu, N, E, (lo, hi, kappa, w, y), (g, z, gt))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_soft_update_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(g), _p(E), _p(lo), _p(hi), _p(kappa), _p(self._rho(rho, batch, g)), _p(z),
                       _p(w), _p(y), _p(gt), _p(res), self._stream(stream)), "admm_lin_soft_update")
        return res.view(batch, 2)

    def admm_lin_soft_step(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res=None,
                           r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_lin_soft_step_*: kkt_resolve with gt in the place of g, then admm_lin_soft_update.  Returns (iters, flags, res)."""
        return self._admm_step("admm_lin_soft_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res, r,
                               p, tol, max_iter, iters, max_iter_exit, stream, rows=(mx, mu, E), kappa=kappa)

    def graph_admm_lin_soft_step(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, r, p, tol,
                                 max_iter, iters, max_iter_exit, z, w, y, gt, res):
        """Capture one soft iteration with rows into a hipGraph (gbdpcg_graph_create_admm_lin_soft_step_*)."""
        return self._graph_admm_step("admm_lin_soft_step", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p, tol,
                                     max_iter, iters, max_iter_exit, z, w, y, gt, res, rows=(mx, mu, E), kappa=kappa)

    def admm_lin_soft_step_shared(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt,
                                  res=None, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_lin_soft_step_shared_*: ONE Ginv, C, S, Pinv and E; bounds, kappa, rho and the state stay per problem."""
        return self._admm_step("admm_lin_soft_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt,
                               res, r, p, tol, max_iter, iters, max_iter_exit, stream, rows=(mx, mu, E), kappa=kappa)

    def graph_admm_lin_soft_step_shared(self, nx, nu, mx, mu, N, batch, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, r, p,
                                        tol, max_iter, iters, max_iter_exit, z, w, y, gt, res):
        """Capture the shared-matrix soft iteration with rows into a hipGraph (gbdpcg_graph_create_admm_lin_soft_step_shared_*)."""
        return self._graph_admm_step("admm_lin_soft_step_shared", nx, nu, N, batch, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r, p,
                                     tol, max_iter, iters, max_iter_exit, z, w, y, gt, res, rows=(mx, mu, E), kappa=kappa)

    def admm_lin_soft_rebalance(self, nx, nu, mx, mu, N, batch, g, E, lo, hi, kappa, res, rho, w, y, gt, expo=None, *, ratio=10.0, shift=1,
                                rho_min, rho_max, stream=None):
        """gbdpcg_admm_lin_soft_rebalance_*: rho and y in place, then admm_lin_soft_init rebuilds gt.  Returns expo."""
        return self._rows_rebalance("admm_lin_soft_rebalance", (mx, mu), nx, nu, mx, mu, N, batch, g, E, lo, hi, res, rho, w, y, gt, expo,
                                    ratio, shift, rho_min, rho_max, stream, kappa=kappa)

    def admm_lin_soft_restep(self, nx, nu, mx, mu, N, batch, G, Gt, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt,
                             res, expo=None, kind=PINV_STAIR, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, *,
                             ratio=10.0, shift=1, rho_min, rho_max, stream=None):
        """gbdpcg_admm_lin_soft_restep_*: admm_lin_soft_rebalance, admm_lin_form into Gt, kkt_step on Gt, admm_lin_soft_update.
        Returns (iters, flags, res [batch, 2], expo)."""
        return self._admm_restep("admm_lin_soft_restep", nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y,
                                 gt, res, expo, kind, r, p, tol, max_iter, iters, max_iter_exit, ratio, shift, rho_min, rho_max, stream,
                                 rows=(mx, mu, E), kappa=kappa)

    def graph_admm_lin_soft_restep(self, nx, nu, mx, mu, N, batch, G, Gt, Ginv, C, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, r, p,
                                   tol, max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind=PINV_STAIR, *, ratio=10.0, shift=1,
                                   rho_min, rho_max):
        """Capture gbdpcg_admm_lin_soft_restep_* into a hipGraph; it keeps the pointers of rho, res and expo."""
        return self._graph_admm_restep("admm_lin_soft_restep", nx, nu, N, batch, G, Gt, Ginv, C, g, c, lo, hi, rho, S, Pinv, gamma, lam, r,
                                       p, tol, max_iter, iters, max_iter_exit, z, w, y, gt, res, expo, kind, ratio, shift, rho_min,
                                       rho_max, rows=(mx, mu, E), kappa=kappa)

    # ---- the backward pass (include/gbdpcg.h): gradients of a scalar in G and C from the forward point (z, lam) and the adjoint pair
    # (az, alam), which is kkt_resolve with g := dl/dz, c := -dl/dlambda on the kept factorisation
    def _grad_args(self, nx, nu, N, batch, z, lam, az, alam, gG, gC, shared):
        import torch
        suf, _ = _suffix(z)
        nz, nl, mats = (nx + nu) * N - nu, nx * N, 1 if shared else batch
        for t, cnt in ((z, batch * nz), (az, batch * nz), (lam, batch * nl), (alam, batch * nl),
                       (gG, mats * ((nx * nx + nu * nu) * N - nu * nu)), (gC, mats * (nx * nx + nx * nu) * (N - 1))):
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.numel() == cnt and t.dtype == z.dtype):
                    raise ValueError("the backward pass takes contiguous device tensors of one dtype in the layouts of include/gbdpcg.h")
        return suf

    def _kkt_grad(self, name, nx, nu, N, batch, z, lam, az, alam, gG, gC, want, stream):
        import torch
        shared = name.endswith("shared")
        mats = 1 if shared else batch
        if gG is None and "G" in want:
            gG = torch.empty(mats * ((nx * nx + nu * nu) * N - nu * nu), dtype=z.dtype, device=z.device)
        if gC is None and "C" in want:
            gC = torch.empty(mats * (nx * nx + nx * nu) * (N - 1), dtype=z.dtype, device=z.device)
        suf = self._grad_args(nx, nu, N, batch, z, lam, az, alam, gG, gC, shared)
        fn = getattr(self.lib, f"gbdpcg_{name}_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(z), _p(lam), _p(az), _p(alam), _p(gG), _p(gC), self._stream(stream)), name)
        return gG, gC

    def kkt_grad(self, nx, nu, N, batch, z, lam, az, alam, gG=None, gC=None, want="GC", stream=None):
        """gbdpcg_kkt_grad_*: (gG, gC) in the layouts of G and C, per problem.  want: which outputs to allocate when none is passed
        ("G", "C" or "GC"); an output that is neither passed nor wanted is skipped (None)."""
        return self._kkt_grad("kkt_grad", nx, nu, N, batch, z, lam, az, alam, gG, gC, want, stream)

    def kkt_grad_shared(self, nx, nu, N, batch, z, lam, az, alam, gG=None, gC=None, want="GC", stream=None):
        """gbdpcg_kkt_grad_shared_*: ONE problem's worth of gG, gC, summed over the batch in a fixed order."""
        return self._kkt_grad("kkt_grad_shared", nx, nu, N, batch, z, lam, az, alam, gG, gC, want, stream)

    def _backward_args(self, shared, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r, p, tol, max_iter, iters,
                       mie, gG, gC):
        suf = self._grad_args(nx, nu, N, batch, z, lam, az, alam, gG, gC, shared)
        self._grad_args(nx, nu, N, batch, gz, nglam, gz, gamma, None, None, shared)
        return suf, (self.h, nx, nu, N, batch, _p(Ginv), _p(C), _p(gz), _p(nglam), _p(S), _p(Pinv), _p(gamma), _p(z), _p(lam), _p(az),
                     _p(alam), _p(r), _p(p), tol, max_iter, _p(iters), _p(mie), _p(gG), _p(gC))

    def _kkt_backward(self, name, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, gG, gC, r, p, tol, max_iter,
                      iters, max_iter_exit, stream):
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=z.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=z.device)
        suf, args = self._backward_args(name.endswith("shared"), nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r,
                                        p, tol, max_iter, iters, max_iter_exit, gG, gC)
        self._check(getattr(self.lib, f"gbdpcg_{name}_{suf}")(*args, self._stream(stream)), name)
        return iters, max_iter_exit

    def _graph_kkt_backward(self, name, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r, p, tol, max_iter,
                            iters, max_iter_exit, gG, gC):
        suf, args = self._backward_args(name.endswith("shared"), nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r,
                                        p, tol, max_iter, iters, max_iter_exit, gG, gC)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_{name}_{suf}")(*args, ctypes.byref(gr)), f"graph_create_{name}")
        return Graph(self, gr, keep=(Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r, p, iters, max_iter_exit, gG, gC))

    def kkt_backward(self, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, gG, gC, r=None, p=None, tol=1e-6,
                     max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_kkt_backward_*: the adjoint solve (kkt_resolve with g := gz, c := nglam = -dl/dlambda, warm start from alam, writing
        alam and az) and kkt_grad on (z, lam, az, alam), one call.  Returns the (iters, flags) of the adjoint solve."""
        return self._kkt_backward("kkt_backward", nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, gG, gC, r, p,
                                  tol, max_iter, iters, max_iter_exit, stream)

    def kkt_backward_shared(self, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, gG, gC, r=None, p=None,
                            tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_kkt_backward_shared_*: ONE Ginv, C, S, Pinv; gG, gC one problem's worth, summed over the batch."""
        return self._kkt_backward("kkt_backward_shared", nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, gG, gC,
                                  r, p, tol, max_iter, iters, max_iter_exit, stream)

    def graph_kkt_backward(self, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r, p, tol, max_iter, iters,
                           max_iter_exit, gG, gC):
        """Capture the adjoint solve and the gradient launch into one hipGraph (gbdpcg_graph_create_kkt_backward_*): rewrite gz and
        nglam in place between replays."""
        return self._graph_kkt_backward("kkt_backward", nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r, p,
                                        tol, max_iter, iters, max_iter_exit, gG, gC)

    def graph_kkt_backward_shared(self, nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, r, p, tol, max_iter,
                                  iters, max_iter_exit, gG, gC):
        """Capture the shared-matrix backward pass into one hipGraph (gbdpcg_graph_create_kkt_backward_shared_*)."""
        return self._graph_kkt_backward("kkt_backward_shared", nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam,
                                        r, p, tol, max_iter, iters, max_iter_exit, gG, gC)

    # ---- the backward pass of the hard box QP (include/gbdpcg.h): the box family with yf, the forward y, where lo, hi stand; gz =
    # dl/dz in the place of g, nglam = -dl/dlambda in the place of c; wa, ya, gta the adjoint's splitting state, in the layout of g
    def admm_adjoint_init(self, nx, nu, N, batch, gz, yf, rho, wa, ya, gta=None, stream=None):
        """gbdpcg_admm_adjoint_init_*: wa <- 0 where yf != 0, gta <- gz - rho (wa - ya); ya is left alone.  Returns gta."""
        import torch
        suf, _ = _suffix(gz)
        if gta is None:
            gta = torch.empty_like(gz)
        self._box(gz, batch, yf, wa, ya, gta)
        fn = getattr(self.lib, f"gbdpcg_admm_adjoint_init_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(gz), _p(yf), _p(self._rho(rho, batch, gz)), _p(wa), _p(ya), _p(gta),
                       self._stream(stream)), "admm_adjoint_init")
        return gta

    def admm_adjoint_update(self, nx, nu, N, batch, gz, yf, rho, az, wa, ya, gta, res=None, stream=None):
        """gbdpcg_admm_adjoint_update_*: the update behind an adjoint solve that wrote az -- wa, ya, gta in place; returns the
        [batch, 2] tensor of (||az - wa||_inf, rho ||wa - wa_old||_inf) per problem."""
        import torch
        suf, _ = _suffix(gz)
        if res is None:
            res = torch.empty(batch, 2, dtype=gz.dtype, device=gz.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == gz.dtype
        self._box(gz, batch, yf, az, wa, ya, gta)
        fn = getattr(self.lib, f"gbdpcg_admm_adjoint_update_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(gz), _p(yf), _p(self._rho(rho, batch, gz)), _p(az), _p(wa), _p(ya), _p(gta),
                       _p(res), self._stream(stream)), "admm_adjoint_update")
        return res.view(batch, 2)

    def _adjoint_step_args(self, nx, nu, N, batch, Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma, alam, r, p, tol, max_iter, iters, mie,
                           az, wa, ya, gta, res):
        suf, _ = _suffix(gz)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == gz.dtype
        self._box(gz, batch, yf, az, wa, ya, gta)
        args = (self.h, nx, nu, N, batch, _p(Ginv), _p(C), _p(gz), _p(nglam), _p(yf), _p(self._rho(rho, batch, gz)), _p(S), _p(Pinv),
                _p(gamma), _p(alam), _p(r), _p(p), tol, max_iter, _p(iters), _p(mie), _p(az), _p(wa), _p(ya), _p(gta), _p(res))
        return suf, args, (Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma, alam, r, p, iters, mie, az, wa, ya, gta, res)

    def admm_adjoint_step(self, nx, nu, N, batch, Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma, alam, az, wa, ya, gta, res=None, r=None,
                          p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_adjoint_step_*: kkt_resolve with g := gta, c := nglam (warm start from alam, writing alam and az), then
        admm_adjoint_update, one call.  Returns (iters, flags, res [batch, 2])."""
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=gz.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=gz.device)
        if res is None:
            res = torch.empty(batch, 2, dtype=gz.dtype, device=gz.device)
        suf, args, _ = self._adjoint_step_args(nx, nu, N, batch, Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma, alam, r, p, tol, max_iter,
                                               iters, max_iter_exit, az, wa, ya, gta, res)
        self._check(getattr(self.lib, f"gbdpcg_admm_adjoint_step_{suf}")(*args, self._stream(stream)), "admm_adjoint_step")
        return iters, max_iter_exit, res.view(batch, 2)

    def graph_admm_adjoint_step(self, nx, nu, N, batch, Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma, alam, r, p, tol, max_iter, iters,
                                max_iter_exit, az, wa, ya, gta, res):
        """Capture one adjoint iteration into a hipGraph (gbdpcg_graph_create_admm_adjoint_step_*): replay it once per iteration;
        the graph keeps rho's pointer."""
        suf, args, keep = self._adjoint_step_args(nx, nu, N, batch, Ginv, C, gz, nglam, yf, rho, S, Pinv, gamma, alam, r, p, tol,
                                                  max_iter, iters, max_iter_exit, az, wa, ya, gta, res)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_admm_adjoint_step_{suf}")(*args, ctypes.byref(gr)),
                    "graph_create_admm_adjoint_step")
        return Graph(self, gr, keep=keep)

    def admm_grad_bounds(self, nx, nu, N, batch, yf, rho, ya, glo=None, ghi=None, stream=None):
        """gbdpcg_admm_grad_bounds_*: (dl/dlo, dl/dhi) = -rho ya where yf < 0 / yf > 0, +0 elsewhere, in the layout of g."""
        import torch
        suf, _ = _suffix(yf)
        if glo is None:
            glo = torch.empty_like(yf)
        if ghi is None:
            ghi = torch.empty_like(yf)
        self._box(yf, batch, ya, glo, ghi)
        fn = getattr(self.lib, f"gbdpcg_admm_grad_bounds_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(yf), _p(self._rho(rho, batch, yf)), _p(ya), _p(glo), _p(ghi), self._stream(stream)),
                    "admm_grad_bounds")
        return glo, ghi

    # ---- the backward pass of the hard linear-row QP (include/gbdpcg.h): the admm_lin family with yf, the forward y, where lo, hi
    # stand; gz = dl/dz in the place of g, nglam = -dl/dlambda in the place of c; wa, ya (layout of the rows), gta, az (layout of g)
    def admm_lin_adjoint_init(self, nx, nu, mx, mu, N, batch, gz, E, yf, rho, wa, ya, gta=None, stream=None):
        """gbdpcg_admm_lin_adjoint_init_*: wa <- 0 where yf != 0, gta <- gz - rho E'(wa - ya); ya is left alone.  Returns gta."""
        import torch
        suf, _ = _suffix(gz)
        if gta is None:
            gta = torch.empty_like(gz)
        self._lin(gz, batch, nx, nu, mx, mu, N, E, (yf, wa, ya), (gz, gta))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_adjoint_init_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(gz), _p(E), _p(yf), _p(self._rho(rho, batch, gz)), _p(wa), _p(ya), _p(gta),
                       self._stream(stream)), "admm_lin_adjoint_init")
        return gta

    def admm_lin_adjoint_update(self, nx, nu, mx, mu, N, batch, gz, E, yf, rho, az, wa, ya, gta, res=None, stream=None):
        """gbdpcg_admm_lin_adjoint_update_*: the update behind an adjoint solve that wrote az -- wa, ya, gta in place; returns the
        [batch, 2] tensor of (||E az - wa||_inf, rho ||E'(wa - wa_old)||_inf) per problem."""
        import torch
        suf, _ = _suffix(gz)
        if res is None:
            res = torch.empty(batch, 2, dtype=gz.dtype, device=gz.device)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == gz.dtype
        self._lin(gz, batch, nx, nu, mx, mu, N, E, (yf, wa, ya), (gz, az, gta))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_adjoint_update_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(gz), _p(E), _p(yf), _p(self._rho(rho, batch, gz)), _p(az), _p(wa), _p(ya),
                       _p(gta), _p(res), self._stream(stream)), "admm_lin_adjoint_update")
        return res.view(batch, 2)

    def _lin_adjoint_step_args(self, nx, nu, mx, mu, N, batch, Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, r, p, tol, max_iter,
                               iters, mie, az, wa, ya, gta, res):
        suf, _ = _suffix(gz)
        assert res.is_cuda and res.is_contiguous() and res.numel() == 2 * batch and res.dtype == gz.dtype
        self._lin(gz, batch, nx, nu, mx, mu, N, E, (yf, wa, ya), (gz, az, gta))
        args = (self.h, nx, nu, mx, mu, N, batch, _p(Ginv), _p(C), _p(gz), _p(nglam), _p(E), _p(yf), _p(self._rho(rho, batch, gz)),
                _p(S), _p(Pinv), _p(gamma), _p(alam), _p(r), _p(p), tol, max_iter, _p(iters), _p(mie), _p(az), _p(wa), _p(ya), _p(gta),
                _p(res))
        return suf, args, (Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, r, p, iters, mie, az, wa, ya, gta, res)

    def admm_lin_adjoint_step(self, nx, nu, mx, mu, N, batch, Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, az, wa, ya, gta,
                              res=None, r=None, p=None, tol=1e-6, max_iter=25, iters=None, max_iter_exit=None, stream=None):
        """gbdpcg_admm_lin_adjoint_step_*: kkt_resolve with g := gta, c := nglam (warm start from alam, writing alam and az), then
        admm_lin_adjoint_update, one call.  Returns (iters, flags, res [batch, 2])."""
        import torch
        if iters is None:
            iters = torch.zeros(batch, dtype=torch.int32, device=gz.device)
        if max_iter_exit is None:
            max_iter_exit = torch.zeros(batch, dtype=torch.uint8, device=gz.device)
        if res is None:
            res = torch.empty(batch, 2, dtype=gz.dtype, device=gz.device)
        suf, args, _ = self._lin_adjoint_step_args(nx, nu, mx, mu, N, batch, Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, r, p,
                                                   tol, max_iter, iters, max_iter_exit, az, wa, ya, gta, res)
        self._check(getattr(self.lib, f"gbdpcg_admm_lin_adjoint_step_{suf}")(*args, self._stream(stream)), "admm_lin_adjoint_step")
        return iters, max_iter_exit, res.view(batch, 2)

    def graph_admm_lin_adjoint_step(self, nx, nu, mx, mu, N, batch, Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, r, p, tol,
                                    max_iter, iters, max_iter_exit, az, wa, ya, gta, res):
        """Capture one adjoint iteration of the rows into a hipGraph (gbdpcg_graph_create_admm_lin_adjoint_step_*): replay it once
        per iteration; the graph keeps rho's pointer."""
        suf, args, keep = self._lin_adjoint_step_args(nx, nu, mx, mu, N, batch, Ginv, C, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, r,
                                                      p, tol, max_iter, iters, max_iter_exit, az, wa, ya, gta, res)
        gr = ctypes.c_void_p()
        self._check(getattr(self.lib, f"gbdpcg_graph_create_admm_lin_adjoint_step_{suf}")(*args, ctypes.byref(gr)),
                    "graph_create_admm_lin_adjoint_step")
        return Graph(self, gr, keep=keep)

    def admm_lin_grad(self, nx, nu, mx, mu, N, batch, z, az, yf, ya, rho, glo=None, ghi=None, gE=None, want="lhE", stream=None):
        """gbdpcg_admm_lin_grad_*: (dl/dlo, dl/dhi) in the layout of the rows and dl/dE in the layout of E from the forward z, yf
        and the adjoint's az, ya.  want: which of "l", "h", "E" to allocate when the tensor is not passed (the others stay NULL)."""
        import torch
        suf, _ = _suffix(z)
        _, nw, ne, _ = self._lin_sizes(nx, nu, mx, mu, N)
        kw = dict(dtype=z.dtype, device=z.device)
        if glo is None and "l" in want:
            glo = torch.empty(batch * nw, **kw)
        if ghi is None and "h" in want:
            ghi = torch.empty(batch * nw, **kw)
        if gE is None and "E" in want:
            gE = torch.empty(batch * ne, **kw)
        nz = (nx + nu) * N - nu
        for t, cnt in ((z, nz), (az, nz), (yf, nw), (ya, nw), (glo, nw), (ghi, nw), (gE, ne)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() == batch * cnt and t.dtype == z.dtype)
        assert None not in (az, yf, ya) and (glo is not None or ghi is not None or gE is not None)
        fn = getattr(self.lib, f"gbdpcg_admm_lin_grad_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(z), _p(az), _p(yf), _p(ya), _p(self._rho(rho, batch, z)), _p(glo), _p(ghi),
                       _p(gE), self._stream(stream)), "admm_lin_grad")
        return glo, ghi, gE

    # ---- the primal infeasibility certificate of the hard paths (include/gbdpcg.h): two iterates (lam0, y0), (lam1, y1) of the
    # splitting in, per problem the scale n, the residual r, the support value sigma and the flag out
    def _infeas(self, name, nx, nu, mx, mu, N, batch, C, c, E, lo, hi, rho, lam0, lam1, y0, y1, eps, cert, flag, want_flag, stream):
        import torch
        suf, _ = _suffix(c)
        box, mats = "lin" not in name, 1 if name.endswith("shared") else batch
        nw = (nx + nu) * N - nu if box else self._lin_sizes(nx, nu, mx, mu, N)[1]
        ne = 0 if box else self._lin_sizes(nx, nu, mx, mu, N)[2]
        if cert is None:
            cert = torch.empty(batch, 3, dtype=c.dtype, device=c.device)
        if flag is None and want_flag:
            flag = torch.empty(batch, dtype=torch.uint8, device=c.device)
        for t, cnt in ((c, batch * nx * N), (lam0, batch * nx * N), (lam1, batch * nx * N), (lo, batch * nw), (hi, batch * nw),
                       (y0, batch * nw), (y1, batch * nw), (cert, 3 * batch)) + (() if box else ((E, mats * ne),)):
            assert t is not None and t.is_cuda and t.is_contiguous() and t.numel() == cnt and t.dtype == c.dtype
        assert (C is None and N == 1) or (C.is_cuda and C.is_contiguous() and C.dtype == c.dtype and
                                          C.numel() == mats * nx * (nx + nu) * (N - 1))
        assert flag is None or (flag.is_cuda and flag.is_contiguous() and flag.numel() == batch and flag.dtype == torch.uint8)
        fn = getattr(self.lib, f"gbdpcg_{name}_{suf}")
        head = (self.h, nx, nu, N, batch, _p(C), _p(c)) if box else (self.h, nx, nu, mx, mu, N, batch, _p(C), _p(c), _p(E))
        self._check(fn(*head, _p(lo), _p(hi), _p(self._rho(rho, batch, c)), _p(lam0), _p(lam1), _p(y0), _p(y1), eps, _p(cert),
                       _p(flag), self._stream(stream)), name)
        return cert.view(batch, 3), flag

    def admm_infeas(self, nx, nu, N, batch, C, c, lo, hi, rho, lam0, lam1, y0, y1, eps, cert=None, flag=None, want_flag=True,
                    stream=None):
        """gbdpcg_admm_infeas_*: (cert [batch, 3] = (n, r, sigma), flag [batch] uint8) of the hard box from two iterates of
        gbdpcg_admm_step_*; flag = n > 0 and r <= eps n and sigma < -eps n.  want_flag=False passes NULL for the flag."""
        return self._infeas("admm_infeas", nx, nu, 0, 0, N, batch, C, c, None, lo, hi, rho, lam0, lam1, y0, y1, eps, cert, flag,
                            want_flag, stream)

    def admm_infeas_shared(self, nx, nu, N, batch, C, c, lo, hi, rho, lam0, lam1, y0, y1, eps, cert=None, flag=None, want_flag=True,
                           stream=None):
        """gbdpcg_admm_infeas_shared_*: one problem's C, `batch` of everything else."""
        return self._infeas("admm_infeas_shared", nx, nu, 0, 0, N, batch, C, c, None, lo, hi, rho, lam0, lam1, y0, y1, eps, cert, flag,
                            want_flag, stream)

    def admm_lin_infeas(self, nx, nu, mx, mu, N, batch, C, c, E, lo, hi, rho, lam0, lam1, y0, y1, eps, cert=None, flag=None,
                        want_flag=True, stream=None):
        """gbdpcg_admm_lin_infeas_*: the certificate of the hard linear rows lo <= E z <= hi from two iterates of
        gbdpcg_admm_lin_step_*."""
        return self._infeas("admm_lin_infeas", nx, nu, mx, mu, N, batch, C, c, E, lo, hi, rho, lam0, lam1, y0, y1, eps, cert, flag,
                            want_flag, stream)

    def admm_lin_infeas_shared(self, nx, nu, mx, mu, N, batch, C, c, E, lo, hi, rho, lam0, lam1, y0, y1, eps, cert=None, flag=None,
                               want_flag=True, stream=None):
        """gbdpcg_admm_lin_infeas_shared_*: one problem's C and E, `batch` of everything else."""
        return self._infeas("admm_lin_infeas_shared", nx, nu, mx, mu, N, batch, C, c, E, lo, hi, rho, lam0, lam1, y0, y1, eps, cert,
                            flag, want_flag, stream)

    # ---- the optimality test of every ADMM family (include/gbdpcg.h): the point (z, lam, w, y) in, per problem the residuals of
    # stationarity (with the row multiplier rho y), dynamics and consensus, their scales and the flag out.  G is the Hessian.
    def _optimality(self, name, nx, nu, mx, mu, N, batch, G, C, g, c, E, rho, z, lam, w, y, eps_abs, eps_rel, opt, done, want_done,
                    stream):
        import torch
        suf, _ = _suffix(g)
        box, mats = "lin" not in name, 1 if name.endswith("shared") else batch
        nz = (nx + nu) * N - nu
        nw = nz if box else self._lin_sizes(nx, nu, mx, mu, N)[1]
        ne = 0 if box else self._lin_sizes(nx, nu, mx, mu, N)[2]
        if opt is None:
            opt = torch.empty(batch, 6, dtype=g.dtype, device=g.device)
        if done is None and want_done:
            done = torch.empty(batch, dtype=torch.uint8, device=g.device)
        for t, cnt in ((G, mats * ((nx * nx + nu * nu) * N - nu * nu)), (g, batch * nz), (z, batch * nz), (c, batch * nx * N),
                       (lam, batch * nx * N), (w, batch * nw), (y, batch * nw), (opt, 6 * batch)) + (() if box else ((E, mats * ne),)):
            assert t is not None and t.is_cuda and t.is_contiguous() and t.numel() == cnt and t.dtype == g.dtype
        assert (C is None and N == 1) or (C.is_cuda and C.is_contiguous() and C.dtype == g.dtype and
                                          C.numel() == mats * nx * (nx + nu) * (N - 1))
        assert done is None or (done.is_cuda and done.is_contiguous() and done.numel() == batch and done.dtype == torch.uint8)
        fn = getattr(self.lib, f"gbdpcg_{name}_{suf}")
        head = (self.h, nx, nu, N, batch) if box else (self.h, nx, nu, mx, mu, N, batch)
        mid = (_p(G), _p(C), _p(g), _p(c)) + (() if box else (_p(E),))
        self._check(fn(*head, *mid, _p(self._rho(rho, batch, g)), _p(z), _p(lam), _p(w), _p(y), eps_abs, eps_rel, _p(opt), _p(done),
                       self._stream(stream)), name)
        return opt.view(batch, 6), done

    def admm_optimality(self, nx, nu, N, batch, G, C, g, c, rho, z, lam, w, y, eps_abs, eps_rel, opt=None, done=None, want_done=True,
                        stream=None):
        """gbdpcg_admm_optimality_*: (opt [batch, 6] = (r_s, r_e, r_r, n_s, n_e, n_r), done [batch] uint8) of the box families (hard
        and soft) at (z, lam, w, y); done = every r <= eps_abs + eps_rel n.  want_done=False passes NULL for done."""
        return self._optimality("admm_optimality", nx, nu, 0, 0, N, batch, G, C, g, c, None, rho, z, lam, w, y, eps_abs, eps_rel, opt,
                                done, want_done, stream)

    def admm_optimality_shared(self, nx, nu, N, batch, G, C, g, c, rho, z, lam, w, y, eps_abs, eps_rel, opt=None, done=None,
                               want_done=True, stream=None):
        """gbdpcg_admm_optimality_shared_*: one problem's G and C, `batch` of everything else."""
        return self._optimality("admm_optimality_shared", nx, nu, 0, 0, N, batch, G, C, g, c, None, rho, z, lam, w, y, eps_abs, eps_rel,
                                opt, done, want_done, stream)

    def admm_lin_optimality(self, nx, nu, mx, mu, N, batch, G, C, g, c, E, rho, z, lam, w, y, eps_abs, eps_rel, opt=None, done=None,
                            want_done=True, stream=None):
        """gbdpcg_admm_lin_optimality_*: the test of the rows families (linear, soft, cones) at (z, lam, w, y)."""
        return self._optimality("admm_lin_optimality", nx, nu, mx, mu, N, batch, G, C, g, c, E, rho, z, lam, w, y, eps_abs, eps_rel,
                                opt, done, want_done, stream)

    def admm_lin_optimality_shared(self, nx, nu, mx, mu, N, batch, G, C, g, c, E, rho, z, lam, w, y, eps_abs, eps_rel, opt=None,
                                   done=None, want_done=True, stream=None):
        """gbdpcg_admm_lin_optimality_shared_*: one problem's G, C and E, `batch` of everything else."""
        return self._optimality("admm_lin_optimality_shared", nx, nu, mx, mu, N, batch, G, C, g, c, E, rho, z, lam, w, y, eps_abs,
                                eps_rel, opt, done, want_done, stream)

    # ---- the backward pass of the soft box and rows QPs (include/gbdpcg.h): the forward y splits the rows into free, held and
    # saturated; the mask turns it into the yf of the hard adjoint methods above, the gradient launches know of kappa
    def admm_soft_mask(self, nx, nu, N, batch, yf, kappa, rho, ym=None, stream=None):
        """gbdpcg_admm_soft_mask_*: ym = |yf| >= kappa / rho ? +0 : yf in the layout of g.  rho is the rho of the update that wrote
        yf.  Returns ym (never yf itself)."""
        import torch
        suf, _ = _suffix(yf)
        if ym is None:
            ym = torch.empty_like(yf)
        self._box(yf, batch, kappa, ym)
        fn = getattr(self.lib, f"gbdpcg_admm_soft_mask_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(yf), _p(kappa), _p(self._rho(rho, batch, yf)), _p(ym), self._stream(stream)),
                    "admm_soft_mask")
        return ym

    def admm_lin_soft_mask(self, nx, nu, mx, mu, N, batch, yf, kappa, rho, ym=None, stream=None):
        """gbdpcg_admm_lin_soft_mask_*: the mask in the layout of the rows."""
        import torch
        suf, _ = _suffix(yf)
        if ym is None:
            ym = torch.empty_like(yf)
        _, nw, _, _ = self._lin_sizes(nx, nu, mx, mu, N)
        for t in (yf, kappa, ym):
            assert t.is_cuda and t.is_contiguous() and t.numel() == batch * nw and t.dtype == yf.dtype
        fn = getattr(self.lib, f"gbdpcg_admm_lin_soft_mask_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(yf), _p(kappa), _p(self._rho(rho, batch, yf)), _p(ym),
                       self._stream(stream)), "admm_lin_soft_mask")
        return ym

    def admm_soft_grad_bounds(self, nx, nu, N, batch, yf, kappa, rho, ya, az, glo=None, ghi=None, gkappa=None, want="lhk", stream=None):
        """gbdpcg_admm_soft_grad_bounds_*: (dl/dlo, dl/dhi, dl/dkappa) of the soft box from the UNMASKED yf, kappa and the adjoint's ya,
        az.  want: which of "l", "h", "k" to allocate when the tensor is not passed (the others stay NULL)."""
        import torch
        suf, _ = _suffix(yf)
        if glo is None and "l" in want:
            glo = torch.empty_like(yf)
        if ghi is None and "h" in want:
            ghi = torch.empty_like(yf)
        if gkappa is None and "k" in want:
            gkappa = torch.empty_like(yf)
        self._box(yf, batch, kappa, ya, az, *[t for t in (glo, ghi, gkappa) if t is not None])
        assert glo is not None or ghi is not None or gkappa is not None
        fn = getattr(self.lib, f"gbdpcg_admm_soft_grad_bounds_{suf}")
        self._check(fn(self.h, nx, nu, N, batch, _p(yf), _p(kappa), _p(self._rho(rho, batch, yf)), _p(ya), _p(az), _p(glo), _p(ghi),
                       _p(gkappa), self._stream(stream)), "admm_soft_grad_bounds")
        return glo, ghi, gkappa

    def admm_lin_soft_grad(self, nx, nu, mx, mu, N, batch, z, az, E, yf, ya, kappa, rho, glo=None, ghi=None, gkappa=None, gE=None,
                           want="lhkE", stream=None):
        """gbdpcg_admm_lin_soft_grad_*: (dl/dlo, dl/dhi, dl/dkappa) in the layout of the rows and dl/dE in the layout of E from the
        forward z, the UNMASKED yf, kappa and the adjoint's az, ya.  want: which of "l", "h", "k", "E" to allocate when the tensor is
        not passed (the others stay NULL)."""
        import torch
        suf, _ = _suffix(z)
        _, nw, ne, _ = self._lin_sizes(nx, nu, mx, mu, N)
        kw = dict(dtype=z.dtype, device=z.device)
        if glo is None and "l" in want:
            glo = torch.empty(batch * nw, **kw)
        if ghi is None and "h" in want:
            ghi = torch.empty(batch * nw, **kw)
        if gkappa is None and "k" in want:
            gkappa = torch.empty(batch * nw, **kw)
        if gE is None and "E" in want:
            gE = torch.empty(batch * ne, **kw)
        nz = (nx + nu) * N - nu
        for t, cnt in ((z, nz), (az, nz), (E, ne), (yf, nw), (ya, nw), (kappa, nw), (glo, nw), (ghi, nw), (gkappa, nw), (gE, ne)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() == batch * cnt and t.dtype == z.dtype)
        assert None not in (az, E, yf, ya, kappa) and any(t is not None for t in (glo, ghi, gkappa, gE))
        fn = getattr(self.lib, f"gbdpcg_admm_lin_soft_grad_{suf}")
        self._check(fn(self.h, nx, nu, mx, mu, N, batch, _p(z), _p(az), _p(E), _p(yf), _p(ya), _p(kappa), _p(self._rho(rho, batch, z)),
                       _p(glo), _p(ghi), _p(gkappa), _p(gE), self._stream(stream)), "admm_lin_soft_grad")
        return glo, ghi, gkappa, gE

    # ---- mixed-precision refinement: fp64 problem data and point, fp32 solves on a kept fp32 factorisation (include/gbdpcg.h)
    def demote(self, src, dst=None, stream=None):
        """gbdpcg_demote_f32: the fp64 tensor rounded to fp32 (to nearest), on the device."""
        import torch
        assert src.is_cuda and src.is_contiguous() and src.dtype == torch.float64
        if dst is None:
            dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
        assert dst.is_cuda and dst.is_contiguous() and dst.dtype == torch.float32 and dst.numel() == src.numel()
        self._check(self.lib.gbdpcg_demote_f32(self.h, src.numel(), _p(src), _p(dst), self._stream(stream)), "demote")
        return dst

    @staticmethod
    def _refine_check(nx, nu, N, batch, f64=(), f32_g=(), f32_c=(), expo=None, res=None):
        import torch
        nz, nl = (nx + nu) * N - nu, nx * N
        for t in f64:
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float64)
        for ts, cnt in ((f32_g, nz), (f32_c, nl)):
            for t in ts:
                assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == batch * cnt)
        assert expo is None or (expo.is_cuda and expo.is_contiguous() and expo.dtype == torch.int32 and expo.numel() == batch)
        assert res is None or (res.is_cuda and res.is_contiguous() and res.dtype == torch.float64 and res.numel() == 2 * batch)

    @staticmethod
    def _rho_args(batch, rho, reg):
        """The arguments that stand directly behind c: rho ([batch], fp64) in the _reg forms, nothing otherwise."""
        import torch
        if not reg:
            return ()
        assert rho is None or (rho.is_cuda and rho.is_contiguous() and rho.dtype == torch.float64 and rho.numel() == batch)
        return (_p(rho),)

    def kkt_defect_mixed(self, nx, nu, N, batch, G, C, g, c, z, lam, rg=None, rc=None, dlam=None, expo=None, res=None, stream=None,
                         zero_dlam=True):
        """gbdpcg_kkt_defect_mixed: the fp64 defect of (z, lam) as the scaled fp32 right-hand side of the correction system.
        Returns (rg, rc, dlam, expo, res [batch, 2]); zero_dlam=False passes NULL for dlam."""
        return self._kkt_defect_mixed("kkt_defect_mixed", nx, nu, N, batch, G, C, g, c, None, False, z, lam, rg, rc, dlam, expo, res,
                                      stream, zero_dlam)

    def kkt_defect_mixed_reg(self, nx, nu, N, batch, G, C, g, c, rho, z, lam, rg=None, rc=None, dlam=None, expo=None, res=None,
                             stream=None, zero_dlam=True):
        """gbdpcg_kkt_defect_mixed_reg: the defect of (G_b + rho_b I) z + g + C' lam; rho [batch], fp64, on the device."""
        return self._kkt_defect_mixed("kkt_defect_mixed_reg", nx, nu, N, batch, G, C, g, c, rho, True, z, lam, rg, rc, dlam, expo, res,
                                      stream, zero_dlam)

    def kkt_defect_mixed_shared(self, nx, nu, N, batch, G, C, g, c, z, lam, rg=None, rc=None, dlam=None, expo=None, res=None,
                                stream=None, zero_dlam=True):
        """gbdpcg_kkt_defect_mixed_shared: ONE problem's G and C for the whole batch; everything else per problem."""
        return self._kkt_defect_mixed("kkt_defect_mixed_shared", nx, nu, N, batch, G, C, g, c, None, False, z, lam, rg, rc, dlam, expo,
                                      res, stream, zero_dlam)

    def _kkt_defect_mixed(self, name, nx, nu, N, batch, G, C, g, c, rho, reg, z, lam, rg, rc, dlam, expo, res, stream, zero_dlam):
        import torch
        if rg is None:
            rg = torch.empty(batch * ((nx + nu) * N - nu), dtype=torch.float32, device=G.device)
        if rc is None:
            rc = torch.empty(batch * nx * N, dtype=torch.float32, device=G.device)
        if dlam is None and zero_dlam:
            dlam = torch.empty(batch * nx * N, dtype=torch.float32, device=G.device)
        if expo is None:
            expo = torch.empty(batch, dtype=torch.int32, device=G.device)
        if res is None:
            res = torch.empty(batch, 2, dtype=torch.float64, device=G.device)
        self._refine_check(nx, nu, N, batch, (G, C, g, c, z, lam), (rg,), (rc, dlam), expo, res)
        fn = getattr(self.lib, "gbdpcg_" + name)
        self._check(fn(self.h, nx, nu, N, batch, _p(G), _p(C), _p(g), _p(c), *self._rho_args(batch, rho, reg), _p(z), _p(lam), _p(rg),
                       _p(rc), _p(dlam), _p(expo), _p(res), self._stream(stream)), name)
        return rg, rc, dlam, expo, res.view(batch, 2)

    def kkt_refine_apply(self, nx, nu, N, batch, dz, dlam, expo, z, lam, stream=None):
        """gbdpcg_kkt_refine_apply: z += ldexp(dz, -e_b), lam += ldexp(dlam, -e_b) in fp64, in place."""
        self._refine_check(nx, nu, N, batch, (z, lam), (dz,), (dlam,), expo)
        self._check(self.lib.gbdpcg_kkt_refine_apply(self.h, nx, nu, N, batch, _p(dz), _p(dlam), _p(expo), _p(z), _p(lam),
                                                     self._stream(stream)), "kkt_refine_apply")
        return z, lam

    def _refine_step_args(self, nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol, max_iter,
                          iters, mie, expo, z, lam, res, rho=None, reg=False):
        self._refine_check(nx, nu, N, batch, (G, C, g, c, z, lam), (rg, dz), (rc, gamma, dlam, r, p), expo, res)
        return (self.h, nx, nu, N, batch, _p(G), _p(C), _p(g), _p(c), *self._rho_args(batch, rho, reg), _p(Ginv32), _p(C32), _p(S32),
                _p(Pinv32), _p(rg), _p(rc),
                _p(gamma), _p(dlam), _p(r), _p(p), _p(dz), tol, max_iter, _p(iters), _p(mie), _p(expo), _p(z), _p(lam), _p(res))

    def refine_work(self, nx, nu, N, batch, device="cuda"):
        """The fp32 work arrays and status words of a refinement step, as a dict of the keyword arguments of kkt_refine_step."""
        import torch
        nz, nl = batch * ((nx + nu) * N - nu), batch * nx * N
        f = dict(dtype=torch.float32, device=device)
        return dict(rg=torch.empty(nz, **f), rc=torch.empty(nl, **f), gamma=torch.empty(nl, **f), dlam=torch.empty(nl, **f),
                    r=torch.empty(nl, **f), p=torch.empty(nl, **f), dz=torch.empty(nz, **f),
                    iters=torch.zeros(batch, dtype=torch.int32, device=device),
                    max_iter_exit=torch.zeros(batch, dtype=torch.uint8, device=device),
                    expo=torch.empty(batch, dtype=torch.int32, device=device),
                    res=torch.empty(batch, 2, dtype=torch.float64, device=device))

    def kkt_refine_step(self, nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, z, lam, *, rg, rc, gamma, dlam, r, p, dz, iters,
                        max_iter_exit, expo, res, tol=1e-4, max_iter=50, stream=None):
        """gbdpcg_kkt_refine_step: defect of (z, lam) -> fp32 correction solve on the kept factorisation -> fp64 accumulation.
        res [batch, 2] holds the norms of the point the step started from.  The work arrays: refine_work()."""
        args = self._refine_step_args(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol,
                                      max_iter, iters, max_iter_exit, expo, z, lam, res)
        self._check(self.lib.gbdpcg_kkt_refine_step(*args, self._stream(stream)), "kkt_refine_step")
        return res.view(batch, 2)

    def graph_kkt_refine_step(self, nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, z, lam, *, rg, rc, gamma, dlam, r, p, dz,
                              iters, max_iter_exit, expo, res, tol=1e-4, max_iter=50):
        """Capture one refinement step into a hipGraph (gbdpcg_graph_create_kkt_refine_step)."""
        args = self._refine_step_args(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol,
                                      max_iter, iters, max_iter_exit, expo, z, lam, res)
        gr = ctypes.c_void_p()
        self._check(self.lib.gbdpcg_graph_create_kkt_refine_step(*args, ctypes.byref(gr)), "graph_create_kkt_refine_step")
        return Graph(self, gr, keep=(G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, iters, max_iter_exit, expo,
                                     z, lam, res))

    def kkt_refine_step_reg(self, nx, nu, N, batch, G, C, g, c, rho, Ginv32, C32, S32, Pinv32, z, lam, *, rg, rc, gamma, dlam, r, p, dz,
                            iters, max_iter_exit, expo, res, tol=1e-4, max_iter=50, stream=None):
        """gbdpcg_kkt_refine_step_reg: the step towards the solution of the system with G_b + rho_b I; the kept factorisation is
        that of kkt_step_reg (fp32) with the demoted rho."""
        args = self._refine_step_args(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol,
                                      max_iter, iters, max_iter_exit, expo, z, lam, res, rho, True)
        self._check(self.lib.gbdpcg_kkt_refine_step_reg(*args, self._stream(stream)), "kkt_refine_step_reg")
        return res.view(batch, 2)

    def kkt_refine_step_shared(self, nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, z, lam, *, rg, rc, gamma, dlam, r, p, dz,
                               iters, max_iter_exit, expo, res, tol=1e-4, max_iter=50, stream=None):
        """gbdpcg_kkt_refine_step_shared: ONE G, C, Ginv32, C32, S32, Pinv32 for the whole batch (the solve: kkt_resolve_shared)."""
        args = self._refine_step_args(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol,
                                      max_iter, iters, max_iter_exit, expo, z, lam, res)
        self._check(self.lib.gbdpcg_kkt_refine_step_shared(*args, self._stream(stream)), "kkt_refine_step_shared")
        return res.view(batch, 2)

    def graph_kkt_refine_step_reg(self, nx, nu, N, batch, G, C, g, c, rho, Ginv32, C32, S32, Pinv32, z, lam, *, rg, rc, gamma, dlam, r,
                                  p, dz, iters, max_iter_exit, expo, res, tol=1e-4, max_iter=50):
        """Capture one regularised refinement step into a hipGraph (gbdpcg_graph_create_kkt_refine_step_reg); the graph keeps the
        pointer of rho: rewrite it in place between replays."""
        args = self._refine_step_args(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol,
                                      max_iter, iters, max_iter_exit, expo, z, lam, res, rho, True)
        gr = ctypes.c_void_p()
        self._check(self.lib.gbdpcg_graph_create_kkt_refine_step_reg(*args, ctypes.byref(gr)), "graph_create_kkt_refine_step_reg")
        return Graph(self, gr, keep=(G, C, g, c, rho, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, iters, max_iter_exit,
                                     expo, z, lam, res))

    def graph_kkt_refine_step_shared(self, nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, z, lam, *, rg, rc, gamma, dlam, r,
                                     p, dz, iters, max_iter_exit, expo, res, tol=1e-4, max_iter=50):
        """Capture one shared-matrix refinement step into a hipGraph (gbdpcg_graph_create_kkt_refine_step_shared)."""
        args = self._refine_step_args(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, tol,
                                      max_iter, iters, max_iter_exit, expo, z, lam, res)
        gr = ctypes.c_void_p()
        self._check(self.lib.gbdpcg_graph_create_kkt_refine_step_shared(*args, ctypes.byref(gr)),
                    "graph_create_kkt_refine_step_shared")
        return Graph(self, gr, keep=(G, C, g, c, Ginv32, C32, S32, Pinv32, rg, rc, gamma, dlam, r, p, dz, iters, max_iter_exit, expo,
                                     z, lam, res))

    def kkt_solve_refined(self, nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, z=None, lam=None, max_steps=12, stop_s=0.0,
                          stop_f=0.0, tol=1e-4, max_iter=50, work=None, rho=None, shared=False):
        """Replay the refinement step from (z, lam) (zeros when not given) until every problem has stationarity <= stop_s and
        feasibility <= stop_f (scalars or [batch] arrays) or max_steps steps have run; res is read back between steps.
        rho ([batch], fp64): the _reg step, on the system with G_b + rho_b I; shared: the _shared step, one problem's matrices.
        Both together are refused, as by the library (write G + rho I into the one G).
        Returns (z, lam, history): history[i] is the [batch, 2] numpy array of the norms of the point step i started from; when
        the loop stops on the norms, the last entry belongs to the point in front of the last step."""
        import torch
        if z is None:
            z = torch.zeros(batch * ((nx + nu) * N - nu), dtype=torch.float64, device=G.device)
        if lam is None:
            lam = torch.zeros(batch * nx * N, dtype=torch.float64, device=G.device)
        work = work or self.refine_work(nx, nu, N, batch, G.device)
        if rho is not None and shared:
            raise ValueError("kkt_solve_refined: rho and shared together are not provided")
        if rho is not None:
            graph = self.graph_kkt_refine_step_reg(nx, nu, N, batch, G, C, g, c, rho, Ginv32, C32, S32, Pinv32, z, lam, tol=tol,
                                                   max_iter=max_iter, **work)
        else:
            make = self.graph_kkt_refine_step_shared if shared else self.graph_kkt_refine_step
            graph = make(nx, nu, N, batch, G, C, g, c, Ginv32, C32, S32, Pinv32, z, lam, tol=tol, max_iter=max_iter, **work)
        history = []
        try:
            for _ in range(max_steps):
                graph.launch()
                torch.cuda.current_stream().synchronize()
                res = work["res"].view(batch, 2).cpu().numpy().copy()
                history.append(res)
                if (res[:, 0] <= stop_s).all() and (res[:, 1] <= stop_f).all():
                    break   # (the step just replayed has refined the point that passed once more)
        finally:
            graph.close()
        return z, lam, history


class Graph:
    def __init__(self, solver, g, keep):
        self.solver, self.g, self.keep = solver, g, keep

    def launch(self, stream=None):
        self.solver._check(self.solver.lib.gbdpcg_graph_launch(self.g, Solver._stream(stream)),
                           "graph_launch")

    def close(self):
        if self.g:
            self.solver.lib.gbdpcg_graph_destroy(self.g)
            self.g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_to_bt(n, N, row_ptr, col_ind, val):
    """gbdpcg_csr_to_bt_* on numpy arrays -> flat [L|D|R] array.  Host-only, no GPU needed."""
    import numpy as np
    lib = load()
    suf = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[val.dtype]
    row_ptr = np.ascontiguousarray(row_ptr, np.uint32)
    col_ind = np.ascontiguousarray(col_ind, np.uint32)
    val = np.ascontiguousarray(val)
    M = np.empty(3 * n * n * N, val.dtype)
    st = getattr(lib, f"gbdpcg_csr_to_bt_{suf}")(
        ctypes.c_uint32(n), ctypes.c_uint32(N), row_ptr.ctypes.data_as(ctypes.c_void_p),
        col_ind.ctypes.data_as(ctypes.c_void_p), val.ctypes.data_as(ctypes.c_void_p),
        M.ctypes.data_as(ctypes.c_void_p))
    if st != OK:
        raise GbdPcgError(f"csr_to_bt: {lib.gbdpcg_status_string(st).decode()}")
    return M
