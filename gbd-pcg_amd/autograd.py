"""torch.autograd through the batched KKT solve: (G, C, g, c[, rho]) -> (z, lambda) with gradients from the device backward pass.

Plumbing over binding.Solver: the forward pass is gbdpcg_kkt_step_* (gbdpcg_kkt_step_reg_* when rho is given; for a shared-matrix
batch gbdpcg_kkt_step_* at batch 1 followed by gbdpcg_kkt_resolve_shared_*), the backward pass is gbdpcg_kkt_backward_* on the S,
Phi^-1 and G^-1 the forward pass left behind -- one adjoint solve and one gradient launch (include/gbdpcg.h has the formulas); for a
shared-matrix batch the two are gbdpcg_kkt_resolve_shared_* and gbdpcg_kkt_grad_shared_*, with the adjoint pairs of problems outside
the loss zeroed in between.  Nothing here computes a gradient in torch except dl/drho = a_z' z, one dot product per problem, and the
selects that give problems with zero cotangents zero gradients.  There is no CPU path.

box_qp_solve adds the hard box lo <= z <= hi: the forward pass is gbdpcg_kkt_step_reg_* followed by a fixed number of
gbdpcg_admm_step_*, the backward pass the same ADMM iteration on the adjoint QP (gbdpcg_admm_adjoint_*: the forward y is the mask of
the active set), gbdpcg_admm_grad_bounds_* and gbdpcg_kkt_grad_*; (G, C, g, c, lo, hi) -> (w, lambda).

lin_qp_solve adds the stage-wise linear rows lo <= E z <= hi: the forward pass is gbdpcg_admm_lin_form_* into a private Gt,
gbdpcg_kkt_step_* on it and a fixed number of gbdpcg_admm_lin_step_*, the backward pass the same iteration on the adjoint QP
(gbdpcg_admm_lin_adjoint_*), gbdpcg_admm_lin_grad_* and gbdpcg_kkt_grad_*; (G, C, g, c, E, lo, hi) -> (z, lambda).

soft_box_qp_solve and soft_lin_qp_solve are their twins with L1-penalised bounds (weights kappa, +Inf: a hard row): the forward pass
is the soft init and step calls, the backward pass gbdpcg_admm_soft_mask_* / gbdpcg_admm_lin_soft_mask_* (saturated rows count as
free), the HARD adjoint iteration on the masked y, gbdpcg_admm_soft_grad_bounds_* / gbdpcg_admm_lin_soft_grad_* and gbdpcg_kkt_grad_*;
they are differentiable in kappa as well.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import binding


def _sizes(nx, nu, N):
    return {"G": (nx * nx + nu * nu) * N - nu * nu, "C": (nx * nx + nx * nu) * (N - 1), "g": (nx + nu) * N - nu, "c": nx * N}


class _KktSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, C, g, c, rho, solver, nx, nu, N, batch, shared, tol, max_iter):
        sz = _sizes(nx, nu, N)
        mats = 1 if shared else batch
        kw = dict(dtype=g.dtype, device=g.device)
        S = torch.empty(mats * 3 * nx * nx * N, **kw)
        Pinv, Ginv = torch.empty_like(S), torch.empty(mats * sz["G"], **kw)
        gamma = torch.empty(batch * sz["c"], **kw)
        lam, z = torch.zeros(batch * sz["c"], **kw), torch.empty(batch * sz["g"], **kw)
        ctx.shapes = tuple(t.shape for t in (G, C, g, c))
        G, C, g, c = (t.detach().reshape(-1) for t in (G, C, g, c))
        if shared:
            # the single matrices are what the step writes at batch 1 (here on the first problem's vectors); every problem is
            # then solved on them
            lam0, z0 = torch.zeros(sz["c"], **kw), torch.empty(sz["g"], **kw)
            solver.kkt_step(nx, nu, N, 1, G, C, g[:sz["g"]], c[:sz["c"]], S, gamma[:sz["c"]], Ginv, Pinv, lam0, z0, tol=tol,
                            max_iter=max_iter)
            solver.kkt_resolve_shared(nx, nu, N, batch, Ginv, C, g, c, S, Pinv, gamma, lam, z, tol=tol, max_iter=max_iter)
        elif rho is not None:
            solver.kkt_step_reg(nx, nu, N, batch, G, C, g, c, rho.detach(), S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        else:
            solver.kkt_step(nx, nu, N, batch, G, C, g, c, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        ctx.save_for_backward(Ginv, S, Pinv, C, z, lam)
        ctx.args = (solver, nx, nu, N, batch, shared, tol, max_iter, rho is not None)
        return z, lam

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, glam):
        Ginv, S, Pinv, C, z, lam = ctx.saved_tensors
        solver, nx, nu, N, batch, shared, tol, max_iter, has_rho = ctx.args
        sz = _sizes(nx, nu, N)
        mats = 1 if shared else batch
        gz = torch.zeros_like(z) if gz is None else gz.contiguous()
        nglam = torch.zeros_like(lam) if glam is None else -glam.contiguous()
        gamma, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(z)
        need_G, need_C = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and N > 1
        gG = torch.empty(mats * sz["G"], dtype=z.dtype, device=z.device) if need_G else None
        gC = torch.empty(mats * sz["C"], dtype=z.dtype, device=z.device) if need_C else None
        # A problem that does not enter the loss (padding, a mask) has an exactly zero right-hand side: the adjoint solve starts from a
        # zero residual and returns NaN for it (the solve's rule, include/gbdpcg.h), where the gradients are exactly zero.  The mask
        # is a device tensor and the selects are stream-ordered: nothing here waits for the device.
        live = ((gz.view(batch, -1) != 0).any(1) | (nglam.view(batch, -1) != 0).any(1)).view(batch, 1)

        def keep(t):
            return None if t is None else torch.where(live, t.view(batch, -1), t.new_zeros(())).view(-1)

        if (need_G or need_C) and not shared:
            solver.kkt_backward(nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, z, lam, az, alam, gG, gC, tol=tol, max_iter=max_iter)
            az, alam, gG, gC = keep(az), keep(alam), keep(gG), keep(gC)
        else:   # the adjoint solve alone; the single gG, gC of a shared batch are summed from the pairs behind the mask
            resolve = solver.kkt_resolve_shared if shared else solver.kkt_resolve
            resolve(nx, nu, N, batch, Ginv, C, gz, nglam, S, Pinv, gamma, alam, az, tol=tol, max_iter=max_iter)
            az, alam = keep(az), keep(alam)
            if need_G or need_C:
                solver.kkt_grad_shared(nx, nu, N, batch, z, lam, az, alam, gG=gG, gC=gC, want="")
        if ctx.needs_input_grad[1] and N == 1:
            gC = torch.zeros(mats * sz["C"], dtype=z.dtype, device=z.device)
        grho = keep((az.view(batch, -1) * z.view(batch, -1)).sum(1)) if has_rho and ctx.needs_input_grad[4] else None
        grads = [t if t is None else t.view(s) for t, s in zip((gG, gC, az, -alam), ctx.shapes)]
        return (*grads, grho) + (None,) * 8


class _BoxQpSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, C, g, c, lo, hi, rho, solver, nx, nu, N, batch, iters, adj_iters, tol, max_iter):
        sz = _sizes(nx, nu, N)
        kw = dict(dtype=g.dtype, device=g.device)
        S = torch.empty(batch * 3 * nx * nx * N, **kw)
        Pinv, Ginv = torch.empty_like(S), torch.empty(batch * sz["G"], **kw)
        gamma = torch.empty(batch * sz["c"], **kw)
        lam, z = torch.zeros(batch * sz["c"], **kw), torch.empty(batch * sz["g"], **kw)
        w, y = torch.zeros(batch * sz["g"], **kw), torch.zeros(batch * sz["g"], **kw)
        res = torch.zeros(batch, 2, **kw)
        ctx.shapes = tuple(t.shape for t in (G, C, g, c, lo, hi))
        G, C, g, c, lo, hi, rho = (t.detach().reshape(-1) for t in (G, C, g, c, lo, hi, rho))
        Cp = C if N > 1 else None
        solver.kkt_step_reg(nx, nu, N, batch, G, Cp, g, c, rho, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        gt = solver.admm_init(nx, nu, N, batch, g, lo, hi, rho, w, y)
        for _ in range(iters):
            solver.admm_step(nx, nu, N, batch, Ginv, Cp, g, c, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=res, tol=tol,
                             max_iter=max_iter)
        ctx.save_for_backward(Ginv, S, Pinv, C, w, lam, y, rho)
        ctx.args = (solver, nx, nu, N, batch, adj_iters, tol, max_iter)
        ctx.mark_non_differentiable(res)
        return w, lam, res

    @staticmethod
    @once_differentiable
    def backward(ctx, gw, glam, _gres):
        Ginv, S, Pinv, C, w, lam, yf, rho = ctx.saved_tensors
        solver, nx, nu, N, batch, adj_iters, tol, max_iter = ctx.args
        sz = _sizes(nx, nu, N)
        Cp = C if N > 1 else None
        gz = torch.zeros_like(w) if gw is None else gw.contiguous().view(-1)
        nglam = torch.zeros_like(lam) if glam is None else -glam.contiguous().view(-1)
        gamma, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(w)
        wa, ya = torch.zeros_like(w), torch.zeros_like(w)
        res = torch.empty(batch, 2, dtype=w.dtype, device=w.device)
        need_G, need_C = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and N > 1
        # (a problem with exactly zero cotangents: as in _KktSolve.backward -- its adjoint solves return NaN, its gradients are
        # exactly zero; the mask and the selects run in stream order)
        live = ((gz.view(batch, -1) != 0).any(1) | (nglam.view(batch, -1) != 0).any(1)).view(batch, 1)

        def keep(t):
            return None if t is None else torch.where(live, t.view(batch, -1), t.new_zeros(())).view(-1)

        gta = solver.admm_adjoint_init(nx, nu, N, batch, gz, yf, rho, wa, ya)
        for _ in range(adj_iters):
            solver.admm_adjoint_step(nx, nu, N, batch, Ginv, Cp, gz, nglam, yf, rho, S, Pinv, gamma, alam, az, wa, ya, gta, res=res,
                                     tol=tol, max_iter=max_iter)
        glo, ghi = solver.admm_grad_bounds(nx, nu, N, batch, yf, rho, ya)
        gG = gC = None
        if need_G or need_C:
            gG = torch.empty(batch * sz["G"], dtype=w.dtype, device=w.device) if need_G else None
            gC = torch.empty(batch * sz["C"], dtype=w.dtype, device=w.device) if need_C else None
            solver.kkt_grad(nx, nu, N, batch, w, lam, wa, alam, gG=gG, gC=gC, want="")
        out = [keep(t) for t in (gG, gC, wa, -alam, glo, ghi)]
        if ctx.needs_input_grad[1] and N == 1:
            out[1] = torch.zeros(batch * sz["C"], dtype=w.dtype, device=w.device)
        grads = [t if t is None else t.view(s) for t, s in zip(out, ctx.shapes)]
        return (*grads, None) + (None,) * 9


def box_qp_solve(solver, nx, nu, N, G, C, g, c, lo, hi, rho, iters, adj_iters, tol=1e-6, max_iter=25):
    """(w, lambda, res) of  min 1/2 z'Gz + g'z  subject to  Cz = c, lo <= z <= hi  for a batch of problems, differentiable in G, C, g,
    c, lo and hi; res [batch, 2] (the ADMM residuals of the last iteration) is not differentiable, and rho gets no gradient (the
    solution does not depend on it).

    Flat contiguous device tensors of one dtype in the packed layouts of include/gbdpcg.h; lo, hi have the layout of g (-Inf / +Inf:
    no bound), rho [batch] > 0 is the ADMM penalty.  Forward: gbdpcg_kkt_step_reg_*, gbdpcg_admm_init_* from w = y = 0, then `iters`
    gbdpcg_admm_step_*; w lies in the box exactly.  Backward: gbdpcg_admm_adjoint_init_* from zeros, `adj_iters`
    gbdpcg_admm_adjoint_step_* on the kept factorisation, gbdpcg_admm_grad_bounds_*, gbdpcg_kkt_grad_*.  Both counts are fixed: nothing
    waits for the device, and the gradients are only as converged as the two loops -- read res to judge the forward one.

    The active set is the sign pattern of the forward y: entry i is clamped iff y_i != 0 (no threshold), its dl/dg_i is exactly 0 and
    dl/dlo_i or dl/dhi_i carries the adjoint's multiplier.  An entry that sits on its bound with y_i = 0 (weakly active) counts as
    free.  A forward loop that has not converged leaves whatever mask y holds.  tol, max_iter: the PCG settings of every solve.
    A problem whose rows of dl/dw and dl/dlambda are exactly zero gets exactly zero gradients (as in kkt_solve)."""
    if not isinstance(solver, binding.Solver):
        raise TypeError("box_qp_solve: solver is a binding.Solver")
    sz = _sizes(nx, nu, N)
    for name, t in (("G", G), ("C", C), ("g", g), ("c", c), ("lo", lo), ("hi", hi), ("rho", rho)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == g.dtype):
            raise ValueError(f"box_qp_solve: {name} must be a contiguous device tensor of g's dtype")
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"box_qp_solve: unsupported dtype {g.dtype}")
    if g.numel() == 0 or g.numel() % sz["g"]:
        raise ValueError("box_qp_solve: g is not a whole number of problems")
    batch = g.numel() // sz["g"]
    want = {"G": batch * sz["G"], "C": batch * sz["C"], "g": batch * sz["g"], "c": batch * sz["c"], "lo": batch * sz["g"],
            "hi": batch * sz["g"], "rho": batch}
    for name, t in (("G", G), ("C", C), ("c", c), ("lo", lo), ("hi", hi), ("rho", rho)):
        if t.numel() != want[name]:
            raise ValueError(f"box_qp_solve: {name} has {t.numel()} elements, the layout takes {want[name]}")
    if int(iters) < 1 or int(adj_iters) < 1:
        raise ValueError("box_qp_solve: iters and adj_iters are at least 1")
    return _BoxQpSolve.apply(G, C, g, c, lo, hi, rho, solver, nx, nu, N, batch, int(iters), int(adj_iters), tol, max_iter)


class _LinQpSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, C, g, c, E, lo, hi, rho, solver, nx, nu, mx, mu, N, batch, iters, adj_iters, tol, max_iter):
        sz = _sizes(nx, nu, N)
        nw = (mx + mu) * N - mu
        kw = dict(dtype=g.dtype, device=g.device)
        S = torch.empty(batch * 3 * nx * nx * N, **kw)
        Pinv, Ginv = torch.empty_like(S), torch.empty(batch * sz["G"], **kw)
        gamma = torch.empty(batch * sz["c"], **kw)
        lam, z = torch.zeros(batch * sz["c"], **kw), torch.empty(batch * sz["g"], **kw)
        w, y = torch.zeros(batch * nw, **kw), torch.zeros(batch * nw, **kw)
        res = torch.zeros(batch, 2, **kw)
        ctx.shapes = tuple(t.shape for t in (G, C, g, c, E, lo, hi))
        G, C, g, c, E, lo, hi, rho = (t.detach().reshape(-1) for t in (G, C, g, c, E, lo, hi, rho))
        Cp = C if N > 1 else None
        Gt = solver.admm_lin_form(nx, nu, mx, mu, N, batch, G, E, rho)
        solver.kkt_step(nx, nu, N, batch, Gt, Cp, g, c, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        gt = solver.admm_lin_init(nx, nu, mx, mu, N, batch, g, E, lo, hi, rho, w, y)
        for _ in range(iters):
            solver.admm_lin_step(nx, nu, mx, mu, N, batch, Ginv, Cp, g, c, E, lo, hi, rho, S, Pinv, gamma, lam, z, w, y, gt, res=res,
                                 tol=tol, max_iter=max_iter)
        ctx.save_for_backward(Ginv, S, Pinv, C, E, z, lam, y, rho)
        ctx.args = (solver, nx, nu, mx, mu, N, batch, adj_iters, tol, max_iter)
        ctx.mark_non_differentiable(res)
        return z, lam, res

    @staticmethod
    @once_differentiable
    def backward(ctx, gzz, glam, _gres):
        Ginv, S, Pinv, C, E, z, lam, yf, rho = ctx.saved_tensors
        solver, nx, nu, mx, mu, N, batch, adj_iters, tol, max_iter = ctx.args
        sz = _sizes(nx, nu, N)
        Cp = C if N > 1 else None
        gz = torch.zeros_like(z) if gzz is None else gzz.contiguous().view(-1)
        nglam = torch.zeros_like(lam) if glam is None else -glam.contiguous().view(-1)
        gamma, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(z)
        wa, ya = torch.zeros_like(yf), torch.zeros_like(yf)
        res = torch.empty(batch, 2, dtype=z.dtype, device=z.device)
        need_G, need_C = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and N > 1
        # (a problem with exactly zero cotangents: as in _KktSolve.backward -- its adjoint solves return NaN, its gradients are
        # exactly zero; the mask and the selects run in stream order)
        live = ((gz.view(batch, -1) != 0).any(1) | (nglam.view(batch, -1) != 0).any(1)).view(batch, 1)

        def keep(t):
            return None if t is None else torch.where(live, t.view(batch, -1), t.new_zeros(())).view(-1)

        gta = solver.admm_lin_adjoint_init(nx, nu, mx, mu, N, batch, gz, E, yf, rho, wa, ya)
        for _ in range(adj_iters):
            solver.admm_lin_adjoint_step(nx, nu, mx, mu, N, batch, Ginv, Cp, gz, nglam, E, yf, rho, S, Pinv, gamma, alam, az, wa, ya,
                                         gta, res=res, tol=tol, max_iter=max_iter)
        glo, ghi, gE = solver.admm_lin_grad(nx, nu, mx, mu, N, batch, z, az, yf, ya, rho)
        gG = gC = None
        if need_G or need_C:
            gG = torch.empty(batch * sz["G"], dtype=z.dtype, device=z.device) if need_G else None
            gC = torch.empty(batch * sz["C"], dtype=z.dtype, device=z.device) if need_C else None
            solver.kkt_grad(nx, nu, N, batch, z, lam, az, alam, gG=gG, gC=gC, want="")
        out = [keep(t) for t in (gG, gC, az, -alam, gE, glo, ghi)]
        if ctx.needs_input_grad[1] and N == 1:
            out[1] = torch.zeros(batch * sz["C"], dtype=z.dtype, device=z.device)
        grads = [t if t is None else t.view(s) for t, s in zip(out, ctx.shapes)]
        return (*grads, None) + (None,) * 11


def lin_qp_solve(solver, nx, nu, mx, mu, N, G, C, g, c, E, lo, hi, rho, iters, adj_iters, tol=1e-6, max_iter=25):
    """(z, lambda, res) of  min 1/2 z'Gz + g'z  subject to  Cz = c, lo <= Ez <= hi  for a batch of problems, differentiable in G, C, g,
    c, E, lo and hi; res [batch, 2] (the ADMM residuals of the last iteration) is not differentiable, and rho gets no gradient (the
    solution does not depend on it).

    Flat contiguous device tensors of one dtype in the packed layouts of include/gbdpcg.h: E = [Ex_0 Eu_0 ... Ex_{N-1}] column-major
    blocks (mx x nx, mu x nu), lo, hi in the layout of the rows [mx | mu | ... | mx] (-Inf / +Inf: no bound), rho [batch] > 0 the ADMM
    penalty.  Forward: gbdpcg_admm_lin_form_* into a private Gt = G + rho E'E, gbdpcg_kkt_step_* on it, gbdpcg_admm_lin_init_* from
    w = y = 0, then `iters` gbdpcg_admm_lin_step_*; z is the last solve's (E z is in the bounds to the residual res[:, 0]).  Backward:
    gbdpcg_admm_lin_adjoint_init_* from zeros, `adj_iters` gbdpcg_admm_lin_adjoint_step_* on the kept factorisation,
    gbdpcg_admm_lin_grad_*, gbdpcg_kkt_grad_* (the gradient in G, not in Gt).  Both counts are fixed: nothing waits for the device,
    and the gradients are only as converged as the two loops -- read res to judge the forward one.

    The active set is the sign pattern of the forward y: row r is active iff y_r != 0 (no threshold); a row that sits on its bound
    with y_r = 0 (weakly active) counts as free.  A forward loop that has not converged leaves whatever mask y holds.  tol, max_iter:
    the PCG settings of every solve.  A problem whose rows of dl/dz and dl/dlambda are exactly zero gets exactly zero gradients."""
    if not isinstance(solver, binding.Solver):
        raise TypeError("lin_qp_solve: solver is a binding.Solver")
    sz = _sizes(nx, nu, N)
    nw, ne = (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu
    for name, t in (("G", G), ("C", C), ("g", g), ("c", c), ("E", E), ("lo", lo), ("hi", hi), ("rho", rho)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == g.dtype):
            raise ValueError(f"lin_qp_solve: {name} must be a contiguous device tensor of g's dtype")
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"lin_qp_solve: unsupported dtype {g.dtype}")
    if nw <= 0:
        raise ValueError("lin_qp_solve: no rows at all")
    if g.numel() == 0 or g.numel() % sz["g"]:
        raise ValueError("lin_qp_solve: g is not a whole number of problems")
    batch = g.numel() // sz["g"]
    want = {"G": batch * sz["G"], "C": batch * sz["C"], "c": batch * sz["c"], "E": batch * ne, "lo": batch * nw, "hi": batch * nw,
            "rho": batch}
    for name, t in (("G", G), ("C", C), ("c", c), ("E", E), ("lo", lo), ("hi", hi), ("rho", rho)):
        if t.numel() != want[name]:
            raise ValueError(f"lin_qp_solve: {name} has {t.numel()} elements, the layout takes {want[name]}")
    if int(iters) < 1 or int(adj_iters) < 1:
        raise ValueError("lin_qp_solve: iters and adj_iters are at least 1")
    return _LinQpSolve.apply(G, C, g, c, E, lo, hi, rho, solver, nx, nu, mx, mu, N, batch, int(iters), int(adj_iters), tol, max_iter)


class _SoftBoxQpSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, C, g, c, lo, hi, kappa, rho, solver, nx, nu, N, batch, iters, adj_iters, tol, max_iter):
        sz = _sizes(nx, nu, N)
        kw = dict(dtype=g.dtype, device=g.device)
        S = torch.empty(batch * 3 * nx * nx * N, **kw)
        Pinv, Ginv = torch.empty_like(S), torch.empty(batch * sz["G"], **kw)
        gamma = torch.empty(batch * sz["c"], **kw)
        lam, z = torch.zeros(batch * sz["c"], **kw), torch.empty(batch * sz["g"], **kw)
        w, y = torch.zeros(batch * sz["g"], **kw), torch.zeros(batch * sz["g"], **kw)
        res = torch.zeros(batch, 2, **kw)
        ctx.shapes = tuple(t.shape for t in (G, C, g, c, lo, hi, kappa))
        G, C, g, c, lo, hi, kappa, rho = (t.detach().reshape(-1) for t in (G, C, g, c, lo, hi, kappa, rho))
        Cp = C if N > 1 else None
        solver.kkt_step_reg(nx, nu, N, batch, G, Cp, g, c, rho, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        gt = solver.admm_soft_init(nx, nu, N, batch, g, lo, hi, kappa, rho, w, y)
        for _ in range(iters):
            solver.admm_soft_step(nx, nu, N, batch, Ginv, Cp, g, c, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt, res=res, tol=tol,
                                  max_iter=max_iter)
        ctx.save_for_backward(Ginv, S, Pinv, C, w, lam, y, kappa, rho)
        ctx.args = (solver, nx, nu, N, batch, adj_iters, tol, max_iter)
        ctx.mark_non_differentiable(res)
        return w, lam, res

    @staticmethod
    @once_differentiable
    def backward(ctx, gw, glam, _gres):
        Ginv, S, Pinv, C, w, lam, yf, kappa, rho = ctx.saved_tensors
        solver, nx, nu, N, batch, adj_iters, tol, max_iter = ctx.args
        sz = _sizes(nx, nu, N)
        Cp = C if N > 1 else None
        gz = torch.zeros_like(w) if gw is None else gw.contiguous().view(-1)
        nglam = torch.zeros_like(lam) if glam is None else -glam.contiguous().view(-1)
        gamma, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(w)
        wa, ya = torch.zeros_like(w), torch.zeros_like(w)
        res = torch.empty(batch, 2, dtype=w.dtype, device=w.device)
        need_G, need_C = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and N > 1
        # (a problem with exactly zero cotangents: as in _KktSolve.backward -- its adjoint solves return NaN, its gradients are
        # exactly zero; the mask and the selects run in stream order)
        live = ((gz.view(batch, -1) != 0).any(1) | (nglam.view(batch, -1) != 0).any(1)).view(batch, 1)

        def keep(t):
            return None if t is None else torch.where(live, t.view(batch, -1), t.new_zeros(())).view(-1)

        ym = solver.admm_soft_mask(nx, nu, N, batch, yf, kappa, rho)       # saturated entries count as free from here on
        gta = solver.admm_adjoint_init(nx, nu, N, batch, gz, ym, rho, wa, ya)
        for _ in range(adj_iters):
            solver.admm_adjoint_step(nx, nu, N, batch, Ginv, Cp, gz, nglam, ym, rho, S, Pinv, gamma, alam, az, wa, ya, gta, res=res,
                                     tol=tol, max_iter=max_iter)
        glo, ghi, gkappa = solver.admm_soft_grad_bounds(nx, nu, N, batch, yf, kappa, rho, ya, az)
        gG = gC = None
        if need_G or need_C:
            gG = torch.empty(batch * sz["G"], dtype=w.dtype, device=w.device) if need_G else None
            gC = torch.empty(batch * sz["C"], dtype=w.dtype, device=w.device) if need_C else None
            solver.kkt_grad(nx, nu, N, batch, w, lam, wa, alam, gG=gG, gC=gC, want="")
        out = [keep(t) for t in (gG, gC, wa, -alam, glo, ghi, gkappa)]
        if ctx.needs_input_grad[1] and N == 1:
            out[1] = torch.zeros(batch * sz["C"], dtype=w.dtype, device=w.device)
        grads = [t if t is None else t.view(s) for t, s in zip(out, ctx.shapes)]
        return (*grads, None) + (None,) * 9


def soft_box_qp_solve(solver, nx, nu, N, G, C, g, c, lo, hi, kappa, rho, iters, adj_iters, tol=1e-6, max_iter=25):
    """(w, lambda, res) of  min 1/2 z'Gz + g'z + sum_i kappa_i dist(z_i, [lo_i, hi_i])  subject to  Cz = c  for a batch of problems,
    differentiable in G, C, g, c, lo, hi and kappa; the outputs and conventions of box_qp_solve, whose bits (gradients included) it
    gives where kappa = +Inf everywhere.  kappa has the layout of lo (+Inf: a hard bound, 0: no bound); rho gets no gradient.

    Forward: gbdpcg_kkt_step_reg_*, gbdpcg_admm_soft_init_* from w = y = 0, then `iters` gbdpcg_admm_soft_step_*.  Backward:
    gbdpcg_admm_soft_mask_* on the forward y, gbdpcg_admm_adjoint_init_* and `adj_iters` gbdpcg_admm_adjoint_step_* on the masked
    y, gbdpcg_admm_soft_grad_bounds_*, gbdpcg_kkt_grad_*.  Both counts are fixed and nothing waits for the device.

    The forward y splits the entries, to the bit: y_i = 0 free; 0 < |y_i| < kappa_i / rho held at its bound (dl/dlo_i or dl/dhi_i
    carries the adjoint's multiplier, dl/dg_i = 0); |y_i| = kappa_i / rho saturated, beyond its bound with the constant multiplier
    +-kappa_i -- free in the adjoint, dl/dkappa_i = sign(y_i) a_z,i, dl/dlo_i = dl/dhi_i = 0.  dl/dkappa is exactly zero everywhere
    else, so where kappa = +Inf.  A problem whose rows of dl/dw and dl/dlambda are exactly zero gets exactly zero gradients."""
    if not isinstance(solver, binding.Solver):
        raise TypeError("soft_box_qp_solve: solver is a binding.Solver")
    sz = _sizes(nx, nu, N)
    named = (("G", G), ("C", C), ("g", g), ("c", c), ("lo", lo), ("hi", hi), ("kappa", kappa), ("rho", rho))
    for name, t in named:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == g.dtype):
            raise ValueError(f"soft_box_qp_solve: {name} must be a contiguous device tensor of g's dtype")
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"soft_box_qp_solve: unsupported dtype {g.dtype}")
    if g.numel() == 0 or g.numel() % sz["g"]:
        raise ValueError("soft_box_qp_solve: g is not a whole number of problems")
    batch = g.numel() // sz["g"]
    want = {"G": batch * sz["G"], "C": batch * sz["C"], "g": batch * sz["g"], "c": batch * sz["c"], "lo": batch * sz["g"],
            "hi": batch * sz["g"], "kappa": batch * sz["g"], "rho": batch}
    for name, t in named:
        if t.numel() != want[name]:
            raise ValueError(f"soft_box_qp_solve: {name} has {t.numel()} elements, the layout takes {want[name]}")
    if int(iters) < 1 or int(adj_iters) < 1:
        raise ValueError("soft_box_qp_solve: iters and adj_iters are at least 1")
    return _SoftBoxQpSolve.apply(G, C, g, c, lo, hi, kappa, rho, solver, nx, nu, N, batch, int(iters), int(adj_iters), tol, max_iter)


class _SoftLinQpSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, C, g, c, E, lo, hi, kappa, rho, solver, nx, nu, mx, mu, N, batch, iters, adj_iters, tol, max_iter):
        sz = _sizes(nx, nu, N)
        nw = (mx + mu) * N - mu
        kw = dict(dtype=g.dtype, device=g.device)
        S = torch.empty(batch * 3 * nx * nx * N, **kw)
        Pinv, Ginv = torch.empty_like(S), torch.empty(batch * sz["G"], **kw)
        gamma = torch.empty(batch * sz["c"], **kw)
        lam, z = torch.zeros(batch * sz["c"], **kw), torch.empty(batch * sz["g"], **kw)
        w, y = torch.zeros(batch * nw, **kw), torch.zeros(batch * nw, **kw)
        res = torch.zeros(batch, 2, **kw)
        ctx.shapes = tuple(t.shape for t in (G, C, g, c, E, lo, hi, kappa))
        G, C, g, c, E, lo, hi, kappa, rho = (t.detach().reshape(-1) for t in (G, C, g, c, E, lo, hi, kappa, rho))
        Cp = C if N > 1 else None
        Gt = solver.admm_lin_form(nx, nu, mx, mu, N, batch, G, E, rho)
        solver.kkt_step(nx, nu, N, batch, Gt, Cp, g, c, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        gt = solver.admm_lin_soft_init(nx, nu, mx, mu, N, batch, g, E, lo, hi, kappa, rho, w, y)
        for _ in range(iters):
            solver.admm_lin_soft_step(nx, nu, mx, mu, N, batch, Ginv, Cp, g, c, E, lo, hi, kappa, rho, S, Pinv, gamma, lam, z, w, y, gt,
                                      res=res, tol=tol, max_iter=max_iter)
        ctx.save_for_backward(Ginv, S, Pinv, C, E, z, lam, y, kappa, rho)
        ctx.args = (solver, nx, nu, mx, mu, N, batch, adj_iters, tol, max_iter)
        ctx.mark_non_differentiable(res)
        return z, lam, res

    @staticmethod
    @once_differentiable
    def backward(ctx, gzz, glam, _gres):
        Ginv, S, Pinv, C, E, z, lam, yf, kappa, rho = ctx.saved_tensors
        solver, nx, nu, mx, mu, N, batch, adj_iters, tol, max_iter = ctx.args
        sz = _sizes(nx, nu, N)
        Cp = C if N > 1 else None
        gz = torch.zeros_like(z) if gzz is None else gzz.contiguous().view(-1)
        nglam = torch.zeros_like(lam) if glam is None else -glam.contiguous().view(-1)
        gamma, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(z)
        wa, ya = torch.zeros_like(yf), torch.zeros_like(yf)
        res = torch.empty(batch, 2, dtype=z.dtype, device=z.device)
        need_G, need_C = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and N > 1
        # (a problem with exactly zero cotangents: as in _KktSolve.backward -- its adjoint solves return NaN, its gradients are
        # exactly zero; the mask and the selects run in stream order)
        live = ((gz.view(batch, -1) != 0).any(1) | (nglam.view(batch, -1) != 0).any(1)).view(batch, 1)

        def keep(t):
            return None if t is None else torch.where(live, t.view(batch, -1), t.new_zeros(())).view(-1)

        ym = solver.admm_lin_soft_mask(nx, nu, mx, mu, N, batch, yf, kappa, rho)       # saturated rows count as free from here on
        gta = solver.admm_lin_adjoint_init(nx, nu, mx, mu, N, batch, gz, E, ym, rho, wa, ya)
        for _ in range(adj_iters):
            solver.admm_lin_adjoint_step(nx, nu, mx, mu, N, batch, Ginv, Cp, gz, nglam, E, ym, rho, S, Pinv, gamma, alam, az, wa, ya,
                                         gta, res=res, tol=tol, max_iter=max_iter)
        glo, ghi, gkappa, gE = solver.admm_lin_soft_grad(nx, nu, mx, mu, N, batch, z, az, E, yf, ya, kappa, rho)
        gG = gC = None
        if need_G or need_C:
            gG = torch.empty(batch * sz["G"], dtype=z.dtype, device=z.device) if need_G else None
            gC = torch.empty(batch * sz["C"], dtype=z.dtype, device=z.device) if need_C else None
            solver.kkt_grad(nx, nu, N, batch, z, lam, az, alam, gG=gG, gC=gC, want="")
        out = [keep(t) for t in (gG, gC, az, -alam, gE, glo, ghi, gkappa)]
        if ctx.needs_input_grad[1] and N == 1:
            out[1] = torch.zeros(batch * sz["C"], dtype=z.dtype, device=z.device)
        grads = [t if t is None else t.view(s) for t, s in zip(out, ctx.shapes)]
        return (*grads, None) + (None,) * 11


def soft_lin_qp_solve(solver, nx, nu, mx, mu, N, G, C, g, c, E, lo, hi, kappa, rho, iters, adj_iters, tol=1e-6, max_iter=25):
    """(z, lambda, res) of  min 1/2 z'Gz + g'z + sum_r kappa_r dist((Ez)_r, [lo_r, hi_r])  subject to  Cz = c  for a batch of problems,
    differentiable in G, C, g, c, E, lo, hi and kappa; the outputs and conventions of lin_qp_solve, whose bits (gradients included) it
    gives where kappa = +Inf everywhere.  kappa has the layout of lo (+Inf: a hard row, 0: no row); rho gets no gradient.

    Forward: gbdpcg_admm_lin_form_* into a private Gt, gbdpcg_kkt_step_* on it, gbdpcg_admm_lin_soft_init_* from w = y = 0, then
    `iters` gbdpcg_admm_lin_soft_step_*.  Backward: gbdpcg_admm_lin_soft_mask_* on the forward y, gbdpcg_admm_lin_adjoint_init_* and
    `adj_iters` gbdpcg_admm_lin_adjoint_step_* on the masked y, gbdpcg_admm_lin_soft_grad_*, gbdpcg_kkt_grad_*.  Both counts are fixed
    and nothing waits for the device.

    The forward y splits the rows, to the bit: y_r = 0 free; 0 < |y_r| < kappa_r / rho held at its bound; |y_r| = kappa_r / rho
    saturated, beyond its bound with the constant multiplier +-kappa_r -- free in the adjoint, dl/dkappa_r = sign(y_r) (E a_z)_r,
    dl/dE(r, .) = rho y_r a_z', dl/dlo_r = dl/dhi_r = 0.  dl/dkappa is exactly zero everywhere else, so where kappa = +Inf.  A problem
    whose rows of dl/dz and dl/dlambda are exactly zero gets exactly zero gradients."""
    if not isinstance(solver, binding.Solver):
        raise TypeError("soft_lin_qp_solve: solver is a binding.Solver")
    sz = _sizes(nx, nu, N)
    nw, ne = (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu
    named = (("G", G), ("C", C), ("g", g), ("c", c), ("E", E), ("lo", lo), ("hi", hi), ("kappa", kappa), ("rho", rho))
    for name, t in named:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == g.dtype):
            raise ValueError(f"soft_lin_qp_solve: {name} must be a contiguous device tensor of g's dtype")
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"soft_lin_qp_solve: unsupported dtype {g.dtype}")
    if nw <= 0:
        raise ValueError("soft_lin_qp_solve: no rows at all")
    if g.numel() == 0 or g.numel() % sz["g"]:
        raise ValueError("soft_lin_qp_solve: g is not a whole number of problems")
    batch = g.numel() // sz["g"]
    want = {"G": batch * sz["G"], "C": batch * sz["C"], "g": batch * sz["g"], "c": batch * sz["c"], "E": batch * ne, "lo": batch * nw,
            "hi": batch * nw, "kappa": batch * nw, "rho": batch}
    for name, t in named:
        if t.numel() != want[name]:
            raise ValueError(f"soft_lin_qp_solve: {name} has {t.numel()} elements, the layout takes {want[name]}")
    if int(iters) < 1 or int(adj_iters) < 1:
        raise ValueError("soft_lin_qp_solve: iters and adj_iters are at least 1")
    return _SoftLinQpSolve.apply(G, C, g, c, E, lo, hi, kappa, rho, solver, nx, nu, mx, mu, N, batch, int(iters), int(adj_iters), tol,
                                 max_iter)


def kkt_solve(solver, nx, nu, N, G, C, g, c, rho=None, shared=False, tol=1e-6, max_iter=25):
    """(z, lambda) of  G z + g + C' lambda = 0,  C z = c  for a batch of problems, differentiable in G, C, g, c (and rho).

    Flat contiguous device tensors of one dtype in the packed layouts of include/gbdpcg.h; the batch is g.numel() over one
    problem's extent.  rho: [batch], the per-problem regularisation of gbdpcg_kkt_step_reg_* (problem b is solved with
    G_b + rho_b I).  shared=True: G and C are ONE problem's blocks, used by every problem of the batch, and their gradients are
    the sums over the batch.  tol, max_iter: the PCG settings of the forward and of the adjoint solve.  The gradient in G is
    the symmetrised one (the library reads G as symmetric).  The handle's symmetric mode and path are left as found.

    Exactly zero right-hand sides.  Forward: a problem whose gamma = -(c + C G^-1 g) is exactly zero (g = 0 and c = 0, say) starts
    the PCG from a zero residual and, by the reference's rule (0/0 in the first step; include/gbdpcg.h), comes back with z and
    lambda NaN in every entry where the answer is zero.  That is confined to its problem -- the others keep every bit -- and shows on
    the device as max_iter_exit = 1 of the step and as NaN norms from Solver.kkt_residual; kkt_solve does not repair it.  Backward:
    a problem whose rows of dl/dz and dl/dlambda are exactly zero (it does not enter the loss: padding, a per-sample mask) gets
    exactly zero gradients in g, c, rho and its rows of G and C, and contributes exact zeros to the summed gradients of a shared
    batch; the mask is built and applied on the device, in stream order."""
    if not isinstance(solver, binding.Solver):
        raise TypeError("kkt_solve: solver is a binding.Solver")
    sz = _sizes(nx, nu, N)
    for name, t in (("G", G), ("C", C), ("g", g), ("c", c)) + ((("rho", rho),) if rho is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == g.dtype):
            raise ValueError(f"kkt_solve: {name} must be a contiguous device tensor of g's dtype")
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"kkt_solve: unsupported dtype {g.dtype}")
    if g.numel() == 0 or g.numel() % sz["g"]:
        raise ValueError("kkt_solve: g is not a whole number of problems")
    batch = g.numel() // sz["g"]
    if shared and rho is not None:
        raise ValueError("kkt_solve: rho is per problem and has no shared-matrix form (regularise the single G instead)")
    mats = 1 if shared else batch
    want = {"G": mats * sz["G"], "C": mats * sz["C"], "g": batch * sz["g"], "c": batch * sz["c"]}
    for name, t in (("G", G), ("C", C), ("g", g), ("c", c)):
        if t.numel() != want[name]:
            raise ValueError(f"kkt_solve: {name} has {t.numel()} elements, the layout takes {want[name]}")
    if rho is not None and rho.numel() != batch:
        raise ValueError("kkt_solve: rho has one element per problem")
    return _KktSolve.apply(G, C, g, c, rho, solver, nx, nu, N, batch, shared, tol, max_iter)
