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

from typing import NamedTuple, Optional

import torch
from torch.autograd.function import once_differentiable

from . import binding


def _sizes(nx, nu, N):
    return {"G": (nx * nx + nu * nu) * N - nu * nu, "C": (nx * nx + nx * nu) * (N - 1), "g": (nx + nu) * N - nu, "c": nx * N}


def _keep_live(gz, nglam, batch):
    """keep(t): t with the rows of the problems whose cotangents gz, nglam are exactly zero replaced by exact zeros (None stays None)."""
    live = ((gz.view(batch, -1) != 0).any(1) | (nglam.view(batch, -1) != 0).any(1)).view(batch, 1)

    def keep(t):
        return None if t is None else torch.where(live, t.view(batch, -1), t.new_zeros(())).view(-1)

    return keep


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
        keep = _keep_live(gz, nglam, batch)
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


class _Family(NamedTuple):
    """One of the four ADMM QPs: what its bounds are on, whether they are soft, and the Solver methods its two loops are made of."""
    rows: bool            # the bounds are on E z (E is an input, z the output); otherwise on z itself (the output is w)
    soft: bool            # L1-penalised bounds with the weights kappa (an input)
    init: str
    step: str
    mask: Optional[str]   # soft: what turns the forward y into the yf of the hard adjoint loop
    adj_init: str
    adj_step: str
    grad: str


_BOX = _Family(False, False, "admm_init", "admm_step", None, "admm_adjoint_init", "admm_adjoint_step", "admm_grad_bounds")
_LIN = _Family(True, False, "admm_lin_init", "admm_lin_step", None, "admm_lin_adjoint_init", "admm_lin_adjoint_step", "admm_lin_grad")
_SOFT_BOX = _Family(False, True, "admm_soft_init", "admm_soft_step", "admm_soft_mask", "admm_adjoint_init", "admm_adjoint_step",
                    "admm_soft_grad_bounds")
_SOFT_LIN = _Family(True, True, "admm_lin_soft_init", "admm_lin_soft_step", "admm_lin_soft_mask", "admm_lin_adjoint_init",
                    "admm_lin_adjoint_step", "admm_lin_soft_grad")


class _AdmmQpSolve(torch.autograd.Function):
    """dims: (nx, nu, N), with rows (nx, nu, mx, mu, N) -- what every Solver call of the family starts with, in front of batch.  E and
    kappa are None where the family has none."""

    @staticmethod
    def forward(ctx, fam, solver, dims, batch, iters, adj_iters, tol, max_iter, G, C, g, c, E, lo, hi, kappa, rho):
        nx, nu, N = dims[0], dims[1], dims[-1]
        sz = _sizes(nx, nu, N)
        kw = dict(dtype=g.dtype, device=g.device)
        S = torch.empty(batch * 3 * nx * nx * N, **kw)
        Pinv, Ginv = torch.empty_like(S), torch.empty(batch * sz["G"], **kw)
        gamma = torch.empty(batch * sz["c"], **kw)
        lam, z = torch.zeros(batch * sz["c"], **kw), torch.empty(batch * sz["g"], **kw)
        w, y = torch.zeros(lo.numel(), **kw), torch.zeros(lo.numel(), **kw)
        res = torch.zeros(batch, 2, **kw)
        ctx.shapes = tuple(None if t is None else t.shape for t in (G, C, g, c, E, lo, hi, kappa))
        G, C, g, c, E, lo, hi, kappa, rho = (None if t is None else t.detach().reshape(-1)
                                             for t in (G, C, g, c, E, lo, hi, kappa, rho))
        Cp = C if N > 1 else None
        sizes = (*dims, batch)
        bounds = ((E,) if fam.rows else ()) + (lo, hi) + ((kappa,) if fam.soft else ())
        if fam.rows:
            Gt = solver.admm_lin_form(*sizes, G, E, rho)
            solver.kkt_step(nx, nu, N, batch, Gt, Cp, g, c, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        else:
            solver.kkt_step_reg(nx, nu, N, batch, G, Cp, g, c, rho, S, gamma, Ginv, Pinv, lam, z, tol=tol, max_iter=max_iter)
        gt = getattr(solver, fam.init)(*sizes, g, *bounds, rho, w, y)
        step = getattr(solver, fam.step)
        for _ in range(iters):
            step(*sizes, Ginv, Cp, g, c, *bounds, rho, S, Pinv, gamma, lam, z, w, y, gt, res=res, tol=tol, max_iter=max_iter)
        out = z if fam.rows else w
        ctx.save_for_backward(Ginv, S, Pinv, C, E, out, lam, y, kappa, rho)
        ctx.args = (fam, solver, dims, batch, adj_iters, tol, max_iter)
        ctx.mark_non_differentiable(res)
        return out, lam, res

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, glam, _gres):
        Ginv, S, Pinv, C, E, x, lam, yf, kappa, rho = ctx.saved_tensors      # x: the forward output, w (box) or z (rows)
        fam, solver, dims, batch, adj_iters, tol, max_iter = ctx.args
        nx, nu, N = dims[0], dims[1], dims[-1]
        sz = _sizes(nx, nu, N)
        Cp = C if N > 1 else None
        gz = torch.zeros_like(x) if gout is None else gout.contiguous().view(-1)
        nglam = torch.zeros_like(lam) if glam is None else -glam.contiguous().view(-1)
        gamma, alam, az = torch.empty_like(lam), torch.zeros_like(lam), torch.empty_like(x)
        wa, ya = torch.zeros_like(yf), torch.zeros_like(yf)
        res = torch.empty(batch, 2, dtype=x.dtype, device=x.device)
        need_G, need_C = ctx.needs_input_grad[8], ctx.needs_input_grad[9] and N > 1
        # (a problem with exactly zero cotangents: as in _KktSolve.backward -- its adjoint solves return NaN, its gradients are
        # exactly zero; the mask and the selects run in stream order)
        keep = _keep_live(gz, nglam, batch)
        sizes = (*dims, batch)
        rows = (E,) if fam.rows else ()
        # soft: saturated entries / rows count as free from here on
        ym = getattr(solver, fam.mask)(*sizes, yf, kappa, rho) if fam.soft else yf
        gta = getattr(solver, fam.adj_init)(*sizes, gz, *rows, ym, rho, wa, ya)
        adj_step = getattr(solver, fam.adj_step)
        for _ in range(adj_iters):
            adj_step(*sizes, Ginv, Cp, gz, nglam, *rows, ym, rho, S, Pinv, gamma, alam, az, wa, ya, gta, res=res, tol=tol,
                     max_iter=max_iter)
        grad, gE, gkappa = getattr(solver, fam.grad), None, None
        if fam.rows and fam.soft:
            glo, ghi, gkappa, gE = grad(*sizes, x, az, E, yf, ya, kappa, rho)
        elif fam.rows:
            glo, ghi, gE = grad(*sizes, x, az, yf, ya, rho)
        elif fam.soft:
            glo, ghi, gkappa = grad(*sizes, yf, kappa, rho, ya, az)
        else:
            glo, ghi = grad(*sizes, yf, rho, ya)
        ax = az if fam.rows else wa      # the adjoint's primal: its z where the output is z, its w where the output is w
        gG = gC = None
        if need_G or need_C:
            gG = torch.empty(batch * sz["G"], dtype=x.dtype, device=x.device) if need_G else None
            gC = torch.empty(batch * sz["C"], dtype=x.dtype, device=x.device) if need_C else None
            solver.kkt_grad(nx, nu, N, batch, x, lam, ax, alam, gG=gG, gC=gC, want="")
        gG, gC, gg, gc, gE, glo, ghi, gkappa = (keep(t) for t in (gG, gC, ax, -alam, gE, glo, ghi, gkappa))
        if ctx.needs_input_grad[9] and N == 1:
            gC = torch.zeros(batch * sz["C"], dtype=x.dtype, device=x.device)
        grads = [t if t is None else t.view(s) for t, s in zip((gG, gC, gg, gc, gE, glo, ghi, gkappa), ctx.shapes)]
        return (None,) * 8 + (*grads, None)


def _check_qp(fn, solver, nx, nu, N, rows, named, iters, adj_iters):
    """The validation the four ADMM QP functions share; fn: the caller's name, rows: (mx, mu) or None, named: (name, tensor) pairs.
    Returns the batch."""
    if not isinstance(solver, binding.Solver):
        raise TypeError(f"{fn}: solver is a binding.Solver")
    sz = _sizes(nx, nu, N)
    g = dict(named)["g"]
    for name, t in named:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == g.dtype):
            raise ValueError(f"{fn}: {name} must be a contiguous device tensor of g's dtype")
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{fn}: unsupported dtype {g.dtype}")
    nw, ne = sz["g"], 0
    if rows is not None:
        mx, mu = rows
        nw, ne = (mx + mu) * N - mu, (mx * nx + mu * nu) * N - mu * nu
        if nw <= 0:
            raise ValueError(f"{fn}: no rows at all")
    if g.numel() == 0 or g.numel() % sz["g"]:
        raise ValueError(f"{fn}: g is not a whole number of problems")
    batch = g.numel() // sz["g"]
    want = {"G": batch * sz["G"], "C": batch * sz["C"], "g": batch * sz["g"], "c": batch * sz["c"], "E": batch * ne, "lo": batch * nw,
            "hi": batch * nw, "kappa": batch * nw, "rho": batch}
    for name, t in named:
        if t.numel() != want[name]:
            raise ValueError(f"{fn}: {name} has {t.numel()} elements, the layout takes {want[name]}")
    if int(iters) < 1 or int(adj_iters) < 1:
        raise ValueError(f"{fn}: iters and adj_iters are at least 1")
    return batch


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
    named = (("G", G), ("C", C), ("g", g), ("c", c), ("lo", lo), ("hi", hi), ("rho", rho))
    batch = _check_qp("box_qp_solve", solver, nx, nu, N, None, named, iters, adj_iters)
    return _AdmmQpSolve.apply(_BOX, solver, (nx, nu, N), batch, int(iters), int(adj_iters), tol, max_iter, G, C, g, c, None, lo, hi, None, rho)


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
    named = (("G", G), ("C", C), ("g", g), ("c", c), ("E", E), ("lo", lo), ("hi", hi), ("rho", rho))
    batch = _check_qp("lin_qp_solve", solver, nx, nu, N, (mx, mu), named, iters, adj_iters)
    return _AdmmQpSolve.apply(_LIN, solver, (nx, nu, mx, mu, N), batch, int(iters), int(adj_iters), tol, max_iter, G, C, g, c, E, lo, hi, None,
                              rho)


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
    named = (("G", G), ("C", C), ("g", g), ("c", c), ("lo", lo), ("hi", hi), ("kappa", kappa), ("rho", rho))
    batch = _check_qp("soft_box_qp_solve", solver, nx, nu, N, None, named, iters, adj_iters)
    return _AdmmQpSolve.apply(_SOFT_BOX, solver, (nx, nu, N), batch, int(iters), int(adj_iters), tol, max_iter, G, C, g, c, None, lo, hi, kappa,
                              rho)


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
    named = (("G", G), ("C", C), ("g", g), ("c", c), ("E", E), ("lo", lo), ("hi", hi), ("kappa", kappa), ("rho", rho))
    batch = _check_qp("soft_lin_qp_solve", solver, nx, nu, N, (mx, mu), named, iters, adj_iters)
    return _AdmmQpSolve.apply(_SOFT_LIN, solver, (nx, nu, mx, mu, N), batch, int(iters), int(adj_iters), tol, max_iter, G, C, g, c, E, lo, hi,
                              kappa, rho)


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
