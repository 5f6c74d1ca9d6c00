// api_kkt.hip -- the KKT side of the C ABI (include/gbdpcg.h): the single launches around the solve (formation, gamma, recovery,
// residual, the ADMM updates, the gradient launch) and the calls composed of them and the solve of api_solve.hip -- kkt_step,
// kkt_resolve, the ADMM steps, the backward pass, with their _shared and _reg forms and their graphs.  Host code only.
#include "api_context.hpp"

#include <limits>

#ifndef GBDPCG_KKT_SKIP_L
#define GBDPCG_KKT_SKIP_L 1   // 0: the stair kernel of gbdpcg_kkt_step_* reads and compares L_{k+1} like everywhere else (A/B runs)
#endif

using namespace gbdpcg;

namespace {

// ---- the single launches
// (reg: gbdpcg_form_schur_reg_* -- problem b is formed from G_b + rho_b I, d_rho [batch] on the device, required)
template <typename T>
gbdpcg_status form_schur_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_G, const T *d_C,
                              const T *d_g, const T *d_c, T *d_S, T *d_gamma, T *d_Ginv, void *stream, const T *d_rho = nullptr, bool reg = false)
{
    if (!h || !d_G || !d_g || !d_c || !d_S || !d_gamma || (!d_C && N > 1) || nu == 0 || !shape_ok(nx, N, batch) || (reg && !d_rho))
        return GBDPCG_ERR_INVALID;
    if (!schur_shape_ok<T>(h->dev, nx, nu)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_form_schur<T>(h->dev, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_S, d_gamma, d_Ginv, (hipStream_t)stream,
                                    reg ? d_rho : nullptr));
    return GBDPCG_OK;
}
// (shared, the next two: d_Ginv and d_C are one problem's blocks, used by every problem of the batch)
template <typename T>
gbdpcg_status recover_primal_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_Ginv,
                                  const T *d_C, const T *d_g, const T *d_lambda, T *d_z, void *stream, bool shared = false)
{
    if (!h || !d_Ginv || !d_g || !d_lambda || !d_z || (!d_C && N > 1) || nu == 0 || !shape_ok(nx, N, batch))
        return GBDPCG_ERR_INVALID;
    if (!schur_shape_ok<T>(h->dev, nx, nu)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_recover_primal<T>(h->dev, nx, nu, N, batch, d_Ginv, d_C, d_g, d_lambda, d_z, (hipStream_t)stream, shared));
    return GBDPCG_OK;
}
template <typename T>
gbdpcg_status form_gamma_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_Ginv, const T *d_C,
                              const T *d_g, const T *d_c, T *d_gamma, void *stream, bool shared = false)
{
    if (!h || !d_Ginv || !d_g || !d_c || !d_gamma || (!d_C && N > 1) || nu == 0 || !shape_ok(nx, N, batch))
        return GBDPCG_ERR_INVALID;
    if (!schur_shape_ok<T>(h->dev, nx, nu)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_form_gamma<T>(h->dev, nx, nu, N, batch, d_Ginv, d_C, d_g, d_c, d_gamma, (hipStream_t)stream, shared));
    return GBDPCG_OK;
}
template <typename T>
gbdpcg_status kkt_residual_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_G, const T *d_C,
                                const T *d_g, const T *d_c, const T *d_z, const T *d_lambda, T *d_res, void *stream, bool shared,
                                const T *d_rho = nullptr, bool reg = false)   // reg: the stationarity of G_b + rho_b I
{
    if (!h || !d_G || !d_g || !d_c || !d_z || !d_lambda || !d_res || (!d_C && N > 1) || nu == 0 || !shape_ok(nx, N, batch) ||
        (reg && !d_rho))
        return GBDPCG_ERR_INVALID;
    if (!schur_shape_ok<T>(h->dev, nx, nu)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_kkt_residual<T>(h->dev, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_res, (hipStream_t)stream, shared,
                                      reg ? d_rho : nullptr));
    return GBDPCG_OK;
}

// The set and the splitting state of the gbdpcg_admm*_step_* calls: rho [batch], res [2 batch].  Box (gbdpcg_admm_step_*): mx = mu = 0
// and no E, every array has the layout of g.  rows (gbdpcg_admm_lin_step_*): the bounds are on E z -- lo, hi, w, y have the layout
// of the rows, E is one problem's in the shared form.  cones (gbdpcg_admm_soc_step_*, with rows): the rows behind the first lx / lu
// of a block are cones of dimension qx / qu, lo holds their offsets.  soft (gbdpcg_admm_soft_*, gbdpcg_admm_lin_soft_*): the bounds are
// L1-penalised with the weights kappa, which have the layout of lo; a hard family leaves kappa null, a soft one is refused without it.
template <typename T> struct AdmmOperands {
    const T *lo, *hi, *rho;
    T *w, *y, *gt, *res;
    bool rows = false;
    const T *E = nullptr;
    uint32_t mx = 0, mu = 0;
    const RowClasses *cones = nullptr;
    const T *kappa = nullptr;
    bool soft = false;
    bool adjoint = false;   // gbdpcg_admm_adjoint_*, gbdpcg_admm_lin_adjoint_*: hard bounds, lo (and hi) hold yf, the forward y -- the mask
};

// The forward point and the outputs of gbdpcg_kkt_backward_*: z has the layout of g, lambda that of c, gG / gC those of G / C (one
// problem's worth in the shared form; either may be null).
template <typename T> struct GradOperands {
    const T *z, *lambda;
    T *gG, *gC;
};
// What the composite calls take next to the solve (PcgArgs, whose n is nx): the blocks read by the gamma launch before it and by
// the recovery launch behind it.  z has the layout of g.  shared: Ginv and C (and the solve's S, Pinv) are ONE problem's.
template <typename T> struct KktOperands {
    uint32_t nu;
    const T *Ginv, *C, *g, *c;
    T *gamma, *z;   // gamma: written in front of the solve, which reads the same array as a.gamma
    bool shared = false;
};

// What gbdpcg_kkt_step_* forms before its solve next to gamma: S and G^-1 from G (and C, g, c), Phi^-1 from that S.  The solve
// reads the same S and Pinv through its PcgArgs.  reg (gbdpcg_kkt_step_reg_*): the step of G_b + rho_b I, rho [batch] on the device.
template <typename T> struct KktFormed {
    const T *G;
    T *S, *Ginv, *Pinv;
    gbdpcg_pinv_kind kind;
    const T *rho = nullptr;
    bool reg = false;
};

// What gbdpcg_kkt_step_* refuses before anything runs.  The eager call has only ever looked at Ginv and z here (the parts refuse
// the rest in their turn, the formation having run by then); capture: the graph-create entry also asks for what the formation and
// the stair kernel write and for the kind, before it reserves anything.
template <typename T> gbdpcg_status kkt_step_refusal(const KktFormed<T> &f, const KktOperands<T> &k, bool capture)
{
    if (!f.Ginv || !k.z) return GBDPCG_ERR_INVALID;
    if (capture && ((f.reg && !f.rho) || !f.S || !k.gamma || !f.Pinv || (int)f.kind < 0 || (int)f.kind > 2)) return GBDPCG_ERR_INVALID;
    return GBDPCG_OK;
}

// KKT blocks -> S, gamma, G^-1 -> Phi^-1 -> PCG -> primal step, on one stream (capturable: no allocation after the first
// call of a shape, no synchronisation).
template <typename T>
gbdpcg_status kkt_step_impl(gbdpcg_handle_t h, const KktFormed<T> &f, const KktOperands<T> &k, const PcgArgs<T> &a, hipStream_t stream)
{
    const uint32_t nx = a.n, N = a.N, batch = a.batch;
    gbdpcg_status st = kkt_step_refusal<T>(f, k, false);
    if (st != GBDPCG_OK) return st;
    st = form_schur_impl<T>(h, nx, k.nu, N, batch, f.G, k.C, k.g, k.c, f.S, k.gamma, f.Ginv, stream, f.rho, f.reg);
    if (st != GBDPCG_OK) return st;
    // (the regularised formation adds rho_b to a block before BOTH of its uses, so what follows holds for it unchanged)
    // form_schur writes S exactly symmetric in storage (R_k and L_{k+1} are copies of the same registers), and where the
    // one-launch stair kernel forms Pinv from such an S it writes every pair as mirror images: in the default symmetric mode
    // the verdicts of gbdpcg_form_pinv_solve_* would all read "symmetric", so they are neither written nor read here and the
    // general-storage launch that would own nothing (11 us of a 0.66 ms step) is not made.  Same kernels on the same numbers:
    // same results as the three calls.
    bool known = false;
    {
        DEVICE_SCOPE(h);        known = f.S && f.Pinv && shape_ok(nx, N, batch) && mappable<T>(nx) && (int)f.kind >= 0 && (int)f.kind <= 2 && h->symmetric == 2 &&
                pick_path<T>(h, nx, N, batch) == GBDPCG_PATH_FUSED && fused_has_symmetric<T>(h->dev, nx, N, batch) &&
                pinv_verdict_chunks<T>(nx, N, (int)f.kind) != 0;
    }
    if (known) {
        if (!a.gamma || !a.lambda || !a.iters) return GBDPCG_ERR_INVALID;
        DEVICE_SCOPE(h);
        HIP_TRY(h, launch_form_pinv<T>(h->dev, nx, N, batch, f.S, f.Pinv, (int)f.kind, stream, nullptr, GBDPCG_KKT_SKIP_L != 0));
        SolveOpts o;
        o.known_symmetric = true;
        st = solve<T>(h, a, stream, o);
    } else {
        st = form_pinv_solve<T>(h, a, f.Pinv, f.kind, stream);
    }
    if (st != GBDPCG_OK) return st;
    return recover_primal_impl<T>(h, nx, k.nu, N, batch, f.Ginv, k.C, k.g, a.lambda, k.z, stream);
}

// What gbdpcg_kkt_resolve_* refuses before anything is written.  eager: the direct call has always answered a shape the shared
// solve cannot take in front of the arguments its gamma launch looks at; the graph-create entry leaves that shape to graph_create,
// which answers it before it reserves anything.  (The limits of the solve itself -- mappable -- are met behind the gamma launch.)
template <typename T> gbdpcg_status kkt_resolve_refusal(gbdpcg_handle_t h, const KktOperands<T> &k, const PcgArgs<T> &a, bool eager)
{
    if (!h || !a.S || !a.lambda || !a.iters || !k.z) return GBDPCG_ERR_INVALID;
    if (eager && k.shared && shape_ok(a.n, a.N, a.batch) && mappable<T>(a.n) && !fused_fits<T>(h->dev, a.n, a.N))
        return GBDPCG_ERR_UNSUPPORTED;
    if (!k.Ginv || !k.g || !k.c || !k.gamma || (!k.C && a.N > 1) || k.nu == 0 || !shape_ok(a.n, a.N, a.batch)) return GBDPCG_ERR_INVALID;
    return schur_shape_ok<T>(h->dev, a.n, k.nu) ? GBDPCG_OK : GBDPCG_ERR_UNSUPPORTED;
}

// The step for a linearisation that is kept (G, C unchanged since the gbdpcg_kkt_step_* or gbdpcg_form_schur_* that wrote S, Pinv
// and G^-1): gamma from the new g and c, the ordinary solve on the caller's S and Pinv, the primal step.  The library cannot know
// that S was left alone, so the solve is told nothing about its symmetry: the handle's mode decides, as in gbdpcg_solve_*.
template <typename T>
gbdpcg_status kkt_resolve_impl(gbdpcg_handle_t h, const KktOperands<T> &k, const PcgArgs<T> &a, hipStream_t stream)
{
    gbdpcg_status st = kkt_resolve_refusal<T>(h, k, a, true);
    if (st != GBDPCG_OK) return st;
    st = form_gamma_impl<T>(h, a.n, k.nu, a.N, a.batch, k.Ginv, k.C, k.g, k.c, k.gamma, stream, k.shared);
    if (st != GBDPCG_OK) return st;
    SolveOpts o;
    o.shared = k.shared;
    st = solve<T>(h, a, stream, o);
    if (st != GBDPCG_OK) return st;
    return recover_primal_impl<T>(h, a.n, k.nu, a.N, a.batch, k.Ginv, k.C, k.g, a.lambda, k.z, stream, k.shared);
}

// The splitting update (admm.hip), one launch.  init: gbdpcg_admm_init_* -- d_z and d_res are not arguments.  No shape is refused:
// the kernel is elementwise over the layout of g.  soft: the gbdpcg_admm_soft_* calls, which need d_kappa.
template <typename T>
gbdpcg_status admm_update_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_g, const T *d_lo,
                               const T *d_hi, const T *d_rho, const T *d_z, T *d_w, T *d_y, T *d_gt, T *d_res, void *stream, bool init,
                               const T *d_kappa = nullptr, bool soft = false)
{
    if (!h || !d_g || !d_lo || !d_hi || !d_rho || !d_w || !d_y || !d_gt || (!init && (!d_z || !d_res)) || nx == 0 || nu == 0 ||
        N == 0 || batch == 0 || (soft && !d_kappa))
        return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_update<T>(nx, nu, N, batch, d_g, d_lo, d_hi, d_rho, d_z, d_w, d_y, d_gt, d_res, (hipStream_t)stream, init,
                                     soft ? d_kappa : nullptr));
    return GBDPCG_OK;
}

// The adjoint of that update (the backward pass of the hard box QP: the forward y, yf, where lo, hi stand), one launch.  init:
// gbdpcg_admm_adjoint_init_* -- d_az and d_res are not arguments.  Elementwise: no shape is refused.
template <typename T>
gbdpcg_status admm_adjoint_update_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_gz,
                                       const T *d_yf, const T *d_rho, const T *d_az, T *d_wa, T *d_ya, T *d_gta, T *d_res, void *stream,
                                       bool init)
{
    if (!h || !d_gz || !d_yf || !d_rho || !d_wa || !d_ya || !d_gta || (!init && (!d_az || !d_res)) || nx == 0 || nu == 0 || N == 0 ||
        batch == 0)
        return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_adjoint_update<T>(nx, nu, N, batch, d_gz, d_yf, d_rho, d_az, d_wa, d_ya, d_gta, d_res, (hipStream_t)stream, init));
    return GBDPCG_OK;
}

// What the stage-wise rows of gbdpcg_admm_lin_* and gbdpcg_admm_soc_* are refused for, before anything is written.  INVALID: no
// rows at all (mx = mu = 0, or mx = 0 with N = 1), row classes that do not fit the blocks (lx > mx, lu > mu, cone rows with q = 0
// or not a whole number of cones).  UNSUPPORTED, behind every INVALID: more than 64 rows per block, a knot that does not fit the
// update kernel's LDS.
template <typename T> gbdpcg_status admm_rows_status(uint32_t nx, uint32_t nu, const AdmmOperands<T> &a, uint32_t N)
{
    if (((uint64_t)a.mx + a.mu) * N == a.mu || (a.cones && !admm_rows_classes_ok(a.mx, a.mu, *a.cones))) return GBDPCG_ERR_INVALID;
    return admm_rows_shape_ok<T>(nx, nu, a.mx, a.mu) ? GBDPCG_OK : GBDPCG_ERR_UNSUPPORTED;
}

// Gt = G + rho E'E (admm_rows.hip), one launch; d_Gt may be d_G.
template <typename T>
gbdpcg_status admm_lin_form_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch,
                                 const T *d_G, const T *d_E, const T *d_rho, T *d_Gt, void *stream)
{
    if (!h || !d_G || !d_E || !d_rho || !d_Gt || nx == 0 || nu == 0 || N == 0 || batch == 0) return GBDPCG_ERR_INVALID;
    AdmmOperands<T> a{};
    a.mx = mx, a.mu = mu;
    const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
    if (st != GBDPCG_OK) return st;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_lin_form<T>(nx, nu, mx, mu, N, batch, d_G, d_E, d_rho, d_Gt, (hipStream_t)stream));
    return GBDPCG_OK;
}

// The splitting update for the rows of a (admm_rows.hip; with a.cones its CONES kernel), one launch.  init: gbdpcg_admm_lin_init_*,
// gbdpcg_admm_soc_init_* -- d_z and a.res are not arguments.
template <typename T>
gbdpcg_status admm_rows_update_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_g,
                                    const AdmmOperands<T> &a, const T *d_z, void *stream, bool init, bool shared = false)
{
    if (!h || !d_g || !a.E || !a.lo || !a.hi || !a.rho || !a.w || !a.y || !a.gt || (!init && (!d_z || !a.res)) || nx == 0 ||
        nu == 0 || N == 0 || batch == 0 || (a.soft && (!a.kappa || a.cones)) || (a.adjoint && (a.soft || a.cones || shared)))
        return GBDPCG_ERR_INVALID;
    const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
    if (st != GBDPCG_OK) return st;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_rows_update<T>(nx, nu, a.mx, a.mu, N, batch, d_g, a.E, a.lo, a.hi, a.rho, d_z, a.w, a.y, a.gt, a.res,
                                          (hipStream_t)stream, init, shared, a.cones, a.soft ? a.kappa : nullptr, a.adjoint));
    return GBDPCG_OK;
}

// What one ADMM iteration (admm_step_impl) is refused for, before anything is written, reserved or captured: whatever the solve or
// the update would refuse for its arguments or the shape, every INVALID before every UNSUPPORTED.  solve_limits: with the limits of
// the solve itself (mappable, fused_fits).  The graph-create entries pass false and leave those to graph_create and the
// capture, which answer them behind the reservation of the handle's workspaces: the entry points have always differed there.
template <typename T>
gbdpcg_status admm_step_refusal(gbdpcg_handle_t h, const KktOperands<T> &k, const AdmmOperands<T> &a, const PcgArgs<T> &p,
                                bool solve_limits = true)
{
    if (!h || !k.Ginv || !k.g || !k.c || !a.lo || !a.hi || !a.rho || !p.S || !p.gamma || !p.lambda || !p.iters || !k.z || !a.w ||
        !a.y || !a.gt || !a.res || (!k.C && p.N > 1) || k.nu == 0 || !shape_ok(p.n, p.N, p.batch) || (a.rows && !a.E) ||
        (a.soft && (!a.kappa || a.cones)))
        return GBDPCG_ERR_INVALID;
    const gbdpcg_status rows = a.rows ? admm_rows_status<T>(p.n, k.nu, a, p.N) : GBDPCG_OK;
    if (rows == GBDPCG_ERR_INVALID) return rows;
    if (!schur_shape_ok<T>(h->dev, p.n, k.nu) || rows != GBDPCG_OK) return GBDPCG_ERR_UNSUPPORTED;
    if (solve_limits && (!mappable<T>(p.n) || (k.shared && !fused_fits<T>(h->dev, p.n, p.N)))) return GBDPCG_ERR_UNSUPPORTED;
    return GBDPCG_OK;
}

// One iteration of ADMM on a kept factorisation of G + rho I (box) or G + rho E'E (rows): kkt_resolve_impl with the shifted
// gradient a.gt in the place of g (the gamma launch and the recovery launch read the same gt), then the update, which alone reads
// k.g, on the same stream.  a.adjoint: the adjoint iteration -- k.g is gz, k.c is nglam, k.z is az, a.lo is yf (a.hi too: the refusal
// of the step is the refusal there), a.w, a.y, a.gt, a.res the adjoint's splitting state.
template <typename T>
gbdpcg_status admm_step_impl(gbdpcg_handle_t h, const KktOperands<T> &k, const AdmmOperands<T> &a, const PcgArgs<T> &p, hipStream_t stream)
{
    gbdpcg_status st = admm_step_refusal<T>(h, k, a, p);
    if (st != GBDPCG_OK) return st;
    KktOperands<T> shifted = k;
    shifted.g = a.gt;
    st = kkt_resolve_impl<T>(h, shifted, p, stream);
    if (st != GBDPCG_OK) return st;
    if (a.rows) return admm_rows_update_impl<T>(h, p.n, k.nu, p.N, p.batch, k.g, a, k.z, stream, false, k.shared);
    if (a.adjoint) return admm_adjoint_update_impl<T>(h, p.n, k.nu, p.N, p.batch, k.g, a.lo, a.rho, k.z, a.w, a.y, a.gt, a.res, stream, false);
    return admm_update_impl<T>(h, p.n, k.nu, p.N, p.batch, k.g, a.lo, a.hi, a.rho, k.z, a.w, a.y, a.gt, a.res, stream, false, a.kappa,
                               a.soft);
}

// ---- the gradient launches of the backward passes (admm_box_grad.hip, admm_lin_grad.hip)
// The gradients in the bounds from the adjoint's y, one launch, elementwise.
template <typename T>
gbdpcg_status admm_grad_bounds_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_yf, const T *d_rho,
                                    const T *d_ya, T *d_glo, T *d_ghi, void *stream)
{
    if (!h || !d_yf || !d_rho || !d_ya || !d_glo || !d_ghi || nx == 0 || nu == 0 || N == 0 || batch == 0) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_grad_bounds<T>(nx, nu, N, batch, d_yf, d_rho, d_ya, d_glo, d_ghi, (hipStream_t)stream));
    return GBDPCG_OK;
}

// The gradients in the rows of the hard linear-row QP (admm_lin_grad.hip), one launch: glo, ghi in the layout of the rows, gE in that
// of E, each may be null, not all three.  The refusals of the rows family.
template <typename T>
gbdpcg_status admm_lin_grad_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch,
                                 const T *d_z, const T *d_az, const T *d_yf, const T *d_ya, const T *d_rho, T *d_glo, T *d_ghi, T *d_gE,
                                 void *stream)
{
    if (!h || !d_z || !d_az || !d_yf || !d_ya || !d_rho || (!d_glo && !d_ghi && !d_gE) || nx == 0 || nu == 0 || N == 0 || batch == 0)
        return GBDPCG_ERR_INVALID;
    AdmmOperands<T> a{};
    a.mx = mx, a.mu = mu;
    const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
    if (st != GBDPCG_OK) return st;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_lin_grad<T>(nx, nu, mx, mu, N, batch, d_z, d_az, d_yf, d_ya, d_rho, d_glo, d_ghi, d_gE, (hipStream_t)stream));
    return GBDPCG_OK;
}

// ---- the backward pass of the soft box and rows QPs (admm_box_grad.hip, the SOFT instantiation of admm_lin_grad.hip): the mask
// that turns the forward y into the yf of the hard adjoint loops above, and the gradient launches that know of kappa.
// The mask, one launch, elementwise.  rows: (mx, mu) and the rows' refusals; otherwise the layout of g.  d_ym == d_yf is refused
// here, in front of everything else that could be: the unmasked yf is still needed behind the adjoint loop.
template <typename T>
gbdpcg_status admm_soft_mask_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch,
                                  const T *d_yf, const T *d_kappa, const T *d_rho, T *d_ym, void *stream, bool rows)
{
    if (!h || !d_yf || !d_kappa || !d_rho || !d_ym || d_ym == d_yf || nx == 0 || nu == 0 || N == 0 || batch == 0)
        return GBDPCG_ERR_INVALID;
    uint64_t len = ((uint64_t)nx + nu) * N - nu;
    if (rows) {
        AdmmOperands<T> a{};
        a.mx = mx, a.mu = mu;
        const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
        if (st != GBDPCG_OK) return st;
        len = ((uint64_t)mx + mu) * N - mu;
    }
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_soft_mask<T>(len, batch, d_yf, d_kappa, d_rho, d_ym, (hipStream_t)stream));
    return GBDPCG_OK;
}

// dl/dlo, dl/dhi, dl/dkappa of the soft box, one launch, elementwise; each output may be null, not all three.
template <typename T>
gbdpcg_status admm_soft_grad_bounds_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_yf,
                                         const T *d_kappa, const T *d_rho, const T *d_ya, const T *d_az, T *d_glo, T *d_ghi,
                                         T *d_gkappa, void *stream)
{
    if (!h || !d_yf || !d_kappa || !d_rho || !d_ya || !d_az || (!d_glo && !d_ghi && !d_gkappa) || nx == 0 || nu == 0 || N == 0 ||
        batch == 0)
        return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_soft_grad_bounds<T>(nx, nu, N, batch, d_yf, d_kappa, d_rho, d_ya, d_az, d_glo, d_ghi, d_gkappa,
                                               (hipStream_t)stream));
    return GBDPCG_OK;
}

// dl/dlo, dl/dhi, dl/dkappa, dl/dE of the soft rows, one launch; each output may be null, not all four.  The refusals of the rows
// family.
template <typename T>
gbdpcg_status admm_lin_soft_grad_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch,
                                      const T *d_z, const T *d_az, const T *d_E, const T *d_yf, const T *d_ya, const T *d_kappa,
                                      const T *d_rho, T *d_glo, T *d_ghi, T *d_gkappa, T *d_gE, void *stream)
{
    if (!h || !d_z || !d_az || !d_E || !d_yf || !d_ya || !d_kappa || !d_rho || (!d_glo && !d_ghi && !d_gkappa && !d_gE) || nx == 0 ||
        nu == 0 || N == 0 || batch == 0)
        return GBDPCG_ERR_INVALID;
    AdmmOperands<T> a{};
    a.mx = mx, a.mu = mu;
    const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
    if (st != GBDPCG_OK) return st;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_lin_grad<T>(nx, nu, mx, mu, N, batch, d_z, d_az, d_yf, d_ya, d_rho, d_glo, d_ghi, d_gE, (hipStream_t)stream,
                                       d_E, d_kappa, d_gkappa));
    return GBDPCG_OK;
}

// ---- the primal infeasibility certificate of the hard box and rows paths (admm_infeas.hip), one launch, no handle state.  box: no
// E, no (mx, mu).  The two iterates must be two: lambda0 == lambda1 or y0 == y1 is refused with the null pointers.  The rows: the
// refusals of the rows family, then the kernel's own knot (it stages [A | B] next to E).
template <typename T>
gbdpcg_status admm_infeas_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch,
                               const T *d_C, const T *d_c, const T *d_E, const T *d_lo, const T *d_hi, const T *d_rho,
                               const T *d_lambda0, const T *d_lambda1, const T *d_y0, const T *d_y1, T eps, T *d_cert, uint8_t *d_flag,
                               void *stream, bool box, bool shared)
{
    if (!h || !d_c || (!box && !d_E) || !d_lo || !d_hi || !d_rho || !d_lambda0 || !d_lambda1 || !d_y0 || !d_y1 || !d_cert ||
        (!d_C && N > 1) || nx == 0 || nu == 0 || N == 0 || batch == 0 || d_lambda0 == d_lambda1 || d_y0 == d_y1)
        return GBDPCG_ERR_INVALID;
    if (!box) {
        AdmmOperands<T> a{};
        a.mx = mx, a.mu = mu;
        const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
        if (st != GBDPCG_OK) return st;
    }
    if (!admm_infeas_shape_ok<T>(nx, nu, box ? nx : mx, box ? nu : mu, box)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_infeas<T>(nx, nu, mx, mu, N, batch, d_C, d_c, d_E, d_lo, d_hi, d_rho, d_lambda0, d_lambda1, d_y0, d_y1, eps,
                                     d_cert, d_flag, (hipStream_t)stream, box, shared));
    return GBDPCG_OK;
}

// ---- the optimality test of every ADMM family (admm_optimality.hip), one launch, no handle state.  box: no E, no (mx, mu).  The
// rows: the refusals of the rows family, then the kernel's own knot (it stages Q, R and [A | B] next to E).
template <typename T>
gbdpcg_status admm_optimality_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch,
                                   const T *d_G, const T *d_C, const T *d_g, const T *d_c, const T *d_E, const T *d_rho, const T *d_z,
                                   const T *d_lambda, const T *d_w, const T *d_y, T eps_abs, T eps_rel, T *d_opt, uint8_t *d_done,
                                   void *stream, bool box, bool shared)
{
    if (!h || !d_G || !d_g || !d_c || (!box && !d_E) || !d_rho || !d_z || !d_lambda || !d_w || !d_y || !d_opt || (!d_C && N > 1) ||
        nx == 0 || nu == 0 || N == 0 || batch == 0)
        return GBDPCG_ERR_INVALID;
    if (!box) {
        AdmmOperands<T> a{};
        a.mx = mx, a.mu = mu;
        const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
        if (st != GBDPCG_OK) return st;
    }
    if (!admm_optimality_shape_ok<T>(nx, nu, box ? nx : mx, box ? nu : mu, box)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_optimality<T>(nx, nu, mx, mu, N, batch, d_G, d_C, d_g, d_c, d_E, d_rho, d_z, d_lambda, d_w, d_y, eps_abs,
                                         eps_rel, d_opt, d_done, (hipStream_t)stream, box, shared));
    return GBDPCG_OK;
}

// ---- adaptive rho (admm_rebalance.hip): residual balancing in powers of two, and the iteration that refactors with the new rho
// The rule of gbdpcg_admm*_rebalance_* and what it writes next to y: rho [batch] in place, expo [batch].
template <typename T> struct RhoRule {
    T ratio;
    uint32_t shift;
    T rho_min, rho_max;
    T *rho;
    int32_t *expo;
};
// (comparisons: a NaN among ratio, rho_min, rho_max is refused; rho_min is finite where rho_max is)
template <typename T> bool rho_rule_ok(const RhoRule<T> &r)
{
    return r.rho && r.expo && r.shift >= 1 && r.shift <= 16 && r.ratio >= T(1) && r.rho_min > T(0) && r.rho_min <= r.rho_max &&
           r.rho_max <= std::numeric_limits<T>::max();
}

// The box form, one launch: rho, y, expo and the gt that gbdpcg_admm_init_* would rebuild.  Elementwise: no shape is refused.
template <typename T>
gbdpcg_status admm_rebalance_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_g, const T *d_res,
                                  const T *d_w, T *d_y, T *d_gt, const RhoRule<T> &rule, void *stream)
{
    if (!h || !d_g || !d_res || !d_w || !d_y || !d_gt || nx == 0 || nu == 0 || N == 0 || batch == 0 || !rho_rule_ok<T>(rule))
        return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_admm_rebalance<T>(((uint64_t)nx + nu) * N - nu, batch, d_g, d_res, rule.rho, d_w, d_y, d_gt, rule.ratio, rule.shift,
                                        rule.rho_min, rule.rho_max, rule.expo, (hipStream_t)stream, true));
    return GBDPCG_OK;
}

// The rows form (admm_lin, admm_soc, admm_lin_soft): rho, y over the rows of a, expo; then the family's init launch rebuilds gt (and
// re-projects w; the soft init clips only the rows with kappa = +Inf).
// a.rho is rule.rho.  Whatever the init launch refuses is refused here before the first launch.
template <typename T>
gbdpcg_status admm_rows_rebalance_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_g,
                                       const AdmmOperands<T> &a, const RhoRule<T> &rule, void *stream)
{
    if (!h || !d_g || !a.E || !a.lo || !a.hi || !a.res || !a.w || !a.y || !a.gt || nx == 0 || nu == 0 || N == 0 || batch == 0 ||
        !rho_rule_ok<T>(rule) || (a.soft && (!a.kappa || a.cones)))
        return GBDPCG_ERR_INVALID;
    const gbdpcg_status st = admm_rows_status<T>(nx, nu, a, N);
    if (st != GBDPCG_OK) return st;
    {
        DEVICE_SCOPE(h);
        HIP_TRY(h, launch_admm_rebalance<T>(((uint64_t)a.mx + a.mu) * N - a.mu, batch, nullptr, a.res, rule.rho, nullptr, a.y, nullptr,
                                            rule.ratio, rule.shift, rule.rho_min, rule.rho_max, rule.expo, (hipStream_t)stream, false));
    }
    return admm_rows_update_impl<T>(h, nx, nu, N, batch, d_g, a, nullptr, stream, true);
}

// What gbdpcg_admm*_restep_* refactors with next to the rule: the original G, and for the families with rows the Gt = G + rho E'E
// that is formed from it (null for the box, whose formation adds rho I itself).
template <typename T> struct Refactor {
    const T *G;
    T *Gt;
    T *S, *Ginv, *Pinv;
    gbdpcg_pinv_kind kind;
    KktFormed<T> formed(const AdmmOperands<T> &a) const
    {
        if (a.rows) return KktFormed<T>{Gt, S, Ginv, Pinv, kind};
        return KktFormed<T>{G, S, Ginv, Pinv, kind, a.rho, true};
    }
};

// What gbdpcg_admm*_restep_* refuses before anything is written, reserved or captured: whatever the rebalance, the formation, the
// step of kkt_step_* (as its graph form asks: everything it writes, and the kind) or the iteration would refuse, every INVALID
// before every UNSUPPORTED.  The families with rows need a Gt of their own: the next restep forms from the original G again.
template <typename T>
gbdpcg_status admm_restep_refusal(gbdpcg_handle_t h, const Refactor<T> &f, const KktOperands<T> &k, const AdmmOperands<T> &a,
                                  const RhoRule<T> &rule, const PcgArgs<T> &p, bool solve_limits)
{
    if (!rho_rule_ok<T>(rule) || !f.G || (a.rows && (!f.Gt || f.Gt == f.G)) || kkt_step_refusal<T>(f.formed(a), k, true) != GBDPCG_OK)
        return GBDPCG_ERR_INVALID;
    return admm_step_refusal<T>(h, k, a, p, solve_limits);
}

// One iteration with a new rho, on one stream: rebalance (rho, y, gt, expo), the formation and the solve of kkt_step_impl with a.gt
// in the place of g -- on G with rho (box) or on Gt = G + rho E'E formed here (rows) --, then the family's update.
template <typename T>
gbdpcg_status admm_restep_impl(gbdpcg_handle_t h, const Refactor<T> &f, const KktOperands<T> &k, const AdmmOperands<T> &a,
                               const RhoRule<T> &rule, const PcgArgs<T> &p, hipStream_t stream)
{
    gbdpcg_status st = admm_restep_refusal<T>(h, f, k, a, rule, p, true);
    if (st != GBDPCG_OK) return st;
    const uint32_t nx = p.n, N = p.N, batch = p.batch;
    if (a.rows) {
        st = admm_rows_rebalance_impl<T>(h, nx, k.nu, N, batch, k.g, a, rule, stream);
        if (st != GBDPCG_OK) return st;
        st = admm_lin_form_impl<T>(h, nx, k.nu, a.mx, a.mu, N, batch, f.G, a.E, a.rho, f.Gt, stream);
    } else {
        st = admm_rebalance_impl<T>(h, nx, k.nu, N, batch, k.g, a.res, a.w, a.y, a.gt, rule, stream);
    }
    if (st != GBDPCG_OK) return st;
    KktOperands<T> shifted = k;
    shifted.g = a.gt;
    st = kkt_step_impl<T>(h, f.formed(a), shifted, p, stream);
    if (st != GBDPCG_OK) return st;
    if (a.rows) return admm_rows_update_impl<T>(h, nx, k.nu, N, batch, k.g, a, k.z, stream, false);
    return admm_update_impl<T>(h, nx, k.nu, N, batch, k.g, a.lo, a.hi, a.rho, k.z, a.w, a.y, a.gt, a.res, stream, false, a.kappa, a.soft);
}

// The gradient launch (kkt_grad.hip), no handle state.  shared: gG, gC are one problem's worth, summed over the batch.
template <typename T>
gbdpcg_status kkt_grad_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const T *d_z, const T *d_lambda,
                            const T *d_az, const T *d_alambda, T *d_gG, T *d_gC, void *stream, bool shared)
{
    if (!h || !d_z || !d_lambda || !d_az || !d_alambda || (!d_gG && !d_gC) || nu == 0 || !shape_ok(nx, N, batch))
        return GBDPCG_ERR_INVALID;
    if (!schur_shape_ok<T>(h->dev, nx, nu)) return GBDPCG_ERR_UNSUPPORTED;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_kkt_grad<T>(nx, nu, N, batch, d_z, d_lambda, d_az, d_alambda, d_gG, d_gC, (hipStream_t)stream, shared));
    return GBDPCG_OK;
}

// What gbdpcg_kkt_backward_* refuses before anything is written, reserved or captured: whatever either part would refuse.
// solve_limits: with the limits of the solve itself (mappable, fused_fits); the graph-create entries pass false and leave those to
// graph_create and the capture, as the ADMM entries do.
template <typename T>
gbdpcg_status kkt_backward_refusal(gbdpcg_handle_t h, const KktOperands<T> &k, const GradOperands<T> &f, const PcgArgs<T> &a,
                                   bool solve_limits)
{
    if (!h || !k.Ginv || !k.g || !k.c || !a.S || !a.gamma || !f.z || !f.lambda || !k.z || !a.lambda || !a.iters || (!f.gG && !f.gC) ||
        (!k.C && a.N > 1) || k.nu == 0 || !shape_ok(a.n, a.N, a.batch))
        return GBDPCG_ERR_INVALID;
    if (!schur_shape_ok<T>(h->dev, a.n, k.nu)) return GBDPCG_ERR_UNSUPPORTED;
    if (solve_limits && (!mappable<T>(a.n) || (k.shared && !fused_fits<T>(h->dev, a.n, a.N)))) return GBDPCG_ERR_UNSUPPORTED;
    return GBDPCG_OK;
}

// The backward pass on a kept factorisation: the KKT matrix is symmetric, so the adjoint pair (az, alambda) is kkt_resolve_impl
// with the upstream gradient gz in the place of g and nglam = -dl/dlambda in the place of c (k.g, k.c; k.z is az, a.lambda is
// alambda, the warm start), and the gradient launch follows on the same stream.
template <typename T>
gbdpcg_status kkt_backward_impl(gbdpcg_handle_t h, const KktOperands<T> &k, const GradOperands<T> &f, const PcgArgs<T> &a,
                                hipStream_t stream)
{
    gbdpcg_status st = kkt_backward_refusal<T>(h, k, f, a, true);
    if (st != GBDPCG_OK) return st;
    st = kkt_resolve_impl<T>(h, k, a, stream);
    if (st != GBDPCG_OK) return st;
    return kkt_grad_impl<T>(h, a.n, k.nu, a.N, a.batch, f.z, f.lambda, k.z, a.lambda, f.gG, f.gC, stream, k.shared);
}

// ---- mixed-precision refinement (kkt_refine.hip): fp64 problem data and point, an fp32 solve on a kept fp32 factorisation
// The fp64 side of a refinement step: the problem, the point that is refined, and what the defect launch writes next to the
// right-hand side.  The fp32 side is a KktOperands<float> (g := rg, c := rc, z := dz) and the PcgArgs<float> of its solve.
// reg (gbdpcg_kkt_*_reg): the defect of G_b + rho_b I, rho [batch] fp64 on the device.  The shared forms set k.shared of the fp32
// side: G and C here are then one problem's too.
struct RefineOperands {
    const double *G, *C, *g, *c;
    double *z, *lambda, *res;
    int32_t *expo;
    float *rg, *rc;   // the right-hand side of the correction system: the g and the c of the fp32 side
    const double *rho = nullptr;
    bool reg = false;
};

// What the fp64 launches refuse: the rules of gbdpcg_kkt_residual_f64.
gbdpcg_status refine_shape_status(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch)
{
    if (nu == 0 || !shape_ok(nx, N, batch)) return GBDPCG_ERR_INVALID;
    return schur_shape_ok<double>(h->dev, nx, nu) ? GBDPCG_OK : GBDPCG_ERR_UNSUPPORTED;
}

gbdpcg_status kkt_defect_mixed_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                    const double *d_C, const double *d_g, const double *d_c, const double *d_z, const double *d_lambda,
                                    float *d_rg, float *d_rc, float *d_dlambda, int32_t *d_expo, double *d_res, void *stream,
                                    bool shared = false, const double *d_rho = nullptr, bool reg = false)
{
    if (!h || !d_G || !d_g || !d_c || !d_z || !d_lambda || !d_rg || !d_rc || !d_expo || !d_res || (!d_C && N > 1) || (reg && !d_rho))
        return GBDPCG_ERR_INVALID;
    const gbdpcg_status st = refine_shape_status(h, nx, nu, N, batch);
    if (st != GBDPCG_OK) return st;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_kkt_defect_mixed(h->dev, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_rg, d_rc, d_dlambda, d_expo, d_res,
                                       (hipStream_t)stream, shared, reg ? d_rho : nullptr));
    return GBDPCG_OK;
}

gbdpcg_status kkt_refine_apply_impl(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_dz,
                                    const float *d_dlambda, const int32_t *d_expo, double *d_z, double *d_lambda, void *stream)
{
    if (!h || !d_dz || !d_dlambda || !d_expo || !d_z || !d_lambda) return GBDPCG_ERR_INVALID;
    const gbdpcg_status st = refine_shape_status(h, nx, nu, N, batch);
    if (st != GBDPCG_OK) return st;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_kkt_refine_apply(nx, nu, N, batch, d_dz, d_dlambda, d_expo, d_z, d_lambda, (hipStream_t)stream));
    return GBDPCG_OK;
}

// What gbdpcg_kkt_refine_step refuses before anything is written, reserved or captured: whatever one of its three parts would
// refuse, every INVALID before every UNSUPPORTED.  solve_limits: as in admm_step_refusal.  The _reg and _shared forms come here too:
// a null rho where f.reg asks for one, and the one-workgroup limit of the shared solve.
gbdpcg_status refine_step_refusal(gbdpcg_handle_t h, const RefineOperands &f, const KktOperands<float> &k, const PcgArgs<float> &a,
                                  bool solve_limits)
{
    if (!h || !f.G || !f.g || !f.c || !f.z || !f.lambda || !f.expo || !f.res || (!f.C && a.N > 1) || !k.Ginv || !k.g || !k.c ||
        !k.gamma || !k.z || (!k.C && a.N > 1) || !a.S || !a.lambda || !a.iters || (f.reg && !f.rho))
        return GBDPCG_ERR_INVALID;
    gbdpcg_status st = refine_shape_status(h, a.n, k.nu, a.N, a.batch);
    if (st != GBDPCG_OK) return st;
    if (!schur_shape_ok<float>(h->dev, a.n, k.nu)) return GBDPCG_ERR_UNSUPPORTED;
    if (solve_limits && (!mappable<float>(a.n) || (k.shared && !fused_fits<float>(h->dev, a.n, a.N)))) return GBDPCG_ERR_UNSUPPORTED;
    return GBDPCG_OK;
}

// One refinement step: the defect of (z, lambda) in fp64 as the scaled fp32 right-hand side (k.g, k.c) and the zeroed start
// a.lambda, kkt_resolve_impl<float> on the kept factorisation, the fp64 accumulation of (k.z, a.lambda), on one stream.
gbdpcg_status kkt_refine_step_impl(gbdpcg_handle_t h, const RefineOperands &f, const KktOperands<float> &k, const PcgArgs<float> &a,
                                   hipStream_t stream)
{
    gbdpcg_status st = refine_step_refusal(h, f, k, a, true);
    if (st != GBDPCG_OK) return st;
    st = kkt_defect_mixed_impl(h, a.n, k.nu, a.N, a.batch, f.G, f.C, f.g, f.c, f.z, f.lambda, f.rg, f.rc, a.lambda, f.expo, f.res, stream,
                               k.shared, f.rho, f.reg);
    if (st != GBDPCG_OK) return st;
    st = kkt_resolve_impl<float>(h, k, a, stream);
    if (st != GBDPCG_OK) return st;
    return kkt_refine_apply_impl(h, a.n, k.nu, a.N, a.batch, k.z, a.lambda, f.expo, f.z, f.lambda, stream);
}

}  // namespace

extern "C" {

// An eager call and its graph_create twin from one parameter list.  PARAMS(TYPE): the parameters in front of the last one (the
// stream, or where the graph goes); SETUP(TYPE, SHARED) builds the operands and `a`, the description of the solve, once, and defines
// `body`, what the call puts on a stream; the eager entry runs the body on the caller's stream, the graph entry hands it to
// graph_create behind REFUSE(TYPE), what it refuses before anything is reserved or captured.
#define GBDPCG_PAIR(NAME, SUF, TYPE, SHARED, PARAMS, SETUP, REFUSE)                                                                 \
    gbdpcg_status gbdpcg_##NAME##_##SUF(PARAMS(TYPE), void *stream)                                                                 \
    {                                                                                                                               \
        SETUP(TYPE, SHARED)                                                                                                         \
        return body((hipStream_t)stream);                                                                                           \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_graph_create_##NAME##_##SUF(PARAMS(TYPE), gbdpcg_graph_t *out)                                             \
    {                                                                                                                               \
        SETUP(TYPE, SHARED)                                                                                                         \
        REFUSE(TYPE)                                                                                                                \
        return graph_create<TYPE>(h, a, SHARED, out, body);                                                                         \
    }
#define GBDPCG_PAIR_BOTH(NAME, TYPE_SHARED, PARAMS, SETUP, REFUSE)                                                                  \
    GBDPCG_PAIR(NAME, f32, float, TYPE_SHARED, PARAMS, SETUP, REFUSE)                                                               \
    GBDPCG_PAIR(NAME, f64, double, TYPE_SHARED, PARAMS, SETUP, REFUSE)

// ---- the single launches.  shared: one problem's Ginv, C (G for the residual) for the whole batch; reg: on G_b + rho_b I, d_rho
// [batch] on the device directly behind d_c.
#define GBDPCG_KKT_LAUNCHES(SUF, TYPE)                                                                                              \
    gbdpcg_status gbdpcg_form_schur_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_G, \
                                          const TYPE *d_C, const TYPE *d_g, const TYPE *d_c, TYPE *d_S, TYPE *d_gamma, TYPE *d_Ginv,\
                                          void *stream)                                                                             \
    {                                                                                                                               \
        return form_schur_impl<TYPE>(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_S, d_gamma, d_Ginv, stream);                        \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_form_schur_reg_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,              \
                                              const TYPE *d_G, const TYPE *d_C, const TYPE *d_g, const TYPE *d_c, const TYPE *d_rho,\
                                              TYPE *d_S, TYPE *d_gamma, TYPE *d_Ginv, void *stream)                                 \
    {                                                                                                                               \
        return form_schur_impl<TYPE>(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_S, d_gamma, d_Ginv, stream, d_rho, true);           \
    }                                                                                                                               \
    GBDPCG_GINV_LAUNCHES(, SUF, TYPE, false)                                                                                        \
    GBDPCG_GINV_LAUNCHES(_shared, SUF, TYPE, true)                                                                                  \
    gbdpcg_status gbdpcg_kkt_residual_reg_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,            \
                                                const TYPE *d_G, const TYPE *d_C, const TYPE *d_g, const TYPE *d_c,                 \
                                                const TYPE *d_rho, const TYPE *d_z, const TYPE *d_lambda, TYPE *d_res, void *stream)\
    {                                                                                                                               \
        return kkt_residual_impl<TYPE>(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_res, stream, false, d_rho, true);  \
    }
#define GBDPCG_GINV_LAUNCHES(NAME, SUF, TYPE, SHARED)                                                                               \
    gbdpcg_status gbdpcg_recover_primal##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,      \
                                                      const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_g, const TYPE *d_lambda,   \
                                                      TYPE *d_z, void *stream)                                                      \
    {                                                                                                                               \
        return recover_primal_impl<TYPE>(h, nx, nu, N, batch, d_Ginv, d_C, d_g, d_lambda, d_z, stream, SHARED);                     \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_form_gamma##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,          \
                                                  const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_g, const TYPE *d_c,            \
                                                  TYPE *d_gamma, void *stream)                                                      \
    {                                                                                                                               \
        return form_gamma_impl<TYPE>(h, nx, nu, N, batch, d_Ginv, d_C, d_g, d_c, d_gamma, stream, SHARED);                          \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_kkt_residual##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,        \
                                                    const TYPE *d_G, const TYPE *d_C, const TYPE *d_g, const TYPE *d_c,             \
                                                    const TYPE *d_z, const TYPE *d_lambda, TYPE *d_res, void *stream)               \
    {                                                                                                                               \
        return kkt_residual_impl<TYPE>(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_res, stream, SHARED);              \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_kkt_grad##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,            \
                                                const TYPE *d_z, const TYPE *d_lambda, const TYPE *d_az, const TYPE *d_alambda,     \
                                                TYPE *d_gG, TYPE *d_gC, void *stream)                                               \
    {                                                                                                                               \
        return kkt_grad_impl<TYPE>(h, nx, nu, N, batch, d_z, d_lambda, d_az, d_alambda, d_gG, d_gC, stream, SHARED);                \
    }
GBDPCG_KKT_LAUNCHES(f32, float)
GBDPCG_KKT_LAUNCHES(f64, double)
#undef GBDPCG_GINV_LAUNCHES
#undef GBDPCG_KKT_LAUNCHES

// ---- gbdpcg_kkt_step_*, and gbdpcg_kkt_step_reg_* on G_b + rho_b I
#define STEP_TAIL(TYPE)                                                                                                             \
    TYPE *d_S, TYPE *d_gamma, TYPE *d_Ginv, TYPE *d_Pinv, gbdpcg_pinv_kind kind, TYPE *d_lambda, TYPE *d_r, TYPE *d_p, TYPE tol,    \
        uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, TYPE *d_z
#define STEP_PARAMS(TYPE)                                                                                                           \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_G, const TYPE *d_C, const TYPE *d_g,     \
        const TYPE *d_c, STEP_TAIL(TYPE)
#define STEP_REG_PARAMS(TYPE)                                                                                                       \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_G, const TYPE *d_C, const TYPE *d_g,     \
        const TYPE *d_c, const TYPE *d_rho, STEP_TAIL(TYPE)
#define STEP_SETUP_OF(TYPE, RHO, REG)                                                                                               \
    const KktFormed<TYPE> f{d_G, d_S, d_Ginv, d_Pinv, kind, RHO, REG};                                                              \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_g, d_c, d_gamma, d_z};                                                             \
    const PcgArgs<TYPE> a = PCG_ARGS(TYPE, nx);                                                                                     \
    auto body = [&](hipStream_t s) { return kkt_step_impl<TYPE>(h, f, k, a, s); };
#define STEP_SETUP(TYPE, SHARED) STEP_SETUP_OF(TYPE, nullptr, false)
#define STEP_REG_SETUP(TYPE, SHARED) STEP_SETUP_OF(TYPE, d_rho, true)
#define STEP_REFUSE(TYPE) \
    if (kkt_step_refusal<TYPE>(f, k, true) != GBDPCG_OK) return GBDPCG_ERR_INVALID;
GBDPCG_PAIR_BOTH(kkt_step, false, STEP_PARAMS, STEP_SETUP, STEP_REFUSE)
GBDPCG_PAIR_BOTH(kkt_step_reg, false, STEP_REG_PARAMS, STEP_REG_SETUP, STEP_REFUSE)

// ---- gbdpcg_kkt_resolve_* on a kept linearisation, and its shared-matrix twin: one Ginv, C, S, Pinv (made by the batch-1 forms of
// gbdpcg_kkt_step_* or gbdpcg_form_schur_* / gbdpcg_form_pinv_*) for `batch` right-hand sides
#define RESOLVE_PARAMS(TYPE)                                                                                                        \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_g,  \
        const TYPE *d_c, const TYPE *d_S, const TYPE *d_Pinv, TYPE *d_gamma, TYPE *d_lambda, TYPE *d_r, TYPE *d_p, TYPE tol,        \
        uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, TYPE *d_z
#define RESOLVE_SETUP(TYPE, SHARED)                                                                                                 \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_g, d_c, d_gamma, d_z, SHARED};                                                     \
    const PcgArgs<TYPE> a = PCG_ARGS(TYPE, nx);                                                                                     \
    auto body = [&](hipStream_t s) { return kkt_resolve_impl<TYPE>(h, k, a, s); };
#define RESOLVE_REFUSE(TYPE)                                                                                                        \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    if (const gbdpcg_status st = kkt_resolve_refusal<TYPE>(h, k, a, false)) return st;
GBDPCG_PAIR_BOTH(kkt_resolve, false, RESOLVE_PARAMS, RESOLVE_SETUP, RESOLVE_REFUSE)
GBDPCG_PAIR_BOTH(kkt_resolve_shared, true, RESOLVE_PARAMS, RESOLVE_SETUP, RESOLVE_REFUSE)

// ---- ADMM iterations on a kept factorisation, whose solve is gbdpcg_kkt_resolve_*.  Three families of one shape:
//   admm       box lo <= z <= hi, the matrices of G + rho I
//   admm_lin   stage-wise linear rows lo <= E z <= hi, the matrices of G + rho E'E (gbdpcg_admm_lin_form_*)
//   admm_soc   second-order cone rows next to the linear ones, the same matrices
// admm and admm_lin have soft twins (admm_soft, admm_lin_soft, behind admm_soc below): L1-penalised bounds, d_kappa behind d_hi.
// Each has init, update, step and graph_create_step, the last two with a _shared twin on one problem's Ginv, C, S, Pinv (and E);
// the set, rho and the splitting state stay per problem.  Adaptive rho: rebalance, restep and graph_create_restep, per problem only.
// A family is described by these macros, defined in front of its entries:
//   ADMM_SIZES           the sizes between h and N
//   ADMM_SET(TYPE)       the set, in front of d_rho
//   ADMM_CONES           the declaration of `cones`, the RowClasses of the family, where it has any
//   ADMM_OPERANDS        the initialiser of its AdmmOperands (rows: its tail behind d_res is ADMM_ROWS_OPERANDS)
//   ADMM_MATS, ADMM_GT   what a restep refactors from (below)
#define ADMM_STEP_PARAMS(TYPE)                                                                                                      \
    gbdpcg_handle_t h, ADMM_SIZES, uint32_t N, uint32_t batch, const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_g,                \
        const TYPE *d_c, ADMM_SET(TYPE), const TYPE *d_rho, const TYPE *d_S, const TYPE *d_Pinv, TYPE *d_gamma, TYPE *d_lambda,     \
        TYPE *d_r, TYPE *d_p, TYPE tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, TYPE *d_z, TYPE *d_w,       \
        TYPE *d_y, TYPE *d_gt, TYPE *d_res
#define ADMM_STEP_SETUP(TYPE, SHARED)                                                                                               \
    ADMM_CONES                                                                                                                      \
    const AdmmOperands<TYPE> ad{ADMM_OPERANDS};                                                                                     \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_g, d_c, d_gamma, d_z, SHARED};                                                     \
    const PcgArgs<TYPE> a = PCG_ARGS(TYPE, nx);                                                                                     \
    auto body = [&](hipStream_t s) { return admm_step_impl<TYPE>(h, k, ad, a, s); };
#define ADMM_STEP_REFUSE(TYPE)                                                                                                      \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    *out = nullptr;                                                                                                                 \
    if (const gbdpcg_status st = admm_step_refusal<TYPE>(h, k, ad, a, false)) return st;
#define GBDPCG_ADMM_STEPS(NAME)                                                                                                     \
    GBDPCG_PAIR_BOTH(NAME, false, ADMM_STEP_PARAMS, ADMM_STEP_SETUP, ADMM_STEP_REFUSE)                                              \
    GBDPCG_PAIR_BOTH(NAME##_shared, true, ADMM_STEP_PARAMS, ADMM_STEP_SETUP, ADMM_STEP_REFUSE)
// One iteration with a new rho (admm_restep_impl): the list of the step with what the refactorisation writes no longer const,
// ADMM_MATS (the original G, and for the families with rows the Gt formed from it) in front of d_Ginv, the kind of Phi^-1 behind
// d_Pinv and the rule at the end.  ADMM_GT: the Gt of the family, nullptr for the box.  No _shared twin: one factorisation, one rho.
#define ADMM_RULE(TYPE) TYPE ratio, uint32_t shift, TYPE rho_min, TYPE rho_max, int32_t *d_expo
#define ADMM_RESTEP_PARAMS(TYPE)                                                                                                    \
    gbdpcg_handle_t h, ADMM_SIZES, uint32_t N, uint32_t batch, ADMM_MATS(TYPE), TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_g,     \
        const TYPE *d_c, ADMM_SET(TYPE), TYPE *d_rho, TYPE *d_S, TYPE *d_Pinv, gbdpcg_pinv_kind kind, TYPE *d_gamma,                \
        TYPE *d_lambda, TYPE *d_r, TYPE *d_p, TYPE tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, TYPE *d_z,  \
        TYPE *d_w, TYPE *d_y, TYPE *d_gt, TYPE *d_res, ADMM_RULE(TYPE)
#define ADMM_RESTEP_SETUP(TYPE, SHARED)                                                                                             \
    ADMM_CONES                                                                                                                      \
    const AdmmOperands<TYPE> ad{ADMM_OPERANDS};                                                                                     \
    const RhoRule<TYPE> rule{ratio, shift, rho_min, rho_max, d_rho, d_expo};                                                        \
    const Refactor<TYPE> f{d_G, ADMM_GT, d_S, d_Ginv, d_Pinv, kind};                                                                \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_g, d_c, d_gamma, d_z};                                                             \
    const PcgArgs<TYPE> a = PCG_ARGS(TYPE, nx);                                                                                     \
    auto body = [&](hipStream_t s) { return admm_restep_impl<TYPE>(h, f, k, ad, rule, a, s); };
#define ADMM_RESTEP_REFUSE(TYPE)                                                                                                    \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    *out = nullptr;                                                                                                                 \
    if (const gbdpcg_status st = admm_restep_refusal<TYPE>(h, f, k, ad, rule, a, false)) return st;
#define GBDPCG_ADMM_RESTEPS(NAME) GBDPCG_PAIR_BOTH(NAME, false, ADMM_RESTEP_PARAMS, ADMM_RESTEP_SETUP, ADMM_RESTEP_REFUSE)
// init, update and rebalance of a family with rows: thin forwards to admm_rows_update_impl (init has neither d_z nor d_res) and
// admm_rows_rebalance_impl
#define GBDPCG_ADMM_ROWS(NAME, SUF, TYPE)                                                                                           \
    gbdpcg_status gbdpcg_##NAME##_init_##SUF(gbdpcg_handle_t h, ADMM_SIZES, uint32_t N, uint32_t batch, const TYPE *d_g,            \
                                             ADMM_SET(TYPE), const TYPE *d_rho, TYPE *d_w, TYPE *d_y, TYPE *d_gt, void *stream)     \
    {                                                                                                                               \
        TYPE *const d_res = nullptr;                                                                                                \
        ADMM_CONES                                                                                                                  \
        const AdmmOperands<TYPE> a{ADMM_OPERANDS};                                                                                  \
        return admm_rows_update_impl<TYPE>(h, nx, nu, N, batch, d_g, a, nullptr, stream, true);                                     \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_##NAME##_update_##SUF(gbdpcg_handle_t h, ADMM_SIZES, uint32_t N, uint32_t batch, const TYPE *d_g,          \
                                               ADMM_SET(TYPE), const TYPE *d_rho, const TYPE *d_z, TYPE *d_w, TYPE *d_y,            \
                                               TYPE *d_gt, TYPE *d_res, void *stream)                                               \
    {                                                                                                                               \
        ADMM_CONES                                                                                                                  \
        const AdmmOperands<TYPE> a{ADMM_OPERANDS};                                                                                  \
        return admm_rows_update_impl<TYPE>(h, nx, nu, N, batch, d_g, a, d_z, stream, false);                                        \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_##NAME##_rebalance_##SUF(gbdpcg_handle_t h, ADMM_SIZES, uint32_t N, uint32_t batch, const TYPE *d_g,       \
                                                  ADMM_SET(TYPE), const TYPE *d_res, TYPE *d_rho, TYPE *d_w, TYPE *d_y, TYPE *d_gt, \
                                                  ADMM_RULE(TYPE), void *stream)                                                    \
    {                                                                                                                               \
        ADMM_CONES                                                                                                                  \
        const AdmmOperands<TYPE> a{d_lo, d_hi, d_rho, d_w, d_y, d_gt, const_cast<TYPE *>(d_res), ADMM_ROWS_OPERANDS};               \
        const RhoRule<TYPE> rule{ratio, shift, rho_min, rho_max, d_rho, d_expo};                                                    \
        return admm_rows_rebalance_impl<TYPE>(h, nx, nu, N, batch, d_g, a, rule, stream);                                           \
    }

#define ADMM_SIZES uint32_t nx, uint32_t nu
#define ADMM_SET(TYPE) const TYPE *d_lo, const TYPE *d_hi
#define ADMM_CONES
#define ADMM_OPERANDS d_lo, d_hi, d_rho, d_w, d_y, d_gt, d_res
#define GBDPCG_ADMM(SUF, TYPE)                                                                                                      \
    gbdpcg_status gbdpcg_admm_init_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_g,  \
                                         const TYPE *d_lo, const TYPE *d_hi, const TYPE *d_rho, TYPE *d_w, TYPE *d_y, TYPE *d_gt,   \
                                         void *stream)                                                                              \
    {                                                                                                                               \
        return admm_update_impl<TYPE>(h, nx, nu, N, batch, d_g, d_lo, d_hi, d_rho, nullptr, d_w, d_y, d_gt, nullptr, stream, true); \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_update_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_g,\
                                           const TYPE *d_lo, const TYPE *d_hi, const TYPE *d_rho, const TYPE *d_z, TYPE *d_w,       \
                                           TYPE *d_y, TYPE *d_gt, TYPE *d_res, void *stream)                                        \
    {                                                                                                                               \
        return admm_update_impl<TYPE>(h, nx, nu, N, batch, d_g, d_lo, d_hi, d_rho, d_z, d_w, d_y, d_gt, d_res, stream, false);      \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_rebalance_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,              \
                                              const TYPE *d_g, const TYPE *d_res, TYPE *d_rho, const TYPE *d_w, TYPE *d_y,          \
                                              TYPE *d_gt, ADMM_RULE(TYPE), void *stream)                                            \
    {                                                                                                                               \
        const RhoRule<TYPE> rule{ratio, shift, rho_min, rho_max, d_rho, d_expo};                                                    \
        return admm_rebalance_impl<TYPE>(h, nx, nu, N, batch, d_g, d_res, d_w, d_y, d_gt, rule, stream);                            \
    }
#define ADMM_MATS(TYPE) const TYPE *d_G
#define ADMM_GT nullptr
GBDPCG_ADMM(f32, float)
GBDPCG_ADMM(f64, double)
GBDPCG_ADMM_STEPS(admm_step)
GBDPCG_ADMM_RESTEPS(admm_restep)
#undef GBDPCG_ADMM
#undef ADMM_MATS
#undef ADMM_GT
#undef ADMM_SIZES
#undef ADMM_SET
#undef ADMM_OPERANDS

// (admm_lin: ADMM_CONES stays empty)
#define ADMM_SIZES uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu
#define ADMM_SET(TYPE) const TYPE *d_E, const TYPE *d_lo, const TYPE *d_hi
#define ADMM_OPERANDS d_lo, d_hi, d_rho, d_w, d_y, d_gt, d_res, ADMM_ROWS_OPERANDS
#define ADMM_ROWS_OPERANDS true, d_E, mx, mu
#define ADMM_MATS(TYPE) const TYPE *d_G, TYPE *d_Gt
#define ADMM_GT d_Gt
#define GBDPCG_ADMM_LIN(SUF, TYPE)                                                                                                  \
    gbdpcg_status gbdpcg_admm_lin_form_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,     \
                                             uint32_t batch, const TYPE *d_G, const TYPE *d_E, const TYPE *d_rho, TYPE *d_Gt,       \
                                             void *stream)                                                                          \
    {                                                                                                                               \
        return admm_lin_form_impl<TYPE>(h, nx, nu, mx, mu, N, batch, d_G, d_E, d_rho, d_Gt, stream);                                \
    }                                                                                                                               \
    GBDPCG_ADMM_ROWS(admm_lin, SUF, TYPE)
GBDPCG_ADMM_LIN(f32, float)
GBDPCG_ADMM_LIN(f64, double)
GBDPCG_ADMM_STEPS(admm_lin_step)
GBDPCG_ADMM_RESTEPS(admm_lin_restep)
#undef GBDPCG_ADMM_LIN
#undef ADMM_SIZES
#undef ADMM_CONES
#undef ADMM_ROWS_OPERANDS

// (admm_soc: ADMM_SET, ADMM_OPERANDS, ADMM_MATS and ADMM_GT stay those of admm_lin)
#define ADMM_SIZES uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t lx, uint32_t qx, uint32_t lu, uint32_t qu
#define ADMM_CONES const RowClasses cones{lx, qx, lu, qu};
#define ADMM_ROWS_OPERANDS true, d_E, mx, mu, &cones
GBDPCG_ADMM_ROWS(admm_soc, f32, float)
GBDPCG_ADMM_ROWS(admm_soc, f64, double)
GBDPCG_ADMM_STEPS(admm_soc_step)
GBDPCG_ADMM_RESTEPS(admm_soc_restep)
#undef ADMM_SIZES
#undef ADMM_SET
#undef ADMM_CONES
#undef ADMM_ROWS_OPERANDS

// ---- soft (L1-penalised) bounds: the box and the linear rows with the weights d_kappa, in the layout of d_lo, directly behind d_hi.
// kappa = +Inf everywhere gives the bits of the hard family; cone rows stay hard (there is no admm_soc_soft).
// (admm_lin_soft: ADMM_OPERANDS, ADMM_MATS and ADMM_GT stay those of admm_lin; its rebalance rebuilds gt with the SOFT init)
#define ADMM_SIZES uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu
#define ADMM_SET(TYPE) const TYPE *d_E, const TYPE *d_lo, const TYPE *d_hi, const TYPE *d_kappa
#define ADMM_CONES
#define ADMM_ROWS_OPERANDS true, d_E, mx, mu, nullptr, d_kappa, true
GBDPCG_ADMM_ROWS(admm_lin_soft, f32, float)
GBDPCG_ADMM_ROWS(admm_lin_soft, f64, double)
GBDPCG_ADMM_STEPS(admm_lin_soft_step)
GBDPCG_ADMM_RESTEPS(admm_lin_soft_restep)
#undef ADMM_SIZES
#undef ADMM_SET
#undef ADMM_OPERANDS
#undef ADMM_ROWS_OPERANDS
#undef ADMM_MATS
#undef ADMM_GT

// (admm_soft: the box.  gbdpcg_admm_rebalance_* is its rebalance too: that launch never looks at the bounds and does not clip w)
#define ADMM_SIZES uint32_t nx, uint32_t nu
#define ADMM_SET(TYPE) const TYPE *d_lo, const TYPE *d_hi, const TYPE *d_kappa
#define ADMM_OPERANDS d_lo, d_hi, d_rho, d_w, d_y, d_gt, d_res, false, nullptr, 0, 0, nullptr, d_kappa, true
#define ADMM_MATS(TYPE) const TYPE *d_G
#define ADMM_GT nullptr
#define GBDPCG_ADMM_SOFT(SUF, TYPE)                                                                                                 \
    gbdpcg_status gbdpcg_admm_soft_init_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,              \
                                              const TYPE *d_g, ADMM_SET(TYPE), const TYPE *d_rho, TYPE *d_w, TYPE *d_y, TYPE *d_gt, \
                                              void *stream)                                                                         \
    {                                                                                                                               \
        return admm_update_impl<TYPE>(h, nx, nu, N, batch, d_g, d_lo, d_hi, d_rho, nullptr, d_w, d_y, d_gt, nullptr, stream, true,  \
                                      d_kappa, true);                                                                               \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_soft_update_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,            \
                                                const TYPE *d_g, ADMM_SET(TYPE), const TYPE *d_rho, const TYPE *d_z, TYPE *d_w,     \
                                                TYPE *d_y, TYPE *d_gt, TYPE *d_res, void *stream)                                   \
    {                                                                                                                               \
        return admm_update_impl<TYPE>(h, nx, nu, N, batch, d_g, d_lo, d_hi, d_rho, d_z, d_w, d_y, d_gt, d_res, stream, false,       \
                                      d_kappa, true);                                                                               \
    }
GBDPCG_ADMM_SOFT(f32, float)
GBDPCG_ADMM_SOFT(f64, double)
GBDPCG_ADMM_STEPS(admm_soft_step)
GBDPCG_ADMM_RESTEPS(admm_soft_restep)
#undef GBDPCG_ADMM_SOFT
#undef ADMM_SIZES
#undef ADMM_SET
#undef ADMM_CONES
#undef ADMM_OPERANDS
#undef ADMM_MATS
#undef ADMM_GT
#undef GBDPCG_ADMM_ROWS
#undef GBDPCG_ADMM_STEPS
#undef GBDPCG_ADMM_RESTEPS
#undef ADMM_RULE
#undef ADMM_RESTEP_PARAMS
#undef ADMM_RESTEP_SETUP
#undef ADMM_RESTEP_REFUSE

// ---- the backward pass of the hard box QP: the adjoint iteration of gbdpcg_admm_step_* with the forward y (d_yf) where d_lo, d_hi
// stand, g := d_gz = dl/dz, c := d_nglam = -dl/dlambda, and the launch that turns the adjoint's y into dl/dlo, dl/dhi.  No _shared twin.
#define ADJOINT_STEP_PARAMS(TYPE)                                                                                                   \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_gz, \
        const TYPE *d_nglam, const TYPE *d_yf, const TYPE *d_rho, const TYPE *d_S, const TYPE *d_Pinv, TYPE *d_gamma,               \
        TYPE *d_alambda, TYPE *d_r, TYPE *d_p, TYPE tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit,            \
        TYPE *d_az, TYPE *d_wa, TYPE *d_ya, TYPE *d_gta, TYPE *d_res
#define ADJOINT_STEP_SETUP(TYPE, SHARED)                                                                                            \
    const AdmmOperands<TYPE> ad{d_yf, d_yf, d_rho, d_wa, d_ya, d_gta, d_res, false, nullptr, 0, 0, nullptr, nullptr, false, true};  \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_gz, d_nglam, d_gamma, d_az, SHARED};                                               \
    const PcgArgs<TYPE> a = pcg_args<TYPE>(nx, N, batch, d_S, d_Pinv, d_gamma, d_alambda, d_r, d_p, tol, max_iter, d_iters, d_max_iter_exit);\
    auto body = [&](hipStream_t s) { return admm_step_impl<TYPE>(h, k, ad, a, s); };
#define ADJOINT_STEP_REFUSE(TYPE)                                                                                                   \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    *out = nullptr;                                                                                                                 \
    if (const gbdpcg_status st = admm_step_refusal<TYPE>(h, k, ad, a, false)) return st;
#define GBDPCG_ADMM_ADJOINT(SUF, TYPE)                                                                                              \
    gbdpcg_status gbdpcg_admm_adjoint_init_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,           \
                                                 const TYPE *d_gz, const TYPE *d_yf, const TYPE *d_rho, TYPE *d_wa, TYPE *d_ya,     \
                                                 TYPE *d_gta, void *stream)                                                         \
    {                                                                                                                               \
        return admm_adjoint_update_impl<TYPE>(h, nx, nu, N, batch, d_gz, d_yf, d_rho, nullptr, d_wa, d_ya, d_gta, nullptr, stream,  \
                                              true);                                                                                \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_adjoint_update_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,         \
                                                   const TYPE *d_gz, const TYPE *d_yf, const TYPE *d_rho, const TYPE *d_az,         \
                                                   TYPE *d_wa, TYPE *d_ya, TYPE *d_gta, TYPE *d_res, void *stream)                  \
    {                                                                                                                               \
        return admm_adjoint_update_impl<TYPE>(h, nx, nu, N, batch, d_gz, d_yf, d_rho, d_az, d_wa, d_ya, d_gta, d_res, stream, false);\
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_grad_bounds_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,            \
                                                const TYPE *d_yf, const TYPE *d_rho, const TYPE *d_ya, TYPE *d_glo, TYPE *d_ghi,    \
                                                void *stream)                                                                       \
    {                                                                                                                               \
        return admm_grad_bounds_impl<TYPE>(h, nx, nu, N, batch, d_yf, d_rho, d_ya, d_glo, d_ghi, stream);                           \
    }
GBDPCG_ADMM_ADJOINT(f32, float)
GBDPCG_ADMM_ADJOINT(f64, double)
GBDPCG_PAIR_BOTH(admm_adjoint_step, false, ADJOINT_STEP_PARAMS, ADJOINT_STEP_SETUP, ADJOINT_STEP_REFUSE)
#undef GBDPCG_ADMM_ADJOINT
#undef ADJOINT_STEP_PARAMS
#undef ADJOINT_STEP_SETUP
#undef ADJOINT_STEP_REFUSE

// ---- the backward pass of the hard linear-row QP: the iteration of gbdpcg_admm_lin_step_* with the forward y (d_yf) where d_lo,
// d_hi stand (the adjoint instantiations of the rows kernel), g := d_gz, c := d_nglam, on the kept matrices of G + rho E'E; and the
// launch that turns (z, az, yf, ya) into dl/dlo, dl/dhi, dl/dE.  The step IS admm_step_impl on these operands.  No _shared twin.
#define LIN_ADJOINT_SIZES gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, uint32_t batch
#define LIN_ADJOINT_OPERANDS d_yf, d_yf, d_rho, d_wa, d_ya, d_gta, d_res, true, d_E, mx, mu, nullptr, nullptr, false, true
#define LIN_ADJOINT_STEP_PARAMS(TYPE)                                                                                               \
    LIN_ADJOINT_SIZES, const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_gz, const TYPE *d_nglam, const TYPE *d_E, const TYPE *d_yf,\
        const TYPE *d_rho, const TYPE *d_S, const TYPE *d_Pinv, TYPE *d_gamma, TYPE *d_alambda, TYPE *d_r, TYPE *d_p, TYPE tol,     \
        uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, TYPE *d_az, TYPE *d_wa, TYPE *d_ya, TYPE *d_gta, TYPE *d_res
#define LIN_ADJOINT_STEP_SETUP(TYPE, SHARED)                                                                                        \
    const AdmmOperands<TYPE> ad{LIN_ADJOINT_OPERANDS};                                                                              \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_gz, d_nglam, d_gamma, d_az, SHARED};                                               \
    const PcgArgs<TYPE> a = pcg_args<TYPE>(nx, N, batch, d_S, d_Pinv, d_gamma, d_alambda, d_r, d_p, tol, max_iter, d_iters, d_max_iter_exit);\
    auto body = [&](hipStream_t s) { return admm_step_impl<TYPE>(h, k, ad, a, s); };
#define LIN_ADJOINT_STEP_REFUSE(TYPE)                                                                                               \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    *out = nullptr;                                                                                                                 \
    if (const gbdpcg_status st = admm_step_refusal<TYPE>(h, k, ad, a, false)) return st;
#define GBDPCG_ADMM_LIN_ADJOINT(SUF, TYPE)                                                                                          \
    gbdpcg_status gbdpcg_admm_lin_adjoint_init_##SUF(LIN_ADJOINT_SIZES, const TYPE *d_gz, const TYPE *d_E, const TYPE *d_yf,        \
                                                     const TYPE *d_rho, TYPE *d_wa, TYPE *d_ya, TYPE *d_gta, void *stream)          \
    {                                                                                                                               \
        TYPE *const d_res = nullptr;                                                                                                \
        const AdmmOperands<TYPE> a{LIN_ADJOINT_OPERANDS};                                                                           \
        return admm_rows_update_impl<TYPE>(h, nx, nu, N, batch, d_gz, a, nullptr, stream, true);                                    \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_lin_adjoint_update_##SUF(LIN_ADJOINT_SIZES, const TYPE *d_gz, const TYPE *d_E, const TYPE *d_yf,      \
                                                       const TYPE *d_rho, const TYPE *d_az, TYPE *d_wa, TYPE *d_ya, TYPE *d_gta,    \
                                                       TYPE *d_res, void *stream)                                                   \
    {                                                                                                                               \
        const AdmmOperands<TYPE> a{LIN_ADJOINT_OPERANDS};                                                                           \
        return admm_rows_update_impl<TYPE>(h, nx, nu, N, batch, d_gz, a, d_az, stream, false);                                      \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_lin_grad_##SUF(LIN_ADJOINT_SIZES, const TYPE *d_z, const TYPE *d_az, const TYPE *d_yf,                \
                                             const TYPE *d_ya, const TYPE *d_rho, TYPE *d_glo, TYPE *d_ghi, TYPE *d_gE, void *stream)\
    {                                                                                                                               \
        return admm_lin_grad_impl<TYPE>(h, nx, nu, mx, mu, N, batch, d_z, d_az, d_yf, d_ya, d_rho, d_glo, d_ghi, d_gE, stream);      \
    }
GBDPCG_ADMM_LIN_ADJOINT(f32, float)
GBDPCG_ADMM_LIN_ADJOINT(f64, double)
GBDPCG_PAIR_BOTH(admm_lin_adjoint_step, false, LIN_ADJOINT_STEP_PARAMS, LIN_ADJOINT_STEP_SETUP, LIN_ADJOINT_STEP_REFUSE)
#undef GBDPCG_ADMM_LIN_ADJOINT
#undef LIN_ADJOINT_SIZES
#undef LIN_ADJOINT_OPERANDS
#undef LIN_ADJOINT_STEP_PARAMS
#undef LIN_ADJOINT_STEP_SETUP
#undef LIN_ADJOINT_STEP_REFUSE

// ---- the backward pass of the soft box and rows QPs: the mask in front of the hard adjoint calls above, and the gradient launches
// with kappa.  No step of their own: the adjoint iteration is gbdpcg_admm_adjoint_step_* / gbdpcg_admm_lin_adjoint_step_* on d_ym.
#define GBDPCG_ADMM_SOFT_ADJOINT(SUF, TYPE)                                                                                         \
    gbdpcg_status gbdpcg_admm_soft_mask_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,              \
                                              const TYPE *d_yf, const TYPE *d_kappa, const TYPE *d_rho, TYPE *d_ym, void *stream)   \
    {                                                                                                                               \
        return admm_soft_mask_impl<TYPE>(h, nx, nu, 0, 0, N, batch, d_yf, d_kappa, d_rho, d_ym, stream, false);                     \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_lin_soft_mask_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,\
                                                  uint32_t batch, const TYPE *d_yf, const TYPE *d_kappa, const TYPE *d_rho,         \
                                                  TYPE *d_ym, void *stream)                                                         \
    {                                                                                                                               \
        return admm_soft_mask_impl<TYPE>(h, nx, nu, mx, mu, N, batch, d_yf, d_kappa, d_rho, d_ym, stream, true);                    \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_soft_grad_bounds_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,       \
                                                     const TYPE *d_yf, const TYPE *d_kappa, const TYPE *d_rho, const TYPE *d_ya,    \
                                                     const TYPE *d_az, TYPE *d_glo, TYPE *d_ghi, TYPE *d_gkappa, void *stream)      \
    {                                                                                                                               \
        return admm_soft_grad_bounds_impl<TYPE>(h, nx, nu, N, batch, d_yf, d_kappa, d_rho, d_ya, d_az, d_glo, d_ghi, d_gkappa,      \
                                                stream);                                                                            \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_lin_soft_grad_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N,\
                                                  uint32_t batch, const TYPE *d_z, const TYPE *d_az, const TYPE *d_E,               \
                                                  const TYPE *d_yf, const TYPE *d_ya, const TYPE *d_kappa, const TYPE *d_rho,       \
                                                  TYPE *d_glo, TYPE *d_ghi, TYPE *d_gkappa, TYPE *d_gE, void *stream)               \
    {                                                                                                                               \
        return admm_lin_soft_grad_impl<TYPE>(h, nx, nu, mx, mu, N, batch, d_z, d_az, d_E, d_yf, d_ya, d_kappa, d_rho, d_glo, d_ghi, \
                                             d_gkappa, d_gE, stream);                                                               \
    }
GBDPCG_ADMM_SOFT_ADJOINT(f32, float)
GBDPCG_ADMM_SOFT_ADJOINT(f64, double)
#undef GBDPCG_ADMM_SOFT_ADJOINT

// ---- the infeasibility certificate of the hard box and rows paths, with the _shared twins (one problem's C [and E])
#define INFEAS_VECTORS(TYPE)                                                                                                        \
    const TYPE *d_lo, const TYPE *d_hi, const TYPE *d_rho, const TYPE *d_lambda0, const TYPE *d_lambda1, const TYPE *d_y0,          \
        const TYPE *d_y1, TYPE eps, TYPE *d_cert, uint8_t *d_flag, void *stream
#define GBDPCG_ADMM_INFEAS(NAME, SHARED, SUF, TYPE)                                                                                 \
    gbdpcg_status gbdpcg_admm_##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,               \
                                             const TYPE *d_C, const TYPE *d_c, INFEAS_VECTORS(TYPE))                                \
    {                                                                                                                               \
        return admm_infeas_impl<TYPE>(h, nx, nu, 0, 0, N, batch, d_C, d_c, nullptr, d_lo, d_hi, d_rho, d_lambda0, d_lambda1, d_y0,  \
                                      d_y1, eps, d_cert, d_flag, stream, true, SHARED);                                             \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_lin_##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, \
                                                 uint32_t batch, const TYPE *d_C, const TYPE *d_c, const TYPE *d_E,                 \
                                                 INFEAS_VECTORS(TYPE))                                                              \
    {                                                                                                                               \
        return admm_infeas_impl<TYPE>(h, nx, nu, mx, mu, N, batch, d_C, d_c, d_E, d_lo, d_hi, d_rho, d_lambda0, d_lambda1, d_y0,    \
                                      d_y1, eps, d_cert, d_flag, stream, false, SHARED);                                            \
    }
GBDPCG_ADMM_INFEAS(infeas, false, f32, float)
GBDPCG_ADMM_INFEAS(infeas, false, f64, double)
GBDPCG_ADMM_INFEAS(infeas_shared, true, f32, float)
GBDPCG_ADMM_INFEAS(infeas_shared, true, f64, double)
#undef GBDPCG_ADMM_INFEAS
#undef INFEAS_VECTORS

// ---- the optimality test of every ADMM family, with the _shared twins (one problem's G, C [and E])
#define OPTIMALITY_VECTORS(TYPE)                                                                                                    \
    const TYPE *d_rho, const TYPE *d_z, const TYPE *d_lambda, const TYPE *d_w, const TYPE *d_y, TYPE eps_abs, TYPE eps_rel,         \
        TYPE *d_opt, uint8_t *d_done, void *stream
#define GBDPCG_ADMM_OPTIMALITY(NAME, SHARED, SUF, TYPE)                                                                             \
    gbdpcg_status gbdpcg_admm_##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,               \
                                             const TYPE *d_G, const TYPE *d_C, const TYPE *d_g, const TYPE *d_c,                    \
                                             OPTIMALITY_VECTORS(TYPE))                                                              \
    {                                                                                                                               \
        return admm_optimality_impl<TYPE>(h, nx, nu, 0, 0, N, batch, d_G, d_C, d_g, d_c, nullptr, d_rho, d_z, d_lambda, d_w, d_y,   \
                                          eps_abs, eps_rel, d_opt, d_done, stream, true, SHARED);                                   \
    }                                                                                                                               \
    gbdpcg_status gbdpcg_admm_lin_##NAME##_##SUF(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t mx, uint32_t mu, uint32_t N, \
                                                 uint32_t batch, const TYPE *d_G, const TYPE *d_C, const TYPE *d_g, const TYPE *d_c, \
                                                 const TYPE *d_E, OPTIMALITY_VECTORS(TYPE))                                         \
    {                                                                                                                               \
        return admm_optimality_impl<TYPE>(h, nx, nu, mx, mu, N, batch, d_G, d_C, d_g, d_c, d_E, d_rho, d_z, d_lambda, d_w, d_y,     \
                                          eps_abs, eps_rel, d_opt, d_done, stream, false, SHARED);                                  \
    }
GBDPCG_ADMM_OPTIMALITY(optimality, false, f32, float)
GBDPCG_ADMM_OPTIMALITY(optimality, false, f64, double)
GBDPCG_ADMM_OPTIMALITY(optimality_shared, true, f32, float)
GBDPCG_ADMM_OPTIMALITY(optimality_shared, true, f64, double)
#undef GBDPCG_ADMM_OPTIMALITY
#undef OPTIMALITY_VECTORS

// ---- the KKT backward pass: the adjoint solve + gradient launch as one call / one graph (the gradient launch alone is with the
// single launches).  shared: one problem's Ginv, C, S, Pinv, and gG, gC summed over the batch.
#define BACKWARD_PARAMS(TYPE)                                                                                                       \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const TYPE *d_Ginv, const TYPE *d_C, const TYPE *d_gz, \
        const TYPE *d_nglam, const TYPE *d_S, const TYPE *d_Pinv, TYPE *d_gamma, const TYPE *d_z, const TYPE *d_lambda, TYPE *d_az, \
        TYPE *d_alambda, TYPE *d_r, TYPE *d_p, TYPE tol, uint32_t max_iter, uint32_t *d_iters, uint8_t *d_max_iter_exit, TYPE *d_gG,\
        TYPE *d_gC
#define BACKWARD_SETUP(TYPE, SHARED)                                                                                                \
    const GradOperands<TYPE> f{d_z, d_lambda, d_gG, d_gC};                                                                          \
    const KktOperands<TYPE> k{nu, d_Ginv, d_C, d_gz, d_nglam, d_gamma, d_az, SHARED};                                               \
    const PcgArgs<TYPE> a = pcg_args<TYPE>(nx, N, batch, d_S, d_Pinv, d_gamma, d_alambda, d_r, d_p, tol, max_iter, d_iters, d_max_iter_exit);\
    auto body = [&](hipStream_t s) { return kkt_backward_impl<TYPE>(h, k, f, a, s); };
#define BACKWARD_REFUSE(TYPE)                                                                                                       \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    if (const gbdpcg_status st = kkt_backward_refusal<TYPE>(h, k, f, a, false)) return st;
GBDPCG_PAIR_BOTH(kkt_backward, false, BACKWARD_PARAMS, BACKWARD_SETUP, BACKWARD_REFUSE)
GBDPCG_PAIR_BOTH(kkt_backward_shared, true, BACKWARD_PARAMS, BACKWARD_SETUP, BACKWARD_REFUSE)

// ---- mixed-precision refinement: the three single launches, then the step (defect, gbdpcg_kkt_resolve_f32, apply) as one call /
// one graph.  No suffix: the precisions are fixed -- fp64 data and point, fp32 solve.
gbdpcg_status gbdpcg_demote_f32(gbdpcg_handle_t h, uint64_t count, const double *d_src, float *d_dst, void *stream)
{
    if (!h || !d_src || !d_dst || count == 0) return GBDPCG_ERR_INVALID;
    DEVICE_SCOPE(h);
    HIP_TRY(h, launch_demote(h->dev, count, d_src, d_dst, (hipStream_t)stream));
    return GBDPCG_OK;
}
gbdpcg_status gbdpcg_kkt_defect_mixed(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                      const double *d_C, const double *d_g, const double *d_c, const double *d_z,
                                      const double *d_lambda, float *d_rg, float *d_rc, float *d_dlambda, int32_t *d_expo,
                                      double *d_res, void *stream)
{
    return kkt_defect_mixed_impl(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_rg, d_rc, d_dlambda, d_expo, d_res, stream);
}
gbdpcg_status gbdpcg_kkt_refine_apply(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const float *d_dz,
                                      const float *d_dlambda, const int32_t *d_expo, double *d_z, double *d_lambda, void *stream)
{
    return kkt_refine_apply_impl(h, nx, nu, N, batch, d_dz, d_dlambda, d_expo, d_z, d_lambda, stream);
}
// The _reg forms take d_rho directly behind d_c, the _shared forms the argument list of the plain ones.
gbdpcg_status gbdpcg_kkt_defect_mixed_reg(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G,
                                          const double *d_C, const double *d_g, const double *d_c, const double *d_rho,
                                          const double *d_z, const double *d_lambda, float *d_rg, float *d_rc, float *d_dlambda,
                                          int32_t *d_expo, double *d_res, void *stream)
{
    return kkt_defect_mixed_impl(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_rg, d_rc, d_dlambda, d_expo, d_res, stream,
                                 false, d_rho, true);
}
gbdpcg_status gbdpcg_kkt_defect_mixed_shared(gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch,
                                             const double *d_G, const double *d_C, const double *d_g, const double *d_c,
                                             const double *d_z, const double *d_lambda, float *d_rg, float *d_rc, float *d_dlambda,
                                             int32_t *d_expo, double *d_res, void *stream)
{
    return kkt_defect_mixed_impl(h, nx, nu, N, batch, d_G, d_C, d_g, d_c, d_z, d_lambda, d_rg, d_rc, d_dlambda, d_expo, d_res, stream,
                                 true);
}
#define REFINE_TAIL                                                                                                                 \
    const float *d_Ginv32, const float *d_C32, const float *d_S32, const float *d_Pinv32, float *d_rg, float *d_rc, float *d_gamma, \
        float *d_dlambda, float *d_r, float *d_p, float *d_dz, float tol, uint32_t max_iter, uint32_t *d_iters,                     \
        uint8_t *d_max_iter_exit, int32_t *d_expo, double *d_z, double *d_lambda, double *d_res
#define REFINE_PARAMS(TYPE)                                                                                                         \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G, const double *d_C,                  \
        const double *d_g, const double *d_c, REFINE_TAIL
#define REFINE_REG_PARAMS(TYPE)                                                                                                     \
    gbdpcg_handle_t h, uint32_t nx, uint32_t nu, uint32_t N, uint32_t batch, const double *d_G, const double *d_C,                  \
        const double *d_g, const double *d_c, const double *d_rho, REFINE_TAIL
#define REFINE_SETUP_OF(SHARED, RHO, REG)                                                                                           \
    const RefineOperands f{d_G, d_C, d_g, d_c, d_z, d_lambda, d_res, d_expo, d_rg, d_rc, RHO, REG};                                 \
    const KktOperands<float> k{nu, d_Ginv32, d_C32, d_rg, d_rc, d_gamma, d_dz, SHARED};                                             \
    const PcgArgs<float> a =                                                                                                        \
        pcg_args<float>(nx, N, batch, d_S32, d_Pinv32, d_gamma, d_dlambda, d_r, d_p, tol, max_iter, d_iters, d_max_iter_exit);      \
    auto body = [&](hipStream_t s) { return kkt_refine_step_impl(h, f, k, a, s); };
#define REFINE_SETUP(TYPE, SHARED) REFINE_SETUP_OF(SHARED, nullptr, false)
#define REFINE_REG_SETUP(TYPE, SHARED) REFINE_SETUP_OF(SHARED, d_rho, true)
#define REFINE_REFUSE(TYPE)                                                                                                         \
    if (!out) return GBDPCG_ERR_INVALID;                                                                                            \
    *out = nullptr;                                                                                                                 \
    if (const gbdpcg_status st = refine_step_refusal(h, f, k, a, false)) return st;
// (GBDPCG_PAIR names its entries NAME_SUF: the step has no precision suffix, so its last word stands in that place)
GBDPCG_PAIR(kkt_refine, step, float, false, REFINE_PARAMS, REFINE_SETUP, REFINE_REFUSE)
GBDPCG_PAIR(kkt_refine_step, reg, float, false, REFINE_REG_PARAMS, REFINE_REG_SETUP, REFINE_REFUSE)
GBDPCG_PAIR(kkt_refine_step, shared, float, true, REFINE_PARAMS, REFINE_SETUP, REFINE_REFUSE)
#undef REFINE_TAIL
#undef REFINE_PARAMS
#undef REFINE_REG_PARAMS
#undef REFINE_SETUP_OF
#undef REFINE_SETUP
#undef REFINE_REG_SETUP
#undef REFINE_REFUSE

}  // extern "C"
