// Host side of the C ABI (include/surfh_amd.h), the solvers: the CG building blocks, the CG frame (cg_start / cg_iteration / cg_loop
// on the maps, their spectra and the planes: surfh_cg, surfh_cg_planes and the device-resident plane loop), the 3MG loops (quadratic,
// Huber, voxel-wise, robust data term) with their prior / curvature diagnostics.  They call the operators of plan_ops.hip and
// nothing calls them.  Plan struct and data layout: plan_internal.h.
#include "plan_internal.h"
#include "mm_step.h"
#include <optional>

extern "C" {

int surfh_dot_dev(surfh_plan *p, const float *a, const float *b, int64_t n, double *out) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    LAUNCH_OK(launch_dot(p->stream, a, b, n, p->dscratch, p->dscal + 7));
    HIP_OK(hipMemcpyAsync(out, p->dscal + 7, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int surfh_cg_step_dev(surfh_plan *p, float *x, float *r, const float *d, const float *q, int64_t n, double rr_in,
                      double *rr_out) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    HIP_OK(hipMemcpyAsync(p->dscal + 0, &rr_in, sizeof(double), hipMemcpyHostToDevice, p->stream));
    LAUNCH_OK(launch_dot(p->stream, d, q, n, p->dscratch, p->dscal + 1));
    LAUNCH_OK(launch_cg_step(p->stream, x, r, d, q, n, p->dscal + 0, p->dscal + 1, p->dscratch, p->dscal + 2));
    HIP_OK(hipMemcpyAsync(rr_out, p->dscal + 2, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int surfh_cg_dir_dev(surfh_plan *p, float *d, const float *r, int64_t n, double beta) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    const double one = 1.0;
    HIP_OK(hipMemcpyAsync(p->dscal + 3, &beta, sizeof(double), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(p->dscal + 4, &one, sizeof(double), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));   // host scalars are stack variables
    LAUNCH_OK(launch_cg_dir(p->stream, d, r, n, p->dscal + 3, p->dscal + 4));
    return 0;
}
// cg_step + cg_dir in one call with one host synchronisation: x += s d, r -= s q, rr' = r.r, d = r + (rr'/rr) d
int surfh_cg_iter_dev(surfh_plan *p, float *x, float *r, float *d, const float *q, int64_t n, double rr_in, double *rr_out) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    HIP_OK(hipMemcpyAsync(p->dscal + 0, &rr_in, sizeof(double), hipMemcpyHostToDevice, p->stream));
    LAUNCH_OK(launch_dot(p->stream, d, q, n, p->dscratch, p->dscal + 1));
    LAUNCH_OK(launch_cg_step(p->stream, x, r, d, q, n, p->dscal + 0, p->dscal + 1, p->dscratch, p->dscal + 2));
    LAUNCH_OK(launch_cg_dir(p->stream, d, r, n, p->dscal + 2, p->dscal + 0));
    HIP_OK(hipMemcpyAsync(rr_out, p->dscal + 2, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));   // also covers the pageable rr_in copy
    return 0;
}
// ---- the same blocks with every scalar kept on the device: nothing here synchronises with the host.  The trace cg_hist IS the
// scalar store: r.r of the current iterate is its last entry, an iteration reads it there and writes the next entry (read back
// with surfh_cg_trace).  An iteration is three launches -- partial sums of d.q; step (sums them, leaves partial sums of the new
// r.r); direction (sums those) -- and no copies (round 2: five launches and two 8-byte device-to-device copies, 42 us of an
// iteration's 2.87 ms on config 3).  For the multi-GPU loop: the only other work of an iteration is the normal operator and
// the all-reduce, both asynchronous on the plan's stream.
static constexpr int CG_HIST_CAP = 1 << 16;
static int cg_hist_room(surfh_plan *p) {
    if (ensure_set(member(p->cg_hist, (size_t)CG_HIST_CAP))) return 1;
    if (p->cg_hist_n >= CG_HIST_CAP) return fail("CG trace full (%d iterations): read it with surfh_cg_trace", CG_HIST_CAP);
    return 0;
}
int surfh_cg_begin_dev(surfh_plan *p, const float *r, int64_t n) {         /* rr = r.r; trace restarts with it */
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    p->cg_hist_n = 0;
    if (cg_hist_room(p)) return 1;
    LAUNCH_OK(launch_dot(p->stream, r, r, n, p->dscratch, p->cg_hist + 0));
    p->cg_hist_n = 1;
    return 0;
}
int surfh_cg_iter_nosync_dev(surfh_plan *p, float *x, float *r, float *d, const float *q, int64_t n) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    if (p->cg_hist_n < 1) return fail("surfh_cg_iter_nosync_dev before surfh_cg_begin_dev");
    if (cg_hist_room(p)) return 1;
    double *const rr = p->cg_hist + p->cg_hist_n - 1, *const pa = p->dscratch, *const pb = p->dscratch + dot_parts_stride();
    LAUNCH_OK(launch_dot_parts(p->stream, d, q, n, pa));
    LAUNCH_OK(launch_cg_step_parts(p->stream, x, r, d, q, n, rr, pa, p->dscal + 1, pb));
    LAUNCH_OK(launch_cg_dir_parts(p->stream, d, r, n, pb, rr, rr + 1));
    ++p->cg_hist_n;
    return 0;
}
/* the residual-refresh iteration of qmm.lcg in two halves around the caller's normal operator on x:
 * x += (rr / d.q) d   ...   r = b - q; rr' = r.r; d = r + (rr' / rr) d; rr = rr'                                   */
int surfh_cg_xupdate_nosync_dev(surfh_plan *p, float *x, const float *d, const float *q, int64_t n) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    if (p->cg_hist_n < 1) return fail("surfh_cg_xupdate_nosync_dev before surfh_cg_begin_dev");
    LAUNCH_OK(launch_dot(p->stream, d, q, n, p->dscratch, p->dscal + 1));
    LAUNCH_OK(launch_cg_xupdate(p->stream, x, d, n, p->cg_hist + p->cg_hist_n - 1, p->dscal + 1));
    return 0;
}
int surfh_cg_refresh_nosync_dev(surfh_plan *p, float *r, const float *b, const float *q, float *d, int64_t n) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    if (p->cg_hist_n < 1) return fail("surfh_cg_refresh_nosync_dev before surfh_cg_begin_dev");
    if (cg_hist_room(p)) return 1;
    double *const rr = p->cg_hist + p->cg_hist_n - 1, *const pb = p->dscratch + dot_parts_stride();
    LAUNCH_OK(launch_residual(p->stream, r, b, q, n));
    LAUNCH_OK(launch_dot_parts(p->stream, r, r, n, pb));
    LAUNCH_OK(launch_cg_dir_parts(p->stream, d, r, n, pb, rr, rr + 1));
    ++p->cg_hist_n;
    return 0;
}
/* synchronises the plan's stream and copies the r.r trace (entry 0 = surfh_cg_begin_dev); returns the number of entries */
int32_t surfh_cg_trace(surfh_plan *p, double *out, int32_t cap) {
    if (!p || !out) return -1;
    if (hipSetDevice(p->dev) != hipSuccess) return -1;
    const int n = p->cg_hist_n < cap ? p->cg_hist_n : cap;
    if (hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    if (n > 0 && hipMemcpy(out, p->cg_hist, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}
int surfh_residual_dev(surfh_plan *p, float *r, const float *b, const float *q, int64_t n) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    LAUNCH_OK(launch_residual(p->stream, r, b, q, n));
    return 0;
}

// ---- what the CG and the 3MG loops share, and their frames ----
namespace {
// out = Q v = mu A^T A v (+ mu_reg prior(v)): the operator of the map- and plane-domain solvers
int normal_prior(surfh_plan *p, const float *v, float *out, double mu, double mu_reg) {
    if (normal_dev(p, v, out, mu)) return 1;
    if (mu_reg != 0.0) {
        Prof pr(p, "prior_add");
        LAUNCH_OK(prior_add(p, p->stream, v, out, p->T > 0 ? p->T : p->Lc, (float)mu_reg));
    }
    if (imager_active(p) && imager_normal_add(p, v, out)) return 1;       // + mu_imager A_im^T W_im A_im v
    return 0;
}
// the solvers that do not carry the imager term say so instead of ignoring it
int imager_refuse(const surfh_plan *p, const char *who) {
    if (p && imager_active(p))
        return fail("%s does not carry the imager data term set on this plan (surfh_set_imager_data): clear it, or use surfh_cg, "
                    "surfh_mmmg or surfh_mmmg_huber", who);
    return 0;
}
// the prior coupling acts on the maps' spatial prior only: the solvers and passes of the planes and of the cube say so
int coupling_refuse(const surfh_plan *p, const char *who) {
    if (p && p->coupling != 0)
        return fail("%s does not carry the prior coupling set on this plan (surfh_set_prior_coupling: %d): set it to 0, or use "
                    "surfh_mmmg_huber or surfh_mmmg_robust", who, p->coupling);
    return 0;
}
// cg_b = mu A^T W y (+ extra), cg_q = Q x, cg_r = cg_b - cg_q; y on the device, x already holding the start
int solver_setup(surfh_plan *p, const float *y, const float *x, double mu, double mu_reg, const float *extra = nullptr) {
    if (!(y = weighted_data(p, y))) return 1;
    if (adjoint_dev(p, y, p->cg_b)) return 1;
    if (mu != 1.0) LAUNCH_OK(launch_scale(p->stream, p->cg_b, p->isize, (float)mu));
    if (imager_active(p) && imager_rhs_add(p, p->cg_b)) return 1;           // + mu_imager A_im^T W_im y_im
    if (extra) LAUNCH_OK(launch_po_add(p->stream, p->cg_b, extra, p->isize));               // + eta (surfh_cg_sample)
    if (normal_prior(p, x, p->cg_q, mu, mu_reg)) return 1;
    LAUNCH_OK(launch_residual(p->stream, p->cg_r, p->cg_b, p->cg_q, p->isize));
    return 0;
}
// hands the iterate x (device) after iteration `it` to the callback, if any; the work buffers hold nothing live between
// iterations, so the callback may run forward / adjoint on this plan
enum { CB_GO_ON = 0, CB_ERROR = 1, CB_STOP = 2 };
int callback_iterate(surfh_plan *p, surfh_cg_callback callback, void *user, int it, const double *grad_norm, const float *x,
                     std::vector<float> &hx, long n = 0) {      // n: floats of the iterate (0: isize)
    if (!callback) return CB_GO_ON;
    if (n == 0) n = p->isize;
    hx.resize((size_t)n);
    HIP_OK(hipMemcpyAsync(hx.data(), x, n * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    if (callback(user, it, grad_norm, hx.data())) return CB_STOP;
    HIP_OK(hipSetDevice(p->dev));
    return CB_GO_ON;
}

// the start of a solver called with host buffers: x0 [isize], or zeros, to cg_x
int start_iterate(surfh_plan *p, const float *x0) {
    if (x0) HIP_OK(hipMemcpyAsync(p->cg_x, x0, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    else LAUNCH_OK(launch_fill_zero(p->stream, p->cg_x, p->isize));
    return 0;
}
// ---- the frame of every 3MG loop (the variants and what each plugs in: the 3MG sections below) ----
// Start: the work buffers (cg_hg where the variant keeps -g apart from r), y [osize] to yd, x0 or zeros to cg_x, zeros to the
// memory direction cg_d and to its image: cg_qm (with cg_dd beside it), or the caller's detector vector `am` [osize].
int mmmg_begin(surfh_plan *p, bool want_hg, const float *y, float *yd, const float *x0, float *am = nullptr) {
    hipStream_t s = p->stream;
    if (ensure_cg(p)) return 1;
    if (!am && ensure_set(member(p->cg_qm, (size_t)p->isize), member(p->cg_dd, (size_t)p->isize))) return 1;
    if (want_hg && ensure_set(member(p->cg_hg, (size_t)p->isize))) return 1;
    HIP_OK(hipMemcpyAsync(yd, y, p->osize * sizeof(float), hipMemcpyHostToDevice, s));
    if (start_iterate(p, x0)) return 1;
    LAUNCH_OK(launch_fill_zero(s, p->cg_d, p->isize));
    if (am)
        LAUNCH_OK(launch_fill_zero(s, am, p->osize));
    else
        LAUNCH_OK(launch_fill_zero(s, p->cg_qm, p->isize));
    return 0;
}
// Top of iteration `it`, once its trace entry is stored: the callback sees the iterate (it > 0), then the stopping rule on
// `norm` (the gradient norm; the largest over the planes) against scale * tol.  CB_STOP: leave the loop, the result stands.
int mmmg_check(surfh_plan *p, surfh_cg_callback callback, void *user, int it, int max_iter, const double *grad_norm, double norm,
               double scale, double tol, std::vector<float> &hx) {
    if (it > 0)
        if (const int rc = callback_iterate(p, callback, user, it, grad_norm, p->cg_x, hx)) return rc;
    return it >= max_iter || norm < scale * tol ? CB_STOP : CB_GO_ON;
}
// the carried vector (r, or u = A x) is recomputed from x in the iterations `refresh` divides
bool refresh_due(int refresh, int it) { return refresh > 0 && it % refresh == 0; }
int mmmg_finish(surfh_plan *p, float *x) {
    HIP_OK(hipMemcpyAsync(x, p->cg_x, p->isize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
// A device diagnostic of one pass: the launch under its Prof name, then k doubles from `src` (device) to `dst` (host).
int diag_pass(surfh_plan *p, const char *name, const std::function<int()> &launch, const double *src, double *dst, size_t k) {
    HIP_OK(hipSetDevice(p->dev));
    {
        Prof pr(p, name);
        LAUNCH_OK(launch());
    }
    HIP_OK(hipMemcpyAsync(dst, src, k * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- the frame of every CG loop (qmm.lcg, see oracle/surfh_oracle.py:lcg): cg_start, cg_iteration, cg_loop on a CgSpace ----
// A CgSpace is the vector space of one run: its buffers, the device scalars of an iteration and the kernels that differ.
//   maps      surfh_cg with SURFH_SPECTRAL_CG=0 or an imager term: normal_prior, one scalar per slot in dscal
//   spectra   surfh_cg, the loop bench.py times: the maps' Parseval-scaled half spectra (surfh_normal_spec_dev: no transform of the
//             maps, no padding, no prior kernel inside an iteration) under the surfh_cg_*_nosync_dev blocks, every scalar in the trace
//   planes    surfh_cg_planes, and _begin_dev / _step_dev under SURFH_PLANES_NATIVE=0: the caller's [Lc][Na][Nb] layout, normal_prior,
//             Lc scalars per slot in pl_sc
//   native    surfh_cg_planes_begin_dev / _step_dev: the cube's wavelength-innermost layout (no layout transpose inside an
//             iteration), pn_normal with d.q fused into its last kernel, LP scalars per slot in pn_sc
struct CgSpace {
    float *x, *r, *d, *q, *b;      // iterate, residual, direction, Q d, right-hand side: `len` floats each
    float *xc;                     // the iterate in the caller's layout, on the device [isize]: x itself where the layouts agree
    long len, n;                   // ... and a row of the trace meets the tolerance when sqrt(its largest r.r) < n tol
    int rows;                      // independent problems: the row length of the r.r trace
    double mu, mu_reg;
    double *rr, *dq, *rrn;         // device scalars, one per problem: r.r, d.q, the new r.r (spectra: they live in the trace)
    int (*setup)(surfh_plan *p, const CgSpace &s, const float *y, const float *x0);   // b = mu A^T W y, x = x0, r = b - Q x
    int (*rr0)(surfh_plan *p, const CgSpace &s);                                      // rr = r.r: entry 0 of the trace
    int (*apply)(surfh_plan *p, const CgSpace &s, const float *v);                    // q = Q v (native: and dq = v.q)
    int (*step)(surfh_plan *p, const CgSpace &s, int update_r);    // dq = d.q, x += (rr / dq) d; update_r: r -= (rr / dq) q, rrn = r.r
    int (*refresh)(surfh_plan *p, const CgSpace &s);               // r = b - q, rrn = r.r
    int (*dir)(surfh_plan *p, const CgSpace &s);                   // d = r + (rrn / rr) d, rr = rrn
    int (*trace)(surfh_plan *p, const CgSpace &s, double *grad_norm, int it);         // rows 0 .. it of the trace on the host
    int (*to_caller)(surfh_plan *p, const CgSpace &s);                                // xc = x in the caller's layout
    long clen = 0;                 // floats of xc the caller and the callback get (0: isize)
    // surfh_cg_sample: an extra right-hand side [isize] in the maps' layout that the set-up of the map and spectral spaces adds to b
    // (null: the launches are exactly those without it); surfh_cg_nonneg: the penalty, the operator of the nn_* applies is Q + rho I
    const float *extra = nullptr;
    double rho = 0.0;
    const float *rho_l = nullptr;  // surfh_cg_planes_nonneg: one penalty per problem, `rows` floats on the device
};
int cg_nop(surfh_plan *, const CgSpace &) { return 0; }     // to_caller: the layouts agree; dir: the step's block went on to the direction
// the maps and the planes keep the current row only: it goes to the host after every iteration
int row_trace(surfh_plan *p, const CgSpace &s, double *grad_norm, int it) {
    HIP_OK(hipMemcpyAsync(grad_norm + (size_t)it * s.rows, s.rr, s.rows * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int img_setup(surfh_plan *p, const CgSpace &s, const float *y, const float *) { return solver_setup(p, y, s.x, s.mu, s.mu_reg, s.extra); }
int img_apply(surfh_plan *p, const CgSpace &s, const float *v) { return normal_prior(p, v, s.q, s.mu, s.mu_reg); }
int maps_rr0(surfh_plan *p, const CgSpace &s) { LAUNCH_OK(launch_dot(p->stream, s.r, s.r, s.len, p->dscratch, s.rr)); return 0; }
int maps_step(surfh_plan *p, const CgSpace &s, int update_r) {
    LAUNCH_OK(launch_dot(p->stream, s.d, s.q, s.len, p->dscratch, s.dq));
    if (update_r) {
        Prof pr(p, "cg_step");
        LAUNCH_OK(launch_cg_step(p->stream, s.x, s.r, s.d, s.q, s.len, s.rr, s.dq, p->dscratch, s.rrn));
    } else LAUNCH_OK(launch_cg_xupdate(p->stream, s.x, s.d, s.len, s.rr, s.dq));
    return 0;
}
int maps_refresh(surfh_plan *p, const CgSpace &s) {
    LAUNCH_OK(launch_residual(p->stream, s.r, s.b, s.q, s.len));
    LAUNCH_OK(launch_dot(p->stream, s.r, s.r, s.len, p->dscratch, s.rrn));
    return 0;
}
int maps_dir(surfh_plan *p, const CgSpace &s) {
    LAUNCH_OK(launch_cg_dir(p->stream, s.d, s.r, s.len, s.rrn, s.rr));
    HIP_OK(hipMemcpyAsync(s.rr, s.rrn, sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    return 0;
}
CgSpace maps_space(surfh_plan *p, double mu, double mu_reg) {
    return {p->cg_x, p->cg_r, p->cg_d, p->cg_q, p->cg_b, p->cg_x, p->isize, p->isize, 1, mu, mu_reg, p->dscal + 0, p->dscal + 1, p->dscal + 2,
            img_setup, maps_rr0, img_apply, maps_step, maps_refresh, maps_dir, row_trace, cg_nop};
}
int spec_setup(surfh_plan *p, const CgSpace &s, const float *y, const float *x0) {
    const float *wy = weighted_data(p, y);
    if (!wy || surfh_adjoint_spec_dev(p, wy, s.b, s.mu, nullptr, 0.0)) return 1;
    if (s.extra) {                                                                          // + eta (surfh_cg_sample), s.q still free
        if (surfh_to_spec_dev(p, s.extra, s.q)) return 1;
        LAUNCH_OK(launch_po_add(p->stream, s.b, s.q, s.len));
    }
    if (x0) {
        if (surfh_to_spec_dev(p, x0, s.x) || surfh_normal_spec_dev(p, s.x, s.q, s.mu, s.mu_reg)) return 1;
        LAUNCH_OK(launch_residual(p->stream, s.r, s.b, s.q, s.len));
    } else {                                                                                // r = b - Q 0
        LAUNCH_OK(launch_fill_zero(p->stream, s.x, s.len));
        HIP_OK(hipMemcpyAsync(s.r, s.b, s.len * sizeof(float), hipMemcpyDeviceToDevice, p->stream));
    }
    return 0;
}
int spec_rr0(surfh_plan *p, const CgSpace &s) { return surfh_cg_begin_dev(p, s.r, s.len); }
int spec_apply(surfh_plan *p, const CgSpace &s, const float *v) { return surfh_normal_spec_dev(p, v, s.q, s.mu, s.mu_reg); }
int spec_step(surfh_plan *p, const CgSpace &s, int update_r) {
    return update_r ? surfh_cg_iter_nosync_dev(p, s.x, s.r, s.d, s.q, s.len) : surfh_cg_xupdate_nosync_dev(p, s.x, s.d, s.q, s.len);
}
int spec_refresh(surfh_plan *p, const CgSpace &s) { return surfh_cg_refresh_nosync_dev(p, s.r, s.b, s.q, s.d, s.len); }
int spec_trace(surfh_plan *p, const CgSpace &, double *grad_norm, int it) {                // synchronises
    return surfh_cg_trace(p, grad_norm, it + 1) != it + 1 ? fail("CG trace read failed") : 0;
}
int spec_to_caller(surfh_plan *p, const CgSpace &s) { return surfh_from_spec_dev(p, s.x, s.xc); }
CgSpace spectral_space(surfh_plan *p, double mu, double mu_reg) {
    return {p->cg_x, p->cg_r, p->cg_d, p->cg_q, p->cg_b, p->io_x, 2L * p->T * p->PL, p->isize, 1, mu, mu_reg, nullptr, nullptr, nullptr,
            spec_setup, spec_rr0, spec_apply, spec_step, spec_refresh, cg_nop, spec_trace, spec_to_caller};
}
int planes_rr0(surfh_plan *p, const CgSpace &s) { LAUNCH_OK(launch_dot_planes(p->stream, s.r, s.r, s.rows, s.n, s.rr)); return 0; }
int planes_step(surfh_plan *p, const CgSpace &s, int update_r) {
    LAUNCH_OK(launch_dot_planes(p->stream, s.d, s.q, s.rows, s.n, s.dq));
    LAUNCH_OK(launch_cg_step_planes(p->stream, s.x, s.r, s.d, s.q, s.rows, s.n, s.rr, s.dq, s.rrn, update_r));
    return 0;
}
int planes_refresh(surfh_plan *p, const CgSpace &s) {
    LAUNCH_OK(launch_residual(p->stream, s.r, s.b, s.q, s.len));
    LAUNCH_OK(launch_dot_planes(p->stream, s.r, s.r, s.rows, s.n, s.rrn));
    return 0;
}
int planes_dir(surfh_plan *p, const CgSpace &s) { LAUNCH_OK(launch_cg_dir_planes(p->stream, s.d, s.r, s.rows, s.n, s.rrn, s.rr)); return 0; }
CgSpace planes_space(surfh_plan *p, float *x, double mu, double mu_reg) {
    const int L = p->Lc;
    return {x, p->cg_r, p->cg_d, p->cg_q, p->cg_b, x, p->isize, (long)p->Na * p->Nb, L, mu, mu_reg, p->pl_sc, p->pl_sc + L, p->pl_sc + 2 * L,
            img_setup, planes_rr0, img_apply, planes_step, planes_refresh, planes_dir, row_trace, cg_nop};
}
// q = mu A^T A v (+ mu_reg prior, fused with the dot product v . q -> dq) on wavelength-innermost vectors
int pn_normal(surfh_plan *p, const float *v, float *q, double *dq) {
    // with interleaved spectra and a prior weight the OTF product of the adjoint applies mu and adds the prior (adjoint_tail): the
    // two halves are called directly so that no scaling pass follows
    // (plans whose inverse transform forms the OTF product in its loader -- Route::prod -- take mu and the prior on that pass)
    // The fold is decided on what the folding kernel sees, in fp32: the OTF product applies mu only beside a prior weight that is
    // non-zero, and the loader scales by mu and carries the prior as (mu_reg / mu) times its third operand, which needs a non-zero
    // mu and a finite ratio.  Every other call takes the unfolded operator, the scaling pass and the prior kernel.
    const bool prod = p->route.prod && (float)p->pl_mu != 0.f && p->pl_mu_reg / p->pl_mu <= 3.4028234e38;
    const bool fold = prod || (!p->route.prod && p->route.interleaved() && (float)p->pl_mu_reg != 0.f);
    if (fold) {
        OpCall c;
        c.head = OpCall::H_CUBE; c.tail = OpCall::T_CUBE; c.fold = true; c.mu = p->pl_mu; c.prior_mu = p->pl_mu_reg;
        if (normal_halves(p, v, q, c)) return 1;
    } else if (normal_dev(p, v, q, p->pl_mu, true)) {
        return 1;
    }
    Prof pr(p, "pn_prior_dot");
    if (fold) LAUNCH_OK(launch_pn_dot(p->stream, v, q, p->Na, p->Nb, p->NAP, p->LP, p->pn_part, dq));
    else LAUNCH_OK(launch_pn_prior_dot(p->stream, v, q, p->Na, p->Nb, p->NAP, p->LP, (float)p->pl_mu_reg, p->pn_part, dq));
    return 0;
}
bool pn_capable(const surfh_plan *p) {
    const bool on = env_on("SURFH_PLANES_NATIVE", true);       // 0: vectors in the caller's [Lc][Na][Nb] layout (two transposes per operator application)
    return on && p->T == 0 && p->segs.size() == 1 && p->segs[0].coff == 0 && p->segs[0].start == 0 && p->Lown == p->Lc && p->prior_kind == 0 &&
           p->LP % 64 == 0;
}
int pn_setup(surfh_plan *p, const CgSpace &s, const float *y, const float *x0) {     // mu and mu_reg: the plan's pl_mu, pl_mu_reg
    LAUNCH_OK(launch_cube_to_lam_inner(p->stream, x0, s.x, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP));
    const float *wy = weighted_data(p, y);
    OpCall c;
    c.tail = OpCall::T_CUBE;
    if (!wy || adjoint_dev(p, wy, s.b, c)) return 1;
    if (s.mu != 1.0) LAUNCH_OK(launch_scale(p->stream, s.b, s.len, (float)s.mu));
    if (pn_normal(p, s.x, s.q, s.dq)) return 1;
    LAUNCH_OK(launch_residual(p->stream, s.r, s.b, s.q, s.len));
    return 0;
}
int pn_rr0(surfh_plan *p, const CgSpace &s) { LAUNCH_OK(launch_pn_dot(p->stream, s.r, s.r, p->Na, p->Nb, p->NAP, p->LP, p->pn_part, s.rr)); return 0; }
int pn_apply(surfh_plan *p, const CgSpace &s, const float *v) { return pn_normal(p, v, s.q, s.dq); }
int pn_step(surfh_plan *p, const CgSpace &s, int update_r) {
    std::optional<Prof> pr;
    if (update_r) pr.emplace(p, "pn_step");
    LAUNCH_OK(launch_pn_step(p->stream, s.x, s.r, s.d, s.q, p->Na, p->Nb, p->NAP, p->LP, s.rr, s.dq, p->pn_part, s.rrn, update_r));
    return 0;
}
int pn_refresh(surfh_plan *p, const CgSpace &s) {
    LAUNCH_OK(launch_residual(p->stream, s.r, s.b, s.q, s.len));
    LAUNCH_OK(launch_pn_dot(p->stream, s.r, s.r, p->Na, p->Nb, p->NAP, p->LP, p->pn_part, s.rrn));
    return 0;
}
int pn_dir(surfh_plan *p, const CgSpace &s) {
    {
        Prof pr(p, "pn_dir");
        LAUNCH_OK(launch_pn_dir(p->stream, s.d, s.r, p->Na, p->Nb, p->NAP, p->LP, s.rrn, s.rr));
    }
    HIP_OK(hipMemcpyAsync(s.rr, s.rrn, (size_t)p->LP * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    return 0;
}
int pn_to_caller(surfh_plan *p, const CgSpace &s) {
    LAUNCH_OK(launch_cube_from_lam_inner(p->stream, s.x, s.xc, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP));
    return 0;
}
// what an entry point of the plane-wise CG checks and allocates before it builds its space
int cg_planes_ready(surfh_plan *p, const char *who, bool native) {
    if (imager_refuse(p, who)) return 1;
    if (p->T != 0) return fail("surfh_cg_planes is the solver of the plane-wise (no template) model; use surfh_cg with templates");
    if (p->ch.empty()) return fail("plan has no channel");
    HIP_OK(hipSetDevice(p->dev));
    if (!native) return ensure_cg(p) || ensure_set(member(p->pl_sc, (size_t)3 * p->Lc));
    // vectors in the cube's layout: the caller's x is transposed in here and out again at the end of every step call
    const size_t nc = (size_t)p->NBP * p->NAP * p->LP;
    return ensure_set_with(
        [&](float *v0, float *v1, float *v2, float *v3, float *v4, double *, double *) {
            // The padding (rows >= Nb, columns >= Na, planes >= Lc) starts at zero.  It stays zero where beta runs on dft_h2 or dense;
            // where beta runs on dft_ct the real passes transform the planes (l, l ^ 1) as one complex column, and the separation
            // leaves a plane some 1e-7 of its partner: the padding plane beside an odd Lc, and q of an all-zero plane, hold such
            // values (finite; the sums of the padding wavelengths are never read)
            for (float *v : {v0, v1, v2, v3, v4})
                if (dev_raw_clear(v, nc * sizeof(float), p->stream, true)) return 1;
            return 0;
        },
        member(p->pn_v[0], nc), member(p->pn_v[1], nc), member(p->pn_v[2], nc), member(p->pn_v[3], nc), member(p->pn_v[4], nc),
        member(p->pn_sc, (size_t)3 * p->LP), member(p->pn_part, pn_part_doubles(p->LP)));
}
// the plane space surfh_cg_planes_begin_dev chose, from what it left in the plan (pn_active, pl_x, pl_mu, pl_mu_reg)
CgSpace stored_space(surfh_plan *p) {
    if (!p->pn_active) return planes_space(p, p->pl_x, p->pl_mu, p->pl_mu_reg);
    const DevBuf<float> *v = p->pn_v;
    return {v[0], v[1], v[2], v[3], v[4], p->pl_x, (long)p->NBP * p->NAP * p->LP, (long)p->Na * p->Nb, p->Lc, p->pl_mu, p->pl_mu_reg,
            p->pn_sc, p->pn_sc + p->LP, p->pn_sc + 2 * p->LP, pn_setup, pn_rr0, pn_apply, pn_step, pn_refresh, pn_dir, row_trace, pn_to_caller};
}

// y and x0 on the device, x0 in the caller's layout (s.xc; the spectra take NULL for zeros): b, r = b - Q x, d = r, trace entry 0
int cg_start(surfh_plan *p, const CgSpace &s, const float *y, const float *x0) {
    if (s.setup(p, s, y, x0)) return 1;
    HIP_OK(hipMemcpyAsync(s.d, s.r, s.len * sizeof(float), hipMemcpyDeviceToDevice, p->stream));
    return s.rr0(p, s);
}
// iteration `it` of qmm.lcg, nothing read by the host; the residual is recomputed from x in the iterations `refresh` divides
int cg_iteration(surfh_plan *p, const CgSpace &s, int it, int refresh) {
    const bool fresh = refresh_due(refresh, it);
    if (s.apply(p, s, s.d) || s.step(p, s, fresh ? 0 : 1)) return 1;
    if (fresh && (s.apply(p, s, s.x) || s.refresh(p, s))) return 1;
    return s.dir(p, s);
}
// The iterations after cg_start and the copy-out to x [isize].  The host reads the trace -- the stopping test of qmm.lcg, on the
// worst problem of a row -- every `check` iterations (1 where the space keeps one row: row_trace) and at max_iter: the loop may run
// up to check - 1 iterations past the one that met the tolerance (nit and x are those of the last iteration run, grad_norm holds
// every r.r).  With a callback the trace so far [it + 1][rows] and the iterate go to the host after every iteration, as its contract says.
constexpr int CG_CHECK = 8;
int cg_loop(surfh_plan *p, const CgSpace &s, int32_t max_iter, double tol, int32_t refresh, int check, float *x, double *grad_norm,
            int32_t *nit, surfh_cg_callback callback, void *user) {
    std::vector<float> hx;             // host copy of the iterate handed to the callback
    if (callback) check = 1;
    if (s.trace(p, s, grad_norm, 0)) return 1;
    *nit = 0;
    for (int it = 0; it < max_iter; ++it) {
        if (cg_iteration(p, s, it, refresh)) return 1;
        *nit = it + 1;
        if ((it + 1) % check != 0 && it + 1 != max_iter) continue;
        if (s.trace(p, s, grad_norm, it + 1) || (callback && s.to_caller(p, s))) return 1;
        if (const int rc = callback_iterate(p, callback, user, it + 1, grad_norm, s.xc, hx, s.clen)) {
            if (rc == CB_STOP) break;
            return 1;
        }
        const double *gn = grad_norm + (size_t)(it + 1) * s.rows;
        if (std::sqrt(*std::max_element(gn, gn + s.rows)) < (double)s.n * tol) break;
    }
    if (s.to_caller(p, s)) return 1;
    if (x) HIP_OK(hipMemcpyAsync(x, s.xc, (s.clen ? s.clen : p->isize) * sizeof(float), hipMemcpyDeviceToHost, p->stream));   // NULL: it stays in s.xc
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
}  // namespace

namespace {
// the vectors of surfh_cg are the maps' spectra unless SURFH_SPECTRAL_CG=0, or an imager term (not diagonal in that basis)
bool cg_spectral(surfh_plan *p, int32_t max_iter) {
    return env_on("SURFH_SPECTRAL_CG", true) && !imager_active(p) && surfh_spec_supported(p) && max_iter < (1 << 16) - 1;
}
// surfh_cg_cb behind its argument checks; y NULL: the data are in io_y already (the perturbed data of surfh_cg_sample, `extra` its
// extra right-hand side on the device)
int cg_run(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol, int32_t refresh, float *x,
           double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user, const float *extra = nullptr) {
    HIP_OK(hipSetDevice(p->dev));
    if (ensure_cg(p)) return 1;
    const bool spectral = cg_spectral(p, max_iter);
    CgSpace s = spectral ? spectral_space(p, mu, mu_reg) : maps_space(p, mu, mu_reg);
    s.extra = extra;
    if (y) HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (spectral && x0) HIP_OK(hipMemcpyAsync(s.xc, x0, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if ((!spectral && start_iterate(p, x0)) || cg_start(p, s, p->io_y, x0 ? s.xc : nullptr)) return 1;
    return cg_loop(p, s, max_iter, tol, refresh, spectral ? CG_CHECK : 1, x, grad_norm, nit, callback, user);
}
}  // namespace

int surfh_cg_cb(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                int32_t refresh, float *x, double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (p->T <= 0) return fail("surfh_cg needs templates (the priors act on abundance maps)");
    return cg_run(p, y, mu, mu_reg, x0, max_iter, tol, refresh, x, grad_norm, nit, callback, user);
}

int surfh_cg(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
             int32_t refresh, float *x, double *grad_norm, int32_t *nit) {
    return surfh_cg_cb(p, y, mu, mu_reg, x0, max_iter, tol, refresh, x, grad_norm, nit, nullptr, nullptr);
}

// ---- template refinement: the CG of surfh_cg on the spectra, maps held fixed ----
// Q_S = mu A_x^T W A_x + mu_spec D^T D on S [T][Lc] (cube-plane order; D the open first difference along the wavelength), right-hand
// side mu A_x^T W y: one more CgSpace on the frame above, with the maps' vector kernels on T Lc floats.  The maps stay in cg_x, their
// spectra in mhat (computed once per solve; again after a callback, which may have run the operators on this plan), and an
// application of Q_S puts its argument in the templates' place -- the plan's own come back through TplScope on every exit, and
// before every callback.
namespace {
int tpl_apply(surfh_plan *p, const CgSpace &s, const float *v) {
    if (tpl_install(p, v) || tpl_normal_dev(p, p->cg_x, s.q)) return 1;
    p->tg_mhat_ready = true;
    if (s.mu != 1.0) LAUNCH_OK(launch_scale(p->stream, s.q, s.len, (float)s.mu));
    if (s.mu_reg != 0.0) {
        Prof pr(p, "tpl_prior_add");
        LAUNCH_OK(launch_tpl_prior_add(p->stream, v, s.q, p->T, p->Lc, (float)s.mu_reg));
    }
    return 0;
}
int tpl_setup(surfh_plan *p, const CgSpace &s, const float *y, const float *) {       // s.x holds the start
    if (!(y = weighted_data(p, y))) return 1;
    if (tpl_adjoint_dev(p, p->cg_x, y, s.b)) return 1;
    p->tg_mhat_ready = true;
    if (s.mu != 1.0) LAUNCH_OK(launch_scale(p->stream, s.b, s.len, (float)s.mu));
    if (tpl_apply(p, s, s.x)) return 1;
    LAUNCH_OK(launch_residual(p->stream, s.r, s.b, s.q, s.len));
    return 0;
}
int tpl_to_caller(surfh_plan *p, const CgSpace &) {       // what follows may run the operators on this plan: its own templates, fresh spectra
    HIP_OK(hipMemcpyAsync(p->tpl, p->tg_keep, (size_t)p->T * p->LP * sizeof(float), hipMemcpyDeviceToDevice, p->stream));
    p->tg_mhat_ready = false;
    return 0;
}
CgSpace tpl_space(surfh_plan *p, double mu, double mu_spec) {
    const DevBuf<float> *v = p->tg_v;
    const long n = (long)p->T * p->Lc;
    return {v[0], v[1], v[2], v[3], v[4], v[0], n, n, 1, mu, mu_spec, p->dscal + 0, p->dscal + 1, p->dscal + 2,
            tpl_setup, maps_rr0, tpl_apply, maps_step, maps_refresh, maps_dir, row_trace, tpl_to_caller, n};
}
}  // namespace

int surfh_cg_templates_cb(surfh_plan *p, const float *y, const float *maps, double mu, double mu_spec, const float *s0, int32_t max_iter,
                          double tol, int32_t refresh, float *s_out, double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user) {
    if (!p || !y || !maps || !s_out || !grad_norm || !nit) return fail("null argument");
    if (p->im_g)
        return fail("surfh_cg_templates does not carry the imager data term, and the attached imager was built from the plan's templates: "
                    "detach it (surfh_set_imager(plan, NULL)) first");
    if (!(mu >= 0.0 && mu <= DBL_MAX) || !(mu_spec >= 0.0 && mu_spec <= DBL_MAX)) return fail("surfh_cg_templates: mu and mu_spec must be finite and >= 0");
    HIP_OK(hipSetDevice(p->dev));
    if (tpl_ensure(p) || ensure_cg(p)) return 1;
    const CgSpace s = tpl_space(p, mu, mu_spec);
    std::vector<float> h((size_t)s.len);
    if (s0) std::copy(s0, s0 + s.len, h.begin());
    else for (long i = 0; i < s.len; ++i) h[i] = (float)p->tpl_host[i];
    HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(p->cg_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(s.x, h.data(), s.len * sizeof(float), hipMemcpyHostToDevice, p->stream));
    TplScope sc(p);
    if (sc.begin() || cg_start(p, s, p->io_y, nullptr)) return 1;
    return cg_loop(p, s, max_iter, tol, refresh, 1, s_out, grad_norm, nit, callback, user);
}
int surfh_cg_templates(surfh_plan *p, const float *y, const float *maps, double mu, double mu_spec, const float *s0, int32_t max_iter,
                       double tol, int32_t refresh, float *s_out, double *grad_norm, int32_t *nit) {
    return surfh_cg_templates_cb(p, y, maps, mu, mu_spec, s0, max_iter, tol, refresh, s_out, grad_norm, nit, nullptr, nullptr);
}

// ---- non-negative fusion: ADMM in scaled form around the CG frame (kernels and conventions: nonneg.hip) ----
//   min x^T Q x / 2 - b^T x, x >= 0, with Q and b those of the space's own solver:  x = z, z >= 0, scaled dual u, v = z - u, rho fixed.
//   x = x0, z = max(x0, 0), u = 0;  r = b + rho v - (Q + rho I) x;  per outer iteration:  d = r and `inner` cg_iteration on Q + rho I
//   (the space's apply, then q += rho d), no refresh inside;  z' = max(x + u, 0), u' = u + x - z' (nn_project);  r += rho (v' - v), or
//   r = b + rho v' - (Q + rho I) x every `refresh` outer iterations;  trace row = |x - z'|^2, rho^2 |z' - z|^2, r.r, #{z' == 0};
//   stop when sqrt(max(rho^2 row[0], row[1])) < n tol.  The result is z: feasible by construction.
// The spectra keep x, r, d in their basis (orthonormal: rho I stays rho I) and z, u on the pixels: x goes there through
// surfh_from_spec_dev, nn_project leaves dv = rho (v' - v), which comes back through surfh_to_spec_dev.
namespace {
struct NnScope {                       // the extra vectors never outlive a solve
    surfh_plan *p;
    explicit NnScope(surfh_plan *pl) : p(pl) {}
    int begin(long n) {
        const size_t pitch = ((size_t)n + 3) / 4 * 4;      // each vector 16-byte aligned
        if (p->nn_z.alloc(3 * pitch)) return 1;
        p->nn_u = p->nn_z + pitch;
        p->nn_w = p->nn_u + pitch;
        return 0;
    }
    // the plane-wise solve: z and u [L][npix] (no work vector: the pass is the fused one), the penalties as floats, the partial
    // sums of the pass with its [4][L] sums behind them
    int begin_planes(int L, long npix, const double *rho) {
        const size_t pitch = ((size_t)L * npix + 3) / 4 * 4, parts = nn_planes_part_doubles(L, npix);
        std::vector<float> h(rho, rho + L);
        if (p->nn_z.alloc(2 * pitch) || p->nn_part.alloc(parts + (size_t)4 * L) || p->nn_rho.upload(h)) return 1;
        p->nn_u = p->nn_z + pitch;
        p->nn_sums = p->nn_part + parts;
        return 0;
    }
    ~NnScope() {
        if (p->nn_z || p->nn_part || p->nn_rho) {
            hipStreamSynchronize(p->stream);
            p->nn_z.reset();
            p->nn_part.reset();
            p->nn_rho.reset();
        }
        p->nn_u = p->nn_w = nullptr;
        p->nn_sums = nullptr;
    }
};
int nn_rho_add(surfh_plan *p, const CgSpace &s, const float *v) {                           // q += rho v: the operator is Q + rho I
    LAUNCH_OK(launch_nn_add(p->stream, s.q, v, nullptr, s.len, (float)s.rho));
    return 0;
}
int nn_img_apply(surfh_plan *p, const CgSpace &s, const float *v) { return img_apply(p, s, v) || nn_rho_add(p, s, v); }
int nn_spec_apply(surfh_plan *p, const CgSpace &s, const float *v) { return spec_apply(p, s, v) || nn_rho_add(p, s, v); }
int nn_tpl_apply(surfh_plan *p, const CgSpace &s, const float *v) { return tpl_apply(p, s, v) || nn_rho_add(p, s, v); }
int nn_refuse(const char *who, double rho, int32_t outer, int32_t inner) {
    if (!(rho > 0.0 && rho <= DBL_MAX)) return fail("%s: rho = %g must be finite and > 0", who, rho);
    if (inner < 1) return fail("%s: inner = %d (at least 1)", who, inner);
    if (outer < 0) return fail("%s: outer = %d", who, outer);
    return 0;
}
// r += c (a - b) for pixel vectors a, b where r lives in the spectra (through nn_w and s.q, both free between iterations)
int nn_spec_add(surfh_plan *p, const CgSpace &s, const float *a, const float *b, long m, double c) {
    Prof pr(p, "nn_spec");
    LAUNCH_OK(launch_fill_zero(p->stream, p->nn_w, m));
    LAUNCH_OK(launch_nn_add(p->stream, p->nn_w, a, b, m, 1.f));
    if (surfh_to_spec_dev(p, p->nn_w, s.q)) return 1;
    LAUNCH_OK(launch_nn_add(p->stream, s.r, s.q, nullptr, s.len, (float)c));
    return 0;
}
// After cg_start on `s` (r = b - Q x, trace entry 0) inside an NnScope.  `sx`: s with its penalty rho, and rho v added by its apply; spectral: x, r, d are spectra and
// s.xc the pixels; h0 [m]: the start on the host (NULL: zeros), m the floats of z.  out [m], trace [outer + 1][4]
int nn_loop(surfh_plan *p, const CgSpace &s, const CgSpace &sx, bool spectral, const float *h0, long m, int32_t outer, int32_t inner,
            double tol, int32_t refresh, float *out, double *trace, int32_t *nit) {
    hipStream_t st = p->stream;
    const double rho = sx.rho;
    double *const sums = p->dscal + 8;
    const float *const xp = spectral ? s.xc : s.x;                                         // the iterate on the pixels
    double pp0 = 0.0, active0 = (double)m;
    HIP_OK(hipMemsetAsync(p->nn_u, 0, m * sizeof(float), st));
    if (h0) {
        std::vector<float> hz((size_t)m);
        active0 = 0.0;
        for (long i = 0; i < m; ++i) {
            hz[i] = h0[i] > 0.f ? h0[i] : 0.f;
            const double e = (double)h0[i] - (double)hz[i];
            pp0 += e * e;
            active0 += hz[i] == 0.f ? 1.0 : 0.0;
        }
        HIP_OK(hipMemcpyAsync(p->nn_z, hz.data(), m * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));                                                   // hz leaves scope
        if (pp0 > 0.0) {                                                                    // r += rho (z - x): v = z, and the rho x of the operator
            if (spectral) {
                if (nn_spec_add(p, s, p->nn_z, xp, m, rho)) return 1;
            } else LAUNCH_OK(launch_nn_add(st, s.r, p->nn_z, xp, m, (float)rho));
            if (s.rr0(p, s)) return 1;
        }
    } else HIP_OK(hipMemsetAsync(p->nn_z, 0, m * sizeof(float), st));
    double rr = 0.0;
    if (s.trace(p, s, &rr, 0)) return 1;
    trace[0] = pp0; trace[1] = 0.0; trace[2] = rr; trace[3] = active0;
    *nit = 0;
    for (int k = 0; k < outer; ++k) {
        HIP_OK(hipMemcpyAsync(s.d, s.r, s.len * sizeof(float), hipMemcpyDeviceToDevice, st));
        for (int j = 0; j < inner; ++j)
            if (cg_iteration(p, sx, j, 0)) return 1;
        if (spectral) {
            Prof pr(p, "nn_spec");
            if (surfh_from_spec_dev(p, s.x, s.xc)) return 1;
        }
        {
            Prof pr(p, "nn_project");
            LAUNCH_OK(launch_nn_project(st, xp, p->nn_z, p->nn_u, spectral ? nullptr : s.r, spectral ? p->nn_w : nullptr, m, (float)rho,
                                        p->dscratch, sums));
        }
        const bool fresh = refresh_due(refresh, k + 1);
        if (fresh) {                                                                        // r = b + rho v' - (Q + rho I) x
            if (sx.apply(p, sx, s.x)) return 1;
            LAUNCH_OK(launch_residual(st, s.r, s.b, s.q, s.len));
            if (spectral) {
                if (nn_spec_add(p, s, p->nn_z, p->nn_u, m, rho)) return 1;
            } else LAUNCH_OK(launch_nn_add(st, s.r, p->nn_z, p->nn_u, m, (float)rho));
        } else if (spectral) {                                                              // r += dv in the spectra
            Prof pr(p, "nn_spec");
            if (surfh_to_spec_dev(p, p->nn_w, s.q)) return 1;
            LAUNCH_OK(launch_nn_add(st, s.r, s.q, nullptr, s.len, 1.f));
        }
        if (spectral || fresh) {
            if (s.rr0(p, s)) return 1;
        } else HIP_OK(hipMemcpyAsync(s.rr, sums + 3, sizeof(double), hipMemcpyDeviceToDevice, st));    // the pass summed the new r.r
        double h[4];
        HIP_OK(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, st));
        if (s.trace(p, s, &rr, 0)) return 1;                                                // synchronises
        double *row = trace + 4 * (size_t)(k + 1);
        row[0] = h[0]; row[1] = rho * rho * h[1]; row[2] = rr; row[3] = h[2];
        *nit = k + 1;
        if (std::sqrt(std::max(rho * rho * row[0], row[1])) < (double)s.n * tol) break;
    }
    HIP_OK(hipMemcpyAsync(out, p->nn_z, m * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}
}  // namespace

int surfh_cg_nonneg(surfh_plan *p, const float *y, double mu, double mu_reg, double rho, const float *x0, int32_t outer, int32_t inner,
                    double tol, int32_t refresh, float *x, double *trace, int32_t *nit) {
    if (!p || !y || !x || !trace || !nit) return fail("null argument");
    if (nn_refuse("surfh_cg_nonneg", rho, outer, inner)) return 1;
    if (p->T <= 0) return fail("surfh_cg_nonneg needs templates (the constraint is on the abundance maps)");
    if (imager_refuse(p, "surfh_cg_nonneg")) return 1;
    HIP_OK(hipSetDevice(p->dev));
    if (ensure_cg(p)) return 1;
    const bool spectral = cg_spectral(p, inner);
    const CgSpace s = spectral ? spectral_space(p, mu, mu_reg) : maps_space(p, mu, mu_reg);
    CgSpace sx = s;
    sx.apply = spectral ? nn_spec_apply : nn_img_apply;
    sx.rho = rho;
    HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (spectral && x0) HIP_OK(hipMemcpyAsync(s.xc, x0, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if ((!spectral && start_iterate(p, x0)) || cg_start(p, s, p->io_y, x0 ? s.xc : nullptr)) return 1;
    NnScope sc(p);
    if (sc.begin(p->isize)) return 1;
    return nn_loop(p, s, sx, spectral, x0, p->isize, outer, inner, tol, refresh, x, trace, nit);
}

int surfh_cg_templates_nonneg(surfh_plan *p, const float *y, const float *maps, double mu, double mu_spec, double rho, const float *s0,
                              int32_t outer, int32_t inner, double tol, int32_t refresh, float *s_out, double *trace, int32_t *nit) {
    if (!p || !y || !maps || !s_out || !trace || !nit) return fail("null argument");
    if (nn_refuse("surfh_cg_templates_nonneg", rho, outer, inner)) return 1;
    if (p->im_g)
        return fail("surfh_cg_templates_nonneg does not carry the imager data term, and the attached imager was built from the plan's "
                    "templates: detach it (surfh_set_imager(plan, NULL)) first");
    if (!(mu >= 0.0 && mu <= DBL_MAX) || !(mu_spec >= 0.0 && mu_spec <= DBL_MAX))
        return fail("surfh_cg_templates_nonneg: mu and mu_spec must be finite and >= 0");
    HIP_OK(hipSetDevice(p->dev));
    if (tpl_ensure(p) || ensure_cg(p)) return 1;
    const CgSpace s = tpl_space(p, mu, mu_spec);
    CgSpace sx = s;
    sx.apply = nn_tpl_apply;
    sx.rho = rho;
    std::vector<float> h((size_t)s.len);
    if (s0) std::copy(s0, s0 + s.len, h.begin());
    else for (long i = 0; i < s.len; ++i) h[i] = (float)p->tpl_host[i];
    HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(p->cg_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(s.x, h.data(), s.len * sizeof(float), hipMemcpyHostToDevice, p->stream));
    TplScope tsc(p);
    NnScope sc(p);
    if (tsc.begin() || cg_start(p, s, p->io_y, nullptr) || sc.begin(s.len)) return 1;
    return nn_loop(p, s, sx, false, h.data(), s.len, outer, inner, tol, refresh, s_out, trace, nit);
}

// ---- the same on independent planes: s.rows problems min x_l^T Q_l x_l / 2 - b_l^T x_l, x_l >= 0 on planes_space, each with its own
// penalty rho_l, its own trace and its own stopping test.  nn_loop stays as it is (one rho, one trace row, the launches of the single
// problem); this sibling differs in what is per plane: nn_project_planes sums per plane, nn_add_planes scales per plane, the host
// reads one [4][rows] block per outer iteration.  The loop ends when EVERY plane meets sqrt(max(rho_l^2 row0_l, row1_l)) < n tol;
// a plane that met it earlier keeps iterating with the others (nothing is frozen: the batched operator runs on all planes anyway,
// so stopping one plane would save nothing).  A plane with b_l = 0 from x0_l = 0 has r = d = 0: the step kernels' d.q = 0 and rr = 0
// guards keep it at rest, the pass returns zeros, its trace is finite.
namespace {
int nn_planes_apply(surfh_plan *p, const CgSpace &s, const float *v) {                     // q_l = Q_l v_l + rho_l v_l
    if (img_apply(p, s, v)) return 1;
    Prof pr(p, "nn_rho_add");
    LAUNCH_OK(launch_nn_add_planes(p->stream, s.q, v, nullptr, s.rows, s.n, s.rho_l, 1.f));
    return 0;
}
// After cg_start on planes_space (r = b - Q x, trace entry 0) inside an NnScope begun with begin_planes.  `s`: that space with its
// penalties rho_l and nn_planes_apply; h0: the start on the host (NULL: zeros); out [len]; trace [outer + 1][4][rows], the four
// rows in nn_loop's order: |x - z'|^2, rho^2 |z' - z|^2, r.r, #{z' == 0}
int nn_planes_loop(surfh_plan *p, const CgSpace &s, const double *rho, const float *h0, int32_t outer, int32_t inner,
                   double tol, int32_t refresh, float *out, double *trace, int32_t *nit) {
    hipStream_t st = p->stream;
    const int L = s.rows;
    const long npix = s.n, m = s.len;
    double *const sums = p->nn_sums;
    std::vector<double> h((size_t)4 * L, 0.0);             // row 0 in the trace's order, then the pass's sums in theirs (count before r.r)
    for (int l = 0; l < L; ++l) h[3 * (size_t)L + l] = (double)npix;                       // row 0: nothing of z = 0 is positive
    HIP_OK(hipMemsetAsync(p->nn_u, 0, m * sizeof(float), st));
    if (h0) {
        std::vector<float> hz((size_t)m);
        bool infeasible = false;
        for (int l = 0; l < L; ++l) {
            double pp = 0.0, active = 0.0;
            for (long i = (long)l * npix; i < (long)(l + 1) * npix; ++i) {
                hz[i] = h0[i] > 0.f ? h0[i] : 0.f;
                const double e = (double)h0[i] - (double)hz[i];
                pp += e * e;
                active += hz[i] == 0.f ? 1.0 : 0.0;
            }
            h[l] = pp;
            h[3 * (size_t)L + l] = active;
            infeasible = infeasible || pp > 0.0;
        }
        HIP_OK(hipMemcpyAsync(p->nn_z, hz.data(), m * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));                                                   // hz leaves scope
        if (infeasible) {                                                                   // r_l += rho_l (z_l - x_l), 0 where x0_l >= 0
            LAUNCH_OK(launch_nn_add_planes(st, s.r, p->nn_z, s.x, L, npix, s.rho_l, 1.f));
            if (s.rr0(p, s)) return 1;
        }
    } else HIP_OK(hipMemsetAsync(p->nn_z, 0, m * sizeof(float), st));
    if (s.trace(p, s, h.data() + 2 * (size_t)L, 0)) return 1;                               // r.r per plane; synchronises
    std::copy(h.begin(), h.end(), trace);
    *nit = 0;
    for (int k = 0; k < outer; ++k) {
        HIP_OK(hipMemcpyAsync(s.d, s.r, m * sizeof(float), hipMemcpyDeviceToDevice, st));
        for (int j = 0; j < inner; ++j)
            if (cg_iteration(p, s, j, 0)) return 1;
        {
            Prof pr(p, "nn_project");
            LAUNCH_OK(launch_nn_project_planes(st, s.x, p->nn_z, p->nn_u, s.r, L, npix, s.rho_l, p->nn_part, sums));
        }
        if (refresh_due(refresh, k + 1)) {                                                  // r = b + rho v' - (Q + rho I) x, its r.r to the sums
            if (s.apply(p, s, s.x)) return 1;
            LAUNCH_OK(launch_residual(st, s.r, s.b, s.q, m));
            LAUNCH_OK(launch_nn_add_planes(st, s.r, p->nn_z, p->nn_u, L, npix, s.rho_l, 1.f));
            if (s.rr0(p, s)) return 1;
            HIP_OK(hipMemcpyAsync(sums + 3 * (size_t)L, s.rr, L * sizeof(double), hipMemcpyDeviceToDevice, st));
        } else HIP_OK(hipMemcpyAsync(s.rr, sums + 3 * (size_t)L, L * sizeof(double), hipMemcpyDeviceToDevice, st));   // the pass summed the new r.r
        HIP_OK(hipMemcpyAsync(h.data(), sums, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));      // the one read of the iteration
        HIP_OK(hipStreamSynchronize(st));
        double *row = trace + (size_t)(k + 1) * 4 * L;
        bool met = true;
        for (int l = 0; l < L; ++l) {
            row[l] = h[l];
            row[L + l] = rho[l] * rho[l] * h[(size_t)L + l];
            row[2 * (size_t)L + l] = h[3 * (size_t)L + l];
            row[3 * (size_t)L + l] = h[2 * (size_t)L + l];
            met = met && std::sqrt(std::max(rho[l] * rho[l] * row[l], row[L + l])) < (double)s.n * tol;
        }
        *nit = k + 1;
        if (met) break;
    }
    HIP_OK(hipMemcpyAsync(out, p->nn_z, m * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}
}  // namespace

int surfh_cg_planes_nonneg(surfh_plan *p, const float *y, double mu, double mu_reg, const double *rho, const float *x0, int32_t outer,
                           int32_t inner, double tol, int32_t refresh, float *x, double *trace, int32_t *nit) {
    if (!p || !y || !rho || !x || !trace || !nit) return fail("null argument");
    if (imager_refuse(p, "surfh_cg_planes_nonneg")) return 1;
    if (p->T != 0) return fail("surfh_cg_planes_nonneg is the solver of the plane-wise (no template) model; use surfh_cg_nonneg with templates");
    for (int l = 0; l < p->Lc; ++l) {
        const float rf = (float)rho[l];
        if (!(rho[l] > 0.0 && rho[l] <= DBL_MAX) || !(rf > 0.f && rf <= FLT_MAX))
            return fail("surfh_cg_planes_nonneg: rho[%d] = %g must be finite and > 0 (as a float too)", l, rho[l]);
    }
    if (nn_refuse("surfh_cg_planes_nonneg", 1.0, outer, inner)) return 1;
    if (cg_planes_ready(p, "surfh_cg_planes_nonneg", false)) return 1;
    const CgSpace s = planes_space(p, p->cg_x, mu, mu_reg);
    HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (start_iterate(p, x0) || cg_start(p, s, p->io_y, s.xc)) return 1;
    NnScope sc(p);
    if (sc.begin_planes(p->Lc, s.n, rho)) return 1;
    CgSpace sx = s;
    sx.apply = nn_planes_apply;
    sx.rho_l = p->nn_rho;
    return nn_planes_loop(p, sx, rho, x0, outer, inner, tol, refresh, x, trace, nit);
}

// out[0] = J(x, S) = (mu out[1] + mu_reg out[2] + mu_spec out[3]) / 2 at the plan's templates S: out[1] = (y - A x)^T W (y - A x) under
// the plan's data weights, out[2] = x^T (the plan's spatial prior) x, out[3] = |D S|^2 along the wavelength -- float64 sums on the device
int surfh_joint_criterion(surfh_plan *p, const float *y, const float *maps, double mu, double mu_reg, double mu_spec, double *out) {
    if (!p || !y || !maps || !out) return fail("null argument");
    HIP_OK(hipSetDevice(p->dev));
    if (tpl_ensure(p) || ensure_cg(p)) return 1;
    hipStream_t st = p->stream;
    const long n = (long)p->T * p->Lc;
    std::vector<float> h((size_t)n);
    for (long i = 0; i < n; ++i) h[i] = (float)p->tpl_host[i];
    HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(p->io_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(p->tg_v[5], h.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
    if (forward_dev(p, p->io_x, p->cg_y)) return 1;
    LAUNCH_OK(launch_wres_sq(st, p->io_y, p->cg_y, p->dw, p->osize, p->dscratch, p->dscal + 3));
    LAUNCH_OK(launch_fill_zero(st, p->cg_q, p->isize));
    LAUNCH_OK(prior_add(p, st, p->io_x, p->cg_q, p->T, 1.f));
    LAUNCH_OK(launch_dot(st, p->io_x, p->cg_q, p->isize, p->dscratch, p->dscal + 4));
    LAUNCH_OK(launch_fill_zero(st, p->tg_v[3], n));
    LAUNCH_OK(launch_tpl_prior_add(st, p->tg_v[5], p->tg_v[3], p->T, p->Lc, 1.f));
    LAUNCH_OK(launch_dot(st, p->tg_v[5], p->tg_v[3], n, p->dscratch, p->dscal + 5));
    HIP_OK(hipMemcpyAsync(out + 1, p->dscal + 3, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    out[0] = 0.5 * (mu * out[1] + mu_reg * out[2] + mu_spec * out[3]);
    return 0;
}

// ---- posterior sampling by perturbation-optimisation (kernels and conventions: posterior.hip) ----
// The criterion of surfh_cg is the negative log of the Gaussian  p(x | y) ~ exp(-x^T Q x / 2 + b^T x),  Q = mu A^T W A + mu_reg
// (Dr^T Dr + Dc^T Dc), b = mu A^T W y, and a draw b~ = mu A^T W (y + eps_y / sqrt(mu w)) + eta ~ N(b, Q), eta = sqrt(mu_reg)
// (Dr^T eps_r + Dc^T eps_c), gives the sample x~ = Q^-1 b~.  The sampler solves for the deviation e = x~ - xhat instead, from
// zero:  Q e = b~ - b = mu A^T W (eps_y / sqrt(mu w)) + eta  -- the CG of surfh_cg on the perturbation alone as its data (io_y)
// with eta as the extra right-hand side of its set-up (CgSpace::extra).  In exact arithmetic and at convergence that is the solve of
// Q x~ = b~ started at xhat; in fp32 it is the one that works: started at xhat, the residual b~ - Q xhat is a difference of two
// vectors some 1e3 times its size, the operator's 3e-7 comes back as 1e-4 of every r.r (measured: 2.3e-4 to 5.4e-4 on config 1
// and two_channel_mid, against 2e-5 for a solve from zero), a perturbation below 1e-4 of the data drowns in the rounding of y~,
// and a solve stopped at max_iter spends its iterations on what xhat left unconverged (r.r 7.0e6 of it against 4.7e5 of the
// perturbation on config 1 after 10 iterations), which all samples share.  The deviation form has none of the three.
namespace {
int po_refuse(const surfh_plan *p, double mu, double mu_reg, const char *who) {
    if (p->T <= 0) return fail("%s needs templates (the posterior is that of the abundance maps)", who);
    if (p->T > SURFH_MAX_TEMPLATES) return fail("%s: %d maps, the moment kernels take %d", who, p->T, SURFH_MAX_TEMPLATES);
    if (p->prior_kind != 0) return fail("%s draws the prior's noise through the separated differences: surfh_set_prior(plan, 0)", who);
    if (imager_active(p)) return fail("%s does not perturb the imager data term set on this plan (surfh_set_imager_data): clear it", who);
    if (!(mu > 0.0 && mu <= DBL_MAX)) return fail("%s: mu = %g must be finite and > 0", who, mu);
    if (!(mu_reg >= 0.0 && mu_reg <= DBL_MAX)) return fail("%s: mu_reg = %g must be finite and >= 0", who, mu_reg);
    return 0;
}
int po_ensure(surfh_plan *p) {
    if (ensure_cg(p)) return 1;
    const size_t no = (size_t)p->osize, ni = (size_t)p->isize;
    return ensure_set(member(p->po_y, no), member(p->po_eps, no), member(p->po_er, ni), member(p->po_ec, ni), member(p->po_eta, ni),
                      member(p->po_xhat, ni), member(p->po_S, (size_t)(2 * po_moment_planes(p->T)) * p->Na * p->Nb));   // the sums, then mean and cov
}
// one noise vector on the device: row `sample` of the caller's, or the generator's stream
int po_noise(surfh_plan *p, float *dst, long n, const float *host, uint64_t seed, uint32_t stream, int sample) {
    if (host) {
        HIP_OK(hipMemcpyAsync(dst, host + (size_t)sample * n, n * sizeof(float), hipMemcpyHostToDevice, p->stream));
        return 0;
    }
    Prof pr(p, "po_randn");
    LAUNCH_OK(launch_randn(p->stream, dst, n, seed, stream, (uint32_t)sample));
    return 0;
}
// draw `sample`: y + eps_y / sqrt(mu w) to io_y (y on the device, or NULL: the perturbation alone), eta to po_eta; *extra =
// po_eta, or NULL where mu_reg = 0.  eps_* are the rows [n_samples][...] of the caller's noise (NULL: the generator under `seed`)
int po_perturb(surfh_plan *p, const float *y, double mu, double mu_reg, uint64_t seed, int sample, const float *eps_y, const float *eps_r,
               const float *eps_c, const float **extra) {
    if (po_noise(p, p->po_eps, p->osize, eps_y, seed, 0, sample)) return 1;
    {
        Prof pr(p, "po_data");
        LAUNCH_OK(launch_po_data(p->stream, y, p->dw, p->po_eps, p->io_y, p->osize, (float)mu));
    }
    *extra = nullptr;
    if (mu_reg == 0.0) return 0;
    if (po_noise(p, p->po_er, p->isize, eps_r, seed, 1, sample) || po_noise(p, p->po_ec, p->isize, eps_c, seed, 2, sample)) return 1;
    Prof pr(p, "po_prior");
    LAUNCH_OK(launch_po_prior(p->stream, p->po_er, p->po_ec, p->po_eta, p->T, p->Na, p->Nb, (float)std::sqrt(mu_reg)));
    *extra = p->po_eta;
    return 0;
}
}  // namespace

int surfh_po_rhs(surfh_plan *p, const float *y, double mu, double mu_reg, uint64_t seed, int32_t sample, const float *eps,
                 float *btilde) {
    if (!p || !y || !btilde) return fail("null argument");
    if (po_refuse(p, mu, mu_reg, "surfh_po_rhs")) return 1;
    if (sample < 0) return fail("surfh_po_rhs: sample = %d", sample);
    HIP_OK(hipSetDevice(p->dev));
    if (po_ensure(p)) return 1;
    HIP_OK(hipMemcpyAsync(p->po_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    const float *extra = nullptr;
    // eps: one draw, eps_y [osize] then eps_r, eps_c [isize] each; row 0 of each
    if (po_perturb(p, p->po_y, mu, mu_reg, seed, eps ? 0 : sample, eps, eps ? eps + p->osize : nullptr, eps ? eps + p->osize + p->isize : nullptr, &extra))
        return 1;
    // the right-hand side as the maps' CG sets it up (solver_setup): mu A^T W y~ + eta
    const float *wy = weighted_data(p, p->io_y);
    if (!wy || adjoint_dev(p, wy, p->cg_b)) return 1;
    if (mu != 1.0) LAUNCH_OK(launch_scale(p->stream, p->cg_b, p->isize, (float)mu));
    if (extra) LAUNCH_OK(launch_po_add(p->stream, p->cg_b, extra, p->isize));
    HIP_OK(hipMemcpyAsync(btilde, p->cg_b, p->isize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

int surfh_cg_sample(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                    int32_t refresh, int32_t n_samples, uint64_t seed, const float *eps_y, const float *eps_r, const float *eps_c,
                    float *x_map, double *mean, double *cov, double *grad_norm, int32_t *nit, double *rr_worst,
                    surfh_sample_callback callback, void *user) {
    if (!p || !y || !x_map || !grad_norm || !nit) return fail("null argument");
    if (po_refuse(p, mu, mu_reg, "surfh_cg_sample")) return 1;
    if (n_samples < 1 || (cov && n_samples < 2))
        return fail("surfh_cg_sample: n_samples = %d (at least 1, and at least 2 for a covariance)", n_samples);
    if (max_iter < 0) return fail("surfh_cg_sample: max_iter = %d", max_iter);
    HIP_OK(hipSetDevice(p->dev));
    if (po_ensure(p)) return 1;
    // the point estimate: surfh_cg itself
    if (cg_run(p, y, mu, mu_reg, x0, max_iter, tol, refresh, x_map, grad_norm, nit, nullptr, nullptr)) return 1;
    hipStream_t s = p->stream;
    const long npix = (long)p->Na * p->Nb;
    const long planes = po_moment_planes(p->T);
    const float *xc = cg_spectral(p, max_iter) ? p->io_x : p->cg_x;         // where a solve leaves its result in the maps' layout
    HIP_OK(hipMemcpyAsync(p->po_xhat, xc, p->isize * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemsetAsync(p->po_S, 0, (size_t)planes * npix * sizeof(double), s));
    std::vector<float> xs((size_t)p->isize);
    std::vector<double> gn((size_t)max_iter + 1);
    double worst = 0.0;
    for (int k = 0; k < n_samples; ++k) {
        const float *extra = nullptr;
        if (po_perturb(p, nullptr, mu, mu_reg, seed, k, eps_y, eps_r, eps_c, &extra)) return 1;
        int32_t nk = 0;
        if (cg_run(p, nullptr, mu, mu_reg, nullptr, max_iter, tol, refresh, xs.data(), gn.data(), &nk, nullptr, nullptr, extra))
            return 1;                                                           // Q e = b~ - b from e = 0
        {
            Prof pr(p, "po_moments");
            LAUNCH_OK(launch_po_moments(s, xc, nullptr, p->po_S, p->T, npix));
        }
        worst = std::max(worst, gn[nk]);
        if (callback)
            for (long i = 0; i < p->isize; ++i) xs[i] += x_map[i];               // x~ = xhat + e
        if (callback && callback(user, k, nk, gn.data(), xs.data())) return fail("surfh_cg_sample: stopped by the callback at sample %d", k);
        HIP_OK(hipSetDevice(p->dev));
    }
    if (rr_worst) *rr_worst = worst;
    if (mean || cov) {
        double *out = p->po_S + planes * npix;
        {
            Prof pr(p, "po_moments");
            LAUNCH_OK(launch_po_finish(s, p->po_xhat, p->po_S, p->T, npix, n_samples, out, cov ? out + p->isize : nullptr));
        }
        if (mean) HIP_OK(hipMemcpyAsync(mean, out, p->isize * sizeof(double), hipMemcpyDeviceToHost, s));
        if (cov) HIP_OK(hipMemcpyAsync(cov, out + p->isize, (size_t)(planes - p->T) * npix * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    }
    return 0;
}

// ---- 3MG (majorize-minimize memory gradient, qmm.mmmg; selected by method != 'lcg' at fusion_CT.py:194-198) ----
// Every variant minimises a quadratic majorant with matrix B(x) at the iterate over span{-g, m}, m the previous move.  qmm
// solves the 2x2 system in the basis [-g, m] with the operator applied to the gradient; in fp32 that form loses the conjugacy
// (the determinant cancels) and was measured to converge visibly slower than CG.  The same subspace is therefore spanned by
// [d, m], d = -g + beta m made B-orthogonal to m with the carried image of m, and the operator is applied to d: the system
//   [[d.Bd, d.Bm], [d.Bm, m.Bm]] step = [d.(-g), m.(-g)]                                   (mm_step.h: mm_step2)
// is then nearly diagonal.  Same iterates in exact arithmetic, one operator application per iteration; the carried residual
// follows by linearity and is recomputed from x every `refresh` iterations.  numpy's pinv cut (1e-15 of the unscaled matrix),
// which in qmm drops the memory direction once |move|^2 / |grad|^2 < 1e-15, is not reproduced: the direction is dropped only
// when the scaled system is singular.  All loops stand on one frame (mmmg_begin, mmmg_check, refresh_due, mmmg_finish):
//   mmmg_huber_loop    surfh_mmmg, surfh_mmmg_huber, surfh_mmmg_huber_vox       beta and the system on the host, 2 syncs / iteration
//   mmmg_robust_loop   surfh_mmmg_robust, surfh_mmmg_robust_vox                 one read-back, 1 sync / iteration
//   mmmg_planes_loop   surfh_mmmg_planes_cb, surfh_mmmg_huber_planes            beta and the system per plane on the device, 1 sync
//
// Huber priors (qmm.Huber on the row and column differences: the reference's lmm_reconstruction,
// surfh/ToolsDir/algorithms.py:73-106).  The majorant at x is half-quadratic (Geman-Reynolds):
//   B(x) = mu A^T A + mu_reg sum_k D_k^T diag(w(D_k x)) D_k,   w(u) = phi'(u) / u.
// beta comes from the carried data image Q_D m = mu A^T A m and the prior block huber_curv(x; -g, m); the data part
// r = b - mu A^T A x of -g is the carried residual.  Two stencil passes per iteration, each followed by a one-block reduction:
// huber_grad gives -g = r - mu_reg sum_k D_k^T phi'(D_k x), |g|^2 and the prior value; huber_curv gives the prior block
// c = [(-g).W(-g), (-g).W m, m.W m] (W = D^T diag(w) D at x).  The block of (d, m) follows from c by linearity in float64
// (mm_block_of_d); d.Bd = g.Bg - (g.Bm)^2 / m.Bm is the Schur complement of a positive semi-definite 2x2 matrix, which float64
// forms from fp64-accumulated sums with no cancellation that matters at fp32 data precision.
// The quadratic solver surfh_mmmg is the same loop with no Huber family: its prior rides in the operator Q = mu A^T A + mu_reg
// prior, so -g is the carried residual r itself, the grad pass is the dot r.r and there is no curv pass; the majorant is the
// criterion, the step its exact minimiser over the subspace.
namespace {
// the kernels take delta in fp32: a positive delta below FLT_MIN would flush to 0 there (every weight off u = 0 would vanish)
int huber_args(double mu_reg, double delta) {
    if (std::isnan(mu_reg) || std::isnan(delta)) return fail("Huber prior: mu_reg and delta must not be NaN");
    if (!(delta >= (double)FLT_MIN)) return fail("Huber prior: delta must be at least %g (fp32 kernels; got %g)", (double)FLT_MIN, delta);
    return 0;
}

// ---- the coupled prior of the maps (surfh_set_prior_coupling; coupled_prior.hip): w(m) of the group magnitudes is computed once
// per iterate into cpl_w and read by the gradient pass and by the curvature pass.
// the plan can run its coupling (0: nothing to do): the separated differences, and room for the weight field
int coupling_ready(surfh_plan *p, const char *who) {
    if (p->coupling == 0) return 0;
    if (p->prior_kind != 0)
        return fail("%s: the prior coupling (surfh_set_prior_coupling: %d) groups the separated differences; the plan is on the joint "
                    "Laplacian prior (surfh_set_prior)", who, p->coupling);
    HIP_OK(hipSetDevice(p->dev));
    return ensure_set(member(p->cpl_w, (size_t)p->isize));
}
// cpl_w = the weight field of x; phi_sum[0] = the prior value sum phi(m)
int coupled_field(surfh_plan *p, const float *x, float delta, int kind, int coupling, double *phi_sum) {
    Prof pr(p, "coupled_weights");
    LAUNCH_OK(launch_coupled_weights(p->stream, x, p->cpl_w, p->T, p->Na, p->Nb, delta, kind, coupling, p->dscratch, phi_sum));
    return 0;
}
// out = src + coef sum_k D_k^T (w D_k x) with the field of x computed first; sums[0] = out.out, sums[1] = sum phi(m)
int coupled_grad(surfh_plan *p, const float *x, const float *src, float *out, float coef, float delta, int kind, int coupling,
                 double *sums) {
    if (coupled_field(p, x, delta, kind, coupling, sums + 1)) return 1;
    Prof pr(p, "coupled_grad");
    LAUNCH_OK(launch_coupled_grad(p->stream, x, p->cpl_w, src, out, p->T, p->Na, p->Nb, coef, coupling, p->dscratch, sums));
    return 0;
}
// sums[0..2] = the prior block of (p0, p1) under the field cpl_w holds
int coupled_curv(surfh_plan *p, const float *p0, const float *p1, int coupling, double *sums) {
    Prof pr(p, "coupled_curv");
    LAUNCH_OK(launch_coupled_curv(p->stream, p->cpl_w, p0, p1, p->T, p->Na, p->Nb, coupling, p->dscratch, sums));
    return 0;
}
}  // namespace

int surfh_huber_prior_dev(surfh_plan *p, const float *x_dev, float *g_dev, double mu_reg, double delta, double *value) {
    if (!p || !x_dev || !g_dev) return fail("null argument");
    if (p->T <= 0) return fail("prior is defined on abundance maps (needs templates)");
    if (huber_args(mu_reg, delta) || coupling_ready(p, "surfh_huber_prior_dev")) return 1;
    double h[2];
    if (p->coupling) {
        if (coupled_grad(p, x_dev, g_dev, g_dev, (float)mu_reg, (float)delta, p->pot[0], p->coupling, p->dscal)) return 1;
        HIP_OK(hipMemcpyAsync(h, p->dscal, 2 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        HIP_OK(hipStreamSynchronize(p->stream));
        if (value) *value = h[1];
        return 0;
    }
    const auto pass = [&] {
        return launch_huber_grad(p->stream, x_dev, g_dev, g_dev, p->T, p->Na, p->Nb, (float)mu_reg, (float)delta, p->pot[0], p->dscratch,
                                 p->dscal);
    };
    if (diag_pass(p, "huber_grad", pass, p->dscal, h, 2)) return 1;
    if (value) *value = h[1];
    return 0;
}
int surfh_huber_curv_dev(surfh_plan *p, const float *x_dev, const float *p0_dev, const float *p1_dev, double delta, double *sums) {
    if (!p || !x_dev || !p0_dev || !p1_dev || !sums) return fail("null argument");
    if (p->T <= 0) return fail("prior is defined on abundance maps (needs templates)");
    if (huber_args(0.0, delta) || coupling_ready(p, "surfh_huber_curv_dev")) return 1;
    if (p->coupling) {                                     // the field of x first (its prior value lands behind the block)
        if (coupled_field(p, x_dev, (float)delta, p->pot[0], p->coupling, p->dscal + 3) ||
            coupled_curv(p, p0_dev, p1_dev, p->coupling, p->dscal))
            return 1;
        HIP_OK(hipMemcpyAsync(sums, p->dscal, 3 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        HIP_OK(hipStreamSynchronize(p->stream));
        return 0;
    }
    const auto pass = [&] {
        return launch_huber_curv(p->stream, x_dev, p0_dev, p1_dev, p->T, p->Na, p->Nb, (float)delta, p->pot[0], p->dscratch, p->dscal);
    };
    return diag_pass(p, "huber_curv", pass, p->dscal, sums, 3);
}

// The maps' prior passes on arrays of any shape [T][na][nb], whatever the plan's own (a plan cannot have an axis of length 1):
// the launchers surfh_huber_prior_dev / surfh_huber_curv_dev call, under an explicit kind and coupling, on the plan's stream and
// scratch.  sums [5] (host) = g.g, the prior value, the curvature block.
int surfh_debug_prior_passes(surfh_plan *p, int32_t T, int32_t na, int32_t nb, int32_t kind, int32_t coupling, const float *x_dev,
                             float *g_dev, const float *p0_dev, const float *p1_dev, double mu_reg, double delta, double *sums) {
    if (!p || !x_dev || !g_dev || !p0_dev || !p1_dev || !sums) return fail("null argument");
    if (T < 1 || na < 1 || nb < 1 || (double)T * na * nb > 2147483647.0) return fail("surfh_debug_prior_passes: shape %d x %d x %d", (int)T, (int)na, (int)nb);
    if (kind < 0 || kind > 2 || coupling < 0 || coupling > 2) return fail("surfh_debug_prior_passes: kind %d, coupling %d", (int)kind, (int)coupling);
    if (huber_args(mu_reg, delta)) return 1;
    HIP_OK(hipSetDevice(p->dev));
    hipStream_t s = p->stream;
    double *sc = p->dscal;
    DevBuf<float> w;
    if (coupling) {
        if (w.alloc(coupled_weights_floats(coupling, T, na, nb))) return 1;
        LAUNCH_OK(launch_coupled_weights(s, x_dev, w, T, na, nb, (float)delta, kind, coupling, p->dscratch, sc + 1));
        LAUNCH_OK(launch_coupled_grad(s, x_dev, w, g_dev, g_dev, T, na, nb, (float)mu_reg, coupling, p->dscratch, sc));
        LAUNCH_OK(launch_coupled_curv(s, w, p0_dev, p1_dev, T, na, nb, coupling, p->dscratch, sc + 2));
    } else {
        LAUNCH_OK(launch_huber_grad(s, x_dev, g_dev, g_dev, T, na, nb, (float)mu_reg, (float)delta, kind, p->dscratch, sc));
        LAUNCH_OK(launch_huber_curv(s, x_dev, p0_dev, p1_dev, T, na, nb, (float)delta, kind, p->dscratch, sc + 2));
    }
    const hipError_t e = hipMemcpyAsync(sums, sc, 5 * sizeof(double), hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);          // before `w` goes away
    HIP_OK(e);
    HIP_OK(e2);
    return 0;
}

namespace {
// The prior of one 3MG run: `nfam` families of differences with their weights, and the two stencil passes on the solver's
// vectors.  grad: out = src - sum_f reg[f] D_f^T phi'(D_f x), sums[0] = out.out, sums[1 + f] = sum phi of family f;
// curv: sums[3 f ..] = the (p0, p0), (p0, p1), (p1, p1) block of family f under w(D_f x).  The weights enter on the host, in float64.
// nfam = 0 is the quadratic solver: out is src itself (grad leaves sums[0] = src.src), the prior is quad_reg's, in the operator.
// Every loop calls grad on the iterate and then curv on the same iterate: under a coupling, curv reads the weight field grad left.
struct HuberPrior {
    int nfam;
    double reg[2];
    const char *what;                                                       // names the solver in its error message
    int (*grad)(surfh_plan *p, const HuberPrior &h, const float *x, const float *src, float *out, double *sums);
    int (*curv)(surfh_plan *p, const HuberPrior &h, const float *x, const float *p0, const float *p1, double *sums);
    float delta[2];
    int kind[2];                                                            // the potential of each family (surfh_set_potential)
    double quad_reg;                                                        // weight of the quadratic prior the operator carries
    int coupling;                                                           // the maps' family: surfh_set_prior_coupling (0: none)
};

// the loop of the map and cube solvers; prior_values receives nfam doubles (may be NULL)
int mmmg_huber_loop(surfh_plan *p, const HuberPrior &hp, const float *y, double mu, const float *x0, int32_t max_iter, double tol,
                    int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *prior_values, surfh_cg_callback callback,
                    void *user) {
    std::vector<float> hx;
    HIP_OK(hipSetDevice(p->dev));
    if (mmmg_begin(p, hp.nfam > 0, y, p->io_y, x0)) return 1;
    hipStream_t s = p->stream;
    const long n = p->isize;
    const int F = hp.nfam;
    float *r = p->cg_r, *m = p->cg_d, *d = p->cg_dd, *qd = p->cg_q, *qm = p->cg_qm, *ng = F ? p->cg_hg : r;
    // [0 .. F] the grad pass (|g|^2, F prior values), [F+1, F+2] dots, [F+3 .. 4F+2] the curv pass; then the step's four dots
    // over the block just read (the quadratic solver's behind it)
    double *sc = p->dscal, *sd = sc + (F ? 0 : 3);
    if (solver_setup(p, p->io_y, p->cg_x, mu, hp.quad_reg)) return 1;  // r = b - Q x: the data part of -g (all of it when F = 0)
    double h[11], prior[2] = {0.0, 0.0};
    *nit = 0;
    for (int it = 0;; ++it) {
        // -g, |g|^2 and the prior values; then -g.Qm, m.Qm and the prior blocks of (-g, m) under w(D x)
        if (hp.grad(p, hp, p->cg_x, r, ng, sc + 0)) return 1;
        LAUNCH_OK(launch_dot(s, ng, qm, n, p->dscratch, sc + F + 1));
        LAUNCH_OK(launch_dot(s, m, qm, n, p->dscratch, sc + F + 2));
        if (hp.curv(p, hp, p->cg_x, ng, m, sc + F + 3)) return 1;
        HIP_OK(hipMemcpyAsync(h, sc, (3 + 4 * F) * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        grad_norm[it] = std::sqrt(h[0]);
        for (int f = 0; f < F; ++f) prior[f] = h[1 + f];
        if (const int rc = mmmg_check(p, callback, user, it, max_iter, grad_norm, grad_norm[it], (double)n, tol, hx)) {
            if (rc == CB_STOP) break;
            return 1;
        }
        double c[2][3], gBm = h[F + 1], mBm = h[F + 2];
        for (int f = 0; f < F; ++f) {
            for (int k = 0; k < 3; ++k) c[f][k] = h[F + 3 + 3 * f + k];
            gBm += hp.reg[f] * c[f][1];
            mBm += hp.reg[f] * c[f][2];
        }
        const double beta = mBm > 0.0 ? -gBm / mBm : 0.0;
        LAUNCH_OK(launch_lincomb(s, d, ng, m, n, beta));
        if (normal_prior(p, d, qd, mu, hp.quad_reg)) return 1;
        // h0 = d.Qd, h1 = d.Qm, h2 = d.(-g), h3 = m.(-g)
        LAUNCH_OK(launch_dot(s, d, qd, n, p->dscratch, sd + 0));
        LAUNCH_OK(launch_dot(s, d, qm, n, p->dscratch, sd + 1));
        LAUNCH_OK(launch_dot(s, d, ng, n, p->dscratch, sd + 2));
        LAUNCH_OK(launch_dot(s, m, ng, n, p->dscratch, sd + 3));
        HIP_OK(hipMemcpyAsync(h, sd, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        double dBd = h[0], dBm = h[1], s0, s1;
        for (int f = 0; f < F; ++f) {
            double dWd, dWm;
            mm_block_of_d(c[f][0], c[f][1], c[f][2], beta, &dWd, &dWm);
            dBd += hp.reg[f] * dWd;
            dBm += hp.reg[f] * dWm;
        }
        if (!(dBd > 0.0))
            return F ? fail("3MG (%s): non-positive curvature d.Bd = %g at iteration %d", hp.what, dBd, it)
                     : fail("3MG: non-positive curvature d.Qd = %g at iteration %d", dBd, it);
        mm_step2(dBd, dBm, mBm, h[2], h[3], &s0, &s1);
        const bool fresh = refresh_due(refresh, it);
        {
            Prof pr(p, "mmmg_update");
            LAUNCH_OK(launch_mmmg_update(s, p->cg_x, r, d, m, qm, qd, n, s0, s1, fresh ? 0 : 1));
        }
        if (fresh) {
            if (normal_prior(p, p->cg_x, qd, mu, hp.quad_reg)) return 1;
            LAUNCH_OK(launch_residual(s, r, p->cg_b, qd, n));
        }
        *nit = it + 1;
    }
    if (prior_values)
        for (int f = 0; f < F; ++f) prior_values[f] = prior[f];
    return mmmg_finish(p, x);
}

// no Huber family (surfh_mmmg): -g is the carried residual, in place
int quad_grad(surfh_plan *p, const HuberPrior &, const float *, const float *src, float *, double *sums) {
    LAUNCH_OK(launch_dot(p->stream, src, src, p->isize, p->dscratch, sums));
    return 0;
}
int quad_curv(surfh_plan *, const HuberPrior &, const float *, const float *, const float *, double *) { return 0; }
// the maps' prior: one family (rows and columns under one weight and one threshold)
int maps_grad(surfh_plan *p, const HuberPrior &h, const float *x, const float *src, float *out, double *sums) {
    if (h.coupling) return coupled_grad(p, x, src, out, -(float)h.reg[0], h.delta[0], h.kind[0], h.coupling, sums);
    Prof pr(p, "huber_grad");
    LAUNCH_OK(launch_huber_grad(p->stream, x, src, out, p->T, p->Na, p->Nb, -(float)h.reg[0], h.delta[0], h.kind[0], p->dscratch, sums));
    return 0;
}
int maps_curv(surfh_plan *p, const HuberPrior &h, const float *x, const float *p0, const float *p1, double *sums) {
    if (h.coupling) return coupled_curv(p, p0, p1, h.coupling, sums);
    Prof pr(p, "huber_curv");
    LAUNCH_OK(launch_huber_curv(p->stream, x, p0, p1, p->T, p->Na, p->Nb, h.delta[0], h.kind[0], p->dscratch, sums));
    return 0;
}
// the cube's prior: the in-plane family and the wavelength family
int vox_grad(surfh_plan *p, const HuberPrior &h, const float *x, const float *src, float *out, double *sums) {
    Prof pr(p, "huber_vox_grad");
    LAUNCH_OK(launch_huber_vox_grad(p->stream, x, src, out, p->Lc, p->Na, p->Nb, -(float)h.reg[0], h.delta[0], -(float)h.reg[1],
                                    h.delta[1], h.kind[0], h.kind[1], p->dscratch, sums));
    return 0;
}
int vox_curv(surfh_plan *p, const HuberPrior &h, const float *x, const float *p0, const float *p1, double *sums) {
    Prof pr(p, "huber_vox_curv");
    LAUNCH_OK(launch_huber_vox_curv(p->stream, x, p0, p1, p->Lc, p->Na, p->Nb, h.delta[0], h.delta[1], h.kind[0], h.kind[1], p->dscratch,
                                    sums));
    return 0;
}
}  // namespace

int surfh_mmmg_huber(surfh_plan *p, const float *y, double mu, double mu_reg, double delta, const float *x0, int32_t max_iter,
                     double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *prior_value,
                     surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (p->T <= 0) return fail("surfh_mmmg_huber needs templates (the priors act on abundance maps)");
    if (huber_args(mu_reg, delta) || coupling_ready(p, "surfh_mmmg_huber")) return 1;
    const HuberPrior hp = {1, {mu_reg, 0.0}, "Huber", maps_grad, maps_curv, {(float)delta, 0.f}, {p->pot[0], 0}, 0.0, p->coupling};
    return mmmg_huber_loop(p, hp, y, mu, x0, max_iter, tol, refresh, x, grad_norm, nit, prior_value, callback, user);
}

int surfh_mmmg(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
               int32_t refresh, float *x, double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (p->T <= 0) return fail("surfh_mmmg needs templates (the priors act on abundance maps)");
    const HuberPrior hp = {0, {0.0, 0.0}, nullptr, quad_grad, quad_curv, {0.f, 0.f}, {0, 0}, mu_reg};
    return mmmg_huber_loop(p, hp, y, mu, x0, max_iter, tol, refresh, x, grad_norm, nit, nullptr, callback, user);
}

// ---- the same solver on the cube itself (the reference's vox_reconstruction, surfh/ToolsDir/algorithms.py:27-71): no templates,
// Huber priors on the row, column and wavelength differences, the two spatial families under (spat_reg, spat_delta), the spectral
// one under (spec_reg, spec_delta).  The majorant gains the block spec_reg Dl^T diag(w(Dl x)) Dl; everything else is the loop above.
int surfh_huber_vox_prior_dev(surfh_plan *p, const float *x_dev, float *g_dev, double spat_reg, double spat_delta, double spec_reg,
                              double spec_delta, double *values) {
    if (!p || !x_dev || !g_dev) return fail("null argument");
    if (p->T > 0) return fail("the voxel-wise prior is defined on the cube (needs a plan without templates)");
    if (huber_args(spat_reg, spat_delta) || huber_args(spec_reg, spec_delta) || coupling_refuse(p, "surfh_huber_vox_prior_dev")) return 1;
    double h[3];
    const auto pass = [&] {
        return launch_huber_vox_grad(p->stream, x_dev, g_dev, g_dev, p->Lc, p->Na, p->Nb, (float)spat_reg, (float)spat_delta,
                                     (float)spec_reg, (float)spec_delta, p->pot[0], p->pot[1], p->dscratch, p->dscal);
    };
    if (diag_pass(p, "huber_vox_grad", pass, p->dscal, h, 3)) return 1;
    if (values) {
        values[0] = h[1];
        values[1] = h[2];
    }
    return 0;
}
int surfh_huber_vox_curv_dev(surfh_plan *p, const float *x_dev, const float *p0_dev, const float *p1_dev, double spat_delta,
                             double spec_delta, double *sums) {
    if (!p || !x_dev || !p0_dev || !p1_dev || !sums) return fail("null argument");
    if (p->T > 0) return fail("the voxel-wise prior is defined on the cube (needs a plan without templates)");
    if (huber_args(0.0, spat_delta) || huber_args(0.0, spec_delta) || coupling_refuse(p, "surfh_huber_vox_curv_dev")) return 1;
    const auto pass = [&] {
        return launch_huber_vox_curv(p->stream, x_dev, p0_dev, p1_dev, p->Lc, p->Na, p->Nb, (float)spat_delta, (float)spec_delta,
                                     p->pot[0], p->pot[1], p->dscratch, p->dscal);
    };
    return diag_pass(p, "huber_vox_curv", pass, p->dscal, sums, 6);
}

int surfh_mmmg_huber_vox(surfh_plan *p, const float *y, double mu, double spat_reg, double spat_delta, double spec_reg,
                         double spec_delta, const float *x0, int32_t max_iter, double tol, int32_t refresh, float *x,
                         double *grad_norm, int32_t *nit, double *prior_values, surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (imager_refuse(p, "surfh_mmmg_huber_vox") || coupling_refuse(p, "surfh_mmmg_huber_vox")) return 1;
    if (p->T > 0) return fail("surfh_mmmg_huber_vox reconstructs the cube: it needs a plan without templates (n_templates = 0)");
    if (huber_args(spat_reg, spat_delta) || huber_args(spec_reg, spec_delta)) return 1;
    const HuberPrior hp = {2, {spat_reg, spec_reg}, "Huber, voxel-wise", vox_grad, vox_curv, {(float)spat_delta, (float)spec_delta},
                           {p->pot[0], p->pot[1]}};
    return mmmg_huber_loop(p, hp, y, mu, x0, max_iter, tol, refresh, x, grad_norm, nit, prior_values, callback, user);
}

// ---- 3MG with a robust (Huber) data term (qmm.Objective(forward, adjoint, Huber(delta_d), data=y)):
//   J(x) = mu sum_i phi_dd(t_i) + priors(x),   t_i = sqrt(w_i) (y_i - (A x)_i),   w the plan's data weights (1 without)
// The half-quadratic majorant's data block is mu A^T diag(w omega(t)) A with omega recomputed from the residual at every iterate
// (IRLS), so neither the carried Q_D m nor the fused normal operator of mmmg_huber_loop applies: the loop keeps u = A x and
// a_m = A m as detector vectors beside the maps and applies one forward and one adjoint per iteration, through y.  Per iteration:
// robust_data (v = sqrt(w) phi'(t), sum phi, count beyond) -> adjoint (the data part of -g) -> the prior's grad pass (-g, |g|^2,
// prior values) -> forward (a_g = A (-g)) -> robust_curv (the data block of (a_g, a_m)) -> the prior's curv pass -> one read-back.
// The host forms, in float64, the blocks of B = mu A^T diag(w omega) A + sum_f reg_f D_f^T diag(w_f) D_f on (-g, m), beta that
// makes d = -g + beta m B-orthogonal to m, the block of (d, m) by linearity, and the step (mm_step2); the move s0 d + s1 m = s0 (-g) + (s0 beta + s1) m is then one pass over the maps and one over the detector
// vectors.  u is recomputed from x every `refresh` iterations.  One host synchronisation per iteration.
namespace {
int robust_args(double data_delta) {
    if (std::isnan(data_delta)) return fail("robust data term: data_delta must not be NaN");
    if (!(data_delta >= (double)FLT_MIN))
        return fail("robust data term: data_delta must be at least %g (fp32 kernels; got %g)", (double)FLT_MIN, data_delta);
    return 0;
}
float robust_delta_f32(double data_delta) { return data_delta > (double)FLT_MAX ? INFINITY : (float)data_delta; }

// values receives sum phi(t), the number of |t| > data_delta, then the nfam prior values (may be NULL); omega_out [osize] (may be NULL)
int mmmg_robust_loop(surfh_plan *p, const HuberPrior &hp, const float *y, double mu, double data_delta, const float *x0,
                     int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *values,
                     float *omega_out, surfh_cg_callback callback, void *user) {
    std::vector<float> hx;
    HIP_OK(hipSetDevice(p->dev));
    if (p->ch.empty() || p->osize <= 0) return fail("3MG (%s, robust data term) needs a plan with detector channels", hp.what);
    const size_t nrb = (size_t)p->osize;
    if (ensure_set(member(p->rb_y, nrb), member(p->rb_u, nrb), member(p->rb_ag, nrb), member(p->rb_am, nrb))) return 1;
    if (mmmg_begin(p, true, y, p->rb_y, x0, p->rb_am)) return 1;
    hipStream_t s = p->stream;
    const long n = p->isize, no = p->osize;
    const int F = hp.nfam;
    const float dd = robust_delta_f32(data_delta);
    const int dk = p->pot[2];                              // the potential of the data term
    float *r = p->cg_r, *m = p->cg_d, *ng = p->cg_hg, *v = p->cg_y, *yd = p->rb_y, *u = p->rb_u, *ag = p->rb_ag, *am = p->rb_am;
    const float *w = p->dw;
    // device scalars: [0, 1] robust_data, [2 .. 2+F] the prior's grad pass, [3+F .. 5+F] robust_curv, [6+F .. 5+4F] the prior's
    // curv pass, [6+4F] m.(-g)
    double *sc = p->dscal;
    const int G = 2, CD = 3 + F, CP = 6 + F, MG = 6 + 4 * F;
    if (forward_dev(p, p->cg_x, u)) return 1;
    double h[16], val[4] = {0.0, 0.0, 0.0, 0.0};
    *nit = 0;
    for (int it = 0;; ++it) {
        const bool last = it >= max_iter;                  // only |g| and the values are wanted: no majorant
        {
            Prof pr(p, "robust_data");
            LAUNCH_OK(launch_robust_data(s, yd, u, w, v, nullptr, no, dd, dk, p->dscratch, sc + 0));
        }
        if (adjoint_dev(p, v, r)) return 1;
        if (mu != 1.0) LAUNCH_OK(launch_scale(s, r, n, (float)mu));
        if (hp.grad(p, hp, p->cg_x, r, ng, sc + G)) return 1;
        if (!last) {
            if (forward_dev(p, ng, ag)) return 1;
            {
                Prof pr(p, "robust_curv");
                LAUNCH_OK(launch_robust_curv(s, yd, u, w, ag, am, no, dd, dk, p->dscratch, sc + CD));
            }
            if (hp.curv(p, hp, p->cg_x, ng, m, sc + CP)) return 1;
            LAUNCH_OK(launch_dot(s, m, ng, n, p->dscratch, sc + MG));
        }
        HIP_OK(hipMemcpyAsync(h, sc, (last ? 3 + F : 7 + 4 * F) * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        grad_norm[it] = std::sqrt(h[G]);
        val[0] = h[0];
        val[1] = h[1];
        for (int f = 0; f < F; ++f) val[2 + f] = h[G + 1 + f];
        if (const int rc = mmmg_check(p, callback, user, it, max_iter, grad_norm, grad_norm[it], (double)n, tol, hx)) {
            if (rc == CB_STOP) break;
            return 1;
        }
        // the block of (-g, m) under B: the data family in detector space, the prior families on the maps
        double gBg = mu * h[CD], gBm = mu * h[CD + 1], mBm = mu * h[CD + 2];
        for (int f = 0; f < F; ++f) {
            gBg += hp.reg[f] * h[CP + 3 * f];
            gBm += hp.reg[f] * h[CP + 3 * f + 1];
            mBm += hp.reg[f] * h[CP + 3 * f + 2];
        }
        const double beta = mBm > 0.0 ? -gBm / mBm : 0.0;
        double dBd, dBm, s0, s1;
        mm_block_of_d(gBg, gBm, mBm, beta, &dBd, &dBm);
        const double mg = h[MG], dg = h[G] + beta * mg;
        if (!(dBd > 0.0)) return fail("3MG (%s, robust data term): non-positive curvature d.Bd = %g at iteration %d", hp.what, dBd, it);
        mm_step2(dBd, dBm, mBm, dg, mg, &s0, &s1);
        {
            Prof pr(p, "robust_move");
            LAUNCH_OK(launch_robust_move(s, p->cg_x, ng, m, n, s0, s0 * beta + s1));
            LAUNCH_OK(launch_robust_move(s, u, ag, am, no, s0, s0 * beta + s1));
        }
        if (refresh_due(refresh, it) && forward_dev(p, p->cg_x, u)) return 1;
        *nit = it + 1;
    }
    if (values)
        for (int k = 0; k < 2 + F; ++k) values[k] = val[k];
    if (omega_out) {                                       // omega at the returned iterate (u = A x of it)
        LAUNCH_OK(launch_robust_data(s, yd, u, w, v, ag, no, dd, dk, p->dscratch, sc + 0));
        HIP_OK(hipMemcpyAsync(omega_out, ag, no * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    return mmmg_finish(p, x);
}
}  // namespace

int surfh_mmmg_robust(surfh_plan *p, const float *y, double mu, double data_delta, double mu_reg, double delta, const float *x0,
                      int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *values,
                      float *omega_out, surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (imager_refuse(p, "surfh_mmmg_robust")) return 1;
    if (p->T <= 0) return fail("surfh_mmmg_robust needs templates (the priors act on abundance maps)");
    if (robust_args(data_delta) || huber_args(mu_reg, delta) || coupling_ready(p, "surfh_mmmg_robust")) return 1;
    const HuberPrior hp = {1, {mu_reg, 0.0}, "Huber", maps_grad, maps_curv, {(float)delta, 0.f}, {p->pot[0], 0}, 0.0, p->coupling};
    return mmmg_robust_loop(p, hp, y, mu, data_delta, x0, max_iter, tol, refresh, x, grad_norm, nit, values, omega_out, callback, user);
}

int surfh_mmmg_robust_vox(surfh_plan *p, const float *y, double mu, double data_delta, double spat_reg, double spat_delta,
                          double spec_reg, double spec_delta, const float *x0, int32_t max_iter, double tol, int32_t refresh,
                          float *x, double *grad_norm, int32_t *nit, double *values, float *omega_out, surfh_cg_callback callback,
                          void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (imager_refuse(p, "surfh_mmmg_robust_vox") || coupling_refuse(p, "surfh_mmmg_robust_vox")) return 1;
    if (p->T > 0) return fail("surfh_mmmg_robust_vox reconstructs the cube: it needs a plan without templates (n_templates = 0)");
    if (robust_args(data_delta) || huber_args(spat_reg, spat_delta) || huber_args(spec_reg, spec_delta)) return 1;
    const HuberPrior hp = {2, {spat_reg, spec_reg}, "Huber, voxel-wise", vox_grad, vox_curv, {(float)spat_delta, (float)spec_delta},
                           {p->pot[0], p->pot[1]}};
    return mmmg_robust_loop(p, hp, y, mu, data_delta, x0, max_iter, tol, refresh, x, grad_norm, nit, values, omega_out, callback, user);
}

int surfh_robust_data_dev(surfh_plan *p, const float *y_dev, const float *u_dev, const float *w_dev, int64_t n, double data_delta,
                          float *v_dev, double *sums_host) {
    if (!p || !y_dev || !u_dev || !v_dev || !sums_host) return fail("null argument");
    if (n < 1) return fail("surfh_robust_data_dev: n = %ld", (long)n);
    if (robust_args(data_delta)) return 1;
    const auto pass = [&] {
        return launch_robust_data(p->stream, y_dev, u_dev, w_dev, v_dev, nullptr, n, robust_delta_f32(data_delta), p->pot[2], p->dscratch,
                                  p->dscal);
    };
    return diag_pass(p, "robust_data", pass, p->dscal, sums_host, 2);
}
int surfh_robust_curv_dev(surfh_plan *p, const float *y_dev, const float *u_dev, const float *w_dev, const float *p0_dev,
                          const float *p1_dev, int64_t n, double data_delta, double *sums_host) {
    if (!p || !y_dev || !u_dev || !p0_dev || !p1_dev || !sums_host) return fail("null argument");
    if (n < 1) return fail("surfh_robust_curv_dev: n = %ld", (long)n);
    if (robust_args(data_delta)) return 1;
    const auto pass = [&] {
        return launch_robust_curv(p->stream, y_dev, u_dev, w_dev, p0_dev, p1_dev, n, robust_delta_f32(data_delta), p->pot[2], p->dscratch,
                                  p->dscal);
    };
    return diag_pass(p, "robust_curv", pass, p->dscal, sums_host, 3);
}

// ---- CG on independent planes: the 2-D deconvolution path (criterion_2D.py:60-250 per image, batched over wavelength)
int surfh_cg_planes_cb(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                       int32_t refresh, float *x, double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (cg_planes_ready(p, "surfh_cg_planes", false)) return 1;
    const CgSpace s = planes_space(p, p->cg_x, mu, mu_reg);
    HIP_OK(hipMemcpyAsync(p->io_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (start_iterate(p, x0) || cg_start(p, s, p->io_y, s.xc)) return 1;
    return cg_loop(p, s, max_iter, tol, refresh, 1, x, grad_norm, nit, callback, user);
}

int surfh_cg_planes(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                    int32_t refresh, float *x, double *grad_norm, int32_t *nit) {
    return surfh_cg_planes_cb(p, y, mu, mu_reg, x0, max_iter, tol, refresh, x, grad_norm, nit, nullptr, nullptr);
}

// ---- the same iterations with the data and the iterate resident on the device and no host synchronisation inside: begin (cg_start),
// any number of step calls, r.r per plane on request.  x_dev stays the caller's buffer and holds the iterate.
int surfh_cg_planes_begin_dev(surfh_plan *p, const float *y_dev, double mu, double mu_reg, float *x_dev) {
    if (!p || !y_dev || !x_dev) return fail("null argument");
    const bool native = pn_capable(p);
    if (cg_planes_ready(p, "surfh_cg_planes_begin_dev", native)) return 1;
    p->pn_active = native;
    p->pl_x = x_dev; p->pl_mu = mu; p->pl_mu_reg = mu_reg; p->pl_it = 0;
    return cg_start(p, stored_space(p), y_dev, x_dev);
}
int surfh_cg_planes_step_dev(surfh_plan *p, int32_t iters, int32_t refresh) {
    if (!p || !p->pl_x || !(p->pn_active ? (void *)p->pn_sc : (void *)p->pl_sc)) return fail("surfh_cg_planes_begin_dev has not been called");
    HIP_OK(hipSetDevice(p->dev));
    const CgSpace s = stored_space(p);
    for (int i = 0; i < iters; ++i, ++p->pl_it)
        if (cg_iteration(p, s, p->pl_it, refresh)) return 1;
    return s.to_caller(p, s);                                              // the caller's iterate
}
int surfh_cg_planes_rr(surfh_plan *p, double *rr_host) {
    if (!p || !rr_host || !p->pl_x || !(p->pn_active ? p->pn_sc : p->pl_sc)) return fail("surfh_cg_planes_begin_dev has not been called");
    HIP_OK(hipSetDevice(p->dev));
    const CgSpace s = stored_space(p);
    return s.trace(p, s, rr_host, 0);
}

// ---- posterior sampling of the planes: surfh_cg_sample's perturbation-optimisation on the Lc independent problems of surfh_cg_planes.
// At the driver's size a vector of the planes is gigabytes, so the map-domain staging does not carry over: with the generator the
// perturbation of the data is written straight into io_y and eta straight into po_eta (po_planes_data / po_planes_eta: the noise lives
// in registers), and the moments are two float64 sums per element that the finish turns into mean and variance in place.  Allocated:
// po_eta, po_xhat [isize] and po_S [2 isize] doubles; the staging buffers po_eps [osize] / po_er, po_ec [isize] only once a caller
// passes explicit draws, which go through the unfused kernels of surfh_cg_sample.
namespace {
int po_planes_refuse(const surfh_plan *p, double mu, double mu_reg, const char *who) {
    if (imager_refuse(p, who)) return 1;
    if (p->T != 0) return fail("%s samples the plane-wise (no template) model, the plan has %d templates: use surfh_cg_sample", who, p->T);
    if (p->prior_kind != 0) return fail("%s draws the prior's noise through the separated differences: surfh_set_prior(plan, 0)", who);
    if (!(mu > 0.0 && mu <= DBL_MAX)) return fail("%s: mu = %g must be finite and > 0", who, mu);
    if (!(mu_reg >= 0.0 && mu_reg <= DBL_MAX)) return fail("%s: mu_reg = %g must be finite and >= 0", who, mu_reg);
    return 0;
}
int po_planes_ensure(surfh_plan *p, bool explicit_y, bool explicit_prior) {
    const size_t no = (size_t)p->osize, ni = (size_t)p->isize;
    if (ensure_set(member(p->po_eta, ni), member(p->po_xhat, ni), member(p->po_S, 2 * ni))) return 1;       // S1, S2: then mean, var
    if (explicit_y && ensure_set(member(p->po_eps, no))) return 1;
    return explicit_prior ? ensure_set(member(p->po_er, ni), member(p->po_ec, ni)) : 0;
}
// draw `sample`: the perturbation eps_y / sqrt(mu w) to io_y (`y` NULL) or y + it (y on the device), eta to po_eta; *extra = po_eta, or
// NULL where mu_reg = 0.  eps_* as in po_perturb; eps_r or eps_c given: both prior vectors are staged (the missing one generated)
int po_planes_perturb(surfh_plan *p, const float *y, double mu, double mu_reg, uint64_t seed, int sample, const float *eps_y, const float *eps_r,
                      const float *eps_c, const float **extra) {
    hipStream_t s = p->stream;
    if (eps_y || y) {
        if (po_noise(p, p->po_eps, p->osize, eps_y, seed, 0, sample)) return 1;
        Prof pr(p, "po_data");
        LAUNCH_OK(launch_po_data(s, y, p->dw, p->po_eps, p->io_y, p->osize, (float)mu));
    } else {
        Prof pr(p, "po_planes_data");
        LAUNCH_OK(launch_po_planes_data(s, p->dw, p->io_y, p->osize, (float)mu, seed, (uint32_t)sample));
    }
    *extra = nullptr;
    if (mu_reg == 0.0) return 0;
    const float sq = (float)std::sqrt(mu_reg);
    if (eps_r || eps_c) {
        if (po_noise(p, p->po_er, p->isize, eps_r, seed, 1, sample) || po_noise(p, p->po_ec, p->isize, eps_c, seed, 2, sample)) return 1;
        Prof pr(p, "po_prior");
        LAUNCH_OK(launch_po_prior(s, p->po_er, p->po_ec, p->po_eta, p->Lc, p->Na, p->Nb, sq));
    } else {
        Prof pr(p, "po_planes_eta");
        LAUNCH_OK(launch_po_planes_eta(s, p->po_eta, p->Lc, p->Na, p->Nb, sq, seed, (uint32_t)sample));
    }
    *extra = p->po_eta;
    return 0;
}
}  // namespace

int surfh_po_planes_rhs(surfh_plan *p, const float *y, double mu, double mu_reg, uint64_t seed, int32_t sample, const float *eps,
                        float *btilde) {
    const char *who = "surfh_po_planes_rhs";
    if (!p || !y || !btilde) return fail("null argument");
    if (po_planes_refuse(p, mu, mu_reg, who)) return 1;
    if (sample < 0) return fail("%s: sample = %d", who, sample);
    // y~ = y + eps_y / sqrt(mu w) needs y beside the noise: the data part goes through the staged kernel (po_y, po_eps)
    if (cg_planes_ready(p, who, false) || po_planes_ensure(p, true, mu_reg != 0.0 && eps) || ensure_set(member(p->po_y, (size_t)p->osize))) return 1;
    HIP_OK(hipMemcpyAsync(p->po_y, y, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    const float *extra = nullptr;
    if (po_planes_perturb(p, p->po_y, mu, mu_reg, seed, eps ? 0 : sample, eps, eps ? eps + p->osize : nullptr,
                          eps ? eps + p->osize + p->isize : nullptr, &extra))
        return 1;
    const float *wy = weighted_data(p, p->io_y);                                    // as solver_setup: mu A^T W y~ + eta
    if (!wy || adjoint_dev(p, wy, p->cg_b)) return 1;
    if (mu != 1.0) LAUNCH_OK(launch_scale(p->stream, p->cg_b, p->isize, (float)mu));
    if (extra) LAUNCH_OK(launch_po_add(p->stream, p->cg_b, extra, p->isize));
    HIP_OK(hipMemcpyAsync(btilde, p->cg_b, p->isize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

int surfh_cg_planes_sample(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                           int32_t refresh, int32_t n_samples, uint64_t seed, const float *eps_y, const float *eps_r, const float *eps_c,
                           float *x_map, double *mean, double *var, double *grad_norm, int32_t *nit, double *rr_first, double *rr_last,
                           surfh_sample_callback callback, void *user) {
    const char *who = "surfh_cg_planes_sample";
    if (!p || !y || !x_map || !grad_norm || !nit) return fail("null argument");
    if (po_planes_refuse(p, mu, mu_reg, who)) return 1;
    if (n_samples < 1 || (var && n_samples < 2)) return fail("%s: n_samples = %d (at least 1, and at least 2 for a variance)", who, n_samples);
    if (max_iter < 0) return fail("%s: max_iter = %d", who, max_iter);
    if (cg_planes_ready(p, who, false) || po_planes_ensure(p, eps_y != nullptr, mu_reg != 0.0 && (eps_r || eps_c))) return 1;
    // the point estimate: surfh_cg_planes itself
    if (surfh_cg_planes_cb(p, y, mu, mu_reg, x0, max_iter, tol, refresh, x_map, grad_norm, nit, nullptr, nullptr)) return 1;
    hipStream_t s = p->stream;
    const int L = p->Lc;
    double *const S1 = p->po_S, *const S2 = S1 + p->isize;
    HIP_OK(hipMemcpyAsync(p->po_xhat, p->cg_x, p->isize * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemsetAsync(S1, 0, 2 * (size_t)p->isize * sizeof(double), s));
    std::vector<float> xs(callback ? (size_t)p->isize : 0);
    std::vector<double> gn(((size_t)max_iter + 1) * L), first((size_t)L, 0.0), last((size_t)L, 0.0);
    for (int k = 0; k < n_samples; ++k) {
        CgSpace sp = planes_space(p, p->cg_x, mu, mu_reg);                          // Q_l e_l = b~_l - b_l from e = 0
        if (po_planes_perturb(p, nullptr, mu, mu_reg, seed, k, eps_y, eps_r, eps_c, &sp.extra)) return 1;
        int32_t nk = 0;
        if (start_iterate(p, nullptr) || cg_start(p, sp, p->io_y, sp.xc)) return 1;
        if (cg_loop(p, sp, max_iter, tol, refresh, 1, callback ? xs.data() : nullptr, gn.data(), &nk, nullptr, nullptr)) return 1;
        {
            Prof pr(p, "po_planes_moments");
            LAUNCH_OK(launch_po_planes_moments(s, p->cg_x, nullptr, S1, S2, p->isize));
        }
        for (int l = 0; l < L; ++l) {
            first[l] = std::max(first[l], gn[l]);
            last[l] = std::max(last[l], gn[(size_t)nk * L + l]);
        }
        if (callback) {
            for (long i = 0; i < p->isize; ++i) xs[i] += x_map[i];                  // x~ = xhat + e
            if (callback(user, k, nk, gn.data(), xs.data())) return fail("%s: stopped by the callback at sample %d", who, k);
            HIP_OK(hipSetDevice(p->dev));
        }
    }
    if (rr_first) std::copy(first.begin(), first.end(), rr_first);
    if (rr_last) std::copy(last.begin(), last.end(), rr_last);
    if (mean || var) {
        {
            Prof pr(p, "po_planes_finish");
            LAUNCH_OK(launch_po_planes_finish(s, p->po_xhat, S1, S2, p->isize, n_samples, var ? 1 : 0));
        }
        if (mean) HIP_OK(hipMemcpyAsync(mean, S1, p->isize * sizeof(double), hipMemcpyDeviceToHost, s));
        if (var) HIP_OK(hipMemcpyAsync(var, S2, p->isize * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_OK(hipMemcpyAsync(p->cg_x, p->po_xhat, p->isize * sizeof(float), hipMemcpyDeviceToDevice, s));   // the plan as surfh_cg_planes leaves it
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

// ---- 3MG on independent planes: every plane's beta, 2x2 system and step on the device, so the host reads one thing per
// iteration, the Lc squared gradient norms `sq` that `dir` leaves.  dir() forms d = -g + beta m per plane from the carried
// residual; the operator (mu A^T A, + op_reg prior) is applied to d for all planes together; step(update_r) solves and moves.
// The iterate is left in cg_x: the caller ends with mmmg_finish.
namespace {
int mmmg_planes_loop(surfh_plan *p, bool want_hg, const float *y, double mu, double op_reg, const float *x0, int32_t max_iter, double tol,
                     int32_t refresh, double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user, const double *sq,
                     const std::function<int()> &dir, const std::function<int(int)> &step) {
    std::vector<float> hx;
    if (mmmg_begin(p, want_hg, y, p->io_y, x0)) return 1;
    hipStream_t s = p->stream;
    const int L = p->Lc;
    const long npix = (long)p->Na * p->Nb;
    if (solver_setup(p, p->io_y, p->cg_x, mu, op_reg)) return 1;
    *nit = 0;
    for (int it = 0;; ++it) {
        if (dir()) return 1;
        double *gn = grad_norm + (size_t)it * L;
        HIP_OK(hipMemcpyAsync(gn, sq, L * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        double worst = 0.0;
        for (int l = 0; l < L; ++l) {
            gn[l] = std::sqrt(gn[l]);
            worst = std::max(worst, gn[l]);
        }
        if (const int rc = mmmg_check(p, callback, user, it, max_iter, grad_norm, worst, (double)npix, tol, hx)) {
            if (rc == CB_STOP) break;
            return 1;
        }
        if (normal_prior(p, p->cg_dd, p->cg_q, mu, op_reg)) return 1;
        const bool fresh = refresh_due(refresh, it);
        if (step(fresh ? 0 : 1)) return 1;
        if (fresh) {
            if (normal_prior(p, p->cg_x, p->cg_q, mu, op_reg)) return 1;
            LAUNCH_OK(launch_residual(s, p->cg_r, p->cg_b, p->cg_q, p->isize));
        }
        *nit = it + 1;
    }
    return 0;
}
}  // namespace

// what `method = "qmm"` of the 2-D deconvolution driver runs (scripts/deconvolution_mrs_noRotation.py:199-212 ->
// criterion_2D.py:190-193 -> qmm.mmmg): the quadratic prior rides in the operator, -g is the carried residual
int surfh_mmmg_planes_cb(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                         int32_t refresh, float *x, double *grad_norm, int32_t *nit, surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (imager_refuse(p, "surfh_mmmg_planes")) return 1;
    if (p->T != 0) return fail("surfh_mmmg_planes is the solver of the plane-wise (no template) model; use surfh_mmmg with templates");
    if (p->ch.empty()) return fail("plan has no channel");
    HIP_OK(hipSetDevice(p->dev));
    const int L = p->Lc;
    const long npix = (long)p->Na * p->Nb;
    if (ensure_set(member(p->pl_sc, (size_t)3 * L))) return 1;
    double *rr = p->pl_sc, *mqm = p->pl_sc + L;
    const auto dir = [&] {
        LAUNCH_OK(launch_mmmg_dir_planes(p->stream, p->cg_dd, p->cg_r, p->cg_d, p->cg_qm, L, npix, rr, mqm));
        return 0;
    };
    const auto step = [&](int update_r) {
        LAUNCH_OK(launch_mmmg_step_planes(p->stream, p->cg_x, p->cg_r, p->cg_dd, p->cg_d, p->cg_qm, p->cg_q, L, npix, mqm, update_r));
        return 0;
    };
    if (mmmg_planes_loop(p, false, y, mu, mu_reg, x0, max_iter, tol, refresh, grad_norm, nit, callback, user, rr, dir, step)) return 1;
    return mmmg_finish(p, x);
}

int surfh_mmmg_planes(surfh_plan *p, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                      int32_t refresh, float *x, double *grad_norm, int32_t *nit) {
    return surfh_mmmg_planes_cb(p, y, mu, mu_reg, x0, max_iter, tol, refresh, x, grad_norm, nit, nullptr, nullptr);
}

// ---- 3MG with Huber priors on independent planes: the criterion of surfh_mmmg_huber per plane,
//   J_l(x_l) = mu |y_l - A_l x_l|^2 / 2 + mu_reg sum_k sum phi(D_k x_l),
// minimised by mmmg_planes_loop: huber_dir_planes gives -g_l, |g_l|^2, the prior value, the prior block of (-g_l, m_l), beta_l
// and d_l = -g_l + beta_l m_l; the operator is the data part Q_D = mu A^T A alone; huber_step_planes forms the block of
// (d_l, m_l) by linearity in float64, solves and moves.  The _ex entry points give every plane its own mu_reg_l and delta_l and
// take a coupling of a pixel's two differences (0 none, 1 isotropic) as an argument of the call; the scalar entry points forward
// to the same code with Lc copies of their value and coupling 0.
namespace {
int huber_planes_ready(surfh_plan *p, const char *who) {
    if (imager_refuse(p, who) || coupling_refuse(p, who)) return 1;
    if (p->T != 0) return fail("%s works on the plane-wise (no template) model; the maps of a template model take surfh_mmmg_huber", who);
    if (p->ch.empty()) return fail("plan has no channel");
    HIP_OK(hipSetDevice(p->dev));
    if (ensure_set(member(p->pl_hsc, (size_t)HUBER_PLANES_SCALARS * p->Lc), member(p->pl_hpar, (size_t)HUBER_PLANES_PARAMS * p->Lc))) return 1;
    return 0;
}

// The per-call coupling of the plane-wise passes: 0 (none) or 1 (isotropic: one potential per pixel on sqrt(u_r^2 + u_c^2)).  It
// is an argument, not plan state -- the plan's slot (surfh_set_prior_coupling) stays the maps' and is refused by coupling_refuse.
int planes_coupling_arg(const char *who, int32_t coupling) {
    if (coupling == 2)
        return fail("%s: the vector coupling (2) would tie the independent planes together -- one trace, one stopping test, a different "
                    "solver; the planes take coupling 0 (none) or 1 (isotropic)", who);
    if (coupling != 0 && coupling != 1) return fail("%s: coupling %d; the planes take 0 (none) or 1 (isotropic)", who, (int)coupling);
    return 0;
}
// The rules of the per-plane arrays of the *_ex entry points: every delta[l] as huber_args asks, every mu_reg[l] >= 0.
int planes_array_args(const char *who, int L, const double *mu_reg, const double *delta) {
    if (!delta) return fail("null argument");
    for (int l = 0; l < L; ++l) {
        if (huber_args(mu_reg ? mu_reg[l] : 0.0, delta[l])) return 1;
        if (mu_reg && !(mu_reg[l] >= 0.0)) return fail("%s: mu_reg[%d] = %g must be >= 0", who, l, mu_reg[l]);
    }
    return 0;
}
// The parameter table of the plane kernels (kernels.h: HUBER_PLANES_PARAMS) for L planes, on the host: the coefficient of the prior
// gradient sign * (float)mu_reg[l], (float)delta[l], and mu_reg[l] in float64 -- the values the scalar kernels took as arguments.
void planes_param_table(int L, const double *mu_reg, const double *delta, float sign, std::vector<double> &par) {
    par.assign((size_t)HUBER_PLANES_PARAMS * L, 0.0);
    for (int l = 0; l < L; ++l) {
        par[l] = mu_reg ? (double)(sign * (float)mu_reg[l]) : 0.0;
        par[(size_t)L + l] = (double)(float)delta[l];
        par[(size_t)2 * L + l] = mu_reg ? mu_reg[l] : 0.0;
    }
}
// ... in the plan's table.  Every entry point synchronises the plan's stream before it returns: no kernel reads the table now.
int planes_params(surfh_plan *p, const double *mu_reg, const double *delta, float sign) {
    std::vector<double> par;
    planes_param_table(p->Lc, mu_reg, delta, sign, par);
    return dev_raw_upload(p->pl_hpar, par.data(), par.size() * sizeof(double));
}

// the three entry points on per-plane arrays (already checked) under a coupling; the scalar ones hand in Lc copies of their value
int planes_prior_dev(surfh_plan *p, const float *x_dev, float *g_dev, const double *mu_reg, const double *delta, int coupling,
                     double *sq_host, double *values_host) {
    const int L = p->Lc;
    if (planes_params(p, mu_reg, delta, 1.f)) return 1;
    {
        Prof pr(p, "huber_planes_grad");
        LAUNCH_OK(launch_huber_planes_grad(p->stream, x_dev, g_dev, g_dev, L, p->Na, p->Nb, p->pl_hpar, p->pot[0], coupling, p->pl_hsc));
    }
    if (sq_host) HIP_OK(hipMemcpyAsync(sq_host, p->pl_hsc, L * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (values_host) HIP_OK(hipMemcpyAsync(values_host, p->pl_hsc + L, L * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int planes_curv_dev(surfh_plan *p, const float *x_dev, const float *p0_dev, const float *p1_dev, const double *delta, int coupling,
                    double *sums_host) {
    const int L = p->Lc;
    if (planes_params(p, nullptr, delta, 0.f)) return 1;
    const auto pass = [&] {
        return launch_huber_planes_curv(p->stream, x_dev, p0_dev, p1_dev, L, p->Na, p->Nb, p->pl_hpar, p->pot[0], coupling, p->pl_hsc);
    };
    return diag_pass(p, "huber_planes_curv", pass, p->pl_hsc + (size_t)(HUBER_PLANES_SCALARS - 3) * L, sums_host, (size_t)3 * L);
}
int planes_mmmg_huber(surfh_plan *p, const float *y, double mu, const double *mu_reg, const double *delta, int coupling, const float *x0,
                      int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *prior_values,
                      surfh_cg_callback callback, void *user) {
    const int L = p->Lc;
    const long npix = (long)p->Na * p->Nb;
    double *sc = p->pl_hsc;
    if (planes_params(p, mu_reg, delta, -1.f)) return 1;
    const auto dir = [&] {
        Prof pr(p, "huber_dir_planes");
        LAUNCH_OK(launch_huber_dir_planes(p->stream, p->cg_x, p->cg_r, p->cg_hg, p->cg_d, p->cg_qm, p->cg_dd, L, p->Na, p->Nb, p->pl_hpar,
                                          p->pot[0], coupling, sc));
        return 0;
    };
    const auto step = [&](int update_r) {
        Prof pr(p, "huber_step_planes");
        LAUNCH_OK(launch_huber_step_planes(p->stream, p->cg_x, p->cg_r, p->cg_dd, p->cg_d, p->cg_qm, p->cg_q, p->cg_hg, L, npix, p->pl_hpar,
                                           sc, update_r));
        return 0;
    };
    if (mmmg_planes_loop(p, true, y, mu, 0.0, x0, max_iter, tol, refresh, grad_norm, nit, callback, user, sc, dir, step)) return 1;
    // the last launch of the dir kernel ran on the returned iterate: its prior values are the result's
    if (prior_values) HIP_OK(hipMemcpyAsync(prior_values, sc + L, L * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    return mmmg_finish(p, x);
}
}  // namespace

int surfh_huber_planes_prior_dev(surfh_plan *p, const float *x_dev, float *g_dev, double mu_reg, double delta, double *sq_host,
                                 double *values_host) {
    if (!p || !x_dev || !g_dev) return fail("null argument");
    if (huber_args(mu_reg, delta) || huber_planes_ready(p, "surfh_huber_planes_prior_dev")) return 1;
    const std::vector<double> r((size_t)p->Lc, mu_reg), d((size_t)p->Lc, delta);
    return planes_prior_dev(p, x_dev, g_dev, r.data(), d.data(), 0, sq_host, values_host);
}
int surfh_huber_planes_prior_dev_ex(surfh_plan *p, const float *x_dev, float *g_dev, const double *mu_reg, const double *delta,
                                    int32_t coupling, double *sq_host, double *values_host) {
    const char *who = "surfh_huber_planes_prior_dev_ex";
    if (!p || !x_dev || !g_dev || !mu_reg || !delta) return fail("null argument");
    if (planes_coupling_arg(who, coupling) || planes_array_args(who, p->Lc, mu_reg, delta) || huber_planes_ready(p, who)) return 1;
    return planes_prior_dev(p, x_dev, g_dev, mu_reg, delta, coupling, sq_host, values_host);
}

int surfh_huber_planes_curv_dev(surfh_plan *p, const float *x_dev, const float *p0_dev, const float *p1_dev, double delta,
                                double *sums_host) {
    if (!p || !x_dev || !p0_dev || !p1_dev || !sums_host) return fail("null argument");
    if (huber_args(0.0, delta) || huber_planes_ready(p, "surfh_huber_planes_curv_dev")) return 1;
    const std::vector<double> d((size_t)p->Lc, delta);
    return planes_curv_dev(p, x_dev, p0_dev, p1_dev, d.data(), 0, sums_host);
}
int surfh_huber_planes_curv_dev_ex(surfh_plan *p, const float *x_dev, const float *p0_dev, const float *p1_dev, const double *delta,
                                   int32_t coupling, double *sums_host) {
    const char *who = "surfh_huber_planes_curv_dev_ex";
    if (!p || !x_dev || !p0_dev || !p1_dev || !delta || !sums_host) return fail("null argument");
    if (planes_coupling_arg(who, coupling) || planes_array_args(who, p->Lc, nullptr, delta) || huber_planes_ready(p, who)) return 1;
    return planes_curv_dev(p, x_dev, p0_dev, p1_dev, delta, coupling, sums_host);
}

int surfh_mmmg_huber_planes(surfh_plan *p, const float *y, double mu, double mu_reg, double delta, const float *x0, int32_t max_iter,
                            double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *prior_values,
                            surfh_cg_callback callback, void *user) {
    if (!p || !y || !x || !grad_norm || !nit) return fail("null argument");
    if (huber_args(mu_reg, delta) || huber_planes_ready(p, "surfh_mmmg_huber_planes")) return 1;
    const std::vector<double> r((size_t)p->Lc, mu_reg), d((size_t)p->Lc, delta);
    return planes_mmmg_huber(p, y, mu, r.data(), d.data(), 0, x0, max_iter, tol, refresh, x, grad_norm, nit, prior_values, callback, user);
}
int surfh_mmmg_huber_planes_ex(surfh_plan *p, const float *y, double mu, const double *mu_reg, const double *delta, int32_t coupling,
                               const float *x0, int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
                               double *prior_values, surfh_cg_callback callback, void *user) {
    const char *who = "surfh_mmmg_huber_planes_ex";
    if (!p || !y || !mu_reg || !delta || !x || !grad_norm || !nit) return fail("null argument");
    if (planes_coupling_arg(who, coupling) || planes_array_args(who, p->Lc, mu_reg, delta) || huber_planes_ready(p, who)) return 1;
    return planes_mmmg_huber(p, y, mu, mu_reg, delta, coupling, x0, max_iter, tol, refresh, x, grad_norm, nit, prior_values, callback, user);
}

// The plane passes on arrays of any shape [L][na][nb] (every extent >= 1; a slit geometry cannot give a plan an axis of length 1 or
// 2): the launchers of the entry points above under an explicit kind and coupling and per-plane mu_reg / delta, on the plan's
// stream, with scratch of the call's own.  g += mu_reg_l sum_k D_k^T (w D_k x); sums [5][L] (host) = g.g, the prior value, the
// curvature block of (p0, p1), per plane.
int surfh_debug_planes_passes(surfh_plan *p, int32_t L, int32_t na, int32_t nb, int32_t kind, int32_t coupling, const float *x_dev,
                              float *g_dev, const float *p0_dev, const float *p1_dev, const double *mu_reg, const double *delta,
                              double *sums) {
    const char *who = "surfh_debug_planes_passes";
    if (!p || !x_dev || !g_dev || !p0_dev || !p1_dev || !mu_reg || !delta || !sums) return fail("null argument");
    if (L < 1 || na < 1 || nb < 1 || (double)L * na * nb > 2147483647.0) return fail("%s: shape %d x %d x %d", who, (int)L, (int)na, (int)nb);
    if (kind < 0 || kind > 2) return fail("%s: kind %d", who, (int)kind);
    if (planes_coupling_arg(who, coupling) || planes_array_args(who, L, mu_reg, delta)) return 1;
    HIP_OK(hipSetDevice(p->dev));
    hipStream_t s = p->stream;
    std::vector<double> table;
    planes_param_table(L, mu_reg, delta, 1.f, table);
    DevBuf<double> par, sc;
    if (par.upload(table) || sc.alloc((size_t)HUBER_PLANES_SCALARS * L)) return 1;
    LAUNCH_OK(launch_huber_planes_grad(s, x_dev, g_dev, g_dev, L, na, nb, par, kind, coupling, sc));
    LAUNCH_OK(launch_huber_planes_curv(s, x_dev, p0_dev, p1_dev, L, na, nb, par, kind, coupling, sc));
    // rows 0, 1 (g.g, the value) and the last three (the block); the buffers go away after the synchronisation
    const hipError_t e0 = hipMemcpyAsync(sums, sc, (size_t)2 * L * sizeof(double), hipMemcpyDeviceToHost, s);
    const hipError_t e1 = hipMemcpyAsync(sums + (size_t)2 * L, sc + (size_t)(HUBER_PLANES_SCALARS - 3) * L, (size_t)3 * L * sizeof(double),
                                         hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    HIP_OK(e0);
    HIP_OK(e1);
    HIP_OK(e2);
    return 0;
}

// One vector kernel of the plane-wise CG / 3MG loops on arrays of explicit extents: the launchers the solvers call, on the plan's
// stream, with scalars and the pn_part_doubles(LP) partial sums in buffers of the call's own.  ext = { L, npix } for the plane-major
// kernels (one scalar per plane), { Na, Nb, NAP, LP, L, l0 } for the wavelength-innermost ones (one scalar per wavelength of LP) and
// the two transposes.  sc_in: the rows of scalars the kernel reads, sc_out: the rows it writes (uploaded first, so that an entry the
// kernel leaves alone comes back as it went in).
int surfh_debug_planes_cg(surfh_plan *p, const char *which, const int64_t *ext, float *v0, float *v1, float *v2, float *v3, float *v4,
                          float *v5, double mu_reg, int32_t update_r, const double *sc_in, double *sc_out) {
    const char *who = "surfh_debug_planes_cg";
    enum { PLANES, PN, TRANSPOSE };
    struct Kind { const char *name; int family, nvec, nin, nout; };
    static const Kind kinds[] = {{"dot", PLANES, 2, 0, 1},      {"cg_step", PLANES, 4, 2, 1},      {"cg_dir", PLANES, 2, 2, 1},
                                 {"mmmg_dir", PLANES, 4, 0, 2}, {"mmmg_step", PLANES, 6, 1, 0},    {"pn_prior_dot", PN, 2, 0, 1},
                                 {"pn_dot", PN, 2, 0, 1},       {"pn_step", PN, 4, 2, 1},          {"pn_dir", PN, 2, 2, 0},
                                 {"to_lam_inner", TRANSPOSE, 2, 0, 0}, {"from_lam_inner", TRANSPOSE, 2, 0, 0}};
    if (!p || !which || !ext) return fail("null argument");
    const Kind *k = nullptr;
    for (const Kind &c : kinds)
        if (!std::strcmp(which, c.name)) k = &c;
    if (!k) return fail("%s: unknown kernel '%s'", who, which);
    float *const v[6] = {v0, v1, v2, v3, v4, v5};
    for (int i = 0; i < k->nvec; ++i)
        if (!v[i]) return fail("%s: %s takes %d vectors, vector %d is null", who, which, k->nvec, i);
    if ((k->nin && !sc_in) || (k->nout && !sc_out)) return fail("%s: %s needs its scalar arrays (null argument)", who, which);
    if (!std::isfinite(mu_reg) || std::fabs(mu_reg) > 3e38) return fail("%s: mu_reg %g", who, mu_reg);
    if (update_r != 0 && update_r != 1) return fail("%s: update_r %d", who, (int)update_r);
    const double lim = 2147483647.0;
    long n = 0;                                   // scalars of one row
    if (k->family == PLANES) {
        if (ext[0] < 1 || ext[1] < 1 || (double)ext[0] * (double)ext[1] > lim)
            return fail("%s: %s on %lld planes of %lld pixels", who, which, (long long)ext[0], (long long)ext[1]);
        n = (long)ext[0];
    } else {
        const int64_t Na = ext[0], Nb = ext[1], NAP = ext[2], LP = ext[3], L = ext[4], l0 = ext[5];
        if (Na < 1 || Nb < 1 || NAP < Na || LP < 64 || L < 1 || L > LP || l0 < 0 || Na > 65535 || (double)Nb * (double)NAP * (double)LP > lim ||
            (double)(l0 + L) * (double)Na * (double)Nb > lim || (k->family == PN && l0 != 0))
            return fail("%s: %s on Na %lld, Nb %lld, NAP %lld, LP %lld, L %lld, l0 %lld", who, which, (long long)Na, (long long)Nb,
                        (long long)NAP, (long long)LP, (long long)L, (long long)l0);
        if (LP % 64) return fail("%s: LP %lld is no multiple of 64", who, (long long)LP);
        n = (long)LP;
    }
    HIP_OK(hipSetDevice(p->dev));
    hipStream_t s = p->stream;
    DevBuf<double> in, out, part;
    if (k->nin && in.upload(std::vector<double>(sc_in, sc_in + (size_t)k->nin * n))) return 1;
    if (k->nout && out.upload(std::vector<double>(sc_out, sc_out + (size_t)k->nout * n))) return 1;
    if (k->family == PN && part.alloc(pn_part_doubles(n))) return 1;
    const double *result = out;                   // the rows that go back
    const int L = (int)ext[0];
    const long npix = (long)ext[1];
    const int Na = (int)ext[0], Nb = (int)ext[1], NAP = k->family == PLANES ? 0 : (int)ext[2], Lc = k->family == PLANES ? 0 : (int)ext[4];
    const int l0 = k->family == PLANES ? 0 : (int)ext[5];
    const std::string w(which);
    if (w == "dot") LAUNCH_OK(launch_dot_planes(s, v0, v1, L, npix, out));
    else if (w == "cg_step") LAUNCH_OK(launch_cg_step_planes(s, v0, v1, v2, v3, L, npix, in, in + n, out, update_r));
    else if (w == "cg_dir") {                     // rr is read and written: the second row of the scalars that came in
        LAUNCH_OK(launch_cg_dir_planes(s, v0, v1, L, npix, in, in + n));
        result = in + n;
    } else if (w == "mmmg_dir") LAUNCH_OK(launch_mmmg_dir_planes(s, v0, v1, v2, v3, L, npix, out, out + n));
    else if (w == "mmmg_step") LAUNCH_OK(launch_mmmg_step_planes(s, v0, v1, v2, v3, v4, v5, L, npix, in, update_r));
    else if (w == "pn_prior_dot") LAUNCH_OK(launch_pn_prior_dot(s, v0, v1, Na, Nb, NAP, n, (float)mu_reg, part, out));
    else if (w == "pn_dot") LAUNCH_OK(launch_pn_dot(s, v0, v1, Na, Nb, NAP, n, part, out));
    else if (w == "pn_step") LAUNCH_OK(launch_pn_step(s, v0, v1, v2, v3, Na, Nb, NAP, n, in, in + n, part, out, update_r));
    else if (w == "pn_dir") LAUNCH_OK(launch_pn_dir(s, v0, v1, Na, Nb, NAP, n, in, in + n));
    else if (w == "to_lam_inner") LAUNCH_OK(launch_cube_to_lam_inner(s, v0, v1, l0, Lc, Na, Nb, NAP, (int)n));
    else LAUNCH_OK(launch_cube_from_lam_inner(s, v0, v1, l0, Lc, Na, Nb, NAP, (int)n));
    // the buffers go away after the synchronisation
    const hipError_t e0 = k->nout ? hipMemcpyAsync(sc_out, result, (size_t)k->nout * n * sizeof(double), hipMemcpyDeviceToHost, s) : hipSuccess;
    const hipError_t e1 = hipStreamSynchronize(s);
    HIP_OK(e0);
    HIP_OK(e1);
    return 0;
}

// The normal operator of the device-resident plane-wise CG on its own: v goes into the cube's layout as pn_setup takes x0 there,
// pn_normal runs on the loop's own buffers under the given mu / mu_reg, q comes back as pn_to_caller brings the iterate.  Every
// argument is checked before the buffers are asked for; the plan's mu / mu_reg are put back, and the loop a begin call left is over.
int surfh_debug_planes_normal(surfh_plan *p, const float *v_dev, float *q_dev, double mu, double mu_reg, double *dq_host, float *q_raw_dev) {
    const char *who = "surfh_debug_planes_normal";
    if (!p) return fail("%s: plan is null", who);
    if (!v_dev) return fail("%s: v_dev is null", who);
    if (!q_dev) return fail("%s: q_dev is null", who);
    if (!dq_host) return fail("%s: dq_host is null", who);
    if (!std::isfinite(mu) || mu < 0.0) return fail("%s: mu %g", who, mu);
    if (!std::isfinite(mu_reg) || mu_reg < 0.0) return fail("%s: mu_reg %g", who, mu_reg);
    if (p->T != 0) return fail("%s: the plan has %d templates, the plane-wise normal operator belongs to the no-template model", who, (int)p->T);
    if (!pn_capable(p)) return fail("%s: the plan does not run the wavelength-innermost loop (SURFH_PLANES_NATIVE=0, a Huber prior or split planes)", who);
    if (cg_planes_ready(p, who, true)) return 1;
    p->pn_active = false;                         // the loop's vectors are overwritten: it has to be begun again
    p->pl_x = nullptr;
    hipStream_t s = p->stream;
    float *const v = p->pn_v[0], *const q = p->pn_v[3];
    double *const dq = p->pn_sc + p->LP;
    LAUNCH_OK(launch_cube_to_lam_inner(s, v_dev, v, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP));
    const double mu0 = p->pl_mu, mu_reg0 = p->pl_mu_reg;
    p->pl_mu = mu; p->pl_mu_reg = mu_reg;
    const int rc = pn_normal(p, v, q, dq);
    p->pl_mu = mu0; p->pl_mu_reg = mu_reg0;
    if (rc) return 1;
    LAUNCH_OK(launch_cube_from_lam_inner(s, q, q_dev, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP));
    HIP_OK(hipMemcpyAsync(dq_host, dq, (size_t)p->Lc * sizeof(double), hipMemcpyDeviceToHost, s));
    if (q_raw_dev) HIP_OK(hipMemcpyAsync(q_raw_dev, q, (size_t)p->NBP * p->NAP * p->LP * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
