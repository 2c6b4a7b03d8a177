/* surfh_amd -- C ABI of the MI355X-native surfh hot path.
 *
 * One `surfh_plan` = one GPU + one HIP stream + the set of MRS channels that GPU
 * owns.  It is the drop-in replacement for the arithmetic behind
 *   spectroSigRLSCT.forward / .adjoint     (surfh/Models/spectroModel.py:158-185)
 *   Channel.forward / .adjoint             (surfh/Models/spectroModelChannel.py:215-264)
 *   Slicer.slicing / slicing_t             (surfh/Models/slicer.py:64-84)
 *   jax_utils.{lmm_*, dft, idft, dft_mult, wblur_subSampling, wblur_t}
 *                                          (surfh/ToolsDir/jax_utils.py:10-91)
 *   cythons_files.solve_2D_hypercube       (surfh/ToolsDir/cythons_files.pyx:163-193)
 *   NpDiff_r / NpDiff_c + qmm.lcg / qmm.mmmg loops (surfh/Simulation/fusion_CT.py:16-43,194-225)
 * All file:line citations are relative to the reference tree (sidiso/surfh @ 2025-02-04).
 *
 * Conventions
 *   - plain C, no torch types.  Host pointers unless the name ends in `_dev`.
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from surfh_last_error() (thread-local, valid until the next call).
 *   - the geometry tables are produced by the host side (surfh_amd/geometry.py),
 *     which restates instru.py / slicer.py; the library only consumes them.
 *   - arithmetic type: fp32 on device.  The dense stages evaluate every fp32 product as a few 16-bit
 *     matrix-core products of split operands, accumulated in fp32: the spectral blur as three products of a
 *     two-piece round-to-nearest fp16 split (22 mantissa bits) with per-row / per-segment operand scales, the DFT passes
 *     the same way under a per-column running block exponent (axis lengths neither transform kernel covers -- a prime
 *     above 255, fewer than 32 points: dense fp32-input MFMA products); fp32-input MFMA kernels behind SURFH_*
 *     environment switches; inner products of the
 *     solvers accumulate in fp64.  surfh_config.verify selects float64-accumulating kernels throughout.
 *   - environment switches read at plan creation (A/B paths, parity-tested where they engage): SURFH_DFT_H2=0 (axes
 *     <= 255 on the Cooley-Tukey kernel too), SURFH_DFT_CT=0, SURFH_DFT_DENSE=1, SURFH_NO_FUSED_MIX=1, SURFH_WBLUR_FP32=1,
 *     SURFH_WBLUR_FAR=0, SURFH_WBLUR_PERM=0, SURFH_GEMM_GROUPED=0, SURFH_ADJ_FUSED=0 (separate adjoint reduction kernel),
 *     SURFH_OTF_SUPPORT=0, SURFH_OTF_RANGES=0, SURFH_ALPHA_RANGE=0 (transform the whole cube), SURFH_LAMBDA_TRIM=0 (... and every padded plane), SURFH_GATHER_SORTED=0,
 *     SURFH_GATHER_GROUPED=0, SURFH_SCATTER_GROUPED=0, SURFH_SCATTER_RMW_ALL=1, SURFH_ADJ_CLEAR=1, SURFH_OVERLAP=1,
 *     SURFH_PLANES_NATIVE=0, SURFH_OTF_PROD=0 (plane-wise model: the OTF products as kernels of their own); surfh_config.exact switches the far class / the support lists off per plan; read per call:
 *     SURFH_SPECTRAL_CG=0 (solver vectors = maps); read once per process: SURFH_NORMAL_FUSED=0 (the normal operator
 *     goes through y).
 */
#ifndef SURFH_AMD_H
#define SURFH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct surfh_plan surfh_plan;

/* One MRS channel (what Channel.__init__ + Slicer derive; spectroModelChannel.py:27-108). */
typedef struct {
    int32_t wslice_start, wslice_stop; /* IFU.wslice on the cube axis (instru.py:649-658)            */
    int32_t n_pointings;               /* P                                                         */
    int32_t n_slit;                    /* S                                                         */
    int32_t n_lambda_out;              /* Ldet = len(instr.wavel_axis)                              */
    int32_t n_alpha_out;               /* ceil(npix_slit_alpha_width / srf)                         */
    int32_t srf;                       /* super-resolution factor (instru.py:67-84)                 */
    int32_t na, nb;                    /* local grid (len(local_alpha_axis), len(local_beta_axis))  */
    int32_t alpha0;                    /* first local alpha row of the slit window (slicer.py:118)  */
    int32_t n_alpha_slit;              /* length of the alpha window                                */
    int32_t n_beta_slit;               /* npix_slit_beta_width (slicer.py:45-48)                    */
    const int32_t *slit_beta0;         /* [S]    first local beta column of each slit               */
    const double *slit_weights;        /* [S][n_beta_slit] beta-edge weights (slicer.py:148-168)    */
    const int32_t *grid_i0;            /* [P][na*nb] lower alpha index (cythons_files.pyx:109-154)  */
    const int32_t *grid_i1;            /* [P][na*nb] lower beta index                               */
    const double *grid_y0;             /* [P][na*nb] normalised alpha distance                      */
    const double *grid_y1;             /* [P][na*nb] normalised beta distance                       */
    const double *wpsf;                /* [Ldet][Lin][n_beta_slit] spectral PSF (instru.py:499-572);
                                          NULL: no spectral blur, y[l][(p,s,a)] = sum over the slit's beta
                                          columns (MRSBlurred, spectro_blind_rectangle.py:193-209)           */
    /* reference-compatible back-interpolation tables for surfh_adjoint_ref (gridding_t,
       spectroModelChannel.py:180-199); may be NULL if adjoint_ref is never called.               */
    const int32_t *gt_i0;              /* [P][Na*Nb] lower local alpha index                        */
    const int32_t *gt_i1;              /* [P][Na*Nb] lower local beta index                         */
    const double *gt_y0;               /* [P][Na*Nb]                                                */
    const double *gt_y1;               /* [P][Na*Nb]                                                */
    const uint8_t *gt_inside;          /* [P][Na*Nb] 1 if the global pixel falls inside the local grid */
    /* alpha window summed into one detector sample: local rows alpha0 + a*srf + box_shift + [0, box_len) (circular).
       box_len = 0 means srf with shift 0, the operator's box sum (`_otf_sr * decalf`, spectroModelChannel.py:81-83,
       104-108).  The real-data projections use other windows: plain decimation (box_len 1,
       realData_cubeToSlice :303-309) and the box kernel without its re-centring shift (box_shift = -int((srf-1)/2),
       realData_sliceToCube :331-332).                                                             */
    int32_t box_len, box_shift;
} surfh_channel_desc;

typedef struct {
    int32_t n_alpha, n_beta;           /* cube spatial shape                                        */
    int32_t n_lambda;                  /* cube planes Lc                                            */
    int32_t n_templates;               /* T <= 8; 0 => no LMM (input is the cube itself)            */
    const double *templates;           /* [T][Lc] or NULL                                           */
    const double *sotf;                /* [Lc][n_alpha][n_beta/2+1] complex128 interleaved (re,im);
                                          NULL (only with n_templates = 0): no spatial blur, H = 1  */
    int32_t n_channels;
    const surfh_channel_desc *channels;
    int32_t device;                    /* HIP device ordinal                                        */
    void *stream;                      /* hipStream_t to run on, or NULL: the plan creates its own  */
    int32_t split_k_forward;           /* 0 = auto                                                  */
    int32_t verify;                    /* 1 = verification plan: every long sum (DFT products, spectral blur, spectral mix,
                                          gather / scatter rows) accumulated in float64 on plain vector kernels.  Same operator,
                                          same fp32 storage, ~100x slower: for the strict dot test
                                          (test/sandbox_dottest.py:16-27 with randn vectors), not for production. */
    int32_t exact;                     /* production plan without its two approximations (both bounded at plan creation, DESIGN.md
                                          section 4): bit 0 = every K step of the spectral-blur GEMMs keeps all three fp16
                                          products (no far class; same as SURFH_WBLUR_FAR=0), bit 1 = the transform passes visit
                                          the whole spectrum (no OTF-support lists; same as SURFH_OTF_SUPPORT=0).  0 = default. */
} surfh_config;

const char *surfh_last_error(void);
int surfh_version(void);

int surfh_plan_create(const surfh_config *cfg, surfh_plan **out);
int surfh_plan_destroy(surfh_plan *plan);

/* sizes: isize = T*Na*Nb (or Lc*Na*Nb without LMM), osize = sum_c P*S*Ldet*alpha_out */
int64_t surfh_isize(const surfh_plan *plan);
int64_t surfh_osize(const surfh_plan *plan);
void *surfh_stream(const surfh_plan *plan);

/* y = A x      (spectroSigRLSCT.forward, spectroModel.py:158-170)                   */
int surfh_forward(surfh_plan *plan, const float *maps, float *y);
/* x = A^T y    exact transpose of surfh_forward (what CG and the dot-test use)      */
int surfh_adjoint(surfh_plan *plan, const float *y, float *maps);
/* x = reference adjoint with the interpolating gridding_t (spectroModel.py:173-185) */
int surfh_adjoint_ref(surfh_plan *plan, const float *y, float *maps);
/* out = A^T A x                                                                      */
int surfh_fwadj(surfh_plan *plan, const float *x, float *out);

/* device-pointer, asynchronous variants (run on the plan's stream) */
int surfh_forward_dev(surfh_plan *plan, const float *maps_dev, float *y_dev);
int surfh_adjoint_dev(surfh_plan *plan, const float *y_dev, float *maps_dev);
int surfh_adjoint_ref_dev(surfh_plan *plan, const float *y_dev, float *maps_dev);
int surfh_fwadj_dev(surfh_plan *plan, const float *x_dev, float *out_dev);

/* ---- Fourier-domain fused W.C.T operator (Model_WCT, surfh/Models/mixing.py:131-272, di = dj = 1) ----
 * Uses only the plan's sotf / templates (a plan may be created with n_channels = 0 for this).
 * cube is [Lc][Na][Nb] (the reference's layout).                                               */
int surfh_wct_forward(surfh_plan *plan, const float *maps, float *cube);     /* mixing.py:232-245 */
int surfh_wct_adjoint(surfh_plan *plan, const float *cube, float *maps);     /* mixing.py:247-268 */
/* explicit normal operator through the per-frequency T x T Hessian sum_l tpl tpl' |H_l|^2
 * (mixing.py:102-126,177-212,270-272)                                                          */
int surfh_wct_fwadj(surfh_plan *plan, const float *x, float *out);
/* explicit inverse of the regularised normal operator: the minimiser of |y - H x|^2 + sum_t mu_reg[t] |D x_t|^2,
 * one T x T solve per frequency (QuadCriterion3.run_expsol, surfh/ToolsDir/fusion_mixing.py:309-438;
 * algorithms.py:156-184).  reg_freq = |D(f)|^2 on the half spectrum [Na][Nb/2+1] (fusion_mixing.py:364-395).
 * Fails when the matrix is singular at some frequency, where the reference's numpy.linalg.inv raises. */
int surfh_wct_expsol(surfh_plan *plan, const float *cube, const double *mu_reg, const double *reg_freq, float *maps);

/* ---- regularised least squares by linear CG (fusion_CT.py:118-238 + qmm.lcg) ----
 * minimises  mu |y - A x|^2 + mu_reg (|Dr x|^2 + |Dc x|^2).
 * grad_norm receives r.r (max_iter+1 doubles), nit the iterations done.
 * Where the plan offers the spectral-domain calls (surfh_spec_supported) the loop keeps its vectors as the maps' scaled half
 * spectra and its scalars on the device, and reads the trace -- qmm.lcg's stopping test sqrt(r.r) < size * tol -- every 8
 * iterations only: it may run up to 7 iterations past the one that met the tolerance (x and nit are those of the last
 * iteration run).  With a callback (surfh_cg_cb) the test is made after every iteration, as in qmm.lcg.             */
int surfh_cg(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0,
             int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit);
/* The same solver with the per-iteration callback of qmm.lcg (`callback=` at fusion_CT.py:194-225): after
 * iteration `it` (1-based) the callback receives the grad_norm trace so far (it+1 values) and the current
 * iterate copied to the host ([T,Na,Nb] floats, valid during the call).  A non-zero return stops the loop.
 * surfh_forward / surfh_adjoint on the same plan may be called from inside the callback (the criterion
 * trace of fusion_CT.py:163-175 does); the CG building blocks below may not.                          */
typedef int (*surfh_cg_callback)(void *user, int32_t it, const double *grad_norm, const float *x);
int surfh_cg_cb(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0,
                int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
                surfh_cg_callback callback, void *user);

/* ---- template refinement: the other half-step of the bilinear model y = A(S) x -- hold the maps x, solve for the spectra S ----
 * Joint criterion  J(x, S) = [ mu (y - A(S) x)^T W (y - A(S) x) + mu_reg (|Dr x|^2 + |Dc x|^2) + mu_spec |D_l S|^2 ] / 2,  D_l the first
 * difference along the wavelength with open ends, W the plan's data weights.  For fixed x it is quadratic in S; A_x : S -> A(S) x is
 * the forward model with S in the templates' place.  Templates and their gradients are [T][Lc] (n_templates x n_lambda) in cube-plane
 * order; T and Lc are fixed at plan creation.  A plane no channel reads gets a gradient of exactly 0: with mu_spec = 0 it keeps its
 * starting value.  Spectral features narrower than the detector's wavelength sampling are not recoverable from the data.
 *
 * surfh_set_templates: the plan's templates from now on -- uploaded with the rounding and the padding of plan creation; Model_WCT's
 *   explicit Hessian is dropped and rebuilt on its next use.  Fails while an imager is attached (its transfer functions were built
 *   from the templates: detach it, set the templates, attach it again).  surfh_get_templates: the templates as given last.         */
int surfh_set_templates(surfh_plan *plan, const double *templates /*[T][Lc]*/);
int surfh_get_templates(const surfh_plan *plan, double *templates /*[T][Lc]*/);
/* y = A_x S: the forward model on `maps` with `templates` in place of the plan's, which are untouched afterwards                     */
int surfh_forward_templates(surfh_plan *plan, const float *maps, const double *templates, float *y);
/* g [T][Lc] = A_x^T u: the transpose of the above.  g[t][l] = sum over pixels of maps_t times the cube-space adjoint of u at plane l,
 * formed in the Fourier domain as a sum over frequency bins (float64 sums in a fixed order: the same inputs give the same bits);
 * plans on the dense transforms (verification plans among them) and plans with more than 4 templates sum over pixels instead.       */
int surfh_adjoint_templates(surfh_plan *plan, const float *maps, const float *u, float *g);
/* the same two on device buffers, asynchronous on the plan's stream; templates_dev and g_dev are floats [T][Lc]                       */
int surfh_forward_templates_dev(surfh_plan *plan, const float *maps_dev, const float *templates_dev, float *y_dev);
int surfh_adjoint_templates_dev(surfh_plan *plan, const float *maps_dev, const float *u_dev, float *g_dev);
/* Linear CG (the loop, stopping test, trace, refresh and callback contract of surfh_cg; the size in the tolerance is T Lc) on
 *     (mu A_x^T W A_x + mu_spec D_l^T D_l) S = mu A_x^T W y
 * from s0 [T][Lc] (NULL: the plan's templates) to s_out.  The plan's own templates are back in place on every exit -- normal return,
 * error, callback stop -- and while the callback runs, which receives the iterate [T][Lc].  Fails while an imager is attached.       */
int surfh_cg_templates(surfh_plan *plan, const float *y, const float *maps, double mu, double mu_spec, const float *s0,
                       int32_t max_iter, double tol, int32_t refresh, float *s_out, double *grad_norm, int32_t *nit);
int surfh_cg_templates_cb(surfh_plan *plan, const float *y, const float *maps, double mu, double mu_spec, const float *s0,
                          int32_t max_iter, double tol, int32_t refresh, float *s_out, double *grad_norm, int32_t *nit,
                          surfh_cg_callback callback, void *user);
/* out[0] = J(maps, the plan's templates); out[1] = (y - A x)^T W (y - A x), out[2] = x^T P x with P the plan's spatial prior
 * (surfh_set_prior; |Dr x|^2 + |Dc x|^2 by default), out[3] = |D_l S|^2: float64 sums on the device                                  */
int surfh_joint_criterion(surfh_plan *plan, const float *y, const float *maps, double mu, double mu_reg, double mu_spec, double *out);

/* ---- non-negative fusion: ADMM in scaled form around the CG of surfh_cg / surfh_cg_templates ----
 *     min x^T Q x / 2 - b^T x  subject to  x >= 0,      Q and b those of surfh_cg (the plan's data weights included)
 * x = x0 (NULL: 0), z = max(x0, 0), u = 0, v = z - u, r = b + rho v - (Q + rho I) x; per outer iteration: d = r and `inner` CG
 * iterations on Q + rho I (x, r, d carried, no refresh inside); z' = max(x + u, 0), u' = u + x - z', v' = z' - u'; r += rho (v' - v),
 * or r = b + rho v' - (Q + rho I) x in the outer iterations k with (k + 1) % refresh == 0 (refresh 0: never).  The result is z.
 * trace [outer + 1][4]: |x - z|^2, rho^2 |z - z_previous|^2 (0 in row 0), r.r of the next inner system, #{z == 0}; row 0 is the start,
 * rows beyond nit are not written.  Stops after the outer iteration whose row has sqrt(max(rho^2 row[0], row[1])) < isize tol.
 * An outer iteration costs `inner` applications of the operator, one more where it refreshes.  Vectors are the maps' spectra under
 * the rule of surfh_cg (SURFH_SPECTRAL_CG), z and u stay on the pixels.  Fails before any work: rho <= 0 or not finite, inner < 1,
 * outer < 0, a plan without templates, an active imager term.                                                                        */
int surfh_cg_nonneg(surfh_plan *plan, const float *y, double mu, double mu_reg, double rho, const float *x0, int32_t outer, int32_t inner,
                    double tol, int32_t refresh, float *x, double *trace, int32_t *nit);
/* the same on the spectra with the maps held fixed: Q and b those of surfh_cg_templates, s0 NULL: the plan's templates, sizes T Lc.
 * Fails while an imager is attached.                                                                                                  */
int surfh_cg_templates_nonneg(surfh_plan *plan, const float *y, const float *maps, double mu, double mu_spec, double rho, const float *s0,
                              int32_t outer, int32_t inner, double tol, int32_t refresh, float *s_out, double *trace, int32_t *nit);
/* the projection / dual update of one outer iteration on n device floats, in place in z and u: z' = max(x + u, 0) (never a set sign
 * bit), u' = u + x - z', and w = rho ((z' - u') - (z - u)) added to r_dev, or written to dv_dev (r_dev NULL), or dropped (both NULL).
 * sums [4] (host) = |x - z'|^2, |z' - z|^2, #{z' == 0}, r.r of the updated r (0 without r_dev): float64, the same bits for the same
 * inputs.  Pointers need no alignment.                                                                                                */
int surfh_nn_project_dev(surfh_plan *plan, const float *x_dev, float *z_dev, float *u_dev, float *r_dev, float *dv_dev, int64_t n,
                         double rho, double *sums);
/* Non-negative plane-wise deconvolution: the Lc independent problems of surfh_cg_planes (same Q_l and b_l: data weights, the
 * separated circular first-difference prior) under x_l >= 0, by the scheme of surfh_cg_nonneg per plane -- rho [Lc] one fixed penalty
 * each, `inner` CG iterations on Q_l + rho_l I per outer iteration (the plane-wise CG's own kernels, every plane with its own step
 * scalars), z_l' = max(x_l + u_l, 0), u_l' = u_l + x_l - z_l', r_l += rho_l (v_l' - v_l), or r recomputed every `refresh` outer
 * iterations (0: never).  y [osize], x0 [Lc][Na][Nb] or NULL (zeros), x [Lc][Na][Nb] = z: every entry >= 0, no set sign bit.
 * trace [outer + 1][4][Lc]: entry 0 the start, then one per outer iteration run; the four rows of an entry are, per plane,
 * |x - z'|^2, rho_l^2 |z' - z|^2, r.r of the next inner system, #{z' == 0}.  *nit: outer iterations run.  The loop ends once EVERY
 * plane has sqrt(max(rho_l^2 |x - z'|^2, rho_l^2 |z' - z|^2)) < Na Nb tol (0: never); a plane that met the test earlier keeps
 * iterating with the others, nothing is frozen.  A plane with no data from a zero start stays at rest: zeros, a finite trace.
 * The vectors are those of surfh_cg_planes (the caller's layout); the wavelength-innermost space of surfh_cg_planes_begin_dev is
 * not used.  Fails before any work: a null argument, a rho_l that is not finite and > 0, inner < 1, outer < 0, a plan with
 * templates, an imager term.                                                                                                       */
int surfh_cg_planes_nonneg(surfh_plan *plan, const float *y, double mu, double mu_reg, const double *rho, const float *x0, int32_t outer,
                           int32_t inner, double tol, int32_t refresh, float *x, double *trace, int32_t *nit);
/* the projection / dual update of one outer iteration of it on device vectors [L][npix] (plane-major), in place in z, u and r (the
 * fused form of surfh_nn_project_dev, r += rho_l (v' - v)); rho [L] on the host.  sums [4][L] (host) = per plane |x - z'|^2,
 * |z' - z|^2, #{z' == 0}, r.r of the updated r: float64, two stages in a fixed order, the same bits for the same inputs.  A plane
 * whose four base pointers are 16-byte aligned goes through 16-byte accesses, the others (npix % 4 != 0) through the scalar path.   */
int surfh_nn_project_planes_dev(surfh_plan *plan, const float *x_dev, float *z_dev, float *u_dev, float *r_dev, int32_t L, int64_t npix,
                                const double *rho, double *sums);

/* ---- posterior sampling: per-pixel uncertainty of the maps surfh_cg returns (perturbation-optimisation, Orieux, Feron &
 * Giovannelli 2012) ----
 * Convention: the criterion of surfh_cg is the negative log of the Gaussian posterior
 *     p(x | y)  ~  exp(-x^T Q x / 2 + b^T x),    Q = mu A^T W A + mu_reg (Dr^T Dr + Dc^T Dc),    b = mu A^T W y,
 * so the precision is Q exactly as surfh_cg defines it (W: surfh_set_data_weights), the maps surfh_cg returns are the mean
 * Q^-1 b, and the covariance is Q^-1.  It is a statistical statement once the caller passes weights = 1 / sigma^2 (mu = 1) and
 * a mu_reg they believe in.  A draw b~ ~ N(b, Q) costs three standard normal vectors,
 *     y~ = y + eps_y / sqrt(mu w)  (samples of weight 0 untouched, NaN included),   eta = sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c),
 *     b~ = mu A^T W y~ + eta,
 * and x~ = Q^-1 b~ is a posterior sample: one CG solve.  The sampler solves for the deviation from the point estimate xhat,
 *     Q e = b~ - b = mu A^T W (eps_y / sqrt(mu w)) + eta  from e = 0,     x~ = xhat + e,
 * which is the solve of Q x~ = b~ started at xhat whenever xhat has converged, and keeps every fp32 vector at the scale of the
 * perturbation (started at xhat the residual would be a small difference of large vectors; DESIGN.md, "Posterior sampling").
 * A sample is exact only if its solve converges: CG stopped at max_iter leaves the slowly converging directions
 * under-dispersed, and the standard deviation is a lower bound there (rr_worst below says how far the solves got).
 *
 * surfh_randn_dev: out_dev[i] = the standard normal of (seed, stream, sample, i), whatever the launch shape or call order.
 * Philox4x32-10, key (seed low, seed high), counter (i / 4 low, i / 4 high, stream, sample); the words (a0, a1) and (a2, a3)
 * give the Box-Muller pairs of elements 4c, 4c+1 and 4c+2, 4c+3:  u = ((a0 >> 8) + 1/2) 2^-24, theta = 2 pi ((a1 >> 8) + 1/2)
 * 2^-24, z0 = sqrt(-2 ln u) cos theta, z1 = sqrt(-2 ln u) sin theta; |z| <= 5.89.  Streams of the sampler: 0 eps_y, 1 eps_r, 2 eps_c. */
int surfh_randn_dev(surfh_plan *plan, float *out_dev, int64_t n, uint64_t seed, uint32_t stream, uint32_t sample);
/* out = y + eps / sqrt(mu w) where w > 0 (w_dev NULL: every weight 1), the bits of y elsewhere; n floats each, on the device.
 * y_dev NULL: the perturbation alone, eps / sqrt(mu w), and 0 where w = 0. */
int surfh_po_data_dev(surfh_plan *plan, const float *y_dev, const float *w_dev, const float *eps_dev, int64_t n, double mu, float *out_dev);
/* out = sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c) on device maps [T][Na][Nb] (the transposes of the separated circular differences) */
int surfh_po_prior_dev(surfh_plan *plan, const float *eps_r_dev, const float *eps_c_dev, double mu_reg, float *out_dev);
/* The moment kernels on their own, host buffers: K samples [K][T][npix] about xhat [T][npix], accumulated in float64 per pixel
 * in a fixed order; mean [T][npix] = xhat + S1 / K, cov [T (T + 1) / 2][npix] = the unbiased covariance of the pairs t <= u in
 * row-major order (NULL: not wanted; needs K >= 2).  1 <= T <= 8. */
int surfh_po_moments(int32_t T, int64_t npix, const float *xhat, const float *samples, int32_t K, double *mean, double *cov,
                     int32_t device);
/* The plane moments of surfh_cg_planes_sample on their own, host buffers: K samples [K][L][npix] about xhat [L][npix]; the planes are
 * independent, so the second moment is the variance alone.  S1 += e, S2 += e e in float64 per element in a fixed order, then in
 * place mean [L][npix] = xhat + S1 / K and var [L][npix] = (S2 - S1^2 / K) / (K - 1), clamped at 0 (NULL: not wanted; needs K >= 2). */
int surfh_po_planes_moments(int32_t L, int64_t npix, const float *xhat, const float *samples, int32_t K, double *mean, double *var,
                            int32_t device);
/* btilde [isize] = the perturbed right-hand side b~ of draw `sample` under `seed`, in the maps' layout.  eps NULL: the generator;
 * else one explicit draw, eps_y [osize] followed by eps_r and eps_c [isize] each (`seed`, `sample` unused).  For statistical
 * tests of the sampler and for callers that run their own loop.  Refuses what surfh_cg_sample refuses. */
int surfh_po_rhs(surfh_plan *plan, const float *y, double mu, double mu_reg, uint64_t seed, int32_t sample, const float *eps,
                 float *btilde);
/* surfh_cg (same arguments, same bits in x_map, grad_norm and nit), then n_samples solves of Q e = b~ - b from zero with the same
 * max_iter, tol and refresh, x~ = x_map + e, and the moments of the samples: mean [T][Na][Nb] = x_map + mean of e and cov
 * [T (T + 1) / 2][Na][Nb] (pairs t <= u, row-major) in float64, either may be NULL.  eps_y [n_samples][osize], eps_r and eps_c [n_samples][isize]: the noise
 * of every draw, or NULL for the generator under `seed` (sample k = counter word `sample`); eps_r / eps_c are not read when
 * mu_reg = 0.  rr_worst (may be NULL): the largest final r.r over the sample solves (to be read against their first, |b~ - b|^2).
 * The callback (may be NULL) receives every
 * finished sample: its index, the iterations of its solve, its r.r trace (nit + 1 values) and x~ [T][Na][Nb] on the host; a
 * non-zero return makes the call fail.  Refuses, before any work: plans without templates, the joint prior (surfh_set_prior),
 * an active imager term, mu <= 0, mu_reg < 0, n_samples < 1, and n_samples < 2 when cov is requested. */
typedef int (*surfh_sample_callback)(void *user, int32_t sample, int32_t nit, const double *rr, const float *x);
int surfh_cg_sample(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                    int32_t refresh, int32_t n_samples, uint64_t seed, const float *eps_y, const float *eps_r, const float *eps_c,
                    float *x_map, double *mean, double *cov, double *grad_norm, int32_t *nit, double *rr_worst,
                    surfh_sample_callback callback, void *user);
/* ---- ... of the plane-wise 2-D deconvolution: per-pixel uncertainty of the planes surfh_cg_planes returns ----
 * The same perturbation-optimisation on the Lc independent problems Q_l x_l = b_l of surfh_cg_planes (plans without templates; the
 * data weights are the plan's).  surfh_cg_planes itself (same arguments, same bits in x_map, grad_norm [nit + 1][Lc] and nit), then
 * n_samples solves of Q_l e_l = b~_l - b_l from zero with the same max_iter, tol and refresh: the perturbation eps_y / sqrt(mu w) alone
 * is the data of the solve and eta its extra right-hand side.  mean and var [Lc][Na][Nb] float64 (either may be NULL): x_map + the mean
 * of e, and the unbiased variance of e per pixel -- the planes are independent, so there is no covariance.
 * Generator (eps_* NULL): eps_y is stream 0 over the flat index of y, eps_r / eps_c are streams 1 / 2 over the flat index of
 * [Lc][Na][Nb], counter = index / 4, sample k = counter word `sample` -- the streams surfh_randn_dev writes -- but generated in
 * registers by the kernels that consume them: no noise vector is stored, and beside the solver's vectors the call holds eta and x_map
 * [isize] floats and two float64 sums per element, which the finish turns into mean and var in place.  Explicit draws (eps_y
 * [n_samples][osize], eps_r / eps_c [n_samples][isize]; eps_r / eps_c not read when mu_reg = 0, one of them NULL: generated) go
 * through the staged kernels of surfh_cg_sample on buffers allocated on that first use.
 * rr_first, rr_last [Lc] (may be NULL): per plane the largest first and the largest final r.r over the sample solves; a plane whose
 * rr_first is exactly 0 drew no perturbation at all (no data weight and mu_reg = 0: its posterior is improper, its var of 0 means
 * "unknown", not "certain").  The callback (may be NULL) receives every finished sample: its index, the iterations of its solve, its
 * r.r trace [nit + 1][Lc] and x~ = x_map + e [Lc][Na][Nb] on the host; without one no sample is copied to the host.  The plan is left
 * as surfh_cg_planes leaves it.  Refuses, before any work: plans with templates, an active imager term, the joint prior, mu not
 * finite and > 0, mu_reg not finite and >= 0, n_samples < 1 (< 2 when var is requested), max_iter < 0, and what surfh_cg_planes refuses. */
int surfh_cg_planes_sample(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter, double tol,
                           int32_t refresh, int32_t n_samples, uint64_t seed, const float *eps_y, const float *eps_r, const float *eps_c,
                           float *x_map, double *mean, double *var, double *grad_norm, int32_t *nit, double *rr_first, double *rr_last,
                           surfh_sample_callback callback, void *user);
/* btilde [Lc][Na][Nb] = b~ = mu A^T W y~ + eta of draw `sample` under `seed`, the twin of surfh_po_rhs for the planes: eps NULL: the
 * generator; else one explicit draw, eps_y [osize] followed by eps_r and eps_c [isize] each.  Refuses what surfh_cg_planes_sample refuses. */
int surfh_po_planes_rhs(surfh_plan *plan, const float *y, double mu, double mu_reg, uint64_t seed, int32_t sample, const float *eps,
                        float *btilde);
/* 3MG, the reference's other solver choice (`method != 'lcg'` -> qmm.mmmg, fusion_CT.py:194-198; algorithms.py:69,106),
 * for the same quadratic criterion: every iteration minimises it exactly over span{-gradient, previous move}
 * (the quadratic majorant of a quadratic objective is the objective).  The 2x2 subspace system is solved in a basis
 * [d, move] with d Q-orthogonal to the previous move and the operator applied to d -- the same iterates as qmm's
 * [-gradient, move] form in exact arithmetic, but as accurate as CG in fp32 (see plan_solvers.hip).  One normal-operator
 * application per iteration; the gradient is carried by linearity and recomputed every `refresh` iterations.
 * grad_norm receives |gradient| of x0 and of every iterate (nit+1 doubles, capacity max_iter+1); stops when it falls
 * below size*tol.  callback as surfh_cg_cb. */
int surfh_mmmg(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0,
               int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
               surfh_cg_callback callback, void *user);
/* 3MG with edge-preserving Huber priors on the separated circular first differences (the reference's lmm_reconstruction,
 * surfh/ToolsDir/algorithms.py:73-106: qmm.mmmg with qmm.Huber(delta) on the row and column differences).  Minimises
 *   J(x) = mu |y - A x|^2 / 2 + mu_reg sum_{k in r,c} sum_pixels phi(D_k x),
 *   phi(u) = u^2 / 2 for |u| <= delta, delta (|u| - delta / 2) beyond;
 * each iteration minimises the half-quadratic (Geman-Reynolds) majorant of J at x, weights w(u) = phi'(u) / u, over
 * span{-gradient, previous move}.  delta = +inf is the quadratic criterion of surfh_mmmg (whatever surfh_set_prior holds,
 * the separated differences are used).  Contract of surfh_mmmg otherwise: grad_norm receives |gradient| of x0 and of every
 * iterate, the loop stops below size*tol, the data gradient is carried and recomputed every `refresh` iterations; callback
 * as surfh_cg_cb.  prior_value (may be NULL) receives sum_k sum phi(D_k x) of the returned iterate.  The kernels work in fp32:
 * fails on delta below FLT_MIN (delta <= 0 included), a NaN delta or mu_reg, and on non-positive curvature.  Template plans
 * only. */
int surfh_mmmg_huber(surfh_plan *plan, const float *y, double mu, double mu_reg, double delta, const float *x0,
                     int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
                     double *prior_value, surfh_cg_callback callback, void *user);
/* the Huber prior alone, on device maps [T][Na][Nb]: g += mu_reg sum_k D_k^T phi'(D_k x); *value_host = sum_k sum phi(D_k x)
 * (float64 sums in a fixed order: repeated calls give the same bits).  Same delta rules as surfh_mmmg_huber. */
int surfh_huber_prior_dev(surfh_plan *plan, const float *x_dev, float *g_dev, double mu_reg, double delta, double *value_host);
/* the prior block of the majorant: sums_host[0..2] = sum_k sum w(D_k x) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2, the weights
 * w(u) = phi'(u) / u recomputed from x (same summation rules) */
int surfh_huber_curv_dev(surfh_plan *plan, const float *x_dev, const float *p0_dev, const float *p1_dev, double delta, double *sums_host);
/* The same solver on the hyperspectral cube itself (the reference's vox_reconstruction, surfh/ToolsDir/algorithms.py:27-71:
 * qmm.mmmg with qmm.Huber on the row, column and spectral differences).  Plans without templates only (n_templates = 0):
 * x is the cube [Lc][Na][Nb], A the cube-domain operator of the plan.  Minimises
 *   J(x) = mu |y - A x|^2 / 2 + spat_reg sum_{k in r,c} sum phi_{spat_delta}(D_k x) + spec_reg sum phi_{spec_delta}(D_l x),
 * phi and w = phi'/u as above.  D_r, D_c: the separated circular differences inside every plane (the planes take the place of
 * the maps).  D_l: (D_l x)[l] = x[l+1] - x[l], l = 0 .. Lc-2, NOT circular (Lc - 1 difference planes; (D_l^T v)[l] = v[l-1] - v[l]
 * with v[-1] = v[Lc-1] = 0): a wrap would tie the shortest to the longest wavelength of the cube, which means nothing
 * physically.  Adjacent planes are differenced whatever their spacing, as the reference does; Lc = 1 leaves the spectral term
 * empty.  Both border conventions are unpinned against aljabr.Diff, which is not available (the reference's legacy Spectro model
 * is (alpha, beta, lambda), hence its Diff(0) / Diff(1) / Diff(2); the cube here is [lambda][alpha][beta]).
 * Majorant at x:  B(x) = mu A^T A + spat_reg sum_k D_k^T diag(w(D_k x)) D_k + spec_reg D_l^T diag(w(D_l x)) D_l, minimised over
 * span{-gradient, previous move} in the [d, m] basis of surfh_mmmg_huber, whose contract holds otherwise (trace, stopping test
 * |gradient| < size * tol, refresh, callback, failure on non-positive curvature).  Either delta may be +inf (that term is then
 * quadratic; both: the quadratic solve of the cube-domain operator); a delta below FLT_MIN or NaN, or a NaN weight, fails; a weight
 * of 0 switches its family off.  prior_values (may be NULL) receives the spatial and the spectral sum of phi at the returned
 * iterate.  Work vectors: 8 cubes. */
int surfh_mmmg_huber_vox(surfh_plan *plan, const float *y, double mu, double spat_reg, double spat_delta, double spec_reg,
                         double spec_delta, const float *x0, int32_t max_iter, double tol, int32_t refresh, float *x,
                         double *grad_norm, int32_t *nit, double *prior_values, surfh_cg_callback callback, void *user);
/* the two stencil passes alone, on device cubes [Lc][Na][Nb] (float64 sums in a fixed order: repeated calls give the same bits):
 * g += spat_reg sum_k D_k^T phi'(D_k x) + spec_reg D_l^T phi'(D_l x) in one pass; values_host[0..1] (may be NULL) = the spatial and
 * the spectral sum of phi */
int surfh_huber_vox_prior_dev(surfh_plan *plan, const float *x_dev, float *g_dev, double spat_reg, double spat_delta,
                              double spec_reg, double spec_delta, double *values_host);
/* sums_host[0..2] = sum_k sum w(D_k x) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2 under the spatial weights, [3..5] the same on D_l
 * under the spectral weights: the host applies spat_reg and spec_reg in float64 */
int surfh_huber_vox_curv_dev(surfh_plan *plan, const float *x_dev, const float *p0_dev, const float *p1_dev, double spat_delta,
                             double spec_delta, double *sums_host);
/* ---- robust (Huber) data term: outlier-tolerant fusion (qmm.Objective(forward, adjoint, Huber(data_delta), data=y)) ----
 * 3MG on
 *   J(x) = mu sum_i phi_{data_delta}(t_i) + mu_reg sum_{k in r,c} sum phi_{delta}(D_k x),   t_i = sqrt(w_i) (y_i - (A x)_i),
 * w the plan's data weights (surfh_set_data_weights; 1 without): with w = 1 / sigma^2 data_delta is in units of sigma.  A sample
 * of weight 0 contributes nothing whatever it holds, NaN and Inf included.  data_delta = +inf is the weighted quadratic data
 * term of surfh_mmmg_huber, delta = +inf the quadratic prior of surfh_mmmg (separated differences).  The majorant's data block is
 * mu A^T diag(w omega(t)) A, omega(t) = phi'(t) / t recomputed at every iterate, so the loop keeps A x and A m as detector vectors
 * and applies one forward and one adjoint per iteration (no normal operator); A x is recomputed every `refresh` iterations.
 * Trace, stopping test, callback and failure on non-positive curvature as surfh_mmmg_huber; data_delta follows delta's rules
 * (at least FLT_MIN, not NaN).  values (may be NULL) receives sum_i phi(t_i), the number of |t_i| > data_delta, then the prior
 * value, all at the returned iterate; omega_out (may be NULL) receives its robustness weights omega(t_i) [osize], in (0, 1], 0
 * where w_i = 0.  Template plans with detector channels only.  Work vectors: 4 maps (x, the data part of -g, -g, m) and 5 detector
 * vectors (y, A x, v, A (-g), A m). */
int surfh_mmmg_robust(surfh_plan *plan, const float *y, double mu, double data_delta, double mu_reg, double delta, const float *x0,
                      int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit, double *values,
                      float *omega_out, surfh_cg_callback callback, void *user);
/* the same data term with the two prior families of surfh_mmmg_huber_vox, on the cube (plans without templates); values receives
 * sum phi(t), the number beyond data_delta, the spatial and the spectral prior value */
int surfh_mmmg_robust_vox(surfh_plan *plan, const float *y, double mu, double data_delta, double spat_reg, double spat_delta,
                          double spec_reg, double spec_delta, const float *x0, int32_t max_iter, double tol, int32_t refresh,
                          float *x, double *grad_norm, int32_t *nit, double *values, float *omega_out, surfh_cg_callback callback,
                          void *user);
/* the detector-space passes alone, on device vectors of n floats (w_dev may be NULL: every weight 1; float64 sums in a fixed
 * order: repeated calls give the same bits): v = sqrt(w) phi'(t), t = sqrt(w) (y - u); sums_host[0] = sum phi(t), [1] = the number
 * of |t| > data_delta */
int surfh_robust_data_dev(surfh_plan *plan, const float *y_dev, const float *u_dev, const float *w_dev, int64_t n, double data_delta,
                          float *v_dev, double *sums_host);
/* sums_host[0..2] = sum w omega(t) p0^2, sum w omega(t) p0 p1, sum w omega(t) p1^2: the data block of the majorant before mu */
int surfh_robust_curv_dev(surfh_plan *plan, const float *y_dev, const float *u_dev, const float *w_dev, const float *p0_dev,
                          const float *p1_dev, int64_t n, double data_delta, double *sums_host);

/* ---- linear mixing model on the device: the drivers' mapsToCube / cubeTomaps
 * (spectroModel.py:187-198, jax_utils.py:10-26).  templates [T][Lc] float64 as in surfh_config,
 * maps [T][Na][Nb], cube [Lc][Na][Nb]; works on any plan (only its device and stream are used).   */
int surfh_maps_to_cube(surfh_plan *plan, const double *templates, int32_t n_templates, int32_t n_lambda,
                       const float *maps, float *cube);
int surfh_cube_to_maps(surfh_plan *plan, const double *templates, int32_t n_templates, int32_t n_lambda,
                       const float *cube, float *maps);

/* The same solver for the plane-wise model (n_templates = 0: x is the cube [Lc][Na][Nb]): every plane is an independent
 * 2-D problem  mu |y_l - A_l x_l|^2 + mu_reg (|Dr x_l|^2 + |Dc x_l|^2)  with its own CG scalars -- the reference's 2-D
 * deconvolution (surfh/Simulation/criterion_2D.py:60-250, scripts/deconvolution_mrs_noRotation.py) batched over
 * wavelength.  grad_norm receives r_l.r_l as [max_iter+1][Lc]; the loop stops when every plane is below the tolerance. */
int surfh_cg_planes(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter,
                    double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit);
/* 3MG on the plane-wise model -- what `method = "qmm"` of the 2-D deconvolution driver selects
 * (scripts/deconvolution_mrs_noRotation.py:199-212 -> criterion_2D.py:190-193 -> qmm.mmmg).  Scheme of surfh_mmmg with
 * per-plane scalars; grad_norm receives |gradient_l| as [max_iter+1][Lc].                                            */
int surfh_mmmg_planes(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter,
                      double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit);

/* The plane-wise CG with the data and the iterate resident on the device and no host synchronisation inside the loop (drivers
 * that keep their cubes in HBM; bench.py --config 5).  begin: b = mu A^T y, r = b - Q x, d = r, with x_dev [Lc][Na][Nb] the start
 * and from then on the current iterate (the caller's buffer, updated in place by step);  step: `iters` more iterations of the loop
 * of surfh_cg_planes (residual recomputed every `refresh` iterations, counted from begin);  rr: r_l.r_l of the current iterate,
 * [Lc] doubles on the host (synchronises the plan's stream).  All pointers except rr_host are device pointers. */
int surfh_cg_planes_begin_dev(surfh_plan *plan, const float *y_dev, double mu, double mu_reg, float *x_dev);
int surfh_cg_planes_step_dev(surfh_plan *plan, int32_t iters, int32_t refresh);
int surfh_cg_planes_rr(surfh_plan *plan, double *rr_host);

/* the two plane-wise solvers with qmm's per-iteration callback (criterion_2D.py:163-225): grad_norm is the trace so far,
 * [it + 1][Lc] values, x the current iterate [Lc][Na][Nb] on the host; a non-zero return stops the loop */
int surfh_cg_planes_cb(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter,
                       double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
                       surfh_cg_callback callback, void *user);
int surfh_mmmg_planes_cb(surfh_plan *plan, const float *y, double mu, double mu_reg, const float *x0, int32_t max_iter,
                         double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
                         surfh_cg_callback callback, void *user);

/* 3MG with edge-preserving Huber priors on the plane-wise model (n_templates = 0 only): every plane l minimises its own
 *   J_l(x_l) = mu |y_l - A_l x_l|^2 / 2 + mu_reg sum_{k in r,c} sum phi_delta(D_k x_l)
 * (phi, D_r, D_c as for surfh_mmmg_huber; mu_reg and delta shared by the planes; data weights act in A_l^T W A_l as in the other
 * solvers) by the majorant scheme of surfh_mmmg_huber with its own beta, 2x2 system and step, all formed on the device.  Loop,
 * trace and callback as surfh_mmmg_planes_cb: grad_norm receives |gradient_l| as [max_iter+1][Lc], the loop stops when the worst
 * plane is below Na Nb tol.  A plane without positive curvature (no data, or at its minimum) keeps still.  delta = +inf gives the
 * quadratic criterion of surfh_mmmg_planes up to its factor 1/2 (same minimiser, same iterates).  prior_values (may be NULL)
 * receives sum_k sum phi(D_k x_l) of the returned iterate, [Lc].  Same delta and mu_reg rules as surfh_mmmg_huber. */
int surfh_mmmg_huber_planes(surfh_plan *plan, const float *y, double mu, double mu_reg, double delta, const float *x0,
                            int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm, int32_t *nit,
                            double *prior_values, surfh_cg_callback callback, void *user);
/* the two stencil passes of that solver alone, on device arrays [Lc][Na][Nb] (float64 sums in a fixed order: repeated calls give
 * the same bits; a plane's results depend on that plane only):  g += mu_reg sum_k D_k^T phi'(D_k x) with sq_host[l] = |g_l|^2 of the
 * result and values_host[l] = sum_k sum phi(D_k x_l) (either may be NULL);  sums_host[k][l], k = 0..2, = sum_k sum w(D_k x_l)
 * (D_k p0_l)^2, (D_k p0_l)(D_k p1_l), (D_k p1_l)^2, as [3][Lc] */
int surfh_huber_planes_prior_dev(surfh_plan *plan, const float *x_dev, float *g_dev, double mu_reg, double delta, double *sq_host,
                                 double *values_host);
int surfh_huber_planes_curv_dev(surfh_plan *plan, const float *x_dev, const float *p0_dev, const float *p1_dev, double delta,
                                double *sums_host);
/* The same solver and passes with every plane's own weight and threshold, and a coupling of the row and the column difference of
 * a pixel.  mu_reg [Lc] and delta [Lc] (host arrays): plane l minimises
 *   J_l(x_l) = mu |y_l - A_l x_l|^2 / 2 + mu_reg[l] sum phi_delta[l](.)
 * -- a cube's flux changes by orders of magnitude along the wavelength, and one threshold in absolute flux units leaves its faint
 * planes fully quadratic.  Every delta[l] follows the rule of surfh_mmmg_huber (positive, at least FLT_MIN, +inf allowed), every
 * mu_reg[l] must be >= 0.  coupling is a per-call argument, not plan state (the plan's slot, surfh_set_prior_coupling, is the maps'
 * and is still refused here while it is not 0):
 *   0  none       sum_ij phi(u_r) + phi(u_c): with Lc copies of one mu_reg and one delta, the arithmetic and the bits of the entry
 *                 points above, which forward here
 *   1  isotropic  sum_ij phi(sqrt(u_r^2 + u_c^2)): total variation for Huber's phi; an edge pays the same whatever its angle to the
 *                 pixel grid.  delta[l] is then the threshold on the group magnitude (sqrt(2) times larger for comparable behaviour);
 *                 the majorant weights every difference of a pixel by w(m) = phi'(m) / m, recomputed in place from a 7-point
 *                 stencil (no weight field is stored); prior_values / values_host receive sum_ij phi(m)
 *   2  vector     refused (the message names "vector"): it would tie the independent planes together under one trace and one
 *                 stopping test, which is a different solver.
 * The planes stay independent: plane l of a run on arrays equals, bit for bit, plane l of a run on the scalars mu_reg[l], delta[l]
 * that takes as many iterations.  curv_dev takes no mu_reg. */
int surfh_mmmg_huber_planes_ex(surfh_plan *plan, const float *y, double mu, const double *mu_reg, const double *delta, int32_t coupling,
                               const float *x0, int32_t max_iter, double tol, int32_t refresh, float *x, double *grad_norm,
                               int32_t *nit, double *prior_values, surfh_cg_callback callback, void *user);
int surfh_huber_planes_prior_dev_ex(surfh_plan *plan, const float *x_dev, float *g_dev, const double *mu_reg, const double *delta,
                                    int32_t coupling, double *sq_host, double *values_host);
int surfh_huber_planes_curv_dev_ex(surfh_plan *plan, const float *x_dev, const float *p0_dev, const float *p1_dev, const double *delta,
                                   int32_t coupling, double *sums_host);

/* CG building blocks on device vectors, for the multi-GPU driver (one plan per rank,
 * RCCL all-reduce of `q` between surfh_normal_dev and surfh_cg_step_dev).            */
int surfh_normal_dev(surfh_plan *plan, const float *d_dev, float *q_dev, double mu);          /* q  = mu A^T A d   */
int surfh_prior_add_dev(surfh_plan *plan, const float *d_dev, float *q_dev, double mu_reg);   /* q += mu_reg L d   */
/* The same building blocks with the solver's vectors in the Fourier domain of the maps (no transform of the maps, no padding and
 * no prior kernel inside the iteration: the forward model reads the spectra in the loader of its first transform pass, the
 * adjoint's last pass writes them).  A vector holds surfh_spec_size() floats: [T][2 (re, im)][KAP][KBP], padding zero, bin
 * (ka, kb) of the unitary half spectrum (rfft2 / sqrt(Na Nb)) multiplied by sqrt(2) unless the bin is its own conjugate
 * (kb = 0 or 2 kb = Nb) -- so plain dot products of such vectors equal the dot products of the maps, and the CG recurrences
 * (surfh_cg_iter_dev ...) run on them unchanged.  The quadratic prior here is the separated circular first differences
 * (surfh_set_prior 0), diagonal in this basis.  Available where the fused transform passes are (surfh_spec_supported).    */
int surfh_spec_supported(surfh_plan *plan);                                                    /* 1 / 0 */
int64_t surfh_spec_size(surfh_plan *plan);
int surfh_to_spec_dev(surfh_plan *plan, const float *x_dev, float *xt_dev);                    /* maps -> vector */
int surfh_from_spec_dev(surfh_plan *plan, const float *xt_dev, float *x_dev);                  /* vector -> maps */
int surfh_forward_spec_dev(surfh_plan *plan, const float *dt_dev, float *y_dev);               /* y = A maps(dt) */
/* qt = mu spectra(A^T y) (+ mu_reg L dt if dt_dev != NULL: only where qt is not summed over ranks afterwards) */
int surfh_adjoint_spec_dev(surfh_plan *plan, const float *y_dev, float *qt_dev, double mu, const float *dt_dev, double mu_reg);
/* qt = mu A^T A dt (+ mu_reg L dt if mu_reg != 0) */
int surfh_normal_spec_dev(surfh_plan *plan, const float *dt_dev, float *qt_dev, double mu, double mu_reg);
int surfh_prior_spec_add_dev(surfh_plan *plan, const float *dt_dev, float *qt_dev, double mu_reg);   /* qt += mu_reg L dt */
/* which quadratic regulariser L the solvers and surfh_prior_add_dev apply (QuadCriterion_MRS's `gradient`, fusion_CT.py:98-106,141-162):
 * 0 = "separated": Dr^T Dr + Dc^T Dc, circular first differences NpDiff_r / NpDiff_c (fusion_CT.py:16-43) -- the default;
 * 1 = "joint": D^T D with D the circular convolution by the 3 x 3 Laplacian (Difference_Operator_Joint, fusion_CT.py:45-62).  */
int surfh_set_prior(surfh_plan *plan, int32_t kind);
/* ---- potentials: plan state, like the prior and the data weights ----
 * Which potential phi the non-quadratic terms of the 3MG solvers use.  Everything said of "Huber" at surfh_mmmg_huber(_vox,
 * _planes), surfh_mmmg_robust(_vox) and their *_dev passes holds for the other kinds with their phi, phi' and w = phi' / u; all
 * are normalised alike (phi(u) ~ u^2 / 2 near 0, w(0) = 1, delta = +inf exactly the quadratic term).  With t = u / delta:
 *   kind 0  huber         phi = u^2 / 2 (|u| <= delta), delta (|u| - delta / 2) beyond    w = 1 or delta / |u|       (the default)
 *   kind 1  hyperbolic    phi = delta^2 (sqrt(1 + t^2) - 1)                                w = 1 / sqrt(1 + t^2)
 *   kind 2  hebert_leahy  phi = delta^2 log(1 + t^2) / 2                                   w = 1 / (1 + t^2)
 * hyperbolic (Charbonnier, pseudo-Huber) is convex with a smooth w; Hebert-Leahy is non-convex, phi' redescends (as a data term
 * the Cauchy / Student-t likelihood): the majorant still holds and every iteration descends, but the limit is a local minimum
 * that depends on the start.  phi' is formed as u w; no NaN or Inf for any finite u and any delta >= FLT_MIN (|t| >= 2^24: the
 * hyperbolic w is delta / |u|; the Hebert-Leahy w flushes to 0 once t^2 overflows fp32).
 *   slot 0  the spatial prior: the maps (surfh_mmmg_huber, surfh_mmmg_robust, surfh_huber_prior_dev / _curv_dev), the planes
 *           (surfh_mmmg_huber_planes, surfh_huber_planes_prior_dev / _curv_dev) and the cube's row / column families
 *   slot 1  the cube's spectral prior (surfh_mmmg_huber_vox, surfh_mmmg_robust_vox, surfh_huber_vox_prior_dev / _curv_dev)
 *   slot 2  the data term (surfh_mmmg_robust(_vox), surfh_robust_data_dev / _curv_dev); the count "number of |t| > data_delta"
 *           keeps its meaning for every kind: the samples past the knee
 * A new plan holds huber in all three.  The quadratic surfh_mmmg and the CG solvers ignore the slots.  set fails on an unknown
 * slot or kind (message in surfh_last_error) and leaves the plan as it was; get returns the kind, or -1 on an unknown slot. */
int surfh_set_potential(surfh_plan *plan, int32_t slot, int32_t kind);
int surfh_get_potential(const surfh_plan *plan, int32_t slot);
/* ---- prior coupling: plan state, like the potentials and orthogonal to them ----
 * How the spatial prior of the MAPS groups the circular first differences u_r = Dr x, u_c = Dc x under its potential phi (slot 0):
 *   coupling 0  none       sum_t sum_ij phi(u_r) + phi(u_c)                one potential per difference (the default: the kernels,
 *                                                                          launches and bits of a plan that never heard of couplings)
 *   coupling 1  isotropic  sum_t sum_ij phi(sqrt(u_r^2 + u_c^2))           an edge pays the same whatever its angle to the pixel grid
 *   coupling 2  vector     sum_ij phi(sqrt(sum_t u_r^2 + u_c^2))           one edge per pixel for all T maps: edges co-locate across maps
 * delta is then the threshold on the GROUP MAGNITUDE m = the square root above: for comparable behaviour it grows like sqrt(2)
 * under isotropic and like sqrt(2 T) under vector.  phi(sqrt(.)) is concave for every kind, so the half-quadratic majorant of
 * surfh_mmmg_huber holds with every difference of a group weighted by w(m) = phi'(m) / m: the gradient is
 * sum_k D_k^T (w(m) D_k x), the curvature sums are sum_k sum w(m) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2 and the prior value is
 * sum phi(m).  delta = +inf is the quadratic prior under every coupling; T = 1 makes vector the same as isotropic.
 * surfh_mmmg_huber, surfh_mmmg_robust, surfh_huber_prior_dev and surfh_huber_curv_dev honour the coupling (the imager term and the
 * data weights compose as before); they fail on a plan whose quadratic prior is the joint Laplacian (surfh_set_prior).  This
 * slot is the maps': the plane-wise and voxel-wise solvers and passes (surfh_mmmg_huber_planes(_ex), surfh_mmmg_huber_vox,
 * surfh_mmmg_robust_vox, the _planes_ and _vox_ *_dev passes) fail with a message naming the coupling while it is not 0.  The
 * plane-wise solver carries the isotropic coupling as a per-call argument instead (surfh_mmmg_huber_planes_ex and the _ex passes);
 * the cube's solvers carry none.  The quadratic surfh_mmmg and the CG solvers ignore the slot.  set fails on an unknown code and on
 * a NULL plan and leaves the plan as it was; get stores the code. */
int surfh_set_prior_coupling(surfh_plan *plan, int32_t coupling);
int surfh_get_prior_coupling(const surfh_plan *plan, int32_t *coupling);
/* ---- data weights: plan state, like the prior ----
 * With weights w [osize] (the layout of y; every w[i] finite and >= 0) the data term of every solver is
 *   mu (y - A x)^T W (y - A x) / 2,  W = diag(w):
 * a 0/1 mask of bad samples, an inverse variance 1/sigma^2, or their product.  They act
 *   - in every normal operator: surfh_normal_dev, surfh_fwadj(_dev), surfh_normal_spec_dev and the operators inside the solvers
 *     apply mu A^T W A;
 *   - in the right-hand side of every solver (surfh_cg(_cb), surfh_mmmg, surfh_mmmg_huber(_vox), surfh_cg_planes(_cb),
 *     surfh_mmmg_planes(_cb), surfh_mmmg_huber_planes, surfh_cg_planes_begin_dev): b = mu A^T W y, with W y formed by a select -- a sample of weight 0
 *     contributes nothing whatever its datum, NaN and Inf included.
 * They do NOT act on surfh_forward*, surfh_adjoint*, surfh_adjoint_ref*, surfh_forward_spec_dev and surfh_adjoint_spec_dev,
 * which stay A and A^T.  Priors, stopping rules and traces are untouched.
 * Both calls copy the weights into the plan (the caller's buffer is free afterwards); NULL clears them and frees the copies.
 * Both fail on a negative, NaN or infinite weight (the device form synchronises the plan's stream for its check) and on plans
 * without detector channels (n_channels = 0, the Model_WCT plans); a failed call leaves the plan's weights as they were. */
int surfh_set_data_weights(surfh_plan *plan, const float *w_host);
int surfh_set_data_weights_dev(surfh_plan *plan, const float *w_dev);
int surfh_has_data_weights(const surfh_plan *plan);                                            /* 1 / 0 */
/* ---- imager data term: a second instrument on the same maps (the reference's instru.MSImager; the slot y_imager / mu_imager /
 * model_imager its criterion classes reserve, fusion_CT.py:68, :243-261) ----
 * A multi-filter broadband imager sees the cube the maps span, blurred plane by plane, integrated over wavelength under F
 * filters, and summed over the decim x decim cube pixels one of its detector pixels spans:
 *   cube[l] = sum_t tpl[t,l] x[t];   blur[l] = irfft2(rfft2(cube[l]) sotf[l])  (ortho);   z[f] = sum_l filters[f,l] blur[l];
 *   y_im[f,a,b] = sum_{i,j < decim} z[f, a decim + i, b decim + j],   a < Na / decim, b < Nb / decim
 * -- whole detector pixels only: no wrap, rows and columns beyond (N / decim) decim are not observed.  filters [F][n_lambda] are
 * finite and >= 0 (WavelFilter.transmittance(wavelength axis, normalized=True) per row), 1 <= F <= 16, 1 <= decim <= min(Na, Nb).
 * sotf = NULL: the plan's own OTF, read on the device -- the plan must then own every cube plane (one channel window over the
 * whole axis, or n_channels = 0: the Model_WCT kind of plan may hold an imager).  Otherwise the imager's own OTF
 * [n_lambda][Na][Nb/2+1] complex128 (re, im pairs), streamed to the device in chunks of at most 128 planes; any plan with
 * templates takes it.  Either way the set-up reduces G[f,t,k] = sum_l filters[f,l] tpl[t,l] sotf[l,k] once, in float64, and an
 * application costs transforms of T + F planes.  surfh_set_imager(NULL desc) detaches: G and the data are freed.
 * surfh_imager_forward / _adjoint are A_im and its exact transpose, host buffers maps [T][Na][Nb] and y_im [surfh_imager_osize];
 * the _dev forms take device buffers and are asynchronous on the plan's stream.  surfh_imager_fwadj is A_im^T W_im A_im x.
 * surfh_set_imager_data(y_im, w_im, mu_imager) adds mu_imager (y_im - A_im x)^T W_im (y_im - A_im x) / 2 to the criterion of
 * surfh_cg(_cb), surfh_mmmg and surfh_mmmg_huber (every potential) -- the factor convention of their spectrometer term:
 * the operator of their loops gains mu_imager A_im^T W_im A_im, their right-hand side mu_imager A_im^T W_im y_im.  w_im
 * [surfh_imager_osize] follows the rules of the data weights (finite, >= 0, weight 0 takes the sample out whatever it holds, NaN
 * included; NULL: 1); mu_imager is finite and >= 0.  y_im = NULL clears the data.  While a term with mu_imager > 0 is set,
 * surfh_cg(_cb) runs its map-domain loop (folding G^H W G into surfh_normal_spec_dev is a follow-up: the term is not diagonal there
 * for decim > 1), and surfh_mmmg_robust(_vox), surfh_mmmg_huber_vox, the plane-wise solvers and surfh_cg_planes_begin_dev fail with
 * a message naming the imager.  With no imager, no data or mu_imager = 0 no kernel of the term is launched and every result has the
 * bits it had without.
 * surfh_forward*, surfh_adjoint*, surfh_fwadj*, surfh_normal_dev and the *_spec_dev calls stay the spectrometer's alone.
 * Failures (the plan is left as it was, the previous imager and data included): F outside 1..16, decim < 1 or larger than Na or
 * Nb, a negative or non-finite filter or weight, a plan without templates, sotf = NULL on a plan that does not own every plane.
 * SURFH_IMAGER_CHUNK (read by surfh_set_imager): planes per chunk of the streamed OTF, a multiple of 32 up to 128 (default 128);
 * the result has the same bits for every value. */
typedef struct {
    int32_t n_filters;
    const double *filters;         /* [n_filters][n_lambda] */
    int32_t decim;
    const double *sotf;            /* NULL: the plan's */
} surfh_imager_desc;
int surfh_set_imager(surfh_plan *plan, const surfh_imager_desc *desc);
int surfh_imager_osize(const surfh_plan *plan);                                                /* F (Na/d) (Nb/d), 0 without */
int surfh_imager_forward(surfh_plan *plan, const float *maps, float *y_im);
int surfh_imager_adjoint(surfh_plan *plan, const float *y_im, float *maps);
int surfh_imager_forward_dev(surfh_plan *plan, const float *maps_dev, float *y_im_dev);
int surfh_imager_adjoint_dev(surfh_plan *plan, const float *y_im_dev, float *maps_dev);
int surfh_imager_fwadj(surfh_plan *plan, const float *x, float *out);
int surfh_set_imager_data(surfh_plan *plan, const float *y_im, const float *w_im, double mu_imager);
int surfh_has_imager_term(const surfh_plan *plan);                                             /* 1: data with mu_imager > 0 is set */
int surfh_dot_dev(surfh_plan *plan, const float *a_dev, const float *b_dev, int64_t n, double *out_host);
/* x += s d ; r -= s q ; returns r.r  (s = rr / d.q computed on device from rr_in)    */
int surfh_cg_step_dev(surfh_plan *plan, float *x_dev, float *r_dev, const float *d_dev,
                      const float *q_dev, int64_t n, double rr_in, double *rr_out_host);
/* d = r + beta d */
int surfh_cg_dir_dev(surfh_plan *plan, float *d_dev, const float *r_dev, int64_t n, double beta);
/* the two calls above fused (one host synchronisation per CG iteration instead of two):
 * x += s d, r -= s q with s = rr_in / d.q; *rr_out = r.r; d = r + (*rr_out / rr_in) d        */
int surfh_cg_iter_dev(surfh_plan *plan, float *x_dev, float *r_dev, float *d_dev, const float *q_dev, int64_t n,
                      double rr_in, double *rr_out);

/* The same recurrences with every scalar resident on the device -- NO host synchronisation: r.r of the current iterate lives in
 * the plan, each call appends the new r.r to a device-side trace.  The multi-GPU loop (surfh_amd/fusion.py) is then
 * normal operator -> RCCL all-reduce -> one of these calls, all asynchronous on the plan's stream; the host reads the trace
 * every few iterations for the stopping test (surfh_cg_trace synchronises).                                                 */
int surfh_cg_begin_dev(surfh_plan *plan, const float *r_dev, int64_t n);                      /* rr = r.r, trace = [rr]        */
int surfh_cg_iter_nosync_dev(surfh_plan *plan, float *x_dev, float *r_dev, float *d_dev, const float *q_dev, int64_t n);
/* residual refresh of qmm.lcg, in two halves around the caller's normal operator on x:
 *   x += (rr / d.q) d          then, with q = Q x:   r = b - q; rr' = r.r; d = r + (rr' / rr) d; rr = rr'                      */
int surfh_cg_xupdate_nosync_dev(surfh_plan *plan, float *x_dev, const float *d_dev, const float *q_dev, int64_t n);
int surfh_cg_refresh_nosync_dev(surfh_plan *plan, float *r_dev, const float *b_dev, const float *q_dev, float *d_dev, int64_t n);
int32_t surfh_cg_trace(surfh_plan *plan, double *out_host, int32_t capacity);                 /* -> number of entries, -1 on error */
/* r = b - q */
int surfh_residual_dev(surfh_plan *plan, float *r_dev, const float *b_dev, const float *q_dev, int64_t n);

/* ---- instrumentation ---- */
/* enable/disable per-kernel HIP-event timing on the plan's stream */
int surfh_profile_enable(surfh_plan *plan, int32_t on);
/* restrict the timing to stages whose name starts with `prefix` (NULL or "": all).  Every bracketed stage costs two event
 * packets on the stream; bracketing all ~45 stages of an iteration was measured to slow it by 4.6 %, so a benchmark times
 * only the kernel group it reports inside its timed region. */
int surfh_profile_filter(surfh_plan *plan, const char *prefix);
/* number of distinct kernel names timed since the last reset */
int32_t surfh_profile_count(surfh_plan *plan);
/* i-th entry: name, launches, total milliseconds */
int surfh_profile_get(surfh_plan *plan, int32_t i, const char **name, int64_t *launches, double *ms);
int surfh_profile_reset(surfh_plan *plan);

/* copy an internal buffer to the host for stage-level parity tests.
 * which: "blurred" [Lown][NaP][NbP], "xs:<c>" [Kp][Np], "gcube" [Lown][NaP][NbP], ...
 * returns the number of floats written (<= capacity) or a negative error.            */
int64_t surfh_debug_copy(surfh_plan *plan, const char *which, float *out, int64_t capacity);
int surfh_debug_dims(surfh_plan *plan, const char *which, int64_t dims[4]);

/* stand-alone fp32 MFMA GEMM self-test hook: C[M][N] = A[M][K] B[K][N] (host buffers) */
int surfh_gemm_selftest(int32_t device, int32_t M, int32_t N, int32_t K, int32_t split_k,
                        const float *A, const float *B, float *C);
/* (tile, K step) pairs the last two-piece fp16 self-test (SURFH_SELFTEST_F16X2=2: with K-step lists, as the spectral-blur
 * GEMMs of a plan) ran with all three products / with the leading product only */
int surfh_gemm_selftest_ksteps(int64_t near_far[2]);
/* mean milliseconds per launch of the last two-piece fp16 self-test run with SURFH_SELFTEST_REPEAT=<n> (n timed launches behind
 * three warm-up ones, device events); -1 when the last self-test did not repeat its launch */
int surfh_gemm_selftest_ms(double *ms);
/* host only (no GPU): the K-step classes the spectral-blur GEMMs of a plan would use for the constant operand B [n][ldb]
 * (k columns, k % 32 == 0): records[(tile) * (2 + k / 32)] = n_near, n_far, near steps ascending, far steps ascending
 * (entry = step | segment << 16).  perm_p / perm_lin: the adjoint's tile shape (0: tiles of 256 consecutive rows).
 * Returns the number of tiles, or a negative error.                                                                     */
int32_t surfh_klist_classify(const float *B, int32_t n, int32_t k, int64_t ldb, int32_t perm_p, int32_t perm_lin,
                             int32_t *records, int64_t capacity);
/* host only (no GPU, no plan): the launch geometry of the capped-grid kernels, from the functions their launchers call.
 * out = { grid x, grid y, partial sums the consumer adds (0: none), most loop trips of one thread }.  which:
 *   "dot" (dot_partial, cg_step, cg_step_parts), "cg_axpy" (cg_dir, cg_xupdate, residual), "cg_dir_parts", "po_data":  a = n
 *   "robust": a = n, b = V floats per thread (4, 2, 1);  "nn_project": a = n, b = 1 for the 16-byte path
 *     (trips of the vector loop; the floats behind the last whole group go one to a thread)
 *   "huber_maps": a, b, c = T, Na, Nb;  "huber_vox": a, b, c = Lc, Na, Nb, out[3] = the most planes of one chunk,
 *     chunk k of C = out[1] owning planes [Lc k / C, Lc (k + 1) / C)                                                     */
int surfh_launch_geometry(const char *which, int64_t a, int64_t b, int64_t c, int64_t out[4]);
/* diagnostic: the prior passes of the maps on device arrays of ANY shape [T][na][nb] (every extent >= 1; a plan cannot have an
 * axis of length 1), under an explicit potential kind and prior coupling -- the launchers surfh_huber_prior_dev and
 * surfh_huber_curv_dev call, on the plan's stream and scratch; the plan's own shape, kind and coupling are not consulted.
 * g += mu_reg sum_k D_k^T phi'(D_k x) (under a coupling: D_k^T (w(m) D_k x)); sums [5] on the host = g.g, the prior value and the
 * curvature block of (p0, p1).  Synchronises. */
int surfh_debug_prior_passes(surfh_plan *plan, int32_t T, int32_t na, int32_t nb, int32_t kind, int32_t coupling, const float *x_dev,
                             float *g_dev, const float *p0_dev, const float *p1_dev, double mu_reg, double delta, double *sums);
/* diagnostic: the same for the PLANE passes (surfh_huber_planes_prior_dev_ex / _curv_dev_ex) on device arrays of any shape
 * [L][na][nb] (every extent >= 1; no slit geometry gives a plan an axis of length 1 or 2), one workgroup per plane, under an
 * explicit kind, a plane-wise coupling (0 or 1; 2 fails naming "vector") and per-plane mu_reg [L] and delta [L] (host arrays, the
 * rules of the _ex entry points).  g += mu_reg[l] sum_k D_k^T (w D_k x) per plane; sums [5][L] on the host = g.g, the prior value
 * and the curvature block of (p0, p1) of every plane.  The plan gives its stream only; the scratch is the call's own.
 * Synchronises. */
int surfh_debug_planes_passes(surfh_plan *plan, int32_t L, int32_t na, int32_t nb, int32_t kind, int32_t coupling, const float *x_dev,
                              float *g_dev, const float *p0_dev, const float *p1_dev, const double *mu_reg, const double *delta,
                              double *sums);
/* diagnostic: ONE vector kernel of the plane-wise CG / 3MG loops (surfh_cg_planes, surfh_mmmg_planes, surfh_cg_planes_begin_dev /
 * _step_dev) on device arrays of explicit extents, through the launcher the solvers call.  The plan gives its stream only; the
 * scalars and the partial sums live in buffers of the call's own.  Synchronises.  which, its vectors v0.. and its scalar rows:
 *   plane-major, arrays [L][npix], ext = { L, npix }, one scalar per plane (rows of L doubles):
 *     "dot"        a, b                      out: a.b
 *     "cg_step"    x, r, d, q                in: rr, d.q   out: r'.r' (update_r; left as it came otherwise)   x += s d, r -= s q
 *     "cg_dir"     d, r                      in: rr', rr   out: rr <- rr'                                    d = r + (rr' / rr) d
 *     "mmmg_dir"   d, r, m, qm               out: r.r, m.Qm                                                  d = r + beta m
 *     "mmmg_step"  x, r, d, m, qm, qd        in: m.Qm                                                        the 2x2 step (surfh_mm_step2)
 *   wavelength-innermost, arrays [Nb][NAP][LP], ext = { Na, Nb, NAP, LP, L, l0 } (L <= LP owned wavelengths, l0 = 0), one scalar
 *   per wavelength (rows of LP doubles):
 *     "pn_prior_dot"  d, q                   out: d.q      q += mu_reg (Dr^T Dr + Dc^T Dc) d (circular)
 *     "pn_dot"        x, y                   out: x.y
 *     "pn_step"       x, r, d, q             in: rr, d.q   out: r'.r' (update_r)
 *     "pn_dir"        d, r                   in: rr', rr
 *   transposes, same ext: "to_lam_inner" src [l0 + L][Na][Nb] -> dst [Nb][NAP][LP] (planes 0 .. L-1), "from_lam_inner" the way back.
 * Vectors a kernel does not take are NULL.  sc_in / sc_out: host arrays of the rows listed, in that order; sc_out is uploaded
 * before the launch, so an entry the kernel does not write comes back unchanged.  Extents below 1, NAP < Na, L > LP, arrays of
 * 2^31 floats or more, LP % 64 != 0, an unknown name and a missing pointer fail with a message and launch nothing. */
int surfh_debug_planes_cg(surfh_plan *plan, const char *which, const int64_t *ext, float *v0, float *v1, float *v2, float *v3,
                          float *v4, float *v5, double mu_reg, int32_t update_r, const double *sc_in, double *sc_out);
/* diagnostic: ONE fused perturbation kernel of surfh_cg_planes_sample on a device array of explicit extents, through the sampler's
 * launcher (the plan gives its stream only; synchronises).  which = "eta": out_dev [L][na][nb] = sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c)
 * of draw (seed, sample) -- surfh_randn_dev on streams 1 and 2 followed by surfh_po_prior_dev on T = L maps, bit for bit (n_out, mu,
 * w_dev unused).  which = "data": out_dev [n_out] = eps_y / sqrt(mu w), 0 where w = 0 (w_dev NULL: 1) -- surfh_randn_dev on stream 0
 * followed by surfh_po_data_dev(y_dev = NULL), bit for bit (L, na, nb, mu_reg unused).  Any alignment of out_dev and w_dev. */
int surfh_debug_po_planes(surfh_plan *plan, const char *which, int32_t L, int32_t na, int32_t nb, int64_t n_out, uint64_t seed,
                          int32_t sample, double mu, double mu_reg, const float *w_dev, float *out_dev);
/* diagnostic: ONE application of the normal operator of the device-resident plane-wise CG (surfh_cg_planes_begin_dev / _step_dev
 * on wavelength-innermost vectors), q = mu A^T W A v + mu_reg (Dr^T Dr + Dc^T Dc) v, through the function the loop calls, on the
 * loop's own buffers: v_dev [Lc][Na][Nb] is transposed into the cube's layout [NBP][NAP][LP] as the begin call transposes x0, the
 * operator runs under the given mu / mu_reg -- on the plan's route: with mu and the prior folded into the adjoint's OTF product
 * (interleaved spectra) or into the loader of the inverse transform (the product loader), or as the unfolded operator followed by
 * the prior kernel (dense plans, mu_reg = 0) -- with the plan's data weights, and q_dev [Lc][Na][Nb] is transposed back as the
 * step call brings the iterate back.  dq_host [Lc]: v_l . q_l per plane, the sum the operator's last kernel leaves for the step.
 * q_raw_dev (or NULL): the padded vector itself, [NBP][NAP][LP] floats (surfh_debug_dims "blurred": NBP, NAP, LP).  Synchronises.
 * The call leaves the plan's mu / mu_reg as they were, but it overwrites the loop's vectors: a loop begun with
 * surfh_cg_planes_begin_dev has to be begun again after it (surfh_cg_planes_step_dev fails until then).
 * A plan with templates, a plan that does not run the wavelength-innermost loop (SURFH_PLANES_NATIVE=0), a null plan, v_dev, q_dev
 * or dq_host and a negative or non-finite mu or mu_reg fail with a message naming the argument and launch nothing. */
int surfh_debug_planes_normal(surfh_plan *plan, const float *v_dev, float *q_dev, double mu, double mu_reg, double *dq_host,
                              float *q_raw_dev);
/* host only (no GPU, no plan): the route plan creation would decide -- which transform kernels run and which fusions ride on
 * them -- from the function plan creation calls.  lp: the plan's plane pitch (owned planes rounded up to 128).  switches: bit i
 * set = switch i is on, in the order SURFH_DFT_H2, SURFH_DFT_CT, SURFH_DFT_DENSE, SURFH_NO_FUSED_MIX, SURFH_ADJ_FUSED,
 * SURFH_OTF_PROD, SURFH_OTF_SUPPORT, SURFH_OTF_RANGES (the defaults: 0xF3).  scan: what the scan of the OTF found, 0 nothing to
 * drop, 1 support lists, 2 lists and k-ranges (ignored where the route does not scan).
 * out = { kernel along alpha, along beta (0 dense, 1 dft_h2, 2 dft_ct), mix in the forward's loader, OTF product in the inverse
 * loader, fused adjoint tail, OTF support in use (0, 1, 2), spectral template tail, spectral-domain calls available }.
 * surfh_debug_dims(plan, "route") / (plan, "route2") report the first / last four of the route a plan holds.              */
int surfh_route_decide(int32_t n_alpha, int32_t n_beta, int32_t n_templates, int64_t lp, int32_t verify, int32_t exact,
                       int32_t has_sotf, uint32_t switches, int32_t scan, int64_t out[8]);
/* host only: the device allocator's process-wide counters.  live = allocations made and not yet freed, total = allocations
 * asked for so far -- every device allocation of the library goes through one function, so "no leak" is live == what it was. */
void surfh_debug_alloc_count(int64_t *live, int64_t *total);
/* host only: the nth allocation from now on (1-based) is refused once with an out-of-memory error -- it counts in total, the
 * device is not asked -- and the trigger disarms itself; 0 disarms it.  A refused allocation is an ordinary error return. */
void surfh_debug_alloc_fail(int64_t nth);
/* host only (no GPU): the 2x2 step solve every 3MG solver shares, step = (s0, s1) with [[dBd, dBm], [dBm, mBm]] step = [dg, mg];
 * (0, 0) without curvature along d (dBd <= 0 or NaN), (dg / dBd, 0) without a memory direction (mBm <= 0) or when the scaled
 * system is singular (1 - dBm^2 / (dBd mBm) <= 1e-12) */
int surfh_mm_step2(double dBd, double dBm, double mBm, double dg, double mg, double step[2]);

/* ---- masked linear mixing model (MixingST, surfh/Models/mixing.py:276-337; kernels c_fast_forward_TST,
 * c_fast_adjoint_TST, c_precompute_TST of surfh/ToolsDir/cythons_files.pyx:370-463) ----
 * voxels: [n_voxels][3] (lambda, i, j) as `fast_selection_arr`; S: [Lc][Na][Nb] float mask for fwadj's TST
 * (ones with zeros at `selection_arr`, mixing.py:320-321) or NULL.  templates are cast to float32 like the reference. */
typedef struct surfh_tst surfh_tst;
int surfh_tst_create(int32_t n_alpha, int32_t n_beta, int32_t n_lambda, int32_t n_templates, const double *templates,
                     const int32_t *voxels, int64_t n_voxels, const float *S, int32_t device, surfh_tst **out);
int surfh_tst_destroy(surfh_tst *t);
int surfh_tst_forward(surfh_tst *t, const float *maps, float *cube);     /* mixing.py:301-306 */
int surfh_tst_adjoint(surfh_tst *t, const float *cube, float *maps);     /* mixing.py:308-313 */
int surfh_tst_fwadj(surfh_tst *t, const float *maps, float *out);        /* mixing.py:316-317 */
const char *surfh_tst_last_error(void);

/* ---- exponential modified-Shepard resampling (surfh/ToolsDir/shepard_interpolation.pyx:78-141), the resampling step of
 * the slit distortion correction (surfh/Preprocessing/distorsion_correction.py:108-178) ----
 * n_seg independent segments (e.g. the slits of one or several exposures) in one call.  Segment s owns the samples
 * [pt_off[s], pt_off[s+1]) of pt_alpha / pt_lambda / pt_value and an n_lambda[s] x n_alpha[s] block of query points,
 * whose outputs are consecutive in `out` (row-major, segment after segment).  separable != 0: q_alpha holds the
 * concatenated per-segment alpha axes (n_alpha[s] each) and q_lambda the concatenated lambda axes (n_lambda[s] each);
 * separable == 0: q_alpha / q_lambda hold one coordinate pair per query point, in the layout of `out`.
 * Per pair:  d = sqrtf(((a_k - a_g) inv_alpha_res[s])^2 + ((l_k - l_g) inv_lambda_res[s])^2) + epsilon, included when
 * d <= pixel_cutoff with weight exp(-alpha d^p); out = sum w v / sum w (0 without any neighbour), the reference's
 * float32 arithmetic.  neighbours (optional): number of included samples per query point.
 * pt_off / n_alpha / n_lambda / inv_*_res are host arrays; the others are device pointers if device_ptrs != 0 (work on
 * `stream`), host arrays otherwise.  kernel_ms (optional): device time from the first kernel to the last.
 * Returns 0, or non-zero with the message in surfh_shepard_last_error().                                             */
int surfh_shepard(int32_t n_seg, const int64_t *pt_off, const float *pt_alpha, const float *pt_lambda,
                  const float *pt_value, const int32_t *n_alpha, const int32_t *n_lambda, int32_t separable,
                  const float *q_alpha, const float *q_lambda, const float *inv_alpha_res, const float *inv_lambda_res,
                  float p, float alpha, float pixel_cutoff, float epsilon, float *out, int32_t *neighbours,
                  int32_t device_ptrs, void *stream, float *kernel_ms);
const char *surfh_shepard_last_error(void);

/* ---- spectral templates (the reference's template notebooks: scipy.ndimage.median_filter(cube, size, axes=[0]) and
 * sklearn.decomposition.NMF(solver="cd", beta_loss="frobenius", shuffle=False), sklearn 1.7) ----
 * surfh_spectral_median: dst = the median along axis 0 of the C-order host array src [L][C], size 1..63, mode 0 reflect,
 * 1 nearest, 2 mirror.  The window and rank are scipy's (origin 0, rank size / 2), for any size, also size > L.
 * surfh_nmf_cd: n_models coordinate-descent NMF models of one host X [P][L], run together.  Model m has K[m] components;
 * W holds the models' [P][K[m]] blocks one after the other, H their [K[m]][L] blocks; both are the initial values on
 * entry and the results on return.  max_iter >= 1 iterations at most; model m stops after the iteration at which its
 * violation / violation of iteration 1 <= tol (or that is 0), n_iter[m] being that iteration.  Optional outputs:
 * violation_trace [n_models][max_iter] (0 past n_iter), recon_err[m] = ||X - W H||_F and mre[m] = the mean over all
 * entries of (X - W H) / X, 0 where X == 0 (both float64), ms_per_iter = device time per queued iteration.
 * Results are deterministic and do not depend on which other models share the call.
 * Both return 0, or non-zero with the message in surfh_templates_last_error().                                       */
int surfh_spectral_median(const float *src, float *dst, int64_t L, int64_t C, int32_t size, int32_t mode,
                          int32_t device);
int surfh_nmf_cd(const float *X, int64_t P, int64_t L, int32_t n_models, const int32_t *K, float *W, float *H,
                 int32_t max_iter, double tol, int32_t *n_iter, double *violation_trace, double *recon_err, double *mre,
                 int32_t device, float *ms_per_iter);
const char *surfh_templates_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SURFH_AMD_H */
