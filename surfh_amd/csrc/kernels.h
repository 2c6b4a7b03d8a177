// Device kernels of the surfh hot path other than the dense GEMM (see gemm_f32.h).
#pragma once
// templates (abundance maps) the spectral-mix kernels hold in registers per frequency bin
constexpr int SURFH_MAX_TEMPLATES = 8;
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- launch geometry of the capped-grid kernels ------------------------------------------------------
// The streaming kernels below launch at most `cap` blocks of VEC_TPB threads and cover the rest of their vector with a
// grid-stride loop.  The launchers and the host-only hook surfh_launch_geometry (plan_diag.hip) call the same functions.
constexpr int VEC_TPB = 256;
constexpr int DOT_BLOCKS = 512;       // dot_partial, cg_step, cg_step_parts: as many float64 partials, summed by the consumer
constexpr int HUBER_BLOCKS = 256;     // huber_grad, huber_curv (maps): [3][256] partials fit the plan's 1024-double scratch
int nblocks(long n, int cap = 2048);                  // cg_kernels.hip
unsigned rob_grid(long n, int V);                     // robust_data.hip: V floats per thread and trip
unsigned grid_for(long n, long cap = 4096);           // posterior.hip
unsigned nn_project_grid(long n, int vec);            // nonneg.hip: vec = the 16-byte path
dim3 march_grid(int Lc, int na, int nb);              // huber_vox.hip: (pixel tiles, wavelength chunks)

// ---- mix_kernels.hip ----
// ---- spectral mix x OTF (T and C fused in the Fourier domain) -------------------------------
// forward : spec[k][l] = sotf[k][l] * sum_t tpl[t,l] * mhat[t][k]   (spectroModel.py:161,166; mixing.py:232-245)
// adjoint : madj[t][k] = sum_l tpl[t,l] * conj(sotf[k][l]) * spec[k][l] (spectroModel.py:178,181; mixing.py:263-266)
// Wavelength is the INNERMOST axis of every large array: spectra are [2 (re,im)][PL][LP] floats,
// PL = KAP*KBP frequency bins, LP = padded number of owned planes (zero padded); mhat is [T][2][PL].
// T == 0 (no LMM): mhat has the spectrum layout and the operation is element-wise.
// ilv = 1: the spectra (sotf, spec, and mhat when T == 0) are interleaved complex [PL][LP][2] instead (plans whose
// transforms run in dft_h2.hip)
int launch_specmix_fwd(hipStream_t s, const float *mhat, const float *sotf, const float *tpl, float *spec,
                       int T, long PL, int LP, int ilv = 0);
// options of the interleaved adjoint reduction (T > 0): `lim` = [2][LP / 128] per chunk of 128 wavelengths the largest k_beta and the
// largest folded k_alpha inside the OTF's support (bins beyond were not written to `spec` and are skipped);  Nb != 0: the output is
// the solver's Parseval-scaled half spectrum (bins that are their own conjugate x out_self, the others x out_pair) with
// prior_mu * |D|^2 * prior_src added (surfh_normal_spec_dev; same arithmetic as the fused tail's reduction, dft_h2.h)
// T == 0 (plane-wise product): prior_src == madj means that `madj` holds, on entry, the spectrum of the vector the normal operator is
// being applied to; the kernel then writes out_self * conj(H) Y + prior_mu * |D|^2 * that (the quadratic prior folded in).
struct SpecmixAdjOpt {
    const int *lim = nullptr;
    int Na = 0;
    long KBP = 0;
    int Nb = 0;
    float out_self = 1.f, out_pair = 1.f;
    const float *prior_src = nullptr;
    float prior_mu = 0.f;
};
int launch_specmix_adj(hipStream_t s, const float *spec, const float *sotf, const float *tpl, float *madj,
                       int T, long PL, int LP, bool f64 = false, int ilv = 0, const SpecmixAdjOpt *opt = nullptr);
// hth[(t,t')][k] = sum_l tpl[t,l] tpl[t',l] |sotf[k][l]|^2   (mixing.py:177-203), full T x T stored
int launch_wct_hessian(hipStream_t s, const float *sotf, const float *tpl, float *hth, int T, long PL, int LP, int ilv = 0);
// out[t][c][k] = sum_t' hth[t][t'][k] in[t'][c][k]            (mixing.py:102-126 with di = dj = 1)
int launch_wct_hess_apply(hipStream_t s, const float *hth, const float *in, float *out, int T, long PL);
// (hth + diag(mu reg)) z = in per frequency bin (reg < 0 marks padding bins); *flag |= 1 on a non-positive pivot
int launch_wct_solve(hipStream_t s, const float *hth, const float *reg, const double *mu, const float *in, float *out, int T,
                     long PL, int *flag);
// linear mixing model, plane-major arrays: cube[l][i] = sum_t tpl[t][l] maps[t][i];  maps[t][i] = sum_l tpl[t][l] cube[l][i]
int launch_lmm_maps2cube(hipStream_t s, const float *maps, const float *tpl, float *cube, int T, int L, long npix);
int launch_lmm_cube2maps(hipStream_t s, const float *cube, const float *tpl, float *maps, int T, int L, long npix);

// ---- gather_kernels.hip ----
// ---- sparse row gather, vectorised over wavelength ----------------------------------------------
// dst[dst_off[r] + l] (+)= sum_{e<cnt[r]} val[r*W+e] * src[col[r*W+e] + l]   for l in [0, nlam)
// One workgroup per (row, 1024-wavelength chunk): the table entries are workgroup-uniform (scalar
// loads), every tap is a contiguous coalesced read.  One table format serves S + box-sum + slit
// window + decimation (forward), its exact transpose, and the reference's interpolating
// gridding_t (adjoint_ref).
struct EllTable {
    int R = 0, W = 0;              // rows, max entries per row
    const int32_t *cnt = nullptr;  // [R]
    const int64_t *col = nullptr;  // [R][W]  source offset (floats) of wavelength 0
    const float *val = nullptr;    // [R][W]
    const int64_t *dst_off = nullptr;  // [R]
    // accumulate mode only, optional: bit j of rmw[r] set = the 1024-wavelength chunk j of row r may already hold another
    // table's contribution and is read-modify-written; clear = the destination is known to be zero, plain store
    const uint32_t *rmw = nullptr;
    // ... or exactly: wavelengths [rng[r].x, rng[r].y) of row r (relative to the window, multiples of 4) were written earlier in
    // this pass and are read-modify-written, all others are plain stores -- the destination then needs NO clearing (takes precedence)
    const int2 *rng = nullptr;
};
// Scatter table with its rows taken SCATTER_G at a time: neighbouring cube pixels receive from almost the same operand
// rows, so a group reads the union of its members' taps once and applies one weight per member (0 where a member does not
// use the tap).  dst < 0 marks a missing member.
constexpr int GATHER_G = 4, SCATTER_G = 8, GROUP_MAX = 8;      // rows per group: gather / scatter (measured: 4 -> 8 rows costs the
                                                                // gather 0.34 -> 0.45 ms and gains the scatter 0.32 -> 0.28 ms per step on config 3; scatter with 16: 0.31)
struct GroupTable {
    int NG = 0, W = 0, G = 0;          // groups, max union taps per group, rows per group (GATHER_G or SCATTER_G)
    const int32_t *cnt = nullptr;      // [NG]
    const int64_t *col = nullptr;      // [NG][W]
    const float *val = nullptr;        // [NG][W][G]
    const int64_t *dst = nullptr;      // [NG][G]
    const uint32_t *rmw = nullptr;     // [NG][G] read-modify-write chunk masks (as EllTable::rmw)
    const int2 *rng = nullptr;         // [NG][G] exact read-modify-write wavelength ranges (as EllTable::rng)
};
int launch_spmm_rows(hipStream_t s, const EllTable &t, const float *src, float *dst, int nlam, int accumulate);
// float64-accumulating twin of launch_spmm_rows (every row, read-modify-write where `accumulate`)
int launch_spmm_rows_f64acc(hipStream_t s, const EllTable &t, const float *src, float *dst, int nlam, int accumulate);
int launch_spmm_group_scatter(hipStream_t s, const GroupTable &t, const float *src, float *dst, int nlam);
// the gather writing its [NP][K] output as two fp16 pieces dst16[q*plane + ...] of value / block scale; one power-of-two
// scale per workgroup, i.e. per (row, segment) with segment = (column / LinP) * nchunk + (column % LinP) / 1024, nchunk =
// ceil(LinP / 1024): bscale[segment][NP] (entries of segments the table never writes must be 1)
int launch_spmm_rows_f16(hipStream_t s, const EllTable &t, const float *src, unsigned short *dst16, long plane, int nlam, float *bscale,
                         int NP, long K, int LinP);
// the gather of launch_spmm_rows_f16 on a grouped table (members = rows neighbouring in cube-location order)
int launch_spmm_group_gather_f16(hipStream_t s, const GroupTable &t, const float *src, unsigned short *dst16, long plane, int nlam,
                                 float *bscale, int NP, long K, int LinP);
int launch_dequant_f16x2(hipStream_t s, const unsigned short *src16, long plane, const float *bscale, float *dst, int NP, long K, int LinP,
                         int nchunk);
// [L][Na][Nb] (wavelength-major, the reference's cube layout) <-> [NBP][NAP][LP] (wavelength innermost)
int launch_cube_to_lam_inner(hipStream_t s, const float *src, float *dst, int l0, int L, int na, int nb, int nap, int LP);
int launch_cube_from_lam_inner(hipStream_t s, const float *src, float *dst, int l0, int L, int na, int nb, int nap, int LP);
// ---- layout helpers -----------------------------------------------------------------------
int launch_pad_planes(hipStream_t s, const float *src, float *dst, int B, int na, int nb, int nap, int nbp);
int launch_unpad_planes(hipStream_t s, const float *src, float *dst, int B, int na, int nb, int nap, int nbp);
// y[(ps*Ldet + l)*aout + a] = sum_k cpart[k][(ps*aout + a)*LdetP + l]
int launch_y_from_cpart(hipStream_t s, const float *cpart, long slab, int nsplit, float *y, int PS, int Ldet,
                        int aout, int LdetP);
long ymat_from_y_waves(int PS, int Ldet, int aout);
// ymat[(ps*aout + a)*LdetP + l] = y[(ps*Ldet + l)*aout + a]
int launch_ymat_from_y(hipStream_t s, const float *y, float *ymat, int PS, int Ldet, int aout, int LdetP, unsigned *pmax = nullptr,
                       unsigned *rowmax = nullptr, int NP = 0);
// normal operator: sum of the forward GEMM's K slabs straight into the adjoint GEMM's operand -- the two fp16 pieces of
// ymat [NP][LdetP] (rows >= nrows and columns >= Ldet zero) with one power-of-two scale per row, rowmax[NP] = max |row| as
// bit patterns.  The same bits as y_from_cpart + ymat_from_y + launch_split_rows2h, without materialising y.
int launch_ymat16_from_cpart(hipStream_t s, const float *cpart, long slab, int nsplit, unsigned short *dst16, long plane, unsigned *rowmax,
                             int NP, int nrows, int Ldet, int LdetP);
// the same with the data weights of the row, wmat [NP][LdetP] in ymat's layout (zero in the padding), multiplied into the slab sum
// before the row maximum is taken: the bits of y_from_cpart + launch_weight_mul + ymat_from_y + launch_split_rows2h
int launch_ymat16w_from_cpart(hipStream_t s, const float *cpart, long slab, int nsplit, unsigned short *dst16, long plane, unsigned *rowmax,
                              int NP, int nrows, int Ldet, int LdetP, const float *wmat);
// data weights: y *= w;  out = (w > 0 ? w y : 0), a select so that a masked NaN stays out;  *count += weights that are negative or
// not finite (count is cleared by the caller)
int launch_weight_mul(hipStream_t s, float *y, const float *w, long n);
int launch_weight_select(hipStream_t s, const float *y, const float *w, float *out, long n);
int launch_weight_count_bad(hipStream_t s, const float *w, long n, unsigned *count);

// ---- cg_kernels.hip ----
// half spectra [planes][KAP][KBP] <-> the spectral-domain solver's Parseval-scaled form; the quadratic prior on such vectors
int launch_spec_scale(hipStream_t s, const float *src, float *dst, int planes, long PL, long KBP, int Nb, float f_self, float f_pair);
int launch_spec_prior_add(hipStream_t s, const float *d, float *q, int planes, int Na, int Nb, long PL, long KBP, float mu_reg);
int launch_fill_zero(hipStream_t s, float *p, long n);
// ---- CG vector kernels (qmm.lcg loop body; fusion_CT.py:16-43 priors) --------------------------
// q += mu_reg * (Dr^T Dr + Dc^T Dc) d   on [T][na][nb], circular
int launch_prior_add(hipStream_t s, const float *d, float *q, int T, int na, int nb, float mu_reg);
// q += mu_reg * L^T L d, L = circular 3 x 3 Laplacian (the reference's joint prior, fusion_CT.py:45-62)
int launch_prior_joint_add(hipStream_t s, const float *d, float *q, int T, int na, int nb, float mu_reg);
int launch_scale(hipStream_t s, float *x, long n, float a);
// out[0] = sum a*b (fp64 accumulation); scratch holds >= 1024 doubles
int launch_dot(hipStream_t s, const float *a, const float *b, long n, double *scratch, double *out);
// step = rr / dq[0];  x += step d ; r -= step q ; out_rr = r.r
int launch_cg_step(hipStream_t s, float *x, float *r, const float *d, const float *q, long n, const double *rr,
                   const double *dq, double *scratch, double *out_rr);
// x += step d only (used when the residual is refreshed from scratch)
int launch_cg_xupdate(hipStream_t s, float *x, const float *d, long n, const double *rr, const double *dq);
// d = r + (rr_new/rr_old) d
int launch_cg_dir(hipStream_t s, float *d, const float *r, long n, const double *rr_new, const double *rr_old);
// the CG iteration with device-resident scalars in three launches: per-block partial sums of a dot product (`parts`: room for
// dot_parts_stride() doubles), consumed by the next launch, which sums them itself (reduce_final_kernel's order)
int launch_dot_parts(hipStream_t s, const float *a, const float *b, long n, double *parts);
int launch_cg_step_parts(hipStream_t s, float *x, float *r, const float *d, const float *q, long n, const double *rr, const double *dq_parts,
                         double *dq_out, double *rr_parts);
int launch_cg_dir_parts(hipStream_t s, float *d, const float *r, long n, const double *rr_parts, const double *rr_old, double *rr_out);
int dot_parts_stride();
// r = b - q
int launch_residual(hipStream_t s, float *r, const float *b, const float *q, long n);
// out = a + beta b
int launch_lincomb(hipStream_t s, float *out, const float *a, const float *b, long n, double beta);
// 3MG move: mv = s0 d + s1 m ; x += mv ; m = mv ; qm = s0 qd + s1 qm ; r -= qm (when update_r)
int launch_mmmg_update(hipStream_t s, float *x, float *r, const float *d, float *m, float *qm, const float *qd, long n, double s0,
                       double s1, int update_r);
// CG on independent planes ([nplanes][npix] arrays, per-plane scalars in double arrays of nplanes)
int launch_dot_planes(hipStream_t s, const float *a, const float *b, int nplanes, long npix, double *out);
int launch_cg_step_planes(hipStream_t s, float *x, float *r, const float *d, const float *q, int nplanes, long npix, const double *rr,
                          const double *dq, double *rrn, int update_r);
int launch_cg_dir_planes(hipStream_t s, float *d, const float *r, int nplanes, long npix, const double *rrn, double *rr);
// the plane-wise CG blocks on wavelength-innermost arrays [Nb rows][NAP][LP] (the cube layout; the pn_* kernels): per-wavelength
// scalars are [LP] doubles, `part` a work buffer of pn_part_doubles(LP) doubles
int launch_pn_prior_dot(hipStream_t s, const float *d, float *q, int Na, int Nb, int NAP, long LP, float mu_reg, double *part, double *out);
int launch_pn_dot(hipStream_t s, const float *x, const float *y, int Na, int Nb, int NAP, long LP, double *part, double *out);
int launch_pn_step(hipStream_t s, float *x, float *r, const float *d, const float *q, int Na, int Nb, int NAP, long LP, const double *rr,
                   const double *dq, double *part, double *rrn, int update_r);
int launch_pn_dir(hipStream_t s, float *d, const float *r, int Na, int Nb, int NAP, long LP, const double *rrn, const double *rr);
size_t pn_part_doubles(long LP);
// 3MG per plane: rr = r.r, mqm = m.Qm, d = r - (r.Qm / m.Qm) m ; then the 2x2 step in [d, m] with the carried images
int launch_mmmg_dir_planes(hipStream_t s, float *d, const float *r, const float *m, const float *qm, int nplanes, long npix,
                           double *rr, double *mqm);
int launch_mmmg_step_planes(hipStream_t s, float *x, float *r, const float *d, float *m, float *qm, const float *qd, int nplanes,
                            long npix, const double *mqm, int update_r);

// ---- huber_kernels.hip ----
// Huber priors on the separated circular first differences of [T][na][nb] maps, u_r = x[i-1][j] - x[i][j], u_c = x[i][j-1] - x[i][j]
// (NpDiff_r / NpDiff_c); phi(u) = u^2/2 (|u| <= delta), delta (|u| - delta/2) beyond; w(u) = phi'(u) / u.  Float64 per-block partials
// in `scratch` (>= 768 doubles), summed in a fixed order: the same inputs give the same bits.
// `kind` (here and below; `ks`, `kl` for the cube's in-plane and wavelength families): the potential, 0 Huber as described,
// 1 hyperbolic, 2 Hebert-Leahy (huber_dev.h); the kernels are instantiated per kind, an unknown kind is hipErrorInvalidValue.
// out = src + coef * sum_k D_k^T phi'(D_k x) (out may alias src); sums[0] = out.out, sums[1] = sum_k sum phi(D_k x)
int launch_huber_grad(hipStream_t s, const float *x, const float *src, float *out, int T, int na, int nb, float coef, float delta,
                      int kind, double *scratch, double *sums);
// sums[0..2] = sum_k sum w(D_k x) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2: the prior block of the half-quadratic majorant
int launch_huber_curv(hipStream_t s, const float *x, const float *p0, const float *p1, int T, int na, int nb, float delta,
                      int kind, double *scratch, double *sums);
// 3MG with Huber priors per plane ([nplanes][na][nb] arrays, one workgroup per plane).  `sc` holds HUBER_PLANES_SCALARS arrays of
// nplanes doubles: |g|^2, sum_k sum phi(D_k x), beta, m.Bm, and the prior block c00, c01, c11 of (g, m) under w(D x).
// dir: g = r - mu_reg sum_k D_k^T phi'(D_k x), those scalars (B = Q_D + mu_reg W, Q_D m carried in qm), d = g + beta m
// step: the 2x2 majorant step in [d, m] with qd = Q_D d; a plane without positive curvature keeps still
// `par` holds HUBER_PLANES_PARAMS arrays of nplanes doubles, every plane's own: the coefficient of the prior gradient (dir: -mu_reg
// as fp32) and delta, both fp32 values widened, and reg = mu_reg in float64.  `coupling`: 0 the separated prior, 1 isotropic
// (one potential per pixel on sqrt(u_r^2 + u_c^2), the weights recomputed from a 7-point stencil); chosen on the host.
constexpr int HUBER_PLANES_SCALARS = 7;
constexpr int HUBER_PLANES_PARAMS = 3;
int launch_huber_dir_planes(hipStream_t s, const float *x, const float *r, float *g, const float *m, const float *qm, float *d,
                            int nplanes, int na, int nb, const double *par, int kind, int coupling, double *sc);
int launch_huber_step_planes(hipStream_t s, float *x, float *r, const float *d, float *m, float *qm, const float *qd, const float *g,
                             int nplanes, long npix, const double *par, const double *sc, int update_r);
// the two passes of the dir kernel alone: out = src + coef sum_k D_k^T phi'(D_k x) (out may alias src) with sc[0], sc[1] = |out|^2 and
// sum phi per plane; sc[4..6] = the prior block of (p0, p1) per plane
int launch_huber_planes_grad(hipStream_t s, const float *x, const float *src, float *out, int nplanes, int na, int nb, const double *par,
                             int kind, int coupling, double *sc);
int launch_huber_planes_curv(hipStream_t s, const float *x, const float *p0, const float *p1, int nplanes, int na, int nb,
                             const double *par, int kind, int coupling, double *sc);

// ---- coupled_prior.hip ----
// The same prior with one potential per group of differences (coupled_prior.hip; surfh_set_prior_coupling): `coupling` 1 isotropic,
// m = sqrt(u_r^2 + u_c^2) per (t, i, j); 2 vector, m = sqrt(sum_t u_r^2 + u_c^2) per (i, j); anything else is hipErrorInvalidValue.
// w = the weight field w(m) = phi'(m) / m, coupled_weights_floats() floats ([T][na][nb] or [na][nb]); phi_sum[0] = sum phi(m)
size_t coupled_weights_floats(int coupling, int T, int na, int nb);
int launch_coupled_weights(hipStream_t s, const float *x, float *w, int T, int na, int nb, float delta, int kind, int coupling,
                           double *scratch, double *phi_sum);
// out = src + coef * sum_k D_k^T (w D_k x) under the field `w` of x (out may alias src); gg_sum[0] = out.out
int launch_coupled_grad(hipStream_t s, const float *x, const float *w, const float *src, float *out, int T, int na, int nb, float coef,
                        int coupling, double *scratch, double *gg_sum);
// sums[0..2] = sum_k sum w (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2 under the field `w`
int launch_coupled_curv(hipStream_t s, const float *w, const float *p0, const float *p1, int T, int na, int nb, int coupling,
                        double *scratch, double *sums);

// ---- huber_vox.hip ----
// The same potentials on the cube [Lc][na][nb] (huber_vox.hip): the in-plane circular differences under the threshold ds and the
// open wavelength difference u_l = x[l+1] - x[l], l = 0 .. Lc-2, under dl.  `scratch` holds launch_huber_vox_scratch_doubles().
// out = src + cs sum_{k in r,c} D_k^T phi'_ds(D_k x) + cl Dl^T phi'_dl(Dl x) in one pass (out may alias src);
// sums[0] = out.out, sums[1] = sum_{k in r,c} sum phi_ds(D_k x), sums[2] = sum phi_dl(Dl x)
int launch_huber_vox_grad(hipStream_t s, const float *x, const float *src, float *out, int Lc, int na, int nb, float cs, float ds,
                          float cl, float dl, int ks, int kl, double *scratch, double *sums);
// sums[0..2] = sum_{k in r,c} sum w_ds(D_k x) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2;  sums[3..5] = the same under w_dl(Dl x) on Dl
int launch_huber_vox_curv(hipStream_t s, const float *x, const float *p0, const float *p1, int Lc, int na, int nb, float ds, float dl,
                          int ks, int kl, double *scratch, double *sums);
size_t launch_huber_vox_scratch_doubles();

// ---- robust_data.hip ----
// Robust (Huber) data term (robust_data.hip), on flat detector vectors [n]: t = sqrt(w) (y - u), a sample with w <= 0 taken out by
// a select (NaN there stays out); w == nullptr: every weight 1.  `scratch` holds launch_robust_scratch_doubles(); float64 sums in a fixed order.
// v = sqrt(w) phi'(t), omega (may be null) = phi'(t) / t in (0, 1], 0 where masked; sums[0] = sum phi(t), sums[1] = number of |t| > delta
int launch_robust_data(hipStream_t s, const float *y, const float *u, const float *w, float *v, float *omega, long n, float delta,
                       int kind, double *scratch, double *sums);
// sums[0..2] = sum w omega(t) p0^2, p0 p1, p1^2: the data block of the half-quadratic majorant
int launch_robust_curv(hipStream_t s, const float *y, const float *u, const float *w, const float *p0, const float *p1, long n,
                       float delta, int kind, double *scratch, double *sums);
// mv = c0 g + c1 m ; u += mv ; m = mv   (the 3MG move in the basis [g, m]; detector vectors and maps alike)
int launch_robust_move(hipStream_t s, float *u, const float *g, float *m, long n, double c0, double c1);
size_t launch_robust_scratch_doubles();

// ---- posterior.hip: posterior sampling ----
// out[i] = standard normal of (seed, stream, sample, i): Philox4x32-10 on the counter (i / 4, stream, sample), Box-Muller; n any
int launch_randn(hipStream_t s, float *out, long n, uint64_t seed, uint32_t stream, uint32_t sample);
// out = y + eps / sqrt(mu w) where w > 0 (w NULL: 1), the bits of y elsewhere (y NULL: eps / sqrt(mu w), and 0 elsewhere)
int launch_po_data(hipStream_t s, const float *y, const float *w, const float *eps, float *out, long n, float mu);
// out = sqrt_mu_reg (Dr^T er + Dc^T ec) on [T][na][nb], circular
int launch_po_prior(hipStream_t s, const float *er, const float *ec, float *out, int T, int na, int nb, float sqrt_mu_reg);
// b += e
int launch_po_add(hipStream_t s, float *b, const float *e, long n);
// S [po_moment_planes(T)][npix] float64: S1[t] += e_t, S2[t <= u] += e_t e_u, e = x - xhat (xhat NULL: x); then mean = xhat + S1 / K and
// cov [T (T + 1) / 2][npix] = (S2 - S1 S1^T / K) / (K - 1) (NULL: skipped).  1 <= T <= SURFH_MAX_TEMPLATES, else hipErrorInvalidValue.
long po_moment_planes(int T);
int launch_po_moments(hipStream_t s, const float *x, const float *xhat, double *S, int T, long npix);
int launch_po_finish(hipStream_t s, const float *xhat, const double *S, int T, long npix, int K, double *mean, double *cov);
// the plane-wise sampler (surfh_cg_planes_sample), the noise generated in registers: out [L][na][nb] = sqrt_mu_reg (Dr^T eps_r + Dc^T eps_c),
// eps_r / eps_c the streams 1 / 2 of (seed, sample) over the flat index -- launch_randn twice and launch_po_prior(T = L), bit for bit;
// out [n] = eps_y / sqrt(mu w), 0 where w = 0 (w NULL: 1), eps_y the stream 0 -- launch_randn and launch_po_data(y NULL), bit for bit
int launch_po_planes_eta(hipStream_t s, float *out, int L, int na, int nb, float sqrt_mu_reg, uint64_t seed, uint32_t sample);
int launch_po_planes_data(hipStream_t s, const float *w, float *out, long n, float mu, uint64_t seed, uint32_t sample);
// S1 [n] += e, S2 [n] += e e in float64, e = x - xhat (xhat NULL: x); then, in place, S1 <- xhat + S1 / K and (want_var) S2 <- the
// unbiased variance (S2 - S1^2 / K) / (K - 1), clamped at 0
int launch_po_planes_moments(hipStream_t s, const float *x, const float *xhat, double *S1, double *S2, long n);
int launch_po_planes_finish(hipStream_t s, const float *xhat, double *S1, double *S2, long n, int K, int want_var);

// ---- nonneg.hip: non-negative fusion ----
// the ADMM projection / dual update in one pass: z' = max(x + u, 0) (no set sign bit), u' = u + x - z', in place in z and u, and with
// w = rho ((z' - u') - (z - u)) either r += w (r given) or dv = w (dv given; neither: z and u only).  sums[0..3] = |x - z'|^2,
// |z' - z|^2, #{z' == 0}, the new r.r (0 without r): float64 per-block partials in `scratch` (1024 doubles) summed in a fixed order
int launch_nn_project(hipStream_t s, const float *x, float *z, float *u, float *r, float *dv, long n, float rho, double *scratch,
                      double *sums);
// out += c (a - b)   (b NULL: out += c a)
int launch_nn_add(hipStream_t s, float *out, const float *a, const float *b, long n, float c);
// the same pass on L independent planes ([L][npix] vectors, plane-major) with one penalty per plane, rho_l [L] floats on the device,
// in the fused form (r += w): sums [4][L] (device) per plane, from nn_planes_part_doubles(L, npix) partial sums added in a fixed
// order.  The 16-byte path is chosen plane by plane, from the plane's own base pointers.
unsigned nn_planes_split(long npix);                  // blocks per plane of the two plane kernels
size_t nn_planes_part_doubles(int L, long npix);
int launch_nn_project_planes(hipStream_t s, const float *x, float *z, float *u, float *r, int L, long npix, const float *rho_l, double *part,
                             double *sums);
// out_l += (scale c_l) (a_l - b_l) per plane, c_l [L] floats on the device   (b NULL: out_l += (scale c_l) a_l)
int launch_nn_add_planes(hipStream_t s, float *out, const float *a, const float *b, int L, long npix, const float *c_l, float scale);

// ---- imager.hip: the imager data term (include/surfh_amd.h: surfh_set_imager) ----
// G[f][t][2][PL] = sum_l wf[f,l] tpl[t,l] sotf[l,k], accumulated in float64 into acc (same layout; read and written back, cleared
// by the caller before the first launch) over the L planes handed in -- L a multiple of 64, tpl [T][ldt] and wf [F][ldw] zero
// beyond the last plane; sotf: re at sotf[k sk + l sl], im at + im_off.  The sum has one order however the planes are split
// over launches, provided every launch but the last takes a multiple of 32 planes.  g_store: the fp32 copy the mixes read.
int launch_imager_build_g(hipStream_t s, const float *sotf, long sk, long sl, long im_off, const float *tpl, long ldt, const double *wf,
                          long ldw, int L, double *acc, int F, int T, int Na, int nkb, long KBP, long PL);
int launch_imager_g_store(hipStream_t s, const double *acc, float *g, long n);
// src [n][Na][nkb] complex fp32 -> dst [2][KAP][KBP][CH] (wavelength innermost, dst cleared by the caller)
int launch_imager_otf_chunk(hipStream_t s, const float *src, float *dst, int n, int CH, int Na, int nkb, long KBP, long PL);
// zhat[f][k] = sum_t G[f,t,k] xhat[t][k];  ghat[t][k] (+)= scale sum_f conj(G[f,t,k]) yhat[f][k]   (half spectra [B][2][PL])
int launch_imager_mix_fwd(hipStream_t s, const float *g, const float *xhat, float *zhat, int F, int T, long PL);
int launch_imager_mix_adj(hipStream_t s, const float *g, const float *yhat, float *ghat, int F, int T, long PL, float scale, int accumulate);
// padded images z [F][NAP][NBP] (plane pitch PLc) <-> detector y [F][Na / d][Nb / d]: d x d sums, their transpose, and both around
// the weights w (null: 1; w <= 0 takes the sample out) in place
int launch_imager_sample(hipStream_t s, const float *z, float *y, int F, int d, int Na, int Nb, long NBP, long PLc);
int launch_imager_spread(hipStream_t s, const float *y, float *z, int F, int d, int Na, int Nb, long NBP, long PLc);
int launch_imager_window(hipStream_t s, float *z, const float *w, int F, int d, int Na, int Nb, long NBP, long PLc);
// out [T][Na][Nb] (+)= pad [T][NAP][NBP]
int launch_imager_unpad(hipStream_t s, const float *pad, float *out, int T, int Na, int Nb, long NBP, long PLc, int accumulate);
