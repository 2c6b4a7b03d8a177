// Host side of the C ABI (include/surfh_amd.h), the operators: the transform passes, the forward, adjoint and normal pipelines
// on device buffers, and the entry points that only wrap them (surfh_forward* / surfh_adjoint* / surfh_fwadj*, Model_WCT,
// surfh_normal_dev, surfh_prior_add_dev, the spectral-domain operator, the LMM helpers).  They read the plan that plan.hip builds;
// the solvers in plan_solvers.hip call them.  Plan struct and data layout: plan_internal.h.  All device work goes through
// gemm_f32.hip, dft_h2.hip, dft_ct.hip and the *_kernels.hip files on the plan's stream.
#include "plan_internal.h"

namespace surfh_impl {

// q += mu_reg * (the plan's regulariser) d, per image of n_img
int prior_add(surfh_plan *p, hipStream_t st, const float *d, float *q, int n_img, float mu_reg) {
    return p->prior_kind == 1 ? launch_prior_joint_add(st, d, q, n_img, p->Na, p->Nb, mu_reg) : launch_prior_add(st, d, q, n_img, p->Na, p->Nb, mu_reg);
}

namespace {

// fp32-MFMA GEMM, or its float64-accumulating twin in verification mode
int gemm32(surfh_plan *p, hipStream_t st, const GemmArgs &g) { return p->verify ? launch_gemm_f64acc(st, g) : launch_gemm_f32(st, g); }

// ---- plane-major 2-D transforms (only for the T abundance maps) ---------------------------------
// real [B][NAP][NBP] -> spec [B][2][KAP][KBP]   (tmp = ycol_maps viewed as [B][NAP][2*KBP])
int rfft2_planes(surfh_plan *p, const float *src, float *dst, int B) {
    GemmArgs g;
    g.A0 = src; g.lda = p->NBP; g.sA = p->PLc;
    g.B0 = p->Gf; g.ldb = 2 * p->KBP; g.sB = 0;
    g.C = p->ycol_maps; g.ldc = 2 * p->KBP; g.sC = (long)p->NAP * 2 * p->KBP;
    g.M = p->NAP; g.N = 2 * p->KBP; g.K = p->NBP; g.batch = B;
    {
        Prof pr(p, "gemm_dft_rows_fwd_maps");
        LAUNCH_OK(gemm32(p, p->stream, g));
    }
    GemmArgs h;
    h.A0 = p->Ff; h.lda = 2 * p->NAP; h.sA = 0;
    h.B0 = p->ycol_maps; h.B1 = p->ycol_maps + p->KBP; h.ksplitB = p->NAP; h.ldb = 2 * p->KBP;
    h.sB = (long)p->NAP * 2 * p->KBP;
    h.C = dst; h.ldc = p->KBP; h.sC = 2 * p->PL;
    h.M = 2 * p->KAP; h.N = p->KBP; h.K = 2 * p->NAP; h.batch = B;
    {
        Prof pr(p, "gemm_dft_cols_fwd_maps");
        LAUNCH_OK(gemm32(p, p->stream, h));
    }
    return 0;
}

// spec [B][2][KAP][KBP] -> real [B][NAP][NBP]   (tmp = ycol_maps viewed as [B][2][NAP][KBP])
int irfft2_planes(surfh_plan *p, const float *src, float *dst, int B) {
    GemmArgs g;
    g.A0 = p->Fi; g.lda = 2 * p->KAP; g.sA = 0;
    g.B0 = src; g.ldb = p->KBP; g.sB = 2 * p->PL;
    g.C = p->ycol_maps; g.ldc = p->KBP; g.sC = (long)2 * p->NAP * p->KBP;
    g.M = 2 * p->NAP; g.N = p->KBP; g.K = 2 * p->KAP; g.batch = B;
    {
        Prof pr(p, "gemm_dft_cols_inv_maps");
        LAUNCH_OK(gemm32(p, p->stream, g));
    }
    GemmArgs h;
    h.A0 = p->ycol_maps; h.A1 = p->ycol_maps + (long)p->NAP * p->KBP; h.ksplitA = p->KBP; h.lda = p->KBP;
    h.sA = (long)2 * p->NAP * p->KBP;
    h.B0 = p->Gi; h.ldb = p->NBP; h.sB = 0;
    h.C = dst; h.ldc = p->NBP; h.sC = p->PLc;
    h.M = p->NAP; h.N = p->NBP; h.K = 2 * p->KBP; h.batch = B;
    {
        Prof pr(p, "gemm_dft_rows_inv_maps");
        LAUNCH_OK(gemm32(p, p->stream, h));
    }
    return 0;
}

// ---- wavelength-innermost 2-D transforms of the whole owned cube -------------------------------
// cube [NBP][NAP][LP] -> spec [2][KAP][KBP][LP]        (tmp ycol viewed as Z[2][KBP][NAP][LP])
int rfft2_lam(surfh_plan *p, const float *src, float *dst) {
    const long LP = p->LP;
    GemmArgs g;   // Z[(c,kb)][(a,l)] = GfT[(c,kb)][b] * cube[b][(a,l)]
    g.A0 = p->GfT; g.lda = p->NBP;
    g.B0 = src; g.ldb = p->NAP * LP;
    g.C = p->ycol; g.ldc = p->NAP * LP;
    g.M = 2 * p->KBP; g.N = (int)(p->NAP * LP); g.K = p->NBP;
    {
        Prof pr(p, "gemm_dft_rows_fwd");
        LAUNCH_OK(gemm32(p, p->stream, g));
    }
    GemmArgs h;   // per kb: S[(c,ka)][l] = Ff[(c,ka)][(c',a)] * Z[c'][kb][a][l]
    h.A0 = p->Ff; h.lda = 2 * p->NAP;
    h.B0 = p->ycol; h.B1 = p->ycol + (long)p->KBP * p->NAP * LP; h.ksplitB = p->NAP; h.ldb = LP; h.sB = p->NAP * LP;
    h.C = dst; h.ldc = p->KBP * LP; h.sC = LP;
    h.M = 2 * p->KAP; h.N = (int)LP; h.K = 2 * p->NAP; h.batch = p->KBP;
    {
        Prof pr(p, "gemm_dft_cols_fwd");
        LAUNCH_OK(gemm32(p, p->stream, h));
    }
    return 0;
}

// spec [2][KAP][KBP][LP] -> cube [NBP][NAP][LP]        (tmp ycol viewed as Y[2][NAP][KBP][LP])
int irfft2_lam(surfh_plan *p, const float *src, float *dst) {
    const long LP = p->LP;
    GemmArgs g;   // Y[(c,a)][(kb,l)] = Fi[(c,a)][(c',ka)] * S[(c',ka)][(kb,l)]
    g.A0 = p->Fi; g.lda = 2 * p->KAP;
    g.B0 = src; g.ldb = p->KBP * LP;
    g.C = p->ycol; g.ldc = p->KBP * LP;
    g.M = 2 * p->NAP; g.N = (int)(p->KBP * LP); g.K = 2 * p->KAP;
    {
        Prof pr(p, "gemm_dft_cols_inv");
        LAUNCH_OK(gemm32(p, p->stream, g));
    }
    GemmArgs h;   // per a: cube[b][a][l] = GiT[b][(c,kb)] * Y[c][a][kb][l]
    h.A0 = p->GiT; h.lda = 2 * p->KBP;
    h.B0 = p->ycol; h.B1 = p->ycol + (long)p->NAP * p->KBP * LP; h.ksplitB = p->KBP; h.ldb = LP; h.sB = p->KBP * LP;
    h.C = dst; h.ldc = p->NAP * LP; h.sC = LP;
    h.M = p->NBP; h.N = (int)LP; h.K = 2 * p->KBP; h.batch = p->NAP;
    {
        Prof pr(p, "gemm_dft_rows_inv");
        LAUNCH_OK(gemm32(p, p->stream, h));
    }
    return 0;
}

// ---- the 2-D transforms on interleaved complex arrays: a pass along beta and a pass along alpha, each on the kernel of its axis
// (Route::ax_a / ax_b) -- dft_h2 (two-piece fp16, matrices resident in LDS, dft_h2.h) or dft_ct (Cooley-Tukey, N = R M, dft_ct.h).
// One pass function per (kernel, axis, direction); rfft2_cube / irfft2_cube work out what the two passes share and compose them.

// element-wise product formed in the loader of the first inverse pass (dft_ct.h, loader PROD): src * prod (sign +1) or
// src * conj(prod) (-1), times `scale` -- the plane-wise path's OTF product without its own kernel and array
struct ProdOperand {
    const float *prod = nullptr;
    float sign = 1.f, scale = 1.f;
    // + add_w |D|^2 add (loader PRODADD): the quadratic prior's term of the plane-wise normal operator, `add` = the spectrum of
    // the vector the operator is applied to, |D|^2 = the circular first differences' transfer function (fusion_CT.py:16-43)
    const float *add = nullptr;
    float add_w = 0.f;
};

// what a caller asks of cube [NBP][NAP][LP] -> spec [KAP][KBP][LP][2]; the defaults are the plain transform
struct RfftCall {
    bool zero_outside_alpha = false;        // the source is zero outside the alpha range [a_lo, a_hi) (the adjoint's accumulator)
    bool support_only = false;              // only the OTF's support of the spectrum is read afterwards (the adjoint's reductions)
    // fused tail (Route::fused_tail): the pass along alpha does not store the spectrum but multiplies it by conj(sotf) and reduces
    // it over the wavelengths with the template weights straight into tail_out [T][2][KAP][KBP] (spectroModel.py:175-181);
    // tail_scaled: tail_out is the solver's scaled half spectrum (OpCall::T_SPECTRA), its mu and quadratic prior ride on the tail
    float *tail_out = nullptr;
    const OpCall *tail_scaled = nullptr;
};
// what a caller asks of spec [KAP][KBP][LP][2] -> cube [NBP][NAP][LP]
struct IrfftCall {
    const float *mix = nullptr;             // the maps' spectra the loader of the first pass mixes: the plan's mhat, or the solver's scaled half spectra
    const ProdOperand *prod = nullptr;      // ... or the product it forms (Route::prod)
    bool alpha_range_only = false;          // only the cube columns alpha in [a_lo, a_hi) are wanted (the gathers read nothing else)
};
// what the two passes of one transform share
struct PassShare {
    float *mid = nullptr;       // the intermediate: ycol, or ycol_adj / ycol_mix with their parts that are zero for good (plan_internal.h)
    int a0 = 0, na = 0;         // the alpha columns [a0, a0 + na) the pass along beta is batched over
    // planes the dft_h2 passes beside a fusion run over: Leff (plan_internal.h) in front of the fused tail and behind the mix loader,
    // every plane for any other caller.  The tail itself keeps LP: its workgroups take equal counts of super-tiles and only some
    // ranges hold a padded chunk, so passing those tiles over (measured) leaves the slowest workgroup, and the launch, where it was.
    int Lrun = 0;
    bool lists = false;         // the OTF's support applies: super-tiles outside it are neither computed nor stored
    bool ranges = false;        // ... and the k-steps / rows beyond the support of a wavelength chunk are not read / stored (otf_tabs)
};

// r2c along beta, batched over alpha
int h2_rows_fwd(surfh_plan *p, const float *src, const PassShare &s) {
    const long LP = p->LP;
    DftH2Args g;
    g.kind = 1; g.src = src + (long)s.a0 * LP; g.ldb = p->NAP * LP; g.sB = LP; g.Kn = p->Nb;
    g.dst = s.mid + 2 * (long)s.a0 * LP; g.ldc = 2 * p->NAP * LP; g.sC = 2 * LP; g.e[0] = 1.f; g.e[3] = -1.f; g.rvalid = p->Nb / 2 + 1;
    g.KP = p->KPb; g.N = s.Lrun; g.batch = s.na;
    if (s.ranges) { g.rtab = p->otf_tabs + 2 * (LP / 128); g.tabLP = (int)LP; }
    Prof pr(p, "dft_h2_rows_fwd");
    LAUNCH_OK(launch_dft_h2(p->stream, g, p->h2img + 2 * DFT_H2_IMAGE_HALFS, p->h2kA[2]));
    return 0;
}
// c2c along alpha, batched over k_beta -- or the fused tail in its place
int h2_cols_fwd(surfh_plan *p, float *dst, const PassShare &s, const RfftCall &c) {
    const long LP = p->LP;
    DftH2Args h;
    h.kind = 0; h.src = s.mid; h.ldb = 2 * LP; h.sB = 2 * p->NAP * LP; h.Kn = p->Na;
    h.dst = dst; h.ldc = 2 * p->KBP * LP; h.sC = 2 * LP; h.Rn = p->Na; h.rvalid = p->Na / 2 + 1;
    h.KP = p->KPa; h.N = (int)LP; h.batch = p->Nb / 2 + 1;
    h.e[0] = 1.f; h.e[1] = 1.f; h.e[2] = 1.f; h.e[3] = -1.f;                 // Re Z[r] = C ae + S bo, Re Z[N-r] = C ae - S bo
    h.e_alt[0] = 1.f; h.e_alt[1] = -1.f; h.e_alt[2] = 1.f; h.e_alt[3] = 1.f;  // Im Z[r] = C be - S ao, Im Z[N-r] = C be + S ao
    if (!c.tail_out) {
        Prof pr(p, "dft_h2_cols_fwd");
        LAUNCH_OK(launch_dft_h2(p->stream, h, p->h2img, p->h2kA[0]));
        return 0;
    }
    DftH2AdjMix am;
    am.hsrc = p->sotf; am.ldh = 2 * p->KBP * LP; am.sH = 2 * LP; am.tpl = p->tpl; am.T = p->T; am.LPt = (int)LP; am.mpart = p->adjmix_part;
    if (s.lists) { am.vlist = p->otf_vlist; am.kbstart = p->otf_kbstart; am.nvalid = p->otf_nvalid; }
    if (s.na < p->Na) {      // rows alpha < a_lo and alpha >= a_hi of the intermediate are zero: leading k-steps (rows k, Na - k) without a non-zero row
        int kt0 = 0;
        while (16 * kt0 + 15 < p->a_lo && p->Na - (16 * kt0 + 15) >= p->a_hi && h.KP / 16 - (kt0 + 1) >= 5) ++kt0;
        am.kt0 = kt0;
    }
    if (c.tail_scaled) {
        am.out_self = (float)c.tail_scaled->mu; am.out_pair = (float)c.tail_scaled->mu * 1.41421356237309505f; am.Nb = p->Nb;
        am.prior_src = c.tail_scaled->prior_src; am.prior_mu = (float)c.tail_scaled->prior_mu;
    }
    Prof pr(p, "dft_h2_cols_fwd_adjmix");
    LAUNCH_OK(launch_dft_h2_adjmix(p->stream, h, am, c.tail_out, p->PL, p->KBP, p->h2img, p->h2kA[0]));
    return 0;
}
// c2c along alpha (optionally with the spectral mix formed in the loader)
int h2_cols_inv(surfh_plan *p, const float *src, const PassShare &s, const IrfftCall &c) {
    const long LP = p->LP;
    const int hb = p->Nb / 2 + 1;
    DftH2Args g;
    g.kind = 0; g.src = src; g.ldb = 2 * p->KBP * LP; g.Kn = p->Na;
    g.dst = s.mid; g.ldc = 2 * p->KBP * LP; g.Rn = p->Na; g.rvalid = p->Na / 2 + 1;
    g.KP = p->KPa; g.N = (int)(hb * LP);
    g.e[0] = 1.f; g.e[1] = -1.f; g.e[2] = 1.f; g.e[3] = 1.f;
    g.e_alt[0] = 1.f; g.e_alt[1] = 1.f; g.e_alt[2] = 1.f; g.e_alt[3] = -1.f;
    if (c.mix) { g.mhat = c.mix; g.tpl = p->tpl; g.T = p->T; g.LP = (int)p->LP; g.PL = p->PL; g.KBP = p->KBP; }
    if (c.mix && c.mix != p->mhat) { g.mhat_self = 1.f; g.mhat_pair = 0.70710678118654752f; g.mix_Nb = p->Nb; }
    if (s.lists) { g.vlist = p->otf_vlist; g.nvalid = p->otf_nvalid; }
    if (s.ranges) { g.ktab = p->otf_tabs; g.tabLP = (int)LP; }          // k_alpha beyond the support: not read
    // the pass keeps its super-tiles of 128 planes of one k_beta (one mix table per super-tile): tiles beyond Lrun are padding
    if (s.Lrun < LP) { g.Nv = s.Lrun; g.NvP = (int)LP; }
    Prof pr(p, c.mix ? "dft_h2_cols_inv_mix" : "dft_h2_cols_inv");
    LAUNCH_OK(launch_dft_h2(p->stream, g, p->h2img, p->h2kA[0]));
    return 0;
}
// c2r along beta, batched over alpha: cube[b] = Gc Yr - Gs Yi, cube[N-b] = Gc Yr + Gs Yi
int h2_rows_inv(surfh_plan *p, float *dst, const PassShare &s) {
    const long LP = p->LP;
    DftH2Args h;
    h.kind = 2; h.src = s.mid + (long)s.a0 * 2 * p->KBP * LP; h.ldb = 2 * LP; h.sB = 2 * p->KBP * LP;
    h.dst = dst + (long)s.a0 * LP; h.ldc = p->NAP * LP; h.sC = LP;
    h.e[0] = 1.f; h.e[1] = -1.f; h.e[2] = 1.f; h.e[3] = 1.f; h.Rn = p->Nb; h.rvalid = p->Nb / 2 + 1;
    h.KP = p->KPb; h.N = s.Lrun; h.batch = s.na;
    if (s.ranges) { h.ktab = p->otf_tabs + LP / 128; h.tabLP = (int)LP; }   // k_beta beyond the support: zero in ycol_mix
    Prof pr(p, "dft_h2_rows_inv");
    LAUNCH_OK(launch_dft_h2(p->stream, h, p->h2img + DFT_H2_IMAGE_HALFS, p->h2kA[1]));
    return 0;
}

// r2c along beta: neighbouring wavelengths as packed pairs a + i b, separated in the epilogue
int ct_rows_fwd(surfh_plan *p, const float *src, const PassShare &s) {
    const long LP = p->LP;
    DftCtArgs g;
    g.R = p->ctB->R; g.M = p->ctB->M; g.loader = DFT_CT_PLAIN; g.epi = DFT_CT_HSEP; g.sgn = -1.f;
    g.scale = (float)(0.5 / std::sqrt((double)p->Nb));
    g.src = src + (long)s.a0 * LP; g.ldb = p->NAP * LP;
    g.dst = s.mid + 2 * (long)s.a0 * LP; g.ldc = 2 * p->NAP * LP;
    g.ncols = (int)(s.na * LP / 2); g.batch = 1;
    // the reduction reads no k_beta beyond the support of a wavelength chunk: those rows are not stored (chunks of 64 packed pairs)
    if (s.ranges) { g.rtab = p->otf_tabs + 2 * (LP / 128); g.tabLP = (int)(LP / 2); g.tabShift = 6; }
    Prof pr(p, "dft_ct_rows_fwd");
    LAUNCH_OK(launch_dft_ct(p->stream, g, *p->ctB));
    return 0;
}
// c2c along alpha, batched over k_beta
int ct_cols_fwd(surfh_plan *p, float *dst, const PassShare &s) {
    const long LP = p->LP;
    DftCtArgs h;
    h.R = p->ctA.R; h.M = p->ctA.M; h.loader = DFT_CT_PLAIN; h.epi = DFT_CT_STORE; h.sgn = -1.f;
    h.scale = (float)(1.0 / std::sqrt((double)p->Na));
    h.src = s.mid; h.ldb = 2 * LP; h.sB = 2 * p->NAP * LP;
    h.dst = dst; h.ldc = 2 * p->KBP * LP; h.sC = 2 * LP;
    h.ncols = (int)LP; h.batch = p->Nb / 2 + 1;
    // only the (k_beta, wavelength chunk) super-tiles and the rows k_alpha inside the OTF's support
    if (s.lists) { h.vlist = p->otf_vlist; h.nvalid = p->otf_nvalid; }
    if (s.ranges) { h.rtab = p->otf_tabs + 3 * (LP / 128); h.tabLP = (int)LP; }
    Prof pr(p, "dft_ct_cols_fwd");
    LAUNCH_OK(launch_dft_ct(p->stream, h, p->ctA));
    return 0;
}
// c2c along alpha (optionally with the spectral mix, or the product, formed in the loader)
int ct_cols_inv(surfh_plan *p, const float *src, const PassShare &s, const IrfftCall &c) {
    const long LP = p->LP;
    DftCtArgs g;
    g.R = p->ctA.R; g.M = p->ctA.M; g.loader = c.mix ? DFT_CT_MIX : DFT_CT_PLAIN; g.epi = DFT_CT_STORE; g.sgn = 1.f;
    g.scale = (float)(1.0 / std::sqrt((double)p->Na));
    g.src = src; g.ldb = 2 * p->KBP * LP;
    g.dst = s.mid; g.ldc = 2 * p->KBP * LP;
    g.ncols = (int)((p->Nb / 2 + 1) * LP); g.batch = 1;
    if (c.mix) { g.mhat = c.mix; g.tpl = p->tpl; g.T = p->T; g.LP = (int)p->LP; g.PL = p->PL; g.KBP = p->KBP; }
    if (c.mix && c.mix != p->mhat) { g.mhat_self = 1.f; g.mhat_pair = 0.70710678118654752f; g.mix_Nb = p->Nb; }
    if (c.prod && c.prod->prod && !c.mix) {
        g.loader = DFT_CT_PROD; g.prod = c.prod->prod; g.ldp = g.ldb; g.sP = 0; g.prod_sign = c.prod->sign; g.scale *= c.prod->scale;
        if (c.prod->add && c.prod->add_w != 0.f) {
            g.loader = DFT_CT_PRODADD; g.add = c.prod->add; g.add_w = c.prod->add_w; g.add_Nb = p->Nb; g.LP = (int)p->LP;
        }
    }
    if (s.lists) { g.vlist = p->otf_vlist; g.nvalid = p->otf_nvalid; }
    if (s.ranges) { g.ktab = p->otf_tabs; g.tabLP = (int)LP; }
    Prof pr(p, c.mix ? "dft_ct_cols_inv_mix" : (g.loader == DFT_CT_PROD ? "dft_ct_cols_inv_prod" : g.loader == DFT_CT_PRODADD ? "dft_ct_cols_inv_prodadd" : "dft_ct_cols_inv"));
    LAUNCH_OK(launch_dft_ct(p->stream, g, p->ctA));
    return 0;
}
// c2r along beta, batched over alpha: two neighbouring half spectra as one Hermitian-extended complex sequence
int ct_rows_inv(surfh_plan *p, float *dst, const PassShare &s) {
    const long LP = p->LP;
    DftCtArgs h;
    h.R = p->ctB->R; h.M = p->ctB->M; h.loader = DFT_CT_HPACK; h.epi = DFT_CT_STORE; h.sgn = 1.f;
    h.scale = (float)(1.0 / std::sqrt((double)p->Nb));
    h.src = s.mid + (long)s.a0 * 2 * p->KBP * LP; h.ldb = 2 * LP; h.sB = 2 * p->KBP * LP;
    h.dst = dst + (long)s.a0 * LP; h.ldc = p->NAP * LP; h.sC = LP;
    h.ncols = (int)(LP / 2); h.batch = s.na;
    if (s.ranges) { h.ktab = p->otf_tabs + LP / 128; h.tabLP = (int)(LP / 2); h.tabShift = 6; }      // k_beta beyond the support: zero in ycol_mix
    Prof pr(p, "dft_ct_rows_inv");
    LAUNCH_OK(launch_dft_ct(p->stream, h, *p->ctB));
    return 0;
}

// ---- pipelines on device buffers ----------------------------------------------------------------
// cube [NBP][NAP][LP] -> the plan's spectrum layout: along beta, then along alpha
int rfft2_cube(surfh_plan *p, const float *src, float *dst, const RfftCall &c = {}) {
    const Route &r = p->route;
    if (!r.interleaved()) return rfft2_lam(p, src, dst);
    const bool sub = c.zero_outside_alpha && p->a_hi - p->a_lo < p->Na;       // the range is a proper one: ycol_adj exists
    PassShare s;
    s.mid = sub ? p->ycol_adj : p->ycol;
    s.a0 = sub ? p->a_lo : 0; s.na = sub ? p->a_hi - p->a_lo : p->Na;
    s.Lrun = c.tail_out ? p->Leff : (int)p->LP;
    s.lists = c.support_only && r.support != OTF_NONE;
    s.ranges = c.support_only && r.support == OTF_LISTS_RANGES;
    if (r.ax_b == AX_H2 ? h2_rows_fwd(p, src, s) : ct_rows_fwd(p, src, s)) return 1;
    return r.ax_a == AX_H2 ? h2_cols_fwd(p, dst, s, c) : ct_cols_fwd(p, dst, s);
}
// the plan's spectrum layout -> cube [NBP][NAP][LP]: along alpha, then along beta
int irfft2_cube(surfh_plan *p, const float *src, float *dst, const IrfftCall &c = {}) {
    const Route &r = p->route;
    if (c.prod && r.ax_a != AX_CT) return fail("irfft2: the product loader needs the Cooley-Tukey pass along alpha");
    if (!r.interleaved()) return irfft2_lam(p, src, dst);
    PassShare s;
    s.lists = c.mix && r.support != OTF_NONE;
    s.ranges = c.mix && r.support == OTF_LISTS_RANGES;
    s.mid = s.lists ? p->ycol_mix : p->ycol;
    s.a0 = c.alpha_range_only ? p->a_lo : 0; s.na = c.alpha_range_only ? p->a_hi - p->a_lo : p->Na;
    s.Lrun = c.mix ? p->Leff : (int)p->LP;
    if (r.ax_a == AX_H2 ? h2_cols_inv(p, src, s, c) : ct_cols_inv(p, src, s, c)) return 1;
    return r.ax_b == AX_H2 ? h2_rows_inv(p, dst, s) : ct_rows_inv(p, dst, s);
}

// mhat[t] = sum_l tpl[t][l] conj(sotf[l]) rfft2(cube[l])  (T > 0), or the per-plane product (T == 0)
// `src`: what the caller knows of the cube (the adjoint's accumulator is zero outside the alpha range of the channels' tables)
// The result goes to mhat, or to the solver's scaled half spectra (c.tail == T_SPECTRA: mu and the quadratic prior folded in).
int adjoint_tail(surfh_plan *p, const float *cube, const OpCall &c = {}, RfftCall src = {}) {
    const Route &r = p->route;
    const bool scaled = c.tail == OpCall::T_SPECTRA;
    float *const out = scaled ? c.spectra_out : p->mhat;
    // the fused tail and the reduction behind a dft_ct pass read the spectrum only inside the OTF's support; the reduction behind
    // two plain dft_h2 passes and the dense one take the transform of the whole cube
    if (r.fused_tail || r.any_ct()) src.support_only = true;
    else src = RfftCall();
    if (r.fused_tail) {
        src.tail_out = out; src.tail_scaled = scaled ? &c : nullptr;
        return rfft2_cube(p, cube, p->spec, src);
    }
    if (rfft2_cube(p, cube, p->spec, src)) return 1;
    if (r.prod) return 0;         // plane-wise: conj(OTF) x spec is formed by the loader of the inverse transform that follows
    SpecmixAdjOpt o;
    o.Na = p->Na; o.KBP = p->KBP;
    Prof pr(p, "specmix_adj");
    if (p->T == 0 && r.interleaved() && c.fold) {
        // plane-wise normal operator: `mhat` still holds the spectrum of the vector the forward half was applied to -- mu and the
        // quadratic prior go into the OTF product, no prior kernel and no scaling pass afterwards
        o.Nb = p->Nb; o.out_self = (float)c.mu; o.prior_src = p->mhat; o.prior_mu = (float)c.prior_mu;
        LAUNCH_OK(launch_specmix_adj(p->stream, p->spec, p->sotf, p->tpl, p->mhat, 0, p->PL, p->LP, false, 1, &o));
        return 0;
    }
    if (!r.any_ct()) {
        LAUNCH_OK(launch_specmix_adj(p->stream, p->spec, p->sotf, p->tpl, p->mhat, p->T, p->PL, p->LP, p->verify, r.interleaved()));
        return 0;
    }
    if (r.support == OTF_LISTS_RANGES) o.lim = p->otf_tabs + 2 * (p->LP / 128);
    if (scaled) {
        o.Nb = p->Nb; o.out_self = (float)c.mu; o.out_pair = (float)c.mu * 1.41421356237309505f;
        o.prior_src = c.prior_src; o.prior_mu = (float)c.prior_mu;
    }
    LAUNCH_OK(launch_specmix_adj(p->stream, p->spec, p->sotf, p->tpl, out, p->T, p->PL, p->LP, false, 1, p->T > 0 ? &o : nullptr));
    return 0;
}

// The template transpose's tail (tplgrad.hip): G [T][Lc] = sum over the frequency bins of conj(mhat_t) conj(sotf) rfft2(cube),
// `cube` the adjoint's accumulator (zero outside the alpha range of the channels' tables), mhat the spectra of the maps.
//   Route::tpl_spectral: the whole half spectrum from the unfused passes without the OTF-support lists -- the fused tail never
//     stores the last pass and the listed passes leave bins outside the support unwritten -- then the reduction over bins;
//   else: the cube-space adjoint through its OTF^T back to pixels, then the reduction over pixels against `maps` (on the device).
int template_tail(surfh_plan *p, const float *cube, float *G, const float *maps) {
    if (p->route.tpl_spectral) {
        RfftCall src;
        src.zero_outside_alpha = true;
        if (rfft2_cube(p, cube, p->spec, src)) return 1;
        Prof pr(p, "tplgrad_spec");
        LAUNCH_OK(launch_tplgrad_spec(p->stream, p->spec, p->sotf, p->mhat, p->tg_part, p->tg_cidx, G, p->T, p->Lc, p->Na, p->Nb, p->KBP,
                                      p->PL, (int)p->LP));
        return 0;
    }
    if (rfft2_cube(p, cube, p->spec)) return 1;
    {
        Prof pr(p, "otf_conj_mul");
        LAUNCH_OK(launch_otf_conj_mul(p->stream, p->spec, p->sotf, p->PL, (int)p->LP, p->route.interleaved()));
    }
    if (irfft2_cube(p, p->spec, p->cube)) return 1;
    Prof pr(p, "tplgrad_pix");
    LAUNCH_OK(launch_tplgrad_pix(p->stream, p->cube, maps, p->tg_part, p->tg_cidx, G, p->T, p->Lc, p->Na, p->Nb, p->NAP, (int)p->LP));
    return 0;
}

}  // namespace

// y = A x, x where call.head says (OpCall, plan_internal.h)
int forward_dev(surfh_plan *p, const float *x, float *y, const OpCall &call) {
    hipStream_t s = p->stream;
    const bool hand_over = call.hand_over;
    if (call.head == OpCall::H_SPECTRA || call.head == OpCall::H_MHAT) {
        // the maps' spectra are the caller's vector, or the template solver has left them in mhat: nothing to transform
    } else if (p->T > 0) {
        if (tpl_maps_spectra(p, x)) return 1;
    } else if (call.head == OpCall::H_CUBE) {
        // plane-wise solver on wavelength-innermost vectors: x is already in the cube's layout [NBP][NAP][LP]
        if (rfft2_cube(p, x, p->mhat)) return 1;
    } else {
        {
            Prof pr(p, "cube_transpose");
            for (auto &g : p->segs)
                LAUNCH_OK(launch_cube_to_lam_inner(s, x, p->cube + g.coff, g.start, g.len, p->Na, p->Nb, p->NAP, p->LP));
        }
        if (rfft2_cube(p, p->cube, p->mhat)) return 1;
    }
    IrfftCall inv;
    if (p->route.mix) {
        // spectral mix x OTF fused into the loader of the first inverse pass: `spec` is never written
        // (the normal operator needs the blurred cube only where a gather reads it)
        inv.mix = call.head == OpCall::H_SPECTRA ? call.spectra_in : p->mhat;
        inv.alpha_range_only = hand_over;
        if (irfft2_cube(p, p->sotf, p->cube, inv)) return 1;
    } else if (p->route.prod) {
        // plane-wise model on the Cooley-Tukey passes: OTF x spectrum in the loader of the first inverse pass, `spec` is never written
        ProdOperand po;
        po.prod = p->sotf;
        inv.prod = &po;
        if (irfft2_cube(p, p->mhat, p->cube, inv)) return 1;
    } else {
        {
            Prof pr(p, "specmix_fwd");
            LAUNCH_OK(launch_specmix_fwd(s, p->mhat, p->sotf, p->tpl, p->spec, p->T, p->PL, p->LP, p->route.interleaved()));
        }
        if (irfft2_cube(p, p->spec, p->cube)) return 1;
    }
    // gather on the main stream, spectral-blur GEMM + slab sum on the second one: GEMM(c) overlaps gather(c+1)
    hipStream_t sB = (p->overlap && p->stream2) ? p->stream2 : s;
    for (auto &c : p->ch) {
        const bool f16 = c.W16 != nullptr;
        {
            Prof pr(p, "spmm_gather_fwd");
            if (c.Xs16 && c.fwd.g.NG)     // straight to the block-scaled fp16 pieces of the all-consumer GEMM
                LAUNCH_OK(launch_spmm_group_gather_f16(s, c.fwd.g, p->cube, c.Xs16, (long)c.NP * c.K, c.nlam, c.bscale, c.NP, c.K, c.LinP));
            else if (c.Xs16)
                LAUNCH_OK(launch_spmm_rows_f16(s, c.fwd.t, p->cube, c.Xs16, (long)c.NP * c.K, c.nlam, c.bscale, c.NP, c.K, c.LinP));
            else if (p->verify)
                LAUNCH_OK(launch_spmm_rows_f64acc(s, c.fwd.t, p->cube, c.Xs, c.nlam, 0));
            else
                LAUNCH_OK(launch_spmm_rows(s, c.fwd.t, p->cube, c.Xs, c.nlam, 0));
        }
        if (c.bsum) {   // y[l][(p,s,a)] = Xs[(p,s,a)][l]
            Prof pr(p, "y_transpose");
            LAUNCH_OK(launch_cube_from_lam_inner(s, c.Xs + c.shift, y + c.yoff, 0, c.Lin, 1, c.P * c.S * c.aout, 1, c.LinP));
            continue;
        }
        if (chain(p, s, sB)) return 1;
        GemmArgs g;   // y^T[n][l'] = sum_k Xs[n][k] W[l'][k]
        g.A0 = c.Xs; g.lda = c.K;
        g.C = c.Cpart; g.ldc = c.LdetP;
        g.M = c.NP; g.N = c.LdetP; g.K = c.K; g.splitK = c.splitK; g.sCsplit = (long)c.NP * c.LdetP;
        {
            Prof pr(p, "gemm_wblur_fwd", sB);
            if (p->wblur_fp32) {
                g.B0 = c.Wt; g.ldb = c.LdetP;        // B as [K][N]
                LAUNCH_OK(gemm32(p, sB, g));
            } else {
                // both operands as fp16 pieces (the gather wrote the block-scaled pieces of Xs): 256 x 256 all-consumer kernel
                g.ldb = c.K;                         // B as [N][K]
                g.B16 = c.W16; g.pB16 = (long)c.LdetP * c.K; g.sB16 = c.sW;
                g.A3 = c.Xs16; g.pA3 = (long)c.NP * c.K;
                g.bscale = c.bscale; g.segLinP = c.LinP; g.segChunks = (c.LinP + 1023) / 1024;
                g.klist = c.klF; g.klistStride = c.klFs;
                LAUNCH_OK(launch_gemm_nt_f16x2_cc(sB, g));
            }
        }
        if (hand_over && c.ymat16 && c.wmat) {          // the normal operator under data weights: mu A^T W A
            Prof pr(p, "ymat16w_from_cpart", sB);
            LAUNCH_OK(launch_ymat16w_from_cpart(sB, c.Cpart, (long)c.NP * c.LdetP, c.splitK, c.ymat16, (long)c.NP * c.LdetP, c.amax, c.NP,
                                                c.P * c.S * c.aout, c.Ldet, c.LdetP, c.wmat));
        } else if (hand_over && c.ymat16) {
            Prof pr(p, "ymat16_from_cpart", sB);
            LAUNCH_OK(launch_ymat16_from_cpart(sB, c.Cpart, (long)c.NP * c.LdetP, c.splitK, c.ymat16, (long)c.NP * c.LdetP, c.amax, c.NP,
                                               c.P * c.S * c.aout, c.Ldet, c.LdetP));
        } else {
            Prof pr(p, "y_from_cpart", sB);
            LAUNCH_OK(launch_y_from_cpart(sB, c.Cpart, (long)c.NP * c.LdetP, c.splitK, y + c.yoff, c.P * c.S, c.Ldet,
                                          c.aout, c.LdetP));
        }
    }
    if (chain(p, sB, s)) return 1;     // everything after this call sees y complete
    return 0;
}

// x = A^T y, x where call.tail says (OpCall, plan_internal.h)
int adjoint_dev(surfh_plan *p, const float *y, float *x, const OpCall &call) {
    hipStream_t s = p->stream;
    const bool ref = call.ref, handed_over = call.hand_over;
    // detector-side work (y -> ymat, R^T GEMM) on the second stream, cube-side scatter on the main one: GEMM(c+1)
    // overlaps scatter(c); the scatters stay in channel order on one stream because their windows overlap
    hipStream_t sB = (p->overlap && p->stream2) ? p->stream2 : s;
    if (chain(p, s, sB)) return 1;     // y (and the previous users of Xs / ymat) are ordered before the second stream's work
    // the exact adjoint accumulates in its own buffer without clearing it (surfh_plan::gcube); the reference adjoint and the
    // verification plan read-modify-write every row of the cleared work cube
    float *const acc = (!ref && p->gcube) ? p->gcube : p->cube;
    if (acc == p->cube) {
        Prof pr(p, "fill_zero");
        LAUNCH_OK(launch_fill_zero(s, p->cube, (long)p->NBP * p->NAP * p->LP));
    }
    // detector side of one channel: y -> ymat (-> its fp16 pieces, unless the forward half has just left them behind)
    auto prepare = [&](Channel &c) -> int {
        const bool f16 = c.W16 != nullptr;
        if (handed_over && f16 && c.ymat16) return 0;
        {
            Prof pr(p, "ymat_from_y", sB);
            LAUNCH_OK(launch_ymat_from_y(sB, y + c.yoff, c.ymat, c.P * c.S, c.Ldet, c.aout, c.LdetP, f16 ? c.pmax : nullptr,
                                         f16 ? c.amax : nullptr, c.NP));
        }
        if (f16 && !p->wblur_fp32)
            LAUNCH_OK(launch_split_rows2h(sB, c.ymat, c.amax, c.ymat16, c.NP, c.LdetP, (long)c.NP * c.LdetP));   // one scale per row
        return 0;
    };
    auto gemm_args = [&](Channel &c) {   // Xs_t[n][k] = sum_l' y^T[n][l'] W[l'][k]
        GemmArgs g;
        g.A0 = c.ymat; g.lda = c.LdetP;
        g.C = c.Xs; g.ldc = c.K;
        g.M = c.NP; g.N = c.K; g.K = c.LdetP;
        if (p->wblur_fp32) {
            g.B0 = c.W; g.ldb = c.K;             // B as [K'=l'][N'=k]
        } else if (c.W16) {
            g.K = (c.Ldet + 31) / 32 * 32;       // the columns of ymat beyond Ldet are zero: whole K steps of them are skipped
            g.ldb = c.LdetP;                     // B as [N'=k][K'=l']
            g.B16 = c.Wt16; g.pB16 = (long)c.LdetP * c.K; g.sB16 = c.sW; g.amax = c.amax;
            g.A3 = c.ymat16; g.pA3 = (long)c.NP * c.LdetP;
            g.klist = c.klA; g.klistStride = c.klAs;
            if (c.klA && c.permA) { g.permP = c.permA; g.permLin = c.LinP; }
        }
        return g;
    };
    // The two-piece fp16 GEMMs of up to four channels go out as ONE launch (each is 1.5-1.8 rounds of workgroups on its own;
    // their operands and outputs are per channel, so nothing orders them among themselves): detector-side preparation of all
    // of them first, the grouped GEMM, then the scatters in channel order.  SURFH_GEMM_GROUPED=0: one launch per channel.
    auto scatter = [&](Channel &c) -> int {      // cube side of one channel: acc (+)= G^T Xs
        Prof pr(p, ref ? "spmm_degrid_ref" : "spmm_scatter_adj");
        if (p->verify)
            LAUNCH_OK(launch_spmm_rows_f64acc(s, ref ? c.adjRef.t : c.adjT.t, c.Xs, acc, c.nlam, 1));
        else if (!ref && c.adjT.g.NG)
            LAUNCH_OK(launch_spmm_group_scatter(s, c.adjT.g, c.Xs, acc, c.nlam));
        else
            LAUNCH_OK(launch_spmm_rows(s, ref ? c.adjRef.t : c.adjT.t, c.Xs, acc, c.nlam, 1));
        return 0;
    };
    std::vector<char> gemm_done(p->ch.size(), 0);
    if (p->gemm_grouped && !p->wblur_fp32 && !p->verify) {
        std::vector<GemmArgs> ga;
        std::vector<size_t> gc;
        for (size_t ci = 0; ci <= p->ch.size(); ++ci) {
            const bool last = ci == p->ch.size();
            if (!last) {
                Channel &c = p->ch[ci];
                if (c.bsum || !c.W16 || (ref && !c.has_ref)) continue;
                if (prepare(c)) return 1;
                ga.push_back(gemm_args(c)); gc.push_back(ci);
            }
            if (!ga.empty() && (last || (int)ga.size() == GEMM_GROUP_MAX)) {
                {
                    Prof pr(p, "gemm_wblur_adj", sB);
                    LAUNCH_OK(launch_gemm_nt_f16x2_cc_group(sB, ga.data(), (int)ga.size()));
                }
                for (size_t i : gc) gemm_done[i] = 1;
                ga.clear(); gc.clear();
            }
        }
    }
    for (size_t ci = 0; ci < p->ch.size(); ++ci) {
        Channel &c = p->ch[ci];
        if (ref && !c.has_ref) return fail("adjoint_ref needs the gridding_t tables (gt_*) in the channel descriptor");
        if (c.bsum) {
            {
                Prof pr(p, "y_transpose");
                LAUNCH_OK(launch_cube_to_lam_inner(s, y + c.yoff, c.Xs + c.shift, 0, c.Lin, 1, c.P * c.S * c.aout, 1, c.LinP));
            }
            if (scatter(c)) return 1;
            continue;
        }
        if (!gemm_done[ci]) {
            if (prepare(c)) return 1;
            const GemmArgs g = gemm_args(c);
            Prof pr(p, "gemm_wblur_adj", sB);
            if (p->wblur_fp32 || !c.W16) LAUNCH_OK(gemm32(p, sB, g));
            else LAUNCH_OK(launch_gemm_nt_f16x2_cc(sB, g));
        }
        if (chain(p, sB, s) || scatter(c)) return 1;
    }
    if (call.tail == OpCall::T_TEMPLATES) return template_tail(p, acc, call.tpl_out, call.tpl_maps);      // the reduction runs over the bins
    RfftCall acc_is;
    acc_is.zero_outside_alpha = true;
    if (adjoint_tail(p, acc, call, acc_is)) return 1;
    if (call.tail == OpCall::T_SPECTRA) return 0;         // the caller's vector is the spectrum
    if (p->T > 0) {
        if (irfft2_planes(p, p->mhat, p->maps_pad, p->T)) return 1;
        Prof pr(p, "unpad_planes");
        LAUNCH_OK(launch_unpad_planes(s, p->maps_pad, x, p->T, p->Na, p->Nb, p->NAP, p->NBP));
        return 0;
    }
    // plane-wise: straight into the caller's wavelength-innermost vector, or through the work cube into the caller's planes
    float *const out = call.tail == OpCall::T_CUBE ? x : p->cube;
    if (p->route.prod) {
        // conj(OTF) x spectrum of the accumulated cube in the loader; inside the plane-wise normal operator mu rides on the pass and
        // the quadratic prior comes in as a third operand: `mhat` still holds the spectrum of the vector the forward half was applied to
        ProdOperand po;
        po.prod = p->sotf; po.sign = -1.f; po.scale = call.fold ? (float)call.mu : 1.f;
        if (call.fold && call.prior_mu != 0.0 && call.mu != 0.0) {      // q = mu (A^T A d + (mu_r / mu) D^T D d)
            po.add = p->mhat; po.add_w = (float)(call.prior_mu / call.mu);
        }
        IrfftCall inv;
        inv.prod = &po;
        if (irfft2_cube(p, p->spec, out, inv)) return 1;
    } else if (irfft2_cube(p, p->mhat, out)) {
        return 1;
    }
    if (out == x) return 0;
    if (p->Lown < p->Lc) LAUNCH_OK(launch_fill_zero(s, x, (long)p->Lc * p->Na * p->Nb));   // planes no channel observes
    Prof pr(p, "cube_transpose");
    for (auto &g : p->segs)
        LAUNCH_OK(launch_cube_from_lam_inner(s, p->cube + g.coff, x, g.start, g.len, p->Na, p->Nb, p->NAP, p->LP));
    return 0;
}

// the normal operator's two halves exchange the GEMM operands directly (SURFH_NORMAL_FUSED=0: through y)
static bool normal_hand_over(const surfh_plan *p) {
    static const bool fused = env_on("SURFH_NORMAL_FUSED", true);
    return fused && !p->verify && !p->wblur_fp32;
}

// A^T W A v, the two halves of every normal operator: y is only the hand-over between them, and the channels' slab sums go
// straight into the adjoint's GEMM operands (SURFH_NORMAL_FUSED=0: through y, as forward() + adjoint() do).  Data weights
// (surfh_set_data_weights) ride on the hand-over: inside launch_ymat16w_from_cpart where y is never written, as one element-wise
// pass over the part of y that is (verify plans, SURFH_WBLUR_FP32, SURFH_NORMAL_FUSED=0, channels without a spectral blur).
int normal_halves(surfh_plan *p, const float *v, float *q, OpCall c) {
    const bool ho = c.hand_over = normal_hand_over(p);
    if (forward_dev(p, v, p->cg_y, c)) return 1;
    if (p->dw) {
        Prof pr(p, "weight_mul");
        for (auto &c : p->ch)
            if (!(ho && !c.bsum && c.ymat16)) LAUNCH_OK(launch_weight_mul(p->stream, p->cg_y + c.yoff, p->dw + c.yoff, c.ysize));
    }
    return adjoint_dev(p, p->cg_y, q, c);
}
// the data of the solvers' right-hand side b = mu A^T W y: y itself without weights, else W y formed once per solve by a select
const float *weighted_data(surfh_plan *p, const float *y) {
    if (!p->dw) return y;
    Prof pr(p, "weight_select");
    if (launch_weight_select(p->stream, y, p->dw, p->dwy, p->osize) != 0) { fail("launch_weight_select failed"); return nullptr; }
    return p->dwy;
}

int normal_dev(surfh_plan *p, const float *d, float *q, double mu, bool cube) {
    OpCall c;
    if (cube) { c.head = OpCall::H_CUBE; c.tail = OpCall::T_CUBE; }
    if (normal_halves(p, d, q, c)) return 1;
    if (mu != 1.0) {
        Prof pr(p, "scale");
        LAUNCH_OK(launch_scale(p->stream, q, cube ? (long)p->NBP * p->NAP * p->LP : p->isize, (float)mu));
    }
    return 0;
}

// explicit per-frequency Hessian of Model_WCT and its work buffer: the launch that fills `hth` is the set's set-up step (a pair
// published without it would make the next call skip the launch)
static int ensure_hessian(surfh_plan *p) {
    return ensure_set_with(
        [&](float *h, float *) {
            const int rc = launch_wct_hessian(p->stream, p->sotf, p->tpl, h, p->T, p->PL, p->LP, p->route.interleaved());
            return rc ? fail("launch_wct_hessian failed: %s", hipGetErrorString((hipError_t)rc)) : 0;
        },
        member(p->hth, (size_t)p->T * p->T * p->PL), member(p->mhat2, (size_t)p->T * 2 * p->PL));
}

int ensure_cg(surfh_plan *p) {
    // room for the vectors in either basis: the maps [T][Na][Nb] or their scaled half spectra [T][2][KAP][KBP]
    const size_t n = std::max((size_t)p->isize, (size_t)2 * std::max(p->T, 0) * (size_t)p->PL);
    return ensure_set(member(p->cg_x, n), member(p->cg_r, n), member(p->cg_d, n), member(p->cg_q, n), member(p->cg_b, n));
}

// ---- template refinement: the operator as a function of the templates, maps held fixed (kernels: tplgrad.hip) ----
int tpl_ensure(surfh_plan *p) {
    if (p->T < 1) return fail("template calls need a plan with templates");
    if (p->T > SURFH_MAX_TEMPLATES) return fail("template calls take at most %d templates (the plan has %d)", SURFH_MAX_TEMPLATES, p->T);
    if (p->ch.empty()) return fail("plan has no channel");
    if (p->tg_part) return 0;
    std::vector<int> cidx((size_t)p->Lc, -1), pidx((size_t)p->LP, -1);
    for (int c = 0; c < p->Lown; ++c)
        if (p->planes[c] >= 0) { pidx[c] = p->planes[c]; cidx[p->planes[c]] = c; }
    const size_t nv = (size_t)p->T * p->Lc;
    return ensure_set(member(p->tg_cidx, cidx), member(p->tg_pidx, pidx), member(p->tg_keep, (size_t)p->T * p->LP),
                      member(p->tg_part, tplgrad_part_doubles(p->T, p->Na, p->Nb, (int)p->LP, p->route.tpl_spectral)), member(p->tg_v[0], nv),
                      member(p->tg_v[1], nv), member(p->tg_v[2], nv), member(p->tg_v[3], nv), member(p->tg_v[4], nv), member(p->tg_v[5], nv));
}
int tpl_maps_spectra(surfh_plan *p, const float *maps) {
    {
        Prof pr(p, "pad_planes");
        LAUNCH_OK(launch_pad_planes(p->stream, maps, p->maps_pad, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    }
    return rfft2_planes(p, p->maps_pad, p->mhat, p->T);
}
int tpl_install(surfh_plan *p, const float *S) {
    Prof pr(p, "tpl_pack");
    LAUNCH_OK(launch_tpl_pack(p->stream, S, p->tg_pidx, p->tpl, p->T, p->Lc, (int)p->LP));
    return 0;
}
int TplScope::begin() {
    HIP_OK(hipMemcpyAsync(p->tg_keep, p->tpl, (size_t)p->T * p->LP * sizeof(float), hipMemcpyDeviceToDevice, p->stream));
    armed = true;
    return 0;
}
TplScope::~TplScope() {
    p->tg_mhat_ready = false;
    if (armed) hipMemcpyAsync(p->tpl, p->tg_keep, (size_t)p->T * p->LP * sizeof(float), hipMemcpyDeviceToDevice, p->stream);
}
namespace {
OpCall tpl_call(const surfh_plan *p, const float *maps, float *G) {      // tail: the template transpose; head: mhat if it holds the maps' spectra
    OpCall c;
    c.tail = OpCall::T_TEMPLATES; c.tpl_out = G; c.tpl_maps = maps;
    if (p->tg_mhat_ready) c.head = OpCall::H_MHAT;
    return c;
}
}  // namespace
int tpl_adjoint_dev(surfh_plan *p, const float *maps, const float *u, float *G) {
    if (!p->tg_mhat_ready && tpl_maps_spectra(p, maps)) return 1;
    return adjoint_dev(p, u, nullptr, tpl_call(p, maps, G));
}
int tpl_normal_dev(surfh_plan *p, const float *maps, float *G) {
    return normal_halves(p, maps, nullptr, tpl_call(p, maps, G));      // the forward half leaves the maps' spectra in mhat, where the tail reads them
}

}  // namespace surfh_impl

extern "C" {

int surfh_forward_dev(surfh_plan *p, const float *x, float *y) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    return forward_dev(p, x, y);
}
int surfh_adjoint_dev(surfh_plan *p, const float *y, float *x) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    return adjoint_dev(p, y, x);
}
int surfh_adjoint_ref_dev(surfh_plan *p, const float *y, float *x) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    OpCall c;
    c.ref = true;
    return adjoint_dev(p, y, x, c);
}
int surfh_fwadj_dev(surfh_plan *p, const float *x, float *out) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    return normal_dev(p, x, out, 1.0);
}

static int host_call(surfh_plan *p, const float *in, long nin, float *outp, long nout, int which) {
    if (!p || !in || !outp) return fail("null argument");
    HIP_OK(hipSetDevice(p->dev));
    float *din = (which == 0 || which == 3) ? p->io_x : p->io_y;
    float *dout = (which == 0) ? p->io_y : p->io_x;
    if (which == 3) {
        if (ensure_cg(p)) return 1;
        dout = p->cg_q;
    }
    HIP_OK(hipMemcpyAsync(din, in, nin * sizeof(float), hipMemcpyHostToDevice, p->stream));
    int rc = 0;
    if (which == 0) rc = forward_dev(p, din, dout);
    else if (which == 1) rc = adjoint_dev(p, din, dout);
    else if (which == 2) rc = surfh_adjoint_ref_dev(p, din, dout);
    else rc = normal_dev(p, din, dout, 1.0);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(outp, dout, nout * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

int surfh_forward(surfh_plan *p, const float *maps, float *y) { return host_call(p, maps, p ? p->isize : 0, y, p ? p->osize : 0, 0); }
int surfh_adjoint(surfh_plan *p, const float *y, float *maps) { return host_call(p, y, p ? p->osize : 0, maps, p ? p->isize : 0, 1); }
int surfh_adjoint_ref(surfh_plan *p, const float *y, float *maps) { return host_call(p, y, p ? p->osize : 0, maps, p ? p->isize : 0, 2); }
int surfh_fwadj(surfh_plan *p, const float *x, float *o) { return host_call(p, x, p ? p->isize : 0, o, p ? p->isize : 0, 3); }

// ---- Model_WCT: the T.C stage alone, cube in the reference's [Lc][Na][Nb] layout ------------------
static int wct_check(surfh_plan *p) {
    if (!p) return fail("null plan");
    if (p->T < 1) return fail("Model_WCT needs templates");
    if (p->segs.size() != 1 || p->segs[0].start != 0 || p->segs[0].len != p->Lc) return fail("Model_WCT needs a plan that owns every cube plane");
    if (hipSetDevice(p->dev) != hipSuccess) return fail("hipSetDevice failed");
    return ensure_set(member(p->io_cube, (size_t)p->Lc * p->Na * p->Nb));
}

int surfh_wct_forward(surfh_plan *p, const float *maps, float *cube) {
    if (wct_check(p)) return 1;
    if (!maps || !cube) return fail("null argument");
    hipStream_t s = p->stream;
    HIP_OK(hipMemcpyAsync(p->io_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, s));
    LAUNCH_OK(launch_pad_planes(s, p->io_x, p->maps_pad, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    if (rfft2_planes(p, p->maps_pad, p->mhat, p->T)) return 1;
    LAUNCH_OK(launch_specmix_fwd(s, p->mhat, p->sotf, p->tpl, p->spec, p->T, p->PL, p->LP, p->route.interleaved()));
    if (irfft2_cube(p, p->spec, p->cube)) return 1;
    LAUNCH_OK(launch_cube_from_lam_inner(s, p->cube, p->io_cube, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP));
    HIP_OK(hipMemcpyAsync(cube, p->io_cube, (size_t)p->Lc * p->Na * p->Nb * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

int surfh_wct_adjoint(surfh_plan *p, const float *cube, float *maps) {
    if (wct_check(p)) return 1;
    if (!maps || !cube) return fail("null argument");
    hipStream_t s = p->stream;
    HIP_OK(hipMemcpyAsync(p->io_cube, cube, (size_t)p->Lc * p->Na * p->Nb * sizeof(float), hipMemcpyHostToDevice, s));
    LAUNCH_OK(launch_fill_zero(s, p->cube, (long)p->NBP * p->NAP * p->LP));
    LAUNCH_OK(launch_cube_to_lam_inner(s, p->io_cube, p->cube, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP));
    if (adjoint_tail(p, p->cube)) return 1;
    if (irfft2_planes(p, p->mhat, p->maps_pad, p->T)) return 1;
    LAUNCH_OK(launch_unpad_planes(s, p->maps_pad, p->io_x, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    HIP_OK(hipMemcpyAsync(maps, p->io_x, p->isize * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

int surfh_wct_fwadj(surfh_plan *p, const float *x, float *out) {
    if (wct_check(p)) return 1;
    if (!x || !out) return fail("null argument");
    hipStream_t s = p->stream;
    if (ensure_hessian(p)) return 1;
    HIP_OK(hipMemcpyAsync(p->io_x, x, p->isize * sizeof(float), hipMemcpyHostToDevice, s));
    LAUNCH_OK(launch_pad_planes(s, p->io_x, p->maps_pad, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    if (rfft2_planes(p, p->maps_pad, p->mhat, p->T)) return 1;
    LAUNCH_OK(launch_wct_hess_apply(s, p->hth, p->mhat, p->mhat2, p->T, p->PL));
    if (irfft2_planes(p, p->mhat2, p->maps_pad, p->T)) return 1;
    LAUNCH_OK(launch_unpad_planes(s, p->maps_pad, p->io_x, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    HIP_OK(hipMemcpyAsync(out, p->io_x, p->isize * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

// explicit inverse of the regularised normal operator (QuadCriterion3.run_expsol, fusion_mixing.py:309-438)
int surfh_wct_expsol(surfh_plan *p, const float *cube, const double *mu_reg, const double *reg_freq, float *maps) {
    if (wct_check(p)) return 1;
    if (!maps || !cube || !mu_reg || !reg_freq) return fail("null argument");
    for (int t = 0; t < p->T; ++t)
        if (!(mu_reg[t] >= 0.0)) return fail("mu_reg[%d] must be >= 0", t);
    hipStream_t s = p->stream;
    if (ensure_hessian(p)) return 1;
    // |D(f)|^2 into the padded spectral layout [KAP][KBP]; -1 marks the padding bins
    const int hb = p->Nb / 2 + 1;
    std::vector<float> reg((size_t)p->PL, -1.f);
    for (int a = 0; a < p->Na; ++a)
        for (int b = 0; b < hb; ++b) {
            const double v = reg_freq[(size_t)a * hb + b];
            if (!(v >= 0.0)) return fail("reg_freq must be >= 0");
            reg[(size_t)a * p->KBP + b] = (float)v;
        }
    DevBuf<float> dreg;
    DevBuf<double> dmu;
    DevBuf<int> dflag;
    if (dreg.upload(reg) || dmu.alloc((size_t)p->T) || dflag.alloc(1)) return 1;
    if (hipMemcpy(dmu, mu_reg, p->T * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dflag, 0, sizeof(int)) != hipSuccess) return fail("copy failed");
    // b = H^T y in the Fourier domain (surfh_wct_adjoint up to the inverse transform).  The mean of every plane is taken out in
    // float64 before the fp32 transforms and put back into the zero-frequency bin of b afterwards: left in, its rounding leaks
    // into the other bins of the k_beta = 0 column, small against the mean but not against the bins themselves, and the solve
    // amplifies it where hth and mu |D|^2 are both small (a band-limited OTF with a small mu)
    const size_t npl = (size_t)p->Na * p->Nb;
    std::vector<float> y0((size_t)p->Lc * npl);
    std::vector<double> mean((size_t)p->Lc);
    for (int l = 0; l < p->Lc; ++l) {
        const float *src = cube + (size_t)l * npl;
        double sum = 0.0;
        for (size_t i = 0; i < npl; ++i) sum += src[i];
        mean[l] = sum / (double)npl;
        for (size_t i = 0; i < npl; ++i) y0[(size_t)l * npl + i] = (float)((double)src[i] - mean[l]);
    }
    std::vector<float> h0((size_t)2 * p->LP);       // the OTF at the zero frequency as the kernels read it: (re, im) of every plane
    if (p->route.interleaved()) {
        if (hipMemcpy(h0.data(), p->sotf, h0.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return fail("copy failed");
    } else {
        std::vector<float> re((size_t)p->LP), im((size_t)p->LP);
        if (hipMemcpy(re.data(), p->sotf, re.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(im.data(), p->sotf + (size_t)p->PL * p->LP, im.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return fail("copy failed");
        for (long l = 0; l < p->LP; ++l) { h0[2 * l] = re[l]; h0[2 * l + 1] = im[l]; }
    }
    std::vector<double> dc((size_t)2 * p->T, 0.0);  // sum_l tpl[t][l] conj(H_l(0)) mean_l sqrt(Na Nb): the transforms are unitary
    const double dcs = std::sqrt((double)npl);
    for (int t = 0; t < p->T; ++t)
        for (int l = 0; l < p->Lc; ++l) {
            const double w = (double)(float)p->tpl_host[(size_t)t * p->Lc + l] * mean[l] * dcs;
            dc[2 * t] += w * (double)h0[2 * l];
            dc[2 * t + 1] -= w * (double)h0[2 * l + 1];
        }
    if (hipMemcpyAsync(p->io_cube, y0.data(), y0.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
        return fail("copy failed");
    int rc = launch_fill_zero(s, p->cube, (long)p->NBP * p->NAP * p->LP);
    if (!rc) rc = launch_cube_to_lam_inner(s, p->io_cube, p->cube, 0, p->Lc, p->Na, p->Nb, p->NAP, p->LP);
    if (rc) return fail("launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (adjoint_tail(p, p->cube)) return 1;
    for (int t = 0; t < p->T; ++t)
        for (int c = 0; c < 2; ++c) {               // bin (0, 0) of mhat [T][2][KAP][KBP]
            float *bin = p->mhat + ((size_t)t * 2 + c) * p->PL;
            float v = 0.f;
            if (hipMemcpyAsync(&v, bin, sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return fail("copy failed");
            v = (float)((double)v + dc[2 * t + c]);
            if (hipMemcpyAsync(bin, &v, sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return fail("copy failed");
        }
    rc = launch_wct_solve(s, p->hth, dreg, dmu, p->mhat, p->mhat2, p->T, p->PL, dflag);
    if (rc) return fail("launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (irfft2_planes(p, p->mhat2, p->maps_pad, p->T)) return 1;
    rc = launch_unpad_planes(s, p->maps_pad, p->io_x, p->T, p->Na, p->Nb, p->NAP, p->NBP);
    int flag = 0;
    if (!rc) rc = (int)hipMemcpyAsync(maps, p->io_x, p->isize * sizeof(float), hipMemcpyDeviceToHost, s);
    if (!rc) rc = (int)hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (!rc) rc = (int)hipStreamSynchronize(s);
    if (rc) return fail("expsol failed: %s", hipGetErrorString((hipError_t)rc));
    if (flag) return fail("the regularised normal matrix is singular at some frequency (numpy.linalg.inv would raise LinAlgError)");
    return 0;
}

// ---- CG building blocks ---------------------------------------------------------------------
int surfh_normal_dev(surfh_plan *p, const float *d, float *q, double mu) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    return normal_dev(p, d, q, mu);
}
int surfh_prior_add_dev(surfh_plan *p, const float *d, float *q, double mu_reg) {
    if (!p) return fail("null plan");
    if (p->T <= 0) return fail("prior is defined on abundance maps (needs templates)");
    HIP_OK(hipSetDevice(p->dev));
    Prof pr(p, "prior_add");
    LAUNCH_OK(prior_add(p, p->stream, d, q, p->T, (float)mu_reg));
    return 0;
}
// ---- the normal operator on the maps' half spectra (the solver's vectors live in the Fourier domain) -------------------------
// A vector is [T][2 (re, im)][KAP][KBP] floats (padding zero), bin (ka, kb) multiplied by sqrt(2) unless it is its own conjugate
// (kb = 0, or 2 kb = Nb): the transforms are unitary, so plain dot products of such vectors are the dot products of the maps.
namespace {
int spec_check(surfh_plan *p) {
    if (!p) return fail("null plan");
    if (!p->route.spec_calls)
        return fail("spectral-domain calls need the fused transform passes (dft_h2 with the fused adjoint tail, or dft_ct)");
    HIP_OK(hipSetDevice(p->dev));
    return 0;
}
// tail of a spectral-domain call: qt = mu * scaled half spectra (+ mu_reg * |D|^2 * dt, the quadratic prior, when dt != NULL)
OpCall spec_tail(float *qt, double mu, const float *dt, double mu_reg) {
    OpCall c;
    c.tail = OpCall::T_SPECTRA; c.spectra_out = qt; c.mu = (float)mu; c.prior_src = dt; c.prior_mu = dt ? (float)mu_reg : 0.f;
    return c;
}
}  // namespace

int surfh_spec_supported(surfh_plan *p) {
    return p && p->route.spec_calls && p->prior_kind == 0;
}
int64_t surfh_spec_size(surfh_plan *p) { return p ? (int64_t)2 * p->T * p->PL : 0; }

// xt = scaled half spectra of the maps x [T][Na][Nb]
int surfh_to_spec_dev(surfh_plan *p, const float *x, float *xt) {
    if (spec_check(p)) return 1;
    hipStream_t s = p->stream;
    LAUNCH_OK(launch_pad_planes(s, x, p->maps_pad, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    if (rfft2_planes(p, p->maps_pad, p->mhat, p->T)) return 1;
    LAUNCH_OK(launch_spec_scale(s, p->mhat, xt, 2 * p->T, p->PL, p->KBP, p->Nb, 1.f, 1.41421356237309505f));
    return 0;
}
// x = maps of the scaled half spectra xt
int surfh_from_spec_dev(surfh_plan *p, const float *xt, float *x) {
    if (spec_check(p)) return 1;
    hipStream_t s = p->stream;
    LAUNCH_OK(launch_spec_scale(s, xt, p->mhat, 2 * p->T, p->PL, p->KBP, p->Nb, 1.f, 0.70710678118654752f));
    if (irfft2_planes(p, p->mhat, p->maps_pad, p->T)) return 1;
    LAUNCH_OK(launch_unpad_planes(s, p->maps_pad, x, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    return 0;
}
// y = A maps(dt)
int surfh_forward_spec_dev(surfh_plan *p, const float *dt, float *y) {
    if (spec_check(p)) return 1;
    OpCall c;
    c.head = OpCall::H_SPECTRA; c.spectra_in = dt;
    return forward_dev(p, nullptr, y, c);
}
// qt = mu * spectra(A^T y)  (+ mu_reg * prior(dt) when dt != NULL: only where q is not summed over ranks afterwards)
int surfh_adjoint_spec_dev(surfh_plan *p, const float *y, float *qt, double mu, const float *dt, double mu_reg) {
    if (spec_check(p)) return 1;
    if (dt && p->prior_kind != 0) return fail("the fused spectral prior is the separated first differences");
    return adjoint_dev(p, y, nullptr, spec_tail(qt, mu, dt, mu_reg));
}
// qt = mu * spectra(A^T A maps(dt)) (+ mu_reg * prior(dt) if mu_reg != 0): the CG's normal operator without a single transform
// of the maps -- no padding, no small DFTs, no prior kernel
int surfh_normal_spec_dev(surfh_plan *p, const float *dt, float *qt, double mu, double mu_reg) {
    if (spec_check(p)) return 1;
    if (mu_reg != 0.0 && p->prior_kind != 0) return fail("the fused spectral prior is the separated first differences");
    OpCall c = spec_tail(qt, mu, mu_reg != 0.0 ? dt : nullptr, mu_reg);
    c.head = OpCall::H_SPECTRA; c.spectra_in = dt;
    return normal_halves(p, nullptr, nullptr, c);
}
// qt += mu_reg * prior(dt) on scaled half spectra (after an all-reduce of qt over ranks)
int surfh_prior_spec_add_dev(surfh_plan *p, const float *dt, float *qt, double mu_reg) {
    if (spec_check(p)) return 1;
    if (p->prior_kind != 0) return fail("the spectral prior is the separated first differences");
    LAUNCH_OK(launch_spec_prior_add(p->stream, dt, qt, 2 * p->T, p->Na, p->Nb, p->PL, p->KBP, (float)mu_reg));
    return 0;
}

// ---- drivers' LMM helpers on the device (spectroModel.py:187-198) -----------------------------
static int lmm_host(surfh_plan *p, const double *templates, int32_t T, int32_t L, const float *in, float *out, bool to_cube) {
    if (!p || !templates || !in || !out) return fail("null argument");
    if (T < 1 || L < 1) return fail("bad template shape");
    HIP_OK(hipSetDevice(p->dev));
    const long npix = (long)p->Na * p->Nb;
    std::vector<float> t((size_t)T * L);
    for (size_t i = 0; i < t.size(); ++i) t[i] = (float)templates[i];
    DevBuf<float> dt, dm, dc;
    int rc = 0;
    if (dt.upload(t) || dm.alloc((size_t)T * npix) || dc.alloc((size_t)L * npix)) return 1;
    hipStream_t s = p->stream;
    if (to_cube) {
        if (hipMemcpyAsync(dm, in, (size_t)T * npix * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) return fail("copy failed");
        rc = launch_lmm_maps2cube(s, dm, dt, dc, T, L, npix);
        if (!rc) rc = (int)hipMemcpyAsync(out, dc, (size_t)L * npix * sizeof(float), hipMemcpyDeviceToHost, s);
    } else {
        if (hipMemcpyAsync(dc, in, (size_t)L * npix * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) return fail("copy failed");
        rc = launch_lmm_cube2maps(s, dc, dt, dm, T, L, npix);
        if (!rc) rc = (int)hipMemcpyAsync(out, dm, (size_t)T * npix * sizeof(float), hipMemcpyDeviceToHost, s);
    }
    if (!rc) rc = (int)hipStreamSynchronize(s);
    if (rc) return fail("lmm: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}
int surfh_maps_to_cube(surfh_plan *p, const double *templates, int32_t T, int32_t L, const float *maps, float *cube) {
    return lmm_host(p, templates, T, L, maps, cube, true);
}
int surfh_cube_to_maps(surfh_plan *p, const double *templates, int32_t T, int32_t L, const float *cube, float *maps) {
    return lmm_host(p, templates, T, L, cube, maps, false);
}

// ---- the templates as plan state, and as the argument of the operator (template refinement) ----
int surfh_get_templates(const surfh_plan *p, double *tpl) {
    if (!p || !tpl) return fail("null argument");
    if (p->T < 1) return fail("the plan has no templates");
    std::copy(p->tpl_host.begin(), p->tpl_host.end(), tpl);
    return 0;
}
int surfh_set_templates(surfh_plan *p, const double *tpl) {
    if (!p || !tpl) return fail("null argument");
    if (p->T < 1) return fail("the plan has no templates: their number and length are fixed at plan creation");
    if (p->im_g)
        return fail("set_templates: an imager is attached, and its transfer functions G[f,t,k] were built from the templates: detach it "
                    "(surfh_set_imager(plan, NULL)), set the templates, then attach the imager again");
    const size_t n = (size_t)p->T * p->Lc;
    for (size_t i = 0; i < n; ++i)
        if (!(std::fabs(tpl[i]) <= FLT_MAX)) return fail("set_templates: template %ld has %g at plane %ld: templates are finite in float32", (long)(i / p->Lc), tpl[i], (long)(i % p->Lc));
    HIP_OK(hipSetDevice(p->dev));
    // the rounding and the padding of plan creation: compact planes, zero in the alignment gaps and beyond the last plane
    std::vector<float> t((size_t)p->T * p->LP, 0.f);
    for (int k = 0; k < p->T; ++k)
        for (int l = 0; l < p->Lown; ++l)
            if (p->planes[l] >= 0) t[(size_t)k * p->LP + l] = (float)tpl[(size_t)k * p->Lc + p->planes[l]];
    HIP_OK(hipStreamSynchronize(p->stream));
    HIP_OK(hipMemcpy(p->tpl, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    p->tpl_host.assign(tpl, tpl + n);
    // Model_WCT's explicit Hessian was built from the old templates: ensure_hessian builds it again on the next call
    p->hth.reset();
    p->mhat2.reset();
    return 0;
}
static int tpl_call_check(surfh_plan *p, const void *a, const void *b, const void *c) {
    if (!p || !a || !b || !c) return fail("null argument");
    HIP_OK(hipSetDevice(p->dev));
    return tpl_ensure(p);
}
int surfh_forward_templates_dev(surfh_plan *p, const float *maps_dev, const float *tpl_dev, float *y_dev) {
    if (tpl_call_check(p, maps_dev, tpl_dev, y_dev)) return 1;
    TplScope sc(p);
    if (sc.begin() || tpl_install(p, tpl_dev)) return 1;
    return forward_dev(p, maps_dev, y_dev);
}
int surfh_adjoint_templates_dev(surfh_plan *p, const float *maps_dev, const float *u_dev, float *g_dev) {
    if (tpl_call_check(p, maps_dev, u_dev, g_dev)) return 1;
    return tpl_adjoint_dev(p, maps_dev, u_dev, g_dev);
}
int surfh_forward_templates(surfh_plan *p, const float *maps, const double *tpl, float *y) {
    if (tpl_call_check(p, maps, tpl, y)) return 1;
    const size_t n = (size_t)p->T * p->Lc;
    std::vector<float> t(n);
    for (size_t i = 0; i < n; ++i) t[i] = (float)tpl[i];
    HIP_OK(hipMemcpyAsync(p->io_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(p->tg_v[5], t.data(), n * sizeof(float), hipMemcpyHostToDevice, p->stream));
    {
        TplScope sc(p);
        if (sc.begin() || tpl_install(p, p->tg_v[5]) || forward_dev(p, p->io_x, p->io_y)) return 1;
    }
    HIP_OK(hipMemcpyAsync(y, p->io_y, p->osize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int surfh_adjoint_templates(surfh_plan *p, const float *maps, const float *u, float *g) {
    if (tpl_call_check(p, maps, u, g)) return 1;
    HIP_OK(hipMemcpyAsync(p->io_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(p->io_y, u, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (tpl_adjoint_dev(p, p->io_x, p->io_y, p->tg_v[5])) return 1;
    HIP_OK(hipMemcpyAsync(g, p->tg_v[5], (size_t)p->T * p->Lc * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

}  // extern "C"

// ---- imager data term (include/surfh_amd.h: surfh_set_imager; kernels: imager.hip) ---------------------------------------------
// A_im = sample . irfft2 . G . rfft2 on T maps -> F images, its transpose the same chain backwards with conj(G); the transforms
// are the plane transforms of the maps (rfft2_planes / irfft2_planes) on the imager's own padded buffers, so an application
// leaves every buffer of the spectrometer's operator alone except their temporary ycol_maps.
namespace surfh_impl {
namespace {
int imager_to_spectra(surfh_plan *p, const float *x) {            // x [T][Na][Nb] -> im_xhat
    {
        Prof pr(p, "imager_pad");
        LAUNCH_OK(launch_pad_planes(p->stream, x, p->im_xpad, p->T, p->Na, p->Nb, p->NAP, p->NBP));
    }
    return rfft2_planes(p, p->im_xpad, p->im_xhat, p->T);
}
int imager_to_images(surfh_plan *p) {                             // im_xhat -> im_zpad (full resolution, before the detector)
    {
        Prof pr(p, "imager_mix_fwd");
        LAUNCH_OK(launch_imager_mix_fwd(p->stream, p->im_g, p->im_xhat, p->im_zhat, p->im_F, p->T, p->PL));
    }
    return irfft2_planes(p, p->im_zhat, p->im_zpad, p->im_F);
}
int imager_from_images(surfh_plan *p, float *out, float scale, bool accumulate) {      // out (+)= scale * (maps of im_zpad)
    if (rfft2_planes(p, p->im_zpad, p->im_zhat, p->im_F)) return 1;
    {
        Prof pr(p, "imager_mix_adj");
        LAUNCH_OK(launch_imager_mix_adj(p->stream, p->im_g, p->im_zhat, p->im_xhat, p->im_F, p->T, p->PL, scale, 0));
    }
    if (irfft2_planes(p, p->im_xhat, p->im_xpad, p->T)) return 1;
    Prof pr(p, "imager_unpad");
    LAUNCH_OK(launch_imager_unpad(p->stream, p->im_xpad, out, p->T, p->Na, p->Nb, p->NBP, p->PLc, accumulate ? 1 : 0));
    return 0;
}
int imager_forward_dev(surfh_plan *p, const float *x, float *y) {
    if (imager_to_spectra(p, x) || imager_to_images(p)) return 1;
    Prof pr(p, "imager_sample");
    LAUNCH_OK(launch_imager_sample(p->stream, p->im_zpad, y, p->im_F, p->im_d, p->Na, p->Nb, p->NBP, p->PLc));
    return 0;
}
int imager_adjoint_dev(surfh_plan *p, const float *y, float *x, float scale, bool accumulate) {
    {
        Prof pr(p, "imager_spread");
        LAUNCH_OK(launch_imager_spread(p->stream, y, p->im_zpad, p->im_F, p->im_d, p->Na, p->Nb, p->NBP, p->PLc));
    }
    return imager_from_images(p, x, scale, accumulate);
}
// q (+)= scale A_im^T diag(w) A_im v
int imager_normal_dev(surfh_plan *p, const float *v, float *q, const float *w, float scale, bool accumulate) {
    if (imager_to_spectra(p, v) || imager_to_images(p)) return 1;
    {
        Prof pr(p, "imager_window");
        LAUNCH_OK(launch_imager_window(p->stream, p->im_zpad, w, p->im_F, p->im_d, p->Na, p->Nb, p->NBP, p->PLc));
    }
    return imager_from_images(p, q, scale, accumulate);
}
}  // namespace

int imager_normal_add(surfh_plan *p, const float *v, float *q) { return imager_normal_dev(p, v, q, p->im_w, (float)p->im_mu, true); }
int imager_rhs_add(surfh_plan *p, float *b) {
    const float *y = p->im_y;
    if (p->im_w) {          // W y by a select: a masked NaN stays out
        Prof pr(p, "imager_weight_select");
        LAUNCH_OK(launch_weight_select(p->stream, p->im_y, p->im_w, p->im_wy, p->im_osize));
        y = p->im_wy;
    }
    return imager_adjoint_dev(p, y, b, (float)p->im_mu, true);
}
}  // namespace surfh_impl

extern "C" {

int surfh_set_imager(surfh_plan *p, const surfh_imager_desc *desc) {
    if (!p) return fail("null plan");
    HIP_OK(hipSetDevice(p->dev));
    hipStream_t s = p->stream;
    if (!desc) {
        HIP_OK(hipStreamSynchronize(s));
        for (DevBuf<float> *v : {&p->im_g, &p->im_xpad, &p->im_xhat, &p->im_zpad, &p->im_zhat, &p->im_io, &p->im_y, &p->im_w, &p->im_wy}) v->reset();
        p->im_F = p->im_d = 0; p->im_osize = 0; p->im_mu = 0.0;
        return 0;
    }
    const int F = desc->n_filters, d = desc->decim, T = p->T, Lc = p->Lc, nkb = p->Nb / 2 + 1;
    if (T < 1) return fail("imager: the plan has no templates (the imager observes the cube the maps span)");
    if (T > SURFH_MAX_TEMPLATES) return fail("imager: at most %d templates (the plan has %d)", SURFH_MAX_TEMPLATES, T);
    if (F < 1 || F > 16) return fail("imager: n_filters = %d is outside 1..16", F);
    if (d < 1 || d > p->Na || d > p->Nb) return fail("imager: decim = %d is outside 1..min(n_alpha, n_beta) = %d", d, std::min(p->Na, p->Nb));
    if (!desc->filters) return fail("imager: null filters");
    for (long i = 0; i < (long)F * Lc; ++i)
        if (!(desc->filters[i] >= 0.0 && desc->filters[i] <= DBL_MAX))
            return fail("imager: filter %ld has %g at plane %ld: transmittances are finite and >= 0", i / Lc, desc->filters[i], i % Lc);
    const bool owns_all = p->segs.size() == 1 && p->segs[0].start == 0 && p->segs[0].len == Lc;
    if (!desc->sotf && !owns_all)
        return fail("imager: the plan does not own every cube plane (its channels' windows cover %d of %d): its own OTF cannot serve the "
                    "imager, hand the imager's OTF in", p->Lown, Lc);
    int chunk = 128;
    if (const char *e = getenv("SURFH_IMAGER_CHUNK")) {
        chunk = atoi(e);
        if (chunk < 32 || chunk > 128 || chunk % 32) return fail("imager: SURFH_IMAGER_CHUNK = %s is not a multiple of 32 in 32..128", e);
    }
    const size_t ng = (size_t)F * T * 2 * p->PL, osz = (size_t)F * (p->Na / d) * (p->Nb / d);
    // the new set (g .. io, a larger ycol_maps) and the call's temporaries, all locals: published by the swaps at the end
    DevBuf<float> g, xpad, xhat, zpad, zhat, io, ycm, otf_in, otf_pl, tplc;
    DevBuf<double> acc, wf;
    const size_t nycm = (size_t)F * 2 * p->NAP * p->KBP;
    if (g.alloc(ng) || acc.alloc(ng) || xpad.alloc((size_t)T * p->PLc) || xhat.alloc((size_t)T * 2 * p->PL) || zpad.alloc((size_t)F * p->PLc) ||
        zhat.alloc((size_t)F * 2 * p->PL) || io.alloc(osz) || (F > p->ycm_planes && ycm.alloc(nycm)))
        return 1;
    if (hipMemsetAsync(acc, 0, ng * sizeof(double), s) != hipSuccess || hipMemsetAsync(xpad, 0, (size_t)T * p->PLc * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(zpad, 0, (size_t)F * p->PLc * sizeof(float), s) != hipSuccess ||
        (ycm && hipMemsetAsync(ycm, 0, nycm * sizeof(float), s) != hipSuccess))
        return fail("memset failed");
    if (!desc->sotf) {       // the plan's device OTF and templates: compact plane index = cube plane
        const long LP = p->LP;
        std::vector<double> h((size_t)F * LP, 0.0);
        for (int f = 0; f < F; ++f) std::copy(desc->filters + (size_t)f * Lc, desc->filters + (size_t)(f + 1) * Lc, h.begin() + (size_t)f * LP);
        if (wf.upload(h)) return 1;
        const int rc = p->route.interleaved() ? launch_imager_build_g(s, p->sotf, 2 * LP, 2, 1, p->tpl, LP, wf, LP, (int)LP, acc, F, T, p->Na, nkb, p->KBP, p->PL)
                              : launch_imager_build_g(s, p->sotf, LP, 1, p->PL * LP, p->tpl, LP, wf, LP, (int)LP, acc, F, T, p->Na, nkb, p->KBP, p->PL);
        if (rc) return fail("launch_imager_build_g failed: %s", hipGetErrorString((hipError_t)rc));
    } else {                 // the imager's own OTF, streamed: chunk -> the plan's padded layout (wavelength innermost) -> the same kernel
        const int CHP = (chunk + 63) / 64 * 64;
        const size_t nbin = (size_t)p->Na * nkb;
        if (otf_in.alloc((size_t)chunk * nbin * 2) || otf_pl.alloc((size_t)2 * p->PL * CHP) || tplc.alloc((size_t)T * CHP) || wf.alloc((size_t)F * CHP))
            return 1;
        std::vector<float> ho((size_t)chunk * nbin * 2), ht((size_t)T * CHP);
        std::vector<double> hw((size_t)F * CHP);
        if (hipMemsetAsync(otf_pl, 0, (size_t)2 * p->PL * CHP * sizeof(float), s) != hipSuccess) return fail("memset failed");
        for (int l0 = 0; l0 < Lc; l0 += chunk) {
            const int n = std::min(chunk, Lc - l0);
            const double *src = desc->sotf + (size_t)l0 * nbin * 2;
            for (size_t i = 0; i < (size_t)n * nbin * 2; ++i) ho[i] = (float)src[i];
            std::fill(ht.begin(), ht.end(), 0.f);
            std::fill(hw.begin(), hw.end(), 0.0);
            for (int l = 0; l < n; ++l) {
                for (int t = 0; t < T; ++t) ht[(size_t)t * CHP + l] = (float)p->tpl_host[(size_t)t * Lc + l0 + l];
                for (int f = 0; f < F; ++f) hw[(size_t)f * CHP + l] = desc->filters[(size_t)f * Lc + l0 + l];
            }
            if (hipMemcpyAsync(otf_in, ho.data(), (size_t)n * nbin * 2 * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(tplc, ht.data(), ht.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(wf, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
                return fail("imager: OTF upload failed");
            int rc = launch_imager_otf_chunk(s, otf_in, otf_pl, n, CHP, p->Na, nkb, p->KBP, p->PL);
            if (!rc) rc = launch_imager_build_g(s, otf_pl, CHP, 1, p->PL * CHP, tplc, CHP, wf, CHP, CHP, acc, F, T, p->Na, nkb, p->KBP, p->PL);
            if (rc) return fail("launch_imager_build_g failed: %s", hipGetErrorString((hipError_t)rc));
            if (hipStreamSynchronize(s) != hipSuccess) return fail("imager: set-up failed on the device");   // the host buffers are reused
        }
    }
    if (const int rc = launch_imager_g_store(s, acc, g, (long)ng)) return fail("launch_imager_g_store failed: %s", hipGetErrorString((hipError_t)rc));
    if (hipStreamSynchronize(s) != hipSuccess) return fail("imager: set-up failed on the device");
    // publish: nothing in flight reads the old buffers; the data of a previous imager go with it (their size is that imager's)
    p->im_g.swap(g); p->im_xpad.swap(xpad); p->im_xhat.swap(xhat); p->im_zpad.swap(zpad); p->im_zhat.swap(zhat); p->im_io.swap(io);
    if (ycm) { p->ycol_maps.swap(ycm); p->ycm_planes = F; }
    for (DevBuf<float> *v : {&p->im_y, &p->im_w, &p->im_wy}) v->reset();
    p->im_mu = 0.0;
    p->im_F = F; p->im_d = d; p->im_osize = (long)osz;
    return 0;
}

int surfh_imager_osize(const surfh_plan *p) { return p && p->im_g ? (int)p->im_osize : 0; }
int surfh_has_imager_term(const surfh_plan *p) { return p && imager_active(p) ? 1 : 0; }

static int imager_check(surfh_plan *p, const void *a, const void *b) {
    if (!p || !a || !b) return fail("null argument");
    if (!p->im_g) return fail("no imager is attached to this plan (surfh_set_imager)");
    HIP_OK(hipSetDevice(p->dev));
    return 0;
}
int surfh_imager_forward_dev(surfh_plan *p, const float *maps, float *y_im) {
    if (imager_check(p, maps, y_im)) return 1;
    return imager_forward_dev(p, maps, y_im);
}
int surfh_imager_adjoint_dev(surfh_plan *p, const float *y_im, float *maps) {
    if (imager_check(p, y_im, maps)) return 1;
    return imager_adjoint_dev(p, y_im, maps, 1.f, false);
}
int surfh_imager_forward(surfh_plan *p, const float *maps, float *y_im) {
    if (imager_check(p, maps, y_im)) return 1;
    HIP_OK(hipMemcpyAsync(p->io_x, maps, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (imager_forward_dev(p, p->io_x, p->im_io)) return 1;
    HIP_OK(hipMemcpyAsync(y_im, p->im_io, p->im_osize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int surfh_imager_adjoint(surfh_plan *p, const float *y_im, float *maps) {
    if (imager_check(p, y_im, maps)) return 1;
    HIP_OK(hipMemcpyAsync(p->im_io, y_im, p->im_osize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (imager_adjoint_dev(p, p->im_io, p->io_x, 1.f, false)) return 1;
    HIP_OK(hipMemcpyAsync(maps, p->io_x, p->isize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}
int surfh_imager_fwadj(surfh_plan *p, const float *x, float *out) {
    if (imager_check(p, x, out)) return 1;
    if (ensure_cg(p)) return 1;
    HIP_OK(hipMemcpyAsync(p->io_x, x, p->isize * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (imager_normal_dev(p, p->io_x, p->cg_q, p->im_y ? p->im_w : nullptr, 1.f, false)) return 1;
    HIP_OK(hipMemcpyAsync(out, p->cg_q, p->isize * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

int surfh_set_imager_data(surfh_plan *p, const float *y_im, const float *w_im, double mu_imager) {
    if (!p) return fail("null plan");
    if (!p->im_g) return fail("no imager is attached to this plan (surfh_set_imager)");
    HIP_OK(hipSetDevice(p->dev));
    DevBuf<float> y, w, wy;
    double mu = 0.0;
    if (y_im) {
        if (!(mu_imager >= 0.0 && mu_imager <= DBL_MAX)) return fail("imager: mu_imager = %g must be finite and >= 0", mu_imager);
        const size_t n = (size_t)p->im_osize;
        if (w_im)
            for (size_t i = 0; i < n; ++i)
                if (!(w_im[i] >= 0.f && w_im[i] <= FLT_MAX)) return fail("imager: weight %ld is %g: weights are finite and >= 0", (long)i, (double)w_im[i]);
        if (y.alloc(n) || (w_im && (w.alloc(n) || wy.alloc(n)))) return 1;
        if (hipMemcpyAsync(y, y_im, n * sizeof(float), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
            (w_im && hipMemcpyAsync(w, w_im, n * sizeof(float), hipMemcpyHostToDevice, p->stream) != hipSuccess))
            return fail("copy failed");
        mu = mu_imager;
    }
    if (hipStreamSynchronize(p->stream) != hipSuccess) return fail("stream synchronisation failed");
    p->im_y.swap(y); p->im_w.swap(w); p->im_wy.swap(wy);
    p->im_mu = mu;
    return 0;
}

}  // extern "C"
