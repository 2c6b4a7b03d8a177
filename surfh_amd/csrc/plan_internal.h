// Internal header of the host side of the C ABI (include/surfh_amd.h), shared by plan.hip (plan build and plan state),
// plan_ops.hip (operators), plan_solvers.hip (solvers) and plan_diag.hip (diagnostics).  The rule of the split: solvers call the
// operators, operators read the plan, plan build knows neither operators nor solvers, diagnostics depend on everything and
// nothing depends on them -- so this header declares only the helpers that cross a file boundary in that direction.  What one
// operator call does beyond the plan -- where its operand comes from, where its result goes -- is its argument (OpCall below):
// the plan holds what lasts from call to call, never the mode of the next one.
// Everything shared lives in namespace surfh_impl, which has hidden visibility: the shared object exports the C ABI and nothing else.
//
// Data layout: WAVELENGTH IS THE INNERMOST AXIS of every large device array (lambda is the batch
// dimension of every stage of the reference, so making it contiguous turns every kernel into
// coalesced streaming and every dense stage into one large GEMM):
//   spectra  sotf, spec      [2 (re,im)][KAP][KBP][LP]
//   cube     blurred / g     [NBP (beta)][NAP (alpha)][LP]
//   operand  Xs (per channel)[NP = (p,s,a)][n_beta_slit][LinP]      K index = (b', lambda)
// LP = owned planes padded to 128, all other dims padded to 64, padding is zero.
// Leff = owned planes rounded up to 32 (the widest wave tile of the transform passes), the extent the passes of the
// fused-mix forward and the adjoint's pass in front of the fused tail are launched over; every stride and allocation stays LP.  The planes [Leff, LP) of ycol, ycol_mix, ycol_adj,
// cube and gcube are zeroed at plan creation and never written by those passes -- "zero for good", like the columns outside
// [a_lo, a_hi) of ycol_adj and the tiles outside the OTF's support of ycol_mix.  (The planes [Lown, Leff) are transformed: their
// sources -- sotf, tpl, what the scatters leave -- are zero, so they come out as zeros.)
//
// Pipeline (per plan = per GPU), reference citations relative to the reference's source tree:
//   forward  (spectroModel.py:158-170, spectroModelChannel.py:215-231)
//     maps --pad--> rfft2 (2 small GEMMs) --> mhat[T][2][KAP][KBP]
//     spec[k][l] = sotf[k][l] * sum_t tpl[t,l] mhat[t][k]             (T and C fused, Fourier domain)
//     blurred    = irfft2(spec): two GEMMs with the DFT matrices as the A operand
//     per channel:  Xs[(p,s,a)][b'][l] = G * blurred                  (S + box-sum + L + decimation, row gather)
//                   y^T[(p,s,a)][l'] = Xs * W^T                       (R + beta-sum, one GEMM, split-K)
//   adjoint  (spectroModel.py:173-185, spectroModelChannel.py:234-264): the transposes, in reverse.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/surfh_amd.h"
#include "dev_buf.h"
#include "dft_h2.h"
#include "dft_ct.h"
#include "gemm_f32.h"
#include "kernels.h"
#include "tplgrad.h"

namespace surfh_impl __attribute__((visibility("hidden"))) {

// fail(): records the message surfh_last_error() returns and returns 1 (declared in dev_buf.h; defined once, in plan.hip, beside
// the thread's error string)

// a boolean SURFH_* switch: `dflt` when the variable is unset or empty; a default-on switch goes off only with a leading '0',
// a default-off switch goes on only with a leading '1'
inline bool env_on(const char *name, bool dflt) {
    const char *e = getenv(name);
    return dflt ? !(e && e[0] == '0') : (e && e[0] == '1');
}

#define HIP_OK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define LAUNCH_OK(expr)                                                                           \
    do {                                                                                          \
        int e_ = (expr);                                                                          \
        if (e_ != 0) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString((hipError_t)e_), __FILE__, __LINE__); \
    } while (0)

inline int pad64(int n) { return (n + 63) / 64 * 64; }

// host-side sparse rows: (source index, weight) lists + one destination per row
struct HostEll {
    std::vector<std::vector<std::pair<int64_t, float>>> rows;
    std::vector<int64_t> dst;
};

struct DevEll {
    EllTable t;                         // views of the buffers below, as the kernels take them
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> col, dst;
    DevBuf<float> val;
    DevBuf<uint32_t> rmw;               // scatter tables: chunks of a row that need read-modify-write (EllTable::rmw)
    DevBuf<int2> rng, g_rng;            // ... or the exact wavelength ranges (EllTable::rng, GroupTable::rng)
    std::vector<int64_t> host_dst;      // kept for the scatter tables until the plan is complete
    // the same table with its rows grouped SCATTER_G at a time (GroupTable, views likewise)
    GroupTable g;
    DevBuf<int32_t> g_cnt;
    DevBuf<int64_t> g_col, g_dst;
    DevBuf<float> g_val;
    DevBuf<uint32_t> g_rmw;
};

struct Channel {
    int ws0 = 0, ws1 = 0, Lin = 0, P = 0, S = 0, Ldet = 0, aout = 0, srf = 0, na = 0, nb = 0, alpha0 = 0, nas = 0,
        nbs = 0;
    int ws0a = 0;      // window start relative to the plan's first plane, rounded down to a multiple of 4
    int LinA = 0;      // planes from ws0a to the window end
    int LinP = 0;      // LinA padded to 64
    int shift = 0;     // (ws0 - lo) - ws0a
    int nlam = 0;      // LinA rounded up to 4: wavelengths the gather kernels process
    int K = 0, NP = 0, LdetP = 0, splitK = 1;
    long yoff = 0, ysize = 0;
    DevBuf<float> W, Wt, Xs, Cpart, ymat;
    DevBuf<unsigned short> W16, Wt16;               // ... or into their two fp16 pieces [2][rows][cols] of W / sW (gemm_cc16.hip)
    DevBuf<unsigned short> Xs16, ymat16;            // the data operands as fp16 pieces (all-consumer kernel, gemm_cc16.hip)
    DevBuf<float> bscale;                           // Xs16's scales, one per (row, K segment): [nbs * ceil(LinP/1024)][NP]
    float sW = 1.f;
    // K-step classes of the two GEMMs (gemm_cc16.hip, build_klist below): per 256-row tile of W16 / Wt16 the steps that keep
    // all three products and the steps kept as h*h only; ksteps = (near, far) of the forward, (near, far) of the adjoint
    DevBuf<int> klF, klA;
    int klFs = 0, klAs = 0;
    int permA = 0;                      // adjoint GEMM: a tile takes 256 / permA wavelengths of each of permA neighbouring beta columns (0: 256 consecutive rows)
    long ksteps[4] = {0, 0, 0, 0};
    DevBuf<unsigned> amax;                          // [2][NP] max |row| of the data operands: Xs (forward), ymat (adjoint)
    DevBuf<unsigned> pmax;                          // per-wave maxima of the kernel that wrote the operand (reduced into amax)
    DevEll fwd, adjT, adjRef;
    HostEll adjT_host;                  // kept until the grouped scatter table is built (plan creation)
    bool has_ref = false;
    bool bsum = false;   // no spectral blur: y[l][(p,s,a)] = sum over the slit's beta columns (MRSBlurred)
    DevBuf<float> wmat;                 // data weights of the channel in ymat's layout [NP][LdetP], padding zero (channels with ymat16; surfh_set_data_weights)
};

struct ProfRec {
    const char *name;
    hipEvent_t a, b;
};

// ---- the route of a plan: which transform kernels run and which fusions ride on them, decided in one place (decide_route, plan.hip).
// Operators read its fields, never the buffers, to learn their mode.  DESIGN.md ("The route of a plan"): what sets each field and
// which stages it switches.
enum AxisKernel { AX_DENSE = 0, AX_H2 = 1, AX_CT = 2 };                 // dense fp32 products, dft_h2.h, dft_ct.h
enum OtfSupport { OTF_NONE = 0, OTF_LISTS = 1, OTF_LISTS_RANGES = 2 };
// the SURFH_<name> switches that feed the route, in the order of the bits of RouteInput::switches (and of surfh_route_decide)
enum RouteSwitch { SW_DFT_H2, SW_DFT_CT, SW_DFT_DENSE, SW_NO_FUSED_MIX, SW_ADJ_FUSED, SW_OTF_PROD, SW_OTF_SUPPORT, SW_OTF_RANGES, SW_COUNT };
struct RouteInput {
    int Na = 0, Nb = 0, T = 0, exact = 0;         // exact: surfh_config.exact
    long NAP = 0, KBP = 0, LP = 0;
    bool verify = false, has_sotf = false;
    unsigned switches = 0;
    bool on(RouteSwitch s) const { return (switches >> s & 1u) != 0; }
};
struct Route {
    AxisKernel ax_a = AX_DENSE, ax_b = AX_DENSE;      // the kernel of each axis; both or neither DENSE
    bool mix = false;              // forward: spectral mix x OTF in the loader of the first inverse pass
    bool prod = false;             // plane-wise plans: the OTF products in the loader of the first inverse pass
    bool fused_tail = false;       // adjoint: conj(OTF) x and the reduction over the wavelengths inside the last forward pass
    bool scan_otf = false;         // plan creation looks for the OTF's support; what it finds completes the route:
    OtfSupport support = OTF_NONE; // the mix loader and the adjoint's tail pass over the super-tiles (LISTS) and the k-steps / rows (RANGES) outside
    bool tpl_spectral = false;     // template transpose: reduction over the frequency bins (else over the pixels)
    bool spec_calls = false;       // spectral-domain entry points available (surfh_spec_supported adds the run-time prior_kind)
    bool interleaved() const { return ax_a != AX_DENSE; }
    bool any_ct() const { return ax_a == AX_CT || ax_b == AX_CT; }
};
Route decide_route(const RouteInput &in, OtfSupport scan);
// the fields as integers, in the order surfh_route_decide and surfh_debug_dims("route" / "route2") report them
inline void route_fields(const Route &r, int64_t f[8]) {
    const int64_t v[8] = {r.ax_a, r.ax_b, r.mix, r.prod, r.fused_tail, r.support, r.tpl_spectral, r.spec_calls};
    std::copy(v, v + 8, f);
}

}  // namespace surfh_impl

using namespace surfh_impl;      // struct surfh_plan is the C ABI's opaque type and stays at global scope

// The plan's streams and events, as a base class of the plan: a base is destroyed after the members of the derived class, so
// `delete p` frees every device buffer (the DevBuf members below) first and destroys the events and streams last -- the order
// surfh_plan_destroy has always kept.  A destructor body of surfh_plan would run BEFORE its members and reverse it.
struct PlanHandles {
    int dev = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // second stream: the spectral-blur GEMMs run here while the gather / scatter of the neighbouring channel runs on
    // `stream` (different units: matrix cores vs L2 bandwidth, and the GEMM leaves registers for them on every SIMD)
    hipStream_t stream2 = nullptr;
    std::vector<hipEvent_t> sync_ev;             // dependency events between the two streams (no timing)
    std::vector<ProfRec> pending;                // profiling: recorded stage brackets, and events free for reuse
    std::vector<hipEvent_t> pool;
    PlanHandles() = default;
    PlanHandles(const PlanHandles &) = delete;
    PlanHandles &operator=(const PlanHandles &) = delete;
    ~PlanHandles() {
        for (auto &r : pending) {
            hipEventDestroy(r.a);
            hipEventDestroy(r.b);
        }
        for (hipEvent_t e : pool) hipEventDestroy(e);
        for (hipEvent_t e : sync_ev) hipEventDestroy(e);
        if (stream2) hipStreamDestroy(stream2);
        if (own_stream && stream) hipStreamDestroy(stream);
    }
};

struct surfh_plan : PlanHandles {
    bool overlap = false;
    size_t sync_next = 0;
    int Na = 0, Nb = 0, Lc = 0, T = 0, NAP = 0, NBP = 0, KAP = 0, KBP = 0;
    long PL = 0, PLc = 0;
    int lo = 0, hi = 0, Lown = 0, LP = 0;
    int Leff = 0;                                // planes the trimmed transform passes run over (SURFH_LAMBDA_TRIM=0: LP)
    // owned cube planes = union of the channels' windows, stored compactly: segment = (first plane, length, compact offset)
    struct Seg { int start, len, coff; };
    std::vector<Seg> segs;
    std::vector<int> planes;   // compact index -> cube plane
    int compact(int l) const {
        for (auto &g : segs) if (l >= g.start && l <= g.start + g.len) return g.coff + (l - g.start);
        return -1;
    }
    // device memory: every DevBuf member owns its buffer (dev_buf.h); the few raw device pointers left are views and say so
    DevBuf<float> sotf, tpl, mhat, spec, ycol, cube, maps_pad, ycol_maps;
    DevBuf<float> Fi, Gi, Gf, Ff, GiT, GfT;
    // folded-DFT matrices [MPx][KPx]: cos/sin along alpha; weighted cos/sin for c2r; plain cos/sin for r2c
    DevBuf<float> Cma, Sma, Gc, Gs, Cf, Sf;
    int MPa = 0, KPa = 0, MPb = 0, KPb = 0;
    int n_cu = 256;
    bool gather_sorted = true;                   // gather rows ordered by cube location (L2 reuse across pointings)
    bool gemm_grouped = true;                    // the adjoint's spectral-blur GEMMs of up to four channels as one launch (SURFH_GEMM_GROUPED=0: one each)
    bool scatter_grouped = true;                 // adjoint scatter with SCATTER_G neighbouring pixels per workgroup (GroupTable)
    bool gather_grouped = true;                  // forward gather (fp16 output) likewise
    bool wblur_fp32 = false;
    // surfh_config.verify: every long sum accumulated in float64 (dense DFT products, spectral blur, adjoint spectral mix,
    // gather / scatter rows) -- the strict dot test; storage stays fp32
    bool verify = false;
    int prior_kind = 0;                          // 0: separated first differences (NpDiff_r / NpDiff_c); 1: joint Laplacian (surfh_set_prior)
    // surfh_set_potential: the potential of the spatial prior (maps, planes, the cube's rows / columns), of the cube's spectral
    // prior and of the robust data term; 0 Huber, 1 hyperbolic, 2 Hebert-Leahy (huber_dev.h)
    int pot[3] = {0, 0, 0};
    // surfh_set_prior_coupling: how the maps' spatial prior groups its differences; 0 none (one potential per difference),
    // 1 isotropic, 2 vector (coupled_prior.hip)
    int coupling = 0;
    // which transform kernels run and which fusions ride on them: written once, by surfh_plan_create from decide_route.  On an
    // interleaved route the plan's complex arrays (sotf, spec, ycol*, and mhat when T == 0) are [..][LP][2] instead of planar [2][..][LP]
    Route route;
    DevBuf<unsigned short> h2img;                // dft_h2's three LDS images: (Cma, Sma), (Gc, Gs), (Cf, Sf)
    DftCtPlan ctA, ctB_own;                      // dft_ct: transform lengths Na / Nb; ctB_own stays empty when they are equal
    const DftCtPlan *ctB = &ctB_own;             // view: the plan that serves beta (&ctA when Nb == Na)
    // cube columns alpha in [a_lo, a_hi) hold every pixel any channel's tables touch: the transform passes that are batched
    // over alpha skip the rest (forward: the cube outside is never read; adjoint: it is zero).  ycol_adj: the adjoint's
    // intermediate in its own buffer (interleaved routes with a proper sub-range), whose columns outside stay zero from plan creation on.
    int a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;  // (b: the same for the cube rows beta)
    DevBuf<float> ycol_adj;
    DevBuf<float> adjmix_part;                   // route.fused_tail: partial sums per (k_beta, slot) of dft_h2_adjmix_kernel
    // route.support (otf_support, plan.hip): the list of super-tiles k_beta * (LP / 128) + chunk inside the OTF's support,
    // otf_kbstart[kb] = first list position of kb; ycol_mix: the forward's intermediate, whose other tiles stay zero from plan
    // creation on; otf_tabs (LISTS_RANGES): per chunk of 128 wavelengths the k-steps / last rows inside the support, [3 or 4][LP / 128]
    DevBuf<int> otf_vlist, otf_kbstart;
    int otf_nvalid = 0;
    DevBuf<int> otf_tabs;
    DevBuf<float> ycol_mix;
    int h2kA[3] = {0, 0, 0};
    DevBuf<float> io_x, io_y, io_cube, hth, mhat2;
    // accumulator of the exact adjoint: cleared ONCE at plan creation.  Every scatter row knows which of its wavelengths an
    // earlier channel has already written in the same pass (read-modify-write) and stores the others, so nothing stale
    // survives a pass and no per-call clear is needed (nullptr: the tables could not express that -- clear `cube` every call)
    DevBuf<float> gcube;
    std::vector<Channel> ch;
    long isize = 0, osize = 0;
    // data weights (surfh_set_data_weights): w [osize] in the layout of y, and room for W y, the data of the solvers' right-hand side;
    // both null = every sample counts 1
    DevBuf<float> dw, dwy;
    // imager data term (surfh_set_imager, surfh_set_imager_data): G [F][T][2][KAP][KBP] and the work buffers of an application --
    // padded maps / images and their half spectra -- then the data y_im, w_im (null: 1) and W y_im [im_osize]; im_g null = no imager
    int im_F = 0, im_d = 0;
    long im_osize = 0;
    DevBuf<float> im_g, im_xpad, im_xhat, im_zpad, im_zhat, im_io;
    DevBuf<float> im_y, im_w, im_wy;
    double im_mu = 0.0;
    int ycm_planes = 0;                            // planes ycol_maps holds (max(T, 1); max(T, F) once an imager has been attached)
    std::vector<double> tpl_host;                  // the templates [T][Lc] as given (the imager's streamed set-up reads them)
    // template refinement (tplgrad.h; surfh_set_templates, surfh_adjoint_templates, surfh_cg_templates), allocated by tpl_ensure:
    // cube plane -> compact plane index [Lc] and back [LP] (-1: none), the slabs' partial sums, the plan's own templates [T][LP]
    // while a call has others in their place (TplScope), and the solver's vectors [T][Lc] in cube-plane order: x, r, d, q, b, staging
    DevBuf<int> tg_cidx, tg_pidx;
    DevBuf<double> tg_part;
    DevBuf<float> tg_keep, tg_v[6];
    // inside one template solve: mhat holds the spectra of the solve's maps (cleared whenever something else may have used mhat);
    // only the tpl_* callers consult it, to choose the head of their operator calls
    bool tg_mhat_ready = false;
    // CG
    DevBuf<float> cg_x, cg_r, cg_d, cg_q, cg_b, cg_y, cg_qm, cg_dd;
    DevBuf<float> cg_hg;                           // surfh_mmmg_huber(_vox): -gradient of the non-quadratic criterion
    DevBuf<float> cpl_w;                           // coupled prior: the weight field of the current iterate [isize], allocated on first use
    DevBuf<float> rb_y, rb_u, rb_ag, rb_am;       // surfh_mmmg_robust(_vox): y, A x, A (-g), A m [osize]
    DevBuf<double> dscal, dscratch;                 // [16] device scalars, partial sums (>= 1024, and what huber_vox.hip and robust_data.hip ask for)
    // posterior sampling (surfh_cg_sample): y, the noise vectors eps_y [osize], eps_r / eps_c [isize], eta and the unperturbed
    // solution [isize]; the moment sums (posterior.hip).  surfh_cg_planes_sample (T = 0) holds po_eta, po_xhat and po_S [2 isize]
    // only; its staging buffers po_eps, po_er / po_ec come with a caller's explicit draws, po_y with surfh_po_planes_rhs
    DevBuf<float> po_y, po_eps, po_er, po_ec, po_eta, po_xhat;
    DevBuf<double> po_S;
    // non-negative fusion (surfh_cg_nonneg, surfh_cg_templates_nonneg), allocated for one solve (NnScope): the split variable, the
    // scaled dual and a work vector
    DevBuf<float> nn_z;
    float *nn_u = nullptr, *nn_w = nullptr;        // views: the second and third thirds of nn_z
    // ... on independent planes (surfh_cg_planes_nonneg): the penalties [Lc], the partial sums of nn_project_planes and, behind
    // them, its sums [4][Lc] (view)
    DevBuf<float> nn_rho;
    DevBuf<double> nn_part;
    double *nn_sums = nullptr;
    DevBuf<double> cg_hist;                        // device-resident r.r trace of the no-host-sync CG blocks (CG_HIST_CAP entries)
    int cg_hist_n = 0;
    // plane-wise CG with device-resident data (surfh_cg_planes_begin_dev / _step_dev): per-plane scalars [3][Lc] (the host-buffer
    // plane-wise solvers use them too), the caller's iterate
    DevBuf<double> pl_sc;
    DevBuf<double> pl_hsc;                         // surfh_mmmg_huber_planes: [HUBER_PLANES_SCALARS][Lc] per-plane scalars
    DevBuf<double> pl_hpar;                        // ... and [HUBER_PLANES_PARAMS][Lc] per-plane coefficient, delta, mu_reg of a call
    float *pl_x = nullptr;                         // view: the caller's device vector, never freed here
    double pl_mu = 1.0, pl_mu_reg = 0.0;
    int pl_it = 0;
    // ... with its vectors in the cube's wavelength-innermost layout [NBP][NAP][LP] (no layout transpose inside an iteration):
    // x, r, d, q, b; per-wavelength scalars [3][LP] + partial sums; pn_active: the solve surfh_cg_planes_begin_dev began runs on them
    DevBuf<float> pn_v[5];
    DevBuf<double> pn_sc, pn_part;
    bool pn_active = false;
    // profiling
    bool prof = false;
    std::string prof_filter;                     // non-empty: only stages whose name starts with it are bracketed by events
    std::map<std::string, std::pair<long, double>> acc;
    std::vector<std::string> acc_names;
};

namespace surfh_impl __attribute__((visibility("hidden"))) {

struct Prof {
    surfh_plan *p;
    ProfRec r;
    bool on;
    hipStream_t st;
    Prof(surfh_plan *pl, const char *name, hipStream_t stream = nullptr) : p(pl), on(pl->prof), st(stream ? stream : pl->stream) {
        if (on && !pl->prof_filter.empty() && strncmp(name, pl->prof_filter.c_str(), pl->prof_filter.size()) != 0) on = false;
        if (!on) return;
        r.name = name;
        for (hipEvent_t *e : {&r.a, &r.b}) {
            if (!p->pool.empty()) {
                *e = p->pool.back();
                p->pool.pop_back();
            } else {
                hipEventCreate(e);
            }
        }
        hipEventRecord(r.a, st);
    }
    ~Prof() {
        if (!on) return;
        hipEventRecord(r.b, st);
        p->pending.push_back(r);
    }
};

// ---- the two ends of one operator call ------------------------------------------------------------------------------------------
// forward_dev reads `head`, adjoint_dev reads `tail`, normal_halves hands both on; the defaults are the plain call on the caller's
// vectors.  DESIGN.md ("Heads and tails of an operator call") lists which entry point uses which pair.
struct OpCall {
    enum Head {
        H_CALLER,        // x in the caller's layout: the maps as pixels [T][Na][Nb], plane-wise plans (T = 0) the planes [Lc][Na][Nb]
        H_SPECTRA,       // `spectra_in`: the caller's Parseval-scaled half spectra of the maps, read by the mix loader; x is not read
        H_MHAT,          // mhat holds the maps' spectra already (inside a template solve); x is not read
        H_CUBE           // T = 0: x in the cube's wavelength-innermost layout [NBP][NAP][LP]
    } head = H_CALLER;
    enum Tail {
        T_CALLER,        // x in the caller's layout, as H_CALLER
        T_SPECTRA,       // `spectra_out` = mu * scaled half spectra (+ prior_mu |D|^2 prior_src, the quadratic prior); x is not written
        T_TEMPLATES,     // the transpose with respect to the templates: `tpl_out` [T][Lc]; `tpl_maps`: the maps on the device
        T_CUBE           // T = 0: x in the cube's wavelength-innermost layout
    } tail = T_CALLER;
    const float *spectra_in = nullptr;
    float *spectra_out = nullptr, *tpl_out = nullptr;
    const float *prior_src = nullptr, *tpl_maps = nullptr;
    // T_SPECTRA, and the T = 0 tails under `fold` -- there mu and the quadratic prior of the plane-wise normal operator go into the
    // adjoint's OTF product: q = mu A^T A v + prior_mu D^T D v, the spectrum of v still in mhat from the forward half
    double mu = 1.0, prior_mu = 0.0;
    bool fold = false;
    bool ref = false;          // adjoint: the reference's interpolating back-projection (surfh_adjoint_ref)
    // forward: the caller is the normal operator -- channels with a spectral-blur GEMM do not write y but leave the adjoint's GEMM
    // operand (fp16 pieces of ymat + row maxima) behind; adjoint: the forward half has just done so.  normal_halves sets it.
    bool hand_over = false;
};

// ---- helpers that cross a file boundary (default arguments live here) --------------------------------------------------------
// plan.hip
int chain(surfh_plan *p, hipStream_t from, hipStream_t to);
void prof_collect(surfh_plan *p);
int build_klist(const float *B, int N, int K, long ldb, int segLinP, int segChunks, double tol1, double tol2, std::vector<int> *out,
                int *stride, long *n_near, long *n_far, int permP = 0, int permLin = 0);
// plan_ops.hip
int prior_add(surfh_plan *p, hipStream_t st, const float *d, float *q, int n_img, float mu_reg);
int forward_dev(surfh_plan *p, const float *x, float *y, const OpCall &c = {});
int adjoint_dev(surfh_plan *p, const float *y, float *x, const OpCall &c = {});
int normal_halves(surfh_plan *p, const float *v, float *q, OpCall c = {});        // A^T W A v, head and tail those of `c`
const float *weighted_data(surfh_plan *p, const float *y);
int normal_dev(surfh_plan *p, const float *d, float *q, double mu, bool cube = false);     // mu A^T W A d; cube: T = 0 vectors in the cube's layout
int ensure_cg(surfh_plan *p);
inline bool imager_active(const surfh_plan *p) { return p->im_g && p->im_y && p->im_mu > 0.0; }
int imager_normal_add(surfh_plan *p, const float *v, float *q);      // q += mu_imager A_im^T W_im A_im v
int imager_rhs_add(surfh_plan *p, float *b);                         // b += mu_imager A_im^T W_im y_im
// template refinement: S, G [T][Lc] floats on the device in cube-plane order, maps [T][Na][Nb] on the device
int tpl_ensure(surfh_plan *p);                                       // checks the plan (templates, channels) and allocates
int tpl_maps_spectra(surfh_plan *p, const float *maps);              // mhat = the maps' half spectra
int tpl_install(surfh_plan *p, const float *S);                      // p->tpl = S in the plan's compact, padded rows
struct TplScope {                                                    // the plan's own templates come back on every exit (begin() saves them)
    surfh_plan *p;
    bool armed = false;
    explicit TplScope(surfh_plan *pl) : p(pl) {}
    int begin();
    ~TplScope();
};
int tpl_normal_dev(surfh_plan *p, const float *maps, float *G);      // G = A_x^T W A_x (the installed templates)
int tpl_adjoint_dev(surfh_plan *p, const float *maps, const float *u, float *G);       // G = A_x^T u

}  // namespace surfh_impl
