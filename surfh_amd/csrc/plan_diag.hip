// Host side of the C ABI (include/surfh_amd.h), diagnostics: the profiler's read-out, the debug accessors, and the self-tests of
// the K-step classifier, the 2x2 step solve and the GEMMs.  Depends on the other three files; nothing depends on it.
// Plan struct and data layout: plan_internal.h.
#include "plan_internal.h"
#include "mm_step.h"

extern "C" {

// ---- instrumentation ------------------------------------------------------------------------
int surfh_profile_enable(surfh_plan *p, int32_t on) {
    if (!p) return fail("null plan");
    p->prof = on != 0;
    return 0;
}
int surfh_profile_filter(surfh_plan *p, const char *prefix) {
    if (!p) return fail("null plan");
    p->prof_filter = prefix ? prefix : "";
    return 0;
}
int32_t surfh_profile_count(surfh_plan *p) {
    if (!p) return -1;
    hipSetDevice(p->dev);
    prof_collect(p);
    return (int32_t)p->acc_names.size();
}
int surfh_profile_get(surfh_plan *p, int32_t i, const char **name, int64_t *launches, double *ms) {
    if (!p || i < 0 || i >= (int32_t)p->acc_names.size()) return fail("bad profile index");
    auto &e = p->acc[p->acc_names[i]];
    *name = p->acc_names[i].c_str();
    *launches = e.first;
    *ms = e.second;
    return 0;
}
int surfh_profile_reset(surfh_plan *p) {
    if (!p) return fail("null plan");
    hipSetDevice(p->dev);
    prof_collect(p);
    p->acc.clear();
    p->acc_names.clear();
    return 0;
}

static int resolve(surfh_plan *p, const char *which, const float **ptr, int64_t dims[4]) {
    std::string w(which ? which : "");
    dims[0] = dims[1] = dims[2] = dims[3] = 1;
    *ptr = nullptr;
    if (w == "blurred" || w == "gcube") {          // [beta][alpha][lambda]; the exact adjoint's accumulator may be its own buffer
        *ptr = (w == "gcube" && p->gcube) ? p->gcube : p->cube; dims[0] = p->NBP; dims[1] = p->NAP; dims[2] = p->LP;
    } else if (w == "spec") {                       // [2][k_alpha][k_beta][lambda]; h2 plans: [k_alpha][k_beta][lambda][2]
        *ptr = p->spec;
        if (p->route.interleaved()) { dims[0] = p->KAP; dims[1] = p->KBP; dims[2] = p->LP; dims[3] = 2; }
        else { dims[0] = 2; dims[1] = p->KAP; dims[2] = p->KBP; dims[3] = p->LP; }
    } else if (w == "mhat" && p->T > 0) {
        *ptr = p->mhat; dims[0] = p->T; dims[1] = 2; dims[2] = p->KAP; dims[3] = p->KBP;
    } else if (w == "hth" && p->T > 0) {            // Model_WCT's Hessian [t][t'][k_alpha][k_beta]; no pointer before its first use
        *ptr = p->hth; dims[0] = p->T; dims[1] = p->T; dims[2] = p->KAP; dims[3] = p->KBP;
    } else if (w == "imager_g" && p->im_g) {        // [(f,t)][2][k_alpha][k_beta]
        *ptr = p->im_g; dims[0] = (int64_t)p->im_F * p->T; dims[1] = 2; dims[2] = p->KAP; dims[3] = p->KBP;
    } else if (w.rfind("xs:", 0) == 0 || w.rfind("xsinfo:", 0) == 0) {
        const bool info = w[2] == 'i';
        const int c = atoi(w.c_str() + (info ? 7 : 3));
        if (c < 0 || c >= (int)p->ch.size()) return fail("bad channel index");
        if (info) {                                 // (LinP, first valid lambda column, n_beta_slit, Lin)
            dims[0] = p->ch[c].LinP; dims[1] = p->ch[c].shift; dims[2] = p->ch[c].nbs; dims[3] = p->ch[c].Lin;
        } else {                                    // [(p,s,a)][b'][LinP]
            Channel &ch = p->ch[c];
            if (ch.Xs16) {     // the forward operand lives as block-scaled fp16 pieces: rebuilt in fp32 for inspection
                if (launch_dequant_f16x2(p->stream, ch.Xs16, (long)ch.NP * ch.K, ch.bscale, ch.Xs, ch.NP, ch.K, ch.LinP,
                                         (ch.LinP + 1023) / 1024))
                    return fail("dequant launch failed");
                if (hipStreamSynchronize(p->stream) != hipSuccess) return fail("dequant failed");
            }
            *ptr = p->ch[c].Xs; dims[0] = p->ch[c].NP; dims[1] = p->ch[c].bsum ? 1 : p->ch[c].nbs; dims[2] = p->ch[c].LinP;
        }
    } else if (w == "range") {         // cube columns / rows the channels' tables touch: [a_lo, a_hi) x [b_lo, b_hi)
        dims[0] = p->a_lo; dims[1] = p->a_hi; dims[2] = p->b_lo; dims[3] = p->b_hi;
    } else if (w == "otf") {           // super-tiles (k_beta, 128 wavelengths) inside the OTF's support / all of them
        dims[1] = (long)(p->Nb / 2 + 1) * (p->LP / 128); dims[0] = p->otf_nvalid ? p->otf_nvalid : dims[1];
    } else if (w == "ksteps") {        // (tile, K step) pairs of the spectral-blur GEMMs: near / far of the forward, near / far of the adjoint
        for (auto &c : p->ch)
            for (int i = 0; i < 4; ++i) dims[i] += c.ksteps[i];
        for (int i = 0; i < 4; ++i) dims[i] -= 1;
    } else if (w == "groups") {        // workgroups of the grouped gather / grouped scatter tables, all channels (0: row by row)
        dims[0] = dims[1] = 0;
        for (auto &c : p->ch) { dims[0] += c.fwd.g.NG; dims[1] += c.adjT.g.NG; }
    } else if (w == "dft") {           // kernel of each transform axis (0: dense, 1: dft_h2, 2: dft_ct), interleaved arrays, fused adjoint tail
        dims[0] = p->route.ax_a; dims[1] = p->route.ax_b; dims[2] = p->route.interleaved(); dims[3] = p->route.fused_tail;
    } else if (w == "route" || w == "route2") {       // the plan's route, in the order surfh_route_decide reports it: fields 0-3, 4-7
        int64_t f[8];
        route_fields(p->route, f);
        for (int i = 0; i < 4; ++i) dims[i] = f[(w == "route2" ? 4 : 0) + i];
    } else if (w == "trim") {         // planes the fused transform passes run over, the plane pitch, owned planes
        dims[0] = p->Leff; dims[1] = p->LP; dims[2] = p->Lown;
    } else if (w == "info") {
        dims[0] = p->lo; dims[1] = p->hi; dims[2] = p->Lown; dims[3] = (int64_t)p->segs.size();
    } else {
        return fail("unknown debug buffer '%s'", w.c_str());
    }
    return 0;
}

int surfh_debug_dims(surfh_plan *p, const char *which, int64_t dims[4]) {
    if (!p) return fail("null plan");
    const float *ptr;
    return resolve(p, which, &ptr, dims);
}

int64_t surfh_debug_copy(surfh_plan *p, const char *which, float *out, int64_t cap) {
    if (!p || !out) return -1;
    const float *ptr = nullptr;
    int64_t d[4];
    if (resolve(p, which, &ptr, d) || !ptr) return -1;
    const int64_t n = d[0] * d[1] * d[2] * d[3];
    if (n > cap) {
        fail("capacity %lld < %lld", (long long)cap, (long long)n);
        return -1;
    }
    hipSetDevice(p->dev);
    hipStreamSynchronize(p->stream);
    if (hipMemcpy(out, ptr, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}

int32_t surfh_klist_classify(const float *B, int32_t n, int32_t k, int64_t ldb, int32_t perm_p, int32_t perm_lin, int32_t *records,
                             int64_t capacity) {
    if (!B || !records || n < 1 || k < 32 || k % 32 || ldb < k) return -fail("surfh_klist_classify: bad arguments");
    if (perm_p && ((perm_p != 1 && perm_p != 2 && perm_p != 4 && perm_p != 8) || perm_lin < 1 || perm_lin % (256 / perm_p) || n % perm_lin))
        return -fail("surfh_klist_classify: bad tile shape");
    std::vector<int> kl;
    int stride = 0;
    long nn = 0, nf = 0;
    build_klist(B, n, k, ldb, 0, 0, 1.0 / 256, 1.0 / 1024, &kl, &stride, &nn, &nf, perm_p, perm_lin);
    if ((int64_t)kl.size() > capacity) return -fail("surfh_klist_classify: capacity too small");
    std::memcpy(records, kl.data(), kl.size() * sizeof(int));
    return (int32_t)(kl.size() / (size_t)stride);
}

int surfh_route_decide(int32_t n_alpha, int32_t n_beta, int32_t n_templates, int64_t lp, int32_t verify, int32_t exact, int32_t has_sotf,
                       uint32_t switches, int32_t scan, int64_t out[8]) {
    if (!out || n_alpha < 2 || n_beta < 2 || n_templates < 0 || lp < 128 || lp % 128 || scan < 0 || scan > 2) return fail("surfh_route_decide: bad arguments");
    RouteInput in;
    in.Na = n_alpha; in.Nb = n_beta; in.T = n_templates; in.NAP = pad64(n_alpha); in.KBP = pad64(n_beta / 2 + 1); in.LP = lp;
    in.verify = verify != 0; in.has_sotf = has_sotf != 0; in.exact = exact; in.switches = switches;
    route_fields(decide_route(in, (OtfSupport)scan), out);
    return 0;
}

int surfh_launch_geometry(const char *which, int64_t a, int64_t b, int64_t c, int64_t out[4]) {
    if (!which || !out) return fail("null argument");
    const std::string w(which);
    const auto trips = [](int64_t items, int64_t blocks) { return (items + blocks * VEC_TPB - 1) / (blocks * VEC_TPB); };
    const auto flat = [&](int64_t grid, int64_t parts, int64_t items) {
        out[0] = grid; out[1] = 1; out[2] = parts; out[3] = trips(items, grid);
    };
    const bool cube = w == "huber_maps" || w == "huber_vox";
    if (a < 1 || (cube && (b < 1 || c < 1 || a > INT32_MAX || b > INT32_MAX || c > INT32_MAX || b * c > INT32_MAX)))
        return fail("surfh_launch_geometry: bad size (%lld, %lld, %lld)", (long long)a, (long long)b, (long long)c);
    if (w == "dot") {                     // dot_partial, cg_step, cg_step_parts: one partial per block
        const int g = nblocks(a, DOT_BLOCKS);
        flat(g, g, a);
    } else if (w == "cg_axpy") {          // cg_dir, cg_xupdate, residual
        flat(nblocks(a), 0, a);
    } else if (w == "cg_dir_parts") {     // every block sums the partials of the dot kernel before it
        flat(nblocks(a), nblocks(a, DOT_BLOCKS), a);
    } else if (w == "po_data") {
        flat(grid_for(a), 0, a);
    } else if (w == "robust") {           // the vector loop; the a % b floats behind it go one to a thread
        if (b != 1 && b != 2 && b != 4) return fail("surfh_launch_geometry: V = %lld", (long long)b);
        const unsigned g = rob_grid(a, (int)b);
        flat(g, g, a / b);
    } else if (w == "nn_project") {       // likewise: groups of four on the 16-byte path
        const unsigned g = nn_project_grid(a, b == 1);
        flat(g, g, b == 1 ? a / 4 : a);
    } else if (w == "huber_maps") {
        const int g = nblocks(a * b * c, HUBER_BLOCKS);
        flat(g, g, a * b * c);
    } else if (w == "huber_vox") {        // chunk k owns planes [a k / C, a (k + 1) / C): the longest has ceil(a / C)
        const dim3 g = march_grid((int)a, (int)b, (int)c);
        out[0] = g.x; out[1] = g.y; out[2] = (int64_t)g.x * g.y; out[3] = (a + g.y - 1) / g.y;
    } else {
        return fail("surfh_launch_geometry: unknown kernel family '%s'", which);
    }
    return 0;
}

// ---- the plane-wise posterior sampler's kernels on their own (posterior.hip; the loop: surfh_cg_planes_sample) ----
// One fused perturbation kernel on a device array of explicit extents, through the sampler's launcher; the plan gives its stream only.
int surfh_debug_po_planes(surfh_plan *p, const char *which, int32_t L, int32_t na, int32_t nb, int64_t n_out, uint64_t seed, int32_t sample,
                          double mu, double mu_reg, const float *w_dev, float *out_dev) {
    const char *who = "surfh_debug_po_planes";
    if (!p || !which || !out_dev) return fail("null argument");
    if (sample < 0) return fail("%s: sample = %d", who, (int)sample);
    const std::string w(which);
    HIP_OK(hipSetDevice(p->dev));
    if (w == "eta") {
        if (L < 1 || na < 1 || nb < 1 || (double)L * (double)na * (double)nb > 2147483647.0)
            return fail("%s: eta on %d planes of %d x %d", who, (int)L, (int)na, (int)nb);
        if (!(mu_reg >= 0.0 && mu_reg <= DBL_MAX)) return fail("%s: mu_reg = %g must be finite and >= 0", who, mu_reg);
        Prof pr(p, "po_planes_eta");
        LAUNCH_OK(launch_po_planes_eta(p->stream, out_dev, L, na, nb, (float)std::sqrt(mu_reg), seed, (uint32_t)sample));
    } else if (w == "data") {
        if (n_out < 0) return fail("%s: n_out = %lld", who, (long long)n_out);
        if (!(mu > 0.0 && mu <= DBL_MAX)) return fail("%s: mu = %g must be finite and > 0", who, mu);
        Prof pr(p, "po_planes_data");
        LAUNCH_OK(launch_po_planes_data(p->stream, w_dev, out_dev, (long)n_out, (float)mu, seed, (uint32_t)sample));
    } else {
        return fail("%s: unknown kernel '%s' (eta, data)", who, which);
    }
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

// The plane moments on host buffers: K samples [K][L][npix] about xhat [L][npix]; mean [L][npix] and var [L][npix] (NULL: not wanted;
// needs K >= 2) in float64 -- the accumulation and the in-place finish of surfh_cg_planes_sample.
int surfh_po_planes_moments(int32_t L, int64_t npix, const float *xhat, const float *samples, int32_t K, double *mean, double *var,
                            int32_t device) {
    if (!xhat || !samples || !mean) return fail("null argument");
    if (L < 1 || npix < 1 || K < 1) return fail("plane moments: L = %d, npix = %ld, K = %d", (int)L, (long)npix, (int)K);
    if (var && K < 2) return fail("plane moments: a variance needs at least 2 samples (got %d)", (int)K);
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)L * npix;
    DevBuf<float> dx, dh;
    DevBuf<double> S;
    if (dx.alloc(n) || dh.alloc(n) || S.alloc(2 * n)) return 1;
    HIP_OK(hipMemcpy(dh, xhat, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(S, 0, 2 * n * sizeof(double)));
    for (int k = 0; k < K; ++k) {
        HIP_OK(hipMemcpy(dx, samples + (size_t)k * n, n * sizeof(float), hipMemcpyHostToDevice));
        LAUNCH_OK(launch_po_planes_moments(nullptr, dx, dh, S, S + n, (long)n));
    }
    LAUNCH_OK(launch_po_planes_finish(nullptr, dh, S, S + n, (long)n, K, var ? 1 : 0));
    HIP_OK(hipMemcpy(mean, S, n * sizeof(double), hipMemcpyDeviceToHost));
    if (var) HIP_OK(hipMemcpy(var, S + n, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int surfh_mm_step2(double dBd, double dBm, double mBm, double dg, double mg, double step[2]) {
    if (!step) return fail("null argument");
    mm_step2(dBd, dBm, mBm, dg, mg, &step[0], &step[1]);
    return 0;
}

static long g_selftest_ksteps[2] = {0, 0};
int surfh_gemm_selftest_ksteps(int64_t near_far[2]) {
    near_far[0] = g_selftest_ksteps[0]; near_far[1] = g_selftest_ksteps[1];
    return 0;
}

// SURFH_SELFTEST_REPEAT=<n>: the two-piece fp16 launch of the self-test is repeated n times behind three warm-up launches,
// bracketed by device events; mean milliseconds per launch of the last such call (-1: none)
static double g_selftest_ms = -1.0;
int surfh_gemm_selftest_ms(double *ms) {
    if (!ms) return fail("null argument");
    *ms = g_selftest_ms;
    return 0;
}

int surfh_gemm_selftest(int32_t device, int32_t M, int32_t N, int32_t K, int32_t split_k, const float *A,
                        const float *B, float *C) {
    HIP_OK(hipSetDevice(device));
    DevBuf<float> dA, dB, dC;
    const int sk = std::max(1, (int)split_k);
    if (dA.alloc((size_t)M * K) || dB.alloc((size_t)K * N) || dC.alloc((size_t)sk * M * N)) return 1;
    HIP_OK(hipMemcpy(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dB, B, (size_t)K * N * 4, hipMemcpyHostToDevice));
    GemmArgs g;
    g.A0 = dA; g.lda = K; g.B0 = dB; g.ldb = N; g.C = dC; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.splitK = sk; g.sCsplit = (long)M * N;
    int rc;
    const char *mode = getenv("SURFH_SELFTEST_F16X2");
    if (mode && (mode[0] == '1' || mode[0] == '2')) {
        // two-piece fp16 kernel, NT form: B is handed over as [K][N]; transpose it on the host into [N][K]
        std::vector<float> bt((size_t)N * K);
        for (int k = 0; k < K; ++k)
            for (int n = 0; n < N; ++n) bt[(size_t)n * K + k] = B[(size_t)k * N + n];
        HIP_OK(hipMemcpy(dB, bt.data(), bt.size() * 4, hipMemcpyHostToDevice));
        g.ldb = K;
        DevBuf<unsigned short> dB16, dA16;       // two fp16 pieces per element
        DevBuf<unsigned> dmax;
        float amB = 0.f;
        for (float v : bt) amB = std::max(amB, std::fabs(v));
        std::vector<unsigned> rows((size_t)M, 0u);           // max |A[m][:]| as bit patterns
        for (int m = 0; m < M; ++m) {
            float am = 0.f;
            for (int k = 0; k < K; ++k) am = std::max(am, std::fabs(A[(size_t)m * K + k]));
            memcpy(&rows[m], &am, 4);
        }
        if (dB16.alloc(bt.size() * 2) || dmax.alloc(rows.size()) || dA16.alloc((size_t)M * K * 2)) return 1;
        HIP_OK(hipMemcpy(dmax, rows.data(), rows.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        g.sB16 = gemm_f16x2_scale(amB); g.B16 = dB16; g.pB16 = (long)bt.size(); g.amax = dmax;
        rc = launch_split2h(nullptr, dB, dB16, (long)bt.size(), (long)bt.size(), g.sB16);
        if (rc == 0) rc = launch_split_rows2h(nullptr, dA, dmax, dA16, M, K, (long)M * K);
        g.A3 = dA16; g.pA3 = (long)M * K;
        DevBuf<int> dkl;
        g_selftest_ksteps[0] = g_selftest_ksteps[1] = 0;
        if (mode[0] == '2') {      // with K-step lists, classes and tolerances as at plan creation
            std::vector<int> kl;
            // SURFH_SELFTEST_PERM=<rows per column of B>: tiles of 64 rows of four neighbouring columns, as the adjoint spectral-blur GEMM
            const char *ep = getenv("SURFH_SELFTEST_PERM");
            const int lin = ep ? atoi(ep) : 0;
            if (lin > 0) { g.permP = 4; g.permLin = lin; }
            build_klist(bt.data(), N, K, K, 0, 0, 1.0 / 256, 1.0 / 1024, &kl, &g.klistStride, &g_selftest_ksteps[0], &g_selftest_ksteps[1], g.permP,
                        g.permLin);
            if (dkl.upload(kl)) return 1;
            g.klist = dkl;
        }
        if (rc == 0) rc = launch_gemm_nt_f16x2_cc(nullptr, g);
        if (rc == 0) rc = (int)hipDeviceSynchronize();
        g_selftest_ms = -1.0;
        const char *er = getenv("SURFH_SELFTEST_REPEAT");
        const int nrep = er ? atoi(er) : 0;
        if (rc == 0 && nrep > 0) {
            hipEvent_t ea, eb;
            HIP_OK(hipEventCreate(&ea));
            HIP_OK(hipEventCreate(&eb));
            for (int i = 0; i < 3 && rc == 0; ++i) rc = launch_gemm_nt_f16x2_cc(nullptr, g);
            hipEventRecord(ea, nullptr);
            for (int i = 0; i < nrep && rc == 0; ++i) rc = launch_gemm_nt_f16x2_cc(nullptr, g);
            hipEventRecord(eb, nullptr);
            if (rc == 0) rc = (int)hipEventSynchronize(eb);
            float ms = 0.f;
            if (rc == 0) rc = (int)hipEventElapsedTime(&ms, ea, eb);
            if (rc == 0) g_selftest_ms = (double)ms / nrep;
            hipEventDestroy(ea);
            hipEventDestroy(eb);
        }
    } else {
        rc = launch_gemm_f32(nullptr, g);
    }
    if (rc == 0) rc = (int)hipDeviceSynchronize();
    std::vector<float> h((size_t)sk * M * N);
    if (rc == 0) rc = (int)hipMemcpy(h.data(), dC, h.size() * 4, hipMemcpyDeviceToHost);
    if (rc) return fail("gemm selftest failed: %s", hipGetErrorString((hipError_t)rc));
    for (size_t i = 0; i < (size_t)M * N; ++i) {
        float s = 0.f;
        for (int k = 0; k < sk; ++k) s += h[(size_t)k * M * N + i];
        C[i] = s;
    }
    return 0;
}

}  // extern "C"
