// Host side of the C ABI (include/surfh_amd.h), plan build and plan state: the error string, channel tables and K-step lists,
// DFT matrices, the OTF's support, surfh_plan_create / surfh_plan_destroy, the size queries, and the state a caller sets on a
// plan (prior, potentials, data weights).  Nothing here calls an operator or a solver.  The plan struct and the description of
// the data layout are in plan_internal.h; the operators are in plan_ops.hip, the solvers in plan_solvers.hip, the profiler and
// debug accessors in plan_diag.hip.
#include "plan_internal.h"

#include <atomic>

namespace surfh_impl {

namespace {
thread_local std::string g_err;
}

int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

// ---- the only two calls of hipMalloc / hipFree in the library (dev_buf.h), counted for surfh_debug_alloc_count ----------------------
namespace {
std::atomic<int64_t> g_alloc_live{0}, g_alloc_total{0}, g_alloc_fail_at{0};      // fail_at: value of `total` at which an allocation is refused (0: none)
}
int dev_raw_alloc(void **p, size_t bytes) {
    *p = nullptr;
    const int64_t nth = ++g_alloc_total;
    int64_t armed = nth;
    const hipError_t e = g_alloc_fail_at.compare_exchange_strong(armed, 0) ? hipErrorOutOfMemory : hipMalloc(p, bytes);
    if (e != hipSuccess) return fail("hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(Tp)) failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    ++g_alloc_live;
    return 0;
}
void dev_raw_free(void *p) {
    if (!p) return;
    hipFree(p);
    --g_alloc_live;
}
int dev_raw_upload(void *dst, const void *src, size_t bytes) {
    HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int dev_raw_clear(void *p, size_t bytes, hipStream_t stream, bool async) {
    if ((async ? hipMemsetAsync(p, 0, bytes, stream) : hipMemset(p, 0, bytes)) != hipSuccess) return fail("memset failed");
    return 0;
}

// make stream `to` wait for the work enqueued so far on stream `from`
int chain(surfh_plan *p, hipStream_t from, hipStream_t to) {
    if (from == to) return 0;
    if (p->sync_next == p->sync_ev.size()) {
        hipEvent_t e;
        HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        p->sync_ev.push_back(e);
    }
    hipEvent_t e = p->sync_ev[p->sync_next++];
    if (p->sync_next >= 64) p->sync_next = 0;       // ring: an event is re-recorded long after its waiters were enqueued
    HIP_OK(hipEventRecord(e, from));
    HIP_OK(hipStreamWaitEvent(to, e, 0));
    return 0;
}

void prof_collect(surfh_plan *p) {
    if (p->pending.empty()) return;
    hipStreamSynchronize(p->stream);
    if (p->stream2) hipStreamSynchronize(p->stream2);
    for (auto &r : p->pending) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.a, r.b);
        auto &e = p->acc[r.name];
        e.first += 1;
        e.second += ms;
        p->pool.push_back(r.a);
        p->pool.push_back(r.b);
    }
    p->pending.clear();
    p->acc_names.clear();
    for (auto &kv : p->acc) p->acc_names.push_back(kv.first);
}

namespace {

int upload_ell(const HostEll &h, DevEll *d) {
    const int R = (int)h.rows.size();
    int W = 1;
    for (auto &r : h.rows) W = std::max(W, (int)r.size());
    std::vector<int32_t> cnt(R);
    std::vector<int64_t> col((size_t)R * W, 0);
    std::vector<float> val((size_t)R * W, 0.f);
    for (int r = 0; r < R; ++r) {
        cnt[r] = (int32_t)h.rows[r].size();
        for (int e = 0; e < cnt[r]; ++e) {
            col[(size_t)r * W + e] = h.rows[r][e].first;
            val[(size_t)r * W + e] = h.rows[r][e].second;
        }
    }
    if (d->cnt.upload(cnt) || d->col.upload(col) || d->val.upload(val) || d->dst.upload(h.dst)) return 1;
    d->t.R = R;
    d->t.W = W;
    d->t.cnt = d->cnt;
    d->t.col = d->col;
    d->t.val = d->val;
    d->t.dst_off = d->dst;
    return 0;
}

// rows [r, r + n) of h taken as one group: union of their taps with one weight per member
int upload_groups(const HostEll &h, const std::vector<std::pair<size_t, size_t>> &runs, const std::vector<uint32_t> *mask, DevEll *d,
                  const int G, const std::vector<int2> *ranges = nullptr) {
    const size_t NG = runs.size();
    std::vector<std::vector<std::pair<int64_t, std::array<float, GROUP_MAX>>>> grows(NG);
    std::vector<int64_t> gdst(NG * G, -1);
    std::vector<uint32_t> grmw(NG * G, 0u);
    std::vector<int2> grng(ranges ? NG * G : 0, make_int2(0, 0));
    int W = 1;
    for (size_t gi = 0; gi < NG; ++gi) {
        const size_t r = runs[gi].first, n = runs[gi].second;
        std::map<int64_t, std::array<float, GROUP_MAX>> u;
        for (size_t m = 0; m < n; ++m) {
            for (auto &e : h.rows[r + m]) {
                auto it = u.find(e.first);
                if (it == u.end()) it = u.emplace(e.first, std::array<float, GROUP_MAX>{}).first;
                it->second[m] += e.second;
            }
            gdst[gi * G + m] = h.dst[r + m];
            if (mask) grmw[gi * G + m] = (*mask)[r + m];
            if (ranges) grng[gi * G + m] = (*ranges)[r + m];
        }
        grows[gi].assign(u.begin(), u.end());
        W = std::max(W, (int)grows[gi].size());
    }
    if (env_on("SURFH_TABLE_STATS", false)) {      // diagnostics: taps per group against taps of its members
        size_t ut = 0, mt = 0;
        for (size_t gi = 0; gi < NG; ++gi) {
            ut += grows[gi].size();
            for (size_t m = 0; m < runs[gi].second; ++m) mt += h.rows[runs[gi].first + m].size();
        }
        fprintf(stderr, "[surfh tables] %zu groups of <= %d rows, widest %d taps, %.2f union taps per group, %.2f taps per member row\n", NG,
                G, W, (double)ut / std::max<size_t>(NG, 1), (double)mt / std::max<size_t>(h.rows.size(), 1));
    }
    std::vector<int32_t> gcnt(NG);
    std::vector<int64_t> gcol(NG * W, 0);
    std::vector<float> gval(NG * W * G, 0.f);
    for (size_t gi = 0; gi < NG; ++gi) {
        gcnt[gi] = (int32_t)grows[gi].size();
        for (size_t e = 0; e < grows[gi].size(); ++e) {
            gcol[gi * W + e] = grows[gi][e].first;
            for (int m = 0; m < G; ++m) gval[(gi * W + e) * G + m] = grows[gi][e].second[m];
        }
    }
    if (d->g_cnt.upload(gcnt) || d->g_col.upload(gcol) || d->g_val.upload(gval) || d->g_dst.upload(gdst) || d->g_rmw.upload(grmw)) return 1;
    d->g.NG = (int)NG; d->g.W = W; d->g.G = G; d->g.cnt = d->g_cnt; d->g.col = d->g_col; d->g.val = d->g_val; d->g.dst = d->g_dst; d->g.rmw = d->g_rmw;
    if (ranges) {
        if (d->g_rng.upload(grng)) return 1;
        d->g.rng = d->g_rng;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// table construction for one channel
// ---------------------------------------------------------------------------------------------
int build_channel(surfh_plan *p, const surfh_channel_desc &d, Channel *c) {
    c->ws0 = d.wslice_start;
    c->ws1 = d.wslice_stop;
    c->Lin = c->ws1 - c->ws0;
    c->P = d.n_pointings;
    c->S = d.n_slit;
    c->Ldet = d.n_lambda_out;
    c->aout = d.n_alpha_out;
    c->srf = d.srf;
    c->na = d.na;
    c->nb = d.nb;
    c->alpha0 = d.alpha0;
    c->nas = d.n_alpha_slit;
    c->nbs = d.n_beta_slit;
    if (c->Lin <= 0 || c->ws0 < 0 || c->ws1 > p->Lc) return fail("channel wslice (%d,%d) outside cube (Lc=%d)", c->ws0, c->ws1, p->Lc);
    if (c->P < 1 || c->S < 1 || c->Ldet < 1 || c->aout < 1 || c->srf < 1 || c->nbs < 1) return fail("bad channel dims");
    const int box = d.box_len > 0 ? d.box_len : c->srf, bsh = d.box_len > 0 ? d.box_shift : 0;
    if (box > c->na || bsh <= -c->na || bsh >= c->na) return fail("bad box window (len %d, shift %d)", box, bsh);
    if ((c->aout - 1) * c->srf >= c->nas) return fail("decimation (alpha_out-1)*srf=%d exceeds the slit alpha window %d", (c->aout - 1) * c->srf, c->nas);
    if (c->alpha0 < 0 || c->alpha0 + c->nas > c->na) return fail("slit alpha window outside the local grid");
    if (!d.slit_beta0 || !d.slit_weights || !d.grid_i0 || !d.grid_i1 || !d.grid_y0 || !d.grid_y1)
        return fail("channel table pointer is NULL");
    c->bsum = (d.wpsf == nullptr);
    if (c->bsum) c->Ldet = c->Lin;
    for (int s = 0; s < c->S; ++s)
        if (d.slit_beta0[s] < 0 || d.slit_beta0[s] + c->nbs > c->nb) return fail("slit %d beta window outside the local grid", s);
    // wavelength window inside the plan's planes, start aligned to 4 floats for 16-byte vector access
    const int cw0 = p->compact(c->ws0);
    if (cw0 < 0) return fail("channel window not inside the plan's planes");
    c->ws0a = (cw0 / 4) * 4;
    c->shift = cw0 - c->ws0a;
    c->LinA = (cw0 + c->Lin) - c->ws0a;
    c->LinP = pad64(c->LinA);
    if (!c->bsum && ((long)c->nbs * c->LinP) % 128) c->LinP += 64;    // K, NP, LdetP multiples of 128: tile grid of the GEMMs
    c->nlam = (c->LinA + 3) / 4 * 4;
    c->K = (c->bsum ? 1 : c->nbs) * c->LinP;
    c->NP = (c->P * c->S * c->aout + 127) / 128 * 128;
    c->LdetP = (c->Ldet + 127) / 128 * 128;
    c->ysize = (long)c->P * c->S * c->Ldet * c->aout;

    const long nloc = (long)c->na * c->nb;
    // bounds: the forward gather mirrors bounds_error=True (cython_2D_interpolation.py:472-478);
    // indices come clamped from find_indices, so only range-check them here.
    for (long i = 0; i < (long)c->P * nloc; ++i)
        if (d.grid_i0[i] < 0 || d.grid_i0[i] > p->Na - 2 || d.grid_i1[i] < 0 || d.grid_i1[i] > p->Nb - 2)
            return fail("bilinear index out of range at local pixel %ld", i);

    const int64_t LP = p->LP;
    auto pix_off = [&](int ia, int ib) -> int64_t { return ((int64_t)ib * p->NAP + ia) * LP + c->ws0a; };
    auto xs_off = [&](int pt, int s, int a, int b) -> int64_t {
        return ((int64_t)((pt * c->S + s) * c->aout + a)) * c->K + (c->bsum ? 0 : (int64_t)b * c->LinP);
    };

    // ---- forward rows (p, a, j-order over (s,b')): S + box-sum + slit window + decimation -------
    HostEll f;
    std::vector<std::vector<std::pair<int, int>>> colslit(c->nb);   // local column -> (slit, b')
    for (int s = 0; s < c->S; ++s)
        for (int b = 0; b < c->nbs; ++b) colslit[d.slit_beta0[s] + b].push_back({s, b});
    for (int pt = 0; pt < c->P; ++pt)
        for (int a = 0; a < c->aout; ++a)
            for (int j = 0; j < c->nb; ++j)
                for (auto &sb : colslit[j]) {
                    const int s = sb.first, b = sb.second;
                    const double ws = d.slit_weights[(long)s * c->nbs + b];
                    std::vector<std::pair<int64_t, float>> row;
                    std::map<int64_t, double> acc;
                    for (int r = 0; r < box; ++r) {
                        const int i = (c->alpha0 + a * c->srf + r + bsh + c->na) % c->na;
                        const long li = (long)pt * nloc + (long)i * c->nb + j;
                        const int i0 = d.grid_i0[li], i1 = d.grid_i1[li];
                        const double y0 = d.grid_y0[li], y1 = d.grid_y1[li];
                        const double w[4] = {(1. - y0) * (1. - y1), (1. - y0) * y1, y0 * (1. - y1), y0 * y1};
                        const int da[4] = {0, 0, 1, 1}, db[4] = {0, 1, 0, 1};
                        for (int k = 0; k < 4; ++k)
                            if (w[k] * ws != 0.0) acc[pix_off(i0 + da[k], i1 + db[k])] += w[k] * ws;
                    }
                    // consecutive samples of the box window share two of their four cube pixels: one tap per distinct
                    // pixel (about 16 instead of 28 reads per output element)
                    for (auto &e : acc) row.push_back({e.first, (float)e.second});
                    f.rows.push_back(std::move(row));
                    f.dst.push_back(xs_off(pt, s, a, b));
                }
    if (c->bsum) {   // rows that share a destination (the slit's beta columns) are merged into one
        std::map<int64_t, std::map<int64_t, double>> mg;
        for (size_t r = 0; r < f.rows.size(); ++r)
            for (auto &e : f.rows[r]) mg[f.dst[r]][e.first] += (double)e.second;
        HostEll f2;
        for (auto &row : mg) {
            std::vector<std::pair<int64_t, float>> v;
            for (auto &e : row.second) v.push_back({e.first, (float)e.second});
            f2.rows.push_back(std::move(v));
            f2.dst.push_back(row.first);
        }
        f = std::move(f2);
    }
    if (p->gather_sorted) {
        // Order the gather rows by the cube pixel of their first tap.  In (pointing, alpha, beta) order the four dither
        // pointings, which cover the same pixels shifted by a few columns, are a quarter of the table apart: every pixel
        // was fetched from HBM once per pointing (measured 0.525 GB per launch for a 0.15 GB window).  Sorted, the rows
        // that share taps run together on one XCD and hit its L2.
        std::vector<size_t> ord(f.rows.size());
        for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
            const int64_t ka = f.rows[a].empty() ? INT64_MAX : f.rows[a][0].first, kb = f.rows[b].empty() ? INT64_MAX : f.rows[b][0].first;
            return ka < kb;
        });
        HostEll g;
        g.rows.reserve(ord.size());
        g.dst.reserve(ord.size());
        for (size_t i : ord) {
            g.rows.push_back(std::move(f.rows[i]));
            g.dst.push_back(f.dst[i]);
        }
        f = std::move(g);
    }
    if (upload_ell(f, &c->fwd)) return 1;
    if (p->gather_grouped && p->gather_sorted && !c->bsum) {      // GATHER_G rows neighbouring in cube-location order per workgroup
        std::vector<std::pair<size_t, size_t>> runs;
        for (size_t r = 0; r < f.rows.size(); r += GATHER_G) runs.push_back({r, std::min<size_t>(GATHER_G, f.rows.size() - r)});
        if (upload_groups(f, runs, nullptr, &c->fwd, GATHER_G)) return 1;
    }

    // ---- exact transpose: rows = touched cube pixels ------------------------------------------
    {
        std::map<int64_t, std::map<int64_t, double>> tr;   // pixel offset -> (Xs offset -> weight)
        for (size_t r = 0; r < f.rows.size(); ++r)
            for (auto &e : f.rows[r]) tr[e.first][f.dst[r]] += (double)e.second;
        HostEll t;
        for (auto &px : tr) {
            std::vector<std::pair<int64_t, float>> row;
            for (auto &e : px.second) row.push_back({e.first, (float)e.second});
            t.rows.push_back(std::move(row));
            t.dst.push_back(px.first);
        }
        if (upload_ell(t, &c->adjT)) return 1;
        for (int64_t o : t.dst) {
            const int ia = (int)((o / LP) % p->NAP), ib = (int)((o / LP) / p->NAP);
            p->a_lo = std::min(p->a_lo, ia); p->a_hi = std::max(p->a_hi, ia + 1);
            p->b_lo = std::min(p->b_lo, ib); p->b_hi = std::max(p->b_hi, ib + 1);
        }
        c->adjT.host_dst = t.dst;
        c->adjT_host = std::move(t);
    }

    // ---- reference-compatible back-interpolation (gridding_t) ---------------------------------
    c->has_ref = d.gt_i0 && d.gt_i1 && d.gt_y0 && d.gt_y1 && d.gt_inside;
    if (c->has_ref) {
        // local row i' -> decimated rows a whose box window contains it
        std::vector<std::vector<int>> arow(c->na);
        for (int a = 0; a < c->aout; ++a)
            for (int r = 0; r < box; ++r) arow[(c->alpha0 + a * c->srf + r + bsh + c->na) % c->na].push_back(a);
        HostEll t;
        const long npix = (long)p->Na * p->Nb;
        for (int ib = 0; ib < p->Nb; ++ib)
            for (int ia = 0; ia < p->Na; ++ia) {
                std::map<int64_t, double> m;
                for (int pt = 0; pt < c->P; ++pt) {
                    const long gi = (long)pt * npix + (long)ia * p->Nb + ib;
                    if (!d.gt_inside[gi]) continue;
                    const int i0 = d.gt_i0[gi], i1 = d.gt_i1[gi];
                    if (i0 < 0 || i0 > c->na - 2 || i1 < 0 || i1 > c->nb - 2) return fail("gridding_t index out of range");
                    const double y0 = d.gt_y0[gi], y1 = d.gt_y1[gi];
                    const double w[4] = {(1. - y0) * (1. - y1), (1. - y0) * y1, y0 * (1. - y1), y0 * y1};
                    const int li[4] = {i0, i0, i0 + 1, i0 + 1}, lj[4] = {i1, i1 + 1, i1, i1 + 1};
                    for (int k = 0; k < 4; ++k)
                        if (w[k] != 0.0)
                        for (int a : arow[li[k]])
                            for (auto &sb : colslit[lj[k]])
                                m[xs_off(pt, sb.first, a, sb.second)] += w[k] * d.slit_weights[(long)sb.first * c->nbs + sb.second];
                }
                if (m.empty()) continue;
                std::vector<std::pair<int64_t, float>> row;
                for (auto &e : m) row.push_back({e.first, (float)e.second});
                t.rows.push_back(std::move(row));
                t.dst.push_back(pix_off(ia, ib));
            }
        if (upload_ell(t, &c->adjRef)) return 1;
        for (int64_t o : t.dst) {
            const int ia = (int)((o / LP) % p->NAP), ib = (int)((o / LP) / p->NAP);
            p->a_lo = std::min(p->a_lo, ia); p->a_hi = std::max(p->a_hi, ia + 1);
            p->b_lo = std::min(p->b_lo, ib); p->b_hi = std::max(p->b_hi, ib + 1);
        }
    }

    // ---- spectral PSF as GEMM operands: W[l'][b'*LinP + shift + l] = wpsf[l'][l][b'] -------------
    if (!c->bsum) {
        std::vector<float> W((size_t)c->LdetP * c->K, 0.f), Wt((size_t)c->K * c->LdetP, 0.f);
        for (int l = 0; l < c->Ldet; ++l)
            for (int lam = 0; lam < c->Lin; ++lam)
                for (int b = 0; b < c->nbs; ++b) {
                    const float v = (float)d.wpsf[((long)l * c->Lin + lam) * c->nbs + b];
                    const size_t k = (size_t)b * c->LinP + c->shift + lam;
                    W[(size_t)l * c->K + k] = v;
                    Wt[k * c->LdetP + l] = v;
                }
        float wmax = 0.f;
        for (float v : W) wmax = std::max(wmax, std::fabs(v));
        c->sW = gemm_f16x2_scale(wmax);
        if (c->W.upload(W) || c->Wt.upload(Wt)) return 1;
    }
    if (c->Xs.zeros((size_t)c->NP * c->K)) return 1;
    return !c->bsum && c->ymat.zeros((size_t)c->NP * c->LdetP);
}

}  // namespace

// K-step classes of the two-piece fp16 GEMM for its constant operand B [N][ldb] (host copy; K columns, tiles of 256 rows).
// A step of 32 columns may be computed from the leading fp16 pieces alone ("far": relative error of its terms <= 2^-10, random
// sign) when what it contributes is small: per tile the steps are taken in ascending order of their largest share of a row,
// and moved to the far class as long as, for EVERY row of the tile, the far steps together hold <= tol1 of the row's l1 norm
// and <= tol2 of its l2 norm.  The error this adds to an output is then <= 2^-10 tol1 of sum |B||x| in the worst case (every
// rounding error aligned) and ~ 3e-4 tol2 of |B row|_2 |x|_2 for rounding errors of random sign: with tol1 = 2^-8, tol2 = 2^-10
// 4e-6 and 3e-7 of the row's own scale.  The spectral response (a grating's sinc^2, instru.py psfs) falls off as 1 / x^2 from
// its diagonal: about two thirds of the steps of a tile qualify.  Record per tile: [n_near, n_far, near..., far...], entry =
// step | segment << 16 (gemm_f32.h).  Fewer than 8 far steps are not worth the second pass: all near.
int build_klist(const float *B, int N, int K, long ldb, int segLinP, int segChunks, double tol1, double tol2, std::vector<int> *out,
                int *stride, long *n_near, long *n_far, int permP, int permLin) {
    // tile columns as in the kernel: 256 consecutive rows, or 256 / permP rows of each of permP neighbouring columns of permLin rows
    const int Q = permP ? 256 / permP : 256, tilesL = permP ? permLin / Q : 0, ncol = permP ? N / permLin : 0;
    const int nb = K / 32, tilesN = permP ? (ncol + permP - 1) / permP * tilesL : (N + 255) / 256;
    auto brow = [&](int tn, int v) {
        if (!permP) { const int n = tn * 256 + v; return n < N ? n : -1; }
        const int c = (tn / tilesL) * permP + v / Q;
        return c < ncol ? c * permLin + (tn % tilesL) * Q + v % Q : -1;
    };
    *stride = 2 + nb;
    out->assign((size_t)tilesN * *stride, 0);
    *n_near = *n_far = 0;
    std::vector<double> l1((size_t)256 * nb), l2((size_t)256 * nb), L1(256), L2(256), c1(256), c2(256), imp(nb);
    std::vector<int> order(nb);
    std::vector<char> far(nb);
    for (int tn = 0; tn < tilesN; ++tn) {
        const int nr = 256;
        for (int r = 0; r < nr; ++r) {
            const int br = brow(tn, r);
            if (br < 0) {          // no such row: nothing to bound
                for (int b = 0; b < nb; ++b) l1[(size_t)r * nb + b] = l2[(size_t)r * nb + b] = 0.0;
                L1[r] = L2[r] = 0.0;
                continue;
            }
            const float *row = B + (long)br * ldb;
            double s1 = 0.0, s2 = 0.0;
            for (int b = 0; b < nb; ++b) {
                double a1 = 0.0, a2 = 0.0;
                for (int k = 0; k < 32; ++k) { const double v = row[b * 32 + k]; a1 += std::fabs(v); a2 += v * v; }
                l1[(size_t)r * nb + b] = a1; l2[(size_t)r * nb + b] = a2;
                s1 += a1; s2 += a2;
            }
            L1[r] = s1; L2[r] = s2;
        }
        for (int b = 0; b < nb; ++b) {
            double m = 0.0;
            for (int r = 0; r < nr; ++r)
                if (L1[r] > 0.0) m = std::max(m, std::max(l1[(size_t)r * nb + b] / (L1[r] * tol1), std::sqrt(l2[(size_t)r * nb + b] / L2[r]) / tol2));
            imp[b] = m;
            order[b] = b;
            far[b] = 0;
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return imp[a] < imp[b]; });
        std::fill(c1.begin(), c1.end(), 0.0);
        std::fill(c2.begin(), c2.end(), 0.0);
        int nf = 0;
        for (int i = 0; i < nb; ++i) {
            const int b = order[i];
            bool ok = true;
            for (int r = 0; r < nr && ok; ++r)
                ok = c1[r] + l1[(size_t)r * nb + b] <= tol1 * L1[r] && c2[r] + l2[(size_t)r * nb + b] <= tol2 * tol2 * L2[r];
            if (!ok) break;
            for (int r = 0; r < nr; ++r) { c1[r] += l1[(size_t)r * nb + b]; c2[r] += l2[(size_t)r * nb + b]; }
            far[b] = 1;
            ++nf;
        }
        if (nf < 8) { std::fill(far.begin(), far.end(), 0); nf = 0; }
        int *rec = out->data() + (size_t)tn * *stride;
        rec[0] = nb - nf; rec[1] = nf;
        int in = 2, ifar = 2 + nb - nf;
        for (int b = 0; b < nb; ++b) {
            const int k = b * 32;
            const int e = b | ((segLinP ? (k / segLinP) * segChunks + (k % segLinP) / 1024 : 0) << 16);
            if (far[b]) rec[ifar++] = e; else rec[in++] = e;
        }
        *n_near += nb - nf; *n_far += nf;
    }
    return 0;
}

namespace {

int pick_split(const Channel &c, int forced, bool f16, int n_cu) {
    if (forced > 0) return (c.K % (32 * forced) == 0) ? forced : 1;
    if (f16) {
        // two-piece fp16 kernel (256 x 256 tiles, one workgroup per CU).  The slab length is set by accuracy first: one fp32
        // accumulation chain of 4096 non-negative products shows a bias of -1.3e-7 (three-piece bf16 products lost their
        // small terms beyond about 1024 k), so chains run up to 4352 k (136 K steps); beyond the fewest such slabs, any
        // divisor that leaves at least 16 K steps per slab and fills the last round of workgroups best.
        constexpr int max_steps = 136, tile_m = 256, tile_n = 256;
        const long tiles = (long)((c.NP + tile_m - 1) / tile_m) * ((c.LdetP + tile_n - 1) / tile_n);
        const int steps = c.K / 32;
        int smin = 0;
        for (int s = 1; s <= steps; ++s)
            if (steps % s == 0 && steps / s <= max_steps) { smin = s; break; }
        if (!smin) return 1;
        int best = smin;
        double best_t = -1.0;
        for (int s = smin; s <= steps / 16 && s <= steps; ++s) {
            if (steps % s) continue;
            const double t = (double)((tiles * s + n_cu - 1) / n_cu) * (steps / s) + 3.0 * s;
            if (best_t < 0 || t < best_t) { best_t = t; best = s; }
        }
        return best;
    }
    const int bm = (c.NP % 128 == 0) ? 128 : 64, bn = (c.LdetP % 128 == 0) ? 128 : 64;
    const long tiles = (long)(c.NP / bm) * (c.LdetP / bn);
    int best = 1;
    for (int s : {1, 2, 3, 4, 6, 8, 12, 16, 24, 32}) {
        if (c.K % (32 * s)) continue;
        if (c.K / s < 256) break;
        best = s;
        if (tiles * s >= 768) break;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------
// DFT matrices (ortho).  Forward r2c along beta then c2c along alpha; inverse c2c along alpha then
// c2r along beta with Hermitian weights w_k (1 for k=0 and Nyquist, else 2) -- numpy's rfft2/irfft2.
// ---------------------------------------------------------------------------------------------
void build_dft(const surfh_plan *p, std::vector<float> &Fi, std::vector<float> &Gi, std::vector<float> &Gf,
               std::vector<float> &Ff, std::vector<float> &GiT, std::vector<float> &GfT) {
    const int Na = p->Na, Nb = p->Nb, NAP = p->NAP, NBP = p->NBP, KAP = p->KAP, KBP = p->KBP;
    const int nkb = Nb / 2 + 1;
    const double sa = 1.0 / std::sqrt((double)Na), sb = 1.0 / std::sqrt((double)Nb);
    Fi.assign((size_t)2 * NAP * 2 * KAP, 0.f);
    Ff.assign((size_t)2 * KAP * 2 * NAP, 0.f);
    Gi.assign((size_t)2 * KBP * NBP, 0.f);
    Gf.assign((size_t)NBP * 2 * KBP, 0.f);
    GiT.assign((size_t)NBP * 2 * KBP, 0.f);
    GfT.assign((size_t)2 * KBP * NBP, 0.f);
    for (int a = 0; a < Na; ++a)
        for (int k = 0; k < Na; ++k) {
            const long m = ((long)a * k) % Na;   // exact phase reduction
            const double th = 2.0 * M_PI * (double)m / (double)Na;
            const double c = std::cos(th) * sa, s = std::sin(th) * sa;
            // inverse along alpha: rows (c,alpha), cols (c',k_alpha)
            Fi[((size_t)0 * NAP + a) * (2 * KAP) + 0 * KAP + k] = (float)c;
            Fi[((size_t)0 * NAP + a) * (2 * KAP) + 1 * KAP + k] = (float)(-s);
            Fi[((size_t)1 * NAP + a) * (2 * KAP) + 0 * KAP + k] = (float)s;
            Fi[((size_t)1 * NAP + a) * (2 * KAP) + 1 * KAP + k] = (float)c;
            // forward along alpha: rows (c,k_alpha), cols (c',alpha)
            Ff[((size_t)0 * KAP + k) * (2 * NAP) + 0 * NAP + a] = (float)c;
            Ff[((size_t)0 * KAP + k) * (2 * NAP) + 1 * NAP + a] = (float)s;
            Ff[((size_t)1 * KAP + k) * (2 * NAP) + 0 * NAP + a] = (float)(-s);
            Ff[((size_t)1 * KAP + k) * (2 * NAP) + 1 * NAP + a] = (float)c;
        }
    for (int b = 0; b < Nb; ++b)
        for (int k = 0; k < nkb; ++k) {
            const long m = ((long)b * k) % Nb;
            const double th = 2.0 * M_PI * (double)m / (double)Nb;
            const double c = std::cos(th) * sb, s = std::sin(th) * sb;
            const double w = (k == 0 || (Nb % 2 == 0 && k == Nb / 2)) ? 1.0 : 2.0;
            Gi[((size_t)0 * KBP + k) * NBP + b] = (float)(w * c);
            Gi[((size_t)1 * KBP + k) * NBP + b] = (float)(-w * s);
            Gf[(size_t)b * (2 * KBP) + 0 * KBP + k] = (float)c;
            Gf[(size_t)b * (2 * KBP) + 1 * KBP + k] = (float)(-s);
            GiT[(size_t)b * (2 * KBP) + 0 * KBP + k] = (float)(w * c);
            GiT[(size_t)b * (2 * KBP) + 1 * KBP + k] = (float)(-w * s);
            GfT[((size_t)0 * KBP + k) * NBP + b] = (float)c;
            GfT[((size_t)1 * KBP + k) * NBP + b] = (float)(-s);
        }
}

// Support of the OTF for the two passes that multiply by it (the forward's complex pass with the fused mix, the fused adjoint
// tail).  A PSF sampled finer than its diffraction limit has an OTF that vanishes beyond a cutoff; the reference's synthetic
// Gaussian PSF (utils.py:40-50) falls below 2^-24 of its peak beyond 50-80 % of the k_beta range.  Products with such entries
// are below the rounding of the plane's leading terms in fp32, so the (k_beta, 128-wavelength chunk) super-tiles in which NO
// entry of any k_alpha reaches 2^-24 of its plane's largest magnitude are dropped from both passes -- the same set in both, so the
// adjoint stays the transpose of the forward.  Nothing is dropped when every tile has such an entry.  Runs where `r`, the route
// before the scan, asks for it (Route::scan_otf); `found` is the outcome that completes the route.
int otf_support(surfh_plan *p, const surfh_config *cfg, const Route &r, bool ranges, OtfSupport *found) {
    *found = OTF_NONE;
    if (!r.scan_otf) return 0;
    const bool ct = r.ax_a == AX_CT;      // both axes on dft_ct (else both on dft_h2)
    const int nkb = p->Nb / 2 + 1, nch = (int)(p->LP / 128);
    std::vector<int> bmax(nch, -1), amaxk(nch, -1);   // largest k_beta / folded k_alpha of the support over a chunk's planes (-1: none)
    std::vector<double> km(nkb), kam(p->Na);
    for (int l = 0; l < p->Lown; ++l) {
        if (p->planes[l] < 0) continue;
        std::fill(km.begin(), km.end(), 0.0);
        std::fill(kam.begin(), kam.end(), 0.0);
        double amax = 0.0;
        const double *pl = cfg->sotf + (size_t)p->planes[l] * p->Na * nkb * 2;
        for (int a = 0; a < p->Na; ++a)
            for (int k = 0; k < nkb; ++k) {
                const double re = pl[((size_t)a * nkb + k) * 2], im = pl[((size_t)a * nkb + k) * 2 + 1], m2 = re * re + im * im;
                if (m2 > km[k]) km[k] = m2;
                if (m2 > kam[a]) kam[a] = m2;
            }
        for (int k = 0; k < nkb; ++k) amax = std::max(amax, km[k]);
        const double thr = amax * std::ldexp(1.0, -48);       // squared magnitudes
        int b = -1;
        for (int k = 0; k < nkb; ++k)
            if (km[k] > thr) b = k;
        bmax[l / 128] = std::max(bmax[l / 128], b);
        int af = -1;
        for (int a = 0; a < p->Na; ++a)
            if (kam[a] > thr) af = std::max(af, std::min(a, p->Na - a));
        amaxk[l / 128] = std::max(amaxk[l / 128], af);
    }
    std::vector<int> vlist, kbstart(nkb + 1, 0);
    for (int kb = 0; kb < nkb; ++kb) {
        kbstart[kb] = (int)vlist.size();
        for (int j = 0; j < nch; ++j)
            if (kb <= bmax[j]) vlist.push_back(kb * nch + j);
    }
    kbstart[nkb] = (int)vlist.size();
    if (vlist.empty() || (long)vlist.size() == (long)nkb * nch) return 0;       // nothing to drop (or nothing to keep: leave the passes as they are)
    const size_t nyc = (size_t)2 * p->NAP * p->KBP * p->LP;
    if (p->otf_vlist.upload(vlist) || p->otf_kbstart.upload(kbstart) || p->ycol_mix.zeros(nyc)) return 1;
    p->otf_nvalid = (int)vlist.size();
    *found = ranges ? OTF_LISTS_RANGES : OTF_LISTS;
    std::vector<int> tabs((size_t)(ct ? 4 : 3) * nch);
    for (int j = 0; j < nch; ++j) {
        if (ct) {
            // sub-sequence n1 of a length R M: element j stands for the rows R j + n1 and N - (R j - n1); inside the support
            // (folded index <= amax) for j <= (amax + R - 1) / R
            const int ja = (std::max(amaxk[j], 0) + p->ctA.R - 1) / p->ctA.R, jb = (std::max(bmax[j], 0) + p->ctB->R - 1) / p->ctB->R;
            tabs[j] = std::min(std::max(ja / 16 + 1, 2), p->ctA.KT);              // forward's complex pass: k-steps in k_alpha
            tabs[nch + j] = std::min(std::max(jb / 16 + 1, 2), p->ctB->KT);        // forward's pass along beta: k-steps in k_beta
            tabs[2 * nch + j] = bmax[j];                                           // adjoint's first pass: last row k_beta stored; reduction: k_beta limit
            tabs[3 * nch + j] = amaxk[j];                                          // adjoint's complex pass: last folded row k_alpha stored; reduction: limit
            continue;
        }
        tabs[j] = std::min(std::max((amaxk[j] + 16) / 16, 2), p->KPa / 16);
        tabs[nch + j] = std::min(std::max((bmax[j] + 16) / 16, 2), p->KPb / 16);
        tabs[2 * nch + j] = bmax[j] + 1;
    }
    if (ranges && p->otf_tabs.upload(tabs)) return 1;
    return 0;
}

// the eight switches that feed the route (RouteSwitch), read once at the top of plan creation; DESIGN.md says what each one does
unsigned read_route_switches() {
    static const struct { const char *name; bool dflt; } sw[SW_COUNT] = {
        {"SURFH_DFT_H2", true}, {"SURFH_DFT_CT", true}, {"SURFH_DFT_DENSE", false}, {"SURFH_NO_FUSED_MIX", false},
        {"SURFH_ADJ_FUSED", true}, {"SURFH_OTF_PROD", true}, {"SURFH_OTF_SUPPORT", true}, {"SURFH_OTF_RANGES", true}};
    unsigned m = 0;
    for (int i = 0; i < SW_COUNT; ++i) m |= (unsigned)env_on(sw[i].name, sw[i].dflt) << i;
    return m;
}

}  // namespace

// The one decision of a plan's route (Route, plan_internal.h; the table in DESIGN.md).  Pure: no HIP call, no environment.  The
// kernel is chosen per axis: dft_h2 (16 < n/2+1 <= 128, row offsets below 4 GB), else dft_ct (n = R M), else none -- and that,
// a verification plan or SURFH_DFT_DENSE=1 put the whole plan on the dense fp32 products.  `scan`: what the OTF scan found.
Route decide_route(const RouteInput &in, OtfSupport scan) {
    Route r;
    auto axis = [&](int n) {
        if (in.on(SW_DFT_H2) && dft_h2_supported(n, n, in.NAP, in.KBP, in.LP)) return AX_H2;
        if (in.on(SW_DFT_CT) && dft_ct_factor(n, nullptr, nullptr)) return AX_CT;
        return AX_DENSE;
    };
    const AxisKernel a = axis(in.Na), b = axis(in.Nb);
    if (in.verify || in.on(SW_DFT_DENSE) || a == AX_DENSE || b == AX_DENSE) return r;       // planar arrays, nothing fused
    r.ax_a = a; r.ax_b = b;
    const bool few = in.T >= 1 && in.T <= 4;          // templates the mix loaders and the fused tail hold in registers
    const bool both_h2 = a == AX_H2 && b == AX_H2, both_ct = a == AX_CT && b == AX_CT;
    r.mix = few && !in.on(SW_NO_FUSED_MIX);
    r.prod = in.on(SW_OTF_PROD) && in.T == 0 && a == AX_CT;
    r.fused_tail = both_h2 && in.on(SW_ADJ_FUSED) && few && in.Na >= 127 && in.Na <= 255;      // the tail's output rows
    r.tpl_spectral = in.T <= 4;
    r.spec_calls = r.mix && (r.fused_tail || !both_h2);
    // the support lists serve the mix loader and the adjoint's tail alike (the same tiles dropped in both, or the adjoint is no
    // transpose): dft_h2's ride on its fused tail, dft_ct's need both axes; exact & 2 asks for the whole spectrum
    r.scan_otf = r.mix && in.has_sotf && !(in.exact & 2) && in.on(SW_OTF_SUPPORT) && (r.fused_tail || both_ct);
    if (r.scan_otf) r.support = scan;
    if (both_ct && r.support == OTF_LISTS) r.support = OTF_NONE;       // dft_ct's listed passes take the k-ranges with the lists, or neither
    return r;
}

}  // namespace surfh_impl

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char *surfh_last_error(void) { return g_err.c_str(); }
int surfh_version(void) { return 100; }

int surfh_plan_destroy(surfh_plan *p) {
    if (!p) return 0;
    hipSetDevice(p->dev);
    if (p->stream) hipStreamSynchronize(p->stream);
    delete p;      // the device buffers first (members), then the events and streams (PlanHandles, the base): plan_internal.h
    return 0;
}

int surfh_plan_create(const surfh_config *cfg, surfh_plan **out) {
    if (!cfg || !out) return fail("null argument");
    *out = nullptr;
    if (cfg->n_alpha < 2 || cfg->n_beta < 2 || cfg->n_lambda < 1) return fail("bad cube shape");
    if (cfg->n_channels < 0 || (cfg->n_channels > 0 && !cfg->channels)) return fail("bad channel list");
    if (cfg->n_channels == 0 && cfg->n_templates < 1) return fail("a plan without channels needs templates (Model_WCT)");
    if (!cfg->sotf && cfg->n_templates > 0) return fail("sotf is NULL");      // NULL = no spatial blur, plane-wise plans only
    if (cfg->n_templates > 0 && !cfg->templates) return fail("templates is NULL");
    if (cfg->n_templates > SURFH_MAX_TEMPLATES)
        return fail("n_templates = %d: at most %d templates are supported", cfg->n_templates, SURFH_MAX_TEMPLATES);
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail("device %d not available (%d devices): the HIP path has no CPU fallback", cfg->device, ndev);
    HIP_OK(hipSetDevice(cfg->device));

    surfh_plan *p = new surfh_plan();
    p->dev = cfg->device;
    if (hipDeviceGetAttribute(&p->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || p->n_cu < 1) p->n_cu = 256;
    auto bail = [&](int) {
        surfh_plan_destroy(p);
        return 1;
    };
    if (cfg->stream) {
        p->stream = (hipStream_t)cfg->stream;
    } else {
        if (hipStreamCreate(&p->stream) != hipSuccess) return bail(fail("hipStreamCreate failed"));
        p->own_stream = true;
    }
    p->Na = cfg->n_alpha;
    p->Nb = cfg->n_beta;
    p->Lc = cfg->n_lambda;
    p->T = cfg->n_templates;
    p->NAP = pad64(p->Na);
    p->NBP = pad64(p->Nb);
    p->KAP = p->NAP;
    p->KBP = pad64(p->Nb / 2 + 1);
    p->PL = (long)p->KAP * p->KBP;
    p->PLc = (long)p->NAP * p->NBP;
    p->lo = p->Lc;
    p->hi = 0;
    for (int i = 0; i < cfg->n_channels; ++i) {
        p->lo = std::min(p->lo, (int)cfg->channels[i].wslice_start);
        p->hi = std::max(p->hi, (int)cfg->channels[i].wslice_stop);
    }
    if (cfg->n_channels == 0) { p->lo = 0; p->hi = p->Lc; }
    if (p->lo < 0 || p->hi > p->Lc || p->lo >= p->hi) return bail(fail("channel wslices outside the cube"));
    {   // merge the channel windows into disjoint segments; the plan stores only those planes
        std::vector<std::pair<int, int>> iv;
        if (cfg->n_channels == 0) iv.push_back({0, p->Lc});
        for (int i = 0; i < cfg->n_channels; ++i) iv.push_back({cfg->channels[i].wslice_start, cfg->channels[i].wslice_stop});
        std::sort(iv.begin(), iv.end());
        int coff = 0;
        for (auto &v : iv) {
            if (v.first >= v.second) return bail(fail("empty channel window"));
            if (!p->segs.empty() && v.first <= p->segs.back().start + p->segs.back().len) {
                auto &g = p->segs.back();
                const int grow = std::max(0, v.second - (g.start + g.len));
                g.len += grow;
                coff += grow;
            } else {
                // every segment starts on a multiple of 4 compact planes (16-byte vector access per channel window)
                coff = (coff + 3) / 4 * 4;
                p->segs.push_back({v.first, v.second - v.first, coff});
                coff += v.second - v.first;
            }
        }
        p->Lown = coff;
        p->planes.assign(p->Lown, -1);
        for (auto &g : p->segs)
            for (int l = 0; l < g.len; ++l) p->planes[g.coff + l] = g.start + l;
    }
    p->LP = (p->Lown + 127) / 128 * 128;
    // the passes of the fused forward / adjoint run over the planes that exist, in whole wave tiles (read at plan creation; 0: over LP)
    p->Leff = env_on("SURFH_LAMBDA_TRIM", true) ? std::min(p->LP, (p->Lown + 31) / 32 * 32) : p->LP;
    p->isize = (long)(p->T > 0 ? p->T : p->Lc) * p->Na * p->Nb;
    const size_t LP = (size_t)p->LP;

    // the route before the OTF scan: everything up to the scan reads `r0`; p->route is written once, with the scan's outcome
    RouteInput rin;
    rin.Na = p->Na; rin.Nb = p->Nb; rin.T = p->T; rin.NAP = p->NAP; rin.KBP = p->KBP; rin.LP = p->LP;
    rin.verify = cfg->verify != 0; rin.has_sotf = cfg->sotf != nullptr; rin.exact = cfg->exact; rin.switches = read_route_switches();
    const Route r0 = decide_route(rin, OTF_NONE);
    const bool ilv = r0.interleaved();
    // ---- constants ------------------------------------------------------------------------
    {   // sotf [Lc][Na][Nb/2+1] complex128  ->  [2][KAP][KBP][LP] float (h2: [KAP][KBP][LP][2]), wavelength innermost
        const int nkb = p->Nb / 2 + 1;
        const size_t nsp = (size_t)2 * p->PL * LP;
        if (p->sotf.zeros(nsp)) return bail(1);
        std::vector<float> row((size_t)2 * p->KBP * LP);
        for (int a = 0; a < p->Na; ++a) {
            std::fill(row.begin(), row.end(), 0.f);
            for (int l = 0; l < p->Lown; ++l) {
                if (p->planes[l] < 0) continue;     // alignment gap between segments: stays zero
                const double *src = cfg->sotf ? cfg->sotf + ((size_t)p->planes[l] * p->Na + a) * nkb * 2 : nullptr;
                for (int k = 0; k < nkb; ++k) {
                    const float vr = src ? (float)src[2 * k] : 1.f, vi = src ? (float)src[2 * k + 1] : 0.f;
                    if (ilv) {
                        row[((size_t)k * LP + l) * 2] = vr;
                        row[((size_t)k * LP + l) * 2 + 1] = vi;
                    } else {
                        row[(size_t)k * LP + l] = vr;
                        row[((size_t)p->KBP + k) * LP + l] = vi;
                    }
                }
            }
            if (ilv) {
                if (hipMemcpy(p->sotf + (size_t)a * p->KBP * LP * 2, row.data(), (size_t)2 * p->KBP * LP * sizeof(float),
                              hipMemcpyHostToDevice) != hipSuccess)
                    return bail(fail("sotf upload failed"));
            } else
            for (int c = 0; c < 2; ++c)
                if (hipMemcpy(p->sotf + ((size_t)c * p->PL + (size_t)a * p->KBP) * LP, row.data() + (size_t)c * p->KBP * LP,
                              (size_t)p->KBP * LP * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
                    return bail(fail("sotf upload failed"));
        }
    }
    if (p->T > 0) {
        std::vector<float> t((size_t)p->T * LP, 0.f);
        for (int k = 0; k < p->T; ++k)
            for (int l = 0; l < p->Lown; ++l)
                if (p->planes[l] >= 0) t[(size_t)k * LP + l] = (float)cfg->templates[(size_t)k * p->Lc + p->planes[l]];
        if (p->tpl.upload(t)) return bail(1);
        p->tpl_host.assign(cfg->templates, cfg->templates + (size_t)p->T * p->Lc);
    }
    {
        std::vector<float> Fi, Gi, Gf, Ff, GiT, GfT;
        build_dft(p, Fi, Gi, Gf, Ff, GiT, GfT);
        if (p->Fi.upload(Fi) || p->Gi.upload(Gi) || p->Gf.upload(Gf) || p->Ff.upload(Ff) || p->GiT.upload(GiT) || p->GfT.upload(GfT)) return bail(1);
    }
    {   // folded-DFT matrices
        p->wblur_fp32 = env_on("SURFH_WBLUR_FP32", false);       // R / R^T on the fp32-input MFMA instead of the split-bf16 path
        // measured on config 3: 7.64 -> 7.53 ms per iteration (+1.5 %), the overlapped kernels slow each other down by
        // almost what they save; off by default so that per-kernel times in profiles stay those of a kernel running alone
        p->overlap = env_on("SURFH_OVERLAP", false);
        if (p->overlap && hipStreamCreateWithFlags(&p->stream2, hipStreamNonBlocking) != hipSuccess) return bail(fail("hipStreamCreate failed"));
        p->gather_grouped = env_on("SURFH_GATHER_GROUPED", true);
        p->gemm_grouped = env_on("SURFH_GEMM_GROUPED", true);
        p->scatter_grouped = env_on("SURFH_SCATTER_GROUPED", true);
        p->gather_sorted = env_on("SURFH_GATHER_SORTED", true);   // 0: gather rows in (pointing, alpha, beta) order
        const int ha = p->Na / 2 + 1, hb = p->Nb / 2 + 1;
        p->MPa = (ha + 127) / 128 * 128; p->KPa = (ha + 15) / 16 * 16;
        p->MPb = (hb + 127) / 128 * 128; p->KPb = (hb + 15) / 16 * 16;
        if (p->KPa > p->NAP || p->KPb > p->NBP || p->KPb > p->KBP) return bail(fail("cube too small for the folded DFT"));
        const double sa = 1.0 / std::sqrt((double)p->Na), sb = 1.0 / std::sqrt((double)p->Nb);
        std::vector<float> Cma((size_t)p->MPa * p->KPa, 0.f), Sma(Cma.size(), 0.f);
        for (int r = 0; r < ha; ++r)
            for (int k = 0; k < ha; ++k) {
                const double th = 2.0 * M_PI * (double)(((long)r * k) % p->Na) / (double)p->Na;
                Cma[(size_t)r * p->KPa + k] = (float)(std::cos(th) * sa);
                Sma[(size_t)r * p->KPa + k] = (float)(std::sin(th) * sa);
            }
        std::vector<float> Gc((size_t)p->MPb * p->KPb, 0.f), Gs(Gc.size(), 0.f), Cf(Gc.size(), 0.f), Sf(Gc.size(), 0.f);
        for (int b = 0; b < hb; ++b)
            for (int k = 0; k < hb; ++k) {
                const double th = 2.0 * M_PI * (double)(((long)b * k) % p->Nb) / (double)p->Nb;
                const double w = (k == 0 || (p->Nb % 2 == 0 && k == p->Nb / 2)) ? 1.0 : 2.0;
                Gc[(size_t)b * p->KPb + k] = (float)(w * std::cos(th) * sb);     // rows beta, cols k_beta
                Gs[(size_t)b * p->KPb + k] = (float)(w * std::sin(th) * sb);
                Cf[(size_t)k * p->KPb + b] = (float)(std::cos(th) * sb);         // rows k_beta, cols beta
                Sf[(size_t)k * p->KPb + b] = (float)(std::sin(th) * sb);
            }
        if (p->Cma.upload(Cma) || p->Sma.upload(Sma) || p->Gc.upload(Gc) || p->Gs.upload(Gs) || p->Cf.upload(Cf) || p->Sf.upload(Sf)) return bail(1);
        if (cfg->verify) {      // verification plan: fp32-operand spectral blur, and the route's dense DFT products and unfused mix -- all float64-accumulated
            p->verify = true;
            p->wblur_fp32 = true;
            p->overlap = false;
        }
        if (r0.ax_a == AX_H2 || r0.ax_b == AX_H2) {   // LDS images of the matrix pairs of the axes that run on dft_h2 (dft_h2.h)
            if ((r0.ax_a == AX_H2 && p->MPa != 128) || (r0.ax_b == AX_H2 && p->MPb != 128)) return bail(fail("internal: dft_h2 needs 128-row folded matrices"));
            std::vector<unsigned short> im(3 * DFT_H2_IMAGE_HALFS, 0);
            if (r0.ax_a == AX_H2) p->h2kA[0] = dft_h2_build_image(Cma.data(), Sma.data(), p->MPa, p->KPa, p->KPa, im.data());
            if (r0.ax_b == AX_H2) {
                p->h2kA[1] = dft_h2_build_image(Gc.data(), Gs.data(), p->MPb, p->KPb, p->KPb, im.data() + DFT_H2_IMAGE_HALFS);
                p->h2kA[2] = dft_h2_build_image(Cf.data(), Sf.data(), p->MPb, p->KPb, p->KPb, im.data() + 2 * DFT_H2_IMAGE_HALFS);
            }
            if (p->h2img.upload(im)) return bail(1);
        }
        // image + twiddles per transform length of the axes that run on dft_ct (dft_ct.h)
        if (r0.ax_a == AX_CT && dft_ct_plan_create(p->Na, &p->ctA)) return bail(fail("dft_ct plan (n_alpha = %d) failed", p->Na));
        if (r0.ax_b == AX_CT) {
            if (r0.ax_a == AX_CT && p->Nb == p->Na) p->ctB = &p->ctA;
            else if (dft_ct_plan_create(p->Nb, &p->ctB_own)) return bail(fail("dft_ct plan (n_beta = %d) failed", p->Nb));
        }
        OtfSupport found;
        if (otf_support(p, cfg, r0, rin.on(SW_OTF_RANGES), &found)) return bail(1);
        p->route = decide_route(rin, found);
        if (p->route.fused_tail) {       // the fused tail's partial sums: as many slots as its workgroups take super-tiles
            const size_t npart = dft_h2_adjmix_part_floats(p->LP, p->Nb / 2 + 1, p->otf_nvalid);
            if (!npart) return bail(fail("the fused adjoint tail could not size its partial sums"));
            if (p->adjmix_part.alloc(npart)) return bail(1);
        }
    }
    // ---- work buffers ---------------------------------------------------------------------
    const size_t nspec = (size_t)2 * p->PL * LP, ncube = (size_t)p->NBP * p->NAP * LP;
    const size_t nycol = (size_t)2 * p->NAP * p->KBP * LP;
    const size_t nmhat = p->T > 0 ? (size_t)p->T * 2 * p->PL : nspec;
    const size_t nmaps = (size_t)std::max(p->T, 1) * p->PLc;
    const size_t nycm = (size_t)std::max(p->T, 1) * 2 * p->NAP * p->KBP;
    // all six allocated, then all six cleared: the order of the allocations is part of what keeps the addresses where they were
    if (p->spec.alloc(nspec) || p->ycol.alloc(nycol) || p->cube.alloc(ncube) || p->mhat.alloc(nmhat) || p->maps_pad.alloc(nmaps) ||
        p->ycol_maps.alloc(nycm))
        return bail(1);
    if (dev_raw_clear(p->spec, nspec * sizeof(float), nullptr, false) || dev_raw_clear(p->ycol, nycol * sizeof(float), nullptr, false) ||
        dev_raw_clear(p->cube, ncube * sizeof(float), nullptr, false) || dev_raw_clear(p->mhat, nmhat * sizeof(float), nullptr, false) ||
        dev_raw_clear(p->maps_pad, nmaps * sizeof(float), nullptr, false) || dev_raw_clear(p->ycol_maps, nycm * sizeof(float), nullptr, false))
        return bail(1);
    p->ycm_planes = std::max(p->T, 1);
    // ---- channels -------------------------------------------------------------------------
    p->a_lo = p->b_lo = 1 << 30; p->a_hi = p->b_hi = 0;      // alpha / beta range of the pixels the channels' tables touch (build_channel)
    p->ch.resize(cfg->n_channels);
    long yoff = 0;
    for (int i = 0; i < cfg->n_channels; ++i) {
        if (build_channel(p, cfg->channels[i], &p->ch[i])) return bail(1);
        Channel &c = p->ch[i];
        c.yoff = yoff;
        yoff += c.ysize;
        if (c.bsum) continue;
        const bool f16 = !p->wblur_fp32;          // spectral-blur GEMMs as two-piece fp16 products (gemm_cc16.hip)
        c.splitK = p->verify ? 1 : pick_split(c, cfg->split_k_forward, f16, p->n_cu);
        if (f16) {
            const long nw = (long)c.LdetP * c.K;
            const long nwv = ymat_from_y_waves(c.P * c.S, c.Ldet, c.aout);
            if (c.W16.alloc((size_t)2 * nw) || c.Wt16.alloc((size_t)2 * nw) || c.amax.alloc((size_t)c.NP) || c.pmax.alloc((size_t)nwv) ||
                c.ymat16.alloc((size_t)2 * c.NP * c.LdetP) || c.Xs16.alloc((size_t)2 * c.NP * c.K))
                return bail(1);
            if (dev_raw_clear(c.pmax, (size_t)nwv * sizeof(unsigned), nullptr, false) ||       // entries of workgroups that exit early stay 0
                dev_raw_clear(c.amax, (size_t)c.NP * sizeof(unsigned), nullptr, false) ||
                dev_raw_clear(c.Xs16, (size_t)2 * c.NP * c.K * sizeof(unsigned short), nullptr, false))       // padding rows / columns stay zero
                return bail(1);
            std::vector<float> ones((size_t)c.nbs * ((c.LinP + 1023) / 1024) * c.NP, 1.f);   // segments never written: scale 1
            if (c.bscale.upload(ones)) return bail(1);
            if (launch_split2h(p->stream, c.W, c.W16, nw, nw, c.sW) || launch_split2h(p->stream, c.Wt, c.Wt16, nw, nw, c.sW))
                return bail(fail("operand split failed"));
            const bool far_steps = !(cfg->exact & 1) && env_on("SURFH_WBLUR_FAR", true);      // read at plan creation
            const double far_tol2 = [] { const char *e = getenv("SURFH_WBLUR_FAR_TOL2"); return std::ldexp(1.0, -(e ? atoi(e) : 10)); }();
            const int segChunks = (c.LinP + 1023) / 1024, KA = (c.Ldet + 31) / 32 * 32;
            if (far_steps && c.K / 32 <= 2048 && c.nbs * segChunks <= 64 && KA / 32 <= 2048) {
                std::vector<float> hw((size_t)nw);
                std::vector<int> kl;
                if (hipMemcpy(hw.data(), c.W, (size_t)nw * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return bail(fail("copy failed"));
                build_klist(hw.data(), c.LdetP, c.K, c.K, c.LinP, segChunks, 1.0 / 256, far_tol2, &kl, &c.klFs, &c.ksteps[0], &c.ksteps[1]);
                if (c.ksteps[1] > 0 && c.klF.upload(kl)) return bail(1);
                if (hipMemcpy(hw.data(), c.Wt, (size_t)nw * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return bail(fail("copy failed"));
                // the adjoint's constant operand has one row per (beta column, wavelength): a tile of 64 wavelengths of four
                // neighbouring columns sees the response's diagonal in 2-3 of its K steps, 256 wavelengths of one column in 9
                const bool perm = env_on("SURFH_WBLUR_PERM", true);
                const int pP = perm && c.LinP % 64 == 0 && c.nbs >= 4 ? 4 : 0;
                build_klist(hw.data(), c.K, KA, c.LdetP, 0, 0, 1.0 / 256, far_tol2, &kl, &c.klAs, &c.ksteps[2], &c.ksteps[3], pP, c.LinP);
                if (c.ksteps[3] > 0) {
                    if (c.klA.upload(kl)) return bail(1);
                    c.permA = pP;
                }
            }
        }
        if (c.Cpart.zeros((size_t)c.splitK * c.LdetP * c.NP)) return bail(1);
    }
    p->osize = yoff;
    if (p->a_hi <= p->a_lo) { p->a_lo = 0; p->a_hi = p->Na; }
    if (p->b_hi <= p->b_lo) { p->b_lo = 0; p->b_hi = p->Nb; }
    {   // transform passes batched over alpha skip the columns no table touches (SURFH_ALPHA_RANGE=0: whole cube)
        if (!env_on("SURFH_ALPHA_RANGE", true)) { p->a_lo = 0; p->a_hi = p->Na; p->b_lo = 0; p->b_hi = p->Nb; }
        if (ilv && p->a_hi - p->a_lo < p->Na) {      // the adjoint's intermediate: columns outside the range zero for good
            const size_t nyc = (size_t)2 * p->NAP * p->KBP * p->LP;
            if (p->ycol_adj.zeros(nyc)) return bail(1);
        }
    }
    {   // The adjoint scatters channel after channel into the cleared cube.  A (pixel, 1024-wavelength chunk) of channel c
        // must be read-modify-written only if an earlier channel's table has that pixel and its window reaches into the
        // chunk; everywhere else the destination is still zero and the kernel stores without reading (the windows of
        // adjacent bands overlap by a tenth, so most of the traffic is of the second kind).
        const long npixrows = (long)p->NBP * p->NAP;
        bool exact_ok = !p->verify;
        if (env_on("SURFH_ADJ_CLEAR", false)) exact_ok = false;      // A/B: clear the accumulator every call, chunk masks
        std::vector<std::vector<uint8_t>> touched(p->ch.size());
        for (size_t ci = 0; ci < p->ch.size(); ++ci) {
            Channel &c = p->ch[ci];
            const std::vector<int64_t> &dst = c.adjT.host_dst;
            touched[ci].assign((size_t)npixrows, 0);
            const int nchunk = (c.nlam / 4 + 255) / 256;
            std::vector<uint32_t> mask(dst.size(), nchunk > 32 ? 0xFFFFFFFFu : 0u);
            std::vector<int2> ranges(dst.size(), make_int2(0, 0));
            for (size_t r = 0; r < dst.size(); ++r) {
                const long pix = (dst[r] - c.ws0a) / p->LP;
                if (pix < 0 || pix >= npixrows) return bail(fail("scatter table: bad destination"));
                touched[ci][pix] = 1;
                {   // exact form: union of the earlier channels' windows at this pixel, inside this channel's window
                    int lo = INT32_MAX, hi = INT32_MIN, covered = 0;
                    for (size_t cj = 0; cj < ci; ++cj) {
                        if (!touched[cj][pix]) continue;
                        const Channel &o = p->ch[cj];
                        const int a = std::max(o.ws0a, c.ws0a), b = std::min(o.ws0a + o.nlam, c.ws0a + c.nlam);
                        if (a >= b) continue;
                        if (covered && (a > hi || b < lo)) exact_ok = false;      // two separate pieces: not one range
                        lo = std::min(lo, a);
                        hi = std::max(hi, b);
                        covered = 1;
                    }
                    if (covered) ranges[r] = make_int2(lo - c.ws0a, hi - c.ws0a);
                }
                if (nchunk > 32) continue;
                for (size_t cj = 0; cj < ci; ++cj) {
                    if (!touched[cj][pix]) continue;
                    const Channel &o = p->ch[cj];
                    for (int j = 0; j < nchunk; ++j) {
                        const int lo = c.ws0a + 1024 * j, hi = std::min(c.ws0a + c.nlam, lo + 1024);
                        if (lo < o.ws0a + o.nlam && o.ws0a < hi) mask[r] |= 1u << j;
                    }
                }
            }
            if (env_on("SURFH_SCATTER_RMW_ALL", false)) std::fill(mask.begin(), mask.end(), 0xFFFFFFFFu);
            if (p->scatter_grouped) {
                // rows are in pixel order: take runs of neighbouring pixels (destinations LP apart), SCATTER_G at a time
                const HostEll &h = c.adjT_host;
                std::vector<std::pair<size_t, size_t>> runs;
                for (size_t r = 0; r < h.rows.size();) {
                    size_t n = 1;
                    while (n < (size_t)SCATTER_G && r + n < h.rows.size() && h.dst[r + n] == h.dst[r + n - 1] + p->LP) ++n;
                    runs.push_back({r, n});
                    r += n;
                }
                if (upload_groups(h, runs, &mask, &c.adjT, SCATTER_G, &ranges)) return bail(1);
            }
            c.adjT_host = HostEll();
            if (c.adjT.rmw.upload(mask) || c.adjT.rng.upload(ranges)) return bail(1);
            c.adjT.t.rng = c.adjT.rng;
            if (!env_on("SURFH_SCATTER_RMW_ALL", false)) c.adjT.t.rmw = c.adjT.rmw;        // 1: read-modify-write everywhere (A/B)
            c.adjT.host_dst.clear();
            c.adjT.host_dst.shrink_to_fit();
        }
        if (exact_ok && !p->ch.empty()) {      // dedicated accumulator, cleared once: the exact ranges keep it consistent
            const size_t ncube = (size_t)p->NBP * p->NAP * p->LP;
            if (p->gcube.zeros(ncube)) return bail(1);
        } else {
            for (auto &c : p->ch) {
                c.adjT.t.rng = nullptr;
                c.adjT.g.rng = nullptr;
            }
        }
    }
    if (p->io_x.alloc((size_t)p->isize) || p->io_y.alloc((size_t)p->osize) || p->cg_y.alloc((size_t)p->osize) || p->dscal.alloc(16) ||
        p->dscratch.alloc(std::max({(size_t)1024, launch_huber_vox_scratch_doubles(), launch_robust_scratch_doubles()})))
        return bail(1);
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail("device error during plan creation: %s", hipGetErrorString(hipGetLastError())));
    *out = p;
    return 0;
}

int64_t surfh_isize(const surfh_plan *p) { return p ? p->isize : -1; }
int64_t surfh_osize(const surfh_plan *p) { return p ? p->osize : -1; }
void *surfh_stream(const surfh_plan *p) { return p ? (void *)p->stream : nullptr; }

int surfh_set_prior(surfh_plan *p, int32_t kind) {
    if (!p) return fail("null plan");
    if (kind != 0 && kind != 1) return fail("prior kind %d: 0 = separated first differences, 1 = joint Laplacian", (int)kind);
    p->prior_kind = kind;
    return 0;
}
int surfh_set_potential(surfh_plan *p, int32_t slot, int32_t kind) {
    if (slot < 0 || slot > 2) return fail("potential slot %d: 0 = spatial prior, 1 = spectral prior, 2 = data term", (int)slot);
    if (kind < 0 || kind > 2) return fail("potential kind %d: 0 = huber, 1 = hyperbolic, 2 = hebert_leahy", (int)kind);
    if (!p) return fail("null plan");
    p->pot[slot] = kind;
    return 0;
}
int surfh_get_potential(const surfh_plan *p, int32_t slot) {
    if (slot < 0 || slot > 2) {
        fail("potential slot %d: 0 = spatial prior, 1 = spectral prior, 2 = data term", (int)slot);
        return -1;
    }
    if (!p) {
        fail("null plan");
        return -1;
    }
    return p->pot[slot];
}
int surfh_set_prior_coupling(surfh_plan *p, int32_t coupling) {
    if (coupling < 0 || coupling > 2) return fail("prior coupling %d: 0 = none, 1 = isotropic, 2 = vector", (int)coupling);
    if (!p) return fail("null plan");
    p->coupling = coupling;
    return 0;
}
int surfh_get_prior_coupling(const surfh_plan *p, int32_t *coupling) {
    if (!p || !coupling) return fail("null argument");
    *coupling = p->coupling;
    return 0;
}
// ---- data weights: plan state, like the prior ------------------------------------------------------------------------------------
namespace {
// installs the validated device weights w_new [osize] (taken over) or, with an empty buffer, clears the state; on failure the
// plan keeps what it had
int install_data_weights(surfh_plan *p, DevBuf<float> w_new) {
    std::vector<DevBuf<float>> wm(p->ch.size());
    DevBuf<float> wy;
    if (w_new) {
        hipStream_t s = p->stream;
        if (wy.alloc((size_t)p->osize)) return 1;
        for (size_t i = 0; i < p->ch.size(); ++i) {
            const Channel &c = p->ch[i];
            if (c.bsum || !c.ymat16) continue;
            if (wm[i].zeros((size_t)c.NP * c.LdetP, s)) return 1;
            if (launch_ymat_from_y(s, w_new + c.yoff, wm[i], c.P * c.S, c.Ldet, c.aout, c.LdetP) != 0) return fail("launch_ymat_from_y failed");
        }
    }
    if (hipStreamSynchronize(p->stream) != hipSuccess) return fail("stream synchronisation failed");   // nothing in flight reads the old buffers
    for (size_t i = 0; i < p->ch.size(); ++i) p->ch[i].wmat.swap(wm[i]);
    p->dwy.swap(wy);
    p->dw.swap(w_new);
    return 0;
}
int data_weights_check(surfh_plan *p) {
    if (!p) return fail("null plan");
    if (p->ch.empty() || p->osize <= 0) return fail("data weights need a plan with detector channels");
    HIP_OK(hipSetDevice(p->dev));
    return 0;
}
}  // namespace

int surfh_set_data_weights(surfh_plan *p, const float *w) {
    if (data_weights_check(p)) return 1;
    if (!w) return install_data_weights(p, {});
    for (long i = 0; i < p->osize; ++i)
        if (!(w[i] >= 0.f && w[i] <= FLT_MAX)) return fail("data weight %ld is %g: weights are finite and >= 0", i, (double)w[i]);
    DevBuf<float> wd;
    if (wd.alloc((size_t)p->osize)) return 1;
    if (hipMemcpyAsync(wd, w, p->osize * sizeof(float), hipMemcpyHostToDevice, p->stream) != hipSuccess) return fail("copy failed");
    return install_data_weights(p, std::move(wd));
}
int surfh_set_data_weights_dev(surfh_plan *p, const float *w_dev) {
    if (data_weights_check(p)) return 1;
    if (!w_dev) return install_data_weights(p, {});
    hipStream_t s = p->stream;
    DevBuf<float> wd;
    DevBuf<unsigned> cnt;
    unsigned bad = 0;
    if (wd.alloc((size_t)p->osize) || cnt.alloc(1)) return 1;
    const bool ok = hipMemcpyAsync(wd, w_dev, p->osize * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess &&
                    hipMemsetAsync(cnt, 0, sizeof(unsigned), s) == hipSuccess && launch_weight_count_bad(s, wd, p->osize, cnt) == 0 &&
                    hipMemcpyAsync(&bad, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    cnt.reset();
    if (!ok || bad) return ok ? fail("%u data weights are negative or not finite: weights are finite and >= 0", bad) : fail("data weight check failed");
    return install_data_weights(p, std::move(wd));
}
int surfh_has_data_weights(const surfh_plan *p) { return p && p->dw ? 1 : 0; }

// ---- diagnostics of the allocator (host code only) ---------------------------------------------------------------------------------
void surfh_debug_alloc_count(int64_t *live, int64_t *total) {
    if (live) *live = g_alloc_live.load();
    if (total) *total = g_alloc_total.load();
}
void surfh_debug_alloc_fail(int64_t nth) { g_alloc_fail_at.store(nth > 0 ? g_alloc_total.load() + nth : 0); }

}  // extern "C"
