// Exponential modified-Shepard resampling of scattered detector samples onto a regular grid
// (surfh/ToolsDir/shepard_interpolation.pyx:78-141, the resampling step of the slit distortion correction,
// surfh/Preprocessing/distorsion_correction.py:108-178).
//
// For every query point g of a segment and every sample k of the same segment:
//   d = sqrtf(((a_k - a_g) * inv_ares)^2 + ((l_k - l_g) * inv_lres)^2)    float32 throughout, sqrt rounded to float
//   if (double)d + (double)eps <= (double)cutoff:                          the reference adds and compares Python floats
//       w = (float)exp((float)(-alpha * exp(p * log((float)(d + eps)))))   d**p is the real part of a complex pow
//       num += w * v_k;  den += w                                          float32 accumulators
//   out[g] = den != 0 ? num / den : 0
// Every float operation is written with an explicit rounding intrinsic so that the compiler cannot contract a multiply and
// an add into one FMA, and the root is taken in double and stored to a float as the reference's generated C does (which
// rounds correctly; the float intrinsic __fsqrt_rn is the hardware's approximate root, an ulp off for some arguments):
// the include / exclude decision of each pair is the reference's, bit for bit.
//
// Instead of the reference's O(grid x samples) double loop, the samples of each segment are binned into square cells of
// the scaled (alpha, lambda) plane with side h >= cutoff * (1 + 1/64) (a counting sort keyed by segment and cell), and a
// query point tests only the samples of the 3 x 3 cells around its own.  The cell coordinates are computed in double
// from the float coordinates, so a pair the reference accepts (|scaled difference| <= cutoff * (1 + 1e-6) per axis) is
// never more than one cell apart: completeness does not depend on rounding at cell edges.  Within every cell, whatever
// its length, the samples are put back in input order (k_cell_sort for short cells, k_long_sort for the others), so the
// result does not depend on the order in which the binning's atomics arrive: the same input gives the same bits, alone
// or inside a batch.  The summation order differs from the reference's (cells, not input order), which moves the float
// sums by a few ulps.
//
// One launch serves any number of segments (every slit of one or several exposures).  A segment has its own samples,
// its own query points and its own inv_ares / inv_lres.  Query points are either a separable grid
// (n_lambda rows x n_alpha columns from per-segment axes, the layout of np.meshgrid(alpha, lambda)) or explicit lists.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/surfh_amd.h"
#include "dev_buf.h"

using surfh_impl::DevBuf;

namespace {

constexpr int TPB = 256;
constexpr int LONG_TPB = 1024;
// Cells of up to SORT_MAX samples are put in input order by one thread each (insertion sort, at most SORT_MAX^2 / 2 = 2048
// moves: real slits hold 5-25 samples per cell).  k_cell_sort lists the longer ones and k_long_sort gives each of them a
// workgroup: a bottom-up merge sort in which every element finds its place in the merged run by a binary search of the
// sibling run.  For a cell of n samples that is ceil(log2 n) passes of n / LONG_TPB elements per thread and at most
// log2 n probes each, n log2^2 n / LONG_TPB steps per thread: 12 passes x 4 elements x 12 probes, about 600 steps, for
// n = 4096, and about 2e5 steps if all 5e5 samples of a full exposure fell into one cell (tens of milliseconds).  Nothing
// grows as n^2.  An exposure without a long cell pays one counter in k_scan and one comparison per cell.
constexpr int SORT_MAX = 64;

thread_local std::string g_shep_err;
int sfail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_shep_err = buf;
    return 1;
}
#define S_OK(x)                                                                                    \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return sfail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// per-segment geometry; the cell grid is filled by k_seg_setup, `base` by the host
struct Seg {
    long p0, p1;          // samples [p0, p1)
    long q0;              // first query point (= first output)
    long ga0, gl0;        // first alpha / lambda coordinate of a separable grid
    int na, nl;           // query grid: nl rows x na columns
    float inv_a, inv_l;
    double a0, l0, h;     // cell origin (float coordinates) and cell side (scaled units)
    int nx, ny;           // cells along alpha / lambda (0: no finite sample)
    long base;            // first cell of the segment in the global cell list
};

__device__ __forceinline__ bool finite_pt(float a, float l) { return isfinite(a) && isfinite(l); }

// bounding box of the segment's finite samples and the cell grid over it (one block per segment)
__global__ void k_seg_setup(Seg *segs, const float *__restrict__ pa, const float *__restrict__ pl, float cutoff) {
    Seg &s = segs[blockIdx.x];
    __shared__ double red[4][TPB];
    __shared__ int cnt[TPB];
    double amin = INFINITY, amax = -INFINITY, lmin = INFINITY, lmax = -INFINITY;
    int n = 0;
    for (long i = s.p0 + threadIdx.x; i < s.p1; i += TPB) {
        const float a = pa[i], l = pl[i];
        if (!finite_pt(a, l)) continue;
        amin = fmin(amin, (double)a); amax = fmax(amax, (double)a);
        lmin = fmin(lmin, (double)l); lmax = fmax(lmax, (double)l);
        ++n;
    }
    red[0][threadIdx.x] = amin; red[1][threadIdx.x] = -amax; red[2][threadIdx.x] = lmin; red[3][threadIdx.x] = -lmax;
    cnt[threadIdx.x] = n;
    __syncthreads();
    for (int w = TPB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = fmin(red[c][threadIdx.x], red[c][threadIdx.x + w]);
            cnt[threadIdx.x] += cnt[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x) return;
    const long nv = cnt[0];
    const double ia = fabs((double)s.inv_a), il = fabs((double)s.inv_l);
    s.nx = s.ny = 0;
    s.a0 = red[0][0]; s.l0 = red[2][0];
    if (nv == 0 || !isfinite(ia) || !isfinite(il)) return;   // no sample, or every distance is inf / NaN: out = 0
    const double sx = (-red[1][0] - red[0][0]) * ia, sy = (-red[3][0] - red[2][0]) * il;
    double h = fmax((double)cutoff, 1e-30) * (1.0 + 1.0 / 64);
    const double cap = 4.0 * (double)nv + 1024.0;            // cells per segment: at most ~4 per sample
    while ((floor(sx / h) + 1.0) * (floor(sy / h) + 1.0) > cap) h *= 2.0;
    s.h = h;
    s.nx = (int)floor(sx / h) + 1;
    s.ny = (int)floor(sy / h) + 1;
}

__device__ __forceinline__ int seg_of(const long *off, int n_seg, long i) {     // off[s] <= i < off[s + 1]
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int cell_coord(double x, double h, int n) {            // x within the segment's bounding box
    return (int)fmin(fmax(floor(x / h), 0.0), (double)(n - 1));
}

// global cell of each sample (-1: non-finite coordinates) and the per-cell counts
__global__ void k_bin(const Seg *__restrict__ segs, const long *__restrict__ poff, int n_seg, long n_pts,
                      const float *__restrict__ pa, const float *__restrict__ pl, int *__restrict__ cell,
                      int *__restrict__ count) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_pts) return;
    const Seg &s = segs[seg_of(poff, n_seg, i)];
    const float a = pa[i], l = pl[i];
    if (s.nx == 0 || !finite_pt(a, l)) { cell[i] = -1; return; }
    const int cx = cell_coord(((double)a - s.a0) * fabs((double)s.inv_a), s.h, s.nx);
    const int cy = cell_coord(((double)l - s.l0) * fabs((double)s.inv_l), s.h, s.ny);
    const int c = (int)(s.base + (long)cy * s.nx + cx);
    cell[i] = c;
    atomicAdd(&count[c], 1);
}

// exclusive scan of count[0..n) into start[0..n] (one block; the cell list is at most a few million long)
__global__ void k_scan(const int *__restrict__ count, int *__restrict__ start, int n) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const long chunk = ((long)n + 1023) / 1024;
    const int b = (int)min((long)n, t * chunk), e = (int)min((long)n, b + chunk);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += count[i];
    part[t] = sum;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {            // Hillis-Steele inclusive scan of the partial sums
        const int v = t >= w ? part[t - w] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int i = b; i < e; ++i) { start[i] = run; run += count[i]; }
    if (t == 1023) {
        start[n] = part[1023];
        start[n + 1] = 0;                           // the number of long cells, counted by k_cell_sort
    }
}

__global__ void k_scatter(const int *__restrict__ cell, long n_pts, const int *__restrict__ start, int *__restrict__ fill,
                          int *__restrict__ order) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_pts) return;
    const int c = cell[i];
    if (c < 0) return;
    order[start[c] + atomicAdd(&fill[c], 1)] = (int)i;
}

// restore input order inside each cell (the atomics above hand out slots in any order); a cell of more than SORT_MAX
// samples is appended to long_cells[] (any order), counted in start[n_cells + 1], and left to k_long_sort
__global__ void k_cell_sort(int *__restrict__ start, int n_cells, int *__restrict__ order, int *__restrict__ long_cells) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= n_cells) return;
    const int b = start[c], e = start[c + 1];
    if (e - b > SORT_MAX) {
        long_cells[atomicAdd(&start[n_cells + 1], 1)] = c;
        return;
    }
    for (int i = b + 1; i < e; ++i) {
        const int v = order[i];
        int j = i - 1;
        while (j >= b && order[j] > v) { order[j + 1] = order[j]; --j; }
        order[j + 1] = v;
    }
}

// input order inside one long cell per block: bottom-up merge sort between order[b, b + n) and the same range of tmp[].
// The sample indices of a cell are distinct, so an element's place in the merged pair of runs is its offset in its own
// run plus the number of smaller elements in the sibling run.
__global__ __launch_bounds__(LONG_TPB) void k_long_sort(const int *__restrict__ start, const int *__restrict__ long_cells,
                                                        int *order, int *tmp) {
    const int c = long_cells[blockIdx.x];
    const long b = start[c], n = start[c + 1] - b;
    int *src = order + b, *dst = tmp + b;
    for (long w = 1; w < n; w <<= 1) {
        for (long i = threadIdx.x; i < n; i += LONG_TPB) {
            const long pair = i / (2 * w) * (2 * w), mid = min(pair + w, n);
            const bool left = i < mid;
            long lo = left ? mid : pair, hi = left ? min(mid + w, n) : mid;      // the sibling run
            const long sib = lo;
            const int v = src[i];
            while (lo < hi) {
                const long m = (lo + hi) >> 1;
                if (src[m] < v) lo = m + 1; else hi = m;
            }
            dst[pair + (i - (left ? pair : mid)) + (lo - sib)] = v;
        }
        __syncthreads();
        int *t = src; src = dst; dst = t;
    }
    if (src != order + b)
        for (long i = threadIdx.x; i < n; i += LONG_TPB) dst[i] = src[i];
}

__global__ void k_gather(const int *__restrict__ order, int n, const float *__restrict__ pa, const float *__restrict__ pl,
                         const float *__restrict__ pv, float4 *__restrict__ sorted) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int k = order[i];
    sorted[i] = make_float4(pa[k], pl[k], pv[k], 0.f);
}

#pragma clang fp contract(off)
// one thread per query point; consecutive lanes are consecutive points of one grid row, so a wave reads the same few
// cells and the sample loads are served by the cache
__global__ __launch_bounds__(TPB) void k_shepard(const Seg *__restrict__ segs, const long *__restrict__ qoff, int n_seg,
                                                 long n_q, int separable, const float *__restrict__ qa,
                                                 const float *__restrict__ ql, const int *__restrict__ start,
                                                 const float4 *__restrict__ sorted, float p, float alpha, float cutoff,
                                                 float eps, float *__restrict__ out, int *__restrict__ nbr) {
    const long q = (long)blockIdx.x * TPB + threadIdx.x;
    if (q >= n_q) return;
    const Seg &s = segs[seg_of(qoff, n_seg, q)];
    const long loc = q - s.q0;
    float ga, gl;
    if (separable) {
        ga = qa[s.ga0 + loc % s.na];
        gl = ql[s.gl0 + loc / s.na];
    } else {
        ga = qa[q];
        gl = ql[q];
    }
    float num = 0.f, den = 0.f;
    int hits = 0;
    const double xq = ((double)ga - s.a0) * fabs((double)s.inv_a), yq = ((double)gl - s.l0) * fabs((double)s.inv_l);
    if (s.nx > 0 && isfinite(xq) && isfinite(yq)) {
        // cells fx-1..fx+1, clipped to the grid in double before any conversion (a query may lie far outside)
        const double fx = floor(xq / s.h), fy = floor(yq / s.h);
        const double xlo = fmax(fx - 1.0, 0.0), xhi = fmin(fx + 1.0, (double)(s.nx - 1));
        const double ylo = fmax(fy - 1.0, 0.0), yhi = fmin(fy + 1.0, (double)(s.ny - 1));
        const bool any = xlo <= xhi && ylo <= yhi;
        const int x0 = any ? (int)xlo : 0, x1 = any ? (int)xhi : -1, y0 = any ? (int)ylo : 0, y1 = any ? (int)yhi : -1;
        const double dcut = (double)cutoff, deps = (double)eps, dp = (double)p, dal = (double)alpha;
        for (int cy = y0; cy <= y1; ++cy) {
            const long row = s.base + (long)cy * s.nx;
            const int e = start[row + x1 + 1];
            for (int k = start[row + x0]; k < e; ++k) {     // the 1-3 cells of a row are contiguous
                const float4 pt = sorted[k];
                const float d1 = __fmul_rn(__fsub_rn(pt.x, ga), s.inv_a);
                const float d2 = __fmul_rn(__fsub_rn(pt.y, gl), s.inv_l);
                // the reference's double sqrt stored to a float, which is the correctly rounded float root;
                // __fsqrt_rn is the hardware's approximate root here and moves d by an ulp
                const float d = (float)sqrt((double)__fadd_rn(__fmul_rn(d1, d1), __fmul_rn(d2, d2)));
                const double dist = (double)d + deps;
                if (dist <= dcut) {
                    const float df = (float)dist;
                    const float value = (float)(-dal * exp(dp * log((double)df)));
                    const float w = (float)exp((double)value);
                    num = __fadd_rn(num, __fmul_rn(w, pt.z));
                    den = __fadd_rn(den, w);
                    ++hits;
                }
            }
        }
    }
    out[q] = den != 0.f ? __fdiv_rn(num, den) : 0.f;
    if (nbr) nbr[q] = hits;
}
#pragma clang fp contract(on)

#define S_ALLOC(expr)                                                                              \
    do {                                                                                           \
        if (expr) return sfail("%s", surfh_last_error());       /* the allocator's message, in this module's error string */ \
    } while (0)

inline unsigned blocks(long n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

extern "C" {

const char *surfh_shepard_last_error(void) { return g_shep_err.c_str(); }

int surfh_shepard(int32_t n_seg, const int64_t *pt_off, const float *pt_alpha, const float *pt_lambda,
                  const float *pt_value, const int32_t *n_alpha, const int32_t *n_lambda, int32_t separable,
                  const float *q_alpha, const float *q_lambda, const float *inv_alpha_res, const float *inv_lambda_res,
                  float p, float alpha, float pixel_cutoff, float epsilon, float *out, int32_t *neighbours,
                  int32_t device_ptrs, void *stream, float *kernel_ms) {
    if (n_seg < 1 || !pt_off || !n_alpha || !n_lambda || !inv_alpha_res || !inv_lambda_res || !out)
        return sfail("surfh_shepard: bad arguments");
    if (pt_off[0] != 0) return sfail("surfh_shepard: pt_off[0] must be 0");
    std::vector<Seg> segs(n_seg);
    std::vector<long> qoff(n_seg + 1, 0);
    long ga = 0, gl = 0;
    for (int s = 0; s < n_seg; ++s) {
        if (pt_off[s + 1] < pt_off[s]) return sfail("surfh_shepard: pt_off must be non-decreasing (segment %d)", s);
        if (n_alpha[s] < 0 || n_lambda[s] < 0) return sfail("surfh_shepard: negative grid size (segment %d)", s);
        Seg &g = segs[s];
        g = Seg{};
        g.p0 = pt_off[s]; g.p1 = pt_off[s + 1];
        g.q0 = qoff[s];
        g.na = n_alpha[s]; g.nl = n_lambda[s];
        g.ga0 = ga; g.gl0 = gl;
        g.inv_a = inv_alpha_res[s]; g.inv_l = inv_lambda_res[s];
        ga += g.na; gl += g.nl;
        qoff[s + 1] = qoff[s] + (long)g.na * g.nl;
    }
    const long n_pts = pt_off[n_seg], n_q = qoff[n_seg];
    if (n_pts > 0x7fffffffL || n_q > 0x7fffffffL) return sfail("surfh_shepard: more than 2^31 samples or query points");
    if (n_q == 0) return 0;
    if (n_pts > 0 && (!pt_alpha || !pt_lambda || !pt_value)) return sfail("surfh_shepard: null sample array");
    if (!q_alpha || !q_lambda) return sfail("surfh_shepard: null query array");
    const long nqa = separable ? ga : n_q, nql = separable ? gl : n_q;

    hipStream_t st = (hipStream_t)stream;
    DevBuf<float> a, l, v, xa, xl, sout;         // host arrays staged on the device
    DevBuf<int> snbr;
    const float *da = pt_alpha, *dl = pt_lambda, *dv = pt_value, *dqa = q_alpha, *dql = q_lambda;
    float *dout = out;
    int *dnbr = neighbours;
    if (!device_ptrs) {        // host arrays: stage them on the device
        S_ALLOC(a.alloc(n_pts) || l.alloc(n_pts) || v.alloc(n_pts) || xa.alloc(nqa) || xl.alloc(nql) || sout.alloc(n_q));
        dout = sout;
        if (n_pts) {
            S_OK(hipMemcpyAsync(a, pt_alpha, n_pts * 4, hipMemcpyHostToDevice, st));
            S_OK(hipMemcpyAsync(l, pt_lambda, n_pts * 4, hipMemcpyHostToDevice, st));
            S_OK(hipMemcpyAsync(v, pt_value, n_pts * 4, hipMemcpyHostToDevice, st));
        }
        if (nqa) S_OK(hipMemcpyAsync(xa, q_alpha, nqa * 4, hipMemcpyHostToDevice, st));
        if (nql) S_OK(hipMemcpyAsync(xl, q_lambda, nql * 4, hipMemcpyHostToDevice, st));
        da = a; dl = l; dv = v; dqa = xa; dql = xl;
        dnbr = nullptr;
        if (neighbours) {
            S_ALLOC(snbr.alloc(n_q));
            dnbr = snbr;
        }
    }
    DevBuf<Seg> dseg;
    DevBuf<long> dpoff, dqoff;
    S_ALLOC(dseg.alloc(n_seg) || dpoff.alloc(n_seg + 1) || dqoff.alloc(n_seg + 1));
    std::vector<long> poff(pt_off, pt_off + n_seg + 1);
    S_OK(hipMemcpyAsync(dseg, segs.data(), n_seg * sizeof(Seg), hipMemcpyHostToDevice, st));
    S_OK(hipMemcpyAsync(dpoff, poff.data(), (n_seg + 1) * sizeof(long), hipMemcpyHostToDevice, st));
    S_OK(hipMemcpyAsync(dqoff, qoff.data(), (n_seg + 1) * sizeof(long), hipMemcpyHostToDevice, st));

    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (kernel_ms) {
        S_OK(hipEventCreate(&e0)); S_OK(hipEventCreate(&e1));
        S_OK(hipEventRecord(e0, st));
    }
    // cell grids: the host needs their sizes to lay out the cell list (one small read-back)
    k_seg_setup<<<n_seg, TPB, 0, st>>>(dseg, da, dl, pixel_cutoff);
    S_OK(hipGetLastError());
    S_OK(hipMemcpyAsync(segs.data(), dseg, n_seg * sizeof(Seg), hipMemcpyDeviceToHost, st));
    S_OK(hipStreamSynchronize(st));
    long n_cells = 0;
    for (Seg &g : segs) {
        g.base = n_cells;
        n_cells += (long)g.nx * g.ny;
    }
    if (n_cells > 0x7fffffffL) return sfail("surfh_shepard: cell list too long (%ld cells)", n_cells);
    S_OK(hipMemcpyAsync(dseg, segs.data(), n_seg * sizeof(Seg), hipMemcpyHostToDevice, st));

    DevBuf<int> cell, count, start, fill, order;
    DevBuf<float4> sorted;
    S_ALLOC(cell.alloc(n_pts) || count.alloc(n_cells) || fill.alloc(n_cells) || start.alloc(n_cells + 2) || order.alloc(n_pts) || sorted.alloc(n_pts));
    S_OK(hipMemsetAsync(count, 0, std::max(n_cells, 1L) * sizeof(int), st));
    S_OK(hipMemsetAsync(fill, 0, std::max(n_cells, 1L) * sizeof(int), st));
    if (n_pts) {
        k_bin<<<blocks(n_pts), TPB, 0, st>>>(dseg, dpoff, n_seg, n_pts, da, dl, cell, count);
        S_OK(hipGetLastError());
    }
    k_scan<<<1, 1024, 0, st>>>(count, start, (int)n_cells);
    S_OK(hipGetLastError());
    if (n_pts) {
        k_scatter<<<blocks(n_pts), TPB, 0, st>>>(cell, n_pts, start, fill, order);
        S_OK(hipGetLastError());
    }
    if (n_cells) {
        k_cell_sort<<<blocks(n_cells), TPB, 0, st>>>(start, (int)n_cells, order, fill);    // fill[] is free again: the list
        S_OK(hipGetLastError());
    }
    // order[] holds the binned samples only (non-finite ones are left out): gather that many
    int tail[2] = {0, 0};                            // binned samples, long cells
    S_OK(hipMemcpyAsync(tail, start + n_cells, sizeof tail, hipMemcpyDeviceToHost, st));
    S_OK(hipStreamSynchronize(st));
    const int n_binned = tail[0], n_long = tail[1];
    if (n_long) {                                    // cell[] is free after k_scatter: the merge sort's second buffer
        k_long_sort<<<n_long, LONG_TPB, 0, st>>>(start, fill, order, cell);
        S_OK(hipGetLastError());
    }
    if (n_binned) {
        k_gather<<<blocks(n_binned), TPB, 0, st>>>(order, n_binned, da, dl, dv, sorted);
        S_OK(hipGetLastError());
    }
    k_shepard<<<blocks(n_q), TPB, 0, st>>>(dseg, dqoff, n_seg, n_q, separable ? 1 : 0, dqa, dql, start, sorted, p, alpha,
                                           pixel_cutoff, epsilon, dout, dnbr);
    S_OK(hipGetLastError());
    if (kernel_ms) {
        S_OK(hipEventRecord(e1, st));
        S_OK(hipEventSynchronize(e1));
        S_OK(hipEventElapsedTime(kernel_ms, e0, e1));
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    if (!device_ptrs) {
        S_OK(hipMemcpyAsync(out, dout, n_q * 4, hipMemcpyDeviceToHost, st));
        if (neighbours) S_OK(hipMemcpyAsync(neighbours, dnbr, n_q * 4, hipMemcpyDeviceToHost, st));
    }
    S_OK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
