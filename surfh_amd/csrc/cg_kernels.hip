// Vector kernels of the solvers: the quadratic priors, the CG blocks in three layouts (maps, planes, wavelength-innermost pn_*) and the
// plane-wise 3MG blocks (see kernels.h for the contracts).
#include "kernels.h"
#include "mm_step.h"
#include "prior_eig.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == RED_TPB, "the shared reductions of reduce_dev.h assume this block size");
static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");
}  // namespace

int nblocks(long n, int cap) {
    long b = (n + TPB - 1) / TPB;
    if (b < 1) b = 1;
    return (int)(b > cap ? cap : b);
}

namespace {
// dst[plane][ka][kb] = src * (f_self if kb = 0 or 2 kb = Nb, else f_pair): spectra <-> the solver's Parseval-scaled form
__global__ __launch_bounds__(TPB) void spec_scale_kernel(const float *__restrict__ src, float *__restrict__ dst, long PL, int KBP, int Nb, float f_self,
                                                         float f_pair) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= PL) return;
    const int kb = (int)(i % KBP);
    const long o = (long)blockIdx.y * PL + i;
    dst[o] = src[o] * ((kb == 0 || 2 * kb == Nb) ? f_self : f_pair);
}
}  // namespace

int launch_spec_scale(hipStream_t s, const float *src, float *dst, int planes, long PL, long KBP, int Nb, float f_self, float f_pair) {
    hipLaunchKernelGGL(spec_scale_kernel, dim3((unsigned)((PL + TPB - 1) / TPB), planes), dim3(TPB), 0, s, src, dst, PL, (int)KBP, Nb, f_self, f_pair);
    return (int)hipGetLastError();
}

namespace {
// q += mu_reg (Dr^T Dr + Dc^T Dc) d on half spectra: circular first differences are diagonal in the Fourier domain
__global__ __launch_bounds__(TPB) void spec_prior_add_kernel(const float *__restrict__ d, float *__restrict__ q, int Na, int Nb, long PL, int KBP,
                                                             float mu_reg) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= PL) return;
    const int kb = (int)(i % KBP), ka = (int)(i / KBP);
    if (ka >= Na || kb > Nb / 2) return;
    const long o = (long)blockIdx.y * PL + i;
    q[o] += mu_reg * (dsq(ka, Na) + dsq(kb, Nb)) * d[o];
}
}  // namespace

int launch_spec_prior_add(hipStream_t s, const float *d, float *q, int planes, int Na, int Nb, long PL, long KBP, float mu_reg) {
    hipLaunchKernelGGL(spec_prior_add_kernel, dim3((unsigned)((PL + TPB - 1) / TPB), planes), dim3(TPB), 0, s, d, q, Na, Nb, PL, (int)KBP, mu_reg);
    return (int)hipGetLastError();
}

namespace {
__global__ __launch_bounds__(TPB) void fill_zero_kernel(float *p, long n) {
    long i = (long)blockIdx.x * TPB + threadIdx.x;
    const long stride = (long)gridDim.x * TPB;
    for (; i < n; i += stride) p[i] = 0.f;      // 1.05 GB cube in 0.16 ms = 6.4 TB/s: at the roofline as it is
}
}  // namespace

int launch_fill_zero(hipStream_t s, float *p, long n) {
    hipLaunchKernelGGL(fill_zero_kernel, dim3(nblocks(n, 4096)), dim3(TPB), 0, s, p, n);
    return (int)hipGetLastError();
}

namespace {
// ---------------------------------------------------------------------------------------------
// CG vector kernels
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void prior_add_kernel(const float *__restrict__ d, float *__restrict__ q, int na,
                                                        int nb, float mu) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    const int i = blockIdx.y;
    const long t = blockIdx.z;
    if (j >= nb) return;
    const float *p = d + t * na * nb;
    const int im = (i == 0) ? na - 1 : i - 1, ip = (i == na - 1) ? 0 : i + 1;
    const int jm = (j == 0) ? nb - 1 : j - 1, jp = (j == nb - 1) ? 0 : j + 1;
    const float c = p[(long)i * nb + j];
    const float lap = (2.f * c - p[(long)im * nb + j] - p[(long)ip * nb + j]) +
                      (2.f * c - p[(long)i * nb + jm] - p[(long)i * nb + jp]);
    q[t * na * nb + (long)i * nb + j] += mu * lap;
}
}  // namespace

int launch_prior_add(hipStream_t s, const float *d, float *q, int T, int na, int nb, float mu_reg) {
    dim3 grid((nb + TPB - 1) / TPB, na, T);
    hipLaunchKernelGGL(prior_add_kernel, grid, dim3(TPB), 0, s, d, q, na, nb, mu_reg);
    return (int)hipGetLastError();
}

namespace {
// joint prior: q += mu * L^T L d with L the circular convolution by udft's 3 x 3 Laplacian [[0,-1,0],[-1,4,-1],[0,-1,0]]
// centred on the pixel (Difference_Operator_Joint.DtD, fusion_CT.py:45-62: |ir2fr(laplacian(2))|^2 in the Fourier domain).
// L is symmetric, L^T L is the 13-tap stencil 20 / -8 (axis neighbours) / 2 (diagonals) / 1 (axis distance 2).
__global__ __launch_bounds__(TPB) void prior_joint_add_kernel(const float *__restrict__ d, float *__restrict__ q, int na, int nb, float mu) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    const int i = blockIdx.y;
    const long t = blockIdx.z;
    if (j >= nb) return;
    const float *p = d + t * na * nb;
    auto wi = [&](int v) { return ((v % na) + na) % na; };
    auto wj = [&](int v) { return ((v % nb) + nb) % nb; };
    auto at = [&](int a, int b) { return p[(long)wi(a) * nb + wj(b)]; };
    const float v = 20.f * at(i, j) - 8.f * (at(i - 1, j) + at(i + 1, j) + at(i, j - 1) + at(i, j + 1)) +
                    2.f * (at(i - 1, j - 1) + at(i - 1, j + 1) + at(i + 1, j - 1) + at(i + 1, j + 1)) +
                    (at(i - 2, j) + at(i + 2, j) + at(i, j - 2) + at(i, j + 2));
    q[t * na * nb + (long)i * nb + j] += mu * v;
}
}  // namespace

int launch_prior_joint_add(hipStream_t s, const float *d, float *q, int T, int na, int nb, float mu_reg) {
    if (na < 3 || nb < 3) return (int)hipErrorInvalidValue;
    dim3 grid((nb + TPB - 1) / TPB, na, T);
    hipLaunchKernelGGL(prior_joint_add_kernel, grid, dim3(TPB), 0, s, d, q, na, nb, mu_reg);
    return (int)hipGetLastError();
}

namespace {
__global__ __launch_bounds__(TPB) void scale_kernel(float *x, long n, float a) {
    long i = (long)blockIdx.x * TPB + threadIdx.x;
    const long stride = (long)gridDim.x * TPB;
    for (; i < n; i += stride) x[i] *= a;
}
}  // namespace

int launch_scale(hipStream_t s, float *x, long n, float a) {
    hipLaunchKernelGGL(scale_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, x, n, a);
    return (int)hipGetLastError();
}

namespace {
// block_sum: reduce_dev.h
__global__ __launch_bounds__(TPB) void dot_partial_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                          long n, double *__restrict__ scratch) {
    double s = 0.0;
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) s += (double)a[i] * (double)b[i];
    s = block_sum(s);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}

__global__ __launch_bounds__(TPB) void reduce_final_kernel(const double *__restrict__ scratch, int nparts,
                                                           double *__restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += TPB) s += scratch[i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}
}  // namespace

int launch_dot(hipStream_t s, const float *a, const float *b, long n, double *scratch, double *out) {
    const int nb = nblocks(n, DOT_BLOCKS);
    hipLaunchKernelGGL(dot_partial_kernel, dim3(nb), dim3(TPB), 0, s, a, b, n, scratch);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(TPB), 0, s, scratch, nb, out);
    return (int)hipGetLastError();
}

namespace {
// ---- the CG vector updates of the map-domain and spectral loops, scalars read from the device.  A residual that is already
// zero (no data, every weight zero, or converged exactly) gives rr = d.q = 0: step and beta are then 0, not 0/0, and the iterate
// keeps still, as in the plane-wise kernels below.
__global__ __launch_bounds__(TPB) void cg_step_kernel(float *__restrict__ x, float *__restrict__ r,
                                                      const float *__restrict__ d, const float *__restrict__ q,
                                                      long n, const double *__restrict__ rr,
                                                      const double *__restrict__ dq, double *__restrict__ scratch) {
    const float step = dq[0] != 0.0 ? (float)(rr[0] / dq[0]) : 0.f;
    double s = 0.0;
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        x[i] += step * d[i];
        const float rn = r[i] - step * q[i];
        r[i] = rn;
        s += (double)rn * (double)rn;
    }
    s = block_sum(s);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}
}  // namespace

int launch_cg_step(hipStream_t s, float *x, float *r, const float *d, const float *q, long n, const double *rr,
                   const double *dq, double *scratch, double *out_rr) {
    const int nb = nblocks(n, DOT_BLOCKS);
    hipLaunchKernelGGL(cg_step_kernel, dim3(nb), dim3(TPB), 0, s, x, r, d, q, n, rr, dq, scratch);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(TPB), 0, s, scratch, nb, out_rr);
    return (int)hipGetLastError();
}

namespace {
__global__ __launch_bounds__(TPB) void cg_xupdate_kernel(float *__restrict__ x, const float *__restrict__ d, long n,
                                                         const double *__restrict__ rr,
                                                         const double *__restrict__ dq) {
    const float step = dq[0] != 0.0 ? (float)(rr[0] / dq[0]) : 0.f;
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) x[i] += step * d[i];
}
}  // namespace

int launch_cg_xupdate(hipStream_t s, float *x, const float *d, long n, const double *rr, const double *dq) {
    hipLaunchKernelGGL(cg_xupdate_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, x, d, n, rr, dq);
    return (int)hipGetLastError();
}

namespace {
__global__ __launch_bounds__(TPB) void cg_dir_kernel(float *__restrict__ d, const float *__restrict__ r, long n,
                                                     const double *__restrict__ rr_new,
                                                     const double *__restrict__ rr_old) {
    const float beta = rr_old[0] != 0.0 ? (float)(rr_new[0] / rr_old[0]) : 0.f;
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) d[i] = r[i] + beta * d[i];
}
}  // namespace

int launch_cg_dir(hipStream_t s, float *d, const float *r, long n, const double *rr_new, const double *rr_old) {
    hipLaunchKernelGGL(cg_dir_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, d, r, n, rr_new, rr_old);
    return (int)hipGetLastError();
}

// ---- CG iteration with device-resident scalars in three launches (dot partials, step, direction) and no copies: a launch sums
// the previous launch's per-block partial sums itself, every block for itself and in reduce_final_kernel's order (same bits),
// instead of waiting for a one-block reduction launch in between (parts_sum: reduce_dev.h).
// scratch: 2 * DOT_BLOCKS doubles.  dot(a, b) partials only (no reduction launch); the consumers below sum them
int launch_dot_parts(hipStream_t s, const float *a, const float *b, long n, double *parts) {
    hipLaunchKernelGGL(dot_partial_kernel, dim3(nblocks(n, DOT_BLOCKS)), dim3(TPB), 0, s, a, b, n, parts);
    return (int)hipGetLastError();
}

namespace {
// x += (rr / d.q) d;  r -= (rr / d.q) q;  partial sums of r.r;  d.q = the sum of `dq_parts`
__global__ __launch_bounds__(TPB) void cg_step_parts_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ d,
                                                            const float *__restrict__ q, long n, const double *__restrict__ rr,
                                                            const double *__restrict__ dq_parts, int nparts, double *__restrict__ dq_out,
                                                            double *__restrict__ scratch) {
    const double dq = parts_sum(dq_parts, nparts);
    if (blockIdx.x == 0 && threadIdx.x == 0) dq_out[0] = dq;
    const float step = dq != 0.0 ? (float)(rr[0] / dq) : 0.f;
    double s = 0.0;
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        x[i] += step * d[i];
        const float rn = r[i] - step * q[i];
        r[i] = rn;
        s += (double)rn * (double)rn;
    }
    s = block_sum(s);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}
}  // namespace

int launch_cg_step_parts(hipStream_t s, float *x, float *r, const float *d, const float *q, long n, const double *rr, const double *dq_parts,
                         double *dq_out, double *rr_parts) {
    const int nb = nblocks(n, DOT_BLOCKS);
    hipLaunchKernelGGL(cg_step_parts_kernel, dim3(nb), dim3(TPB), 0, s, x, r, d, q, n, rr, dq_parts, nb, dq_out, rr_parts);
    return (int)hipGetLastError();
}

namespace {
// rr' = the sum of `rr_parts` -> rr_out (a slot nobody reads in this launch);  d = r + (rr' / rr_old) d
__global__ __launch_bounds__(TPB) void cg_dir_parts_kernel(float *__restrict__ d, const float *__restrict__ r, long n,
                                                           const double *__restrict__ rr_parts, int nparts,
                                                           const double *__restrict__ rr_old, double *__restrict__ rr_out) {
    const double rrn = parts_sum(rr_parts, nparts);
    if (blockIdx.x == 0 && threadIdx.x == 0) rr_out[0] = rrn;
    const float beta = rr_old[0] != 0.0 ? (float)(rrn / rr_old[0]) : 0.f;
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) d[i] = r[i] + beta * d[i];
}
}  // namespace

int launch_cg_dir_parts(hipStream_t s, float *d, const float *r, long n, const double *rr_parts, const double *rr_old, double *rr_out) {
    hipLaunchKernelGGL(cg_dir_parts_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, d, r, n, rr_parts, nblocks(n, DOT_BLOCKS), rr_old, rr_out);
    return (int)hipGetLastError();
}
int dot_parts_stride() { return DOT_BLOCKS; }

namespace {
__global__ __launch_bounds__(TPB) void residual_kernel(float *__restrict__ r, const float *__restrict__ b,
                                                       const float *__restrict__ q, long n) {
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) r[i] = b[i] - q[i];
}
}  // namespace

int launch_residual(hipStream_t s, float *r, const float *b, const float *q, long n) {
    hipLaunchKernelGGL(residual_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, r, b, q, n);
    return (int)hipGetLastError();
}

namespace {
// ---- memory-gradient (3MG) vector kernels.  The subspace span{r, m} is handled in the basis [d, m] with d = r + beta m
// Q-orthogonal to the previous move m; the operator images are carried by linearity.
__global__ __launch_bounds__(TPB) void lincomb_kernel(float *__restrict__ out, const float *__restrict__ a,
                                                      const float *__restrict__ b, long n, float beta) {
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) out[i] = a[i] + beta * b[i];
}
}  // namespace

int launch_lincomb(hipStream_t s, float *out, const float *a, const float *b, long n, double beta) {
    hipLaunchKernelGGL(lincomb_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, out, a, b, n, (float)beta);
    return (int)hipGetLastError();
}

namespace {
__global__ __launch_bounds__(TPB) void mmmg_update_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ d,
                                                          float *__restrict__ m, float *__restrict__ qm,
                                                          const float *__restrict__ qd, long n, float s0, float s1, int update_r) {
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        const float mv = s0 * d[i] + s1 * m[i];
        const float qv = s0 * qd[i] + s1 * qm[i];
        x[i] += mv;
        m[i] = mv;
        qm[i] = qv;
        if (update_r) r[i] -= qv;
    }
}
}  // namespace

int launch_mmmg_update(hipStream_t s, float *x, float *r, const float *d, float *m, float *qm, const float *qd, long n, double s0,
                       double s1, int update_r) {
    hipLaunchKernelGGL(mmmg_update_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, x, r, d, m, qm, qd, n, (float)s0, (float)s1, update_r);
    return (int)hipGetLastError();
}

namespace {
// ---- CG on a batch of independent planes (the 2-D deconvolution path, one problem per wavelength): every plane has
// its own step and direction scalars.  One workgroup per plane; fp64 sums; a plane whose residual is already zero
// (no data, or converged exactly) keeps still.
__global__ __launch_bounds__(TPB) void dot_planes_kernel(const float *__restrict__ a, const float *__restrict__ b, long npix,
                                                         double *__restrict__ out) {
    const long off = (long)blockIdx.x * npix;
    double s = 0.0;
    for (long i = threadIdx.x; i < npix; i += TPB) s += (double)a[off + i] * (double)b[off + i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}
}  // namespace

int launch_dot_planes(hipStream_t s, const float *a, const float *b, int nplanes, long npix, double *out) {
    hipLaunchKernelGGL(dot_planes_kernel, dim3(nplanes), dim3(TPB), 0, s, a, b, npix, out);
    return (int)hipGetLastError();
}

namespace {
// x += s d ; (update_r) r -= s q, rr' = r.r      with s = rr / dq of this plane
__global__ __launch_bounds__(TPB) void cg_step_planes_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ d,
                                                             const float *__restrict__ q, long npix, const double *__restrict__ rr,
                                                             const double *__restrict__ dq, double *__restrict__ rrn, int update_r) {
    const long off = (long)blockIdx.x * npix;
    const double den = dq[blockIdx.x];
    const float step = den != 0.0 ? (float)(rr[blockIdx.x] / den) : 0.f;
    double s = 0.0;
    for (long i = threadIdx.x; i < npix; i += TPB) {
        x[off + i] += step * d[off + i];
        if (update_r) {
            const float rn = r[off + i] - step * q[off + i];
            r[off + i] = rn;
            s += (double)rn * (double)rn;
        }
    }
    if (update_r) {
        s = block_sum(s);
        if (threadIdx.x == 0) rrn[blockIdx.x] = s;
    }
}
}  // namespace

int launch_cg_step_planes(hipStream_t s, float *x, float *r, const float *d, const float *q, int nplanes, long npix, const double *rr,
                          const double *dq, double *rrn, int update_r) {
    hipLaunchKernelGGL(cg_step_planes_kernel, dim3(nplanes), dim3(TPB), 0, s, x, r, d, q, npix, rr, dq, rrn, update_r);
    return (int)hipGetLastError();
}

namespace {
// d = r + (rr' / rr) d per plane, then rr <- rr'
__global__ __launch_bounds__(TPB) void cg_dir_planes_kernel(float *__restrict__ d, const float *__restrict__ r, long npix,
                                                            const double *__restrict__ rrn, double *__restrict__ rr) {
    const long off = (long)blockIdx.x * npix;
    const double old = rr[blockIdx.x];
    const float beta = old != 0.0 ? (float)(rrn[blockIdx.x] / old) : 0.f;
    for (long i = threadIdx.x; i < npix; i += TPB) d[off + i] = r[off + i] + beta * d[off + i];
    __syncthreads();
    if (threadIdx.x == 0) rr[blockIdx.x] = rrn[blockIdx.x];
}
}  // namespace

int launch_cg_dir_planes(hipStream_t s, float *d, const float *r, int nplanes, long npix, const double *rrn, double *rr) {
    hipLaunchKernelGGL(cg_dir_planes_kernel, dim3(nplanes), dim3(TPB), 0, s, d, r, npix, rrn, rr);
    return (int)hipGetLastError();
}

namespace {
// ---- the same CG blocks on WAVELENGTH-INNERMOST arrays [NB rows beta][NAP][LP] (the plan's cube layout): the plane-wise solver keeps its
// vectors in the layout the transforms read and write, so an iteration holds no layout transpose.  A thread owns one wavelength
// and walks a slice of the pixels; the per-wavelength sums are formed in two deterministic stages (PN_SPLIT partial sums each).
constexpr int PN_SPLIT = 128;
__device__ __forceinline__ void pn_partial(double s, double *__restrict__ part, long LP, int l) {
    __shared__ double sm[TPB / 64][64];
    sm[threadIdx.x >> 6][threadIdx.x & 63] = s;
    __syncthreads();
    if (threadIdx.x < 64) {
        double t = 0.0;
        for (int w = 0; w < TPB / 64; ++w) t += sm[w][threadIdx.x];
        part[(long)blockIdx.y * LP + l] = t;
    }
}
// q += mu_reg (Dr^T Dr + Dc^T Dc) d (circular first differences, fusion_CT.py:16-43 / criterion_2D.py:16-43), part = d . q per wavelength
__global__ __launch_bounds__(TPB) void pn_prior_dot_kernel(const float *__restrict__ d, float *__restrict__ q, int Na, int Nb, int NAP, long LP,
                                                           float mu_reg, double *__restrict__ part) {
    const int l = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const long npix = (long)Na * Nb, p0 = npix * blockIdx.y / gridDim.y, p1 = npix * (blockIdx.y + 1) / gridDim.y;
    double s = 0.0;
    for (long pix = p0 + sub; pix < p1; pix += TPB / 64) {
        const int b = (int)(pix / Na), a = (int)(pix % Na);
        const long idx = ((long)b * NAP + a) * LP + l;
        const float dv = d[idx];
        float qv = q[idx];
        if (mu_reg != 0.f) {
            const int am = a ? a - 1 : Na - 1, ap = a + 1 < Na ? a + 1 : 0, bm = b ? b - 1 : Nb - 1, bp = b + 1 < Nb ? b + 1 : 0;
            const float lap = (2.f * dv - d[((long)b * NAP + am) * LP + l] - d[((long)b * NAP + ap) * LP + l]) +
                              (2.f * dv - d[((long)bm * NAP + a) * LP + l] - d[((long)bp * NAP + a) * LP + l]);
            qv += mu_reg * lap;
            q[idx] = qv;
        }
        s += (double)dv * (double)qv;
    }
    pn_partial(s, part, LP, l);
}
__global__ __launch_bounds__(TPB) void pn_dot_kernel(const float *__restrict__ x, const float *__restrict__ y, int Na, int Nb, int NAP, long LP,
                                                     double *__restrict__ part) {
    const int l = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const long npix = (long)Na * Nb, p0 = npix * blockIdx.y / gridDim.y, p1 = npix * (blockIdx.y + 1) / gridDim.y;
    double s = 0.0;
    for (long pix = p0 + sub; pix < p1; pix += TPB / 64) {
        const long idx = ((long)(pix / Na) * NAP + pix % Na) * LP + l;
        s += (double)x[idx] * (double)y[idx];
    }
    pn_partial(s, part, LP, l);
}
__global__ __launch_bounds__(TPB) void pn_reduce_kernel(const double *__restrict__ part, int S, long LP, double *__restrict__ out) {
    const long l = (long)blockIdx.x * TPB + threadIdx.x;
    if (l >= LP) return;
    double t = 0.0;
    for (int k = 0; k < S; ++k) t += part[(long)k * LP + l];
    out[l] = t;
}
}  // namespace

// the wavelength-innermost forms: part = work buffer of PN_SPLIT * LP doubles, out / rr / dq / rrn = [LP] doubles
int launch_pn_prior_dot(hipStream_t s, const float *d, float *q, int Na, int Nb, int NAP, long LP, float mu_reg, double *part, double *out) {
    if (LP % 64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pn_prior_dot_kernel, dim3((unsigned)(LP / 64), PN_SPLIT), dim3(TPB), 0, s, d, q, Na, Nb, NAP, LP, mu_reg, part);
    hipLaunchKernelGGL(pn_reduce_kernel, dim3((unsigned)((LP + TPB - 1) / TPB)), dim3(TPB), 0, s, part, PN_SPLIT, LP, out);
    return (int)hipGetLastError();
}
int launch_pn_dot(hipStream_t s, const float *x, const float *y, int Na, int Nb, int NAP, long LP, double *part, double *out) {
    if (LP % 64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pn_dot_kernel, dim3((unsigned)(LP / 64), PN_SPLIT), dim3(TPB), 0, s, x, y, Na, Nb, NAP, LP, part);
    hipLaunchKernelGGL(pn_reduce_kernel, dim3((unsigned)((LP + TPB - 1) / TPB)), dim3(TPB), 0, s, part, PN_SPLIT, LP, out);
    return (int)hipGetLastError();
}

namespace {
// x += s d ; (update_r) r -= s q, part = r . r      with s = rr / dq of the wavelength
__global__ __launch_bounds__(TPB) void pn_step_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ d, const float *__restrict__ q,
                                                      int Na, int Nb, int NAP, long LP, const double *__restrict__ rr, const double *__restrict__ dq,
                                                      double *__restrict__ part, int update_r) {
    const int l = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const long npix = (long)Na * Nb, p0 = npix * blockIdx.y / gridDim.y, p1 = npix * (blockIdx.y + 1) / gridDim.y;
    const double den = dq[l];
    const float step = den != 0.0 ? (float)(rr[l] / den) : 0.f;
    double s = 0.0;
    for (long pix = p0 + sub; pix < p1; pix += TPB / 64) {
        const long idx = ((long)(pix / Na) * NAP + pix % Na) * LP + l;
        x[idx] += step * d[idx];
        if (update_r) {
            const float rn = r[idx] - step * q[idx];
            r[idx] = rn;
            s += (double)rn * (double)rn;
        }
    }
    if (update_r) pn_partial(s, part, LP, l);
}
}  // namespace

int launch_pn_step(hipStream_t s, float *x, float *r, const float *d, const float *q, int Na, int Nb, int NAP, long LP, const double *rr,
                   const double *dq, double *part, double *rrn, int update_r) {
    if (LP % 64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pn_step_kernel, dim3((unsigned)(LP / 64), PN_SPLIT), dim3(TPB), 0, s, x, r, d, q, Na, Nb, NAP, LP, rr, dq, part, update_r);
    if (update_r) hipLaunchKernelGGL(pn_reduce_kernel, dim3((unsigned)((LP + TPB - 1) / TPB)), dim3(TPB), 0, s, part, PN_SPLIT, LP, rrn);
    return (int)hipGetLastError();
}

namespace {
// d = r + (rr' / rr) d per wavelength
__global__ __launch_bounds__(TPB) void pn_dir_kernel(float *__restrict__ d, const float *__restrict__ r, int Na, int Nb, int NAP, long LP,
                                                     const double *__restrict__ rrn, const double *__restrict__ rr) {
    const int l = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const long npix = (long)Na * Nb, p0 = npix * blockIdx.y / gridDim.y, p1 = npix * (blockIdx.y + 1) / gridDim.y;
    const double old = rr[l];
    const float beta = old != 0.0 ? (float)(rrn[l] / old) : 0.f;
    for (long pix = p0 + sub; pix < p1; pix += TPB / 64) {
        const long idx = ((long)(pix / Na) * NAP + pix % Na) * LP + l;
        d[idx] = r[idx] + beta * d[idx];
    }
}
}  // namespace

int launch_pn_dir(hipStream_t s, float *d, const float *r, int Na, int Nb, int NAP, long LP, const double *rrn, const double *rr) {
    if (LP % 64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pn_dir_kernel, dim3((unsigned)(LP / 64), PN_SPLIT), dim3(TPB), 0, s, d, r, Na, Nb, NAP, LP, rrn, rr);
    return (int)hipGetLastError();
}
size_t pn_part_doubles(long LP) { return (size_t)PN_SPLIT * (size_t)LP; }

namespace {
// ---- 3MG on a batch of independent planes (the 2-D deconvolution drivers select it: deconvolution_mrs_noRotation.py:199-212).
// Same two-step scheme as surfh_mmmg, every plane with its own scalars, one workgroup per plane (block_sum_bcast: reduce_dev.h).
// rr = r.r (trace), mQm kept for the step; d = r + beta m with beta = -(r.Qm)/(m.Qm)
__global__ __launch_bounds__(TPB) void mmmg_dir_planes_kernel(float *__restrict__ d, const float *__restrict__ r,
                                                              const float *__restrict__ m, const float *__restrict__ qm, long npix,
                                                              double *__restrict__ rr, double *__restrict__ mqm) {
    const long off = (long)blockIdx.x * npix;
    double v[3] = {0.0, 0.0, 0.0};
    for (long i = threadIdx.x; i < npix; i += TPB) {
        const double ri = r[off + i], qi = qm[off + i];
        v[0] += ri * ri;
        v[1] += ri * qi;
        v[2] += (double)m[off + i] * qi;
    }
    block_sum_bcast<3>(v);
    const float beta = v[2] > 0.0 ? (float)(-v[1] / v[2]) : 0.f;
    for (long i = threadIdx.x; i < npix; i += TPB) d[off + i] = r[off + i] + beta * m[off + i];
    if (threadIdx.x == 0) {
        rr[blockIdx.x] = v[0];
        mqm[blockIdx.x] = v[2];
    }
}
}  // namespace

int launch_mmmg_dir_planes(hipStream_t s, float *d, const float *r, const float *m, const float *qm, int nplanes, long npix,
                           double *rr, double *mqm) {
    hipLaunchKernelGGL(mmmg_dir_planes_kernel, dim3(nplanes), dim3(TPB), 0, s, d, r, m, qm, npix, rr, mqm);
    return (int)hipGetLastError();
}

namespace {
// 2x2 subspace step of every plane in the basis [d, m]; a plane without curvature (no data, or converged) keeps still
__global__ __launch_bounds__(TPB) void mmmg_step_planes_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ d,
                                                               float *__restrict__ m, float *__restrict__ qm,
                                                               const float *__restrict__ qd, long npix,
                                                               const double *__restrict__ mqm, int update_r) {
    const long off = (long)blockIdx.x * npix;
    double v[4] = {0.0, 0.0, 0.0, 0.0};                    // d.Qd, d.Qm, d.r, m.r
    for (long i = threadIdx.x; i < npix; i += TPB) {
        const double di = d[off + i], ri = r[off + i];
        v[0] += di * (double)qd[off + i];
        v[1] += di * (double)qm[off + i];
        v[2] += di * ri;
        v[3] += (double)m[off + i] * ri;
    }
    block_sum_bcast<4>(v);
    double s0, s1;
    mm_step2(v[0], v[1], mqm[blockIdx.x], v[2], v[3], &s0, &s1);
    const float f0 = (float)s0, f1 = (float)s1;
    for (long i = threadIdx.x; i < npix; i += TPB) {
        const float mv = f0 * d[off + i] + f1 * m[off + i];
        const float qv = f0 * qd[off + i] + f1 * qm[off + i];
        x[off + i] += mv;
        m[off + i] = mv;
        qm[off + i] = qv;
        if (update_r) r[off + i] -= qv;
    }
}
}  // namespace

int launch_mmmg_step_planes(hipStream_t s, float *x, float *r, const float *d, float *m, float *qm, const float *qd, int nplanes,
                            long npix, const double *mqm, int update_r) {
    hipLaunchKernelGGL(mmmg_step_planes_kernel, dim3(nplanes), dim3(TPB), 0, s, x, r, d, m, qm, qd, npix, mqm, update_r);
    return (int)hipGetLastError();
}
