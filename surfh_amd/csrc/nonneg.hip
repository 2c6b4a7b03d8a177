// Non-negative fusion (ADMM in scaled form on the CG frame; the loop: nn_loop, plan_solvers.hip), the device kernels and their launchers.
//   min x^T Q x / 2 - b^T x  subject to  x >= 0   split as  x = z, z >= 0,  scaled dual u,  v = z - u:
//   x  <-  (Q + rho I)^-1 (b + rho v)     `inner` CG iterations on the carried residual
//   z' = max(x + u, 0);  u' = u + x - z';  v' = z' - u'        nn_project, one pass, with the sums of an outer iteration's trace
// and the residual of the next inner system follows from the carried one: r += rho (v' - v) (fused into the pass, or left in dv
// where r lives in another basis).  nn_add is the rho I of the operator and every other axpy of the loop.
// The plane-wise deconvolution (nn_planes_loop, surfh_cg_planes_nonneg) runs L such problems at once on [L][npix] vectors with one
// penalty per plane: nn_project_planes is the fused pass with per-plane sums [4][L] (S blocks a plane, their partial sums added
// per plane in a fixed order by a second kernel: no atomics, the same bits for the same inputs), nn_add_planes the axpy with a
// per-plane coefficient.  Both choose the 16-byte path plane by plane: a plane base is aligned only when npix % 4 == 0, or by chance.
#include "plan_internal.h"
#include "reduce_dev.h"

namespace {
constexpr int NN_MAX_BLOCKS = 256;       // 4 sums x 256 partials: the 1024 doubles every plan's dscratch holds

enum { NN_PLAIN = 0, NN_FUSED = 1, NN_DV = 2 };

// one element: t = x + u, z' = t > 0 ? t : 0 (never a set sign bit; NaN goes to 0), u' = t - z' (0 where t > 0, t elsewhere: exact),
// w = rho ((z' - u') - (z - u)).  acc: |x - z'|^2, |z' - z|^2, #{z' == 0}, and the new r.r (NN_FUSED), in float64
template <int MODE>
__device__ __forceinline__ void nn_element(float x, float &z, float &u, float &w, float rho, double (&acc)[4]) {
    const float t = x + u;
    const float zn = t > 0.f ? t : 0.f;
    const float un = t - zn;
    const float dv = rho * ((zn - un) - (z - u));
    const double ex = (double)x - (double)zn, ez = (double)zn - (double)z;
    acc[0] += ex * ex;
    acc[1] += ez * ez;
    acc[2] += zn == 0.f ? 1.0 : 0.0;
    if constexpr (MODE == NN_FUSED) {
        w += dv;
        acc[3] += (double)w * (double)w;
    } else {
        w = dv;
    }
    z = zn;
    u = un;
}

// `vec`: every pointer is 16-byte aligned and the whole groups of four go through 16-byte accesses; the tail, and everything where
// a pointer is not aligned, takes the scalar path.  w: r (NN_FUSED, read and written), dv (NN_DV, written) or unused.
// part[k * gridDim.x + block]: the block's sum k
template <int MODE>
__global__ __launch_bounds__(RED_TPB) void nn_project_kernel(const float *x, float *z, float *u, float *w, long n, float rho, int vec,
                                                             double *__restrict__ part) {
    const long stride = (long)gridDim.x * RED_TPB, tid = (long)blockIdx.x * RED_TPB + threadIdx.x;
    const long n4 = vec ? n / 4 : 0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long c = tid; c < n4; c += stride) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[c];
        float4 zv = reinterpret_cast<float4 *>(z)[c], uv = reinterpret_cast<float4 *>(u)[c], wv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE == NN_FUSED) wv = reinterpret_cast<float4 *>(w)[c];
        nn_element<MODE>(xv.x, zv.x, uv.x, wv.x, rho, acc);
        nn_element<MODE>(xv.y, zv.y, uv.y, wv.y, rho, acc);
        nn_element<MODE>(xv.z, zv.z, uv.z, wv.z, rho, acc);
        nn_element<MODE>(xv.w, zv.w, uv.w, wv.w, rho, acc);
        reinterpret_cast<float4 *>(z)[c] = zv;
        reinterpret_cast<float4 *>(u)[c] = uv;
        if constexpr (MODE != NN_PLAIN) reinterpret_cast<float4 *>(w)[c] = wv;
    }
    for (long i = 4 * n4 + tid; i < n; i += stride) {
        float zi = z[i], ui = u[i], wi = 0.f;
        if constexpr (MODE == NN_FUSED) wi = w[i];
        nn_element<MODE>(x[i], zi, ui, wi, rho, acc);
        z[i] = zi;
        u[i] = ui;
        if constexpr (MODE != NN_PLAIN) w[i] = wi;
    }
    block_sums_to<4>(acc, part);
}

// out += c (a - b)   (b NULL: out += c a)
__global__ __launch_bounds__(RED_TPB) void nn_add_kernel(float *__restrict__ out, const float *__restrict__ a, const float *__restrict__ b, long n,
                                                         float c) {
    const long stride = (long)gridDim.x * RED_TPB;
    for (long i = (long)blockIdx.x * RED_TPB + threadIdx.x; i < n; i += stride) out[i] += c * (b ? a[i] - b[i] : a[i]);
}

inline bool aligned16(const void *q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; }

// ---- the same on L independent planes ([L][npix] vectors, plane-major: the layout of planes_space), one penalty per plane ----
// Grid (S, L): S blocks share a plane, a thread takes one group of four or one float per trip.  The 16-byte path is chosen per
// plane, from the plane's own base pointers: with npix % 4 != 0 only some planes of an aligned vector are aligned themselves.
constexpr int NN_PL_TRIPS = 4;           // trips a thread is sized for (a wave's trip: 1 KiB of each vector on the 16-byte path)
constexpr int NN_PL_MAX_SPLIT = 64;      // blocks per plane at most: the partial sums the second stage adds per plane and sum

__device__ __forceinline__ bool dev_aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// part[(k L + l) S + block]: the block's sum k of plane l;  k = |x - z'|^2, |z' - z|^2, #{z' == 0}, the new r.r
__global__ __launch_bounds__(RED_TPB) void nn_project_planes_kernel(const float *xa, float *za, float *ua, float *ra, long npix,
                                                                    const float *__restrict__ rho_l, double *__restrict__ part) {
    const int l = blockIdx.y, S = gridDim.x;
    const long off = (long)l * npix;
    const float *x = xa + off;
    float *z = za + off, *u = ua + off, *r = ra + off;
    const float rho = rho_l[l];
    const bool vec = dev_aligned16(x) && dev_aligned16(z) && dev_aligned16(u) && dev_aligned16(r);
    const long stride = (long)S * RED_TPB, tid = (long)blockIdx.x * RED_TPB + threadIdx.x;
    const long n4 = vec ? npix / 4 : 0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long c = tid; c < n4; c += stride) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[c];
        float4 zv = reinterpret_cast<float4 *>(z)[c], uv = reinterpret_cast<float4 *>(u)[c], wv = reinterpret_cast<float4 *>(r)[c];
        nn_element<NN_FUSED>(xv.x, zv.x, uv.x, wv.x, rho, acc);
        nn_element<NN_FUSED>(xv.y, zv.y, uv.y, wv.y, rho, acc);
        nn_element<NN_FUSED>(xv.z, zv.z, uv.z, wv.z, rho, acc);
        nn_element<NN_FUSED>(xv.w, zv.w, uv.w, wv.w, rho, acc);
        reinterpret_cast<float4 *>(z)[c] = zv;
        reinterpret_cast<float4 *>(u)[c] = uv;
        reinterpret_cast<float4 *>(r)[c] = wv;
    }
    for (long i = 4 * n4 + tid; i < npix; i += stride) {
        float zi = z[i], ui = u[i], wi = r[i];
        nn_element<NN_FUSED>(x[i], zi, ui, wi, rho, acc);
        z[i] = zi;
        u[i] = ui;
        r[i] = wi;
    }
    block_sums_to<4>(acc, part, l * S + (int)blockIdx.x, (int)gridDim.y * S);
}
// sums[k L + l] = the S partial sums of (k, l) in their order: one thread each
__global__ __launch_bounds__(RED_TPB) void nn_planes_reduce_kernel(const double *__restrict__ part, int S, int rows, double *__restrict__ sums) {
    const int j = blockIdx.x * RED_TPB + threadIdx.x;
    if (j >= rows) return;
    double t = 0.0;
    for (int k = 0; k < S; ++k) t += part[(long)j * S + k];
    sums[j] = t;
}
// out_l += (scale c_l) (a_l - b_l)   (b NULL: out_l += (scale c_l) a_l)
__global__ __launch_bounds__(RED_TPB) void nn_add_planes_kernel(float *outa, const float *aa, const float *ba, long npix,
                                                                const float *__restrict__ c_l, float scale) {
    const long off = (long)blockIdx.y * npix;
    float *out = outa + off;
    const float *a = aa + off, *b = ba ? ba + off : nullptr;
    const float c = scale * c_l[blockIdx.y];
    const bool vec = dev_aligned16(out) && dev_aligned16(a) && dev_aligned16(b);       // a null b counts as aligned
    const long stride = (long)gridDim.x * RED_TPB, tid = (long)blockIdx.x * RED_TPB + threadIdx.x;
    const long n4 = vec ? npix / 4 : 0;
    for (long k = tid; k < n4; k += stride) {
        float4 o = reinterpret_cast<float4 *>(out)[k];
        float4 v = reinterpret_cast<const float4 *>(a)[k];
        if (b) {
            const float4 w = reinterpret_cast<const float4 *>(b)[k];
            v.x -= w.x; v.y -= w.y; v.z -= w.z; v.w -= w.w;
        }
        o.x += c * v.x; o.y += c * v.y; o.z += c * v.z; o.w += c * v.w;
        reinterpret_cast<float4 *>(out)[k] = o;
    }
    for (long i = 4 * n4 + tid; i < npix; i += stride) out[i] += c * (b ? a[i] - b[i] : a[i]);
}
}  // namespace

// blocks per plane of the two plane kernels: a thread takes NN_PL_TRIPS groups of four (npix % 4 == 0: every plane of an aligned
// vector runs the 16-byte path) or floats, up to the cap
unsigned nn_planes_split(long npix) {
    const long items = npix % 4 == 0 ? npix / 4 : npix, per = (long)RED_TPB * NN_PL_TRIPS;
    return (unsigned)std::max<long>(1, std::min<long>((items + per - 1) / per, NN_PL_MAX_SPLIT));
}
size_t nn_planes_part_doubles(int L, long npix) { return (size_t)4 * L * nn_planes_split(npix); }
// sums [4][L] (device) = per plane |x - z'|^2, |z' - z|^2, #{z' == 0}, r.r of the updated r; part: nn_planes_part_doubles(L, npix)
int launch_nn_project_planes(hipStream_t s, const float *x, float *z, float *u, float *r, int L, long npix, const float *rho_l, double *part,
                             double *sums) {
    if (L < 1 || npix < 1 || L > 65535) return (int)hipErrorInvalidValue;
    const unsigned S = nn_planes_split(npix);
    hipLaunchKernelGGL(nn_project_planes_kernel, dim3(S, (unsigned)L), dim3(RED_TPB), 0, s, x, z, u, r, npix, rho_l, part);
    if (const int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(nn_planes_reduce_kernel, dim3((unsigned)((4 * L + RED_TPB - 1) / RED_TPB)), dim3(RED_TPB), 0, s, part, (int)S, 4 * L, sums);
    return (int)hipGetLastError();
}
int launch_nn_add_planes(hipStream_t s, float *out, const float *a, const float *b, int L, long npix, const float *c_l, float scale) {
    if (L < 1 || npix < 1 || L > 65535) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_add_planes_kernel, dim3(nn_planes_split(npix), (unsigned)L), dim3(RED_TPB), 0, s, out, a, b, npix, c_l, scale);
    return (int)hipGetLastError();
}

static_assert(RED_TPB == VEC_TPB, "kernels.h states the block size of the capped grids");
// a thread takes one group of four (`vec`) or one float per trip; the n % 4 floats behind the groups go one to a thread
unsigned nn_project_grid(long n, int vec) {
    const long items = vec ? n / 4 + n % 4 : n;
    return (unsigned)std::max<long>(1, std::min<long>((items + RED_TPB - 1) / RED_TPB, NN_MAX_BLOCKS));
}

// sums[0..3] (device) = |x - z'|^2, |z' - z|^2, #{z' == 0}, r.r of the updated r (0 without r); scratch: 1024 doubles.  r and dv
// are alternatives (r wins); with neither only z and u move
int launch_nn_project(hipStream_t s, const float *x, float *z, float *u, float *r, float *dv, long n, float rho, double *scratch,
                      double *sums) {
    if (n < 0) return (int)hipErrorInvalidValue;
    float *const w = r ? r : dv;
    const int vec = aligned16(x) && aligned16(z) && aligned16(u) && aligned16(w);
    const unsigned grid = nn_project_grid(n, vec);
    if (r) hipLaunchKernelGGL(nn_project_kernel<NN_FUSED>, dim3(grid), dim3(RED_TPB), 0, s, x, z, u, w, n, rho, vec, scratch);
    else if (dv) hipLaunchKernelGGL(nn_project_kernel<NN_DV>, dim3(grid), dim3(RED_TPB), 0, s, x, z, u, w, n, rho, vec, scratch);
    else hipLaunchKernelGGL(nn_project_kernel<NN_PLAIN>, dim3(grid), dim3(RED_TPB), 0, s, x, z, u, w, n, rho, vec, scratch);
    if (const int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(4), dim3(RED_TPB), 0, s, scratch, (int)grid, sums);
    return (int)hipGetLastError();
}
int launch_nn_add(hipStream_t s, float *out, const float *a, const float *b, long n, float c) {
    if (n <= 0) return 0;
    const unsigned grid = (unsigned)std::max<long>(1, std::min<long>((n + RED_TPB - 1) / RED_TPB, 2048));
    hipLaunchKernelGGL(nn_add_kernel, dim3(grid), dim3(RED_TPB), 0, s, out, a, b, n, c);
    return (int)hipGetLastError();
}

extern "C" {

int surfh_nn_project_dev(surfh_plan *p, const float *x_dev, float *z_dev, float *u_dev, float *r_dev, float *dv_dev, int64_t n, double rho,
                         double *sums) {
    if (!p || !x_dev || !z_dev || !u_dev || !sums) return fail("null argument");
    if (n < 0) return fail("surfh_nn_project_dev: n = %ld", (long)n);
    if (!(rho > 0.0 && rho <= DBL_MAX)) return fail("surfh_nn_project_dev: rho = %g must be finite and > 0", rho);
    HIP_OK(hipSetDevice(p->dev));
    {
        Prof pr(p, "nn_project");
        LAUNCH_OK(launch_nn_project(p->stream, x_dev, z_dev, u_dev, r_dev, dv_dev, n, (float)rho, p->dscratch, p->dscal + 8));
    }
    HIP_OK(hipMemcpyAsync(sums, p->dscal + 8, 4 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

int surfh_nn_project_planes_dev(surfh_plan *p, const float *x_dev, float *z_dev, float *u_dev, float *r_dev, int32_t L, int64_t npix,
                                const double *rho, double *sums) {
    if (!p || !x_dev || !z_dev || !u_dev || !r_dev || !rho || !sums) return fail("null argument");
    if (L < 1 || L > 65535 || npix < 1) return fail("surfh_nn_project_planes_dev: L = %d, npix = %ld", L, (long)npix);
    std::vector<float> h((size_t)L);
    for (int l = 0; l < L; ++l) {
        h[l] = (float)rho[l];
        if (!(rho[l] > 0.0 && rho[l] <= DBL_MAX) || !(h[l] > 0.f && h[l] <= FLT_MAX))
            return fail("surfh_nn_project_planes_dev: rho[%d] = %g must be finite and > 0 (as a float too)", l, rho[l]);
    }
    HIP_OK(hipSetDevice(p->dev));
    const size_t parts = nn_planes_part_doubles(L, npix);
    DevBuf<float> rho_dev;                 // this call's own: freed on every return
    DevBuf<double> part;
    if (rho_dev.upload(h) || part.alloc(parts + (size_t)4 * L)) return 1;
    {
        Prof pr(p, "nn_project");
        LAUNCH_OK(launch_nn_project_planes(p->stream, x_dev, z_dev, u_dev, r_dev, L, npix, rho_dev, part, part + parts));
    }
    HIP_OK(hipMemcpyAsync(sums, part + parts, (size_t)4 * L * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_OK(hipStreamSynchronize(p->stream));
    return 0;
}

}  // extern "C"
