// Robust (Huber) data term of the 3MG solvers (surfh_mmmg_robust, surfh_mmmg_robust_vox): the three detector-space passes of an
// iteration, on flat vectors of any length n.  With t_i = sqrt(w_i) (y_i - u_i), u = A x:
//   data  : v = sqrt(w) phi'(t) (A^T v is the data part of -g), sum phi(t), number of |t| > delta, optionally omega(t) = phi'(t) / t
//   curv  : sum w omega p0^2, sum w omega p0 p1, sum w omega p1^2 (the data block of the half-quadratic majorant, p = A g, A m)
//   move  : mv = c0 g + c1 m;  u += mv;  m = mv   (one pass for the detector vectors and one for the maps)
// A sample of weight 0 is taken out by a select: it contributes nothing whatever y holds there, NaN and Inf included (v = 0,
// omega = 0).  w == nullptr: every weight is 1.
// Mapping: streaming, one pass over every operand.  A thread owns V consecutive floats per grid-stride step, V = 4 / 2 / 1 =
// the widest access every operand's address allows (16 / 8 / 4 bytes), so a wavefront reads 1 KiB contiguous per operand and
// step with V = 4; the n % V last elements go to the first threads of the grid, one each.  At most ROB_BLOCKS blocks of 256.
// Reductions: float64 per thread, per block in a fixed order into `scratch` [K][blocks], then one block per sum -- the same
// inputs give the same bits (reduce_dev.h).
#include <cstdint>
#include <initializer_list>

#include "huber_dev.h"
#include "kernels.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = RED_TPB;
constexpr int ROB_BLOCKS = 2048;      // 8 blocks per CU; [3][2048] partials = launch_robust_scratch_doubles()

template <int V>
struct Vec;
template <>
struct Vec<4> {
    typedef float4 type;
};
template <>
struct Vec<2> {
    typedef float2 type;
};
template <>
struct Vec<1> {
    typedef float type;
};

template <int V>
__device__ __forceinline__ void load(float (&r)[V], const float *p, long iv) {
    const typename Vec<V>::type q = reinterpret_cast<const typename Vec<V>::type *>(p)[iv];
    const float *f = reinterpret_cast<const float *>(&q);
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = f[k];
}
template <int V>
__device__ __forceinline__ void store(const float (&r)[V], float *p, long iv) {
    typename Vec<V>::type q;
    float *f = reinterpret_cast<float *>(&q);
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = r[k];
    reinterpret_cast<typename Vec<V>::type *>(p)[iv] = q;
}
template <int V>
__device__ __forceinline__ void fill(float (&r)[V], float a) {
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = a;
}

// the scaled residual t of one sample, 0 where the sample is masked (keep = false)
__device__ __forceinline__ float scaled_residual(float y, float u, float w, float &sw, bool &keep) {
    keep = w > 0.f;
    sw = keep ? sqrtf(w) : 0.f;
    return keep ? sw * (y - u) : 0.f;
}

template <int KIND>
__device__ __forceinline__ void data_one(float y, float u, float w, float delta, float &v, float &om, double (&acc)[2]) {
    float sw;
    bool keep;
    const float t = scaled_residual(y, u, w, sw, keep);
    v = sw * pot_dphi<KIND>(t, delta);
    om = keep ? pot_w<KIND>(t, delta) : 0.f;
    acc[0] += pot_phi<KIND>(t, delta);
    acc[1] += fabsf(t) > delta ? 1.0 : 0.0;
}

template <int KIND>
__device__ __forceinline__ void curv_one(float y, float u, float w, float a, float b, float delta, double (&acc)[3]) {
    float sw;
    bool keep;
    const float t = scaled_residual(y, u, w, sw, keep);
    const double ww = keep ? (double)w * (double)pot_w<KIND>(t, delta) : 0.0, da = a, db = b;
    acc[0] += ww * da * da;
    acc[1] += ww * da * db;
    acc[2] += ww * db * db;
}

// part [2][blocks]: sum phi(t), number of |t| > delta (the samples past the knee, whatever the potential).  om may be null.
// KIND: the potential of the data term (huber_dev.h).
template <int V, int KIND>
__global__ __launch_bounds__(TPB) void robust_data_kernel(const float *__restrict__ y, const float *__restrict__ u,
                                                          const float *__restrict__ w, float *__restrict__ v, float *__restrict__ om,
                                                          long n, float delta, double *__restrict__ part) {
    double acc[2] = {0.0, 0.0};
    const long nv = n / V, gid = (long)blockIdx.x * TPB + threadIdx.x, stride = (long)gridDim.x * TPB;
    for (long i = gid; i < nv; i += stride) {
        float ry[V], ru[V], rw[V], rv[V], ro[V];
        load<V>(ry, y, i);
        load<V>(ru, u, i);
        if (w) load<V>(rw, w, i);
        else fill<V>(rw, 1.f);
#pragma unroll
        for (int k = 0; k < V; ++k) data_one<KIND>(ry[k], ru[k], rw[k], delta, rv[k], ro[k], acc);
        store<V>(rv, v, i);
        if (om) store<V>(ro, om, i);
    }
    const long e = nv * V + gid;                         // the tail: fewer than V elements
    if (V > 1 && e < n) {
        float tv, to;
        data_one<KIND>(y[e], u[e], w ? w[e] : 1.f, delta, tv, to, acc);
        v[e] = tv;
        if (om) om[e] = to;
    }
    block_sums_to<2>(acc, part);
}

// part [3][blocks]: sum w omega p0^2, sum w omega p0 p1, sum w omega p1^2
template <int V, int KIND>
__global__ __launch_bounds__(TPB) void robust_curv_kernel(const float *__restrict__ y, const float *__restrict__ u,
                                                          const float *__restrict__ w, const float *__restrict__ p0,
                                                          const float *__restrict__ p1, long n, float delta,
                                                          double *__restrict__ part) {
    double acc[3] = {0.0, 0.0, 0.0};
    const long nv = n / V, gid = (long)blockIdx.x * TPB + threadIdx.x, stride = (long)gridDim.x * TPB;
    for (long i = gid; i < nv; i += stride) {
        float ry[V], ru[V], rw[V], ra[V], rb[V];
        load<V>(ry, y, i);
        load<V>(ru, u, i);
        if (w) load<V>(rw, w, i);
        else fill<V>(rw, 1.f);
        load<V>(ra, p0, i);
        load<V>(rb, p1, i);
#pragma unroll
        for (int k = 0; k < V; ++k) curv_one<KIND>(ry[k], ru[k], rw[k], ra[k], rb[k], delta, acc);
    }
    const long e = nv * V + gid;
    if (V > 1 && e < n) curv_one<KIND>(y[e], u[e], w ? w[e] : 1.f, p0[e], p1[e], delta, acc);
    block_sums_to<3>(acc, part);
}

// mv = c0 g + c1 m;  u += mv;  m = mv
template <int V>
__global__ __launch_bounds__(TPB) void robust_move_kernel(float *__restrict__ u, const float *__restrict__ g, float *__restrict__ m,
                                                          long n, float c0, float c1) {
    const long nv = n / V, gid = (long)blockIdx.x * TPB + threadIdx.x, stride = (long)gridDim.x * TPB;
    for (long i = gid; i < nv; i += stride) {
        float ru[V], rg[V], rm[V];
        load<V>(ru, u, i);
        load<V>(rg, g, i);
        load<V>(rm, m, i);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            rm[k] = c0 * rg[k] + c1 * rm[k];
            ru[k] += rm[k];
        }
        store<V>(ru, u, i);
        store<V>(rm, m, i);
    }
    const long e = nv * V + gid;
    if (V > 1 && e < n) {
        const float mv = c0 * g[e] + c1 * m[e];
        u[e] += mv;
        m[e] = mv;
    }
}

// the widest access (in floats) that every operand's address allows; null operands do not count
inline int vec_width(std::initializer_list<const void *> ptrs) {
    uintptr_t bits = 0;
    for (const void *q : ptrs) bits |= (uintptr_t)q;
    return (bits & 15) == 0 ? 4 : (bits & 7) == 0 ? 2 : 1;
}
}  // namespace

static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");
unsigned rob_grid(long n, int V) {
    const long want = (n / V + TPB - 1) / TPB;
    return (unsigned)(want > ROB_BLOCKS ? ROB_BLOCKS : want < 1 ? 1 : want);
}

#define ROB_DISPATCH(V, kernel, grid, ...)                                                                   \
    switch (V) {                                                                                             \
    case 4: hipLaunchKernelGGL(kernel<4>, dim3(grid), dim3(TPB), 0, s, __VA_ARGS__); break;                  \
    case 2: hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(TPB), 0, s, __VA_ARGS__); break;                  \
    default: hipLaunchKernelGGL(kernel<1>, dim3(grid), dim3(TPB), 0, s, __VA_ARGS__); break;                 \
    }

// the same for a kernel<V, KIND>; evaluates to false on an unknown kind
#define ROB_POT_DISPATCH(V, kind, kernel, grid, ...)                                                         \
    pot_dispatch(kind, [&](auto K) {                                                                         \
        constexpr int KIND = decltype(K)::value;                                                             \
        switch (V) {                                                                                         \
        case 4: hipLaunchKernelGGL((kernel<4, KIND>), dim3(grid), dim3(TPB), 0, s, __VA_ARGS__); break;      \
        case 2: hipLaunchKernelGGL((kernel<2, KIND>), dim3(grid), dim3(TPB), 0, s, __VA_ARGS__); break;      \
        default: hipLaunchKernelGGL((kernel<1, KIND>), dim3(grid), dim3(TPB), 0, s, __VA_ARGS__); break;     \
        }                                                                                                    \
    })

size_t launch_robust_scratch_doubles() { return (size_t)3 * ROB_BLOCKS; }

int launch_robust_data(hipStream_t s, const float *y, const float *u, const float *w, float *v, float *omega, long n, float delta,
                       int kind, double *scratch, double *sums) {
    if (n < 1 || !(delta > 0.f)) return (int)hipErrorInvalidValue;
    const int V = vec_width({y, u, w, v, omega});
    const unsigned g = rob_grid(n, V);
    if (!ROB_POT_DISPATCH(V, kind, robust_data_kernel, g, y, u, w, v, omega, n, delta, scratch)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(2), dim3(TPB), 0, s, scratch, (int)g, sums);
    return (int)hipGetLastError();
}

int launch_robust_curv(hipStream_t s, const float *y, const float *u, const float *w, const float *p0, const float *p1, long n,
                       float delta, int kind, double *scratch, double *sums) {
    if (n < 1 || !(delta > 0.f)) return (int)hipErrorInvalidValue;
    const int V = vec_width({y, u, w, p0, p1});
    const unsigned g = rob_grid(n, V);
    if (!ROB_POT_DISPATCH(V, kind, robust_curv_kernel, g, y, u, w, p0, p1, n, delta, scratch)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(3), dim3(TPB), 0, s, scratch, (int)g, sums);
    return (int)hipGetLastError();
}

int launch_robust_move(hipStream_t s, float *u, const float *g, float *m, long n, double c0, double c1) {
    if (n < 1) return (int)hipErrorInvalidValue;
    const int V = vec_width({u, g, m});
    ROB_DISPATCH(V, robust_move_kernel, rob_grid(n, V), u, g, m, n, (float)c0, (float)c1);
    return (int)hipGetLastError();
}
