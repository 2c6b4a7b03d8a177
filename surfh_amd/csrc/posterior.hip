// Posterior sampling by perturbation-optimisation (Orieux, Feron, Giovannelli 2012), the device kernels and their launchers.
// The posterior of the quadratic criterion is  p(x | y) ~ exp(-x^T Q x / 2 + b^T x),  Q = mu A^T W A + mu_reg (Dr^T Dr + Dc^T Dc),
// b = mu A^T W y.  A draw b~ ~ N(b, Q) solved through Q x~ = b~ is a draw x~ ~ N(Q^-1 b, Q^-1):
//   y~  = y + eps_y / sqrt(mu w)              po_data     (b~ data part = mu A^T W y~, covariance mu A^T W A)
//   eta = sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c)   po_prior    (covariance mu_reg (Dr^T Dr + Dc^T Dc)), added to the right-hand side
// with eps_* standard normal (randn below, or the caller's).  The sampler solves for the deviation e = x~ - Q^-1 b, whose
// right-hand side b~ - b is the same chain on the perturbation alone (po_data without y).  po_moments accumulates the first and
// second moments of the deviations in float64 per pixel.  The loop around them: surfh_cg_sample, plan_solvers.hip.
#include "plan_internal.h"

namespace {
constexpr int TPB = 256;

// ---- randn: Philox4x32-10 (Salmon et al. 2011) + Box-Muller, counter-based ------------------------------------------------------
// key = (seed low, seed high), counter = (c low, c high, stream, sample), c = element index / 4: the value of element i depends
// on (seed, stream, sample, i) alone.  Words (a0, a1) give elements 4c, 4c+1 and (a2, a3) give 4c+2, 4c+3.
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = {hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
// z0 = sqrt(-2 ln u) cos(theta), z1 = ... sin(theta); u = (m0 + 1/2) 2^-24, theta = 2 pi (m1 + 1/2) 2^-24, m = word >> 8.
// Both arguments reach the library functions exactly: u >= 1/2 goes through log1p(-(1 - u)) with 1 - u = (2^24 - m0 - 1/2) 2^-24
// (24 significant bits, like u below 1/2), the angle through sincospi of the odd integer 2 m1 + 1 reduced by 2^24 (half a turn:
// both signs flip).  |z| <= sqrt(50 ln 2) = 5.887.
__device__ __forceinline__ void box_muller(uint32_t a0, uint32_t a1, float &z0, float &z1) {
    const uint32_t m0 = a0 >> 8;
    const float neg_ln = m0 < (1u << 23) ? -logf(((float)m0 + 0.5f) * 0x1p-24f) : -log1pf(-(((float)((1u << 24) - m0) - 0.5f) * 0x1p-24f));
    const float rad = sqrtf(2.f * neg_ln);
    const uint32_t k = 2u * (a1 >> 8) + 1u;                          // theta / pi = k 2^-24, k odd below 2^25
    const bool flip = k >= (1u << 24);
    float sn, cs;
    sincospif((float)(flip ? k - (1u << 24) : k) * 0x1p-24f, &sn, &cs);
    z0 = flip ? -rad * cs : rad * cs;
    z1 = flip ? -rad * sn : rad * sn;
}
// ---- the per-element pieces the unfused kernels (randn, po_data, po_prior) and the fused plane-wise ones share: one definition each
// the four normals of counter c -- elements 4c .. 4c+3 of the stream (key, stream, sample)
struct Key { uint32_t k0, k1, sample; };
__device__ __forceinline__ float4 randn4(long c, Key key, uint32_t stream) {
    const U4 a = philox4x32_10({(uint32_t)c, (uint32_t)((unsigned long)c >> 32), stream, key.sample}, key.k0, key.k1);
    float4 z;
    box_muller(a.x, a.y, z.x, z.y);
    box_muller(a.z, a.w, z.z, z.w);
    return z;
}
__device__ __forceinline__ float pick4(const float4 &z, int k) { return k == 0 ? z.x : k == 1 ? z.y : k == 2 ? z.z : z.w; }
// a group of four floats to out + 4c: one 16-byte store where `vec` (out 16-byte aligned) and the group is whole, else float by float up to n
__device__ __forceinline__ void store4(float *__restrict__ out, long c, long n, const float4 &z, int vec) {
    if (vec && 4 * c + 4 <= n) {
        *reinterpret_cast<float4 *>(out + 4 * c) = z;
    } else {
        for (int j = 0; j < 4; ++j)
            if (4 * c + j < n) out[4 * c + j] = pick4(z, j);
    }
}
// the bits of y + eps / sqrt(mu w) where w > 0, those of y elsewhere
__device__ __forceinline__ uint32_t po_data_value(uint32_t v, float wi, float eps, float mu) {
    return wi > 0.f ? __float_as_uint(__uint_as_float(v) + eps / sqrtf(mu * wi)) : v;
}
// one element of s (Dr^T eps_r + Dc^T eps_c): eps_r below (row i+1) and here, eps_c to the right (column j+1) and here
__device__ __forceinline__ float po_prior_value(float s, float er_ip, float er_o, float ec_jp, float ec_o) {
    return s * ((er_ip - er_o) + (ec_jp - ec_o));
}

// one thread per counter; `vec`: out is 16-byte aligned, whole groups of four go out as one store
__global__ __launch_bounds__(TPB) void randn_kernel(float *__restrict__ out, long n, Key key, uint32_t stream, int vec) {
    const long c = (long)blockIdx.x * TPB + threadIdx.x;
    if (4 * c >= n) return;
    store4(out, c, n, randn4(c, key, stream), vec);
}

// y~ = y + eps / sqrt(mu w) where w > 0 (w NULL: 1); a sample of weight 0 keeps its bits, whatever they are.  y NULL: the
// perturbation alone, eps / sqrt(mu w), and 0 at weight 0
__global__ __launch_bounds__(TPB) void po_data_kernel(const uint32_t *__restrict__ y, const float *__restrict__ w, const float *__restrict__ eps,
                                                      uint32_t *__restrict__ out, long n, float mu) {
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        out[i] = po_data_value(y ? y[i] : 0u, w ? w[i] : 1.f, eps[i], mu);
    }
}

// eta = s (Dr^T eps_r + Dc^T eps_c) on [T][na][nb], circular: (Dr^T e)[i][j] = e[i+1][j] - e[i][j], (Dc^T e)[i][j] = e[i][j+1] - e[i][j]
__global__ __launch_bounds__(TPB) void po_prior_kernel(const float *__restrict__ er, const float *__restrict__ ec, float *__restrict__ out, int na,
                                                       int nb, float s) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= nb) return;
    const long base = (long)blockIdx.z * na * nb;
    const int ip = (i == na - 1) ? 0 : i + 1, jp = (j == nb - 1) ? 0 : j + 1;
    const long o = base + (long)i * nb + j;
    out[o] = po_prior_value(s, er[base + (long)ip * nb + j], er[o], ec[base + (long)i * nb + jp], ec[o]);
}

__global__ __launch_bounds__(TPB) void po_add_kernel(float *__restrict__ b, const float *__restrict__ e, long n) {
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) b[i] += e[i];
}

// ---- the plane-wise sampler's perturbations (surfh_cg_planes_sample): the noise is generated in registers, never stored ---------
// Capped grid, grid-stride loop over the counters: a thread makes the four elements 4c .. 4c+3 of its counter and stores them as one
// 16-byte group (store4).
//
// The normals of one stream a thread has at hand: the group of its own counter and the last other group it asked for.  Element i
// comes from counter i / 4 whatever the thread, so a neighbour's value is recomputed from its own counter -- the bits randn_kernel
// would have stored there.
struct Near {
    float4 own, other;
    long c_own, c_other;
};
__device__ __forceinline__ float normal_at(long i, Near &g, Key key, uint32_t stream) {
    const long c = i >> 2;
    if (c == g.c_own) return pick4(g.own, (int)(i & 3));
    if (c != g.c_other) {
        g.c_other = c;
        g.other = randn4(c, key, stream);
    }
    return pick4(g.other, (int)(i & 3));
}
// eta = s (Dr^T eps_r + Dc^T eps_c) on [L][na][nb], eps_r = stream 1 and eps_c = stream 2 over the flat index of [L][na][nb]: what
// randn_kernel twice and po_prior_kernel on T = L maps write, bit for bit, with neither noise array in memory.  Row i+1 and column
// j+1 wrap inside the plane.  With nb a multiple of 4 the row below is one counter (4 of them per group: eps_r and eps_c here, eps_r
// below, eps_c of the next group for the last column); other widths and the wraps cost a counter more.
__global__ __launch_bounds__(TPB) void po_planes_eta_kernel(float *__restrict__ out, long n, int na, int nb, float s, Key key, int vec) {
    const long stride = (long)gridDim.x * TPB, npix = (long)na * nb;
    for (long c = (long)blockIdx.x * TPB + threadIdx.x; 4 * c < n; c += stride) {
        Near er = {randn4(c, key, 1), {}, c, -1}, ec = {randn4(c, key, 2), {}, c, -1};
        long o = 4 * c;
        const long p = o % npix;
        int i = (int)(p / nb), j = (int)(p % nb);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k, ++o) {
            if (o >= n) break;
            const long ip = (i == na - 1) ? o - (long)i * nb : o + nb;          // row 0 of the same plane
            const long jp = (j == nb - 1) ? o - j : o + 1;                      // column 0 of the same row
            v[k] = po_prior_value(s, normal_at(ip, er, key, 1), pick4(er.own, k), normal_at(jp, ec, key, 2), pick4(ec.own, k));
            if (++j == nb) {
                j = 0;
                if (++i == na) i = 0;
            }
        }
        store4(out, c, n, make_float4(v[0], v[1], v[2], v[3]), vec);
    }
}
// out = eps_y / sqrt(mu w), 0 where w = 0 (w NULL: 1), eps_y = stream 0: randn_kernel and po_data_kernel(y NULL), bit for bit.
// `vec`: out and w are 16-byte aligned
__global__ __launch_bounds__(TPB) void po_planes_data_kernel(const float *__restrict__ w, float *__restrict__ out, long n, float mu, Key key, int vec) {
    const long stride = (long)gridDim.x * TPB;
    for (long c = (long)blockIdx.x * TPB + threadIdx.x; 4 * c < n; c += stride) {
        const float4 z = randn4(c, key, 0);
        float4 wi = make_float4(1.f, 1.f, 1.f, 1.f);
        if (w && vec && 4 * c + 4 <= n) {
            wi = *reinterpret_cast<const float4 *>(w + 4 * c);
        } else if (w) {
            wi.x = w[4 * c];
            if (4 * c + 1 < n) wi.y = w[4 * c + 1];
            if (4 * c + 2 < n) wi.z = w[4 * c + 2];
            if (4 * c + 3 < n) wi.w = w[4 * c + 3];
        }
        store4(out, c, n,
               make_float4(__uint_as_float(po_data_value(0u, wi.x, z.x, mu)), __uint_as_float(po_data_value(0u, wi.y, z.y, mu)),
                           __uint_as_float(po_data_value(0u, wi.z, z.z, mu)), __uint_as_float(po_data_value(0u, wi.w, z.w, mu))),
               vec);
    }
}
// The planes are independent: the only second moment is the variance.  S1 += e, S2 += e e per element in float64, e = x - xhat (xhat
// NULL: x); every element has one owner and one order of additions, so the same inputs give the same bits.  `vec`: n % 2 == 0 and all
// bases 16-byte aligned -- two elements per thread and trip, the sums as 16-byte accesses
__global__ __launch_bounds__(TPB) void po_planes_moments_kernel(const float *__restrict__ x, const float *__restrict__ xhat, double *__restrict__ S1,
                                                                double *__restrict__ S2, long n, int vec) {
    const long stride = (long)gridDim.x * TPB, t = (long)blockIdx.x * TPB + threadIdx.x;
    if (vec) {
        for (long i = t; 2 * i < n; i += stride) {
            const float2 xv = reinterpret_cast<const float2 *>(x)[i];
            const float2 hv = xhat ? reinterpret_cast<const float2 *>(xhat)[i] : make_float2(0.f, 0.f);
            const double e0 = xhat ? (double)xv.x - (double)hv.x : (double)xv.x, e1 = xhat ? (double)xv.y - (double)hv.y : (double)xv.y;
            double2 a = reinterpret_cast<double2 *>(S1)[i], b = reinterpret_cast<double2 *>(S2)[i];
            a.x += e0; a.y += e1;
            b.x += e0 * e0; b.y += e1 * e1;
            reinterpret_cast<double2 *>(S1)[i] = a;
            reinterpret_cast<double2 *>(S2)[i] = b;
        }
    } else {
        for (long i = t; i < n; i += stride) {
            const double e = xhat ? (double)x[i] - (double)xhat[i] : (double)x[i];
            S1[i] += e;
            S2[i] += e * e;
        }
    }
}
// in place: S1 <- mean = xhat + S1 / K, S2 <- var = (S2 - S1^2 / K) / (K - 1) clamped at 0 (want_var = 0: S2 is left alone).  S1^2 / K
// is formed as S1 (S1 / K): for a constant sample set S1 / K is the constant exactly and the difference is exactly 0
__global__ __launch_bounds__(TPB) void po_planes_finish_kernel(const float *__restrict__ xhat, double *__restrict__ S1, double *__restrict__ S2, long n,
                                                               int K, int want_var) {
    const long stride = (long)gridDim.x * TPB;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        const double s1 = S1[i], m = s1 / K;
        S1[i] = (double)xhat[i] + m;
        if (want_var) S2[i] = fmax((S2[i] - s1 * m) / (K - 1), 0.0);
    }
}

// ---- moments: S = [T + T (T + 1) / 2][npix] doubles, S1[t] += e_t, S2[(t, u >= t)] += e_t e_u, e = x - xhat (xhat NULL: e = x);
// one thread per pixel
__host__ __device__ constexpr int pair_index(int T, int t, int u) { return T + t * T - t * (t - 1) / 2 + (u - t); }
template <int T>
__global__ __launch_bounds__(TPB) void po_moments_kernel(const float *__restrict__ x, const float *__restrict__ xhat, double *__restrict__ S, long npix) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    double e[T];
#pragma unroll
    for (int t = 0; t < T; ++t) e[t] = xhat ? (double)x[t * npix + i] - (double)xhat[t * npix + i] : (double)x[t * npix + i];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        S[t * npix + i] += e[t];
#pragma unroll
        for (int u = t; u < T; ++u) S[pair_index(T, t, u) * npix + i] += e[t] * e[u];
    }
}
// mean = xhat + S1 / K; cov[(t, u >= t)] = (S2 - S1_t S1_u / K) / (K - 1)   (cov NULL: the mean only)
template <int T>
__global__ __launch_bounds__(TPB) void po_finish_kernel(const float *__restrict__ xhat, const double *__restrict__ S, long npix, int K,
                                                        double *__restrict__ mean, double *__restrict__ cov) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    double s1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        s1[t] = S[t * npix + i];
        mean[t * npix + i] = (double)xhat[t * npix + i] + s1[t] / K;
    }
    if (!cov) return;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int u = t; u < T; ++u) {
            const int k = pair_index(T, t, u);
            cov[(k - T) * npix + i] = (S[k * npix + i] - s1[t] * s1[u] / K) / (K - 1);
        }
}

template <int T>
int moments_T(hipStream_t s, int Tn, const float *x, const float *xhat, double *S, long npix) {
    if constexpr (T <= SURFH_MAX_TEMPLATES) {
        if (Tn != T) return moments_T<T + 1>(s, Tn, x, xhat, S, npix);
        hipLaunchKernelGGL(po_moments_kernel<T>, dim3((unsigned)((npix + TPB - 1) / TPB)), dim3(TPB), 0, s, x, xhat, S, npix);
        return (int)hipGetLastError();
    } else {
        return (int)hipErrorInvalidValue;
    }
}
template <int T>
int finish_T(hipStream_t s, int Tn, const float *xhat, const double *S, long npix, int K, double *mean, double *cov) {
    if constexpr (T <= SURFH_MAX_TEMPLATES) {
        if (Tn != T) return finish_T<T + 1>(s, Tn, xhat, S, npix, K, mean, cov);
        hipLaunchKernelGGL(po_finish_kernel<T>, dim3((unsigned)((npix + TPB - 1) / TPB)), dim3(TPB), 0, s, xhat, S, npix, K, mean, cov);
        return (int)hipGetLastError();
    } else {
        return (int)hipErrorInvalidValue;
    }
}
}  // namespace

static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");
unsigned grid_for(long n, long cap) { return (unsigned)std::max<long>(1, std::min<long>((n + TPB - 1) / TPB, cap)); }
static bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }      // NULL counts as aligned

int launch_randn(hipStream_t s, float *out, long n, uint64_t seed, uint32_t stream, uint32_t sample) {
    if (n <= 0) return 0;
    const long nc = (n + 3) / 4;
    hipLaunchKernelGGL(randn_kernel, dim3((unsigned)((nc + TPB - 1) / TPB)), dim3(TPB), 0, s, out, n, Key{(uint32_t)seed, (uint32_t)(seed >> 32), sample},
                       stream, (int)aligned16(out));
    return (int)hipGetLastError();
}
int launch_po_data(hipStream_t s, const float *y, const float *w, const float *eps, float *out, long n, float mu) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(po_data_kernel, dim3(grid_for(n)), dim3(TPB), 0, s, reinterpret_cast<const uint32_t *>(y), w, eps,
                       reinterpret_cast<uint32_t *>(out), n, mu);
    return (int)hipGetLastError();
}
int launch_po_prior(hipStream_t s, const float *er, const float *ec, float *out, int T, int na, int nb, float sqrt_mu_reg) {
    hipLaunchKernelGGL(po_prior_kernel, dim3((nb + TPB - 1) / TPB, na, T), dim3(TPB), 0, s, er, ec, out, na, nb, sqrt_mu_reg);
    return (int)hipGetLastError();
}
int launch_po_add(hipStream_t s, float *b, const float *e, long n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(po_add_kernel, dim3(grid_for(n, 2048)), dim3(TPB), 0, s, b, e, n);
    return (int)hipGetLastError();
}
// the fused plane-wise kernels: a thread covers four elements per trip, so the cap of grid_for is met at 4 cap TPB elements
int launch_po_planes_eta(hipStream_t s, float *out, int L, int na, int nb, float sqrt_mu_reg, uint64_t seed, uint32_t sample) {
    const long n = (long)L * na * nb;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(po_planes_eta_kernel, dim3(grid_for((n + 3) / 4)), dim3(TPB), 0, s, out, n, na, nb, sqrt_mu_reg,
                       Key{(uint32_t)seed, (uint32_t)(seed >> 32), sample}, (int)aligned16(out));
    return (int)hipGetLastError();
}
int launch_po_planes_data(hipStream_t s, const float *w, float *out, long n, float mu, uint64_t seed, uint32_t sample) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(po_planes_data_kernel, dim3(grid_for((n + 3) / 4)), dim3(TPB), 0, s, w, out, n, mu,
                       Key{(uint32_t)seed, (uint32_t)(seed >> 32), sample}, (int)(aligned16(out) && aligned16(w)));
    return (int)hipGetLastError();
}
int launch_po_planes_moments(hipStream_t s, const float *x, const float *xhat, double *S1, double *S2, long n) {
    if (n <= 0) return 0;
    const int vec = n % 2 == 0 && reinterpret_cast<uintptr_t>(x) % 8 == 0 && reinterpret_cast<uintptr_t>(xhat) % 8 == 0 && aligned16(S1) && aligned16(S2);
    hipLaunchKernelGGL(po_planes_moments_kernel, dim3(grid_for(vec ? n / 2 : n)), dim3(TPB), 0, s, x, xhat, S1, S2, n, vec);
    return (int)hipGetLastError();
}
int launch_po_planes_finish(hipStream_t s, const float *xhat, double *S1, double *S2, long n, int K, int want_var) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(po_planes_finish_kernel, dim3(grid_for(n)), dim3(TPB), 0, s, xhat, S1, S2, n, K, want_var);
    return (int)hipGetLastError();
}
long po_moment_planes(int T) { return (long)T + (long)T * (T + 1) / 2; }
int launch_po_moments(hipStream_t s, const float *x, const float *xhat, double *S, int T, long npix) {
    return T < 1 ? (int)hipErrorInvalidValue : moments_T<1>(s, T, x, xhat, S, npix);
}
int launch_po_finish(hipStream_t s, const float *xhat, const double *S, int T, long npix, int K, double *mean, double *cov) {
    return T < 1 ? (int)hipErrorInvalidValue : finish_T<1>(s, T, xhat, S, npix, K, mean, cov);
}

extern "C" {

int surfh_randn_dev(surfh_plan *p, float *out_dev, int64_t n, uint64_t seed, uint32_t stream, uint32_t sample) {
    if (!p || (!out_dev && n > 0)) return fail("null argument");
    if (n < 0) return fail("surfh_randn_dev: n = %ld", (long)n);
    HIP_OK(hipSetDevice(p->dev));
    Prof pr(p, "po_randn");
    LAUNCH_OK(launch_randn(p->stream, out_dev, n, seed, stream, sample));
    return 0;
}
int surfh_po_data_dev(surfh_plan *p, const float *y_dev, const float *w_dev, const float *eps_dev, int64_t n, double mu, float *out_dev) {
    if (!p || !eps_dev || !out_dev) return fail("null argument");          // y_dev NULL: the perturbation alone
    if (n < 0) return fail("surfh_po_data_dev: n = %ld", (long)n);
    if (!(mu > 0.0 && mu <= DBL_MAX)) return fail("posterior sampling: mu = %g must be finite and > 0", mu);
    HIP_OK(hipSetDevice(p->dev));
    Prof pr(p, "po_data");
    LAUNCH_OK(launch_po_data(p->stream, y_dev, w_dev, eps_dev, out_dev, n, (float)mu));
    return 0;
}
int surfh_po_prior_dev(surfh_plan *p, const float *eps_r_dev, const float *eps_c_dev, double mu_reg, float *out_dev) {
    if (!p || !eps_r_dev || !eps_c_dev || !out_dev) return fail("null argument");
    if (p->T <= 0) return fail("prior is defined on abundance maps (needs templates)");
    if (!(mu_reg >= 0.0 && mu_reg <= DBL_MAX)) return fail("posterior sampling: mu_reg = %g must be finite and >= 0", mu_reg);
    HIP_OK(hipSetDevice(p->dev));
    Prof pr(p, "po_prior");
    LAUNCH_OK(launch_po_prior(p->stream, eps_r_dev, eps_c_dev, out_dev, p->T, p->Na, p->Nb, (float)std::sqrt(mu_reg)));
    return 0;
}

// the moments of K explicit samples [K][T][npix] about xhat [T][npix], host buffers: the accumulation and the finishing kernel of
// surfh_cg_sample on their own.  mean [T][npix], cov [T (T + 1) / 2][npix] (pairs t <= u, row-major; NULL: not wanted), float64.
int surfh_po_moments(int32_t T, int64_t npix, const float *xhat, const float *samples, int32_t K, double *mean, double *cov, int32_t device) {
    if (!xhat || !samples || !mean) return fail("null argument");
    if (T < 1 || T > SURFH_MAX_TEMPLATES) return fail("posterior moments: %d maps, the kernels take 1 to %d", T, SURFH_MAX_TEMPLATES);
    if (npix < 1 || K < 1) return fail("posterior moments: npix = %ld, K = %d", (long)npix, K);
    if (cov && K < 2) return fail("posterior moments: a covariance needs at least 2 samples (got %d)", K);
    HIP_OK(hipSetDevice(device));
    const size_t n = (size_t)T * npix, np = (size_t)po_moment_planes(T) * npix;
    DevBuf<float> dx, dh;
    DevBuf<double> S, out;
    if (dx.alloc(n) || dh.alloc(n) || S.alloc(np) || out.alloc(np)) return 1;
    HIP_OK(hipMemcpy(dh, xhat, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(S, 0, np * sizeof(double)));
    for (int k = 0; k < K; ++k) {
        HIP_OK(hipMemcpy(dx, samples + (size_t)k * n, n * sizeof(float), hipMemcpyHostToDevice));
        LAUNCH_OK(launch_po_moments(nullptr, dx, dh, S, T, npix));
    }
    LAUNCH_OK(launch_po_finish(nullptr, dh, S, T, npix, K, out, cov ? out + n : nullptr));
    HIP_OK(hipMemcpy(mean, out, n * sizeof(double), hipMemcpyDeviceToHost));
    if (cov) HIP_OK(hipMemcpy(cov, out + n, (np - n) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
