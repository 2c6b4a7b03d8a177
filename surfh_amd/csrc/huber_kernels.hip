// Huber-family priors of the maps and of the planes: gradient and curvature passes, and the plane-wise 3MG blocks built on them
// (see kernels.h for the contracts).
#include "kernels.h"
#include "huber_dev.h"
#include "mm_step.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == RED_TPB, "the shared reductions of reduce_dev.h assume this block size");
static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");

// ---- Huber priors on the separated circular first differences (surfh_mmmg_huber) ----------------
// One thread per map pixel (grid-stride): the pixel owns u_r = x[i-1][j] - x[i][j] and u_c = x[i][j-1] - x[i][j] and, for the
// gradient, reads the differences it shares with its successors.  Maps are a few MB: the neighbour reads hit L2 (the cube's
// kernels, where that no longer holds, are in huber_vox.hip).  pot_phi / pot_dphi / pot_w<KIND>: huber_dev.h;
// block_sums_to<K>, parts_reduce_kernel: reduce_dev.h.
struct PixelNbrs {   // (t, i, j) of element e of [T][na][nb] and the circular neighbour offsets inside its plane
    long base;
    int c, im, ip, jm, jp;
};
__device__ __forceinline__ PixelNbrs pixel_nbrs(long e, int na, int nb) {
    const long plane = (long)na * nb;
    const long t = e / plane;
    const int rem = (int)(e - t * plane), i = rem / nb, j = rem - i * nb;
    PixelNbrs q;
    q.base = t * plane;
    q.c = rem;
    q.im = (i == 0 ? na - 1 : i - 1) * nb + j;
    q.ip = (i == na - 1 ? 0 : i + 1) * nb + j;
    q.jm = i * nb + (j == 0 ? nb - 1 : j - 1);
    q.jp = i * nb + (j == nb - 1 ? 0 : j + 1);
    return q;
}

// out = src + coef (Dr^T phi'(Dr x) + Dc^T phi'(Dc x)),  (D^T v)[i] = v[i+1] - v[i];  part: [2][gridDim.x] (out.out, sum phi)
// src and out may be the same array (each element is read and written by one thread).  KIND: the potential (huber_dev.h)
template <int KIND>
__global__ __launch_bounds__(TPB) void huber_grad_kernel(const float *__restrict__ x, const float *src, float *out, long n, int na,
                                                         int nb, float coef, float delta, double *__restrict__ part) {
    double acc[2] = {0.0, 0.0};
    const long stride = (long)gridDim.x * TPB;
    for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        const PixelNbrs q = pixel_nbrs(e, na, nb);
        const float *p = x + q.base;
        const float c = p[q.c];
        const float ur = p[q.im] - c, uc = p[q.jm] - c;            // (Dr x)[i][j], (Dc x)[i][j]
        const float urn = c - p[q.ip], ucn = c - p[q.jp];          // (Dr x)[i+1][j], (Dc x)[i][j+1]
        const float pg = (pot_dphi<KIND>(urn, delta) - pot_dphi<KIND>(ur, delta)) + (pot_dphi<KIND>(ucn, delta) - pot_dphi<KIND>(uc, delta));
        const float g = src[e] + coef * pg;
        out[e] = g;
        acc[0] += (double)g * (double)g;
        acc[1] += pot_phi<KIND>(ur, delta) + pot_phi<KIND>(uc, delta);
    }
    block_sums_to<2>(acc, part);
}
}  // namespace

int launch_huber_grad(hipStream_t s, const float *x, const float *src, float *out, int T, int na, int nb, float coef, float delta,
                      int kind, double *scratch, double *sums) {
    if (T < 1 || na < 1 || nb < 1) return (int)hipErrorInvalidValue;
    const long n = (long)T * na * nb;
    const int nbk = nblocks(n, HUBER_BLOCKS);
    const auto go = [&](auto K) {
        hipLaunchKernelGGL(huber_grad_kernel<decltype(K)::value>, dim3(nbk), dim3(TPB), 0, s, x, src, out, n, na, nb, coef, delta, scratch);
    };
    if (!pot_dispatch(kind, go)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(2), dim3(TPB), 0, s, scratch, nbk, sums);
    return (int)hipGetLastError();
}

namespace {
// part: [3][gridDim.x] = sum_k w(D_k x) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2 (weights recomputed, none stored)
template <int KIND>
__global__ __launch_bounds__(TPB) void huber_curv_kernel(const float *__restrict__ x, const float *__restrict__ p0,
                                                         const float *__restrict__ p1, long n, int na, int nb, float delta,
                                                         double *__restrict__ part) {
    double acc[3] = {0.0, 0.0, 0.0};
    const long stride = (long)gridDim.x * TPB;
    for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        const PixelNbrs q = pixel_nbrs(e, na, nb);
        const float *p = x + q.base, *a = p0 + q.base, *b = p1 + q.base;
        const float c = p[q.c], ac = a[q.c], bc = b[q.c];
        const double wr = pot_w<KIND>(p[q.im] - c, delta), wc = pot_w<KIND>(p[q.jm] - c, delta);
        const double ar = a[q.im] - ac, acl = a[q.jm] - ac, br = b[q.im] - bc, bcl = b[q.jm] - bc;
        acc[0] += wr * ar * ar + wc * acl * acl;
        acc[1] += wr * ar * br + wc * acl * bcl;
        acc[2] += wr * br * br + wc * bcl * bcl;
    }
    block_sums_to<3>(acc, part);
}
}  // namespace

int launch_huber_curv(hipStream_t s, const float *x, const float *p0, const float *p1, int T, int na, int nb, float delta,
                      int kind, double *scratch, double *sums) {
    if (T < 1 || na < 1 || nb < 1) return (int)hipErrorInvalidValue;
    const long n = (long)T * na * nb;
    const int nbk = nblocks(n, HUBER_BLOCKS);
    const auto go = [&](auto K) {
        hipLaunchKernelGGL(huber_curv_kernel<decltype(K)::value>, dim3(nbk), dim3(TPB), 0, s, x, p0, p1, n, na, nb, delta, scratch);
    };
    if (!pot_dispatch(kind, go)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(3), dim3(TPB), 0, s, scratch, nbk, sums);
    return (int)hipGetLastError();
}

namespace {
// ---- 3MG with Huber priors on a batch of independent planes (surfh_mmmg_huber_planes): the scheme of surfh_mmmg_huber with
// every plane's beta, 2x2 system and step formed on the device, one workgroup per plane as in mmmg_dir_planes_kernel /
// mmmg_step_planes_kernel.  Per-plane scalars sc[k * L + l] (L = gridDim.x), k = HP_*.  A thread walks its plane row-major
// with stride TPB, (i, j) carried along (no division per pixel); the neighbour rows come from L1 / L2.  Float64 sums in a fixed
// order (block_sum_bcast, reduce_dev.h): the same inputs give the same bits; nothing outside the plane is read.
enum { HP_GG = 0, HP_PHI, HP_BETA, HP_MBM, HP_C00, HP_C01, HP_C11 };
static_assert(HP_C11 + 1 == HUBER_PLANES_SCALARS, "kernels.h sizes the callers' scratch");

struct PlaneWalk {   // element e = i * nb + j of a [na][nb] plane, e = threadIdx.x, threadIdx.x + TPB, ...
    int e, i, j, si, sj;
    __device__ PlaneWalk(int nb) : e(threadIdx.x), i(threadIdx.x / nb), j(threadIdx.x - i * nb), si(TPB / nb), sj(TPB - si * nb) {}
    __device__ void next(int nb) {
        e += TPB;
        i += si;
        j += sj;
        if (j >= nb) {
            j -= nb;
            ++i;
        }
    }
};

// PHASES & 1, the gradient pass: g = src + coef sum_k D_k^T phi'(D_k x) (huber_grad_kernel's arithmetic; src may be g),
//   sc[HP_GG] = |g|^2, sc[HP_PHI] = sum_k sum phi(D_k x).
// PHASES & 2, the curvature pass on (g, m): sc[HP_C00 .. HP_C11] = sum_k sum w(D_k x) (D_k g)^2, (D_k g)(D_k m), (D_k m)^2
//   (huber_curv_kernel's arithmetic, weights recomputed).
// PHASES == 3, the solver's launch (src = r, coef = -mu_reg, g = -gradient): also g.Q_D m and m.Q_D m from the carried image
//   qm, beta = -(g.Bm) / (m.Bm) with B = Q_D + reg W, d = g + beta m; sc[HP_BETA] = the fp32 beta that formed d, sc[HP_MBM] = m.Bm.
// coef, delta and reg are the plane's own: par[k * L + l], k = HPP_* (coef and delta hold fp32 values).
// COUPLING 1, the isotropic prior sum phi(m), m^2 = u_r^2 + u_c^2 per pixel (coupled_prior.hip's conventions: m^2 in float64, m
//   rounded to fp32 once, w = pot_w(m) in fp32, phi in float64, phi' formed as u w): the gradient of pixel (i, j) takes the weights
//   of the groups (i, j), (i+1, j) and (i, j+1), recomputed here from a 7-point stencil (a stored field would be one more array of
//   the planes' size through HBM in every pass: 2 GB on 2048 x 512 x 512); both differences of a pixel take w(m) in the curvature
//   pass.  COUPLING 0 is the separated prior, as it always was.
enum { HPP_COEF = 0, HPP_DELTA, HPP_REG };
static_assert(HPP_REG + 1 == HUBER_PLANES_PARAMS, "kernels.h sizes the callers' parameter arrays");

__device__ __forceinline__ float group_magnitude(float ur, float uc) {
    return (float)sqrt((double)ur * (double)ur + (double)uc * (double)uc);
}

template <int PHASES, int KIND, int COUPLING>
__global__ __launch_bounds__(TPB) void huber_dir_planes_kernel(const float *__restrict__ x, const float *src, float *g,
                                                               const float *__restrict__ m, const float *__restrict__ qm,
                                                               float *__restrict__ d, int na, int nb, const double *__restrict__ par,
                                                               double *__restrict__ sc) {
    const int l = blockIdx.x, L = gridDim.x, npix = na * nb;
    const long off = (long)l * npix;
    const float *px = x + off;
    const float coef = (float)par[HPP_COEF * L + l], delta = (float)par[HPP_DELTA * L + l];
    const double reg = par[HPP_REG * L + l];
    if constexpr ((PHASES & 1) != 0) {
        double v[2] = {0.0, 0.0};
        for (PlaneWalk q(nb); q.e < npix; q.next(nb)) {
            const int im = q.e - nb + (q.i == 0 ? npix : 0), ip = q.e + nb - (q.i == na - 1 ? npix : 0);
            const int jm = q.e - 1 + (q.j == 0 ? nb : 0), jp = q.e + 1 - (q.j == nb - 1 ? nb : 0);
            const float c = px[q.e];
            const float ur = px[im] - c, uc = px[jm] - c;              // (Dr x)[i][j], (Dc x)[i][j]
            const float urn = c - px[ip], ucn = c - px[jp];            // (Dr x)[i+1][j], (Dc x)[i][j+1]
            float pg, m0 = 0.f;
            if constexpr (COUPLING == 0) {
                pg = (pot_dphi<KIND>(urn, delta) - pot_dphi<KIND>(ur, delta)) + (pot_dphi<KIND>(ucn, delta) - pot_dphi<KIND>(uc, delta));
            } else {
                // the groups of (i, j), (i+1, j) and (i, j+1): the column difference of the row below, the row difference of the
                // column to the right (jm - e and jp - e are the same offsets in every row)
                m0 = group_magnitude(ur, uc);
                const float m1 = group_magnitude(urn, px[ip + (jm - q.e)] - px[ip]);
                const float m2 = group_magnitude(px[im + (jp - q.e)] - px[jp], ucn);
                const float w0 = pot_w<KIND>(m0, delta);
                pg = (pot_w<KIND>(m1, delta) * urn - w0 * ur) + (pot_w<KIND>(m2, delta) * ucn - w0 * uc);
            }
            const float gv = src[off + q.e] + coef * pg;
            g[off + q.e] = gv;
            v[0] += (double)gv * (double)gv;
            if constexpr (COUPLING == 0) v[1] += pot_phi<KIND>(ur, delta) + pot_phi<KIND>(uc, delta);
            else v[1] += pot_phi<KIND>(m0, delta);
        }
        block_sum_bcast<2>(v);
        if (threadIdx.x == 0) {
            sc[HP_GG * L + l] = v[0];
            sc[HP_PHI * L + l] = v[1];
        }
    }
    if constexpr ((PHASES & 2) != 0) {
        // The pass below reads neighbours of g that other threads of this workgroup stored above.  A workgroup runs on one
        // compute unit and its waves share that unit's vector L1, which stores write through; __syncthreads() makes every wave
        // wait for its outstanding stores before the barrier and is a workgroup-scope release / acquire fence for the
        // compiler, so the loads after it see the stores before it.  g is neither __restrict__ nor const: the compiler may not
        // assume the plane unchanged across the barrier, nor move these loads over it.  No other workgroup touches this plane.
        __syncthreads();
        const float *a = g + off, *b = m + off;
        constexpr int NV = PHASES == 3 ? 5 : 3;
        double v[NV] = {};
        for (PlaneWalk q(nb); q.e < npix; q.next(nb)) {
            const int im = q.e - nb + (q.i == 0 ? npix : 0), jm = q.e - 1 + (q.j == 0 ? nb : 0);
            const float c = px[q.e], ac = a[q.e], bc = b[q.e];
            double wr, wc;                                             // COUPLING 1: both differences take the group's weight
            if constexpr (COUPLING == 0) wr = pot_w<KIND>(px[im] - c, delta), wc = pot_w<KIND>(px[jm] - c, delta);
            else wr = wc = pot_w<KIND>(group_magnitude(px[im] - c, px[jm] - c), delta);
            const double ar = a[im] - ac, acl = a[jm] - ac, br = b[im] - bc, bcl = b[jm] - bc;
            v[0] += wr * ar * ar + wc * acl * acl;
            v[1] += wr * ar * br + wc * acl * bcl;
            v[2] += wr * br * br + wc * bcl * bcl;
            if constexpr (PHASES == 3) {
                const double qv = qm[off + q.e];
                v[3] += (double)ac * qv;
                v[4] += (double)bc * qv;
            }
        }
        block_sum_bcast<NV>(v);
        float beta = 0.f;
        if constexpr (PHASES == 3) {
            const double gBm = v[3] + reg * v[1], mBm = v[4] + reg * v[2];
            beta = mBm > 0.0 ? (float)(-gBm / mBm) : 0.f;
            for (int e = threadIdx.x; e < npix; e += TPB) d[off + e] = a[e] + beta * b[e];
            if (threadIdx.x == 0) {
                sc[HP_BETA * L + l] = (double)beta;
                sc[HP_MBM * L + l] = mBm;
            }
        }
        if (threadIdx.x == 0) {
            sc[HP_C00 * L + l] = v[0];
            sc[HP_C01 * L + l] = v[1];
            sc[HP_C11 * L + l] = v[2];
        }
    }
}

inline bool plane_fits(int nplanes, int na, int nb) { return nplanes > 0 && na > 0 && nb > 0 && (long)na * nb <= 0x7fffffffL - TPB; }
// calls f(std::integral_constant<int, kind>(), std::integral_constant<int, coupling>()) for a potential and a plane-wise coupling
// (0 separated, 1 isotropic); false on anything else
template <class F>
inline bool planes_dispatch(int kind, int coupling, F &&f) {
    if (coupling == 0) return pot_dispatch(kind, [&](auto K) { f(K, std::integral_constant<int, 0>()); });
    if (coupling == 1) return pot_dispatch(kind, [&](auto K) { f(K, std::integral_constant<int, 1>()); });
    return false;
}
}  // namespace

int launch_huber_dir_planes(hipStream_t s, const float *x, const float *r, float *g, const float *m, const float *qm, float *d,
                            int nplanes, int na, int nb, const double *par, int kind, int coupling, double *sc) {
    if (!plane_fits(nplanes, na, nb)) return (int)hipErrorInvalidValue;
    const auto go = [&](auto K, auto C) {
        hipLaunchKernelGGL((huber_dir_planes_kernel<3, decltype(K)::value, decltype(C)::value>), dim3(nplanes), dim3(TPB), 0, s, x, r, g,
                           m, qm, d, na, nb, par, sc);
    };
    if (!planes_dispatch(kind, coupling, go)) return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int launch_huber_planes_grad(hipStream_t s, const float *x, const float *src, float *out, int nplanes, int na, int nb, const double *par,
                             int kind, int coupling, double *sc) {
    if (!plane_fits(nplanes, na, nb)) return (int)hipErrorInvalidValue;
    const auto go = [&](auto K, auto C) {
        hipLaunchKernelGGL((huber_dir_planes_kernel<1, decltype(K)::value, decltype(C)::value>), dim3(nplanes), dim3(TPB), 0, s, x, src,
                           out, (const float *)nullptr, (const float *)nullptr, (float *)nullptr, na, nb, par, sc);
    };
    if (!planes_dispatch(kind, coupling, go)) return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int launch_huber_planes_curv(hipStream_t s, const float *x, const float *p0, const float *p1, int nplanes, int na, int nb,
                             const double *par, int kind, int coupling, double *sc) {
    if (!plane_fits(nplanes, na, nb)) return (int)hipErrorInvalidValue;
    const auto go = [&](auto K, auto C) {
        hipLaunchKernelGGL((huber_dir_planes_kernel<2, decltype(K)::value, decltype(C)::value>), dim3(nplanes), dim3(TPB), 0, s, x,
                           (const float *)nullptr, const_cast<float *>(p0), p1, (const float *)nullptr, (float *)nullptr, na, nb, par, sc);
    };
    if (!planes_dispatch(kind, coupling, go)) return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

namespace {
// The 2x2 majorant step of every plane in the basis [d, m]: qd = Q_D d from the operator, the prior block of (d, m) from that of
// (g, m) by linearity in float64 (d = g + beta m).  A plane without positive curvature (no data, or at its minimum) keeps still.
__global__ __launch_bounds__(TPB) void huber_step_planes_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ d,
                                                                float *__restrict__ m, float *__restrict__ qm,
                                                                const float *__restrict__ qd, const float *__restrict__ g, long npix,
                                                                const double *__restrict__ par, const double *__restrict__ sc,
                                                                int update_r) {
    const int l = blockIdx.x, L = gridDim.x;
    const long off = (long)l * npix;
    const double reg = par[HPP_REG * L + l];
    double v[4] = {0.0, 0.0, 0.0, 0.0};                    // d.Q_D d, d.Q_D m, d.g, m.g
    for (long i = threadIdx.x; i < npix; i += TPB) {
        const double di = d[off + i], gi = g[off + i];
        v[0] += di * (double)qd[off + i];
        v[1] += di * (double)qm[off + i];
        v[2] += di * gi;
        v[3] += (double)m[off + i] * gi;
    }
    block_sum_bcast<4>(v);
    const double beta = sc[HP_BETA * L + l], mBm = sc[HP_MBM * L + l];
    const double c00 = sc[HP_C00 * L + l], c01 = sc[HP_C01 * L + l], c11 = sc[HP_C11 * L + l];
    double dWd, dWm, s0, s1;
    mm_block_of_d(c00, c01, c11, beta, &dWd, &dWm);
    mm_step2(v[0] + reg * dWd, v[1] + reg * dWm, mBm, v[2], v[3], &s0, &s1);
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

int launch_huber_step_planes(hipStream_t s, float *x, float *r, const float *d, float *m, float *qm, const float *qd, const float *g,
                             int nplanes, long npix, const double *par, const double *sc, int update_r) {
    hipLaunchKernelGGL(huber_step_planes_kernel, dim3(nplanes), dim3(TPB), 0, s, x, r, d, m, qm, qd, g, npix, par, sc, update_r);
    return (int)hipGetLastError();
}
