// Coupled priors of the maps (surfh_set_prior_coupling): one potential per GROUP of circular first differences instead of one
// per difference.  With u_r = x[i-1][j] - x[i][j] and u_c = x[i][j-1] - x[i][j] (huber_kernels.hip: huber_grad_kernel's differences):
//   COUPLING 1, isotropic   group = (t, i, j):  m^2 = u_r^2 + u_c^2               prior sum_t sum_ij phi(m)
//   COUPLING 2, vector      group = (i, j):     m^2 = sum_t u_r^2 + u_c^2         prior sum_ij phi(m)
// phi(sqrt(.)) is concave for every kind of huber_dev.h, so the Geman-Reynolds majorant of the separated prior holds with the
// weight of a difference replaced by its group's, w(m) = phi'(m) / m: gradient sum_k D_k^T (w(m) D_k x), curvature sums
// sum_k sum w(m) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2.
// Layout: the weight field is computed ONCE per iterate (coupled_weights_kernel: w [T][na][nb] or [na][nb] in fp32, sum phi(m) in
// float64) and read by the gradient and by the curvature pass.  A pixel's gradient needs the weights of the groups (i, j),
// (i+1, j) and (i, j+1); recomputing them in place costs 3 groups x 2 T differences per element under "vector" (10 T loads
// against 5 + 3), and the curvature pass would pay the group's 2 T differences again per element.  The field is at most the size
// of the maps (a few MB: it stays in L2 between the passes) and the extra launch is one more stream-ordered kernel without a
// host synchronisation.  Only the weight pass depends on the potential: it is instantiated per <KIND, COUPLING>, the two
// readers per <COUPLING>; there is no per-element branch on a runtime value.
// Conventions of the separated pair: TPB = RED_TPB threads, at most HUBER_BLOCKS blocks and a grid-stride loop, float64 block
// sums in a fixed order (block_sums_to, parts_reduce_kernel of reduce_dev.h: the same inputs give the same bits), differences and w in fp32,
// phi in float64, phi' formed as u w so that the gradient and the curvature see the same weight; src and out may alias.
// m^2 is accumulated in float64 (no overflow for any fp32 differences, any T) and m rounded to fp32 once.
#include "huber_dev.h"
#include "kernels.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = RED_TPB;

struct Nbrs {        // offsets of pixel `rem` = i * nb + j and of its circular neighbours inside one [na][nb] plane
    int c, im, ip, jm, jp;
};
__device__ __forceinline__ Nbrs nbrs_of(int rem, int na, int nb) {
    const int i = rem / nb, j = rem - i * nb;
    Nbrs q;
    q.c = rem;
    q.im = (i == 0 ? na - 1 : i - 1) * nb + j;
    q.ip = (i == na - 1 ? 0 : i + 1) * nb + j;
    q.jm = i * nb + (j == 0 ? nb - 1 : j - 1);
    q.jp = i * nb + (j == nb - 1 ? 0 : j + 1);
    return q;
}

// w[g] = pot_w<KIND>(m_g, delta) for the ng groups (COUPLING 1: ng = T plane, g = t * plane + pixel; 2: ng = plane, g = pixel);
// part: [1][gridDim.x] = sum_g phi(m_g)
template <int KIND, int COUPLING>
__global__ __launch_bounds__(TPB) void coupled_weights_kernel(const float *__restrict__ x, float *__restrict__ w, long ng, int T, int na,
                                                              int nb, float delta, double *__restrict__ part) {
    double acc[1] = {0.0};
    const long plane = (long)na * nb, stride = (long)gridDim.x * TPB;
    for (long g = (long)blockIdx.x * TPB + threadIdx.x; g < ng; g += stride) {
        double m2 = 0.0;
        if constexpr (COUPLING == 1) {
            const long t = g / plane;
            const Nbrs q = nbrs_of((int)(g - t * plane), na, nb);
            const float *p = x + t * plane;
            const float c = p[q.c], ur = p[q.im] - c, uc = p[q.jm] - c;
            m2 = (double)ur * (double)ur + (double)uc * (double)uc;
        } else {
            const Nbrs q = nbrs_of((int)g, na, nb);
            for (int t = 0; t < T; ++t) {
                const float *p = x + t * plane;
                const float c = p[q.c], ur = p[q.im] - c, uc = p[q.jm] - c;
                m2 += (double)ur * (double)ur + (double)uc * (double)uc;
            }
        }
        const float m = (float)sqrt(m2);
        w[g] = pot_w<KIND>(m, delta);
        acc[0] += pot_phi<KIND>(m, delta);
    }
    block_sums_to<1>(acc, part);
}

// the weight field's plane of map element e = t * plane + pixel
template <int COUPLING>
__device__ __forceinline__ const float *weights_of(const float *w, long t, long plane) {
    return COUPLING == 1 ? w + t * plane : w;
}

// out = src + coef sum_k D_k^T (w D_k x),  (D^T v)[i] = v[i+1] - v[i];  part: [1][gridDim.x] = out.out
template <int COUPLING>
__global__ __launch_bounds__(TPB) void coupled_grad_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *src,
                                                           float *out, long n, int na, int nb, float coef, double *__restrict__ part) {
    double acc[1] = {0.0};
    const long plane = (long)na * nb, stride = (long)gridDim.x * TPB;
    for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        const long t = e / plane;
        const Nbrs q = nbrs_of((int)(e - t * plane), na, nb);
        const float *p = x + t * plane, *wp = weights_of<COUPLING>(w, t, plane);
        const float c = p[q.c], w0 = wp[q.c];
        const float ur = p[q.im] - c, uc = p[q.jm] - c;            // (Dr x)[i][j], (Dc x)[i][j]: the group of (i, j)
        const float urn = c - p[q.ip], ucn = c - p[q.jp];          // (Dr x)[i+1][j], (Dc x)[i][j+1]: the groups of the successors
        const float pg = (wp[q.ip] * urn - w0 * ur) + (wp[q.jp] * ucn - w0 * uc);
        const float g = src[e] + coef * pg;
        out[e] = g;
        acc[0] += (double)g * (double)g;
    }
    block_sums_to<1>(acc, part);
}

// part: [3][gridDim.x] = sum_k sum w (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2 under the stored weights
template <int COUPLING>
__global__ __launch_bounds__(TPB) void coupled_curv_kernel(const float *__restrict__ w, const float *__restrict__ p0,
                                                           const float *__restrict__ p1, long n, int na, int nb,
                                                           double *__restrict__ part) {
    double acc[3] = {0.0, 0.0, 0.0};
    const long plane = (long)na * nb, stride = (long)gridDim.x * TPB;
    for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        const long t = e / plane;
        const Nbrs q = nbrs_of((int)(e - t * plane), na, nb);
        const float *a = p0 + t * plane, *b = p1 + t * plane;
        const double wg = weights_of<COUPLING>(w, t, plane)[q.c];
        const float ac = a[q.c], bc = b[q.c];
        const double ar = a[q.im] - ac, acl = a[q.jm] - ac, br = b[q.im] - bc, bcl = b[q.jm] - bc;
        acc[0] += wg * (ar * ar + acl * acl);
        acc[1] += wg * (ar * br + acl * bcl);
        acc[2] += wg * (br * br + bcl * bcl);
    }
    block_sums_to<3>(acc, part);
}

inline bool maps_fit(int T, int na, int nb) { return T >= 1 && na >= 1 && nb >= 1 && (long)na * nb <= 0x7fffffffL; }

// calls f(std::integral_constant<int, coupling>()) for a coupled prior; false on anything else
template <class F>
inline bool coupling_dispatch(int coupling, F &&f) {
    switch (coupling) {
    case 1: f(std::integral_constant<int, 1>()); return true;
    case 2: f(std::integral_constant<int, 2>()); return true;
    default: return false;
    }
}

}  // namespace

size_t coupled_weights_floats(int coupling, int T, int na, int nb) { return (size_t)(coupling == 1 ? T : 1) * na * nb; }

int launch_coupled_weights(hipStream_t s, const float *x, float *w, int T, int na, int nb, float delta, int kind, int coupling,
                           double *scratch, double *phi_sum) {
    if (!maps_fit(T, na, nb)) return (int)hipErrorInvalidValue;
    const long ng = (long)coupled_weights_floats(coupling, T, na, nb);
    const int nbk = nblocks(ng, HUBER_BLOCKS);
    bool ok = false;
    const auto go = [&](auto K) {
        ok = coupling_dispatch(coupling, [&](auto C) {
            hipLaunchKernelGGL((coupled_weights_kernel<decltype(K)::value, decltype(C)::value>), dim3(nbk), dim3(TPB), 0, s, x, w, ng, T, na,
                               nb, delta, scratch);
        });
    };
    if (!pot_dispatch(kind, go) || !ok) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(1), dim3(TPB), 0, s, scratch, nbk, phi_sum);
    return (int)hipGetLastError();
}

int launch_coupled_grad(hipStream_t s, const float *x, const float *w, const float *src, float *out, int T, int na, int nb, float coef,
                        int coupling, double *scratch, double *gg_sum) {
    if (!maps_fit(T, na, nb)) return (int)hipErrorInvalidValue;
    const long n = (long)T * na * nb;
    const int nbk = nblocks(n, HUBER_BLOCKS);
    const auto go = [&](auto C) {
        hipLaunchKernelGGL(coupled_grad_kernel<decltype(C)::value>, dim3(nbk), dim3(TPB), 0, s, x, w, src, out, n, na, nb, coef, scratch);
    };
    if (!coupling_dispatch(coupling, go)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(1), dim3(TPB), 0, s, scratch, nbk, gg_sum);
    return (int)hipGetLastError();
}

int launch_coupled_curv(hipStream_t s, const float *w, const float *p0, const float *p1, int T, int na, int nb, int coupling,
                        double *scratch, double *sums) {
    if (!maps_fit(T, na, nb)) return (int)hipErrorInvalidValue;
    const long n = (long)T * na * nb;
    const int nbk = nblocks(n, HUBER_BLOCKS);
    const auto go = [&](auto C) {
        hipLaunchKernelGGL(coupled_curv_kernel<decltype(C)::value>, dim3(nbk), dim3(TPB), 0, s, w, p0, p1, n, na, nb, scratch);
    };
    if (!coupling_dispatch(coupling, go)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(3), dim3(TPB), 0, s, scratch, nbk, sums);
    return (int)hipGetLastError();
}
