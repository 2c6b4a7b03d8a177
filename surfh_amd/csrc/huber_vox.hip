// Huber priors on the cube [Lc][na][nb] (surfh_mmmg_huber_vox): the separated circular differences inside every plane
// (u_r = x[l][i-1][j] - x[l][i][j], u_c = x[l][i][j-1] - x[l][i][j], as on the maps) under one threshold, and the open
// difference along wavelength (u_l = x[l+1] - x[l], l = 0 .. Lc-2: Lc - 1 difference planes, no wrap) under another.
//
// Mapping: marching along wavelength.  A thread owns pixel (i, j) of a tile of 256 consecutive pixels of the plane and walks a
// chunk of planes with the previous, current and next value along wavelength in registers (one halo plane per chunk): each voxel
// of x (and of p0, p1) is loaded once as a centre value, lanes read consecutive floats of a row, and the in-plane neighbours are
// neighbouring lanes and rows of the plane that is being loaded anyway.  The grid is (pixel tiles, wavelength chunks), at most
// 2048 blocks.  A flat one-thread-per-voxel mapping was measured against it and dropped (1.3x to 1.6x slower, 1.4x / 1.5x
// the memory traffic).  No 16-byte accesses: with an odd plane size (251 x 251, 501 x 501) neither the rows nor the planes
// l - 1, l + 1 are 16-byte aligned with respect to each other.
// Reductions: float64 per thread, per block in a fixed order into `scratch` [K][blocks], then one block per sum -- the same
// inputs give the same bits (reduce_dev.h).
#include "huber_dev.h"
#include "kernels.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = RED_TPB;
constexpr int VOX_BLOCKS = 2048;      // 8 blocks per CU; [6][2048] partials fit launch_huber_vox_scratch_doubles()

// grad: out = src + cs (Dr^T phi'_ds(Dr x) + Dc^T phi'_ds(Dc x)) + cl Dl^T phi'_dl(Dl x);  (D^T v)[i] = v[i+1] - v[i] in the plane,
// (Dl^T v)[l] = v[l-1] - v[l] with v[-1] = v[Lc-1] = 0.  part: [3][blocks] (out.out, sum phi_ds, sum phi_dl).
// src and out may be the same array (each element is read and written by one thread).
// curv: part [6][blocks]: sum w (D p0)^2, (D p0)(D p1), (D p1)^2 over the two in-plane families with w = w_ds(D_k x), then the
// same three over the wavelength differences with w = w_dl(Dl x) (weights recomputed, none stored).
// Grid (pixel tiles, wavelength chunks); chunk c owns planes [Lc c / C, Lc (c + 1) / C)
// KS, KL: the potential of the in-plane families and of the wavelength family (huber_dev.h), all 3 x 3 pairs instantiated
struct PixNbrs {
    int up, dn, lf, rt;                // offsets inside a plane of the four circular neighbours
    __device__ PixNbrs(int p, int na, int nb) {
        const int i = p / nb, j = p - i * nb;
        up = (i == 0 ? na - 1 : i - 1) * nb + j;
        dn = (i == na - 1 ? 0 : i + 1) * nb + j;
        lf = i * nb + (j == 0 ? nb - 1 : j - 1);
        rt = i * nb + (j == nb - 1 ? 0 : j + 1);
    }
};

template <int KS, int KL>
__global__ __launch_bounds__(TPB) void huber_vox_grad_kernel(const float *__restrict__ x, const float *src, float *out, int Lc,
                                                                   int na, int nb, float cs, float ds, float cl, float dl,
                                                                   double *__restrict__ part) {
    double acc[3] = {0.0, 0.0, 0.0};
    const int npix = na * nb;
    const int l0 = (int)((long)Lc * blockIdx.y / gridDim.y), l1 = (int)((long)Lc * (blockIdx.y + 1) / gridDim.y);
    for (int p = blockIdx.x * TPB + threadIdx.x; p < npix; p += gridDim.x * TPB) {
        const PixNbrs q(p, na, nb);
        const float *pl = x + (long)l0 * npix;
        float c = pl[p];
        float vprev = l0 > 0 ? pot_dphi<KL>(c - pl[p - (long)npix], dl) : 0.f;      // phi'(Dl x) at l0 - 1: the halo plane
        for (int l = l0; l < l1; ++l, pl += npix) {
            float nxt = 0.f, vown = 0.f;
            if (l < Lc - 1) {
                nxt = pl[p + (long)npix];
                const float ul = nxt - c;
                vown = pot_dphi<KL>(ul, dl);
                acc[2] += pot_phi<KL>(ul, dl);
            }
            const float ur = pl[q.up] - c, uc = pl[q.lf] - c, urn = c - pl[q.dn], ucn = c - pl[q.rt];
            const float pgs = (pot_dphi<KS>(urn, ds) - pot_dphi<KS>(ur, ds)) + (pot_dphi<KS>(ucn, ds) - pot_dphi<KS>(uc, ds));
            const long e = (long)l * npix + p;
            const float g = src[e] + cs * pgs + cl * (vprev - vown);
            out[e] = g;
            acc[0] += (double)g * (double)g;
            acc[1] += pot_phi<KS>(ur, ds) + pot_phi<KS>(uc, ds);
            vprev = vown;
            c = nxt;
        }
    }
    block_sums_to<3>(acc, part, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
}

template <int KS, int KL>
__global__ __launch_bounds__(TPB) void huber_vox_curv_kernel(const float *__restrict__ x, const float *__restrict__ p0,
                                                                   const float *__restrict__ p1, int Lc, int na, int nb, float ds,
                                                                   float dl, double *__restrict__ part) {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int npix = na * nb;
    const int l0 = (int)((long)Lc * blockIdx.y / gridDim.y), l1 = (int)((long)Lc * (blockIdx.y + 1) / gridDim.y);
    for (int p = blockIdx.x * TPB + threadIdx.x; p < npix; p += gridDim.x * TPB) {
        const PixNbrs q(p, na, nb);
        const long off = (long)l0 * npix;
        const float *px = x + off, *pa = p0 + off, *pb = p1 + off;
        float c = px[p], ac = pa[p], bc = pb[p];
        for (int l = l0; l < l1; ++l, px += npix, pa += npix, pb += npix) {
            const double wr = pot_w<KS>(px[q.up] - c, ds), wc = pot_w<KS>(px[q.lf] - c, ds);
            const double ar = pa[q.up] - ac, acl = pa[q.lf] - ac, br = pb[q.up] - bc, bcl = pb[q.lf] - bc;
            acc[0] += wr * ar * ar + wc * acl * acl;
            acc[1] += wr * ar * br + wc * acl * bcl;
            acc[2] += wr * br * br + wc * bcl * bcl;
            float cn = 0.f, an = 0.f, bn = 0.f;
            if (l < Lc - 1) {
                cn = px[p + (long)npix];
                an = pa[p + (long)npix];
                bn = pb[p + (long)npix];
                const double wl = pot_w<KL>(cn - c, dl), al = an - ac, bl = bn - bc;
                acc[3] += wl * al * al;
                acc[4] += wl * al * bl;
                acc[5] += wl * bl * bl;
            }
            c = cn;
            ac = an;
            bc = bn;
        }
    }
    block_sums_to<6>(acc, part, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
}

// pot_dispatch on the spatial kind around one on the spectral kind: f(KS) returns what the inner dispatch returned
template <class F>
inline bool vox_dispatch(int ks, F &&f) {
    bool ok = false;
    return pot_dispatch(ks, [&](auto KS) { ok = f(KS); }) && ok;
}

}  // namespace

static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");
// tiles x chunks <= VOX_BLOCKS blocks: every tile of 256 pixels its own block where that leaves room, as many chunks as fit
dim3 march_grid(int Lc, int na, int nb) {
    const long tiles = ((long)na * nb + TPB - 1) / TPB;
    const int gx = (int)(tiles > VOX_BLOCKS ? VOX_BLOCKS : tiles);
    int gy = VOX_BLOCKS / gx;
    if (gy > Lc) gy = Lc;
    return dim3(gx, gy < 1 ? 1 : gy);
}

size_t launch_huber_vox_scratch_doubles() { return (size_t)6 * VOX_BLOCKS; }

int launch_huber_vox_grad(hipStream_t s, const float *x, const float *src, float *out, int Lc, int na, int nb, float cs, float ds,
                          float cl, float dl, int ks, int kl, double *scratch, double *sums) {
    if (Lc < 1 || na < 1 || nb < 1 || (long)na * nb > 0x7fffffffL - 2 * TPB * (long)VOX_BLOCKS) return (int)hipErrorInvalidValue;
    const dim3 g = march_grid(Lc, na, nb);
    const auto go = [&](auto KS) {
        return pot_dispatch(kl, [&](auto KL) {
            hipLaunchKernelGGL((huber_vox_grad_kernel<decltype(KS)::value, decltype(KL)::value>), g, dim3(TPB), 0, s, x, src, out, Lc, na,
                               nb, cs, ds, cl, dl, scratch);
        });
    };
    if (!vox_dispatch(ks, go)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(3), dim3(TPB), 0, s, scratch, (int)(g.x * g.y), sums);
    return (int)hipGetLastError();
}

int launch_huber_vox_curv(hipStream_t s, const float *x, const float *p0, const float *p1, int Lc, int na, int nb, float ds, float dl,
                          int ks, int kl, double *scratch, double *sums) {
    if (Lc < 1 || na < 1 || nb < 1 || (long)na * nb > 0x7fffffffL - 2 * TPB * (long)VOX_BLOCKS) return (int)hipErrorInvalidValue;
    const dim3 g = march_grid(Lc, na, nb);
    const auto go = [&](auto KS) {
        return pot_dispatch(kl, [&](auto KL) {
            hipLaunchKernelGGL((huber_vox_curv_kernel<decltype(KS)::value, decltype(KL)::value>), g, dim3(TPB), 0, s, x, p0, p1, Lc, na,
                               nb, ds, dl, scratch);
        });
    };
    if (!vox_dispatch(ks, go)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3(6), dim3(TPB), 0, s, scratch, (int)(g.x * g.y), sums);
    return (int)hipGetLastError();
}
