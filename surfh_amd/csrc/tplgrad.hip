// Template refinement (include/surfh_amd.h: surfh_adjoint_templates, surfh_cg_templates): the transpose of the operator with
// respect to the templates, maps held fixed, and the small vector kernels of the template solver.
//
// A_x : S -> A(S) x is the forward model with S in the templates' place.  Its transpose takes the cube-space adjoint g = B^T u (what
// the adjoint's scatters leave in the accumulator) to
//     G[t, l] = sum_pixels x_t (C_l^T g_l)  =  sum_k c_k Re( conj(xhat_t(k)) conj(otf_l(k)) ghat_l(k) )
// -- the transforms are unitary (plan.hip: 1 / sqrt(N) on every matrix), so Parseval holds with weight 1; c_k = 1 on the bins of
// the half spectrum that are their own conjugate (kb = 0, 2 kb = Nb) and 2 on the others.  It is the adjoint mix (specmix_adj) with
// its reduction axis swapped: a sum over frequency bins instead of over wavelengths.
//
// Spectral route (interleaved spectra [KAP][KBP][LP][2]): a workgroup of 64 lanes owns 128 wavelengths (one float4 = two complex
// values of each array per lane: whole contiguous lines per wave instruction) and walks a slab of frequency bins; the maps' spectra
// of a bin are workgroup-uniform (scalar loads).  Products in fp32, sums in float64.  The slabs' partial sums [slab][T][LP] are
// added by a second kernel in slab order: no atomics, the same inputs give the same bits.  It reads the spectrum and the OTF once
// (2 x 8 bytes per bin and wavelength, four bins in flight per lane), like specmix_adj.  Only the bins ka < Na, kb <= Nb / 2 are visited and only the plan's
// planes are written out: the padding of KAP / KBP / LP contributes and receives nothing.
// Spatial route (plans without that spectrum: dense transforms, verification plans, T > 4): the same two stages over slabs of
// pixels of the cube-space adjoint after its OTF^T, cube [NBP][NAP][LP], against the maps [T][Na][Nb].
#include "tplgrad.h"

#include <algorithm>

#include "kernels.h"

namespace {

constexpr int TG_TPB = 64;             // lanes of a workgroup: 128 wavelengths, two per lane
constexpr int TG_MAXT = SURFH_MAX_TEMPLATES;

template <int MT>
__global__ __launch_bounds__(TG_TPB) void tplgrad_spec_kernel(const float *__restrict__ spec, const float *__restrict__ sotf,
                                                              const float *__restrict__ mhat, double *__restrict__ part, int T, int Na,
                                                              int Nb, long KBP, long PL, int LP, int per) {
    const int l2 = (blockIdx.x * TG_TPB + threadIdx.x) * 2;
    const int hb = Nb / 2 + 1, nbin = Na * hb;
    const int j0 = blockIdx.y * per, j1 = min(j0 + per, nbin);
    double a0[MT], a1[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) a0[t] = a1[t] = 0.0;
    auto bin = [&](int j, const float4 h, const float4 g) {
        const int ka = j / hb, kb = j - ka * hb;
        const long k = (long)ka * KBP + kb;
        const float w = (kb == 0 || 2 * kb == Nb) ? 1.f : 2.f;
        // z = conj(otf) ghat for the lane's two wavelengths
        const float zr0 = h.x * g.x + h.y * g.y, zi0 = h.x * g.y - h.y * g.x;
        const float zr1 = h.z * g.z + h.w * g.w, zi1 = h.z * g.w - h.w * g.z;
#pragma unroll
        for (int t = 0; t < MT; ++t)
            if (t < T) {
                const float xr = w * mhat[((long)t * 2 + 0) * PL + k], xi = w * mhat[((long)t * 2 + 1) * PL + k];
                a0[t] += (double)(xr * zr0 + xi * zi0);
                a1[t] += (double)(xr * zr1 + xi * zi1);
            }
    };
    auto at = [&](int j) {
        const int ka = j / hb, kb = j - ka * hb;
        return (((long)ka * KBP + kb) * LP + l2) * 2;
    };
    int j = j0;
    for (; j + 3 < j1; j += 4) {       // four bins = eight float4 in flight per lane; the sums keep the order of the bins
        const long o0 = at(j), o1 = at(j + 1), o2 = at(j + 2), o3 = at(j + 3);
        const float4 h0 = *reinterpret_cast<const float4 *>(sotf + o0), g0 = *reinterpret_cast<const float4 *>(spec + o0);
        const float4 h1 = *reinterpret_cast<const float4 *>(sotf + o1), g1 = *reinterpret_cast<const float4 *>(spec + o1);
        const float4 h2 = *reinterpret_cast<const float4 *>(sotf + o2), g2 = *reinterpret_cast<const float4 *>(spec + o2);
        const float4 h3 = *reinterpret_cast<const float4 *>(sotf + o3), g3 = *reinterpret_cast<const float4 *>(spec + o3);
        bin(j, h0, g0);
        bin(j + 1, h1, g1);
        bin(j + 2, h2, g2);
        bin(j + 3, h3, g3);
    }
    for (; j < j1; ++j) {
        const long o0 = at(j);
        bin(j, *reinterpret_cast<const float4 *>(sotf + o0), *reinterpret_cast<const float4 *>(spec + o0));
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
        if (t < T) *reinterpret_cast<double2 *>(part + ((long)blockIdx.y * T + t) * LP + l2) = make_double2(a0[t], a1[t]);
}

// the same reduction over slabs of pixels: cube [NBP][NAP][LP] (rows beta), maps [T][Na][Nb]
__global__ __launch_bounds__(TG_TPB) void tplgrad_pix_kernel(const float *__restrict__ cube, const float *__restrict__ maps,
                                                             double *__restrict__ part, int T, int Na, int Nb, int NAP, int LP, int per) {
    const int l2 = (blockIdx.x * TG_TPB + threadIdx.x) * 2;
    const long npix = (long)Na * Nb;
    const long j0 = (long)blockIdx.y * per, j1 = min(j0 + (long)per, npix);
    double a0[TG_MAXT], a1[TG_MAXT];
#pragma unroll
    for (int t = 0; t < TG_MAXT; ++t) a0[t] = a1[t] = 0.0;
    for (long j = j0; j < j1; ++j) {
        const int b = (int)(j / Na), a = (int)(j - (long)b * Na);
        const float2 h = *reinterpret_cast<const float2 *>(cube + ((long)b * NAP + a) * LP + l2);
#pragma unroll
        for (int t = 0; t < TG_MAXT; ++t)
            if (t < T) {
                const float x = maps[((long)t * Na + a) * Nb + b];
                a0[t] += (double)(x * h.x);
                a1[t] += (double)(x * h.y);
            }
    }
#pragma unroll
    for (int t = 0; t < TG_MAXT; ++t)
        if (t < T) *reinterpret_cast<double2 *>(part + ((long)blockIdx.y * T + t) * LP + l2) = make_double2(a0[t], a1[t]);
}

// G[t][l] = sum over the slabs, in slab order, of part[slab][t][cidx[l]]; 0 on a plane the plan does not hold (cidx < 0)
__global__ __launch_bounds__(256) void tplgrad_sum_kernel(const double *__restrict__ part, const int *__restrict__ cidx, float *__restrict__ G,
                                                          int T, int Lc, int LP, int nslab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * Lc) return;
    const int t = i / Lc, l = i - t * Lc, c = cidx[l];
    double s = 0.0;
    if (c >= 0)
        for (int k = 0; k < nslab; ++k) s += part[((long)k * T + t) * LP + c];
    G[i] = (float)s;
}

// spec *= conj(sotf), in place, one thread per complex value (interleaved [PL][LP][2] or planar [2][PL][LP])
__global__ __launch_bounds__(256) void otf_conj_mul_kernel(float *spec, const float *__restrict__ sotf, long PL, int LP, int ilv) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= PL * LP) return;
    if (ilv) {
        const float2 h = *reinterpret_cast<const float2 *>(sotf + 2 * i), g = *reinterpret_cast<const float2 *>(spec + 2 * i);
        *reinterpret_cast<float2 *>(spec + 2 * i) = make_float2(h.x * g.x + h.y * g.y, h.x * g.y - h.y * g.x);
    } else {
        const float hr = sotf[i], hi = sotf[PL * LP + i], gr = spec[i], gi = spec[PL * LP + i];
        spec[i] = hr * gr + hi * gi;
        spec[PL * LP + i] = hr * gi - hi * gr;
    }
}

// templates in cube-plane order S [T][Lc] <-> the plan's compact, padded rows tpl [T][LP] (pidx: compact index -> plane, -1: none)
__global__ __launch_bounds__(256) void tpl_pack_kernel(const float *__restrict__ S, const int *__restrict__ pidx, float *__restrict__ tpl, int T,
                                                       int Lc, int LP) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * LP) return;
    const int t = i / LP, c = i - t * LP, l = pidx[c];
    tpl[i] = l >= 0 ? S[(long)t * Lc + l] : 0.f;
}

// q += mu_spec D^T D d along the wavelength, D the first difference with open ends, on [T][Lc]
__global__ __launch_bounds__(256) void tpl_prior_add_kernel(const float *__restrict__ d, float *__restrict__ q, int T, int Lc, float mu_spec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * Lc) return;
    const int l = i % Lc;
    float v = 0.f;
    if (l > 0) v += d[i] - d[i - 1];
    if (l + 1 < Lc) v += d[i] - d[i + 1];
    q[i] += mu_spec * v;
}

// per-block float64 partial sums of  sum w (y - u)^2  (w null: 1; a sample with w <= 0 is taken out by a select, NaN included)
__global__ __launch_bounds__(256) void wres_sq_kernel(const float *__restrict__ y, const float *__restrict__ u, const float *__restrict__ w,
                                                      long n, double *__restrict__ part) {
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float wi = w ? w[i] : 1.f;
        const float r = y[i] - u[i];
        s += wi > 0.f ? (double)wi * (double)r * (double)r : 0.0;
    }
    __shared__ double red[4];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void sum_parts_kernel(const double *__restrict__ part, int n, double *__restrict__ out) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += part[i];
    *out = s;
}

int last_error() { return (int)hipGetLastError(); }

}  // namespace

// slabs of the first stage: about 2048 workgroups in all, at most 512 rows of partial sums for the second stage to add
static int tplgrad_slabs(long work, int LP) {
    const long chunks = LP / 128;
    long n = 2048 / (chunks > 0 ? chunks : 1);
    if (n > 512) n = 512;
    if (n > work) n = work;
    return (int)(n < 1 ? 1 : n);
}

size_t tplgrad_part_doubles(int T, int Na, int Nb, int LP, bool spectral) {
    const long work = spectral ? (long)Na * (Nb / 2 + 1) : (long)Na * Nb;
    return (size_t)tplgrad_slabs(work, LP) * (size_t)T * (size_t)LP;
}

int launch_tplgrad_spec(hipStream_t s, const float *spec, const float *sotf, const float *mhat, double *part, const int *cidx, float *G, int T,
                        int Lc, int Na, int Nb, long KBP, long PL, int LP) {
    if (T < 1 || T > 4 || LP % 128 != 0) return (int)hipErrorInvalidValue;
    const int nbin = Na * (Nb / 2 + 1), nslab = tplgrad_slabs(nbin, LP), per = (nbin + nslab - 1) / nslab;
    // every slab writes its rows of `part`, an empty one (nbin not a multiple of per) zeros
    hipLaunchKernelGGL(tplgrad_spec_kernel<4>, dim3(LP / 128, nslab), dim3(TG_TPB), 0, s, spec, sotf, mhat, part, T, Na, Nb, KBP, PL, LP, per);
    hipLaunchKernelGGL(tplgrad_sum_kernel, dim3((T * Lc + 255) / 256), dim3(256), 0, s, part, cidx, G, T, Lc, LP, nslab);
    return last_error();
}

int launch_tplgrad_pix(hipStream_t s, const float *cube, const float *maps, double *part, const int *cidx, float *G, int T, int Lc, int Na,
                       int Nb, int NAP, int LP) {
    if (T < 1 || T > TG_MAXT || LP % 128 != 0) return (int)hipErrorInvalidValue;
    const long npix = (long)Na * Nb;
    const int nslab = tplgrad_slabs(npix, LP), per = (int)((npix + nslab - 1) / nslab);
    hipLaunchKernelGGL(tplgrad_pix_kernel, dim3(LP / 128, nslab), dim3(TG_TPB), 0, s, cube, maps, part, T, Na, Nb, NAP, LP, per);
    hipLaunchKernelGGL(tplgrad_sum_kernel, dim3((T * Lc + 255) / 256), dim3(256), 0, s, part, cidx, G, T, Lc, LP, nslab);
    return last_error();
}

int launch_otf_conj_mul(hipStream_t s, float *spec, const float *sotf, long PL, int LP, int ilv) {
    const long n = PL * LP;
    hipLaunchKernelGGL(otf_conj_mul_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, spec, sotf, PL, LP, ilv);
    return last_error();
}

int launch_tpl_pack(hipStream_t s, const float *S, const int *pidx, float *tpl, int T, int Lc, int LP) {
    hipLaunchKernelGGL(tpl_pack_kernel, dim3((T * LP + 255) / 256), dim3(256), 0, s, S, pidx, tpl, T, Lc, LP);
    return last_error();
}

int launch_tpl_prior_add(hipStream_t s, const float *d, float *q, int T, int Lc, float mu_spec) {
    hipLaunchKernelGGL(tpl_prior_add_kernel, dim3((T * Lc + 255) / 256), dim3(256), 0, s, d, q, T, Lc, mu_spec);
    return last_error();
}

int launch_wres_sq(hipStream_t s, const float *y, const float *u, const float *w, long n, double *scratch, double *out) {
    const int nb = (int)std::min<long>(512, (n + 255) / 256);
    hipLaunchKernelGGL(wres_sq_kernel, dim3(nb < 1 ? 1 : nb), dim3(256), 0, s, y, u, w, n, scratch);
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(1), 0, s, scratch, nb < 1 ? 1 : nb, out);
    return last_error();
}
