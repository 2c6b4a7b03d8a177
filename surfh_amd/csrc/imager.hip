// Kernels of the imager data term (include/surfh_amd.h: surfh_set_imager): a multi-filter broadband imager observes the cube the
// maps span, blurred plane by plane, integrated over wavelength under F filters and summed over d x d cube pixels,
//   y_im[f] = S_d sum_l wf[f,l] irfft2(sotf[l] rfft2(sum_t tpl[t,l] x[t])).
// In the Fourier domain of the maps that is F*T complex values per bin, G[f,t,k] = sum_l wf[f,l] tpl[t,l] sotf[l,k], built once
// (imager_build_g); an application is then two pointwise mixes of T and F half spectra around the plan's own plane transforms and
// a pass over F images.  Every kernel here is a bandwidth-bound pass over at most max(T, F) planes, lanes along the contiguous
// axis (k_beta / beta), no atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace {

constexpr int IM_BLOCK = 256;
constexpr int IM_TMAX = SURFH_MAX_TEMPLATES;

// ---- G -----------------------------------------------------------------------------------------------------------------------
// One wavefront per frequency bin and filter, lanes along the wavelength (the contiguous axis of sotf).  The sum over l has ONE
// order whatever the number of launches it is spread over: wavelengths are taken in aligned groups of 32, a group is summed by a
// fixed butterfly, the groups are added one after the other to the float64 accumulator acc [F][T][2][PL] (read and written back
// by every launch).  So a build streamed in chunks of any multiple of 32 planes gives the bits of the build in one piece.
// sotf: re at sotf[k * sk + l * sl], im at + im_off; tpl [T][ldt] fp32, wf [F][ldw] float64, both zero beyond the last plane;
// L a multiple of 64.
__global__ __launch_bounds__(IM_BLOCK) void imager_build_g_kernel(const float *__restrict__ sotf, long sk, long sl, long im_off,
                                                                  const float *__restrict__ tpl, long ldt, const double *__restrict__ wf,
                                                                  long ldw, int L, double *__restrict__ acc, int T, int Na, int nkb,
                                                                  long KBP, long PL) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long bin = (long)blockIdx.x * (IM_BLOCK / 64) + wave;
    if (bin >= (long)Na * nkb) return;                       // whole wavefronts leave: the shuffles below see full ones
    const int f = blockIdx.y;
    const long k = (bin / nkb) * KBP + bin % nkb;
    double ar[IM_TMAX], ai[IM_TMAX];
    double *const out = acc + (size_t)f * T * 2 * PL + k;
#pragma unroll
    for (int t = 0; t < IM_TMAX; ++t) {
        ar[t] = (lane == 0 && t < T) ? out[(size_t)(2 * t) * PL] : 0.0;
        ai[t] = (lane == 0 && t < T) ? out[(size_t)(2 * t + 1) * PL] : 0.0;
    }
    const float *const sp = sotf + k * sk;
    for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        const double w = wf[(size_t)f * ldw + l];
        const double sr = (double)sp[l * sl], si = (double)sp[l * sl + im_off];
#pragma unroll
        for (int t = 0; t < IM_TMAX; ++t) {
            if (t >= T) break;
            const double c = w * (double)tpl[(size_t)t * ldt + l];
            double pr = c * sr, pi = c * si;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {              // stays inside each half of the wavefront: two groups of 32
                pr += __shfl_xor(pr, o);
                pi += __shfl_xor(pi, o);
            }
            const double pr2 = __shfl(pr, 32), pi2 = __shfl(pi, 32);
            ar[t] = (ar[t] + pr) + pr2;
            ai[t] = (ai[t] + pi) + pi2;
        }
    }
    if (lane != 0) return;
#pragma unroll
    for (int t = 0; t < IM_TMAX; ++t) {
        if (t >= T) break;
        out[(size_t)(2 * t) * PL] = ar[t];
        out[(size_t)(2 * t + 1) * PL] = ai[t];
    }
}

__global__ __launch_bounds__(IM_BLOCK) void imager_g_store_kernel(const double *__restrict__ acc, float *__restrict__ g, long n) {
    const long i = (long)blockIdx.x * IM_BLOCK + threadIdx.x;
    if (i < n) g[i] = (float)acc[i];
}

// host OTF chunk [n][Na][nkb] complex (as float pairs) -> planar [2][KAP][KBP][CH], wavelength innermost: a transpose, through a
// 32 x 32 tile in LDS so that both sides move whole lines (the loads run along the bin, the stores along the wavelength).  Planes
// n <= l < CH of the observed bins are written as zero; the padding bins are never read by imager_build_g.  CH a multiple of 32.
__global__ __launch_bounds__(IM_BLOCK) void imager_otf_chunk_kernel(const float2 *__restrict__ src, float *__restrict__ dst, int n, int CH,
                                                                    int Na, int nkb, long KBP, long PL) {
    __shared__ float2 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const long nbin = (long)Na * nkb, b0 = (long)blockIdx.x * 32;
    const int l0 = blockIdx.y * 32;
#pragma unroll
    for (int r = 0; r < 32; r += IM_BLOCK / 32) {
        const int l = l0 + ty + r;
        const long bin = b0 + tx;
        tile[ty + r][tx] = (l < n && bin < nbin) ? src[(size_t)l * nbin + bin] : make_float2(0.f, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 32; r += IM_BLOCK / 32) {
        const long bin = b0 + ty + r;
        if (bin >= nbin) continue;
        const long k = (bin / nkb) * KBP + bin % nkb;
        const float2 v = tile[tx][ty + r];
        dst[k * CH + l0 + tx] = v.x;
        dst[(PL + k) * CH + l0 + tx] = v.y;
    }
}

// ---- the two mixes: pointwise in the frequency bin, k across lanes; half spectra planar [B][2][PL] as rfft2_planes leaves them and
// irfft2_planes takes them (ortho transforms, Hermitian weights inside the inverse: no scale here; G is zero in the padding bins, so
// is every output there)
__global__ __launch_bounds__(IM_BLOCK) void imager_mix_fwd_kernel(const float *__restrict__ g, const float *__restrict__ xhat,
                                                                  float *__restrict__ zhat, int F, int T, long PL) {
    const long k = (long)blockIdx.x * IM_BLOCK + threadIdx.x;
    if (k >= PL) return;
    float xr[IM_TMAX], xi[IM_TMAX];
#pragma unroll
    for (int t = 0; t < IM_TMAX; ++t) {
        xr[t] = t < T ? xhat[(size_t)(2 * t) * PL + k] : 0.f;
        xi[t] = t < T ? xhat[(size_t)(2 * t + 1) * PL + k] : 0.f;
    }
    for (int f = 0; f < F; ++f) {
        const float *const gf = g + (size_t)f * T * 2 * PL + k;
        float zr = 0.f, zi = 0.f;
#pragma unroll
        for (int t = 0; t < IM_TMAX; ++t) {
            if (t >= T) break;
            const float gr = gf[(size_t)(2 * t) * PL], gi = gf[(size_t)(2 * t + 1) * PL];
            zr += gr * xr[t] - gi * xi[t];
            zi += gr * xi[t] + gi * xr[t];
        }
        zhat[(size_t)(2 * f) * PL + k] = zr;
        zhat[(size_t)(2 * f + 1) * PL + k] = zi;
    }
}

// ghat[t] (+)= scale * sum_f conj(G[f,t]) yhat[f]
__global__ __launch_bounds__(IM_BLOCK) void imager_mix_adj_kernel(const float *__restrict__ g, const float *__restrict__ yhat,
                                                                  float *__restrict__ ghat, int F, int T, long PL, float scale,
                                                                  int accumulate) {
    const long k = (long)blockIdx.x * IM_BLOCK + threadIdx.x;
    if (k >= PL) return;
    float ar[IM_TMAX], ai[IM_TMAX];
#pragma unroll
    for (int t = 0; t < IM_TMAX; ++t) ar[t] = ai[t] = 0.f;
    for (int f = 0; f < F; ++f) {
        const float *const gf = g + (size_t)f * T * 2 * PL + k;
        const float yr = yhat[(size_t)(2 * f) * PL + k], yi = yhat[(size_t)(2 * f + 1) * PL + k];
#pragma unroll
        for (int t = 0; t < IM_TMAX; ++t) {
            if (t >= T) break;
            const float gr = gf[(size_t)(2 * t) * PL], gi = gf[(size_t)(2 * t + 1) * PL];
            ar[t] += gr * yr + gi * yi;
            ai[t] += gr * yi - gi * yr;
        }
    }
#pragma unroll
    for (int t = 0; t < IM_TMAX; ++t) {
        if (t >= T) break;
        float *const o = ghat + (size_t)(2 * t) * PL + k;
        o[0] = accumulate ? o[0] + scale * ar[t] : scale * ar[t];
        o[PL] = accumulate ? o[PL] + scale * ai[t] : scale * ai[t];
    }
}

// ---- the detector: images are the padded planes [F][NAP][NBP] of the transforms; detector pixel (ta, tb) sums the cube pixels
// [ta d, ta d + d) x [tb d, tb d + d); rows and columns beyond (Na / d) d, (Nb / d) d are not observed.  One row of detector pixels
// per block row, lanes along beta: a wavefront reads and writes whole contiguous lines.
__global__ __launch_bounds__(IM_BLOCK) void imager_sample_kernel(const float *__restrict__ z, float *__restrict__ y, int d, int nao,
                                                                 int nbo, long NBP, long PLc) {
    const int tb = blockIdx.x * IM_BLOCK + threadIdx.x, ta = blockIdx.y, f = blockIdx.z;
    if (tb >= nbo) return;
    const float *const src = z + (size_t)f * PLc + (size_t)ta * d * NBP + (size_t)tb * d;
    float s = 0.f;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) s += src[(size_t)i * NBP + j];
    y[((size_t)f * nao + ta) * nbo + tb] = s;
}

// its transpose: every observed cube pixel receives its detector pixel's value, the others 0 (rows a < Na, columns b < Nb)
__global__ __launch_bounds__(IM_BLOCK) void imager_spread_kernel(const float *__restrict__ y, float *__restrict__ z, int d, int nao,
                                                                 int nbo, int Nb, long NBP, long PLc) {
    const int b = blockIdx.x * IM_BLOCK + threadIdx.x, a = blockIdx.y, f = blockIdx.z;
    if (b >= Nb) return;
    const int ta = a / d, tb = b / d;
    z[(size_t)f * PLc + (size_t)a * NBP + b] = (ta < nao && tb < nbo) ? y[((size_t)f * nao + ta) * nbo + tb] : 0.f;
}

// sample, weight and spread in one pass, in place: every d x d tile becomes w * (its sum), unobserved pixels 0.  A thread owns a
// tile (its sum is formed in one fixed order before any of its pixels is written); block row nao clears the rows nobody observes.
__global__ __launch_bounds__(IM_BLOCK) void imager_window_kernel(float *__restrict__ z, const float *__restrict__ w, int d, int nao,
                                                                 int nbo, int Na, int Nb, long NBP, long PLc) {
    const int tb = blockIdx.x * IM_BLOCK + threadIdx.x, ta = blockIdx.y, f = blockIdx.z;
    float *const pl = z + (size_t)f * PLc;
    if (ta == nao) {                                         // rows [nao d, Na), every column
        for (int a = nao * d; a < Na; ++a)
            for (int b = tb; b < Nb; b += gridDim.x * IM_BLOCK) pl[(size_t)a * NBP + b] = 0.f;
        return;
    }
    float *const rows = pl + (size_t)ta * d * NBP;
    if (tb < nbo) {
        float *const t = rows + (size_t)tb * d;
        float s = 0.f;
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) s += t[(size_t)i * NBP + j];
        if (w) {
            const float wv = w[((size_t)f * nao + ta) * nbo + tb];
            s = wv > 0.f ? wv * s : 0.f;
        }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) t[(size_t)i * NBP + j] = s;
    } else {
        const int b = nbo * d + (tb - nbo);                  // the columns nobody observes: one thread each
        if (b < Nb)
            for (int i = 0; i < d; ++i) rows[(size_t)i * NBP + b] = 0.f;
    }
}

// out[t][a][b] (+)= pad[t][a][b]: the maps out of the padded planes, added to what the spectrometer's operator left
__global__ __launch_bounds__(IM_BLOCK) void imager_unpad_kernel(const float *__restrict__ pad, float *__restrict__ out, int Nb, long NBP,
                                                                long PLc, int Na, int accumulate) {
    const int b = blockIdx.x * IM_BLOCK + threadIdx.x, a = blockIdx.y, t = blockIdx.z;
    if (b >= Nb) return;
    const float v = pad[(size_t)t * PLc + (size_t)a * NBP + b];
    float *const o = out + ((size_t)t * Na + a) * Nb + b;
    *o = accumulate ? *o + v : v;
}

inline int launched() { return (int)hipGetLastError(); }
inline unsigned blocks(long n) { return (unsigned)((n + IM_BLOCK - 1) / IM_BLOCK); }

}  // namespace

int launch_imager_build_g(hipStream_t s, const float *sotf, long sk, long sl, long im_off, const float *tpl, long ldt, const double *wf,
                          long ldw, int L, double *acc, int F, int T, int Na, int nkb, long KBP, long PL) {
    if (T < 1 || T > IM_TMAX || F < 1 || L < 0 || L % 64) return (int)hipErrorInvalidValue;
    const long nbin = (long)Na * nkb;
    hipLaunchKernelGGL(imager_build_g_kernel, dim3((unsigned)((nbin + IM_BLOCK / 64 - 1) / (IM_BLOCK / 64)), F), dim3(IM_BLOCK), 0, s, sotf,
                       sk, sl, im_off, tpl, ldt, wf, ldw, L, acc, T, Na, nkb, KBP, PL);
    return launched();
}
int launch_imager_g_store(hipStream_t s, const double *acc, float *g, long n) {
    hipLaunchKernelGGL(imager_g_store_kernel, dim3(blocks(n)), dim3(IM_BLOCK), 0, s, acc, g, n);
    return launched();
}
int launch_imager_otf_chunk(hipStream_t s, const float *src, float *dst, int n, int CH, int Na, int nkb, long KBP, long PL) {
    if (n < 1 || n > CH || CH % 32) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(imager_otf_chunk_kernel, dim3((unsigned)(((long)Na * nkb + 31) / 32), CH / 32), dim3(IM_BLOCK), 0, s,
                       (const float2 *)src, dst, n, CH, Na, nkb, KBP, PL);
    return launched();
}
int launch_imager_mix_fwd(hipStream_t s, const float *g, const float *xhat, float *zhat, int F, int T, long PL) {
    if (T < 1 || T > IM_TMAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(imager_mix_fwd_kernel, dim3(blocks(PL)), dim3(IM_BLOCK), 0, s, g, xhat, zhat, F, T, PL);
    return launched();
}
int launch_imager_mix_adj(hipStream_t s, const float *g, const float *yhat, float *ghat, int F, int T, long PL, float scale, int accumulate) {
    if (T < 1 || T > IM_TMAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(imager_mix_adj_kernel, dim3(blocks(PL)), dim3(IM_BLOCK), 0, s, g, yhat, ghat, F, T, PL, scale, accumulate);
    return launched();
}
int launch_imager_sample(hipStream_t s, const float *z, float *y, int F, int d, int Na, int Nb, long NBP, long PLc) {
    const int nao = Na / d, nbo = Nb / d;
    hipLaunchKernelGGL(imager_sample_kernel, dim3(blocks(nbo), nao, F), dim3(IM_BLOCK), 0, s, z, y, d, nao, nbo, NBP, PLc);
    return launched();
}
int launch_imager_spread(hipStream_t s, const float *y, float *z, int F, int d, int Na, int Nb, long NBP, long PLc) {
    hipLaunchKernelGGL(imager_spread_kernel, dim3(blocks(Nb), Na, F), dim3(IM_BLOCK), 0, s, y, z, d, Na / d, Nb / d, Nb, NBP, PLc);
    return launched();
}
int launch_imager_window(hipStream_t s, float *z, const float *w, int F, int d, int Na, int Nb, long NBP, long PLc) {
    const int nao = Na / d, nbo = Nb / d;
    // a thread per tile of a row of tiles, then one per unobserved column; the extra block row clears the unobserved rows
    hipLaunchKernelGGL(imager_window_kernel, dim3(blocks(nbo + (Nb - nbo * d)), nao + 1, F), dim3(IM_BLOCK), 0, s, z, w, d, nao, nbo, Na, Nb,
                       NBP, PLc);
    return launched();
}
int launch_imager_unpad(hipStream_t s, const float *pad, float *out, int T, int Na, int Nb, long NBP, long PLc, int accumulate) {
    hipLaunchKernelGGL(imager_unpad_kernel, dim3(blocks(Nb), Na, T), dim3(IM_BLOCK), 0, s, pad, out, Nb, NBP, PLc, Na, accumulate);
    return launched();
}
