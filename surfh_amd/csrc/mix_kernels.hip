// Spectral mix x OTF, the WCT Hessian with its closed-form solve, and the linear mixing model (see kernels.h for the contracts).
#include "kernels.h"
#include "prior_eig.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == RED_TPB, "the shared reductions of reduce_dev.h assume this block size");
static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");

// ---------------------------------------------------------------------------------------------
// spectral mix x OTF   (wavelength innermost; spectra are planar [2][PL][LP], or with `ilv` interleaved
// [PL][LP][2] -- the layout of the plans whose transforms run in dft_h2.hip)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void cld4(const float *__restrict__ a, long PL, long k, int LP, int l4, int ilv, float4 &re, float4 &im) {
    if (ilv) {
        const float4 v0 = *reinterpret_cast<const float4 *>(a + (k * LP + l4) * 2);
        const float4 v1 = *reinterpret_cast<const float4 *>(a + (k * LP + l4) * 2 + 4);
        re = make_float4(v0.x, v0.z, v1.x, v1.z);
        im = make_float4(v0.y, v0.w, v1.y, v1.w);
    } else {
        re = *reinterpret_cast<const float4 *>(a + k * LP + l4);
        im = *reinterpret_cast<const float4 *>(a + (PL + k) * LP + l4);
    }
}
__device__ __forceinline__ void cst4(float *__restrict__ a, long PL, long k, int LP, int l4, int ilv, const float4 &re, const float4 &im) {
    if (ilv) {
        *reinterpret_cast<float4 *>(a + (k * LP + l4) * 2) = make_float4(re.x, im.x, re.y, im.y);
        *reinterpret_cast<float4 *>(a + (k * LP + l4) * 2 + 4) = make_float4(re.z, im.z, re.w, im.w);
    } else {
        *reinterpret_cast<float4 *>(a + k * LP + l4) = re;
        *reinterpret_cast<float4 *>(a + (PL + k) * LP + l4) = im;
    }
}

__global__ __launch_bounds__(TPB) void specmix_fwd_kernel(const float *__restrict__ mhat,
                                                          const float *__restrict__ sotf,
                                                          const float *__restrict__ tpl, float *__restrict__ spec,
                                                          int T, long PL, int LP, int ilv) {
    const int l4 = (blockIdx.x * TPB + threadIdx.x) * 4;
    if (l4 >= LP) return;
    const long k = blockIdx.y;
    float4 sr = make_float4(0.f, 0.f, 0.f, 0.f), si = sr;
    if (T > 0) {
        for (int t = 0; t < T; ++t) {
            const float4 w = *reinterpret_cast<const float4 *>(tpl + (long)t * LP + l4);
            const float mr = mhat[((long)t * 2 + 0) * PL + k];
            const float mi = mhat[((long)t * 2 + 1) * PL + k];
            sr.x += w.x * mr; sr.y += w.y * mr; sr.z += w.z * mr; sr.w += w.w * mr;
            si.x += w.x * mi; si.y += w.y * mi; si.z += w.z * mi; si.w += w.w * mi;
        }
    } else {
        cld4(mhat, PL, k, LP, l4, ilv, sr, si);
    }
    float4 hr, hi;
    cld4(sotf, PL, k, LP, l4, ilv, hr, hi);
    float4 xr, xi;
    xr.x = hr.x * sr.x - hi.x * si.x; xi.x = hr.x * si.x + hi.x * sr.x;
    xr.y = hr.y * sr.y - hi.y * si.y; xi.y = hr.y * si.y + hi.y * sr.y;
    xr.z = hr.z * sr.z - hi.z * si.z; xi.z = hr.z * si.z + hi.z * sr.z;
    xr.w = hr.w * sr.w - hi.w * si.w; xi.w = hr.w * si.w + hi.w * sr.w;
    cst4(spec, PL, k, LP, l4, ilv, xr, xi);
}

constexpr int MAXT = SURFH_MAX_TEMPLATES;

// one workgroup per frequency bin k: madj[t][c][k] = sum_l tpl[t][l] (conj(H) Y)[c][k][l]
template <typename ACC>
__global__ __launch_bounds__(TPB) void specmix_adj_kernel(const float *__restrict__ spec,
                                                          const float *__restrict__ sotf,
                                                          const float *__restrict__ tpl, float *__restrict__ madj,
                                                          int T, long PL, int LP, int ilv) {
    const long k = blockIdx.x;
    ACC ar[MAXT], ai[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) ar[t] = ai[t] = (ACC)0;
    for (int l4 = threadIdx.x * 4; l4 < LP; l4 += TPB * 4) {
        float4 hr, hi, yr, yi;
        cld4(sotf, PL, k, LP, l4, ilv, hr, hi);
        cld4(spec, PL, k, LP, l4, ilv, yr, yi);
        float4 pr, pi;
        pr.x = hr.x * yr.x + hi.x * yi.x; pi.x = hr.x * yi.x - hi.x * yr.x;
        pr.y = hr.y * yr.y + hi.y * yi.y; pi.y = hr.y * yi.y - hi.y * yr.y;
        pr.z = hr.z * yr.z + hi.z * yi.z; pi.z = hr.z * yi.z - hi.z * yr.z;
        pr.w = hr.w * yr.w + hi.w * yi.w; pi.w = hr.w * yi.w - hi.w * yr.w;
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
            if (t < T) {
                const float4 w = *reinterpret_cast<const float4 *>(tpl + (long)t * LP + l4);
                ar[t] += (ACC)w.x * (ACC)pr.x + (ACC)w.y * (ACC)pr.y + (ACC)w.z * (ACC)pr.z + (ACC)w.w * (ACC)pr.w;
                ai[t] += (ACC)w.x * (ACC)pi.x + (ACC)w.y * (ACC)pi.y + (ACC)w.z * (ACC)pi.z + (ACC)w.w * (ACC)pi.w;
            }
    }
    __shared__ ACC red[TPB / 64][2 * MAXT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        ACC a = ar[t], b = ai[t];
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_down(a, o, 64);
            b += __shfl_down(b, o, 64);
        }
        if (lane == 0) {
            red[wv][2 * t] = a;
            red[wv][2 * t + 1] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * T) {
        ACC s = (ACC)0;
        for (int w = 0; w < TPB / 64; ++w) s += red[w][threadIdx.x];
        const int t = threadIdx.x >> 1, c = threadIdx.x & 1;
        madj[((long)t * 2 + c) * PL + k] = (float)s;
    }
}

// no-LMM adjoint: out[c][k][l] = (conj(H) Y)[c][k][l]
__global__ __launch_bounds__(TPB) void specmix_adj_plane_kernel(const float *__restrict__ spec,
                                                                const float *__restrict__ sotf,
                                                                float *__restrict__ out, long PL, int LP, int ilv) {
    const int l4 = (blockIdx.x * TPB + threadIdx.x) * 4;
    if (l4 >= LP) return;
    const long k = blockIdx.y;
    float4 hr, hi, yr, yi;
    cld4(sotf, PL, k, LP, l4, ilv, hr, hi);
    cld4(spec, PL, k, LP, l4, ilv, yr, yi);
    float4 pr, pi;
    pr.x = hr.x * yr.x + hi.x * yi.x; pi.x = hr.x * yi.x - hi.x * yr.x;
    pr.y = hr.y * yr.y + hi.y * yi.y; pi.y = hr.y * yi.y - hi.y * yr.y;
    pr.z = hr.z * yr.z + hi.z * yi.z; pi.z = hr.z * yi.z - hi.z * yr.z;
    pr.w = hr.w * yr.w + hi.w * yi.w; pi.w = hr.w * yi.w - hi.w * yr.w;
    cst4(out, PL, k, LP, l4, ilv, pr, pi);
}

// ---- the same three operations on interleaved spectra [PL][LP][2]: a thread handles two complex values = one
// float4 of each array, so every wave instruction reads whole contiguous lines -------------------------------------
__global__ __launch_bounds__(TPB) void specmix_fwd_ilv_kernel(const float *__restrict__ mhat, const float *__restrict__ sotf,
                                                              const float *__restrict__ tpl, float *__restrict__ spec,
                                                              int T, long PL, int LP) {
    const int l2 = (blockIdx.x * TPB + threadIdx.x) * 2;
    if (l2 >= LP) return;
    const long k = blockIdx.y;
    float sr0 = 0.f, si0 = 0.f, sr1 = 0.f, si1 = 0.f;
    if (T > 0) {
        for (int t = 0; t < T; ++t) {
            const float2 w = *reinterpret_cast<const float2 *>(tpl + (long)t * LP + l2);
            const float mr = mhat[((long)t * 2 + 0) * PL + k];
            const float mi = mhat[((long)t * 2 + 1) * PL + k];
            sr0 += w.x * mr; si0 += w.x * mi; sr1 += w.y * mr; si1 += w.y * mi;
        }
    } else {
        const float4 m = *reinterpret_cast<const float4 *>(mhat + (k * LP + l2) * 2);
        sr0 = m.x; si0 = m.y; sr1 = m.z; si1 = m.w;
    }
    const float4 hh = *reinterpret_cast<const float4 *>(sotf + (k * LP + l2) * 2);
    *reinterpret_cast<float4 *>(spec + (k * LP + l2) * 2) =
        make_float4(hh.x * sr0 - hh.y * si0, hh.x * si0 + hh.y * sr0, hh.z * sr1 - hh.w * si1, hh.z * si1 + hh.w * sr1);
}
}  // namespace

int launch_specmix_fwd(hipStream_t s, const float *mhat, const float *sotf, const float *tpl, float *spec, int T,
                       long PL, int LP, int ilv) {
    if (T > MAXT) return (int)hipErrorInvalidValue;
    if (ilv) {
        dim3 grid((LP / 2 + TPB - 1) / TPB, (unsigned)PL);
        hipLaunchKernelGGL(specmix_fwd_ilv_kernel, grid, dim3(TPB), 0, s, mhat, sotf, tpl, spec, T, PL, LP);
        return (int)hipGetLastError();
    }
    dim3 grid((LP / 4 + TPB - 1) / TPB, (unsigned)PL);
    hipLaunchKernelGGL(specmix_fwd_kernel, grid, dim3(TPB), 0, s, mhat, sotf, tpl, spec, T, PL, LP, 0);
    return (int)hipGetLastError();
}

namespace {
template <typename ACC>
__global__ __launch_bounds__(TPB) void specmix_adj_ilv_kernel(const float *__restrict__ spec, const float *__restrict__ sotf,
                                                              const float *__restrict__ tpl, float *__restrict__ madj,
                                                              int T, long PL, int LP, SpecmixAdjOpt o) {
    const long k = blockIdx.x;
    ACC ar[MAXT], ai[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) ar[t] = ai[t] = (ACC)0;
    const float *hk = sotf + k * LP * 2, *yk = spec + k * LP * 2;
    // support of the OTF (plan.hip otf_support): chunk c of 128 wavelengths holds nothing at k_beta > lim[c] or at a folded
    // k_alpha > lim[LP / 128 + c]; `spec` was not written there
    const int ka = o.KBP ? (int)(k / o.KBP) : 0, kb = o.KBP ? (int)(k % o.KBP) : 0;
    const int af = ka < o.Na - ka ? ka : o.Na - ka, nch = LP >> 7;
    for (int l0 = threadIdx.x * 2; l0 < LP; l0 += TPB * 4) {      // two float4 of each array in flight per thread
        const int l1 = l0 + TPB * 2;
        // outside the support the loads are redirected to the bin's first wavelengths (cached lines, finite values) and weighted
        // by zero: no branch around a load, no traffic for the skipped chunk
        const bool one = !o.lim || (kb <= o.lim[l0 >> 7] && af <= o.lim[nch + (l0 >> 7)]);
        const bool two = l1 < LP && (!o.lim || (kb <= o.lim[l1 >> 7] && af <= o.lim[nch + (l1 >> 7)]));
        const int e0 = one ? l0 : (int)threadIdx.x % 64 * 2, e1 = two ? l1 : (int)threadIdx.x % 64 * 2;
        const float4 ha = *reinterpret_cast<const float4 *>(hk + (long)e0 * 2);
        const float4 ya = *reinterpret_cast<const float4 *>(yk + (long)e0 * 2);
        const float4 hb = *reinterpret_cast<const float4 *>(hk + (long)e1 * 2);
        const float4 yb = *reinterpret_cast<const float4 *>(yk + (long)e1 * 2);
        const float pr0 = ha.x * ya.x + ha.y * ya.y, pi0 = ha.x * ya.y - ha.y * ya.x;
        const float pr1 = ha.z * ya.z + ha.w * ya.w, pi1 = ha.z * ya.w - ha.w * ya.z;
        const float pr2 = hb.x * yb.x + hb.y * yb.y, pi2 = hb.x * yb.y - hb.y * yb.x;
        const float pr3 = hb.z * yb.z + hb.w * yb.w, pi3 = hb.z * yb.w - hb.w * yb.z;
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
            if (t < T) {
                const float2 wa = one ? *reinterpret_cast<const float2 *>(tpl + (long)t * LP + l0) : make_float2(0.f, 0.f);
                const float2 wb = two ? *reinterpret_cast<const float2 *>(tpl + (long)t * LP + l1) : make_float2(0.f, 0.f);
                ar[t] += (ACC)wa.x * (ACC)pr0 + (ACC)wa.y * (ACC)pr1 + (ACC)wb.x * (ACC)pr2 + (ACC)wb.y * (ACC)pr3;
                ai[t] += (ACC)wa.x * (ACC)pi0 + (ACC)wa.y * (ACC)pi1 + (ACC)wb.x * (ACC)pi2 + (ACC)wb.y * (ACC)pi3;
            }
    }
    __shared__ ACC red[TPB / 64][2 * MAXT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        ACC a = ar[t], b = ai[t];
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_down(a, o, 64);
            b += __shfl_down(b, o, 64);
        }
        if (lane == 0) {
            red[wv][2 * t] = a;
            red[wv][2 * t + 1] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * T) {
        ACC s = (ACC)0;
        for (int w = 0; w < TPB / 64; ++w) s += red[w][threadIdx.x];
        const int t = threadIdx.x >> 1, c = threadIdx.x & 1;
        const long oo = ((long)t * 2 + c) * PL + k;
        float v = (float)s;
        if (o.Nb) {     // the solver's Parseval-scaled half spectrum, mu and the quadratic prior folded in (dft_h2.h DftH2AdjMix)
            v *= (kb == 0 || 2 * kb == o.Nb) ? o.out_self : o.out_pair;
            if (o.prior_src && ka < o.Na && 2 * kb <= o.Nb)
                v += o.prior_mu * (dsq(kb, o.Nb) + dsq(ka, o.Na)) * o.prior_src[oo];
        }
        madj[oo] = v;
    }
}

// `out` may hold, on entry, the spectrum of the vector the normal operator was applied to (the forward model left it there): with
// prior_w != 0 the quadratic prior is added in the same pass, out = mu conj(H) Y + prior_w |D(k)|^2 out_old (circular first
// differences are diagonal in the Fourier domain: |D|^2 = dsq(ka, Na) + dsq(kb, Nb), prior_eig.h)
__global__ __launch_bounds__(TPB) void specmix_adj_plane_ilv_kernel(const float *__restrict__ spec, const float *__restrict__ sotf,
                                                                    float *out, long PL, int LP, float mu, float prior_w, int Na, int Nb, long KBP) {
    const int l2 = (blockIdx.x * TPB + threadIdx.x) * 2;
    if (l2 >= LP) return;
    const long k = blockIdx.y;
    const float4 hh = *reinterpret_cast<const float4 *>(sotf + (k * LP + l2) * 2);
    const float4 y = *reinterpret_cast<const float4 *>(spec + (k * LP + l2) * 2);
    float4 v = make_float4(hh.x * y.x + hh.y * y.y, hh.x * y.y - hh.y * y.x, hh.z * y.z + hh.w * y.w, hh.z * y.w - hh.w * y.z);
    if (prior_w != 0.f) {
        const int ka = (int)(k / KBP), kb = (int)(k % KBP);
        const float w = prior_w * (dsq(ka, Na) + dsq(kb, Nb));
        const float4 o = *reinterpret_cast<const float4 *>(out + (k * LP + l2) * 2);
        v = make_float4(mu * v.x + w * o.x, mu * v.y + w * o.y, mu * v.z + w * o.z, mu * v.w + w * o.w);
    }
    *reinterpret_cast<float4 *>(out + (k * LP + l2) * 2) = v;
}
}  // namespace

int launch_specmix_adj(hipStream_t s, const float *spec, const float *sotf, const float *tpl, float *madj, int T,
                       long PL, int LP, bool f64, int ilv, const SpecmixAdjOpt *opt) {
    if (T > MAXT) return (int)hipErrorInvalidValue;
    const SpecmixAdjOpt o = opt ? *opt : SpecmixAdjOpt();
    if (opt && T == 0 && (!ilv || o.lim || (o.prior_src && (o.prior_src != madj || o.KBP < 1 || o.Na < 1 || o.Nb < 1)))) return (int)hipErrorInvalidValue;
    if (opt && T != 0 && (!ilv || (o.lim && LP % 128) || ((o.lim || o.Nb) && (o.KBP < 1 || o.Na < 1)))) return (int)hipErrorInvalidValue;
    if (ilv) {
        if (T == 0) {
            dim3 grid((LP / 2 + TPB - 1) / TPB, (unsigned)PL);
            hipLaunchKernelGGL(specmix_adj_plane_ilv_kernel, grid, dim3(TPB), 0, s, spec, sotf, madj, PL, LP, o.out_self, o.prior_src ? o.prior_mu : 0.f,
                               o.Na, o.Nb, o.KBP);
        } else if (f64) hipLaunchKernelGGL(specmix_adj_ilv_kernel<double>, dim3((unsigned)PL), dim3(TPB), 0, s, spec, sotf, tpl, madj, T, PL, LP, o);
        else hipLaunchKernelGGL(specmix_adj_ilv_kernel<float>, dim3((unsigned)PL), dim3(TPB), 0, s, spec, sotf, tpl, madj, T, PL, LP, o);
        return (int)hipGetLastError();
    }
    if (T == 0) {
        dim3 grid((LP / 4 + TPB - 1) / TPB, (unsigned)PL);
        hipLaunchKernelGGL(specmix_adj_plane_kernel, grid, dim3(TPB), 0, s, spec, sotf, madj, PL, LP, 0);
    } else {
        if (f64) hipLaunchKernelGGL(specmix_adj_kernel<double>, dim3((unsigned)PL), dim3(TPB), 0, s, spec, sotf, tpl, madj, T, PL, LP, 0);
        else hipLaunchKernelGGL(specmix_adj_kernel<float>, dim3((unsigned)PL), dim3(TPB), 0, s, spec, sotf, tpl, madj, T, PL, LP, 0);
    }
    return (int)hipGetLastError();
}

namespace {
// one workgroup per frequency bin: the T x T Hessian block sum_l tpl tpl' |H|^2
__global__ __launch_bounds__(TPB) void wct_hessian_kernel(const float *__restrict__ sotf, const float *__restrict__ tpl,
                                                          float *__restrict__ hth, int T, long PL, int LP, int ilv) {
    const long k = blockIdx.x;
    float acc[MAXT * (MAXT + 1) / 2];
#pragma unroll
    for (int i = 0; i < MAXT * (MAXT + 1) / 2; ++i) acc[i] = 0.f;
    for (int l = threadIdx.x; l < LP; l += TPB) {
        const float hr = ilv ? sotf[(k * LP + l) * 2] : sotf[k * LP + l], hi = ilv ? sotf[(k * LP + l) * 2 + 1] : sotf[(PL + k) * LP + l];
        const float h2 = hr * hr + hi * hi;
        float w[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t) w[t] = (t < T) ? tpl[(long)t * LP + l] : 0.f;
        int i = 0;
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
#pragma unroll
            for (int u = t; u < MAXT; ++u, ++i) acc[i] += w[t] * w[u] * h2;
    }
    __shared__ float red[TPB / 64][MAXT * (MAXT + 1) / 2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < MAXT * (MAXT + 1) / 2; ++i) {
        float a = acc[i];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) red[wv][i] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int i = 0;
        for (int t = 0; t < MAXT; ++t)
            for (int u = t; u < MAXT; ++u, ++i) {
                if (u >= T) continue;
                float s = 0.f;
                for (int w = 0; w < TPB / 64; ++w) s += red[w][i];
                hth[((long)t * T + u) * PL + k] = s;
                hth[((long)u * T + t) * PL + k] = s;
            }
    }
}
}  // namespace

int launch_wct_hessian(hipStream_t s, const float *sotf, const float *tpl, float *hth, int T, long PL, int LP, int ilv) {
    if (T < 1 || T > MAXT) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(wct_hessian_kernel, dim3((unsigned)PL), dim3(TPB), 0, s, sotf, tpl, hth, T, PL, LP, ilv);
    return (int)hipGetLastError();
}

namespace {
__global__ __launch_bounds__(TPB) void wct_hess_apply_kernel(const float *__restrict__ hth, const float *__restrict__ in,
                                                             float *__restrict__ out, int T, long PL) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= PL) return;
    for (int t = 0; t < T; ++t) {
        float sr = 0.f, si = 0.f;
        for (int u = 0; u < T; ++u) {
            const float h = hth[((long)t * T + u) * PL + k];
            sr += h * in[((long)u * 2 + 0) * PL + k];
            si += h * in[((long)u * 2 + 1) * PL + k];
        }
        out[((long)t * 2 + 0) * PL + k] = sr;
        out[((long)t * 2 + 1) * PL + k] = si;
    }
}
}  // namespace

int launch_wct_hess_apply(hipStream_t s, const float *hth, const float *in, float *out, int T, long PL) {
    hipLaunchKernelGGL(wct_hess_apply_kernel, dim3((unsigned)((PL + TPB - 1) / TPB)), dim3(TPB), 0, s, hth, in, out, T, PL);
    return (int)hipGetLastError();
}

namespace {
// explicit inverse of the regularised normal operator, one thread per frequency bin: solves
// (HtH(f) + diag(mu_t reg(f))) z = b(f) for the real and the imaginary part of b (HtH is real symmetric for
// di = dj = 1).  T <= 8 unknowns, Cholesky in fp64 registers; a vanishing pivot raises `flag`.
__global__ __launch_bounds__(TPB) void wct_solve_kernel(const float *__restrict__ hth, const float *__restrict__ reg,
                                                        const double *__restrict__ mu, const float *__restrict__ in,
                                                        float *__restrict__ out, int T, long PL, int *flag) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= PL) return;
    const float rg = reg[k];
    if (rg < 0.f) {                     // padding bin of the spectral layout
        for (int t = 0; t < T; ++t) out[((long)t * 2 + 0) * PL + k] = out[((long)t * 2 + 1) * PL + k] = 0.f;
        return;
    }
    double A[MAXT][MAXT], br[MAXT], bi[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
#pragma unroll
        for (int u = 0; u < MAXT; ++u) A[t][u] = (t < T && u < T) ? (double)hth[((long)t * T + u) * PL + k] : (t == u ? 1.0 : 0.0);
        if (t < T) {
            A[t][t] += mu[t] * (double)rg;
            br[t] = in[((long)t * 2 + 0) * PL + k];
            bi[t] = in[((long)t * 2 + 1) * PL + k];
        } else {
            br[t] = bi[t] = 0.0;
        }
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {    // A = L L^T in place (lower triangle), forward substitution on the fly
        const double ajj = A[j][j];
        double d = ajj;
#pragma unroll
        for (int q = 0; q < MAXT; ++q)
            if (q < j) d -= A[j][q] * A[j][q];
        // HtH reaches this kernel in fp32: a pivot below 1e-6 of its diagonal entry is rounding noise, the matrix is singular
        if (!(d > 1e-6 * ajj)) { bad = true; d = 1.0; }
        const double l = sqrt(d), il = 1.0 / l;
        A[j][j] = l;
#pragma unroll
        for (int i = 0; i < MAXT; ++i)
            if (i > j) {
                double v = A[i][j];
#pragma unroll
                for (int q = 0; q < MAXT; ++q)
                    if (q < j) v -= A[i][q] * A[j][q];
                A[i][j] = v * il;
            }
        double vr = br[j], vi = bi[j];
#pragma unroll
        for (int q = 0; q < MAXT; ++q)
            if (q < j) { vr -= A[j][q] * br[q]; vi -= A[j][q] * bi[q]; }
        br[j] = vr * il;
        bi[j] = vi * il;
    }
#pragma unroll
    for (int j = MAXT - 1; j >= 0; --j) {   // back substitution with L^T
        double vr = br[j], vi = bi[j];
#pragma unroll
        for (int q = 0; q < MAXT; ++q)
            if (q > j) { vr -= A[q][j] * br[q]; vi -= A[q][j] * bi[q]; }
        br[j] = vr / A[j][j];
        bi[j] = vi / A[j][j];
    }
    if (bad) atomicOr(flag, 1);
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
        if (t < T) {
            out[((long)t * 2 + 0) * PL + k] = (float)br[t];
            out[((long)t * 2 + 1) * PL + k] = (float)bi[t];
        }
}
}  // namespace

int launch_wct_solve(hipStream_t s, const float *hth, const float *reg, const double *mu, const float *in, float *out, int T,
                     long PL, int *flag) {
    hipLaunchKernelGGL(wct_solve_kernel, dim3((unsigned)((PL + TPB - 1) / TPB)), dim3(TPB), 0, s, hth, reg, mu, in, out, T, PL, flag);
    return (int)hipGetLastError();
}

namespace {
// ---------------------------------------------------------------------------------------------
// linear mixing model on plane-major arrays (driver utilities, not on the iteration path)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void lmm_maps2cube_kernel(const float *__restrict__ maps, const float *__restrict__ tpl,
                                                            float *__restrict__ cube, int T, int L, long npix) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    const int l = blockIdx.y;
    if (i >= npix) return;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += tpl[(long)t * L + l] * maps[(long)t * npix + i];
    cube[(long)l * npix + i] = acc;
}

// one thread per pixel walks the planes; T <= 8 running sums in registers, every plane read is coalesced
__global__ __launch_bounds__(TPB) void lmm_cube2maps_kernel(const float *__restrict__ cube, const float *__restrict__ tpl,
                                                            float *__restrict__ maps, int T, int L, long npix) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    for (int t0 = 0; t0 < T; t0 += 8) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < L; ++l) {
            const float v = cube[(long)l * npix + i];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t0 + t < T) acc[t] += tpl[(long)(t0 + t) * L + l] * v;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (t0 + t < T) maps[(long)(t0 + t) * npix + i] = acc[t];
    }
}
}  // namespace

int launch_lmm_maps2cube(hipStream_t s, const float *maps, const float *tpl, float *cube, int T, int L, long npix) {
    dim3 grid((unsigned)((npix + TPB - 1) / TPB), (unsigned)L);
    hipLaunchKernelGGL(lmm_maps2cube_kernel, grid, dim3(TPB), 0, s, maps, tpl, cube, T, L, npix);
    return (int)hipGetLastError();
}

int launch_lmm_cube2maps(hipStream_t s, const float *cube, const float *tpl, float *maps, int T, int L, long npix) {
    hipLaunchKernelGGL(lmm_cube2maps_kernel, dim3((unsigned)((npix + TPB - 1) / TPB)), dim3(TPB), 0, s, cube, tpl, maps, T, L, npix);
    return (int)hipGetLastError();
}
