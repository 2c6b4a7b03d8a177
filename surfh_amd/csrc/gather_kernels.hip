// Sparse gather and scatter with their fp16 quantisation, the layout helpers between the GEMM operands and the detector, and the
// data weights (see kernels.h for the contracts).
#include "kernels.h"
#include "f16_split.h"
#include "reduce_dev.h"
#include <algorithm>
#include <cfloat>

namespace {

constexpr int TPB = 256;
static_assert(TPB == RED_TPB, "the shared reductions of reduce_dev.h assume this block size");
static_assert(TPB == VEC_TPB, "kernels.h states the block size of the capped grids");

// ---------------------------------------------------------------------------------------------
// sparse row gather vectorised over wavelength: one workgroup = one table row x 1024 wavelengths
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(TPB) void spmm_rows_kernel(EllTable t, const float *__restrict__ src,
                                                        float *__restrict__ dst, int nlam, int accumulate) {
    // workgroups are dealt round-robin over the 8 XCDs (each with its own L2): give every XCD one
    // contiguous band of table rows, so neighbouring rows -- which share most of their taps -- hit the same L2
    const int per = (t.R + 7) / 8;
    const int r = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    const int l4 = (blockIdx.y * TPB + threadIdx.x) * 4;
    if (r >= t.R) return;                                 // workgroup-uniform
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l4 < nlam) {
        const int n = t.cnt[r];
        const int64_t *col = t.col + (long)r * t.W;
        const float *val = t.val + (long)r * t.W;
        int e = 0;
        for (; e + 4 <= n; e += 4) {
            const float4 x0 = *reinterpret_cast<const float4 *>(src + col[e] + l4);
            const float4 x1 = *reinterpret_cast<const float4 *>(src + col[e + 1] + l4);
            const float4 x2 = *reinterpret_cast<const float4 *>(src + col[e + 2] + l4);
            const float4 x3 = *reinterpret_cast<const float4 *>(src + col[e + 3] + l4);
            const float v0 = val[e], v1 = val[e + 1], v2 = val[e + 2], v3 = val[e + 3];
            acc.x += v0 * x0.x; acc.y += v0 * x0.y; acc.z += v0 * x0.z; acc.w += v0 * x0.w;
            acc.x += v1 * x1.x; acc.y += v1 * x1.y; acc.z += v1 * x1.z; acc.w += v1 * x1.w;
            acc.x += v2 * x2.x; acc.y += v2 * x2.y; acc.z += v2 * x2.z; acc.w += v2 * x2.w;
            acc.x += v3 * x3.x; acc.y += v3 * x3.y; acc.z += v3 * x3.z; acc.w += v3 * x3.w;
        }
        for (; e < n; ++e) {
            const float4 x0 = *reinterpret_cast<const float4 *>(src + col[e] + l4);
            const float v0 = val[e];
            acc.x += v0 * x0.x; acc.y += v0 * x0.y; acc.z += v0 * x0.z; acc.w += v0 * x0.w;
        }
        float4 *p = reinterpret_cast<float4 *>(dst + t.dst_off[r] + l4);
        bool rm = accumulate != 0;
        if (rm && t.rng) { const int2 g2 = t.rng[r]; rm = l4 >= g2.x && l4 < g2.y; }
        else if (rm && t.rmw) rm = ((t.rmw[r] >> blockIdx.y) & 1u) != 0;      // workgroup-uniform
        if (rm) {
            const float4 o = *p;
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
        *p = acc;
    }
}
}  // namespace

int launch_spmm_rows(hipStream_t s, const EllTable &t, const float *src, float *dst, int nlam, int accumulate) {
    if (t.R == 0 || nlam <= 0) return 0;
    if (nlam % 4) return (int)hipErrorInvalidValue;
    dim3 grid((t.R + 7) / 8 * 8, (nlam / 4 + TPB - 1) / TPB);
    hipLaunchKernelGGL(spmm_rows_kernel, grid, dim3(TPB), 0, s, t, src, dst, nlam, accumulate);
    return (int)hipGetLastError();
}

namespace {
// verification twin of spmm_rows_kernel: the same rows with float64 accumulation (surfh_config.verify)
__global__ __launch_bounds__(TPB) void spmm_rows_f64acc_kernel(EllTable t, const float *__restrict__ src, float *__restrict__ dst, int nlam,
                                                               int accumulate) {
    const int r = blockIdx.x;
    const int l = blockIdx.y * TPB + threadIdx.x;
    if (r >= t.R || l >= nlam) return;
    const int n = t.cnt[r];
    const int64_t *col = t.col + (long)r * t.W;
    const float *val = t.val + (long)r * t.W;
    double acc = 0.0;
    for (int e = 0; e < n; ++e) acc += (double)val[e] * (double)src[col[e] + l];
    float *p = dst + t.dst_off[r] + l;
    *p = (float)(accumulate ? (double)*p + acc : acc);
}
}  // namespace

int launch_spmm_rows_f64acc(hipStream_t s, const EllTable &t, const float *src, float *dst, int nlam, int accumulate) {
    if (t.R == 0 || nlam <= 0) return 0;
    dim3 grid((unsigned)t.R, (nlam + TPB - 1) / TPB);
    hipLaunchKernelGGL(spmm_rows_f64acc_kernel, grid, dim3(TPB), 0, s, t, src, dst, nlam, accumulate);
    return (int)hipGetLastError();
}

namespace {
// grouped scatter: one workgroup = SCATTER_G neighbouring cube pixels x 1024 wavelengths (see GroupTable)
template <int G>
__global__ __launch_bounds__(TPB) void spmm_group_scatter_kernel(GroupTable t, const float *__restrict__ src, float *__restrict__ dst,
                                                                 int nlam) {
    const int per = (t.NG + 7) / 8;
    const int gi = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    const int l4 = (blockIdx.y * TPB + threadIdx.x) * 4;
    if (gi >= t.NG || l4 >= nlam) return;
    const int n = t.cnt[gi];
    const int64_t *col = t.col + (long)gi * t.W;
    const float *val = t.val + (long)gi * t.W * G;
    float4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    int e = 0;
    constexpr int SCATTER_UNROLL = 8;      // taps in flight (groups of four: 2 ... 16 alike; groups of eight: 4 -> 8 taps 0.289 -> 0.277 ms per step)
    for (; e + SCATTER_UNROLL <= n; e += SCATTER_UNROLL) {
        float4 xv[SCATTER_UNROLL];
#pragma unroll
        for (int u = 0; u < SCATTER_UNROLL; ++u) xv[u] = *reinterpret_cast<const float4 *>(src + col[e + u] + l4);
#pragma unroll
        for (int u = 0; u < SCATTER_UNROLL; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float v0 = val[(e + u) * G + g];
                acc[g].x += v0 * xv[u].x; acc[g].y += v0 * xv[u].y; acc[g].z += v0 * xv[u].z; acc[g].w += v0 * xv[u].w;
            }
    }
    for (; e < n; ++e) {
        const float4 x0 = *reinterpret_cast<const float4 *>(src + col[e] + l4);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v0 = val[e * G + g];
            acc[g].x += v0 * x0.x; acc[g].y += v0 * x0.y; acc[g].z += v0 * x0.z; acc[g].w += v0 * x0.w;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t d = t.dst[(long)gi * G + g];
        if (d < 0) continue;                               // workgroup-uniform
        float4 *p = reinterpret_cast<float4 *>(dst + d + l4);
        float4 a = acc[g];
        bool rm;
        if (t.rng) { const int2 g2 = t.rng[(long)gi * G + g]; rm = l4 >= g2.x && l4 < g2.y; }
        else rm = ((t.rmw[(long)gi * G + g] >> blockIdx.y) & 1u) != 0;
        if (rm) {
            const float4 o = *p;
            a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
        }
        *p = a;
    }
}
}  // namespace

int launch_spmm_group_scatter(hipStream_t s, const GroupTable &t, const float *src, float *dst, int nlam) {
    if (t.NG == 0 || nlam <= 0) return 0;
    if (nlam % 4 || (nlam / 4 + TPB - 1) / TPB > 32) return (int)hipErrorInvalidValue;
    dim3 grid((t.NG + 7) / 8 * 8, (nlam / 4 + TPB - 1) / TPB);
    if (t.G == 4) hipLaunchKernelGGL(spmm_group_scatter_kernel<4>, grid, dim3(TPB), 0, s, t, src, dst, nlam);
    else if (t.G == 8) hipLaunchKernelGGL(spmm_group_scatter_kernel<8>, grid, dim3(TPB), 0, s, t, src, dst, nlam);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

namespace {
// The gather with its output written as the two fp16 pieces the all-consumer GEMM reads (gemm_cc16.hip).  The scale is
// per workgroup, i.e. per (operand row, segment of <= 1024 wavelengths of one beta column): the workgroup's maximum is known
// before anything is stored, so no second pass over the operand is needed, and the scale is finer than one per row.
// bscale[seg][NP] receives the power of two (f16x2_scale, f16_split.h); seg = (column offset / LinP) * nchunk + chunk.
__global__ __launch_bounds__(TPB) void spmm_rows_f16_kernel(EllTable t, const float *__restrict__ src, unsigned short *__restrict__ dst16,
                                                            long plane, int nlam, float *__restrict__ bscale, int NP, long K, int LinP,
                                                            int nchunk) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const int per = (t.R + 7) / 8;
    const int r = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    const int l4 = (blockIdx.y * TPB + threadIdx.x) * 4;
    if (r >= t.R) return;                                 // workgroup-uniform
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l4 < nlam) {
        const int n = t.cnt[r];
        const int64_t *col = t.col + (long)r * t.W;
        const float *val = t.val + (long)r * t.W;
        int e = 0;
        for (; e + 4 <= n; e += 4) {
            const float4 x0 = *reinterpret_cast<const float4 *>(src + col[e] + l4);
            const float4 x1 = *reinterpret_cast<const float4 *>(src + col[e + 1] + l4);
            const float4 x2 = *reinterpret_cast<const float4 *>(src + col[e + 2] + l4);
            const float4 x3 = *reinterpret_cast<const float4 *>(src + col[e + 3] + l4);
            const float v0 = val[e], v1 = val[e + 1], v2 = val[e + 2], v3 = val[e + 3];
            acc.x += v0 * x0.x; acc.y += v0 * x0.y; acc.z += v0 * x0.z; acc.w += v0 * x0.w;
            acc.x += v1 * x1.x; acc.y += v1 * x1.y; acc.z += v1 * x1.z; acc.w += v1 * x1.w;
            acc.x += v2 * x2.x; acc.y += v2 * x2.y; acc.z += v2 * x2.z; acc.w += v2 * x2.w;
            acc.x += v3 * x3.x; acc.y += v3 * x3.y; acc.z += v3 * x3.z; acc.w += v3 * x3.w;
        }
        for (; e < n; ++e) {
            const float4 x0 = *reinterpret_cast<const float4 *>(src + col[e] + l4);
            const float v0 = val[e];
            acc.x += v0 * x0.x; acc.y += v0 * x0.y; acc.z += v0 * x0.z; acc.w += v0 * x0.w;
        }
    }
    // workgroup maximum -> power-of-two scale
    float m = fmaxf(fmaxf(fabsf(acc.x), fabsf(acc.y)), fmaxf(fabsf(acc.z), fabsf(acc.w)));
    m = wave_max(m);
    __shared__ float sm[TPB / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    const float scale = f16x2_scale(m), inv = 1.f / scale;
    const int64_t off = t.dst_off[r];
    if (threadIdx.x == 0) bscale[((off % K) / LinP * nchunk + blockIdx.y) * (long)NP + off / K] = scale;
    if (l4 < nlam) {
        const float x0 = acc.x * inv, x1 = acc.y * inv, x2 = acc.z * inv, x3 = acc.w * inv;
        const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1, h2 = (_Float16)x2, h3 = (_Float16)x3;
        f16x4 h = {h0, h1, h2, h3};
        f16x4 l = {(_Float16)(x0 - (float)h0), (_Float16)(x1 - (float)h1), (_Float16)(x2 - (float)h2), (_Float16)(x3 - (float)h3)};
        *reinterpret_cast<f16x4 *>(dst16 + off + l4) = h;
        *reinterpret_cast<f16x4 *>(dst16 + plane + off + l4) = l;
    }
}
}  // namespace

int launch_spmm_rows_f16(hipStream_t s, const EllTable &t, const float *src, unsigned short *dst16, long plane, int nlam, float *bscale,
                         int NP, long K, int LinP) {
    if (t.R == 0 || nlam <= 0) return 0;
    if (nlam % 4 || plane % 4 || K % LinP || LinP % 32 || !bscale) return (int)hipErrorInvalidValue;
    dim3 grid((t.R + 7) / 8 * 8, (nlam / 4 + TPB - 1) / TPB);
    hipLaunchKernelGGL(spmm_rows_f16_kernel, grid, dim3(TPB), 0, s, t, src, dst16, plane, nlam, bscale, NP, K, LinP, (LinP + 1023) / 1024);
    return (int)hipGetLastError();
}

namespace {
// the same on a grouped table: the members' taps are read once; every member keeps its own block scale
template <int G>
__global__ __launch_bounds__(TPB) void spmm_group_gather_f16_kernel(GroupTable t, const float *__restrict__ src,
                                                                    unsigned short *__restrict__ dst16, long plane, int nlam,
                                                                    float *__restrict__ bscale, int NP, long K, int LinP, int nchunk) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const int per = (t.NG + 7) / 8;
    const int gi = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    const int l4 = (blockIdx.y * TPB + threadIdx.x) * 4;
    if (gi >= t.NG) return;                               // workgroup-uniform
    float4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l4 < nlam) {
        const int n = t.cnt[gi];
        const int64_t *col = t.col + (long)gi * t.W;
        const float *val = t.val + (long)gi * t.W * G;
        int e = 0;
        // eight taps requested before the first is used: with two the kernel waited on memory latency (0.45 -> 0.34 ms per
        // step on config 3; 4: 0.36, 12 / 16 / 24: 0.36 / 0.38 / 0.36; fewer resident workgroups only cost time)
        constexpr int GATHER_UNROLL = 8;
        for (; e + GATHER_UNROLL <= n; e += GATHER_UNROLL) {
            float4 xv[GATHER_UNROLL];
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; ++u) xv[u] = *reinterpret_cast<const float4 *>(src + col[e + u] + l4);
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float v0 = val[(e + u) * G + g];
                    acc[g].x += v0 * xv[u].x; acc[g].y += v0 * xv[u].y; acc[g].z += v0 * xv[u].z; acc[g].w += v0 * xv[u].w;
                }
        }
        for (; e < n; ++e) {
            const float4 x0 = *reinterpret_cast<const float4 *>(src + col[e] + l4);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float v0 = val[e * G + g];
                acc[g].x += v0 * x0.x; acc[g].y += v0 * x0.y; acc[g].z += v0 * x0.z; acc[g].w += v0 * x0.w;
            }
        }
    }
    __shared__ float sm[G][TPB / 64];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float m = fmaxf(fmaxf(fabsf(acc[g].x), fabsf(acc[g].y)), fmaxf(fabsf(acc[g].z), fabsf(acc[g].w)));
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) sm[g][threadIdx.x >> 6] = m;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t off = t.dst[(long)gi * G + g];
        if (off < 0) continue;                             // workgroup-uniform
        const float scale = f16x2_scale(fmaxf(fmaxf(sm[g][0], sm[g][1]), fmaxf(sm[g][2], sm[g][3]))), inv = 1.f / scale;
        if (threadIdx.x == 0) bscale[((off % K) / LinP * nchunk + blockIdx.y) * (long)NP + off / K] = scale;
        if (l4 < nlam) {
            const float x0 = acc[g].x * inv, x1 = acc[g].y * inv, x2 = acc[g].z * inv, x3 = acc[g].w * inv;
            const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1, h2 = (_Float16)x2, h3 = (_Float16)x3;
            f16x4 h = {h0, h1, h2, h3};
            f16x4 l = {(_Float16)(x0 - (float)h0), (_Float16)(x1 - (float)h1), (_Float16)(x2 - (float)h2), (_Float16)(x3 - (float)h3)};
            *reinterpret_cast<f16x4 *>(dst16 + off + l4) = h;
            *reinterpret_cast<f16x4 *>(dst16 + plane + off + l4) = l;
        }
    }
}
}  // namespace

int launch_spmm_group_gather_f16(hipStream_t s, const GroupTable &t, const float *src, unsigned short *dst16, long plane, int nlam,
                                 float *bscale, int NP, long K, int LinP) {
    if (t.NG == 0 || nlam <= 0) return 0;
    if (nlam % 4 || plane % 4 || K % LinP || LinP % 32 || !bscale) return (int)hipErrorInvalidValue;
    dim3 grid((t.NG + 7) / 8 * 8, (nlam / 4 + TPB - 1) / TPB);
    if (t.G == 4)
        hipLaunchKernelGGL(spmm_group_gather_f16_kernel<4>, grid, dim3(TPB), 0, s, t, src, dst16, plane, nlam, bscale, NP, K, LinP, (LinP + 1023) / 1024);
    else if (t.G == 8)
        hipLaunchKernelGGL(spmm_group_gather_f16_kernel<8>, grid, dim3(TPB), 0, s, t, src, dst16, plane, nlam, bscale, NP, K, LinP, (LinP + 1023) / 1024);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

namespace {
// debugging: the block-scaled fp16 operand back as fp32 [NP][K]
__global__ __launch_bounds__(TPB) void dequant_f16x2_kernel(const unsigned short *__restrict__ src16, long plane, const float *__restrict__ bscale,
                                                            float *__restrict__ dst, int NP, long K, int LinP, int nchunk) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)NP * K) return;
    const long row = i / K, k = i % K;
    const float sc = bscale[((k / LinP) * nchunk + (k % LinP) / 1024) * (long)NP + row];
    const _Float16 h = reinterpret_cast<const _Float16 *>(src16)[i], l = reinterpret_cast<const _Float16 *>(src16)[plane + i];
    dst[i] = ((float)h + (float)l) * sc;
}
}  // namespace

int launch_dequant_f16x2(hipStream_t s, const unsigned short *src16, long plane, const float *bscale, float *dst, int NP, long K, int LinP,
                         int nchunk) {
    const long n = (long)NP * K;
    hipLaunchKernelGGL(dequant_f16x2_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, src16, plane, bscale, dst, NP, K, LinP,
                       nchunk);
    return (int)hipGetLastError();
}

namespace {
// [L][na][nb] planes l0.. of a wavelength-major cube -> [nb][nap][LP] wavelength innermost (32x32 LDS tile transpose)
__global__ __launch_bounds__(256) void cube_to_lam_inner_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                int l0, int L, int na, int nb, int nap, int LP) {
    __shared__ float tile[32][33];
    const int a = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int l = blockIdx.y * 32 + i, b = blockIdx.x * 32 + tx;
        tile[i][tx] = (l < L && b < nb) ? src[((long)(l0 + l) * na + a) * nb + b] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int b = blockIdx.x * 32 + i, l = blockIdx.y * 32 + tx;
        if (b < nb && l < L) dst[((long)b * nap + a) * LP + l] = tile[tx][i];
    }
}

__global__ __launch_bounds__(256) void cube_from_lam_inner_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                  int l0, int L, int na, int nb, int nap, int LP) {
    __shared__ float tile[32][33];
    const int a = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int b = blockIdx.x * 32 + i, l = blockIdx.y * 32 + tx;
        tile[i][tx] = (b < nb && l < L) ? src[((long)b * nap + a) * LP + l] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int l = blockIdx.y * 32 + i, b = blockIdx.x * 32 + tx;
        if (l < L && b < nb) dst[((long)(l0 + l) * na + a) * nb + b] = tile[tx][i];
    }
}
}  // namespace

int launch_cube_to_lam_inner(hipStream_t s, const float *src, float *dst, int l0, int L, int na, int nb, int nap, int LP) {
    dim3 grid((nb + 31) / 32, (L + 31) / 32, na);
    hipLaunchKernelGGL(cube_to_lam_inner_kernel, grid, dim3(256), 0, s, src, dst, l0, L, na, nb, nap, LP);
    return (int)hipGetLastError();
}

int launch_cube_from_lam_inner(hipStream_t s, const float *src, float *dst, int l0, int L, int na, int nb, int nap, int LP) {
    dim3 grid((nb + 31) / 32, (L + 31) / 32, na);
    hipLaunchKernelGGL(cube_from_lam_inner_kernel, grid, dim3(256), 0, s, src, dst, l0, L, na, nb, nap, LP);
    return (int)hipGetLastError();
}

namespace {
// ---------------------------------------------------------------------------------------------
// layout helpers
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void pad_planes_kernel(const float *__restrict__ src, float *__restrict__ dst, int na,
                                                         int nb, int nap, int nbp) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    const int i = blockIdx.y;
    const long b = blockIdx.z;
    if (j < nb) dst[(b * nap + i) * nbp + j] = src[(b * na + i) * nb + j];
}

__global__ __launch_bounds__(TPB) void unpad_planes_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                           int na, int nb, int nap, int nbp) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    const int i = blockIdx.y;
    const long b = blockIdx.z;
    if (j < nb) dst[(b * na + i) * nb + j] = src[(b * nap + i) * nbp + j];
}
}  // namespace

int launch_pad_planes(hipStream_t s, const float *src, float *dst, int B, int na, int nb, int nap, int nbp) {
    dim3 grid((nb + TPB - 1) / TPB, na, B);
    hipLaunchKernelGGL(pad_planes_kernel, grid, dim3(TPB), 0, s, src, dst, na, nb, nap, nbp);
    return (int)hipGetLastError();
}

int launch_unpad_planes(hipStream_t s, const float *src, float *dst, int B, int na, int nb, int nap, int nbp) {
    dim3 grid((nb + TPB - 1) / TPB, na, B);
    hipLaunchKernelGGL(unpad_planes_kernel, grid, dim3(TPB), 0, s, src, dst, na, nb, nap, nbp);
    return (int)hipGetLastError();
}

namespace {
// thread index runs over l fastest so the slab reads are coalesced
__global__ __launch_bounds__(TPB) void y_from_cpart_kernel(const float *__restrict__ cpart, long slab, int nsplit,
                                                           float *__restrict__ y, int PS, int Ldet, int aout,
                                                           int LdetP) {
    const int l = (blockIdx.x * TPB + threadIdx.x) * 4;          // four detector wavelengths per thread: 16-byte slab reads
    const int n = blockIdx.y;           // ps*aout + a
    if (l >= Ldet) return;
    const int ps = n / aout, a = n % aout;
    const long src = (long)n * LdetP + l;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < nsplit; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(cpart + k * slab + src);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float *o = y + ((long)ps * Ldet + l) * aout + a;
    o[0] = s.x;
    if (l + 1 < Ldet) o[aout] = s.y;
    if (l + 2 < Ldet) o[2 * aout] = s.z;
    if (l + 3 < Ldet) o[3 * aout] = s.w;
}
}  // namespace

int launch_y_from_cpart(hipStream_t s, const float *cpart, long slab, int nsplit, float *y, int PS, int Ldet,
                        int aout, int LdetP) {
    if (LdetP % 4 || slab % 4) return (int)hipErrorInvalidValue;
    dim3 grid(((Ldet + 3) / 4 + TPB - 1) / TPB, PS * aout);
    hipLaunchKernelGGL(y_from_cpart_kernel, grid, dim3(TPB), 0, s, cpart, slab, nsplit, y, PS, Ldet, aout, LdetP);
    return (int)hipGetLastError();
}

namespace {
// max |value| of ymat for the per-row operand scales of the two-piece fp16 GEMM: every wave stores its maximum (bit pattern
// of a non-negative float) in its own entry of `pmax`, one small workgroup reduces the entries afterwards (no atomics:
// atomicMax into shared slots serialises in L2 at about 140 ns each).
__device__ __forceinline__ void wave_amax_store(float m, unsigned *pmax, unsigned wave_id) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) pmax[wave_id] = __float_as_uint(m);
}

// per-wave maxima -> max |A[m][:]| per GEMM row.  ymat: the entries of a row are contiguous (one thread per row).
__global__ __launch_bounds__(TPB) void rowmax_contiguous_kernel(const unsigned *__restrict__ pmax, int per_row, int nrows, int NP,
                                                                unsigned *__restrict__ rowmax) {
    const int n = blockIdx.x * TPB + threadIdx.x;
    if (n >= NP) return;
    unsigned m = 0;
    if (n < nrows)
        for (int i = 0; i < per_row; ++i) m = max(m, pmax[(long)n * per_row + i]);
    rowmax[n] = m;                                                   // padding rows of the operand are zero
}

__global__ __launch_bounds__(TPB) void ymat_from_y_kernel(const float *__restrict__ y, float *__restrict__ ymat, int PS,
                                                          int Ldet, int aout, int LdetP, unsigned *amax) {
    const int l = blockIdx.x * TPB + threadIdx.x;
    const int n = blockIdx.y;
    float v = 0.f;
    if (l < Ldet) {
        const int ps = n / aout, a = n % aout;
        v = y[((long)ps * Ldet + l) * aout + a];
        ymat[(long)n * LdetP + l] = v;
    }
    if (amax) wave_amax_store(fabsf(v), amax, (blockIdx.y * gridDim.x + blockIdx.x) * (TPB / 64) + (threadIdx.x >> 6));
}
}  // namespace

long ymat_from_y_waves(int PS, int Ldet, int aout) { return (long)((Ldet + TPB - 1) / TPB) * PS * aout * (TPB / 64); }

int launch_ymat_from_y(hipStream_t s, const float *y, float *ymat, int PS, int Ldet, int aout, int LdetP, unsigned *pmax,
                       unsigned *rowmax, int NP) {
    if (pmax && (!rowmax || NP < PS * aout)) return (int)hipErrorInvalidValue;
    dim3 grid((Ldet + TPB - 1) / TPB, PS * aout);
    hipLaunchKernelGGL(ymat_from_y_kernel, grid, dim3(TPB), 0, s, y, ymat, PS, Ldet, aout, LdetP, pmax);
    if (pmax)
        hipLaunchKernelGGL(rowmax_contiguous_kernel, dim3((NP + TPB - 1) / TPB), dim3(TPB), 0, s, pmax, (int)grid.x * (TPB / 64), PS * aout,
                           NP, rowmax);
    return (int)hipGetLastError();
}

namespace {
// Normal operator A^T A d: the forward model's output y is only the hand-over to the adjoint, whose GEMM operand
// ymat[n][l] = y[ps][l][a] (n = ps * aout + a) is again the slab sum in the slabs' own layout.  One workgroup per operand row:
// sum of the K slabs (same order as y_from_cpart_kernel), the row's maximum, the two fp16 pieces of the row at its
// power-of-two scale -- the bits y_from_cpart -> ymat_from_y -> rowmax -> split_rows2h produce, in one pass over the slabs.  The GEMM
// recomputes the scale from rowmax with the same f16x2_scale (f16_split.h).
// WGT: the data weights of the row (surfh_set_data_weights; wmat in ymat's layout, zero in the padding) multiply the slab sum once,
// BEFORE the row maximum -- a masked outlier must not take the row's fp16 range.  The bits are those of the chain with the
// element-wise weight kernel on y between y_from_cpart and ymat_from_y.
template <int NV, bool WGT>      // float4 per thread: LdetP <= NV * 1024
__device__ __forceinline__ void ymat16_from_cpart_row(const float *__restrict__ cpart, long slab, int nsplit, unsigned short *__restrict__ dst16,
                                                      long plane, unsigned *__restrict__ rowmax, int nrows, int Ldet, int LdetP,
                                                      const float *__restrict__ wmat) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const int n = blockIdx.x;
    float4 v[NV];
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int l = (j * TPB + threadIdx.x) * 4;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < nrows && l < Ldet) {
            const long src = (long)n * LdetP + l;
            for (int k = 0; k < nsplit; ++k) {
                const float4 x = *reinterpret_cast<const float4 *>(cpart + k * slab + src);
                s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
            }
            if (l + 1 >= Ldet) s.y = 0.f;        // columns beyond Ldet hold the products of the zero rows of W: not part of y
            if (l + 2 >= Ldet) s.z = 0.f;
            if (l + 3 >= Ldet) s.w = 0.f;
            if (WGT) {
                const float4 w = *reinterpret_cast<const float4 *>(wmat + src);
                s.x *= w.x; s.y *= w.y; s.z *= w.z; s.w *= w.w;
            }
        }
        v[j] = s;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fmaxf(fabsf(s.z), fabsf(s.w))));
    }
    m = wave_max(m);
    __shared__ float sm[TPB / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    if (threadIdx.x == 0) rowmax[n] = __float_as_uint(m);
    const float inv = 1.f / f16x2_scale(m);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int l = (j * TPB + threadIdx.x) * 4;
        if (l >= LdetP) continue;
        const float x0 = v[j].x * inv, x1 = v[j].y * inv, x2 = v[j].z * inv, x3 = v[j].w * inv;
        const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1, h2 = (_Float16)x2, h3 = (_Float16)x3;
        f16x4 h = {h0, h1, h2, h3};
        f16x4 lo = {(_Float16)(x0 - (float)h0), (_Float16)(x1 - (float)h1), (_Float16)(x2 - (float)h2), (_Float16)(x3 - (float)h3)};
        const long o = (long)n * LdetP + l;
        *reinterpret_cast<f16x4 *>(dst16 + o) = h;
        *reinterpret_cast<f16x4 *>(dst16 + plane + o) = lo;
    }
}
template <int NV>
__global__ __launch_bounds__(TPB) void ymat16_from_cpart_kernel(const float *__restrict__ cpart, long slab, int nsplit, unsigned short *__restrict__ dst16,
                                                                long plane, unsigned *__restrict__ rowmax, int nrows, int Ldet, int LdetP) {
    ymat16_from_cpart_row<NV, false>(cpart, slab, nsplit, dst16, plane, rowmax, nrows, Ldet, LdetP, nullptr);
}
template <int NV>
__global__ __launch_bounds__(TPB) void ymat16w_from_cpart_kernel(const float *__restrict__ cpart, long slab, int nsplit, unsigned short *__restrict__ dst16,
                                                                 long plane, unsigned *__restrict__ rowmax, int nrows, int Ldet, int LdetP,
                                                                 const float *__restrict__ wmat) {
    ymat16_from_cpart_row<NV, true>(cpart, slab, nsplit, dst16, plane, rowmax, nrows, Ldet, LdetP, wmat);
}
}  // namespace

int launch_ymat16_from_cpart(hipStream_t s, const float *cpart, long slab, int nsplit, unsigned short *dst16, long plane, unsigned *rowmax,
                             int NP, int nrows, int Ldet, int LdetP) {
    if (LdetP % 4 || slab % 4 || plane % 4 || LdetP > 4 * 4 * TPB || nrows > NP) return (int)hipErrorInvalidValue;
    const int nv = (LdetP + 4 * TPB - 1) / (4 * TPB);
#define SURFH_Y16(NV_) hipLaunchKernelGGL(ymat16_from_cpart_kernel<NV_>, dim3(NP), dim3(TPB), 0, s, cpart, slab, nsplit, dst16, plane, rowmax, nrows, Ldet, LdetP)
    if (nv <= 1) SURFH_Y16(1);
    else if (nv == 2) SURFH_Y16(2);
    else if (nv == 3) SURFH_Y16(3);
    else SURFH_Y16(4);
#undef SURFH_Y16
    return (int)hipGetLastError();
}

int launch_ymat16w_from_cpart(hipStream_t s, const float *cpart, long slab, int nsplit, unsigned short *dst16, long plane, unsigned *rowmax,
                              int NP, int nrows, int Ldet, int LdetP, const float *wmat) {
    if (LdetP % 4 || slab % 4 || plane % 4 || LdetP > 4 * 4 * TPB || nrows > NP || !wmat) return (int)hipErrorInvalidValue;
    const int nv = (LdetP + 4 * TPB - 1) / (4 * TPB);
#define SURFH_Y16W(NV_) hipLaunchKernelGGL(ymat16w_from_cpart_kernel<NV_>, dim3(NP), dim3(TPB), 0, s, cpart, slab, nsplit, dst16, plane, rowmax, nrows, Ldet, LdetP, wmat)
    if (nv <= 1) SURFH_Y16W(1);
    else if (nv == 2) SURFH_Y16W(2);
    else if (nv == 3) SURFH_Y16W(3);
    else SURFH_Y16W(4);
#undef SURFH_Y16W
    return (int)hipGetLastError();
}

namespace {
// ---- data weights (surfh_set_data_weights): W = diag(w) in the criterion mu (y - A x)^T W (y - A x) / 2 ------------------------
// y *= w: the hand-over of the normal operator wherever it goes through y
__global__ __launch_bounds__(TPB) void weight_mul_kernel(float *__restrict__ y, const float *__restrict__ w, long n) {
    long i = (long)blockIdx.x * TPB + threadIdx.x;
    const long stride = (long)gridDim.x * TPB;
    for (; i < n; i += stride) y[i] *= w[i];
}
// out = W y for the right-hand side, as a select: a sample of weight 0 gives 0 whatever its datum (0 * NaN is NaN)
__global__ __launch_bounds__(TPB) void weight_select_kernel(const float *__restrict__ y, const float *__restrict__ w, float *__restrict__ out, long n) {
    long i = (long)blockIdx.x * TPB + threadIdx.x;
    const long stride = (long)gridDim.x * TPB;
    for (; i < n; i += stride) {
        const float wi = w[i];
        out[i] = wi > 0.f ? wi * y[i] : 0.f;
    }
}
// *count += number of weights that are negative, NaN or infinite
__global__ __launch_bounds__(TPB) void weight_count_bad_kernel(const float *__restrict__ w, long n, unsigned *__restrict__ count) {
    long i = (long)blockIdx.x * TPB + threadIdx.x;
    const long stride = (long)gridDim.x * TPB;
    unsigned bad = 0;
    for (; i < n; i += stride) {
        const float wi = w[i];
        bad += !(wi >= 0.f && wi <= FLT_MAX);
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    __shared__ unsigned sm[TPB / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        bad = sm[0] + sm[1] + sm[2] + sm[3];
        if (bad) atomicAdd(count, bad);
    }
}
}  // namespace

static unsigned weight_grid(long n) { return (unsigned)std::min<long>((n + TPB - 1) / TPB, 4096); }
int launch_weight_mul(hipStream_t s, float *y, const float *w, long n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(weight_mul_kernel, dim3(weight_grid(n)), dim3(TPB), 0, s, y, w, n);
    return (int)hipGetLastError();
}
int launch_weight_select(hipStream_t s, const float *y, const float *w, float *out, long n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(weight_select_kernel, dim3(weight_grid(n)), dim3(TPB), 0, s, y, w, out, n);
    return (int)hipGetLastError();
}
int launch_weight_count_bad(hipStream_t s, const float *w, long n, unsigned *count) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(weight_count_bad_kernel, dim3(weight_grid(n)), dim3(TPB), 0, s, w, n, count);
    return (int)hipGetLastError();
}
