// What the prior kernels of the maps (kernels.hip) and of the cube (huber_vox.hip) share: the Huber potential in one arithmetic,
// and the fixed-order float64 reductions that make repeated calls give the same bits.
// phi(u) = u^2 / 2 (|u| <= delta), delta (|u| - delta / 2) beyond; phi'(u) = u or delta sign(u); w(u) = phi'(u) / u, w(0) = 1.
// Differences and phi' in fp32, phi in float64 (it is only ever summed); delta = +inf is the quadratic potential.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int RED_TPB = 256;          // block size of every kernel that uses the reductions below

__device__ __forceinline__ float huber_dphi(float u, float delta) { return fabsf(u) <= delta ? u : copysignf(delta, u); }
__device__ __forceinline__ float huber_w(float u, float delta) { return fabsf(u) <= delta ? 1.f : delta / fabsf(u); }
__device__ __forceinline__ double huber_phi(float u, float delta) {
    const float a = fabsf(u);
    return a <= delta ? 0.5 * (double)a * (double)a : (double)delta * ((double)a - 0.5 * (double)delta);
}

__device__ inline double block_sum(double v) {
    __shared__ double sm[RED_TPB / 64];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sm[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < RED_TPB / 64; ++k) s += sm[k];
    return s;   // valid in thread 0
}

// K block sums in a fixed order; part[k * nparts + b] = sum over block b of v[k]
template <int K>
__device__ inline void block_sums_to(double (&v)[K], double *__restrict__ part, int b, int nparts) {
    __shared__ double sm[K][RED_TPB / 64];
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sm[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x < K) {
        double s = 0.0;
        for (int w = 0; w < RED_TPB / 64; ++w) s += sm[threadIdx.x][w];
        part[(long)threadIdx.x * nparts + b] = s;
    }
}
template <int K>
__device__ inline void block_sums_to(double (&v)[K], double *__restrict__ part) {
    block_sums_to<K>(v, part, blockIdx.x, gridDim.x);
}

// out[k] = sum_i part[k * nparts + i], one block per k, reduce_final_kernel's order
__global__ __launch_bounds__(RED_TPB) void parts_reduce_kernel(const double *__restrict__ part, int nparts, double *__restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += RED_TPB) s += part[(long)blockIdx.x * nparts + i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace
