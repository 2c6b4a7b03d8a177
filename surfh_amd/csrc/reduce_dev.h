// The fixed-order reductions of the workgroup kernels: float64 sums formed per wave by shuffles, per block from the waves' sums in
// wave order, and per launch from the blocks' partial sums in block order -- the same inputs give the same bits on every call.
// Every kernel that uses them runs RED_TPB threads per block.  The namespace is anonymous: every translation unit has its own
// parts_reduce_kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int RED_TPB = 256;          // block size of every kernel that uses the reductions below

// the maximum over the wave's 64 lanes, in every lane
__device__ __forceinline__ float wave_max(float m) {
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
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

template <int N>
__device__ inline void block_sum_bcast(double (&v)[N]) {   // sums over the workgroup, result in every thread
    __shared__ double sm[N][RED_TPB / 64];
    __shared__ double tot[N];
    __syncthreads();                                       // previous use of the buffers is over
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double t = v[k];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
        if ((threadIdx.x & 63) == 0) sm[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double t = 0.0;
        for (int w = 0; w < RED_TPB / 64; ++w) t += sm[threadIdx.x][w];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = tot[k];
}

// the sum of a previous launch's per-block partial sums, every block for itself and in reduce_final_kernel's order (same bits)
__device__ inline double parts_sum(const double *__restrict__ scratch, int nparts) {      // valid in every thread
    __shared__ double smp[RED_TPB / 64];
    __shared__ double tot;
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += RED_TPB) s += scratch[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) smp[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < RED_TPB / 64; ++k) t += smp[k];
        tot = t;
    }
    __syncthreads();
    return tot;
}

// out[k] = sum_i part[k * nparts + i], one block per k, reduce_final_kernel's order
__global__ __launch_bounds__(RED_TPB) void parts_reduce_kernel(const double *__restrict__ part, int nparts, double *__restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += RED_TPB) s += part[(long)blockIdx.x * nparts + i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace
