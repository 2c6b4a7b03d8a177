// The operand scale of the two-piece fp16 split (gemm_cc16.hip), in its one definition: the producers that write fp16 pieces under
// a scale taken from a maximum (gather_kernels.hip) and the GEMM that recomputes the scale from the same maximum must agree bit for bit.
// A plain C++ compiler may include this header: the qualifiers exist only under a HIP compiler.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define F16_SPLIT_FN __host__ __device__ __forceinline__
#else
#define F16_SPLIT_FN inline
#endif

// power of two that brings `amax` to [2^13, 2^14), clamped to the normal range; 1 for a zero row (and for a negative or NaN `amax`)
F16_SPLIT_FN float f16x2_scale(float amax) {
    if (!(amax > 0.f)) return 1.f;
    const int e = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xFF) - 127;
    int sc = e - 13;
    sc = sc < -126 ? -126 : (sc > 127 ? 127 : sc);
    return __builtin_bit_cast(float, (unsigned)(sc + 127) << 23);
}
