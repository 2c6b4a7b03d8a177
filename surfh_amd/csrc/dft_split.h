// What the two-piece fp16 DFT passes (dft_h2.hip, dft_ct.hip) share: the fragment types, the three-product MFMA group, the split
// of scaled values into (hi, lo) fp16 fragments and the per-column block exponent's bounds.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int E_TARGET = 10, E_LIMIT = 15;            // a column's largest scaled magnitude: set below 2^10, rescaled at 2^15

#define MFMA3(acc_, ah_, al_, bh_, bl_)                                             \
    {                                                                               \
        f32x16 c_ = acc_;                                                           \
        c_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(al_, bh_, c_, 0, 0, 0);         \
        c_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah_, bl_, c_, 0, 0, 0);         \
        c_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah_, bh_, c_, 0, 0, 0);         \
        acc_ = c_;                                                                  \
    }

// 8 scaled values -> (hi, lo) fp16 fragments
__device__ __forceinline__ void split8h(const float (&x)[8], int e, f16x8 &fh, f16x8 &fl) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float xs = __builtin_amdgcn_ldexpf(x[j], e);
        const _Float16 hh = (_Float16)xs;
        fh[j] = hh;
        fl[j] = (_Float16)(xs - (float)hh);
    }
}

// the value held by the neighbouring lane (lane ^ 1): the other component of the same complex column
__device__ __forceinline__ float pair_swap(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
}

}  // namespace
