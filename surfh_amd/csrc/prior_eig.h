// The quadratic prior in the Fourier domain: the circular first difference along an axis of n samples is diagonal there, with
// |D(k)|^2 = 2 - 2 cos(2 pi k / n) = 4 sin^2(pi k / n).  The cosine form cancels in fp32 at the low frequencies, the bins that
// carry most of a map's energy (relative error 6e-5 at k = 1 of n = 251, 3e-4 at n = 501); the sine form has nothing to cancel.
// k folds to the lower half of the axis first (sin(pi k / n) = sin(pi (n - k) / n), exact in integers): the fp32 quotient next to 1
// is off by up to 2^-25, which is n 2^-25 of the distance to 1 the sine measures there.  Relative error <= 6e-7 at every k.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float dsq(int k, int n) {
    const float s = sinpif((float)(2 * k > n ? n - k : k) / (float)n);
    return 4.f * s * s;
}

}  // namespace
