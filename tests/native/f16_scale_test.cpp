// Stand-alone host test of surfh_amd/csrc/f16_split.h: f16x2_scale, the one definition of the fp16 operand scale that the device
// kernels share, against the frexp / ldexp formula of the host function gemm_f16x2_scale (gemm_cc16.hip), copied below.
// tests/test_f16_scale_host.py compiles and runs it (no GPU, no HIP header, no library load).
#include "../../surfh_amd/csrc/f16_split.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace {
long g_checks = 0, g_fails = 0;

float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// gemm_f16x2_scale of gemm_cc16.hip, verbatim
float reference_scale(float amax) {
    if (!(amax > 0.f)) return 1.f;
    int e = 0;
    std::frexp(amax, &e);                  // amax = f * 2^e, f in [0.5, 1)  ->  floor(log2(amax)) = e - 1
    int s = (e - 1) - 13;
    s = s < -126 ? -126 : (s > 127 ? 127 : s);
    return std::ldexp(1.f, s);
}

void check(bool ok, const char *what, float a) {
    ++g_checks;
    if (!ok) {
        ++g_fails;
        fprintf(stderr, "FAILED: %s at a = %a (bits 0x%08x): f16x2_scale = %a, reference = %a\n", what, (double)a, bits_of(a),
                (double)f16x2_scale(a), (double)reference_scale(a));
    }
}
}  // namespace

int main() {
    // every biased exponent of a positive finite fp32 (0: the denormals; 254: up to FLT_MAX) with four mantissas.
    // +inf (exponent 255, mantissa 0) is the one input where the two formulas differ -- the bit-field form gives 2^115, frexp leaves
    // its exponent unspecified -- and no maximum of finite data reaches it: not asserted.
    const uint32_t mant[4] = {0u, 1u, 0x400000u, 0x7FFFFFu};
    for (uint32_t ex = 0; ex <= 254; ++ex)
        for (uint32_t m : mant) {
            const float a = from_bits((ex << 23) | m);            // ex = 0, m = 0 is +0: both give 1
            const float s = f16x2_scale(a);
            check(bits_of(s) == bits_of(reference_scale(a)), "agrees with the frexp / ldexp formula", a);
            const int sc = (int)ex - 127 - 13;                    // a normal input whose scale the clamp leaves alone
            if (ex >= 1 && sc >= -126 && sc <= 127) check(a / s >= 8192.f && a / s < 16384.f, "a / scale in [2^13, 2^14)", a);
        }
    check(bits_of(from_bits(1u << 23)) == bits_of(FLT_MIN) && bits_of(from_bits((254u << 23) | 0x7FFFFFu)) == bits_of(FLT_MAX),
          "the sweep covers FLT_MIN and FLT_MAX", FLT_MIN);

    const float ones[4] = {0.f, -0.f, -1.f, std::nanf("")};
    for (float a : ones) check(bits_of(f16x2_scale(a)) == bits_of(1.f), "exactly 1 for zero, negative and NaN", a);

    check(f16x2_scale(8192.f) == 1.f, "f16x2_scale(8192) == 1", 8192.f);
    check(f16x2_scale(16383.f) == 1.f, "f16x2_scale(16383) == 1", 16383.f);
    check(f16x2_scale(16384.f) == 2.f, "f16x2_scale(16384) == 2", 16384.f);
    check(f16x2_scale(1.f) == ldexpf(1.f, -13), "f16x2_scale(1) == 2^-13", 1.f);

    if (g_fails) {
        fprintf(stderr, "%ld of %ld checks FAILED\n", g_fails, g_checks);
        return 1;
    }
    printf("%ld checks passed\n", g_checks);
    return 0;
}
