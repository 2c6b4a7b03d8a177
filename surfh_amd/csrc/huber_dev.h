// What the prior kernels of the maps and planes (huber_kernels.hip, coupled_prior.hip), of the cube (huber_vox.hip) and the robust data
// term (robust_data.hip) share: the Huber potential and its two siblings, each in one arithmetic.
// phi(u) = u^2 / 2 (|u| <= delta), delta (|u| - delta / 2) beyond; phi'(u) = u or delta sign(u); w(u) = phi'(u) / u, w(0) = 1.
// Differences and phi' in fp32, phi in float64 (it is only ever summed); delta = +inf is the quadratic potential.
// The other potentials of the 3MG solvers (surfh_set_potential), normalised alike (phi ~ u^2 / 2 at 0, w(0) = 1), t = u / delta:
//   hyperbolic    phi = delta^2 (sqrt(1 + t^2) - 1),   w = 1 / sqrt(1 + t^2)      (convex, w smooth)
//   Hebert-Leahy  phi = delta^2 log(1 + t^2) / 2,      w = 1 / (1 + t^2)          (non-convex, phi' redescends)
// in forms without a delta^2 factor, so that delta = +inf gives u^2 / 2, u and 1 exactly; phi' = u w.  pot_phi / pot_dphi /
// pot_w<KIND> are what the kernels call, KIND a template parameter chosen on the host (pot_dispatch); KIND = POT_HUBER is the
// three functions above, unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace {

__device__ __forceinline__ float huber_dphi(float u, float delta) { return fabsf(u) <= delta ? u : copysignf(delta, u); }
__device__ __forceinline__ float huber_w(float u, float delta) { return fabsf(u) <= delta ? 1.f : delta / fabsf(u); }
__device__ __forceinline__ double huber_phi(float u, float delta) {
    const float a = fabsf(u);
    return a <= delta ? 0.5 * (double)a * (double)a : (double)delta * ((double)a - 0.5 * (double)delta);
}

enum { POT_HUBER = 0, POT_HYPERBOLIC = 1, POT_HEBERT_LEAHY = 2, POT_KINDS = 3 };

// t^2 overflows fp32 above |t| ~ 1.8e19.  From |t| = 2^24 on, 1 + t^2 rounds to t^2 and the hyperbolic w is 1 / |t| = delta / |u|
// (phi' -> delta sign u, as Huber's); the Hebert-Leahy w is below FLT_MIN once t^2 overflows and flushes to 0.
template <int KIND>
__device__ __forceinline__ float pot_w(float u, float delta) {
    if constexpr (KIND == POT_HUBER) return huber_w(u, delta);
    const float t = u / delta;
    if constexpr (KIND == POT_HYPERBOLIC) return fabsf(t) >= 16777216.f ? delta / fabsf(u) : 1.f / sqrtf(1.f + t * t);
    return 1.f / (1.f + t * t);
}
// phi' = u w: a solver's gradient pass and its curvature pass see the same weight
template <int KIND>
__device__ __forceinline__ float pot_dphi(float u, float delta) {
    if constexpr (KIND == POT_HUBER) return huber_dphi(u, delta);
    return u * pot_w<KIND>(u, delta);
}
template <int KIND>
__device__ __forceinline__ double pot_phi(float u, float delta) {
    if constexpr (KIND == POT_HUBER) return huber_phi(u, delta);
    const double du = u, t = du / (double)delta, t2 = t * t;           // |t| < 3e76: t2 is finite in float64
    if constexpr (KIND == POT_HYPERBOLIC) return du * du / (1.0 + sqrt(1.0 + t2));
    return 0.5 * du * du * (t2 < 1e-8 ? 1.0 - 0.5 * t2 : log1p(t2) / t2);
}

// calls f(std::integral_constant<int, kind>()); false on an unknown kind
template <class F>
inline bool pot_dispatch(int kind, F &&f) {
    switch (kind) {
    case POT_HUBER: f(std::integral_constant<int, POT_HUBER>()); return true;
    case POT_HYPERBOLIC: f(std::integral_constant<int, POT_HYPERBOLIC>()); return true;
    case POT_HEBERT_LEAHY: f(std::integral_constant<int, POT_HEBERT_LEAHY>()); return true;
    default: return false;
    }
}

}  // namespace
