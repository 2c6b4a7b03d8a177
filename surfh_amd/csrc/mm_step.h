// The float64 scalar algebra every 3MG step shares, on the host (plan_solvers.hip) and in the plane kernels (cg_kernels.hip, huber_kernels.hip).
// A plain C++ compiler may include this header: the qualifiers exist only under a HIP compiler.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_STEP_FN __host__ __device__ __forceinline__
#else
#define MM_STEP_FN inline
#endif

// The block (d.Wd, d.Wm) of d = g + beta m from the block c00 = g.Wg, c01 = g.Wm, c11 = m.Wm, by linearity.
MM_STEP_FN void mm_block_of_d(double c00, double c01, double c11, double beta, double *dWd, double *dWm) {
    *dWd = c00 + beta * (2.0 * c01 + beta * c11);
    *dWm = c01 + beta * c11;
}

// Minimiser (s0, s1) of the majorant over span{d, m}: [[dBd, dBm], [dBm, mBm]] s = [dg, mg], solved in the scaled form
// (unit diagonal, c = dBm / sqrt(dBd mBm)).  Without curvature along d (dBd <= 0 or NaN) nothing moves; without a memory
// direction (mBm <= 0), or with the scaled system singular (det = 1 - c^2 not above the guard), the step is the one along d alone.
MM_STEP_FN void mm_step2(double dBd, double dBm, double mBm, double dg, double mg, double *s0, double *s1) {
    *s0 = dBd > 0.0 ? dg / dBd : 0.0;
    *s1 = 0.0;
    if (dBd > 0.0 && mBm > 0.0) {
        const double sq = sqrt(dBd * mBm), c = dBm / sq, det = 1.0 - c * c;
        if (det > 1e-12) {
            *s0 = (dg / dBd - c * mg / sq) / det;
            *s1 = (mg / mBm - c * dg / sq) / det;
        }
    }
}
