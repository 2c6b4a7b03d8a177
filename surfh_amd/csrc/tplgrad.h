// Template refinement: the operator's transpose with respect to the templates and the template solver's vector kernels
// (tplgrad.hip, which states the identity and the mapping).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// Spectral route.  spec, sotf: interleaved spectra [KAP][KBP][LP][2] (spec = the unitary half spectrum of the cube-space adjoint,
// every bin ka < Na, kb <= Nb / 2 written); mhat: the maps' half spectra [T][2][KAP][KBP], 1 <= T <= 4; part: room for
// tplgrad_part_doubles(..., true) doubles; cidx [Lc]: cube plane -> the plan's compact plane index, -1 where the plan holds none.
// G [T][Lc] in cube-plane order, exactly 0 on the planes without a compact index.  LP a multiple of 128.
int launch_tplgrad_spec(hipStream_t s, const float *spec, const float *sotf, const float *mhat, double *part, const int *cidx, float *G, int T,
                        int Lc, int Na, int Nb, long KBP, long PL, int LP);
// Spatial route.  cube [NBP][NAP][LP]: the cube-space adjoint after its OTF^T; maps [T][Na][Nb], 1 <= T <= SURFH_MAX_TEMPLATES.
int launch_tplgrad_pix(hipStream_t s, const float *cube, const float *maps, double *part, const int *cidx, float *G, int T, int Lc, int Na,
                       int Nb, int NAP, int LP);
size_t tplgrad_part_doubles(int T, int Na, int Nb, int LP, bool spectral);
// spec *= conj(sotf) in place: interleaved [PL][LP][2] (ilv) or planar [2][PL][LP]
int launch_otf_conj_mul(hipStream_t s, float *spec, const float *sotf, long PL, int LP, int ilv);
// tpl [T][LP] (compact planes, zero where pidx [LP] is negative) = S [T][Lc] (cube-plane order)
int launch_tpl_pack(hipStream_t s, const float *S, const int *pidx, float *tpl, int T, int Lc, int LP);
// q += mu_spec D^T D d on [T][Lc], D the first difference along the wavelength with open ends
int launch_tpl_prior_add(hipStream_t s, const float *d, float *q, int T, int Lc, float mu_spec);
// out[0] = sum w (y - u)^2 in float64, fixed order (w null: 1; w <= 0 takes the sample out, NaN included); scratch >= 512 doubles
int launch_wres_sq(hipStream_t s, const float *y, const float *u, const float *w, long n, double *scratch, double *out);
