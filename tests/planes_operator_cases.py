"""The normal operator of the plane-wise (no-template) model, q = mu A^T W A v + mu_reg (Dr^T Dr + Dc^T Dc) v, element by element
on every route of the device-resident CG: the problems, the float64 references and the checks shared by
tests/test_planes_operator_host.py (no GPU) and tests/test_gpu_planes_operator.py (``planes_normal_dev``,
surfh_debug_planes_normal).  Nothing here touches a GPU.

Shapes: one per route of a plan without templates (ROUTES).  A 12-slit field of view as tests/test_gpu_variants.py:blurred_case,
on image axes of their own lengths, so that alpha and beta can sit on different transform kernels.  Both float64 checkers
(oracle.surfh_oracle.BlurredOracle, rotated_oracle.RotatedOracle at 20 degrees) take every shape.

Planes: Lc = 3 (plane pitch 128: 125 padding planes) everywhere, Lc = 130 at (96, 96) (the second 128-wavelength super-tile holds
two planes), and Lc = 4 where beta runs on dft_ct.  v is standard normal, every plane scaled by a factor of its own, log-uniform
in [1e-2, 1e2], plane ZERO_PLANE = 2 all zero.  The real passes of dft_ct transform the planes (l, l ^ 1) as one complex column
(``paired``): planes 0 and 1 are two live planes of different factors in one pair at every Lc, and at Lc = 4 the all-zero plane
shares its pair with the live plane 3 (at Lc = 3 with a padding plane).  Weights: none, or uniform in [0.5, 2] with 15 % zeros.
(mu, mu_reg): PAIRS, and OWN_PAIRS for the fold's decision in fp32.

Measures: tests/helpers.py:local_errs PER PLANE (rel, max, worst row, worst column) -- the planes are independent problems and a
faint plane must not be judged on a bright neighbour's scale -- every one below the project's gate TOL; the all-zero plane has to
come back exactly zero.  No route gets another bound.  Where a paired route misses one (the faint plane of a pair, the all-zero
plane beside a live one), the GPU test records which plane of which route as a strict expected failure with the measured value
(``over_tol``, EXPECTED_OVER there), and holds every plane to ``pair_bound`` so that the expected failure cannot grow unseen."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rotated_oracle as ro  # noqa: E402
from helpers import TOL, local_errs  # noqa: E402
from oracle import surfh_oracle as orc  # noqa: E402

f32 = np.float32
DENSE, H2, CT = 0, 1, 2
STEP, STEP_DEG = ro.STEP, ro.STEP_DEG
ANGLE = 20.0
ZERO_PLANE = 2
EPS = 2.0 ** -24
# what a plane may hold of its pair's partner, as a fraction of the partner's largest value: an application runs four paired real
# passes (r2c and c2r in the forward and in the adjoint half), each separation (X[k] +- conj X[N - k]) / 2 leaves at most one fp32
# rounding of the partner's magnitude
PAIR_LEAK = 4 * EPS
PLANE_AXES = dict(row=0, col=1)
SWITCHES = ("SURFH_DFT_H2", "SURFH_DFT_CT", "SURFH_DFT_DENSE", "SURFH_NO_FUSED_MIX", "SURFH_ADJ_FUSED", "SURFH_OTF_PROD",
            "SURFH_OTF_SUPPORT", "SURFH_OTF_RANGES")                   # bit i of surfh_route_decide's mask: switch i is on
SWITCH_DEFAULTS = 0b11110011

# name -> (Na, Nb), the environment at plan creation, (kernel along alpha, along beta, OTF product in the inverse's loader)
ROUTES = {
    "h2_even": ((96, 96), {}, (H2, H2, 0)),                             # even axes: Nyquist bins exist
    "h2_odd": ((83, 85), {}, (H2, H2, 0)),                              # odd axes: no Nyquist bin
    "h2_ct": ((80, 300), {}, (H2, CT, 0)),                              # the folded specmix_adj behind a dft_ct pass
    "ct_h2": ((300, 80), {}, (CT, H2, 1)),                              # the product loader, dft_h2 rows
    "ct_ct": ((256, 258), {}, (CT, CT, 1)),                             # 256 = 4 x 64, the smallest dft_ct length; 258 = 3 x 86
    "dense": ((257, 80), {}, (DENSE, DENSE, 0)),                        # 257 is prime: planar arrays, no fold
    "ct_ct_own_products": ((256, 258), {"SURFH_OTF_PROD": "0"}, (CT, CT, 0)),      # the interleaved fold on dft_ct axes
}
ROTATED = ("h2_even", "ct_h2")
PLANES = {name: (3, 130) if name == "h2_even" else (3, 4) if r[2][1] == CT else (3,) for name, r in ROUTES.items()}
PAIRS = ((1.0, 0.05), (1.3, 0.07), (1.3, 0.0), (0.0, 0.07), (0.02, 5.0), (1.3, 1e-50))
# the product loader scales by (float) mu and weighs the prior by (float) (mu_reg / mu): a mu that is 0 in fp32, a ratio that is not finite
OWN_PAIRS = ((1e-50, 0.07), (1e-30, 1e10))
WEIGHTS = ("none", "weighted")


def switch_mask(env):
    mask = SWITCH_DEFAULTS
    for i, k in enumerate(SWITCHES):
        if k in env:
            mask = (mask | 1 << i) if env[k] == "1" else (mask & ~(1 << i))
    return mask


def pitch(Lc):
    return -(-Lc // 128) * 128


# ---- the problems -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(name, Lc, rotated=False):
    """The arguments of the model and of its float64 checker, as rotated_oracle.small_case gives them."""
    (Na, Nb), _, _ = ROUTES[name]
    s = STEP_DEG
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), ANGLE if rotated else 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    sotf = orc.ir2fr(orc.gaussian_psf(np.linspace(7.0, 8.2, Lc), STEP), (Na, Nb))
    pts = [(0.0, 0.0), (2.3 * s, -3.1 * s), (-4.6 * s, 1.7 * s)] if rotated else [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s)]
    return dict(name=name, Lc=Lc, rotated=rotated, spec=spec, sotf=sotf, alpha_axis=orc.synthetic_axes(Na, s),
                beta_axis=orc.synthetic_axes(Nb, s), step_deg=s, pointings=pts, imshape=(Na, Nb))


@functools.lru_cache(maxsize=None)
def oracle(name, Lc, rotated=False):
    c = problem(name, Lc, rotated)
    cls = ro.RotatedOracle if rotated else orc.BlurredOracle
    return cls(c["sotf"], c["alpha_axis"], c["beta_axis"], c["spec"], c["step_deg"], c["pointings"])


def _seed(name, Lc, rotated):
    return 9000 + 37 * sorted(ROUTES).index(name) + Lc + (5 if rotated else 0)


@functools.lru_cache(maxsize=None)
def vector(name, Lc, rotated=False):
    """v [Lc][Na][Nb] float32 (what the device is given; the references start from these very values) and the planes' factors."""
    rng = np.random.default_rng(_seed(name, Lc, rotated))
    scale = 10.0 ** rng.uniform(-2.0, 2.0, Lc)
    scale[ZERO_PLANE] = 0.0
    v = (rng.standard_normal((Lc,) + ROUTES[name][0]) * scale[:, None, None]).astype(f32)
    v.flags.writeable = False
    return v, scale


@functools.lru_cache(maxsize=None)
def data_weights(name, Lc, rotated=False):
    """[Lc][P S a] float32: uniform in [0.5, 2], 15 % zeros"""
    bo = oracle(name, Lc, rotated)
    rng = np.random.default_rng(_seed(name, Lc, rotated) + 1)
    shape = (Lc, int(np.prod(bo.slices_shape)))
    w = rng.uniform(0.5, 2.0, shape)
    w[rng.random(shape) < 0.15] = 0.0
    w = w.astype(f32)
    w.flags.writeable = False
    return w


def laplacian(v):
    """(Dr^T Dr + Dc^T Dc) v, circular first differences, per plane, float64"""
    v = np.asarray(v, dtype=np.float64)
    return sum(2 * v - np.roll(v, 1, axis=ax) - np.roll(v, -1, axis=ax) for ax in (-2, -1))


@functools.lru_cache(maxsize=None)
def halves(name, Lc, rotated=False, weights="none"):
    """(A^T W A v, Lap v) in float64: the two terms every (mu, mu_reg) combines"""
    bo = oracle(name, Lc, rotated)
    v = np.asarray(vector(name, Lc, rotated)[0], dtype=np.float64)
    y = bo.forward(v)
    if weights == "weighted":
        y = y * np.asarray(data_weights(name, Lc, rotated), dtype=np.float64)
    out = bo.adjoint(y), laplacian(v)
    for a in out:
        a.flags.writeable = False
    return out


def reference(name, Lc, rotated, weights, mu, mu_reg):
    """mu A^T (w . A v) + mu_reg sum_ax (2 v - roll+ - roll-), float64"""
    ata, lap = halves(name, Lc, rotated, weights)
    return mu * ata + mu_reg * lap


# ---- the checks -------------------------------------------------------------------------------------------------------------------
MEASURES = ("rel", "max", "row", "col")


def paired(name):
    """Whether the route transforms the planes in pairs: the real passes of dft_ct (the beta axis) read the planes (l, l ^ 1) as
    one complex column a + i b and separate the two spectra afterwards (surfh_amd/csrc/dft_ct.h: loaders PLAIN / HPACK, epilogue
    HSEP)."""
    return ROUTES[name][2][1] == CT


def plane_errs(got, ref):
    """[(plane, local_errs)] of the planes whose reference is not zero.  A plane whose reference is zero has no scale of its own:
    every measure of it is infinite unless it is exactly zero, and then 0."""
    out = []
    for l in range(ref.shape[0]):
        if ref[l].any():
            out.append((l, local_errs(got[l], ref[l], PLANE_AXES)))
        else:
            n = int(np.count_nonzero(got[l]))
            out.append((l, dict({m: (np.inf if n else 0.0) for m in MEASURES}, row_at=None, col_at=None, nonzero=n)))
    return out


def worst(errs):
    """{measure: (value, plane, index)}: the worst plane of every measure"""
    out = {}
    for m in MEASURES:
        l, e = max(errs, key=lambda le: le[1][m])
        out[m] = (e[m], l, e.get(m + "_at"))
    return out


def over_tol(got, ref, tol=TOL):
    """{plane: "measure value at index; ..."} of the planes that miss ``tol`` on a measure (an all-zero plane: that is not exactly
    zero), and {measure: worst value over the planes that meet it}"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    over, within = {}, {m: 0.0 for m in MEASURES}
    for l, e in plane_errs(got, ref):
        bad = [m for m in MEASURES if not e[m] < tol]
        if "nonzero" in e and bad:
            over[l] = f"the reference is zero, {e['nonzero']} elements are not (largest {np.max(np.abs(got[l])):.3e})"
        elif bad:
            over[l] = "; ".join(f"{m} {e[m]:.3e}" + ("" if e.get(m + "_at") is None else f" at {m} {e[m + '_at']}") for m in bad)
        else:
            within = {m: max(within[m], e[m]) for m in MEASURES}
    return over, within


def check_planes(got, ref, what, tol=TOL):
    """Every per-plane measure below ``tol``, an all-zero plane exactly zero; the failure names the plane, the measure and the
    index.  Returns {measure: worst value}."""
    assert np.isfinite(np.asarray(got)).all(), f"{what}: {np.count_nonzero(~np.isfinite(got))} values are not finite"
    over, within = over_tol(got, ref, tol)
    assert not over, f"{what}: " + "; ".join(f"plane {l}: {t}" for l, t in over.items()) + f" (allowed {tol:g})"
    return within


def pair_bound(got, ref, tol=TOL, leak=PAIR_LEAK):
    """Routes that transform the planes (l, l ^ 1) together: the largest error of a plane in units of
    tol max |ref_l| + leak max |ref_partner| -- its own gate plus what the separation may leave of the partner.  Above 1 nothing is
    expected any more.  Returns (worst, its plane)."""
    got, L = np.asarray(got, dtype=np.float64), ref.shape[0]
    worst_v, worst_l = 0.0, 0
    for l in range(L):
        p = l ^ 1
        scale = tol * np.max(np.abs(ref[l])) + (leak * np.max(np.abs(ref[p])) if p < L else 0.0)
        err = float(np.max(np.abs(got[l] - ref[l])))
        v = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
        if v > worst_v:
            worst_v, worst_l = v, l
    return worst_v, worst_l


# ---- which kernels one application launches ------------------------------------------------------------------------------------
def folds(name, mu, mu_reg):
    """Whether pn_normal folds mu and the prior into the adjoint half (no scaling pass, no prior kernel): on the product loader
    whenever mu is non-zero and mu_reg / mu finite, on the other interleaved routes whenever the prior weight is non-zero -- all as the
    kernels see them, in fp32."""
    a, _, prod = ROUTES[name][2]
    if prod:
        return bool(f32(mu) != 0 and mu_reg / mu <= float(np.finfo(f32).max))
    return a != DENSE and f32(mu_reg) != 0


def expected_kernels(name, mu, mu_reg, weighted):
    """(stages that must appear with their launch counts, stages that must not) in the profile of one application"""
    a, b, prod = ROUTES[name][2]
    fold = folds(name, mu, mu_reg)
    k = {DENSE: "gemm_dft", H2: "dft_h2", CT: "dft_ct"}
    # an application is a forward and an adjoint half: two forward and two inverse transforms along each axis
    must = {"pn_prior_dot": 1, f"{k[b]}_rows_fwd": 2, f"{k[b]}_rows_inv": 2, f"{k[a]}_cols_fwd": 2}
    never = []
    if prod:                                    # the forward's OTF product rides on its inverse pass as well
        if fold and f32(mu_reg / mu) != 0:
            must.update({"dft_ct_cols_inv_prod": 1, "dft_ct_cols_inv_prodadd": 1})
        else:
            must["dft_ct_cols_inv_prod"] = 2
            never.append("dft_ct_cols_inv_prodadd")
        never += ["specmix_adj", "specmix_fwd", "dft_ct_cols_inv"]
    else:
        must.update({"specmix_fwd": 1, "specmix_adj": 1, f"{k[a]}_cols_inv": 2})
        never += ["dft_ct_cols_inv_prod", "dft_ct_cols_inv_prodadd"]
    if not fold and mu != 1.0:
        must["scale"] = 1
    else:
        never.append("scale")
    if weighted:
        must["weight_mul"] = 1
    else:
        never.append("weight_mul")
    return must, never


def check_kernels(prof, name, mu, mu_reg, weighted):
    must, never = expected_kernels(name, mu, mu_reg, weighted)
    got = {k: int(v[0]) for k, v in prof.items()}
    bad = {k: (got.get(k, 0), n) for k, n in must.items() if got.get(k, 0) != n}
    bad.update({k: (got[k], 0) for k in never if k in got})
    assert not bad, f"{name} mu {mu} mu_reg {mu_reg}: (launched, expected) {bad} in {got}"
