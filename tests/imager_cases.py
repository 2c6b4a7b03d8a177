"""The imager operator (include/surfh_amd.h: surfh_set_imager; kernels surfh_amd/csrc/imager.hip, set-up in plan_ops.hip) bin by
bin and at its edge shapes: the problems, the float64 references, the bound on G and the fault catalogue shared by
tests/test_imager_cases_host.py (no GPU) and tests/test_gpu_imager_edges.py.  Nothing here touches a GPU.

OTFs: ``broadband_psfs`` -- signed standard-normal kernels of 5 x 5 pixels, normalised by their absolute sum, through ``orc.ir2fr``.
Real point-spread functions keep the transpose exact (tests/imager_oracle.py); their |OTF| has no roll-off (median about 0.2, max
about 0.7), so every frequency bin of G weighs in every output -- under the Gaussian OTFs of ``imager_oracle.case`` the upper bins
carry less than the whole-array gate (tests/test_imager_cases_host.py records the number).

Inputs representable in fp32: the templates and an imager's own OTF are rounded once to fp32 (complex64) before the oracle and the
device get them, so the device's (float) conversions are exact; x, u and w likewise.  The plan's own OTF is the plan's fp32
rounding of the float64 ``ir2fr`` of the point-spread functions, which ``g_bound`` allows for.

PLANS: stand-alone ``Model_WCT`` plans (no channels, pce = 1) with the attachments (F, d) made on them one after the other.
Plan creation takes (48, 264) as it stands (alpha on dft_h2, beta on dft_ct; a route is decided per axis and falls
back to the dense products, no shape is refused), so ``wide_beta`` has the shape of the table.  The imager's own transforms of
the T maps and F images are the dense plane transforms on every route; the route decides the layout of the plan's OTF that
imager_build_g reads (interleaved on dft_h2 / dft_ct, planar on the dense route) and what shares the temporary with them.

  h2_T1           (40, 45)  Lc 24  T 1  (16, 4) then (1, 1)  F > T: the shared transform temporary is reallocated; F at its
                                                             maximum, T at its minimum, odd Nb, one unobserved column, a smaller
                                                             F after a larger one
  dense_T8        (20, 48)  Lc 24  T 8  (1, 3), (5, 20)      planar OTF (the route of wct_cases.dense_short_T8), T = IM_TMAX, two
                                                             unobserved rows; d = Na: one row of tiles
  h2_tiles        (40, 36)  Lc 24  T 2  (3, 36), (3, 19)     d = min(Na, Nb): one tile, 4 unobserved rows; d > Na / 2 with 17
                                                             unobserved columns; even Nb (a Nyquist bin)
  wide_beta       (48, 264) Lc 24  T 3  (5, 1), (5, 5)       Nb > 256: a second block of lanes in sample / spread / unpad; d = 5
                                                             leaves 3 rows and 4 columns unobserved, a second trip of the row
                                                             clear; F > T
  ragged_own_otf  (40, 36)  Lc 150 T 3  (3, 4), own OTF      Lc = 128 + 22: a ragged last chunk of the streamed build; filter 0
                                                             is one at plane 0, filter 1 one at plane 149, filter 2 smooth
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import imager_oracle as io  # noqa: E402
from oracle import surfh_oracle as orc  # noqa: E402

f32 = np.float32
DENSE, H2, CT = 0, 1, 2
SUPPORT = 5

# name -> shape, planes, templates, the attachments (F, d) in the order they are made, the imager brings an OTF of its own, the
# transform kernels of the plan's axes (surfh_route_decide)
PLANS = {
    "h2_T1": dict(shape=(40, 45), Lc=24, T=1, attach=((16, 4), (1, 1)), own=False, axes=(H2, H2)),
    "dense_T8": dict(shape=(20, 48), Lc=24, T=8, attach=((1, 3), (5, 20)), own=False, axes=(DENSE, DENSE)),
    "h2_tiles": dict(shape=(40, 36), Lc=24, T=2, attach=((3, 36), (3, 19)), own=False, axes=(H2, H2)),
    "wide_beta": dict(shape=(48, 264), Lc=24, T=3, attach=((5, 1), (5, 5)), own=False, axes=(H2, CT)),
    "ragged_own_otf": dict(shape=(40, 36), Lc=150, T=3, attach=((3, 4),), own=True, axes=(H2, H2)),
}
CASES = [(name, i) for name, p in PLANS.items() for i in range(len(p["attach"]))]
IDS = [f"{name}-F{PLANS[name]['attach'][i][0]}-d{PLANS[name]['attach'][i][1]}" for name, i in CASES]
CHUNKS = (None, "96", "32")              # SURFH_IMAGER_CHUNK of the streamed build: 128 + 22, 96 + 54, 32 x 4 + 22 planes


def broadband_psfs(L, rng, support=SUPPORT):
    """[L, support, support] signed standard-normal kernels, each normalised by its absolute sum"""
    k = rng.standard_normal((L, support, support))
    return k / np.abs(k).sum(axis=(1, 2), keepdims=True)


def gaussian_filters(Lc, F):
    """The overlapping Gaussians of ``imager_oracle.case``"""
    l = np.arange(Lc)
    filters = np.array([np.exp(-0.5 * ((l - c) / (Lc / 6.0)) ** 2) for c in np.linspace(Lc / 4.0, 3 * Lc / 4.0, F)])
    return filters / filters.sum(axis=1, keepdims=True)


def _seed(name):
    return 7100 + 13 * sorted(PLANS).index(name)


@functools.lru_cache(maxsize=None)
def plan(name):
    """What ``Model_WCT(psf, tpl, shape, pce)`` is given, and the float64 OTF of those point-spread functions"""
    p = PLANS[name]
    rng = np.random.default_rng(_seed(name))
    tpl = (rng.random((p["T"], p["Lc"])) + 0.1).astype(f32).astype(np.float64)
    psf = broadband_psfs(p["Lc"], rng)
    sotf = orc.ir2fr(psf, p["shape"])
    for a in (tpl, psf, sotf):
        a.flags.writeable = False
    return dict(p, name=name, tpl=tpl, psf=psf, sotf=sotf, pce=np.ones(p["Lc"]))


@functools.lru_cache(maxsize=None)
def case(name, i=0):
    """One attachment: the filters, the detector step, the OTF the imager uses, the oracle on it, maps x, a detector vector u and
    weights w with about 15 % zeros (all three representable in fp32)"""
    p = plan(name)
    F, d = p["attach"][i]
    Lc, shape = p["Lc"], p["shape"]
    rng = np.random.default_rng(_seed(name) + 1 + i)
    own = None
    if p["own"]:
        own = orc.ir2fr(broadband_psfs(Lc, rng), shape).astype(np.complex64).astype(np.complex128)      # a second set, not the plan's
        filters = gaussian_filters(Lc, F)
        filters[0], filters[1] = 0.0, 0.0
        filters[0, 0], filters[1, Lc - 1] = 1.0, 1.0
    else:
        filters = gaussian_filters(Lc, F)
    sotf = p["sotf"] if own is None else own
    im = io.ImagerOracle(sotf, p["tpl"], filters, d, shape)
    x = rng.standard_normal(im.ishape).astype(f32).astype(np.float64)
    u = rng.standard_normal(im.oshape).astype(f32).astype(np.float64)
    w = np.exp(rng.uniform(np.log(0.5), np.log(2.0), im.oshape))
    w[rng.random(im.oshape) < 0.15] = 0.0
    w = w.astype(f32).astype(np.float64)
    if w.size >= 20:
        assert np.any(w == 0)
    for a in (filters, x, u, w) + (() if own is None else (own,)):
        a.flags.writeable = False
    return dict(name=name, index=i, id=IDS[CASES.index((name, i))], F=F, T=p["T"], d=d, Lc=Lc, imshape=shape, tpl=p["tpl"], filters=filters,
                sotf=sotf, own=own, im=im, x=x, u=u, w=w)


@functools.lru_cache(maxsize=None)
def outputs(name, i=0):
    """The float64 references of one attachment, each computed once and never changed: forward(x), adjoint(u), fwadj(x) without and
    with the weights"""
    c = case(name, i)
    im = c["im"]
    out = dict(forward=im.forward(c["x"]), adjoint=im.adjoint(c["u"]), fwadj=im.fwadj(c["x"]), fwadj_weighted=im.fwadj(c["x"], c["w"]))
    for a in out.values():
        a.flags.writeable = False
    return out


FORWARD_AXES = dict(filter=0, det_row=1, det_col=2)
MAP_AXES = dict(template=0, alpha=1, beta=2)
MEASURES = {"forward": ("rel", "max") + tuple(FORWARD_AXES), "maps": ("rel", "max") + tuple(MAP_AXES)}


def axes_of(what):
    return FORWARD_AXES if what == "forward" else MAP_AXES


# ---- G -----------------------------------------------------------------------------------------------------------------------------
def g_parts(G):
    """complex [F, T, Na, nkb] -> the device's layout without its padding, [F T][2][Na][nkb]"""
    F, T, Na, nkb = G.shape
    return np.stack([G.real, G.imag], axis=2).reshape(F * T, 2, Na, nkb)


@functools.lru_cache(maxsize=None)
def g_reference(name, i=0):
    g = g_parts(case(name, i)["im"].G)
    g.flags.writeable = False
    return g


@functools.lru_cache(maxsize=None)
def g_bound(name, i=0):
    """The bound on |g - G| of every real and imaginary component [F T][2][Na][nkb], g the device's fp32 G and G ``io.build_g`` in
    float64, derived from the kernel's arithmetic (imager_build_g_kernel, imager_g_store_kernel):

    the operands are representable in fp32 (the filters stay float64 on the device), every term wf tpl sotf_component is a float64
    product and the Lc terms are added in float64, then the sum is stored as fp32 once.  So with S = sum_l |wf tpl sotf_component|
        |g - G| <= 2^-24 |G| + 2^-40 S,
    the second term covering Lc <= 256 float64 roundings of at most 2^-53 S each with a 32-fold margin (it also keeps the bound
    above zero where a component cancels exactly).  Where the imager builds G from the plan's OTF, the device holds the plan's fp32
    rounding of an OTF this file knows in float64: one rounding per term, and one more for the template against a plan that had
    not been given rounded ones,
        + 2^-23 S."""
    c = case(name, i)
    wt = np.einsum("fl,tl->ftl", c["filters"], c["tpl"])
    S = np.stack([np.einsum("ftl,lab->ftab", wt, np.abs(c["sotf"].real)), np.einsum("ftl,lab->ftab", wt, np.abs(c["sotf"].imag))], axis=2)
    S = S.reshape(g_reference(name, i).shape)
    b = 2.0 ** -24 * np.abs(g_reference(name, i)) + 2.0 ** -40 * S
    if c["own"] is None:
        b = b + 2.0 ** -23 * S
    b.flags.writeable = False
    return b


def g_excess(g, name, i=0):
    """(the largest |g - G| / bound over the components, its index (pair, part, k_alpha, k_beta)): within the bound up to 1.  A
    component whose bound is zero (an OTF component that is zero on every plane) has to be exactly zero."""
    ref, b = g_reference(name, i), g_bound(name, i)
    err = np.abs(np.asarray(g, dtype=np.float64) - ref)
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(r))
    return float(r.flat[k]), tuple(int(v) for v in np.unravel_index(k, r.shape))


# ---- faults: each the kind of error one branch of one kernel can make ----------------------------------------------------------------
G_FAULTS = ("last_kbeta", "kalpha_swap", "nyquist", "two_ulp")
OUTPUT_FAULTS = ("row_not_cleared", "short_tile")


def faulty_g(c, fault):
    """The oracle's G [F, T, Na, nkb] with one fault, or None where the case has no such bin"""
    G = c["im"].G.copy()
    Na, Nb = c["imshape"]
    if fault == "last_kbeta":                 # the last k_beta column not written
        G[..., -1] = 0.0
    elif fault == "kalpha_swap":              # the folded k_alpha rows: row Na - 1 and row 1 swapped
        G[:, :, [1, Na - 1]] = G[:, :, [Na - 1, 1]]
    elif fault == "nyquist":                  # the Nyquist bins conjugated: row Na / 2 and column Nb / 2 where the axis is even
        if Na % 2 and Nb % 2:
            return None
        if Na % 2 == 0:
            G[:, :, Na // 2] = np.conj(G[:, :, Na // 2])
        if Nb % 2 == 0:
            G[..., Nb // 2] = np.conj(G[..., Nb // 2])
    elif fault == "two_ulp":                  # the last (f, t) pair two fp32 ulps off
        G[-1, -1] *= 1.0 + 3e-7
    else:
        raise KeyError(fault)
    return G


def _from_images(im, z):
    """The adjoint's second half: the maps of F full-resolution images"""
    return np.fft.irfft2(np.einsum("ftab,fab->tab", np.conj(im.G), np.fft.rfft2(z, norm="ortho")), s=im.imshape, norm="ortho")


def faulty_output(c, fault):
    """(which output, its faulty value) in float64, or None where the case cannot show the fault"""
    im, d = c["im"], c["d"]
    Na, Nb = c["imshape"]
    _, nao, nbo = im.oshape
    xh = np.fft.rfft2(c["x"], norm="ortho")
    z = np.fft.irfft2(np.einsum("ftab,tab->fab", im.G, xh), s=im.imshape, norm="ortho")       # the images before the detector
    if fault == "row_not_cleared":            # imager_window_kernel's extra block row: the last unobserved row keeps the image
        if nao * d == Na:
            return None
        win = io.spread(np.where(c["w"] > 0, c["w"] * io.sample(z, d), 0.0), d, im.imshape)
        win[:, Na - 1, :] = z[:, Na - 1, :]
        return "fwadj_weighted", _from_images(im, win)
    if fault == "short_tile":                 # the last tile of the last row summed over (d - 1) x d pixels
        y = io.sample(z, d)
        y[:, -1, -1] -= z[:, nao * d - 1, (nbo - 1) * d:nbo * d].sum(axis=1)
        return "forward", y
    raise KeyError(fault)
