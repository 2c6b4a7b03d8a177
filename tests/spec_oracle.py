"""The solver's Fourier-domain vectors restated in float64 (NumPy only): include/surfh_amd.h, surfh_normal_spec_dev and friends.

A vector is ``[T][2 (re, im)][KAP][KBP]``: bin (ka, kb) of the unitary half spectrum ``rfft2(x, norm="ortho")`` (the convention
``build_dft`` of plan.hip encodes: exp(-i theta), 1 / sqrt(N) per axis), column kb multiplied by 1 where the bin is its own
conjugate along beta (kb = 0 or 2 kb = Nb) and by sqrt(2) elsewhere, padding (ka >= Na, kb > Nb / 2) zero.  With that factor the
plain dot product of two vectors is the dot product of the maps, and the separated circular first differences are the diagonal
``prior_eig``.  tests/test_spec_host.py holds these statements without a GPU."""
from __future__ import annotations

import numpy as np

from oracle import surfh_oracle as orc


def pad64(n):
    return (int(n) + 63) // 64 * 64


def pads(Na, Nb):
    """(KAP, KBP) of an Na x Nb image: the plan's padded spectrum pitches."""
    return pad64(Na), pad64(Nb // 2 + 1)


def col_scale(Nb):
    """[Nb // 2 + 1]: 1 on the columns that are their own conjugate, sqrt(2) on the others."""
    kb = np.arange(Nb // 2 + 1)
    return np.where((kb == 0) | (2 * kb == Nb), 1.0, np.sqrt(2.0))


def to_spec(x, KAP=None, KBP=None):
    x = np.asarray(x, dtype=np.float64)
    T, Na, Nb = x.shape
    kap, kbp = pads(Na, Nb)
    KAP, KBP = KAP or kap, KBP or kbp
    s = np.fft.rfft2(x, norm="ortho") * col_scale(Nb)
    out = np.zeros((T, 2, KAP, KBP))
    out[:, 0, :Na, : Nb // 2 + 1] = s.real
    out[:, 1, :Na, : Nb // 2 + 1] = s.imag
    return out


def from_spec(v, Na, Nb):
    v = np.asarray(v, dtype=np.float64)
    hb = Nb // 2 + 1
    s = (v[:, 0, :Na, :hb] + 1j * v[:, 1, :Na, :hb]) / col_scale(Nb)
    return np.fft.irfft2(s, s=(Na, Nb), norm="ortho")


def valid_mask(Na, Nb, KAP, KBP):
    """[KAP][KBP] bool: the bins of the half spectrum; the rest is padding."""
    m = np.zeros((KAP, KBP), dtype=bool)
    m[:Na, : Nb // 2 + 1] = True
    return m


def prior_eig(Na, Nb):
    """[Na][Nb // 2 + 1]: Dr^T Dr + Dc^T Dc of the circular first differences in the Fourier domain,
    4 sin^2(pi ka / Na) + 4 sin^2(pi kb / Nb)."""
    ka, kb = np.arange(Na)[:, None], np.arange(Nb // 2 + 1)[None, :]
    return 4.0 * np.sin(np.pi * ka / Na) ** 2 + 4.0 * np.sin(np.pi * kb / Nb) ** 2


def prior_spec(v, Na, Nb):
    """prior_eig applied to a vector (padding stays zero)."""
    out = np.zeros_like(np.asarray(v, dtype=np.float64))
    out[:, :, :Na, : Nb // 2 + 1] = prior_eig(Na, Nb) * np.asarray(v)[:, :, :Na, : Nb // 2 + 1]
    return out


def prior_maps(x):
    """The same operator on the maps, with the oracle's circular differences."""
    return orc.diff_r_t(orc.diff_r(x)) + orc.diff_c_t(orc.diff_c(x))


def normal(om, x, mu, mu_reg, KAP=None, KBP=None):
    """The vector of mu A^T A x + mu_reg (Dr^T Dr + Dc^T Dc) x for maps ``x``: the data half through the oracle model's forward and
    adjoint, the prior as the diagonal."""
    x = np.asarray(x, dtype=np.float64)
    _, Na, Nb = x.shape
    q = to_spec(mu * om.adjoint(om.forward(x)), KAP, KBP)
    return q + mu_reg * prior_spec(to_spec(x, KAP, KBP), Na, Nb) if mu_reg else q


def lcg(apply_q, b, x0, max_iter):
    """orc.lcg (qmm.lcg restated) for any symmetric operator ``apply_q`` and right-hand side ``b``: the residual is formed from
    scratch after the first step, by recurrence afterwards (refresh = 50)."""
    x = np.array(x0, dtype=np.float64, copy=True)
    r = b - apply_q(x)
    d = r.copy()
    gn = [float(np.sum(r * r))]
    for it in range(max_iter):
        q = apply_q(d)
        step = gn[-1] / float(np.sum(d * q))
        x += step * d
        r = b - apply_q(x) if it % 50 == 0 else r - step * q
        gn.append(float(np.sum(r * r)))
        d = r + (gn[-1] / gn[-2]) * d
    return {"x": x, "grad_norm": gn, "nit": max_iter}


# ---- the prior's eigenvalue of one axis as fp32 arithmetic evaluates it (emulation; fp32 cos / sin of the fp32 argument taken as
# correctly rounded) ---------------------------------------------------------------------------------------------------------------
_F = np.float32


def axis_eig_exact(N):
    k = np.arange(N)
    return 4.0 * np.sin(np.pi * k / N) ** 2


def axis_eig_cos_fp32(N):
    """2 - 2 cospif(2 k / N): cancels at low k."""
    k = np.arange(N).astype(_F)
    arg = (_F(2) * k / _F(N)).astype(_F)
    c = np.cos(np.pi * arg.astype(np.float64)).astype(_F)
    return (_F(2) - _F(2) * c).astype(_F)


def axis_eig_sin_fp32(N, fold=True):
    """4 sinpif(k' / N)^2 with k' = min(k, N - k) (``fold``): no cancellation.  Without the fold the rounding of k / N near 1 is an
    absolute error of the distance to 1 that the sine then measures: the same loss at the top of the axis."""
    k = np.arange(N)
    if fold:
        k = np.minimum(k, N - k)
    arg = (k.astype(_F) / _F(N)).astype(_F)
    s = np.sin(np.pi * arg.astype(np.float64)).astype(_F)
    return (_F(4) * s * s).astype(_F)
