"""Float64 restatement of the rotated-field 2-D operator ``MRSBlurred`` (the reference's surfh/Models/spectro_blind.py:27-416),
composed from the checker's primitives (oracle/surfh_oracle.py is not changed), and the problems its tests share.

    y[p, s, a] = sum_beta  w_s[beta] * boxsum_alpha(G_p C x)[alpha0 + a*srf, beta]

G_p = bilinear interpolation of the image at the rotated local grid of pointing p (``gridding``, :283-301).  The exact adjoint
uses G_p^T; the reference's own adjoint (:212-236) uses the interpolating back-projection R_p (``gridding_t``, :303-323: the image
grid taken into the local frame, bilinear, 0 outside), which is not G_p^T.  ``data_to_img`` is :238-281.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import surfh_oracle as orc  # noqa: E402

STEP = 0.025                 # arcsec
STEP_DEG = STEP / 3600.0


def _bilinear_matrix(i0, i1, y0, y1, n_cols, n_beta, keep=None):
    """Rows = sample points, columns = flat pixels of an [., n_beta] grid; the four weights of ``orc.bilinear_apply``."""
    n = len(i0)
    keep = np.ones(n, dtype=bool) if keep is None else keep
    rows, cols, vals = [], [], []
    for di, dj, w in ((0, 0, (1 - y0) * (1 - y1)), (0, 1, (1 - y0) * y1), (1, 0, y0 * (1 - y1)), (1, 1, y0 * y1)):
        rows.append(np.arange(n)[keep])
        cols.append(((i0 + di) * n_beta + (i1 + dj))[keep])
        vals.append(w[keep])
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n_cols))


class RotatedOracle(orc.BlurredOracle):
    """Slit windows, weights, box sum and decimation as ``orc.BlurredOracle`` (the two reference files share them); the
    gridding is bilinear at the rotated local grid.  ``sotf`` may carry a leading axis of independent planes."""

    def __init__(self, sotf, alpha_axis, beta_axis, spec: orc.ChannelSpec, step_degree, pointings):
        super().__init__(sotf, alpha_axis, beta_axis, spec, step_degree, pointings)
        del self.crops
        na, nb = len(self.la), len(self.lb)
        Na, Nb = self.ishape
        self.grid, self.gridt, self.taps = [], [], []
        for p in self.pointings:
            org = (spec.origin[0] + p[0], spec.origin[1] + p[1])
            ga, gb = orc.local2global(self.la, self.lb, spec.angle, org)
            for dim, (ax, v) in enumerate(((self.alpha_axis, ga), (self.beta_axis, gb))):
                if not (np.all(ax[0] <= v) and np.all(v <= ax[-1])):
                    raise ValueError("One of the requested xi is out of bounds in dimension %d" % dim)
            i0, y0 = orc.find_indices(self.alpha_axis, ga.ravel())
            i1, y1 = orc.find_indices(self.beta_axis, gb.ravel())
            self.taps.append((i0, i1, y0, y1))
            self.grid.append(_bilinear_matrix(i0, i1, y0, y1, Na * Nb, Nb))                   # [na*nb, Na*Nb]
            ca, cb = orc.global2local(self.alpha_axis, self.beta_axis, spec.angle, org)
            ca, cb = ca.ravel(), cb.ravel()
            j0, z0 = orc.find_indices(self.la, ca)
            j1, z1 = orc.find_indices(self.lb, cb)
            inside = ~((ca < self.la[0]) | (ca > self.la[-1]) | (cb < self.lb[0]) | (cb > self.lb[-1]))
            self.gridt.append(_bilinear_matrix(j0, j1, z0, z1, na * nb, nb, inside))         # [Na*Nb, na*nb]

    def gridding(self, img, p):
        """``gridding`` of one pointing on [L, Na, Nb] -> [L, na, nb] (the reference's own sum order)."""
        i0, i1, y0, y1 = self.taps[p]
        return orc.bilinear_apply(img, i0, i1, y0, y1).reshape(img.shape[0], len(self.la), len(self.lb))

    def _slit_backproject(self, d, p, scale=1.0):
        """slicing_t of every slit's samples (spread over the slit's beta columns, placed every srf rows) on the local grid."""
        L = d.shape[0]
        local = np.zeros((L, len(self.la), len(self.lb)))
        for s, (sa0, sa1, sb0, sb1) in enumerate(self.slit_slices):
            over = np.repeat(d[:, p, s][:, :, None], self.npix_b, axis=2) / scale
            bts = np.zeros((L, sa1 - sa0, sb1 - sb0))
            bts[:, : self.n_out * self.srf: self.srf, :] = over
            local[:, sa0:sa1, sb0:sb1] += bts * self.slit_weights[s][None]
        return local

    def forward(self, x):
        x = np.asarray(x, dtype=np.float64)
        xb = x if self.batched else x[None]
        sf = self.sotf if self.batched else self.sotf[None]
        blurred = orc.idft(orc.dft(xb) * sf, self.ishape)
        out = np.zeros((xb.shape[0],) + self.slices_shape)
        for p in range(len(self.pointings)):
            ss = self._box(self.gridding(blurred, p))
            for s, (sa0, sa1, sb0, sb1) in enumerate(self.slit_slices):
                sl = ss[:, sa0:sa1, sb0:sb1] * self.slit_weights[s][None]
                out[:, p, s] = np.sum(sl[:, : self.n_out * self.srf: self.srf], axis=2)
        out = out.reshape(xb.shape[0], -1)
        return out if self.batched else out[0]

    def _adjoint(self, data, mats):
        L = self.sotf.shape[0] if self.batched else 1
        d = np.asarray(data, dtype=np.float64).reshape((L,) + self.slices_shape)
        g = np.zeros((L, int(np.prod(self.ishape))))
        for p in range(len(self.pointings)):
            st = self._box(self._slit_backproject(d, p), t=True).reshape(L, -1)
            g += np.asarray(mats(p) @ st.T).T
        sf = self.sotf if self.batched else self.sotf[None]
        out = orc.idft(orc.dft(g.reshape((L,) + self.ishape)) * sf.conj(), self.ishape)
        return out if self.batched else out[0]

    def adjoint(self, data):
        """The exact transpose of ``forward`` (G_p^T)."""
        return self._adjoint(data, lambda p: self.grid[p].T)

    def adjoint_ref(self, data):
        """The reference's ``MRSBlurred.adjoint`` (:212-236): the interpolating back-projection R_p."""
        return self._adjoint(data, lambda p: self.gridt[p])

    def data_to_img(self, data):
        """``MRSBlurred.data_to_img`` (:238-281): samples / (npix_slit_beta_width * srf) spread on the local grid, the transposed
        box, values below 1 zeroed, local columns 5 <- 6 and 153 <- 152, interpolating back-projection; a pixel counts for the
        mean where a pointing's back-projection exceeds 100.  Returns (mean, sum over pointings), the mean 0 where no pointing
        counts (uninitialised in the reference)."""
        if self.batched:
            raise ValueError("data_to_img is defined for a single image")
        d = np.asarray(data, dtype=np.float64).reshape((1,) + self.slices_shape)
        cum = np.zeros((len(self.pointings),) + self.ishape)
        for p in range(len(self.pointings)):
            st = self._box(self._slit_backproject(d, p, self.npix_b * self.srf), t=True)[0]
            st[st < 1] = 0
            st[:, 5] = st[:, 6]
            st[:, 153] = st[:, 152]
            cum[p] = (self.gridt[p] @ st.ravel()).reshape(self.ishape)
        valid = np.sum(cum > 100, axis=0)
        total = np.sum(cum, axis=0)
        return np.divide(total, valid, out=np.zeros(self.ishape), where=valid != 0), total


class PlaneOp:
    """One plane of a 2-D oracle presented as a [1, N, N] operator (the checker's lcg / mmmg and priors act on [T, N, N])."""

    def __init__(self, op):
        self.op = op

    def forward(self, x):
        return self.op.forward(x[0])

    def adjoint(self, y):
        return self.op.adjoint(y)[None]


# ---- the problems of the fixtures (tests/golden/make_golden_rotated.py) and of the tests ------------------------------------
def _axes(N):
    return orc.synthetic_axes(N, STEP_DEG)


def small_case(L=None, N=96, angle=20.0):
    """96 x 96 image, 12 slits, field of view at ``angle`` degrees, three pointings, two of them fractional."""
    s = STEP_DEG
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), angle, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    wav = np.array([7.6]) if L is None else np.linspace(7.0, 8.2, L)
    sotf = orc.ir2fr(orc.gaussian_psf(wav, STEP), (N, N))
    return dict(spec=spec, sotf=sotf[0] if L is None else sotf, alpha_axis=_axes(N), beta_axis=_axes(N), step_deg=s,
                pointings=[(0.0, 0.0), (2.3 * s, -3.1 * s), (-4.6 * s, 1.7 * s)], imshape=(N, N), x_seed=23, u_seed=24)


def d2i_case():
    """Band-1C field of view at 8.2 degrees (the reference scripts' 8.2 - rotation_ref with rotation_ref = 0), 251 x 251 image,
    four pointings; the image is scaled along beta so that both thresholds of ``data_to_img`` (1 and 100) cut pixels."""
    N, s = 251, STEP_DEG
    spec = orc.ChannelSpec(3.2 / 3600, 3.7 / 3600, (0.0, 0.0), 8.2, 0.196, 21, 3355.0, np.linspace(6.6, 7.6, 10), "1C")
    sotf = orc.ir2fr(orc.gaussian_psf(np.array([7.0]), STEP), (N, N))[0]
    return dict(spec=spec, sotf=sotf, alpha_axis=_axes(N), beta_axis=_axes(N), step_deg=s,
                pointings=[(0.0, 0.0), (5.4 * s, -7.2 * s), (-9.3 * s, 4.6 * s), (3.7 * s, 8.1 * s)], imshape=(N, N),
                x_seed=33, x_scale=np.linspace(0.0, 400.0, N)[None, :])


def oracle_of(case, sotf=None):
    return RotatedOracle(case["sotf"] if sotf is None else sotf, case["alpha_axis"], case["beta_axis"], case["spec"],
                         case["step_deg"], case["pointings"])
