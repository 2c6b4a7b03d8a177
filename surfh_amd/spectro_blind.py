"""``MRSBlurred``: the 2-D operator of the reference's deconvolution path for a ROTATED field of view
(surfh/Models/spectro_blind.py:27-416; the class scripts/deconvolution_mrs_single_wavelength.py:148 and
scripts/simulate_deconvolution_mrs_rectangle.py:149 build) evaluated by the HIP library.

    y[p, s, a] = sum_beta  w_s[beta] * boxsum_alpha(G_p C x)[alpha0 + a*srf, beta]

C = 2-D OTF multiply, G_p = bilinear interpolation of the image at the local grid of ``instr.fov + pointing`` (rotated by
``fov.angle``; pointings may be fractional; ``gridding``, :283-301), box-sum = srf consecutive alpha rows, slit window with
beta-edge weights, alpha decimation and beta sum -- the stages after G_p are those of ``spectro_blind_rectangle.MRSBlurred``
(shared in ``blurred2d``).  G_p is not a crop, so two adjoints exist: ``adjoint`` is the exact transpose (G_p^T, what the
solvers use), ``adjoint_ref`` the reference's ``MRSBlurred.adjoint`` (:212-236), whose back-projection interpolates the local
image at the image grid (``gridding_t``, :303-323) and is not G_p^T.

``sotf`` may be ``[N_alpha, N_beta/2+1]`` or ``[L, N_alpha, N_beta/2+1]`` (L independent planes evaluated as one batch).
"""
from __future__ import annotations

import numpy as np

from . import instru
from .blurred2d import Blurred2D
from .geometry import find_indices
from .spectro_blind_rectangle import QuadCriterion_MRS_2D  # noqa: F401  (criterion_2D.QuadCriterion_MRS_2D, duck-typed)


class MRSBlurred(Blurred2D):
    def __init__(self, sotf, alpha_axis, beta_axis, instr: instru.IFU, step_degree: float,
                 pointings: instru.CoordList, *, device: int = 0, stream=None):
        self._init_tables(sotf, alpha_axis, beta_axis, instr, step_degree, pointings)
        self._create_plan(device, stream)

    @classmethod
    def host_only(cls, sotf, alpha_axis, beta_axis, instr: instru.IFU, step_degree: float, pointings: instru.CoordList):
        """The model's geometry and host tables (``grid_tables``, ``gridding_t``, ``data_to_img``, ...) without a device
        plan: the operator methods are not available on it."""
        m = cls.__new__(cls)
        m._init_tables(sotf, alpha_axis, beta_axis, instr, step_degree, pointings)
        m._plan = None
        return m

    def _init_tables(self, sotf, alpha_axis, beta_axis, instr, step_degree, pointings):
        Blurred2D.__init__(self, sotf, alpha_axis, beta_axis, instr, step_degree, pointings)
        slices, weights = self._slit_tables()
        P = len(pointings)
        g = [self.grid_tables(p) for p in range(P)]
        r = [self.gridt_tables(p) for p in range(P)]
        i0, i1, y0, y1 = (np.ascontiguousarray(np.stack([t[k] for t in g]), dtype=dt)
                          for k, dt in enumerate((np.int32, np.int32, np.float64, np.float64)))
        gt = tuple(np.stack([t[k] for t in r]) for k in range(5))
        self._set_tables(slices, weights, i0, i1, y0, y1, gt=gt)

    # ---- gridding tables ------------------------------------------------------------------------------
    def grid_tables(self, p: int):
        """Bilinear taps (i0, i1, y0, y1) [na*nb] of the local grid of pointing p in the image (``gridding``, :283-301); a
        local point off the image raises like the reference's ``bounds_error=True``."""
        ga, gb = (self.instr.fov + self.pointings[p]).local2global(self.local_alpha_axis, self.local_beta_axis)
        for dim, (ax, v) in enumerate(((self.alpha_axis, ga), (self.beta_axis, gb))):
            if not (np.all(ax[0] <= v) and np.all(v <= ax[-1])):
                raise ValueError(f"pointing {p}: one of the requested xi is out of bounds in dimension {dim}")
        i0, y0 = find_indices(self.alpha_axis, ga.ravel())
        i1, y1 = find_indices(self.beta_axis, gb.ravel())
        return i0, i1, y0, y1

    def gridt_tables(self, p: int):
        """Taps (i0, i1, y0, y1, inside) [Na*Nb] of the reference's back-projection (``gridding_t``, :303-323): every image pixel
        taken into the local frame of pointing p, bilinear in the local grid, 0 outside it (``inside`` = 0)."""
        ca, cb = (self.instr.fov + self.pointings[p]).global2local(self.alpha_axis, self.beta_axis)
        ca, cb = ca.ravel(), cb.ravel()
        la, lb = self.local_alpha_axis, self.local_beta_axis
        i0, y0 = find_indices(la, ca)
        i1, y1 = find_indices(lb, cb)
        inside = ~((ca < la[0]) | (ca > la[-1]) | (cb < lb[0]) | (cb > lb[-1]))
        return i0, i1, y0, y1, inside.astype(np.uint8)

    def gridding_t(self, local_img, p: int):
        """The reference's ``gridding_t`` of a local image [na, nb] for pointing p (host, float64)."""
        t = self._tab
        i0, i1, y0, y1 = t["gt_i0"][p], t["gt_i1"][p], t["gt_y0"][p], t["gt_y1"][p]
        out = (local_img[i0, i1] * ((1.0 - y0) * (1.0 - y1)) + local_img[i0, i1 + 1] * ((1.0 - y0) * y1)
               + local_img[i0 + 1, i1] * (y0 * (1.0 - y1)) + local_img[i0 + 1, i1 + 1] * (y0 * y1))
        return np.where(t["gt_inside"][p] != 0, out, 0.0).reshape(self.imshape)

    # ---- operator -------------------------------------------------------------------------------------
    def adjoint_ref(self, data):
        """The reference's ``MRSBlurred.adjoint`` (interpolating back-projection, not the transpose of ``forward``)."""
        return self._host(self._L.surfh_adjoint_ref, data, self.osize, self.ishape)

    def fwadj(self, x):
        """A^T A x (exact transpose) in one call."""
        return self._host(self._L.surfh_fwadj, x, self.isize, self.ishape)

    def cg(self, data, mu=1.0, mu_reg=0.0, x0=None, max_iter=10, tol=1e-12, refresh=50, callback=None):
        """Device-resident linear CG on  mu |y - A x|^2 + mu_reg (|Dr x|^2 + |Dc x|^2), one problem per plane, as
        ``spectro_blind_rectangle.MRSBlurred.cg``.  The normal operator uses the exact transpose A^T (as
        ``spectroSigRLSCT.cg`` does), not the reference's ``adjoint``: the reference's ``lcg`` on its non-transpose pair is
        not reproduced."""
        return super().cg(data, mu, mu_reg, x0, max_iter, tol, refresh, callback)

    def mmmg(self, data, mu=1.0, mu_reg=0.0, x0=None, max_iter=10, tol=1e-12, refresh=50, callback=None, delta=None, weights=None,
             potential="huber", coupling="none"):
        """Device-resident 3MG on the criterion of ``cg``, with the exact transpose likewise; ``delta``: Huber priors (or those of
        ``potential``), per-plane ``mu_reg`` / ``delta`` arrays, ``coupling`` ("none" or "isotropic") and
        ``weights``, as ``Blurred2D.mmmg``."""
        return super().mmmg(data, mu, mu_reg, x0, max_iter, tol, refresh, callback, delta=delta, weights=weights, potential=potential,
                            coupling=coupling)

    # ---- reference helpers on the host ------------------------------------------------------------------
    def data_to_img(self, data):
        """The reference's quick-look back-projection of slit data (spectro_blind.py:238-281; called by
        scripts/deconvolution_mrs_single_wavelength.py:159,194 and scripts/simulate_deconvolution_mrs_rectangle.py:193): every
        sample divided by ``npix_slit_beta_width * srf`` and spread over its slit's beta columns on the local grid, the
        transposed box, values below 1 zeroed, local columns 5 / 153 overwritten by 6 / 152, then the interpolating
        ``gridding_t`` into the image.  A pixel counts for the mean where a pointing's back-projection exceeds 100.  Returns
        ``(weighted_mean, global_img)``, the mean 0 where no pointing counts (the reference leaves those entries
        uninitialised).  Host NumPy: a plotting aid on one image, not part of the operator."""
        d = self._d2i_data(data)
        scale = self.npix_slit_beta_width * self.srf
        cum = np.stack([self.gridding_t(self._d2i_local(d, p, scale), p) for p in range(len(self.pointings))])
        valid = np.sum(cum > 100, axis=0)
        total = np.sum(cum, axis=0)
        return np.divide(total, valid, out=np.zeros(self.imshape), where=valid != 0), total

    def real_data_janskySR_to_jansky(self, data):
        """Raw 2-D slit data from Jy/sr to Jy (spectro_blind.py:406-416): every slit's samples times the sum of its beta
        weights and srf.  Works on (and returns) a flat copy."""
        d = np.array(data, dtype=np.float64).reshape(self.slices_shape)
        for s in range(self.slices_shape[1]):
            w = self.get_slit_weights(s, self.get_slit_slices(s))
            d[:, s, :] = d[:, s, :] * np.sum(w[0, 0, :]) * self.srf
        return d.ravel()
