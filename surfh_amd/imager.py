"""The second instrument of the fusion: a multi-filter broadband imager on the maps of a spectrometer model
(the reference's ``instru.MSImager`` / ``WavelFilter``; its criterion classes reserve ``y_imager`` / ``mu_imager`` /
``model_imager`` for it, fusion_CT.py:68, :243-261, but ``mirim_model_for_fusion`` never shipped).

``ImagerModel`` is the operator (include/surfh_amd.h: surfh_set_imager)

    cube[l] = sum_t tpl[t,l] x[t];  blur[l] = irfft2(rfft2(cube[l]) sotf[l]);  z[f] = sum_l wf[f,l] blur[l];
    y_im[f,a,b] = sum_{i,j<d} z[f, a d + i, b d + j],   a < Na // d, b < Nb // d

evaluated on the plan of the model it is attached to: ``forward``, the exact transpose ``adjoint`` and ``fwadj``.  Row ``f`` of
``wf`` is ``WavelFilter.transmittance(wavelength_axis, normalized=True)``, the weights of ``integrate_hsi``.  Attached with
``model.set_imager(imager_model)``, its data enter ``cg`` / ``mmmg`` as a second data term (``set_imager_data``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .linop import LinOp

MAX_FILTERS = 16


def synthetic_filters(wavelength_axis, n: int) -> np.ndarray:
    """``[n, L]`` Gaussian passbands tiling the axis: centres at the middles of ``n`` equal intervals, a standard deviation of
    half an interval, each row normalised to sum 1 (the weights ``WavelFilter.transmittance(..., normalized=True)`` gives)."""
    wav = np.asarray(wavelength_axis, dtype=np.float64)
    n = int(n)
    if n < 1 or n > MAX_FILTERS:
        raise ValueError(f"the imager takes 1 to {MAX_FILTERS} filters, not {n}")
    width = (wav[-1] - wav[0]) / n if len(wav) > 1 else 1.0
    centres = wav[0] + (np.arange(n) + 0.5) * width
    f = np.exp(-0.5 * ((wav[None, :] - centres[:, None]) / (0.5 * width if width > 0 else 1.0)) ** 2)
    return f / f.sum(axis=1, keepdims=True)


def check_filters(filters, n_lambda: int) -> np.ndarray:
    """The filters as the contiguous float64 ``[F, n_lambda]`` the library takes; ``ValueError`` unless 1 <= F <= 16 and every
    value is finite and >= 0.  No library call."""
    f = np.ascontiguousarray(np.atleast_2d(np.asarray(filters, dtype=np.float64)))
    if f.ndim != 2 or f.shape[1] != n_lambda:
        raise ValueError(f"imager filters have shape {f.shape}, expected [F, {n_lambda}]")
    if not 1 <= f.shape[0] <= MAX_FILTERS:
        raise ValueError(f"the imager takes 1 to {MAX_FILTERS} filters, not {f.shape[0]}")
    if not np.all(np.isfinite(f)):
        raise ValueError("imager filters must be finite")
    if np.any(f < 0):
        raise ValueError("imager filters must be >= 0")
    return f


def decim_from_pixel(det_pix_size: float, cube_step: float) -> int:
    """Cube pixels per detector pixel; ``ValueError`` unless the ratio is within 1e-6 of an integer >= 1."""
    ratio = float(det_pix_size) / float(cube_step)
    d = int(round(ratio))
    if d < 1 or abs(ratio - d) > 1e-6:
        raise ValueError(f"imager: detector pixel {det_pix_size} is {ratio} cube steps of {cube_step}, not a whole number: give decim")
    return d


def check_decim(decim, imshape) -> int:
    d = int(decim)
    if d != decim or d < 1 or d > min(imshape):
        raise ValueError(f"imager decim must be a whole number in 1..{min(imshape)}, not {decim!r}")
    return d


class ImagerModel(LinOp):
    def __init__(self, model_or_plan, msimager_or_filters, wavelength_axis=None, decim=None):
        """``model_or_plan``: a model that owns a plan with templates (``spectroSigRLSCT``, ``Model_WCT``).
        ``msimager_or_filters``: an ``instru.MSImager`` (its ``wfilters`` are sampled on the axis, its ``sotf`` -- if not None,
        ``[L, Na, Nb//2+1]`` -- is the imager's own OTF, and ``decim`` defaults to ``det_pix_size`` over the cube step in
        arcsec) or the filter weights ``[F, L]`` themselves.  ``wavelength_axis``: the cube's (default: the model's).
        Without an OTF of its own the imager takes the model's: read from the plan where the plan owns every plane, handed in
        from ``model.sotf`` otherwise.  The operator is installed on the plan by ``model.set_imager(self)`` (or ``attach()``)."""
        m = model_or_plan
        self.model = m
        ish = tuple(m.ishape)
        if len(ish) != 3:
            raise ValueError("the imager acts on abundance maps [T, Na, Nb]")
        if getattr(m, "lmm", True) is False:
            raise ValueError("the imager needs a model with templates (it observes the cube the maps span)")
        wav = getattr(m, "wavelength_axis", None) if wavelength_axis is None else wavelength_axis
        n_lambda = int(m.cube_shape[0]) if hasattr(m, "cube_shape") else int(m.oshape[0])
        sotf = None
        if hasattr(msimager_or_filters, "wfilters"):
            ms = msimager_or_filters
            if wav is None:
                raise ValueError("an MSImager needs the wavelength axis its filters are sampled on")
            if not len(ms.wfilters):
                raise ValueError(f"the imager takes 1 to {MAX_FILTERS} filters, not 0")
            filters = np.array([f.transmittance(np.asarray(wav, dtype=np.float64), normalized=True) for f in ms.wfilters])
            sotf = ms.sotf
            if decim is None:
                decim = decim_from_pixel(ms.det_pix_size, m.step_degree * 3600)
        else:
            filters = msimager_or_filters
        self.filters = check_filters(filters, n_lambda)
        self.decim = check_decim(1 if decim is None else decim, ish[1:])
        nkb = ish[2] // 2 + 1
        if sotf is not None:
            sotf = np.ascontiguousarray(sotf, dtype=np.complex128)
            if sotf.shape != (n_lambda, ish[1], nkb):
                raise ValueError(f"imager sotf shape {sotf.shape} != {(n_lambda, ish[1], nkb)}")
        self.sotf = sotf
        super().__init__(ishape=ish, oshape=(self.filters.shape[0], ish[1] // self.decim, ish[2] // self.decim))

    # ---- plan state ---------------------------------------------------------------------------------------------------------
    def attach(self):
        """Install this imager on the model's plan (replacing the one it held; its imager data are cleared)."""
        m = self.model
        desc = _lib.ImagerDesc()
        desc.n_filters, desc.filters, desc.decim = self.filters.shape[0], _lib.dptr(self.filters), self.decim
        sotf = self.sotf
        if sotf is None and not _owns_every_plane(m):
            own = getattr(m, "sotf", None)
            if own is None:
                raise ValueError("imager: the model's plan does not own every cube plane and the model keeps no OTF to hand in")
            sotf = np.ascontiguousarray(own, dtype=np.complex128)
        desc.sotf = None if sotf is None else sotf.view(np.float64).ctypes.data_as(_lib.c_double_p)
        _lib.check(m._L.surfh_set_imager(m._plan, C.byref(desc)), ValueError)
        assert m._L.surfh_imager_osize(m._plan) == self.osize
        m._imager = self
        return self

    def _attached(self):
        if getattr(self.model, "_imager", None) is not self:
            raise RuntimeError("this ImagerModel is not the one installed on its model's plan: model.set_imager(imager) first")
        return self.model

    def _host(self, fn, x, nin, shape_out):
        m = self._attached()
        return _lib.host_call(getattr(m._L, fn), m._plan, x, nin, shape_out)

    def forward(self, maps):
        return self._host("surfh_imager_forward", maps, self.isize, self.oshape)

    def adjoint(self, y_im):
        return self._host("surfh_imager_adjoint", y_im, self.osize, self.ishape)

    def fwadj(self, x):
        """``A_im^T W_im A_im x``, ``W_im`` the weights of the imager data set on the plan (1 without)."""
        return self._host("surfh_imager_fwadj", x, self.isize, self.ishape)


def _owns_every_plane(m) -> bool:
    if not hasattr(m, "debug_buffer"):
        return True                                   # plans without detector channels own the whole cube
    lo, hi, lown, nseg = (int(v) for v in m.debug_buffer("info"))
    return nseg == 1 and lo == 0 and lown == int(m.cube_shape[0])


def check_imager_data(y_im, mu_imager, weights, osize: int):
    """``(y, w, mu)`` as the library takes them; ``ValueError`` on a wrong size, a negative or non-finite weight or
    ``mu_imager``.  No library call."""
    y = _lib.f32_vec(y_im, osize, f"imager data have {np.size(y_im)} elements, the imager {osize}")
    mu = float(mu_imager)
    if not (np.isfinite(mu) and mu >= 0):
        raise ValueError(f"mu_imager must be finite and >= 0, not {mu_imager!r}")
    w = None
    if weights is not None:
        from .weights import check_data_weights
        w = check_data_weights(weights, osize)
    return y, w, mu
