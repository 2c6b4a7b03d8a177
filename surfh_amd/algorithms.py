"""Reconstruction algorithms of surfh/ToolsDir/algorithms.py on the library's device-resident solvers.

``lmm_reconstruction`` (algorithms.py:73-106) minimises, over the abundance maps x of the linear mixing model,

    J(x) = |y - A x|^2 / 2  +  spat_reg * sum_k sum_pixels phi(D_k x),   k in {rows, columns}

with phi the Huber potential of threshold ``spat_th`` (qmm.Huber): the reference hands qmm.mmmg one quadratic data objective
and two Huber objectives on aljabr.Diff(0) / aljabr.Diff(1).  Here the same criterion runs through
``spectroSigRLSCT.mmmg(..., delta=spat_th)`` (include/surfh_amd.h: surfh_mmmg_huber).

``vox_reconstruction`` (algorithms.py:27-71) minimises the same kind of criterion over the hyperspectral cube x itself, without
templates, with a third Huber objective on the spectral differences:

    J(x) = |y - A x|^2 / 2  +  spat_reg * sum_{k in rows, columns} sum phi_spat_th(D_k x)  +  spec_reg * sum phi_spec_th(D_l x)

through ``spectroSigRLSCT.mmmg_vox`` (include/surfh_amd.h: surfh_mmmg_huber_vox).  The reference's legacy ``Spectro`` model is
``(alpha, beta, lambda)``, hence its ``Diff(0) / Diff(1) / Diff(2)``; the cube here is ``[lambda][alpha][beta]``.  The spectral
difference ``D_l x = x[l+1] - x[l]`` is open (``Lc - 1`` difference planes): a wrap would tie the shortest to the longest
wavelength of the cube, which means nothing physically.

Parity is unpinned on two counts: qmm is not available to check the 3MG restatement against, and neither is aljabr, so
``aljabr.Diff``'s border and axis conventions are not known here -- the circular spatial differences of fusion_CT.py:16-43
(NpDiff_r / NpDiff_c) are used instead, and the open spectral difference above.
"""
from __future__ import annotations

import time

import numpy as np

from . import potentials as _pot
from .fusion import OptimizeResult, robust_data_value
from .weights import weighted_sq_residual


def lmm_reconstruction(data, data_model, spat_reg: float = 1.0, spat_th: float = 1.0, init=None, max_iter: int = 500,
                       tol: float = 1e-4, callback=None, weights=None, data_th=None, spat_potential="huber",
                       data_potential="huber", coupling="none") -> OptimizeResult:
    """Edge-preserving reconstruction of the abundance maps (algorithms.py:73-106).

    ``data_model`` is a template model (``spectroSigRLSCT``); ``init=None`` starts from ``data_model.adjoint(data)``, the exact
    transpose applied to the data (qmm's ``ht_data``, read the same way ``QuadCriterion_MRS`` reads the data term).
    ``max_iter`` = 500 as the reference; ``tol`` = 1e-4 is qmm.mmmg's default, applied as the library's 3MG stopping test
    |grad| < size * tol.  ``callback(it, grad_norm, x)`` as ``spectroSigRLSCT.mmmg``; a truthy return stops.
    ``weights`` (not in the reference): per-sample data weights ``[osize]``, data term (y - A x)^T diag(w) (y - A x) / 2
    (``spectroSigRLSCT.set_data_weights``); the default start is then ``A^T (w y)``, masked data left out.
    ``data_th`` (not in the reference): Huber threshold of a robust data term, sum_i phi(sqrt(w_i) (y_i - (A x)_i)) instead of the
    quadratic one (``spectroSigRLSCT.mmmg(data_delta=...)``); ``None``: quadratic.
    ``spat_potential`` / ``data_potential`` (the reference builds qmm.Huber; qmm takes any potential): "huber", "hyperbolic" or
    "hebert_leahy" (``surfh_amd.potentials``) under ``spat_th`` and ``data_th``; a data potential other than Huber needs ``data_th``.
    ``coupling`` (not in the reference): "none", "isotropic" or "vector" -- which differences share one potential, ``spat_th`` then
    the threshold on the group magnitude (``spectroSigRLSCT.mmmg(coupling=...)``).
    Returns the ``OptimizeResult`` of ``fusion.py`` (x raveled, |grad| of every iterate)."""
    if init is None:
        init = _weighted_start(data, data_model, weights)
    t0 = time.time()
    x, gn, nit = data_model.mmmg(data, mu=1.0, mu_reg=float(spat_reg), x0=init, max_iter=int(max_iter), tol=float(tol),
                                 callback=callback, delta=float(spat_th), weights=weights, potential=spat_potential,
                                 data_potential=data_potential, coupling=coupling, **_robust_kw(data_th))
    return OptimizeResult(x=x.ravel(), grad_norm=list(gn), nit=nit, success=bool(gn[-1] < x.size * tol), time=time.time() - t0)


def vox_reconstruction(data, data_model, spat_reg: float = 1.0, spat_th: float = 1.0, spec_reg: float = 1.0, spec_th: float = 1.0,
                       init=None, max_iter: int = 500, tol: float = 1e-4, callback=None, weights=None, data_th=None,
                       spat_potential="huber", spec_potential="huber", data_potential="huber") -> OptimizeResult:
    """Edge-preserving reconstruction of the hyperspectral cube (algorithms.py:27-71).

    ``data_model`` is a model without templates (``spectroSigRLSCT(sotf, None, ...)``); ``init=None`` starts from
    ``data_model.adjoint(data)`` (qmm's ``ht_data``).  ``max_iter``, ``tol``, ``callback``, ``weights``, ``data_th`` and the result as
    ``lmm_reconstruction``; x is the raveled cube ``[Lc, Na, Nb]``.  ``spat_potential`` / ``spec_potential`` / ``data_potential``:
    the potentials under ``spat_th``, ``spec_th`` and ``data_th``, as ``lmm_reconstruction``'s."""
    if init is None:
        init = _weighted_start(data, data_model, weights)
    t0 = time.time()
    x, gn, nit = data_model.mmmg_vox(data, mu=1.0, spat_reg=float(spat_reg), spat_delta=float(spat_th), spec_reg=float(spec_reg),
                                     spec_delta=float(spec_th), x0=init, max_iter=int(max_iter), tol=float(tol), callback=callback,
                                     weights=weights, spat_potential=spat_potential, spec_potential=spec_potential,
                                     data_potential=data_potential, **_robust_kw(data_th))
    return OptimizeResult(x=x.ravel(), grad_norm=list(gn), nit=nit, success=bool(gn[-1] < x.size * tol), time=time.time() - t0)


def vox_criterion(data, data_model, x, spat_reg: float = 1.0, spat_th: float = 1.0, spec_reg: float = 1.0, spec_th: float = 1.0,
                  mu: float = 1.0, weights=None, data_th=None, spat_potential="huber", spec_potential="huber",
                  data_potential="huber") -> float:
    """J(x) of ``vox_reconstruction`` at the cube ``x`` (``mu`` weighs the data term, 1 in the reference): the forward model and
    the two prior sums run on the device (``huber_vox_prior_dev``), the data term is summed in float64 on the host -- under
    ``weights`` as sum w (y - A x)^2 over the samples with w > 0, with ``data_th`` as the robust term mu sum phi(sqrt(w) (y - A x)).
    The potentials as ``vox_reconstruction``'s."""
    _pot.need_delta(data_potential, data_th, "data_th")
    import torch
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(data_model.ishape))
    dev = f"cuda:{data_model.device}"
    x_t = torch.as_tensor(x, device=dev)
    g_t = torch.zeros_like(x_t)
    torch.cuda.synchronize(dev)
    with _pot.installed(data_model, spatial=spat_potential, spectral=spec_potential):
        v_spat, v_spec = data_model.huber_vox_prior_dev(x_t, g_t, 0.0, spat_th, 0.0, spec_th)
    if data_th is not None:
        data_term = mu * robust_data_value(data, data_model.forward(x), weights, float(data_th), data_potential)
    else:
        data_term = mu * weighted_sq_residual(data, data_model.forward(x), weights) / 2
    return float(data_term + spat_reg * v_spat + spec_reg * v_spec)


def _robust_kw(data_th):
    """``data_delta`` for the solvers, only when a robust data term is asked for."""
    return {} if data_th is None else {"data_delta": float(data_th)}


def _weighted_start(data, data_model, weights):
    """The default start ``A^T y``, or ``A^T (w y)`` with the data of weight 0 left out (they may be NaN)."""
    if weights is None:
        return data_model.adjoint(data)
    w = np.asarray(weights, dtype=np.float64).ravel()
    y = np.asarray(data, dtype=np.float64).ravel()
    return data_model.adjoint(np.where(w > 0, w * np.where(w > 0, y, 0.0), 0.0))
