"""Reconstruction algorithms of surfh/ToolsDir/algorithms.py on the library's device-resident solvers.

``lmm_reconstruction`` (algorithms.py:73-106) minimises, over the abundance maps x of the linear mixing model,

    J(x) = |y - A x|^2 / 2  +  spat_reg * sum_k sum_pixels phi(D_k x),   k in {rows, columns}

with phi the Huber potential of threshold ``spat_th`` (qmm.Huber): the reference hands qmm.mmmg one quadratic data objective
and two Huber objectives on aljabr.Diff(0) / aljabr.Diff(1).  Here the same criterion runs through
``spectroSigRLSCT.mmmg(..., delta=spat_th)`` (include/surfh_amd.h: surfh_mmmg_huber).

Parity is unpinned on two counts: qmm is not available to check the 3MG restatement against, and neither is aljabr, so
``aljabr.Diff``'s border and axis conventions are not known here -- the circular spatial differences of fusion_CT.py:16-43
(NpDiff_r / NpDiff_c) are used instead.
"""
from __future__ import annotations

import time

from .fusion import OptimizeResult


def lmm_reconstruction(data, data_model, spat_reg: float = 1.0, spat_th: float = 1.0, init=None, max_iter: int = 500,
                       tol: float = 1e-4, callback=None) -> OptimizeResult:
    """Edge-preserving reconstruction of the abundance maps (algorithms.py:73-106).

    ``data_model`` is a template model (``spectroSigRLSCT``); ``init=None`` starts from ``data_model.adjoint(data)``, the exact
    transpose applied to the data (qmm's ``ht_data``, read the same way ``QuadCriterion_MRS`` reads the data term).
    ``max_iter`` = 500 as the reference; ``tol`` = 1e-4 is qmm.mmmg's default, applied as the library's 3MG stopping test
    |grad| < size * tol.  ``callback(it, grad_norm, x)`` as ``spectroSigRLSCT.mmmg``; a truthy return stops.
    Returns the ``OptimizeResult`` of ``fusion.py`` (x raveled, |grad| of every iterate)."""
    if init is None:
        init = data_model.adjoint(data)
    t0 = time.time()
    x, gn, nit = data_model.mmmg(data, mu=1.0, mu_reg=float(spat_reg), x0=init, max_iter=int(max_iter), tol=float(tol),
                                 callback=callback, delta=float(spat_th))
    return OptimizeResult(x=x.ravel(), grad_norm=list(gn), nit=nit, success=bool(gn[-1] < x.size * tol), time=time.time() - t0)
