"""Per-sample data weights of the solvers: the criterion is ``J(x) = mu (y - A x)^T W (y - A x) / 2 + priors`` with
``W = diag(w)``, ``w`` ``[osize]`` in the layout of ``y``, every ``w[i]`` finite and >= 0 -- a 0/1 mask of bad samples, an inverse
variance ``1 / sigma^2``, or their product.  The weights are state of the plan (include/surfh_amd.h: surfh_set_data_weights); this
module holds what the Python classes share: the argument check, the plan-state methods, and the host-side helpers."""
from __future__ import annotations

import numpy as np

from . import _lib


def check_data_weights(weights, osize: int) -> np.ndarray:
    """The weights as the contiguous float32 vector the library takes.  ``ValueError`` unless they have ``osize`` elements, all
    finite (in float32 too) and >= 0.  No library call."""
    w = np.asarray(weights)
    if w.size != osize:
        raise ValueError(f"data weights have {w.size} elements, the data {osize}")
    with np.errstate(over="ignore"):
        w = np.ascontiguousarray(w.reshape(-1), dtype=np.float32)
    if not np.all(np.isfinite(w)):
        raise ValueError("data weights must be finite")
    if np.any(w < 0):
        raise ValueError("data weights must be >= 0")
    return w


def weights_from_data(y, sigma=None):
    """``(y_clean, w)`` for real exposures: where ``y`` is not finite (NaN samples, bad pixels flagged as NaN or Inf) ``w = 0`` and
    ``y_clean = 0``; elsewhere ``w = 1``, or the inverse variance ``1 / sigma^2`` when ``sigma`` (a scalar, or an array of y's
    shape) is given.  A non-positive or non-finite ``sigma`` gives weight 0 too.  Both results have y's shape, float64."""
    y = np.asarray(y, dtype=np.float64)
    good = np.isfinite(y)
    w = good.astype(np.float64)
    if sigma is not None:
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), y.shape)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = 1.0 / (sg * sg)
        ok = good & np.isfinite(sg) & (sg > 0) & np.isfinite(inv)
        w = np.where(ok, inv, 0.0)
    return np.where(good, y, 0.0), w


def weighted_sq_residual(y, ax, weights=None):
    """``sum w (y - A x)^2`` in float64, the data of weight 0 ignored whatever they hold (``weights=None``: ``sum (y - A x)^2``)."""
    y, ax = np.asarray(y, dtype=np.float64).ravel(), np.asarray(ax, dtype=np.float64).ravel()
    if weights is None:
        return np.sum((y - ax) ** 2)
    w = np.asarray(weights, dtype=np.float64).ravel()
    keep = w > 0
    return np.sum(w[keep] * (y[keep] - ax[keep]) ** 2)


class DataWeights:
    """The plan-state methods of a ``PlanOwner`` (``self.osize``)."""
    _data_weights = None

    def set_data_weights(self, weights=None):
        """Per-sample weights ``w`` ``[osize]`` of the data term (see the module).  Plan state, like the prior: the solvers and
        the normal operators of this model use them from now on; a sample of weight 0 contributes nothing whatever its datum,
        NaN included.  ``forward`` / ``adjoint`` stay ``A`` / ``A^T``.  ``None`` clears them.  ``ValueError`` on a wrong size, a
        negative or a non-finite weight."""
        w = None if weights is None else check_data_weights(weights, self.osize)
        _lib.check(self._L.surfh_set_data_weights(self._plan, None if w is None else _lib.fptr(w)))
        self._data_weights = w

    @property
    def data_weights(self):
        """The weights ``set_data_weights`` installed last (float32 ``[osize]``, a copy), or None."""
        return None if self._data_weights is None else self._data_weights.copy()

    def installed_weights(self, weights):
        """``with model.installed_weights(w):`` -- a solve inside runs under ``w``, and what the plan held before is put back
        afterwards.  ``None`` leaves the plan's state alone.  The check of ``w`` comes before any library call."""
        return _Installed(self, weights)


class _Installed:
    def __init__(self, model, weights):
        self.model = model
        self.w = None if weights is None else check_data_weights(weights, model.osize)

    def __enter__(self):
        if self.w is not None:
            self.saved = self.model.data_weights
            self.model.set_data_weights(self.w)

    def __exit__(self, *exc):
        if self.w is not None:
            self.model.set_data_weights(self.saved)
        return False
