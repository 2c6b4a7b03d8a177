"""Weighted least squares as ordinary least squares, for the float64 oracles: with W = diag(w), w >= 0,

    mu (y - A x)^T W (y - A x) / 2  =  mu |y~ - A~ x|^2 / 2,   A~ = W^(1/2) A,   y~ = W^(1/2) y.

``Weighted`` wraps any oracle model (``forward``, ``adjoint``, ``ishape``, ``oshape``) as A~; the wrapped model and ``wdata(w, y)``
go into the unchanged ``orc.lcg``, ``orc.mmmg``, ``huber_oracle.mmmg``, ``vox_oracle.mmmg`` and ``orc.crit_val``.  ``standard`` is the
weighted problem the tests share."""
from __future__ import annotations

import numpy as np


class Weighted:
    def __init__(self, op, w):
        self.op = op
        self.ishape, self.oshape = tuple(op.ishape), tuple(op.oshape)
        self.sw = np.sqrt(np.asarray(w, dtype=np.float64)).reshape(self.oshape)

    @property
    def isize(self):
        return int(np.prod(self.ishape))

    @property
    def osize(self):
        return int(np.prod(self.oshape))

    def forward(self, x):
        return self.sw * self.op.forward(x)

    def adjoint(self, y):
        return self.op.adjoint(self.sw * np.asarray(y, dtype=np.float64).reshape(self.oshape))

    def matvec(self, x):
        return self.forward(x.reshape(self.ishape)).ravel()

    def rmatvec(self, y):
        return self.adjoint(y.reshape(self.oshape)).ravel()


def wdata(w, y):
    """y~ = sqrt(w) y, 0 where w = 0 whatever y holds there (a select: 0 * NaN is NaN)."""
    w = np.asarray(w, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(w.shape)
    keep = w > 0
    return np.where(keep, np.sqrt(w) * np.where(keep, y, 0.0), 0.0)


def recipe(y_true, y_clean, seed=2):
    """From default_rng(seed): w = exp(U(log 0.5, log 2)); the samples where random() < 0.12 get w = 0 and their data are
    replaced by 1e3 max |y_true|.  Returns (w, y_spiked, masked)."""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(np.log(0.5), np.log(2.0), y_clean.shape))
    masked = rng.random(y_clean.shape) < 0.12
    w[masked] = 0.0
    y_spiked = np.where(masked, 1e3 * np.max(np.abs(y_true)), y_clean)
    return w, y_spiked, masked


MU, MUR, NIT = 1.0, 5e3, 12          # of test_cg_matches_oracle_lcg


def standard(cfg, om):
    """The standard weighted problem: ``cfg`` with noise 1e-2 rms from seed 1 (as test_cg_matches_oracle_lcg), and ``recipe``.
    Returns dict(y_clean, y, w, masked)."""
    y_true = om.forward(cfg["maps"])
    y_clean = y_true + np.random.default_rng(1).standard_normal(y_true.size) * 1e-2 * np.sqrt(np.mean(y_true ** 2))
    w, y, masked = recipe(y_true, y_clean)
    return dict(y_clean=y_clean, y=y, w=w, masked=masked)
