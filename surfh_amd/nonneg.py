"""Non-negative fusion: ``min x^T Q x / 2 - b^T x`` subject to ``x >= 0`` with the ``Q`` and ``b`` of ``cg`` (or of ``cg_templates``), by
ADMM in scaled form around the CG frame (include/surfh_amd.h: surfh_cg_nonneg; the kernels: csrc/nonneg.hip).

``x`` solves ``(Q + rho I) x = b + rho (z - u)`` by ``inner`` CG iterations on the residual carried over from the outer iteration
before, ``z = max(x + u, 0)`` is the feasible iterate and the result, ``u`` the scaled dual.  Every map of the scheme is Lipschitz,
so a float32 run follows its float64 restatement (tests/nonneg_oracle.py) iterate by iterate.  Convergence is what ADMM gives on an
ill-conditioned ``Q``: steady, not fast -- tens of outer iterations bring the criterion down, the traces tell how far the run got.
The penalty is fixed for a run; there is no residual balancing.  This module holds what the Python classes share: the result type,
the argument checks, and the methods of a model with templates that owns a plan."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _lib


class NonnegResult(NamedTuple):
    """``x``: the feasible iterate ``z`` (min >= 0 exactly).  One trace entry for the start and one per outer iteration run:
    ``primal`` ``|x - z|``, ``dual`` ``rho |z - z_previous|`` (0 at the start), ``grad_norm`` ``|r|`` of the next inner system,
    ``n_active`` the number of entries of ``z`` at 0.  ``rho``: the penalty used; ``nit``: outer iterations run.  The plane-wise
    solver (``Blurred2D.cg_nonneg``) returns every trace per plane, ``[nit+1, n_planes]``, and ``rho`` as the array ``[n_planes]``."""
    x: np.ndarray
    primal: np.ndarray
    dual: np.ndarray
    grad_norm: np.ndarray
    n_active: np.ndarray
    rho: float
    nit: int


def check_nonneg_args(rho, outer, inner, refresh=0, what="cg_nonneg"):
    """``ValueError`` for a penalty that is not finite and > 0 (None passes: it asks for the estimate), ``inner < 1``, ``outer < 0``,
    ``refresh < 0``.  No library call."""
    if rho is not None and not (np.isfinite(rho) and rho > 0):
        raise ValueError(f"{what}: rho = {rho!r} must be finite and > 0 (None: the estimate of nonneg_rho)")
    if int(inner) < 1:
        raise ValueError(f"{what}: inner = {inner} (at least one CG iteration per outer iteration)")
    if int(outer) < 0:
        raise ValueError(f"{what}: outer = {outer}")
    if int(refresh) < 0:
        raise ValueError(f"{what}: refresh = {refresh}")


def result_from_trace(x, trace, rho, nit) -> NonnegResult:
    t = trace[: nit + 1]
    return NonnegResult(x, np.sqrt(t[:, 0]), np.sqrt(t[:, 1]), np.sqrt(t[:, 2]), np.rint(t[:, 3]).astype(np.int64), float(rho), int(nit))


def result_from_planes_trace(x, trace, rho, nit, squeeze=False) -> NonnegResult:
    """The plane-wise solver's trace ``[outer+1, 4, n_planes]`` (include/surfh_amd.h: surfh_cg_planes_nonneg) as a ``NonnegResult``
    whose traces are ``[nit+1, n_planes]`` and whose ``rho`` is the array used; ``squeeze`` (a single image): ``[nit+1]`` and a float."""
    t = trace[: nit + 1]
    cols = [np.sqrt(t[:, 0]), np.sqrt(t[:, 1]), np.sqrt(t[:, 2]), np.rint(t[:, 3]).astype(np.int64)]
    if squeeze:
        cols = [c[:, 0].copy() for c in cols]
    return NonnegResult(x, *cols, float(rho[0]) if squeeze else np.array(rho, dtype=np.float64), int(nit))


def rayleigh_rho(quad, shape, seed=0) -> float:
    """``v^T Q v / v^T v`` for one standard normal probe ``v`` of ``default_rng(seed)``: the mean eigenvalue of ``Q``, at the cost of
    one application.  ``quad(v)`` returns ``v^T Q v``."""
    v = np.random.default_rng(seed).standard_normal(shape)
    return float(quad(v) / np.sum(v * v))


class NonnegOps:
    """Methods of a ``PlanOwner`` with templates (``forward``, ``ishape``, ``installed_weights``)."""

    def _weighted_sq(self, av, weights):
        w = self.data_weights if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        av = np.asarray(av, dtype=np.float64).reshape(-1)
        return float(np.sum(av * av)) if w is None else float(np.sum(np.where(w > 0, w * av * av, 0.0)))

    def nonneg_rho(self, mu=1.0, mu_reg=0.0, seed=0, weights=None) -> float:
        """The default penalty of ``cg_nonneg``: ``v^T Q v / v^T v`` for one standard normal probe ``v`` (``default_rng(seed)``),
        ``Q = mu A^T W A + mu_reg (Dr^T Dr + Dc^T Dc)`` -- the mean eigenvalue of ``Q``, one forward application.  ``weights``: as in
        ``cg`` (None: the model's own).  ``ValueError`` under the joint prior: pass ``rho`` there."""
        if self.get_prior() != "separated":
            raise ValueError("nonneg_rho estimates the penalty under the separated prior: pass rho with set_prior('joint')")

        def quad(v):
            prior = np.sum((v - np.roll(v, 1, axis=1)) ** 2) + np.sum((v - np.roll(v, 1, axis=2)) ** 2) if mu_reg else 0.0
            return mu * self._weighted_sq(self.forward(v), weights) + mu_reg * prior

        return rayleigh_rho(quad, self.ishape, seed)

    def cg_nonneg(self, data, mu=1.0, mu_reg=0.0, rho=None, x0=None, outer=30, inner=10, tol=0.0, refresh=10, weights=None) -> NonnegResult:
        """The maps of ``cg`` under ``x >= 0`` (see the module): ``outer`` ADMM iterations of ``inner`` CG iterations each, from
        ``x0`` (None: zeros); an outer iteration costs ``inner`` applications of the operator, one more every ``refresh`` outer
        iterations, where the carried residual is recomputed (0: never).  ``rho=None``: ``nonneg_rho(mu, mu_reg, weights=weights)``.
        Stops early once ``max(rho primal, dual) < x.size * tol`` (gradient units, as ``cg``'s test).  ``weights`` as in ``cg``.
        Runs on the maps' spectra under the rule of ``cg``.  ``ValueError`` for a bad argument, a model without templates, an
        active imager term."""
        check_nonneg_args(rho, outer, inner, refresh)
        if getattr(self, "templates", None) is None:
            raise ValueError("cg_nonneg needs templates (the constraint is on the abundance maps)")
        self._refuse_imager("cg_nonneg")
        y = _lib.f32_vec(data, self.osize, f"data have {np.size(data)} elements, expected {self.osize}")
        x0a = _lib.f32_vec(x0, self.isize, f"x0 has {np.size(x0)} elements, expected {self.isize}", optional=True)
        if rho is None:
            rho = self.nonneg_rho(mu, mu_reg, weights=weights)
        with self.installed_weights(weights):
            x, trace, nit = _lib._solve_nonneg(self, self._L.surfh_cg_nonneg, y, (mu, mu_reg, rho), x0a, outer, inner, tol, refresh)
        return result_from_trace(x, trace, rho, nit)

    def nonneg_rho_templates(self, maps, mu=1.0, mu_spec=0.0, seed=0, weights=None) -> float:
        """``nonneg_rho`` for the operator of ``cg_templates`` at ``maps``: ``mu A_x^T W A_x + mu_spec D_l^T D_l``."""
        def quad(v):
            return mu * self._weighted_sq(self.forward_templates(v, maps), weights) + mu_spec * np.sum(np.diff(v, axis=1) ** 2)

        return rayleigh_rho(quad, self.templates.shape, seed)

    def nn_project_dev(self, x_t, z_t, u_t, n: int, rho: float, r_t=None, dv_t=None) -> np.ndarray:
        """The projection / dual update of one outer iteration on device vectors of ``n`` floats, in place in ``z_t`` and ``u_t``
        (include/surfh_amd.h: surfh_nn_project_dev); returns ``|x - z'|^2, |z' - z|^2, #{z' == 0}, r.r`` (synchronises).  The
        arguments are device tensors or raw device addresses."""
        ptr = _lib.dev_ptr
        sums = np.zeros(4, dtype=np.float64)
        _lib.check(self._L.surfh_nn_project_dev(self._plan, ptr(x_t), ptr(z_t), ptr(u_t), ptr(r_t), ptr(dv_t), int(n), float(rho),
                                                _lib.dptr(sums)), ValueError)
        return sums
