"""Template refinement: the other half-step of the bilinear model ``y = A(S) x`` -- hold the maps ``x``, solve for the spectra ``S``.

The joint criterion is ``J(x, S) = [mu (y - A(S) x)^T W (y - A(S) x) + mu_reg (|Dr x|^2 + |Dc x|^2) + mu_spec |D_l S|^2] / 2`` with
``D_l`` the first difference along the wavelength with open ends; for fixed maps it is quadratic in ``S`` and ``A_x : S -> A(S) x`` is
the forward model with ``S`` in the templates' place (include/surfh_amd.h: surfh_set_templates ... surfh_cg_templates).  This module
holds what the Python classes share: the argument check and the plan-state methods of a model that owns a plan.

What the data can say about a spectrum is limited by the detector: a feature narrower than the detector's wavelength sampling
(config 1 has 48 detector samples for 128 planes) is not recovered, whatever the solver does; ``mu_spec`` fills such planes, and
the planes no channel reads, from their neighbours."""
from __future__ import annotations

import numpy as np

from . import _lib


def check_templates(S, shape) -> np.ndarray:
    """``S`` as the contiguous float64 ``[T, Lc]`` array the library takes.  ``ValueError`` unless it has the model's shape (the
    number of templates and of planes are fixed at plan creation) and is finite, in float32 too.  No library call."""
    a = np.asarray(S, dtype=np.float64)
    if a.shape != tuple(shape):
        raise ValueError(f"templates have shape {a.shape}, the model's are {tuple(shape)}: T and Lc are fixed at plan creation")
    if not np.all(np.abs(a) <= np.finfo(np.float32).max):        # NaN fails the comparison too
        raise ValueError("templates must be finite (in float32 too)")
    return np.ascontiguousarray(a)


class TemplateOps:
    """Methods of a ``PlanOwner`` with templates (``self.templates``, ``ishape``, ``osize``)."""

    def _need_templates(self):
        if getattr(self, "templates", None) is None:
            raise ValueError("the model has no templates")

    def set_templates(self, S):
        """Replace the model's templates ``[T, Lc]`` (plan state: every operator and solver uses them from now on, as if the model
        had been built with them; ``mapsToCube`` and ``cube_std`` read ``self.templates``).  ``ValueError`` on a wrong shape, a
        non-finite value, or while an imager is attached -- its transfer functions were built from the templates: detach it
        (``set_imager(None)``), set the templates, attach it again."""
        self._need_templates()
        a = check_templates(S, self.templates.shape)
        _lib.check(self._L.surfh_set_templates(self._plan, _lib.dptr(a)), ValueError)
        self.templates = a.copy()

    def forward_templates(self, S, maps):
        """``A_x S``: the forward model on ``maps`` with ``S`` in the templates' place; the model's templates are untouched."""
        self._need_templates()
        a = check_templates(S, self.templates.shape)
        x = _lib.f32_vec(maps, self.isize, f"maps have {np.size(maps)} elements, expected {self.isize}")
        y = np.empty(self.osize, dtype=np.float32)
        _lib.check(self._L.surfh_forward_templates(self._plan, _lib.fptr(x), _lib.dptr(a), _lib.fptr(y)))
        return y.astype(np.float64).reshape(self.oshape)

    def adjoint_templates(self, u, maps):
        """``A_x^T u`` ``[T, Lc]``: the transpose of ``forward_templates``; exactly 0 on the planes no channel reads."""
        self._need_templates()
        message = f"maps / data have {np.size(maps)} / {np.size(u)} elements, expected {self.isize} / {self.osize}"
        x, v = _lib.f32_vec(maps, self.isize, message), _lib.f32_vec(u, self.osize, message)
        g = np.empty(self.templates.size, dtype=np.float32)
        _lib.check(self._L.surfh_adjoint_templates(self._plan, _lib.fptr(x), _lib.fptr(v), _lib.fptr(g)))
        return g.astype(np.float64).reshape(self.templates.shape)

    def _data_and_maps(self, data, maps):
        message = "data or maps size mismatch"
        return _lib.f32_vec(data, self.osize, message), _lib.f32_vec(maps, self.isize, message)

    def cg_templates(self, data, maps, mu=1.0, mu_spec=0.0, s0=None, max_iter=10, tol=1e-12, refresh=50, callback=None, weights=None):
        """Linear CG on ``(mu A_x^T W A_x + mu_spec D_l^T D_l) S = mu A_x^T W y`` from ``s0`` (None: the model's templates): the
        loop, stopping test, trace and callback contract of ``cg``, the size in the tolerance being ``T Lc``.  ``callback(it,
        grad_norm, S)``; ``weights`` as in ``cg``.  Returns ``(S, grad_norm, nit)``; the model's templates are unchanged (the
        plan's own are back in place on every exit, and while the callback runs).  ``ValueError`` while an imager is attached."""
        self._need_templates()
        if getattr(self, "_imager", None) is not None:
            raise ValueError("cg_templates does not carry the imager data term and the attached imager was built from the model's "
                             "templates: detach it (set_imager(None)) first")
        shape = self.templates.shape
        y, x = self._data_and_maps(data, maps)
        s0a = None if s0 is None else check_templates(s0, shape).astype(np.float32).reshape(-1)
        with self.installed_weights(weights):
            return _lib._solve(self, self._L.surfh_cg_templates_cb, y, (_lib.fptr(x), mu, mu_spec), s0a, max_iter, tol, refresh, (),
                               callback, size=self.templates.size, shape=shape, exc=ValueError)

    def cg_templates_nonneg(self, data, maps, mu=1.0, mu_spec=0.0, rho=None, s0=None, outer=30, inner=10, tol=0.0, refresh=10,
                            weights=None):
        """The spectra of ``cg_templates`` under ``S >= 0``: the ADMM loop of ``cg_nonneg`` (surfh_amd/nonneg.py) around the CG of
        ``cg_templates``, from ``s0`` (None: the model's templates), sizes ``T Lc``.  ``rho=None``: ``nonneg_rho_templates(maps, mu,
        mu_spec, weights=weights)``.  Returns a ``NonnegResult`` whose ``x`` is ``S`` ``[T, Lc]``; the model's templates are
        unchanged.  ``ValueError`` for a bad argument, or while an imager is attached."""
        from . import nonneg
        nonneg.check_nonneg_args(rho, outer, inner, refresh, "cg_templates_nonneg")
        self._need_templates()
        if getattr(self, "_imager", None) is not None:
            raise ValueError("cg_templates_nonneg does not carry the imager data term and the attached imager was built from the "
                             "model's templates: detach it (set_imager(None)) first")
        shape = self.templates.shape
        y, x = self._data_and_maps(data, maps)
        s0a = None if s0 is None else check_templates(s0, shape).astype(np.float32).reshape(-1)
        if rho is None:
            rho = self.nonneg_rho_templates(maps, mu, mu_spec, weights=weights)
        with self.installed_weights(weights):
            S, trace, nit = _lib._solve_nonneg(self, self._L.surfh_cg_templates_nonneg, y, (_lib.fptr(x), mu, mu_spec, rho), s0a, outer,
                                               inner, tol, refresh, size=self.templates.size, shape=shape)
        return nonneg.result_from_trace(S, trace, rho, nit)

    def joint_criterion(self, data, maps, mu=1.0, mu_reg=0.0, mu_spec=0.0, weights=None):
        """``(J, data term, spatial prior, spectral prior)`` at ``maps`` and the model's templates, summed on the device in float64:
        ``J = (mu data + mu_reg spatial + mu_spec spectral) / 2`` (the module's criterion; ``weights`` as in ``cg``)."""
        self._need_templates()
        y, x = self._data_and_maps(data, maps)
        out = np.zeros(4, dtype=np.float64)
        with self.installed_weights(weights):
            _lib.check(self._L.surfh_joint_criterion(self._plan, _lib.fptr(y), _lib.fptr(x), float(mu), float(mu_reg), float(mu_spec),
                                                     _lib.dptr(out)))
        return tuple(float(v) for v in out)
