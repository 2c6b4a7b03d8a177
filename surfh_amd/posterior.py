"""Posterior sampling of the maps ``cg`` returns, by perturbation-optimisation (Orieux, Feron & Giovannelli 2012;
include/surfh_amd.h: surfh_cg_sample).

Convention: the criterion ``cg`` minimises is the negative log of the Gaussian posterior

    p(x | y)  ~  exp(-x^T Q x / 2 + b^T x),    Q = mu A^T W A + mu_reg (Dr^T Dr + Dc^T Dc),    b = mu A^T W y,

so the precision is ``Q`` exactly as ``cg`` defines it and the covariance is ``Q^-1``; it becomes a statistical statement once
the caller passes ``weights = 1 / sigma^2`` (``mu = 1``).  ``Q^-1`` is a dense ``T N^2 x T N^2`` matrix and is never formed: a
draw ``b~ ~ N(b, Q)`` solved through ``Q x~ = b~`` is a posterior sample -- the library solves for its deviation ``e = x~ - x_map``
from zero, ``Q e = b~ - b``, which keeps every fp32 vector at the perturbation's scale -- and the device accumulates the per-pixel
``T x T`` moments of the samples.  This module holds the host side: the result object, the model method and ``cube_std``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

MAX_MAPS = 8                 # SURFH_MAX_TEMPLATES: the moment kernels hold T (T + 3) / 2 sums per pixel in registers


@dataclass
class PosteriorResult:
    """What ``sample_posterior`` returns.

    ``x_map`` ``[T, Na, Nb]``: the unperturbed solution, bit for bit what ``cg`` returns for the same arguments (the posterior
    mean up to the solve's convergence); ``grad_norm`` / ``nit``: the r.r trace and iteration count of that solve.
    ``mean`` ``[T, Na, Nb]``: the samples' mean; ``cov`` ``[T, T, Na, Nb]``: their unbiased covariance per pixel (symmetric);
    ``std`` ``[T, Na, Nb]``: the square root of its diagonal.
    ``rr_worst``: the largest final ``r.r`` over the sample solves ``Q e = b~ - b``.  A sample is exact only if its solve
    converges: CG stopped at ``max_iter`` leaves the slowly converging directions under-dispersed, so where ``rr_worst`` is not
    small against the first entry of the samples' traces (``|b~ - b|^2``, the ``rr[0]`` the callback sees) the ``std`` is a lower
    bound, not an estimate."""
    x_map: np.ndarray
    mean: np.ndarray
    cov: np.ndarray
    std: np.ndarray
    nit: int
    grad_norm: np.ndarray
    rr_worst: float
    n_samples: int


def unpack_cov(packed, T):
    """``[T (T + 1) / 2, ...]`` (pairs t <= u, row-major) -> the symmetric ``[T, T, ...]``."""
    packed = np.asarray(packed)
    out = np.empty((T, T) + packed.shape[1:], dtype=packed.dtype)
    k = 0
    for t in range(T):
        for u in range(t, T):
            out[t, u] = out[u, t] = packed[k]
            k += 1
    return out


def cube_std(cov, templates, planes=None):
    """Per-pixel standard deviation of the cube ``sum_t s[t, lambda] x_t`` under the maps' covariance ``cov`` ``[T, T, Na, Nb]``:
    ``sqrt(s_lambda^T Sigma s_lambda)`` for the chosen ``planes`` (indices into the wavelength axis; None: all).  ``templates``
    ``[T, Lc]``.  Returns ``[len(planes), Na, Nb]``.  Host side (NumPy)."""
    s = np.asarray(templates, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 4 or cov.shape[0] != cov.shape[1] or cov.shape[0] != s.shape[0]:
        raise ValueError(f"cov {cov.shape} is not [T, T, Na, Nb] with T = {s.shape[0]} templates")
    if planes is not None:
        s = s[:, np.atleast_1d(np.asarray(planes, dtype=np.int64))]
    return np.sqrt(np.maximum(np.einsum("tl,tuab,ul->lab", s, cov, s), 0.0))


def check_args(model, mu, mu_reg, n_samples):
    """The refusals of surfh_cg_sample, as ``ValueError`` before any library call."""
    if not model.lmm:
        raise ValueError("sample_posterior needs a model with templates (the posterior is that of the abundance maps)")
    if model.ishape[0] > MAX_MAPS:
        raise ValueError(f"sample_posterior: {model.ishape[0]} maps, the moment kernels take {MAX_MAPS}")
    if model.get_prior() != "separated":
        raise ValueError("sample_posterior draws the prior's noise through the separated differences: set_prior('separated')")
    if model.has_imager_term():
        raise ValueError("sample_posterior does not perturb the imager data term: clear it (set_imager_data(None))")
    if not (np.isfinite(mu) and mu > 0):
        raise ValueError(f"sample_posterior: mu = {mu!r} must be finite and > 0")
    if not (np.isfinite(mu_reg) and mu_reg >= 0):
        raise ValueError(f"sample_posterior: mu_reg = {mu_reg!r} must be finite and >= 0")
    if int(n_samples) < 2:
        raise ValueError(f"sample_posterior: n_samples = {n_samples!r}, a covariance needs at least 2")


def _noise(perturbations, n_samples, osize, isize, mu_reg):
    if perturbations is None:
        return None, None, None
    if len(perturbations) != 3:
        raise ValueError("perturbations must be (eps_y [K, osize], eps_r [K, isize], eps_c [K, isize])")
    out = []
    for name, e, n in zip(("eps_y", "eps_r", "eps_c"), perturbations, (osize, isize, isize)):
        if e is None and name != "eps_y" and mu_reg == 0:
            out.append(None)
            continue
        a = np.ascontiguousarray(np.asarray(e, dtype=np.float32).reshape(n_samples, -1))
        if a.shape[1] != n:
            raise ValueError(f"perturbations: {name} has {a.shape[1]} elements per draw, expected {n}")
        out.append(a)
    return tuple(out)


def sample_posterior(model, data, mu=1.0, mu_reg=0.0, n_samples=16, seed=0, x0=None, max_iter=10, tol=1e-12, refresh=50,
                     weights=None, perturbations=None, callback=None):
    """See ``spectroSigRLSCT.sample_posterior``."""
    check_args(model, mu, mu_reg, n_samples)
    K, T = int(n_samples), model.ishape[0]
    npix = model.isize // T
    y = _lib.f32_vec(data, model.osize, "data size mismatch")
    x0a = _lib.f32_vec(x0, model.isize, "x0 size mismatch", optional=True)
    ey, er, ec = _noise(perturbations, K, model.osize, model.isize, float(mu_reg))
    x_map = np.empty(model.isize, dtype=np.float32)
    mean = np.empty(model.isize, dtype=np.float64)
    cov = np.empty((T * (T + 1) // 2, npix), dtype=np.float64)
    gn = np.zeros(int(max_iter) + 1, dtype=np.float64)
    nit, worst = C.c_int32(), C.c_double()
    cb, finish = _lib.trampoline(_lib.SAMPLE_CALLBACK, callback, _lib.iterate_args(model.isize, model.ishape))
    opt = _lib.opt_fptr
    with model.installed_weights(weights):
        rc = model._L.surfh_cg_sample(model._plan, _lib.fptr(y), float(mu), float(mu_reg), opt(x0a), int(max_iter), float(tol),
                                      int(refresh), K, _lib.seed64(seed), opt(ey), opt(er), opt(ec), _lib.fptr(x_map),
                                      _lib.dptr(mean), _lib.dptr(cov), _lib.dptr(gn), C.byref(nit), C.byref(worst), cb, None)
    finish(rc)
    cov = unpack_cov(cov.reshape((-1,) + tuple(model.ishape[1:])), T)
    std = np.sqrt(np.maximum(cov[np.arange(T), np.arange(T)], 0.0))
    return PosteriorResult(x_map=x_map.astype(np.float64).reshape(model.ishape), mean=mean.reshape(model.ishape), cov=cov, std=std,
                           nit=nit.value, grad_norm=gn[: nit.value + 1].copy(), rr_worst=worst.value, n_samples=K)


def po_rhs(model, data, mu, mu_reg, seed=0, sample=0, perturbation=None):
    """``surfh_po_rhs``: the perturbed right-hand side ``b~ = mu A^T W y~ + eta`` ``[T, Na, Nb]`` of draw ``sample`` under
    ``seed`` and the model's data weights; ``perturbation=(eps_y, eps_r, eps_c)`` replaces the generator."""
    y = _lib.f32_vec(data, model.osize, "data size mismatch")
    eps = None
    if perturbation is not None:
        eps = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.float32).reshape(-1) for e in perturbation]))
        if eps.size != model.osize + 2 * model.isize:
            raise ValueError("perturbation must be (eps_y [osize], eps_r [isize], eps_c [isize])")
    out = np.empty(model.isize, dtype=np.float32)
    _lib.check(model._L.surfh_po_rhs(model._plan, _lib.fptr(y), float(mu), float(mu_reg), _lib.seed64(seed), int(sample),
                                     _lib.opt_fptr(eps), _lib.fptr(out)))
    return out.astype(np.float64).reshape(model.ishape)


def po_moments(xhat, samples, cov=True, device=0):
    """``surfh_po_moments``: ``(mean [T, ...], cov [T, T, ...] or None)`` of the samples ``[K, T, ...]`` about ``xhat`` ``[T, ...]``."""
    xh = np.ascontiguousarray(np.asarray(xhat, dtype=np.float32))
    sm = np.ascontiguousarray(np.asarray(samples, dtype=np.float32))
    if sm.shape[1:] != xh.shape:
        raise ValueError(f"samples {sm.shape} are not [K] + {xh.shape}")
    T, K = xh.shape[0], sm.shape[0]
    npix = xh.size // T
    mean = np.empty((T, npix), dtype=np.float64)
    packed = np.empty((T * (T + 1) // 2, npix), dtype=np.float64) if cov else None
    _lib.check(_lib.load().surfh_po_moments(T, npix, _lib.fptr(xh), _lib.fptr(sm), K, _lib.dptr(mean),
                                            None if packed is None else _lib.dptr(packed), int(device)), ValueError)
    return mean.reshape(xh.shape), None if packed is None else unpack_cov(packed.reshape((-1,) + xh.shape[1:]), T)


# ---- the plane-wise 2-D deconvolution (``MRSBlurred.sample_posterior``; include/surfh_amd.h: surfh_cg_planes_sample) ---------------------
@dataclass
class PlanesPosteriorResult:
    """What ``MRSBlurred.sample_posterior`` returns.  The arrays have ``cg``'s shapes: ``[n_planes, Na, Nb]`` and one trace column
    per plane for a stack of planes, ``[Na, Nb]`` and scalars per plane squeezed away for a single image.

    ``x_map``: the unperturbed solution, bit for bit what ``cg`` returns for the same arguments; ``grad_norm`` ``[nit+1, n_planes]``
    and ``nit``: its r.r trace and iteration count.  ``mean``: the samples' mean; ``var``: their unbiased variance per pixel (the
    planes are independent problems: there is no covariance between them to report); ``std = sqrt(var)``.
    ``rr_first`` / ``rr_last`` ``[n_planes]``: per plane the largest first and the largest final ``r.r`` over the sample solves
    ``Q_l e_l = b~_l - b_l``.  A sample is exact only if its solve converges: where ``rr_last`` is not small against ``rr_first``
    the ``std`` of that plane is a lower bound, not an estimate.

    Improper planes: a plane whose ``rr_first`` is exactly 0 drew no perturbation at all -- none of its data has a weight and
    ``mu_reg = 0``, so ``Q_l = 0`` and its posterior is flat.  The device reports a variance of 0 there (every deviation is 0);
    read as "certain" that would be the opposite of the truth, so such a plane gets ``var = std = +inf`` (decided on the host,
    ``improper_planes``); its ``mean`` is ``x_map``."""
    x_map: np.ndarray
    mean: np.ndarray
    var: np.ndarray
    std: np.ndarray
    nit: int
    grad_norm: np.ndarray
    rr_first: np.ndarray
    rr_last: np.ndarray
    n_samples: int


def check_planes_args(mu, mu_reg, n_samples, max_iter=0):
    """The numeric refusals of surfh_cg_planes_sample, as ``ValueError`` before any library call."""
    if not (np.ndim(mu) == 0 and np.isfinite(mu) and mu > 0):
        raise ValueError(f"sample_posterior: mu = {mu!r} must be finite and > 0")
    if not (np.ndim(mu_reg) == 0 and np.isfinite(mu_reg) and mu_reg >= 0):
        raise ValueError(f"sample_posterior: mu_reg = {mu_reg!r} must be one finite number >= 0")
    if int(n_samples) != n_samples or int(n_samples) < 2:
        raise ValueError(f"sample_posterior: n_samples = {n_samples!r}, a variance needs at least 2")
    if int(max_iter) < 0:
        raise ValueError(f"sample_posterior: max_iter = {max_iter!r}")


def improper_planes(rr_first):
    """The planes without a proper posterior: ``rr_first`` exactly 0 (``PlanesPosteriorResult``)."""
    return np.atleast_1d(np.asarray(rr_first, dtype=np.float64)) == 0.0


def planes_result(x_map, mean, var, gn, nit, rr_first, rr_last, n_samples, shape, squeeze):
    """The result object from the flat arrays of the library: shapes, the improper-plane rule, ``std``."""
    L = rr_first.size
    var = np.array(var, dtype=np.float64).reshape(L, -1)
    var[improper_planes(rr_first)] = np.inf
    var = var.reshape(shape)
    gn = np.asarray(gn)[: nit + 1]
    return PlanesPosteriorResult(x_map=np.asarray(x_map, dtype=np.float64).reshape(shape), mean=np.asarray(mean).reshape(shape), var=var,
                                 std=np.sqrt(var), nit=int(nit), grad_norm=(gn[:, 0] if squeeze else gn).copy(),
                                 rr_first=float(rr_first[0]) if squeeze else rr_first, rr_last=float(rr_last[0]) if squeeze else rr_last,
                                 n_samples=int(n_samples))


def sample_posterior_planes(model, data, mu=1.0, mu_reg=0.0, n_samples=16, seed=0, x0=None, max_iter=10, tol=1e-12, refresh=50,
                            weights=None, perturbations=None, callback=None):
    """See ``Blurred2D.sample_posterior``."""
    check_planes_args(mu, mu_reg, n_samples, max_iter)
    K, L = int(n_samples), model.n_planes
    y = _lib.f32_vec(data, model.osize, "data size mismatch")
    x0a = _lib.f32_vec(x0, model.isize, "x0 size mismatch", optional=True)
    ey, er, ec = _noise(perturbations, K, model.osize, model.isize, float(mu_reg))
    x_map = np.empty(model.isize, dtype=np.float32)
    mean, var = (np.empty(model.isize, dtype=np.float64) for _ in range(2))
    gn = np.zeros((int(max_iter) + 1, L), dtype=np.float64)
    first, last = np.zeros(L, dtype=np.float64), np.zeros(L, dtype=np.float64)
    nit = C.c_int32()
    squeeze = not model.batched
    cb, finish = _lib.trampoline(_lib.SAMPLE_CALLBACK, callback, _lib.iterate_args(model.isize, model.ishape, L, squeeze))
    opt = _lib.opt_fptr
    with model.installed_weights(weights):
        rc = model._L.surfh_cg_planes_sample(model._plan, _lib.fptr(y), float(mu), float(mu_reg), opt(x0a), int(max_iter), float(tol),
                                             int(refresh), K, _lib.seed64(seed), opt(ey), opt(er), opt(ec), _lib.fptr(x_map),
                                             _lib.dptr(mean), _lib.dptr(var), _lib.dptr(gn), C.byref(nit), _lib.dptr(first),
                                             _lib.dptr(last), cb, None)
    finish(rc)
    return planes_result(x_map, mean, var, gn, nit.value, first, last, K, model.ishape, squeeze)


def po_planes_rhs(model, data, mu, mu_reg, seed=0, sample=0, perturbation=None):
    """``surfh_po_planes_rhs``: the perturbed right-hand side ``b~ = mu A^T W y~ + eta`` (the model's input shape) of draw ``sample``
    under ``seed`` and the model's data weights; ``perturbation=(eps_y, eps_r, eps_c)`` replaces the generator."""
    y = _lib.f32_vec(data, model.osize, "data size mismatch")
    eps = None
    if perturbation is not None:
        eps = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.float32).reshape(-1) for e in perturbation]))
        if eps.size != model.osize + 2 * model.isize:
            raise ValueError("perturbation must be (eps_y [osize], eps_r [isize], eps_c [isize])")
    out = np.empty(model.isize, dtype=np.float32)
    _lib.check(model._L.surfh_po_planes_rhs(model._plan, _lib.fptr(y), float(mu), float(mu_reg), _lib.seed64(seed), int(sample),
                                            _lib.opt_fptr(eps), _lib.fptr(out)))
    return out.astype(np.float64).reshape(model.ishape)


def po_planes_moments(xhat, samples, var=True, device=0):
    """``surfh_po_planes_moments``: ``(mean, var or None)`` of the samples ``[K, L, ...]`` about ``xhat`` ``[L, ...]``, per element."""
    xh = np.ascontiguousarray(np.asarray(xhat, dtype=np.float32))
    sm = np.ascontiguousarray(np.asarray(samples, dtype=np.float32))
    if xh.ndim < 2 or sm.shape[1:] != xh.shape:
        raise ValueError(f"samples {sm.shape} are not [K] + {xh.shape}, xhat [L, ...]")
    L, K = xh.shape[0], sm.shape[0]
    mean = np.empty(xh.shape, dtype=np.float64)
    v = np.empty(xh.shape, dtype=np.float64) if var else None
    _lib.check(_lib.load().surfh_po_planes_moments(L, xh.size // L, _lib.fptr(xh), _lib.fptr(sm), K, _lib.dptr(mean),
                                                   None if v is None else _lib.dptr(v), int(device)), ValueError)
    return mean, v
