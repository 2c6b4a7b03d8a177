"""Spectral templates of the linear mixing model, as the reference's template notebooks make them
(notebooks/nmf_orion_allband.ipynb): a median filter along the wavelength axis, a coordinate-descent NMF of the
(pixels x wavelengths) matrix of the filtered cube, and every ``step``-th wavelength of the components, saved as the
``nmf_*`` / ``wavel_axis_*`` files that ``scripts/main_fusion.py`` loads.

Both computations run on the GPU (include/surfh_amd.h): ``surfh_spectral_median`` gives the values of
``scipy.ndimage.median_filter(a, size, axes=[0], mode=mode)`` exactly, and ``surfh_nmf_cd`` runs sklearn's
coordinate-descent NMF (``NMF(solver="cd")``, Frobenius loss, no regularisation, no shuffle) in float32 for several
models at once, sharing each pass over X.  The ``random`` initialisation is sklearn's ``_initialize_nmf``, on the host."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

__all__ = ["median_filter_spectral", "NMF", "nmf_sweep", "init_random", "cube_to_matrix", "subsample_templates",
           "write_templates", "template_file_names", "MEDIAN_MODES"]

MEDIAN_MODES = {"reflect": 0, "nearest": 1, "mirror": 2}
MAX_MEDIAN_SIZE = 63


def _check(rc):
    if rc != 0:
        raise RuntimeError(_lib.load().surfh_templates_last_error().decode("utf-8", "replace"))


def median_filter_spectral(a, size: int, mode: str = "reflect", device: int = 0) -> np.ndarray:
    """``scipy.ndimage.median_filter(a, size=size, axes=[0], mode=mode)`` on the GPU, for ``a`` of any ndim >= 1.

    The result has ``a``'s float dtype (float32 arithmetic is exact here: a median is one of its inputs, so float64
    input is filtered as float32 and must be representable as such).  ``size`` 1..63; modes reflect, nearest, mirror."""
    if mode not in MEDIAN_MODES:
        raise ValueError(f"mode {mode!r}: only {sorted(MEDIAN_MODES)} are supported")
    size = int(size)
    if not 1 <= size <= MAX_MEDIAN_SIZE:
        raise ValueError(f"size {size} outside 1..{MAX_MEDIAN_SIZE}")
    a = np.asarray(a)
    if a.ndim < 1:
        raise ValueError("median_filter_spectral needs an array of ndim >= 1")
    out_dtype = a.dtype if a.dtype in (np.float32, np.float64) else np.float32
    src = np.ascontiguousarray(a, dtype=np.float32)
    if a.size == 0:
        return src.astype(out_dtype)
    dst = np.empty_like(src)
    L = src.shape[0]
    _check(_lib.load().surfh_spectral_median(_lib.fptr(src), _lib.fptr(dst), L, src.size // L, size,
                                              MEDIAN_MODES[mode], int(device)))
    return dst.astype(out_dtype, copy=False)


def _validate_X(X):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"X must be 2-D (samples x features), got shape {X.shape}")
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    if X.size == 0:
        raise ValueError("X is empty")
    if not np.all(np.isfinite(X)):
        raise ValueError("X contains NaN or infinity")
    if X.min() < 0:
        raise ValueError("Negative values in data passed to NMF (input X)")
    return X


def init_random(X, n_components: int, random_state=None):
    """sklearn's ``_initialize_nmf(X, n_components, init="random", random_state)``: ``avg = sqrt(X.mean() / K)``,
    standard normal draws of H, then of W, scaled by avg, cast to X's dtype, made non-negative."""
    X = np.asarray(X)
    n_samples, n_features = X.shape
    avg = np.sqrt(X.mean() / n_components)
    rng = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    H = avg * rng.standard_normal(size=(n_components, n_features)).astype(X.dtype, copy=False)
    W = avg * rng.standard_normal(size=(n_samples, n_components)).astype(X.dtype, copy=False)
    np.abs(H, out=H)
    np.abs(W, out=W)
    return W, H


def _run(X, inits, max_iter, tol, device=0):
    """One ``surfh_nmf_cd`` call on float32 X for the (W, H) pairs in ``inits``.  Returns, per model,
    (W, H, n_iter, violation trace, Frobenius error, MRE) and the device time per iteration (ms)."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    P, L = X32.shape
    K = np.array([h.shape[0] for _, h in inits], dtype=np.int32)
    W = np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w, _ in inits]))
    H = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.float32).reshape(-1) for _, h in inits]))
    n = len(inits)
    n_iter = np.zeros(n, dtype=np.int32)
    trace = np.zeros((n, max_iter), dtype=np.float64)
    err = np.zeros(n, dtype=np.float64)
    mre = np.zeros(n, dtype=np.float64)
    ms = C.c_float()
    _check(_lib.load().surfh_nmf_cd(_lib.fptr(X32), P, L, n, _lib.iptr(K), _lib.fptr(W), _lib.fptr(H), int(max_iter),
                                     float(tol), _lib.iptr(n_iter), _lib.dptr(trace), _lib.dptr(err), _lib.dptr(mre),
                                     int(device), C.byref(ms)))
    res, wo, ho = [], 0, 0
    for m, k in enumerate(K):
        Wm = W[wo:wo + P * k].reshape(P, k)
        Hm = H[ho:ho + k * L].reshape(k, L)
        wo += P * k
        ho += k * L
        res.append((Wm, Hm, int(n_iter[m]), trace[m, :n_iter[m]].copy(), float(err[m]), float(mre[m])))
    return res, ms.value


class NMF:
    """sklearn.decomposition.NMF with ``solver="cd"`` and Frobenius loss, on the GPU in float32.

    Supported: ``init`` "random" (sklearn's, on the host) or "custom" (W and H given to ``fit_transform``), ``tol``,
    ``max_iter``, ``random_state``.  Other solvers, losses, inits and any regularisation raise NotImplementedError.
    Results come back in X's dtype; ``violation_`` holds the per-iteration violation trace (not in sklearn)."""

    def __init__(self, n_components=None, *, init="random", solver="cd", beta_loss="frobenius", tol=1e-4,
                 max_iter=200, random_state=None, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, shuffle=False,
                 device=0):
        if solver != "cd":
            raise NotImplementedError(f"solver {solver!r}: only 'cd' is implemented")
        if beta_loss not in ("frobenius", 2, 2.0):
            raise NotImplementedError(f"beta_loss {beta_loss!r}: only 'frobenius' is implemented")
        if init not in ("random", "custom"):
            raise NotImplementedError(f"init {init!r}: only 'random' and 'custom' are implemented")
        if alpha_W != 0 or alpha_H not in ("same", 0, 0.0):
            raise NotImplementedError("regularised NMF (alpha_W / alpha_H) is not implemented")
        if shuffle:
            raise NotImplementedError("shuffle=True is not implemented")
        if n_components is None or int(n_components) < 1:
            raise ValueError(f"n_components must be a positive integer, got {n_components!r}")
        if int(max_iter) < 1:
            raise ValueError(f"max_iter must be >= 1, got {max_iter}")
        if tol < 0:
            raise ValueError(f"tol must be >= 0, got {tol}")
        self.n_components = int(n_components)
        self.init = init
        self.solver = solver
        self.beta_loss = beta_loss
        self.tol = float(tol)
        self.max_iter = int(max_iter)
        self.random_state = random_state
        self.alpha_W, self.alpha_H, self.l1_ratio, self.shuffle = alpha_W, alpha_H, l1_ratio, shuffle
        self.device = device

    def _init(self, X, W, H):
        if self.init == "custom":
            if W is None or H is None:
                raise ValueError("init='custom' needs W and H")
            W, H = np.asarray(W), np.asarray(H)
            if W.shape != (X.shape[0], self.n_components) or H.shape != (self.n_components, X.shape[1]):
                raise ValueError(f"W {W.shape} / H {H.shape} do not fit X {X.shape} with {self.n_components} components")
            if W.min() < 0 or H.min() < 0:
                raise ValueError("Negative values in the initial W or H")
            return W, H
        return init_random(X, self.n_components, self.random_state)

    def fit_transform(self, X, y=None, W=None, H=None):
        X = _validate_X(X)
        W0, H0 = self._init(X, W, H)
        (res,), ms = _run(X, [(W0, H0)], self.max_iter, self.tol, self.device)
        self._set(X.dtype, res)
        return self._W

    def fit(self, X, y=None, **params):
        self.fit_transform(X, **params)
        return self

    def _set(self, dtype, res):
        W, H, n_iter, trace, err, mre = res
        self._W = W.astype(dtype, copy=False)
        self.components_ = H.astype(dtype, copy=False)
        self.n_components_ = H.shape[0]
        self.n_iter_ = n_iter
        self.reconstruction_err_ = err
        self.mre_ = mre
        self.violation_ = trace


def nmf_sweep(X, component_range=range(1, 12), random_state=None, max_iter=200, tol=1e-4, device=0):
    """The notebook's model-order sweep, every order in one batched GPU call.  Each model starts from sklearn's random
    init with ``random_state``.  Returns ``(models, info)``: the fitted ``NMF`` per order, and a dict of arrays
    ``n_components``, ``error`` (||X - WH||_F), ``mre`` (mean of (X - WH) / X where X != 0, else 0), ``n_iter`` and
    ``ms_per_iter`` (device time per batched iteration)."""
    X = _validate_X(X)
    ks = [int(k) for k in component_range]
    if not ks:
        raise ValueError("empty component range")
    models = [NMF(k, init="random", random_state=random_state, max_iter=max_iter, tol=tol, device=device) for k in ks]
    inits = [init_random(X, k, random_state) for k in ks]
    res, ms = _run(X, inits, max_iter, tol, device)
    for m, r in zip(models, res):
        m._set(X.dtype, r)
    info = {"n_components": np.array(ks), "error": np.array([m.reconstruction_err_ for m in models]),
            "mre": np.array([m.mre_ for m in models]), "n_iter": np.array([m.n_iter_ for m in models]),
            "ms_per_iter": ms}
    return models, info


def cube_to_matrix(cube, box=None) -> np.ndarray:
    """``[L, y, x]`` -> ``[pixels, L]`` (pixels in C order), after an optional crop ``box = (y0, y1, x0, x1)``."""
    cube = np.asarray(cube)
    if cube.ndim != 3:
        raise ValueError(f"cube must be [L, y, x], got shape {cube.shape}")
    if box is not None:
        y0, y1, x0, x1 = (int(b) for b in box)
        cube = cube[:, y0:y1, x0:x1]
    return np.ascontiguousarray(cube.reshape(cube.shape[0], -1).T)


def subsample_templates(components, wavel, step: int = 4):
    """Every ``step``-th wavelength: ``components[:, ::step]``, ``wavel[::step]`` (the notebook's SS4)."""
    components, wavel = np.asarray(components), np.asarray(wavel)
    if components.shape[-1] != wavel.shape[0]:
        raise ValueError(f"components {components.shape} and wavel {wavel.shape} disagree")
    return np.ascontiguousarray(components[:, ::step]), np.ascontiguousarray(wavel[::step])


def template_file_names(tag: str, n_templates: int, step: int):
    stem = f"{tag}_{n_templates}_templates_SS{step}.npy"
    return "nmf_" + stem, "wavel_axis_" + stem


def write_templates(directory, components, wavel, tag: str = "orion_1ABC_2ABC_3ABC_4ABC", step: int = 4):
    """Save ``nmf_{tag}_{K}_templates_SS{step}.npy`` ([K, L // step] or so) and the matching ``wavel_axis_`` file, as
    the notebook does and as ``scripts/main_fusion.load_simulation_data`` reads them.  Returns the two paths."""
    comp, wl = subsample_templates(components, wavel, step)
    os.makedirs(directory, exist_ok=True)
    n_t, n_w = template_file_names(tag, comp.shape[0], step)
    p_t, p_w = os.path.join(directory, n_t), os.path.join(directory, n_w)
    np.save(p_t, comp)
    np.save(p_w, wl)
    return p_t, p_w
