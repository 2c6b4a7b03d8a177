"""Generate tests/golden/templates.npz: scipy's spectral median filter and sklearn's coordinate-descent NMF, the two
steps of the reference's template notebooks (notebooks/nmf_orion_allband.ipynb).  CPU only, needs scipy and sklearn:

    python tests/golden/make_golden_templates.py

Contents (arrays only):

* ``med<i>_in`` / ``med<i>_out`` / ``med<i>_size`` / ``med<i>_mode``: ``scipy.ndimage.median_filter(a, size, axes=[0],
  mode)`` for sizes 1, 3, 4, 11, 15 and modes reflect / nearest / mirror, on a [40, 37] slice image, a [50, 6, 7] cube,
  a [5, 9] array (an axis shorter than the windows of 11 and 15) and a 1-D line;
* ``X``: a float32 [96, 640] low-rank non-negative matrix plus noise;
* ``it<n>_W`` / ``it<n>_H`` / ``it<n>_err``: ``NMF(4, init="random", random_state=0, tol=0, max_iter=n)`` for n in
  1, 5, 30 (W = fit_transform, H = components_, reconstruction_err_);
* ``full_*``: the default run ``NMF(4, init="random", random_state=0)``: n_iter, reconstruction_err_, components_, and
  ``full_ratio``, violation / violation_init of every iteration (the stopping test's value);
* ``sweep_*``: K = 1..6 with random_state=0 and the defaults: reconstruction_err_ and n_iter_.

and tests/golden/templates_edges.npz, the tile edges of the batched GEMMs (templates.hip: 64 components per tile column, K steps
of 16 wavelengths):

* ``sweep_*``: K = 7..11 on the same ``X``, random_state=0 and the defaults (with K = 1..6 the batch holds 66 components);
* ``Xr``: a float32 [97, 650] matrix of rank 5 plus noise from ``matrix()``: 650 = 512 + 138 and 138 % 16 = 10;
* ``r_it<n>_W`` / ``r_it<n>_H`` / ``r_it<n>_err``: ``NMF(5, init="random", random_state=0, tol=0, max_iter=n)`` on ``Xr`` for n in
  1, 5.
"""
from __future__ import annotations

import json
import os

import numpy as np
import scipy
import sklearn
from scipy import ndimage
from sklearn.decomposition import NMF
from sklearn.decomposition._nmf import _initialize_nmf, _update_coordinate_descent

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "templates.npz")
OUT_EDGES = os.path.join(HERE, "templates_edges.npz")
EDGE_KS = (7, 8, 9, 10, 11)
RAGGED = dict(n=97, m=650, k=5)
RAGGED_ITERS = (1, 5)
MODES = ("reflect", "nearest", "mirror")
SIZES = (1, 3, 4, 11, 15)
ITERS = (1, 5, 30)
K = 4


def _fold(j, n, mode):
    """scipy.ndimage's boundary extension of index j on an axis of n samples."""
    if 0 <= j < n:
        return j
    if mode == "nearest":
        return 0 if j < 0 else n - 1
    if mode == "reflect":
        p = 2 * n
        k = j % p
        return k if k < n else p - 1 - k
    if n == 1:
        return 0
    p = 2 * n - 2
    k = j % p
    return k if k < n else p - k


def _median_by_definition(a, size, mode):
    """Sorted-window median of rank size // 2, window rows l - size // 2 .. l - size // 2 + size - 1: what the cases
    are expected to be (scipy's N-D rank filter reads outside the line when the window's left half reaches 4 x the
    axis length; no case here does)."""
    out = np.empty_like(a)
    for l in range(a.shape[0]):
        w = np.stack([a[_fold(l - size // 2 + q, a.shape[0], mode)] for q in range(size)])
        out[l] = np.sort(w, axis=0)[size // 2]
    return out


def median_cases(rng):
    arrays = [rng.gamma(2.0, 1.0, (40, 37)).astype(np.float32),
              rng.standard_normal((50, 6, 7)).astype(np.float32),
              rng.standard_normal((5, 9)).astype(np.float32),
              rng.standard_normal(33).astype(np.float32)]
    arrays[1][10:20, 2, 3] = 0.5                       # ties
    cases = []
    for a in arrays:
        for s in SIZES:
            for mode in MODES:
                if a.ndim == 1 and s > a.shape[0]:
                    continue
                out = ndimage.median_filter(a, size=s, axes=[0], mode=mode)
                assert np.array_equal(out, _median_by_definition(a, s, mode)), (a.shape, s, mode)
                cases.append((a, out, s, mode))
    return cases


def matrix(rng, n=96, m=640, k=4):
    lam = np.linspace(0.0, 1.0, m)
    H = np.stack([1.0 + np.sin(2 * np.pi * (j + 1) * lam + j) ** 2 + np.exp(-0.5 * ((lam - 0.2 * (j + 1)) / 0.03) ** 2)
                  for j in range(k)])
    W = rng.gamma(2.0, 1.0, (n, k))
    X = W @ H + 0.05 * rng.standard_normal((n, m))
    return np.maximum(X, 0.0).astype(np.float32)


def violation_ratios(X, k, random_state, max_iter, tol):
    """_fit_coordinate_descent's loop, recording violation / violation_init."""
    W, H = _initialize_nmf(X, k, init="random", random_state=random_state)
    Ht = np.ascontiguousarray(H.T)
    ratios, v0 = [], None
    for it in range(1, max_iter + 1):
        v = _update_coordinate_descent(X, W, Ht, 0, 0, False, None)
        v += _update_coordinate_descent(X.T, Ht, W, 0, 0, False, None)
        if it == 1:
            v0 = v
        ratios.append(v / v0 if v0 else 0.0)
        if v0 == 0 or v / v0 <= tol:
            break
    return np.array(ratios), W, Ht.T


def main():
    rng = np.random.default_rng(20261016)
    z = {}
    for i, (a, out, s, mode) in enumerate(median_cases(rng)):
        z[f"med{i}_in"], z[f"med{i}_out"] = a, out
        z[f"med{i}_size"], z[f"med{i}_mode"] = np.int32(s), np.array(mode)
    z["med_count"] = np.int32(i + 1)
    X = matrix(rng)
    z["X"] = X
    for n in ITERS:
        m = NMF(K, init="random", random_state=0, tol=0.0, max_iter=n)
        W = m.fit_transform(X)
        z[f"it{n}_W"], z[f"it{n}_H"], z[f"it{n}_err"] = W, m.components_, np.float64(m.reconstruction_err_)
    m = NMF(K, init="random", random_state=0)
    m.fit(X)
    ratios, _, H = violation_ratios(X, K, 0, 200, 1e-4)
    assert len(ratios) == m.n_iter_ and np.array_equal(H, m.components_)
    z["full_n_iter"], z["full_err"], z["full_H"] = np.int32(m.n_iter_), np.float64(m.reconstruction_err_), m.components_
    z["full_ratio"] = ratios
    ks = np.arange(1, 7)
    errs, nits = [], []
    for k in ks:
        m = NMF(int(k), init="random", random_state=0)
        m.fit(X)
        errs.append(m.reconstruction_err_)
        nits.append(m.n_iter_)
    z["sweep_k"], z["sweep_err"], z["sweep_n_iter"] = ks, np.array(errs), np.array(nits, dtype=np.int32)
    z["meta"] = np.array(json.dumps({"scipy": scipy.__version__, "sklearn": sklearn.__version__}))
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes;", int(z["med_count"]), "median cases; full run n_iter", int(z["full_n_iter"]),
          "sweep n_iter", nits)


def edges(X):
    z = {}
    errs, nits = [], []
    for k in EDGE_KS:
        m = NMF(int(k), init="random", random_state=0)
        m.fit(X)
        errs.append(m.reconstruction_err_)
        nits.append(m.n_iter_)
    z["sweep_k"], z["sweep_err"], z["sweep_n_iter"] = np.array(EDGE_KS), np.array(errs), np.array(nits, dtype=np.int32)
    Xr = matrix(np.random.default_rng(20261019), **RAGGED)
    z["Xr"] = Xr
    for n in RAGGED_ITERS:
        m = NMF(RAGGED["k"], init="random", random_state=0, tol=0.0, max_iter=n)
        W = m.fit_transform(Xr)
        z[f"r_it{n}_W"], z[f"r_it{n}_H"], z[f"r_it{n}_err"] = W, m.components_, np.float64(m.reconstruction_err_)
    z["meta"] = np.array(json.dumps({"scipy": scipy.__version__, "sklearn": sklearn.__version__}))
    np.savez_compressed(OUT_EDGES, **z)
    print(OUT_EDGES, os.path.getsize(OUT_EDGES), "bytes; sweep n_iter", nits)


if __name__ == "__main__":
    import sys
    if "--edges" in sys.argv:          # the tile-edge vectors alone, on the X of the existing file
        edges(np.load(OUT)["X"])
    else:
        main()
        edges(np.load(OUT)["X"])
