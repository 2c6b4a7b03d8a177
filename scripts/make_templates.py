#!/usr/bin/env python
"""Spectral templates for the fusion -- the reference's template notebooks (notebooks/nmf_orion_allband.ipynb) as one
command:

    cube[NaN] = 0;  f = median_filter(cube, size, axes=[0]);  f[f == 0] = NaN          (notebook cell 4)
    X = f[:, box] as [pixels, L] (NaN -> 0)                                             (cells 3, 5)
    optional model-order sweep K = a..b: Frobenius error, mean relative error, n_iter  (cell 6)
    NMF(n_components=nt, init="random", random_state, max_iter).fit(X)                   (cell 7)
    nmf_{tag}_{nt}_templates_SS{step}.npy = components_[:, ::step], wavel_axis_... = wavel[::step]  (cells 10, 12)

The cube comes from ``--input``: an .npz with ``cube`` ([L, y, x]) and ``wavel`` ([L]), or a FITS cube (data in HDU 1,
wavelengths in HDU 5 as the notebook reads them; needs astropy) -- or from ``--synthetic``
(surfh_amd.synth.synthetic_template_cube).  The files go to ``<out>/Templates/``, where
``scripts/main_fusion.py -fd <out>`` loads them.  The median filter and the NMF run on the GPU.

    python scripts/make_templates.py --synthetic -o fusion_dir -nt 4 --sweep 1 11
    python scripts/make_templates.py --input cube.npz -o fusion_dir -nt 6 --box 31 54 22 52
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_cube(path):
    if path.endswith(".npz"):
        with np.load(path) as z:
            return np.asarray(z["cube"], dtype=np.float32), np.asarray(z["wavel"], dtype=np.float64)
    try:
        from astropy.io import fits
    except ImportError:
        raise SystemExit(f"{path}: reading FITS needs astropy, which is not installed; give an .npz with cube and wavel")
    with fits.open(path) as hdul:
        return np.asarray(hdul[1].data, dtype=np.float32), np.array(hdul[5].data[0])[0, :, 0].astype(np.float64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", help=".npz (cube, wavel) or FITS cube")
    src.add_argument("--synthetic", action="store_true", help="a synthetic 4-template cube (256 wavelengths, 23 x 30)")
    ap.add_argument("-o", "--out", default=".", help="fusion directory; files go to <out>/Templates/ (default .)")
    ap.add_argument("-nt", dest="n_templates", type=int, default=4, help="number of templates (default 4)")
    ap.add_argument("--size", type=int, default=15, help="median window along lambda, 1 disables (default 15)")
    ap.add_argument("--box", type=int, nargs=4, metavar=("Y0", "Y1", "X0", "X1"), help="spatial crop cube[:, Y0:Y1, X0:X1]")
    ap.add_argument("--sweep", type=int, nargs=2, metavar=("KMIN", "KMAX"), help="model-order sweep, writes sweep.npz")
    ap.add_argument("--random_state", type=int, default=0, help="seed of the random init (default 0)")
    ap.add_argument("--max_iter", type=int, default=1000, help="NMF iterations at most (default 1000)")
    ap.add_argument("--tol", type=float, default=1e-4, help="NMF stopping tolerance (default 1e-4)")
    ap.add_argument("--step", type=int, default=4, help="keep every step-th wavelength (default 4)")
    ap.add_argument("--tag", default="orion_1ABC_2ABC_3ABC_4ABC", help="file name tag (default: the fusion driver's)")
    args = ap.parse_args(argv)

    from surfh_amd import synth
    from surfh_amd import templates as T

    if args.synthetic:
        d = synth.synthetic_template_cube(n_lambda=256, ny=23, nx=30, n_templates=4, noise=0.01, nan_fraction=0.02)
        cube, wavel = d["cube"], d["wavel"]
    else:
        cube, wavel = load_cube(args.input)
    if cube.ndim != 3 or cube.shape[0] != wavel.shape[0]:
        raise SystemExit(f"cube {cube.shape} and wavel {wavel.shape} do not fit [L, y, x] / [L]")
    t0 = time.perf_counter()
    f = np.nan_to_num(cube, nan=0.0)
    if args.size > 1:
        f = T.median_filter_spectral(f, args.size)
    t1 = time.perf_counter()
    X = np.nan_to_num(T.cube_to_matrix(f, args.box), nan=0.0)   # f[f == 0] = NaN, then NaN -> 0: zeros stay zeros
    n_neg = int((X < 0).sum())
    if n_neg:
        print(f"{n_neg} negative values set to 0 (NMF needs non-negative data)")
        X = np.maximum(X, 0.0)
    tpl_dir = os.path.join(args.out, "Templates")
    os.makedirs(tpl_dir, exist_ok=True)
    print(f"cube {cube.shape} -> X {X.shape}; median (size {args.size}) {1e3 * (t1 - t0):.1f} ms")
    if args.sweep:
        ks = range(args.sweep[0], args.sweep[1] + 1)
        t2 = time.perf_counter()
        _, info = T.nmf_sweep(X, ks, random_state=args.random_state, max_iter=args.max_iter, tol=args.tol)
        np.savez(os.path.join(tpl_dir, "sweep.npz"), n_components=info["n_components"], error=info["error"],
                 mre=info["mre"], n_iter=info["n_iter"])
        print(f"sweep K={ks.start}..{ks.stop - 1} in {time.perf_counter() - t2:.2f} s "
              f"({info['ms_per_iter']:.3f} ms per batched iteration)")
        for k, e, m, n in zip(info["n_components"], info["error"], info["mre"], info["n_iter"]):
            print(f"  K={k:2d}  error {e:.6g}  MRE {m:+.3e}  n_iter {n}")
    t3 = time.perf_counter()
    nmf = T.NMF(args.n_templates, init="random", random_state=args.random_state, max_iter=args.max_iter, tol=args.tol)
    nmf.fit(X)
    p_t, p_w = T.write_templates(tpl_dir, nmf.components_, wavel, tag=args.tag, step=args.step)
    print(f"NMF K={args.n_templates}: {nmf.n_iter_} iterations, error {nmf.reconstruction_err_:.6g}, "
          f"{time.perf_counter() - t3:.2f} s -> {p_t}, {p_w}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
