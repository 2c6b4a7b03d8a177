"""Generate tests/golden/shepard.npz from the REAL reference's distortion correction.

Run only in the build container:   python tests/golden/make_golden_shepard.py
The reference's ``surfh/ToolsDir/shepard_interpolation.pyx`` is cythonized and compiled from where it lies into the
git-ignored build directory of ``oracle/ref_harness.py`` ($SURFH_REF_BUILD or oracle/_ref/), with the harness's flags
(-O3, no -march=native: no FMA contraction, the arithmetic the source states).  ``surfh/Preprocessing/
distorsion_correction.py`` is imported with the harness's stubs (astropy) plus ``skimage.measure.label``, which is not
installed, restated as scipy.ndimage.label with full 8-connectivity.  Only arrays are written:

* ``k<i>_*``: direct kernel cases (random scatter, cutoffs 1 and 2, p 1 and 2, grid points without neighbours,
  duplicate samples, absolute sky coordinates) -- inputs and the reference's output;
* ``exp_*`` / ``m<mode>_*``: a reduced synthetic exposure (surfh_amd.synth.synthetic_mrs_exposure, 256 rows, 5 slits,
  NaN pixels, one slit shifted up and one down in wavelength) run through the reference's label -> sort -> correct chain
  for modes 0, 1 and 2;
* ``ref_slit_seconds``: the reference's time for one full-size slit (channel 1A: 24 576 samples onto 1050 x 19).
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import os
import subprocess
import sys
import sysconfig
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402
from surfh_amd import synth  # noqa: E402

META = {"reference": "sidiso/surfh @ 2025-02-04",
        "functions": ["surfh.ToolsDir.shepard_interpolation.exponential_modified_shepard",
                      "surfh.Preprocessing.distorsion_correction.sort_labels_by_centroid",
                      "surfh.Preprocessing.distorsion_correction.mrs_slices_distrorsion_correction"],
        "restated_third_party": ["skimage.measure.label -> scipy.ndimage.label, 3x3 structure"],
        "compiled_with": "gcc -O3 (no -march=native)"}

# the reduced exposure: 5 slits, slit 1 shifted beyond max + 1 um (skipped in mode 0), slit 3 below min - 1 um (mode 1)
EXPOSURE = dict(band="1a", n_rows=256, n_slit=5, slit_px=12, gap_px=4, nan_fraction=0.01, seed=5,
                lam_shift={1: 1.5, 3: -1.5})
LAM_STRIDE = 5           # channel wavelengths: every 5th of band 1A's axis
N_ALPHA = 9


def build_shepard():
    os.makedirs(rh.OUT, exist_ok=True)
    so = os.path.join(rh.OUT, "shepard_interpolation" + sysconfig.get_config_var("EXT_SUFFIX"))
    src = os.path.join(rh.REF, "surfh/ToolsDir/shepard_interpolation.pyx")
    if not (os.path.exists(so) and os.path.getmtime(so) >= os.path.getmtime(src)):
        c_file = os.path.join(rh.OUT, "shepard_interpolation.c")
        subprocess.check_call([sys.executable, "-m", "cython", "-3", src, "-o", c_file])
        subprocess.check_call(["gcc", "-O3", "-shared", "-fPIC", "-w", "-DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION",
                               "-I", sysconfig.get_paths()["include"], "-I", np.get_include(), c_file, "-o", so])
        os.remove(c_file)
    spec = importlib.util.spec_from_file_location("surfh.ToolsDir.shepard_interpolation", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    ns = rh.load()                                  # stubs astropy & co, puts the reference on sys.path
    shep = build_shepard()
    sys.modules["surfh.ToolsDir.shepard_interpolation"] = shep
    sys.modules["surfh.ToolsDir"].shepard_interpolation = shep
    if "skimage" not in sys.modules:
        from scipy import ndimage
        sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
        skm.label = lambda img: ndimage.label(np.asarray(img) != 0, structure=np.ones((3, 3), dtype=bool))[0]
        sk.measure = skm
        sys.modules["skimage"], sys.modules["skimage.measure"] = sk, skm
    dc = importlib.import_module("surfh.Preprocessing.distorsion_correction")
    return ns, shep, dc


def kernel_cases(rng):
    """(a, l, v, alpha_mesh, lambda_mesh, p, cutoff, alpha_res, lambda_res) of the direct cases."""
    cases = []
    a = rng.uniform(0, 10, 400); l = rng.uniform(0, 10, 400); v = rng.standard_normal(400)
    ga, gl = np.meshgrid(np.linspace(-2, 12, 15), np.linspace(-2, 12, 13))           # border rows without neighbours
    cases.append((a, l, v, ga, gl, 2.0, 1.0, 1.0, 1.0))
    cases.append((a, l, v, ga, gl, 1.0, 2.0, 1.0, 1.0))
    # duplicates, anisotropic resolution
    d = rng.integers(0, 300, 100)
    a2, l2 = np.concatenate([a[:300], a[d]]), np.concatenate([l[:300] * 3, l[d] * 3])
    v2 = np.concatenate([v[:300], rng.standard_normal(100)])
    ga2, gl2 = np.meshgrid(np.linspace(0, 10, 21), np.linspace(0, 30, 17))
    cases.append((a2, l2, v2, ga2, gl2, 2.0, 2.0, 0.7, 2.1))
    cases.append((a2, l2, v2, ga2, gl2, 1.0, 1.0, 0.7, 2.1))
    # absolute sky coordinates (RA ~ 84 deg: one float32 ulp is ~0.16 alpha pixel here) and microns
    n = 3000
    ra = 83.8221 + rng.uniform(0, 19, n) * 4.7e-5
    lam = 4.9 + rng.uniform(0, 120, n) * 8e-4
    val = 1 + rng.random(n)
    gra, gla = np.meshgrid(83.8221 + np.arange(19) * 4.7e-5, 4.9 + np.arange(120) * 8e-4)
    cases.append((ra, lam, val, gra, gla, 2.0, 2.0, 4.7e-5, 8e-4))
    # a tilted, non-separable mesh
    th = np.radians(20.0)
    u, w = np.meshgrid(np.linspace(0, 10, 16), np.linspace(0, 10, 14))
    cases.append((a, l, v, np.cos(th) * u - np.sin(th) * w + 3, np.sin(th) * u + np.cos(th) * w - 1,
                  2.0, 2.0, 1.0, 1.0))
    return cases


class _Chan:
    def __init__(self, oshape):
        self.oshape = tuple(oshape)


def main():
    ns, shep, dc = load_reference()
    rng = np.random.default_rng(20261015)
    out = {"meta": json.dumps(META)}
    cases = kernel_cases(rng)
    for i, (a, l, v, ga, gl, p, cut, ares, lres) in enumerate(cases):
        f = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32))  # noqa: E731
        r = shep.exponential_modified_shepard(f(a), f(l), f(v), f(ga), f(gl), p=p, alpha=2.0, pixel_cutoff=cut,
                                              alpha_res=ares, lambda_res=lres)
        out.update({f"k{i}_a": f(a), f"k{i}_l": f(l), f"k{i}_v": f(v), f"k{i}_ga": f(ga), f"k{i}_gl": f(gl),
                    f"k{i}_par": np.array([p, cut, ares, lres]), f"k{i}_out": np.asarray(r)})
    out["n_kernel_cases"] = np.int64(len(cases))

    e = synth.synthetic_mrs_exposure(**EXPOSURE)
    cw = e["wavelengths"][::LAM_STRIDE]
    binary = (~np.isnan(e["alpha"])).astype(np.float64)
    with contextlib.redirect_stdout(io.StringIO()):
        lab = dc.generate_label_image(binary)
        slab = dc.sort_labels_by_centroid(lab)
    tab = (e["alpha"], e["beta"], e["lam"])
    out.update(exp_data=e["data"], exp_alpha=e["alpha"], exp_beta=e["beta"], exp_lam=e["lam"], exp_cw=cw,
               exp_labels=lab, exp_sorted=slab, exp_oshape=np.array([1, EXPOSURE["n_slit"], len(cw), N_ALPHA]))
    for mode in (0, 1, 2):
        with contextlib.redirect_stdout(io.StringIO()):
            cs = dc.mrs_slices_distrorsion_correction(_Chan(out["exp_oshape"]), slab,
                                                      lambda x, y: tuple(t[y, x] for t in tab), e["data"], cw, mode)
        out[f"m{mode}_slices"] = np.asarray(cs)

    # one full-size slit: the reference's time
    full = synth.synthetic_mrs_exposure()
    flab = dc.sort_labels_by_centroid(dc.generate_label_image(~np.isnan(full["alpha"])))
    pix = np.where(flab == 1)
    al, lm, it = full["alpha"][pix], full["lam"][pix], full["data"][pix]
    ok = ~np.isnan(it)
    wl = full["wavelengths"]
    gax = np.linspace(al.min(), al.max(), 19)
    am, lmm = np.meshgrid(gax, wl)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        ref_full = dc.perform_shepard_interpolation(al[ok], lm[ok], it[ok], am, lmm, 2, 2.0, 2,
                                                    (gax.max() - gax.min()) / 19, (wl.max() - wl.min()) / len(wl))
    dt = time.perf_counter() - t0
    out["ref_slit_seconds"] = np.float64(dt)
    out["ref_slit_samples"] = np.int64(ok.sum())
    out["full_slit0_out"] = np.asarray(ref_full, dtype=np.float32)
    print(f"reference, one full-size slit ({ok.sum()} samples onto {am.shape}): {dt:.1f} s")
    path = os.path.join(HERE, "shepard.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
