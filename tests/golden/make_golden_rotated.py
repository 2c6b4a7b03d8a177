"""Generate the fixtures of the rotated-field 2-D operator from the REAL reference.

Run only in the build container:   python tests/golden/make_golden_rotated.py
The reference's ``surfh.Models.spectro_blind.MRSBlurred`` (the rotated variant of the 2-D deconvolution operator, bilinear
gridding at the rotated local grid, interpolating back-projection) is imported through ``oracle/ref_harness.py`` exactly as
``make_golden.py`` imports the other reference modules.  Every array written here was computed by reference code; the
inputs are regenerated from the stored seeds by the tests (tests/rotated_oracle.py holds the problems).
"""
from __future__ import annotations

import contextlib
import importlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness as rh  # noqa: E402
import rotated_oracle as ro  # noqa: E402

META = {
    "reference": "sidiso/surfh @ 2025-02-04",
    "class": "surfh.Models.spectro_blind.MRSBlurred",
    "restated_third_party": ["udft.ir2fr (udft 3.4.0)", "aljabr.LinOp (aljabr 0.4.0)"],
    "jax_utils_mapped_to": "surfh/ToolsDir/python_utils.py (float64)",
}


def _ref_model(ns, case):
    mod = importlib.import_module("surfh.Models.spectro_blind")
    I = ns.instru
    with contextlib.redirect_stdout(io.StringIO()):
        return mod.MRSBlurred(case["sotf"], case["alpha_axis"], case["beta_axis"], rh.make_ifu(ns, case["spec"]), case["step_deg"],
                              I.CoordList([I.Coord(a, b) for a, b in case["pointings"]]))


def rotated():
    """96 x 96 image, 12 slits, field of view at 20 degrees, three pointings (two fractional)."""
    ns = rh.load()
    case = ro.small_case()
    rm = _ref_model(ns, case)
    x = np.random.default_rng(case["x_seed"]).random(case["imshape"])
    y = np.asarray(rm.forward(x))
    u = np.random.default_rng(case["u_seed"]).standard_normal(y.size)
    sl = [rm.get_slit_slices(k) for k in range(case["spec"].n_slit)]
    np.savez_compressed(os.path.join(HERE, "mrs_blurred_rot.npz"), y=y, adjoint_ref=np.asarray(rm.adjoint(u)),
                        x_seed=np.int64(case["x_seed"]), u_seed=np.int64(case["u_seed"]),
                        slit_slices=np.array([[a.start, a.stop, b.start, b.stop] for a, b in sl]),
                        slit_w=np.array([rm.get_slit_weights(k, sl[k])[0][0] for k in range(len(sl))]),
                        meta=json.dumps(META))


def rotated_d2i():
    """``data_to_img`` (spectro_blind.py:238-281) on the band-1C geometry at 8.2 degrees, 251 x 251 image, four pointings; data =
    the reference's own forward of a random image.  ``covered`` marks the pixels where some pointing's back-projection exceeds
    the reference's threshold of 100 (recorded from the reference's own ``gridding_t`` outputs): elsewhere its weighted mean
    is uninitialised memory and is stored as 0."""
    ns = rh.load()
    case = ro.d2i_case()
    rm = _ref_model(ns, case)
    x = np.random.default_rng(case["x_seed"]).random(case["imshape"]) * case["x_scale"]
    y = np.asarray(rm.forward(x))
    cum = []
    gridding_t = rm.gridding_t

    def recording_gridding_t(local_img, pointing):
        out = gridding_t(local_img, pointing)
        cum.append(np.array(out))
        return out

    rm.gridding_t = recording_gridding_t
    with contextlib.redirect_stdout(io.StringIO()):
        wm, gl = rm.data_to_img(np.copy(y))
    assert len(cum) == len(case["pointings"])
    covered = np.sum(np.stack(cum) > 100, axis=0) != 0
    np.savez_compressed(os.path.join(HERE, "mrs_blurred_rot_d2i.npz"), y=y, global_img=np.asarray(gl),
                        weighted_mean=np.where(covered, np.asarray(wm), 0.0), covered=covered, x_seed=np.int64(case["x_seed"]),
                        meta=json.dumps(dict(META, note="weighted_mean is kept only where some pointing's back-projection exceeds 100: "
                                                         "elsewhere the reference returns uninitialised memory")))


if __name__ == "__main__":
    rh.build_cython()
    rotated()
    rotated_d2i()
