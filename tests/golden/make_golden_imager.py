"""Generate tests/golden/imager.npz from the REAL reference's ``instru.WavelFilter`` (surfh/Models/instru.py:700-737).

Run only in the build container:   python tests/golden/make_golden_imager.py
The reference's ``surfh/Models/instru.py`` is imported through the unchanged ``oracle/ref_harness.py``.  Only arrays are
written: one filter with 7 measured points, a 24-point wavelength axis that overhangs the filter on both sides (the ``left=0`` /
``right=0`` sides of ``np.interp``), a seeded 24 x 6 x 5 cube and a seeded spectrum, with the reference's ``transmittance``
(normalised and not), ``integrate_hsi`` and ``integrate_spectrum`` of them.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402

META = {"reference": "sidiso/surfh @ 2025-02-04",
        "functions": ["surfh.Models.instru.WavelFilter.transmittance", "surfh.Models.instru.WavelFilter.integrate_hsi",
                      "surfh.Models.instru.WavelFilter.integrate_spectrum"]}


def main():
    ns = rh.load()
    rng = np.random.default_rng(20261018)
    meas_w = np.array([5.20, 5.35, 5.50, 5.80, 6.10, 6.30, 6.45])
    meas_v = np.array([0.00, 0.12, 0.55, 0.83, 0.78, 0.31, 0.02])
    axis = np.linspace(4.9, 6.8, 24)                  # 4 points below the filter, 5 above
    cube = rng.random((24, 6, 5))
    spectrum = rng.random(24)
    f = ns.instru.WavelFilter(meas_w, meas_v, name="F560W-like")
    out = dict(meta=json.dumps(META), measured_wavelength=meas_w, measured_values=meas_v, axis=axis, cube=cube, spectrum=spectrum,
               transmittance=np.asarray(f.transmittance(axis)), transmittance_normalized=np.asarray(f.transmittance(axis, normalized=True)),
               integrate_hsi=np.asarray(f.integrate_hsi(cube, axis)), integrate_spectrum=np.float64(f.integrate_spectrum(spectrum, axis)))
    path = os.path.join(HERE, "imager.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
