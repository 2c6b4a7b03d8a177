#!/usr/bin/env python
"""Distortion correction of one MRS detector exposure onto the model's slice grid -- the run of the reference's
``scripts/correction_mrs_data.py:90-197``:

    labels  = sort_labels_by_centroid(generate_label_image(pixels with world coordinates))            (:126-131)
    channel = Channel(ifu, alpha_axis, beta_axis, wavelengths, get_srf(det_pix_size, step), [(0, 0)])   (:60-86)
    slices  = mrs_slices_distrorsion_correction(channel, labels, detector2world, data, wavel, mode)   (:135-140)
    sorted  = the channel's slit permutation and roll                                                  (:149-185)
    payload = sorted.transpose(1, 0, 2).reshape(L, n_slit * n_alpha)                                   (:192)

The reference reads a JWST ``rate`` file and its WCS; here the exposure comes from ``--input`` (an .npz with ``data``
and ``alpha``, ``beta``, ``lam`` per detector pixel, as ``detector2world(xx, yy)`` gives them, NaN off the slits) or is
synthetic (``--synthetic``: surfh_amd.synth.synthetic_mrs_exposure of the band).  Writes ``corrected.npy``
([n_slit, L, n_alpha], model slit order) and ``payload.npy`` ([L, n_slit * n_alpha]) under ``--out``; ``--cube`` also
runs ``Channel.realData_sliceToCube`` on the slices and writes ``cube.npy``.  The resampling runs on the GPU.
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

STEP = 0.025                       # arcsec per cube pixel (correction_mrs_data.py:64)


def setup_channel(chan: str, npix: int):
    """correction_mrs_data.py:60-86: the band's IFU, super-resolution factor det_pix_size // step, one pointing."""
    from surfh_amd import instru, models, synth
    ifu = synth.band_ifu(chan.lower())
    srf = instru.get_srf([ifu.det_pix_size], STEP)[0]
    ax = synth.axes(npix)
    return models.Channel(ifu, ax, ax, np.asarray(ifu.wavel_axis), srf, instru.CoordList([instru.Coord(0, 0)]),
                          synth.STEP_DEG)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", help=".npz with data, alpha, beta, lam (detector layout)")
    src.add_argument("--synthetic", action="store_true", help="a synthetic exposure of the band")
    ap.add_argument("--chan", default="1A", help="sub-band, e.g. 1A, 2C (default 1A)")
    ap.add_argument("--mode", type=int, default=0, choices=(0, 1, 2),
                    help="0: skip slits beyond max(lambda)+1, 1: below min(lambda)-1, 2: keep all (default 0)")
    ap.add_argument("-np", dest="npix", type=int, default=501, help="cube pixels per side (default 501)")
    ap.add_argument("--out", default=".", help="output directory (default .)")
    ap.add_argument("--cube", action="store_true", help="also write realData_sliceToCube of the slices (cube.npy)")
    args = ap.parse_args(argv)

    from surfh_amd import preprocessing as P
    from surfh_amd import synth

    chan = setup_channel(args.chan, args.npix)
    if args.synthetic:
        e = synth.synthetic_mrs_exposure(args.chan.lower())
        data, world = e["data"], (e["alpha"], e["beta"], e["lam"])
    else:
        with np.load(args.input) as z:
            data, world = z["data"], (z["alpha"], z["beta"], z["lam"])
    t0 = time.perf_counter()
    labels = P.sort_labels_by_centroid(P.generate_label_image(~np.isnan(world[0])))
    t1 = time.perf_counter()
    slices, info = P.mrs_slices_distrorsion_correction(chan, labels, world, data, chan.raw_instr.wavel_axis, args.mode,
                                                       return_info=True)
    t2 = time.perf_counter()
    ordered = P.reorder_corrected_slices(slices, args.chan)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "corrected.npy"), ordered)
    np.save(os.path.join(args.out, "payload.npy"), P.slices_to_payload(ordered))
    print(f"{len(info['labels'])} slits corrected, {len(info['skipped'])} skipped -> {ordered.shape}; labelling "
          f"{1e3 * (t1 - t0):.1f} ms, correction {1e3 * (t2 - t1):.1f} ms (kernels {info['kernel_ms']:.2f} ms)")
    if args.cube:
        cube = chan.realData_sliceToCube(ordered, (chan.oshape[2],) + chan.imshape)
        np.save(os.path.join(args.out, "cube.npy"), cube)
        print("cube", cube.shape)
        chan.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
