"""The local error measures of tests/helpers.py (max_err, slice_err) catch what the whole-array figure ``rel`` averages away.
No GPU: faults are seeded into the float64 oracle's own output of problems.long_windows (43 360 detector samples) and the
measures are asserted on both sides of the project's gate TOL = 1e-5.  The edge problems' wavelength windows, on which
tests/test_gpu_local_parity.py relies for its code paths, are asserted here too."""
import numpy as np
import pytest

import problems
from helpers import TOL, local_errs, max_err, rel, slice_err
from oracle import surfh_oracle as orc

FWD_AXES = dict(row=(0, 1, 3), lam=2)              # a channel's data as (P, S, Ldet, a)
MAP_AXES = dict(template=0, alpha=1, beta=2)


@pytest.fixture(scope="module")
def long_case():
    cfg = problems.long_windows()
    om = problems.oracle_model(cfg, box="direct")
    y = om.forward(cfg["maps"])
    return cfg, om, y


def test_edge_problem_windows(long_case):
    cfg, om, _ = long_case
    assert [c.wslice for c in om.channels] == problems.LONG_WINDOWS
    assert [c.oshape for c in om.channels] == [(2, 3, 1100, 4), (2, 2, 1060, 4)]
    (a0, a1), (b0, b1) = problems.LONG_WINDOWS
    assert a1 - a0 > 1024 and b1 - b0 > 1024 and b0 < a1 <= b0 + 1024        # the overlap lies in the second channel's chunk 0 only
    for order in ("ABC", "ACB"):
        om3 = problems.oracle_model(problems.three_channels(order), box="direct")
        assert [c.wslice for c in om3.channels] == [problems.THREE_WINDOWS[k] for k in order]
    w = problems.THREE_WINDOWS
    assert w["A"][1] < w["C"][0] and w["B"][0] < w["A"][1] and w["C"][0] < w["B"][1]   # B meets A and C, which leave a gap
    om5 = problems.oracle_model(problems.five_channels(), box="direct")
    assert [c.wslice for c in om5.channels] == problems.FIVE_WINDOWS
    cover = np.zeros(problems.five_channels()["Lc"], dtype=int)
    for lo, hi in problems.FIVE_WINDOWS:
        cover[lo:hi] += 1
    assert cover[7:141].min() >= 2 and cover.max() >= 3       # every interior plane belongs to several channels


def test_measures_on_known_arrays():
    ref = np.zeros((3, 4, 5))
    ref[0], ref[1] = 1.0, 2.0                                 # slice 2 is empty: judged against the average slice norm
    a = ref.copy()
    a[2, 1, 3] = 1e-3
    e, at = slice_err(a, ref, 0)
    avg = np.linalg.norm(ref) * np.sqrt(20 / 60)
    assert at == 2 and abs(e - 1e-3 / avg) < 1e-15
    assert abs(max_err(a, ref) - 1e-3 / 2.0) < 1e-15
    e, at = slice_err(a, ref, (1, 2))                         # slices over two axes: the index is a tuple
    assert at == (1, 3) and e > 0
    assert slice_err(ref, ref, 2) == (0.0, 0)
    d = local_errs(a, ref, dict(plane=0, col=(1, 2)))
    assert set(d) == {"rel", "max", "plane", "plane_at", "col", "col_at"} and d["plane_at"] == 2


def test_float32_round_trip_is_below_every_measure(long_case):
    _, om, y = long_case
    for k in range(2):
        r = y[om._idx[k]:om._idx[k + 1]].reshape(om.channels[k].oshape)
        e = local_errs(r.astype(np.float32), r, FWD_AXES)
        assert max(v for n, v in e.items() if not n.endswith("_at")) < 1e-6, e


def test_seeded_detector_faults(long_case):
    """Faults in one channel's data, (P, S, Ldet, a) = (2, 3, 1100, 4).  Computed here: the 2^-12 stretch gives rel 7.2e-6 -- under
    the gate, ``rel`` misses it -- with a worst element of 1.2e-4 and a worst row of 3.5e-5; the zeroed sample gives rel 1.0e-2
    (worst element 0.95, worst wavelength 0.2) and the swapped rows rel 2.7e-4 (worst row 9.1e-4): ``rel`` sees these two at this
    size, as one figure without a place, and at the ten million samples of config 3 every ``rel`` here is another 15 times
    smaller; the local measures do not shrink with the array and name the row."""
    _, om, y = long_case
    ref = y[:om._idx[1]].reshape(om.channels[0].oshape)
    out = {}
    a = ref.copy()
    a[1, 2, 500:532, 3] *= 1.0 + 2.0 ** -12                   # a K step that lost its low fp16 piece
    out["stretch"] = local_errs(a, ref, FWD_AXES)
    assert out["stretch"]["rel"] < TOL                        # the gap: the whole-array figure passes
    assert out["stretch"]["max"] > TOL and out["stretch"]["row"] > TOL and out["stretch"]["row_at"] == (1, 2, 3)
    a = ref.copy()
    a[0, 1, 1099, 2] = 0.0                                    # the last sample of a ragged tile
    out["zeroed"] = local_errs(a, ref, FWD_AXES)
    assert out["zeroed"]["max"] > 100 * TOL and out["zeroed"]["row_at"] == (0, 1, 2) and out["zeroed"]["lam_at"] == 1099
    a = ref.copy()
    a[1, 0, :, [1, 2]] = ref[1, 0, :, [2, 1]]                 # two neighbouring rows swapped
    out["swapped"] = local_errs(a, ref, FWD_AXES)
    assert out["swapped"]["row"] > 10 * TOL and out["swapped"]["row_at"] in ((1, 0, 1), (1, 0, 2))
    for k, e in out.items():
        print(k, {n: (f"{v:.2e}" if isinstance(v, float) else v) for n, v in e.items()})
        assert max(e["max"], e["row"], e["lam"]) > TOL


def test_seeded_adjoint_fault(long_case):
    """One (pixel, 1024-plane chunk) of the second channel stored where it should have been added to the first channel's
    contribution: the adjoint's accumulated cube holds the second channel alone on the overlap 813..1315 of one pixel.  After
    the conjugate OTF and the templates the fault is a PSF-sized blot in every map.  Computed here: rel 7.1e-4 (500 planes of a
    48 x 48 image: ``rel`` sees it at this size, and would not at 251 x 251, 27 times smaller), worst element 3.2e-3, worst map
    row and column 1.6e-3 and 1.5e-3, both at the pixel."""
    cfg, om, y = long_case
    u = np.random.default_rng(3).random(om.osize)
    parts = [orc.channel_adjoint(t, u[om._idx[k]:om._idx[k + 1]], om.alpha_axis, om.beta_axis, "exact", "direct")
             for k, t in enumerate(om.channels)]

    def finish(g):
        return orc.lmm_cube2maps(orc.idft(orc.dft(g) * om.sotf.conj(), om.ishape[1:]), om.templates)
    g = np.zeros(om.cube_shape)
    for t, part in zip(om.channels, parts):
        g[t.wslice[0]:t.wslice[1]] += part
    ref = finish(g)
    assert rel(ref, om.adjoint(u)) < 1e-14
    (a0, a1), (b0, b1) = problems.LONG_WINDOWS
    pix = (24, 23)
    assert np.all(parts[0][b0 - a0:, pix[0], pix[1]] != 0) and np.all(parts[1][:a1 - b0, pix[0], pix[1]] != 0)   # both channels see it
    g[b0:a1, pix[0], pix[1]] = parts[1][:a1 - b0, pix[0], pix[1]]
    e = local_errs(finish(g), ref, MAP_AXES)
    print("stored instead of added:", {n: (f"{v:.2e}" if isinstance(v, float) else v) for n, v in e.items()})
    assert e["max"] > TOL and e["alpha"] > TOL and e["beta"] > TOL
    assert abs(e["alpha_at"] - pix[0]) <= 1 and abs(e["beta_at"] - pix[1]) <= 1
