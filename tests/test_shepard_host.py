"""Host side of the distortion correction (surfh_amd.preprocessing): labelling and centroid sort against the reference's
fixture, the float32 pair-test replica and the float64 checker against the reference's kernel, the slit reorder helper
and the driver's command line.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shepard_oracle as so
from surfh_amd import preprocessing as P
from surfh_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    return np.load(so.GOLDEN)


def test_labels_and_centroid_sort_match_reference(z):
    binary = ~np.isnan(z["exp_alpha"])
    lab = P.generate_label_image(binary)
    assert np.array_equal(lab, z["exp_labels"])
    assert np.array_equal(P.sort_labels_by_centroid(lab), z["exp_sorted"])
    # sorted labels run left to right
    cols = [np.mean(np.nonzero(z["exp_sorted"] == k)[1]) for k in range(1, int(lab.max()) + 1)]
    assert np.all(np.diff(cols) > 0)


def test_label_image_is_8_connected():
    img = np.array([[1, 0, 0, 1],
                    [0, 1, 0, 0],
                    [0, 0, 0, 0],
                    [1, 0, 1, 0]])
    lab = P.generate_label_image(img)
    assert lab.max() == 4 and lab[0, 0] == lab[1, 1] == 1 and lab[0, 3] == 2 and lab[3, 0] == 3 and lab[3, 2] == 4
    s = P.sort_labels_by_centroid(lab)
    assert s[3, 0] == 1 and s[0, 0] == s[1, 1] == 2 and s[3, 2] == 3 and s[0, 3] == 4


@pytest.mark.parametrize("i", range(6))
def test_replica_and_checker_match_reference_kernel(z, i):
    c = so.kernel_cases(z)[i]
    out, n = so.replica(c["a"], c["l"], c["v"], c["ga"], c["gl"], c["p"], c["cutoff"], c["ares"], c["lres"])
    mask = so.neighbour_mask(c["a"], c["l"], c["ga"], c["gl"], c["ares"], c["lres"], c["cutoff"])
    chk = so.checker(c["a"], c["l"], c["v"], c["ga"], c["gl"], mask, c["p"], c["cutoff"], c["ares"], c["lres"])
    ref = c["out"].ravel()
    scale = np.abs(c["v"]).max()
    assert np.max(np.abs(out - ref)) <= 1e-6 * scale
    assert np.max(np.abs(chk - ref)) <= 1e-6 * scale
    assert np.array_equal(ref == 0, n == 0)          # exactly the points without a neighbour are 0


def test_fixture_covers_the_cases(z):
    cases = so.kernel_cases(z)
    assert {c["cutoff"] for c in cases} == {1.0, 2.0} and {c["p"] for c in cases} == {1.0, 2.0}
    assert any((c["out"] == 0).any() for c in cases)                                    # points without neighbours
    assert any(len(np.unique(np.stack([c["a"], c["l"]]), axis=1)[0]) < len(c["a"]) for c in cases)   # duplicates
    assert any(c["ga"].min() > 80 for c in cases)                                       # absolute sky coordinates
    assert np.isnan(z["exp_data"][~np.isnan(z["exp_alpha"])]).any()                    # NaN pixels on the slits
    written = [np.count_nonzero(np.abs(z[f"m{m}_slices"]).sum(axis=(1, 2))) for m in range(3)]
    assert z["exp_oshape"][1] == 5 and written == [3, 3, 3]
    assert float(z["ref_slit_seconds"]) > 0


def test_edges_fixture_covers_the_cases():
    """tests/golden/shepard_edges.npz (make_golden_shepard_edges.py) holds what shepard.npz leaves out: parameters other
    than p in {1, 2}, alpha = 2, epsilon = 1e-6, non-finite inputs and outputs, cutoffs one ulp apart.  Arrays only."""
    import shepard_cases as sc
    e = np.load(sc.GOLDEN_EDGES)                         # allow_pickle is off: an object array would raise below
    assert os.path.getsize(sc.GOLDEN_EDGES) < os.path.getsize(so.GOLDEN) and len(e["raised"]) == 0
    cases = [sc.load_reference(e, str(n)) for n in e["names"]]
    assert len(cases) == 28 and all(c["out"].shape == c["ga"].shape for c in cases)
    assert {c["p"] for c in cases} == {0.5, 2.0, 3.0} and {c["alpha"] for c in cases} == {0.5, 2.0, 8.0}
    assert {c["eps"] for c in cases} == {0.0, 1e-6, 1e-3} and any(c["ares"] < 0 for c in cases)
    assert len({c["cutoff"] for c in cases}) >= 9
    assert any(np.isnan(c["out"]).any() for c in cases) and any(np.isinf(c["out"]).any() for c in cases)
    assert any(not np.isfinite(c["a"]).any() or not np.isfinite(c["l"]).any() or
               not (np.isfinite(c["a"]) & np.isfinite(c["l"])).any() for c in cases)
    assert json.loads(str(e["meta"]))["compiled_with"].startswith("gcc -O3")


def test_reorder_corrected_slices():
    s = np.arange(21, dtype=float)[:, None, None] * np.ones((21, 3, 2))
    r = P.reorder_corrected_slices(s, "1A")
    order, roll = P.SLIT_ORDER[1]
    expect = np.zeros(21)
    expect[order] = np.arange(21)
    assert np.array_equal(r[:, 0, 0], np.roll(expect, roll))
    r2 = P.reorder_corrected_slices(np.arange(17.0)[:, None, None] * np.ones((17, 2, 2)), "ch2-long")
    e2 = np.zeros(17)
    e2[P.SLIT_ORDER[2][0]] = np.arange(17)
    assert np.array_equal(r2[:, 0, 0], np.roll(e2, 9))
    r4 = P.reorder_corrected_slices(np.arange(12.0)[:, None, None] * np.ones((12, 1, 1)), 4)
    assert np.array_equal(r4[[0, 6, 1, 7], 0, 0], [0, 1, 2, 3])
    for ch, n in ((1, 21), (2, 17), (3, 16), (4, 12)):
        assert sorted(P.SLIT_ORDER[ch][0]) == list(range(n))
    with pytest.raises(ValueError):
        P.reorder_corrected_slices(np.zeros((13, 1, 1)), "4B")
    with pytest.raises(ValueError):
        P.reorder_corrected_slices(np.zeros((3, 1, 1)), "mirimage")
    pay = P.slices_to_payload(r)
    assert pay.shape == (3, 42) and np.array_equal(pay[:, 2:4], r[1])


def test_synthetic_exposure_layout():
    e = synth.synthetic_mrs_exposure(n_rows=128, n_slit=4, slit_px=10, gap_px=4, lam_shift={2: 1.5})
    on = ~np.isnan(e["alpha"])
    lab = P.generate_label_image(on)
    assert lab.max() == 4 and np.array_equal(on, ~np.isnan(e["lam"]))
    assert abs(np.nanmean(e["alpha"]) - e["ra"]) < 1e-3 and abs(np.nanmean(e["beta"]) - e["dec"]) < 1e-3
    x, y = np.nonzero(on.T)
    a, b, lam = e["detector2world"](x, y)
    assert np.array_equal(a, e["alpha"][y, x]) and np.array_equal(lam, e["lam"][y, x])
    s = P.sort_labels_by_centroid(lab)
    assert np.nanmax(e["lam"][s == 3]) > e["wavelengths"].max() + 1                     # the shifted slit
    assert np.all(np.isnan(e["data"][~on]))


def test_driver_help_and_flags():
    script = os.path.join(ROOT, "scripts", "correction_mrs_data.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--input", "--synthetic", "--chan", "--mode", "-np", "--out"):
        assert flag in out.stdout
    bad = subprocess.run([sys.executable, script, "--chan", "1A"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--input" in bad.stderr
