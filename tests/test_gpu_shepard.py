"""The GPU distortion correction (surfh_shepard, surfh_amd.preprocessing) against the reference's fixture
(tests/golden/shepard.npz), the float32 replica of the pair test and the float64 checker (tests/shepard_oracle.py)."""
import time

import numpy as np
import pytest

import shepard_oracle as so
from surfh_amd import instru, models
from surfh_amd import preprocessing as P
from surfh_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(so.GOLDEN)


def _world(z):
    return (z["exp_alpha"], z["exp_beta"], z["exp_lam"])


@pytest.mark.parametrize("i", range(6))
def test_kernel_matches_reference(z, i):
    c = so.kernel_cases(z)[i]
    out, nbr = P.exponential_modified_shepard(c["a"], c["l"], c["v"], c["ga"], c["gl"], p=c["p"], alpha=2.0,
                                              pixel_cutoff=c["cutoff"], alpha_res=c["ares"], lambda_res=c["lres"],
                                              return_neighbours=True)
    assert out.shape == c["out"].shape and out.dtype == np.float32
    _, n = so.replica(c["a"], c["l"], c["v"], c["ga"], c["gl"], c["p"], c["cutoff"], c["ares"], c["lres"])
    assert np.array_equal(nbr.ravel(), n)
    err = np.max(np.abs(out - c["out"]))
    print(f"kernel case {i}: max |d| {err:.2e}, neighbours {n.min()}..{n.max()}")
    assert err <= 1e-5 * np.abs(c["v"]).max()


def test_separable_batch_equals_single_calls(z):
    cs = so.kernel_cases(z)
    segs = []
    for c in cs[:5]:                     # the first five cases are meshgrids: axes are row 0 / column 0
        segs.append((c["a"], c["l"], c["v"], c["ga"][0], c["gl"][:, 0], c["ares"], c["lres"]))
    for cut in (1.0, 2.0):
        res, cnt = P.shepard_segments(segs, p=2.0, pixel_cutoff=cut, neighbours=True)
        for k, s in enumerate(segs):
            one, n1 = P.exponential_modified_shepard(s[0], s[1], s[2], *np.meshgrid(s[3], s[4]), p=2.0,
                                                     pixel_cutoff=cut, alpha_res=s[5], lambda_res=s[6],
                                                     return_neighbours=True)
            assert np.array_equal(res[k], one) and np.array_equal(cnt[k], n1)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pipeline_matches_reference(z, mode):
    ch = so.ChannelShape(z["exp_oshape"])
    out, info = P.mrs_slices_distrorsion_correction(ch, z["exp_sorted"], _world(z), z["exp_data"], z["exp_cw"], mode,
                                                    return_info=True)
    ref = z[f"m{mode}_slices"]
    assert out.shape == ref.shape
    assert info["skipped"] == {0: [2], 1: [4], 2: []}[mode]          # sorted labels of the shifted slits
    # the same through a callable detector2world
    tab = _world(z)
    out2 = P.mrs_slices_distrorsion_correction(ch, z["exp_sorted"], lambda x, y: tuple(t[y, x] for t in tab),
                                               z["exp_data"], z["exp_cw"], mode)
    assert np.array_equal(out, out2)
    err = np.max(np.abs(out - ref))
    print(f"pipeline mode {mode}: max |d| {err:.2e}, skipped {info['skipped']}")
    assert err <= 1e-5 * np.nanmax(np.abs(z["exp_data"]))


def test_error_paths(z):
    data, lab = z["exp_data"], z["exp_sorted"]
    with pytest.raises(ValueError):          # 5 slits on the detector, a channel of 3
        P.mrs_slices_distrorsion_correction(so.ChannelShape((1, 3, len(z["exp_cw"]), 9)), lab, _world(z), data,
                                            z["exp_cw"], 2)
    ch = so.ChannelShape(z["exp_oshape"])
    with pytest.raises(ValueError):
        P.mrs_slices_distrorsion_correction(ch, lab, _world(z), data[:, :-1], z["exp_cw"], 2)
    with pytest.raises(ValueError):
        P.mrs_slices_distrorsion_correction(ch, lab, (z["exp_alpha"][:-1], z["exp_beta"], z["exp_lam"]), data,
                                            z["exp_cw"], 2)
    with pytest.raises(ValueError):
        P.mrs_slices_distrorsion_correction(ch, lab, _world(z), data, z["exp_cw"][:-1], 2)
    with pytest.raises(ValueError):
        P.exponential_modified_shepard(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros((2, 2)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        P.shepard_segments([(np.zeros(3), np.zeros(2), np.zeros(3), np.zeros(2), np.zeros(2), 1.0, 1.0)])


@pytest.fixture(scope="module")
def full():
    """A full-size channel-1A exposure (1024 rows, 21 slits of 24 columns) and its correction onto 1050 x 19."""
    e = synth.synthetic_mrs_exposure("1a")
    ifu = synth.band_ifu("1a")
    srf = instru.get_srf([ifu.det_pix_size], synth.STEP)[0]
    ax = synth.axes(251)
    ch = models.Channel(ifu, ax, ax, np.asarray(ifu.wavel_axis), srf, instru.CoordList([instru.Coord(0, 0)]),
                        synth.STEP_DEG)
    assert ch.oshape[1:] == (21, 1050, 19)
    world = (e["alpha"], e["beta"], e["lam"])
    wl = np.asarray(ifu.wavel_axis)
    P.mrs_slices_distrorsion_correction(ch, P.sort_labels_by_centroid(P.generate_label_image(~np.isnan(e["alpha"]))),
                                        world, e["data"], wl, 0)            # warm-up (library load, first launch)
    t0 = time.perf_counter()
    lab = P.sort_labels_by_centroid(P.generate_label_image(~np.isnan(e["alpha"])))
    t1 = time.perf_counter()
    out, info = P.mrs_slices_distrorsion_correction(ch, lab, world, e["data"], wl, 0, return_info=True)
    t2 = time.perf_counter()
    print(f"full-size 1A exposure: labelling {1e3 * (t1 - t0):.1f} ms, correction call {1e3 * (t2 - t1):.1f} ms "
          f"(GPU kernels {info['kernel_ms']:.2f} ms, HIP events), end to end {1e3 * (t2 - t0):.1f} ms")
    yield dict(e=e, ch=ch, lab=lab, out=out, info=info, wl=wl)
    ch.close()


def test_full_size_against_checker(full):
    e, lab, out, wl = full["e"], full["lab"], full["out"], full["wl"]
    assert out.shape == (21, 1050, 19) and full["info"]["skipped"] == []
    rng = np.random.default_rng(7)
    worst = 0.0
    for i, slit in enumerate(full["info"]["labels"]):
        pix = np.nonzero(lab == slit)
        a, l, v = e["alpha"][pix], e["lam"][pix], e["data"][pix]
        ga = np.linspace(a.min(), a.max(), 19)
        ok = ~np.isnan(v)
        ares, lres = (ga.max() - ga.min()) / 19, (wl.max() - wl.min()) / len(wl)
        q = rng.choice(1050 * 19, 2000, replace=False)
        qa, ql = ga[q % 19], wl[q // 19]
        m = so.neighbour_mask(a[ok], l[ok], qa, ql, ares, lres, 2.0)
        ref = so.checker(a[ok], l[ok], v[ok], qa, ql, m, 2.0, 2.0, ares, lres)
        worst = max(worst, float(np.max(np.abs(out[i].ravel()[q] - ref))))
    print(f"full size vs float64 checker: max |d| {worst:.2e} over 21 x 2000 grid points")
    assert worst <= 1e-5 * np.nanmax(np.abs(e["data"]))


def test_full_size_physics_and_cube(full):
    """On the smooth scene the corrected slices reproduce f(alpha, lambda) on the grid, and realData_sliceToCube takes
    them."""
    e, lab, out, wl, ch = full["e"], full["lab"], full["out"], full["wl"], full["ch"]
    errs = []
    for i, slit in enumerate(full["info"]["labels"]):
        a = e["alpha"][lab == slit]
        ga = np.linspace(a.min(), a.max(), 19)
        truth = e["scene"](*np.meshgrid(ga, wl))
        errs.append(np.max(np.abs(out[i] - truth)[5:-5, 1:-1]))          # away from the grid's border
    print(f"corrected slices vs the scene (interior): max |d| {max(errs):.3e} (scene amplitude 0.4)")
    assert max(errs) < 0.03
    cube = ch.realData_sliceToCube(P.reorder_corrected_slices(out, "1A"), (ch.oshape[2],) + ch.imshape)
    assert cube.shape == (1050, 251, 251) and np.isfinite(cube).all() and np.abs(cube).max() > 0
