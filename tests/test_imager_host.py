"""The imager data term without a GPU: the mirrored ``instru.WavelFilter`` against the reference's recorded results
(tests/golden/imager.npz), the float64 oracle of tests/imager_oracle.py that tests/test_gpu_imager.py compares the device with
(dot test, Fourier form through G against the plane-by-plane form), and every refusal that is raised before the library."""
import os

import numpy as np
import pytest

import imager_oracle as io
import problems
from surfh_amd import imager, instru
from surfh_amd.models import spectroSigRLSCT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "imager.npz")) as z:
        return {k: z[k] for k in z.files}


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.abs(b))))


def test_wavel_filter_reproduces_the_reference(golden):
    g = golden
    f = instru.WavelFilter(g["measured_wavelength"], g["measured_values"], name="f")
    assert np.array_equal(f.transmittance(g["axis"]), g["transmittance"])                       # bit for bit
    assert np.array_equal(f.transmittance(g["axis"], normalized=True), g["transmittance_normalized"])
    t = g["transmittance"]
    assert t[0] == 0 and t[-1] == 0 and np.count_nonzero(t) < len(t) - 4                         # the axis overhangs both sides
    hsi, spec = f.integrate_hsi(g["cube"], g["axis"]), f.integrate_spectrum(g["spectrum"], g["axis"])
    print(f"integrate_hsi {_ulps(hsi, g['integrate_hsi']):.1f} ulp, integrate_spectrum {_ulps(spec, g['integrate_spectrum']):.1f} ulp")
    assert hsi.shape == (6, 5) and _ulps(hsi, g["integrate_hsi"]) <= 4
    assert _ulps(spec, g["integrate_spectrum"]) <= 4


def test_msimager_is_the_references_dataclass():
    f = instru.WavelFilter([1.0, 2.0], [0.5, 0.5])
    ms = instru.MSImager(sotf=None, fov=instru.FOV(1.0, 1.0), wfilters=[f], det_pix_size=0.11)
    assert ms.wfilters == [f] and ms.det_pix_size == 0.11 and [x.name for x in instru.MSImager.__dataclass_fields__.values()] == \
        ["sotf", "fov", "wfilters", "det_pix_size"]


@pytest.mark.parametrize("d", [4, 1])
def test_oracle_dot_test_and_fourier_form(d):
    """Na=40, Nb=45 (odd), Lc=24, T=3, F=2: <u, A v> = <A^T u, v> to 1e-12, and the form through G equals the spatial form."""
    c = io.case(Na=40, Nb=45, Lc=24, T=3, F=2, d=d)
    im = c["im"]
    assert im.oshape == (2, 40 // d, 45 // d)
    av, atu = im.forward(c["x"]), im.adjoint(c["u"])
    gap = abs(np.vdot(c["u"], av) - np.vdot(atu, c["x"])) / (np.linalg.norm(c["u"]) * np.linalg.norm(av))
    ef = np.max(np.abs(im.forward_g(c["x"]) - av)) / np.max(np.abs(av))
    ea = np.max(np.abs(im.adjoint_g(c["u"]) - atu)) / np.max(np.abs(atu))
    print(f"d={d}: dot-test gap {gap:.2e}, Fourier form forward {ef:.2e}, adjoint {ea:.2e}")
    assert gap < 1e-12 and ef < 1e-12 and ea < 1e-12
    # the weighted normal operator is the composition, a weight of 0 takes its sample out
    w = c["w"]
    assert np.any(w == 0)
    want = im.adjoint(w * av)
    assert np.max(np.abs(im.fwadj(c["x"], w) - want)) <= 1e-12 * np.max(np.abs(want))
    if d == 4:                    # the last column (44) is not observed: it is in the null space of A and outside the range of A^T
        x2 = c["x"].copy()
        x2[:, :, 44] += 1.0
        assert np.any(atu[:, :, 44] != 0)          # (the blur spreads the observed columns into it)
        z = io.spread(c["u"], d, (40, 45))
        assert np.all(z[:, :, 44] == 0) and np.array_equal(io.sample(z, d), d * d * c["u"])


def test_joint_operator_restates_the_joint_criterion():
    from oracle import surfh_oracle as orc
    cfg = problems.two_channel_small()
    om = problems.oracle_model(cfg, box="direct")
    filters = imager.synthetic_filters(cfg["wavel"], 2)
    im = io.ImagerOracle(cfg["sotf"], cfg["templates"], filters, 3, (cfg["N"], cfg["N"]), fast=True)
    rng = np.random.default_rng(0)
    x = rng.random(om.ishape)
    y, y_im = rng.standard_normal(om.osize), rng.standard_normal(im.oshape)
    w = rng.random(om.osize)
    w_im = rng.random(im.oshape)
    w_im[0, 0, :3] = 0.0
    y_im_nan = y_im.copy()
    y_im_nan[0, 0, :3] = np.nan
    mu, mu_im, mur = 2.0, 0.7, 0.3
    j = io.Joint(om, im, mu, mu_im, w, w_im)
    assert orc.dottest_gap(j, np.random.default_rng(1)) < 1e-12
    r, ri = y - om.forward(x).ravel(), y_im - im.forward(x)
    want = (mu * np.sum(w * r * r) + mu_im * np.sum(w_im * ri * ri)) / 2 + orc.crit_val(om, om.forward(x), x, mu, mur)
    got = orc.crit_val(j, j.data(y, y_im_nan), x, mu, mur)
    assert abs(got - want) < 1e-12 * want


def test_synthetic_filters_tile_the_axis():
    wav = np.linspace(5.0, 7.0, 50)
    f = imager.synthetic_filters(wav, 4)
    assert f.shape == (4, 50) and np.all(f >= 0) and np.allclose(f.sum(axis=1), 1.0)
    assert list(np.argmax(f, axis=1)) == sorted(np.argmax(f, axis=1)) and len(set(np.argmax(f, axis=1))) == 4
    for bad in (0, 17):
        with pytest.raises(ValueError, match="1 to 16 filters"):
            imager.synthetic_filters(wav, bad)


def test_refusals_before_the_library():
    ok = np.ones((2, 24)) / 24
    with pytest.raises(ValueError, match="1 to 16 filters"):
        imager.check_filters(np.ones((17, 24)), 24)
    with pytest.raises(ValueError, match="expected \\[F, 24\\]"):
        imager.check_filters(np.ones((2, 23)), 24)
    for v, msg in ((-1e-3, ">= 0"), (np.nan, "finite"), (np.inf, "finite")):
        bad = ok.copy()
        bad[1, 5] = v
        with pytest.raises(ValueError, match=msg):
            imager.check_filters(bad, 24)
    for d in (0, -1, 41, 2.5):
        with pytest.raises(ValueError, match="decim"):
            imager.check_decim(d, (40, 45))
    assert imager.check_decim(40, (40, 45)) == 40
    assert imager.decim_from_pixel(0.11, 0.11 / 4 * (1 + 1e-7)) == 4
    with pytest.raises(ValueError, match="not a whole number"):
        imager.decim_from_pixel(0.11, 0.025)
    with pytest.raises(ValueError, match="not a whole number"):
        imager.decim_from_pixel(0.01, 0.025)                       # less than one cube pixel
    y = np.zeros(12)
    with pytest.raises(ValueError, match="12"):
        imager.check_imager_data(np.zeros(11), 1.0, None, 12)
    for mu in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="mu_imager"):
            imager.check_imager_data(y, mu, None, 12)
    for v, msg in ((-1.0, ">= 0"), (np.nan, "finite")):
        w = np.ones(12)
        w[3] = v
        with pytest.raises(ValueError, match=msg):
            imager.check_imager_data(y, 1.0, w, 12)

    class _Im:
        osize = 12

    m = object.__new__(spectroSigRLSCT)          # no plan: everything below is refused before the library is reached
    with pytest.raises(ValueError, match="no imager is attached"):
        m.set_imager_data(y, 1.0)
    with pytest.raises(ValueError, match="needs an attached imager"):
        m.cg(np.zeros(3), imager=(y, 1.0))
    m._imager = _Im()
    with pytest.raises(ValueError, match="data_delta"):
        m.cg(np.zeros(3), data_delta=3.0, imager=(y, 1.0))
    with pytest.raises(ValueError, match="imager data term"):
        m.mmmg(np.zeros(3), data_delta=3.0, imager=(y, 1.0))
    with pytest.raises(ValueError, match="mu_imager"):
        m.mmmg(np.zeros(3), imager=(y, -1.0))
    with pytest.raises(ValueError, match=r"\(y_im, mu_imager\)"):
        m.cg(np.zeros(3), imager=(y,))
    m._imager_data = (y, 1.0, None)               # a term set on the plan
    with pytest.raises(ValueError, match="imager data term"):
        m.mmmg(np.zeros(3), data_delta=3.0)
    with pytest.raises(ValueError, match="mmmg_vox does not carry the imager"):
        m.mmmg_vox(np.zeros(3))
    m._plan = None


class _Model:
    """What ``ImagerModel.__init__`` reads of a model; it makes no library call."""
    lmm = True
    ishape, cube_shape = (3, 40, 45), (24, 40, 45)
    step_degree = 0.025 / 3600
    wavelength_axis = np.linspace(5.0, 7.3, 24)


def test_model_from_an_msimager_without_the_library():
    """The ``MSImager`` branch: filters sampled with ``transmittance(normalized=True)``, the imager's own OTF, decim from
    ``det_pix_size`` over the cube step in arcsec."""
    m, wav = _Model(), _Model.wavelength_axis
    pts, vals = [[5.05, 5.5, 6.1, 6.4], [6.9, 7.2, 7.6, 8.0]], [[0.0, 1.0, 0.6, 0.0], [0.0, 0.5, 1.0, 0.0]]   # the second half off the axis
    fs = [instru.WavelFilter(a, b) for a, b in zip(pts, vals)]
    sotf = np.ones((24, 40, 23), dtype=np.complex64)
    ms = instru.MSImager(sotf=sotf, fov=instru.FOV(1.0, 1.0), wfilters=fs, det_pix_size=0.1)
    im = imager.ImagerModel(m, ms)
    want = np.array([np.interp(wav, a, b, left=0, right=0) for a, b in zip(pts, vals)])
    want /= want.sum(axis=1, keepdims=True)
    assert np.array_equal(im.filters, want) and want[1, -1] > 0 and want[0, 0] == 0
    assert im.decim == 4 and im.ishape == (3, 40, 45) and im.oshape == (2, 10, 11)
    assert im.sotf.dtype == np.complex128 and im.sotf.flags.c_contiguous and np.array_equal(im.sotf, sotf)
    assert imager.ImagerModel(m, ms, decim=5).oshape == (2, 8, 9)                       # a given decim wins
    other = np.linspace(5.0, 6.0, 24)                                                   # a given axis wins over the model's
    assert np.array_equal(imager.ImagerModel(m, ms.__class__(None, None, fs[:1], 0.1), wavelength_axis=other).filters[0],
                          fs[0].transmittance(other, normalized=True))
    assert imager.ImagerModel(m, ms.__class__(None, None, fs, 0.025)).sotf is None
    with pytest.raises(ValueError, match="not a whole number"):
        imager.ImagerModel(m, instru.MSImager(sotf=None, fov=None, wfilters=fs, det_pix_size=0.11))
    with pytest.raises(ValueError, match="imager sotf shape"):
        imager.ImagerModel(m, instru.MSImager(sotf=sotf[:, :, :22], fov=None, wfilters=fs, det_pix_size=0.1))
    with pytest.raises(ValueError, match="1 to 16 filters"):
        imager.ImagerModel(m, instru.MSImager(sotf=None, fov=None, wfilters=[], det_pix_size=0.1))
    with pytest.raises(ValueError, match="decim"):
        imager.ImagerModel(m, instru.MSImager(sotf=None, fov=None, wfilters=fs, det_pix_size=0.025 * 41))
    no_axis = _Model()
    no_axis.wavelength_axis = None
    with pytest.raises(ValueError, match="needs the wavelength axis"):
        imager.ImagerModel(no_axis, ms)
    no_tpl = _Model()
    no_tpl.lmm = False
    with pytest.raises(ValueError, match="templates"):
        imager.ImagerModel(no_tpl, want)
    with pytest.raises(RuntimeError, match="not the one installed"):
        im.forward(np.zeros(im.ishape))


def test_criterion_refusals_before_the_library():
    from surfh_amd.fusion import DistributedFusion, QuadCriterion_MRS
    m = _Model()
    im = imager.ImagerModel(m, np.ones((2, 24)) / 24, decim=4)
    y_im, y = np.zeros(im.oshape), np.zeros(7)
    names = dict(mu_imager=1.0, y_imager=y_im, model_imager=im)
    for given in (("mu_imager",), ("y_imager",), ("model_imager",), ("mu_imager", "y_imager"), ("y_imager", "model_imager")):
        with pytest.raises(ValueError, match="mu_imager, y_imager and model_imager together"):
            QuadCriterion_MRS(1.0, y, m, 1.0, **{k: names[k] for k in given})
    with pytest.raises(ValueError, match="weights_imager come with"):
        QuadCriterion_MRS(1.0, y, m, 1.0, weights_imager=np.ones(im.oshape))
    with pytest.raises(ValueError, match="data_delta.* does not carry the imager"):
        QuadCriterion_MRS(1.0, y, m, 1.0, data_delta=3.0, **names)
    with pytest.raises(ValueError, match="model_imager is not built on model_spectro"):
        QuadCriterion_MRS(1.0, y, _Model(), 1.0, **names)
    with pytest.raises(ValueError, match="the imager"):                                 # y_imager of another size than the imager's
        QuadCriterion_MRS(1.0, y, m, 1.0, **dict(names, y_imager=y_im[:, 1:]))
    with pytest.raises(ValueError, match="mu_imager"):
        QuadCriterion_MRS(1.0, y, m, 1.0, **dict(names, mu_imager=-1.0))
    bad_w = np.ones(im.oshape)
    bad_w[0, 0, 0] = -1.0
    with pytest.raises(ValueError, match=">= 0"):
        QuadCriterion_MRS(1.0, y, m, 1.0, weights_imager=bad_w, **names)
    with pytest.raises(ValueError, match="built on another model"):
        spectroSigRLSCT.set_imager(object.__new__(spectroSigRLSCT), im)
    for given in (("mu_imager",), ("y_imager",), ("model_imager",), tuple(names)):
        with pytest.raises(NotImplementedError, match="imager data term is not part of the multi-GPU solver"):
            DistributedFusion({}, **{k: names[k] for k in given})
