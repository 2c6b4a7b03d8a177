"""The imager data term on the device (surfh_set_imager, surfh_imager_forward / _adjoint / _fwadj, surfh_set_imager_data and the
solvers that carry the term) against the float64 restatement of tests/imager_oracle.py, whose own consistency
tests/test_imager_host.py checks without a GPU.  Needs an MI355X.

Bounds: the operator at the project's TOL (test_gpu_parity.py); the solvers at the bounds of their weighted twins in
test_gpu_weights.py (named at each test) -- the joint problem is the stacked least-squares problem of ``imager_oracle.Joint``, the
same algebra with more rows."""
import ctypes as C

import numpy as np
import pytest

import huber_oracle as ho
import imager_oracle as io
import problems
import weights_oracle as wo
from helpers import build_model, rel
from oracle import surfh_oracle as orc
from surfh_amd import _lib, imager, instru
from surfh_amd.imager import ImagerModel
from test_gpu_parity import TOL, note

pytestmark = pytest.mark.gpu
MU, MUR, NIT = wo.MU, wo.MUR, wo.NIT
MU_IM = 1.0
CG_GRADNORM_TOL, CG_ITERATE_TOL = 2e-4, 3e-3          # test_cg_matches_joint_oracle: the first ten r.r, the iterate


def _max_rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / b))


def _gap(u, av, atu, v):
    return abs(np.vdot(u, av) - np.vdot(atu, v)) / (np.linalg.norm(u) * np.linalg.norm(av))


def _set_data(m, y_im, w_im, mu):
    """surfh_set_imager_data on any model that owns a plan (Model_WCT has no Python method for it)."""
    y = np.ascontiguousarray(y_im, dtype=np.float32).ravel()
    w = None if w_im is None else np.ascontiguousarray(w_im, dtype=np.float32).ravel()
    _lib.check(m._L.surfh_set_imager_data(m._plan, _lib.fptr(y), None if w is None else _lib.fptr(w), float(mu)))


def _check_operator(tag, dev, im, x, u, w, m):
    """forward, adjoint, fwadj under weights with zeros, and the dot test of the device pair."""
    av, atu = dev.forward(x), dev.adjoint(u)
    ef, ea = rel(av, im.forward(x)), rel(atu, im.adjoint(u))
    _set_data(m, np.zeros(im.oshape), w, 0.0)                 # the weights of fwadj; mu = 0: no term
    en = rel(dev.fwadj(x), im.fwadj(x, w))
    _lib.check(m._L.surfh_set_imager_data(m._plan, None, None, 0.0))
    en1 = rel(dev.fwadj(x), im.fwadj(x))
    gap = _gap(u, av, atu, x)
    note("imager_operator", case=tag, err_forward=ef, err_adjoint=ea, err_fwadj_weighted=en, err_fwadj=en1, dot_gap=gap)
    assert av.shape == im.oshape and atu.shape == im.ishape
    assert ef < TOL and ea < TOL and en < TOL and en1 < TOL
    assert gap < 1e-6


# ---- 1. the stand-alone operator on a plan without channels ------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 1])
def test_stand_alone_operator(d):
    from surfh_amd.mixing import Model_WCT
    c = io.case(Na=40, Nb=45, Lc=24, T=3, F=2, d=d)
    wct = Model_WCT(c["psf"], c["tpl"], c["imshape"], np.ones(c["Lc"]))
    try:
        assert wct._L.surfh_imager_osize(wct._plan) == 0
        dev = ImagerModel(wct, c["filters"], decim=d).attach()
        assert dev.oshape == c["im"].oshape and wct._L.surfh_imager_osize(wct._plan) == c["im"].osize
        _check_operator(f"wct_d{d}", dev, c["im"], c["x"], c["u"], c["w"], wct)
        # the spectrometer-side calls of the plan are untouched by the imager
        cube = wct.forward(c["x"])
        want = np.fft.irfft2(np.fft.rfft2(np.einsum("tl,tab->lab", c["tpl"], c["x"]), norm="ortho") * c["sotf"], s=c["imshape"], norm="ortho")
        assert rel(cube, want) < TOL
    finally:
        wct.close()


# ---- 2. filters, the imager's own OTF, the streamed set-up ------------------------------------------------------------------------
def _three_filters(wav):
    """One over the whole axis, one two planes wide, one half off the axis (its measured points start below the axis)."""
    whole = np.full(len(wav), 1.0 / len(wav))
    two = np.zeros(len(wav))
    two[60:62] = 0.5
    step = wav[1] - wav[0]
    off = instru.WavelFilter([wav[0] - 6 * step, wav[0], wav[0] + 6 * step], [0.0, 1.0, 0.0]).transmittance(wav, normalized=True)
    assert off[0] > 0 and np.count_nonzero(off) == 6
    return np.array([whole, two, off])


@pytest.fixture(scope="module")
def c1():
    cfg = problems.config1()
    m = build_model(cfg)
    rng = np.random.default_rng(11)
    yield cfg, m, rng.standard_normal(m.ishape), rng
    m.close()


def test_filters_on_config1(c1):
    cfg, m, x, rng = c1
    N, d = cfg["N"], 3
    filters = _three_filters(cfg["wavel"])
    im = io.ImagerOracle(cfg["sotf"], cfg["templates"], filters, d, (N, N))
    assert im.oshape == (3, 21, 21)                             # 64 // 3: one row and one column are not observed
    dev = ImagerModel(m, filters, decim=d)
    m.set_imager(dev)
    try:
        u = rng.standard_normal(im.oshape)
        w = np.exp(rng.uniform(np.log(0.5), np.log(2.0), im.oshape))
        w[rng.random(im.oshape) < 0.15] = 0.0
        _check_operator("config1_three_filters", dev, im, x, u, w, m)
    finally:
        m.set_imager(None)
    assert m._L.surfh_imager_osize(m._plan) == 0


def test_own_otf_and_chunked_build(c1, monkeypatch):
    cfg, m, x, rng = c1
    N, d = cfg["N"], 3
    filters = _three_filters(cfg["wavel"])
    own = io.gaussian_sotf(np.linspace(1.5, 3.0, cfg["Lc"]), (N, N))          # not the spectrometer's widths
    im = io.ImagerOracle(own, cfg["templates"], filters, d, (N, N))
    dev = ImagerModel(m, filters, decim=d)
    dev.sotf = np.ascontiguousarray(own, dtype=np.complex128)
    try:
        m.set_imager(dev)
        e = rel(dev.forward(x), im.forward(x))
        e_other = rel(dev.forward(x), io.ImagerOracle(cfg["sotf"], cfg["templates"], filters, d, (N, N)).forward(x))
        g_one = m.debug_buffer("imager_g").copy()               # Lc = 128: one chunk
        monkeypatch.setenv("SURFH_IMAGER_CHUNK", "32")
        m.set_imager(dev)
        g_four = m.debug_buffer("imager_g").copy()
        monkeypatch.delenv("SURFH_IMAGER_CHUNK")
        note("imager_own_otf", err_forward=e, against_the_spectrometers_otf=e_other)
        assert e < TOL and e_other > 1e2 * TOL
        assert g_one.shape[0] == 3 * 4 and np.any(g_one != 0) and np.array_equal(g_one, g_four)
        want = np.zeros(g_one.shape)
        G = im.G.reshape(12, N, N // 2 + 1)
        want[:, 0, :N, :N // 2 + 1], want[:, 1, :N, :N // 2 + 1] = G.real, G.imag
        assert rel(g_one, want) < 1e-6                          # float64 accumulation of fp32 operands, stored fp32
        monkeypatch.setenv("SURFH_IMAGER_CHUNK", "48")
        with pytest.raises(ValueError, match="SURFH_IMAGER_CHUNK"):
            m.set_imager(dev)
    finally:
        monkeypatch.delenv("SURFH_IMAGER_CHUNK", raising=False)
        m.set_imager(None)


def test_model_from_an_msimager(c1):
    """``ImagerModel(model, MSImager)``: the filters are the ``WavelFilter``s sampled on the model's wavelength axis and normalised,
    the OTF is the imager's own, decim comes from the detector pixel over the cube step.  The oracle gets all three restated."""
    cfg, m, x, rng = c1
    N, wav = cfg["N"], cfg["wavel"]
    step = wav[1] - wav[0]
    pts = [wav[20] + step * np.array([0.3, 9.1, 17.5, 26.2, 33.9, 41.4, 50.7]), wav[-1] + step * np.array([-30.5, -12.25, 0.5, 14.0])]
    vals = [np.array([0.0, 0.4, 0.9, 1.0, 0.7, 0.2, 0.0]), np.array([0.0, 0.8, 1.0, 0.0])]          # the second one half off the axis
    own = io.gaussian_sotf(np.linspace(1.5, 3.0, cfg["Lc"]), (N, N))
    ms = instru.MSImager(sotf=own, fov=instru.FOV(1.0, 1.0), wfilters=[instru.WavelFilter(a, b, name=f"f{i}") for i, (a, b) in enumerate(zip(pts, vals))],
                         det_pix_size=3 * problems.STEP)
    want = np.array([np.interp(wav, a, b, left=0, right=0) for a, b in zip(pts, vals)])
    want /= want.sum(axis=1, keepdims=True)
    assert want[1, -1] > 0 and np.count_nonzero(want[1]) == 31 and np.count_nonzero(want[0]) == 50
    dev = ImagerModel(m, ms)
    assert dev.decim == 3 and dev.oshape == (2, 21, 21) and np.array_equal(dev.filters, want) and np.array_equal(dev.sotf, own)
    assert ImagerModel(m, ms, decim=2).decim == 2                                                   # a given decim wins
    with pytest.raises(ValueError, match="not a whole number"):
        ImagerModel(m, instru.MSImager(sotf=own, fov=None, wfilters=ms.wfilters, det_pix_size=2.5 * problems.STEP))
    im = io.ImagerOracle(own, cfg["templates"], want, 3, (N, N))
    m.set_imager(dev)
    try:
        u = rng.standard_normal(im.oshape)
        _check_operator("config1_msimager", dev, im, x, u, np.where(rng.random(im.oshape) < 0.2, 0.0, 1.5), m)
    finally:
        m.set_imager(None)


def _spec_is_interleaved(wct):
    dims = (C.c_int64 * 4)()
    _lib.check(wct._L.surfh_debug_dims(wct._plan, b"spec", dims))
    return dims[3] == 2


@pytest.mark.parametrize("dense", [False, True], ids=["interleaved_otf", "planar_otf"])
def test_the_plans_own_otf_in_both_layouts(dense, monkeypatch):
    """Without an OTF of its own the imager builds G from the plan's device OTF, which a plan keeps interleaved (re, im innermost)
    for the fast transform kernels and planar under SURFH_DFT_DENSE=1 (read at plan creation): G, through the operator, in both."""
    from surfh_amd.mixing import Model_WCT
    c = io.case(Na=64, Nb=64, Lc=128, T=3, F=2, d=4)
    if dense:
        monkeypatch.setenv("SURFH_DFT_DENSE", "1")
    wct = Model_WCT(c["psf"], c["tpl"], c["imshape"], np.ones(c["Lc"]))
    monkeypatch.delenv("SURFH_DFT_DENSE", raising=False)
    try:
        assert _spec_is_interleaved(wct) == (not dense)
        dev = ImagerModel(wct, c["filters"], decim=4).attach()
        assert dev.sotf is None
        _check_operator(f"wct_own_otf_dense{int(dense)}", dev, c["im"], c["x"], c["u"], c["w"], wct)
    finally:
        wct.close()


# ---- 3. the solvers on the joint problem --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joint():
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    N, d = cfg["N"], 3
    filters = imager.synthetic_filters(cfg["wavel"], 3)
    im = io.ImagerOracle(cfg["sotf"], cfg["templates"], filters, d, (N, N), fast=True)
    m.set_imager(ImagerModel(m, filters, decim=d))
    p = wo.standard(cfg, om)
    yi = im.forward(cfg["maps"])
    p["y_im"] = yi + np.random.default_rng(2).standard_normal(yi.shape) * 1e-2 * np.sqrt(np.mean(yi ** 2))
    rng = np.random.default_rng(6)
    p["w_im"] = np.exp(rng.uniform(np.log(0.5), np.log(2.0), yi.shape))
    p["w_im"][rng.random(yi.shape) < 0.12] = 0.0
    yield cfg, om, im, m, p
    m.close()


def test_cg_matches_joint_oracle(joint):
    """Bounds of test_gpu_weights.py::test_cg_matches_weighted_oracle."""
    cfg, om, im, m, p = joint
    j = io.Joint(om, im, MU, MU_IM)
    ref = orc.lcg(j, j.data(p["y_clean"], p["y_im"]), MU, MUR, np.zeros(om.ishape), tol=1e-12, max_iter=NIT)
    gr = np.array(ref["grad_norm"])
    x, gn, n = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=NIT, tol=1e-12, imager=(p["y_im"], MU_IM))
    e, ge = rel(x, ref["x"]), _max_rel(gn[:10], gr[:10])
    note("imager_cg", err_x=e, err_gradnorm_first10=ge, err_gradnorm_all=_max_rel(gn, gr))
    assert n == NIT and len(gn) == NIT + 1 and m.imager_data is None and not m.has_imager_term()
    assert ge < CG_GRADNORM_TOL and e < CG_ITERATE_TOL


def test_the_term_bites(joint):
    """Same problem and iteration count: the iterate moves by more than ten times the iterate tolerance of the test above, towards
    the imager's data."""
    cfg, om, im, m, p = joint
    x1, _, _ = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=NIT, imager=(p["y_im"], MU_IM))
    x0, _, _ = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=NIT, imager=(p["y_im"], 0.0))
    r1, r0 = np.linalg.norm(p["y_im"] - im.forward(x1)), np.linalg.norm(p["y_im"] - im.forward(x0))
    note("imager_bites", iterate_change=rel(x1, x0), imager_residual_with=r1, imager_residual_without=r0)
    assert rel(x1, x0) > 10 * 3e-3 and r1 < r0


def test_cg_with_weights_on_both_instruments(joint):
    """The bounds of test_cg_matches_joint_oracle; a NaN under a zero imager weight and the spikes under zero data weights."""
    cfg, om, im, m, p = joint
    j = io.Joint(om, im, MU, MU_IM, p["w"], p["w_im"])
    y_im_nan = np.where(p["w_im"] == 0, np.nan, p["y_im"])
    y_nan = np.where(p["masked"], np.nan, p["y"])
    ref = orc.lcg(j, j.data(y_nan, y_im_nan), MU, MUR, np.zeros(om.ishape), tol=1e-12, max_iter=NIT)
    gr = np.array(ref["grad_norm"])
    x, gn, n = m.cg(y_nan, mu=MU, mu_reg=MUR, max_iter=NIT, tol=1e-12, weights=p["w"], imager=(y_im_nan, MU_IM, p["w_im"]))
    e, ge = rel(x, ref["x"]), _max_rel(gn[:10], gr[:10])
    note("imager_cg_weighted", err_x=e, err_gradnorm_first10=ge)
    assert np.isfinite(x).all() and n == NIT and ge < CG_GRADNORM_TOL and e < CG_ITERATE_TOL


def test_mmmg_matches_joint_oracle(joint):
    """Bounds of test_gpu_weights.py::test_mmmg_matches_weighted_oracle (x0 = 0.5, 8 iterations)."""
    cfg, om, im, m, p = joint
    j = io.Joint(om, im, MU, MU_IM)
    x0 = np.ones(m.ishape) * 0.5
    ref = orc.mmmg(j, j.data(p["y_clean"], p["y_im"]), MU, MUR, x0, max_iter=8)
    x, gn, n = m.mmmg(p["y_clean"], mu=MU, mu_reg=MUR, x0=x0, max_iter=8, imager=(p["y_im"], MU_IM))
    e, ge = rel(x, ref["x"]), _max_rel(gn, ref["grad_norm"])
    note("imager_mmmg", err_x=e, err_gradnorm=ge)
    assert n == 8 and gn.shape == (9,) and e < 1e-4 and ge < 2e-4


def test_mmmg_huber_matches_joint_oracle(joint):
    """Bounds and regime of test_gpu_weights.py::test_mmmg_huber_matches_weighted_oracle (textured start, delta 0.1)."""
    cfg, om, im, m, p = joint
    j = io.Joint(om, im, MU, MU_IM)
    delta = 0.1
    x0 = cfg["maps"] + 0.1 * np.random.default_rng(3).standard_normal(m.ishape)
    ref = ho.mmmg(j, j.data(p["y_clean"], p["y_im"]), MU, MUR, delta, x0, max_iter=8)
    x, gn, n = m.mmmg(p["y_clean"], mu=MU, mu_reg=MUR, x0=x0, max_iter=8, delta=delta, imager=(p["y_im"], MU_IM))
    e, ge = rel(x, ref["x"]), _max_rel(gn, ref["grad_norm"])
    note("imager_mmmg_huber", err_x=e, err_gradnorm=ge)
    assert n == 8 and gn.shape == (9,) and e < 1e-4 and ge < 2e-4


@pytest.mark.parametrize("delta", [None, 0.1], ids=["quadratic", "huber"])
def test_mmmg_with_weights_on_both_instruments(joint, delta):
    """The 3MG loops under data weights on both instruments (the window with w_im inside the loop), a NaN under every zero weight;
    bounds and starts of the two tests above."""
    cfg, om, im, m, p = joint
    j = io.Joint(om, im, MU, MU_IM, p["w"], p["w_im"])
    y_im_nan = np.where(p["w_im"] == 0, np.nan, p["y_im"])
    y_nan = np.where(p["masked"], np.nan, p["y"])
    data = j.data(y_nan, y_im_nan)
    if delta is None:
        x0 = np.ones(m.ishape) * 0.5
        ref = orc.mmmg(j, data, MU, MUR, x0, max_iter=8)
    else:
        x0 = cfg["maps"] + 0.1 * np.random.default_rng(3).standard_normal(m.ishape)
        ref = ho.mmmg(j, data, MU, MUR, delta, x0, max_iter=8)
    x, gn, n = m.mmmg(y_nan, mu=MU, mu_reg=MUR, x0=x0, max_iter=8, delta=delta, weights=p["w"], imager=(y_im_nan, MU_IM, p["w_im"]))
    e, ge = rel(x, ref["x"]), _max_rel(gn, ref["grad_norm"])
    note("imager_mmmg_weighted", delta=delta or 0.0, err_x=e, err_gradnorm=ge)
    print(f"weighted mmmg, delta {delta}: iterate {e:.2e}, trace {ge:.2e}")
    assert np.isfinite(x).all() and n == 8 and gn.shape == (9,) and e < 1e-4 and ge < 2e-4
    assert m.imager_data is None and m.data_weights is None


def test_a_term_set_before_is_put_back(joint):
    """``cg(imager=...)`` sets its term for the call; a term ``set_imager_data`` had set before is back afterwards, the way
    ``weights=`` puts the model's weights back."""
    cfg, om, im, m, p = joint
    m.set_imager_data(p["y_im"], 0.5, p["w_im"])
    try:
        held = m.imager_data
        a = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=3)
        b = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=3, imager=(p["y_im"], MU_IM))
        assert m.has_imager_term() and m.imager_data[1] == 0.5
        assert all(np.array_equal(u, v) for u, v in zip(held[::2], m.imager_data[::2]))
        c = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=3)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and not np.array_equal(a[0], b[0])
    finally:
        m.set_imager_data(None)
    assert m.imager_data is None and not m.has_imager_term()


def test_criterion_includes_the_term(joint):
    from surfh_amd.fusion import QuadCriterion_MRS
    cfg, om, im, m, p = joint
    j = io.Joint(om, im, MU, MU_IM, None, p["w_im"])
    y_im_nan = np.where(p["w_im"] == 0, np.nan, p["y_im"])
    q = QuadCriterion_MRS(MU, p["y_clean"], m, MUR, mu_imager=MU_IM, y_imager=y_im_nan, model_imager=m.imager, weights_imager=p["w_im"])
    res = q.run_method("lcg", 6, value_init=0)
    x = res.x.reshape(m.ishape)
    got, want = q.get_crit_val(x), orc.crit_val(j, j.data(p["y_clean"], y_im_nan), x, MU, MUR)
    assert abs(got - want) < 1e-5 * want and m.imager_data is None
    assert np.array_equal(x, m.cg(p["y_clean"], mu=MU, mu_reg=MUR, x0=np.zeros(m.ishape), max_iter=6, imager=(y_im_nan, MU_IM, p["w_im"]))[0])
    plain = QuadCriterion_MRS(MU, p["y_clean"], m, MUR)
    assert got > plain.get_crit_val(x)


# ---- 4. nothing changes without it -----------------------------------------------------------------------------------------------------
def test_nothing_changes_without_the_term(joint):
    cfg, om, im, m, p = joint
    fresh = build_model(cfg)
    x0 = np.ones(m.ishape) * 0.5
    try:
        def run(mm):
            a = mm.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=NIT)[:2]
            b = mm.mmmg(p["y_clean"], mu=MU, mu_reg=MUR, x0=x0, max_iter=4)[:2]
            c = mm.mmmg(p["y_clean"], mu=MU, mu_reg=MUR, x0=x0, max_iter=4, delta=0.1)[:2]
            return a + b + c
        want = run(fresh)

        def same(got):
            return all(np.array_equal(g, w) for g, w in zip(got, want))
        assert m.imager is not None and m.imager_data is None
        m.profile_enable(True)
        m.profile_reset()
        assert same(run(m))                                           # attached, no data
        m.set_imager_data(p["y_im"], 0.0, p["w_im"])
        assert not m.has_imager_term() and same(run(m))               # attached, mu_imager = 0
        names = list(m.profile())
        m.profile_enable(False)
        assert names and not [k for k in names if k.startswith("imager")], names
        m.set_imager_data(p["y_im"], MU_IM)
        assert m.has_imager_term() and not same(run(m))
        m.profile_enable(True)
        m.profile_reset()
        m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=2)
        with_term = set(m.profile())
        m.profile_enable(False)
        assert {"imager_mix_fwd", "imager_mix_adj", "imager_window", "imager_spread"} <= with_term, with_term
        m.set_imager_data(None)
        assert not m.has_imager_term() and same(run(m))               # data cleared
        kept = m.imager
        m.set_imager(None)
        assert m._L.surfh_imager_osize(m._plan) == 0 and same(run(m))   # detached
        m.set_imager(kept)
    finally:
        fresh.close()


# ---- 5. a plan that has the spectral-domain loop -----------------------------------------------------------------------------------------
def test_spectral_capable_plan_takes_the_map_domain_loop():
    """two_channel_mid, the iteration count of test_gpu_weights.py::test_spectral_cg_matches_weighted_oracle, at the bounds of
    test_cg_matches_joint_oracle: first ten r.r and the iterate."""
    cfg = problems.two_channel_mid()
    om = problems.oracle_model(cfg, box="direct")
    N, d = cfg["N"], 4
    filters = imager.synthetic_filters(cfg["wavel"], 2)
    im = io.ImagerOracle(cfg["sotf"], cfg["templates"], filters, d, (N, N), fast=True)
    p = wo.standard(cfg, om)
    yi = im.forward(cfg["maps"])
    y_im = yi + np.random.default_rng(2).standard_normal(yi.shape) * 1e-2 * np.sqrt(np.mean(yi ** 2))
    j = io.Joint(om, im, MU, MU_IM)
    ref = orc.lcg(j, j.data(p["y_clean"], y_im), MU, MUR, np.zeros(om.ishape), tol=1e-12, max_iter=9)
    gr = np.array(ref["grad_norm"])
    m = build_model(cfg)
    try:
        assert m.spec_supported()
        m.set_imager(ImagerModel(m, filters, decim=d))
        m.profile_enable(True)
        x, gn, n = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=9, tol=1e-12, imager=(y_im, MU_IM))
        stages = set(m.profile())
        m.profile_reset()
        x0, gn0, n0 = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=9, tol=1e-12)
        stages0 = set(m.profile())
        m.profile_enable(False)
    finally:
        m.close()
    e, ge = rel(x, ref["x"]), _max_rel(gn[:10], gr[:10])
    note("imager_cg_spectral_capable", err_x=e, err_gradnorm_first10=ge)
    print(f"two_channel_mid, 9 iterations: iterate {e:.2e}, first ten r.r {ge:.2e}")
    assert n == 9 and len(gn) == 10 and ge < 2e-4 and e < 3e-3
    assert "prior_add" in stages and "imager_window" in stages              # the map-domain loop ran
    assert n0 == 9 and len(gn0) == 10 and "prior_add" not in stages0 and not [k for k in stages0 if k.startswith("imager")]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_solvers_without_the_term_refuse_it(joint):
    import torch
    cfg, om, im, m, p = joint
    y = p["y_clean"]
    with pytest.raises(ValueError, match="imager"):
        m.mmmg(y, data_delta=3.0, imager=(p["y_im"], MU_IM))
    m.set_imager_data(p["y_im"], MU_IM)
    try:
        with pytest.raises(ValueError, match="imager"):
            m.mmmg(y, data_delta=3.0)
        with pytest.raises(ValueError, match="imager"):
            m.mmmg_vox(y)
        L = m._L
        with pytest.raises(RuntimeError, match="surfh_mmmg_robust does not carry the imager"):
            _lib.solve_robust(m, y, 1.0, 3.0, 1.0, 1.0, None, 2, 1e-12, 50, None)
        with pytest.raises(RuntimeError, match="surfh_mmmg_robust_vox does not carry the imager"):
            _lib.solve_robust_vox(m, y, 1.0, 3.0, 1.0, 1.0, 1.0, 1.0, None, 2, 1e-12, 50, None)
        with pytest.raises(RuntimeError, match="surfh_mmmg_huber_vox does not carry the imager"):
            _lib.solve_huber_vox(m, y, 1.0, 1.0, 1.0, 1.0, 1.0, None, 2, 1e-12, 50, None)
        with pytest.raises(RuntimeError, match="surfh_cg_planes does not carry the imager"):
            _lib.solve(m, L.surfh_cg_planes_cb, y, 1.0, 1.0, None, 2, 1e-12, 50, None)
        with pytest.raises(RuntimeError, match="surfh_mmmg_planes does not carry the imager"):
            _lib.solve(m, L.surfh_mmmg_planes_cb, y, 1.0, 1.0, None, 2, 1e-12, 50, None)
        with pytest.raises(RuntimeError, match="surfh_mmmg_huber_planes does not carry the imager"):
            _lib.solve_huber_planes(m, y, 1.0, 1.0, 1.0, None, 2, 1e-12, 50, None, 1, True)
        y_t = torch.zeros(m.osize, device="cuda:0")
        x_t = torch.zeros(m.isize, device="cuda:0")
        torch.cuda.synchronize()
        assert L.surfh_cg_planes_begin_dev(m._plan, C.c_void_p(y_t.data_ptr()), 1.0, 1.0, C.c_void_p(x_t.data_ptr())) != 0
        assert "surfh_cg_planes_begin_dev does not carry the imager" in L.surfh_last_error().decode()
    finally:
        m.set_imager_data(None)


def test_refused_imager_leaves_the_previous_one_working(joint):
    cfg, om, im, m, p = joint
    L = m._L
    dev = m.imager
    before = dev.forward(cfg["maps"])
    ok = np.ascontiguousarray(dev.filters)
    sotf = np.ascontiguousarray(cfg["sotf"], dtype=np.complex128)

    def attempt(filters, decim, own=True):
        d = _lib.ImagerDesc()
        f = np.ascontiguousarray(filters, dtype=np.float64)
        d.n_filters, d.filters, d.decim = f.shape[0], _lib.dptr(f), decim
        d.sotf = sotf.view(np.float64).ctypes.data_as(_lib.c_double_p) if own else None
        rc = L.surfh_set_imager(m._plan, C.byref(d))
        return rc, L.surfh_last_error().decode()
    neg, nan = ok.copy(), ok.copy()
    neg[1, 7], nan[2, 100] = -1e-3, np.nan
    for args, word in (((np.ones((17, ok.shape[1])), 3), "1..16"), ((ok[:0], 3), "1..16"), ((ok, 0), "decim"), ((ok, 65), "decim"),
                       ((neg, 3), ">= 0"), ((nan, 3), ">= 0"), ((ok, 3, False), "does not own every cube plane")):
        rc, msg = attempt(*args)
        assert rc != 0 and "imager" in msg and word in msg, (args[1:], msg)
        assert L.surfh_imager_osize(m._plan) == dev.osize
    assert np.array_equal(dev.forward(cfg["maps"]), before)
    # weights and mu_imager
    y = np.zeros(dev.osize, dtype=np.float32)
    for v in (-1.0, np.nan, np.inf):
        w = np.ones(dev.osize, dtype=np.float32)
        w[5] = v
        assert L.surfh_set_imager_data(m._plan, _lib.fptr(y), _lib.fptr(w), 1.0) != 0 and "weight" in L.surfh_last_error().decode()
    assert L.surfh_set_imager_data(m._plan, _lib.fptr(y), None, -1.0) != 0 and "mu_imager" in L.surfh_last_error().decode()
    assert not m.has_imager_term()
    # a plan without templates
    cfg0 = dict(cfg, templates=None)
    m0 = build_model(cfg0)
    try:
        with pytest.raises(ValueError, match="templates"):
            ImagerModel(m0, np.ones((1, cfg["Lc"])), decim=1)
        d = _lib.ImagerDesc()
        d.n_filters, d.filters, d.decim, d.sotf = ok.shape[0], _lib.dptr(ok), 3, None
        assert L.surfh_set_imager(m0._plan, C.byref(d)) != 0 and "templates" in L.surfh_last_error().decode()
        x = np.zeros(4, dtype=np.float32)
        assert L.surfh_imager_forward(m0._plan, _lib.fptr(x), _lib.fptr(x)) != 0 and "no imager" in L.surfh_last_error().decode()
    finally:
        m0.close()
