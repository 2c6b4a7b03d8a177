"""Per-sample data weights on the device (surfh_set_data_weights): the criterion mu (y - A x)^T W (y - A x) / 2 + priors against the
float64 oracles on A~ = W^(1/2) A, y~ = W^(1/2) y (tests/weights_oracle.py), whose preconditions tests/test_weights_host.py
checks without a GPU.  Needs an MI355X.

Every bound is the one its unweighted twin asserts (named at each test): the weights of the standard problem lie in [0.5, 2] or
are 0, so A~ has the conditioning of A up to that factor, and the weighted operator adds one fp32 multiplication per sample."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import huber_oracle as ho
import problems
import vox_oracle as vo
import weights_oracle as wo
from helpers import build_model, rel
from oracle import surfh_oracle as orc
from test_gpu_parity import TOL, note

pytestmark = pytest.mark.gpu
MU, MUR, NIT = wo.MU, wo.MUR, wo.NIT


@pytest.fixture(scope="module")
def std():
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    p = wo.standard(cfg, om)
    p["om_w"], p["y_w"] = wo.Weighted(om, p["w"]), wo.wdata(p["w"], p["y"])
    yield cfg, om, m, p
    m.close()


def _normal(m, d, mu=1.0):
    import torch
    d_t = torch.as_tensor(np.ascontiguousarray(d, dtype=np.float32), device="cuda:0")
    q_t = torch.empty_like(d_t)
    torch.cuda.synchronize()
    m.normal_dev(d_t, q_t, mu)
    torch.cuda.synchronize()
    return q_t.cpu().numpy()


def _max_rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / b))


# ---- 1. w = 1 is the unweighted path, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["config1", "two_channel_mid"])
def test_unit_weights_are_the_unweighted_path(name):
    cfg = getattr(problems, name)()
    m, fresh = build_model(cfg), build_model(cfg)
    try:
        if name == "two_channel_mid":
            assert m.spec_supported()          # fused tail, grouped adjoint GEMMs, K-step classes, Ldet = 390 (390 % 4 = 2)
        y = fresh.forward(cfg["maps"])
        y = y + np.random.default_rng(1).standard_normal(y.size) * 1e-2 * np.sqrt(np.mean(y ** 2))
        d = np.random.default_rng(3).standard_normal(m.ishape)

        def run(mm):
            return (_normal(mm, d),) + tuple(mm.cg(y, mu=MU, mu_reg=MUR, max_iter=NIT)[:2])
        q0, x0, g0 = run(fresh)
        assert m.data_weights is None
        m.set_data_weights(np.ones(m.osize))
        assert m._L.surfh_has_data_weights(m._plan) == 1 and np.array_equal(m.data_weights, np.ones(m.osize, dtype=np.float32))
        q1, x1, g1 = run(m)
        assert np.array_equal(q1, q0) and np.array_equal(x1, x0) and np.array_equal(g1, g0)
        x1b, g1b, _ = fresh.cg(y, mu=MU, mu_reg=MUR, max_iter=NIT, weights=np.ones(m.osize))     # installed for one solve
        assert np.array_equal(x1b, x0) and np.array_equal(g1b, g0) and fresh.data_weights is None
        m.set_data_weights(None)
        assert m._L.surfh_has_data_weights(m._plan) == 0 and m.data_weights is None
        q2, x2, g2 = run(m)
        assert np.array_equal(q2, q0) and np.array_equal(x2, x0) and np.array_equal(g2, g0)
    finally:
        m.close()
        fresh.close()


# ---- 2. the hand-over kernel's shapes ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """config1 with a detector axis of 1101 samples: operand rows of pitch 1152 (the hand-over kernel's second register tile),
    1101 % 4 = 1, 80 of 128 operand rows."""
    cfg = problems.config1()
    cfg["specs"] = [dataclasses.replace(cfg["specs"][0], wavel_axis=np.linspace(7.52, 7.68, 1101))]
    om = problems.oracle_model(cfg, box="direct")
    assert om.osize == 88080
    y_true = om.forward(cfg["maps"])
    w, _, masked = wo.recipe(y_true, y_true)
    return cfg, om, w, om.adjoint(w * y_true)


@pytest.mark.parametrize("plan", ["default", "verify", "wblur_fp32"])
def test_weighted_normal_operator_on_a_wide_detector(wide, plan, monkeypatch):
    """A^T W A d against the oracle, at the bound of the unweighted operator tests (TOL of test_gpu_parity.py): through the
    weighted hand-over kernel (default plan) and through the element-wise weight kernel on y (verify, SURFH_WBLUR_FP32=1)."""
    cfg, om, w, want = wide
    if plan == "wblur_fp32":
        monkeypatch.setenv("SURFH_WBLUR_FP32", "1")
    m = build_model(cfg, verify=plan == "verify")
    try:
        m.set_data_weights(w)
        e = rel(_normal(m, cfg["maps"]), want)
        e_host = rel(m.fwadj(cfg["maps"]), want)
        m.set_data_weights(None)
        e_off = rel(_normal(m, cfg["maps"]), want)
    finally:
        m.close()
    note("weights_normal_wide", plan=plan, err=e, err_fwadj=e_host, unweighted_vs_weighted=e_off)
    assert e < TOL and e_host < TOL
    assert e_off > 1e3 * TOL                    # the weights are in play: without them the result is far outside the tolerance


# ---- 3. the solvers on the standard weighted problem against the wrapped oracle ---------------------------------------------------
def test_cg_matches_weighted_oracle(std):
    """Bounds of test_gpu_parity.py::test_cg_matches_oracle_lcg, production and verification plan."""
    cfg, om, m, p = std
    ref = orc.lcg(p["om_w"], p["y_w"], MU, MUR, np.zeros(om.ishape), tol=1e-12, max_iter=NIT)
    gr = np.array(ref["grad_norm"])
    x, gn, n = m.cg(p["y"], mu=MU, mu_reg=MUR, max_iter=NIT, tol=1e-12, weights=p["w"])
    e, ge = rel(x, ref["x"]), _max_rel(gn[:10], gr[:10])
    note("weights_cg", err_x=e, err_gradnorm_first10=ge, err_gradnorm_all=_max_rel(gn, gr))
    assert n == NIT and len(gn) == NIT + 1 and m.data_weights is None
    assert ge < 2e-4 and e < 3e-3
    mv = build_model(cfg, verify=True)
    try:
        xv, gv, _ = mv.cg(p["y"], mu=MU, mu_reg=MUR, max_iter=NIT, tol=1e-12, weights=p["w"])
    finally:
        mv.close()
    ev, gev = rel(xv, ref["x"]), _max_rel(gv[:10], gr[:10])
    note("weights_cg_verify", err_x=ev, err_gradnorm_first10=gev)
    assert gev < 5e-5 and ev < 1e-3


def test_spectral_cg_matches_weighted_oracle():
    """The spectral-domain loop (surfh_normal_spec_dev) on two_channel_mid, the standard recipe: the first ten r.r at the bound of
    test_cg_matches_oracle_lcg."""
    cfg = problems.two_channel_mid()
    om = problems.oracle_model(cfg, box="direct")
    p = wo.standard(cfg, om)
    ref = orc.lcg(wo.Weighted(om, p["w"]), wo.wdata(p["w"], p["y"]), MU, MUR, np.zeros(om.ishape), tol=1e-12, max_iter=9)
    gr = np.array(ref["grad_norm"])
    m = build_model(cfg)
    try:
        assert m.spec_supported()
        x, gn, n = m.cg(p["y"], mu=MU, mu_reg=MUR, max_iter=9, tol=1e-12, weights=p["w"])
    finally:
        m.close()
    ge = _max_rel(gn[:10], gr[:10])
    note("weights_cg_spectral", err_x=rel(x, ref["x"]), err_gradnorm_first10=ge)
    assert n == 9 and len(gn) == 10 and ge < 2e-4


def test_mmmg_matches_weighted_oracle(std):
    """Bounds of test_gpu_driver.py::test_mmmg_matches_oracle_and_cg (x0 = 0.5, 8 iterations)."""
    cfg, om, m, p = std
    x0 = np.ones(m.ishape) * 0.5
    ref = orc.mmmg(p["om_w"], p["y_w"], MU, MUR, x0, max_iter=8)
    x, gn, n = m.mmmg(p["y"], mu=MU, mu_reg=MUR, x0=x0, max_iter=8, weights=p["w"])
    e, ge = rel(x, ref["x"]), _max_rel(gn, ref["grad_norm"])
    note("weights_mmmg", err_x=e, err_gradnorm=ge)
    assert n == 8 and gn.shape == (9,) and e < 1e-4 and ge < 2e-4


def test_mmmg_huber_matches_weighted_oracle(std):
    """Bounds and regime "rough" (textured start, delta 0.1) of test_gpu_huber.py::test_mmmg_huber_matches_oracle."""
    cfg, om, m, p = std
    delta = 0.1
    x0 = cfg["maps"] + 0.1 * np.random.default_rng(3).standard_normal(m.ishape)
    ref = ho.mmmg(p["om_w"], p["y_w"], MU, MUR, delta, x0, max_iter=8)
    x, gn, n = m.mmmg(p["y"], mu=MU, mu_reg=MUR, x0=x0, max_iter=8, delta=delta, weights=p["w"])
    e, ge = rel(x, ref["x"]), _max_rel(gn, ref["grad_norm"])
    note("weights_mmmg_huber", err_x=e, err_gradnorm=ge)
    assert n == 8 and gn.shape == (9,) and e < 1e-4 and ge < 2e-4
    assert abs(m.huber_prior_value - ho.prior_value(x, delta)) < 1e-5 * m.huber_prior_value


def test_mmmg_vox_matches_weighted_oracle():
    """Bounds and regime "both" of test_gpu_vox.py::test_mmmg_vox_matches_oracle, on vox_oracle.small_cfg() (32 x 48 x 48)."""
    cfg, om, cube, y_clean = vo.small_cfg()
    w, y, _ = wo.recipe(om.forward(cube), y_clean)
    sr, ds, lr, dl, st, nit = vo.REGIMES["both"]
    x0 = vo.start(st, om, cube)
    ref = vo.mmmg(wo.Weighted(om, w), wo.wdata(w, y), MU, sr, ds, lr, dl, x0, max_iter=nit)
    m = build_model(cfg)
    try:
        x, gn, n = m.mmmg_vox(y, mu=MU, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=nit, weights=w)
        xu, _, _ = m.mmmg_vox(y, mu=MU, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=nit)
    finally:
        m.close()
    e, ge = rel(x, ref["x"]), _max_rel(gn, ref["grad_norm"])
    note("weights_mmmg_vox", err_x=e, err_gradnorm=ge, unweighted_vs_weighted=rel(xu, x))
    assert n == nit and e < vo.X_TOL_BOUND and ge < vo.G_TOL_BOUND
    assert rel(xu, x) > 20 * vo.X_TOL_BOUND                                    # the weights are in play


class _PlaneOp:
    """One plane of the 2-D oracle as a [1, N, N] operator (the checker's lcg and priors act on [T, N, N])."""
    def __init__(self, bo, N, n_out):
        self.bo, self.ishape, self.oshape = bo, (1, N, N), (n_out,)

    def forward(self, x):
        return self.bo.forward(x[0]).ravel()

    def adjoint(self, y):
        return self.bo.adjoint(y)[None]


def test_plane_wise_cg_matches_weighted_oracle():
    """MRSBlurred.cg (a channel without spectral blur: the element-wise weight kernel) on the problem and at the bounds of
    test_gpu_variants.py::test_plane_wise_cg_2d_deconvolution, plane by plane."""
    from test_gpu_variants import blurred_case
    L = 5
    N, bo, m = blurred_case(L=L)
    truth = np.random.default_rng(4).random((L, N, N))
    y_true = bo.forward(truth)
    w, y, _ = wo.recipe(y_true, y_true)
    mu, mur, nit = 1.0, 0.05, 10
    try:
        x, gn, n = m.cg(y, mu=mu, mu_reg=mur, max_iter=nit, weights=w)
        assert m.data_weights is None
    finally:
        m.close()
    assert n == nit and gn.shape == (nit + 1, L)
    wav, ax, s_ = np.linspace(7.0, 8.2, L), orc.synthetic_axes(N, problems.STEP_DEG), problems.STEP_DEG
    pts = [(0.0, 0.0), (2 * s_, -3 * s_), (-4 * s_, 1 * s_)]
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    for l in (0, 2, 4):
        sotf_l = orc.ir2fr(orc.gaussian_psf(wav[l:l + 1], problems.STEP), (N, N))[0]
        op = _PlaneOp(orc.BlurredOracle(sotf_l, ax, ax, spec, s_, pts), N, y[l].size)
        ref = orc.lcg(wo.Weighted(op, w[l].ravel()), wo.wdata(w[l].ravel(), y[l].ravel()), mu, mur, np.zeros((1, N, N)), tol=1e-12, max_iter=nit)
        gr = np.array(ref["grad_norm"])
        e, ge = rel(x[l], ref["x"][0]), _max_rel(gn[:5, l], gr[:5])
        note("weights_cg_planes", plane=l, err_x=e, err_gradnorm_first5=ge)
        assert e < 5e-3 and ge < 1e-2 and gn[-1, l] < 1e-2 * gn[0, l], l


# ---- 4. masking is total -----------------------------------------------------------------------------------------------------------
def test_masked_samples_do_not_count_whatever_they_hold(std):
    cfg, om, m, p = std
    y_nan = np.where(p["masked"], np.nan, p["y"])
    xs, gs, _ = m.cg(p["y"], mu=MU, mu_reg=MUR, max_iter=NIT, weights=p["w"])
    xn, gn, _ = m.cg(y_nan, mu=MU, mu_reg=MUR, max_iter=NIT, weights=p["w"])
    assert np.isfinite(xn).all() and np.array_equal(xs, xn) and np.array_equal(gs, gn)
    xc, _, _ = m.cg(p["y_clean"], mu=MU, mu_reg=MUR, max_iter=NIT)
    e = rel(xs, xc)
    note("weights_masking", weighted_vs_clean=e)
    # 1.1e-2 in float64 (tests/test_weights_host.py) plus margin; the unweighted solve of the spiked data lies 4.5e2 away
    assert e < 5e-2


# ---- 5. the criterion ----------------------------------------------------------------------------------------------------------------
def test_weighted_criterion(std):
    from surfh_amd.fusion import QuadCriterion_MRS
    cfg, om, m, p = std
    y_nan = np.where(p["masked"], np.nan, p["y"])
    q = QuadCriterion_MRS(MU, y_nan, m, MUR, weights=p["w"])
    js = []
    for k in (1, 4, 8):
        x = m.cg(y_nan, mu=MU, mu_reg=MUR, max_iter=k, weights=p["w"])[0]
        j, want = q.get_crit_val(x), orc.crit_val(p["om_w"], p["y_w"], x, MU, MUR)
        note("weights_criterion", iterations=k, err=abs(j - want) / want)
        assert abs(j - want) < 1e-5 * want
        js.append(j)
    assert js[0] > js[1] > js[2]
    # run_method installs the criterion's weights for the solve and leaves the plan's state as it found it
    res = q.run_method("lcg", 8, value_init=0)
    assert m.data_weights is None and m._L.surfh_has_data_weights(m._plan) == 0
    assert np.array_equal(res.x.reshape(m.ishape), m.cg(y_nan, mu=MU, mu_reg=MUR, x0=np.zeros(m.ishape), max_iter=8, weights=p["w"])[0])
    other = np.full(m.osize, 0.5)
    m.set_data_weights(other)
    try:
        res2 = q.run_method("lcg", 8, value_init=0)
        assert np.array_equal(m.data_weights, other.astype(np.float32)) and m._L.surfh_has_data_weights(m._plan) == 1
        assert np.array_equal(res2.x, res.x)
    finally:
        m.set_data_weights(None)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refused_weights_leave_the_plan_as_it_was(std):
    import torch
    from surfh_amd import _lib
    from surfh_amd.mixing import Model_WCT
    cfg, om, m, p = std
    L = m._L
    d = cfg["maps"]
    m.set_data_weights(p["w"])
    try:
        q_before = _normal(m, d)
        for bad_value in (-1.0, float("nan"), float("inf")):
            bad = np.ones(m.osize, dtype=np.float32)
            bad[m.osize // 3] = bad_value
            assert L.surfh_set_data_weights(m._plan, _lib.fptr(bad)) != 0
            assert L.surfh_last_error().decode()
            bad_t = torch.as_tensor(bad, device="cuda:0")
            torch.cuda.synchronize()
            assert L.surfh_set_data_weights_dev(m._plan, C.c_void_p(bad_t.data_ptr())) != 0
            assert L.surfh_last_error().decode()
            assert L.surfh_has_data_weights(m._plan) == 1
        assert np.array_equal(_normal(m, d), q_before)                         # the previous weights survive
        # the device form installs what the host form installs
        w_t = torch.as_tensor(p["w"].astype(np.float32), device="cuda:0")
        torch.cuda.synchronize()
        assert L.surfh_set_data_weights_dev(m._plan, C.c_void_p(w_t.data_ptr())) == 0
        assert np.array_equal(_normal(m, d), q_before)
        assert L.surfh_set_data_weights_dev(m._plan, None) == 0 and L.surfh_has_data_weights(m._plan) == 0
    finally:
        m.set_data_weights(None)
    # a plan without detector channels
    Lc, N = 16, 48
    wct = Model_WCT(orc.gaussian_psf(np.linspace(7.5, 7.7, Lc), problems.STEP), orc.synthetic_templates(Lc), (N, N), np.ones(Lc))
    try:
        one = np.ones(4, dtype=np.float32)
        assert L.surfh_set_data_weights(wct._plan, _lib.fptr(one)) != 0 and "channel" in L.surfh_last_error().decode()
        assert L.surfh_set_data_weights_dev(wct._plan, None) != 0
        assert L.surfh_has_data_weights(wct._plan) == 0
    finally:
        wct.close()
