"""3MG with edge-preserving Huber priors on the device (surfh_mmmg_huber, surfh_huber_prior_dev) against the float64
restatement of tests/huber_oracle.py, the quadratic solver it reduces to, the criterion class, lmm_reconstruction and the
fusion driver (needs an MI355X)."""
import importlib.util
import os
import time

import numpy as np
import pytest
from click.testing import CliRunner

import huber_oracle as ho
import problems
from helpers import build_model, rel
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU, MUR, NIT = 1.0, 5e3, 8


# Regimes in which the Huber branch is active along the path: a large share of |D_k x| beyond delta (weights below 1, phi'
# clipped) and iterates far from the quadratic solver's.  With delta ~ median |D x| of the true maps and mu_reg = 5e3 from a
# flat start the iterates stay so smooth that no difference exceeds delta -- that only re-checks quadratic 3MG.
#   rough: a start with the true maps' texture (truth + noise), mu_reg 5e3, delta 0.1
#   half / zero: the flat starts of the quadratic test, mu_reg 5e6 (prior-dominated), delta at the scale of those iterates'
#   differences; from x0 = 0 only 6 iterations are compared (numpy's pinv cut, see test_gpu_driver.py)
REGIMES = {"rough": (5e3, 0.1, NIT), "half": (5e6, 1e-3, NIT), "zero": (5e6, 1e-2, 6)}


@pytest.fixture(scope="module")
def setup():
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    y = om.forward(cfg["maps"])
    y = y + np.random.default_rng(1).standard_normal(y.shape) * 1e-2 * np.sqrt(np.mean(y ** 2))
    starts = {"rough": cfg["maps"] + 0.1 * np.random.default_rng(3).standard_normal(m.ishape),
              "half": np.full(m.ishape, 0.5), "zero": np.zeros(m.ishape)}
    yield cfg, om, m, y, starts
    m.close()


def _share_beyond(x, delta):
    u = np.abs(np.concatenate([orc.diff_r(x).ravel(), orc.diff_c(x).ravel()]))
    return float(np.mean(u > delta))


def _rect_problem(na, nb, T, Lc=64):
    rng = np.random.default_rng(31)
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(0.8 / 3600, 0.9 / 3600, (0.0, 0.0), 8.2, 0.196, 4, 3050.0, np.linspace(7.53, 7.67, 40), "S1")
    return dict(N=na, Lc=Lc, alpha_axis=orc.synthetic_axes(na, problems.STEP_DEG), beta_axis=orc.synthetic_axes(nb, problems.STEP_DEG),
                wavel=wav, specs=[spec], templates=rng.random((T, Lc)) + 0.5,
                sotf=orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (na, nb)),
                pointings=[orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)], maps=rng.random((T, na, nb)),
                step_deg=problems.STEP_DEG)


def _check_kernels(m, delta, seed):
    import torch
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(m.ishape) * 2 * delta).astype(np.float32)          # differences on both sides of delta
    g0 = rng.standard_normal(m.ishape).astype(np.float32)
    p0 = rng.standard_normal(m.ishape).astype(np.float32)
    p1 = rng.standard_normal(m.ishape).astype(np.float32)
    x64, a, b = x.astype(np.float64), p0.astype(np.float64), p1.astype(np.float64)
    assert 0.1 < _share_beyond(x64, delta) < 0.9
    want = g0 + 0.7 * ho.prior_grad(x64, delta)
    ws = [ho.weight(d(x64), delta) for d, _ in ho.DIFFS]
    want_c = np.array([sum(np.sum(w * d(u) * d(v)) for w, (d, _) in zip(ws, ho.DIFFS)) for u, v in ((a, a), (a, b), (b, b))])
    vals, outs, curv = [], [], []
    x_t, p0_t, p1_t = (torch.as_tensor(v, device="cuda:0") for v in (x, p0, p1))
    for _ in range(2):
        g_t = torch.as_tensor(g0, device="cuda:0")
        torch.cuda.synchronize()
        vals.append(m.huber_prior_dev(x_t, g_t, 0.7, delta))
        curv.append(m.huber_curv_dev(x_t, p0_t, p1_t, delta))
        torch.cuda.synchronize()
        outs.append(g_t.cpu().numpy())
    ref = ho.prior_value(x64, delta)
    ec = float(np.max(np.abs(curv[0] - want_c)) / np.max(np.abs(want_c)))
    print(m.ishape, f"prior grad {rel(outs[0], want):.2e}, value {abs(vals[0] - ref) / ref:.2e}, curvature {ec:.2e}")
    assert rel(outs[0], want) < 1e-6 and abs(vals[0] - ref) < 1e-6 * ref and ec < 1e-6
    # deterministic reductions
    assert vals[0] == vals[1] and np.array_equal(outs[0], outs[1]) and np.array_equal(curv[0], curv[1])
    # the weights matter: the unweighted sums are far off
    plain = np.array([sum(np.sum(d(u) * d(v)) for d, _ in ho.DIFFS) for u, v in ((a, a), (a, b), (b, b))])
    assert abs(plain[0] - want_c[0]) > 0.1 * want_c[0]
    # the border pixels, where the circular wrap acts, entry by entry
    T, Na, Nb = m.ishape
    for idx in [(0, 0, 0), (T - 1, Na - 1, 0), (0, 0, Nb - 1), (T - 1, Na - 1, Nb - 1)]:
        assert abs(outs[0][idx] - want[idx]) < 1e-5 * (1 + abs(want[idx]))


def test_huber_kernels_match_numpy(setup):
    cfg, om, m, y, starts = setup
    _check_kernels(m, 0.3, 0)                                                 # 64 x 64
    m2 = build_model(_rect_problem(72, 77, 3))                                # Na != Nb, odd Nb, not a multiple of 64
    try:
        assert m2.ishape == (3, 72, 77)
        _check_kernels(m2, 0.3, 1)
        import torch
        x_t = torch.zeros(m2.ishape, device="cuda:0")
        for bad in (0.0, -1.0, float("nan"), 1e-40):                          # 1e-40 does not survive the fp32 kernels
            with pytest.raises(RuntimeError):
                m2.huber_prior_dev(x_t, x_t.clone(), 1.0, bad)
            with pytest.raises(RuntimeError):
                m2.huber_curv_dev(x_t, x_t, x_t, bad)
        with pytest.raises(RuntimeError):
            m2.huber_prior_dev(x_t, x_t.clone(), float("nan"), 1.0)
        assert m2.huber_prior_dev(x_t, x_t.clone(), 1.0, float("inf")) == 0.0
    finally:
        m2.close()


@pytest.mark.parametrize("regime", list(REGIMES))
def test_mmmg_huber_matches_oracle(setup, regime):
    cfg, om, m, y, starts = setup
    mur, delta, nit = REGIMES[regime]
    x0 = starts[regime]
    ref = ho.mmmg(om, y, MU, mur, delta, x0, max_iter=nit)
    quad = orc.mmmg(om, y, MU, mur, x0, max_iter=nit)
    share, away = _share_beyond(ref["x"], delta), rel(ref["x"], quad["x"])
    x, gn, n = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=nit, delta=delta)
    prior_value = m.huber_prior_value
    xq, _, _ = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=nit)
    assert m.huber_prior_value is None                                        # a quadratic run leaves no stale value
    gr = np.array(ref["grad_norm"])
    ex, eg = rel(x, ref["x"]), float(np.max(np.abs(gn - gr) / gr))
    print(f"{regime}: |Dx| > delta for {share:.0%}, oracle Huber vs quadratic {away:.1e}, device vs oracle: x {ex:.2e}, "
          f"grad_norm {eg:.2e}; device Huber vs quadratic {rel(x, xq):.1e}")
    assert share > 0.1 and away > 20 * 1e-4 and rel(x, xq) > 20 * 1e-4       # the Huber branch is in play
    assert n == nit and gn.shape == (nit + 1,) and ex < 1e-4 and eg < 2e-4
    pv = ho.prior_value(x, delta)
    assert abs(prior_value - pv) < 1e-5 * pv
    if regime == "rough":       # the refresh period changes rounding only
        xf, _, _ = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=nit, delta=delta, refresh=1)
        assert rel(xf, x) < 1e-4


def test_infinite_delta_is_the_quadratic_solver(setup):
    cfg, om, m, y, starts = setup
    x0 = np.full(m.ishape, 0.5)
    xq, gq, _ = m.mmmg(y, mu=MU, mu_reg=MUR, x0=x0, max_iter=NIT)
    assert m.huber_prior_value is None
    for big in (1e30, float("inf")):
        xh, gh, nh = m.mmmg(y, mu=MU, mu_reg=MUR, x0=x0, max_iter=NIT, delta=big)
        assert nh == NIT and rel(xh, xq) < 1e-4 and float(np.max(np.abs(gh - gq) / gq)) < 2e-4
        jq = orc.crit_val(om, y, xh, MU, MUR)
        assert abs(m.huber_prior_value * MUR - (jq - MU * np.sum((y - om.forward(xh)) ** 2) / 2)) < 1e-5 * jq


def test_criterion_descends_and_stops(setup):
    from surfh_amd.fusion import QuadCriterion_MRS
    cfg, om, m, y, starts = setup
    mur, delta, _ = REGIMES["rough"]
    x0 = starts["rough"]
    q = QuadCriterion_MRS(MU, y, m, mur, delta=delta)
    js = []
    x, gn, n = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=40, delta=delta,
                      callback=lambda it, g, xx: js.append(q.get_crit_val(xx)) and False)
    js = np.array([q.get_crit_val(x0)] + js)
    assert n == 40 and len(js) == 41 and _share_beyond(x, delta) > 0.1
    assert np.all(np.diff(js) <= 1e-6 * js[:-1]) and js[-1] < js[0]           # MM: non-increasing up to fp32 noise
    assert abs(js[4] - ho.crit(om, y, ho.mmmg(om, y, MU, mur, delta, x0, max_iter=4)["x"], MU, mur, delta)) < 1e-5 * js[4]
    # early stop through the callback, tolerance stop
    seen = []
    x3, g3, n3 = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=NIT, delta=delta,
                        callback=lambda it, g, xx: seen.append(it) or it == 3)
    x8, g8, _ = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=NIT, delta=delta)
    assert n3 == 3 and seen == [1, 2, 3] and np.array_equal(g3, g8[:4])
    xt, gt, nt = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=NIT, delta=delta, tol=g8[4] * 1.0001 / x8.size)
    assert nt == 4 and np.array_equal(gt, g8[:5])


def test_criterion_class_and_lmm_reconstruction(setup, tmp_path):
    from surfh_amd.algorithms import lmm_reconstruction
    from surfh_amd.fusion import QuadCriterion_MRS, load_checkpoint
    cfg, om, m, y, starts = setup
    mur, delta, _ = REGIMES["rough"]
    x0 = starts["rough"]
    x, gn, _ = m.mmmg(y, mu=MU, mu_reg=mur, x0=x0, max_iter=NIT, delta=delta)
    q = QuadCriterion_MRS(MU, y, m, mur, delta=delta)
    res = q.run_method("mmmg", NIT, value_init=x0, checkpoint=(tmp_path / "ck.npz", 4))
    assert res.nit == NIT and rel(res.x.reshape(m.ishape), x) == 0.0 and np.array_equal(res.grad_norm, gn)
    assert load_checkpoint(tmp_path / "ck.npz")[1] == NIT
    jr = ho.crit(om, y, x, MU, mur, delta)
    assert abs(q.get_crit_val(res.x) - jr) < 1e-5 * jr
    # the Huber criterion, not the quadratic one, is what get_crit_val reports
    jq = QuadCriterion_MRS(MU, y, m, mur).get_crit_val(res.x)
    assert abs(jq - jr) > 1e-2 * jr
    q2 = QuadCriterion_MRS(MU, y, m, mur, delta=delta)
    q2.run_method("mmmg", 6, calc_crit=True, perf_crit=1, value_init=x0)
    assert len(q2.L_crit_val) == 2 and q2.L_crit_val[1] < q2.L_crit_val[0]
    with pytest.raises(ValueError):
        q.run_method("lcg", NIT)
    # the reference's entry point: same criterion with mu = 1, spat_reg = mu_reg, spat_th = delta
    r = lmm_reconstruction(y, m, spat_reg=mur, spat_th=delta, init=x0, max_iter=NIT)
    assert r.nit == NIT and rel(r.x.reshape(m.ishape), x) == 0.0
    r0 = lmm_reconstruction(y, m, spat_reg=mur, spat_th=delta, max_iter=3)
    x1, _, _ = m.mmmg(y, mu=1.0, mu_reg=mur, x0=m.adjoint(y), max_iter=3, delta=delta)
    assert rel(r0.x.reshape(m.ishape), x1) == 0.0


def test_config3_size_against_quadratic():
    """A few iterations at the benchmark's size (N = 251, bands 1C, 2A, 2B, 2C): delta = inf against the quadratic solver, and
    from a textured start a delta with the Huber branch in play; prints the per-iteration time of each."""
    from surfh_amd import synth
    from surfh_amd.fusion import QuadCriterion_MRS
    from surfh_amd.models import spectroSigRLSCT
    prob = synth.config3()
    m = spectroSigRLSCT(prob["sotf"], prob["templates"], prob["alpha_axis"], prob["beta_axis"], prob["wavel"], prob["ifus"],
                        prob["step_deg"], prob["pointings"])
    try:
        y = m.forward(prob["maps"])
        x0 = np.full(m.ishape, 0.5)
        xr = prob["maps"] + 0.1 * np.random.default_rng(3).standard_normal(m.ishape)
        m.mmmg(y, mu=1.0, mu_reg=5e3, x0=x0, max_iter=1)                       # warm-up
        m.mmmg(y, mu=1.0, mu_reg=5e3, x0=x0, max_iter=1, delta=0.1)
        k = 6
        t = {}
        # at this size the data term outweighs mu_reg = 5e3 so much that 6 iterations from the textured start hardly feel the
        # prior (Huber and quadratic agree to 1e-6): that pair runs with mu_reg = 5e7
        for name, start, mur, kw in (("quadratic", x0, 5e3, {}), ("huber_inf", x0, 5e3, {"delta": float("inf")}),
                                     ("quadratic_textured", xr, 5e7, {}), ("huber_0.1_textured", xr, 5e7, {"delta": 0.1})):
            t0 = time.perf_counter()
            t[name] = m.mmmg(y, mu=1.0, mu_reg=mur, x0=start, max_iter=k, **kw)
            t1 = time.perf_counter()
            t0b = time.perf_counter()
            m.mmmg(y, mu=1.0, mu_reg=mur, x0=start, max_iter=0, **kw)
            t1b = time.perf_counter()
            print(f"config3 mmmg {name}: {((t1 - t0) - (t1b - t0b)) / k * 1e3:.2f} ms per iteration")
        (xq, gq, _), (xi, gi, _) = t["quadratic"], t["huber_inf"]
        assert rel(xi, xq) < 1e-4 and float(np.max(np.abs(gi - gq) / gq)) < 2e-4
        xh, xqt = t["huber_0.1_textured"][0], t["quadratic_textured"][0]
        # 6.3e-4 measured: a few iterations from a start the data already fit move little, but the two solvers part well beyond
        # the 1e-4 at which they agree when they minimise the same criterion (huber_inf above)
        assert _share_beyond(xh, 0.1) > 0.1 and rel(xh, xqt) > 3e-4
        q = QuadCriterion_MRS(1.0, y, m, 5e7, delta=0.1)
        assert q.get_crit_val(xh) < q.get_crit_val(xr)
    finally:
        m.close()


def test_driver_writes_huber_results(tmp_path):
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "3", "--synthetic", "config2",
                                      "--method", "mmmg", "--delta", "0.1"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False, 0.1)
    assert d.name.endswith("_huber_1.00e-01")
    x, cube, crit = np.load(d / "res_x.npy"), np.load(d / "res_cube.npy"), np.load(d / "criterion.npy")
    assert x.shape == (4 * 251 * 251,) and cube.shape == (1024, 251, 251) and crit.shape == (1,) and np.isfinite(x).all()
