"""The float64 restatement of the robust data term (tests/robust_oracle.py) checked on its own, without a GPU: gradient, majorant,
descent, the reductions to the existing oracles, and the preconditions of the device comparisons of tests/test_gpu_robust.py."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

import huber_oracle as ho
import robust_oracle as ro
import vox_oracle as vo
import weights_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def small():
    """huber_oracle's small problem with the standard spikes, 5 % of the samples masked (NaN in the data there), at a textured
    point where both branches of the data potential and of the prior potential are taken."""
    om, maps, _ = ho.small_problem()
    d = ro.spiked(om.forward(maps))
    rng = np.random.default_rng(11)
    w = d["w"] * np.exp(rng.uniform(np.log(0.5), np.log(2.0), d["w"].shape))
    masked = rng.random(w.shape) < 0.05
    w[masked] = 0.0
    y = d["y"].copy()
    y[masked] = np.nan
    x = maps + 0.02 * rng.standard_normal(om.ishape)
    return dict(om=om, maps=maps, y=y, w=w, masked=masked, x=x, mur=0.5 / d["sigma"] ** 2, delta=0.1, sigma=d["sigma"])


def test_both_branches_are_taken(small):
    s = small
    t = ro.residual(s["om"], s["y"], s["x"], s["w"])
    assert np.all(np.isfinite(t)) and np.all(t.ravel()[s["masked"]] == 0.0)
    assert 0.01 < np.mean(np.abs(t) > ro.DATA_DELTA) < 0.9
    om = ro.omega(s["om"], s["y"], s["x"], ro.DATA_DELTA, s["w"])
    assert np.all(om[s["masked"]] == 0.0) and np.all(om[~s["masked"]] > 0.0) and om.max() == 1.0 and om[~s["masked"]].min() < 0.5


def test_gradient_matches_finite_differences(small):
    s = small
    args = (1.3, ro.DATA_DELTA, s["mur"], s["delta"], s["w"])
    g = ro.gradient(s["om"], s["y"], s["x"], *args)
    rng = np.random.default_rng(12)
    for _ in range(3):
        v = rng.standard_normal(s["om"].ishape)
        h = 1e-6
        fd = (ro.crit(s["om"], s["y"], s["x"] + h * v, *args) - ro.crit(s["om"], s["y"], s["x"] - h * v, *args)) / (2 * h)
        # central differences of a C^1 criterion with piecewise constant curvature: O(h) where a residual crosses the threshold
        assert abs(fd - np.sum(g * v)) < 1e-5 * abs(np.sum(g * v))


def test_majorant_lies_above_the_criterion(small):
    s = small
    args = (1.3, ro.DATA_DELTA, s["mur"], s["delta"], s["w"])
    j0, g = ro.crit(s["om"], s["y"], s["x"], *args), ro.gradient(s["om"], s["y"], s["x"], *args)
    rng = np.random.default_rng(13)
    for scale in (1e-3, 1e-2, 1e-1, 1.0):
        v = scale * rng.standard_normal(s["om"].ishape)
        maj = j0 + np.sum(g * v) + ro.majorant_quad(s["om"], s["y"], s["x"], v, *args) / 2
        j = ro.crit(s["om"], s["y"], s["x"] + v, *args)
        assert j <= maj * (1 + 1e-12), (scale, j, maj)
    # tangent: the gap closes quadratically
    v = 1e-5 * rng.standard_normal(s["om"].ishape)
    maj = j0 + np.sum(g * v) + ro.majorant_quad(s["om"], s["y"], s["x"], v, *args) / 2
    assert abs(maj - ro.crit(s["om"], s["y"], s["x"] + v, *args)) < 1e-9 * j0


def test_descent_is_monotone(small):
    s = small
    r = ro.mmmg(s["om"], s["y"], 1.0, ro.DATA_DELTA, s["mur"], s["delta"], np.full(s["om"].ishape, 0.5), w=s["w"], max_iter=25)
    j = np.array(r["crit"])
    assert r["nit"] == 25 and np.all(np.diff(j) < 0) and j[-1] < 0.2 * j[0] and r["grad_norm"][-1] < 0.05 * r["grad_norm"][0]


def test_infinite_threshold_is_the_existing_oracles_bit_for_bit(small):
    s = small
    om, x0 = s["om"], np.full(s["om"].ishape, 0.5)
    y = np.where(s["masked"], 0.0, s["y"])                                        # finite data for the unweighted route
    for delta in (s["delta"], INF):
        a = ro.mmmg(om, y, 1.3, INF, 7.0, delta, x0, max_iter=6)                   # w = 1
        b = ho.mmmg(om, y, 1.3, 7.0, delta, x0, max_iter=6)
        assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"]
        assert np.allclose(a["crit"], b["crit"], rtol=1e-12, atol=0)
        a = ro.mmmg(om, s["y"], 1.3, INF, s["mur"], delta, x0, w=s["w"], max_iter=6)     # the weights_oracle route, NaN masked
        b = ho.mmmg(wo.Weighted(om, s["w"]), wo.wdata(s["w"], s["y"]), 1.3, s["mur"], delta, x0, max_iter=6)
        assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"]
    # and a finite threshold is another criterion
    c = ro.mmmg(om, s["y"], 1.3, ro.DATA_DELTA, s["mur"], INF, x0, w=s["w"], max_iter=6)
    assert np.linalg.norm(c["x"] - a["x"]) > 1e-3 * np.linalg.norm(a["x"])


def test_voxel_variant_reduces_to_vox_oracle():
    c = ro.vox_case()
    sr, sd, lr, ld, _ = ro.VOX_REGIME
    y = c["y"]
    a = ro.mmmg_vox(c["om"], y, 1.0, INF, sr, sd, lr, ld, c["x0"], max_iter=3)
    b = vo.mmmg(c["om"], y, 1.0, sr, sd, lr, ld, c["x0"], max_iter=3)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"]
    g = ro.gradient_vox(c["om"], y, c["x0"], 1.0, ro.DATA_DELTA, sr, sd, lr, ld, c["w"])
    v = np.random.default_rng(14).standard_normal(c["om"].ishape)
    h = 1e-6
    args = (1.0, ro.DATA_DELTA, sr, sd, lr, ld, c["w"])
    fd = (ro.crit_vox(c["om"], y, c["x0"] + h * v, *args) - ro.crit_vox(c["om"], y, c["x0"] - h * v, *args)) / (2 * h)
    assert abs(fd - np.sum(g * v)) < 1e-5 * abs(np.sum(g * v))


def _check_preconditions(om, case, runs, x_bound):
    share, away, to_clean, quad_to_clean = ro.preconditions(om, case, runs)
    print(f"|t| > delta for {share:.1%}; robust vs quadratic {away:.1e}; vs the clean solve: robust {to_clean:.1e}, "
          f"quadratic {quad_to_clean:.1e}")
    assert 0.01 < share < 0.20                                     # the robust branch is in play, and only on a minority
    assert away > 20 * x_bound                                      # a device that ran the quadratic data term would be caught
    assert 3 * to_clean <= quad_to_clean                            # and the term does its job
    j = np.array(runs["rob"]["crit"])
    assert np.all(np.diff(j) < 0)
    return share, away, to_clean, quad_to_clean


@pytest.mark.parametrize("regime", list(ro.C1_REGIMES))
def test_preconditions_of_the_config1_comparison(regime):
    c = ro.config1_case()
    assert c["om"].ishape == (4, 64, 64) and c["y"].size == 3840 and c["spikes"].size == 3840 // 50
    share, away, to_clean, quad_to_clean = _check_preconditions(c["om"], c, ro.config1_runs(regime), 1e-4)
    if regime == "quadratic":      # the figures the issue records: 2.4 %, 1.0e-2, 1.6e-3 against 1.1e-2
        assert abs(share - 0.024) < 0.002 and 0.8e-2 < away < 1.2e-2 and 1.0e-3 < to_clean < 2.0e-3 and 0.9e-2 < quad_to_clean < 1.3e-2
    else:                          # the Huber prior is in play as well
        x, delta = ro.config1_runs(regime)["rob"]["x"], ro.C1_REGIMES[regime][0]
        u = np.abs(np.concatenate([ro.orc.diff_r(x).ravel(), ro.orc.diff_c(x).ravel()]))
        assert 0.1 < np.mean(u > delta) < 0.9


def test_preconditions_of_the_voxel_comparison():
    c = ro.vox_case()
    assert c["om"].ishape == (32, 48, 48)
    _check_preconditions(c["om"], c, ro.vox_runs(), ro.X_TOL_BOUND)
    sr, sd, lr, ld, _ = ro.VOX_REGIME
    ss, sl = vo.shares(ro.vox_runs()["rob"]["x"], sd, ld)
    assert 0.1 < ss < 0.9 and 0.1 < sl < 0.9


def _driver():
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_python_layer_refuses_without_touching_a_model():
    from surfh_amd.fusion import QuadCriterion_MRS, robust_data_value

    class Shape:
        ishape, oshape = (4, 8, 8), (10,)
    with pytest.raises(ValueError):
        QuadCriterion_MRS(1.0, np.zeros(10), Shape(), 1.0, data_delta=0.0)
    with pytest.raises(ValueError):
        QuadCriterion_MRS(1.0, np.zeros(10), Shape(), 1.0, data_delta=3.0, gradient="joint")
    with pytest.raises(ValueError):
        QuadCriterion_MRS(1.0, np.zeros(10), Shape(), 1.0, data_delta=3.0).run_method("lcg", 3)
    # the host-side data value is the oracle's, masked NaN left out
    rng = np.random.default_rng(15)
    y, ax, w = rng.standard_normal(50) * 5, rng.standard_normal(50), rng.random(50)
    w[:5], y[:5] = 0.0, np.nan
    t = np.sqrt(w[5:]) * (y[5:] - ax[5:])
    assert abs(robust_data_value(y, ax, w, 1.5) - np.sum(ro.phi(t, 1.5))) < 1e-12 * np.sum(ro.phi(t, 1.5))
    assert robust_data_value(y[5:], ax[5:], None, INF) == float(np.sum((y[5:] - ax[5:]) ** 2 / 2))
    drv = _driver()
    assert drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False, data_delta=3.0).endswith("_rob_3/")
    assert drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False, 0.1, weighted=True, data_delta=2.5).endswith("_huber_1.00e-01_wgt_rob_2.5/")
    assert drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False) == drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False, data_delta=None)
