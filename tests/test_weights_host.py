"""Data weights without a GPU: the oracle wrapper of tests/weights_oracle.py, the preconditions of the standard weighted problem
that tests/test_gpu_weights.py relies on, and the host-side pieces (weights_from_data, the argument check, the driver's flags)."""
import importlib.util
import os

import numpy as np
import pytest

import problems
import weights_oracle as wo
from helpers import rel
from oracle import surfh_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def std():
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    return cfg, om, wo.standard(cfg, om)


def test_wrapper_is_a_linear_operator_pair(std):
    cfg, om, p = std
    assert orc.dottest_gap(wo.Weighted(om, p["w"]), np.random.default_rng(0)) < 1e-12


def test_unit_weights_reproduce_lcg_bit_for_bit(std):
    cfg, om, p = std
    one = np.ones(om.osize)
    a = orc.lcg(om, p["y_clean"], wo.MU, wo.MUR, np.zeros(om.ishape), max_iter=4)
    b = orc.lcg(wo.Weighted(om, one), wo.wdata(one, p["y_clean"]), wo.MU, wo.MUR, np.zeros(om.ishape), max_iter=4)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"]


def test_preconditions_of_the_standard_problem(std):
    cfg, om, p = std
    share = float(np.mean(p["masked"]))
    z = np.zeros(om.ishape)
    clean = orc.lcg(om, p["y_clean"], wo.MU, wo.MUR, z, max_iter=wo.NIT)["x"]
    weighted = orc.lcg(wo.Weighted(om, p["w"]), wo.wdata(p["w"], p["y"]), wo.MU, wo.MUR, z, max_iter=wo.NIT)["x"]
    spiked = orc.lcg(om, p["y"], wo.MU, wo.MUR, z, max_iter=wo.NIT)["x"]
    print(f"masked share {share:.3f}, weighted vs clean {rel(weighted, clean):.2e}, unweighted spiked vs clean {rel(spiked, clean):.2e}")
    assert 0.08 <= share <= 0.16 and np.all(p["w"][p["masked"]] == 0) and np.all(p["w"][~p["masked"]] >= 0.5)
    assert rel(weighted, clean) < 5e-2 and rel(spiked, clean) > 10
    # masking is total in the oracle too: NaN at the masked samples changes nothing
    y_nan = np.where(p["masked"], np.nan, p["y"])
    assert np.array_equal(wo.wdata(p["w"], y_nan), wo.wdata(p["w"], p["y"]))


def test_weights_from_data():
    from surfh_amd.fusion import weights_from_data
    y = np.array([[1.0, np.nan, -2.0], [np.inf, 3.0, -np.inf]])
    yc, w = weights_from_data(y)
    assert np.array_equal(yc, [[1, 0, -2], [0, 3, 0]]) and np.array_equal(w, [[1, 0, 1], [0, 1, 0]])
    sigma = np.array([[2.0, 1.0, 0.0], [1.0, -1.0, 1.0]])
    yc2, w2 = weights_from_data(y, sigma)
    assert np.array_equal(yc2, yc) and np.array_equal(w2, [[0.25, 0, 0], [0, 0, 0]])
    _, w3 = weights_from_data(np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.5, np.nan, np.inf, 1e-200]))
    assert np.array_equal(w3, [4.0, 0.0, 0.0, 0.0])                       # 1 / sigma^2 overflows: weight 0, never inf
    _, w4 = weights_from_data(np.array([1.0, np.nan]), 0.5)
    assert np.array_equal(w4, [4.0, 0.0])


def test_bad_weights_raise_value_error():
    from surfh_amd.weights import check_data_weights, weighted_sq_residual
    w = check_data_weights(np.ones((2, 3)), 6)
    assert w.dtype == np.float32 and w.shape == (6,)
    for bad in (np.ones(5), np.array([1, 1, -1e-3, 1, 1, 1]), np.array([1, np.nan, 1, 1, 1, 1]), np.array([1, np.inf, 1, 1, 1, 1]),
                np.array([1, 1e39, 1, 1, 1, 1])):                        # 1e39 is infinite in float32
        with pytest.raises(ValueError):
            check_data_weights(bad, 6)
    # the criterion's data term ignores the data of weight 0
    assert weighted_sq_residual([1.0, np.nan, 5.0], [0.0, 1.0, 3.0], [2.0, 0.0, 0.5]) == 2.0 * 1.0 + 0.5 * 4.0


def test_criteria_check_weights_before_any_library_call():
    from surfh_amd.fusion import QuadCriterion_MRS
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D

    class Stub:
        ishape, oshape, osize = (2, 4, 4), (6,), 6
    for cls in (QuadCriterion_MRS, QuadCriterion_MRS_2D):
        assert cls(1.0, np.zeros(6), Stub(), 1.0, weights=np.ones(6)).weights.dtype == np.float32
        for bad in (np.ones(7), -np.ones(6), np.full(6, np.nan)):
            with pytest.raises(ValueError):
                cls(1.0, np.zeros(6), Stub(), 1.0, weights=bad)


def _driver():
    spec = importlib.util.spec_from_file_location("main_fusion_w", os.path.join(ROOT, "scripts", "main_fusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flags(tmp_path):
    drv = _driver()
    names = {o for p in drv.main.params for o in p.opts}
    assert {"--weights", "--mask_nan"} <= names
    # without either flag nothing changes
    assert drv.result_dir_name("lcg", 12, 4, 50, 5e3, False) == "lcg_MC_12_MO_4_Temp_4_nit_50_mu_5.00e+03_SD_False/"
    assert drv.result_dir_name("mmmg", 1, 0, 8, 40.0, False, 0.005, voxel=True) == "mmmg_MC_1_MO_4_Temp_0_nit_8_mu_4.00e+01_SD_False_huber_5.00e-03_vox/"
    assert drv.result_dir_name("lcg", 12, 4, 50, 5e3, False, weighted=True) == "lcg_MC_12_MO_4_Temp_4_nit_50_mu_5.00e+03_SD_False_wgt/"
    y = np.array([1.0, np.nan, 3.0, np.inf])
    out, w = drv.data_weights(y)
    assert out is y and w is None
    out, w = drv.data_weights(y, mask_nan=True)
    assert np.array_equal(out, [1, 0, 3, 0]) and np.array_equal(w, [1, 0, 1, 0])
    np.save(tmp_path / "w.npy", np.array([0.5, 2.0, 0.0, 1.0]))
    out, w = drv.data_weights(y, str(tmp_path / "w.npy"), True)
    assert np.array_equal(out, [1, 0, 3, 0]) and np.array_equal(w, [0.5, 0, 0, 0])
    out, w = drv.data_weights(y, str(tmp_path / "w.npy"))
    assert out is y and np.array_equal(w, [0.5, 2.0, 0.0, 1.0])
    np.save(tmp_path / "bad.npy", np.array([0.5, -2.0, 0.0, 1.0]))
    with pytest.raises(ValueError):
        drv.data_weights(y, str(tmp_path / "bad.npy"))
    with pytest.raises(ValueError):
        drv.data_weights(y[:3], str(tmp_path / "w.npy"))
