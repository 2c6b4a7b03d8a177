"""The fusion driver's --data_delta: the usage error (no GPU needed) and a small run (needs an MI355X)."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver():
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_data_delta_needs_mmmg():
    """raised before any model is built: this runs without a GPU"""
    drv = _driver()
    for method in (["--method", "lcg"], []):                                  # lcg is the default
        r = CliRunner().invoke(drv.main, ["--synthetic", "small", "--data_delta", "3"] + method)
        assert r.exit_code == 2 and "--data_delta" in r.output and "mmmg" in r.output, r.output
    r = CliRunner().invoke(drv.main, ["--synthetic", "small", "--method", "mmmg", "--data_delta", "0"])
    assert r.exit_code == 2 and "--data_delta" in r.output


@pytest.mark.gpu
def test_driver_writes_robust_weights(tmp_path):
    drv = _driver()
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "2", "--synthetic", "small",
                                      "--method", "mmmg", "--data_delta", "3"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 4, 2, 5e3, False, data_delta=3.0)
    assert d.name.endswith("_rob_3")
    x, om = np.load(d / "res_x.npy"), np.load(d / "robust_weights.npy")
    assert x.shape == (4 * 251 * 251,) and np.isfinite(x).all()
    from surfh_amd.models import spectroSigRLSCT
    prob = drv.synthetic_problem("small", 251)
    m = spectroSigRLSCT(prob["sotf"], prob["templates"], prob["alpha_axis"], prob["beta_axis"], prob["wavel"], prob["ifus"],
                        prob["step_deg"], prob["pointings"])
    try:
        assert om.shape == (m.osize,) and om.min() > 0 and om.max() == 1.0
    finally:
        m.close()
