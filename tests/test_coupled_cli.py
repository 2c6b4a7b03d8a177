"""The fusion driver's --coupling: option parsing, refusals and the directory name (no GPU needed), and a small run (needs an
MI355X)."""
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


def test_directory_names():
    drv = _driver()
    base = ("mmmg", 1, 4, 8, 5e3, False)
    plain = drv.result_dir_name(*base, 0.1)
    assert plain == "mmmg_MC_1_MO_4_Temp_4_nit_8_mu_5.00e+03_SD_False_huber_1.00e-01/"          # today's directory
    assert drv.result_dir_name(*base, 0.1, coupling="none") == plain
    assert drv.result_dir_name(*base, 0.1, coupling="vector") == plain[:-1] + "_cpl_vector/"
    assert drv.result_dir_name(*base, 0.1, potential="hyperbolic", coupling="isotropic").endswith("_hyperbolic_1.00e-01_cpl_isotropic/")
    assert drv.result_dir_name(*base, 0.1, weighted=True, data_delta=3.0, coupling="vector").endswith(
        "_huber_1.00e-01_cpl_vector_wgt_rob_3/")


def test_coupling_is_refused_where_it_means_nothing():
    """raised before any model is built: this runs without a GPU"""
    drv = _driver()
    run = CliRunner()
    for args, word in ((["--coupling", "tv"], "tv"),
                       (["--coupling", "vector"], "--method mmmg"),                                 # lcg is the default
                       (["-m", "lcg", "--coupling", "isotropic"], "--method mmmg"),
                       (["-m", "mmmg", "--coupling", "vector"], "--delta"),
                       (["-m", "mmmg", "--data_delta", "3", "--coupling", "vector"], "--delta"),
                       (["-m", "mmmg", "--voxel", "--delta", "0.1", "--coupling", "isotropic"], "--voxel")):
        r = run.invoke(drv.main, ["--synthetic", "small"] + args)
        assert r.exit_code == 2 and word in r.output, (args, r.output)


@pytest.mark.gpu
def test_driver_writes_under_the_suffixed_directory(tmp_path):
    drv = _driver()
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "7", "--synthetic", "config2",
                                      "--method", "mmmg", "--delta", "0.3", "--coupling", "vector"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 4, 7, 5e3, False, 0.3, coupling="vector")
    assert d.name.endswith("_huber_3.00e-01_cpl_vector") and d.is_dir()
    assert not (tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 4, 7, 5e3, False, 0.3)).exists()
    x, crit = np.load(d / "res_x.npy"), np.load(d / "criterion.npy")
    assert x.shape == (4 * 251 * 251,) and np.isfinite(x).all() and np.linalg.norm(x) > 0
    assert crit.shape == (2,) and np.all(np.isfinite(crit)) and crit[1] < crit[0]          # the criterion after iterations 1 and 6
