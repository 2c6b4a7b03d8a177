"""The fusion driver's --refine_templates / --mu_spec / --tpl_iter: the usage errors (no GPU needed) and a small run (needs an MI355X)."""
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


def test_refine_usage_errors():
    """raised before any model is built: this runs without a GPU"""
    drv = _driver()
    base = ["--synthetic", "config2"]
    for extra, word in ((["--refine_templates", "2", "-m", "mmmg"], "lcg"), (["--refine_templates", "-1"], "--refine_templates"),
                        (["--mu_spec", "1e2"], "--refine_templates"), (["--tpl_iter", "5"], "--refine_templates"),
                        (["--refine_templates", "2", "--mu_spec", "-1"], "--mu_spec"), (["--refine_templates", "2", "--tpl_iter", "0"], "--tpl_iter"),
                        (["--refine_templates", "2", "--samples", "4"], "--refine_templates"),
                        (["--refine_templates", "2", "--imager", "3"], "--refine_templates")):
        r = CliRunner().invoke(drv.main, base + extra)
        assert r.exit_code == 2 and word in r.output, (extra, r.output)
    assert drv.result_dir_name("lcg", 1, 4, 3, 5e3, False, refine=2).endswith("_tpl_2/")
    assert drv.result_dir_name("lcg", 1, 4, 3, 5e3, False) == drv.result_dir_name("lcg", 1, 4, 3, 5e3, False, refine=0)
    assert drv.result_dir_name("lcg", 1, 4, 3, 5e3, False) == "lcg_MC_1_MO_4_Temp_4_nit_3_mu_5.00e+03_SD_False/"


@pytest.mark.gpu
def test_driver_refines_templates(tmp_path):
    drv = _driver()
    N, T = 251, 4
    common = ["-np", str(N), "-hp", "5e3", "-ni", "3", "--synthetic", "config2"]
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path / "a")] + common + ["--refine_templates", "2", "--mu_spec", "1e2", "--tpl_iter", "3"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    runs = list((tmp_path / "a" / "Results").iterdir())
    assert len(runs) == 1 and runs[0].name.endswith("_tpl_2")
    d = runs[0]
    assert sorted(p.name for p in d.iterdir()) == ["criterion.npy", "res_templates.npy", "res_x.npy", "templates_start.npy"]
    x, S, S0, J = (np.load(d / f) for f in ("res_x.npy", "res_templates.npy", "templates_start.npy", "criterion.npy"))
    Lc = S0.shape[1]
    assert x.shape == (T, N, N) and S.shape == (T, Lc) and S0.shape == (T, Lc) and J.shape == (5,)
    assert all(np.isfinite(a).all() for a in (x, S, S0, J))
    assert np.all(np.diff(J) <= 0) and not np.array_equal(S, S0)
    # without the flag: the directory and the files of the plain run, nothing of the refinement
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path / "b")] + common)
    assert r.exit_code == 0, r.output + repr(r.exception)
    runs = list((tmp_path / "b" / "Results").iterdir())
    assert [p.name for p in runs] == ["lcg_MC_1_MO_4_Temp_4_nit_3_mu_5.00e+03_SD_False"]
    assert sorted(p.name for p in runs[0].iterdir()) == ["criterion.npy", "res_cube.npy", "res_x.npy"]
