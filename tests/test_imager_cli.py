"""The fusion driver's --imager / --mu_imager / --imager_decim: the usage errors (no GPU needed) and a small run (needs an MI355X)."""
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


def test_imager_flags_are_validated_before_any_model_is_built():
    drv = _driver()
    run = lambda *a: CliRunner().invoke(drv.main, list(a))  # noqa: E731
    r = run("--synthetic", "small", "--method", "mmmg", "--imager", "3", "--data_delta", "3")
    assert r.exit_code == 2 and "--imager" in r.output and "--data_delta" in r.output, r.output
    r = run("--synthetic", "small", "--method", "mmmg", "--imager", "3", "--voxel")
    assert r.exit_code == 2 and "--imager" in r.output and "--voxel" in r.output, r.output
    for n in ("17", "-1"):
        r = run("--synthetic", "small", "--imager", n)
        assert r.exit_code == 2 and "--imager" in r.output and "1 to 16" in r.output, r.output
    r = run("--imager", "3")
    assert r.exit_code == 2 and "--synthetic" in r.output, r.output
    r = run("--synthetic", "small", "--imager", "3", "--mu_imager", "-1")
    assert r.exit_code == 2 and "--mu_imager" in r.output, r.output
    for d in ("0", "1000"):
        r = run("--synthetic", "small", "-np", "251", "--imager", "3", "--imager_decim", d)
        assert r.exit_code == 2 and "--imager_decim" in r.output, r.output
    for flag in (("--mu_imager", "2"), ("--imager_decim", "4")):
        r = run("--synthetic", "small", *flag)
        assert r.exit_code == 2 and "--imager" in r.output, r.output
    assert drv.result_dir_name("lcg", 1, 4, 2, 5e3, False, imager=9).endswith("_img_9/")
    assert drv.result_dir_name("lcg", 1, 4, 2, 5e3, False) == drv.result_dir_name("lcg", 1, 4, 2, 5e3, False, imager=0)


@pytest.mark.gpu
def test_driver_runs_with_an_imager(tmp_path):
    drv = _driver()
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "2", "--synthetic", "small",
                                      "--imager", "3", "--mu_imager", "2", "--imager_decim", "4"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("lcg", 1, 4, 2, 5e3, False, imager=3)
    x, y_im = np.load(d / "res_x.npy"), np.load(d / "y_imager.npy")
    assert x.shape == (4 * 251 * 251,) and np.isfinite(x).all()
    assert y_im.shape == (3, 62, 62) and np.isfinite(y_im).all()
