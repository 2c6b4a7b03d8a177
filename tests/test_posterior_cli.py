"""The fusion driver's --samples / --seed: the usage errors (no GPU needed) and a small run (needs an MI355X)."""
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


def test_samples_usage_errors():
    """raised before any model is built: this runs without a GPU"""
    drv = _driver()
    base = ["--synthetic", "config2"]
    for extra, word in ((["--samples", "4", "-m", "mmmg"], "lcg"), (["--samples", "1"], "--samples"), (["--samples", "-3"], "--samples"),
                        (["--seed", "5"], "--samples"), (["--samples", "4", "--seed", "-1"], "--seed"),
                        (["--samples", "4", "--imager", "3"], "--imager"), (["--samples", "4", "--voxel", "-m", "mmmg"], "lcg")):
        r = CliRunner().invoke(drv.main, base + extra)
        assert r.exit_code == 2 and word in r.output, (extra, r.output)
    assert drv.result_dir_name("lcg", 1, 4, 3, 5e3, False, samples=4).endswith("_po_4/")
    assert drv.result_dir_name("lcg", 1, 4, 3, 5e3, False) == drv.result_dir_name("lcg", 1, 4, 3, 5e3, False, samples=0)


def test_criterion_sample_refuses_non_gaussian_criteria():
    from surfh_amd.fusion import QuadCriterion_MRS

    class Stub:
        ishape, oshape = (2, 4, 4), (10,)

    y = np.zeros(10)
    for kw in (dict(delta=1.0), dict(data_delta=3.0), dict(gradient="joint")):
        with pytest.raises(ValueError):
            QuadCriterion_MRS(1, y, Stub(), 1.0, **kw).sample(n_samples=2)


@pytest.mark.gpu
def test_driver_writes_posterior_files(tmp_path):
    drv = _driver()
    N = 251
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", str(N), "-hp", "5e3", "-ni", "3", "--synthetic", "config2",
                                      "--samples", "4", "--seed", "7"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    runs = list((tmp_path / "Results").iterdir())
    assert len(runs) == 1 and runs[0].name.endswith("_po_4")
    d = runs[0]
    x, mean, std, cov = (np.load(d / f"res_{k}.npy") for k in ("x", "mean", "std", "cov"))
    T = 4
    assert x.shape == (T * N * N,) and mean.shape == (T, N, N) and std.shape == (T, N, N) and cov.shape == (T, T, N, N)
    assert all(np.isfinite(a).all() for a in (x, mean, std, cov)) and std.min() >= 0 and std.max() > 0
    assert np.array_equal(cov, cov.transpose(1, 0, 2, 3)) and np.array_equal(std, np.sqrt(np.einsum("ttab->tab", cov)))
