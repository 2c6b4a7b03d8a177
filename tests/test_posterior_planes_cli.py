"""scripts/deconvolution_mrs.py --samples: the usage errors, raised before any model is built (no GPU), and the result directory."""
import importlib.util
import os

import pytest
from click.testing import CliRunner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drv():
    spec = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,word", [(["--samples", "4", "-m", "qmm"], "lcg"), (["--samples", "4", "-m", "qmm", "--delta", "0.1"], "lcg"),
                                        (["--samples", "4", "--delta", "0.1"], "--delta"), (["--samples", "4", "--nonneg"], "--nonneg"),
                                        (["--samples", "1"], "at least 2"), (["--samples", "0"], "at least 2"),
                                        (["--samples", "-3"], "at least 2")])
def test_samples_usage_errors(drv, extra, word, tmp_path):
    out = str(tmp_path / "res")
    r = CliRunner().invoke(drv.main, extra + ["--out", out])
    assert r.exit_code == 2 and word in r.output and "--samples" in r.output, r.output
    assert not os.path.exists(out) and not os.path.exists(drv.samples_dir(out, extra[1]))


def test_result_directory_name(drv):
    assert drv.samples_dir("deconvolution_results", 16) == "deconvolution_results_po_16"
    assert drv.samples_dir("a/b", 2) == "a/b_po_2"
