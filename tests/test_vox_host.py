"""Host checks of the voxel-wise Huber criterion and of its float64 3MG restatement (tests/vox_oracle.py), of the preconditions
of the GPU comparison (tests/test_gpu_vox.py imports the same regime table), and of the fusion driver's --voxel option.
No GPU needed."""
import importlib.util
import os

import numpy as np
import pytest

import huber_oracle as ho
import vox_oracle as vo
from helpers import rel
from oracle import surfh_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def small():
    return vo.small_problem()


@pytest.mark.parametrize("Lc", [1, 2, 5])
def test_spectral_difference_and_its_transpose(Lc):
    rng = np.random.default_rng(Lc)
    x = rng.standard_normal((Lc, 6, 7))
    v = rng.standard_normal((Lc - 1, 6, 7))
    assert vo.diff_l(x).shape == (Lc - 1, 6, 7) and vo.diff_l_t(v).shape == (Lc, 6, 7)
    a, b = np.sum(vo.diff_l(x) * v), np.sum(x * vo.diff_l_t(v))
    assert abs(a - b) <= 1e-14 * max(np.linalg.norm(x) * np.linalg.norm(v), 1.0)
    if Lc == 1:
        assert np.array_equal(vo.diff_l_t(v), np.zeros_like(x))                   # the spectral term is empty
    else:                                                                        # open ends: one neighbour only, no wrap
        assert np.array_equal(vo.diff_l(x)[0], x[1] - x[0])
        assert np.array_equal(vo.diff_l_t(v)[0], -v[0]) and np.array_equal(vo.diff_l_t(v)[-1], v[-1])


def test_gradient_matches_finite_differences(small):
    """Central differences of J along standard-normal directions v, step h = 1e-5, in float64.
    Truncation: J is piecewise quadratic, so the central difference is exact except for the differences D x that cross a
    threshold inside the step.  A difference crosses when |D x| is within h |D v| ~ 1e-5 of delta ~ 1e-2, about one entry in a
    thousand, and each such entry is off by at most h |D v| of its own term phi'(D x) D v: a relative error near 1e-3 * 1e-3 = 1e-6
    of the prior part if all added up with one sign, and far less as they come with both signs.
    Rounding: eps J / h = 2e-16 J / 1e-5 = 2e-11 J, and J is about 10 |g.v| here, so 2e-10 of the derivative.
    A smaller h lowers the first and raises the second; at 1e-5 both are well below the asserted level of 1e-7 |g| |v|
    (|g.v| is itself of the order |g| |v| / sqrt(n) with n = 73 728, so the level is about 3e-5 of |g.v|)."""
    om, cube, y = small
    mu, sr, ds, lr, dl = 1.0, 40.0, 0.005, 20.0, 0.01
    rng = np.random.default_rng(2)
    x = cube + 0.1 * rng.standard_normal(om.ishape)
    g = vo.gradient(om, mu * om.adjoint(y), x, mu, sr, ds, lr, dl)
    h = 1e-5
    for _ in range(6):
        v = rng.standard_normal(om.ishape)
        fd = (vo.crit(om, y, x + h * v, mu, sr, ds, lr, dl) - vo.crit(om, y, x - h * v, mu, sr, ds, lr, dl)) / (2 * h)
        assert abs(fd - np.sum(g * v)) < 1e-7 * np.linalg.norm(g) * np.linalg.norm(v)
    # the prior alone, entry by entry: the four corners of the first and of the last plane, and an interior voxel
    gp = vo.prior_grad(x, sr, ds, lr, dl)
    L = om.ishape[0]
    for idx in [(0, 0, 0), (0, 47, 0), (0, 0, 47), (0, 47, 47), (L - 1, 0, 0), (L - 1, 47, 0), (L - 1, 0, 47), (L - 1, 47, 47),
                (11, 20, 31)]:
        e = np.zeros(om.ishape)
        e[idx] = h
        pp, pm = vo.prior_values(x + e, ds, dl), vo.prior_values(x - e, ds, dl)
        fd = (sr * (pp[0] - pm[0]) + lr * (pp[1] - pm[1])) / (2 * h)
        assert abs(fd - gp[idx]) < 1e-6 * (1 + abs(gp[idx]))


def test_majorant_touches_and_dominates(small):
    om, cube, y = small
    rng = np.random.default_rng(4)
    for name, (sr, ds, lr, dl, _, _) in vo.REGIMES.items():
        x = cube + 0.02 * rng.standard_normal(om.ishape)
        g = vo.gradient(om, om.adjoint(y), x, 1.0, sr, ds, lr, dl)
        j = vo.crit(om, y, x, 1.0, sr, ds, lr, dl)
        for scale in (0.0, 1e-3, 1e-2, 0.1, 1.0):
            v = scale * rng.standard_normal(om.ishape)
            maj = j + np.sum(g * v) + 0.5 * vo.majorant_quad(om, x, v, 1.0, sr, ds, lr, dl)
            jn = vo.crit(om, y, x + v, 1.0, sr, ds, lr, dl)
            assert jn <= maj + 1e-12 * abs(maj), (name, scale)
            if scale == 0.0:
                assert jn == maj == j


def test_anchored_to_the_map_domain_restatement(small):
    """With spec_reg = 0 the arrays are those of huber_oracle.mmmg on the same template-free model, bit for bit; with both
    thresholds infinite as well, those of orc.mmmg."""
    om, cube, y = small
    x0 = vo.start("rough", om, cube)
    a = vo.mmmg(om, y, 1.0, 40.0, 0.005, 0.0, 0.01, x0, max_iter=6)
    b = ho.mmmg(om, y, 1.0, 40.0, 0.005, x0, max_iter=6)
    assert a["nit"] == b["nit"] == 6 and np.array_equal(a["x"], b["x"])
    assert a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]
    c = vo.mmmg(om, y, 1.0, 40.0, INF, 0.0, INF, x0, max_iter=6)
    d = orc.mmmg(om, y, 1.0, 40.0, x0, max_iter=6)
    assert c["nit"] == d["nit"] == 6 and np.array_equal(c["x"], d["x"]) and c["grad_norm"] == d["grad_norm"]
    # and the spectral family does act when its weight is not 0
    e = vo.mmmg(om, y, 1.0, 40.0, 0.005, 20.0, 0.01, x0, max_iter=6)
    assert rel(e["x"], a["x"]) > 1e-2


@pytest.mark.parametrize("regime", list(vo.REGIMES))
def test_criterion_never_increases(small, regime):
    om, cube, y = small
    sr, ds, lr, dl, st, _ = vo.REGIMES[regime]
    r = vo.mmmg(om, y, 1.0, sr, ds, lr, dl, vo.start(st, om, cube), max_iter=24)
    c = np.array(r["crit"])
    assert r["nit"] == 24 and np.all(np.diff(c) <= 1e-12 * c[:-1]) and c[-1] < 0.5 * c[0]


@pytest.mark.parametrize("regime", list(vo.REGIMES))
def test_gpu_comparison_preconditions(small, regime):
    """What tests/test_gpu_vox.py relies on, checked on the oracle alone: both branches of both potentials are in play at the
    final iterate, and the Huber solution is far from the quadratic one."""
    om, cube, y = small
    sr, ds, lr, dl, st, nit = vo.REGIMES[regime]
    x0 = vo.start(st, om, cube)
    r = vo.mmmg(om, y, 1.0, sr, ds, lr, dl, x0, max_iter=nit)
    q = vo.mmmg(om, y, 1.0, sr, INF, lr, INF, x0, max_iter=nit)
    s_spat, s_spec = vo.shares(r["x"], ds, dl)
    assert r["nit"] == nit and 0.1 < s_spat < 0.9 and 0.1 < s_spec < 0.9, (s_spat, s_spec)
    assert rel(r["x"], q["x"]) > 20 * vo.X_TOL_BOUND


def test_regimes_cover_the_three_balances(small):
    om, cube, y = small
    ratio = {}
    for name, (sr, ds, lr, dl, st, nit) in vo.REGIMES.items():
        x = vo.mmmg(om, y, 1.0, sr, ds, lr, dl, vo.start(st, om, cube), max_iter=nit)["x"]
        ps, pl = vo.prior_values(x, ds, dl)
        ratio[name] = sr * ps / (lr * pl)
    assert ratio["spatial"] > 2 and ratio["spectral"] < 0.5 and 0.5 <= ratio["both"] <= 2


def _driver():
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_driver_voxel_option():
    from click.testing import CliRunner
    drv = _driver()
    defaults = {p.name: p.default for p in drv.main.params}
    assert defaults["voxel"] is False and defaults["spec_reg"] == 1.0 and defaults["spec_delta"] == 1.0
    r = CliRunner().invoke(drv.main, ["--help"])
    assert r.exit_code == 0 and "--voxel" in r.output and "--spec_reg" in r.output and "--spec_delta" in r.output
    # lcg and bad thresholds are refused before anything is built
    r = CliRunner().invoke(drv.main, ["--synthetic", "small", "--voxel", "--method", "lcg"])
    assert r.exit_code == 2 and "--voxel" in r.output
    r = CliRunner().invoke(drv.main, ["--synthetic", "small", "--voxel", "--method", "mmmg", "--spec_delta", "0"])
    assert r.exit_code == 2
    # present callers of result_dir_name see no change; the voxel run gets its own directory
    base = drv.result_dir_name("mmmg", 12, 4, 50, 5e3, False)
    assert base == "mmmg_MC_12_MO_4_Temp_4_nit_50_mu_5.00e+03_SD_False/"
    assert drv.result_dir_name("mmmg", 12, 4, 50, 5e3, False, 0.25) == base[:-1] + "_huber_2.50e-01/"
    assert drv.result_dir_name("mmmg", 12, 0, 50, 5e3, False, 0.25, voxel=True).endswith("_huber_2.50e-01_vox/")


def test_python_entry_points_exist():
    from surfh_amd import _lib, algorithms
    from surfh_amd.models import spectroSigRLSCT
    for n in ("surfh_mmmg_huber_vox", "surfh_huber_vox_prior_dev", "surfh_huber_vox_curv_dev"):
        assert n in _lib.EXPORTS
    assert callable(algorithms.vox_reconstruction) and callable(algorithms.vox_criterion)
    assert all(hasattr(spectroSigRLSCT, n) for n in ("mmmg_vox", "huber_vox_prior_dev", "huber_vox_curv_dev"))
    assert spectroSigRLSCT.huber_prior_values is None
