"""Host checks of the Huber-prior criterion and of its float64 3MG restatement (tests/huber_oracle.py), and of the fusion
driver's --delta option.  No GPU needed."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.optimize

import huber_oracle as ho
from oracle import surfh_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    return ho.small_problem()


def test_potential_at_the_breakpoints():
    d = 0.7
    u = np.array([0.0, d, -d, np.nextafter(d, 2), 2.0, -3.0, 0.3])
    assert np.array_equal(ho.phi(u, d), [0.0, d * d / 2, d * d / 2, d * (np.nextafter(d, 2) - d / 2), d * (2.0 - d / 2),
                                         d * (3.0 - d / 2), 0.3 * 0.3 / 2])
    assert np.array_equal(ho.dphi(u, d), [0.0, d, -d, d, d, -d, 0.3])
    assert np.array_equal(ho.weight(u, d), [1.0, 1.0, 1.0, d / np.nextafter(d, 2), d / 2.0, d / 3.0, 1.0])
    # continuous with a continuous derivative at |u| = delta; w = phi' / u away from 0
    e = 1e-9
    assert abs(ho.phi(d + e, d) - ho.phi(d - e, d)) < 2 * d * e * 1.01
    nz = u != 0
    assert np.allclose(ho.weight(u, d)[nz], ho.dphi(u, d)[nz] / u[nz], rtol=1e-15, atol=0)
    # delta = inf: the quadratic potential
    assert np.array_equal(ho.phi(u, np.inf), u * u / 2) and np.array_equal(ho.dphi(u, np.inf), u)
    assert np.array_equal(ho.weight(u, np.inf), np.ones_like(u))


def test_gradient_matches_finite_differences(small):
    om, maps, y = small
    mu, mur, delta = 1.0, 0.3, 0.1
    rng = np.random.default_rng(2)
    x = maps + 0.1 * rng.standard_normal(om.ishape)
    g = ho.gradient(om, mu * om.adjoint(y), x, mu, mur, delta)
    h = 1e-6
    for _ in range(6):
        v = rng.standard_normal(om.ishape)
        fd = (ho.crit(om, y, x + h * v, mu, mur, delta) - ho.crit(om, y, x - h * v, mu, mur, delta)) / (2 * h)
        assert abs(fd - np.sum(g * v)) < 1e-5 * (abs(fd) + np.linalg.norm(g) * np.linalg.norm(v) * 1e-3)
    # the prior alone, entry by entry, across both borders of both axes (the circular wrap)
    gp = ho.prior_grad(x, delta)
    for idx in [(0, 0, 0), (1, 47, 0), (2, 0, 47), (3, 47, 47), (0, 20, 31)]:
        e = np.zeros(om.ishape)
        e[idx] = h
        fd = (ho.prior_value(x + e, delta) - ho.prior_value(x - e, delta)) / (2 * h)
        assert abs(fd - gp[idx]) < 1e-6


def test_infinite_delta_is_the_quadratic_3mg(small):
    om, maps, y = small
    for x0 in (np.full(om.ishape, 0.5), np.zeros(om.ishape)):
        a = ho.mmmg(om, y, 1.0, 0.3, np.inf, x0, max_iter=8)
        b = orc.mmmg(om, y, 1.0, 0.3, x0, max_iter=8)
        assert a["nit"] == b["nit"] == 8
        assert np.max(np.abs(a["x"] - b["x"])) <= 1e-12 * np.max(np.abs(b["x"]))
        assert np.allclose(a["grad_norm"], b["grad_norm"], rtol=1e-12, atol=0)
        assert abs(a["crit"][-1] - orc.crit_val(om, y, a["x"], 1.0, 0.3)) < 1e-12 * a["crit"][-1]


@pytest.mark.parametrize("delta", [0.01, 0.1, 1.0])
def test_criterion_never_increases(small, delta):
    """The MM guarantee: each step minimises a majorant that touches J at the current iterate."""
    om, maps, y = small
    r = ho.mmmg(om, y, 1.0, 0.3, delta, np.full(om.ishape, 0.5), max_iter=30)
    c = np.array(r["crit"])
    assert r["nit"] == 30 and np.all(np.diff(c) <= 1e-12 * c[:-1]) and c[-1] < 0.5 * c[0]


def test_converges_to_the_minimiser(small):
    """mu scaled so that the data and prior curvatures are comparable (with mu = 1 neither solver gets there in minutes)."""
    om, maps, y = small
    mu, mur, delta = 1e-4, 1.0, 0.5
    b = mu * om.adjoint(y)

    def fun(v):
        x = v.reshape(om.ishape)
        return ho.crit(om, y, x, mu, mur, delta), ho.gradient(om, b, x, mu, mur, delta).ravel()

    ref = scipy.optimize.minimize(fun, np.full(om.isize, 0.5), jac=True, method="L-BFGS-B",
                                  options={"maxiter": 2000, "ftol": 1e-15, "gtol": 1e-10})
    r = ho.mmmg(om, y, mu, mur, delta, np.full(om.ishape, 0.5), max_iter=300)
    j_ref, j = float(ref.fun), r["crit"][-1]
    assert abs(j - j_ref) < 1e-6 * j_ref
    assert np.linalg.norm(r["x"].ravel() - ref.x) < 1e-3 * np.linalg.norm(ref.x)


def _driver():
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_driver_delta_option():
    from click.testing import CliRunner
    drv = _driver()
    defaults = {p.name: p.default for p in drv.main.params}
    assert defaults["delta"] is None
    r = CliRunner().invoke(drv.main, ["--help"])
    assert r.exit_code == 0 and "--delta" in r.output
    # lcg and a non-positive threshold are refused before anything is built
    r = CliRunner().invoke(drv.main, ["--synthetic", "config2", "--method", "lcg", "--delta", "0.1"])
    assert r.exit_code == 2 and "--delta" in r.output
    r = CliRunner().invoke(drv.main, ["--synthetic", "config2", "--method", "mmmg", "--delta", "0"])
    assert r.exit_code == 2
    # the result directory changes only when --delta is given
    base = drv.result_dir_name("mmmg", 12, 4, 50, 5e3, False)
    assert base == "mmmg_MC_12_MO_4_Temp_4_nit_50_mu_5.00e+03_SD_False/"
    assert drv.result_dir_name("mmmg", 12, 4, 50, 5e3, False, None) == base
    assert drv.result_dir_name("mmmg", 12, 4, 50, 5e3, False, 0.25) == "mmmg_MC_12_MO_4_Temp_4_nit_50_mu_5.00e+03_SD_False_huber_2.50e-01/"


def test_criterion_class_rejects_quadratic_only_options():
    from surfh_amd.fusion import QuadCriterion_MRS, huber_phi

    class Dummy:
        ishape = (4, 8, 8)

    with pytest.raises(ValueError):
        QuadCriterion_MRS(1.0, np.zeros(3), Dummy(), 1.0, gradient="joint", delta=0.1)
    with pytest.raises(ValueError):
        QuadCriterion_MRS(1.0, np.zeros(3), Dummy(), 1.0, delta=0.0)
    with pytest.raises(ValueError):
        QuadCriterion_MRS(1.0, np.zeros(3), Dummy(), 1.0, delta=0.1).run_method("lcg", 3)
    u = np.array([0.0, 0.5, -2.0])
    assert np.array_equal(huber_phi(u, 0.5), ho.phi(u, 0.5)) and np.array_equal(huber_phi(u, np.inf), ho.phi(u, np.inf))
