"""Non-negative fusion without a GPU: the float64 restatement (tests/nonneg_oracle.py) against an independent solver, its two residual
forms, the preconditions that keep the device comparison (tests/test_gpu_nonneg.py) from being vacuous, the penalty estimate and
the argument checks of the Python wrappers and of the driver."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner
from scipy.optimize import nnls

import nonneg_oracle as no
import problems
from oracle import surfh_oracle as orc
from surfh_amd import nonneg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense_problem(n=60, seed=3):
    """A [2n, n] and y with Q = A^T A SPD, b = A^T y, and a solution with about half its constraints active."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((2 * n, n))
    xt = np.where(rng.random(n) < 0.5, 0.0, rng.random(n) + 0.5) - np.where(rng.random(n) < 0.5, 0.0, 1.0)
    y = A @ xt + 0.05 * rng.standard_normal(2 * n)
    return A, y


def test_long_run_reaches_nnls():
    A, y = dense_problem()
    Q, b = A.T @ A, A.T @ y
    ref, _ = nnls(A, y, maxiter=10000)
    share = np.mean(ref == 0)
    assert 0.3 <= share <= 0.7, share                        # about half the constraints active
    normal = lambda v: Q @ v
    rho = float(np.trace(Q) / Q.shape[0])                    # the mean eigenvalue, what nonneg_rho estimates
    res = no.admm(normal, b, rho, outer=4000, inner=3, refresh=10)
    err = np.linalg.norm(res["z"] - ref) / np.linalg.norm(ref)
    print(f"dense n=60: active share {share:.2f}, |z - nnls| / |nnls| = {err:.2e}, KKT {no.kkt(res['z'], normal, b):.2e}")
    assert err < 1e-8
    assert no.kkt(res["z"], normal, b) < 1e-8 * np.linalg.norm(b)
    assert res["z"].min() >= 0.0
    k0 = no.kkt(no.admm(normal, b, rho, outer=5, inner=3)["z"], normal, b)
    assert no.kkt(res["z"], normal, b) < 1e-6 * k0           # it goes to zero from where a short run stands


def test_refreshed_and_carried_forms_agree():
    A, y = dense_problem(seed=4)
    Q, b = A.T @ A, A.T @ y
    rho = float(np.trace(Q) / Q.shape[0])
    x0 = np.random.default_rng(1).standard_normal(b.size)    # a start with negative entries: the r of row 0 carries rho (z - x)
    a = no.admm(lambda v: Q @ v, b, rho, x0=x0, outer=12, inner=4, refresh=1)
    c = no.admm(lambda v: Q @ v, b, rho, x0=x0, outer=12, inner=4, refresh=0)
    assert np.linalg.norm(a["z"] - c["z"]) <= 1e-12 * np.linalg.norm(a["z"])
    assert np.allclose(a["trace"], c["trace"], rtol=1e-9, atol=1e-18)


def test_infinite_penalty_keeps_a_feasible_start():
    A, y = dense_problem(seed=5)
    Q, b = A.T @ A, A.T @ y
    x0 = np.random.default_rng(2).random(b.size)
    res = no.admm(lambda v: Q @ v, b, 1e30, x0=x0, outer=3, inner=3)
    assert np.array_equal(res["z"], x0)


def test_tolerance_stops_after_the_first_outer_iteration():
    A, y = dense_problem(seed=6)
    res = no.admm(lambda v: A.T @ (A @ v), A.T @ y, 100.0, outer=9, inner=2, tol=1e30)
    assert res["nit"] == 1 and res["trace"].shape == (2, 4)


# ---- the device comparison's problem: what must hold for it to test anything --------------------------------------------------------
@pytest.fixture(scope="module")
def blob_case():
    cfg = problems.config1()
    om = problems.oracle_model(cfg)
    truth, y = no.blob_data(om, 4, cfg["N"])
    return cfg, om, truth, y


def test_preconditions_of_the_device_comparison(blob_case):
    """Config 1, the four blobs, 1 % noise, mu = 1, mu_reg = 5e3, rho = 6e4, 4 x 4.  The start is ``case_start``, not zeros: from zeros
    the last precondition fails (29 - 30 % of the entries within 1e-4 max|x| of zero at every outer iteration: the pixels outside
    the field of view, which 16 iterations from zero have not reached), and the rule is to change the problem, not the assertion.
    Measured with this start: 40 % negative, active share 0.40 - 0.41, 5.8e-2 from the clipped iterate, at most 0.05 % near zero."""
    cfg, om, truth, y = blob_case
    c = no.CASE
    x0 = no.case_start(om.ishape)
    assert truth.shape == (4, 64, 64) and truth.min() == 0.0 and np.mean(truth == 0) > 0.5
    normal, b, _, _ = no.maps_problem(om, y, c["mu"], c["mu_reg"])
    free = orc.lcg(om, y, c["mu"], c["mu_reg"], x0, max_iter=c["outer"] * c["inner"])["x"]
    neg = float(np.mean(free < 0))
    res = no.admm(normal, b, c["rho"], x0=x0, outer=c["outer"], inner=c["inner"])
    active = res["trace"][1:, 3] / b.size
    clipped = np.maximum(free, 0.0)
    dist = float(np.linalg.norm(res["z"] - clipped) / np.linalg.norm(clipped))
    near = np.array(res["near"]) / b.size
    print(f"unconstrained lcg after 16: {neg:.1%} negative (min {free.min():.3f}, max {free.max():.3f}); active share "
          f"{' '.join(f'{a:.3f}' for a in active)}; |z - clip| / |clip| = {dist:.3f}; near-zero share {near.max():.2e}")
    assert neg >= 0.20
    assert np.all((active >= 0.15) & (active <= 0.6))
    assert dist > 1e-2
    assert np.all(near < 0.01)
    assert res["z"].min() >= 0.0


# ---- the penalty estimate and the wrappers' checks ----------------------------------------------------------------------------------
def test_rayleigh_rho_is_the_probes_quotient():
    Q = np.diag(np.arange(1.0, 41.0))
    v = np.random.default_rng(7).standard_normal(40)
    rho = nonneg.rayleigh_rho(lambda u: float(u @ Q @ u), (40,), seed=7)
    assert rho == pytest.approx(float(v @ Q @ v) / float(v @ v), rel=1e-14)
    assert 10 < rho < 31                                     # about the mean eigenvalue, 20.5
    assert rho != nonneg.rayleigh_rho(lambda u: float(u @ Q @ u), (40,), seed=8)


class _FakeModel(nonneg.NonnegOps):
    """The operator pieces nonneg_rho reads, on a dense A."""

    def __init__(self, A, T, n, weights=None):
        self.A, self.ishape, self.data_weights = A, (T, n, n), weights

    def get_prior(self):
        return "separated"

    def forward(self, x):
        return self.A @ np.asarray(x).reshape(-1)


def test_nonneg_rho_formula():
    rng = np.random.default_rng(11)
    T, n = 2, 5
    A = rng.standard_normal((70, T * n * n))
    w = rng.random(70)
    w[::7] = 0.0
    v = np.random.default_rng(3).standard_normal((T, n, n))
    prior = np.sum(orc.diff_r(v) ** 2) + np.sum(orc.diff_c(v) ** 2)
    for weights, own in ((None, None), (w, None), (None, w)):
        m = _FakeModel(A, T, n, own)
        ww = np.ones(70) if weights is None and own is None else w
        want = (2.0 * np.sum(ww * (A @ v.ravel()) ** 2) + 30.0 * prior) / np.sum(v * v)
        assert m.nonneg_rho(2.0, 30.0, seed=3, weights=weights) == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("kw", [dict(rho=0.0), dict(rho=-1.0), dict(rho=np.inf), dict(rho=np.nan), dict(inner=0), dict(outer=-1),
                                dict(refresh=-1)])
def test_wrapper_argument_checks(kw):
    args = dict(rho=1.0, outer=3, inner=2, refresh=0)
    nonneg.check_nonneg_args(**args)
    nonneg.check_nonneg_args(**dict(args, rho=None))
    with pytest.raises(ValueError, match=next(iter(kw))):
        nonneg.check_nonneg_args(**dict(args, **kw))


def test_refine_templates_checks_before_any_library_call():
    from surfh_amd.fusion import refine_templates
    with pytest.raises(ValueError, match="rho"):
        refine_templates(None, None, 1.0, 1.0, 1.0, 1, 1, 1, nonneg=True, rho=-2.0)
    with pytest.raises(ValueError, match="inner"):
        refine_templates(None, None, 1.0, 1.0, 1.0, 1, 1, 1, nonneg=True, inner=0)
    with pytest.raises(ValueError, match="nonneg"):
        refine_templates(None, None, 1.0, 1.0, 1.0, 1, 1, 1, rho=3.0)


def _driver():
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_driver_flags():
    """raised before any model is built: this runs without a GPU"""
    drv = _driver()
    base = ["--synthetic", "small", "--nonneg"]
    for extra, word in ((["--method", "mmmg"], "lcg"), (["--samples", "4"], "--samples"), (["--voxel", "--method", "mmmg"], "lcg"),
                        (["--imager", "2"], "--imager"), (["--checkpoint_every", "2"], "checkpoints"),
                        (["--refine_templates", "2", "--outer", "3"], "--outer")):
        r = CliRunner().invoke(drv.main, base + extra)
        assert r.exit_code == 2 and word in r.output, r.output
    for extra, hint in ((["--rho", "0"], "--rho"), (["--rho", "nan"], "--rho"), (["--inner", "0"], "--inner"), (["--outer", "0"], "--outer")):
        r = CliRunner().invoke(drv.main, base + extra)
        assert r.exit_code == 2 and "Invalid value" in r.output and hint in r.output, r.output
    for extra in (["--rho", "5"], ["--outer", "3"], ["--inner", "3"]):
        r = CliRunner().invoke(drv.main, ["--synthetic", "small"] + extra)
        assert r.exit_code == 2 and "--nonneg" in r.output, r.output
    assert drv.result_dir_name("lcg", 1, 4, 5, 5e3, False, nonneg=True).endswith("_nn/")
    assert drv.result_dir_name("lcg", 1, 4, 5, 5e3, False, refine=2, nonneg=True).endswith("_tpl_2_nn/")
    assert drv.result_dir_name("lcg", 1, 4, 5, 5e3, False) == drv.result_dir_name("lcg", 1, 4, 5, 5e3, False, nonneg=False)
