"""Host checks of the plane-wise isotropic coupling: the preconditions the device comparison of tests/test_gpu_coupled_planes.py
rests on, asserted on the float64 oracle alone (tests/coupled_planes_oracle.py), and the argument rules of the Python layer.  No
GPU, no library."""
import numpy as np
import pytest

import coupled_planes_oracle as cp
import huber_planes_oracle as hp
from helpers import rel


@pytest.mark.parametrize("kind", cp.KINDS)
def test_preconditions_of_the_device_comparison(kind):
    """At the oracle's last iterate: the share of groups with w < 0.9 lies in the project's 5 % .. 95 % band in the planes of
    amplitude 1, and the coupled iterate is more than 100 x the comparison tolerance away from the "none" iterate of the same
    threshold -- a solver that ignored the coupling would fail the comparison by two orders of magnitude."""
    _, x0, y = hp.problem()
    ref, none = cp.reference(kind), cp.reference(kind, "none")
    for l in cp.ACTIVE:
        share, away = cp.share_small_weights(ref[l]["x"], kind), rel(ref[l]["x"], none[l]["x"])
        print(f"{kind}, plane {l}: w < 0.9 for {share:.2f} of the groups; {away:.2e} away from the 'none' iterate")
        assert 0.05 <= share <= 0.95
        assert away > 100 * hp.TOL_X
        c = np.array(ref[l]["crit"])
        assert ref[l]["nit"] == hp.NIT and np.all(np.diff(c) <= 0)                  # MM: the criterion never increases
    # the plane of amplitude 1e-3 stays quadratic under the shared threshold: what per-plane thresholds are for
    assert cp.share_small_weights(ref[hp.QUIET]["x"], kind) == 0.0
    assert not y[hp.EMPTY].any() and not x0[hp.EMPTY].any()


def test_the_mask_is_felt_under_the_coupling():
    _, x0, y = hp.problem()
    mask = hp.sample_mask(y.shape[1])
    masked = cp.solve_plane(0, y[0], x0[0], mask=mask)
    assert rel(masked["x"], cp.reference()[0]["x"]) > 100 * hp.TOL_X


def test_hebert_leahy_is_outside_the_band():
    """0.98 of the groups under w = 0.9: kernel checks only for this kind, no solver comparison"""
    _, x0, y = hp.problem()
    assert cp.share_small_weights(cp.solve_plane(0, y[0], x0[0], "hebert_leahy")["x"], "hebert_leahy") > 0.95


class _NoModel:
    ishape, osize, n_planes, batched = (2, 8, 8), 2 * 6, 2, True

    def __getattr__(self, name):
        raise AssertionError(f"the argument checks must not reach the model ({name})")


def test_argument_rules_without_the_library():
    from surfh_amd import blurred2d as b2
    from surfh_amd.spectro_blind_rectangle import MRSBlurred, QuadCriterion_MRS_2D
    y = np.zeros(12)
    # numbers without a coupling go to the scalar entry points as they came
    assert b2.plane_prior_args(2, 1.5, 0.1) == (1.5, 0.1, 0, False) and b2.plane_prior_args(2, 1.5, None) == (1.5, None, 0, False)
    r, d, code, ext = b2.plane_prior_args(2, 1.5, 0.1, "isotropic")
    assert ext and code == 1 and np.array_equal(r, [1.5, 1.5]) and np.array_equal(d, [0.1, 0.1]) and r.dtype == d.dtype == np.float64
    r, d, code, ext = b2.plane_prior_args(2, [1.0, 0.0], [0.1, float("inf")])
    assert ext and code == 0 and np.array_equal(r, [1.0, 0.0]) and np.array_equal(d, [0.1, np.inf])
    with pytest.raises(ValueError, match="needs delta"):
        b2.plane_prior_args(2, 1.0, None, "isotropic")
    with pytest.raises(ValueError, match="vector"):
        b2.plane_prior_args(2, 1.0, 0.1, "vector")
    with pytest.raises(ValueError, match="coupling must be one of"):
        b2.plane_prior_args(2, 1.0, 0.1, "radial")
    for bad in ([0.1, 0.2, 0.3], [[0.1, 0.2]], []):
        with pytest.raises(ValueError, match=r"delta has shape .* expected a number or \[2\]"):
            b2.plane_prior_args(2, 1.0, bad)
        with pytest.raises(ValueError, match=r"mu_reg has shape .* expected a number or \[2\]"):
            b2.plane_prior_args(2, bad, 0.1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="delta must be positive"):
            b2.plane_prior_args(2, 1.0, [0.1, bad])
        with pytest.raises(ValueError, match="delta must be positive"):
            b2.plane_prior_args(2, 1.0, bad, "isotropic")
    with pytest.raises(ValueError, match="mu_reg must be >= 0"):
        b2.plane_prior_args(2, [1.0, -1.0], 0.1)
    with pytest.raises(ValueError, match="needs delta"):
        b2.plane_prior_args(2, [1.0, 1.0], None)
    # the solver's own checks come before any library call (the model here has no plan)
    m = _NoModel()
    for kw, msg in ((dict(coupling="isotropic"), "needs delta"), (dict(delta=0.1, coupling="vector"), "vector"),
                    (dict(delta=[0.1] * 3), "delta has shape"), (dict(delta=[0.1, -0.1]), "delta must be positive"),
                    (dict(delta=0.0, coupling="isotropic"), "delta must be positive")):
        with pytest.raises(ValueError, match=msg):
            MRSBlurred.mmmg(m, y, mu_reg=1.0, **kw)
    with pytest.raises(ValueError, match="vector"):
        MRSBlurred.huber_planes_prior_dev(m, None, None, 1.0, 0.1, coupling="vector")
    with pytest.raises(ValueError, match="delta has shape"):
        MRSBlurred.huber_planes_curv_dev(m, None, None, None, [0.1] * 3)
    # the criterion class
    with pytest.raises(ValueError, match="needs delta"):
        QuadCriterion_MRS_2D(1.0, y, m, 1.0, coupling="isotropic")
    with pytest.raises(ValueError, match="vector"):
        QuadCriterion_MRS_2D(1.0, y, m, 1.0, delta=0.1, coupling="vector")
    with pytest.raises(ValueError, match="delta must be positive"):
        QuadCriterion_MRS_2D(1.0, y, m, 1.0, delta=0.0, coupling="isotropic")
    q = QuadCriterion_MRS_2D(1.0, y, m, 1.0, delta=0.1, coupling="isotropic")
    assert q.coupling == "isotropic" and QuadCriterion_MRS_2D(1.0, y, m, 1.0, delta=0.1).coupling == "none"
    with pytest.raises(ValueError, match="lcg minimises quadratic criteria only"):
        q.run_method("lcg", 3)


def test_criterion_value_is_the_isotropic_prior():
    """``get_crit_val`` under a coupling: mu |y - A x|^2 / 2 + mu_reg sum phi(sqrt(u_r^2 + u_c^2)), the planes summed"""
    from surfh_amd import potentials as P
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D

    class _Zero:
        ishape, osize, data_weights = (2, 8, 8), 12, None

        def forward(self, x):
            return np.zeros(12)

    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((2, 8, 8)), rng.standard_normal(12)
    for kind in ("huber", "hyperbolic"):
        q = QuadCriterion_MRS_2D(2.0, y, _Zero(), 1.5, delta=0.4, potential=kind, coupling="isotropic")
        want = 2.0 * np.sum(y ** 2) / 2 + 1.5 * sum(P.prior_value(x[l:l + 1], 0.4, kind, "isotropic") for l in range(2))
        assert abs(q.get_crit_val(x) - want) <= 1e-12 * want
        sep = QuadCriterion_MRS_2D(2.0, y, _Zero(), 1.5, delta=0.4, potential=kind)
        assert sep.get_crit_val(x) > q.get_crit_val(x) * 1.01                  # |u_r| + |u_c| >= sqrt(u_r^2 + u_c^2)


def test_driver_result_dir_and_usage():
    import importlib.util
    import os
    from click.testing import CliRunner
    sp = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                   "scripts", "deconvolution_mrs.py"))
    dd = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(dd)
    assert dd.result_dir("out", 0.05) == "out_huber_0.05" == dd.result_dir("out", 0.05, "huber", "none")
    assert dd.result_dir("out", 0.05, "hyperbolic", "isotropic") == "out_hyperbolic_0.05_cpl_isotropic"
    r = CliRunner().invoke(dd.main, ["-m", "qmm", "--coupling", "isotropic"])
    assert r.exit_code == 2 and "--coupling needs --delta" in r.output
    r = CliRunner().invoke(dd.main, ["-m", "qmm", "--delta", "0.1", "--coupling", "vector"])
    assert r.exit_code == 2 and "vector" in r.output
