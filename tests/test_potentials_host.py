"""The potentials of the 3MG solvers on the host: the float64 restatements of surfh_amd/potentials.py, the generalised oracle of
tests/potentials_oracle.py (majorant, descent, bit identity with the Huber oracles), the preconditions of the device comparisons
of tests/test_gpu_potentials.py, the slot / kind validation of the C ABI, the drivers' options and directory names, and the
ValueError cases of the Python interface.  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

import huber_oracle as ho
import huber_planes_oracle as hpo
import potentials_oracle as po
import robust_oracle as ro
import vox_oracle as vo
from oracle import surfh_oracle as orc
from surfh_amd import fusion, potentials as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
KINDS = list(P.NAMES)


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- surfh_amd/potentials.py -------------------------------------------------------------------------------------------------------
def test_names_and_codes():
    assert P.KINDS == {"huber": 0, "hyperbolic": 1, "hebert_leahy": 2} and P.NAMES == ("huber", "hyperbolic", "hebert_leahy")
    assert P.SLOTS == {"spatial": 0, "spectral": 1, "data": 2}
    assert [P.kind_code(k) for k in KINDS] == [0, 1, 2] and P.kind_code(2) == 2 and P.kind_name(1) == "hyperbolic"
    for bad in ("Huber", "geman_mcclure", 3, -1, None, True, 1.0):
        with pytest.raises(ValueError):
            P.kind_code(bad)


@pytest.mark.parametrize("kind", KINDS)
def test_dphi_is_the_derivative_of_phi(kind):
    delta = 0.7
    # away from Huber's kink, where the central difference of the piecewise phi is not its derivative to second order
    u = np.concatenate([np.linspace(-20, 20, 4001) * delta, np.array([1e-3, -1e-3, 0.0]) * delta])
    u = u[np.abs(np.abs(u) - delta) > 1e-3 * delta]
    h = 1e-6 * delta
    fd = (P.phi(u + h, delta, kind) - P.phi(u - h, delta, kind)) / (2 * h)
    # truncation h^2 phi''' / 6 <= 1e-12 / delta, rounding eps phi / h <= 2.2e-16 * 200 delta^2 / (1e-6 delta)
    assert np.max(np.abs(fd - P.dphi(u, delta, kind))) < 1e-7 * delta
    np.testing.assert_allclose(P.weight(u, delta, kind) * u, P.dphi(u, delta, kind), rtol=1e-15, atol=0)
    assert np.all(P.phi(u, delta, kind) >= 0) and P.phi(0.0, delta, kind) == 0.0 and P.weight(0.0, delta, kind) == 1.0
    # normalisation: phi ~ u^2 / 2 near 0
    assert abs(P.phi(1e-4 * delta, delta, kind) / (0.5 * (1e-4 * delta) ** 2) - 1) < 1e-7


@pytest.mark.parametrize("kind", KINDS)
def test_weight_meets_the_geman_reynolds_condition(kind):
    delta = 0.3
    a = np.concatenate([[0.0], np.logspace(-30, 30, 2001)]) * delta
    w = P.weight(a, delta, kind)
    assert np.all(w > 0) and np.all(w <= 1) and np.all(np.diff(w) <= 0)          # in (0, 1], non-increasing in |u|
    np.testing.assert_array_equal(P.weight(-a, delta, kind), w)                  # even
    if kind != "huber":
        assert np.all(np.diff(w[a > 1e-6 * delta]) < 0)                          # strictly decreasing once t^2 is above rounding


@pytest.mark.parametrize("kind", KINDS)
def test_infinite_delta_is_the_quadratic_bit_for_bit(kind):
    u = np.random.default_rng(0).standard_normal(1000) * np.logspace(-20, 20, 1000)
    np.testing.assert_array_equal(P.phi(u, INF, kind), np.abs(u) * np.abs(u) / 2)
    np.testing.assert_array_equal(P.dphi(u, INF, kind), u)
    np.testing.assert_array_equal(P.weight(u, INF, kind), np.ones_like(u))


@pytest.mark.parametrize("kind", KINDS)
def test_no_nan_over_sixty_decades(kind):
    t = np.logspace(-30, 30, 601)
    for delta in (1.0, 1e-20, float(np.finfo(np.float32).tiny), 1e20):
        u = np.concatenate([t, -t]) * delta
        u = u[np.isfinite(u)]
        for f in (P.phi, P.dphi, P.weight):
            assert np.all(np.isfinite(f(u, delta, kind))), (f.__name__, delta)
    # the large-|t| limits: phi' -> delta sign u (hyperbolic), phi' -> delta^2 / u (Hebert-Leahy)
    if kind == "hyperbolic":
        np.testing.assert_allclose(P.dphi(np.array([1e25, -1e25]), 1.0, kind), [1.0, -1.0], rtol=1e-15)
        np.testing.assert_allclose(P.phi(1e25, 1.0, kind), 1e25 - 1.0, rtol=1e-15)
    if kind == "hebert_leahy":
        np.testing.assert_allclose(P.dphi(1e25, 1.0, kind), 1e-25, rtol=1e-15)
        np.testing.assert_allclose(P.phi(1e25, 1.0, kind), 0.5 * np.log1p(1e50), rtol=1e-15)
        # the two branches of log1p(t^2) / t^2 meet
        np.testing.assert_allclose(P.phi(np.array([0.99e-4, 1.01e-4]), 1.0, kind), 0.5 * np.log1p(np.array([0.99e-4, 1.01e-4]) ** 2),
                                   rtol=1e-15)


def test_delta_squared_forms_agree_with_the_textbook_ones():
    u, delta = np.linspace(-9, 9, 181), 0.8
    t = u / delta
    np.testing.assert_allclose(P.phi(u, delta, "hyperbolic"), delta ** 2 * (np.sqrt(1 + t * t) - 1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(P.phi(u, delta, "hebert_leahy"), delta ** 2 / 2 * np.log(1 + t * t), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(P.dphi(u, delta, "hyperbolic"), u / np.sqrt(1 + t * t), rtol=1e-15)
    np.testing.assert_allclose(P.dphi(u, delta, "hebert_leahy"), u / (1 + t * t), rtol=1e-15)


def test_huber_is_the_existing_arithmetic():
    u = np.random.default_rng(1).standard_normal((7, 50)) * 3
    for delta in (0.5, 2.0, INF):
        np.testing.assert_array_equal(P.phi(u, delta, "huber"), fusion.huber_phi(u, delta))
        np.testing.assert_array_equal(P.phi(u, delta), ho.phi(u, delta))
        np.testing.assert_array_equal(P.dphi(u, delta), ho.dphi(u, delta))
        np.testing.assert_array_equal(P.weight(u, delta), ho.weight(u, delta))
    y, ax, w = u[0], u[1], np.abs(u[2])
    assert fusion.robust_data_value(y, ax, w, 1.5, potential="huber") == fusion.robust_data_value(y, ax, w, 1.5)
    for kind in po.NEW_KINDS:
        want = float(P.phi(np.sqrt(w) * (y - ax), 1.5, kind).sum())
        assert abs(fusion.robust_data_value(y, ax, w, 1.5, potential=kind) - want) <= 1e-14 * want
        assert fusion.robust_data_value(y, ax, None, 1.5, kind) == float(P.phi(y - ax, 1.5, kind).sum())


# ---- the generalised oracle ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    om, maps, y = ho.small_problem()
    x0 = maps + 0.1 * np.random.default_rng(3).standard_normal(om.ishape)
    return om, y, x0


def test_huber_runs_are_the_existing_oracles_bit_for_bit(small):
    om, y, x0 = small
    a, b = po.mmmg(om, y, 1.0, 50.0, 0.05, x0, "huber", max_iter=4), ho.mmmg(om, y, 1.0, 50.0, 0.05, x0, max_iter=4)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]
    w = np.random.default_rng(2).random(om.oshape) + 0.5
    a = po.mmmg_robust(om, y, 1.0, 0.02, 50.0, 0.05, x0, w=w, max_iter=3)
    b = ro.mmmg(om, y, 1.0, 0.02, 50.0, 0.05, x0, w=w, max_iter=3)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]
    c = po.vox_case()
    a = po.mmmg_vox(c["om"], c["y"], 1.0, 40.0, 0.005, 20.0, 0.01, c["x0"], max_iter=3)
    b = vo.mmmg(c["om"], c["y"], 1.0, 40.0, 0.005, 20.0, 0.01, c["x0"], max_iter=3)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]
    _, px0, py = hpo.problem()
    a, b = po.solve_plane(0, py[0], px0[0], max_iter=3), hpo.solve_plane(0, py[0], px0[0], max_iter=3)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"]
    # and the oracle modules are as they were
    assert ho.phi.__module__ == "huber_oracle" and vo.weight is ho.weight and ro.dphi is ho.dphi


@pytest.mark.parametrize("kind", po.NEW_KINDS)
def test_infinite_delta_reproduces_the_huber_oracle_at_infinite_delta(small, kind):
    om, y, x0 = small
    a, b = po.mmmg(om, y, 1.0, 50.0, INF, x0, kind, max_iter=5), ho.mmmg(om, y, 1.0, 50.0, INF, x0, max_iter=5)
    # the potentials agree bit for bit at delta = inf (above); the only difference is ho.weight's expression of the ones
    assert po.rel(a["x"], b["x"]) < 1e-12 and np.allclose(a["grad_norm"], b["grad_norm"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("kind", po.NEW_KINDS)
def test_majorant_touches_and_dominates(small, kind):
    om, y, x0 = small
    mu, dd, mur, delta = 1.0, po.Th(0.02, kind), 50.0, po.Th(0.05, kind)
    rng = np.random.default_rng(7)
    with po.patched():
        j0 = ro.crit(om, y, x0, mu, dd, mur, delta)
        g = ro.gradient(om, y, x0, mu, dd, mur, delta)
        assert ro.majorant_quad(om, y, x0, np.zeros_like(x0), mu, dd, mur, delta) == 0.0          # touches J at x
        for scale in (1e-3, 1e-1, 1.0, 30.0):
            v = scale * rng.standard_normal(x0.shape)
            q = j0 + np.sum(g * v) + 0.5 * ro.majorant_quad(om, y, x0, v, mu, dd, mur, delta)
            j = ro.crit(om, y, x0 + v, mu, dd, mur, delta)
            assert q >= j * (1 - 1e-12), (scale, q, j)
        # tangent: the gap is second order in the move
        v = rng.standard_normal(x0.shape)
        gaps = []
        for eps in (1e-3, 1e-4):
            q = j0 + eps * np.sum(g * v) + 0.5 * eps ** 2 * ro.majorant_quad(om, y, x0, v, mu, dd, mur, delta)
            gaps.append(q - ro.crit(om, y, x0 + eps * v, mu, dd, mur, delta))
        assert 0 <= gaps[1] < gaps[0] * 0.02
    # the cube's majorant with mixed kinds
    c = po.vox_case()
    ds, dl = po.Th(0.005, kind), po.Th(0.01, "hebert_leahy" if kind == "hyperbolic" else "hyperbolic")
    with po.patched():
        x = c["x0"]
        j0 = vo.crit(c["om"], c["y"], x, 1.0, 40.0, ds, 20.0, dl)
        g = vo.gradient(c["om"], 1.0 * c["om"].adjoint(c["y"]), x, 1.0, 40.0, ds, 20.0, dl)
        for scale in (1e-2, 1.0):
            v = scale * rng.standard_normal(x.shape)
            q = j0 + np.sum(g * v) + 0.5 * vo.majorant_quad(c["om"], x, v, 1.0, 40.0, ds, 20.0, dl)
            assert q >= vo.crit(c["om"], c["y"], x + v, 1.0, 40.0, ds, 20.0, dl) * (1 - 1e-12)


@pytest.mark.parametrize("kind", po.NEW_KINDS)
def test_criterion_never_increases_over_eight_iterations(small, kind):
    om, y, x0 = small
    runs = [po.mmmg(om, y, 1.0, 50.0, 0.05, x0, kind, max_iter=8),
            po.mmmg_robust(om, y, 1.0, 0.02, 50.0, 0.05, x0, potential=kind, data_potential=kind, max_iter=8),
            po.vox_run(kind, "hebert_leahy" if kind == "hyperbolic" else "hyperbolic"),
            po.planes_run(kind, 0)]
    for r in runs:
        assert r["nit"] == 8 and len(r["crit"]) == 9 and np.all(np.diff(r["crit"]) <= 0) and r["crit"][-1] < r["crit"][0]


# ---- preconditions of the device comparisons (tests/test_gpu_potentials.py) -----------------------------------------------------------
def _check(name, share, away):
    print(f"{name}: w < 0.9 for {share:.0%} of the differences, {away:.1e} away from the delta = inf iterate")
    assert share >= 0.30 and away >= 1e-2


@pytest.mark.parametrize("kind", po.NEW_KINDS)
def test_gpu_comparison_preconditions(kind):
    import problems
    # the problems are the existing regimes
    c = po.maps_case()
    assert c["om"].ishape == problems.oracle_model(problems.config1(), box="direct").ishape
    assert po.vox_case()["om"].ishape == (32, 48, 48) and (hpo.L, hpo.N) == (5, 96)
    x = po.maps_run(kind)["x"]
    _check(f"maps {kind}", po.share_small_weights([orc.diff_r(x), orc.diff_c(x)], po.MAPS["delta"], kind),
           po.rel(x, po.maps_run(kind, INF)["x"]))
    other = "hebert_leahy" if kind == "hyperbolic" else "huber"
    for ks, kl in ((kind, other), (kind, kind)):
        x, xq = po.vox_run(ks, kl)["x"], po.vox_run(ks, kl, inf=True)["x"]
        _check(f"cube {ks} (spatial)", po.share_small_weights([orc.diff_r(x), orc.diff_c(x)], po.VOX["spat_delta"], ks), po.rel(x, xq))
        _check(f"cube {kl} (spectral)", po.share_small_weights([vo.diff_l(x)], po.VOX["spec_delta"], kl), po.rel(x, xq))
    for l in (0, 1, 4):                                   # plane 2 is the fully quadratic one by construction, plane 3 has no data
        x = po.planes_run(kind, l)["x"]
        _check(f"plane {l} {kind}", po.share_small_weights([orc.diff_r(x[None]), orc.diff_c(x[None])], po.PLANES["delta"], kind),
               po.rel(x, po.planes_run(kind, l, INF)["x"]))
    x = po.planes_run(kind, hpo.QUIET)["x"]
    assert po.share_small_weights([orc.diff_r(x[None]), orc.diff_c(x[None])], po.PLANES["delta"], kind) == 0.0
    rc = ro.config1_case()
    x = po.robust_run(kind)["x"]
    _check(f"data term {kind}", po.share_small_weights([ro.residual(rc["om"], rc["y"], x, rc["w"])], po.ROBUST["data_delta"], kind),
           po.rel(x, po.robust_run(kind, INF)["x"]))


def test_hebert_leahy_and_huber_iterates_are_far_apart_on_the_cube():
    """what tests/test_gpu_potentials.py::test_kind_reaches_the_cube_kernels relies on: 100 x the cube's solver tolerance, with room
    for the device's own distance from the oracle (under 2e-4, against the 20 % asked here)"""
    xh = po.vox_run("huber", "huber")["x"]
    far = {k: po.rel(po.vox_run(*k)["x"], xh) for k in (("hebert_leahy", "hebert_leahy"), ("hebert_leahy", "huber"), ("huber", "hebert_leahy"))}
    far["slots"] = po.rel(po.vox_run("hebert_leahy", "huber")["x"], po.vox_run("huber", "hebert_leahy")["x"])
    print(far)
    assert min(far.values()) > 1.2 * 100 * vo.X_TOL_BOUND


# ---- C ABI: slot and kind validation ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from surfh_amd import _lib
    return _lib.load()


def test_capi_rejects_unknown_slots_and_kinds(lib):
    assert hasattr(lib, "surfh_set_potential") and hasattr(lib, "surfh_get_potential")
    for slot, kind, word in ((3, 0, "slot 3"), (-1, 0, "slot -1"), (0, 3, "kind 3"), (2, -1, "kind -1"), (0, 1, "null plan")):
        assert lib.surfh_set_potential(None, slot, kind) != 0
        assert word in lib.surfh_last_error().decode(), (slot, kind, lib.surfh_last_error())
    assert lib.surfh_get_potential(None, 5) == -1 and "slot 5" in lib.surfh_last_error().decode()
    assert lib.surfh_get_potential(None, 0) == -1 and "null plan" in lib.surfh_last_error().decode()


# ---- drivers ------------------------------------------------------------------------------------------------------------------------
def test_fusion_driver_options_and_directory_names():
    mf = _script("main_fusion")
    base = ("mmmg", 1, 4, 8, 5e3, False)
    # Huber names are exactly the former ones
    assert mf.result_dir_name(*base) == "mmmg_MC_1_MO_4_Temp_4_nit_8_mu_5.00e+03_SD_False/"
    assert mf.result_dir_name(*base, 0.1) == "mmmg_MC_1_MO_4_Temp_4_nit_8_mu_5.00e+03_SD_False_huber_1.00e-01/"
    assert mf.result_dir_name(*base, 0.1, weighted=True, data_delta=3.0, potential="huber", data_potential="huber") == \
        "mmmg_MC_1_MO_4_Temp_4_nit_8_mu_5.00e+03_SD_False_huber_1.00e-01_wgt_rob_3/"
    assert mf.result_dir_name(*base, 0.1, voxel=True) == "mmmg_MC_1_MO_4_Temp_4_nit_8_mu_5.00e+03_SD_False_huber_1.00e-01_vox/"
    # the other kinds take Huber's place
    assert mf.result_dir_name(*base, 0.1, potential="hebert_leahy").endswith("_SD_False_hebert_leahy_1.00e-01/")
    assert mf.result_dir_name(*base, 0.1, data_delta=3.0, data_potential="hyperbolic").endswith("_huber_1.00e-01_rob_hyperbolic_3/")
    assert mf.result_dir_name(*base, None, data_delta=2.5, data_potential="hebert_leahy").endswith("_SD_False_rob_hebert_leahy_2.5/")
    assert mf.result_dir_name(*base, 0.1, voxel=True, potential="hyperbolic", spec_potential="hebert_leahy").endswith(
        "_hyperbolic_1.00e-01_vox_spec_hebert_leahy/")
    run = CliRunner()
    for args, word in ((["--potential", "cauchy"], "cauchy"),
                       (["-m", "lcg", "--delta", "0.1", "--potential", "hyperbolic"], "--method mmmg"),
                       (["-m", "mmmg", "--potential", "hyperbolic"], "--delta"),
                       (["-m", "mmmg", "--data_potential", "hebert_leahy"], "--data_delta"),
                       (["-m", "lcg", "--data_delta", "3", "--data_potential", "hebert_leahy"], "--method mmmg"),
                       (["-m", "mmmg", "--delta", "0.1", "--spec_potential", "hyperbolic"], "--voxel")):
        r = run.invoke(mf.main, ["--synthetic", "small"] + args)
        assert r.exit_code == 2 and word in r.output, (args, r.output)


def test_deconvolution_driver_options_and_directory_names():
    dm = _script("deconvolution_mrs")
    assert dm.result_dir("out", 0.025) == "out_huber_0.025" and dm.result_dir("out", 0.025, "huber") == "out_huber_0.025"
    assert dm.result_dir("out", 0.025, "hyperbolic") == "out_hyperbolic_0.025"
    run = CliRunner()
    r = run.invoke(dm.main, ["-m", "qmm", "--potential", "hyperbolic"])
    assert r.exit_code == 2 and "--delta" in r.output
    r = run.invoke(dm.main, ["-m", "qmm", "--delta", "0.1", "--potential", "tukey"])
    assert r.exit_code == 2 and "tukey" in r.output


# ---- Python: a potential of a quadratic term is an error ------------------------------------------------------------------------------
class _Model:
    ishape, oshape, osize, lmm = (2, 4, 4), (8,), 8, True

    def get_prior(self):
        return "separated"


def test_potential_without_its_threshold_is_a_value_error():
    from surfh_amd.algorithms import vox_criterion
    from surfh_amd.blurred2d import Blurred2D
    from surfh_amd.models import spectroSigRLSCT
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D
    y, m = np.zeros(8), _Model()
    for kw in (dict(potential="hyperbolic"), dict(data_potential="hebert_leahy"), dict(delta=0.1, data_potential="hyperbolic"),
               dict(data_delta=3.0, potential="hebert_leahy")):
        with pytest.raises(ValueError, match="needs"):
            fusion.QuadCriterion_MRS(1.0, y, m, 1.0, **kw)
        with pytest.raises(ValueError, match="needs"):
            spectroSigRLSCT.mmmg(m, y, **kw)
    with pytest.raises(ValueError, match="needs data_delta"):
        spectroSigRLSCT.mmmg_vox(m, y, data_potential="hyperbolic")
    with pytest.raises(ValueError, match="needs data_th"):
        vox_criterion(y, m, np.zeros(m.ishape), data_potential="hyperbolic")
    with pytest.raises(ValueError, match="needs delta"):
        Blurred2D.mmmg(m, y, potential="hebert_leahy")
    with pytest.raises(ValueError, match="needs delta"):
        QuadCriterion_MRS_2D(1.0, y, m, 1.0, potential="hyperbolic")
    for cls in (fusion.QuadCriterion_MRS, QuadCriterion_MRS_2D):
        with pytest.raises(ValueError, match="must be one of"):
            cls(1.0, y, m, 1.0, delta=0.1, potential="cauchy")
    q = fusion.QuadCriterion_MRS(1.0, y, m, 1.0, delta=0.1, data_delta=3.0, potential="hyperbolic", data_potential="hebert_leahy")
    assert (q.potential, q.data_potential) == ("hyperbolic", "hebert_leahy")
    assert fusion.QuadCriterion_MRS(1.0, y, m, 1.0).potential == "huber"
