"""The prior coupling on the host: the float64 restatements of surfh_amd/potentials.py, the coupled oracle of
tests/coupled_oracle.py (derivative, majorant, descent, bit identities), the preconditions of the device comparisons of
tests/test_gpu_coupled.py, the C ABI's validation and the ValueError cases of the Python interface.  No GPU."""
import sys
import os

import numpy as np
import pytest

import coupled_oracle as co
import huber_oracle as ho
import potentials_oracle as po
from surfh_amd import fusion, potentials as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
KINDS = list(P.NAMES)
CASES = [(k, c) for k in KINDS for c in co.COUPLED]


# ---- surfh_amd/potentials.py -------------------------------------------------------------------------------------------------------
def test_names_and_codes():
    assert P.COUPLINGS == {"none": 0, "isotropic": 1, "vector": 2} and P.COUPLING_NAMES == ("none", "isotropic", "vector")
    assert [P.coupling_code(c) for c in P.COUPLING_NAMES] == [0, 1, 2] and P.coupling_code(2) == 2 and P.coupling_name(1) == "isotropic"
    for bad in ("None", "tv", 3, -1, None, True, 1.0):
        with pytest.raises(ValueError):
            P.coupling_code(bad)


def test_restatements_agree_with_the_oracle():
    x = np.random.default_rng(0).standard_normal((3, 5, 6))
    m = P.group_magnitude(x, "none")
    assert m.shape == (2, 3, 5, 6)
    np.testing.assert_array_equal(m[0], np.abs(co.diffs(x)[0]))
    np.testing.assert_array_equal(m[1], np.abs(co.diffs(x)[1]))
    assert P.group_magnitude(x, "isotropic").shape == (3, 5, 6) and P.group_magnitude(x, "vector").shape == (5, 6)
    for c in co.COUPLED:
        np.testing.assert_array_equal(P.group_magnitude(x, c), co.magnitude(x, c))
        for k in KINDS:
            assert P.prior_value(x, 0.7, k, c) == co.prior_value(x, 0.7, c, k)
    for k in KINDS:        # "none" is the separated prior of the existing criterion
        want = float(fusion._phi(np.roll(x, 1, 1) - x, 0.7, k).sum() + fusion._phi(np.roll(x, 1, 2) - x, 0.7, k).sum())
        assert abs(P.prior_value(x, 0.7, k, "none") - want) <= 1e-14 * want
    with pytest.raises(ValueError):
        P.group_magnitude(x[0], "vector")


@pytest.mark.parametrize("kind,coupling", CASES)
def test_gradient_is_the_derivative_of_the_coupled_prior(kind, coupling):
    rng = np.random.default_rng(11)
    x, delta = rng.standard_normal((3, 5, 6)), 0.9
    # off Huber's kink: the central difference of the piecewise phi is not its derivative to second order across it
    assert np.min(np.abs(co.magnitude(x, coupling) - delta)) > 1e-3
    g = co.prior_grad(x, delta, coupling, kind)
    h = 1e-6
    fd = np.zeros_like(x)
    for i in np.ndindex(x.shape):
        e = np.zeros_like(x)
        e[i] = h
        fd[i] = (co.prior_value(x + e, delta, coupling, kind) - co.prior_value(x - e, delta, coupling, kind)) / (2 * h)
    # truncation h^2 |phi'''| / 6 ~ 1e-12, rounding eps J / h ~ 2.2e-16 * 100 / 1e-6 = 2e-8 on entries of order 1
    assert np.max(np.abs(fd - g)) < 1e-7 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))


@pytest.fixture(scope="module")
def small():
    om, maps, y = ho.small_problem()
    x0 = maps + 0.1 * np.random.default_rng(3).standard_normal(om.ishape)
    return om, y, x0


@pytest.mark.parametrize("kind,coupling", CASES)
def test_majorant_touches_and_dominates(small, kind, coupling):
    om, y, x0 = small
    mu, mur, delta = 1.0, 50.0, 0.1
    rng = np.random.default_rng(7)

    def quad(v):
        return mu * np.sum(om.forward(v) ** 2) + mur * co.prior_quad(x0, v, delta, coupling, kind)

    j0 = co.crit(om, y, x0, mu, mur, delta, coupling, kind)
    g = co.gradient(om, mu * om.adjoint(y), x0, mu, mur, delta, coupling, kind)
    assert quad(np.zeros_like(x0)) == 0.0                                                     # touches J at x
    for scale in (1e-3, 1e-1, 1.0, 30.0):
        v = scale * rng.standard_normal(x0.shape)
        q = j0 + np.sum(g * v) + 0.5 * quad(v)
        j = co.crit(om, y, x0 + v, mu, mur, delta, coupling, kind)
        assert q >= j * (1 - 1e-12), (scale, q, j)
    v = rng.standard_normal(x0.shape)                                                          # tangent: the gap is second order
    gaps = []
    for eps in (1e-3, 1e-4):
        q = j0 + eps * np.sum(g * v) + 0.5 * eps ** 2 * quad(v)
        gaps.append(q - co.crit(om, y, x0 + eps * v, mu, mur, delta, coupling, kind))
    assert 0 <= gaps[1] < gaps[0] * 0.02


@pytest.mark.parametrize("kind,coupling", CASES)
def test_criterion_never_increases_over_eight_iterations(small, kind, coupling):
    om, y, x0 = small
    for mur in (5e3, 50.0):
        r = co.mmmg(om, y, 1.0, mur, 0.1, x0, coupling, kind, max_iter=8)
        assert r["nit"] == 8 and len(r["crit"]) == 9 and np.all(np.diff(r["crit"]) <= 0) and r["crit"][-1] < r["crit"][0]
    r = co.mmmg_robust(om, y, 1.0, 0.02, 50.0, 0.1, x0, coupling=coupling, potential=kind, data_potential=kind, max_iter=8)
    assert r["nit"] == 8 and np.all(np.diff(r["crit"]) <= 0) and r["crit"][-1] < r["crit"][0]


def test_none_is_the_huber_oracle_bit_for_bit(small):
    om, y, x0 = small
    a, b = co.mmmg(om, y, 1.0, 50.0, 0.05, x0, "none", max_iter=4), ho.mmmg(om, y, 1.0, 50.0, 0.05, x0, max_iter=4)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]
    a, b = co.mmmg(om, y, 1.0, 50.0, 0.05, x0, 0, "hyperbolic", max_iter=3), po.mmmg(om, y, 1.0, 50.0, 0.05, x0, "hyperbolic", max_iter=3)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]
    w = np.random.default_rng(2).random(om.oshape) + 0.5
    a = co.mmmg_robust(om, y, 1.0, 0.02, 50.0, 0.05, x0, w=w, max_iter=3)
    b = po.mmmg_robust(om, y, 1.0, 0.02, 50.0, 0.05, x0, w=w, max_iter=3)
    assert np.array_equal(a["x"], b["x"]) and a["grad_norm"] == b["grad_norm"] and a["crit"] == b["crit"]


def test_one_map_makes_vector_the_same_as_isotropic():
    x = np.random.default_rng(4).standard_normal((1, 9, 7))
    for k in KINDS:
        np.testing.assert_array_equal(co.group_weight(x, 0.5, "vector", k), co.group_weight(x, 0.5, "isotropic", k))
        np.testing.assert_array_equal(co.prior_grad(x, 0.5, "vector", k), co.prior_grad(x, 0.5, "isotropic", k))
        assert co.prior_value(x, 0.5, "vector", k) == co.prior_value(x, 0.5, "isotropic", k)
        assert P.prior_value(x, 0.5, k, "vector") == P.prior_value(x, 0.5, k, "isotropic")


@pytest.mark.parametrize("kind", KINDS)
def test_infinite_delta_is_the_quadratic_run_bit_for_bit(small, kind):
    om, y, x0 = small
    q = ho.mmmg(om, y, 1.0, 50.0, INF, x0, max_iter=5)
    for c in co.COUPLED:
        a = co.mmmg(om, y, 1.0, 50.0, INF, x0, c, kind, max_iter=5)
        # every weight is exactly 1: the iterates and the gradients are the quadratic run's; the criterion sums phi over the
        # groups in another order
        assert np.array_equal(a["x"], q["x"]) and a["grad_norm"] == q["grad_norm"]
        np.testing.assert_allclose(a["crit"], q["crit"], rtol=1e-13, atol=0)
    if kind == "huber":
        a = co.mmmg(om, y, 1.0, 50.0, INF, x0, "none", kind, max_iter=5)
        assert np.array_equal(a["x"], q["x"]) and a["grad_norm"] == q["grad_norm"] and a["crit"] == q["crit"]


# ---- preconditions of the device comparisons (tests/test_gpu_coupled.py) -----------------------------------------------------------
@pytest.mark.parametrize("coupling,kind", list(co.DELTAS))
def test_gpu_comparison_preconditions(coupling, kind):
    import problems
    assert po.maps_case()["om"].ishape == problems.oracle_model(problems.config1(), box="direct").ishape
    delta = co.DELTAS[(coupling, kind)]
    r = co.maps_run(coupling, kind)
    share = co.share_small_weights(r["x"], delta, coupling, kind)
    away = co.rel(r["x"], co.maps_run("none", kind, delta)["x"])
    print(f"maps {coupling} {kind}: w < 0.9 for {share:.0%} of the groups, {away:.1e} away from the 'none' iterate")
    assert 0.05 <= share <= 0.95 and away >= 1e-2
    assert r["nit"] == co.NIT and np.all(np.diff(r["crit"]) <= 0)


def test_gpu_robust_comparison_preconditions():
    import robust_oracle as ro
    r = co.robust_run("vector")
    share = co.share_small_weights(r["x"], co.ROBUST["delta"], "vector")
    away = co.rel(r["x"], co.robust_run("none")["x"])
    print(f"robust vector: w < 0.9 for {share:.0%} of the groups, {away:.1e} away from the 'none' iterate")
    assert 0.05 <= share <= 0.95 and away >= 1e-2
    assert r["nit"] == co.NIT and np.all(np.diff(r["crit"]) <= 0) and ro.config1_case()["om"].ishape == po.maps_case()["om"].ishape


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from surfh_amd import _lib
    return _lib.load()


def test_capi_exports_and_rejects(lib):
    """the library loads without a GPU; the coupling entry points exist and fail on a NULL plan and on an unknown code"""
    import ctypes as C
    from surfh_amd import _lib
    assert {"surfh_set_prior_coupling", "surfh_get_prior_coupling"} <= set(_lib.EXPORTS)
    assert hasattr(lib, "surfh_set_prior_coupling") and hasattr(lib, "surfh_get_prior_coupling")
    for code, word in ((3, "coupling 3"), (-1, "coupling -1"), (0, "null plan"), (2, "null plan")):
        assert lib.surfh_set_prior_coupling(None, code) != 0
        assert word in lib.surfh_last_error().decode(), (code, lib.surfh_last_error())
    out = C.c_int32(7)
    assert lib.surfh_get_prior_coupling(None, C.byref(out)) != 0 and out.value == 7
    assert "null" in lib.surfh_last_error().decode()


# ---- Python interface: what is refused before any library call -------------------------------------------------------------------
def test_coupling_without_delta_is_a_value_error():
    from surfh_amd.models import spectroSigRLSCT

    class Model:
        oshape, ishape = (10,), (2, 3, 3)

    for c in co.COUPLED:
        with pytest.raises(ValueError, match="needs delta"):
            fusion.QuadCriterion_MRS(1, np.zeros(10), Model(), 1.0, coupling=c)
        with pytest.raises(ValueError, match="needs delta"):
            fusion.QuadCriterion_MRS(1, np.zeros(10), Model(), 1.0, coupling=c, data_delta=2.0)
        with pytest.raises(ValueError, match="needs delta"):
            spectroSigRLSCT.mmmg(None, np.zeros(10), coupling=c)
        with pytest.raises(ValueError, match="needs delta"):
            spectroSigRLSCT.mmmg(None, np.zeros(10), coupling=c, data_delta=2.0)
    with pytest.raises(ValueError, match="coupling must be one of"):
        fusion.QuadCriterion_MRS(1, np.zeros(10), Model(), 1.0, delta=0.1, coupling="tv")
    with pytest.raises(ValueError, match="coupling must be one of"):
        spectroSigRLSCT.mmmg(None, np.zeros(10), delta=0.1, coupling="tv")
    crit = fusion.QuadCriterion_MRS(1, np.zeros(10), Model(), 1.0, delta=0.1, coupling="vector")
    assert crit.coupling == "vector" and fusion.QuadCriterion_MRS(1, np.zeros(10), Model(), 1.0).coupling == "none"
