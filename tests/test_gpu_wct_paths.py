"""``Model_WCT.fwadj`` and ``QuadCriterion3.run_expsol`` on every transform path (needs an MI355X).

The per-frequency Hessian (wct_hessian_kernel), its application (wct_hess_apply_kernel) and the closed-form solve
(wct_solve_kernel) are held against the float64 oracle on the cases of tests/wct_cases.py: both axes on dft_h2 with the
separate reduction and with the fused adjoint tail (first and last admissible Na), one and both axes on dft_ct with and without
OTF support lists, the dense fallback with planar arrays (a prime and a short axis), 1 to 8 spectra, one to three 128-plane
chunks.  Every case asserts the path it ran on (debug accessors "dft" and "otf").  The spectra are Gaussian bumps along lambda,
so the T x T systems stay well conditioned for every T; at mu = 1e-3 the Hessian decides the solution (condition number up to
2e3), at mu = 0.7 the prior does (median condition number 1.00).  Every comparison uses the local measures of tests/helpers.py
at TOL = 1e-5 and goes to the parity log; tests/test_wct_checks_host.py shows which faults they catch.

``ct_lists`` keeps the inputs of the other cases (the noisy PSFs of test_gpu_dft.build): their OTF has a noise floor far above
2^-24 of the peak, so the plan finds no super-tile to drop and keeps no list (asserted against the plan's rule restated in
numpy).  ``ct_band_limited`` is the same shape with the clean Gaussians of ``band_limited``: there the lists drop tiles.

The singular spectra of check 5 make the system singular at the zero frequency for ANY mu: |D(0)|^2 = 0 for both priors.  The
float64 oracle returns an arbitrary mean there (sum of two spectra) or raises itself (two equal spectra), so the regular run
on those spectra adds a ridge to the prior, |D(f)|^2 + 10, passed to ``Model_WCT.expsol`` as its ``reg_freq``: the
reference-only precondition then holds (measured on the CPU: 5e-8 to 3e-7; with + 0.1 it is 2e-5 at (127, 40), with + 1 still 2e-6) and the run is held to TOL like check 3."""
import ctypes

import numpy as np
import pytest

import wct_cases as W
from helpers import TOL
from test_gpu_local_parity import check_local
from test_gpu_parity import note

pytestmark = pytest.mark.gpu

MAP_AXES = dict(template=0, alpha=1, beta=2)
HESS_AXES = dict(k_alpha=0, k_beta=1)
MUS = (0.7, W.MU_SMALL, "list")
RIDGE = W.RIDGE


def make_model(c):
    from surfh_amd.mixing import Model_WCT
    return Model_WCT(c.psfs, c.specs, c.shape, c.pce)


def debug_dims(m, which):
    d = (ctypes.c_int64 * 4)()
    assert m._L.surfh_debug_dims(m._plan, which.encode(), d) == 0
    return tuple(int(v) for v in d)


def device_hessian(m):
    """The plan's Hessian [T][T][KAP][KBP], or None while the plan has none."""
    from surfh_amd import _lib
    shape = debug_dims(m, "hth")
    out = np.empty(int(np.prod(shape)), dtype=np.float32)
    n = m._L.surfh_debug_copy(m._plan, b"hth", _lib.fptr(out), out.size)
    return out.reshape(shape) if n == out.size else None


def run_expsol(m, c, mu, gradient="separated"):
    from surfh_amd.mixing import QuadCriterion3
    mu = c.mu(mu)
    return QuadCriterion3(c.data, m, mu if np.isscalar(mu) else list(mu), gradient=gradient).run_expsol()


def check_precondition(c, mu, gradient="separated", ridge=0.0):
    pre = c.precondition(mu, gradient, ridge)
    note("wct_expsol_precondition", case=c.name, T=c.T, mu=str(mu), gradient=gradient, ridge=ridge, moved=pre)
    assert pre < TOL / 10, f"{c.name} mu={mu}: fp32 inputs alone move the float64 solve by {pre:.2e}"
    return pre


@pytest.fixture(scope="module", params=list(W.CASES))
def plan(request):
    """One plan per case for the tests that do not ask for a fresh one."""
    c = W.case(request.param)
    m = make_model(c)
    yield c, m
    m.close()


def test_path_taken(plan):
    c, m = plan
    dft, (kept, total) = debug_dims(m, "dft"), debug_dims(m, "otf")[:2]
    tiles = W.otf_tiles(c.wo.otf)
    note("wct_path", case=c.name, shape=list(c.shape), L=c.L, T=c.T, dft=list(dft), otf=[kept, total], rule=list(tiles))
    print(c.name, "dft", dft, "otf", (kept, total), "rule", tiles)
    assert dft == c.dft, (c.name, dft)
    assert total == tiles[1]
    if c.lists:
        assert 0 < kept < total and (kept, total) == tiles, (kept, total, tiles)
    else:
        assert kept == total, (kept, total)
        if c.lists is None:                                   # the plan looked for tiles to drop and the OTF has none
            assert tiles[0] == tiles[1], tiles


def test_hessian_element_by_element(plan):
    c, m = plan
    m.fwadj(c.x["uniform"])
    dev = device_hessian(m)
    Na, hb = c.shape[0], c.shape[1] // 2 + 1
    assert dev is not None and dev.shape[:2] == (c.T, c.T) and dev.shape[2] >= Na and dev.shape[3] >= hb
    assert not dev[:, :, Na:, :].any() and not dev[:, :, :, hb:].any(), "padding bins of the Hessian are not zero"
    assert np.array_equal(dev, dev.transpose(1, 0, 2, 3)), "hth[t, u] and hth[u, t] differ"
    from helpers import local_errs
    worst = {}
    for t in range(c.T):
        for u in range(c.T):
            e = local_errs(dev[t, u, :Na, :hb], c.hth[t, u], HESS_AXES)
            for k in ("rel", "max", "k_alpha", "k_beta"):
                if k not in worst or e[k] > worst[k][0]:
                    worst[k] = (e[k], [t, u], e.get(k + "_at"))
    note("wct_hessian", case=c.name, T=c.T, **{k: v[0] for k, v in worst.items()}, **{k + "_block": v[1] for k, v in worst.items()})
    print(c.name, {k: (f"{v[0]:.2e}", v[1], v[2]) for k, v in worst.items()})
    bad = [f"{k} = {v[0]:.3e} in block {v[1]} at {v[2]}" for k, v in worst.items() if not v[0] < TOL]
    assert not bad, f"{c.name}: " + "; ".join(bad)


@pytest.mark.parametrize("kind", ["uniform", "zero_mean"])
def test_fwadj(plan, kind):
    c, m = plan
    check_local("wct_fwadj", m.fwadj(c.x[kind]), c.fwadj(kind), MAP_AXES, case=c.name, x=kind)


@pytest.mark.parametrize("mu", MUS, ids=["mu_0.7", "mu_1e-3", "mu_per_map"])
def test_expsol(plan, mu):
    """Measured on an MI355X, worst local measure over the cases: 3.6e-6 at mu = 0.7, 2.2e-6 at mu = 1e-3, 2.6e-6 with the per-map mu.
    ``band_limited`` at mu = 1e-3 is the case that exposed a defect of ``surfh_wct_expsol``: with the planes' means left in the
    data, their fp32 rounding leaked into the other bins of the k_beta = 0 column of H^T y (relative error 3e-5 at k_alpha 25..30,
    where hth and mu |D|^2 are both about 1e-3 and the solve amplifies 400 times) and the worst alpha row stood at 1.096e-5
    (1.050e-5 with the per-map mu), on either form of the adjoint tail; the dense fp32 plan showed the same pattern at 3.5e-6.  The means are now taken
    out in float64 and put back into the zero-frequency bin: 1.5e-6 and 1.1e-6."""
    c, m = plan
    check_precondition(c, mu)
    check_local("wct_expsol", run_expsol(m, c, mu), c.expsol(mu), MAP_AXES, case=c.name, mu=str(mu))


@pytest.mark.parametrize("name", W.JOINT)
def test_expsol_joint_prior(name):
    c = W.case(name)
    check_precondition(c, 0.7, "joint")
    m = make_model(c)
    try:
        check_local("wct_expsol", run_expsol(m, c, 0.7, "joint"), c.expsol(0.7, "joint"), MAP_AXES, case=c.name, mu="0.7", gradient="joint")
    finally:
        m.close()


@pytest.mark.parametrize("name", list(W.CASES))
def test_state(name):
    """``mhat``, ``mhat2`` and ``hth`` are shared by the four calls and the Hessian is built by whichever of ``fwadj`` and
    ``expsol`` comes first: nothing one call leaves behind changes a bit of the next."""
    c = W.case(name)
    x = c.x["zero_mean"]
    a, b = make_model(c), make_model(c)
    try:
        assert device_hessian(a) is None                      # the accessor neither builds the Hessian nor hands out a pointer
        assert device_hessian(a) is None
        e1, f1, h1 = run_expsol(a, c, W.MU_SMALL), a.fwadj(x), device_hessian(a)
        adj, fwd = a.adjoint(c.cube), a.forward(c.maps)
        e2, f2, h2 = run_expsol(a, c, W.MU_SMALL), a.fwadj(x), device_hessian(a)
        fb, eb, hb = b.fwadj(x), run_expsol(b, c, W.MU_SMALL), device_hessian(b)
    finally:
        a.close()
        b.close()
    assert np.isfinite(adj).all() and np.isfinite(fwd).all()
    assert np.array_equal(e1, e2) and np.array_equal(f1, f2) and np.array_equal(h1, h2), "a second call differs from the first"
    assert np.array_equal(e1, eb) and np.array_equal(f1, fb) and np.array_equal(h1, hb), "expsol first and fwadj first differ"


@pytest.mark.parametrize("T8", [False, True], ids=["last_is_sum_of_first_two", "T8_two_equal"])
@pytest.mark.parametrize("name", W.SINGULAR)
def test_singular_systems(name, T8):
    from surfh_amd.mixing import QuadCriterion3
    c = W.Case(name, specs=W.two_equal, T=8) if T8 else W.Case(name, specs=W.sum_of_first_two)
    m = make_model(c)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            QuadCriterion3(c.data, m, 0.0).run_expsol()
        # the same spectra with a prior that is positive at every frequency (module docstring)
        check_precondition(c, 0.7, ridge=RIDGE)
        z = m.expsol(c.data, np.full(c.T, 0.7), c.reg(ridge=RIDGE))
        check_local("wct_expsol_singular_spectra", z, c.solve(0.7, ridge=RIDGE), MAP_AXES, case=c.name, T=c.T, mu="0.7")
    finally:
        m.close()


@pytest.mark.parametrize("name", ["h2_fused_first", "dense_short_T8"])
def test_arguments(name):
    c = W.case(name)
    m = make_model(c)
    reg = c.reg()
    try:
        for bad in (-1.0, np.nan):
            mu = np.full(c.T, 0.7)
            mu[-1] = bad
            with pytest.raises(np.linalg.LinAlgError, match="mu_reg"):
                m.expsol(c.data, mu, reg)
            r = reg.copy()
            r[-1, -1] = bad
            with pytest.raises(np.linalg.LinAlgError, match="reg_freq"):
                m.expsol(c.data, np.full(c.T, 0.7), r)
        for kind in ("uniform", "zero_mean"):                 # the plan still works
            check_local("wct_fwadj_after_refusals", m.fwadj(c.x[kind]), c.fwadj(kind), MAP_AXES, case=c.name, x=kind)
    finally:
        m.close()
