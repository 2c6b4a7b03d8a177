"""The contract of the CG loop of the library (plan_solvers.hip: cg_loop, which surfh_cg_cb runs on the maps or on their scaled half
spectra and surfh_cg_planes_cb plane by plane) and of ``DistributedFusion.lcg``, the spectral loop driven from Python, on the smallest problem the
suite has for each: what max_iter = 0 returns, what the callback sees, where a callback's stop and the tolerance stop leave the
iterate, that a run is a prefix of every longer run on either side of a CG_CHECK boundary, and that a residual which is exactly
zero keeps the iterate still.  Warm starts and residual refreshes are compared with the float64 oracle (needs an MI355X).

The spectral loop reads its trace every CG_CHECK = 8 iterations when no callback is installed: a tolerance met at iteration k stops
it at the next multiple of 8 (or at max_iter), with nit, x and grad_norm those of the last iteration run.  With a callback every
loop tests after every iteration."""
import math
import os

import numpy as np
import pytest

import huber_planes_oracle as hp
import problems
from helpers import build_model, rel
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
FREE = 12                                         # iterations of the run nothing stops
CG_CHECK = 8                                      # plan_solvers.hip
STOP = 3                                          # the iteration the callback stop and the tolerance stop aim at


def _noisy(y):
    return y + np.random.default_rng(1).standard_normal(y.shape) * 1e-2 * np.sqrt(np.mean(y ** 2))


def _map_start(shape):
    return 0.5 + 0.25 * (np.random.default_rng(5).random(shape) - 0.5)


def _maps(cfg, spectral):
    m = build_model(cfg)
    assert m.spec_supported() == spectral
    return dict(m=m, y=_noisy(m.forward(cfg["maps"])), x0=_map_start(m.ishape), planes=1, spectral=spectral, cfg=cfg,
                kw=dict(mu=1.0, mu_reg=5e3))


def _maps_ct():
    from dist_worker import small_problem
    from surfh_amd.fusion import DistributedFusion
    prob = small_problem(300)
    fus = DistributedFusion(prob, rank=0, world=1, device=0)
    m = fus.model
    assert fus.spec and m.spec_supported()
    return dict(m=m, y=fus.make_data(prob["maps"]).cpu().numpy().astype(np.float64), x0=_map_start(m.ishape), planes=1, spectral=True,
                prob=prob, fus=fus, kw=dict(mu=1.0, mu_reg=50.0))


def _planes():
    from test_gpu_huber_planes import _plane_model
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    x0 = 0.5 * np.asarray(hp.AMPL)[:, None, None] * np.ones((hp.L, hp.N, hp.N))
    x0[hp.EMPTY] = 0.0                                     # as hp.problem() starts the plane without data
    return dict(m=m, y=hp.problem()[2], x0=x0, planes=hp.L, spectral=False, empty=hp.EMPTY, kw=dict(mu=hp.MU, mu_reg=hp.MUR))


ENTRIES = {"maps, map domain": lambda: _maps(problems.config1(), False),
           "maps, spectral h2": lambda: _maps(problems.two_channel_mid(), True),
           "maps, spectral ct": _maps_ct,
           "planes": _planes}
MAPS = list(ENTRIES)[:3]                                   # the entries with a reference for warm starts and refreshes
ORACLE = MAPS[:2]                                          # ... against the float64 oracle; the third against the map-domain loop


@pytest.fixture(scope="module", params=list(ENTRIES))
def entry(request):
    """The model, its data and start, ``solve(x0=, max_iter=, ...)``, and the run of FREE iterations from the start with what its
    callback saw: (it, length of the trace, |A x|^2 computed on the same model, x)."""
    e = ENTRIES[request.param]()
    m = e["m"]
    e["name"] = request.param
    e["solve"] = lambda **a: m.cg(e["y"], **{**e["kw"], **a})
    e["scale"] = e["x0"].size // e["planes"]
    seen = []

    def record(it, g, x):
        seen.append((it, g.shape[0], float(np.sum(m.forward(x) ** 2)), x.copy()))
        return False

    try:
        e["free"] = e["solve"](x0=e["x0"], max_iter=FREE, tol=0.0, callback=record)
        e["seen"] = seen
        print(f"{request.param}: nit {e['free'][2]}, r.r {_worst(e['free'][1])}")
        yield e
    finally:
        m.close()


def _worst(gn):
    """the largest r.r over the planes, per iteration: what the stopping test of every loop reads"""
    return np.asarray(gn).reshape(len(gn), -1).max(axis=1)


def _never(*a):
    raise AssertionError("the callback ran")


def _first_below(trace, bound):
    return int(np.argmax(np.sqrt(trace) < bound))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_no_iteration_returns_the_start(entry):
    solve, x0 = entry["solve"], entry["x0"]
    x, gn, nit = solve(x0=None, max_iter=0, callback=_never)
    assert nit == 0 and gn.shape[0] == 1 and np.array_equal(x, np.zeros(x0.shape))
    want = x0.astype(np.float32).astype(np.float64)
    x, gn, nit = solve(x0=x0, max_iter=0, callback=_never)
    assert nit == 0 and gn.shape[0] == 1
    if entry["spectral"]:                                  # the start went to the spectra and came back
        print(f"{entry['name']}: start through to_spec / from_spec {rel(x, want):.2e}")
        assert rel(x, want) < 2e-6
    else:
        assert np.array_equal(x, want)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_callback_sees_every_iterate_and_does_not_disturb(entry):
    (x, gn, nit), seen = entry["free"], entry["seen"]
    assert nit == FREE and gn.shape[0] == nit + 1
    assert [(s[0], s[1]) for s in seen] == [(it, it + 1) for it in range(1, nit + 1)]
    assert all(np.isfinite(s[2]) for s in seen)
    xq, gq, nq = entry["solve"](x0=entry["x0"], max_iter=FREE, tol=0.0)
    assert nq == nit and np.array_equal(gq, gn) and np.array_equal(xq, x)
    assert np.array_equal(seen[-1][3], x)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_callback_stop_leaves_the_iterate_of_that_iteration(entry):
    solve, x0, (_, gn, _), seen = entry["solve"], entry["x0"], entry["free"], entry["seen"]
    xs, gs, ns = solve(x0=x0, max_iter=FREE, tol=0.0, callback=lambda it, g, xx: it == STOP)
    x3, g3, n3 = solve(x0=x0, max_iter=STOP, tol=0.0)
    assert ns == STOP and n3 == STOP
    assert np.array_equal(gs, gn[:STOP + 1]) and np.array_equal(g3, gn[:STOP + 1])
    assert np.array_equal(xs, seen[STOP - 1][3]) and np.array_equal(xs, x3)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", (5, CG_CHECK, CG_CHECK + 1))
def test_a_run_is_a_prefix_of_the_free_run(entry, max_iter):
    (_, gn, _), seen = entry["free"], entry["seen"]
    x, g, n = entry["solve"](x0=entry["x0"], max_iter=max_iter, tol=0.0)
    assert n == max_iter and np.array_equal(g, gn[:max_iter + 1]) and np.array_equal(x, seen[max_iter - 1][3])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_tolerance_stop(entry):
    """tol just above entry STOP of the free run's trace.  With a callback, and in the map-domain and plane-wise loops, the run stops
    at the first iteration k below it; the spectral loop without a callback at the first check at or after k."""
    solve, x0, (_, gn, _), seen = entry["solve"], entry["x0"], entry["free"], entry["seen"]
    worst, scale = _worst(gn), entry["scale"]
    tol = math.sqrt(worst[STOP]) * 1.0001 / scale
    k = _first_below(worst, scale * tol)
    late = min(FREE, CG_CHECK * math.ceil(k / CG_CHECK))
    print(f"{entry['name']}: r.r {worst}, tolerance met first at {k}, next check at {late}")
    assert 1 <= k <= 7                                    # the precondition: iterations run, and the next check lies past k
    for cb, want in ((lambda it, g, xx: False, k), (None, late if entry["spectral"] else k)):
        xt, gt, nt = solve(x0=x0, max_iter=FREE, tol=tol, callback=cb)
        assert nt == want, (nt, want)
        assert np.array_equal(gt, gn[:nt + 1]) and np.array_equal(xt, seen[nt - 1][3])


def test_tolerance_stop_of_the_python_loop():
    """``DistributedFusion.lcg``, the spectral loop driven from Python: check_every = 1 stops where the tolerance is met, check_every
    = 8 at the next multiple of 8."""
    from dist_worker import small_problem
    from surfh_amd.fusion import DistributedFusion
    prob = small_problem(128)
    fus = DistributedFusion(prob, rank=0, world=1, device=0)
    try:
        assert fus.spec
        y = fus.make_data(prob["maps"])
        free = fus.lcg(y, mu=1.0, mu_reg=50.0, max_iter=FREE, tol=0.0, check_every=100)
        gn = np.asarray(free.grad_norm)
        assert free.nit == FREE and gn.shape[0] == FREE + 1 and not free.success
        tol = math.sqrt(gn[STOP]) * 1.0001 / fus.n
        k = _first_below(gn, fus.n * tol)
        late = min(FREE, CG_CHECK * math.ceil(k / CG_CHECK))
        print(f"lcg: r.r {gn}, tolerance met first at {k}, next check at {late}")
        assert 1 <= k <= 7
        for every, want in ((1, k), (CG_CHECK, late)):
            res = fus.lcg(y, mu=1.0, mu_reg=50.0, max_iter=FREE, tol=tol, check_every=every)
            assert res.nit == want and res.success, (every, res.nit, want)
            assert np.array_equal(np.asarray(res.grad_norm), gn[:want + 1])
        assert np.array_equal(fus.lcg(y, mu=1.0, mu_reg=50.0, max_iter=late, tol=0.0, check_every=100).x, res.x)
    finally:
        fus.model.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refresh", (50, 0))
@pytest.mark.parametrize("case", ("no data", "no weight"))
def test_zero_residual_keeps_still(entry, case, refresh):
    """b = mu A^T W y = 0 from x0 = None: r.r = d.q = 0 in every iteration.  The step is then 0, not 0/0: x stays 0 and the trace
    holds zeros.  The tolerance test (0 < n tol) is met at the first check: after iteration 1, or, in the spectral loop without a
    callback, only at max_iter = 3.  refresh = 50 takes the refresh branch in iteration 0, refresh = 0 never."""
    m, y = entry["m"], entry["y"]
    if case == "no data":
        a = dict(data=np.zeros(y.shape))
    else:
        a = dict(data=np.random.default_rng(3).standard_normal(y.shape), weights=np.zeros(y.shape))
    for cb, want in ((None, 3 if entry["spectral"] else 1), (lambda it, g, xx: False, 1)):
        x, gn, nit = m.cg(a["data"], **entry["kw"], x0=None, max_iter=3, refresh=refresh, callback=cb, weights=a.get("weights"))
        print(f"{entry['name']}, {case}, refresh {refresh}, callback {cb is not None}: nit {nit}, r.r {gn.ravel()}, "
              f"x finite {np.isfinite(x).all()}, max |x| {np.abs(x).max()}")
        assert np.isfinite(gn).all() and np.array_equal(gn, np.zeros(gn.shape))
        assert np.array_equal(x, np.zeros(x.shape))
        assert nit == want and gn.shape[0] == nit + 1


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_free_run_is_finite_and_a_plane_without_data_keeps_still(entry):
    """hp.problem() holds a plane without data that starts from 0: its r.r is 0 from the first entry on, and it must come back as
    exact zeros beside planes that moved.  Every entry: nothing in the result or the trace is NaN or infinite."""
    x, gn, nit = entry["free"]
    assert np.isfinite(x).all() and np.isfinite(gn).all()
    if "empty" in entry:
        l = entry["empty"]
        assert np.array_equal(x[l], np.zeros(x[l].shape)) and np.array_equal(gn[:, l], np.zeros(nit + 1))
        assert all(np.abs(x[j]).max() > 0 and gn[0, j] > 0 for j in range(entry["planes"]) if j != l)


# ---- 8, 9 ---------------------------------------------------------------------------------------------------------------------------
def _cases(shape):
    """name -> the arguments of the run: warm starts over 9 iterations, refresh periods over 10 from x0 = None"""
    c = {"warm flat": dict(x0=np.full(shape, 0.5), max_iter=9), "warm random": dict(x0=np.random.default_rng(11).random(shape), max_iter=9)}
    c.update({f"refresh {r}": dict(x0=None, max_iter=10, refresh=r) for r in (0, 1, 3)})
    return c


@pytest.fixture(scope="module")
def refs(entry):
    """The reference runs of the entry's problem, each computed once: name -> (x, r.r trace).  The float64 oracle's lcg where
    tests/problems.py has the problem; for the Cooley-Tukey entry the map-domain loop of a second model (SURFH_SPECTRAL_CG=0)."""
    cases = _cases(entry["x0"].shape)
    if entry["name"] in ORACLE:
        om = problems.oracle_model(entry["cfg"], box="direct")

        def run(a):
            r = orc.lcg(om, entry["y"], 1.0, 5e3, np.zeros(om.ishape) if a["x0"] is None else a["x0"], tol=1e-12, max_iter=a["max_iter"],
                        refresh=a.get("refresh", 50))
            assert r["nit"] == a["max_iter"]
            return r["x"], np.asarray(r["grad_norm"])

        return {n: run(a) for n, a in cases.items()}
    from surfh_amd.fusion import DistributedFusion
    saved = os.environ.get("SURFH_SPECTRAL_CG")
    os.environ["SURFH_SPECTRAL_CG"] = "0"
    try:
        ref = DistributedFusion(entry["prob"], rank=0, world=1, device=0)
        try:
            assert not ref.spec
            return {n: ref.model.cg(entry["y"], **entry["kw"], tol=1e-12, **a)[:2] for n, a in cases.items()}
        finally:
            ref.model.close()
    finally:
        if saved is None:
            del os.environ["SURFH_SPECTRAL_CG"]
        else:
            os.environ["SURFH_SPECTRAL_CG"] = saved


def _against_reference(entry, refs, name):
    """The bounds of test_gpu_parity.py::test_cg_matches_oracle_lcg against the oracle (the first ten r.r within 2e-4, x within
    3e-3); against the map-domain loop those of test_gpu_spectral.py on the same problem (the first four r.r within 1e-4, x within
    5e-3: two fp32 loops of a badly conditioned system separate from there on)."""
    a = _cases(entry["x0"].shape)[name]
    x, gn, nit = entry["solve"](tol=1e-12, **a)
    xr, gr = refs[name]
    assert nit == a["max_iter"] and gn.shape == gr.shape
    e_g, e_x = np.abs(gn - gr) / gr, rel(x, xr)
    print(f"{entry['name']}, {name}: r.r against the reference", " ".join(f"{v:.1e}" for v in e_g), f"; x within {e_x:.2e}")
    if entry["name"] in ORACLE:
        assert np.max(e_g[:10]) < 2e-4 and e_x < 3e-3
    else:
        assert np.max(e_g[:4]) < 1e-4 and e_x < 5e-3


@pytest.mark.parametrize("entry", MAPS, indirect=True)
@pytest.mark.parametrize("start", ("flat", "random"))
def test_warm_start_matches_reference(entry, refs, start):
    _against_reference(entry, refs, f"warm {start}")


@pytest.mark.parametrize("entry", MAPS, indirect=True)
@pytest.mark.parametrize("refresh", (0, 1, 3))
def test_refresh_matches_reference(entry, refs, refresh):
    _against_reference(entry, refs, f"refresh {refresh}")
