"""The contract of the frame all seven 3MG entry points of the library stand on (plan_solvers.hip: mmmg_begin, mmmg_check, mmmg_finish),
on the smallest problem the suite has for each: what max_iter = 0 returns, what the callback sees, where a callback's stop and
the tolerance stop leave the iterate.  What the solvers compute is pinned by their own test files (needs an MI355X).

3MG lowers the criterion, not the gradient norm, at every step: from a start near the truth the norm of the map and plane solvers
rises before it falls, and a tolerance just above trace entry 2 is then met earlier.  These solvers therefore start from a flat
0.5, as test_gpu_driver.py's tolerance stop does; the float64 oracles give, for entries 0..2 of the largest norm, maps
2.1e7, 4.5e6, 9.5e5 (both priors), planes 1.5e3, 3.0e2, 1.1e2 (both priors), vox 209, 188, 168, robust maps 5.0e3, 1.9e3, 9.8e2,
robust vox 2.2e3, 2.0e3, 1.8e3."""
import numpy as np
import pytest

import huber_oracle as ho
import huber_planes_oracle as hp
import robust_oracle as ro
import vox_oracle as vo
from helpers import build_model
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
FREE = 4                                          # iterations of the run nothing stops


def _maps(**kw):
    om, _, y = ho.small_problem()
    m = build_model(dict(vo.small_cfg()[0], templates=orc.synthetic_templates(32)))       # the geometry of ho.small_problem
    return m, np.full(om.ishape, 0.5), 1, lambda **a: m.mmmg(y, mu=1.0, mu_reg=5e3, **kw, **a)


def _vox():
    cfg, om, cube, y = vo.small_cfg()
    m = build_model(cfg)
    sr, sd, lr, ld = vo.REGIMES["both"][:4]
    return m, vo.start("rough", om, cube), 1, lambda **a: m.mmmg_vox(y, mu=1.0, spat_reg=sr, spat_delta=sd, spec_reg=lr, spec_delta=ld, **a)


def _robust_maps():
    c = ro.config1_case()
    m = build_model(c["cfg"])
    return m, c["starts"]["huber"], 1, lambda **a: m.mmmg(c["y"], mu=1.0, mu_reg=c["mur"], delta=ro.C1_REGIMES["huber"][0],
                                                         weights=c["w"], data_delta=ro.DATA_DELTA, **a)


def _robust_vox():
    c = ro.vox_case()
    m = build_model(c["cfg"])
    sr, sd, lr, ld = ro.VOX_REGIME[:4]
    return m, c["x0"], 1, lambda **a: m.mmmg_vox(c["y"], mu=1.0, spat_reg=sr * c["scale"], spat_delta=sd, spec_reg=lr * c["scale"],
                                                spec_delta=ld, weights=c["w"], data_delta=ro.DATA_DELTA, **a)


def _planes(**kw):
    from test_gpu_huber_planes import _plane_model
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    y = hp.problem()[2]
    x0 = 0.5 * np.asarray(hp.AMPL)[:, None, None] * np.ones((hp.L, hp.N, hp.N))
    x0[hp.EMPTY] = 0.0                                     # as hp.problem() starts the plane without data
    return m, x0, hp.L, lambda **a: m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, **kw, **a)


ENTRIES = {"maps quadratic": _maps, "maps Huber": lambda: _maps(delta=0.1), "vox": _vox, "robust maps": _robust_maps,
           "robust vox": _robust_vox, "planes quadratic": _planes, "planes Huber": lambda: _planes(delta=hp.DELTA)}


@pytest.fixture(scope="module", params=list(ENTRIES))
def entry(request):
    """(solve(x0=, max_iter=, ...), start, planes, the run of FREE iterations with what its callback saw)"""
    m, x0, planes, solve = ENTRIES[request.param]()
    seen = []
    free = solve(x0=x0, max_iter=FREE, callback=lambda it, g, xx: seen.append((it, g.shape[0])) and False)
    print(f"{request.param}: nit {free[2]}, grad_norm {free[1].reshape(free[2] + 1, -1).max(axis=1)}")
    yield solve, x0, planes, free, seen
    m.close()


def _never(*a):
    raise AssertionError("the callback ran")


def test_no_iteration_returns_the_start(entry):
    solve, x0, planes, _, _ = entry
    for start, want in ((x0, x0.astype(np.float32).astype(np.float64)), (None, np.zeros(x0.shape))):
        x, gn, nit = solve(x0=start, max_iter=0, callback=_never)
        assert nit == 0 and gn.shape[0] == 1 and np.array_equal(x, want)


def test_callback_sees_every_iterate_in_order(entry):
    _, _, _, (x, gn, nit), seen = entry
    assert nit >= 1 and seen == [(it, it + 1) for it in range(1, nit + 1)] and gn.shape[0] == nit + 1


def test_callback_stop_leaves_the_iterate_of_that_iteration(entry):
    solve, x0, _, _, _ = entry
    xs, gs, ns = solve(x0=x0, max_iter=FREE, callback=lambda it, g, xx: it == 2)
    x2, g2, n2 = solve(x0=x0, max_iter=2)
    assert ns == 2 and n2 == 2 and np.array_equal(xs, x2) and np.array_equal(gs, g2)


def test_tolerance_stop(entry):
    """tol just above trace entry 2 of the free run: the scale is the number of unknowns for the map and cube solvers, the
    pixels of one plane with the largest norm over the planes for the plane solvers."""
    solve, x0, planes, (x, gn, nit), _ = entry
    worst = gn.reshape(nit + 1, -1).max(axis=1)
    scale = x.size // planes
    xt, gt, nt = solve(x0=x0, max_iter=FREE, tol=worst[2] * 1.0001 / scale)
    print(f"worst norms {worst}, stopped at {nt}")
    assert nt == 2 and np.array_equal(gt, gn[:3])
