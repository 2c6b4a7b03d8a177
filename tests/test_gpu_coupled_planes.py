"""The plane-wise prior coupling and the per-plane mu_reg / delta on the device (surfh_mmmg_huber_planes_ex and the _ex passes):
the two passes of ``huber_dir_planes_kernel`` under COUPLING 1 against the float64 restatement of tests/coupled_oracle.py,
``MRSBlurred.mmmg(delta=, coupling="isotropic")`` against tests/coupled_planes_oracle.py (whose preconditions
tests/test_coupled_planes_host.py asserts without a GPU), and the per-plane parameters bit for bit.  Needs an MI355X.

Kernel bound: ten times the relative error of the unchanged coupling-0 ``huber`` gradient output on the same arrays, measured in
the same test -- the rule of tests/test_gpu_coupled.py.  The coupled passes add a float64 square root, a division and two products
per difference, a few ulp each.  A slit geometry cannot give a plan an axis of length 1 or 2, so every kernel shape goes through
``planes_passes_dev``, the same launchers on explicit extents; the 2 x 72 x 77 case asserts that the plan's own passes give the
same bits.  Where that reference error is exactly 0 (1 x 1 x 1: every difference is 0) the outputs must be exact as well.

Solver bounds: hp.TOL_X in x and hp.TOL_G in |g|, the project's own plane-wise bounds (tests/huber_planes_oracle.py)."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

import coupled_oracle as co
import coupled_planes_oracle as cp
import huber_planes_oracle as hp
import problems
from capped_cases import COEF, DELTA, TINY
from capped_cases import curv_err as _curv_err
from capped_cases import pot_arrays as _arrays
from capped_cases import spat_want as _spat_want
from helpers import rel
from oracle import surfh_oracle as orc
from surfh_amd import potentials as P
from test_gpu_huber_planes import _plane_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = list(P.NAMES)
ISO = DELTA * np.sqrt(2.0)                   # the threshold on the group magnitude that behaves like DELTA on one difference


def _dev(*arrays):
    import torch
    out = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def _per_plane(v, L):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (L,))


def _want(x, g0, p0, p1, coef, delta, kind, coupling):
    """float64, plane by plane (``coef`` and ``delta`` numbers or [L]): g0 + coef_l sum_k D_k^T (w D_k x_l), the prior values [L],
    the curvature blocks [L, 3]"""
    L = x.shape[0]
    coef, delta = _per_plane(coef, L), _per_plane(delta, L)
    grad, val, curv = np.empty(x.shape), np.empty(L), np.empty((L, 3))
    for l in range(L):
        s = slice(l, l + 1)
        if coupling == "none":
            g, v, c = _spat_want(x[s], g0[s], p0[s], p1[s], coef[l], delta[l], kind)
            grad[s], val[l], curv[l] = g, v[0], c[0]
            continue
        x64, a, b = (v[s].astype(np.float64) for v in (x, p0, p1))
        w = co.group_weight(x64, delta[l], coupling, kind)
        grad[s] = g0[s].astype(np.float64) + coef[l] * co.prior_grad(x64, delta[l], coupling, kind)
        val[l] = co.prior_value(x64, delta[l], coupling, kind)
        curv[l] = [sum(np.sum(w * d(u) * d(v)) for d in (orc.diff_r, orc.diff_c)) for u, v in ((a, a), (a, b), (b, b))]
    return grad, val, curv


def _hook(m, kind, coupling, x, g0, p0, p1, coef, delta):
    """the two passes on the arrays' own extents: (g, g.g [L], values [L], blocks [L, 3])"""
    x_t, g_t, p0_t, p1_t = _dev(x, g0, p0, p1)
    gg, val, curv = m.planes_passes_dev(x_t, g_t, p0_t, p1_t, coef, delta, kind, coupling)
    out = g_t.cpu().numpy()
    want_gg = np.sum(out.astype(np.float64) ** 2, axis=(1, 2))
    assert np.all(np.abs(gg - want_gg) <= 1e-12 * want_gg)
    return out, val, curv


def _plan(m, kind, coupling, x, g0, p0, p1, coef, delta):
    """huber_planes_prior_dev / huber_planes_curv_dev under the plan's kind and the call's coupling"""
    x_t, g_t, p0_t, p1_t = _dev(x, g0, p0, p1)
    with P.installed(m, spatial=kind):
        _, val = m.huber_planes_prior_dev(x_t, g_t, coef, delta, coupling=coupling)
        curv = m.huber_planes_curv_dev(x_t, p0_t, p1_t, delta, coupling=coupling)
    return g_t.cpu().numpy(), val, curv


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _errs(got, want):
    """the worst plane of every measure"""
    (out, val, curv), (wg, wv, wc) = got, want
    assert np.isfinite(out).all() and np.isfinite(val).all() and np.isfinite(curv).all()
    phi = max(abs(v - w) / w if w > 0 else abs(v) for v, w in zip(val, wv))
    ce = max(_curv_err(c, w) if np.max(np.abs(w)) > 0 else float(np.max(np.abs(c))) for c, w in zip(curv, wc))
    return dict(grad=rel(out, wg) if np.any(wg) else float(np.max(np.abs(out))), phi=float(phi), curv=float(ce))


def _under(e, bound):
    """under the bound; where the reference error is exactly 0 the outputs are exact too"""
    worst = max(e.values())
    return worst < bound or (bound == 0.0 and worst == 0.0)


def _check_shape(m, shape, seed):
    """the 3 kinds under coupling 1 within ten times the error of the none / huber gradient on the same arrays; repeated calls
    give the same bits; delta = +inf is the quadratic prior within the same bound"""
    x, g0, p0, p1, _ = _arrays(shape, seed)
    ref = _errs(_hook(m, "huber", "none", x, g0, p0, p1, COEF, DELTA), _want(x, g0, p0, p1, COEF, DELTA, "huber", "none"))
    bound = 10 * ref["grad"]
    print(f"planes {shape}: none / huber {ref}, bound {bound:.2e}")
    assert bound < 1e-5 and (bound > 1e-9 or shape == (1, 1, 1))
    for kind in KINDS:
        got = _hook(m, kind, "isotropic", x, g0, p0, p1, COEF, ISO)
        e = _errs(got, _want(x, g0, p0, p1, COEF, ISO, kind, "isotropic"))
        print(f"planes {shape} {kind} isotropic:", e)
        assert _under(e, bound), (shape, kind, e, bound)
        assert _same(got, _hook(m, kind, "isotropic", x, g0, p0, p1, COEF, ISO))               # fixed-order sums: the same bits
    quad = _want(x, g0, p0, p1, COEF, float("inf"), "huber", "none")
    for kind in KINDS:
        e = _errs(_hook(m, kind, "isotropic", x, g0, p0, p1, COEF, float("inf")), quad)
        assert _under(e, bound), (shape, kind, "delta = inf", e, bound)
    return bound


@pytest.fixture(scope="module")
def host():
    wav = np.linspace(7.0, 8.2, 2)
    m = _plane_model(orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (72, 77)), 72, 77)
    assert m.ishape == (2, 72, 77) and m.get_prior_coupling() == "none"
    yield m
    m.close()


@pytest.mark.parametrize("L", [1, 2, 5])
def test_plane_kernels_match_numpy(host, L):
    """72 x 77: Na != Nb, an odd width that is no multiple of 64, 22 trips of the block over a plane; L = 1, 2, 5 workgroups"""
    shape = (L, 72, 77)
    bound = _check_shape(host, shape, 10 + L)
    x, g0, p0, p1, _ = _arrays(shape, 10 + L)
    if L == 2:            # the plan's own passes are the hook's, under both couplings; "none" with numbers is the scalar entry point
        for coupling, d in (("none", DELTA), ("isotropic", ISO)):
            assert _same(_plan(host, "hyperbolic", coupling, x, g0, p0, p1, COEF, d), _hook(host, "hyperbolic", coupling, x, g0, p0, p1, COEF, d))
            assert _same(_plan(host, "hyperbolic", coupling, x, g0, p0, p1, [COEF] * 2, [d] * 2),
                         _hook(host, "hyperbolic", coupling, x, g0, p0, p1, COEF, d))
        assert host.get_prior_coupling() == "none" and host.get_potential("spatial") == "huber"
    if L == 5:            # every plane its own coefficient and threshold, against float64 and against the runs on one plane's numbers
        coef, delta = COEF * np.array([1.0, 0.5, 2.0, 0.0, 3.0]), ISO * np.array([1.0, 0.5, 2.0, 1.5, np.inf])
        for coupling in ("none", "isotropic"):
            got = _hook(host, "huber", coupling, x, g0, p0, p1, coef, delta)
            e = _errs(got, _want(x, g0, p0, p1, coef, delta, "huber", coupling))
            print(f"per-plane parameters, {coupling}:", e)
            assert _under(e, bound), (coupling, e, bound)
            for l in range(L):
                one = _hook(host, "huber", coupling, x, g0, p0, p1, coef[l], delta[l])
                assert np.array_equal(one[0][l], got[0][l]) and one[1][l] == got[1][l] and np.array_equal(one[2][l], got[2][l])


@pytest.mark.parametrize("shape", [(2, 1, 7), (2, 7, 1), (2, 2, 2), (2, 3, 300), (1, 1, 1)])
def test_plane_kernels_match_numpy_smallest_shapes(host, shape):
    """an axis of length 1 (the circular neighbour is the pixel itself: every difference along it is 0, and the diagonal points
    of the 7-point stencil fall on the row or column neighbours), 2 x 2 (the predecessor and the successor are the same pixel), a
    row longer than the block (the walk's row step is 0), one pixel"""
    _check_shape(host, shape, 60 + sum(shape))


def test_overflow_arrays_stay_finite(host):
    """piecewise-constant planes with jumps of ~1e5 under delta = 1e-20: m / delta ~ 1e25, t^2 overflows fp32"""
    _, g0, p0, p1, xo = _arrays(host.ishape, 12)
    for kind in KINDS:
        out, val, curv = _hook(host, kind, "isotropic", xo, g0, p0, p1, 1.0 / TINY, TINY)
        assert np.isfinite(out).all() and np.isfinite(val).all() and np.isfinite(curv).all(), kind
        wg, wv, wc = _want(xo, g0, p0, p1, 1.0 / TINY, TINY, kind, "isotropic")
        print(f"overflow {kind}: grad {rel(out, wg):.2e}, phi {np.max(np.abs(val - wv) / wv):.2e}")


def test_argument_rules_of_the_library(host):
    import ctypes as C
    from surfh_amd import _lib
    L, plan = host._L, host._plan
    x, g0, p0, p1, _ = _arrays(host.ishape, 5)
    x_t, g_t, p0_t, p1_t = _dev(x, g0, p0, p1)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ok, out = np.array([1.0, 0.3]), np.zeros((5, 2))
    err = lambda: L.surfh_last_error().decode()  # noqa: E731
    assert L.surfh_debug_planes_passes(plan, 2, 72, 77, 0, 2, ptr(x_t), ptr(g_t), ptr(p0_t), ptr(p1_t), _lib.dptr(ok), _lib.dptr(ok), _lib.dptr(out)) != 0
    assert "vector" in err()
    assert L.surfh_huber_planes_prior_dev_ex(plan, ptr(x_t), ptr(g_t), _lib.dptr(ok), _lib.dptr(ok), 2, None, None) != 0 and "vector" in err()
    assert L.surfh_huber_planes_curv_dev_ex(plan, ptr(x_t), ptr(p0_t), ptr(p1_t), _lib.dptr(ok), 3, _lib.dptr(out)) != 0 and "coupling 3" in err()
    for bad in (0.0, -1.0, float("nan"), 1e-40):
        d = np.array([0.3, bad])
        assert L.surfh_huber_planes_prior_dev_ex(plan, ptr(x_t), ptr(g_t), _lib.dptr(ok), _lib.dptr(d), 1, None, None) != 0 and "delta" in err()
    with pytest.raises(RuntimeError, match="delta"):                              # positive, but it does not survive the fp32 kernels
        host.mmmg(np.zeros(host.oshape), mu_reg=1.0, delta=[0.3, 1e-40], max_iter=1)
    r = np.array([1.0, -1.0])
    assert L.surfh_huber_planes_prior_dev_ex(plan, ptr(x_t), ptr(g_t), _lib.dptr(r), _lib.dptr(ok), 0, None, None) != 0 and "mu_reg[1]" in err()
    assert np.array_equal(g_t.cpu().numpy(), g0)                                 # a refused call touches nothing
    # the plan's slot stays the maps': the coupled call is refused too while it is set, and runs once it is cleared
    y = np.zeros(host.oshape, dtype=np.float32)
    host.set_prior_coupling("isotropic")
    try:
        with pytest.raises(RuntimeError, match="coupling"):
            host.mmmg(y, mu_reg=1.0, max_iter=1, delta=0.1, coupling="isotropic")
        with pytest.raises(RuntimeError, match="coupling"):
            host.huber_planes_prior_dev(x_t, g_t, [1.0, 1.0], 0.1)
    finally:
        host.set_prior_coupling("none")
    host.mmmg(y, mu_reg=1.0, max_iter=1, delta=0.1, coupling="isotropic")
    with pytest.raises(ValueError, match="vector"):
        host.mmmg(y, mu_reg=1.0, max_iter=1, delta=0.1, coupling="vector")


# ---- the solver against the oracle ------------------------------------------------------------------------------------------------
def _max_rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


@pytest.fixture(scope="module")
def dev():
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    _, x0, y = hp.problem()
    yield m, x0, y
    m.close()


def _kw(x0, **more):
    return dict(mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=cp.DELTA, **more)


@pytest.mark.parametrize("kind", cp.KINDS)
def test_solver_matches_oracle_plane_by_plane(dev, kind):
    m, x0, y = dev
    ref = cp.reference(kind)
    xn, _, _ = m.mmmg(y, potential=kind, **_kw(x0))                                       # the device's own "none" run, same delta
    assert m.get_prior_coupling() == "none"
    x, gn, nit = m.mmmg(y, potential=kind, coupling="isotropic", **_kw(x0))
    pv = m.last_prior_values.copy()
    assert m.get_prior_coupling() == "none" and m.get_potential("spatial") == "huber"
    assert nit == hp.NIT and x.shape == (hp.L, hp.N, hp.N) and gn.shape == (hp.NIT + 1, hp.L) and pv.shape == (hp.L,)
    assert not x[hp.EMPTY].any() and not gn[:, hp.EMPTY].any() and pv[hp.EMPTY] == 0.0     # the plane without data keeps still
    assert np.isfinite(x).all() and np.isfinite(gn).all()
    for l in hp.COMPARED:
        ex, eg = rel(x[l], ref[l]["x"]), _max_rel(gn[:, l], ref[l]["grad_norm"])
        want = P.prior_value(x[l:l + 1], cp.DELTA, kind, "isotropic")
        print(f"{kind}, plane {l}: w < 0.9 for {cp.share_small_weights(x[l], kind):.0%}; device vs oracle: x {ex:.2e} (bound {hp.TOL_X:.1e}), "
              f"|g| {eg:.2e} (bound {hp.TOL_G:.1e}); prior value {abs(pv[l] - want) / want:.1e}; vs none {rel(x[l], xn[l]):.1e}")
        assert ex < hp.TOL_X and eg < hp.TOL_G, l
        assert abs(pv[l] - want) < 1e-3 * want
    for l in cp.ACTIVE:
        assert rel(x[l], xn[l]) > 20 * hp.TOL_X                                           # the coupling is in play
    # the same inputs give the same bits, and a coupled call leaves nothing behind
    x2, g2, _ = m.mmmg(y, potential=kind, coupling="isotropic", **_kw(x0))
    assert np.array_equal(x2, x) and np.array_equal(g2, gn) and np.array_equal(m.last_prior_values, pv)
    assert np.array_equal(m.mmmg(y, potential=kind, **_kw(x0))[0], xn)


def test_masked_samples_are_ignored_under_the_coupling(dev):
    m, x0, y = dev
    mask = hp.sample_mask(y.shape[1])
    w = np.tile(mask, (hp.L, 1))
    xw, gw, nw = m.mmmg(np.where(w > 0, y, np.nan), weights=w, coupling="isotropic", **_kw(x0))
    assert nw == hp.NIT and np.isfinite(xw).all() and np.isfinite(gw).all() and m.data_weights is None
    assert not xw[hp.EMPTY].any() and not gw[:, hp.EMPTY].any()
    for l in (0, hp.QUIET):
        ref = cp.solve_plane(l, y[l], x0[l], mask=mask)
        ex, eg = rel(xw[l], ref["x"]), _max_rel(gw[:, l], ref["grad_norm"])
        print(f"plane {l}, masked: x {ex:.2e}, |g| {eg:.2e}")
        assert ex < hp.TOL_X and eg < hp.TOL_G
    assert rel(xw[0], cp.reference()[0]["x"]) > 100 * hp.TOL_X                             # the mask is felt


@pytest.mark.parametrize("coupling", ["none", "isotropic"])
def test_per_plane_parameters_bit_for_bit(dev, coupling):
    """Plane l of the run on arrays is plane l of the run on the numbers delta[l], mu_reg[l]: the planes are independent and
    the sums keep a fixed order.  tol = 0: no run stops early.  Under "none" the runs on numbers take the scalar entry point."""
    m, x0, y = dev
    # plane 2 (amplitude 1e-3) gets a threshold on its own scale: on the oracle w < 0.9 then holds for 0.71 ("none") and 0.73
    # ("isotropic") of its groups after 8 iterations, against none at all under the shared threshold
    delta = cp.DELTA * np.array([1.0, 0.5, 1e-3, 2.0, 1.5])
    mu_reg = hp.MUR * np.array([1.0, 2.0, 0.5, 3.0, 0.25])
    kw = dict(mu=hp.MU, x0=x0, max_iter=hp.NIT, tol=0.0, coupling=coupling)
    x, gn, nit = m.mmmg(y, mu_reg=mu_reg, delta=delta, **kw)
    pv = m.last_prior_values.copy()
    assert nit == hp.NIT and gn.shape == (hp.NIT + 1, hp.L)
    share = cp.share_small_weights(x[hp.QUIET], delta=delta[hp.QUIET])
    assert 0.05 < share < 0.95, share                                                     # its own threshold bites in the faint plane
    for l in range(hp.L):
        xl, gl, nl = m.mmmg(y, mu_reg=float(mu_reg[l]), delta=float(delta[l]), **kw)
        assert nl == hp.NIT
        assert np.array_equal(xl[l], x[l]) and np.array_equal(gl[:, l], gn[:, l]) and m.last_prior_values[l] == pv[l], l
        others = [k for k in range(hp.L) if k not in (l, hp.EMPTY)]
        assert not any(np.array_equal(xl[k], x[k]) for k in others)                       # the other planes ran on other numbers


def test_criterion_class_and_rotated_field_model(dev):
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D
    m, x0, y = dev
    x, gn, _ = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=2, delta=cp.DELTA, coupling="isotropic")
    q = QuadCriterion_MRS_2D(hp.MU, y, m, hp.MUR, delta=cp.DELTA, coupling="isotropic")
    res = q.run_method("qmm", 2, value_init=x0)
    assert np.array_equal(res.x.reshape(x.shape), x) and q.get_crit_val(res.x) < q.get_crit_val(x0)
    want = sum(co.crit(hp.plane_op(l), y[l], x[l:l + 1], hp.MU, hp.MUR, cp.DELTA, "isotropic") for l in range(hp.L))
    assert abs(q.get_crit_val(x) - want) < 1e-5 * want
    # the rotated-field class runs the same call
    import rotated_oracle as ro
    from surfh_amd.spectro_blind import MRSBlurred
    from surfh_amd.spectro_blind import QuadCriterion_MRS_2D as Q2
    case = ro.small_case(L=3, angle=20.0)
    mr = _plane_model(case["sotf"], 96, 96, cls=MRSBlurred, spec=case["spec"], pts=case["pointings"])
    try:
        truth, x0r, _ = hp.problem()
        truth, x0r = truth[[0, 1, 4]], x0r[[0, 1, 4]]
        yr = mr.forward(truth)
        qr = Q2(hp.MU, yr, mr, hp.MUR, delta=cp.DELTA, coupling="isotropic")
        js = []
        xr, _, nit = mr.mmmg(yr, coupling="isotropic", callback=lambda it, g, xx: js.append(qr.get_crit_val(xx)) and False, **_kw(x0r))
        js = np.array([qr.get_crit_val(x0r)] + js)
        assert nit == hp.NIT and mr.last_prior_values.shape == (3,)
        assert np.all(np.diff(js) <= 1e-6 * js[:-1]) and js[-1] < 0.5 * js[0]                 # MM: non-increasing up to fp32 noise
        assert rel(xr, mr.mmmg(yr, **_kw(x0r))[0]) > 20 * hp.TOL_X
    finally:
        mr.close()


def test_driver_writes_coupled_results(tmp_path):
    sp = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    dd = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(dd)
    out = str(tmp_path / "res")
    r = CliRunner().invoke(dd.main, ["-np", "192", "--planes", "2", "-ni", "5", "-m", "qmm", "--delta", "0.05", "--coupling", "isotropic",
                                     "--quiet", "--out", out])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = out + "_huber_0.05_cpl_isotropic"
    assert os.path.isdir(d) and not os.path.exists(out) and not os.path.exists(out + "_huber_0.05")
    x, crit = np.load(os.path.join(d, "res_x.npy")), np.load(os.path.join(d, "criterion.npy"))
    assert x.shape == (2, 192, 192) and np.isfinite(x).all() and len(crit) == 2 and crit[1] < crit[0]
