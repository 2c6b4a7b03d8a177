"""The hyperbolic and the Hebert-Leahy potential on the device (surfh_set_potential): every kernel family against the float64
restatement of surfh_amd/potentials.py, the four solvers against tests/potentials_oracle.py, slot selection, descent and the two
drivers (needs an MI355X).

Kernel bound: the relative error of the unchanged ``huber`` instantiation's gradient output on the same arrays, measured in the
same test, times 10 -- the new kinds add a division, a square root and a product per difference, a few ulp each.  The overflow
arrays (|u| / delta ~ 1e25) are held to the bound measured on the regular arrays of the same test: on them Huber's phi' is
exactly +-delta and its error 0.  They are piecewise constant with jumps of ~1e5 under delta = 1e-20, so that the sums hold
terms of weight exactly 1 beside the overflowing ones (the Hebert-Leahy weight of those is below FLT_MIN and flushes to 0)."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

import huber_planes_oracle as hpo
import potentials_oracle as po
import problems
import robust_oracle as ro
import vox_oracle as vo
from capped_cases import COEF, DELTA, HUGE, SPAT, TINY
from capped_cases import curv_err as _curv_err
from capped_cases import pot_arrays as _arrays
from capped_cases import spat_want as _spat_want
from capped_cases import spec_want as _spec_want
from helpers import build_model, make_ifu, rel
from oracle import surfh_oracle as orc
from surfh_amd import potentials as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = po.NEW_KINDS
# the arrays (DELTA, COEF, TINY, HUGE are theirs) and the float64 expectations: tests/capped_cases.py, shared with the capped-grid tests


def _dev(*arrays):
    import torch
    out = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def _max_rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def _rect_problem(na, nb, T, Lc=64):
    rng = np.random.default_rng(31)
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(0.8 / 3600, 0.9 / 3600, (0.0, 0.0), 8.2, 0.196, 4, 3050.0, np.linspace(7.53, 7.67, 40), "S1")
    return dict(N=na, Lc=Lc, alpha_axis=orc.synthetic_axes(na, problems.STEP_DEG), beta_axis=orc.synthetic_axes(nb, problems.STEP_DEG),
                wavel=wav, specs=[spec], templates=rng.random((T, Lc)) + 0.5,
                sotf=orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (na, nb)),
                pointings=[orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)], maps=rng.random((T, na, nb)),
                step_deg=problems.STEP_DEG)


def _plane_model(L, na, nb, sotf=None):
    """the batched 2-D model: a plan without templates on an [L, na, nb] cube, for the plane kernels and the cube kernels alike"""
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    s = problems.STEP_DEG
    if sotf is None:
        wav = np.linspace(7.0, 8.2, L) if L > 1 else np.array([7.6])
        sotf = orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (na, nb))
    return MRSBlurred(sotf, orc.synthetic_axes(na, s), orc.synthetic_axes(nb, s), make_ifu(hpo.SPEC), s,
                      instru.CoordList([instru.Coord(a, b) for a, b in hpo.PTS]))


# ---- maps: huber_grad_kernel, huber_curv_kernel -------------------------------------------------------------------------------------
def _maps_outputs(m, kind, x, g0, p0, p1, coef, delta):
    x_t, g_t, p0_t, p1_t = _dev(x, g0, p0, p1)
    with P.installed(m, spatial=kind):
        val = m.huber_prior_dev(x_t, g_t, coef, delta)
        curv = m.huber_curv_dev(x_t, p0_t, p1_t, delta)
    out = g_t.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(val) and np.isfinite(curv).all()
    return out, val, curv


@pytest.mark.parametrize("T", [1, 2, 5])
def test_map_kernels_match_numpy(T):
    m = build_model(_rect_problem(72, 77, T))
    try:
        assert m.ishape == (T, 72, 77) and m.get_potential("spatial") == "huber"
        x, g0, p0, p1, xo = _arrays(m.ishape, 10 + T)
        errs = {}
        for kind in P.NAMES:
            out, val, curv = _maps_outputs(m, kind, x, g0, p0, p1, COEF, DELTA)
            wg, wv, wc = _spat_want(x, g0, p0, p1, COEF, DELTA, kind)
            errs[kind] = dict(grad=rel(out, wg), phi=abs(val - wv.sum()) / wv.sum(), curv=_curv_err(curv, wc.sum(axis=0)))
        bound = 10 * errs["huber"]["grad"]
        print(f"maps {m.ishape}: bound {bound:.2e}", errs)
        assert 1e-9 < bound < 1e-5
        for kind in NEW:
            assert max(errs[kind].values()) < bound, (kind, errs[kind])
            # the overflow array: phi' scaled up by 1 / delta so that the hyperbolic +-delta shows beside g0
            out, val, curv = _maps_outputs(m, kind, xo, g0, p0, p1, 1.0 / TINY, TINY)
            wg, wv, wc = _spat_want(xo, g0, p0, p1, 1.0 / TINY, TINY, kind)
            e = dict(grad=rel(out, wg), phi=abs(val - wv.sum()) / wv.sum(), curv=_curv_err(curv, wc.sum(axis=0)))
            print(f"maps {m.ishape} {kind}, |u| / delta = 1e25:", e)
            assert max(e.values()) < bound, (kind, e)
            assert rel(out, g0) > 0.5 if kind == "hyperbolic" else rel(out, g0) < 1e-6           # +-delta / delta, or flushed
        assert m.get_potential("spatial") == "huber"
    finally:
        m.close()


# ---- planes and cube on one template-free plan ---------------------------------------------------------------------------------------
def _planes_outputs(m, kind, x, g0, p0, p1, coef, delta):
    x_t, g_t, p0_t, p1_t = _dev(x, g0, p0, p1)
    with P.installed(m, spatial=kind):
        sq, val = m.huber_planes_prior_dev(x_t, g_t, coef, delta)
        curv = m.huber_planes_curv_dev(x_t, p0_t, p1_t, delta)
    out = g_t.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(val).all() and np.isfinite(curv).all() and np.isfinite(sq).all()
    return out, sq, val, curv


def _planes_errs(got, want):
    (out, sq, val, curv), (wg, wv, wc) = got, want
    L = out.shape[0]
    return dict(grad=max(rel(out[l], wg[l]) for l in range(L)), sq=_max_rel(sq, np.sum(wg ** 2, axis=(1, 2))),
                phi=float(np.max(np.abs(val - wv) / np.maximum(wv, 1e-300))),
                curv=float(np.max(np.abs(curv - wc) / np.max(np.abs(wc), axis=1, keepdims=True))))


def _vox_outputs(m, ks, kl, x, g0, p0, p1, cs, ds, cl, dl):
    from surfh_amd.models import spectroSigRLSCT as S      # the methods need a plan only: any template-free model serves
    x_t, g_t, p0_t, p1_t = _dev(x, g0, p0, p1)
    with P.installed(m, spatial=ks, spectral=kl):
        vals = S.huber_vox_prior_dev(m, x_t, g_t, cs, ds, cl, dl)
        curv = S.huber_vox_curv_dev(m, x_t, p0_t, p1_t, ds, dl)
    out = g_t.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(vals).all() and np.isfinite(curv).all()
    return out, vals, curv


def _vox_errs(got, x, g0, p0, p1, cs, ds, cl, dl, ks, kl):
    out, vals, curv = got
    wg, wv, wc = _spat_want(x, g0, p0, p1, cs, ds, ks)
    lg, lv, lc = _spec_want(x, p0, p1, cl, dl, kl)
    e = dict(grad=rel(out, wg + lg), phi_s=abs(vals[0] - wv.sum()) / wv.sum(), curv_s=_curv_err(curv[0], wc.sum(axis=0)))
    if x.shape[0] > 1:
        e.update(phi_l=abs(vals[1] - lv) / lv, curv_l=_curv_err(curv[1], lc))
    else:
        assert vals[1] == 0.0 and not curv[1].any()
    return e


PAIRS = [(ks, kl) for ks in P.NAMES for kl in P.NAMES if (ks, kl) != ("huber", "huber")]     # the mixed pairs tell the slots apart


def _check_vox(m, seed):
    x, g0, p0, p1, xo = _arrays(m.ishape, seed)
    dl = 0.4
    e_ref = _vox_errs(_vox_outputs(m, "huber", "huber", x, g0, p0, p1, COEF, DELTA, 0.4, dl), x, g0, p0, p1, COEF, DELTA, 0.4, dl,
                      "huber", "huber")
    bound = 10 * e_ref["grad"]
    print(f"cube {tuple(m.ishape)}: huber {e_ref}, bound {bound:.2e}")
    assert 1e-9 < bound < 1e-5
    for ks, kl in PAIRS:
        e = _vox_errs(_vox_outputs(m, ks, kl, x, g0, p0, p1, COEF, DELTA, 0.4, dl), x, g0, p0, p1, COEF, DELTA, 0.4, dl, ks, kl)
        print(f"cube {tuple(m.ishape)} ({ks}, {kl}):", e)
        assert max(e.values()) < bound, (ks, kl, e)
    for ks, kl in (("hyperbolic", "hebert_leahy"), ("hebert_leahy", "hyperbolic")):
        args = (1.0 / TINY, TINY, 0.5 / TINY, TINY)
        e = _vox_errs(_vox_outputs(m, ks, kl, xo, g0, p0, p1, *args), xo, g0, p0, p1, *args, ks, kl)
        print(f"cube {tuple(m.ishape)} ({ks}, {kl}), |u| / delta = 1e25:", e)
        assert max(e.values()) < bound, (ks, kl, e)


@pytest.mark.parametrize("L", [1, 2, 5])
def test_plane_and_cube_kernels_match_numpy(L):
    m = _plane_model(L, 72, 77)
    try:
        assert tuple(m.ishape) == (L, 72, 77)
        x, g0, p0, p1, xo = _arrays(m.ishape, 20 + L, even_only=True)
        errs = {kind: _planes_errs(_planes_outputs(m, kind, x, g0, p0, p1, COEF, DELTA), _spat_want(x, g0, p0, p1, COEF, DELTA, kind))
                for kind in P.NAMES}
        bound = 10 * errs["huber"]["grad"]
        print(f"planes {L} x 72 x 77: bound {bound:.2e}", errs)
        assert 1e-9 < bound < 1e-5
        for kind in NEW:
            assert max(errs[kind].values()) < bound, (kind, errs[kind])
            # weights below 1 in the even planes only
            w = P.weight(np.concatenate([d(x.astype(np.float64)).reshape(L, -1) for d, _ in SPAT], axis=1), DELTA, kind)
            assert all((np.mean(w[l] < 0.9) > 0.3) if l % 2 == 0 else (np.min(w[l]) > 0.9) for l in range(L))
            got = _planes_outputs(m, kind, xo, g0, p0, p1, 1.0 / TINY, TINY)
            e = _planes_errs(got, _spat_want(xo, g0, p0, p1, 1.0 / TINY, TINY, kind))
            print(f"planes {L} x 72 x 77 {kind}, |u| / delta = 1e25:", e)
            assert max(e.values()) < bound, (kind, e)
        _check_vox(m, 30 + L)
        assert [m.get_potential(s) for s in P.SLOTS] == ["huber"] * 3
    finally:
        m.close()


@pytest.fixture(scope="module")
def vox():
    c = po.vox_case()
    m = build_model(c["cfg"])
    assert m.ishape == (32, 48, 48) and not m.lmm
    yield c, m
    m.close()


def test_cube_kernels_match_numpy_32_48_48(vox):
    _check_vox(vox[1], 40)


# ---- robust data term: robust_data_kernel, robust_curv_kernel -------------------------------------------------------------------------
def test_robust_kernels_match_numpy(vox):
    import torch
    m = vox[1]
    n = 5 * 256 * 4 + 3                                       # odd, no multiple of 256 (nor of 4), more than one block
    rng = np.random.default_rng(50)
    dd = 1.5
    u = rng.standard_normal(n).astype(np.float32)
    w = (rng.random(n) + 0.5).astype(np.float32)
    t = dd * np.logspace(-3, 3, n) * rng.choice([-1.0, 1.0], n)              # residuals from 1e-3 delta to 1e3 delta
    y = (u + t / np.sqrt(w.astype(np.float64))).astype(np.float32)
    masked = rng.random(n) < 0.1
    w[masked] = 0.0
    y[masked] = np.nan                                                       # weight 0 takes the sample out whatever it holds
    p0, p1 = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    yo = u.copy()                                                            # the overflow array: t = 0 but for jumps of ~1e5
    jump = rng.random(n) < 0.25
    yo[jump] += (HUGE * rng.integers(1, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)[jump]
    yo[masked] = np.nan

    def run(kind, yy, delta):
        y_t, u_t, w_t, a_t, b_t = _dev(yy, u, w, p0, p1)
        v_t = torch.empty_like(y_t)
        with P.installed(m, data=kind):
            val, beyond = m.robust_data_dev(y_t, u_t, w_t, v_t, n, delta)
            curv = m.robust_curv_dev(y_t, u_t, w_t, a_t, b_t, n, delta)
        v = v_t.cpu().numpy()
        keep = w > 0
        w64 = w.astype(np.float64)
        t64 = np.where(keep, np.sqrt(w64) * (np.where(keep, yy, 0).astype(np.float64) - u), 0.0)
        want_v = np.sqrt(w64) * P.dphi(t64, delta, kind)
        om = np.where(keep, w64 * P.weight(t64, delta, kind), 0.0)
        want_c = np.array([np.sum(om * a * b) for a, b in ((p0 * 1.0, p0), (p0 * 1.0, p1), (p1 * 1.0, p1))])
        want_val = float(np.sum(P.phi(t64, delta, kind)))
        assert np.isfinite(v).all() and not v[masked].any() and np.isfinite(curv).all() and np.isfinite(val)
        assert beyond == int(np.sum(np.abs(t64.astype(np.float32)) > np.float32(delta)))          # the samples past the knee
        return dict(v=rel(v, want_v), phi=abs(val - want_val) / want_val, curv=_curv_err(curv, want_c))

    errs = {kind: run(kind, y, dd) for kind in P.NAMES}
    bound = 10 * errs["huber"]["v"]
    print(f"robust data term, n = {n}: bound {bound:.2e}", errs)
    assert 1e-9 < bound < 1e-5
    for kind in NEW:
        assert max(errs[kind].values()) < bound, (kind, errs[kind])
        e = run(kind, yo, TINY)
        print(f"robust data term {kind}, |t| / delta = 1e25:", e)
        # v = sqrt(w) phi'(t): +-delta for the hyperbolic potential (relative error as above), below FLT_MIN for Hebert-Leahy
        assert e["phi"] < bound and e["curv"] < bound and (e["v"] < bound if kind == "hyperbolic" else True), (kind, e)
    assert m.get_potential("data") == "huber"


# ---- the solvers against the oracle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps():
    c = po.maps_case()
    m = build_model(c["cfg"])
    yield c, m
    m.close()


def _against(ref, x, gn, tol_x, tol_g, what):
    gr = np.array(ref["grad_norm"])
    ex, eg = rel(x, ref["x"]), _max_rel(gn, gr)
    print(f"{what}: device vs oracle: x {ex:.2e} (bound {tol_x:.1e}), |g| {eg:.2e} (bound {tol_g:.1e})")
    assert gn.shape == gr.shape and ex < tol_x and eg < tol_g, what


@pytest.mark.parametrize("kind", NEW)
def test_mmmg_maps_matches_oracle(maps, kind):
    c, m = maps
    x, gn, nit = m.mmmg(c["y"], mu=1.0, mu_reg=po.MAPS["mu_reg"], x0=c["x0"], max_iter=po.NIT, delta=po.MAPS["delta"], potential=kind)
    assert nit == po.NIT and m.get_potential("spatial") == "huber"
    _against(po.maps_run(kind), x, gn, 1e-4, 2e-4, f"maps, {kind}")
    d = [f(x) for f, _ in SPAT]
    want = float(sum(np.sum(P.phi(u, po.MAPS["delta"], kind)) for u in d))
    assert abs(m.huber_prior_value - want) < 1e-5 * want


@pytest.mark.parametrize("ks,kl", [("hyperbolic", "hebert_leahy"), ("hebert_leahy", "huber"), ("hyperbolic", "hyperbolic"),
                                   ("hebert_leahy", "hebert_leahy")])
def test_mmmg_vox_matches_oracle(vox, ks, kl):
    c, m = vox
    x, gn, nit = m.mmmg_vox(c["y"], mu=1.0, x0=c["x0"], max_iter=po.NIT, spat_potential=ks, spec_potential=kl, **po.VOX)
    assert nit == po.NIT and [m.get_potential(s) for s in P.SLOTS] == ["huber"] * 3
    _against(po.vox_run(ks, kl), x, gn, vo.X_TOL_BOUND, vo.G_TOL_BOUND, f"cube, ({ks}, {kl})")


@pytest.fixture(scope="module")
def planes():
    m = _plane_model(hpo.L, hpo.N, hpo.N, hpo.sotf())
    _, x0, y = hpo.problem()
    yield m, x0, y
    m.close()


@pytest.mark.parametrize("kind", NEW)
def test_mmmg_planes_matches_oracle(planes, kind):
    m, x0, y = planes
    x, gn, nit = m.mmmg(y, mu=hpo.MU, mu_reg=hpo.MUR, x0=x0, max_iter=po.NIT, delta=hpo.DELTA, potential=kind)
    assert nit == po.NIT and not x[hpo.EMPTY].any() and m.get_potential("spatial") == "huber"
    for l in hpo.COMPARED:
        _against(po.planes_run(kind, l), x[l], gn[:, l], hpo.TOL_X, hpo.TOL_G, f"plane {l}, {kind}")


@pytest.fixture(scope="module")
def robust():
    c = ro.config1_case()
    m = build_model(c["cfg"])
    yield c, m
    m.close()


@pytest.mark.parametrize("kind", NEW)
def test_mmmg_robust_matches_oracle(robust, kind):
    c, m = robust
    kw = dict(mu=1.0, mu_reg=c["mur"], x0=c["starts"]["huber"], max_iter=po.NIT, delta=po.ROBUST["delta"], weights=c["w"],
              data_delta=po.ROBUST["data_delta"])
    x, gn, nit = m.mmmg(c["y"], data_potential=kind, **kw)
    assert nit == po.NIT and m.get_potential("data") == "huber"
    _against(po.robust_run(kind), x, gn, ro.X_TOL_BOUND, ro.G_TOL_BOUND, f"data term, {kind}")
    t = ro.residual(c["om"], c["y"], x, c["w"])
    assert m.robust_n_beyond == pytest.approx(int(np.sum(np.abs(t) > po.ROBUST["data_delta"])), abs=3)
    assert rel(m.robust_weights, P.weight(t.ravel(), po.ROBUST["data_delta"], kind)) < 1e-4


# ---- selection -------------------------------------------------------------------------------------------------------------------------
def test_selection_and_plan_state(maps):
    c, m = maps
    kw = dict(mu=1.0, mu_reg=po.MAPS["mu_reg"], x0=c["x0"], max_iter=po.NIT)
    assert [m.get_potential(s) for s in P.SLOTS] == ["huber"] * 3                  # the default of a new plan
    xh, gh, _ = m.mmmg(c["y"], delta=po.MAPS["delta"], **kw)
    xe, ge, _ = m.mmmg(c["y"], delta=po.MAPS["delta"], potential="huber", **kw)
    assert np.array_equal(xh, xe) and np.array_equal(gh, ge)                       # naming the default changes no bit
    xl, _, _ = m.mmmg(c["y"], delta=po.MAPS["delta"], potential="hebert_leahy", **kw)
    assert not np.array_equal(xl, xh)            # how far apart the kind must put the iterates: test_kind_reaches_the_cube_kernels
    # a per-call potential leaves the plan's slot as it was, whatever it was
    m.set_potential("spatial", "hyperbolic")
    try:
        xp, _, _ = m.mmmg(c["y"], delta=po.MAPS["delta"], potential="hebert_leahy", **kw)
        assert m.get_potential("spatial") == "hyperbolic" and np.array_equal(xp, xl)
        # and the diagnostic passes, which take no keyword, read the plan's slot
        x_t, g_t = _dev(c["x0"], np.zeros(m.ishape))
        d = [f(c["x0"].astype(np.float32).astype(np.float64)) for f, _ in SPAT]
        want = float(sum(np.sum(P.phi(u, po.MAPS["delta"], "hyperbolic")) for u in d))
        assert abs(m.huber_prior_dev(x_t, g_t, 1.0, po.MAPS["delta"]) - want) < 1e-6 * want
    finally:
        m.set_potential("spatial", "huber")
    # hyperbolic with a huge delta is the quadratic solver (the tolerances of test_infinite_delta_is_the_quadratic_solver)
    x0 = np.full(m.ishape, 0.5)
    xq, gq, _ = m.mmmg(c["y"], mu=1.0, mu_reg=5e3, x0=x0, max_iter=po.NIT)
    for big in (1e30, float("inf")):
        for kind in NEW:
            xb, gb, nb = m.mmmg(c["y"], mu=1.0, mu_reg=5e3, x0=x0, max_iter=po.NIT, delta=big, potential=kind)
            assert nb == po.NIT and rel(xb, xq) < 1e-4 and _max_rel(gb, gq) < 2e-4, (big, kind)
    with pytest.raises(ValueError):
        m.set_potential("prior", "huber")
    with pytest.raises(ValueError):
        m.set_potential("spatial", "cauchy")
    with pytest.raises(ValueError):
        m.mmmg(c["y"], potential="hyperbolic", **kw)


def test_kind_reaches_the_cube_kernels(vox):
    """A Hebert-Leahy run differs from the Huber run of the same thresholds by more than 100 x the solver tolerance.  On the cube:
    its oracle iterates are 1.1e-1 apart (tests/test_potentials_host.py asserts it), the maps' -- a problem the data term
    dominates -- only 1.7e-3."""
    c, m = vox
    xh, _, _ = m.mmmg_vox(c["y"], mu=1.0, x0=c["x0"], max_iter=po.NIT, **po.VOX)
    xe, _, _ = m.mmmg_vox(c["y"], mu=1.0, x0=c["x0"], max_iter=po.NIT, spat_potential="huber", spec_potential="huber", **po.VOX)
    assert np.array_equal(xh, xe)
    xl, _, _ = m.mmmg_vox(c["y"], mu=1.0, x0=c["x0"], max_iter=po.NIT, spat_potential="hebert_leahy", spec_potential="hebert_leahy",
                          **po.VOX)
    print(f"cube: Hebert-Leahy vs Huber {rel(xl, xh):.2e}")
    assert rel(xl, xh) > 100 * vo.X_TOL_BOUND
    # one slot at a time: each family's kind reaches its own kernel argument
    xs, _, _ = m.mmmg_vox(c["y"], mu=1.0, x0=c["x0"], max_iter=po.NIT, spat_potential="hebert_leahy", **po.VOX)
    xw, _, _ = m.mmmg_vox(c["y"], mu=1.0, x0=c["x0"], max_iter=po.NIT, spec_potential="hebert_leahy", **po.VOX)
    assert rel(xs, xw) > 100 * vo.X_TOL_BOUND and rel(xs, xh) > 100 * vo.X_TOL_BOUND and rel(xw, xh) > 100 * vo.X_TOL_BOUND


# ---- descent ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NEW)
def test_criteria_never_increase(maps, vox, kind):
    from surfh_amd.algorithms import vox_criterion
    from surfh_amd.fusion import QuadCriterion_MRS
    c, m = maps
    q = QuadCriterion_MRS(1.0, c["y"], m, po.MAPS["mu_reg"], delta=po.MAPS["delta"], potential=kind)
    js = [q.get_crit_val(c["x0"])]
    x, _, n = m.mmmg(c["y"], mu=1.0, mu_reg=po.MAPS["mu_reg"], x0=c["x0"], max_iter=12, delta=po.MAPS["delta"], potential=kind,
                     callback=lambda it, g, xx: js.append(q.get_crit_val(xx)) and False)
    js = np.array(js)
    assert n == 12 and len(js) == 13 and np.all(np.diff(js) <= 1e-6 * js[:-1]) and js[-1] < js[0]     # MM: up to fp32 noise
    ref = po.maps_run(kind)
    assert abs(js[8] - ref["crit"][8]) < 1e-5 * js[8]
    res = q.run_method("mmmg", 12, value_init=c["x0"])
    assert np.array_equal(res.x.reshape(m.ishape), x) and m.get_potential("spatial") == "huber"
    cv, mv = vox
    other = "hebert_leahy" if kind == "hyperbolic" else "hyperbolic"
    pots = dict(spat_potential=kind, spec_potential=other)
    args = (po.VOX["spat_reg"], po.VOX["spat_delta"], po.VOX["spec_reg"], po.VOX["spec_delta"])
    jv = [vox_criterion(cv["y"], mv, cv["x0"], *args, **pots)]
    mv.mmmg_vox(cv["y"], mu=1.0, x0=cv["x0"], max_iter=po.NIT, callback=lambda it, g, xx: jv.append(vox_criterion(cv["y"], mv, xx, *args, **pots)) and False,
                **po.VOX, **pots)
    jv = np.array(jv)
    assert len(jv) == po.NIT + 1 and np.all(np.diff(jv) <= 1e-6 * jv[:-1]) and jv[-1] < jv[0]
    assert abs(jv[-1] - po.vox_run(kind, other)["crit"][-1]) < 1e-4 * jv[-1]


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fusion_driver_writes_to_the_new_directory(tmp_path):
    drv = _script("main_fusion")
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "3", "--synthetic", "small", "-m", "mmmg",
                                      "--delta", "0.1", "--potential", "hebert_leahy"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False, 0.1, potential="hebert_leahy")
    assert d.name.endswith("_hebert_leahy_1.00e-01") and d.is_dir()
    x, crit = np.load(d / "res_x.npy"), np.load(d / "criterion.npy")
    assert x.shape == (4 * 251 * 251,) and np.isfinite(x).all() and np.isfinite(crit).all()
    assert not (tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 4, 3, 5e3, False, 0.1)).exists()


def test_deconvolution_driver_writes_to_the_new_directory(tmp_path):
    dd = _script("deconvolution_mrs")
    out = str(tmp_path / "res")
    r = CliRunner().invoke(dd.main, ["-np", "192", "-ni", "5", "-m", "qmm", "--delta", "0.05", "--potential", "hyperbolic", "--out", out])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = out + "_hyperbolic_0.05"
    assert os.path.isdir(d) and not os.path.exists(out) and not os.path.exists(out + "_huber_0.05")
    x = np.load(os.path.join(d, "res_x.npy"))
    assert x.shape[-2:] == (192, 192) and np.isfinite(x).all()
