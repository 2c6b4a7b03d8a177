"""3MG with Huber priors on independent planes on the device (surfh_mmmg_huber_planes, ``MRSBlurred.mmmg(delta=...)``) against the
float64 restatement of tests/huber_planes_oracle.py, whose preconditions tests/test_huber_planes_host.py checks without a GPU; the
two kernels alone against NumPy; the quadratic solver it reduces to, the criterion class and the driver.  Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

import huber_oracle as ho
import huber_planes_oracle as hp
import problems
from helpers import build_model, make_ifu, rel
from oracle import surfh_oracle as orc
from test_gpu_huber import _rect_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = [l for l in range(hp.L) if l != hp.EMPTY]


def _plane_model(sotf, na, nb, cls=None, spec=hp.SPEC, pts=hp.PTS):
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    s = problems.STEP_DEG
    return (cls or MRSBlurred)(sotf, orc.synthetic_axes(na, s), orc.synthetic_axes(nb, s), make_ifu(spec), s,
                               instru.CoordList([instru.Coord(a, b) for a, b in pts]))


@pytest.fixture(scope="module")
def dev():
    """The shared problem, its model and the device run every comparison below starts from."""
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    truth, x0, y = hp.problem()
    x, gn, nit = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA)
    yield m, x0, y, (x, gn, nit, m.last_prior_values.copy())
    m.close()


def _max_rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


# ---- the two kernels alone -----------------------------------------------------------------------------------------------------
def _planes_outputs(m, x, g0, p0, p1, coef, delta):
    import torch
    x_t, p0_t, p1_t = (torch.as_tensor(v, device="cuda:0") for v in (x, p0, p1))
    g_t = torch.as_tensor(g0, device="cuda:0")
    torch.cuda.synchronize()
    sq, val = m.huber_planes_prior_dev(x_t, g_t, coef, delta)
    curv = m.huber_planes_curv_dev(x_t, p0_t, p1_t, delta)
    torch.cuda.synchronize()
    return g_t.cpu().numpy(), sq, val, curv


@pytest.mark.parametrize("L,na,nb", [(1, 72, 77), (2, 72, 77), (5, 72, 77), (5, 96, 96)])
def test_kernels_match_numpy_plane_by_plane(L, na, nb):
    """72 x 77: Na != Nb, an odd width that is no multiple of 64 -- the wrap rows and columns and the tail lanes of the block
    reduction.  Bound: 10 x the error of huber_grad_kernel (the map kernel, through a template model with T = L maps of the same
    size) on the same arrays, measured here."""
    import torch
    delta, coef = 0.3, 0.7
    rng = np.random.default_rng(100 * L + na)
    scale = np.where(np.arange(L) % 2 == 0, 2 * delta, 0.1 * delta)[:, None, None]       # weights below 1 in the even planes only
    x = (rng.standard_normal((L, na, nb)) * scale).astype(np.float32)
    g0, p0, p1 = (rng.standard_normal((L, na, nb)).astype(np.float32) for _ in range(3))
    x64, a, b = x.astype(np.float64), p0.astype(np.float64), p1.astype(np.float64)
    beyond = [hp.share_beyond(x64[l], delta) for l in range(L)]
    assert all((0.1 < s < 0.9) if l % 2 == 0 else s == 0.0 for l, s in enumerate(beyond)), beyond
    want = g0 + coef * ho.prior_grad(x64, delta)
    want_sq = np.sum(want ** 2, axis=(1, 2))
    want_val = np.array([ho.prior_value(x64[l:l + 1], delta) for l in range(L)])
    ws = [ho.weight(d(x64), delta) for d, _ in ho.DIFFS]
    want_c = np.array([[sum(np.sum((w * d(u) * d(v))[l]) for w, (d, _) in zip(ws, ho.DIFFS)) for u, v in ((a, a), (a, b), (b, b))]
                       for l in range(L)])
    # the yardstick: the map kernel on the same arrays
    mt = build_model(_rect_problem(na, nb, L))
    try:
        assert mt.ishape == (L, na, nb)
        g_t = torch.as_tensor(g0, device="cuda:0")
        torch.cuda.synchronize()
        mt.huber_prior_dev(torch.as_tensor(x, device="cuda:0"), g_t, coef, delta)
        torch.cuda.synchronize()
        e_ref = rel(g_t.cpu().numpy(), want)
    finally:
        mt.close()
    bound = 10 * e_ref
    wav = np.linspace(7.0, 8.2, L) if L > 1 else np.array([7.6])
    m = _plane_model(orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (na, nb)), na, nb)
    try:
        assert m.ishape == (L, na, nb)
        out, sq, val, curv = _planes_outputs(m, x, g0, p0, p1, coef, delta)
        e = dict(ng=max(rel(out[l], want[l]) for l in range(L)), sq=_max_rel(sq, want_sq), phi=_max_rel(val, want_val),
                 curv=float(np.max(np.abs(curv - want_c) / np.max(np.abs(want_c), axis=1, keepdims=True))))
        print(f"{L} x {na} x {nb}: huber_grad_kernel {e_ref:.2e} (bound {bound:.2e}); plane kernels", {k: f"{v:.2e}" for k, v in e.items()})
        assert max(e.values()) < bound
        for idx in [(0, 0, 0), (L - 1, na - 1, 0), (0, 0, nb - 1), (L - 1, na - 1, nb - 1)]:      # the wrap corners, entry by entry
            assert abs(out[idx] - want[idx]) < 1e-5 * (1 + abs(want[idx]))
        # the weights matter: the unweighted sums are far off in the planes with weights below 1
        plain = sum(np.sum(d(a)[0] ** 2) for d, _ in ho.DIFFS)
        assert abs(plain - want_c[0, 0]) > 0.1 * want_c[0, 0]
        # the same inputs give the same bits
        again = _planes_outputs(m, x, g0, p0, p1, coef, delta)
        assert all(np.array_equal(u, v) for u, v in zip((out, sq, val, curv), again))
        # a plane's outputs depend on that plane alone: change every input of one plane, the others keep their bits
        if L > 1:
            k = L - 1
            x2, g2, a2, b2 = x.copy(), g0.copy(), p0.copy(), p1.copy()
            x2[k] = x2[k] * 3 + 1
            g2[k], a2[k], b2[k] = g2[k] - 2, a2[k] * 2, b2[k] + 1
            out2, sq2, val2, curv2 = _planes_outputs(m, x2, g2, a2, b2, coef, delta)
            keep = [l for l in range(L) if l != k]
            assert np.array_equal(out2[keep], out[keep]) and np.array_equal(sq2[keep], sq[keep])
            assert np.array_equal(val2[keep], val[keep]) and np.array_equal(curv2[keep], curv[keep])
            assert not np.array_equal(out2[k], out[k]) and sq2[k] != sq[k] and val2[k] != val[k]
        x_t = torch.zeros(m.ishape, device="cuda:0")
        for bad in (0.0, -1.0, float("nan"), 1e-40):                          # 1e-40 does not survive the fp32 kernels
            with pytest.raises(RuntimeError):
                m.huber_planes_prior_dev(x_t, x_t.clone(), 1.0, bad)
            with pytest.raises(RuntimeError):
                m.huber_planes_curv_dev(x_t, x_t, x_t, bad)
            with pytest.raises(RuntimeError):
                m.mmmg(np.zeros(m.oshape), mu_reg=1.0, delta=bad, max_iter=1)
        assert not m.huber_planes_prior_dev(x_t, x_t.clone(), 1.0, float("inf"))[1].any()
    finally:
        m.close()


# ---- the solver against the oracle ------------------------------------------------------------------------------------------------
def test_solver_matches_oracle_plane_by_plane(dev):
    """Bounds hp.TOL_X, hp.TOL_G (tests/huber_planes_oracle.py).  Measured on MI355X: see DESIGN.md section 9."""
    m, x0, y, (x, gn, nit, pv) = dev
    ref = hp.reference()
    assert nit == hp.NIT and x.shape == (hp.L, hp.N, hp.N) and gn.shape == (hp.NIT + 1, hp.L) and pv.shape == (hp.L,)
    # the plane without data stays exactly at rest
    assert not x[hp.EMPTY].any() and not gn[:, hp.EMPTY].any() and np.isfinite(x).all() and np.isfinite(gn).all()
    for l in hp.COMPARED:
        gr = np.array(ref[l]["grad_norm"])
        ex, eg = rel(x[l], ref[l]["x"]), _max_rel(gn[:, l], gr)
        print(f"plane {l}: |D x| > delta for {hp.share_beyond(x[l], hp.DELTA):.0%}; device vs oracle: x {ex:.2e} (bound {hp.TOL_X:.1e}), "
              f"|g| {eg:.2e} (bound {hp.TOL_G:.1e})")
        assert ex < hp.TOL_X and eg < hp.TOL_G, l
        want = ho.prior_value(x[l:l + 1], hp.DELTA)
        assert abs(pv[l] - want) < 1e-5 * want
    assert pv[hp.EMPTY] == 0.0
    # the refresh period changes rounding only
    xf, gf, _ = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA, refresh=1)
    for l in hp.COMPARED:
        ex, eg = rel(xf[l], x[l]), _max_rel(gf[:, l], gn[:, l])
        print(f"plane {l}: refresh 1 vs 50: x {ex:.2e}, |g| {eg:.2e}")
        assert ex < hp.TOL_X and eg < hp.TOL_G
    assert not xf[hp.EMPTY].any() and not gf[:, hp.EMPTY].any()


def test_infinite_delta_is_the_quadratic_solver(dev):
    """mu |y - A x|^2 / 2 + mu_reg sum u^2 / 2 is half the quadratic criterion of ``mmmg()``: same iterates, same trace."""
    m, x0, y, _ = dev
    xq, gq, nq = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT)
    assert m.last_prior_values is None
    xh, gh, nh = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=1e30)
    assert nh == nq == hp.NIT and not xh[hp.EMPTY].any() and not gh[:, hp.EMPTY].any()
    for l in LIVE:
        ex, eg = rel(xh[l], xq[l]), _max_rel(gh[:, l], gq[:, l])
        print(f"plane {l}: delta = 1e30 vs quadratic: x {ex:.2e}, |g| {eg:.2e}")
        assert ex < 1e-4 and eg < 1e-4
        assert abs(m.last_prior_values[l] - np.sum(orc.diff_r(xh[l:l + 1]) ** 2 + orc.diff_c(xh[l:l + 1]) ** 2) / 2) < 1e-5 * m.last_prior_values[l]


def test_single_image_model_and_criterion_class(dev):
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D
    m, x0, y, (x, gn, nit, pv) = dev
    l = 0
    m1 = _plane_model(hp.sotf(l), hp.N, hp.N)
    try:
        x1, g1, n1 = m1.mmmg(y[l], mu=hp.MU, mu_reg=hp.MUR, x0=x0[l], max_iter=hp.NIT, delta=hp.DELTA)
        assert x1.shape == (hp.N, hp.N) and g1.shape == (n1 + 1,) and n1 == hp.NIT and m1.last_prior_values.shape == (1,)
        assert rel(x1, x[l]) < 1e-4 and _max_rel(g1, gn[:, l]) < 1e-4
        q = QuadCriterion_MRS_2D(hp.MU, y[l], m1, hp.MUR, delta=hp.DELTA)
        res = q.run_method("qmm", hp.NIT, value_init=x0[l])
        assert res.nit == hp.NIT and np.array_equal(res.x.reshape(hp.N, hp.N), x1) and np.array_equal(res.grad_norm, g1)
        j0, j1 = q.get_crit_val(x0[l]), q.get_crit_val(res.x)
        jr = ho.crit(hp.plane_op(l), y[l], x1[None], hp.MU, hp.MUR, hp.DELTA)
        assert j1 < j0 and abs(j1 - jr) < 1e-5 * jr
        assert abs(QuadCriterion_MRS_2D(hp.MU, y[l], m1, hp.MUR).get_crit_val(res.x) - j1) > 1e-2 * j1     # not the quadratic one
        with pytest.raises(ValueError):
            q.run_method("lcg", hp.NIT)
    finally:
        m1.close()
    # the batched criterion: the sum over the planes decreases
    qb = QuadCriterion_MRS_2D(hp.MU, y, m, hp.MUR, delta=hp.DELTA)
    rb = qb.run_method("qmm", hp.NIT, value_init=x0)
    assert np.array_equal(rb.x.reshape(x.shape), x) and qb.get_crit_val(rb.x) < qb.get_crit_val(x0)


def test_masked_samples_are_ignored(dev):
    """``weights=`` as a 0/1 mask with NaN in the masked samples of y: the iterate of the oracle run on the masked problem."""
    m, x0, y, (x, _, _, _) = dev
    mask = hp.sample_mask(y.shape[1])
    w = np.tile(mask, (hp.L, 1))
    y_nan = np.where(w > 0, y, np.nan)
    xw, gw, nw = m.mmmg(y_nan, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA, weights=w)
    assert nw == hp.NIT and np.isfinite(xw).all() and np.isfinite(gw).all() and m.data_weights is None
    assert not xw[hp.EMPTY].any() and not gw[:, hp.EMPTY].any()
    for l in (0, hp.QUIET):
        ref = hp.solve_plane(l, y[l], x0[l], mask=mask)
        ex, eg = rel(xw[l], ref["x"]), _max_rel(gw[:, l], ref["grad_norm"])
        print(f"plane {l}, masked: x {ex:.2e}, |g| {eg:.2e}; masked vs unmasked device iterate {rel(xw[l], x[l]):.1e}")
        assert ex < hp.TOL_X and eg < hp.TOL_G
    assert rel(xw[0], x[0]) > 100 * hp.TOL_X                # the mask is felt (tests/test_huber_planes_host.py, on the oracle)


def test_repeatable_and_callback(dev):
    m, x0, y, (x, gn, nit, pv) = dev
    seen = []
    x2, g2, n2 = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA,
                        callback=lambda it, g, xx: seen.append((it, g.shape, xx.shape)) and False)
    assert np.array_equal(x2, x) and np.array_equal(g2, gn) and np.array_equal(m.last_prior_values, pv)      # same bits
    assert seen == [(it, (it + 1, hp.L), x.shape) for it in range(1, hp.NIT + 1)]
    stop = []
    x3, g3, n3 = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA,
                        callback=lambda it, g, xx: stop.append(it) or it == 3)
    assert n3 == 3 and stop == [1, 2, 3] and np.array_equal(g3, gn[:4])
    # the tolerance stop looks at the worst plane
    worst = gn.max(axis=1)
    k = int(np.argmin(worst))                           # the first iteration whose worst plane is below every earlier one's
    assert k > 0 and worst[:k].min() > worst[k] * 1.001
    xt, gt, nt = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA, tol=worst[k] * 1.0001 / hp.N ** 2)
    assert nt == k and np.array_equal(gt, gn[:k + 1])


def test_rotated_field_model_runs_the_same_solver():
    import rotated_oracle as ro
    from surfh_amd.spectro_blind import MRSBlurred
    case = ro.small_case(L=3, angle=20.0)
    m = _plane_model(case["sotf"], 96, 96, cls=MRSBlurred, spec=case["spec"], pts=case["pointings"])
    try:
        truth, x0, _ = hp.problem()
        truth, x0 = truth[[0, 1, 4]], x0[[0, 1, 4]]
        y = m.forward(truth)
        js = []
        from surfh_amd.spectro_blind import QuadCriterion_MRS_2D
        q = QuadCriterion_MRS_2D(hp.MU, y, m, hp.MUR, delta=hp.DELTA)
        x, gn, nit = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT, delta=hp.DELTA,
                            callback=lambda it, g, xx: js.append(q.get_crit_val(xx)) and False)
        js = np.array([q.get_crit_val(x0)] + js)
        assert nit == hp.NIT and m.last_prior_values.shape == (3,) and min(hp.share_beyond(x[l], hp.DELTA) for l in range(3)) > 0.2
        assert np.all(np.diff(js) <= 1e-6 * js[:-1]) and js[-1] < 0.5 * js[0]                 # MM: non-increasing up to fp32 noise
        xq, _, _ = m.mmmg(y, mu=hp.MU, mu_reg=hp.MUR, x0=x0, max_iter=hp.NIT)
        assert rel(x, xq) > 1e-2                                                              # not the quadratic solver
    finally:
        m.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def test_driver_writes_huber_results(tmp_path):
    """-np 192: the band-1C field of view of the driver's problem (139 x 159 pixels) does not fit a smaller image such as 96."""
    sp = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    dd = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(dd)
    out = str(tmp_path / "res")
    r = CliRunner().invoke(dd.main, ["-np", "192", "--planes", "2", "-ni", "5", "-m", "qmm", "--delta", "0.05", "--out", out])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = out + "_huber_0.05"
    assert os.path.isdir(d) and not os.path.exists(out)
    x, crit = np.load(os.path.join(d, "res_x.npy")), np.load(os.path.join(d, "criterion.npy"))
    assert x.shape == (2, 192, 192) and np.isfinite(x).all() and len(crit) == 1 and r.output.count("Iteration n°") == 5
    r = CliRunner().invoke(dd.main, ["-np", "192", "--planes", "2", "-ni", "5", "-m", "lcg", "--delta", "0.05", "--out", out])
    assert r.exit_code != 0 and isinstance(r.exception, ValueError)
    assert "lcg minimises quadratic criteria only: a Huber prior (delta) needs method='mmmg'" in str(r.exception)
    assert not os.path.exists(out)
