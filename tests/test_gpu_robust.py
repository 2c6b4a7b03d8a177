"""The robust (Huber) data term on the device (surfh_mmmg_robust, surfh_mmmg_robust_vox, surfh_robust_data_dev,
surfh_robust_curv_dev) against the float64 restatement of tests/robust_oracle.py, the weighted quadratic solvers it reduces to,
the criterion class and the algorithms (needs an MI355X).  tests/test_robust_host.py asserts, without a GPU, the preconditions
under which these comparisons mean something."""
import numpy as np
import pytest

import robust_oracle as ro
import vox_oracle as vo
from capped_cases import ROBUST_CALLS, robust_arrays
from helpers import build_model, rel
from test_gpu_parity import note

pytestmark = pytest.mark.gpu
INF = float("inf")
DD = ro.DATA_DELTA


@pytest.fixture(scope="module")
def setup():
    c = ro.config1_case()
    m = build_model(c["cfg"])
    yield c, m
    m.close()


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 1101, 3840, 100003, ROBUST_CALLS[0][0]])
def test_kernels_match_numpy(setup, n):
    """single lane, partial block, the odd detector-axis length of the weights test, config 1's osize, multi-block with a tail,
    and 2 100 227: past the 2048 blocks of the 16-byte path, three blocks on a second trip and a tail of 3 (the 8- and 4-byte
    calls further down are then on their second and fifth trips)"""
    import torch
    _, m = setup
    u, w, y, p0, p1 = robust_arrays(n)                                        # a fifth masked, NaN there, both sides of the knee
    keep = w > 0
    w64, a, b = w.astype(np.float64), p0.astype(np.float64), p1.astype(np.float64)
    t = np.where(keep, np.sqrt(w64) * (np.where(keep, y, 0.0).astype(np.float64) - u), 0.0)
    share = np.mean(np.abs(t[keep]) > DD)
    if n > 1:
        assert 0.1 < share < 0.9
    want_v = np.sqrt(w64) * ro.dphi(t, DD)
    want_s = np.array([np.sum(ro.phi(t, DD)), np.sum(np.abs(t) > DD)])
    ww = w64 * np.where(keep, ro.weight(t, DD), 0.0)
    want_c = np.array([np.sum(ww * a * a), np.sum(ww * a * b), np.sum(ww * b * b)])
    near = int(np.sum(np.abs(np.abs(t) - DD) < 1e-6 * DD))                    # samples whose side fp32 rounding may change
    y_t, u_t, w_t, p0_t, p1_t = (torch.as_tensor(v, device="cuda:0") for v in (y, u, w, p0, p1))
    vs, sums, curv = [], [], []
    for _ in range(2):
        v_t = torch.full((n,), 7.0, device="cuda:0")
        torch.cuda.synchronize()
        sums.append(m.robust_data_dev(y_t, u_t, w_t, v_t, n, DD))
        curv.append(m.robust_curv_dev(y_t, u_t, w_t, p0_t, p1_t, n, DD))
        torch.cuda.synchronize()
        vs.append(v_t.cpu().numpy())
    ev = float(np.max(np.abs(vs[0] - want_v)) / np.max(np.abs(want_v)))
    ep = abs(sums[0][0] - want_s[0]) / want_s[0]
    ec = float(np.max(np.abs(curv[0] - want_c)) / np.max(np.abs(want_c)))
    print(f"n = {n}: beyond {share:.0%}, v {ev:.2e}, sum phi {ep:.2e}, count {sums[0][1]} / {int(want_s[1])}, curvature {ec:.2e}")
    note("robust_kernels", n=n, v=ev, phi=ep, curv=ec, count_off=abs(sums[0][1] - want_s[1]), near=near)
    assert np.all(np.isfinite(vs[0])) and np.all(vs[0][~keep] == 0.0)
    assert ev < 1e-6 and ep < 1e-6 and ec < 1e-6 and abs(sums[0][1] - want_s[1]) <= near
    assert sums[0] == sums[1] and np.array_equal(vs[0], vs[1]) and np.array_equal(curv[0], curv[1])      # deterministic reductions
    plain = np.sum(w64 * a * a)
    if n > 1:
        assert abs(plain - want_c[0]) > 0.1 * want_c[0]                       # omega matters
    # an infinite threshold: omega = 1, v = w (y - u), nothing beyond
    v_t = torch.zeros(n, device="cuda:0")
    si = m.robust_data_dev(y_t, u_t, w_t, v_t, n, INF)
    ci = m.robust_curv_dev(y_t, u_t, w_t, p0_t, p1_t, n, INF)
    assert si[1] == 0 and abs(si[0] - np.sum(t * t) / 2) < 1e-6 * np.sum(t * t) / 2 and abs(ci[0] - plain) < 1e-6 * plain
    assert float(np.max(np.abs(v_t.cpu().numpy() - np.sqrt(w64) * t))) < 1e-6 * np.max(np.abs(t))
    # without weights, and from addresses that allow only 8- and 4-byte accesses
    if n > 8:
        for off in (0, 2, 1):
            k = n - off
            t1 = y.astype(np.float64)[off:] - u[off:]
            ok = np.isfinite(t1)
            yy = torch.as_tensor(np.where(ok, y[off:], u[off:]), device="cuda:0")
            buf = torch.zeros(n, device="cuda:0")
            s1 = m.robust_data_dev(yy, u_t[off:], None, buf[off:], k, DD)
            t1 = np.where(ok, t1, 0.0)
            assert abs(s1[0] - np.sum(ro.phi(t1, DD))) < 1e-6 * np.sum(ro.phi(t1, DD))
            assert float(np.max(np.abs(buf.cpu().numpy()[off:] - ro.dphi(t1, DD)))) < 1e-6 * DD and np.all(buf.cpu().numpy()[:off] == 0)
            c1 = m.robust_curv_dev(yy, u_t[off:], None, p0_t[off:], p1_t[off:], k, DD)
            assert abs(c1[1] - np.sum(ro.weight(t1, DD) * a[off:] * b[off:])) < 1e-6 * np.sum(ro.weight(t1, DD) * a[off:] ** 2)


def test_bad_threshold_is_refused(setup):
    import torch
    c, m = setup
    z = torch.zeros(16, device="cuda:0")
    for bad in (0.0, -1.0, float("nan"), 1e-40):                              # 1e-40 does not survive the fp32 kernels
        with pytest.raises(RuntimeError):
            m.robust_data_dev(z, z, None, z.clone(), 16, bad)
        with pytest.raises(RuntimeError):
            m.robust_curv_dev(z, z, None, z, z, 16, bad)
        with pytest.raises(RuntimeError):
            m.mmmg(c["y"], mu_reg=c["mur"], max_iter=1, weights=c["w"], data_delta=bad)
    with pytest.raises(ValueError):
        m.cg(c["y"], mu_reg=c["mur"], max_iter=1, weights=c["w"], data_delta=DD)


# ---- 2. the solver against the oracle ---------------------------------------------------------------------------------------------
def _kw(c, regime):
    delta, nit = ro.C1_REGIMES[regime]
    return dict(mu=1.0, mu_reg=c["mur"], x0=c["starts"][regime], max_iter=nit, weights=c["w"], **({} if np.isinf(delta) else {"delta": delta}))


@pytest.mark.parametrize("regime", list(ro.C1_REGIMES))
def test_mmmg_robust_matches_oracle(setup, regime):
    c, m = setup
    om, runs = c["om"], ro.config1_runs(regime)
    delta, nit = ro.C1_REGIMES[regime]
    share, away, to_clean, quad_to_clean = ro.preconditions(om, c, runs)
    assert 0.01 < share < 0.20 and away > 20 * 1e-4 and 3 * to_clean <= quad_to_clean
    x, gn, n = m.mmmg(c["y"], data_delta=DD, **_kw(c, regime))
    value, beyond, omega, prior = m.robust_data_value, m.robust_n_beyond, m.robust_weights, m.huber_prior_value
    gr = np.array(runs["rob"]["grad_norm"])
    ex, eg = rel(x, runs["rob"]["x"]), float(np.max(np.abs(gn - gr) / gr))
    xq, _, _ = m.mmmg(c["y"], **_kw(c, regime))
    assert m.robust_weights is None and m.robust_data_value is None and m.robust_n_beyond is None     # no stale diagnostics
    print(f"{regime}: |t| > delta for {share:.1%}, oracle robust vs quadratic {away:.1e}, device vs oracle: x {ex:.2e}, grad_norm "
          f"{eg:.2e}; device robust vs quadratic {rel(x, xq):.1e}; to the clean solve {rel(x, runs['clean']['x']):.1e} against "
          f"{rel(xq, runs['clean']['x']):.1e}")
    assert n == nit and gn.shape == (nit + 1,) and ex < ro.X_TOL_BOUND and eg < ro.G_TOL_BOUND
    assert rel(x, xq) > 20 * 1e-4
    # the diagnostics, against the oracle at the device's iterate
    t = ro.residual(om, c["y"], x, c["w"]).ravel()
    near = int(np.sum(np.abs(np.abs(t) - DD) < 1e-4 * DD))
    dv = ro.data_value(om, c["y"], x, DD, c["w"])
    assert abs(value - dv) < 1e-5 * dv and abs(beyond - ro.n_beyond(om, c["y"], x, DD, c["w"])) <= near
    want_om = ro.omega(om, c["y"], x, DD, c["w"])
    print(f"   sum phi {abs(value - dv) / dv:.2e}, count {beyond} (+- {near}), omega {rel(omega, want_om):.2e} "
          f"(max {float(np.max(np.abs(omega - want_om))):.2e})")
    assert omega.shape == (om.osize,) and rel(omega, want_om) < 1e-5
    assert omega.max() == 1.0 and omega.min() > 0 and np.median(omega[c["spikes"]]) < 0.2
    if np.isinf(delta):
        assert prior is None
    else:
        assert abs(prior - ro.ho.prior_value(x, delta)) < 1e-5 * prior
    xf, _, _ = m.mmmg(c["y"], data_delta=DD, refresh=1, **_kw(c, regime))       # the refresh period changes rounding only
    assert rel(xf, x) < 1e-4


# ---- 3. reduction to the weighted quadratic data term ------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(ro.C1_REGIMES))
def test_huge_threshold_is_the_weighted_solver(setup, regime):
    c, m = setup
    xq, gq, nq = m.mmmg(c["y"], **_kw(c, regime))
    for big in (1e30, INF):
        xr, gr, nr = m.mmmg(c["y"], data_delta=big, **_kw(c, regime))
        ex, eg = rel(xr, xq), float(np.max(np.abs(gr - gq) / gq))
        print(f"{regime}, data_delta = {big}: x {ex:.2e}, grad_norm {eg:.2e}")
        assert nr == nq and ex < ro.X_TOL_BOUND and eg < ro.G_TOL_BOUND
        assert m.robust_n_beyond == 0 and np.all(m.robust_weights == 1.0)


# ---- 4. masking --------------------------------------------------------------------------------------------------------------------
def test_masked_samples_do_not_matter(setup):
    c, m = setup
    w = c["w"].copy()
    w[c["spikes"]] = 0.0
    outs = []
    for filling in (np.nan, 1e3 * np.max(np.abs(c["y"]))):
        y = c["y"].copy()
        y[c["spikes"]] = filling
        kw = dict(_kw(c, "quadratic"), weights=w)
        x, gn, n = m.mmmg(y, data_delta=DD, **kw)
        outs.append((x, gn, m.robust_weights.copy(), m.robust_data_value))
        assert np.all(np.isfinite(x)) and np.all(m.robust_weights[c["spikes"]] == 0.0)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]


# ---- 5. the cube ---------------------------------------------------------------------------------------------------------------------
def test_mmmg_robust_vox_matches_oracle():
    from surfh_amd.algorithms import vox_criterion, vox_reconstruction
    c, runs = ro.vox_case(), ro.vox_runs()
    sr, sd, lr, ld, nit = ro.VOX_REGIME
    sr, lr = sr * c["scale"], lr * c["scale"]
    share, away, to_clean, quad_to_clean = ro.preconditions(c["om"], c, runs)
    assert 0.01 < share < 0.20 and away > 20 * ro.X_TOL_BOUND and 3 * to_clean <= quad_to_clean
    m = build_model(c["cfg"])
    try:
        kw = dict(mu=1.0, spat_reg=sr, spat_delta=sd, spec_reg=lr, spec_delta=ld, x0=c["x0"], max_iter=nit, weights=c["w"])
        x, gn, n = m.mmmg_vox(c["y"], data_delta=DD, **kw)
        value, omega, priors = m.robust_data_value, m.robust_weights, m.huber_prior_values
        gr = np.array(runs["rob"]["grad_norm"])
        ex, eg = rel(x, runs["rob"]["x"]), float(np.max(np.abs(gn - gr) / gr))
        xq, gq, _ = m.mmmg_vox(c["y"], **kw)
        assert m.robust_weights is None
        print(f"voxel-wise: |t| > delta for {share:.1%}, oracle robust vs quadratic {away:.1e}, device vs oracle: x {ex:.2e}, "
              f"grad_norm {eg:.2e}; device robust vs quadratic {rel(x, xq):.1e}")
        assert n == nit and ex < vo.X_TOL_BOUND and eg < vo.G_TOL_BOUND and rel(x, xq) > 20 * vo.X_TOL_BOUND
        dv = ro.data_value(c["om"], c["y"], x, DD, c["w"])
        pv = vo.prior_values(x, sd, ld)
        assert abs(value - dv) < 1e-5 * dv and abs(priors[0] - pv[0]) < 1e-5 * pv[0] and abs(priors[1] - pv[1]) < 1e-5 * pv[1]
        assert rel(omega, ro.omega(c["om"], c["y"], x, DD, c["w"])) < 1e-5
        xb, gb, _ = m.mmmg_vox(c["y"], data_delta=1e30, **kw)                    # the reduction, on the cube
        assert rel(xb, xq) < vo.X_TOL_BOUND and float(np.max(np.abs(gb - gq) / gq)) < vo.G_TOL_BOUND
        # the algorithms' entry points
        r = vox_reconstruction(c["y"], m, spat_reg=sr, spat_th=sd, spec_reg=lr, spec_th=ld, init=c["x0"], max_iter=nit, weights=c["w"],
                               data_th=DD)
        assert r.nit == nit and rel(r.x.reshape(m.ishape), x) == 0.0
        j = ro.crit_vox(c["om"], c["y"], x, 1.0, DD, sr, sd, lr, ld, c["w"])
        assert abs(vox_criterion(c["y"], m, x, sr, sd, lr, ld, weights=c["w"], data_th=DD) - j) < 1e-5 * j
    finally:
        m.close()


# ---- 6. the criterion class and the algorithms ---------------------------------------------------------------------------------------
def test_criterion_class_and_lmm_reconstruction(setup):
    from surfh_amd.algorithms import lmm_reconstruction
    from surfh_amd.fusion import QuadCriterion_MRS
    c, m = setup
    delta, nit = ro.C1_REGIMES["huber"]
    x0 = c["starts"]["huber"]
    x, gn, _ = m.mmmg(c["y"], data_delta=DD, **_kw(c, "huber"))
    q = QuadCriterion_MRS(1.0, c["y"], m, c["mur"], delta=delta, weights=c["w"], data_delta=DD)
    res = q.run_method("mmmg", nit, value_init=x0)
    assert res.nit == nit and rel(res.x.reshape(m.ishape), x) == 0.0 and np.array_equal(res.grad_norm, gn)
    assert m.robust_weights is not None and m.data_weights is None            # the solve's weights are taken off again
    jr = ro.crit(c["om"], c["y"], x, 1.0, DD, c["mur"], delta, c["w"])
    assert abs(q.get_crit_val(res.x) - jr) < 1e-5 * jr
    jq = QuadCriterion_MRS(1.0, c["y"], m, c["mur"], delta=delta, weights=c["w"]).get_crit_val(res.x)
    assert abs(jq - jr) > 1e-2 * jr                                           # the robust criterion, not the quadratic one
    # quadratic priors under the robust term
    xq, _, _ = m.mmmg(c["y"], data_delta=DD, **_kw(c, "quadratic"))
    q2 = QuadCriterion_MRS(1.0, c["y"], m, c["mur"], weights=c["w"], data_delta=DD)
    r2 = q2.run_method("mmmg", ro.C1_REGIMES["quadratic"][1], value_init=0.5)
    j2 = ro.crit(c["om"], c["y"], xq, 1.0, DD, c["mur"], INF, c["w"])
    assert rel(r2.x.reshape(m.ishape), xq) == 0.0 and abs(q2.get_crit_val(r2.x) - j2) < 1e-5 * j2
    with pytest.raises(ValueError):
        q.run_method("lcg", nit)
    with pytest.raises(ValueError):
        m.cg(c["y"], mu_reg=c["mur"], data_delta=DD)
    r = lmm_reconstruction(c["y"], m, spat_reg=c["mur"], spat_th=delta, init=x0, max_iter=nit, weights=c["w"], data_th=DD)
    assert r.nit == nit and rel(r.x.reshape(m.ishape), x) == 0.0
    # the criterion descends along the device's path, and the callback sees every iterate
    js = []
    m.mmmg(c["y"], data_delta=DD, callback=lambda it, g, xx: js.append(q.get_crit_val(xx)) and False, **_kw(c, "huber"))
    js = np.array([q.get_crit_val(x0)] + js)
    assert len(js) == nit + 1 and np.all(np.diff(js) <= 1e-6 * js[:-1]) and js[-1] < js[0]
    assert abs(js[-1] - jr) < 1e-6 * jr
