"""Voxel-wise 3MG with Huber priors on the device (surfh_mmmg_huber_vox, surfh_huber_vox_prior_dev, surfh_huber_vox_curv_dev)
against numpy and the float64 restatement of tests/vox_oracle.py, vox_reconstruction and the fusion driver's --voxel
(needs an MI355X).  The regimes and their preconditions are those of tests/test_vox_host.py.

Bounds of the solver comparison.  tests/test_gpu_huber.py holds the map-domain solver to 1e-4 (x) and 2e-4 (grad_norm) on the
config1 template model.  The solver's error follows the fp32 error of the operator it applies once per iteration, so those
tolerances are scaled by max(1, e_a / e_b) * 2, with e = the relative error of m.adjoint(m.forward(d)) against the oracle's
for a standard-normal d, (a) on the template-free small problem of vox_oracle, (b) on that config1 model, both measured with
the operator as it was before this solver existed; the factor 2 because the two problems' conditioning differs in a way this
ratio does not see.  Measured over three seeds: e_a = 3.1e-07, 3.7e-07, 2.7e-07 (mean 3.2e-07), e_b = 4.3e-07, 3.4e-07, 3.0e-07 (mean 3.6e-07):
e_a / e_b = 0.89, so max(1, e_a / e_b) = 1 and the bounds are 2e-4 and 4e-4
(vox_oracle.X_TOL_BOUND, G_TOL_BOUND)."""
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

import huber_oracle as ho
import problems
import vox_oracle as vo
from capped_cases import vox_arrays
from helpers import build_model, rel
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU = 1.0
INF = float("inf")


@pytest.fixture(scope="module")
def setup():
    cfg, om, cube, y = vo.small_cfg()
    m = build_model(cfg)
    assert m.ishape == om.ishape == (32, 48, 48) and not m.lmm
    yield om, m, cube, y
    m.close()


def _awkward_model(Lc):
    """A plan with an Lc x 72 x 77 cube (Na != Nb, odd Nb, not multiples of 64) for any Lc >= 1: the batched 2-D model, whose
    plan has no templates either (a fusion model needs a band of several planes)."""
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    from helpers import make_ifu
    na, nb, s = 72, 77, problems.STEP_DEG
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    sotf = orc.ir2fr(orc.gaussian_psf(np.linspace(7.0, 8.2, Lc), problems.STEP), (na, nb))
    pts = [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s)]
    return MRSBlurred(sotf, orc.synthetic_axes(na, s), orc.synthetic_axes(nb, s), make_ifu(spec), s,
                      instru.CoordList([instru.Coord(a, b) for a, b in pts]))


def _prior_dev(m, *a):
    from surfh_amd.models import spectroSigRLSCT
    return spectroSigRLSCT.huber_vox_prior_dev(m, *a)          # the method needs a plan only: any template-free model serves


def _curv_dev(m, *a):
    from surfh_amd.models import spectroSigRLSCT
    return spectroSigRLSCT.huber_vox_curv_dev(m, *a)


def _curv_want(x, a, b, ds, dl, weighted=True):
    out = np.zeros((2, 3))
    for k, (u, v) in enumerate(((a, a), (a, b), (b, b))):
        out[0, k] = sum(np.sum((ho.weight(d(x), ds) if weighted else 1.0) * d(u) * d(v)) for d, _ in ho.DIFFS)
        out[1, k] = np.sum((ho.weight(vo.diff_l(x), dl) if weighted else 1.0) * vo.diff_l(u) * vo.diff_l(v))
    return out


def _check_kernels(m, ds, dl, seed):
    import torch
    Lc, Na, Nb = m.ishape
    x, g0, p0, p1 = vox_arrays(tuple(m.ishape), ds, seed)                        # differences on both sides of both thresholds
    x64, a, b = x.astype(np.float64), p0.astype(np.float64), p1.astype(np.float64)
    s_spat, s_spec = vo.shares(x64, ds, dl)
    assert 0.1 < s_spat < 0.9 and (Lc == 1 or 0.1 < s_spec < 0.9)
    want = g0 + vo.prior_grad(x64, 0.7, ds, 0.4, dl)
    want_v = vo.prior_values(x64, ds, dl)
    want_c = _curv_want(x64, a, b, ds, dl)
    vals, outs, curv = [], [], []
    x_t, p0_t, p1_t = (torch.as_tensor(v, device="cuda:0") for v in (x, p0, p1))
    for _ in range(2):
        g_t = torch.as_tensor(g0, device="cuda:0")
        torch.cuda.synchronize()
        vals.append(_prior_dev(m, x_t, g_t, 0.7, ds, 0.4, dl))
        curv.append(_curv_dev(m, x_t, p0_t, p1_t, ds, dl))
        torch.cuda.synchronize()
        outs.append(g_t.cpu().numpy())
    assert curv[0].shape == (2, 3)
    nfam = 2 if Lc > 1 else 1
    ev = [abs(vals[0][f] - want_v[f]) / want_v[f] for f in range(nfam)]
    ec = [float(np.max(np.abs(curv[0][f] - want_c[f])) / np.max(np.abs(want_c[f]))) for f in range(nfam)]
    print(m.ishape, f"prior grad {rel(outs[0], want):.2e}, values {ev}, curvature {ec}")
    assert rel(outs[0], want) < 1e-6 and max(ev) < 1e-6 and max(ec) < 1e-6
    if Lc == 1:                                                                  # the spectral term is empty
        assert vals[0][1] == 0.0 and np.array_equal(curv[0][1], np.zeros(3))
    # deterministic reductions
    assert vals[0] == vals[1] and np.array_equal(outs[0], outs[1]) and np.array_equal(curv[0], curv[1])
    # the weights matter: the unweighted sums are far off, in both families
    plain = _curv_want(x64, a, b, ds, dl, weighted=False)
    for f in range(nfam):
        assert abs(plain[f, 0] - want_c[f, 0]) > 0.1 * want_c[f, 0]
    # the four spatial corners of the first and of the last plane (circular in-plane, open along wavelength), entry by entry
    for l in (0, Lc - 1):
        for idx in [(l, 0, 0), (l, Na - 1, 0), (l, 0, Nb - 1), (l, Na - 1, Nb - 1)]:
            assert abs(outs[0][idx] - want[idx]) < 1e-5 * (1 + abs(want[idx]))


def test_vox_kernels_match_numpy(setup):
    import torch
    om, m, cube, y = setup
    _check_kernels(m, 0.3, 0.4, 0)                                               # 32 x 48 x 48
    for Lc in (1, 2, 5):
        m2 = _awkward_model(Lc)
        try:
            assert tuple(m2.ishape) == (Lc, 72, 77)
            _check_kernels(m2, 0.3, 0.4, Lc)
            if Lc != 5:
                continue
            x_t = torch.zeros(m2.ishape, device="cuda:0")
            for bad in (0.0, -1.0, float("nan"), 1e-40):                         # 1e-40 does not survive the fp32 kernels
                for args in ((1.0, bad, 1.0, 1.0), (1.0, 1.0, 1.0, bad)):
                    with pytest.raises(RuntimeError):
                        _prior_dev(m2, x_t, x_t.clone(), *args)
                for args in ((bad, 1.0), (1.0, bad)):
                    with pytest.raises(RuntimeError):
                        _curv_dev(m2, x_t, x_t, x_t, *args)
            for args in ((float("nan"), 1.0, 1.0, 1.0), (1.0, 1.0, float("nan"), 1.0)):
                with pytest.raises(RuntimeError):
                    _prior_dev(m2, x_t, x_t.clone(), *args)
            assert _prior_dev(m2, x_t, x_t.clone(), 1.0, INF, 1.0, INF) == (0.0, 0.0)
        finally:
            m2.close()


@pytest.mark.parametrize("regime", list(vo.REGIMES))
def test_mmmg_vox_matches_oracle(setup, regime):
    om, m, cube, y = setup
    sr, ds, lr, dl, st, nit = vo.REGIMES[regime]
    x0 = vo.start(st, om, cube)
    ref = vo.mmmg(om, y, MU, sr, ds, lr, dl, x0, max_iter=nit)
    x, gn, n = m.mmmg_vox(y, mu=MU, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=nit)
    pv = m.huber_prior_values
    xq, _, _ = m.mmmg_vox(y, mu=MU, spat_reg=sr, spat_delta=INF, spec_reg=lr, spec_delta=INF, x0=x0, max_iter=nit)
    gr = np.array(ref["grad_norm"])
    ex, eg = rel(x, ref["x"]), float(np.max(np.abs(gn - gr) / gr))
    want_pv = vo.prior_values(x, ds, dl)
    epv = [abs(pv[f] - want_pv[f]) / want_pv[f] for f in range(2)]
    print(f"{regime}: shares {vo.shares(x, ds, dl)}, device vs oracle: x {ex:.2e}, grad_norm {eg:.2e}, prior values {epv}; "
          f"device Huber vs quadratic {rel(x, xq):.1e}")
    assert rel(x, xq) > 20 * vo.X_TOL_BOUND                                     # the Huber branches are in play on the device too
    assert n == nit and gn.shape == (nit + 1,)
    assert ex < vo.X_TOL_BOUND and eg < vo.G_TOL_BOUND
    assert max(epv) < 1e-5
    if regime == "both":        # the refresh period changes rounding only
        xf, _, _ = m.mmmg_vox(y, mu=MU, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=nit, refresh=1)
        print(f"refresh = 1 against refresh = 50: {rel(xf, x):.2e}")
        assert rel(xf, x) < vo.X_TOL_BOUND


def test_infinite_deltas_solve_the_quadratic_problem(setup):
    """Both thresholds infinite: the quadratic solve of the cube-domain operator, against orc.mmmg with the spectral term off and
    against the oracle with it on; a weight of 0 switches its family off."""
    om, m, cube, y = setup
    x0 = vo.start("rough", om, cube)
    ref = orc.mmmg(om, y, MU, 40.0, x0, max_iter=8)
    x, gn, n = m.mmmg_vox(y, mu=MU, spat_reg=40.0, spat_delta=INF, spec_reg=0.0, spec_delta=INF, x0=x0, max_iter=8)
    gr = np.array(ref["grad_norm"])
    assert n == 8 and rel(x, ref["x"]) < vo.X_TOL_BOUND and float(np.max(np.abs(gn - gr) / gr)) < vo.G_TOL_BOUND
    x2, _, _ = m.mmmg_vox(y, mu=MU, spat_reg=40.0, spat_delta=INF, spec_reg=0.0, spec_delta=0.01, x0=x0, max_iter=8)
    assert rel(x2, x) == 0.0                                                     # a switched-off family's threshold is idle


def test_criterion_descends_and_stops(setup):
    from surfh_amd.algorithms import vox_criterion
    om, m, cube, y = setup
    sr, ds, lr, dl, st, nit = vo.REGIMES["both"]
    x0 = vo.start(st, om, cube)
    js = []
    x, gn, n = m.mmmg_vox(y, mu=MU, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=40,
                          callback=lambda it, g, xx: js.append(vox_criterion(y, m, xx, sr, ds, lr, dl)) and False)
    js = np.array([vox_criterion(y, m, x0, sr, ds, lr, dl)] + js)
    assert n == 40 and len(js) == 41
    assert np.all(np.diff(js) <= 1e-6 * js[:-1]) and js[-1] < js[0]              # MM: non-increasing up to fp32 noise
    jr = vo.crit(om, y, vo.mmmg(om, y, MU, sr, ds, lr, dl, x0, max_iter=4)["x"], MU, sr, ds, lr, dl)
    assert abs(js[4] - jr) < 1e-5 * jr
    # early stop through the callback, tolerance stop
    kw = dict(mu=MU, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=nit)
    seen = []
    x3, g3, n3 = m.mmmg_vox(y, callback=lambda it, g, xx: seen.append(it) or it == 3, **kw)
    x8, g8, _ = m.mmmg_vox(y, **kw)
    assert n3 == 3 and seen == [1, 2, 3] and np.array_equal(g3, g8[:4])
    xt, gt, nt = m.mmmg_vox(y, tol=g8[4] * 1.0001 / x8.size, **kw)
    assert nt == 4 and np.array_equal(gt, g8[:5])


def test_vox_reconstruction_and_guard_rails(setup):
    from surfh_amd.algorithms import vox_reconstruction
    om, m, cube, y = setup
    sr, ds, lr, dl, st, nit = vo.REGIMES["both"]
    x0 = vo.start(st, om, cube)
    x, gn, _ = m.mmmg_vox(y, mu=1.0, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0, max_iter=nit, tol=1e-4)
    r = vox_reconstruction(y, m, spat_reg=sr, spat_th=ds, spec_reg=lr, spec_th=dl, init=x0, max_iter=nit)
    assert r.nit == nit and rel(r.x.reshape(m.ishape), x) == 0.0 and np.array_equal(r.grad_norm, gn)
    r0 = vox_reconstruction(y, m, spat_reg=sr, spat_th=ds, spec_reg=lr, spec_th=dl, max_iter=3)
    x1, _, _ = m.mmmg_vox(y, mu=1.0, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=m.adjoint(y), max_iter=3, tol=1e-4)
    assert rel(r0.x.reshape(m.ishape), x1) == 0.0
    # the map-domain Huber solver still refuses a template-free model, in its own words; the voxel solver refuses templates
    with pytest.raises(RuntimeError, match="needs templates"):
        m.mmmg(y, mu=1.0, mu_reg=1.0, x0=x0, max_iter=2, delta=0.1)
    mt = build_model(problems.config1())
    try:
        with pytest.raises((ValueError, RuntimeError)):
            mt.mmmg_vox(np.zeros(mt.osize), max_iter=1)
        import torch
        z = torch.zeros(mt.ishape, device="cuda:0")
        with pytest.raises(RuntimeError, match="without templates"):
            mt.huber_vox_prior_dev(z, z.clone(), 1.0, 1.0, 1.0, 1.0)
    finally:
        mt.close()


def test_config2_size_template_free():
    """A few iterations on the config-2 problem built without templates (1024 x 251 x 251, band 2A) from a textured start: the
    criterion decreases with both branches of both potentials in play; prints the device time per iteration and the profile lines of
    the two prior kernels next to mmmg_update and the rest of an iteration."""
    from surfh_amd import synth
    from surfh_amd.algorithms import vox_criterion
    from surfh_amd.models import spectroSigRLSCT
    prob = synth.config2()
    m = spectroSigRLSCT(prob["sotf"], None, prob["alpha_axis"], prob["beta_axis"], prob["wavel"], prob["ifus"], prob["step_deg"],
                        prob["pointings"])
    try:
        cube = np.tensordot(prob["templates"].T, prob["maps"], 1)
        assert cube.shape == m.ishape == (1024, 251, 251)
        y = m.forward(cube)
        x0 = cube + 0.1 * np.std(cube) * np.random.default_rng(3).standard_normal(m.ishape)
        # thresholds at the medians of the start's differences: half of each family beyond, by construction of the input
        ds = float(np.median(np.abs(np.concatenate([orc.diff_r(x0).ravel(), orc.diff_c(x0).ravel()]))))
        dl = float(np.median(np.abs(vo.diff_l(x0))))
        # weights that balance each family's gradient against the data gradient at the start (also a property of the input):
        # strong enough to act within a few iterations, not so strong that they flatten every difference below its threshold
        gd = np.linalg.norm(m.adjoint(m.forward(x0) - y))
        sr = float(gd / np.linalg.norm(ho.prior_grad(x0, ds)))
        lr = float(gd / np.linalg.norm(vo.diff_l_t(vo.dphi(vo.diff_l(x0), dl))))
        kw = dict(mu=1.0, spat_reg=sr, spat_delta=ds, spec_reg=lr, spec_delta=dl, x0=x0)
        m.mmmg_vox(y, max_iter=1, **kw)                                          # warm-up
        k = 4
        x, gn, n = m.mmmg_vox(y, max_iter=k, **kw)
        s_spat, s_spec = vo.shares(x, ds, dl)
        j0, j1 = vox_criterion(y, m, x0, sr, ds, lr, dl), vox_criterion(y, m, x, sr, ds, lr, dl)
        print(f"shares {s_spat:.2f} {s_spec:.2f}, criterion {j0:.6e} -> {j1:.6e}, delta {ds:.3e} {dl:.3e}, reg {sr:.3e} {lr:.3e}")
        assert n == k and j1 < j0 and 0.1 < s_spat < 0.9 and 0.1 < s_spec < 0.9
        nvox = float(np.prod(m.ishape))
        m.profile_enable(True)
        m.profile_reset()
        m.mmmg_vox(y, max_iter=k, **kw)
        prof = m.profile()
        m.profile_enable(False)
        rest = sum(ms for name, (_, ms) in prof.items() if name not in ("huber_vox_grad", "huber_vox_curv", "mmmg_update"))
        for name, byt in (("huber_vox_grad", 12), ("huber_vox_curv", 12), ("mmmg_update", 40)):
            cnt, ms = prof[name]
            print(f"profile {name}: {cnt} launches, {ms / cnt:.3f} ms each, {byt * nvox / (ms / cnt) / 1e6:.0f} GB/s algorithmic")
        print(f"profile all other stages (operator, dots): {rest / k:.2f} ms per iteration; "
              f"whole iteration {sum(ms for _, ms in prof.values()) / k:.2f} ms (device events, every stage bracketed)")
    finally:
        m.close()


def test_driver_writes_voxel_results(tmp_path):
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(ROOT, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    r = CliRunner().invoke(drv.main, ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "3", "--synthetic", "small", "--voxel",
                                      "--method", "mmmg", "--delta", "0.1", "--spec_reg", "5e3", "--spec_delta", "0.1"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("mmmg", 1, 0, 3, 5e3, False, 0.1, voxel=True)
    assert d.name.endswith("_vox")
    cube, crit = np.load(d / "res_cube.npy"), np.load(d / "criterion.npy")
    assert cube.shape == (256, 251, 251) and np.isfinite(cube).all() and crit.shape == (2,) and crit[1] < crit[0]   # the start, iteration 1
