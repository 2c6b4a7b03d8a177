"""GPU parity of the operator variants on the hot path: nearest-neighbour gridding
(spectroModelChannel.py:201-212, 391-415) and the 2-D no-rotation operator MRSBlurred
(spectro_blind_rectangle.py)."""
import os

import numpy as np
import pytest

import problems
from helpers import build_model, make_ifu, rel
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-5


@pytest.mark.parametrize("mode", ["nn", "nn_ref"])
def test_nn_gridding(mode):
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct", gridding=mode)
    m = build_model(cfg, gridding=mode)
    u = np.random.default_rng(1).standard_normal(om.osize)
    e = dict(fwd=rel(m.forward(cfg["maps"]), om.forward(cfg["maps"])),
             adj=rel(m.adjoint(u), om.adjoint(u)),              # scatter-add transpose of the index gather
             adj_ref=rel(m.adjoint_ref(u), om.adjoint_ref(u)))  # NN_gridding_t: gather back, no support mask
    print(mode, e)
    assert max(e.values()) < TOL
    rng = np.random.default_rng(2)
    v, uu = rng.random(m.isize), rng.random(m.osize)
    l = float(np.vdot(m.rmatvec(uu), v)); r = float(np.vdot(uu, m.matvec(v)))
    assert abs(l - r) / abs(r) < 1e-6
    m.close()


def blurred_case(L=None, N=96):
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    wav = np.array([7.6]) if L is None else np.linspace(7.0, 8.2, L)
    sotf = orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (N, N))
    if L is None:
        sotf = sotf[0]
    s = problems.STEP_DEG
    pts = [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s)]
    bo = orc.BlurredOracle(sotf, ax, ax, spec, s, pts)
    m = MRSBlurred(sotf, ax, ax, make_ifu(spec), s, instru.CoordList([instru.Coord(a, b) for a, b in pts]))
    return N, bo, m


def test_mrs_blurred_single_image_vs_reference():
    N, bo, m = blurred_case()
    g = np.load(os.path.join(G, "mrs_blurred.npz"))
    assert m.slices_shape == bo.slices_shape == (3, 12, 6)
    assert np.array_equal([[a.start, a.stop, b.start, b.stop] for a, b in (m.get_slit_slices(k) for k in range(12))],
                          g["slit_slices"])                                           # index path: bit-exact
    assert np.array_equal([m.get_slit_weights(k, m.get_slit_slices(k))[0][0] for k in range(12)], g["slit_w"])
    x = np.random.default_rng(int(g["x_seed"])).random((N, N))
    u = np.random.default_rng(int(g["u_seed"])).standard_normal(m.osize)
    e = dict(fwd=rel(m.forward(x), g["y"]), adj=rel(m.adjoint(u), g["adjoint"]))      # the real reference's outputs
    print(e)
    assert max(e.values()) < TOL
    rng = np.random.default_rng(7)
    v, uu = rng.random(m.isize), rng.random(m.osize)
    l = float(np.vdot(m.rmatvec(uu), v)); r = float(np.vdot(uu, m.matvec(v)))
    assert abs(l - r) / abs(r) < 1e-6
    m.close()


def test_mrs_blurred_data_to_img_vs_reference():
    """The quick-look back-projection ``MRSBlurred.data_to_img`` (spectro_blind_rectangle.py:240-283) of the product class against
    the reference's own output (tests/golden/mrs_blurred_d2i.npz), on data the HIP forward produced from the same image."""
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    from test_oracle_golden import d2i_case
    g = np.load(os.path.join(G, "mrs_blurred_d2i.npz"))
    N, ax, spec, sotf, s, pts = d2i_case()
    m = MRSBlurred(sotf, ax, ax, make_ifu(spec), s, instru.CoordList([instru.Coord(a, b) for a, b in pts]))
    try:
        wm, gl = m.data_to_img(g["y"])
        assert np.array_equal(gl != 0, g["covered"])
        assert rel(gl, g["global_img"]) < 1e-13 and rel(wm, g["weighted_mean"]) < 1e-13
        x = np.random.default_rng(int(g["x_seed"])).random((N, N)) * np.linspace(0.0, 3.0, N)[None, :]
        y = m.forward(x)
        assert rel(y, g["y"]) < TOL
        wm2, gl2 = m.data_to_img(y)                                   # fp32 data: the threshold may flip a pixel at its edge
        assert np.mean((gl2 != 0) != g["covered"]) < 1e-3 and rel(gl2, g["global_img"]) < 1e-3
    finally:
        m.close()


def test_mrs_blurred_batched_over_wavelength():
    N, bo, m = blurred_case(L=40)
    x = np.random.default_rng(1).random((40, N, N))
    u = np.random.default_rng(2).standard_normal(m.oshape)
    e = dict(fwd=rel(m.forward(x), bo.forward(x)), adj=rel(m.adjoint(u), bo.adjoint(u)))
    print(e)
    assert m.forward(x).shape == (40, 3 * 12 * 6)
    assert max(e.values()) < TOL
    m.close()


def test_model_wct_vs_reference():
    """Fourier-domain fused W.C.T operator (mixing.py:131-272) against the reference's own outputs."""
    from surfh_amd.mixing import Model_WCT
    src = open(os.path.join(G, "make_golden.py")).read()
    ns = {}
    exec(src[src.index("def wct_inputs"):src.index("def wct():")], {"problems": problems, "np": np}, ns)
    psfs, specs, shape, pce, x, y = ns["wct_inputs"]()
    g = np.load(os.path.join(G, "model_wct.npz"))
    m = Model_WCT(psfs, specs, shape, pce)
    assert m.ishape == (3, 40, 36) and m.oshape == (24, 40, 36)
    e = dict(fwd=rel(m.forward(x), g["forward"]), adj=rel(m.adjoint(y), g["adjoint"]), fwadj=rel(m.fwadj(x), g["fwadj"]))
    print(e)
    assert max(e.values()) < TOL
    assert rel(m.fwadj(x), m.adjoint(m.forward(x))) < 1e-5
    m.close()


def test_explicit_inverse_solver_vs_reference():
    """QuadCriterion3.run_expsol (fusion_mixing.py:261-438) against the reference's own output."""
    from surfh_amd.mixing import Model_WCT, QuadCriterion3
    src = open(os.path.join(G, "make_golden.py")).read()
    ns = {}
    exec(src[src.index("def wct_inputs"):src.index("def wct():")], {"problems": problems, "np": np}, ns)
    psfs, specs, shape, pce, x, y = ns["wct_inputs"]()
    g = np.load(os.path.join(G, "model_wct.npz"))
    m = Model_WCT(psfs, specs, shape, pce)
    r1 = QuadCriterion3(y, m, 0.7, gradient="separated").run_expsol()
    r2 = QuadCriterion3(y, m, list(g["mu_list"]), gradient="separated").run_expsol()
    e = dict(scalar=rel(r1, g["expsol"]), per_map=rel(r2, g["expsol_mu_list"]))
    print(e)
    assert r1.shape == (3, 40, 36) and max(e.values()) < TOL
    # "joint" prior (Laplacian kernel restated from udft: parity unpinned against the reference) vs the float64 oracle
    wo = orc.WCTOracle(psfs, specs, shape, pce)
    assert rel(QuadCriterion3(y, m, 0.7, gradient="joint").run_expsol(), wo.expsol(y, 0.7, "joint")) < TOL
    # the closed form is the fixed point of the regularised CG: one application of the normal operator gives H^T y back
    lhs = m.fwadj(r1) + 0.7 * (orc.diff_r_t(orc.diff_r(r1)) + orc.diff_c_t(orc.diff_c(r1)))
    assert rel(lhs, m.adjoint(y)) < 1e-4
    # singular system: mu = 0 and a spectrum basis that is rank deficient -> LinAlgError like numpy.linalg.inv
    specs2 = specs.copy()
    specs2[2] = specs2[0] + specs2[1]
    m2 = Model_WCT(psfs, specs2, shape, pce)
    with pytest.raises(np.linalg.LinAlgError):
        QuadCriterion3(y, m2, 0.0).run_expsol()
    m.close()
    m2.close()


def _variant_problem(n_alpha, n_beta, n_templates, Lc=96):
    """A config-1-like problem on a rectangular image with `n_templates` abundance maps."""
    rng = np.random.default_rng(31)
    ax_a = orc.synthetic_axes(n_alpha, problems.STEP_DEG)
    ax_b = orc.synthetic_axes(n_beta, problems.STEP_DEG)
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(0.8 / 3600, 0.9 / 3600, (0.0, 0.0), 8.2, 0.196, 4, 3050.0, np.linspace(7.53, 7.67, 40), "S1")
    tpl = rng.random((n_templates, Lc)) + 0.5
    sotf = orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (n_alpha, n_beta))
    pts = orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)
    return dict(N=n_alpha, Lc=Lc, alpha_axis=ax_a, beta_axis=ax_b, wavel=wav, specs=[spec], templates=tpl, sotf=sotf,
                pointings=[pts], maps=rng.random((n_templates, n_alpha, n_beta)), step_deg=problems.STEP_DEG)


@pytest.mark.parametrize("na,nb,T", [(72, 64, 4), (64, 80, 6), (66, 66, 1)], ids=["rect_72x64", "rect_64x80_T6", "one_template"])
def test_rectangular_images_and_template_counts(na, nb, T):
    """Image axes of different lengths and template counts other than 4 (the reference driver also runs with 6:
    scripts/main_fusion.py:88-93; more than 4 templates take the un-fused spectral mix)."""
    cfg = _variant_problem(na, nb, T)
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    rng = np.random.default_rng(2)
    try:
        assert m.ishape == (T, na, nb)
        y = m.forward(cfg["maps"])
        u = rng.random(y.shape)
        e = dict(fwd=rel(y, om.forward(cfg["maps"])), adj=rel(m.adjoint(u), om.adjoint(u)))
        print(na, nb, T, e)
        assert max(e.values()) < TOL
        x, gn, nit = m.cg(y, mu=1.0, mu_reg=10.0, max_iter=5)
        assert nit == 5 and gn[-1] < gn[0] and x.shape == (T, na, nb)
    finally:
        m.close()


@pytest.mark.parametrize("T", [5, 8], ids=["first_unfused_count", "max_templates"])
def test_template_counts_on_the_unfused_mix(T):
    """T = 5 is the first count on the un-fused spectral mix, T = 8 = SURFH_MAX_TEMPLATES the last one a plan takes: forward and
    both adjoints on every local measure at TOL, no spectral-domain solver, and five CG iterations against the float64 oracle at
    the bounds of test_gpu_parity.test_cg_matches_oracle_lcg (iterate 3e-3, every r.r of the trace 2e-4)."""
    from test_gpu_local_parity import FWD_AXES, MAP_AXES, check_local
    from test_gpu_parity import note
    cfg = _variant_problem(66, 66, T)
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    rng = np.random.default_rng(2)
    try:
        assert m.ishape == (T, 66, 66) and not m.spec_supported()
        yo = om.forward(cfg["maps"])
        check_local("template_count_forward", m.forward(cfg["maps"]).reshape(om.channels[0].oshape), yo.reshape(om.channels[0].oshape),
                    FWD_AXES, T=T)
        u = rng.random(om.osize)
        check_local("template_count_adjoint", m.adjoint(u), om.adjoint(u), MAP_AXES, T=T)
        check_local("template_count_adjoint_ref", m.adjoint_ref(u), om.adjoint_ref(u), MAP_AXES, T=T)
        y = yo + np.random.default_rng(1).standard_normal(yo.size) * 1e-2 * np.sqrt(np.mean(yo ** 2))
        mu, mur, nit = 1.0, 5e3, 5
        ref = orc.lcg(om, y, mu, mur, np.zeros(om.ishape), tol=1e-12, max_iter=nit)
        x, gn, n = m.cg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit, tol=1e-12)
        gr = np.array(ref["grad_norm"])
        e, ge = rel(x, ref["x"]), float(np.max(np.abs(gn - gr) / gr))
        note("template_count_cg", T=T, err_x=e, err_gradnorm=ge, nit=n)
        print(f"T = {T}: five CG iterations, iterate {e:.2e}, r.r trace {ge:.2e}")
        assert n == nit and len(gn) == nit + 1
        assert e < 3e-3 and ge < 2e-4, (e, ge)
    finally:
        m.close()


def test_nine_templates_are_refused():
    cfg = _variant_problem(66, 66, 9)
    with pytest.raises(ValueError, match="at most 8 templates"):
        build_model(cfg)


def test_masked_mixing_model_vs_reference():
    """MixingST (mixing.py:276-337) against the outputs of the reference's own Cython kernels."""
    from surfh_amd.mixing import MixingST
    src = open(os.path.join(G, "make_golden.py")).read()
    ns = {}
    exec(src[src.index("def mixing_st_inputs"):src.index("def mixing_st():")], {"np": np}, ns)
    tpl, (na, nb), L, sel, fast, maps, cube = ns["mixing_st_inputs"]()
    g = np.load(os.path.join(G, "mixing_st.npz"))
    m = MixingST(tpl, np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), sel, fast)
    assert m.ishape == (3, na, nb) and m.oshape == (L, na, nb)
    e = dict(fwd=rel(m.forward(maps), g["forward"]), adj=rel(m.adjoint(cube), g["adjoint"]), fwadj=rel(m.fwadj(maps), g["fwadj"]))
    print(e)
    assert max(e.values()) < 1e-6
    assert np.array_equal(m.forward(maps) == 0, g["forward"] == 0)
    assert rel(m.mapsToCube(maps), np.tensordot(tpl.T, maps, axes=(1, 0))) < 1e-12
    # a voxel listed twice counts twice (the reference's +=); an empty list gives zeros
    dup = np.concatenate([fast, fast[:50]])
    m2 = MixingST(tpl, np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), None, dup)
    f1, f2 = m.forward(maps), m2.forward(maps)
    idx = tuple(fast[:50].T)
    assert np.allclose(f2[idx], 2 * f1[idx], rtol=1e-6) and rel(m2.adjoint(cube), m.adjoint(cube) + orc.MixingSTOracle(tpl, (na, nb), sel, fast[:50]).adjoint(cube)) < 1e-6
    with pytest.raises(RuntimeError):
        m2.fwadj(maps)                                      # no mask given -> no TST
    m3 = MixingST(tpl, np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), sel, np.zeros((0, 3), dtype=int))
    assert not m3.forward(maps).any() and not m3.adjoint(cube).any()
    with pytest.raises(ValueError):
        MixingST(tpl, np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), sel, np.array([[L, 0, 0]]))
    for mm in (m, m2, m3):
        mm.close()


class _PlaneOp:
    """One plane of the 2-D oracle presented as a [1, N, N] operator (the checker's lcg and priors act on [T, N, N])."""
    def __init__(self, bo):
        self.bo = bo
    def forward(self, x):
        return self.bo.forward(x[0])
    def adjoint(self, y):
        return self.bo.adjoint(y)[None]


def test_plane_wise_cg_2d_deconvolution():
    """SURVEY.md 8f-3 (solver part): regularised least squares by CG on the 2-D model, one independent problem per plane
    (criterion_2D.py:66-250 with qmm.lcg restated -- parity unpinned like the fusion solver, checked against the float64
    restatement plane by plane)."""
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred, QuadCriterion_MRS_2D
    L = 5
    N, bo, m = blurred_case(L=L)
    rng = np.random.default_rng(4)
    truth = rng.random((L, N, N))
    y = bo.forward(truth)
    y[3] = 0.0                                                # a plane without data must stay at rest (no 0/0)
    mu, mur, nit = 1.0, 0.05, 10
    x, gn, n = m.cg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit)
    assert n == nit and gn.shape == (nit + 1, L) and x.shape == (L, N, N)
    assert not x[3].any() and not gn[:, 3].any() and np.isfinite(x).all()
    # per-plane oracle: the same plane solved alone in float64
    wav = np.linspace(7.0, 8.2, L)
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    s_ = problems.STEP_DEG
    pts = [(0.0, 0.0), (2 * s_, -3 * s_), (-4 * s_, 1 * s_)]
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    for l in (0, 2, 4):
        sotf_l = orc.ir2fr(orc.gaussian_psf(wav[l:l + 1], problems.STEP), (N, N))[0]
        op = _PlaneOp(orc.BlurredOracle(sotf_l, ax, ax, spec, s_, pts))
        ref = orc.lcg(op, y[l], mu, mur, np.zeros((1, N, N)), tol=1e-12, max_iter=nit)
        gr = np.array(ref["grad_norm"])
        assert rel(x[l], ref["x"][0]) < 5e-3, l
        assert float(np.max(np.abs(gn[:5, l] - gr[:5]) / gr[:5])) < 1e-2 and gn[-1, l] < 1e-2 * gn[0, l]
    # the single-image model solves its plane to the same iterate
    sotf2 = orc.ir2fr(orc.gaussian_psf(wav[2:3], problems.STEP), (N, N))[0]
    m1 = MRSBlurred(sotf2, ax, ax, make_ifu(spec), s_, instru.CoordList([instru.Coord(a, b) for a, b in pts]))
    x1, gn1, _ = m1.cg(y[2], mu=mu, mu_reg=mur, max_iter=nit)
    assert x1.shape == (N, N) and gn1.shape == (nit + 1,) and rel(x1, x[2]) < 1e-4 and np.allclose(gn1, gn[:, 2], rtol=1e-3)
    # the criterion mirror
    crit = QuadCriterion_MRS_2D(mu, y[2], m1, mur)
    res = crit.run_method("lcg", maximum_iterations=nit, value_init=0.0)
    assert res.nit == nit and rel(res.x.reshape(N, N), x1) < 1e-6
    assert crit.get_crit_val(res.x) < crit.get_crit_val(np.zeros((N, N)))
    # 3MG, which the 2-D deconvolution driver selects with method = "qmm" (deconvolution_mrs_noRotation.py:199-212):
    # same iterates as CG on this quadratic criterion, plane by plane; |grad| instead of r.r in the trace
    xm, gm, nm = m.mmmg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit)
    assert nm == nit and gm.shape == (nit + 1, L) and not xm[3].any() and not gm[:, 3].any() and np.isfinite(xm).all()
    live = [0, 1, 2, 4]
    assert rel(xm[live], x[live]) < 1e-4 and float(np.max(np.abs(gm[:, live] ** 2 - gn[:, live]) / gn[:, live])) < 1e-3
    for l in (0, 4):
        sotf_l = orc.ir2fr(orc.gaussian_psf(wav[l:l + 1], problems.STEP), (N, N))[0]
        op = _PlaneOp(orc.BlurredOracle(sotf_l, ax, ax, spec, s_, pts))
        ref = orc.mmmg(op, y[l], mu, mur, np.zeros((1, N, N)), max_iter=nit)
        k = 7       # the float64 restatement itself leaves the CG path later (numpy pinv cut, see test_gpu_driver)
        assert float(np.max(np.abs(gm[:k, l] - ref["grad_norm"][:k]) / np.array(ref["grad_norm"][:k]))) < 1e-3, l
    res = crit.run_method("qmm", maximum_iterations=nit, value_init=0.0)
    xm1, gm1, _ = m1.mmmg(y[2], mu=mu, mu_reg=mur, x0=np.zeros((N, N)), max_iter=nit)
    assert res.nit == nit and rel(res.x.reshape(N, N), xm1) == 0.0 and rel(xm1, xm[2]) < 1e-4 and gm1.shape == (nit + 1,)
    m.close()
    m1.close()


@pytest.mark.parametrize("native", ["1", "0"], ids=["wavelength_innermost_vectors", "plane_major_vectors"])
def test_plane_wise_cg_device_resident_loop(native, monkeypatch):
    """``surfh_cg_planes_begin_dev / _step_dev / _rr`` (what bench.py --config 5 times): data and iterate stay on the device, no
    host synchronisation inside; the same iterates as ``surfh_cg_planes`` from host buffers, stepped in uneven blocks across a
    residual refresh.  By default the loop keeps its vectors in the cube's wavelength-innermost layout (no layout transpose inside
    an iteration, the prior fused into the d.q kernel; sums in another order: fp32-level agreement); SURFH_PLANES_NATIVE=0 runs the
    kernels of ``surfh_cg_planes`` on the caller's layout (same bits)."""
    import torch
    monkeypatch.setenv("SURFH_PLANES_NATIVE", native)
    L = 6
    N, bo, m = blurred_case(L=L)
    try:
        rng = np.random.default_rng(14)
        y = bo.forward(rng.random((L, N, N)))
        y[4] = 0.0
        mu, mur, nit, refresh = 1.0, 0.05, 9, 4
        x_ref, gn_ref, n = m.cg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit, refresh=refresh)
        dev = torch.device("cuda:0")
        yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32).reshape(-1), device=dev)
        xt = torch.zeros((L, N, N), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.cg_begin_dev(yt, xt, mu, mur)
        assert np.allclose(m.cg_rr(), gn_ref[0], rtol=1e-6)
        for block in (2, 3, 4):
            m.cg_step_dev(block, refresh)
        rr = m.cg_rr()
        x = xt.cpu().numpy()
        if native == "0":
            assert np.array_equal(x, np.asarray(x_ref, dtype=np.float32)) and np.array_equal(rr, gn_ref[-1])     # same kernels, same order
        else:
            live = [0, 1, 2, 3, 5]
            e_x, e_r = rel(x[live], x_ref[live]), float(np.max(np.abs(rr[live] - gn_ref[-1][live]) / gn_ref[-1][live]))
            print(f"plane-wise CG on wavelength-innermost vectors vs plane-major: x {e_x:.1e}, r.r {e_r:.1e}")
            assert e_x < 1e-4 and e_r < 1e-2
        assert not x[4].any() and rr[4] == 0.0
    finally:
        m.close()


def test_plane_wise_model_on_the_cooley_tukey_passes(monkeypatch):
    """The 2-D deconvolution path at an image size of the Cooley-Tukey passes (300 = 2 x 150; the benchmark's 512 x 512 is
    tests/test_gpu_fullsize.py): forward and adjoint against the oracle; by default the OTF products are formed in the loader
    of the inverse transforms (dft_ct.h PROD / PRODADD -- inside the normal operator with mu and the quadratic prior riding on
    the adjoint's pass), SURFH_OTF_PROD=0 keeps the separate product kernels: same results to fp32 rounding, different bits, and
    the same iterates of the device-resident solver."""
    import torch
    L, mu, mur, nit = 5, 1.3, 0.07, 6
    res = {}
    for prod in ("1", "0"):
        monkeypatch.setenv("SURFH_OTF_PROD", prod)
        N, bo, m = blurred_case(L=L, N=300)
        try:
            rng = np.random.default_rng(21)
            x = rng.random((L, N, N))
            u = rng.standard_normal((L,) + tuple(bo.slices_shape)).reshape(L, -1)
            yf, ya = m.forward(x), m.adjoint(u)
            ef, ea = rel(yf, bo.forward(x)), rel(ya, bo.adjoint(u))
            assert ef < TOL and ea < TOL, (prod, ef, ea)
            y = bo.forward(x) + 1e-2 * rng.standard_normal(yf.shape)
            xh, gn, n = m.cg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit, refresh=4)
            dev = torch.device("cuda:0")
            yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32).reshape(-1), device=dev)
            xt = torch.zeros((L, N, N), dtype=torch.float32, device=dev)
            m.cg_begin_dev(yt, xt, mu, mur)
            m.cg_step_dev(nit, 4)
            res[prod] = (yf, ya, xh, gn, xt.cpu().numpy(), m.cg_rr())
        finally:
            m.close()
    a, b = res["1"], res["0"]
    assert rel(a[0], b[0]) < 2e-6 and rel(a[1], b[1]) < 2e-6 and not np.array_equal(a[0], b[0])      # the switch engaged
    assert rel(a[2], b[2]) < 1e-4 and rel(a[4], b[4]) < 1e-4                                        # six CG iterations either way
    assert rel(a[4], a[2]) < 1e-4 and float(np.max(np.abs(a[5] - a[3][-1]) / a[3][-1])) < 1e-2       # device loop = host-buffer solver


def test_slice_cube_projections():
    """the reference's slice <-> cube projections (spectroModelChannel.py:266-336) through
    ``model.channels[k]``, against the golden vectors of the real reference and the oracle."""
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    g1 = np.load(os.path.join(G, "config1_chain.npz"))
    g = np.load(os.path.join(G, "channel_projections.npz"))
    m = build_model(cfg)
    ch = m.channels[0]
    y = g1["y"]
    s2c = ch.sliceToCube(y)
    ref = orc.slice_to_cube(om.channels[0], y, cfg["alpha_axis"], cfg["beta_axis"], len(cfg["wavel"]))
    assert s2c.shape == ref.shape == (len(cfg["wavel"]), 64, 64)
    e = dict(s2c=rel(s2c, ref), s2c_gold=rel(s2c[g["sel"]], g["s2c_sel"]))
    assert np.array_equal(np.abs(s2c).sum(axis=(1, 2)) > 0, g["s2c_abs_sums"] > 0)      # empty planes are exactly zero
    tab0 = orc.build_channel(cfg["specs"][0], cfg["alpha_axis"], cfg["beta_axis"], cfg["wavel"], cfg["step_deg"], [(0.0, 0.0)])
    cube = np.random.default_rng(int(g["cube_seed"])).random((ch.oshape[2], 64, 64))
    c2s = ch.realData_cubeToSlice(cube)
    assert c2s.shape == g["c2s"].shape
    e.update(c2s=rel(c2s, orc.realdata_cube_to_slice(tab0, cube)), c2s_gold=rel(c2s, g["c2s"]))
    back = ch.realData_sliceToCube(g["c2s"], cube.shape)
    e.update(back=rel(back, orc.realdata_slice_to_cube(tab0, g["c2s"], cube.shape, cfg["alpha_axis"], cfg["beta_axis"])),
             back_gold=rel(back[g["sel_rd"]], g["s2c_rd_sel"]))
    print(e)
    assert max(e.values()) < TOL
    with pytest.raises(ValueError):
        ch.realData_cubeToSlice(cube[1:])
    # the operator itself is untouched by the auxiliary plans
    assert rel(m.forward(cfg["maps"]), y) < TOL
    m.close()
