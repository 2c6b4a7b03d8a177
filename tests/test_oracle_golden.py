"""The oracle against the golden vectors produced by the real reference
(tests/golden/make_golden.py).  CPU only; this is what pins the oracle."""
import os

import numpy as np
import pytest

import problems
from oracle import surfh_oracle as orc

G = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def c1():
    cfg = problems.config1()
    return cfg, problems.oracle_model(cfg), np.load(os.path.join(G, "config1_chain.npz"))


def check_tables(tab, g, pre):
    assert tab.srf == int(g[pre + "srf"])
    assert tuple(tab.wslice) == tuple(g[pre + "wslice"])
    assert np.array_equal(tab.local_alpha_axis, g[pre + "local_alpha_axis"])      # bit-exact
    assert np.array_equal(tab.local_beta_axis, g[pre + "local_beta_axis"])
    assert (tab.npix_slit_alpha_width, tab.npix_slit_beta_width) == tuple(g[pre + "npix_ab"])
    assert tuple(tab.oshape) == tuple(g[pre + "oshape"])
    assert np.array_equal(np.array(tab.slit_slices), g[pre + "slit_slices"])       # integer path: bit-exact
    assert np.array_equal([w[0, 0] for w in tab.slit_weights], g[pre + "slit_w_first"])
    assert np.array_equal([w[0, -1] for w in tab.slit_weights], g[pre + "slit_w_last"])
    assert np.array_equal(np.array(tab.pointings), g[pre + "pointings_pix"])
    assert np.array_equal(np.array(tab.origin_pix), g[pre + "origin_pix"])


def test_config1_tables_bit_exact(c1):
    cfg, om, g = c1
    tab = om.channels[0]
    check_tables(tab, g, "c0_")
    assert np.array_equal(tab.wpsf, g["wpsf"])
    for p in range(4):
        assert np.array_equal(np.stack(tab.grid_idx[p]), g[f"bil_idx_p{p}"])
        assert np.array_equal(np.stack(tab.grid_frac[p]), g[f"bil_frac_p{p}"])


def test_config1_forward_stages(c1):
    cfg, om, g = c1
    st = {}
    y = om.forward(cfg["maps"], stages=st)
    sel = g["lam_sel"]
    assert rel(st["blurred"][sel], g["blurred_sel"]) < 1e-13
    for p in range(4):
        assert rel(st["gridded"][p][sel], g[f"gridded_p{p}"]) < 1e-13
        assert rel(st["sum_cube"][p][sel], g[f"sum_cube_p{p}"]) < 1e-12
    assert rel(y, g["y"]) < 1e-13


def test_config1_adjoint_ref(c1):
    cfg, om, g = c1
    u = np.random.default_rng(int(g["u_seed"])).standard_normal(om.osize)
    st = {}
    a = om.adjoint_ref(u, stages=st)
    sel = g["lam_sel"]
    assert rel(st["local_cube"][0][sel], g["adj_local_cube_p0_sel"]) < 1e-13
    assert rel(st["sum_t"][0][sel], g["adj_sum_t_p0_sel"]) < 1e-12
    assert rel(st["degridded"][0][sel], g["adj_degridded_ref_p0_sel"]) < 1e-12
    assert rel(a, g["adjoint_ref"]) < 1e-12


def test_box_sum_is_window_sum(c1):
    cfg, om, g = c1
    tab = om.channels[0]
    x = np.random.default_rng(3).standard_normal((3, len(tab.local_alpha_axis), len(tab.local_beta_axis)))
    assert rel(orc.box_sum_direct(tab, x), orc.box_sum_fft(tab, x)) < 1e-13
    assert rel(orc.box_sum_direct_t(tab, x), orc.box_sum_fft_t(tab, x)) < 1e-13


def test_exact_adjoint_dottest(c1):
    cfg, om, g = c1
    assert orc.dottest_gap(om, np.random.default_rng(5)) < 1e-12
    # the reference's own pair is NOT adjoint: gap ~1e-3
    u = np.random.default_rng(1).standard_normal(om.osize)
    v = np.random.default_rng(2).standard_normal(om.isize)
    gap = abs(np.vdot(om.adjoint_ref(u).ravel(), v) - np.vdot(u, om.matvec(v))) / abs(np.vdot(u, om.matvec(v)))
    assert 1e-5 < gap < 1e-1


def test_two_channel_overlap():
    cfg = problems.two_channel_small()
    om = problems.oracle_model(cfg)
    g = np.load(os.path.join(G, "two_channel.npz"))
    assert np.array_equal(om._idx, g["idx"])
    for k, tab in enumerate(om.channels):
        check_tables(tab, g, f"c{k}_")
    assert rel(om.forward(cfg["maps"]), g["y"]) < 1e-13
    u = np.random.default_rng(int(g["u_seed"])).standard_normal(om.osize)
    assert rel(om.adjoint_ref(u), g["adjoint_ref"]) < 1e-12
    assert orc.dottest_gap(om, np.random.default_rng(6)) < 1e-12


def test_real_band_geometry_bit_exact():
    g = np.load(os.path.join(G, "bands_geometry.npz"))
    N = 251
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    lo, hi, n = g["axis_cfg4"]
    wav4 = np.linspace(lo, hi, int(n))
    for name in problems.BANDS:
        wa = g[f"{name}_wavel"]
        assert np.array_equal(problems.band_wavel(name), wa)
        spec = problems.band_spec(name, wavel_axis=wa)
        pts = orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)
        tab = orc.build_channel(spec, ax, ax, wav4, problems.STEP_DEG, pts, with_grid=(name == "2a"))
        check_tables(tab, g, f"{name}_")
        assert tuple(tab.wpsf.shape) == tuple(g[f"{name}_wpsf_shape"])
        assert np.array_equal(tab.wpsf[::97, ::53, :], g[f"{name}_wpsf_sample"])
        for k in ("cfg2", "cfg3"):
            lo2, hi2, n2 = g["axis_" + k]
            ws = orc.wslice_of(np.linspace(lo2, hi2, int(n2)), wa[0], wa[-1], 0.1)
            assert tuple(ws) == tuple(g[f"{name}_wslice_{k}"])
        if name == "2a":
            for p in range(4):
                assert np.array_equal(np.stack(tab.grid_idx[p])[:, ::5], g[f"2a_bil_idx_p{p}"])
                assert np.array_equal(np.stack(tab.grid_frac[p])[:, ::5], g[f"2a_bil_frac_p{p}"])


def test_lcg_matches_dense_solve():
    """qmm.lcg is absent (parity unpinned): pin the restated solver on a dense solve."""
    cfg = problems.two_channel_small()
    om = problems.oracle_model(cfg, box="direct")
    # shrink: dense normal matrix on a tiny operator built from a random projection of the oracle
    rng = np.random.default_rng(0)

    class Small:
        ishape = (2, 5, 6)
        A = rng.standard_normal((80, 60))

        def forward(self, x):
            return self.A @ x.ravel()

        def adjoint(self, y):
            return (self.A.T @ y).reshape(self.ishape)

    op = Small()
    y = rng.standard_normal(80)
    mu, mur = 1.0, 0.7
    res = orc.lcg(op, y, mu, mur, np.zeros(op.ishape), tol=1e-14, max_iter=200)
    n = 60
    Q = np.zeros((n, n))
    for k in range(n):
        e = np.zeros(n); e[k] = 1
        Q[:, k] = orc.normal_apply(op, e.reshape(op.ishape), mu, mur).ravel()
    xs = np.linalg.solve(Q, (mu * op.adjoint(y)).ravel())
    assert rel(res["x"].ravel(), xs) < 1e-9
    gn = res["grad_norm"]
    assert gn[-1] < gn[0] * 1e-12
    # criterion decreases monotonically along the iterates
    c = [orc.crit_val(op, y, orc.lcg(op, y, mu, mur, np.zeros(op.ishape), max_iter=k)["x"], mu, mur) for k in (1, 3, 6)]
    assert c[0] > c[1] > c[2]


def test_slice_cube_projections_match_reference(c1):
    """Channel.sliceToCube / realData_cubeToSlice / realData_sliceToCube (spectroModelChannel.py:266-336)."""
    cfg, om, g1 = c1
    g = np.load(os.path.join(G, "channel_projections.npz"))
    tab = om.channels[0]
    assert np.array_equal(tab.wpsf_dirac.sum(axis=1), g["wpsf_dirac_count"])          # one-hot selector: bit-exact
    assert np.array_equal(np.argmax(tab.wpsf_dirac, axis=1), g["wpsf_dirac_argmax"])
    s2c = orc.slice_to_cube(tab, g1["y"], cfg["alpha_axis"], cfg["beta_axis"], len(cfg["wavel"]))
    # the reference casts the repeated data to float32 before the spectral step (:283): 1e-7 is that rounding
    assert rel(s2c[g["sel"]], g["s2c_sel"]) < 2e-7 and rel(s2c.sum(axis=(1, 2)), g["s2c_plane_sums"]) < 2e-7
    assert np.array_equal(np.abs(s2c).sum(axis=(1, 2)) > 0, g["s2c_abs_sums"] > 0)     # only the peak planes receive data
    tab0 = orc.build_channel(cfg["specs"][0], cfg["alpha_axis"], cfg["beta_axis"], cfg["wavel"], cfg["step_deg"], [(0.0, 0.0)])
    cube = np.random.default_rng(int(g["cube_seed"])).random((tab0.oshape[2], 64, 64))
    c2s = orc.realdata_cube_to_slice(tab0, cube)
    assert c2s.shape == g["c2s"].shape and rel(c2s, g["c2s"]) < 1e-14
    back = orc.realdata_slice_to_cube(tab0, g["c2s"], cube.shape, cfg["alpha_axis"], cfg["beta_axis"])
    assert rel(back[g["sel_rd"]], g["s2c_rd_sel"]) < 1e-13 and rel(back.sum(axis=(1, 2)), g["s2c_rd_plane_sums"]) < 1e-13


def test_mmmg_matches_dense_solve_and_lcg_iterates():
    """qmm.mmmg is absent (parity unpinned): the restated 3MG reaches the dense solution, and on a quadratic criterion
    its iterates are those of linear CG (both minimise over the same Krylov subspaces)."""
    rng = np.random.default_rng(3)

    class Small:
        ishape = (2, 5, 6)
        A = rng.standard_normal((80, 60))

        def forward(self, x):
            return self.A @ x.ravel()

        def adjoint(self, y):
            return (self.A.T @ y).reshape(self.ishape)

    op = Small()
    y = rng.standard_normal(80)
    mu, mur = 1.3, 0.7
    x0 = rng.standard_normal(op.ishape)
    res = orc.mmmg(op, y, mu, mur, x0, tol=1e-14, max_iter=200)
    Q = np.zeros((60, 60))
    for k in range(60):
        e = np.zeros(60); e[k] = 1
        Q[:, k] = orc.normal_apply(op, e.reshape(op.ishape), mu, mur).ravel()
    xs = np.linalg.solve(Q, (mu * op.adjoint(y)).ravel())
    assert rel(res["x"].ravel(), xs) < 1e-9
    assert len(res["grad_norm"]) == res["nit"] + 1 and res["grad_norm"][-1] < 60 * 1e-14 * 10
    for k in (1, 2, 5, 9):
        a = orc.mmmg(op, y, mu, mur, x0, max_iter=k)
        b = orc.lcg(op, y, mu, mur, x0, max_iter=k)
        assert a["nit"] == k and rel(a["x"], b["x"]) < 1e-9
        assert abs(a["grad_norm"][-1] ** 2 - b["grad_norm"][-1]) < 1e-8 * b["grad_norm"][0]      # |grad| vs r.r


def test_nn_indices_match_reference_ckdtree():
    """NN gridding index tables (Channel.precompute_mask recipe) against the reference's cKDTree output."""
    cfg = problems.config1()
    g = np.load(os.path.join(G, "config1_nn_indices.npz"))
    tab = problems.oracle_model(cfg, gridding="nn_ref").channels[0]
    for p in range(4):
        assert np.array_equal(tab.nn_idx[p], g[f"nn_idx_p{p}"].ravel())          # integer path: bit-exact
        assert np.array_equal(tab.nn_idx_t[p], g[f"nn_idx_t_p{p}"].ravel())
    # the gather the reference performs with these indices reads the alpha/beta-TRANSPOSED pixel
    cube = np.random.default_rng(0).random((2, 64, 64))
    tab2 = problems.oracle_model(cfg, gridding="nn").channels[0]
    assert np.array_equal(orc.gridding(tab, cube, 0), orc.gridding(tab2, cube.transpose(0, 2, 1), 0))
    om = problems.oracle_model(cfg, box="direct", gridding="nn")
    assert orc.dottest_gap(om, np.random.default_rng(9)) < 1e-12


def test_mrs_blurred_oracle_vs_reference():
    """BlurredOracle against the reference's MRSBlurred outputs (tests/golden/mrs_blurred.npz)."""
    g = np.load(os.path.join(G, "mrs_blurred.npz"))
    N = 96
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    sotf = orc.ir2fr(orc.gaussian_psf(np.array([7.6]), problems.STEP), (N, N))[0]
    s = problems.STEP_DEG
    bo = orc.BlurredOracle(sotf, ax, ax, spec, s, [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s)])
    x = np.random.default_rng(int(g["x_seed"])).random((N, N))
    u = np.random.default_rng(int(g["u_seed"])).standard_normal(g["y"].size)
    assert np.array_equal(np.array(bo.slit_slices), g["slit_slices"])
    assert np.array_equal(np.array([w[0] for w in bo.slit_weights]), g["slit_w"])
    assert rel(bo.forward(x), g["y"]) < 1e-13 and rel(bo.adjoint(u), g["adjoint"]) < 1e-13
    v = np.random.default_rng(5).standard_normal(x.shape)
    assert abs(np.vdot(bo.adjoint(u), v) - np.vdot(u, bo.forward(v))) / abs(np.vdot(u, bo.forward(v))) < 1e-12


def d2i_case():
    """The problem of tests/golden/make_golden.py:blurred_d2i (band-1C geometry without rotation, 200 x 200 image)."""
    N = 200
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    spec = orc.ChannelSpec(3.2 / 3600, 3.7 / 3600, (0.0, 0.0), 0.0, 0.196, 21, 3355.0, np.linspace(6.6, 7.6, 10), "1C")
    sotf = orc.ir2fr(orc.gaussian_psf(np.array([7.0]), problems.STEP), (N, N))[0]
    s = problems.STEP_DEG
    return N, ax, spec, sotf, s, [(0.0, 0.0), (5 * s, -7 * s), (-9 * s, 4 * s)]


def test_mrs_blurred_data_to_img_oracle_vs_reference():
    """``MRSBlurred.data_to_img`` (spectro_blind_rectangle.py:240-283; live call sites: scripts/simulate_deconvolution_mrs_rectangle.py:193,
    scripts/deconvolution_mrs_single_wavelength.py:159,194) restated, against the reference's own output.  The mean is compared where
    some pointing contributes; elsewhere the reference returns uninitialised memory."""
    g = np.load(os.path.join(G, "mrs_blurred_d2i.npz"))
    N, ax, spec, sotf, s, pts = d2i_case()
    bo = orc.BlurredOracle(sotf, ax, ax, spec, s, pts)
    x = np.random.default_rng(int(g["x_seed"])).random((N, N)) * np.linspace(0.0, 3.0, N)[None, :]
    assert rel(bo.forward(x), g["y"]) < 1e-13
    wm, gl = bo.data_to_img(g["y"])
    assert np.array_equal(gl != 0, g["covered"])                       # the threshold and the column patches cut the same pixels
    assert rel(gl, g["global_img"]) < 1e-13 and rel(wm, g["weighted_mean"]) < 1e-13
    assert (gl == 0).sum() > 0 and ((gl != 0) & (wm != gl)).sum() > 0  # uncovered pixels exist, and pixels seen by several pointings


def test_model_wct_oracle_vs_reference():
    """WCTOracle against the reference's Model_WCT outputs (tests/golden/model_wct.npz)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(G, "make_golden.py"))
    # only the seeded inputs are taken from the generator module (its reference import is lazy)
    src = open(os.path.join(G, "make_golden.py")).read()
    ns = {}
    exec(src[src.index("def wct_inputs"):src.index("def wct():")], {"problems": problems, "np": np}, ns)
    psfs, specs, shape, pce, x, y = ns["wct_inputs"]()
    g = np.load(os.path.join(G, "model_wct.npz"))
    wo = orc.WCTOracle(psfs, specs, shape, pce)
    assert rel(wo.forward(x), g["forward"]) < 1e-13
    assert rel(wo.adjoint(y), g["adjoint"]) < 1e-13
    assert rel(wo.fwadj(x), g["fwadj"]) < 1e-13
    # explicit-inverse solver: the reference's QuadCriterion3.run_expsol (fusion_mixing.py:309-438)
    assert rel(wo.expsol(y, 0.7), g["expsol"]) < 1e-12
    assert rel(wo.expsol(y, g["mu_list"]), g["expsol_mu_list"]) < 1e-12
    # and it is the minimiser: the normal equations hold
    xs = wo.expsol(y, 0.7)
    lhs = wo.fwadj(xs) + 0.7 * (orc.diff_r_t(orc.diff_r(xs)) + orc.diff_c_t(orc.diff_c(xs)))
    assert rel(lhs, wo.adjoint(y)) < 1e-12


def test_mixing_st_oracle_vs_reference():
    """MixingSTOracle against the reference's MixingST run through its compiled Cython kernels
    (tests/golden/mixing_st.npz; float32 there, float64 here)."""
    src = open(os.path.join(G, "make_golden.py")).read()
    ns = {}
    exec(src[src.index("def mixing_st_inputs"):src.index("def mixing_st():")], {"np": np}, ns)
    tpl, shape, L, sel, fast, maps, cube = ns["mixing_st_inputs"]()
    g = np.load(os.path.join(G, "mixing_st.npz"))
    o = orc.MixingSTOracle(tpl, shape, sel, fast)
    assert rel(o.forward(maps), g["forward"]) < 2e-7
    assert rel(o.adjoint(cube), g["adjoint"]) < 2e-7
    assert rel(o.fwadj(maps), g["fwadj"]) < 2e-7 and rel(o.TST, g["TST"]) < 2e-7
    assert np.array_equal(g["forward"] == 0, o.forward(maps) == 0)          # same support
    # adjointness of the masked pair (inputs are rounded to float32 like the reference's kernels)
    assert abs(np.vdot(o.forward(maps), cube) - np.vdot(maps, o.adjoint(cube))) < 1e-6 * abs(np.vdot(maps, o.adjoint(cube)))


@pytest.mark.parametrize("kshape", [(7, 1), (10, 1), (9, 1), (40, 40), (6, 5)], ids=["srf7", "srf10_even", "srf9", "psf40", "mixed"])
def test_ir2fr_is_centred_circular_convolution(kshape):
    """``udft.ir2fr`` (udft 3.4.0) is absent from the reference tree: the restatement the oracle and the product share is
    pinned by what its call sites need (spectroModelChannel.py:81-83, scripts/main_fusion.py:98) --
    ``idft(dft(x) * ir2fr(h, shape))`` is the circular convolution of x with h whose tap ``floor(n/2)`` sits on the output
    pixel, for odd AND even kernel lengths (band 4: srf = 10).  Parity with udft itself stays unpinned."""
    from surfh_amd import synth
    rng = np.random.default_rng(11)
    N1, N2 = 61, 47
    x = rng.standard_normal((3, N1, N2))
    h = rng.standard_normal(kshape)
    H = orc.ir2fr(h, (N1, N2))
    assert np.array_equal(H, synth.ir2fr(h, (N1, N2)))                    # the product's copy is the same function
    y = orc.idft(orc.dft(x) * H[np.newaxis], (N1, N2))
    c1, c2 = kshape[0] // 2, kshape[1] // 2
    ref = np.zeros_like(x)
    for j1 in range(kshape[0]):
        for j2 in range(kshape[1]):
            ref += h[j1, j2] * np.roll(x, (j1 - c1, j2 - c2), axis=(1, 2))     # y[i] = sum_j h[j] x[i - (j - c)]
    assert np.abs(y - ref).max() < 1e-12 * np.abs(ref).max()
    # a unit impulse at the centre tap is the identity
    d = np.zeros(kshape)
    d[c1, c2] = 1.0
    assert np.abs(orc.idft(orc.dft(x) * orc.ir2fr(d, (N1, N2))[np.newaxis], (N1, N2)) - x).max() < 1e-12


@pytest.mark.parametrize("srf", [7, 9, 10])
def test_box_sum_window_alignment_for_every_srf(srf):
    """The reference's local-domain filter ``_otf_sr * decalf`` (spectroModelChannel.py:81-83,104-108) is the forward
    window sum y[n] = sum_{j<srf} x[n + j] for the three sampling factors of the MRS bands, the even one included
    (with the restated ir2fr centred at floor(n/2) and the reference's shift dsi = int((srf - 1) / 2))."""
    class T:       # the two fields _box_filters reads
        pass
    t = T()
    t.srf = srf
    t.local_alpha_axis, t.local_beta_axis = np.zeros(53), np.zeros(17)
    x = np.random.default_rng(srf).standard_normal((2, 53, 17))
    a, b = orc.box_sum_fft(t, x), orc.box_sum_direct(t, x)
    assert np.abs(a - b).max() < 1e-12 * np.abs(b).max()
    at, bt = orc.box_sum_fft_t(t, x), orc.box_sum_direct_t(t, x)
    assert np.abs(at - bt).max() < 1e-12 * np.abs(bt).max()


def test_templates_edges_fixture():
    """tests/golden/templates_edges.npz (make_golden_templates.py) is what tests/test_gpu_templates.py takes it for: the sweep
    continues the one of templates.npz, the ragged matrix has the lengths that leave ragged K steps, and sklearn's factors
    reproduce its own reconstruction error."""
    path = os.path.join(os.path.dirname(__file__), "golden", "templates_edges.npz")
    assert os.path.getsize(path) < 300 * 1024
    z, z0 = np.load(path), np.load(os.path.join(os.path.dirname(__file__), "golden", "templates.npz"))
    assert list(z0["sweep_k"]) + list(z["sweep_k"]) == list(range(1, 12)) and sum(range(1, 12)) == 66
    errs = np.concatenate([z0["sweep_err"], z["sweep_err"]])
    assert np.all(np.diff(errs[:4]) < 0) and np.all(np.abs(errs[3:] / errs[3] - 1) < 0.1)   # rank 4 plus noise: from K = 4 on, the noise floor
    X = z["Xr"]
    assert X.dtype == np.float32 and X.shape == (97, 650) and X.min() >= 0 and X.shape[1] % 16 == 10
    for n in (1, 5):
        W, H = z[f"r_it{n}_W"].astype(np.float64), z[f"r_it{n}_H"].astype(np.float64)
        assert W.shape == (97, 5) and H.shape == (5, 650) and W.min() >= 0 and H.min() >= 0
        assert abs(np.linalg.norm(X - W @ H) - z[f"r_it{n}_err"]) < 1e-4 * z[f"r_it{n}_err"]
    assert z["r_it5_err"] < z["r_it1_err"]

