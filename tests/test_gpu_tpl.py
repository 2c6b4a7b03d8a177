"""Template refinement on the device (surfh_amd/spectra.py, csrc/tplgrad.hip) against its float64 restatement (tests/tpl_oracle.py):
the transpose with respect to the templates on every plan route, the plan state behind set_templates, the template solver, the
recovery of lines the start lacks and the alternation.  Needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import problems
import tpl_oracle as to
from helpers import build_model, rel
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu


def templates_T(Lc, T):
    """T = 1 ... 4: rows of the synthetic templates; 5: one more row, a slow oscillation on a ramp (more than the spectral mix holds
    in registers: the plan leaves the fused passes)."""
    base = orc.synthetic_templates(Lc)
    if T <= 4:
        return base[:T].copy()
    lam = np.arange(Lc, dtype=np.float64)
    return np.vstack([base, 0.05 * lam + 9.0 + 3.0 * np.sin(lam / 7.0)])


def with_T(cfg, T):
    out = dict(cfg)
    out["templates"] = templates_T(cfg["Lc"], T)
    out["maps"] = np.random.default_rng(100 + T).random((T, cfg["N"], cfg["N"]))
    return out


def ct_smallest():
    """256 x 256: the smallest axis the plan sends to dft_ct (n / 2 + 1 = 129 no longer fits dft_h2); 128 planes = one padded LP."""
    return problems.mk(256, 128, 7.40, 7.92, [(0.8, 0.9, 8.2, 4, 3050, np.linspace(7.42, 7.90, 48), 2, "A")], seed=41)


PROBLEMS = {
    "config1": problems.config1,
    "two_channel_small": problems.two_channel_small,
    "two_channel_disjoint": problems.two_channel_disjoint,
    "three_channels_ACB": lambda: problems.three_channels("ACB"),
    "two_channel_mid": problems.two_channel_mid,
    "ct_smallest": ct_smallest,
}


def dft_dims(m):
    d = (C.c_int64 * 4)()
    assert m._L.surfh_debug_dims(m._plan, b"dft", d) == 0
    return tuple(int(v) for v in d)


def weights_for(osize, seed):
    """Inverse-variance-like weights with a tenth of the samples masked."""
    rng = np.random.default_rng(seed)
    w = 0.5 + rng.random(osize)
    w[rng.random(osize) < 0.1] = 0.0
    return w


# ---- kernel parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_adjoint_templates_vs_oracle(name):
    """A_x^T u against the oracle for T = 1, 4, 5 (5: the route over pixels), on u and on W u (what the solver hands in under data
    weights).  Bound: 10 x the error the maps' adjoint of the same model shows against the oracle on the same u."""
    base = PROBLEMS[name]()
    om = to.cube_model(base)
    seen = to.seen_planes(om)
    rng = np.random.default_rng(5)
    u = rng.standard_normal(om.osize)
    us = {"plain": u, "weighted": to.select(weights_for(om.osize, 6), rng.standard_normal(om.osize))}
    gcs = {k: om.adjoint(v) for k, v in us.items()}              # the cube-space adjoint after its OTF^T: once per u
    for T in (1, 4, 5):
        cfg = with_T(base, T)
        m = build_model(cfg, with_ref=False)
        try:
            d = dft_dims(m)
            if name == "two_channel_mid":
                assert d == (1, 1, 1, 1 if T <= 4 else 0)        # dft_h2 on both axes, the fused adjoint tail where T allows
            if name == "ct_smallest":
                assert d[:3] == (2, 2, 1)                        # dft_ct on both axes
            for k, v in us.items():
                ref_G = np.einsum("tab,lab->tl", cfg["maps"], gcs[k])
                ref_x = orc.lmm_cube2maps(gcs[k], cfg["templates"])
                G = m.adjoint_templates(v, cfg["maps"])
                e_maps, e_tpl = rel(m.adjoint(v), ref_x), rel(G, ref_G)
                print(f"{name} T={T} {k}: adjoint_templates {e_tpl:.3e}, maps' adjoint {e_maps:.3e}")
                assert e_tpl <= 10 * e_maps
                assert np.all(G[:, ~seen] == 0.0)                 # planes no channel reads: exactly zero
                assert np.array_equal(G, m.adjoint_templates(v, cfg["maps"]))      # fixed summation order: the same bits
        finally:
            m.close()


@pytest.fixture(scope="module")
def c1():
    cfg = problems.config1()
    om = to.cube_model(cfg)
    m = build_model(cfg, with_ref=False)
    yield cfg, om, m
    m.close()


@pytest.mark.parametrize("name", ["config1", "two_channel_disjoint"])
def test_dot_test_on_the_device(name):
    cfg = PROBLEMS[name]()
    m = build_model(cfg, with_ref=False)
    try:
        rng = np.random.default_rng(21)
        x = cfg["maps"]
        shape = cfg["templates"].shape
        pg, ng = [], []
        for _ in range(3):                 # non-negative vectors: no cancellation in the inner products, the strict bar
            S, u = rng.random(shape), rng.random(m.osize)
            l, r = float(np.vdot(m.forward_templates(S, x), u)), float(np.vdot(S, m.adjoint_templates(u, x)))
            pg.append(abs(l - r) / abs(r))
        for _ in range(3):                 # zero-mean vectors: the gap against the natural scale |u| |A_x S| (test_gpu_parity.py)
            S, u = rng.standard_normal(shape), rng.standard_normal(m.osize)
            a = m.forward_templates(S, x)
            l, r = float(np.vdot(a, u)), float(np.vdot(S, m.adjoint_templates(u, x)))
            ng.append(abs(l - r) / (np.linalg.norm(u) * np.linalg.norm(a)))
        print(f"{name}: dot-test gaps non-negative {max(pg):.2e}, randn normalised {max(ng):.2e}")
        assert max(pg) < 1e-6
        assert max(ng) < 1e-6
        # forward_templates is the forward of a model built with those templates, bit for bit, and leaves the model's own alone
        S2 = cfg["templates"] * (1.0 + 0.3 * np.sin(np.arange(shape[1]) / 5.0))
        before = m.forward(x)
        y2 = m.forward_templates(S2, x)
        assert np.array_equal(m.forward(x), before)
        m2 = build_model(dict(cfg, templates=S2), with_ref=False)
        try:
            assert np.array_equal(y2, m2.forward(x))
        finally:
            m2.close()
    finally:
        m.close()


# ---- plan state ------------------------------------------------------------------------------------------------------------------
def test_set_templates_equals_a_fresh_model(c1):
    cfg, om, _ = c1
    S2 = to.templates_with_lines(cfg["Lc"])
    x = cfg["maps"]
    y = np.random.default_rng(2).random(om.osize)
    m = build_model(cfg, with_ref=False)
    fresh = build_model(dict(cfg, templates=S2), with_ref=False)
    try:
        m.forward(x)                                  # the plan has run with the old templates
        m.set_templates(S2)
        assert np.array_equal(m.templates, S2)
        for f, a in (("forward", x), ("adjoint", y), ("fwadj", x)):
            assert np.array_equal(getattr(m, f)(a), getattr(fresh, f)(a)), f
        a, b = m.cg(y, mu=1.0, mu_reg=5e3, max_iter=5), fresh.cg(y, mu=1.0, mu_reg=5e3, max_iter=5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(m.mapsToCube(x), fresh.mapsToCube(x))
        with pytest.raises(ValueError, match="fixed at plan creation"):
            m.set_templates(S2[:3])
        bad = S2.copy()
        bad[1, 7] = np.nan
        with pytest.raises(ValueError, match="finite"):
            m.set_templates(bad)
        assert np.array_equal(m.forward(x), fresh.forward(x))
    finally:
        m.close()
        fresh.close()


def test_model_wct_set_specs():
    from surfh_amd.mixing import Model_WCT, regularisation_freq
    rng = np.random.default_rng(4)
    L, N = 24, 48
    psf = orc.gaussian_psf(np.linspace(7.4, 7.9, L), problems.STEP)
    s1, s2 = orc.synthetic_templates(L)[:3], to.templates_with_lines(L)[:3]
    pce = np.ones(L)
    m, fresh = Model_WCT(psf, s1, (N, N), pce), Model_WCT(psf, s2, (N, N), pce)
    try:
        x, cube = rng.random((3, N, N)), rng.random((L, N, N))
        reg = regularisation_freq((N, N))
        mu = np.full(3, 1e-2)
        m.fwadj(x)                                    # builds the Hessian of the old spectra
        m.set_specs(s2)
        assert np.array_equal(m.forward(x), fresh.forward(x))
        assert np.array_equal(m.fwadj(x), fresh.fwadj(x))
        assert np.array_equal(m.expsol(cube, mu, reg), fresh.expsol(cube, mu, reg))
        with pytest.raises(ValueError):
            m.set_specs(s2[:2])
    finally:
        m.close()
        fresh.close()


def test_cg_templates_restores_the_plan(c1):
    cfg, om, m = c1
    x = cfg["maps"]
    y = to.TemplateOp(om, x).forward(to.templates_with_lines(cfg["Lc"]))
    tpl0, f0 = m.templates.copy(), m.forward(x)
    m.cg_templates(y, x, mu=1.0, mu_spec=1e2, max_iter=3)
    assert np.array_equal(m.templates, tpl0) and np.array_equal(m.forward(x), f0)
    seen_f = []

    def stop_at_2(it, gn, S):
        seen_f.append(np.array_equal(m.forward(x), f0))      # the plan's own templates are in place while the callback runs
        assert S.shape == tpl0.shape and len(gn) == it + 1
        return it == 2

    S, gn, nit = m.cg_templates(y, x, mu=1.0, mu_spec=1e2, max_iter=6, callback=stop_at_2)
    assert nit == 2 and len(gn) == 3 and seen_f == [True, True]
    assert np.array_equal(m.templates, tpl0) and np.array_equal(m.forward(x), f0)
    # the callback, which ran the operator in between, changes nothing of the solve
    S_plain = m.cg_templates(y, x, mu=1.0, mu_spec=1e2, max_iter=2)[0]
    assert np.array_equal(S, S_plain)


def test_imager_refuses_template_calls(c1):
    from surfh_amd.imager import ImagerModel, synthetic_filters
    cfg, om, _ = c1
    m = build_model(cfg, with_ref=False)
    try:
        x = cfg["maps"]
        f0 = m.forward(x)
        m.set_imager(ImagerModel(m, synthetic_filters(cfg["wavel"], 2), decim=2))
        with pytest.raises(ValueError, match="imager"):
            m.set_templates(to.templates_with_lines(cfg["Lc"]))
        with pytest.raises(ValueError, match="imager"):
            m.cg_templates(f0, x, max_iter=1)
        assert np.array_equal(m.forward(x), f0)
        m.set_imager(None)
        m.set_templates(cfg["templates"] * 2.0)
        assert rel(m.forward(x), 2.0 * f0) < 1e-6
    finally:
        m.close()


# ---- solver ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["config1", "two_channel_small"])
@pytest.mark.parametrize("mu_spec,weighted", [(0.0, False), (1e2, True)])
def test_cg_templates_vs_oracle_lcg(name, mu_spec, weighted):
    """8 iterations against oracle.lcg on A_x: the iterate within 1e-4, every r.r within 2e-4 (the project's bounds for the maps'
    CG).  Under weights the masked samples hold NaN.  The start is not the model's templates."""
    cfg = PROBLEMS[name]()
    om = to.cube_model(cfg)
    op = to.TemplateOp(om, cfg["maps"])
    truth = to.templates_with_lines(cfg["Lc"])
    y0 = op.forward(truth)
    y = y0 + np.random.default_rng(0).standard_normal(y0.shape) * 1e-2 * np.mean(np.abs(y0))
    w = weights_for(om.osize, 8) if weighted else None
    s0 = cfg["templates"] * 0.9 + 1.0
    ref = to.lcg_templates(op, y, 1.0, mu_spec, s0, weights=w, max_iter=8)
    if weighted:
        y = np.where(w > 0, y, np.nan)
    m = build_model(cfg, with_ref=False)
    try:
        S, gn, nit = m.cg_templates(y, cfg["maps"], mu=1.0, mu_spec=mu_spec, s0=s0, max_iter=8, weights=w)
    finally:
        m.close()
    gr = np.asarray(ref["grad_norm"])
    e_x, e_g = rel(S, ref["x"]), float(np.max(np.abs(gn - gr) / gr))
    print(f"{name} mu_spec={mu_spec:g} weighted={weighted}: iterate {e_x:.3e}, r.r {e_g:.3e}; r.r {gr[0]:.3e} -> {gr[-1]:.3e}")
    assert nit == 8 and len(gn) == 9
    assert e_x < 1e-4
    assert e_g < 2e-4


# ---- recovery and alternation ----------------------------------------------------------------------------------------------------
def test_recovery_on_the_device(c1):
    """The setup of tests/test_tpl_host.py::test_recovery_of_lines_the_start_lacks with the data from the oracle: the core-plane
    error ends at <= 0.5 x the start's, and the device's templates are within a fifth of the oracle's own distance to the truth."""
    cfg, om, m = c1
    op = to.TemplateOp(om, cfg["maps"])
    truth, start = to.templates_with_lines(cfg["Lc"]), cfg["templates"]
    y0 = op.forward(truth)
    y = y0 + np.random.default_rng(0).standard_normal(y0.shape) * 1e-2 * np.mean(np.abs(y0))
    # sensitivity |A_x E_l|^2 on the device (128 applications; the oracle's takes 20 s), the planes chosen as in the host test
    T, Lc = start.shape
    sens = np.zeros(Lc)
    for l in range(Lc):
        E = np.zeros((T, Lc))
        E[:, l] = 1.0
        sens[l] = np.sum(m.forward_templates(E, cfg["maps"]) ** 2)
    core = to.core_planes(sens)
    assert core.sum() == 86
    ref = to.lcg_templates(op, y, 1.0, 1e2, start, max_iter=30)["x"]
    S, gn, nit = m.cg_templates(y, cfg["maps"], mu=1.0, mu_spec=1e2, max_iter=30)
    e0, e1, eo = to.core_err(start, truth, core), to.core_err(S, truth, core), to.core_err(ref, truth, core)
    dist = float(np.linalg.norm((S - ref)[:, core]) / np.linalg.norm(truth[:, core]))
    print(f"core-plane error {e0:.4f} -> {e1:.4f} (oracle {eo:.4f}); device to oracle {dist:.2e}")
    assert e1 <= 0.5 * e0
    assert dist <= eo / 5


def test_alternation_on_the_device(c1):
    from surfh_amd.fusion import refine_templates
    cfg, om, _ = c1
    truth, start = to.templates_with_lines(cfg["Lc"]), cfg["templates"]
    y0 = to.TemplateOp(om, cfg["maps"]).forward(truth)
    y = y0 + np.random.default_rng(0).standard_normal(y0.shape) * 1e-2 * np.mean(np.abs(y0))
    m = build_model(cfg, with_ref=False)
    try:
        iterates = []
        res = refine_templates(m, y, 1.0, 5e3, 1.0, 3, 15, 10, x0=cfg["maps"])
        assert np.array_equal(res.templates_start, start) and np.array_equal(m.templates, res.templates)
        J = res.criterion
        assert J.shape == (7,)
        print("J:", " -> ".join(f"{j:.4e}" for j in J))
        assert np.all(np.diff(J) < 0)                      # strictly down at every half-step
        # the last entry against the float64 criterion at the returned iterates; the earlier ones by replaying the half-steps
        Jo = to.joint_criterion(om, y, res.x, res.templates, 1.0, 5e3, 1.0)
        assert abs(J[-1] - Jo) <= 1e-4 * Jo
        m.set_templates(start)
        x, S, k = cfg["maps"], start, 0
        assert abs(J[0] - to.joint_criterion(om, y, x, S, 1.0, 5e3, 1.0)) <= 1e-4 * J[0]
        for _ in range(3):
            x = m.cg(y, mu=1.0, mu_reg=5e3, x0=x, max_iter=15)[0]
            k += 1
            iterates.append(abs(J[k] - to.joint_criterion(om, y, x, S, 1.0, 5e3, 1.0)) / J[k])
            S = m.cg_templates(y, x, mu=1.0, mu_spec=1.0, max_iter=10)[0]
            m.set_templates(S)
            k += 1
            iterates.append(abs(J[k] - to.joint_criterion(om, y, x, S, 1.0, 5e3, 1.0)) / J[k])
        print("J against float64 at the iterates:", " ".join(f"{e:.1e}" for e in iterates))
        assert max(iterates) <= 1e-4
    finally:
        m.close()
