"""Non-negative fusion on the device (surfh_amd/nonneg.py, csrc/nonneg.hip, the loop in csrc/plan_solvers.hip) against its float64
restatement (tests/nonneg_oracle.py): the projection kernel element by element, the solver in both vector spaces, the template step
and the alternation.  The preconditions that keep the comparisons from being vacuous: tests/test_nonneg_host.py.  Needs a real
MI355X (`-m gpu`)."""
import numpy as np
import pytest

import nonneg_oracle as no
import posterior_oracle as po
import problems
import tpl_oracle as to
from capped_cases import NN_CALLS, check_nn, kernel_arrays, project_ref
from helpers import build_model, rel
from test_gpu_parity import note
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
C = no.CASE
# The bound of every comparison with the restatement: B for the vectors, 2B for r.r.  The recipe for B is 2 max(1e-4, e_cg) with e_cg
# the error of cg against oracle.lcg over outer x inner = 16 iterations on the same data (the larger of its error in x and half
# its worst relative error in r.r), so B is never below 2e-4.  Measured on the device, e_cg is of order one on all three problems,
# from zero and from ``case_start`` alike (x 1e-2 ... 1.4e-1, r.r within 4e-6 for ten iterations, then 1e-4, 1e-2, 0.3, 2: r.r has
# fallen six decades by then and two CG runs in different precisions part ways), which makes that B vacuous; for the template
# step it is 9.8e-5.  The tests hold to the floor of the recipe instead, the project's 1e-4 / 2e-4 convention with the factor 2
# it grants a loop built on another: never wider than the recipe's B.
B = 2e-4


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0")


def _err(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


def weights_for(osize, seed):
    """Inverse-variance-like weights with a tenth of the samples masked."""
    rng = np.random.default_rng(seed)
    w = 0.5 + rng.random(osize)
    w[rng.random(osize) < 0.1] = 0.0
    return w


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def run_project(m, x, u, z, r, rho, mode, off=0):
    """One call on fresh device copies `off` floats into their buffers; returns z', u', w (r or dv or None), sums, and the guards."""
    import torch
    n = x.size
    bufs = {}
    for name, a in (("x", x), ("z", z), ("u", u), ("w", r if mode == "r" else np.zeros_like(x))):
        b = torch.full((n + 12,), 123.0, dtype=torch.float32, device="cuda:0")
        b[off: off + n] = _dev(a.ravel())
        bufs[name] = b
    w = bufs["w"][off:]
    sums = m.nn_project_dev(bufs["x"][off:], bufs["z"][off:], bufs["u"][off:], n, rho, r_t=w if mode == "r" else None,
                            dv_t=w if mode == "dv" else None)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, h in host.items():
        assert np.all(h[:off] == 123.0) and np.all(h[off + n:] == 123.0), (k, "written outside its n floats")
    assert np.array_equal(host["x"][off: off + n].view(np.uint32), x.ravel().view(np.uint32))
    return host["z"][off: off + n], host["u"][off: off + n], host["w"][off: off + n], sums


@pytest.mark.parametrize("T", [1, 2, 5])
def test_project_kernel_matches_numpy(T):
    """T x 72 x 77 vectors through aligned pointers and a 5123-float vector through pointers one float off (the scalar path), in the
    fused and the dv form.  z' and u' to the bit, the count exactly, r / dv within ten times the error prior_add shows against
    NumPy on arrays of the same size, the float64 sums to 1e-12, no set sign bit in z', the same bits from a second call."""
    import torch
    m = build_model(po.rect_problem(72, 77, T))
    try:
        rng = np.random.default_rng(40 + T)
        er, ec = (rng.standard_normal(m.ishape).astype(np.float32) for _ in range(2))
        q_t = _dev(ec)
        m.prior_add_dev(_dev(er), q_t, 9.0)
        torch.cuda.synchronize()
        er64 = er.astype(np.float64)
        bound = 10 * _err(q_t.cpu().numpy(), ec.astype(np.float64) + 9.0 * (orc.diff_r_t(orc.diff_r(er64)) + orc.diff_c_t(orc.diff_c(er64))))
        assert 0 < bound < 1e-5
        rho = 3e2
        # ... and, once, past the kernel's 256 blocks: a second trip with a tail of 3 on the 16-byte path, a second trip on the scalar one
        for n, off in ((T * 72 * 77, 0), (5123, 1)) + (NN_CALLS if T == 5 else ()):
            x, u, z, r = kernel_arrays(n, 7 + T)
            zn, un, dv, rn = project_ref(x, u, z, r, rho)
            case = dict(n=n, x=x, u=u, z=z, r=r, zn=zn, un=un, dv=dv, rn=rn)
            for mode in ("r", "dv", "plain"):
                gz, gu, gw, sums = run_project(m, x, u, z, r, rho, mode, off)
                gz2, gu2, gw2, sums2 = run_project(m, x, u, z, r, rho, mode, off)
                assert np.array_equal(gz.view(np.uint32), gz2.view(np.uint32)) and np.array_equal(gu.view(np.uint32), gu2.view(np.uint32))
                assert np.array_equal(gw.view(np.uint32), gw2.view(np.uint32)) and np.array_equal(sums, sums2)
                # both branches and a denormal z' present; z', u', the count exact; no set sign bit; the sums to 1e-12; r / dv < bound
                e = check_nn(case, mode, gz, gu, gw, sums, bound)
                if mode != "plain":
                    print(f"T = {T} n = {n} off = {off} {mode}: {e:.2e} (bound {bound:.2e})")
                    note("nn_project", T=T, n=n, off=off, mode=mode, err=e, bound=bound)
        with pytest.raises(ValueError, match="rho"):
            m.nn_project_dev(q_t, q_t, q_t, 4, 0.0)
    finally:
        m.close()


# ---- the solver --------------------------------------------------------------------------------------------------------------------
def spectral_small():
    """127 x 48, T = 4: the smallest problem of the suite whose plan has the spectral calls (tests/test_gpu_spec_vectors.py, case A).
    Config 1 and two_channel_small do not have them: there the rule of ``cg`` picks the maps, and only this problem reaches the
    loop on the spectra."""
    from test_gpu_spec_vectors import spec_problem
    return spec_problem("A")


# name: (config, map shape, whether the plan runs cg on the spectra)
PROBLEMS = {"config1": (problems.config1, (64, 64), False), "two_channel_small": (problems.two_channel_small, (48, 48), False),
            "spectral_small": (spectral_small, (127, 48), True)}
_cases = {}


def solver_case(name, weighted):
    """The float64 side of one problem, computed once: the data and the restatement's run."""
    key = (name, weighted)
    if key not in _cases:
        cfgf, (na, nb), spectral = PROBLEMS[name]
        cfg = cfgf()
        om = problems.oracle_model(cfg)
        _, y = no.blob_data(om, 4, na, nb)
        w = weights_for(om.osize, 8) if weighted else None
        x0 = no.case_start(om.ishape)
        normal, b, wop, yw = no.maps_problem(om, y, C["mu"], C["mu_reg"], w)
        ref = no.admm(normal, b, C["rho"], x0=x0, outer=C["outer"], inner=C["inner"])
        # the preconditions of tests/test_nonneg_host.py on this problem's own run: the constraint is active, and decided
        share = ref["trace"][1:, 3] / b.size
        assert np.all((share >= 0.15) & (share <= 0.6)) and np.all(np.array(ref["near"]) < 0.01 * b.size), (name, share, ref["near"])
        yd = y if w is None else np.where(w.reshape(y.shape) > 0, y, np.nan)      # the masked samples hold NaN on the device
        _cases[key] = dict(cfg=cfg, y=yd, w=w, x0=x0, ref=ref, spectral=spectral)
    return _cases[key]


def compare(res, ref, label):
    tr = ref["trace"]
    xn = float(np.linalg.norm(ref["x"]))
    e_z = rel(res.x, ref["z"])
    e_p = float(np.max(np.abs(res.primal - np.sqrt(tr[:, 0])))) / xn
    e_d = float(np.max(np.abs(res.dual - np.sqrt(tr[:, 1])))) / res.rho / xn
    e_r = float(np.max(np.abs(res.grad_norm ** 2 - tr[:, 2]) / tr[:, 2]))
    d_a = np.abs(res.n_active - tr[:, 3])
    print(f"{label}: z {e_z:.2e}, primal {e_p:.2e}, dual/rho {e_d:.2e} (B {B:.2e}); r.r {e_r:.2e} (2B); n_active off by "
          f"{d_a.astype(int).tolist()} (near zero {ref['near']})")
    assert res.nit == ref["nit"] and len(res.primal) == len(tr)
    assert res.x.min() >= 0.0 and not np.any(np.signbit(res.x))
    assert e_z < B and e_p < B and e_d < B
    assert e_r < 2 * B
    assert d_a[0] == 0 and np.all(d_a[1:] <= np.asarray(ref["near"]))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_cg_nonneg_vs_oracle(name, weighted, monkeypatch):
    """4 x 4 from ``case_start`` in the loop the rule of ``cg`` picks and with SURFH_SPECTRAL_CG=0, against the restatement within B
    (the vectors) and 2B (r.r); the two runs within B of each other.  On spectral_small the first is the loop on the spectra."""
    case = solver_case(name, weighted)
    m = build_model(case["cfg"], with_ref=False)
    try:
        assert bool(m.spec_supported()) == case["spectral"]
        kw = dict(mu=C["mu"], mu_reg=C["mu_reg"], rho=C["rho"], x0=case["x0"], outer=C["outer"], inner=C["inner"], weights=case["w"])
        spec = m.cg_nonneg(case["y"], **kw)
        compare(spec, case["ref"], f"{name} {'spectra' if case['spectral'] else 'default'}")
        monkeypatch.setenv("SURFH_SPECTRAL_CG", "0")
        maps = m.cg_nonneg(case["y"], **kw)
        compare(maps, case["ref"], f"{name} maps")
        assert rel(spec.x, maps.x) < B
        assert np.array_equal(spec.x, maps.x) != case["spectral"]      # two loops where the plan has both, else the same bits
    finally:
        m.close()


@pytest.fixture(scope="module")
def c1():
    case = solver_case("config1", False)
    m = build_model(case["cfg"], with_ref=False)
    yield case, m
    m.close()


@pytest.fixture(scope="module")
def sp():
    case = solver_case("spectral_small", False)
    m = build_model(case["cfg"], with_ref=False)
    assert m.spec_supported()
    yield case, m
    m.close()


def test_refreshed_and_carried_residuals_agree(sp, monkeypatch):
    case, m = sp
    kw = dict(mu=C["mu"], mu_reg=C["mu_reg"], rho=C["rho"], x0=case["x0"], outer=C["outer"], inner=C["inner"])
    for env in ("1", "0"):
        monkeypatch.setenv("SURFH_SPECTRAL_CG", env)
        a, c = m.cg_nonneg(case["y"], refresh=1, **kw), m.cg_nonneg(case["y"], refresh=0, **kw)
        e = rel(a.x, c.x)
        e_r = float(np.max(np.abs(a.grad_norm ** 2 - c.grad_norm ** 2) / c.grad_norm ** 2))
        print(f"SURFH_SPECTRAL_CG={env}: refresh 1 against 0: z {e:.2e}, r.r {e_r:.2e} (B {B:.2e})")
        assert e < B and e_r < 2 * B
        assert not np.array_equal(a.grad_norm, c.grad_norm)            # the refresh did recompute


def test_zero_data_and_tolerance(sp, monkeypatch):
    case, m = sp
    for env in ("1", "0"):
        monkeypatch.setenv("SURFH_SPECTRAL_CG", env)
        res = m.cg_nonneg(np.zeros(m.osize), mu=1.0, mu_reg=5e3, rho=6e4, outer=3, inner=3)
        assert res.nit == 3 and np.all(res.x == 0.0) and not np.any(np.signbit(res.x))
        for t in (res.primal, res.dual, res.grad_norm):
            assert np.all(np.isfinite(t)) and np.all(t == 0.0)
        assert np.all(res.n_active == res.x.size)
        res = m.cg_nonneg(case["y"], mu=C["mu"], mu_reg=C["mu_reg"], outer=5, inner=2, tol=1e30)      # rho: the estimate
        assert res.nit == 1 and len(res.primal) == 2 and res.x.min() >= 0.0
        assert res.rho == m.nonneg_rho(C["mu"], C["mu_reg"]) and 1e4 < res.rho < 1e6


def test_refusals(c1):
    case, m = c1
    y = case["y"]
    for kw in (dict(rho=0.0), dict(rho=np.inf), dict(inner=0), dict(outer=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            m.cg_nonneg(y, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            m.cg_templates_nonneg(y, case["cfg"]["maps"], **kw)
    # the library's own checks, behind the wrappers'
    import ctypes
    from surfh_amd import _lib
    yf, out, tr, nit = y.astype(np.float32).ravel(), np.empty(m.isize, np.float32), np.zeros((2, 4)), ctypes.c_int32()
    for rho, outer, inner, word in ((-1.0, 1, 1, "rho"), (float("nan"), 1, 1, "rho"), (1.0, 1, 0, "inner"), (1.0, -1, 1, "outer")):
        assert m._L.surfh_cg_nonneg(m._plan, _lib.fptr(yf), 1.0, 0.0, rho, None, outer, inner, 0.0, 0, _lib.fptr(out), _lib.dptr(tr),
                                    ctypes.byref(nit)) != 0
        assert word in m._L.surfh_last_error().decode()
    from surfh_amd.imager import ImagerModel, synthetic_filters
    mi = build_model(case["cfg"], with_ref=False)
    try:
        im = ImagerModel(mi, synthetic_filters(case["cfg"]["wavel"], 2), decim=2)
        mi.set_imager(im)
        with pytest.raises(ValueError, match="imager"):
            mi.cg_templates_nonneg(y, case["cfg"]["maps"], outer=1, inner=1, rho=1.0)
        mi.set_imager_data(np.ones(im.osize), 1.0)
        with pytest.raises(ValueError, match="imager"):
            mi.cg_nonneg(y, outer=1, inner=1, rho=1.0)
    finally:
        mi.close()


# ---- the template step and the alternation -----------------------------------------------------------------------------------------
def tpl_case(cfg, om_cube):
    """y = A_x (templates with lines) + noise at the maps of the config; the start: the continuum less the constant that makes a
    quarter of its entries negative."""
    op = to.TemplateOp(om_cube, cfg["maps"])
    y0 = op.forward(to.templates_with_lines(cfg["Lc"]))
    y = y0 + np.random.default_rng(0).standard_normal(y0.shape) * 1e-2 * np.mean(np.abs(y0))
    s0 = cfg["templates"] - np.quantile(cfg["templates"], 0.25)
    return op, y, s0


def test_cg_templates_nonneg_vs_oracle(c1):
    case, m = c1
    cfg = case["cfg"]
    op, y, s0 = tpl_case(cfg, to.cube_model(cfg))
    mu, mu_spec = 1.0, 1e2
    assert 0.2 < np.mean(s0 < 0) < 0.3
    rho = m.nonneg_rho_templates(cfg["maps"], mu, mu_spec)
    st = to._Stacked(op, mu, mu_spec, None)
    rhs = np.concatenate([st.sw * y, np.zeros(op.ishape[0] * (op.ishape[1] - 1))])
    ref = no.admm(lambda v: st.adjoint(st.forward(v)), st.adjoint(rhs), rho, x0=s0, outer=C["outer"], inner=C["inner"])
    share = ref["trace"][:, 3] / s0.size
    print(f"templates: rho {rho:.3e}, active share {np.round(share, 3).tolist()}")
    # the constraint is active where the run starts (row 0's r carries rho (z - s0); float64: nothing is held at zero afterwards,
    # the data want positive spectra), and no entry is within rounding of the projection's corner
    assert 0.2 < share[0] < 0.3 and ref["trace"][0, 0] > 0 and np.all(np.array(ref["near"]) < 0.01 * s0.size)
    tpl0 = m.templates.copy()
    res = m.cg_templates_nonneg(y, cfg["maps"], mu=mu, mu_spec=mu_spec, rho=rho, s0=s0, outer=C["outer"], inner=C["inner"])
    compare(res, ref, "templates")
    assert res.x.shape == tpl0.shape and np.array_equal(m.templates, tpl0)
    f0 = m.forward(cfg["maps"])
    m.cg_templates_nonneg(y, cfg["maps"], mu=mu, mu_spec=mu_spec, rho=rho, outer=1, inner=2)           # s0 None: the model's templates
    assert np.array_equal(m.forward(cfg["maps"]), f0)                  # the plan's own templates are back in place


def test_nonneg_alternation(c1):
    from surfh_amd.fusion import refine_templates
    case, _ = c1
    cfg = case["cfg"]
    om = to.cube_model(cfg)
    _, y, s0 = tpl_case(cfg, om)
    x0 = cfg["maps"] - 0.25                                            # a quarter of the maps' start infeasible too
    mu, mu_reg, mu_spec = 1.0, 5e3, 1.0
    m = build_model(dict(cfg, templates=np.maximum(s0, 0.0)), with_ref=False)
    try:
        start = m.templates.copy()
        rhos = (m.nonneg_rho(mu, mu_reg), m.nonneg_rho_templates(np.maximum(x0, 0.0), mu, mu_spec))
        res = refine_templates(m, y, mu, mu_reg, mu_spec, 2, 3, 3, x0=x0, nonneg=True, rho=rhos, inner=4)
        J = res.criterion
        print("J:", " -> ".join(f"{j:.4e}" for j in J))
        assert J.shape == (5,) and res.x.min() >= 0.0 and res.templates.min() >= 0.0
        assert np.array_equal(m.templates, res.templates) and np.array_equal(res.templates_start, start)
        assert J[-1] < J[0]
        # every entry against the float64 criterion at the same iterates, by replaying the half-steps
        m.set_templates(start)
        x, S, errs = x0, start, []
        errs.append(abs(J[0] - to.joint_criterion(om, y, x, S, mu, mu_reg, mu_spec)) / J[0])
        for k in range(2):
            x = m.cg_nonneg(y, mu=mu, mu_reg=mu_reg, rho=rhos[0], x0=x, outer=3, inner=4).x
            errs.append(abs(J[2 * k + 1] - to.joint_criterion(om, y, x, S, mu, mu_reg, mu_spec)) / J[2 * k + 1])
            S = m.cg_templates_nonneg(y, x, mu=mu, mu_spec=mu_spec, rho=rhos[1], outer=3, inner=4).x
            m.set_templates(S)
            errs.append(abs(J[2 * k + 2] - to.joint_criterion(om, y, x, S, mu, mu_reg, mu_spec)) / J[2 * k + 2])
        print("J against float64 at the iterates:", " ".join(f"{e:.1e}" for e in errs))
        assert np.array_equal(x, res.x) and np.array_equal(S, res.templates)
        assert max(errs) <= 1e-4                                       # the bound of test_gpu_tpl's alternation test
        # rho None: both penalties estimated once, at the start
        m.set_templates(start)
        auto = refine_templates(m, y, mu, mu_reg, mu_spec, 1, 1, 1, x0=x0, nonneg=True, inner=2)
        assert auto.criterion.shape == (3,) and auto.x.min() >= 0.0 and auto.templates.min() >= 0.0
    finally:
        m.close()


def test_cg_bits_survive_the_nonneg_runs(sp, monkeypatch):
    """cg (on the spectra and on the maps) and cg_templates before and after every non-negative entry point on the same plan: the
    same bits."""
    case, m = sp
    cfg, y = case["cfg"], case["y"]

    def bits():
        out = []
        for env in ("1", "0"):
            monkeypatch.setenv("SURFH_SPECTRAL_CG", env)
            x, gn, _ = m.cg(y, mu=C["mu"], mu_reg=C["mu_reg"], x0=case["x0"], max_iter=6)
            out += [x, gn]
        S, gn, _ = m.cg_templates(y, cfg["maps"], mu=1.0, mu_spec=1e2, max_iter=4)
        return out + [S, gn, m.forward(cfg["maps"])]

    before = bits()
    for env in ("1", "0"):
        monkeypatch.setenv("SURFH_SPECTRAL_CG", env)
        m.cg_nonneg(y, mu=C["mu"], mu_reg=C["mu_reg"], rho=C["rho"], x0=case["x0"], outer=2, inner=3, refresh=1)
    m.cg_templates_nonneg(y, cfg["maps"], mu=1.0, mu_spec=1e2, rho=1e3, outer=2, inner=3, refresh=1)
    t = _dev(np.random.default_rng(0).standard_normal(300))
    m.nn_project_dev(t, _dev(np.zeros(300)), _dev(np.zeros(300)), 300, 2.0, r_t=_dev(np.ones(300)))
    with pytest.raises(ValueError):
        m.cg_nonneg(y, rho=-1.0)
    after = bits()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_writes_the_nonneg_results(tmp_path):
    import importlib.util
    import os
    from click.testing import CliRunner
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("main_fusion", os.path.join(root, "scripts", "main_fusion.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    base = ["-fd", str(tmp_path), "-np", "251", "-hp", "5e3", "-ni", "2", "--synthetic", "small", "--nonneg", "--inner", "2"]
    r = CliRunner().invoke(drv.main, base + ["--outer", "3"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("lcg", 1, 4, 3, 5e3, False, nonneg=True)
    x, tr = np.load(d / "res_x.npy"), np.load(d / "nn_trace.npy")
    assert x.shape == (4, 251, 251) and x.min() >= 0.0
    assert tr.shape == (4, 4) and np.all(np.isfinite(tr)) and tr[-1, 3] == np.sum(x == 0)
    r = CliRunner().invoke(drv.main, base + ["--refine_templates", "1", "--tpl_iter", "2", "--mu_spec", "1"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = tmp_path / "Results" / drv.result_dir_name("lcg", 1, 4, 2, 5e3, False, refine=1, nonneg=True)
    assert np.load(d / "res_x.npy").min() >= 0.0 and np.load(d / "res_templates.npy").min() >= 0.0
    assert np.load(d / "criterion.npy").shape == (3,)
