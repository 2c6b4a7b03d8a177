"""The vector kernels of the plane-wise CG and 3MG loops on the device, element by element against float64: the cases, checks and
bounds of tests/planes_cases.py (whose teeth tests/test_planes_cases_host.py shows without a GPU) through
``planes_cg_dev`` -- surfh_debug_planes_cg, the launchers the solvers call on explicit extents -- on one small plan.  Every measured
error goes to the parity log in units of its bound.  The last test ties the kernel-level pins to what the loops launch: one CG
iteration of the device-resident loop on both vector layouts against the float64 step of its own vectors.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import planes_cases as pc
from test_gpu_parity import note
from test_gpu_variants import blurred_case

pytestmark = pytest.mark.gpu
L_MODEL = 3


@pytest.fixture(scope="module")
def model():
    N, bo, m = blurred_case(L=L_MODEL)
    assert m.ishape == (L_MODEL, N, N)
    yield N, bo, m
    m.close()


@pytest.fixture(scope="module")
def launch(model):
    import torch
    m = model[2]

    def go(which, ext, v, sc_in, so, mu_reg, update_r):
        ts = [torch.as_tensor(a, device="cuda:0") for a in v]
        torch.cuda.synchronize()
        m.planes_cg_dev(which, ext, ts, sc_in, so, mu_reg, update_r)
        for a, t in zip(v, ts):
            a[:] = t.cpu().numpy()
    return go


def _log(name, e, **kw):
    print(name, kw, e)
    note(name, **kw, **e)
    assert all(v <= 1.0 for v in e.values())


@pytest.mark.parametrize("L", pc.PM_L)
@pytest.mark.parametrize("npix", pc.PM_NPIX)
def test_plane_major_cg_kernels(launch, L, npix):
    c = pc.pm_case(L, npix)
    _log("planes_dot", pc.run_pm_dot(c, launch), L=L, npix=npix)
    _log("planes_cg_dir", pc.run_pm_dir(c, launch), L=L, npix=npix)
    for update_r in (1, 0):
        _log("planes_cg_step", pc.run_pm_step(c, launch, update_r), L=L, npix=npix, update_r=update_r)


@pytest.mark.parametrize("L", pc.PM_L)
@pytest.mark.parametrize("npix", pc.PM_NPIX)
def test_plane_major_mmmg_kernels(launch, L, npix):
    c = pc.pm_case(L, npix)
    for mode in ({}, dict(first=True), dict(neg=True)):
        tag = next(iter(mode), "live")
        _log("planes_mmmg_dir", pc.run_mmmg_dir(c, launch, **mode), L=L, npix=npix, mode=tag)
        for update_r in (1, 0):
            _log("planes_mmmg_step", pc.run_mmmg_step(c, launch, update_r, **mode), L=L, npix=npix, mode=tag, update_r=update_r)


@pytest.mark.parametrize("shape", pc.PN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_wavelength_innermost_kernels(launch, shape):
    c = pc.pn_case(shape)
    kw = dict(shape=list(shape))
    _log("pn_dot", pc.run_pn_dot(c, launch), **kw)
    _log("pn_dir", pc.run_pn_dir(c, launch), **kw)
    for mu_reg in pc.MU_REGS + (0.0,):
        _log("pn_prior_dot", pc.run_pn_prior_dot(c, launch, mu_reg), mu_reg=mu_reg, **kw)
    for update_r in (1, 0):
        _log("pn_step", pc.run_pn_step(c, launch, update_r), update_r=update_r, **kw)


def test_layout_transposes(launch):
    for case in pc.TR_CASES:
        pc.run_transposes(pc.tr_case(*case), launch)
    note("planes_transposes", cases=len(pc.TR_CASES), exact=1.0)


def test_argument_rules_of_the_library(model):
    import torch
    m = model[2]
    c = pc.pn_case(pc.PN_SHAPES[4])
    before = [pc.pn_buf(c, c["x"], "acc"), pc.pn_buf(c, c["r"], "rw"), pc.pn_buf(c, c["d"], "in"), pc.pn_buf(c, c["q"], "in")]
    ts = [torch.as_tensor(a, device="cuda:0") for a in before]
    torch.cuda.synchronize()
    Na, Nb, NAP, LP, Lc = c["shape"]
    sc_in, out = np.stack([c["rr"], c["dq"]]), np.full(LP, pc.GUARD64)
    for ext, word in (((0, Nb, NAP, LP, Lc, 0), "Na 0"), ((Na, 0, NAP, LP, Lc, 0), "Nb 0"), ((Na, Nb, Na - 1, LP, Lc, 0), "NAP"),
                      ((Na, Nb, NAP, LP, 0, 0), "L 0"), ((Na, Nb, NAP, LP, LP + 1, 0), "L 65"), ((Na, Nb, NAP, LP, Lc, -1), "l0 -1"),
                      ((Na, Nb, NAP, LP, Lc, 1), "l0 1"), ((Na, Nb, NAP, 96, Lc, 0), "multiple of 64"), ((Na, Nb, NAP, 32, 32, 0), "LP 32"),
                      ((Na, 70000, 64, 512, Lc, 0), "Nb 70000")):
        with pytest.raises(RuntimeError, match=word):
            m.planes_cg_dev("pn_step", ext, ts, sc_in, out)
    with pytest.raises(RuntimeError, match="vector 3 is null"):
        m.planes_cg_dev("pn_step", c["ext"], ts[:3], sc_in, out)
    with pytest.raises(RuntimeError, match="scalar arrays"):
        m.planes_cg_dev("pn_step", c["ext"], ts, None, out)
    with pytest.raises(RuntimeError, match="unknown kernel"):
        m.planes_cg_dev("pn_stop", c["ext"], ts, sc_in, out)
    for ext in ((0, 5), (3, 0), (70000, 70000)):
        with pytest.raises(RuntimeError, match="planes of"):
            m.planes_cg_dev("dot", ext, ts[:2], None, out)
    with pytest.raises(RuntimeError, match="update_r 2"):
        m.planes_cg_dev("pn_step", c["ext"], ts, sc_in, out, update_r=2)
    torch.cuda.synchronize()
    assert np.all(out == pc.GUARD64) and all(pc.same_bits(t.cpu().numpy(), a) for t, a in zip(ts, before))      # nothing was launched


def test_one_cg_iteration_of_the_loop_on_both_layouts(model, monkeypatch):
    """One iteration of cg_begin_dev / cg_step_dev from x0 = 0 with SURFH_PLANES_NATIVE at 0 (plane-major vectors) and at 1
    (wavelength-innermost): x1 = s d with d = r = b.  b and q = Q b are taken from the plan's own operators in the plane-major layout
    (the calls the plane-major loop makes: the adjoint, the normal operator; the quadratic prior is added in float64), s = b.b / b.q
    per plane from float64 sums, and x1 of both runs is held to the AXPY bound of planes_cases.py.  The wavelength-innermost run forms
    q in another order: its d.q differs from the plane-major one by the sum of L N N rounding errors of random sign, some 1e-9 of
    it, against the EPS = 6e-8 the bound leaves beside the two roundings of s d."""
    import torch
    N, bo, m = model
    y = bo.forward(np.random.default_rng(31).random((L_MODEL, N, N)))
    mu, mur = 1.0, 0.05
    dev = torch.device("cuda:0")
    yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32).reshape(-1), device=dev)
    bt, qt = (torch.zeros((L_MODEL, N, N), dtype=torch.float32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    from surfh_amd import _lib
    _lib.check(m._L.surfh_adjoint_dev(m._plan, ptr(yt), ptr(bt)))
    _lib.check(m._L.surfh_normal_dev(m._plan, ptr(bt), ptr(qt), mu))
    torch.cuda.synchronize()
    b = pc.f64(bt.cpu().numpy())
    lap = sum(2 * b - np.roll(b, 1, axis=ax) - np.roll(b, -1, axis=ax) for ax in (1, 2))
    q = pc.f64(qt.cpu().numpy()) + mur * lap
    s = pc.ratio(pc.rowdot(b, b), pc.rowdot(b, q))
    assert np.all(s > 0)
    want = s[:, None, None] * b
    for native in ("0", "1"):
        monkeypatch.setenv("SURFH_PLANES_NATIVE", native)
        xt = torch.zeros((L_MODEL, N, N), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.profile_enable(True)
        m.profile_reset()
        m.cg_begin_dev(yt, xt, mu, mur)
        rr0 = m.cg_rr()
        m.cg_step_dev(1, 50)
        m.cg_rr()                                                   # synchronises
        prof = m.profile()
        m.profile_enable(False)
        assert ("pn_dir" in prof) == (native == "1"), (native, sorted(prof))         # the layout asked for is the one that ran
        x = xt.cpu().numpy()
        e = dict(x=pc.units(x, want, pc.AXPY * np.abs(want), f"x0 + s d, SURFH_PLANES_NATIVE={native}"),
                 rr0=max(pc.dot_ok(rr0[l], b[l], b[l], f"r0.r0 of plane {l}") for l in range(L_MODEL)))
        _log("planes_cg_one_iteration", e, native=native)
