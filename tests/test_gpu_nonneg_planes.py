"""Non-negative plane-wise deconvolution on the device (``MRSBlurred.cg_nonneg``, surfh_cg_planes_nonneg; csrc/nonneg.hip, the loop in
csrc/plan_solvers.hip) against its float64 restatement (tests/nonneg_planes_oracle.py): the per-plane projection kernel element by
element, the solver plane by plane on both operator classes, the per-plane stopping test, the refusals, the bits of the other
solvers and the driver.  The preconditions that keep the comparisons from being vacuous: tests/test_nonneg_planes_host.py.  Needs a
real MI355X (`-m gpu`).

Measured on MI355X (worst over the compared planes; bounds 2e-4 on z, 4e-4 on the rest): see DESIGN.md section 6g, "Plane-wise"."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import huber_planes_oracle as hp
import nonneg_planes_oracle as npo
import posterior_oracle as po
import problems
from capped_cases import check_nn, kernel_arrays, project_ref
from helpers import build_model, max_err
from oracle import surfh_oracle as orc
from test_gpu_huber_planes import _plane_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(mu=npo.MU, mu_reg=npo.MUR, outer=npo.OUTER, inner=npo.INNER, refresh=0)
# penalties decades apart, all exact in float32: a plane that reads its neighbour's is far off
RHO = (0.5, 6.0, 6e4, 3e2, 0.0078125)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0")


@pytest.fixture(scope="module")
def dev():
    """The shared problem, its model and the device run the comparisons below start from."""
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    _, x0, y = npo.problem()
    rho = npo.rho()
    res = m.cg_nonneg(y, rho=rho, x0=x0, **KW)
    yield m, x0, y, rho, res
    m.close()


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def run_project_planes(m, arrs, L, npix, rho, off=0):
    """One call on fresh device copies `off` floats into their buffers: z', u', r' [L, npix], sums [4, L]; checks the guards."""
    import torch
    n = L * npix
    bufs = {}
    for name, a in arrs.items():
        b = torch.full((n + 12,), 123.0, dtype=torch.float32, device="cuda:0")
        b[off: off + n] = _dev(a.ravel())
        bufs[name] = b
    sums = m.nn_project_planes_dev(*(bufs[k][off:] for k in ("x", "z", "u", "r")), L, npix, rho)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, h in host.items():
        assert np.all(h[:off] == 123.0) and np.all(h[off + n:] == 123.0), (k, "written outside its L x npix floats")
    assert np.array_equal(host["x"][off: off + n].view(np.uint32), arrs["x"].ravel().view(np.uint32))
    return tuple(host[k][off: off + n].reshape(L, npix) for k in ("z", "u", "r")) + (sums,)


def planes_case(L, npix, seed):
    """kernel_arrays per plane (x + u exactly 0, +-0, denormals), each plane its own draw, and the float64 reference per plane."""
    planes = [kernel_arrays(npix, seed + 10 * l) for l in range(L)]
    arrs = {k: np.stack([p[i] for p in planes]) for i, k in enumerate(("x", "u", "z", "r"))}
    cases = []
    for l in range(L):
        x, u, z, r = planes[l]
        zn, un, dv, rn = project_ref(x, u, z, r, RHO[l])
        cases.append(dict(n=npix, x=x, u=u, z=z, r=r, zn=zn, un=un, dv=dv, rn=rn))
    return arrs, cases


@pytest.mark.parametrize("L", [1, 2, 5])
def test_project_planes_kernel_matches_numpy(dev, L):
    """L x (72 x 76) through aligned pointers: every plane base is 16-byte aligned, the 16-byte path.  With L = 5 also 5543 floats per
    plane (plane bases 3 l floats off: planes 1 - 3 take the scalar path, planes 0 and 4 the 16-byte path with a tail of 3), 3 floats
    per plane (fewer elements than threads), 96 x 96 (three blocks a plane, three trips a thread) and, L = 2, the 72 x 76 planes one
    float off (every plane on the scalar path).  The rule of tests/test_gpu_nonneg.py: z', u' to the bit and the count exactly, r
    within ten times the error prior_add shows against NumPy on L x 72 x 76 arrays (measured here, and itself under 1e-5), the
    float64 sums to 1e-12, no set sign bit in z', the same bits from a second call."""
    import torch
    m = dev[0]
    na, nb = 72, 76
    mt = build_model(po.rect_problem(na, nb, L))
    try:
        rng = np.random.default_rng(40 + L)
        er, ec = (rng.standard_normal(mt.ishape).astype(np.float32) for _ in range(2))
        q_t = _dev(ec)
        mt.prior_add_dev(_dev(er), q_t, 9.0)
        torch.cuda.synchronize()
        er64 = er.astype(np.float64)
        got = q_t.cpu().numpy()
        bound = 10 * max_err(got, ec.astype(np.float64) + 9.0 * (orc.diff_r_t(orc.diff_r(er64)) + orc.diff_c_t(orc.diff_c(er64))))
    finally:
        mt.close()
    assert 0 < bound < 1e-5
    calls = [(na * nb, 0)]
    if L == 2:
        calls += [(na * nb, 1)]
    if L == 5:
        calls += [(5543, 0), (96 * 96, 0)]
    rho = np.array(RHO[:L])
    for npix, off in calls:
        arrs, cases = planes_case(L, npix, 7 + L)
        gz, gu, gr, sums = run_project_planes(m, arrs, L, npix, rho, off)
        gz2, gu2, gr2, sums2 = run_project_planes(m, arrs, L, npix, rho, off)
        for a, b in ((gz, gz2), (gu, gu2), (gr, gr2)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(sums, sums2) and sums.shape == (4, L)
        for l in range(L):
            e = check_nn(cases[l], "r", gz[l], gu[l], gr[l], sums[:, l], bound)
            print(f"L = {L} npix = {npix} off = {off} plane {l} rho {RHO[l]:g}: r {e:.2e} (bound {bound:.2e})")
    if L == 5:                                                         # 3 floats a plane: every plane but 0 and 4 unaligned
        x = np.array([[1.5, -2.0, 0.0], [-0.0, 3.0, -1.0], [2.0, 2.0, 2.0], [-1.0, -1.0, -1.0], [0.25, -0.5, 1e-40]], dtype=np.float32)
        u = np.array([[-0.5, 1.0, -0.0], [0.0, -3.0, 4.0], [-2.0, 1.0, 0.5], [0.5, 2.0, 1.0], [0.25, 0.25, 0.0]], dtype=np.float32)
        z, r = np.abs(x[::-1]).copy(), (x * 3 + 1).astype(np.float32)
        gz, gu, gr, sums = run_project_planes(m, dict(x=x, u=u, z=z, r=r), 5, 3, rho)
        d = lambda a: a.astype(np.float64)  # noqa: E731
        for l in range(5):
            zn, un, dv, rn = project_ref(x[l], u[l], z[l], r[l], RHO[l])
            assert np.array_equal(gz[l], zn) and np.array_equal(gu[l], un) and not np.any(np.signbit(gz[l]))
            assert np.max(np.abs(gr[l] - rn)) <= bound * np.max(np.abs(rn))
            want = [np.sum((d(x[l]) - d(zn)) ** 2), np.sum((d(zn) - d(z[l])) ** 2), float(np.sum(zn == 0)), np.sum(d(gr[l]) ** 2)]
            assert sums[2, l] == want[2] and np.allclose(sums[:, l], want, rtol=1e-12, atol=0.0)
    t = _dev(np.zeros(8))
    for bad in ([0.0, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -2.0], [1e-60, 1.0]):
        with pytest.raises(ValueError, match="rho"):
            m.nn_project_planes_dev(t, t.clone(), t.clone(), t.clone(), 2, 4, np.array(bad))


# ---- the solver against the restatement ----------------------------------------------------------------------------------------------
def compare_run(res, refs, rho, label, planes=npo.COMPARED):
    worst = np.zeros(5)
    for l in planes:
        e = npo.compare_plane(res.x[l], res.primal[:, l], res.dual[:, l], res.grad_norm[:, l], res.n_active[:, l], rho[l], refs[l],
                              f"{label} plane {l}")
        worst = np.maximum(worst, e)
    print(f"{label} worst: z {worst[0]:.2e}, |x - z| {worst[1]:.2e}, |z - z_prev| {worst[2]:.2e}, r.r {worst[3]:.2e}, n_active off by {int(worst[4])}")


def empty_plane_rests(res, l=npo.EMPTY):
    n = res.x[l].size
    assert not res.x[l].any() and not np.any(np.signbit(res.x[l]))
    for t in (res.primal, res.dual, res.grad_norm):
        assert np.all(np.isfinite(t)) and not t[:, l].any()
    assert np.all(res.n_active[:, l] == n)


def test_solver_matches_oracle_plane_by_plane(dev):
    """4 x 4 on the shared problem from its start, refresh 0: every compared plane within B_Z (z, relative to the plane's max|z|) and
    B_R (r.r, |x - z|, |z - z_prev|) of ``nonneg_oracle.admm`` on that plane alone; n_active off by at most the restatement's count
    of near-zero entries; the plane without data returns exact zeros and a finite trace."""
    m, x0, y, rho, res = dev
    assert res.nit == npo.OUTER and res.x.shape == (npo.L, npo.N, npo.N) and np.array_equal(res.rho, rho)
    for t in (res.primal, res.dual, res.grad_norm, res.n_active):
        assert t.shape == (npo.OUTER + 1, npo.L)
    assert res.x.min() >= 0.0 and np.isfinite(res.x).all()
    compare_run(res, npo.reference(), rho, "shared")
    empty_plane_rests(res)
    again = m.cg_nonneg(y, rho=rho, x0=x0, **KW)                       # the same inputs give the same bits
    assert all(np.array_equal(a, b) for a, b in zip(res[:5], again[:5]))


def test_masked_samples_are_ignored(dev):
    """``weights=`` as the 0/1 mask of ``huber_planes_oracle.sample_mask`` with NaN under the zero weights."""
    m, x0, y, rho, res = dev
    mask = hp.sample_mask(y.shape[1])
    w = np.tile(mask, (npo.L, 1))
    rw = m.cg_nonneg(np.where(w > 0, y, np.nan), rho=rho, x0=x0, weights=w, **KW)
    assert rw.nit == npo.OUTER and np.isfinite(rw.x).all() and m.data_weights is None
    compare_run(rw, npo.reference(masked=True), rho, "masked")
    empty_plane_rests(rw)
    assert max_err(rw.x[0], res.x[0]) > 100 * npo.B_Z                  # the mask is felt (the host test, on the oracle)


def test_rotated_field_model(dev):
    """The same comparison on ``spectro_blind.MRSBlurred`` at 8.2 degrees, two planes."""
    from surfh_amd.spectro_blind import MRSBlurred
    c = npo.rotated_case()
    n = npo.N * npo.N
    for r in c["ref"].values():                                        # the preconditions of the host test on this problem's own run
        assert np.all(np.array(r["near"]) < 0.01 * n) and np.all(r["trace"][:, 3] >= 0.02 * n)
    m = _plane_model(c["case"]["sotf"], npo.N, npo.N, cls=MRSBlurred, spec=c["case"]["spec"], pts=c["case"]["pointings"])
    try:
        res = m.cg_nonneg(c["y"], rho=c["rho"], x0=c["x0"], **KW)
        assert res.nit == npo.OUTER
        compare_run(res, c["ref"], c["rho"], "rotated 8.2", planes=(0, 1))
        est = m.nonneg_rho(npo.MU, npo.MUR)
        assert est.shape == (2,) and np.max(np.abs(est - c["rho"]) / c["rho"]) < 1e-5
    finally:
        m.close()


def test_refreshed_and_carried_residuals_agree(dev):
    m, x0, y, rho, res = dev
    a = m.cg_nonneg(y, rho=rho, x0=x0, **dict(KW, refresh=1))
    for l in npo.COMPARED:
        e_z = max_err(a.x[l], res.x[l])
        e_r = float(np.max(np.abs(a.grad_norm[:, l] ** 2 - res.grad_norm[:, l] ** 2) / res.grad_norm[:, l] ** 2))
        print(f"plane {l}: refresh 1 against 0: z {e_z:.2e} (bound {npo.B_Z:.1e}), r.r {e_r:.2e} (bound {npo.B_R:.1e})")
        assert e_z < npo.B_Z and e_r < npo.B_R
    assert not np.array_equal(a.grad_norm, res.grad_norm)              # the refresh did recompute
    empty_plane_rests(a)


def test_penalty_forms(dev):
    """A number is the array of that number, bit for bit; None is ``nonneg_rho``, which is the float64 quotient of the same probe."""
    m, x0, y, rho, _ = dev
    kw = dict(KW, outer=2, inner=2)
    a, b = m.cg_nonneg(y, rho=6.0, x0=x0, **kw), m.cg_nonneg(y, rho=np.full(npo.L, 6.0), x0=x0, **kw)
    assert all(np.array_equal(u, v) for u, v in zip(a[:6], b[:6])) and np.array_equal(a.rho, np.full(npo.L, 6.0))
    est = m.nonneg_rho(npo.MU, npo.MUR)
    e = np.max(np.abs(est - rho) / rho)
    print(f"nonneg_rho {np.round(est, 4).tolist()} against float64: {e:.2e}")
    assert est.shape == (npo.L,) and e < 1e-5
    c = m.cg_nonneg(y, x0=x0, **kw)
    d = m.cg_nonneg(y, rho=est, x0=x0, **kw)
    assert np.array_equal(c.rho, est) and all(np.array_equal(u, v) for u, v in zip(c[:5], d[:5]))
    mask = hp.sample_mask(y.shape[1])
    w = np.tile(mask, (npo.L, 1))
    want = npo.probe_rho(mask, planes=(0, npo.QUIET))
    got = m.nonneg_rho(npo.MU, npo.MUR, weights=w)
    assert all(abs(got[l] - v) < 1e-5 * v for l, v in want.items()) and m.data_weights is None


def test_single_image_is_squeezed():
    m1 = _plane_model(hp.sotf(0), hp.N, hp.N)
    try:
        _, x0, y = npo.problem()
        r1 = m1.cg_nonneg(y[0], mu=npo.MU, mu_reg=npo.MUR, x0=x0[0], outer=2, inner=2, refresh=0)
        assert r1.x.shape == (hp.N, hp.N) and r1.x.min() >= 0.0 and isinstance(r1.rho, float) and r1.nit == 2
        assert r1.rho == m1.nonneg_rho(npo.MU, npo.MUR)
        for t in (r1.primal, r1.dual, r1.grad_norm, r1.n_active):
            assert t.shape == (3,)
    finally:
        m1.close()


def test_every_plane_must_meet_the_tolerance(dev):
    """The quiet plane (amplitude 1e-3) meets at outer iteration 1 a tolerance the others meet at iteration k > 1 only: the loop
    runs to k, not to 1, and not on to ``outer``; the planes keep iterating meanwhile (the quiet plane's trace is the full run's)."""
    m, x0, y, rho, res = dev
    crit = np.maximum(rho[None] * res.primal, res.dual)[1:]            # rows: outer iterations 1 ..
    worst = crit.max(axis=1)
    ks = [k for k in range(1, len(worst) - 1) if worst[k] < 0.999 * worst[:k].min()]
    assert ks, worst
    k = ks[0] + 1                                                      # as an outer-iteration count: 1 < k < outer
    tol = worst[k - 1] * 1.0001 / (npo.N * npo.N)
    assert 1 < k < npo.OUTER and crit[0, npo.QUIET] < npo.N * npo.N * tol < worst[0]
    rt = m.cg_nonneg(y, rho=rho, x0=x0, **dict(KW, tol=tol))
    assert rt.nit == k and rt.primal.shape == (k + 1, npo.L)
    assert np.array_equal(rt.primal, res.primal[: k + 1]) and np.array_equal(rt.dual, res.dual[: k + 1])
    assert np.array_equal(rt.grad_norm, res.grad_norm[: k + 1])
    assert rt.x.min() >= 0.0 and not np.array_equal(rt.x[npo.QUIET], res.x[npo.QUIET])
    r1 = m.cg_nonneg(y, rho=rho, x0=x0, **dict(KW, tol=1e30))          # met by every plane at once
    assert r1.nit == 1 and r1.primal.shape == (2, npo.L)


def test_refusals_leave_the_plan_usable(dev):
    from surfh_amd import _lib
    m, x0, y, rho, res = dev
    for kw, word in ((dict(rho=0.0), "rho"), (dict(rho=np.inf), "rho"), (dict(rho=[1, 2, np.nan, 4, 5]), "rho"), (dict(rho=[1.0, 2.0]), "rho"),
                     (dict(inner=0), "inner"), (dict(outer=-1), "outer")):
        with pytest.raises(ValueError, match=word):
            m.cg_nonneg(y, **dict(dict(KW, rho=rho, x0=x0), **kw))
    # the library's own checks, behind the wrapper's
    L = m._L
    yf, out, tr, nit = y.astype(np.float32).ravel(), np.empty(m.isize, np.float32), np.zeros((2, 4, npo.L)), ctypes.c_int32()
    good = dict(plan=m._plan, y=_lib.fptr(yf), rho=_lib.dptr(rho), outer=1, inner=1, x=_lib.fptr(out), trace=_lib.dptr(tr), nit=ctypes.byref(nit))

    def call(**kw):
        a = dict(good, **kw)
        return L.surfh_cg_planes_nonneg(a["plan"], a["y"], 1.0, 0.0, a["rho"], None, a["outer"], a["inner"], 0.0, 0, a["x"], a["trace"], a["nit"])

    for name in ("plan", "y", "rho", "x", "trace", "nit"):
        assert call(**{name: None}) != 0 and "null" in L.surfh_last_error().decode()
    for bad in (-1.0, 0.0, float("nan"), float("inf"), 1e-60):
        r = rho.copy()
        r[npo.L - 1] = bad
        assert call(rho=_lib.dptr(r)) != 0 and "rho[4]" in L.surfh_last_error().decode()
    assert call(inner=0) != 0 and "inner" in L.surfh_last_error().decode()
    assert call(outer=-1) != 0 and "outer" in L.surfh_last_error().decode()
    assert call() == 0 and nit.value == 1
    again = m.cg_nonneg(y, rho=rho, x0=x0, **KW)
    assert all(np.array_equal(a, b) for a, b in zip(res[:5], again[:5]))
    # a plan with templates, and one with an imager term
    cfg = problems.config1()
    mt = build_model(cfg, with_ref=False)
    try:
        from surfh_amd.imager import ImagerModel, synthetic_filters
        yt, ot = np.zeros(mt.osize, np.float32), np.empty(mt.isize, np.float32)
        rt, tt = np.ones(cfg["Lc"]), np.zeros((2, 4, cfg["Lc"]))
        args = (mt._plan, _lib.fptr(yt), 1.0, 0.0, _lib.dptr(rt), None, 1, 1, 0.0, 0, _lib.fptr(ot), _lib.dptr(tt), ctypes.byref(nit))
        assert L.surfh_cg_planes_nonneg(*args) != 0 and "template" in L.surfh_last_error().decode()
        f0 = mt.forward(cfg["maps"])
        im = ImagerModel(mt, synthetic_filters(cfg["wavel"], 2), decim=2)
        mt.set_imager(im)
        mt.set_imager_data(np.ones(im.osize), 1.0)
        assert L.surfh_cg_planes_nonneg(*args) != 0 and "imager" in L.surfh_last_error().decode()
        assert np.array_equal(mt.forward(cfg["maps"]), f0)
    finally:
        mt.close()


def test_other_solvers_keep_their_bits(dev):
    """cg, mmmg and mmmg(delta=) on the same plan before and after the non-negative runs: identical bits."""
    m, x0, y, rho, _ = dev

    def bits():
        out = []
        for fn, kw in ((m.cg, {}), (m.mmmg, {}), (m.mmmg, dict(delta=hp.DELTA))):
            x, gn, _ = fn(y, mu=npo.MU, mu_reg=npo.MUR, x0=x0, max_iter=5, **kw)
            out += [x, gn]
        return out

    before = bits()
    m.cg_nonneg(y, rho=rho, x0=x0, **dict(KW, outer=2, inner=3, refresh=1))
    m.cg_nonneg(y, **dict(KW, outer=1, inner=2))
    with pytest.raises(ValueError):
        m.cg_nonneg(y, rho=-1.0)
    after = bits()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_writes_the_nonneg_results(tmp_path):
    """-np 192: the driver's smallest image that holds the band-1C field of view (tests/test_gpu_huber_planes.py); 251 with --angle."""
    from click.testing import CliRunner
    sp = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    dd = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(dd)
    out = str(tmp_path / "res")
    r = CliRunner().invoke(dd.main, ["-np", "192", "--planes", "2", "-ni", "3", "--nonneg", "--inner", "2", "--out", out])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = out + "_nn"
    assert os.path.isdir(d) and not os.path.exists(out) and r.output.count("Outer iteration n°") == 4
    x, tr, crit = (np.load(os.path.join(d, f)) for f in ("res_x.npy", "nn_trace.npy", "criterion.npy"))
    assert x.shape == (2, 192, 192) and x.min() >= 0.0 and np.isfinite(x).all()
    assert tr.shape == (4, 4, 2) and np.all(np.isfinite(tr)) and np.array_equal(tr[-1, 3], np.sum(x == 0, axis=(1, 2)))
    assert crit.shape == (2,) and crit[1] < crit[0]
    r = CliRunner().invoke(dd.main, ["--angle", "8.2", "-np", "251", "-ni", "5", "--nonneg", "--outer", "2", "--inner", "2", "--rho", "40",
                                     "--out", out, "--quiet"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    x, tr = np.load(os.path.join(d, "res_x.npy")), np.load(os.path.join(d, "nn_trace.npy"))
    assert x.shape == (251, 251) and x.min() >= 0.0 and tr.shape == (3, 4, 1) and tr[-1, 3, 0] == np.sum(x == 0)
