"""GPU parity of the rotated-field 2-D operator ``spectro_blind.MRSBlurred`` (the reference's surfh/Models/spectro_blind.py):
bilinear gridding taps at a rotated local grid on the beta-sum channel of the HIP library, against the real reference's outputs
(tests/golden/mrs_blurred_rot*.npz) and the float64 checker (tests/rotated_oracle.py); its solvers, the deconvolution driver
with ``--angle`` and the full-size problem."""
import importlib.util
import os
import time

import numpy as np
import pytest

import rotated_oracle as ro
from helpers import make_ifu, rel
from oracle import surfh_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


def _coords(pts):
    from surfh_amd import instru
    return instru.CoordList([instru.Coord(a, b) for a, b in pts])


def model_of(case, cls=None):
    if cls is None:
        from surfh_amd.spectro_blind import MRSBlurred as cls
    return cls(case["sotf"], case["alpha_axis"], case["beta_axis"], make_ifu(case["spec"]), case["step_deg"], _coords(case["pointings"]))


def _dot_gap(m, seed):
    rng = np.random.default_rng(seed)
    v, uu = rng.random(m.isize), rng.random(m.osize)
    l = float(np.vdot(m.rmatvec(uu), v)); r = float(np.vdot(uu, m.matvec(v)))
    return abs(l - r) / abs(r)


def test_rotated_single_image_vs_reference():
    g = np.load(os.path.join(G, "mrs_blurred_rot.npz"))
    case = ro.small_case()
    bo, m = ro.oracle_of(case), model_of(case)
    try:
        x = np.random.default_rng(int(g["x_seed"])).random(case["imshape"])
        u = np.random.default_rng(int(g["u_seed"])).standard_normal(m.osize)
        a, a_ref = m.adjoint(u), m.adjoint_ref(u)
        e = dict(fwd=rel(m.forward(x), g["y"]), adj_ref=rel(a_ref, g["adjoint_ref"]),    # the real reference's outputs
                 adj=rel(a, bo.adjoint(u)), fwadj=rel(m.fwadj(x), bo.adjoint(bo.forward(x))))
        d = rel(a, a_ref)
        gap = _dot_gap(m, 7)
        print(e, f"|A^T u - A_ref^T u| / |A_ref^T u| = {d:.2e}, dot gap {gap:.1e}")
        assert max(e.values()) < TOL
        assert gap < 1e-6
        assert d > 100 * TOL                     # the reference's back-projection really is another operator
    finally:
        m.close()


def test_rotated_batched_over_wavelength():
    L = 40
    case = ro.small_case(L=L)
    bo, m = ro.oracle_of(case), model_of(case)
    try:
        rng = np.random.default_rng(1)
        x = rng.random((L,) + case["imshape"])
        u = rng.standard_normal(m.oshape)
        y, a, ar = m.forward(x), m.adjoint(u), m.adjoint_ref(u)
        assert y.shape == (L, 3 * 12 * 6) and a.shape == ar.shape == (L,) + case["imshape"]
        yo, ao, aro = bo.forward(x), bo.adjoint(u), bo.adjoint_ref(u)
        e = max(max(rel(y[l], yo[l]), rel(a[l], ao[l]), rel(ar[l], aro[l])) for l in range(L))
        print(f"rotated x{L}: worst plane {e:.2e}")
        assert e < TOL
    finally:
        m.close()


def test_rotated_data_to_img_vs_reference():
    g = np.load(os.path.join(G, "mrs_blurred_rot_d2i.npz"))
    case = ro.d2i_case()
    m = model_of(case)
    try:
        wm, gl = m.data_to_img(g["y"])
        assert np.array_equal(wm != 0, g["covered"])
        assert rel(gl, g["global_img"]) < 1e-13 and rel(wm, g["weighted_mean"]) < 1e-13
        x = np.random.default_rng(int(g["x_seed"])).random(case["imshape"]) * case["x_scale"]
        y = m.forward(x)
        assert rel(y, g["y"]) < TOL
        wm2, gl2 = m.data_to_img(y)                       # fp32 data: the thresholds may flip a pixel at their edge
        flips = float(np.mean((wm2 != 0) != g["covered"])), float(np.mean((gl2 != 0) != (g["global_img"] != 0)))
        print(f"data_to_img on the HIP forward: threshold flips {flips}")
        assert max(flips) < 1e-3 and rel(gl2, g["global_img"]) < 1e-3
    finally:
        m.close()


def test_rotated_plane_wise_cg_and_mmmg():
    """CG and 3MG on L = 5 planes (one without data, which stays at rest) against the checker's lcg / mmmg plane by plane, and the
    criterion mirror on the rotated model (criterion_2D.QuadCriterion_MRS_2D(..., model_spectro=spectro_blind.MRSBlurred(...)))."""
    from surfh_amd.spectro_blind import QuadCriterion_MRS_2D
    L, nit, mu, mur = 5, 10, 1.0, 0.05
    case = ro.small_case(L=L)
    bo, m = ro.oracle_of(case), model_of(case)
    N = case["imshape"][0]
    try:
        y = bo.forward(np.random.default_rng(4).random((L, N, N)))
        y[3] = 0.0
        x, gn, n = m.cg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit)
        assert n == nit and gn.shape == (nit + 1, L) and x.shape == (L, N, N)
        assert not x[3].any() and not gn[:, 3].any() and np.isfinite(x).all()
        for l in (0, 2, 4):
            op = ro.PlaneOp(ro.oracle_of(case, sotf=case["sotf"][l]))
            ref = orc.lcg(op, y[l], mu, mur, np.zeros((1, N, N)), tol=1e-12, max_iter=nit)
            gr = np.array(ref["grad_norm"])
            assert rel(x[l], ref["x"][0]) < 5e-3, l
            assert float(np.max(np.abs(gn[:5, l] - gr[:5]) / gr[:5])) < 1e-2 and gn[-1, l] < 1e-2 * gn[0, l]
        xm, gm, nm = m.mmmg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit)
        assert nm == nit and gm.shape == (nit + 1, L) and not xm[3].any() and not gm[:, 3].any() and np.isfinite(xm).all()
        live = [0, 1, 2, 4]
        assert rel(xm[live], x[live]) < 1e-4 and float(np.max(np.abs(gm[:, live] ** 2 - gn[:, live]) / gn[:, live])) < 1e-3
        for l in (0, 4):
            op = ro.PlaneOp(ro.oracle_of(case, sotf=case["sotf"][l]))
            ref = orc.mmmg(op, y[l], mu, mur, np.zeros((1, N, N)), max_iter=nit)
            k = 7
            assert float(np.max(np.abs(gm[:k, l] - ref["grad_norm"][:k]) / np.array(ref["grad_norm"][:k]))) < 1e-3, l
    finally:
        m.close()
    one = dict(case, sotf=case["sotf"][2])
    m1 = model_of(one)
    try:
        crit = QuadCriterion_MRS_2D(mu, y[2], m1, mur)
        res = crit.run_method("lcg", maximum_iterations=nit, value_init=0.0)
        x1, gn1, _ = m1.cg(y[2], mu=mu, mu_reg=mur, x0=np.zeros((N, N)), max_iter=nit)
        assert res.nit == nit and rel(res.x.reshape(N, N), x1) == 0.0 and rel(x1, x[2]) < 1e-4
        assert crit.get_crit_val(res.x) < crit.get_crit_val(np.zeros((N, N)))
        res = crit.run_method("qmm", maximum_iterations=nit, value_init=0.0)
        xm1, _, _ = m1.mmmg(y[2], mu=mu, mu_reg=mur, x0=np.zeros((N, N)), max_iter=nit)
        assert res.nit == nit and rel(res.x.reshape(N, N), xm1) == 0.0 and rel(xm1, xm[2]) < 1e-4
    finally:
        m1.close()


def test_rotated_device_resident_loop():
    import torch
    L, mu, mur, nit, refresh = 6, 1.0, 0.05, 9, 4
    case = ro.small_case(L=L)
    bo, m = ro.oracle_of(case), model_of(case)
    N = case["imshape"][0]
    try:
        y = bo.forward(np.random.default_rng(14).random((L, N, N)))
        y[4] = 0.0
        x_ref, gn_ref, _ = m.cg(y, mu=mu, mu_reg=mur, x0=None, max_iter=nit, refresh=refresh)
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
        live = [0, 1, 2, 3, 5]
        e_x, e_r = rel(x[live], x_ref[live]), float(np.max(np.abs(rr[live] - gn_ref[-1][live]) / gn_ref[-1][live]))
        print(f"rotated device-resident CG vs host-buffer CG: x {e_x:.1e}, r.r {e_r:.1e}")
        assert e_x < 1e-4 and e_r < 1e-2
        assert not x[4].any() and rr[4] == 0.0
    finally:
        m.close()


def _driver():
    sp = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    dd = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(dd)
    return dd


@pytest.mark.parametrize("planes", [1, 4])
def test_rotated_deconvolution_driver_end_to_end(tmp_path, planes):
    from click.testing import CliRunner
    dd = _driver()
    out = str(tmp_path / "res")
    niter, N = 20, 251
    args = ["--angle", "8.2", "-np", str(N), "-ni", str(niter), "--planes", str(planes), "--out", out, "--quiet"]
    r = CliRunner().invoke(dd.main, args + (["--data_to_img"] if planes == 1 else []))
    assert r.exit_code == 0, r.output
    x = np.load(os.path.join(out, "res_x.npy"))
    crit = np.load(os.path.join(out, "criterion.npy"))
    data = np.load(os.path.join(out, "data.npy"))
    assert x.shape == ((N, N) if planes == 1 else (planes, N, N))
    assert len(crit) == 2 and crit[1] < 1e-2 * crit[0]
    prob = dd.build_problem(N, planes, 19940407, None, angle=8.2)
    spec = orc.ChannelSpec(3.2 / 3600, 3.7 / 3600, (0.0, 0.0), 8.2, 0.196, 21, float(np.mean([3100, 3610])), prob["ifu"].wavel_axis, "1C")
    pts = [(c.alpha, c.beta) for c in prob["pointings"]]
    sotf = prob["sotf"] if planes > 1 else prob["sotf"][None]
    bo = ro.RotatedOracle(sotf, prob["alpha_axis"], prob["beta_axis"], spec, prob["step_deg"], pts)
    truth = prob["truth"] if planes > 1 else prob["truth"][None]
    yo = bo.forward(truth)
    assert rel(data.reshape(yo.shape), yo) < TOL
    if planes == 1:
        for suffix in ("", "_fit"):
            am, a = np.load(os.path.join(out, f"adj_mean{suffix}.npy")), np.load(os.path.join(out, f"adj{suffix}.npy"))
            assert am.shape == a.shape == (N, N) and np.isfinite(am).all() and (a != 0).any()
        wm, gl = ro.RotatedOracle(prob["sotf"], prob["alpha_axis"], prob["beta_axis"], spec, prob["step_deg"], pts).data_to_img(yo[0])
        assert rel(np.load(os.path.join(out, "adj.npy")), gl) < 1e-4

    def Q(v):
        return bo.adjoint(bo.forward(v)) + 5.0 * ((2 * v - np.roll(v, 1, -2) - np.roll(v, -1, -2)) + (2 * v - np.roll(v, 1, -1) - np.roll(v, -1, -1)))
    xo = np.zeros_like(truth); b = bo.adjoint(yo); rr_ = b - Q(xo); d = rr_.copy()
    rr = np.sum(rr_ * rr_, axis=(1, 2))
    for it in range(niter):
        q = Q(d); step = rr / np.sum(d * q, axis=(1, 2)); xo += step[:, None, None] * d
        rr_ = b - Q(xo) if it % 50 == 0 else rr_ - step[:, None, None] * q
        rn = np.sum(rr_ * rr_, axis=(1, 2)); d = rr_ + (rn / rr)[:, None, None] * d; rr = rn
    e = rel(x.reshape(xo.shape), xo)
    print(f"rotated deconvolution driver ({planes} plane(s)) vs float64 CG after {niter} iterations: {e:.2e}")
    assert e < 1e-3


def test_rotated_full_size():
    """The band-1C geometry at 8.2 degrees on 512 x 512 x 2048 planes: shapes, finite values, a few CG iterations; the device
    loop's it/s beside the rectangle class on the same problem is printed as a record (not a gate)."""
    import torch
    from surfh_amd.spectro_blind import MRSBlurred as Rot
    from surfh_amd.spectro_blind_rectangle import MRSBlurred as Rect
    N, Lc, s = 512, 2048, ro.STEP_DEG
    ax = orc.synthetic_axes(N, s)
    sotf = orc.ir2fr(orc.gaussian_psf(np.linspace(6.53, 7.65, Lc), ro.STEP), (N, N))
    pts = [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s), (3 * s, 5 * s)]
    rng = np.random.default_rng(5)
    x = rng.random((Lc, N, N), dtype=np.float32)
    dev = torch.device("cuda:0")
    rates = {}
    for name, cls, angle in (("rotated", Rot, 8.2), ("rectangle", Rect, 0.0)):
        spec = orc.ChannelSpec(3.2 / 3600, 3.7 / 3600, (0.0, 0.0), angle, 0.196, 21, 3355.0, np.linspace(6.6, 7.6, 10), "1C")
        t0 = time.time()
        m = cls(sotf, ax, ax, make_ifu(spec), s, _coords(pts))
        t_plan = time.time() - t0
        try:
            y = m.forward(x)
            assert y.shape == (Lc, 4 * 21 * 19) and np.isfinite(y).all()
            if name == "rotated":
                sel = [0, 2047]
                e = rel(y[sel], ro.RotatedOracle(sotf[sel], ax, ax, spec, s, pts).forward(x[sel].astype(np.float64)))
                xh, gn, nit = m.cg(y, mu=1.0, mu_reg=0.05, max_iter=4)
                print(f"rotated x{Lc}: plan {t_plan:.1f}s, forward parity on planes {sel}: {e:.2e}", flush=True)
                assert e < TOL and nit == 4 and gn.shape == (5, Lc) and np.all(gn[-1] < gn[0]) and np.isfinite(xh).all()
                assert xh.shape == (Lc, N, N)
                del xh
            yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32).reshape(-1), device=dev)
            xt = torch.zeros((Lc, N, N), dtype=torch.float32, device=dev)
            m.cg_begin_dev(yt, xt, 1.0, 0.05)
            m.cg_step_dev(2, 50)
            torch.cuda.synchronize()
            k = 10
            t1 = time.time()
            m.cg_step_dev(k, 50)
            torch.cuda.synchronize()
            rates[name] = k / (time.time() - t1)
            assert np.isfinite(m.cg_rr()).all() and torch.isfinite(xt).all().item()
            del yt, xt
        finally:
            m.close()
    print(f"plane-wise CG on 512x512x{Lc}, band 1C, 4 pointings: rotated (8.2 deg) {rates['rotated']:.1f} it/s, "
          f"rectangle {rates['rectangle']:.1f} it/s", flush=True)
