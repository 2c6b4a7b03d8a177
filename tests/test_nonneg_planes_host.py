"""Non-negative plane-wise deconvolution without a GPU: the preconditions that keep the device comparison
(tests/test_gpu_nonneg_planes.py) from being vacuous, on the float64 side of tests/nonneg_planes_oracle.py; the per-plane scheme
(independent problems, one penalty each) against an independent solver on a small dense batch; and that the entry points exist."""
import os
import re

import numpy as np
import pytest
from scipy.optimize import nnls

import nonneg_oracle as no
import nonneg_planes_oracle as npo
from oracle import surfh_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preconditions_of_the_device_comparison():
    """On every compared plane: under 1 % of the entries within 1e-4 max|x| of the projection's corner at every outer iteration
    (measured 0.02 - 0.5 %), at least 2 % of z at zero in every trace row (0.50, 0.27, 0.18, 0.07, 0.03), at least 30 % of the
    unconstrained lcg iterate after 16 iterations negative (31 - 35 %), and clipping that iterate at least 5 % away from z (7 - 11 %)."""
    _, x0, y = npo.problem()
    rho = npo.rho()
    print("rho:", np.round(rho, 4).tolist())
    assert np.all((rho > 5.5) & (rho < 7.0))                          # the probe's quotients, 6.1 - 6.2 on every plane
    assert not y[npo.EMPTY].any() and not x0[npo.EMPTY].any()
    ref = npo.reference()
    n = npo.N * npo.N
    for l in npo.COMPARED:
        r = ref[l]
        near, active = np.array(r["near"]) / n, r["trace"][:, 3] / n
        free = orc.lcg(npo.hp.plane_op(l), y[l], npo.MU, npo.MUR, x0[l][None], max_iter=npo.OUTER * npo.INNER, refresh=0)["x"][0]
        neg = float(np.mean(free < 0))
        apart = float(np.linalg.norm(np.maximum(free, 0.0) - r["z"]) / np.linalg.norm(r["z"]))
        print(f"plane {l}: near-zero share {near.max():.2e}; active share {' '.join(f'{a:.3f}' for a in active)}; unconstrained "
              f"{neg:.1%} negative; |clip - z| / |z| = {apart:.3f}")
        assert r["nit"] == npo.OUTER and r["trace"].shape == (npo.OUTER + 1, 4)
        assert np.all(near < 0.01)
        assert np.all(active >= 0.02)
        assert neg >= 0.30
        assert apart >= 0.05
        assert r["z"].min() >= 0.0 and r["trace"][0, 0] > 0.0            # the start is infeasible: row 0's r carries rho (z - x0)
    # the planes are not copies of each other: the amplitudes scale the iterates, the operators differ with the wavelength
    assert np.max(ref[npo.QUIET]["z"]) < 1e-2 * np.max(ref[0]["z"])


def test_the_mask_is_felt_and_the_empty_plane_rests():
    _, x0, y = npo.problem()
    rho = npo.rho()
    plain, masked = npo.reference()[0], npo.reference(masked=True)[0]
    d = float(np.linalg.norm(masked["z"] - plain["z"]) / np.linalg.norm(plain["z"]))
    print(f"plane 0: masked against unmasked z {d:.2e} (device bound {npo.B_Z:.1e})")
    assert d > 100 * npo.B_Z
    e = npo.solve_plane(npo.EMPTY, y[npo.EMPTY], x0[npo.EMPTY], rho[npo.EMPTY])
    assert not e["z"].any() and np.all(np.isfinite(e["trace"])) and not e["trace"][:, :3].any()
    assert np.all(e["trace"][:, 3] == npo.N * npo.N)


def test_dense_batch_reaches_nnls_problem_by_problem():
    """Three independent SPD problems with penalties decades apart, run long: the KKT residual of each goes to zero and each is at
    the solution of scipy's nnls -- a plane's result depends on its own rho's value only through the path, not at the end."""
    n = 40
    for k, (seed, scale) in enumerate(((3, 1.0), (4, 0.1), (5, 10.0))):
        rng = np.random.default_rng(seed)
        A = rng.standard_normal((2 * n, n))
        xt = np.where(rng.random(n) < 0.5, 0.0, rng.random(n) + 0.5) - np.where(rng.random(n) < 0.5, 0.0, 1.0)
        y = A @ xt + 0.05 * rng.standard_normal(2 * n)
        Q, b = A.T @ A, A.T @ y
        want, _ = nnls(A, y, maxiter=10000)
        assert 0.2 <= np.mean(want == 0) <= 0.8
        normal = lambda v: Q @ v  # noqa: E731
        rho = scale * float(np.trace(Q) / n)
        res = no.admm(normal, b, rho, outer=6000, inner=3, refresh=10)
        err = np.linalg.norm(res["z"] - want) / np.linalg.norm(want)
        kkt = no.kkt(res["z"], normal, b)
        print(f"problem {k}: rho {rho:.3g}, |z - nnls| / |nnls| = {err:.2e}, KKT {kkt:.2e}")
        assert err < 1e-8 and kkt < 1e-8 * np.linalg.norm(b) and res["z"].min() >= 0.0
        assert kkt < 1e-6 * no.kkt(no.admm(normal, b, rho, outer=5, inner=3)["z"], normal, b)


def test_entry_points_exist():
    """No GPU and no library: the C header declares the two entry points, the binding lists them, the model class has the methods."""
    with open(os.path.join(ROOT, "include", "surfh_amd.h")) as f:
        header = f.read()
    for name in ("surfh_cg_planes_nonneg", "surfh_nn_project_planes_dev"):
        assert re.search(r"^int " + name + r"\(surfh_plan \*plan,", header, re.M), name
    from surfh_amd import _lib
    from surfh_amd.blurred2d import Blurred2D
    from surfh_amd import spectro_blind, spectro_blind_rectangle
    assert {"surfh_cg_planes_nonneg", "surfh_nn_project_planes_dev"} <= set(_lib.EXPORTS)
    for cls in (Blurred2D, spectro_blind.MRSBlurred, spectro_blind_rectangle.MRSBlurred):
        assert callable(getattr(cls, "cg_nonneg", None)) and callable(getattr(cls, "nonneg_rho", None)), cls


def test_driver_flags():
    """raised before any model is built: this runs without a GPU"""
    import importlib.util
    from click.testing import CliRunner
    spec = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    for extra, word in ((["--nonneg", "-m", "qmm"], "lcg"), (["--nonneg", "--delta", "0.1"], "--delta"), (["--rho", "5"], "--nonneg"),
                        (["--outer", "3"], "--nonneg"), (["--inner", "3"], "--nonneg"), (["--nonneg", "--rho", "0"], "--rho"),
                        (["--nonneg", "--rho", "nan"], "--rho"), (["--nonneg", "--inner", "0"], "--inner"),
                        (["--nonneg", "--outer", "0"], "--outer")):
        r = CliRunner().invoke(drv.main, extra)
        assert r.exit_code == 2 and word in r.output, r.output


def test_wrapper_checks_come_before_any_library_call():
    """``cg_nonneg`` on an object without a plan: the argument checks raise first."""
    from surfh_amd.blurred2d import Blurred2D
    m = object.__new__(Blurred2D)
    m.n_planes, m.batched = 3, True
    for kw, word in ((dict(rho=0.0), "rho"), (dict(rho=[1.0, -1.0, 2.0]), "rho"), (dict(rho=[1.0, np.nan, 2.0]), "rho"),
                     (dict(rho=[1.0, 2.0]), "rho"), (dict(inner=0), "inner"), (dict(outer=-1), "outer"), (dict(refresh=-1), "refresh")):
        with pytest.raises(ValueError, match=word):
            m.cg_nonneg(np.zeros(4), **kw)
