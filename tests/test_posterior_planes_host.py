"""Plane-wise posterior sampling without a GPU: the float64 restatement (tests/posterior_planes_oracle.py) obeys the covariance
identity plane by plane -- so the device comparison in tests/test_gpu_posterior_planes.py is against a sampler that samples what
it claims -- and the Python layer refuses bad arguments before it reaches the library."""
import os
import re

import numpy as np
import pytest

import huber_planes_oracle as hp
import posterior_oracle as po
import posterior_planes_oracle as ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_covariance_identity_plane_by_plane():
    """5 planes of 96 x 96, 216 samples each, weights ``po.identity_weights`` with NaN data at weight 0, mu = 4, mu_reg = 9, 400
    draws of seed 0: for the probes ones, checkerboard and random on every plane v^T b~_l has mean v^T b_l within 5 standard
    errors and a variance within 5 sqrt(2 / 399) = 0.354 of v^T Q_l v; the prior's share of v^T Q_l v is below 1e-3 for ones and
    above 0.999 for the checkerboard."""
    mu, mu_reg, draws, seed = (po.IDENTITY[k] for k in ("mu", "mu_reg", "draws", "seed"))
    w, yn, y0 = ppo.identity_problem()
    ops = [ppo.plane(l) for l in range(hp.L)]
    V = ppo.probes()
    proj = {(l, k): np.empty(draws) for l in range(hp.L) for k in V}
    for d in range(draws):
        eps = ppo.draw(seed, d)
        for l, op in enumerate(ops):
            bt = ppo.rhs(op, yn[l], w[l], mu, mu_reg, ppo.of_plane(eps, l))
            assert np.all(np.isfinite(bt))
            for k, v in V.items():
                proj[l, k][d] = np.vdot(v[0], bt)
    b = [mu * op.adjoint(w[l] * y0[l])[0] for l, op in enumerate(ops)]
    dev, ratio = ppo.identity_checks(lambda l, k, v: proj[l, k], lambda l, v: float(np.vdot(v[0], b[l])),
                                     lambda l, k, v: po.quad_parts(v, ops[l].forward(v), w[l], mu, mu_reg))
    assert dev < 5.0 and ratio < 5.0 * np.sqrt(2.0 / (draws - 1))


def test_streams_run_over_the_flat_index_of_the_stack():
    """Plane l of a draw is the slice of one stream over [L][...]: not a stream of its own, and eta wraps inside the plane."""
    eps = ppo.draw(7, 2, L=3, na=5, nb=7, nout=11)
    assert np.array_equal(eps[0].ravel(), po.randn(33, 7, po.STREAM_Y, 2)) and np.array_equal(eps[1][2].ravel(), po.randn(35, 7, po.STREAM_R, 2, start=70))
    e = ppo.eta(eps[1], eps[2], 9.0)
    l, i, j = 1, 4, 6                                                   # the last row and column of the middle plane
    assert e[l, i, j] == 3.0 * ((eps[1][l, 0, j] - eps[1][l, i, j]) + (eps[2][l, i, 0] - eps[2][l, i, j]))


def _stub(batched=True):
    """A model object without a plan that knows its sizes."""
    from surfh_amd.blurred2d import Blurred2D
    m = object.__new__(Blurred2D)
    m.n_planes, m.batched, m.imshape = (3 if batched else 1), batched, (4, 5)
    m.ishape, m.oshape = ((3, 4, 5), (3, 6)) if batched else ((4, 5), (6,))
    m._plan = None
    return m


def test_wrapper_checks_come_before_any_library_call():
    """``sample_posterior`` on an object without a plan: every argument check raises ``ValueError`` first."""
    m = _stub()
    y = np.zeros(m.osize)
    ok = dict(mu=1.0, mu_reg=1.0, n_samples=2, max_iter=2)
    for bad, word in ((dict(mu=0.0), "mu ="), (dict(mu=-1.0), "mu ="), (dict(mu=float("nan")), "mu ="), (dict(mu=float("inf")), "mu ="),
                      (dict(mu_reg=-1.0), "mu_reg"), (dict(mu_reg=float("nan")), "mu_reg"), (dict(mu_reg=[1.0, 2.0, 3.0]), "mu_reg"),
                      (dict(n_samples=1), "n_samples"), (dict(n_samples=0), "n_samples"), (dict(max_iter=-1), "max_iter")):
        with pytest.raises(ValueError, match=word):
            m.sample_posterior(y, **{**ok, **bad})
    with pytest.raises(ValueError, match="data size"):
        m.sample_posterior(np.zeros(m.osize + 1), **ok)
    with pytest.raises(ValueError, match="x0 size"):
        m.sample_posterior(y, x0=np.zeros(3), **ok)
    K, no, ni = 2, m.osize, m.isize
    good = (np.zeros((K, no)), np.zeros((K, ni)), np.zeros((K, ni)))
    for pert, word in (((good[0], good[1]), "perturbations must be"), ((np.zeros((K, no + 1)), good[1], good[2]), "eps_y"),
                       ((good[0], np.zeros((K, ni - 1)), good[2]), "eps_r"), ((good[0], good[1], np.zeros((K, 2 * ni))), "eps_c")):
        with pytest.raises(ValueError, match=word):
            m.sample_posterior(y, perturbations=pert, **ok)
    for pert in ((good[0], None, None),                                   # no prior noise is no option while mu_reg > 0
                 (np.zeros((3, no)), good[1], good[2])):                  # K rows each
        with pytest.raises(ValueError):
            m.sample_posterior(y, perturbations=pert, **ok)


def test_improper_plane_reports_infinity():
    """A plane whose first r.r is exactly 0 over all samples drew nothing: var = std = +inf there, the device's numbers elsewhere."""
    from surfh_amd import posterior
    L, shape = 3, (3, 4, 5)
    rng = np.random.default_rng(0)
    x_map, mean = rng.standard_normal(60).astype(np.float32), rng.standard_normal(60)
    var = rng.random(60) + 0.5
    var[20:40] = 0.0
    gn = rng.random((5, L))
    first, last = np.array([2.0, 0.0, 1e-300]), np.array([1.0, 0.0, 0.0])
    assert np.array_equal(posterior.improper_planes(first), [False, True, False])
    r = posterior.planes_result(x_map, mean, var, gn, 3, first, last, 4, shape, squeeze=False)
    assert r.var.shape == r.std.shape == r.mean.shape == r.x_map.shape == shape and r.grad_norm.shape == (4, L) and r.nit == 3 and r.n_samples == 4
    assert np.all(np.isposinf(r.var[1])) and np.all(np.isposinf(r.std[1]))
    assert np.array_equal(r.var[[0, 2]], var.reshape(shape)[[0, 2]]) and np.array_equal(r.std[[0, 2]], np.sqrt(var.reshape(shape)[[0, 2]]))
    assert np.array_equal(r.mean.ravel(), mean) and np.array_equal(r.rr_first, first) and np.array_equal(r.rr_last, last)
    assert var[20] == 0.0                                                 # the caller's array is left alone
    # a single image: squeezed shapes, the same rule
    r1 = posterior.planes_result(x_map[:20], mean[:20], np.zeros(20), gn[:, :1], 4, np.zeros(1), np.zeros(1), 2, (4, 5), squeeze=True)
    assert r1.var.shape == (4, 5) and np.all(np.isposinf(r1.std)) and r1.grad_norm.shape == (5,) and r1.rr_first == 0.0 and isinstance(r1.rr_last, float)


def test_entry_points_exist():
    """No GPU and no library: the header declares the entry points, the binding lists them, the classes have the methods."""
    with open(os.path.join(ROOT, "include", "surfh_amd.h")) as f:
        header = f.read()
    names = ("surfh_cg_planes_sample", "surfh_po_planes_rhs", "surfh_debug_po_planes")
    for name in names:
        assert re.search(r"^int " + name + r"\(surfh_plan \*plan,", header, re.M), name
    assert re.search(r"^int surfh_po_planes_moments\(int32_t L,", header, re.M)
    from surfh_amd import _lib, posterior, spectro_blind, spectro_blind_rectangle
    from surfh_amd.blurred2d import Blurred2D
    assert set(names) | {"surfh_po_planes_moments"} <= set(_lib.EXPORTS)
    for cls in (Blurred2D, spectro_blind.MRSBlurred, spectro_blind_rectangle.MRSBlurred):
        assert callable(getattr(cls, "sample_posterior", None)) and callable(getattr(cls, "po_planes_dev", None)), cls
    assert callable(spectro_blind.QuadCriterion_MRS_2D.sample)
    for fn in ("sample_posterior_planes", "po_planes_rhs", "po_planes_moments", "PlanesPosteriorResult"):
        assert hasattr(posterior, fn)
    with pytest.raises(ValueError, match="samples"):
        posterior.po_planes_moments(np.zeros((2, 3)), np.zeros((4, 2, 4)))


def test_criterion_sample_refuses_a_huber_prior():
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D
    m = _stub()
    q = QuadCriterion_MRS_2D(1.0, np.zeros(m.osize), m, 2.0, delta=0.1)
    with pytest.raises(ValueError, match="Gaussian"):
        q.sample(n_samples=2)
    with pytest.raises(ValueError, match="n_samples"):                    # the quadratic criterion reaches the model's checks
        QuadCriterion_MRS_2D(1.0, np.zeros(m.osize), m, 2.0).sample(n_samples=1)
