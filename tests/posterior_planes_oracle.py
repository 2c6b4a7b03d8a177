"""Float64 side of the plane-wise posterior sampler (``MRSBlurred.sample_posterior``, include/surfh_amd.h: surfh_cg_planes_sample):
``posterior_oracle`` (generator, eta, perturb_data, lcg, sample) applied plane by plane to the 2-D oracle of
``huber_planes_oracle``.  Plane l is its own problem

    Q_l = mu A_l^T W_l A_l + mu_reg (Dr^T Dr + Dc^T Dc),   b_l = mu A_l^T W_l y_l,

and a draw's noise is one stream per vector over the flat index of the whole stack: eps_y over [L][n_out] (stream 0), eps_r and
eps_c over [L][Na][Nb] (streams 1 and 2) -- plane l reads its slice.
"""
from __future__ import annotations

import numpy as np

import huber_planes_oracle as hp
import posterior_oracle as po


class Plane:
    """One plane of a 2-D oracle as the [1, Na, Nb] -> [n_out] operator ``posterior_oracle`` works on (with its sizes)."""

    def __init__(self, bo):
        self.bo = bo
        self.ishape = (1,) + tuple(bo.ishape)
        self.oshape = (int(np.prod(bo.slices_shape)),)
        self.isize, self.osize = int(np.prod(self.ishape)), self.oshape[0]

    def forward(self, x):
        return self.bo.forward(np.asarray(x).reshape(self.ishape)[0])

    def adjoint(self, y):
        return self.bo.adjoint(np.asarray(y).reshape(self.oshape))[None]


def plane(l):
    return Plane(hp.plane_op(l).bo)


def n_out():
    return int(np.prod(hp.batch_oracle().slices_shape))


def draw(seed, sample, L=hp.L, na=hp.N, nb=hp.N, nout=None):
    """(eps_y [L, n_out], eps_r, eps_c [L, na, nb]) of draw ``sample``: the generator's streams 0, 1, 2 over the flat indices."""
    nout = n_out() if nout is None else nout
    return (po.randn(L * nout, seed, po.STREAM_Y, sample).reshape(L, nout), po.randn(L * na * nb, seed, po.STREAM_R, sample).reshape(L, na, nb),
            po.randn(L * na * nb, seed, po.STREAM_C, sample).reshape(L, na, nb))


def of_plane(eps, l):
    """Plane l's share of a draw, in the shapes ``posterior_oracle`` takes: (eps_y [n_out], eps_r, eps_c [1, na, nb])."""
    return eps[0][l], eps[1][l:l + 1], eps[2][l:l + 1]


def eta(eps_r, eps_c, mu_reg):
    """sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c) on [L, na, nb]: the differences wrap inside every plane."""
    return po.eta(eps_r, eps_c, mu_reg)


def rhs(op, y_l, w_l, mu, mu_reg, eps_l):
    """b~_l = mu A_l^T W_l y~_l + eta_l."""
    return po.rhs(op, y_l, w_l, mu, mu_reg, eps_l)[0]


def sample(op, w_l, mu, mu_reg, eps_l, xhat_l, max_iter):
    """``po.sample`` on one plane: dict with "e" and "x" [na, nb] and the r.r trace "grad_norm"."""
    out = po.sample(op, w_l, mu, mu_reg, eps_l, np.asarray(xhat_l)[None], max_iter)
    out["e"], out["x"] = out["e"][0], out["x"][0]
    return out


# ---- the covariance identity per plane: v^T b~_l has mean v^T b_l and variance v^T Q_l v ----------------------------------------
def identity_problem():
    """Weights ``po.identity_weights`` [L, n_out], data at the statistical scale they state with NaN at weight 0, and the data with
    0 there: (w, y_nan, y0).  The signal of every plane is scaled to rms 10 (``po.identity_data``)."""
    mu = po.IDENTITY["mu"]
    truth, _, _ = hp.problem()
    y = hp.batch_oracle().forward(truth)
    rms = np.sqrt(np.mean(y ** 2, axis=1, keepdims=True))
    y = y * (10.0 / np.where(rms > 0, rms, 1.0))
    w = po.identity_weights(y.size).reshape(y.shape)
    keep = w > 0
    y = y + np.random.default_rng(1).standard_normal(y.shape) / np.sqrt(mu * np.where(keep, w, 1.0))
    return w, np.where(keep, y, np.nan), np.where(keep, y, 0.0)


def probes(na=hp.N, nb=hp.N):
    """ones, checkerboard, random as [1, na, nb] (``po.probes`` without its map-selecting probe)."""
    v = po.probes((1, na, nb))
    return {k: v[k] for k in ("ones", "checker", "random")}


def identity_checks(project, mean_of, quad_of, L=hp.L):
    """The bands of ``po.identity_check`` on every plane and probe.  ``project(l, name, v)`` -> the draws' v^T b~_l [draws],
    ``mean_of(l, v)`` -> v^T b_l, ``quad_of(l, name, v)`` -> (data, prior) parts of v^T Q_l v.  Returns (worst |mean deviation| in
    standard errors, worst |variance ratio - 1|)."""
    draws = po.IDENTITY["draws"]
    worst_dev = worst_ratio = 0.0
    V = probes()
    for l in range(L):
        shares = {}
        for name, v in V.items():
            qd, qp = quad_of(l, name, v)
            shares[name] = qp / (qd + qp)
            dev, ratio = po.identity_check(f"plane {l} {name}", project(l, name, v), mean_of(l, v), qd + qp, draws)
            worst_dev, worst_ratio = max(worst_dev, abs(dev)), max(worst_ratio, abs(ratio - 1.0))
        assert shares["ones"] < 1e-3 and shares["checker"] > 0.999, (l, shares)
    print(f"identity, worst over planes and probes: mean off by {worst_dev:.2f} standard errors, |variance ratio - 1| = {worst_ratio:.3f}")
    return worst_dev, worst_ratio
