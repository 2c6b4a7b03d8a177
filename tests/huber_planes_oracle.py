"""Float64 restatement of the plane-wise Huber criterion (surfh_mmmg_huber_planes): ``huber_oracle.mmmg`` applied plane by plane
to the 2-D oracle ``orc.BlurredOracle``, and the problem the host and the device tests share.

    J_l(x_l) = mu |y_l - A_l x_l|^2 / 2 + mu_reg sum_{k in r,c} sum phi_delta(D_k x_l)

The problem is that of tests/test_gpu_variants.py::blurred_case (L = 5 planes of 96 x 96, 12 slits, 3 pointings).  The planes differ
in the amplitude of their truth -- a piecewise-constant image under a fine texture, amplitude 1 in four planes and 1e-3 in plane 2 --
and start from the truth plus noise of a tenth of that amplitude, so that one threshold delta leaves plane 2 fully quadratic and puts
a large share of the other planes' differences on the linear branch.  Plane 3 has no data (y_3 = 0) and starts from 0.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import huber_oracle as ho  # noqa: E402
import problems  # noqa: E402
from oracle import surfh_oracle as orc  # noqa: E402

L, N, NIT = 5, 96, 8
MU, MUR, DELTA = 1.0, 1.5, 0.025
AMPL = (1.0, 1.0, 1e-3, 1.0, 1.0)
QUIET, EMPTY = 2, 3                       # the fully quadratic plane, the plane without data
COMPARED = (0, 1, 2, 4)
SPEC = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
WAV = np.linspace(7.0, 8.2, L)
_S = problems.STEP_DEG
PTS = [(0.0, 0.0), (2 * _S, -3 * _S), (-4 * _S, 1 * _S)]

# Bounds of the device comparison: the map-domain Huber tolerances (1e-4 in x, 2e-4 in |g| over 8 iterations)
# scaled by how much less exactly this operator is evaluated than the one they were measured on, times 2 -- the rule of the
# voxel-wise solver.  E_B = 3.6e-7 is the relative error of adjoint(forward(d)) of the map-domain model against its oracle;
# E_PLANE is the same figure of this plane-wise model, the worst of three seeds, measured with the operator this solver was
# added to.
E_B, E_PLANE = 3.6e-7, 2.9e-7
SCALE = 2 * max(1.0, E_PLANE / E_B)
TOL_X, TOL_G = 1e-4 * SCALE, 2e-4 * SCALE


class PlaneOp:
    """One plane of the 2-D oracle presented as a [1, N, N] operator (the checker's solvers and priors act on [T, N, N]);
    ``mask`` (0/1 per sample) makes it M A, the operator of the problem with the masked samples removed."""

    def __init__(self, bo, mask=None):
        self.bo, self.mask = bo, mask
        self.ishape = (1,) + tuple(bo.ishape)

    def forward(self, x):
        y = self.bo.forward(np.asarray(x).reshape(self.ishape)[0])
        return y if self.mask is None else y * self.mask

    def adjoint(self, y):
        return self.bo.adjoint(y if self.mask is None else y * self.mask)[None]


def axes():
    return orc.synthetic_axes(N, _S)


def sotf(planes=None):
    s = orc.ir2fr(orc.gaussian_psf(WAV, problems.STEP), (N, N))
    return s if planes is None else s[planes]


def plane_op(l, mask=None):
    ax = axes()
    return PlaneOp(orc.BlurredOracle(sotf(l), ax, ax, SPEC, _S, PTS), mask)


def batch_oracle():
    ax = axes()
    return orc.BlurredOracle(sotf(), ax, ax, SPEC, _S, PTS)


def problem():
    """truth [L, N, N], start x0 [L, N, N], data y [L, n_out] (plane EMPTY zeroed, its start 0)."""
    rng = np.random.default_rng(23)
    base = np.zeros((N, N))
    base[20:60, 30:80] = 1.0
    base[50:85, 10:45] += 0.5
    truth = np.stack([a * (base + 0.05 * rng.standard_normal((N, N))) for a in AMPL])
    x0 = truth + 0.1 * np.asarray(AMPL)[:, None, None] * rng.standard_normal(truth.shape)
    y = batch_oracle().forward(truth)
    y = y + 1e-2 * np.sqrt(np.mean(y ** 2, axis=1, keepdims=True)) * rng.standard_normal(y.shape)
    y[EMPTY] = 0.0
    x0[EMPTY] = 0.0
    return truth, x0, y


def solve_plane(l, y_l, x0_l, delta=DELTA, mu=MU, mu_reg=MUR, max_iter=NIT, mask=None):
    """``huber_oracle.mmmg`` on plane l alone; x comes back as [N, N]."""
    op = plane_op(l, mask)
    data = y_l if mask is None else np.where(mask > 0, y_l, 0.0)
    ref = ho.mmmg(op, data, mu, mu_reg, delta, np.asarray(x0_l)[None], max_iter=max_iter)
    ref["x"] = ref["x"][0]
    return ref


def sample_mask(n_out):
    """0/1 data weights over one plane's samples (about a quarter masked), the same for every plane"""
    return (np.random.default_rng(41).random(n_out) > 0.25).astype(np.float64)


def share_beyond(x, delta):
    """fraction of the row and column differences of one plane on the linear branch of phi"""
    u = np.abs(np.concatenate([orc.diff_r(x[None]).ravel(), orc.diff_c(x[None]).ravel()]))
    return float(np.mean(u > delta))


_CACHE = {}


def reference(delta=DELTA):
    """The per-plane oracle runs of the shared problem, computed once per process: {l: result of solve_plane}."""
    if delta not in _CACHE:
        _, x0, y = problem()
        _CACHE[delta] = {l: solve_plane(l, y[l], x0[l], delta) for l in COMPARED}
    return _CACHE[delta]
