"""Float64 restatement of the plane-wise 3MG solver under the isotropic prior coupling (surfh_mmmg_huber_planes_ex,
``MRSBlurred.mmmg(delta=, coupling="isotropic")``): ``coupled_oracle.mmmg`` applied plane by plane to the problem of
``huber_planes_oracle`` -- a plane is a [1, N, N] map, so "isotropic" there is the plane's own coupling.

    J_l(x_l) = mu |y_l - A_l x_l|^2 / 2 + mu_reg_l sum_ij phi_delta_l(sqrt(u_r^2 + u_c^2))

The threshold is on the group magnitude: DELTA = huber_planes_oracle.DELTA sqrt(2).  Scanned on the oracle (8 iterations, the share
of groups with w < 0.9 at the last iterate and the relative l2 distance to the "none" iterate at the same threshold):
    huber        planes 0, 1, 4: 0.49 .. 0.51 and 2.6e-2;   plane 2 (amplitude 1e-3): share 0
    hyperbolic   planes 0, 1, 4: 0.87         and 2.4e-2;   plane 2: share 0
    hebert_leahy plane 0: above 0.95 -- outside the project's 5 % .. 95 % band: kernel checks only, no solver comparison
The comparison tolerance is hp.TOL_X = 2e-4: the coupling moves the iterate by more than 100 times that.
tests/test_coupled_planes_host.py asserts these preconditions without a GPU.
"""
from __future__ import annotations

import numpy as np

import coupled_oracle as co
import huber_planes_oracle as hp

DELTA = hp.DELTA * np.sqrt(2.0)
KINDS = ("huber", "hyperbolic")                 # the kinds of the solver comparison
ACTIVE = (0, 1, 4)                              # the planes whose groups are on both sides of the threshold


def solve_plane(l, y_l, x0_l, kind="huber", coupling="isotropic", delta=DELTA, mu_reg=hp.MUR, mask=None):
    """``coupled_oracle.mmmg`` on plane l alone (``hp.solve_plane`` with a coupling and a kind); x comes back as [N, N]."""
    op = hp.plane_op(l, mask)
    data = y_l if mask is None else np.where(mask > 0, y_l, 0.0)
    ref = co.mmmg(op, data, hp.MU, mu_reg, delta, np.asarray(x0_l)[None], coupling=coupling, potential=kind, max_iter=hp.NIT)
    ref["x"] = ref["x"][0]
    return ref


_CACHE = {}


def reference(kind="huber", coupling="isotropic"):
    """The per-plane oracle runs of the shared problem at DELTA, computed once per process: {l: result of solve_plane}."""
    key = (kind, coupling)
    if key not in _CACHE:
        _, x0, y = hp.problem()
        _CACHE[key] = {l: solve_plane(l, y[l], x0[l], kind, coupling) for l in hp.COMPARED}
    return _CACHE[key]


def share_small_weights(x_l, kind="huber", delta=DELTA):
    """share of the pixels of one plane whose group weight w(m) is under 0.9"""
    return co.share_small_weights(np.asarray(x_l)[None], delta, "isotropic", kind)
