"""The float64 oracles of the 3MG solvers with a potential argument: ``huber_oracle.mmmg``, ``vox_oracle.mmmg``,
``huber_planes_oracle.solve_plane`` and ``robust_oracle.mmmg`` run unchanged, on the hyperbolic and the Hebert-Leahy potential of
``surfh_amd.potentials`` as well as on Huber's.

Those oracles reach their potential through three functions, ``phi(u, delta)``, ``dphi(u, delta)`` and ``weight(u, delta)``, and
hand the threshold through untouched.  A threshold here is ``Th(delta, kind)``: a float that also names its potential.  Inside
``patched()`` the three functions of the oracle modules look at that name: "huber", and every plain float, goes to the oracle's own
function -- so with "huber" every array is the existing oracle's, bit for bit -- and the other kinds to the float64 restatements
of ``surfh_amd.potentials`` (the forms without a delta^2 factor: delta = inf is u^2 / 2, u and 1 exactly).  Nothing else of the
oracles changes: the loop, the basis, the majorant and the operation order are theirs.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import huber_oracle as ho  # noqa: E402
import huber_planes_oracle as hpo  # noqa: E402
import robust_oracle as ro  # noqa: E402
import vox_oracle as vo  # noqa: E402
from surfh_amd import potentials as P  # noqa: E402

NEW_KINDS = ("hyperbolic", "hebert_leahy")


class Th(float):
    """A threshold that names its potential."""

    def __new__(cls, delta, kind="huber"):
        o = float.__new__(cls, delta)
        o.kind = P.kind_name(kind)
        return o


def _dispatch(name, own):
    new = getattr(P, name)

    def f(u, delta):
        kind = getattr(delta, "kind", "huber")
        return own(u, delta) if kind == "huber" else new(u, float(delta), kind)
    return f


@contextlib.contextmanager
def patched():
    """The oracle modules' phi / dphi / weight read the kind of a ``Th`` threshold inside this block."""
    saved = [(mod, name, getattr(mod, name)) for mod in (ho, vo, ro) for name in ("phi", "dphi", "weight")]
    own = {name: getattr(ho, name) for name in ("phi", "dphi", "weight")}
    try:
        for mod, name, _ in saved:
            setattr(mod, name, _dispatch(name, own[name]))
        yield
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)


def mmmg(op, data, mu, mu_reg, delta, x0, potential="huber", **kw):
    """``huber_oracle.mmmg`` with the priors' potential"""
    with patched():
        return ho.mmmg(op, data, mu, mu_reg, Th(delta, potential), x0, **kw)


def mmmg_vox(op, data, mu, spat_reg, spat_delta, spec_reg, spec_delta, x0, spat_potential="huber", spec_potential="huber", **kw):
    """``vox_oracle.mmmg`` with the potential of the in-plane families and of the wavelength family"""
    with patched():
        return vo.mmmg(op, data, mu, spat_reg, Th(spat_delta, spat_potential), spec_reg, Th(spec_delta, spec_potential), x0, **kw)


def solve_plane(l, y_l, x0_l, delta=hpo.DELTA, potential="huber", **kw):
    """``huber_planes_oracle.solve_plane`` with the priors' potential"""
    with patched():
        return hpo.solve_plane(l, y_l, x0_l, Th(delta, potential), **kw)


def mmmg_robust(op, data, mu, data_delta, mu_reg, delta, x0, w=None, potential="huber", data_potential="huber", **kw):
    """``robust_oracle.mmmg`` with the potential of the priors and of the data term"""
    with patched():
        return ro.mmmg(op, data, mu, Th(data_delta, data_potential), mu_reg, Th(delta, potential), x0, w=w, **kw)


def share_small_weights(diffs, delta, potential, below=0.9):
    """share of the differences ``diffs`` (a list of arrays) whose weight w(u) is under ``below``"""
    u = np.concatenate([np.ravel(d) for d in diffs])
    return float(np.mean(P.weight(u, delta, potential) < below))


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


# ---- the regimes of the device comparisons (tests/test_gpu_potentials.py), chosen on the oracle alone; tests/test_potentials_host.py
# checks their preconditions: at the oracle's final iterate at least 30 % of the differences (of the scaled residuals, for the data
# term) have w < 0.9, and the iterate is at least 1e-2 (relative) away from the delta = inf iterate of the same start.
# w < 0.9 is |u| > 0.48 delta for the hyperbolic potential and |u| > delta / 3 for Hebert-Leahy's (Huber: |u| > 1.11 delta), so the
# existing regimes' prior thresholds serve unchanged; the data term's does not (below).
NIT = 8
MAPS = dict(mu_reg=5e3, delta=0.1)                       # test_gpu_huber.py's "rough" on problems.config1()
VOX = dict(zip(("spat_reg", "spat_delta", "spec_reg", "spec_delta"), vo.REGIMES["both"][:4]))     # 32 x 48 x 48
PLANES = dict(mu_reg=hpo.MUR, delta=hpo.DELTA)           # blurred_case, 5 planes of 96 x 96
# robust_oracle.config1_case(), its "huber" regime, with the threshold at 2 sigma instead of 3: the scaled residuals are N(0, 1) but
# for the spikes, so at 3 only 16 % of them have a hyperbolic weight under 0.9 (|t| > 1.45); at 2 it is |t| > 0.97, a third
ROBUST = dict(data_delta=2.0, delta=0.1)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def maps_case():
    def make():
        import problems
        cfg = problems.config1()
        om = problems.oracle_model(cfg, box="direct")
        rng = np.random.default_rng(1)
        y0 = om.forward(cfg["maps"])
        y = y0 + rng.standard_normal(y0.shape) * 1e-2 * np.sqrt(np.mean(y0 ** 2))
        x0 = cfg["maps"] + 0.1 * np.random.default_rng(3).standard_normal(om.ishape)
        return dict(cfg=cfg, om=om, y=y, x0=x0)
    return cached("maps", make)


def maps_run(potential, delta=None):
    c = maps_case()
    d = MAPS["delta"] if delta is None else delta
    return cached(("maps", potential, d), lambda: mmmg(c["om"], c["y"], 1.0, MAPS["mu_reg"], d, c["x0"], potential, max_iter=NIT))


def vox_case():
    def make():
        cfg, om, cube, y = vo.small_cfg()
        return dict(cfg=cfg, om=om, cube=cube, y=y, x0=vo.start("rough", om, cube))
    return cached("vox", make)


def vox_run(spat_potential, spec_potential, inf=False):
    c = vox_case()
    sd, ld = (float("inf"),) * 2 if inf else (VOX["spat_delta"], VOX["spec_delta"])
    return cached(("vox", spat_potential, spec_potential, inf),
                  lambda: mmmg_vox(c["om"], c["y"], 1.0, VOX["spat_reg"], sd, VOX["spec_reg"], ld, c["x0"], spat_potential, spec_potential,
                                   max_iter=NIT))


def planes_run(potential, l, delta=None):
    d = PLANES["delta"] if delta is None else delta
    _, x0, y = cached("planes", hpo.problem)
    return cached(("planes", potential, l, d), lambda: solve_plane(l, y[l], x0[l], d, potential, mu_reg=PLANES["mu_reg"], max_iter=NIT))


def robust_run(data_potential, data_delta=None):
    c = ro.config1_case()
    dd = ROBUST["data_delta"] if data_delta is None else data_delta
    return cached(("robust", data_potential, dd),
                  lambda: mmmg_robust(c["om"], c["y"], 1.0, dd, c["mur"], ROBUST["delta"], c["starts"]["huber"], w=c["w"],
                                      data_potential=data_potential, max_iter=NIT))
