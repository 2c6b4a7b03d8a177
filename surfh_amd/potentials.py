"""The potentials of the 3MG solvers: names, the kind codes of the C ABI (include/surfh_amd.h: surfh_set_potential) and float64
NumPy restatements of ``phi``, ``phi'`` and ``w(u) = phi'(u) / u``.

All are normalised like the project's Huber: ``phi(u) ~ u^2 / 2`` near 0, ``w(0) = 1``, and ``delta = inf`` is exactly the
quadratic potential.  With ``t = u / delta``:

    huber (0)         u^2 / 2 inside delta, delta (|u| - delta / 2) beyond       w = 1 or delta / |u|
    hyperbolic (1)    delta^2 (sqrt(1 + t^2) - 1)      = u^2 / (1 + sqrt(1 + t^2))   w = 1 / sqrt(1 + t^2)
    hebert_leahy (2)  delta^2 log(1 + t^2) / 2         = (u^2 / 2) log1p(t^2) / t^2  w = 1 / (1 + t^2)

The right-hand forms carry no ``delta^2`` factor, so ``delta = inf`` gives ``u^2 / 2``, ``u`` and ``1`` with no NaN; ``phi'`` is
``u w``.  Every ``w`` is in (0, 1] and non-increasing in |u|: ``phi(sqrt(.))`` is concave, the Geman-Reynolds majorant holds.
Hebert-Leahy is not convex: 3MG still descends, to a local minimum that depends on the start.

The spatial prior of the maps also has a **coupling** (include/surfh_amd.h: surfh_set_prior_coupling), orthogonal to the potential:
which circular first differences ``u_r = Dr x``, ``u_c = Dc x`` share one ``phi``:

    none (0)       sum_t sum_ij phi(u_r) + phi(u_c)              one potential per difference (the default)
    isotropic (1)  sum_t sum_ij phi(sqrt(u_r^2 + u_c^2))         edges pay the same at every angle to the pixel grid
    vector (2)     sum_ij phi(sqrt(sum_t u_r^2 + u_c^2))         one edge per pixel for all maps: edges co-locate across maps

``delta`` is then the threshold on the **group magnitude** (the square root): for comparable behaviour it grows like ``sqrt(2)``
under "isotropic" and like ``sqrt(2 T)`` under "vector".  ``group_magnitude`` and ``prior_value`` restate both in float64;
``installed_coupling`` sets the coupling for one call.

A model's potentials are plan state in three slots (``SLOTS``); ``installed(model, spatial=..., spectral=..., data=...)`` sets them
for the duration of a solve and puts back what the plan held, the way ``installed_weights`` treats the data weights.
"""
from __future__ import annotations

import numpy as np

from . import _lib

KINDS = {"huber": 0, "hyperbolic": 1, "hebert_leahy": 2}
NAMES = tuple(KINDS)                                       # NAMES[code] is the name
SLOTS = {"spatial": 0, "spectral": 1, "data": 2}


def kind_code(potential) -> int:
    """The C ABI's code of a potential given by name (or by code).  ``ValueError`` on anything else."""
    if isinstance(potential, str) and potential in KINDS:
        return KINDS[potential]
    if isinstance(potential, (int, np.integer)) and not isinstance(potential, bool) and 0 <= int(potential) < len(NAMES):
        return int(potential)
    raise ValueError(f"potential must be one of {', '.join(NAMES)}, not {potential!r}")


def kind_name(potential) -> str:
    return NAMES[kind_code(potential)]


COUPLINGS = {"none": 0, "isotropic": 1, "vector": 2}
COUPLING_NAMES = tuple(COUPLINGS)                          # COUPLING_NAMES[code] is the name


def coupling_code(coupling) -> int:
    """The C ABI's code of a prior coupling given by name (or by code).  ``ValueError`` on anything else."""
    if isinstance(coupling, str) and coupling in COUPLINGS:
        return COUPLINGS[coupling]
    if isinstance(coupling, (int, np.integer)) and not isinstance(coupling, bool) and 0 <= int(coupling) < len(COUPLING_NAMES):
        return int(coupling)
    raise ValueError(f"coupling must be one of {', '.join(COUPLING_NAMES)}, not {coupling!r}")


def coupling_name(coupling) -> str:
    return COUPLING_NAMES[coupling_code(coupling)]


def need_delta_coupling(coupling, delta):
    """A coupling of the quadratic prior means nothing (every coupling of it is the same prior): ``ValueError``."""
    if coupling_code(coupling) != 0 and delta is None:
        raise ValueError(f"coupling {coupling_name(coupling)!r} needs delta: a coupling of the quadratic prior means nothing")


def need_delta(potential, delta, what="delta"):
    """A potential other than Huber without its threshold means nothing (the term is then quadratic): ``ValueError``."""
    if kind_code(potential) != 0 and delta is None:
        raise ValueError(f"potential {kind_name(potential)!r} needs {what}: a potential of the quadratic term means nothing")


def _ut(u, delta):
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(over="ignore"):
        t = u / float(delta)
        return u, t, t * t


def weight(u, delta, potential="huber"):
    """``w(u) = phi'(u) / u`` in float64, ``w(0) = 1``."""
    k = kind_code(potential)
    u, t, t2 = _ut(u, delta)
    if k == 0:
        a = np.abs(u)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(a <= delta, 1.0, float(delta) / a)
    if k == 1:
        return 1.0 / np.sqrt(1.0 + t2)
    return 1.0 / (1.0 + t2)


def dphi(u, delta, potential="huber"):
    """``phi'(u)`` in float64: ``u w(u)`` (Huber: ``u`` inside, ``delta sign u`` beyond)."""
    k = kind_code(potential)
    u = np.asarray(u, dtype=np.float64)
    if k == 0:
        return np.where(np.abs(u) <= delta, u, np.copysign(float(delta), u))
    return u * weight(u, delta, k)


def phi(u, delta, potential="huber"):
    """``phi(u)`` in float64, in the forms without a ``delta^2`` factor.  ``huber`` is ``fusion.huber_phi``, bit for bit."""
    k = kind_code(potential)
    if k == 0:
        from .fusion import huber_phi
        return huber_phi(u, delta)
    u, t, t2 = _ut(u, delta)
    if k == 1:
        return u * u / (1.0 + np.sqrt(1.0 + t2))
    small = t2 < 1e-8
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(small, 1.0 - 0.5 * t2, np.log1p(t2) / np.where(small, 1.0, t2))
    return 0.5 * u * u * ratio


def group_magnitude(x, coupling="none"):
    """The magnitudes the potential is applied to, in float64, for maps ``x`` ``[T, Na, Nb]`` and the circular differences
    ``u_r = roll(x, 1, axis 1) - x``, ``u_c = roll(x, 1, axis 2) - x``: "none" ``[2, T, Na, Nb]`` (|u_r|, |u_c|), "isotropic"
    ``[T, Na, Nb]`` (sqrt(u_r^2 + u_c^2)), "vector" ``[Na, Nb]`` (sqrt(sum_t u_r^2 + u_c^2))."""
    c = coupling_code(coupling)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError(f"group_magnitude takes maps [T, Na, Nb], not an array of shape {x.shape}")
    ur, uc = np.roll(x, 1, axis=1) - x, np.roll(x, 1, axis=2) - x
    if c == 0:
        return np.abs(np.stack([ur, uc]))
    m2 = ur * ur + uc * uc
    return np.sqrt(m2 if c == 1 else m2.sum(axis=0))


def prior_value(x, delta, potential="huber", coupling="none"):
    """``sum phi(m)`` over the magnitudes of ``group_magnitude(x, coupling)`` in float64: the value of the maps' spatial prior
    (before ``mu_reg``); ``delta`` is the threshold on the group magnitude."""
    return float(np.sum(phi(group_magnitude(x, coupling), delta, potential)))


class installed_coupling:
    """``with installed_coupling(model, coupling):`` -- the plan's prior coupling is ``coupling`` inside and what the plan held
    before afterwards, as ``installed`` does for the kinds.  ``None`` leaves it alone.  The name is checked before any library
    call."""

    def __init__(self, model, coupling=None):
        self.model = model
        self.want = None if coupling is None else coupling_code(coupling)

    def __enter__(self):
        self.saved = None
        if self.want is not None:
            self.saved = get_coupling_code(self.model)
            _lib.check(self.model._L.surfh_set_prior_coupling(self.model._plan, self.want))

    def __exit__(self, *exc):
        if self.saved is not None:
            _lib.check(self.model._L.surfh_set_prior_coupling(self.model._plan, self.saved))
        return False


def get_coupling_code(model) -> int:
    import ctypes as C
    out = C.c_int32(-1)
    _lib.check(model._L.surfh_get_prior_coupling(model._plan, C.byref(out)))
    return int(out.value)


class installed:
    """``with installed(model, spatial=..., spectral=..., data=...):`` -- the plan's potential slots hold the given kinds inside
    and what they held before afterwards.  ``None`` leaves a slot alone.  The names are checked before any library call."""

    def __init__(self, model, spatial=None, spectral=None, data=None):
        self.model = model
        self.want = {SLOTS[s]: kind_code(k) for s, k in (("spatial", spatial), ("spectral", spectral), ("data", data)) if k is not None}

    def __enter__(self):
        L, plan = self.model._L, self.model._plan
        self.saved = {slot: get_slot(self.model, slot) for slot in self.want}
        for slot, k in self.want.items():
            _lib.check(L.surfh_set_potential(plan, slot, k))

    def __exit__(self, *exc):
        for slot, k in self.saved.items():
            _lib.check(self.model._L.surfh_set_potential(self.model._plan, slot, k))
        return False


def get_slot(model, slot) -> int:
    k = model._L.surfh_get_potential(model._plan, SLOTS.get(slot, slot))
    if k < 0:
        _lib.check(1)
    return k


class Potentials:
    """The plan-state methods of a ``PlanOwner``."""

    def set_potential(self, slot, potential="huber"):
        """The potential of one of the plan's slots from now on: ``slot`` "spatial" (the priors of the maps, of the planes and of
        the cube's rows and columns), "spectral" (the cube's wavelength prior) or "data" (the robust data term); ``potential``
        "huber" (the default of a new model), "hyperbolic" or "hebert_leahy".  The solvers' ``potential=`` keywords set a slot for
        one call only."""
        if slot not in SLOTS:
            raise ValueError(f"slot must be one of {', '.join(SLOTS)}, not {slot!r}")
        _lib.check(self._L.surfh_set_potential(self._plan, SLOTS[slot], kind_code(potential)))

    def get_potential(self, slot) -> str:
        if slot not in SLOTS:
            raise ValueError(f"slot must be one of {', '.join(SLOTS)}, not {slot!r}")
        return NAMES[get_slot(self, slot)]

    def set_prior_coupling(self, coupling="none"):
        """The coupling of the maps' spatial prior from now on: "none" (one potential per difference, the default of a new
        model), "isotropic" or "vector" (module docstring).  ``mmmg(delta=...)``, ``mmmg(data_delta=...)``, ``huber_prior_dev`` and
        ``huber_curv_dev`` follow it, their ``delta`` then the threshold on the group magnitude; the plane-wise and voxel-wise
        solvers refuse a plan whose coupling is not "none".  ``mmmg(coupling=...)`` sets it for one call only."""
        _lib.check(self._L.surfh_set_prior_coupling(self._plan, coupling_code(coupling)))

    def get_prior_coupling(self) -> str:
        return COUPLING_NAMES[get_coupling_code(self)]
