"""Float64 restatement of 3MG on the maps under a COUPLED spatial prior: ``huber_oracle.mmmg`` generalised by the prior coupling of
``surfh_amd.potentials`` (and, like ``potentials_oracle``, by the potential kind).

    J(x) = mu |y - A x|^2 / 2 + mu_reg sum_g phi(m_g),    m_g = |u_g|_2 over the group g of differences

    "none"        every difference its own group:                   ``huber_oracle.mmmg`` through ``potentials_oracle.mmmg``, unchanged,
                                                                    so every array formed is that oracle's, bit for bit
    "isotropic"   g = (t, i, j):  m^2 = u_r^2 + u_c^2
    "vector"      g = (i, j):     m^2 = sum_t u_r^2 + u_c^2

u_r = D_r x, u_c = D_c x are ``orc.diff_r`` / ``orc.diff_c``.  phi(sqrt(.)) is concave for every kind, so the Geman-Reynolds
majorant of ``huber_oracle`` holds with the weight of a difference replaced by its group's, w(m_g) = phi'(m_g) / m_g:

    grad  = mu A^T (A x) - b + mu_reg sum_k D_k^T (w(m) D_k x)
    B(x)  = mu (A P)^T (A P) + mu_reg sum_k (D_k P)^T diag(w(m)) (D_k P)

The loop is ``huber_oracle.mmmg``'s, line for line (qmm's literal [-grad, move] basis, the operator images of the move carried);
only the weights and the gradient's phi' = u w(m) differ.  With delta = inf every weight is exactly 1 and the iterates are those of
the quadratic run bit for bit, under every coupling.  ``mmmg_robust`` composes the same prior with the robust data term of
``robust_oracle`` (its whitened operator, its data weights omega(t)).
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import huber_oracle as ho  # noqa: E402
import potentials_oracle as po  # noqa: E402
import robust_oracle as ro  # noqa: E402
from oracle import surfh_oracle as orc  # noqa: E402
from surfh_amd import potentials as P  # noqa: E402

COUPLED = ("isotropic", "vector")


def diffs(x):
    return orc.diff_r(x), orc.diff_c(x)


def magnitude(x, coupling):
    """m of every group: [T, Na, Nb] ("isotropic") or [Na, Nb] ("vector")"""
    ur, uc = diffs(np.asarray(x, dtype=np.float64))
    m2 = ur * ur + uc * uc
    return np.sqrt(m2 if P.coupling_name(coupling) == "isotropic" else m2.sum(axis=0))


def group_weight(x, delta, coupling, potential="huber"):
    """w(m_g) of the group of every difference, in the shape of the maps"""
    w = P.weight(magnitude(x, coupling), delta, potential)
    return np.broadcast_to(w, np.shape(x))


def prior_value(x, delta, coupling, potential="huber"):
    """sum_g phi(m_g)"""
    return float(np.sum(P.phi(magnitude(x, coupling), delta, potential)))


def prior_grad(x, delta, coupling, potential="huber"):
    """sum_k D_k^T (w(m) D_k x)"""
    ur, uc = diffs(x)
    w = group_weight(x, delta, coupling, potential)
    return orc.diff_r_t(w * ur) + orc.diff_c_t(w * uc)


def prior_quad(x, v, delta, coupling, potential="huber"):
    """v^T (sum_k D_k^T diag(w(m(x))) D_k) v"""
    vr, vc = diffs(v)
    return float(np.sum(group_weight(x, delta, coupling, potential) * (vr * vr + vc * vc)))


def crit(op, data, x, mu, mu_reg, delta, coupling, potential="huber"):
    x = np.asarray(x, dtype=np.float64).reshape(op.ishape)
    return float(mu * np.sum((data - op.forward(x)) ** 2) / 2 + mu_reg * prior_value(x, delta, coupling, potential))


def gradient(op, b, x, mu, mu_reg, delta, coupling, potential="huber"):
    """``huber_oracle.gradient``'s operation order with phi' = u w(m)"""
    q = mu * op.adjoint(op.forward(x))
    if mu_reg:
        q = q + mu_reg * prior_grad(x, delta, coupling, potential)
    return q - b


def _run(fwd, ishape, mu, mu_reg, grad_of, crit_of, data_weight_of, delta, coupling, potential, x0, tol, max_iter):
    """``huber_oracle.mmmg``'s loop; the data family's majorant weights are ``data_weight_of(x)`` (ones: the quadratic data term)"""
    x = np.array(x0, dtype=np.float64, copy=True).reshape(ishape)
    ops = [(mu, fwd), (mu_reg, orc.diff_r), (mu_reg, orc.diff_c)]
    move = np.zeros_like(x)
    vd = [np.stack([np.zeros_like(f(x)).ravel()] * 2, axis=1) for _, f in ops]
    step = np.ones((2, 1))
    grad_norm, crits = [], []
    nit = 0
    for it in range(max_iter + 1):
        grad = grad_of(x)
        grad_norm.append(float(np.sqrt(np.sum(grad * grad))))
        crits.append(crit_of(x))
        if it == max_iter or grad_norm[-1] < x.size * tol:
            break
        D = np.stack([-grad.ravel(), move.ravel()], axis=1)
        vd = [np.stack([f(-grad).ravel(), (v @ step).ravel()], axis=1) for (_, f), v in zip(ops, vd)]
        wg = group_weight(x, delta, coupling, potential).ravel()
        ws = [data_weight_of(x, vd[0].shape[0]), wg, wg]
        B = sum(h * ((v * w[:, None]).T @ v) for (h, _), v, w in zip(ops, vd, ws))
        step = -np.linalg.pinv(B) @ (D.T @ grad.ravel()).reshape(2, 1)
        move = (D @ step).reshape(x.shape)
        x = x + move
        nit = it + 1
    return {"x": x, "grad_norm": grad_norm, "nit": nit, "crit": crits}


def mmmg(op, data, mu, mu_reg, delta, x0, coupling="none", potential="huber", tol=1e-12, max_iter=10):
    """3MG on J.  Returns x, grad_norm (|grad| of x0 and of every iterate), nit, crit (J of x0 and of every iterate)."""
    if P.coupling_name(coupling) == "none":
        return po.mmmg(op, data, mu, mu_reg, delta, x0, potential, tol=tol, max_iter=max_iter)
    b = mu * op.adjoint(data)
    return _run(op.forward, op.ishape, mu, mu_reg, lambda x: gradient(op, b, x, mu, mu_reg, delta, coupling, potential),
                lambda x: crit(op, data, x, mu, mu_reg, delta, coupling, potential), lambda x, n: np.ones(n), delta, coupling,
                potential, x0, tol, max_iter)


def mmmg_robust(op, data, mu, data_delta, mu_reg, delta, x0, w=None, coupling="none", potential="huber", data_potential="huber",
                tol=1e-12, max_iter=10):
    """``robust_oracle.mmmg`` with the coupled prior: J = mu sum phi_dd(t) + mu_reg sum_g phi(m_g), t = sqrt(w) (y - A x)"""
    if P.coupling_name(coupling) == "none":
        return po.mmmg_robust(op, data, mu, data_delta, mu_reg, delta, x0, w=w, potential=potential, data_potential=data_potential,
                              tol=tol, max_iter=max_iter)
    aw, yw = ro.whiten(op, data, w)

    def grad_of(x):
        g = -mu * aw.adjoint(P.dphi(yw - aw.forward(x), data_delta, data_potential))
        return g + mu_reg * prior_grad(x, delta, coupling, potential) if mu_reg else g

    def crit_of(x):
        return float(mu * np.sum(P.phi(yw - aw.forward(x), data_delta, data_potential)) + mu_reg * prior_value(x, delta, coupling, potential))

    return _run(aw.forward, aw.ishape, mu, mu_reg, grad_of, crit_of,
                lambda x, n: P.weight(yw - aw.forward(x), data_delta, data_potential).ravel(), delta, coupling, potential, x0, tol,
                max_iter)


def share_small_weights(x, delta, coupling, potential="huber", below=0.9):
    """share of the groups whose weight w(m_g) is under ``below``"""
    return float(np.mean(P.weight(magnitude(x, coupling), delta, potential) < below))


rel = po.rel

# ---- the regimes of the device comparisons (tests/test_gpu_coupled.py), chosen on the oracle alone; tests/test_coupled_host.py
# checks their preconditions: at the oracle's last iterate between 5 % and 95 % of the groups have w < 0.9, and the iterate is at
# least 1e-2 (relative) away from the "none" iterate of the same regime.  The problem is potentials_oracle.maps_case():
# problems.config1() (4 x 64 x 64), the "rough" start, 8 iterations.
# The weight.  At potentials_oracle's mu_reg = 5e3 the prior moves the iterate by 7e-4 only in 8 iterations, whatever the coupling
# and the threshold; the distance grows with mu_reg, so the prior weighs 5e5 times the data term here.
# The scale.  At mu = 1 that weight puts |grad| at 5e7 against moves of order 1, and the literal [-grad, move] system of the loop
# has a condition number past 1e15: numpy's pinv (cut at 1e-15 of the largest singular value) drops the memory direction, and the
# run -- "none" included -- is no longer 3MG nor invariant under a scaling of J (0.29 away from the same run on 1e-6 J or 1e-8 J,
# which agree to 1e-15).  The library does not reproduce that cut (plan_solvers.hip: "3MG").  So the criterion is scaled:
# mu = 1e-6, mu_reg = 0.5, the same minimiser and the same iterates in exact arithmetic, with the cut out of reach.
# The thresholds follow the group magnitudes: 0.1 for "isotropic", 0.1 sqrt(2 T) / sqrt(2) = 0.2 for "vector"; the hyperbolic
# weight falls under 0.9 from m = 0.48 delta on, so its threshold is doubled.  Scanned on the oracle:
#   isotropic, huber, 0.1: 59 % and 6.9e-2;  vector, huber, 0.2: 63 % and 9.3e-2;  vector, hyperbolic, 0.4: 30 % and 3.3e-2
NIT = po.NIT
MU, MU_REG = 1e-6, 0.5
DELTAS = {("isotropic", "huber"): 0.1, ("vector", "huber"): 0.2, ("vector", "hyperbolic"): 0.4}
# the robust case: the spiked config 1 of robust_oracle at data_delta = 2 (potentials_oracle.ROBUST), the prior's weight raised as
# above -- 3e5 times robust_oracle's 0.5 / sigma^2, under which the prior moves nothing -- and delta = 0.3: 55 % and 8.3e-2.  Its
# data term is weighted by 1 / sigma^2 = 4e-4 and its runs are invariant under a scaling of J (2e-15): mu stays 1.
ROBUST = dict(data_delta=po.ROBUST["data_delta"], delta=0.3, reg_scale=3e5)


def maps_run(coupling, potential="huber", delta=None):
    """the oracle run of a regime; ``coupling="none"`` with the ``delta`` of the regime it is compared with"""
    c = po.maps_case()
    d = DELTAS[(coupling, potential)] if delta is None else delta
    return po.cached(("coupled", coupling, potential, d),
                     lambda: mmmg(c["om"], c["y"], MU, MU_REG, d, c["x0"], coupling, potential, max_iter=NIT))


def robust_run(coupling):
    c = ro.config1_case()
    return po.cached(("coupled_robust", coupling),
                     lambda: mmmg_robust(c["om"], c["y"], 1.0, ROBUST["data_delta"], ROBUST["reg_scale"] * c["mur"], ROBUST["delta"],
                                         c["starts"]["huber"], w=c["w"], coupling=coupling, max_iter=NIT))
