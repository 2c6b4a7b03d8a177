"""Float64 restatement of the robust (Huber) data term and of 3MG on it, as qmm.mmmg runs it when the data objective is
``qmm.Objective(forward, adjoint, qmm.Huber(delta_d), data=y)`` instead of a QuadObjective.  qmm is not installed here: like
``huber_oracle.mmmg`` this restatement is unpinned against qmm itself.

    J(x) = mu sum_i phi_dd(t_i) + priors(x),   t = sqrt(w) (y - A x) = y~ - A~ x

with A~ = W^(1/2) A and y~ = W^(1/2) y of ``weights_oracle`` (a sample of weight 0 is taken out by a select: t = 0 there whatever
y holds) and phi / phi' / omega = phi'(t) / t of ``huber_oracle``.  ``mmmg`` is ``huber_oracle.mmmg`` on (A~, y~) with two changes:
the data family of the majorant carries the weights omega(t) -- in terms of A, w omega(t) -- instead of ones, and the data
gradient is -mu A~^T phi'(t) = -mu A^T (sqrt(w) phi'(t)).  With delta_d = inf, phi'(t) = t and the gradient is linear in x; that
case is written in ``huber_oracle.gradient``'s operation order, mu A~^T (A~ x) - mu A~^T y~, so that every array formed is bit
for bit the one ``huber_oracle.mmmg`` forms on (A~, y~) -- on (A, y) itself without weights.  ``mmmg_vox`` is the same on
``vox_oracle.mmmg``.
"""
from __future__ import annotations

import numpy as np

import huber_oracle as ho
import vox_oracle as vo
import weights_oracle as wo
from huber_oracle import dphi, phi, weight  # noqa: F401
from oracle import surfh_oracle as orc


def whiten(op, data, w):
    """(A~, y~): the operator and the data of the scaled residual; (op, data) themselves without weights."""
    if w is None:
        return op, np.asarray(data, dtype=np.float64).reshape(op.oshape)
    return wo.Weighted(op, w), wo.wdata(np.asarray(w, dtype=np.float64).reshape(op.oshape), data)


def residual(op, data, x, w=None):
    """t = sqrt(w) (y - A x), in the shape of the data"""
    aw, yw = whiten(op, data, w)
    return yw - aw.forward(np.asarray(x, dtype=np.float64).reshape(op.ishape))


def omega(op, data, x, data_delta, w=None):
    """phi'(t) / t in (0, 1], raveled; 0 where w = 0"""
    om = weight(residual(op, data, x, w), data_delta).ravel()
    return om if w is None else np.where(np.asarray(w).ravel() > 0, om, 0.0)


def data_value(op, data, x, data_delta, w=None):
    """sum_i phi(t_i)"""
    return float(np.sum(phi(residual(op, data, x, w), data_delta)))


def n_beyond(op, data, x, data_delta, w=None):
    return int(np.sum(np.abs(residual(op, data, x, w)) > data_delta))


def crit(op, data, x, mu, data_delta, mu_reg, delta, w=None):
    x = np.asarray(x, dtype=np.float64).reshape(op.ishape)
    return float(mu * data_value(op, data, x, data_delta, w) + mu_reg * ho.prior_value(x, delta))


def gradient(op, data, x, mu, data_delta, mu_reg, delta, w=None):
    """-mu A^T (sqrt(w) phi'(t)) + mu_reg sum_k D_k^T phi'(D_k x)"""
    aw, yw = whiten(op, data, w)
    if np.isinf(data_delta):
        return ho.gradient(aw, mu * aw.adjoint(yw), x, mu, mu_reg, delta)
    g = -mu * aw.adjoint(dphi(yw - aw.forward(x), data_delta))
    if mu_reg:
        g = g + mu_reg * (orc.diff_r_t(dphi(orc.diff_r(x), delta)) + orc.diff_c_t(dphi(orc.diff_c(x), delta)))
    return g


def majorant_quad(op, data, x, v, mu, data_delta, mu_reg, delta, w=None):
    """v^T B(x) v, B(x) = mu A^T diag(w omega(t)) A + mu_reg sum_k D_k^T diag(w(D_k x)) D_k"""
    aw, yw = whiten(op, data, w)
    q = mu * np.sum(weight(yw - aw.forward(x), data_delta) * aw.forward(v) ** 2)
    for d in (orc.diff_r, orc.diff_c):
        q += mu_reg * np.sum(weight(d(x), delta) * d(v) ** 2)
    return float(q)


def _run(aw, yw, ops, grad_of, crit_of, data_delta, x0, tol, max_iter):
    """qmm's literal [-grad, move] loop of ``huber_oracle.mmmg``; ops = [(weight, operator, threshold)], ops[0] the data family,
    whose majorant weights are omega(t)."""
    x = np.array(x0, dtype=np.float64, copy=True).reshape(aw.ishape)
    move = np.zeros_like(x)
    vd = [np.stack([np.zeros_like(f(x)).ravel()] * 2, axis=1) for _, f, _ in ops]
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
        vd = [np.stack([f(-grad).ravel(), (v @ step).ravel()], axis=1) for (_, f, _), v in zip(ops, vd)]
        ws = [weight(yw - aw.forward(x), data_delta).ravel()] + [weight(f(x), dl).ravel() for _, f, dl in ops[1:]]
        B = sum(h * ((v * wk[:, None]).T @ v) for (h, _, _), v, wk in zip(ops, vd, ws))
        step = -np.linalg.pinv(B) @ (D.T @ grad.ravel()).reshape(2, 1)
        move = (D @ step).reshape(x.shape)
        x = x + move
        nit = it + 1
    return {"x": x, "grad_norm": grad_norm, "nit": nit, "crit": crits}


def mmmg(op, data, mu, data_delta, mu_reg, delta, x0, w=None, tol=1e-12, max_iter=10):
    """3MG on J (qmm.mmmg with one Huber data objective and two Huber prior objectives; delta = inf: quadratic priors).  Returns
    x, grad_norm (|grad| of x0 and of every iterate), nit, crit (J of x0 and of every iterate)."""
    aw, yw = whiten(op, data, w)
    ops = [(mu, aw.forward, None), (mu_reg, orc.diff_r, delta), (mu_reg, orc.diff_c, delta)]
    return _run(aw, yw, ops, lambda x: gradient(op, data, x, mu, data_delta, mu_reg, delta, w),
                lambda x: crit(op, data, x, mu, data_delta, mu_reg, delta, w), data_delta, x0, tol, max_iter)


# ---- the cube itself: the prior families of vox_oracle ---------------------------------------------------------------------------
def crit_vox(op, data, x, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta, w=None):
    x = np.asarray(x, dtype=np.float64).reshape(op.ishape)
    vs, vl = vo.prior_values(x, spat_delta, spec_delta)
    return float(mu * data_value(op, data, x, data_delta, w) + spat_reg * vs + spec_reg * vl)


def gradient_vox(op, data, x, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta, w=None):
    aw, yw = whiten(op, data, w)
    if np.isinf(data_delta):
        return vo.gradient(aw, mu * aw.adjoint(yw), x, mu, spat_reg, spat_delta, spec_reg, spec_delta)
    return -mu * aw.adjoint(dphi(yw - aw.forward(x), data_delta)) + vo.prior_grad(x, spat_reg, spat_delta, spec_reg, spec_delta)


def mmmg_vox(op, data, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta, x0, w=None, tol=1e-12, max_iter=10):
    """3MG on the voxel-wise criterion with the robust data term (``vox_oracle.mmmg`` with the two changes above)."""
    aw, yw = whiten(op, data, w)
    ops = [(mu, aw.forward, None), (spat_reg, orc.diff_r, spat_delta), (spat_reg, orc.diff_c, spat_delta)]
    if spec_reg:
        ops.append((spec_reg, vo.diff_l, spec_delta))
    return _run(aw, yw, ops, lambda x: gradient_vox(op, data, x, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta, w),
                lambda x: crit_vox(op, data, x, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta, w), data_delta, x0, tol,
                max_iter)


# ---- the problems of tests/test_gpu_robust.py, checked on the oracle alone by tests/test_robust_host.py --------------------------
DATA_DELTA = 3.0
# device against oracle: the map-domain bounds of test_gpu_huber.py (1e-4 in x, 2e-4 in grad_norm) x 2 -- the margin the voxel-wise
# and the plane-wise solvers took, here because the operator runs as separate forward and adjoint instead of the hand-over
X_TOL_BOUND, G_TOL_BOUND = 2e-4, 4e-4


def spiked(y0, seed_noise=1, seed_spikes=2):
    """y = y0 + sigma randn (sigma = 1e-2 rms(y0), seed 1) with spikes of +-30 sigma on osize // 50 samples (seed 2).
    Returns dict(sigma, y_clean, y, spikes (indices), w = 1 / sigma^2)."""
    y0 = np.asarray(y0, dtype=np.float64).ravel()
    sigma = 1e-2 * np.sqrt(np.mean(y0 ** 2))
    y_clean = y0 + sigma * np.random.default_rng(seed_noise).standard_normal(y0.size)
    rng = np.random.default_rng(seed_spikes)
    idx = rng.choice(y0.size, y0.size // 50, replace=False)
    y = y_clean.copy()
    y[idx] += 30 * sigma * rng.choice([-1.0, 1.0], idx.size)
    return dict(sigma=sigma, y_clean=y_clean, y=y, spikes=idx, w=np.full(y0.size, 1.0 / sigma ** 2))


_CACHE = {}


def config1_case():
    """The standard spiked problem on ``problems.config1()``: w = 1 / sigma^2, data_delta = 3, mu_reg = 0.5 / sigma^2."""
    if "c1" not in _CACHE:
        import problems
        cfg = problems.config1()
        om = problems.oracle_model(cfg, box="direct")
        d = spiked(om.forward(cfg["maps"]))
        starts = {"quadratic": np.full(om.ishape, 0.5),
                  "huber": cfg["maps"] + 0.1 * np.random.default_rng(3).standard_normal(om.ishape)}       # test_gpu_huber.py's "rough"
        _CACHE["c1"] = dict(cfg=cfg, om=om, mur=0.5 / d["sigma"] ** 2, starts=starts, **d)
    return _CACHE["c1"]


# regime: (prior delta, iterations); the start is config1_case()["starts"][regime]
C1_REGIMES = {"quadratic": (float("inf"), 8), "huber": (0.1, 8)}


def config1_runs(regime):
    """Oracle runs of one regime, computed once: the robust solve of the spiked data, and the weighted quadratic solves
    (data_delta = inf) of the spiked and of the clean data."""
    key = ("c1", regime)
    if key not in _CACHE:
        c = config1_case()
        delta, nit = C1_REGIMES[regime]
        x0, inf = c["starts"][regime], float("inf")
        _CACHE[key] = dict(
            rob=mmmg(c["om"], c["y"], 1.0, DATA_DELTA, c["mur"], delta, x0, w=c["w"], max_iter=nit),
            quad=mmmg(c["om"], c["y"], 1.0, inf, c["mur"], delta, x0, w=c["w"], max_iter=nit),
            clean=mmmg(c["om"], c["y_clean"], 1.0, inf, c["mur"], delta, x0, w=c["w"], max_iter=nit))
    return _CACHE[key]


# (spat_reg, spat_delta, spec_reg, spec_delta, iterations), the weights in units of 1 / sigma^2 like the data term: three times
# vox_oracle.REGIMES["spatial"].  The cube has 64 unknowns per datum, so weak priors let the quadratic solve absorb a spike locally
# and the robust solve gains little over it; at these weights (scanned on the oracle alone, tests/test_robust_host.py asserts the
# outcome) the robust iterate is 5.5 times closer to the clean solve than the quadratic one, with 46 % / 68 % of the spatial /
# spectral differences beyond their thresholds.
VOX_REGIME = (300.0, 0.005, 30.0, 0.01, 8)


def vox_case():
    """``vox_oracle.small_cfg()`` (32 x 48 x 48, no templates) with the spikes of ``spiked`` on its noiseless data, from vox_oracle's
    "rough" start."""
    if "vox" not in _CACHE:
        cfg, om, cube, _ = vo.small_cfg()
        d = spiked(om.forward(cube))
        _CACHE["vox"] = dict(cfg=cfg, om=om, cube=cube, x0=vo.start("rough", om, cube), scale=1.0 / d["sigma"] ** 2, **d)
    return _CACHE["vox"]


def vox_runs():
    if "vox_runs" not in _CACHE:
        c = vox_case()
        sr, sd, lr, ld, nit = VOX_REGIME
        sr, lr, inf = sr * c["scale"], lr * c["scale"], float("inf")
        args = (sr, sd, lr, ld, c["x0"])
        _CACHE["vox_runs"] = dict(
            rob=mmmg_vox(c["om"], c["y"], 1.0, DATA_DELTA, *args, w=c["w"], max_iter=nit),
            quad=mmmg_vox(c["om"], c["y"], 1.0, inf, *args, w=c["w"], max_iter=nit),
            clean=mmmg_vox(c["om"], c["y_clean"], 1.0, inf, *args, w=c["w"], max_iter=nit))
    return _CACHE["vox_runs"]


def preconditions(op, c, runs):
    """(share of |t| > data_delta at the robust iterate, robust vs quadratic on the spiked data, robust vs the clean quadratic
    solve, quadratic on the spiked data vs the clean quadratic solve)"""
    def rel(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))
    t = residual(op, c["y"], runs["rob"]["x"], c["w"])
    return (float(np.mean(np.abs(t) > DATA_DELTA)), rel(runs["rob"]["x"], runs["quad"]["x"]),
            rel(runs["rob"]["x"], runs["clean"]["x"]), rel(runs["quad"]["x"], runs["clean"]["x"]))
