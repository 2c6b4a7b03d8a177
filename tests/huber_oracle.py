"""Float64 restatement of the Huber-prior criterion and of 3MG on it, as qmm.mmmg runs it with qmm.Huber objectives
(the reference's lmm_reconstruction, surfh/ToolsDir/algorithms.py:73-106).  qmm is not installed here: like
``orc.mmmg`` this restatement is unpinned against qmm itself.

    J(x) = mu |y - A x|^2 / 2 + mu_reg sum_{k in r,c} sum phi(D_k x)
    phi(u) = u^2 / 2 (|u| <= delta), delta (|u| - delta / 2) beyond;  phi'(u) = u or delta sign(u);  w(u) = phi'(u) / u, w(0) = 1

D_r / D_c are ``orc.diff_r`` / ``orc.diff_c`` (fusion_CT.py:16-43).  ``mmmg`` keeps the structure of ``orc.mmmg`` (qmm's
literal [-grad, move] basis, operator images of the move carried) with the half-quadratic majorant
B = mu (A P)^T (A P) + mu_reg sum_k (D_k P)^T diag(w(D_k x)) (D_k P): with delta = inf every array it forms is bit for bit
the one ``orc.mmmg`` forms.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import surfh_oracle as orc  # noqa: E402

DIFFS = ((orc.diff_r, orc.diff_r_t), (orc.diff_c, orc.diff_c_t))


def phi(u, delta):
    a = np.abs(np.asarray(u, dtype=np.float64))
    if np.isinf(delta):
        return a * a / 2
    return np.where(a <= delta, a * a / 2, delta * (a - delta / 2))


def dphi(u, delta):
    u = np.asarray(u, dtype=np.float64)
    if np.isinf(delta):
        return u
    return np.where(np.abs(u) <= delta, u, delta * np.sign(u))


def weight(u, delta):
    a = np.abs(np.asarray(u, dtype=np.float64))
    return np.where(a <= delta, 1.0, delta / np.where(a > 0, a, 1.0))


def prior_value(x, delta):
    """sum_k sum phi(D_k x)"""
    return float(sum(np.sum(phi(d(x), delta)) for d, _ in DIFFS))


def prior_grad(x, delta):
    """sum_k D_k^T phi'(D_k x)"""
    return sum(dt(dphi(d(x), delta)) for d, dt in DIFFS)


def crit(op, data, x, mu, mu_reg, delta):
    x = np.asarray(x, dtype=np.float64).reshape(op.ishape)
    return float(mu * np.sum((data - op.forward(x)) ** 2) / 2 + mu_reg * prior_value(x, delta))


def gradient(op, b, x, mu, mu_reg, delta):
    """mu A^T (A x) - b + mu_reg sum_k D_k^T phi'(D_k x), b = mu A^T y (the operation order of orc.normal_apply)."""
    q = mu * op.adjoint(op.forward(x))
    if mu_reg:
        q = q + mu_reg * (orc.diff_r_t(dphi(orc.diff_r(x), delta)) + orc.diff_c_t(dphi(orc.diff_c(x), delta)))
    return q - b


def mmmg(op, data, mu, mu_reg, delta, x0, tol=1e-12, max_iter=10):
    """3MG on J (qmm.mmmg with one QuadObjective and two Huber objectives).  Returns x, grad_norm (|grad| of x0 and of every
    iterate), nit, crit (J of x0 and of every iterate)."""
    x = np.array(x0, dtype=np.float64, copy=True).reshape(op.ishape)
    b = mu * op.adjoint(data)
    ops = [(mu, op.forward), (mu_reg, orc.diff_r), (mu_reg, orc.diff_c)]
    move = np.zeros_like(x)
    vd = [np.stack([np.zeros_like(f(x)).ravel()] * 2, axis=1) for _, f in ops]
    step = np.ones((2, 1))
    grad_norm, crits = [], []
    nit = 0
    for it in range(max_iter + 1):
        grad = gradient(op, b, x, mu, mu_reg, delta)
        grad_norm.append(float(np.sqrt(np.sum(grad * grad))))
        crits.append(crit(op, data, x, mu, mu_reg, delta))
        if it == max_iter or grad_norm[-1] < x.size * tol:
            break
        D = np.stack([-grad.ravel(), move.ravel()], axis=1)
        vd = [np.stack([f(-grad).ravel(), (v @ step).ravel()], axis=1) for (_, f), v in zip(ops, vd)]
        ws = [np.ones(vd[0].shape[0]), weight(orc.diff_r(x), delta).ravel(), weight(orc.diff_c(x), delta).ravel()]
        B = sum(h * ((v * w[:, None]).T @ v) for (h, _), v, w in zip(ops, vd, ws))
        step = -np.linalg.pinv(B) @ (D.T @ grad.ravel()).reshape(2, 1)
        move = (D @ step).reshape(x.shape)
        x = x + move
        nit = it + 1
    return {"x": x, "grad_norm": grad_norm, "nit": nit, "crit": crits}


def small_problem():
    """48 x 48 maps, 4 templates over 32 wavelengths, one 2-slit channel at one pointing: the float64 operator costs a few ms,
    so that the restatement can run to convergence on a CPU."""
    import problems
    N, Lc = 48, 32
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(0.5 / 3600, 0.55 / 3600, (0.0, 0.0), 8.2, 0.196, 2, 3050.0, np.linspace(7.55, 7.65, 12), "S")
    psf = orc.gaussian_psf(wav, problems.STEP)[:, 13:27, 13:27]
    psf = psf / psf.sum(axis=(1, 2), keepdims=True)
    sotf = orc.ir2fr(psf, (N, N))
    pts = orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)[:1]
    om = orc.OracleModel(sotf, orc.synthetic_templates(Lc), ax, ax.copy(), wav, [spec], problems.STEP_DEG, [pts], box="direct")
    rng = np.random.default_rng(5)
    maps = np.zeros(om.ishape)
    maps[:, :, N // 2:] = 1.0                                     # a sharp front in every map
    maps += 0.05 * rng.standard_normal(om.ishape)
    y = om.forward(maps)
    y = y + rng.standard_normal(y.shape) * 1e-2 * np.sqrt(np.mean(y ** 2))
    return om, maps, y
