"""Float64 restatement of the voxel-wise Huber criterion and of 3MG on it, as qmm.mmmg runs it with three qmm.Huber objectives
(the reference's vox_reconstruction, surfh/ToolsDir/algorithms.py:27-71).  qmm and aljabr are not installed here: like
``huber_oracle.mmmg`` this restatement is unpinned against qmm itself, and the border conventions against aljabr.Diff.

    J(x) = mu |y - A x|^2 / 2 + spat_reg sum_{k in r,c} sum phi_ds(D_k x) + spec_reg sum phi_dl(D_l x)

x is the cube [Lc][Na][Nb] (the reference's legacy Spectro model is (alpha, beta, lambda), hence its Diff(0) / Diff(1) / Diff(2)).
phi / phi' / w are those of ``huber_oracle``; D_r / D_c are ``orc.diff_r`` / ``orc.diff_c`` applied to the planes; D_l is the open
difference ``diff_l`` along wavelength (Lc - 1 planes).  ``mmmg`` keeps the structure of ``huber_oracle.mmmg`` with three prior
operators instead of two; a spectral family of weight 0 is skipped, not added as zeros, so that with ``spec_reg = 0`` every array
it forms is bit for bit the one ``huber_oracle.mmmg`` forms, and with every threshold infinite as well the one ``orc.mmmg`` forms.
"""
from __future__ import annotations

import numpy as np

import huber_oracle as ho
from huber_oracle import dphi, phi, weight  # noqa: F401
from oracle import surfh_oracle as orc


def diff_l(x):
    """(D_l x)[l] = x[l+1] - x[l], l = 0 .. Lc-2: no wrap between the two ends of the wavelength axis."""
    return x[1:] - x[:-1]


def diff_l_t(v):
    """(D_l^T v)[l] = v[l-1] - v[l] with v[-1] = v[Lc-1] = 0."""
    out = np.zeros((v.shape[0] + 1,) + v.shape[1:], dtype=v.dtype)
    out[1:] += v
    out[:-1] -= v
    return out


def prior_values(x, spat_delta, spec_delta):
    """(sum_{k in r,c} sum phi(D_k x), sum phi(D_l x))"""
    return ho.prior_value(x, spat_delta), float(np.sum(phi(diff_l(x), spec_delta)))


def prior_grad(x, spat_reg, spat_delta, spec_reg, spec_delta):
    """spat_reg sum_k D_k^T phi'(D_k x) + spec_reg D_l^T phi'(D_l x)"""
    return spat_reg * ho.prior_grad(x, spat_delta) + spec_reg * diff_l_t(dphi(diff_l(x), spec_delta))


def crit(op, data, x, mu, spat_reg, spat_delta, spec_reg, spec_delta):
    x = np.asarray(x, dtype=np.float64).reshape(op.ishape)
    j = float(mu * np.sum((data - op.forward(x)) ** 2) / 2 + spat_reg * ho.prior_value(x, spat_delta))
    if spec_reg:
        j = float(j + spec_reg * np.sum(phi(diff_l(x), spec_delta)))
    return j


def gradient(op, b, x, mu, spat_reg, spat_delta, spec_reg, spec_delta):
    """mu A^T (A x) - b + the prior gradient, b = mu A^T y (operation order of huber_oracle.gradient)."""
    q = mu * op.adjoint(op.forward(x))
    if spat_reg:
        q = q + spat_reg * (orc.diff_r_t(dphi(orc.diff_r(x), spat_delta)) + orc.diff_c_t(dphi(orc.diff_c(x), spat_delta)))
    if spec_reg:
        q = q + spec_reg * diff_l_t(dphi(diff_l(x), spec_delta))
    return q - b


def majorant_quad(op, x, v, mu, spat_reg, spat_delta, spec_reg, spec_delta):
    """v^T B(x) v, B(x) = mu A^T A + spat_reg sum_k D_k^T diag(w(D_k x)) D_k + spec_reg D_l^T diag(w(D_l x)) D_l"""
    q = mu * np.sum(op.forward(v) ** 2)
    for d in (orc.diff_r, orc.diff_c):
        q += spat_reg * np.sum(weight(d(x), spat_delta) * d(v) ** 2)
    return float(q + spec_reg * np.sum(weight(diff_l(x), spec_delta) * diff_l(v) ** 2))


def mmmg(op, data, mu, spat_reg, spat_delta, spec_reg, spec_delta, x0, tol=1e-12, max_iter=10):
    """3MG on J (qmm.mmmg with one QuadObjective and three Huber objectives).  Returns x, grad_norm (|grad| of x0 and of every
    iterate), nit, crit (J of x0 and of every iterate)."""
    x = np.array(x0, dtype=np.float64, copy=True).reshape(op.ishape)
    b = mu * op.adjoint(data)
    ops = [(mu, op.forward, None), (spat_reg, orc.diff_r, spat_delta), (spat_reg, orc.diff_c, spat_delta)]
    if spec_reg:
        ops.append((spec_reg, diff_l, spec_delta))
    move = np.zeros_like(x)
    vd = [np.stack([np.zeros_like(f(x)).ravel()] * 2, axis=1) for _, f, _ in ops]
    step = np.ones((2, 1))
    grad_norm, crits = [], []
    nit = 0
    for it in range(max_iter + 1):
        grad = gradient(op, b, x, mu, spat_reg, spat_delta, spec_reg, spec_delta)
        grad_norm.append(float(np.sqrt(np.sum(grad * grad))))
        crits.append(crit(op, data, x, mu, spat_reg, spat_delta, spec_reg, spec_delta))
        if it == max_iter or grad_norm[-1] < x.size * tol:
            break
        D = np.stack([-grad.ravel(), move.ravel()], axis=1)
        vd = [np.stack([f(-grad).ravel(), (v @ step).ravel()], axis=1) for (_, f, _), v in zip(ops, vd)]
        if all(np.isinf(dl) for _, _, dl in ops[1:]):      # every weight is 1: the majorant is J, in orc.mmmg's expression
            B = sum(h * (v.T @ v) for (h, _, _), v in zip(ops, vd))       # (v.T @ v and (v * 1).T @ v round differently in BLAS)
        else:
            ws = [np.ones(vd[0].shape[0])] + [weight(f(x), dl).ravel() for _, f, dl in ops[1:]]
            B = sum(h * ((v * w[:, None]).T @ v) for (h, _, _), v, w in zip(ops, vd, ws))
        step = -np.linalg.pinv(B) @ (D.T @ grad.ravel()).reshape(2, 1)
        move = (D @ step).reshape(x.shape)
        x = x + move
        nit = it + 1
    return {"x": x, "grad_norm": grad_norm, "nit": nit, "crit": crits}


def shares(x, spat_delta, spec_delta):
    """share of |D_k x| > spat_delta (rows and columns together) and of |D_l x| > spec_delta"""
    us = np.abs(np.concatenate([orc.diff_r(x).ravel(), orc.diff_c(x).ravel()]))
    ul = np.abs(diff_l(x))
    return float(np.mean(us > spat_delta)), float(np.mean(ul > spec_delta)) if ul.size else 0.0


def small_problem():
    """A 32 x 48 x 48 cube without templates, one 2-slit channel at one pointing (the geometry of huber_oracle.small_problem):
    the float64 operator costs a few ms.  The truth has a sharp spatial front in every plane, an emission line and a step along
    wavelength, and noise: both families of differences have values on both sides of a threshold."""
    import problems
    N, Lc = 48, 32
    ax = orc.synthetic_axes(N, problems.STEP_DEG)
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(0.5 / 3600, 0.55 / 3600, (0.0, 0.0), 8.2, 0.196, 2, 3050.0, np.linspace(7.55, 7.65, 12), "S")
    psf = orc.gaussian_psf(wav, problems.STEP)[:, 13:27, 13:27]
    psf = psf / psf.sum(axis=(1, 2), keepdims=True)
    sotf = orc.ir2fr(psf, (N, N))
    pts = orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)[:1]
    om = orc.OracleModel(sotf, None, ax, ax.copy(), wav, [spec], problems.STEP_DEG, [pts], box="direct")
    rng = np.random.default_rng(5)
    spectrum = 0.5 + 0.5 * (np.arange(Lc) >= 20) + 1.5 * np.exp(-0.5 * ((np.arange(Lc) - 10) / 1.2) ** 2)   # step + line
    cube = np.zeros(om.ishape)
    cube[:, :, N // 2:] = 1.0                                     # a sharp front in every plane
    cube = (0.3 + cube) * spectrum[:, None, None]
    cube += 0.05 * rng.standard_normal(om.ishape)
    y = om.forward(cube)
    y = y + rng.standard_normal(y.shape) * 1e-2 * np.sqrt(np.mean(y ** 2))
    return om, cube, y


def small_cfg():
    """``small_problem`` as a tests/problems.py config, for ``helpers.build_model``."""
    import problems
    om, cube, y = small_problem()
    spec = orc.ChannelSpec(0.5 / 3600, 0.55 / 3600, (0.0, 0.0), 8.2, 0.196, 2, 3050.0, np.linspace(7.55, 7.65, 12), "S")
    pts = orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)[:1]
    cfg = dict(N=48, Lc=32, alpha_axis=om.alpha_axis, beta_axis=om.beta_axis, wavel=om.wavelength_axis, specs=[spec], templates=None,
               sotf=om.sotf, pointings=[pts], maps=cube, step_deg=problems.STEP_DEG)
    return cfg, om, cube, y


# The regimes of tests/test_gpu_vox.py, chosen on the oracle alone (tests/test_vox_host.py checks their preconditions):
# name: (spat_reg, spat_delta, spec_reg, spec_delta, start, iterations).  Starts: "rough" = truth + 0.1 noise (seed 3).
# Picked so that, at the oracle's final iterate, between 10 % and 90 % of each family's differences lie beyond its threshold and
# the iterate is far from the quadratic solver's: weights around 1e4 (as on the maps) let the priors dwarf this problem's
# data term (one channel sees 12 of the 32 planes through two slits) and smooth every difference below delta ~ 0.1 in a few
# iterations; weights of 10 .. 100 with thresholds of 0.005 .. 0.01 keep both branches of phi in play.
#   spatial : the in-plane families carry most of the prior (1.7e3 against 0.7e3 at the final iterate)
#   spectral: the wavelength family does (5.6e3 against 0.7e3)
#   both    : comparable (0.6e3 and 1.2e3)
REGIMES = {"spatial": (100.0, 0.005, 10.0, 0.01, "rough", 8), "spectral": (10.0, 0.01, 100.0, 0.01, "rough", 8),
           "both": (40.0, 0.005, 20.0, 0.01, "rough", 8)}
# Bounds of the device-against-oracle comparison (tests/test_gpu_vox.py derives them): x, grad_norm
X_TOL_BOUND, G_TOL_BOUND = 2e-4, 4e-4


def start(name, om, cube):
    if name == "rough":
        return cube + 0.1 * np.random.default_rng(3).standard_normal(om.ishape)
    raise KeyError(name)
