"""Float64 side of the non-negative plane-wise deconvolution (``MRSBlurred.cg_nonneg``, include/surfh_amd.h: surfh_cg_planes_nonneg):
``nonneg_oracle.admm`` applied plane by plane to the 2-D oracle of tests/huber_planes_oracle.py, and the problem the host test
(tests/test_nonneg_planes_host.py) and the device test (tests/test_gpu_nonneg_planes.py) share.

The geometry is ``huber_planes_oracle``'s: 5 planes of 96 x 96, 12 slits, 3 pointings.  The truth of plane l is ``AMPL[l]`` times the
four blobs of ``nonneg_oracle.blobs(96)`` on a zero background, the noise 1e-2 of every plane's own rms, plane EMPTY has no data and
starts at zero, the others start from ``0.05 AMPL[l] N(0, 1)`` (``nonneg_oracle.case_start``'s reason: entries of both signs, few of
them within rounding of the projection's corner).  The penalties are the Rayleigh quotients of one probe, the one
``Blurred2D.nonneg_rho(seed=0)`` draws, in float64.
"""
from __future__ import annotations

import numpy as np

import huber_planes_oracle as hp
import nonneg_oracle as no
from oracle import surfh_oracle as orc

L, N = hp.L, hp.N
AMPL = (1.0, 0.3, 1e-3, 1.0, 2.0)
QUIET, EMPTY = 2, 3                       # amplitude 1e-3; no data
COMPARED = (0, 1, 2, 4)
MU, MUR = 1.0, 1.5
OUTER, INNER = 4, 4

# Bounds of the device comparison: those of the map-domain non-negative solver (2e-4 on z, 4e-4 on r.r and on
# the two residual norms), scaled by how much less exactly this operator is evaluated than the one they were set on (the rule of
# huber_planes_oracle: E_PLANE / E_B, below 1 today).
SCALE = max(1.0, hp.E_PLANE / hp.E_B)
B_Z, B_R = 2e-4 * SCALE, 4e-4 * SCALE

_CACHE = {}


def problem():
    """truth [L, N, N], start x0 [L, N, N], data y [L, n_out]; plane EMPTY: y = 0, x0 = 0."""
    if "problem" not in _CACHE:
        ampl = np.asarray(AMPL)[:, None, None]
        truth = ampl * no.blobs(N).sum(axis=0)
        y = hp.batch_oracle().forward(truth)
        y = y + 1e-2 * np.sqrt(np.mean(y ** 2, axis=1, keepdims=True)) * np.random.default_rng(5).standard_normal(y.shape)
        x0 = 0.05 * ampl * np.random.default_rng(6).standard_normal(truth.shape)
        y[EMPTY] = 0.0
        x0[EMPTY] = 0.0
        _CACHE["problem"] = (truth, x0, y)
    return tuple(a.copy() for a in _CACHE["problem"])


def plane_problem(l, y_l, mask=None, mu=MU, mu_reg=MUR):
    """(normal, b, op) of plane l: Q_l v = mu A_l^T M A_l v + mu_reg (Dr^T Dr + Dc^T Dc) v on [1, N, N], b_l = mu A_l^T M y_l."""
    op = hp.plane_op(l, mask)
    data = y_l if mask is None else np.where(mask > 0, y_l, 0.0)
    return (lambda v: orc.normal_apply(op, v, mu, mu_reg)), mu * op.adjoint(data), op


def probe_rho(mask=None, seed=0, mu=MU, mu_reg=MUR, planes=range(L)):
    """{l: v_l^T Q_l v_l / v_l^T v_l} for the probe ``default_rng(seed).standard_normal((L, N, N))``."""
    v = np.random.default_rng(seed).standard_normal((L, N, N))
    out = {}
    for l in planes:
        op = hp.plane_op(l, mask)
        out[l] = float(np.sum(v[l] * orc.normal_apply(op, v[l][None], mu, mu_reg)[0]) / np.sum(v[l] ** 2))
    return out


def rho():
    """The penalties of the shared runs, [L]: the unmasked probe's quotients (every plane's, the empty one's too)."""
    if "rho" not in _CACHE:
        r = probe_rho()
        _CACHE["rho"] = np.array([r[l] for l in range(L)])
    return _CACHE["rho"].copy()


def solve_plane(l, y_l, x0_l, rho_l, mask=None, outer=OUTER, inner=INNER, refresh=0, tol=0.0):
    """``nonneg_oracle.admm`` on plane l alone; z and x come back as [N, N]."""
    normal, b, _ = plane_problem(l, y_l, mask)
    ref = no.admm(normal, b, rho_l, x0=np.asarray(x0_l)[None], outer=outer, inner=inner, tol=tol, refresh=refresh)
    ref["z"], ref["x"] = ref["z"][0], ref["x"][0]
    return ref


def reference(masked=False):
    """The per-plane runs of the shared problem after OUTER x INNER, refresh 0, computed once per process: {l: admm's result}."""
    key = ("ref", masked)
    if key not in _CACHE:
        _, x0, y = problem()
        mask = hp.sample_mask(y.shape[1]) if masked else None
        r = rho()
        _CACHE[key] = {l: solve_plane(l, y[l], x0[l], r[l], mask) for l in COMPARED}
    return _CACHE[key]


def rotated_case(angle=8.2, ampl=(1.0, 0.3)):
    """The same recipe on the rotated-field operator (tests/rotated_oracle.py: 96 x 96, 12 slits, the field of view at ``angle``
    degrees, three pointings of which two are fractional) with len(ampl) planes: the case, x0, y, rho [L] and {l: admm's result}."""
    key = ("rotated", angle, ampl)
    if key not in _CACHE:
        import rotated_oracle as ro
        Lr = len(ampl)
        case = ro.small_case(L=Lr, angle=angle)
        a = np.asarray(ampl)[:, None, None]
        truth = a * no.blobs(N).sum(axis=0)
        y = ro.oracle_of(case).forward(truth)
        y = y + 1e-2 * np.sqrt(np.mean(y ** 2, axis=1, keepdims=True)) * np.random.default_rng(5).standard_normal(y.shape)
        x0 = 0.05 * a * np.random.default_rng(6).standard_normal(truth.shape)
        v = np.random.default_rng(0).standard_normal(truth.shape)
        rho, ref = np.zeros(Lr), {}
        for l in range(Lr):
            op = ro.PlaneOp(ro.oracle_of(case, sotf=case["sotf"][l]))
            normal = lambda u, op=op: orc.normal_apply(op, u, MU, MUR)  # noqa: E731
            rho[l] = float(np.sum(v[l] * normal(v[l][None])[0]) / np.sum(v[l] ** 2))
            ref[l] = no.admm(normal, MU * op.adjoint(y[l]), rho[l], x0=x0[l][None], outer=OUTER, inner=INNER, refresh=0)
            ref[l]["z"], ref[l]["x"] = ref[l]["z"][0], ref[l]["x"][0]
        _CACHE[key] = dict(case=case, x0=x0, y=y, rho=rho, ref=ref)
    return _CACHE[key]


def compare_plane(z, primal, dual, grad_norm, n_active, rho_l, ref, label):
    """One plane of a device run against its restatement: z relative to max|z| under B_Z; |x - z| and |z - z_prev| relative to |x|
    (as tests/test_gpu_nonneg.py measures them) and r.r relatively under B_R; n_active off by at most the restatement's count of
    entries within 1e-4 max|x| of zero.  Returns the four errors and the worst count difference."""
    tr = ref["trace"]
    xn = float(np.linalg.norm(ref["x"]))
    e_z = float(np.max(np.abs(z - ref["z"])) / np.max(np.abs(ref["z"])))
    e_p = float(np.max(np.abs(primal - np.sqrt(tr[:, 0])))) / xn
    e_d = float(np.max(np.abs(dual - np.sqrt(tr[:, 1])))) / rho_l / xn
    e_r = float(np.max(np.abs(grad_norm ** 2 - tr[:, 2]) / tr[:, 2]))
    d_a = np.abs(n_active - tr[:, 3])
    print(f"{label}: z {e_z:.2e} (bound {B_Z:.1e}); |x - z| {e_p:.2e}, |z - z_prev| {e_d:.2e}, r.r {e_r:.2e} (bound {B_R:.1e}); n_active off by "
          f"{d_a.astype(int).tolist()} (near zero {ref['near']})")
    assert len(primal) == len(tr)
    assert z.min() >= 0.0 and not np.any(np.signbit(z))
    assert e_z < B_Z, (label, e_z)
    assert e_p < B_R and e_d < B_R and e_r < B_R, (label, e_p, e_d, e_r)
    assert d_a[0] == 0 and np.all(d_a[1:] <= np.asarray(ref["near"])), (label, d_a, ref["near"])
    return e_z, e_p, e_d, e_r, int(d_a.max())
