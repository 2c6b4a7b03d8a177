"""Float64 restatement of the non-negative solvers (surfh_amd/nonneg.py; include/surfh_amd.h: surfh_cg_nonneg), step for step: ADMM in
scaled form on ``min x^T Q x / 2 - b^T x, x >= 0`` with ``inner`` iterations of ``oracle.lcg``'s body on ``Q + rho I`` per outer
iteration.  Written on callables -- ``normal(v) = Q v`` and the vector ``b`` -- so that it runs on ``OracleModel``, on the template
operator of tests/tpl_oracle.py and on a dense matrix."""
import numpy as np

from oracle import surfh_oracle as orc

# the blobs of the device comparison: (ci, cj, s, a) on a 64 x 64 map, scaled with the map's size
BLOBS = [(20, 22, 5, 1.0), (40, 30, 4, 0.8), (30, 44, 6, 0.6), (44, 46, 3, 1.0)]
CASE = dict(mu=1.0, mu_reg=5e3, rho=6e4, outer=4, inner=4)


def case_start(shape):
    """The start of the device comparison.  Not zeros: from zero, 16 CG iterations leave the pixels no slit sees below 1e-4 max|x|
    (29 - 30 % of config 1's entries at every outer iteration), and the side of the projection a float32 run takes there is
    rounding.  With this start 0.05 % of the entries are that close to zero, and it has entries of both signs, so the r of trace
    row 0 carries rho (z - x0)."""
    return 0.05 * np.random.default_rng(6).standard_normal(shape)


def admm(normal, b, rho, x0=None, outer=30, inner=10, tol=0.0, refresh=10):
    """Returns ``z``, ``x``, ``trace`` [nit + 1, 4] = (|x - z|^2, rho^2 |z - z_prev|^2, r.r, #{z == 0}), ``nit``, and per outer
    iteration ``near`` = #{|x + u| <= 1e-4 max|x|} (the entries whose side of the projection a float32 run may take differently)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64).reshape(b.shape)
    z = np.maximum(x, 0.0)
    u = np.zeros_like(b)
    v = z - u
    r = b + rho * v - (normal(x) + rho * x)
    trace = [(float(np.sum((x - z) ** 2)), 0.0, float(np.sum(r * r)), float(np.sum(z == 0)))]
    near, nit = [], 0
    for k in range(outer):
        d = r.copy()
        rr = float(np.sum(r * r))
        for _ in range(inner):                                  # lcg's body on Q + rho I, no refresh inside
            q = normal(d) + rho * d
            dq = float(np.sum(d * q))
            step = rr / dq if dq != 0.0 else 0.0                  # a zero residual keeps still, as the device's step does
            x = x + step * d
            r = r - step * q
            rrn = float(np.sum(r * r))
            d = r + (rrn / rr if rr != 0.0 else 0.0) * d
            rr = rrn
        t = x + u
        near.append(int(np.sum(np.abs(t) <= 1e-4 * np.max(np.abs(x)))))
        zn = np.maximum(t, 0.0)
        un = u + x - zn
        vn = zn - un
        if refresh > 0 and (k + 1) % refresh == 0:
            r = b + rho * vn - (normal(x) + rho * x)
        else:
            r = r + rho * (vn - v)
        trace.append((float(np.sum((x - zn) ** 2)), rho * rho * float(np.sum((zn - z) ** 2)), float(np.sum(r * r)), float(np.sum(zn == 0))))
        z, u, v = zn, un, vn
        nit = k + 1
        if np.sqrt(max(rho * rho * trace[-1][0], trace[-1][1])) < b.size * tol:
            break
    return {"z": z, "x": x, "trace": np.array(trace), "nit": nit, "near": near}


def select(w, y):
    """W y with the samples of weight 0 taken out whatever they hold (NaN included); ``w`` None: y."""
    y = np.asarray(y, dtype=np.float64)
    return y if w is None else np.where(w > 0, w * np.where(w > 0, y, 0.0), 0.0)


class Weighted:
    """sqrt(W) A for an oracle operator A: ``oracle.lcg`` and ``normal_apply`` on it carry the data weights."""

    def __init__(self, op, weights):
        self.op = op
        self.sw = None if weights is None else np.sqrt(np.where(weights > 0, weights, 0.0)).reshape(-1)

    def forward(self, x):
        a = self.op.forward(x)
        return a if self.sw is None else (self.sw * a.reshape(-1)).reshape(a.shape)

    def adjoint(self, u):
        return self.op.adjoint(u if self.sw is None else (self.sw * np.asarray(u).reshape(-1)).reshape(np.shape(u)))

    def data(self, y):
        y = np.asarray(y, dtype=np.float64)
        return y if self.sw is None else (self.sw * np.where(self.sw > 0, y.reshape(-1), 0.0)).reshape(y.shape)


def maps_problem(om, y, mu, mu_reg, weights=None):
    """(normal, b, weighted operator, weighted data) of ``cg`` on the oracle model ``om``."""
    wop = Weighted(om, weights)
    yw = wop.data(y)
    return (lambda v: orc.normal_apply(wop, v, mu, mu_reg)), mu * wop.adjoint(yw), wop, yw


def blobs(na, nb=None):
    """The four blobs on an na x nb map (the recipe is stated on 64 x 64 and scaled per axis), zeroed below 0.05."""
    nb = na if nb is None else nb
    fa, fb = na / 64.0, nb / 64.0
    i, j = np.mgrid[0:na, 0:nb].astype(np.float64)
    out = []
    for ci, cj, s, a in BLOBS:
        m = a * np.exp(-(((i - ci * fa) / fa) ** 2 + ((j - cj * fb) / fb) ** 2) / (2 * s ** 2))
        out.append(np.where(m < 0.05, 0.0, m))
    return np.stack(out)


def blob_data(om, T, na, nb=None):
    """(truth [T, na, nb], y): the first T blobs through the oracle model, noise 1e-2 rms(y) from ``default_rng(5)``."""
    truth = blobs(na, nb)[:T]
    y = om.forward(truth)
    y = y + 1e-2 * np.sqrt(np.mean(y ** 2)) * np.random.default_rng(5).standard_normal(y.shape)
    return truth, y


def kkt(z, normal, b):
    """|min(z, Q z - b)|: zero exactly at the constrained minimiser."""
    return float(np.linalg.norm(np.minimum(z, normal(z) - b)))
