"""Float64 restatement of the posterior sampler (include/surfh_amd.h: surfh_cg_sample): the counter-based normal generator,
the perturbed right-hand side and a CG with an extra right-hand side.

Convention: p(x | y) ~ exp(-x^T Q x / 2 + b^T x), Q = mu A^T W A + mu_reg (Dr^T Dr + Dc^T Dc), b = mu A^T W y.  A draw is

    y~ = y + eps_y / sqrt(mu w)  (w > 0; untouched where w = 0),   eta = sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c),
    b~ = mu A^T W y~ + eta  ~  N(b, Q),                              x~ = Q^-1 b~,
and the sampler solves for the deviation from the point estimate: Q e = b~ - b from e = 0, x~ = xhat + e.
"""
from __future__ import annotations

import numpy as np

import problems  # noqa: F401  (puts the repository root on sys.path)
from oracle import surfh_oracle as orc
from weights_oracle import Weighted, wdata

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM_Y, STREAM_R, STREAM_C = 0, 1, 2
ZMAX = 5.89                               # sqrt(-2 ln(2^-25)) = 5.887


def philox4x32_10(ctr, key):
    """Philox4x32-10 on counters ``ctr`` [..., 4] under ``key`` (k0, k1): uint32 words in, uint32 words [..., 4] out."""
    c = [np.asarray(ctr)[..., j].astype(np.uint64) & MASK for j in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def randn(n, seed=0, stream=0, sample=0, start=0):
    """Elements ``start .. start + n`` of the normal stream (seed, stream, sample), float64: key (seed low, seed high), counter
    (i / 4 low, i / 4 high, stream, sample); words (a0, a1) give elements 4c, 4c+1, words (a2, a3) give 4c+2, 4c+3 as
    sqrt(-2 ln u) (cos, sin)(theta), u = ((a0 >> 8) + 1/2) 2^-24, theta = 2 pi ((a1 >> 8) + 1/2) 2^-24."""
    seed = int(seed) & (2 ** 64 - 1)
    c0, c1 = start // 4, (start + n + 3) // 4
    idx = np.arange(c0, c1, dtype=np.uint64)
    ctr = np.stack([idx & MASK, idx >> np.uint64(32), np.full(idx.shape, stream, np.uint64), np.full(idx.shape, sample, np.uint64)], axis=-1)
    a = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.float64)
    a = np.floor(a / 256.0)                                             # word >> 8
    z = np.empty((len(idx), 4))
    for k in (0, 2):
        rad = np.sqrt(-2.0 * np.log((a[:, k] + 0.5) * 2.0 ** -24))
        th = 2.0 * np.pi * (a[:, k + 1] + 0.5) * 2.0 ** -24
        z[:, k], z[:, k + 1] = rad * np.cos(th), rad * np.sin(th)
    return z.reshape(-1)[start - 4 * c0: start - 4 * c0 + n]


def draw(om, seed, sample):
    """(eps_y [osize], eps_r, eps_c [ishape]) of draw ``sample``: the generator's streams 0, 1, 2."""
    return (randn(om.osize, seed, STREAM_Y, sample), randn(om.isize, seed, STREAM_R, sample).reshape(om.ishape),
            randn(om.isize, seed, STREAM_C, sample).reshape(om.ishape))


def perturb_data(y, w, eps_y, mu):
    """y~ = y + eps_y / sqrt(mu w) where w > 0 (w None: 1), y itself elsewhere (NaN included)."""
    y = np.asarray(y, dtype=np.float64)
    if w is None:
        return y + eps_y / np.sqrt(mu)
    keep = np.asarray(w) > 0
    return np.where(keep, y + eps_y / np.sqrt(mu * np.where(keep, w, 1.0)), y)


def eta(eps_r, eps_c, mu_reg):
    """sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c)."""
    return np.sqrt(mu_reg) * (orc.diff_r_t(eps_r) + orc.diff_c_t(eps_c))


def rhs(om, y, w, mu, mu_reg, eps):
    """b~ = mu A^T W y~ + eta for the draw ``eps`` = (eps_y, eps_r, eps_c)."""
    yt = perturb_data(y, w, eps[0], mu)
    wy = yt if w is None else np.where(np.asarray(w) > 0, w * np.where(np.asarray(w) > 0, yt, 0.0), 0.0)
    return mu * om.adjoint(wy) + eta(eps[1], eps[2], mu_reg)


def lcg(op, data, mu, mu_reg, x0, extra=None, tol=1e-12, max_iter=10, refresh=50):
    """``orc.lcg`` with b = mu A^T data + extra: the same statements in the same order, so extra None (or zeros) gives its bits."""
    x = np.array(x0, dtype=np.float64, copy=True)
    b = mu * op.adjoint(data)
    if extra is not None:
        b = b + extra
    r = b - orc.normal_apply(op, x, mu, mu_reg)
    d = r.copy()
    grad_norm = [float(np.sum(r * r))]
    nit = 0
    for it in range(max_iter):
        q = orc.normal_apply(op, d, mu, mu_reg)
        step = grad_norm[-1] / float(np.sum(d * q))
        x += step * d
        if refresh and it % refresh == 0:
            r = b - orc.normal_apply(op, x, mu, mu_reg)
        else:
            r -= step * q
        grad_norm.append(float(np.sum(r * r)))
        d = r + (grad_norm[-1] / grad_norm[-2]) * d
        nit = it + 1
        if np.sqrt(grad_norm[-1]) < x.size * tol:
            break
    return {"x": x, "grad_norm": grad_norm, "nit": nit}


def sample(om, w, mu, mu_reg, eps, xhat, max_iter, tol=1e-12, refresh=50):
    """One posterior sample about ``xhat`` as the library draws it: the CG above for the deviation, Q e = b~ - b from e = 0 -- the
    perturbation eps_y / sqrt(mu w) as its data, eta as the extra right-hand side -- under the weights ``w`` (None: 1).  Returns
    the CG's dict with "e" and "x" = xhat + e."""
    dy = perturb_data(np.zeros(om.osize), w, eps[0], mu)
    e = eta(eps[1], eps[2], mu_reg) if mu_reg else None
    zero = np.zeros(om.ishape)
    if w is None:
        out = lcg(om, dy, mu, mu_reg, zero, e, tol, max_iter, refresh)
    else:
        out = lcg(Weighted(om, w), wdata(w, dy), mu, mu_reg, zero, e, tol, max_iter, refresh)
    out["e"], out["x"] = out["x"], np.asarray(xhat, dtype=np.float64) + out["x"]
    return out


# ---- the covariance identity: v^T b~ has mean v^T b and variance v^T Q v ----------------------------------------------------
IDENTITY = dict(mu=4.0, mu_reg=9.0, draws=400, seed=0)


def identity_weights(osize, seed=5):
    """Uniform in [0.5, 2] with 5 % zeros."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, osize)
    w[rng.random(osize) < 0.05] = 0.0
    return w


def identity_data(om, maps, w, mu, seed=1, rms=10.0):
    """Data at the statistical scale the weights state: the signal A maps scaled to ``rms``, plus noise of standard deviation
    1 / sqrt(mu w); NaN where w = 0.  The scale matters on the device: b~ = b + noise is formed in fp32, where b carries a
    rounding error of some 3e-7 |b|, and in a direction the data do not see (the checkerboard) that error must stay small against
    the prior's noise -- with the signal 5e3 times the noise it does not ("Posterior sampling")."""
    y = om.forward(maps)
    y = y * (rms / np.sqrt(np.mean(y ** 2)))
    keep = w > 0
    y = y + np.random.default_rng(seed).standard_normal(y.size) / np.sqrt(mu * np.where(keep, w, 1.0))
    return np.where(keep, y, np.nan)


def probes(ishape, seed=6):
    """all-ones (pure data term: D 1 = 0), checkerboard (-1)^(i+j) (pure prior on even sizes where A^T W A sees no such
    frequency), Gaussian random, one map of ones."""
    T, na, nb = ishape
    i, j = np.mgrid[0:na, 0:nb]
    one_map = np.zeros(ishape)
    one_map[0] = 1.0
    return {"ones": np.ones(ishape), "checker": np.broadcast_to((-1.0) ** (i + j), ishape).copy(),
            "random": np.random.default_rng(seed).standard_normal(ishape), "one_map": one_map}


def quad_parts(v, av, w, mu, mu_reg):
    """(data, prior) parts of v^T Q v from A v: mu (A v)^T W (A v), mu_reg (|Dr v|^2 + |Dc v|^2)."""
    return mu * float(np.sum(w * av * av)), mu_reg * float(np.sum(orc.diff_r(v) ** 2 + orc.diff_c(v) ** 2))


def identity_check(name, vb, vb_mean, vqv, draws):
    """The two assertions on the projections ``vb`` [draws] of a probe; returns (mean deviation in standard errors, variance ratio)."""
    dev = (np.mean(vb) - vb_mean) / np.sqrt(vqv / draws)
    ratio = np.var(vb, ddof=1) / vqv
    band = 5.0 * np.sqrt(2.0 / (draws - 1))
    print(f"identity {name}: mean off by {dev:+.2f} standard errors, variance ratio {ratio:.3f} (band 1 +- {band:.3f})")
    assert abs(dev) < 5.0, (name, dev)
    assert abs(ratio - 1.0) < band, (name, ratio)
    return dev, ratio


def rect_problem(na, nb, T, Lc=64):
    """A one-channel problem with T x na x nb maps (Na != Nb, odd sizes, no multiple of 64 allowed)."""
    rng = np.random.default_rng(31)
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(0.8 / 3600, 0.9 / 3600, (0.0, 0.0), 8.2, 0.196, 4, 3050.0, np.linspace(7.53, 7.67, 40), "S1")
    return dict(N=na, Lc=Lc, alpha_axis=orc.synthetic_axes(na, problems.STEP_DEG), beta_axis=orc.synthetic_axes(nb, problems.STEP_DEG),
                wavel=wav, specs=[spec], templates=rng.random((T, Lc)) + 0.5,
                sotf=orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (na, nb)),
                pointings=[orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)], maps=rng.random((T, na, nb)),
                step_deg=problems.STEP_DEG)
