"""Posterior sampling on the device (include/surfh_amd.h: surfh_randn_dev ... surfh_cg_sample) against the float64 restatement
of tests/posterior_oracle.py (needs an MI355X)."""
import numpy as np
import pytest

import posterior_oracle as po
import problems
from helpers import TOL, build_model, rel
from oracle import surfh_oracle as orc
from surfh_amd import posterior

pytestmark = pytest.mark.gpu
SEED = (0x1234ABCD << 32) | 0x9E3779B9              # a 64-bit seed with a non-zero high word
MU, MUR = 1.0, 5e3                                   # of test_cg_matches_oracle_lcg


def _data(cfg, om):
    y = om.forward(cfg["maps"])
    return y + np.random.default_rng(1).standard_normal(y.size) * 1e-2 * np.sqrt(np.mean(y ** 2))


@pytest.fixture(scope="module")
def c1():
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    yield cfg, om, m, _data(cfg, om)
    m.close()


def _sigma2(om, y):
    """The variance of the noise of ``_data``, from the data themselves (1e-4 of their mean square, to 1e-4)."""
    return 1e-4 * float(np.mean(y ** 2)) / (1.0 + 1e-4)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0")


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def test_randn_matches_restatement(c1):
    """Every size around the four-value group and the block, the three streams, two samples, a seed with a high word: within
    1e-5 absolute of the float64 restatement (about ten times fp32 rounding through log, sqrt and sincos at |z| <= 5.89), nothing
    written past n, the same bits from a second call and from a destination that is not 16-byte aligned."""
    import torch
    m = c1[2]
    worst = 0.0
    for n in (1, 3, 4, 5, 1023, 5123):
        for stream in (0, 1, 2):
            for sample in (0, 7):
                want = po.randn(n, SEED, stream, sample)
                outs = []
                for off in (0, 0, 1):                                  # off = 1: the scalar stores of an unaligned destination
                    buf = torch.full((n + 12,), 123.0, dtype=torch.float32, device="cuda:0")
                    m.randn_dev(buf[off:], n, SEED, stream, sample)
                    torch.cuda.synchronize()
                    h = buf.cpu().numpy()
                    assert np.all(h[:off] == 123.0) and np.all(h[off + n:] == 123.0), (n, stream, sample, off)
                    outs.append(h[off: off + n])
                assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
                worst = max(worst, float(np.max(np.abs(outs[0] - want))))
                assert np.max(np.abs(outs[0])) <= po.ZMAX
    print(f"randn: max |device - float64 restatement| = {worst:.2e}")
    assert worst < 1e-5
    a, b = (torch.empty(64, dtype=torch.float32, device="cuda:0") for _ in range(2))
    m.randn_dev(a, 64, SEED, 0, 0)
    m.randn_dev(b, 64, SEED & 0xFFFFFFFF, 0, 0)                       # the high word of the seed is part of the key
    assert not bool((a == b).any())


def _err(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("T", [1, 2, 5])
def test_po_data_and_prior_match_numpy(T):
    """T x 72 x 77 maps (Na != Nb, odd Nb, no multiple of 64) and a 5123-sample detector vector whose weight-0 samples hold NaN.
    Bound: ten times the error prior_add shows against NumPy on the same arrays."""
    import torch
    m = build_model(po.rect_problem(72, 77, T))
    try:
        assert m.ishape == (T, 72, 77)
        rng = np.random.default_rng(40 + T)
        er, ec = (rng.standard_normal(m.ishape).astype(np.float32) for _ in range(2))
        er64, ec64 = er.astype(np.float64), ec.astype(np.float64)
        mu_reg = 9.0
        q_t = _dev(ec)
        m.prior_add_dev(_dev(er), q_t, mu_reg)
        torch.cuda.synchronize()
        bound = 10 * _err(q_t.cpu().numpy(), ec64 + mu_reg * (orc.diff_r_t(orc.diff_r(er64)) + orc.diff_c_t(orc.diff_c(er64))))
        out_t = torch.full(m.ishape, 7.0, dtype=torch.float32, device="cuda:0")
        m.po_prior_dev(_dev(er), _dev(ec), out_t, mu_reg)
        torch.cuda.synchronize()
        e_prior = _err(out_t.cpu().numpy(), po.eta(er64, ec64, mu_reg))
        # the detector vector
        n, mu = 5123, 4.0
        y = (3.0 * rng.standard_normal(n)).astype(np.float32)
        w = rng.uniform(0.5, 2.0, n).astype(np.float32)
        dead = rng.random(n) < 0.05
        w[dead] = 0.0
        y[dead] = np.nan
        y.view(np.uint32)[np.flatnonzero(dead)[::2]] = 0x7FC12345       # NaNs with a payload: the bits pass through
        eps = rng.standard_normal(n).astype(np.float32)
        buf = torch.full((n + 8,), 123.0, dtype=torch.float32, device="cuda:0")
        m.po_data_dev(_dev(y), _dev(w), _dev(eps), buf, n, mu)
        plain = torch.empty(n, dtype=torch.float32, device="cuda:0")
        m.po_data_dev(_dev(np.where(dead, 0.0, y)), None, _dev(eps), plain, n, mu)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.all(got[n:] == 123.0)
        got = got[:n]
        assert np.array_equal(got.view(np.uint32)[dead], y.view(np.uint32)[dead]) and np.all(np.isfinite(got[~dead]))
        want = po.perturb_data(y.astype(np.float64), w.astype(np.float64), eps.astype(np.float64), mu)
        e_data = _err(got[~dead], want[~dead])
        e_plain = _err(plain.cpu().numpy(), np.where(dead, 0.0, y).astype(np.float64) + eps.astype(np.float64) / np.sqrt(mu))
        print(f"T = {T}: prior_add bound {bound:.2e}; po_prior {e_prior:.2e}, po_data {e_data:.2e}, without weights {e_plain:.2e}")
        assert 0 < bound < 1e-5
        assert e_prior < bound and e_data < bound and e_plain < bound
        # a factor sqrt(mu) or sqrt(mu_reg) amiss is far outside
        assert _err(got[~dead], po.perturb_data(y.astype(np.float64), w.astype(np.float64), eps.astype(np.float64), mu * mu)[~dead]) > 1e-2
    finally:
        m.close()


def _np_moments(xhat, samples):
    e = samples.astype(np.float64) - xhat.astype(np.float64)
    K = e.shape[0]
    d = e - e.mean(axis=0)
    return xhat.astype(np.float64) + e.mean(axis=0), np.einsum("kt...,ku...->tu...", d, d) / (K - 1)


@pytest.mark.parametrize("T", [1, 2, 5])
def test_po_moments_match_numpy(T):
    rng = np.random.default_rng(50 + T)
    xhat = rng.standard_normal((T, 72, 77)).astype(np.float32)
    for K in (2, 7):
        samples = (xhat + 0.1 * rng.standard_normal((K, T, 72, 77)) * (1 + np.arange(T))[None, :, None, None]).astype(np.float32)
        want_mean, want_cov = _np_moments(xhat, samples)
        for pix in ((0, 0), (71, 76), (13, 40)):                       # np.cov itself on a few pixels
            obs = samples[(slice(None), slice(None)) + pix].astype(np.float64) - xhat[(slice(None),) + pix]
            assert np.allclose(np.cov(obs, rowvar=False, ddof=1).reshape(T, T), want_cov[(slice(None), slice(None)) + pix], rtol=1e-12, atol=1e-15)
        runs = [posterior.po_moments(xhat, samples) for _ in range(2)]
        mean, cov = runs[0]
        assert cov.shape == (T, T, 72, 77) and np.array_equal(cov, cov.transpose(1, 0, 2, 3))
        em, ecv = _err(mean, want_mean), _err(cov, want_cov)
        print(f"T = {T}, K = {K}: mean {em:.2e}, cov {ecv:.2e}")
        assert em < 1e-6 and ecv < 1e-6
        assert np.array_equal(mean, runs[1][0]) and np.array_equal(cov, runs[1][1])
        only_mean, none = posterior.po_moments(xhat, samples, cov=False)
        assert none is None and np.array_equal(only_mean, mean)
    with pytest.raises(ValueError):
        posterior.po_moments(xhat, samples[:1])                          # a covariance of one sample


def test_po_moments_refuses_nine_maps():
    x = np.zeros((9, 72, 77), dtype=np.float32)
    with pytest.raises(ValueError, match="9 maps"):
        posterior.po_moments(x, np.zeros((2,) + x.shape, dtype=np.float32))


# ---- the perturbed right-hand side ---------------------------------------------------------------------------------------------
def _weighted(om, y):
    w = po.identity_weights(om.osize)
    yn = y.copy()
    yn[w == 0] = np.nan
    return w, yn


def test_po_rhs_with_the_generator_matches_oracle(c1):
    """The same draw (same seed, restated generator) under weights with NaN data at weight 0: the bound of the adjoint's parity."""
    cfg, om, m, y = c1
    w, yn = _weighted(om, y)
    mu, mu_reg = po.IDENTITY["mu"], po.IDENTITY["mu_reg"]
    m.set_data_weights(w)
    try:
        for sample in (0, 3):
            bt = posterior.po_rhs(m, yn, mu, mu_reg, SEED, sample)
            want = po.rhs(om, yn, w, mu, mu_reg, po.draw(om, SEED, sample))
            e = rel(bt, want)
            print(f"po_rhs sample {sample}: {e:.2e}")
            assert np.all(np.isfinite(bt)) and e < TOL
        assert np.array_equal(posterior.po_rhs(m, yn, mu, mu_reg, SEED, 3), bt)
        eps = po.draw(om, 11, 0)
        assert rel(posterior.po_rhs(m, yn, mu, mu_reg, perturbation=eps), po.rhs(om, yn, w, mu, mu_reg, eps)) < TOL
    finally:
        m.set_data_weights(None)
    bt = posterior.po_rhs(m, y, mu, 0.0, SEED, 1)                       # no weights, no prior
    assert rel(bt, po.rhs(om, y, None, mu, 0.0, po.draw(om, SEED, 1))) < TOL


def test_covariance_identity_on_the_device(c1):
    """tests/test_posterior_host.py::test_covariance_identity with the 400 draws made by surfh_po_rhs: same probes, same bands.
    v^T Q v comes from fwadj (A^T W A v under the installed weights) plus the prior."""
    cfg, om, m, y = c1
    mu, mu_reg, draws, seed = (po.IDENTITY[k] for k in ("mu", "mu_reg", "draws", "seed"))
    w = po.identity_weights(om.osize)
    yn = po.identity_data(om, cfg["maps"], w, mu)
    y = np.where(w > 0, yn, 0.0)
    V = po.probes(om.ishape)
    m.set_data_weights(w)
    try:
        proj = {k: np.empty(draws) for k in V}
        for d in range(draws):
            bt = posterior.po_rhs(m, yn, mu, mu_reg, seed, d)
            for k, v in V.items():
                proj[k][d] = np.vdot(v, bt)
        b = mu * m.adjoint(np.where(w > 0, w * np.where(w > 0, y, 0.0), 0.0))
        shares = {}
        for k, v in V.items():
            qd = mu * float(np.vdot(v, m.fwadj(v)))
            qp = mu_reg * float(np.sum(orc.diff_r(v) ** 2 + orc.diff_c(v) ** 2))
            shares[k] = qp / (qd + qp)
            po.identity_check(k, proj[k], float(np.vdot(v, b)), qd + qp, draws)
        assert shares["ones"] < 1e-3 and shares["checker"] > 0.999
    finally:
        m.set_data_weights(None)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
def _explicit(om, K, seed):
    d = [po.draw(om, seed, k) for k in range(K)]
    return tuple(np.stack([e[j].reshape(-1) for e in d]) for j in range(3))


def _check_samples(om, m, y, K, nit, checked=None):
    """K explicit draws; the first ``checked`` (all by default) against the oracle's CG, all of them against NumPy's moments.
    The system is that of test_cg_matches_oracle_lcg (mu = 1, mu_reg = 5e3) at the statistical scale of its data: both weights
    divided by sigma^2, the variance of the noise ``_data`` adds, so that a draw is a second noise realisation and x~ - x_map is
    large enough to be read back from the fp32 x~ the callback receives."""
    checked = K if checked is None else checked
    sig2 = _sigma2(om, y)
    mu, mur = 1.0 / sig2, 5e3 / sig2
    pert = _explicit(om, K, 21)
    seen = []
    res = m.sample_posterior(y, mu=mu, mu_reg=mur, n_samples=K, max_iter=nit, perturbations=pert,
                             callback=lambda k, rr, x: seen.append((k, rr, x)))
    x, gn, n = m.cg(y, mu=mu, mu_reg=mur, max_iter=nit)
    assert np.array_equal(res.x_map, x) and np.array_equal(res.grad_norm, gn) and res.nit == n == nit
    assert [s[0] for s in seen] == list(range(K))
    for k in range(checked):
        eps = (pert[0][k], pert[1][k].reshape(om.ishape), pert[2][k].reshape(om.ishape))
        # the device's eps are float32: the oracle gets the same numbers
        eps = tuple(e.astype(np.float32).astype(np.float64) for e in eps)
        ref = po.sample(om, None, mu, mur, eps, res.x_map, nit)
        gr, rr = np.array(ref["grad_norm"]), seen[k][1]
        ex, eg = rel(seen[k][2], ref["x"]), float(np.max(np.abs(rr[:10] - gr[:10]) / gr[:10]))
        ee = rel(seen[k][2] - res.x_map, ref["e"])                     # the deviation itself, not hidden behind x_map
        print(f"sample {k}: x~ {ex:.2e}, x~ - x_map {ee:.2e}, first ten r.r {eg:.2e}; |x~ - x_map| / |x_map| = "
              f"{rel(seen[k][2], res.x_map):.2e}")
        assert len(rr) == nit + 1 and ex < 3e-3 and ee < 3e-3 and eg < 2e-4
        assert rel(seen[k][2], res.x_map) > 100 * ex                   # a draw, not the point estimate again
    xs = np.stack([s[2] for s in seen]).astype(np.float32)
    want_mean, want_cov = _np_moments(res.x_map.astype(np.float32), xs)
    # the device sums the deviations e themselves; here they are read back from the fp32 x~ = x_map + e the callback received,
    # each off by up to 2^-24 |x~|: relative to the largest variance that is 4 * 2^-24 max |x~| / max std on top of the 1e-6 at
    # which test_po_moments_match_numpy pins the kernels
    slack = 4 * 2.0 ** -24 * float(np.max(np.abs(xs))) / float(np.sqrt(np.max(want_cov)))
    print(f"moments: mean {_err(res.mean, want_mean):.2e}, cov {_err(res.cov, want_cov):.2e} (bound {1e-6 + slack:.2e})")
    assert _err(res.mean, want_mean) < 1e-6 and _err(res.cov, want_cov) < 1e-6 + slack
    assert np.array_equal(res.std, np.sqrt(np.einsum("ttab->tab", res.cov)))
    assert res.rr_worst == max(s[1][-1] for s in seen)
    return res


def test_sample_posterior_matches_oracle_map_domain(c1):
    """K = 3 explicit draws on config 1, 10 iterations, against the posterior oracle's CG at the bounds of
    test_cg_matches_oracle_lcg (first ten r.r within 2e-4, x~ within 3e-3); x_map is m.cg's bit for bit."""
    cfg, om, m, y = c1
    print("config1 spectral loop:", m.spec_supported())
    res = _check_samples(om, m, y, 3, 10)
    cs = m.cube_std(res.cov, planes=[0, 64, 127])
    want = np.sqrt(np.einsum("tl,tuab,ul->lab", cfg["templates"][:, [0, 64, 127]], res.cov, cfg["templates"][:, [0, 64, 127]]))
    assert cs.shape == (3, 64, 64) and np.allclose(cs, want, rtol=1e-12)


def test_sample_posterior_matches_oracle_spectral():
    """One draw on two_channel_mid: the spectral loop, where the extra right-hand side goes through surfh_to_spec_dev."""
    cfg = problems.two_channel_mid()
    om = problems.oracle_model(cfg, box="direct")
    m = build_model(cfg)
    try:
        assert m.spec_supported()
        _check_samples(om, m, _data(cfg, om), 2, 10, checked=1)
    finally:
        m.close()


def test_determinism_and_plumbing(c1):
    cfg, om, m, y = c1
    kw = dict(mu=MU, mu_reg=MUR, n_samples=4, max_iter=5)
    before = m.cg(y, mu=MU, mu_reg=MUR, max_iter=5)
    a, b, c = m.sample_posterior(y, seed=SEED, **kw), m.sample_posterior(y, seed=SEED, **kw), m.sample_posterior(y, seed=SEED + 1, **kw)
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.cov, b.cov) and a.rr_worst == b.rr_worst
    assert not np.array_equal(a.mean, c.mean) and not np.array_equal(a.cov, c.cov)
    assert a.cov.shape == (4, 4, 64, 64) and a.std.shape == (4, 64, 64) and np.all(a.std > 0) and a.n_samples == 4
    # the extra right-hand side does not leak into the next solve
    after = m.cg(y, mu=MU, mu_reg=MUR, max_iter=5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # weights= is installed for the run and what the model held is put back
    w, yn = _weighted(om, y)
    rw = m.sample_posterior(yn, seed=SEED, weights=w, **kw)
    assert m.data_weights is None and np.all(np.isfinite(rw.mean)) and np.all(np.isfinite(rw.cov))
    xw = m.cg(yn, mu=MU, mu_reg=MUR, max_iter=5, weights=w)[0]
    assert np.array_equal(rw.x_map, xw) and not np.array_equal(rw.x_map, a.x_map)
    held = np.full(om.osize, 2.0)
    m.set_data_weights(held)
    try:
        m.sample_posterior(yn, seed=SEED, weights=w, **kw)
        assert np.array_equal(m.data_weights, held.astype(np.float32))
    finally:
        m.set_data_weights(None)
    # mu_reg = 0: no prior noise is drawn or read
    r0 = m.sample_posterior(y, mu=MU, mu_reg=0.0, n_samples=2, max_iter=3, perturbations=(_explicit(om, 2, 3)[0], None, None))
    assert np.all(np.isfinite(r0.cov))


def test_refusals(c1):
    from surfh_amd import imager
    from surfh_amd.imager import ImagerModel
    cfg, om, m, y = c1
    for bad in (dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(mu_reg=-1.0), dict(n_samples=1), dict(n_samples=0)):
        with pytest.raises(ValueError):
            m.sample_posterior(y, **{**dict(mu=MU, mu_reg=MUR, n_samples=2, max_iter=2), **bad})
    m.set_prior("joint")
    try:
        with pytest.raises(ValueError, match="separated"):
            m.sample_posterior(y, mu=MU, mu_reg=MUR, n_samples=2, max_iter=2)
        with pytest.raises(RuntimeError, match="separated"):             # the library refuses on its own
            posterior.po_rhs(m, y, MU, MUR)
    finally:
        m.set_prior("separated")
    im = ImagerModel(m, imager.synthetic_filters(cfg["wavel"], 3), decim=3)
    m.set_imager(im)
    try:
        m.set_imager_data(np.zeros(im.osize), 0.5)
        with pytest.raises(ValueError, match="imager"):
            m.sample_posterior(y, mu=MU, mu_reg=MUR, n_samples=2, max_iter=2)
        with pytest.raises(RuntimeError, match="imager"):
            posterior.po_rhs(m, y, MU, MUR)
    finally:
        m.set_imager(None)
    with pytest.raises(RuntimeError, match="mu ="):
        posterior.po_rhs(m, y, 0.0, MUR)
    plain = build_model(dict(cfg, templates=None))
    try:
        with pytest.raises(ValueError, match="templates"):
            plain.sample_posterior(np.zeros(plain.osize), mu=MU, mu_reg=MUR, n_samples=2, max_iter=2)
    finally:
        plain.close()
    x, gn, n = m.cg(y, mu=MU, mu_reg=MUR, max_iter=2)                   # the model is as it was
    assert n == 2 and np.all(np.isfinite(x))
