"""Plane-wise posterior sampling on the device (``MRSBlurred.sample_posterior``; include/surfh_amd.h: surfh_cg_planes_sample,
surfh_po_planes_rhs, surfh_po_planes_moments, surfh_debug_po_planes) against the staged kernels of the map-domain sampler, bit
for bit, and against the float64 restatement of tests/posterior_planes_oracle.py, whose own identity
tests/test_posterior_planes_host.py checks without a GPU.  Needs an MI355X.

How a sample's deviation is read: e = x~ - x_map does not depend on the data (Q e = b~ - b), so a run on zero data from zero has
x_map = 0 exactly and hands the callback e itself, with no fp32 rounding of x_map + e on top.  The oracle comparison uses that run.
Measured on MI355X: DESIGN.md, "Plane-wise posterior sampling"."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
from click.testing import CliRunner

import huber_planes_oracle as hp
import posterior_oracle as po
import posterior_planes_oracle as ppo
import rotated_oracle as ro
from helpers import TOL, build_model, rel
from oracle import surfh_oracle as orc
from surfh_amd import _lib, posterior
from test_gpu_huber_planes import _plane_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0x1234ABCD << 32) | 0x9E3779B9              # a 64-bit seed with a non-zero high word
NIT = 8
# the fused kernels make four elements per thread and trip on grid_for's 4096 blocks of 256 threads: a launch meets the cap, and its
# threads take a second trip, beyond 4 * 4096 * 256 elements
GRID_CAP_ELEMENTS = 4 * 4096 * 256


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0")


def _err(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def pm():
    """The shared plane-wise model (5 planes of 96 x 96)."""
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    yield m
    m.close()


# ---- 1. the fused kernels against the staged ones, bit for bit ---------------------------------------------------------------------
def _fused(m, which, n, off, **kw):
    """One fused kernel into a guarded buffer, `off` floats in: the n floats written; the guards are checked."""
    import torch
    buf = torch.full((n + 12,), 123.0, dtype=torch.float32, device="cuda:0")
    m.po_planes_dev(which, buf[off:], **kw)
    h = buf.cpu().numpy()
    assert np.all(h[:off] == 123.0) and np.all(h[off + n:] == 123.0), (which, kw.get("shape"), n, off, "written outside its floats")
    return h[off: off + n]


def _staged_prior_fp32(er, ec, L, na, nb, mu_reg):
    """po_prior_kernel's one expression, s ((er[i+1] - er) + (ec[j+1] - ec)), in fp32 NumPy on the values randn_dev stored: four
    IEEE operations with nothing to contract, so the same bits as the staged kernel."""
    er, ec = er.reshape(L, na, nb), ec.reshape(L, na, nb)
    s = np.float32(np.sqrt(mu_reg))
    return (s * ((np.roll(er, -1, axis=1) - er) + (np.roll(ec, -1, axis=2) - ec))).ravel()


@pytest.mark.parametrize("L,na,nb", [(1, 1, 1), (1, 2, 3), (3, 5, 7), (2, 72, 77), (17, 512, 512)])
def test_fused_eta_is_the_staged_kernels_bit_for_bit(pm, L, na, nb):
    """Rows that are no multiple of 4: the Philox groups straddle row and plane ends, and the wraps stay inside a plane.
    (17, 512, 512) = 4456448 elements passes GRID_CAP_ELEMENTS = 4194304: the grid is capped and the loop takes a second trip.
    Staged: randn_dev on streams 1 and 2 (any plan: it gives its stream only), then po_prior_dev, which takes its extents from its
    plan -- a ``po.rect_problem`` model with T = L maps of 72 x 77, and with T = 1 map of 512 x 512 for the 17 planes one by one (the
    kernel takes every map alike; 17 templates are more than a plan holds).  The three smallest shapes are smaller than that problem's
    field of view (32 x 36 pixels), so no template model has their extents: there, and on the others as well, the staged prior is
    ``_staged_prior_fp32`` on the staged noise."""
    import torch
    n, mu_reg = L * na * nb, 9.0
    assert (n > GRID_CAP_ELEMENTS) == (L == 17)
    big = L == 17
    mt = build_model(po.rect_problem(na, nb, 1 if big else L)) if na >= 72 else None
    try:
        worst = 0.0
        for sample in (0, 7):
            er, ec, want_t = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(3))
            for t, stream in ((er, po.STREAM_R), (ec, po.STREAM_C)):
                _lib.check(pm._L.surfh_randn_dev(pm._plan, _lib.dev_ptr(t), n, _lib.seed64(SEED), stream, sample))
            torch.cuda.synchronize()
            want = _staged_prior_fp32(er.cpu().numpy(), ec.cpu().numpy(), L, na, nb, mu_reg)
            if mt is not None:
                for l in (range(L) if big else (0,)):
                    s = slice(l * na * nb, (l + 1) * na * nb) if big else slice(None)
                    mt.po_prior_dev(er[s], ec[s], want_t[s], mu_reg)
                torch.cuda.synchronize()
                assert np.array_equal(want_t.cpu().numpy().view(np.uint32), want.view(np.uint32))
            outs = [_fused(pm, "eta", n, off, shape=(L, na, nb), seed=SEED, sample=sample, mu_reg=mu_reg) for off in (0, 0, 1)]
            for o in outs:                                              # off = 1: a destination that is not 16-byte aligned
                assert np.array_equal(o.view(np.uint32), want.view(np.uint32)), (L, na, nb, sample)
            if not big:                                                 # the float64 restatement
                eps = ppo.draw(SEED, sample, L, na, nb, nout=1)
                worst = max(worst, float(np.max(np.abs(outs[0].reshape(L, na, nb) - ppo.eta(eps[1], eps[2], mu_reg)))))
        bound = 1e-5 * np.sqrt(mu_reg) * 4                              # four normals, each within 1e-5, times sqrt(mu_reg)
        print(f"eta {L} x {na} x {nb}: max |device - float64| = {worst:.2e} (bound {bound:.1e})")
        assert worst < bound
        other = _fused(pm, "eta", n, 0, shape=(L, na, nb), seed=SEED & 0xFFFFFFFF, sample=0, mu_reg=mu_reg)
        assert n == 1 or not np.array_equal(other, outs[0])             # the high word of the seed is part of the key (1 x 1: eta = 0)
    finally:
        if mt is not None:
            mt.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_fused_data_is_the_staged_kernels_bit_for_bit(pm, weighted):
    """randn_dev on stream 0 followed by po_data_dev(y = None), with and without weights (5 % of them zero: the output is 0 there)."""
    import torch
    mu = 4.0
    worst = 0.0
    for n in (1, 3, 4, 5, 1023, 5123):
        rng = np.random.default_rng(n)
        w = rng.uniform(0.5, 2.0, n).astype(np.float32)
        w[rng.random(n) < 0.05] = 0.0
        if n == 5:
            w[2] = 0.0
        for sample in (0, 7):
            eps, want_t = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
            pm._L.surfh_randn_dev(pm._plan, _lib.dev_ptr(eps), n, _lib.seed64(SEED), po.STREAM_Y, sample)
            for off in (0, 0, 1):
                wbuf = torch.zeros(n + 4, dtype=torch.float32, device="cuda:0")
                wbuf[off: off + n] = _dev(w)
                w_t = wbuf[off:] if weighted else None
                _lib.check(pm._L.surfh_po_data_dev(pm._plan, None, _lib.dev_ptr(w_t), _lib.dev_ptr(eps), n, mu, _lib.dev_ptr(want_t)))
                torch.cuda.synchronize()
                want = want_t.cpu().numpy()
                got = _fused(pm, "data", n, off, n_out=n, seed=SEED, sample=sample, mu=mu, w_t=w_t)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, sample, off)
            ref = po.randn(n, SEED, po.STREAM_Y, sample) / np.sqrt(mu * np.where(w > 0, w, 1.0) if weighted else mu)
            if weighted:
                assert not got[w == 0].any() and (n < 1000 or np.any(w == 0))
                ref[w == 0] = 0.0
            worst = max(worst, float(np.max(np.abs(got - ref))))
    print(f"data, weights {weighted}: max |device - float64| = {worst:.2e}")
    # one normal within 1e-5 (test_randn_matches_restatement), three fp32 roundings of |z| <= ZMAX on top, over sqrt(mu w), w >= 0.5
    assert worst < (1e-5 + 3 * 2.0 ** -24 * po.ZMAX) / np.sqrt(mu * 0.5)


def test_debug_entry_refuses_bad_arguments(pm):
    import torch
    t = torch.zeros(16, dtype=torch.float32, device="cuda:0")
    for kw in (dict(which="eta", shape=(0, 2, 2)), dict(which="eta", shape=(1, 2, 2), mu_reg=-1.0), dict(which="data", n_out=-1),
               dict(which="data", n_out=4, mu=0.0), dict(which="noise", n_out=4), dict(which="eta", shape=(1, 2, 2), sample=-1)):
        which = kw.pop("which")
        with pytest.raises(ValueError):
            pm.po_planes_dev(which, t, **kw)


# ---- 2. the moments ---------------------------------------------------------------------------------------------------------------
def _np_moments(xhat, samples):
    e = samples.astype(np.float64) - xhat.astype(np.float64)
    return xhat.astype(np.float64) + e.mean(axis=0), e.var(axis=0, ddof=1)


@pytest.mark.parametrize("shape", [(3, 72, 77), (3, 5, 7)])
def test_po_planes_moments_match_numpy(shape):
    """L = 3, npix = 72 * 77 (an even count: the 16-byte path) and 5 * 7 (odd: the scalar path); mean and variance within 1e-6
    relative to the largest variance, the bound of test_po_moments_match_numpy; a second run gives the same bits."""
    rng = np.random.default_rng(60)
    xhat = rng.standard_normal(shape).astype(np.float32)
    for K in (2, 7):
        samples = (xhat + 0.1 * rng.standard_normal((K,) + shape) * (1 + np.arange(3))[None, :, None, None]).astype(np.float32)
        want_mean, want_var = _np_moments(xhat, samples)
        runs = [posterior.po_planes_moments(xhat, samples) for _ in range(2)]
        mean, var = runs[0]
        em, ev = float(np.max(np.abs(mean - want_mean)) / np.max(want_var)), _err(var, want_var)
        print(f"{shape}, K = {K}: mean {em:.2e}, var {ev:.2e}")
        assert mean.shape == var.shape == shape and em < 1e-6 and ev < 1e-6 and np.all(var > 0)
        assert np.array_equal(mean, runs[1][0]) and np.array_equal(var, runs[1][1])
        only_mean, none = posterior.po_planes_moments(xhat, samples, var=False)
        assert none is None and np.array_equal(only_mean, mean)
    with pytest.raises(ValueError, match="at least 2"):
        posterior.po_planes_moments(xhat, samples[:1])                   # a variance of one sample
    assert np.array_equal(posterior.po_planes_moments(xhat, samples[:1], var=False)[0], xhat.astype(np.float64) + (samples[0].astype(np.float64) - xhat))
    # a constant sample set: the variance is exactly 0, never negative.  The deviations are fp32 numbers, as the sampler's are (it
    # accumulates the fp32 solution of Q e = b~ - b): about zero, and a constant 0.25 above small integers
    for base, const in ((np.zeros(shape, np.float32), xhat), (np.rint(8 * xhat).astype(np.float32), np.rint(8 * xhat).astype(np.float32) + np.float32(0.25))):
        mean, var = posterior.po_planes_moments(base, np.broadcast_to(const[None], (7,) + shape))
        assert not var.any() and not np.signbit(var).any() and np.array_equal(mean, const.astype(np.float64))


# ---- 3. the right-hand side and the identity ----------------------------------------------------------------------------------------
def test_po_planes_rhs_with_the_generator_matches_oracle(pm):
    """The same draw (same seed, restated generator) under weights with NaN data at weight 0: helpers.TOL per plane."""
    mu, mu_reg = po.IDENTITY["mu"], po.IDENTITY["mu_reg"]
    w, yn, _ = ppo.identity_problem()
    pm.set_data_weights(w)
    try:
        for sample in (0, 3):
            bt = posterior.po_planes_rhs(pm, yn, mu, mu_reg, SEED, sample)
            eps = ppo.draw(SEED, sample)
            assert bt.shape == (hp.L, hp.N, hp.N) and np.all(np.isfinite(bt))
            for l in range(hp.L):
                e = rel(bt[l], ppo.rhs(ppo.plane(l), yn[l], w[l], mu, mu_reg, ppo.of_plane(eps, l)))
                print(f"po_planes_rhs sample {sample}, plane {l}: {e:.2e}")
                assert e < TOL
        assert np.array_equal(posterior.po_planes_rhs(pm, yn, mu, mu_reg, SEED, 3), bt)
        eps = ppo.draw(11, 0)
        be = posterior.po_planes_rhs(pm, yn, mu, mu_reg, perturbation=eps)
        for l in (0, hp.L - 1):
            assert rel(be[l], ppo.rhs(ppo.plane(l), yn[l], w[l], mu, mu_reg, ppo.of_plane(eps, l))) < TOL
    finally:
        pm.set_data_weights(None)


def test_covariance_identity_on_the_device(pm):
    """tests/test_posterior_planes_host.py::test_covariance_identity_plane_by_plane with the 400 draws made by surfh_po_planes_rhs:
    same probes, same bands.  v^T Q_l v comes from the device's A v under the weights, plus the prior."""
    mu, mu_reg, draws, seed = (po.IDENTITY[k] for k in ("mu", "mu_reg", "draws", "seed"))
    w, yn, y0 = ppo.identity_problem()
    V = ppo.probes()
    pm.set_data_weights(w)
    try:
        proj = {(l, k): np.empty(draws) for l in range(hp.L) for k in V}
        for d in range(draws):
            bt = posterior.po_planes_rhs(pm, yn, mu, mu_reg, seed, d)
            for l in range(hp.L):
                for k, v in V.items():
                    proj[l, k][d] = np.vdot(v[0], bt[l])
        b = mu * pm.adjoint(w * y0)
        av = {k: pm.forward(np.broadcast_to(v, (hp.L, hp.N, hp.N))) for k, v in V.items()}

        ppo.identity_checks(lambda l, k, v: proj[l, k], lambda l, v: float(np.vdot(v[0], b[l])),
                            lambda l, k, v: po.quad_parts(v, av[k][l], w[l], mu, mu_reg))
    finally:
        pm.set_data_weights(None)


# ---- 4. the sampler against the oracle ------------------------------------------------------------------------------------------------
def _explicit(L, na, nb, nout, K, seed):
    """K draws of the restated generator, rounded to fp32 as the device holds them: ([K, osize], [K, isize], [K, isize])."""
    d = [ppo.draw(seed, k, L, na, nb, nout) for k in range(K)]
    return tuple(np.stack([e[j].reshape(-1) for e in d]).astype(np.float32) for j in range(3))


def _scale(y_plane):
    """mu and mu_reg at the statistical scale of the data, as test_gpu_posterior._check_samples puts them: both weights of the
    problem divided by the variance of the noise ``hp.problem`` adds to a plane (1e-4 of its mean square)."""
    sig2 = 1e-4 * float(np.mean(np.asarray(y_plane) ** 2)) / (1.0 + 1e-4)
    return hp.MU / sig2, hp.MUR / sig2


def _yardstick(m, ops, y, x0, mu, mur, planes):
    """The error of the unperturbed ``m.cg`` -- code from before the sampler -- against ``orc.lcg`` on the given planes over NIT
    iterations: (x, r.r trace), each the worst plane's.  The samples run the same operator and the same loop and are held to twice it."""
    x, gn, nit = m.cg(y, mu=mu, mu_reg=mur, x0=x0, max_iter=NIT)
    x, gn = x.reshape((len(ops),) + x.shape[-2:]), gn.reshape(NIT + 1, len(ops))
    ex = eg = 0.0
    for l in planes:
        ref = orc.lcg(ops[l], np.asarray(y).reshape(len(ops), -1)[l], mu, mur, np.asarray(x0).reshape(x.shape)[l][None], max_iter=NIT)
        gr = np.array(ref["grad_norm"])
        ex, eg = max(ex, rel(x[l], ref["x"][0])), max(eg, float(np.max(np.abs(gn[:, l] - gr) / gr)))
    assert nit == NIT and ex > 0 and eg > 0
    return ex, eg


def _check_samples(m, ops, y, x0, mu, mur, K, checked, yard, squeeze=False):
    """K explicit draws (seed 21).  Run A on the data: x_map, grad_norm, nit are m.cg's bits, the moments are NumPy's of the
    callback's samples, rr_first / rr_last the maxima of the callback's traces.  Run B on zero data from zero: x_map = 0 and the
    callback's x~ is the deviation e itself; the first ``checked`` draws, every plane, against ``po.sample`` within twice ``yard``."""
    L = len(ops)
    na, nb = ops[0].ishape[1:]
    pert = _explicit(L, na, nb, ops[0].osize, K, 21)
    shape = (na, nb) if squeeze else (L, na, nb)
    seen, devs = [], []
    res = m.sample_posterior(y, mu=mu, mu_reg=mur, n_samples=K, x0=x0, max_iter=NIT, perturbations=pert,
                             callback=lambda k, rr, x: seen.append((k, rr, x)))
    x, gn, n = m.cg(y, mu=mu, mu_reg=mur, x0=x0, max_iter=NIT)
    assert np.array_equal(res.x_map, x) and np.array_equal(res.grad_norm, gn) and res.nit == n == NIT
    assert [s[0] for s in seen] == list(range(K)) and all(s[1].shape == ((NIT + 1,) if squeeze else (NIT + 1, L)) and s[2].shape == shape for s in seen)
    assert res.mean.shape == res.var.shape == res.std.shape == res.x_map.shape == shape and res.n_samples == K
    zero = m.sample_posterior(np.zeros(m.oshape), mu=mu, mu_reg=mur, n_samples=K, max_iter=NIT, perturbations=pert,
                              callback=lambda k, rr, xx: devs.append((rr.reshape(NIT + 1, L), xx.reshape(L, na, nb))))
    assert not zero.x_map.any() and np.isfinite(zero.var).all()
    ex_y, eg_y = yard
    worst_e = worst_g = 0.0
    for k in range(checked):
        eps = tuple(p[k].astype(np.float64) for p in pert)
        eps = (eps[0].reshape(L, -1), eps[1].reshape(L, na, nb), eps[2].reshape(L, na, nb))
        for l in range(L):
            ref = ppo.sample(ops[l], None, mu, mur, ppo.of_plane(eps, l), np.zeros((na, nb)), NIT)
            gr = np.array(ref["grad_norm"])
            ee, eg = rel(devs[k][1][l], ref["e"]), float(np.max(np.abs(devs[k][0][:, l] - gr) / gr))
            worst_e, worst_g = max(worst_e, ee), max(worst_g, eg)
            a = seen[k][2].reshape(L, na, nb)[l] - res.x_map.reshape(L, na, nb)[l]
            print(f"sample {k}, plane {l}: e {ee:.2e} (bound {2 * ex_y:.2e}), r.r trace {eg:.2e} (bound {2 * eg_y:.2e}); "
                  f"|e| = {np.linalg.norm(a):.2e}, |x_map| = {np.linalg.norm(res.x_map.reshape(L, na, nb)[l]):.2e}")
            # the deviations of run A are those of run B up to the fp32 rounding of x_map + e
            assert np.max(np.abs(a - devs[k][1][l])) <= 2.0 ** -23 * np.max(np.abs(seen[k][2]))
    print(f"cg against lcg: x {ex_y:.2e}, r.r trace {eg_y:.2e}; samples against po.sample: e {worst_e:.2e}, r.r trace {worst_g:.2e}")
    assert worst_e < 2 * ex_y and worst_g < 2 * eg_y
    xs = np.stack([s[2] for s in seen]).astype(np.float32)
    want_mean, want_var = _np_moments(res.x_map.astype(np.float32), xs)
    # the device sums the deviations e themselves; here they are read back from the fp32 x~ = x_map + e the callback received, each
    # off by up to 2^-24 |x~|: relative to the largest variance that is 4 * 2^-24 max |x~| / max std on top of the 1e-6 of the kernels
    slack = 4 * 2.0 ** -24 * float(np.max(np.abs(xs))) / float(np.sqrt(np.max(want_var)))
    em, ev = float(np.max(np.abs(res.mean - want_mean)) / np.max(want_var)), _err(res.var, want_var)
    print(f"moments: mean {em:.2e}, var {ev:.2e} (bound {1e-6 + slack:.2e})")
    assert em < 1e-6 + slack and ev < 1e-6 + slack and np.array_equal(res.std, np.sqrt(res.var))
    first, last = (np.max([np.atleast_2d(s[1].reshape(NIT + 1, L))[i] for s in seen], axis=0) for i in (0, -1))
    assert np.array_equal(np.atleast_1d(res.rr_first), first) and np.array_equal(np.atleast_1d(res.rr_last), last) and np.all(first > 0)
    return res


@pytest.fixture(scope="module")
def shared(pm):
    """The shared problem at its statistical scale, the float64 planes and the yardstick of the comparisons."""
    _, x0, y = hp.problem()
    mu, mur = _scale(y[0])
    ops = [ppo.plane(l) for l in range(hp.L)]
    return ops, y, x0, mu, mur, _yardstick(pm, ops, y, x0, mu, mur, hp.COMPARED)


def test_sampler_matches_oracle_plane_by_plane(pm, shared):
    """K = 3 explicit draws, 8 iterations, on hp.problem(): one plane without data, plane QUIET of amplitude 1e-3.  Every sample's
    deviation and r.r trace against ``po.sample`` on every plane -- hp.COMPARED and the empty one -- within twice the error ``m.cg``
    shows against ``orc.lcg`` on hp.COMPARED (the empty plane's unperturbed solve is 0 = 0 and measures nothing)."""
    ops, y, x0, mu, mur, yard = shared
    res = _check_samples(pm, ops, y, x0, mu, mur, 3, 3, yard)
    assert np.all(res.std > 0) and np.all(np.isfinite(res.std))


def test_sampler_on_the_rotated_field_model():
    from surfh_amd.spectro_blind import MRSBlurred
    case = ro.small_case(L=2)
    m = _plane_model(case["sotf"], 96, 96, cls=MRSBlurred, spec=case["spec"], pts=case["pointings"])
    try:
        ops = [ppo.Plane(ro.oracle_of(case, sotf=case["sotf"][l])) for l in range(2)]
        truth, x0, _ = hp.problem()
        truth, x0 = truth[[0, 1]], x0[[0, 1]]
        y = np.stack([ops[l].forward(truth[l][None]) for l in range(2)])
        y = y + 1e-2 * np.sqrt(np.mean(y ** 2, axis=1, keepdims=True)) * np.random.default_rng(3).standard_normal(y.shape)
        mu, mur = _scale(y[0])
        _check_samples(m, ops, y, x0, mu, mur, 2, 1, _yardstick(m, ops, y, x0, mu, mur, (0, 1)))
    finally:
        m.close()


def test_sampler_on_a_single_image_model(shared):
    ops, y, x0, mu, mur, _ = shared
    m1 = _plane_model(hp.sotf(0), hp.N, hp.N)
    try:
        res = _check_samples(m1, ops[:1], y[0], x0[0], mu, mur, 2, 1, _yardstick(m1, ops[:1], y[0], x0[0], mu, mur, (0,)), squeeze=True)
        assert res.grad_norm.shape == (NIT + 1,) and isinstance(res.rr_first, float) and isinstance(res.rr_last, float)
        from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D
        q = QuadCriterion_MRS_2D(mu, y[0], m1, mur)
        r = q.sample(n_samples=2, seed=SEED, maximum_iterations=NIT, value_init=x0[0])
        assert np.array_equal(r.x_map.ravel(), q.run_method("lcg", NIT, value_init=x0[0]).x) and r.std.shape == (hp.N, hp.N)
    finally:
        m1.close()


# ---- 5. determinism and plumbing ------------------------------------------------------------------------------------------------------
def counts():
    live, total = C.c_int64(), C.c_int64()
    _lib.load().surfh_debug_alloc_count(C.byref(live), C.byref(total))
    return live.value, total.value


def test_determinism_and_plumbing(pm, shared):
    ops, y, x0, mu, mur, yard = shared
    kw = dict(mu=mu, mu_reg=mur, n_samples=4, max_iter=5)
    before = pm.cg(y, mu=mu, mu_reg=mur, max_iter=5)
    a, b, c = (pm.sample_posterior(y, seed=s, **kw) for s in (SEED, SEED, SEED + 1))
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("x_map", "mean", "var", "std", "rr_first", "rr_last", "grad_norm"))
    assert not np.array_equal(a.mean, c.mean) and not np.array_equal(a.var, c.var) and np.array_equal(a.x_map, c.x_map)
    assert a.var.shape == (hp.L, hp.N, hp.N) and np.all(a.std > 0) and np.all(np.isfinite(a.std)) and a.n_samples == 4
    # the extra right-hand side does not leak into the next solve
    after = pm.cg(y, mu=mu, mu_reg=mur, max_iter=5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(a.x_map, before[0])
    # the generator's draws are the restated generator's: its path and the explicit one given the same values agree within the
    # bound of the oracle comparison (the deviations themselves: zero data)
    zeros, K = np.zeros(pm.oshape), 2
    g, e = [], []
    pm.sample_posterior(zeros, mu=mu, mu_reg=mur, n_samples=K, seed=SEED, max_iter=NIT, callback=lambda k, rr, x: g.append(x))
    pm.sample_posterior(zeros, mu=mu, mu_reg=mur, n_samples=K, max_iter=NIT, perturbations=_explicit(hp.L, hp.N, hp.N, ops[0].osize, K, SEED),
                        callback=lambda k, rr, x: e.append(x))
    for k in range(K):
        d = max(rel(g[k][l], e[k][l]) for l in range(hp.L))
        print(f"draw {k}: generator against explicit path {d:.2e} (bound {2 * yard[0]:.2e})")
        assert d < 2 * yard[0]
    assert rel(g[0], g[1]) > 0.5                                         # two draws, not one twice
    # weights= is installed for the run and what the model held is put back
    w = po.identity_weights(pm.osize).reshape(pm.oshape)
    yn = np.where(w > 0, y, np.nan)
    rw = pm.sample_posterior(yn, seed=SEED, weights=w, **kw)
    assert pm.data_weights is None and np.all(np.isfinite(rw.mean)) and np.all(np.isfinite(rw.var))
    assert np.array_equal(rw.x_map, pm.cg(yn, mu=mu, mu_reg=mur, max_iter=5, weights=w)[0]) and not np.array_equal(rw.x_map, a.x_map)
    held = np.full(pm.oshape, 2.0)
    pm.set_data_weights(held)
    try:
        pm.sample_posterior(yn, seed=SEED, weights=w, **kw)
        assert np.array_equal(np.asarray(pm.data_weights).reshape(pm.oshape), held.astype(np.float32))
    finally:
        pm.set_data_weights(None)
    # mu_reg = 0: no prior noise is drawn or read
    r0 = pm.sample_posterior(y, mu=mu, mu_reg=0.0, n_samples=2, max_iter=3, perturbations=(_explicit(hp.L, hp.N, hp.N, ops[0].osize, 2, 3)[0], None, None))
    assert np.all(np.isfinite(r0.var))


def test_improper_plane_reports_infinite_std(pm, shared):
    """A plane whose weights are all zero, under mu_reg = 0, draws nothing: rr_first exactly 0, std = +inf; the others are finite."""
    ops, y, x0, mu, mur, _ = shared
    w = np.ones(pm.oshape)
    w[1] = 0.0
    r = pm.sample_posterior(np.where(w > 0, y, np.nan), mu=mu, mu_reg=0.0, n_samples=3, seed=SEED, max_iter=4, weights=w)
    print("rr_first per plane:", r.rr_first)
    assert r.rr_first[1] == 0.0 and r.rr_last[1] == 0.0 and np.all(r.rr_first[[0, 2, 3, 4]] > 0)
    assert np.all(np.isposinf(r.std[1])) and np.all(np.isposinf(r.var[1])) and np.all(np.isfinite(r.std[[0, 2, 3, 4]]))
    assert not r.x_map[1].any() and np.array_equal(r.mean[1], r.x_map[1])
    # with a prior the same plane is proper: the prior's noise alone
    r = pm.sample_posterior(np.where(w > 0, y, np.nan), mu=mu, mu_reg=mur, n_samples=3, seed=SEED, max_iter=4, weights=w)
    assert r.rr_first[1] > 0 and np.all(np.isfinite(r.std)) and np.all(r.std[1] > 0)


def test_generator_path_allocates_no_noise_buffers(shared):
    """The allocator's counters: beside what ``cg`` holds, a run on the generator allocates three buffers (eta, x_map, the float64
    sums) and none of the staging vectors; explicit draws then bring their three (eps_y, eps_r, eps_c), once."""
    ops, y, x0, mu, mur, _ = shared
    start = counts()[0]
    m = _plane_model(hp.sotf(), hp.N, hp.N)
    try:
        kw = dict(mu=mu, mu_reg=mur, n_samples=2, max_iter=2)
        m.cg(y, mu=mu, mu_reg=mur, max_iter=2)
        l0, t0 = counts()
        m.sample_posterior(y, seed=1, **kw)
        l1, t1 = counts()
        assert (l1 - l0, t1 - t0) == (3, 3)
        m.sample_posterior(y, seed=2, **kw)
        assert counts() == (l1, t1)
        pert = _explicit(hp.L, hp.N, hp.N, ops[0].osize, 2, 5)
        m.sample_posterior(y, perturbations=(pert[0], None, None), **{**kw, "mu_reg": 0.0})
        l2, t2 = counts()
        assert (l2 - l1, t2 - t1) == (1, 1)                              # eps_y alone
        m.sample_posterior(y, perturbations=pert, **kw)
        l3, t3 = counts()
        assert (l3 - l2, t3 - t2) == (2, 2)                              # eps_r and eps_c, together
        m.sample_posterior(y, perturbations=pert, **kw)
        m.sample_posterior(y, seed=3, **kw)
        assert counts() == (l3, t3)
    finally:
        m.close()
    assert counts()[0] == start                                          # closing returns everything


# ---- 6. refusals at the library ---------------------------------------------------------------------------------------------------------
def _raw_sample(m, y, mu=1.0, mu_reg=1.0, K=2, max_iter=2, want_var=True):
    """surfh_cg_planes_sample itself, past the Python checks."""
    y = _lib.f32_vec(y, m.osize, "data")
    n = m.isize
    x_map, mean, var = np.empty(n, np.float32), np.empty(n), np.empty(n)
    gn, nit = np.zeros((max(max_iter, 0) + 1) * max(getattr(m, "n_planes", 1), 1)), C.c_int32()
    return m._L.surfh_cg_planes_sample(m._plan, _lib.fptr(y), float(mu), float(mu_reg), None, int(max_iter), 1e-12, 50, int(K), _lib.seed64(0),
                                       None, None, None, _lib.fptr(x_map), _lib.dptr(mean), _lib.dptr(var) if want_var else None,
                                       _lib.dptr(gn), C.byref(nit), None, None, _lib.SAMPLE_CALLBACK(), None)


def test_library_refusals(pm):
    from surfh_amd import imager
    from surfh_amd.imager import ImagerModel
    import problems
    y = np.zeros(pm.osize)
    for kw, word in ((dict(mu=0.0), "mu ="), (dict(mu=-1.0), "mu ="), (dict(mu=float("nan")), "mu ="), (dict(mu=float("inf")), "mu ="),
                     (dict(mu_reg=-1.0), "mu_reg ="), (dict(mu_reg=float("nan")), "mu_reg ="), (dict(K=0), "n_samples"), (dict(K=1), "n_samples"),
                     (dict(max_iter=-1), "max_iter")):
        with pytest.raises(RuntimeError, match=word):
            _lib.check(_raw_sample(pm, y, **kw))
    assert _raw_sample(pm, y, K=1, want_var=False) == 0                  # one sample is enough for a mean
    with pytest.raises(RuntimeError, match="mu ="):
        posterior.po_planes_rhs(pm, y, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="sample ="):
        posterior.po_planes_rhs(pm, y, 1.0, 1.0, sample=-1)
    cfg = problems.config1()
    mt = build_model(cfg)                                                # a plan with templates
    try:
        yt = np.zeros(mt.osize)
        with pytest.raises(RuntimeError, match="templates"):
            _lib.check(_raw_sample(mt, yt))
        with pytest.raises(RuntimeError, match="templates"):
            posterior.po_planes_rhs(mt, yt, 1.0, 1.0)
        im = ImagerModel(mt, imager.synthetic_filters(cfg["wavel"], 3), decim=3)
        mt.set_imager(im)
        try:
            mt.set_imager_data(np.zeros(im.osize), 0.5)
            with pytest.raises(RuntimeError, match="imager"):
                _lib.check(_raw_sample(mt, yt))
        finally:
            mt.set_imager(None)
    finally:
        mt.close()
    x, gn, n = pm.cg(y + 1.0, mu=1.0, mu_reg=1.0, max_iter=2)            # the model is as it was
    assert n == 2 and np.all(np.isfinite(x))


# ---- 7. the driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_writes_the_error_bar(tmp_path):
    """-np 192: the band-1C field of view of the driver's problem does not fit a smaller image (test_gpu_huber_planes)."""
    sp = importlib.util.spec_from_file_location("deconvolution_mrs", os.path.join(ROOT, "scripts", "deconvolution_mrs.py"))
    dd = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(dd)
    out = str(tmp_path / "res")
    r = CliRunner().invoke(dd.main, ["-np", "192", "--planes", "2", "-ni", "5", "--samples", "3", "--sample_seed", "7", "--quiet", "--out", out])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = out + "_po_3"
    assert os.path.isdir(d) and not os.path.exists(out)
    x, mean, std, tr = (np.load(os.path.join(d, f)) for f in ("res_x.npy", "res_mean.npy", "res_std.npy", "po_trace.npy"))
    assert x.shape == mean.shape == std.shape == (2, 192, 192) and tr.shape == (2, 2)
    assert np.isfinite(mean).all() and np.isfinite(std).all() and np.all(std > 0) and np.all(tr[0] > 0) and np.all(tr[1] < tr[0])
