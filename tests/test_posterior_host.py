"""The float64 restatement of the posterior sampler (tests/posterior_oracle.py): the generator's known answers and moments, the
extra right-hand side of the CG, and the covariance identity of the perturbed right-hand side.  No GPU."""
import numpy as np
import pytest

import posterior_oracle as po
import problems
from oracle import surfh_oracle as orc


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """Philox4x32-10, counter / key -> output (the first two are the Random123 known-answer vectors)."""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        assert _hex(po.philox4x32_10(np.array(ctr, dtype=np.uint64), key)) == want
    both = po.philox4x32_10(np.array([c[0] for c in cases[:1]] * 2, dtype=np.uint64), (0, 0))           # batched counters
    assert _hex(both[1]) == cases[0][2]


def test_stream_is_independent_of_the_cut():
    """A value depends on (seed, stream, sample, element index) alone: any cut of a stream into calls gives the same numbers."""
    seed = (0x1234ABCD << 32) | 0x9E3779B9
    whole = po.randn(5123, seed, 1, 7)
    parts = np.concatenate([po.randn(n, seed, 1, 7, start=s) for s, n in ((0, 1), (1, 3), (4, 1), (5, 1018), (1023, 4100))])
    assert np.array_equal(whole, parts)
    for other in (po.randn(64, seed, 2, 7), po.randn(64, seed, 1, 6), po.randn(64, seed + (1 << 32), 1, 7), po.randn(64, seed + 1, 1, 7)):
        assert not np.any(other == whole[:64])                       # stream, sample and both key words all matter


def test_normal_moments():
    """2^20 normals of seed 0 at distribution bounds (5 standard errors of each statistic under N(0, 1)), not measurements."""
    n = 1 << 20
    z = po.randn(n, 0, 0, 0)
    mean, var = float(np.mean(z)), float(np.var(z))
    kurt = float(np.mean((z - mean) ** 4) / var ** 2 - 3.0)
    print(f"mean {mean:+.2e} (bound {5 / np.sqrt(n):.2e}), var - 1 {var - 1:+.2e} ({5 * np.sqrt(2 / n):.2e}), "
          f"excess kurtosis {kurt:+.2e} ({5 * np.sqrt(24 / n):.2e}), max |z| {np.max(np.abs(z)):.3f}")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(kurt) < 5 * np.sqrt(24 / n)
    assert np.max(np.abs(z)) <= po.ZMAX
    pairs = z.reshape(-1, 4)                                           # the two values of a Box-Muller pair, and the two pairs
    for a, b in ((0, 1), (0, 2), (1, 3)):
        assert abs(np.mean(pairs[:, a] * pairs[:, b])) < 5 / np.sqrt(n / 4)


@pytest.fixture(scope="module")
def c1():
    cfg = problems.config1()
    return cfg, problems.oracle_model(cfg, box="direct")


def test_lcg_with_zero_extra_is_orc_lcg(c1):
    cfg, om = c1
    y = om.forward(cfg["maps"])
    ref = orc.lcg(om, y, 1.0, 5e3, np.zeros(om.ishape), max_iter=4)
    for extra in (None, np.zeros(om.ishape)):
        got = po.lcg(om, y, 1.0, 5e3, np.zeros(om.ishape), extra, max_iter=4)
        assert np.array_equal(got["x"], ref["x"]) and got["grad_norm"] == ref["grad_norm"] and got["nit"] == ref["nit"]
    e = np.random.default_rng(0).standard_normal(om.ishape)
    moved = po.lcg(om, y, 1.0, 5e3, np.zeros(om.ishape), e, max_iter=4)
    assert not np.array_equal(moved["x"], ref["x"])


def test_transposed_differences_are_the_oracles(c1):
    """eta's stencils: <D^T e, v> = <e, D v> for the circular differences of the prior."""
    cfg, om = c1
    rng = np.random.default_rng(2)
    e, v = rng.standard_normal((3, 7, 9)), rng.standard_normal((3, 7, 9))
    assert abs(np.vdot(orc.diff_r_t(e), v) - np.vdot(e, orc.diff_r(v))) < 1e-12
    assert abs(np.vdot(orc.diff_c_t(e), v) - np.vdot(e, orc.diff_c(v))) < 1e-12
    assert np.array_equal(orc.diff_r_t(e), np.roll(e, -1, axis=1) - e) and np.array_equal(orc.diff_c_t(e), np.roll(e, -1, axis=2) - e)


def test_covariance_identity(c1):
    """v^T b~ over 400 draws has mean v^T b (5 standard errors) and variance v^T Q v (+- 5 sqrt(2 / 399) = +- 0.354) for
    each probe.  The all-ones probe is pure data term and the checkerboard pure prior, so mu against sqrt(mu) (a factor 4 in
    the variance ... or 1/4) and mu_reg against sqrt(mu_reg) (9) are each pinned.  v^T b~ = mu (A v)^T W y~ + v^T eta needs A v
    once per probe instead of an adjoint per draw; two draws check that against ``rhs`` itself."""
    cfg, om = c1
    mu, mu_reg, draws, seed = (po.IDENTITY[k] for k in ("mu", "mu_reg", "draws", "seed"))
    w = po.identity_weights(om.osize)
    assert 0.03 < np.mean(w == 0) < 0.07
    y = po.identity_data(om, cfg["maps"], w, mu)                        # NaN where w = 0: weight 0 takes the sample out
    V = po.probes(om.ishape)
    AV = {k: om.forward(v) for k, v in V.items()}
    proj = {k: np.empty(draws) for k in V}
    for d in range(draws):
        eps = po.draw(om, seed, d)
        wy = np.where(w > 0, w * np.where(w > 0, po.perturb_data(y, w, eps[0], mu), 0.0), 0.0)
        e = po.eta(eps[1], eps[2], mu_reg)
        for k, v in V.items():
            proj[k][d] = mu * np.vdot(AV[k], wy) + np.vdot(v, e)
        if d < 2:
            bt = po.rhs(om, y, w, mu, mu_reg, eps)
            assert np.all(np.isfinite(bt))
            for k, v in V.items():
                assert abs(np.vdot(v, bt) - proj[k][d]) < 1e-8 * np.linalg.norm(v) * np.linalg.norm(bt)      # the oracle's dot-test gap
    b = mu * om.adjoint(np.where(w > 0, w * np.where(w > 0, y, 0.0), 0.0))
    shares = {}
    for k, v in V.items():
        qd, qp = po.quad_parts(v, AV[k], w, mu, mu_reg)
        shares[k] = qp / (qd + qp)
        po.identity_check(k, proj[k], float(np.vdot(v, b)), qd + qp, draws)
    print("prior share of v^T Q v:", {k: round(s, 3) for k, s in shares.items()})
    assert shares["ones"] < 1e-3 and shares["checker"] > 0.999
