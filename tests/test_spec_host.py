"""tests/spec_oracle.py without a GPU: the float64 restatement of the solver's Fourier-domain vectors is what it says it is (an
orthonormal change of basis in which the circular first differences are diagonal), the fp32 emulation of the two ways to evaluate
that diagonal separates them at the bound tests/test_gpu_spec_vectors.py holds the device to, and the problems of that file are
well posed (every field of view inside its image) and small enough for the float64 oracle."""
import time

import numpy as np
import pytest

import spec_oracle as so
from oracle import surfh_oracle as orc
from test_gpu_spec_vectors import CASES, PRIOR_TOL, refs

SHAPES = [(6, 8), (7, 9), (8, 7), (7, 6)]          # every parity of both axes


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("shape", SHAPES)
def test_basis_is_orthonormal_and_round_trips(shape):
    Na, Nb = shape
    rng = np.random.default_rng(Na * 16 + Nb)
    x, z = rng.standard_normal((3, Na, Nb)), rng.standard_normal((3, Na, Nb))
    KAP, KBP = so.pads(Na, Nb)
    assert (KAP, KBP) == (64, 64)
    xt, zt = so.to_spec(x), so.to_spec(z)
    assert xt.shape == (3, 2, KAP, KBP)
    assert not xt[~np.broadcast_to(so.valid_mask(Na, Nb, KAP, KBP), xt.shape)].any()
    assert abs(np.sum(xt * zt) - np.sum(x * z)) <= 1e-12 * np.sqrt(np.sum(x * x) * np.sum(z * z))
    assert rel(so.from_spec(xt, Na, Nb), x) <= 1e-12
    # other pitches hold the same bins
    wide = so.to_spec(x, 128, 192)
    assert np.array_equal(wide[:, :, :KAP, :KBP], xt) and not wide[:, :, KAP:].any() and not wide[:, :, :, KBP:].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_first_differences_are_the_diagonal(shape):
    Na, Nb = shape
    d = np.random.default_rng(Na * 16 + Nb + 1).standard_normal((2, Na, Nb))
    ref = so.to_spec(orc.diff_r_t(orc.diff_r(d)) + orc.diff_c_t(orc.diff_c(d)))
    assert rel(so.prior_spec(so.to_spec(d), Na, Nb), ref) <= 1e-12
    eig = so.prior_eig(Na, Nb)
    assert eig.shape == (Na, Nb // 2 + 1) and eig[0, 0] == 0.0
    assert np.allclose(eig, orc.reg_freq((Na, Nb), "separated"), rtol=0, atol=1e-12)


def test_pads():
    assert so.pads(127, 48) == (128, 64) and so.pads(128, 51) == (128, 64) and so.pads(200, 254) == (256, 128)
    assert so.pads(48, 260) == (64, 192) and so.pads(260, 267) == (320, 192) and so.pads(255, 40) == (256, 64)


@pytest.mark.parametrize("N", [127, 255, 501, 512])
def test_fp32_eigenvalue_forms(N):
    """Why the per-bin bound separates the two: 2 - 2 cos(2 pi k / N) in fp32 cancels at low k, 4 sin^2(pi k' / N) with k' folded to
    the lower half of the axis does not."""
    exact = so.axis_eig_exact(N)[1:]
    err = lambda v: np.abs(v[1:].astype(np.float64) - exact) / exact
    e_cos, e_sin = err(so.axis_eig_cos_fp32(N)), err(so.axis_eig_sin_fp32(N))
    print(N, f"cos form at k = 1: {e_cos[0]:.2e}, worst {e_cos.max():.2e}; sin form worst {e_sin.max():.2e}")
    assert e_cos[0] > 1e-5
    assert e_sin.max() < PRIOR_TOL
    assert so.axis_eig_cos_fp32(N)[0] == 0 and so.axis_eig_sin_fp32(N)[0] == 0


def test_sin_form_needs_the_fold():
    """k / N rounded to fp32 near 1 is off by up to 3e-8 of 1, which is 3e-8 N of the distance 1 / N the sine measures there: without
    the fold the top of an axis loses what the cos form loses at the bottom."""
    e = {}
    for N in (251, 501):
        exact = so.axis_eig_exact(N)[1:]
        e[N] = float(np.max(np.abs(so.axis_eig_sin_fp32(N, fold=False)[1:].astype(np.float64) - exact) / exact))
    print("sin form without the fold:", e)
    assert min(e.values()) > 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_problems_are_well_posed(name):
    r = refs(name)
    om, cfg = r.om, r.cfg
    assert om.ishape == (r.T, r.Na, r.Nb)
    for tab in om.channels:
        assert 96 <= cfg["Lc"] <= 128 and 0 <= tab.wslice[0] < tab.wslice[1] <= cfg["Lc"]
        assert 2 <= len(tab.pointings) <= 4
        for p in tab.pointings:
            ga, gb = orc.local2global(tab.local_alpha_axis, tab.local_beta_axis, tab.spec.angle,
                                      (tab.origin_pix[0] + p[0], tab.origin_pix[1] + p[1]))
            assert cfg["alpha_axis"][0] <= ga.min() and ga.max() <= cfg["alpha_axis"][-1]
            assert cfg["beta_axis"][0] <= gb.min() and gb.max() <= cfg["beta_axis"][-1]
    t0 = time.perf_counter()
    y = om.forward(r.maps)
    t1 = time.perf_counter()
    a = om.adjoint(r.y)
    t2 = time.perf_counter()
    print(name, f"oracle forward {t1 - t0:.2f} s, adjoint {t2 - t1:.2f} s, {np.prod(om.cube_shape) / 1e6:.1f} M voxels")
    assert y.shape == (om.osize,) and a.shape == om.ishape and np.isfinite(y).all() and np.isfinite(a).all()
    assert t1 - t0 < 5.0 and t2 - t1 < 5.0
