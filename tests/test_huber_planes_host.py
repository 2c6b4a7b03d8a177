"""Host checks of the plane-wise Huber solver's float64 restatement (tests/huber_planes_oracle.py), of the preconditions the device
comparison of tests/test_gpu_huber_planes.py rests on, and of the argument rules of the Python layer.  No GPU, no library."""
import numpy as np
import pytest

import huber_oracle as ho
import huber_planes_oracle as hp
from helpers import rel
from oracle import surfh_oracle as orc


def test_oracle_gradient_descent_and_quadratic_limit():
    _, x0, y = hp.problem()
    l = 0
    op = hp.plane_op(l)
    # the gradient the solver uses is the gradient of J_l: central differences along random directions.  phi is C1 with a jump
    # of phi'' at |u| = delta: the differences that cross it within the step add an error of order h^2 times their number
    # (2e-6 relative at h = 1e-5 here, 2e-8 at h = 1e-6), the float64 rounding of J / h is 2e-9: h = 1e-6, bound 1e-6
    b = hp.MU * op.adjoint(y[l])
    x = x0[l][None]
    g = ho.gradient(op, b, x, hp.MU, hp.MUR, hp.DELTA)
    rng = np.random.default_rng(0)
    for _ in range(3):
        v = rng.standard_normal(x.shape)
        h = 1e-6
        fd = (ho.crit(op, y[l], x + h * v, hp.MU, hp.MUR, hp.DELTA) - ho.crit(op, y[l], x - h * v, hp.MU, hp.MUR, hp.DELTA)) / (2 * h)
        assert abs(fd - np.sum(g * v)) < 1e-6 * abs(fd)
    # MM: the criterion never increases, plane by plane
    for l, ref in hp.reference().items():
        c = np.array(ref["crit"])
        assert ref["nit"] == hp.NIT and np.all(np.diff(c) <= 0) and c[-1] < 0.5 * c[0], l
    # delta = inf is orc.mmmg on the same plane: every array the two form is the same, bit for bit, except the 2 x 2 matrix B,
    # which NumPy sums in another order for (v * 1).T @ v (a general product) than for v.T @ v (a symmetric rank-k update).  So
    # the first iterate, whose memory column is zero, is equal bit for bit; the later ones to float64 rounding (5e-15 measured
    # after 8 iterations; 1e-12 is the bound tests/test_huber_host.py holds the same pair of solvers to).
    l = 0
    inf = hp.solve_plane(l, y[l], x0[l], float("inf"), max_iter=1)
    quad = orc.mmmg(op, y[l], hp.MU, hp.MUR, x0[l][None], max_iter=1)
    assert np.array_equal(inf["x"], quad["x"][0]) and inf["grad_norm"] == quad["grad_norm"]
    inf = hp.solve_plane(l, y[l], x0[l], float("inf"))
    quad = orc.mmmg(op, y[l], hp.MU, hp.MUR, x0[l][None], max_iter=hp.NIT)
    assert np.max(np.abs(inf["x"] - quad["x"][0])) <= 1e-12 * np.max(np.abs(quad["x"]))
    assert np.allclose(inf["grad_norm"], quad["grad_norm"], rtol=1e-12, atol=0)


def test_preconditions_of_the_device_comparison():
    """Measured on the oracle's final iterates (delta = 0.025, mu_reg = 1.5, 8 iterations): the share of differences beyond delta
    is 50.8 %, 50.2 % and 49.3 % in planes 0, 1 and 4 and 0 in plane 2; the Huber iterate is 0.186, 0.190 and 0.187 away from the
    delta = inf iterate (relative l2) in planes 0, 1 and 4."""
    _, x0, y = hp.problem()
    ref = hp.reference()
    share = {l: hp.share_beyond(r["x"], hp.DELTA) for l, r in ref.items()}
    print("share of |D x| beyond delta per plane:", share)
    assert any(0.2 <= s <= 0.8 for s in share.values())
    assert share[hp.QUIET] == 0.0                                              # a fully quadratic plane
    assert not y[hp.EMPTY].any() and not x0[hp.EMPTY].any()                  # the plane that must stay at rest
    for l in hp.COMPARED:
        if share[l] > 0:
            away = rel(ref[l]["x"], hp.solve_plane(l, y[l], x0[l], float("inf"))["x"])
            print(f"plane {l}: Huber iterate {away:.3f} away from the quadratic one; comparison tolerance {hp.TOL_X:.1e}")
            assert away > 100 * hp.TOL_X
    # the masked problem of the weights test: masking changes the answer by more than the comparison tolerance
    mask = hp.sample_mask(y.shape[1])
    assert 0.1 < 1 - mask.mean() < 0.5
    masked = hp.solve_plane(0, y[0], x0[0], mask=mask)
    assert rel(masked["x"], ref[0]["x"]) > 100 * hp.TOL_X


class _NoModel:
    ishape, osize = (2, 8, 8), 2 * 6

    def __getattr__(self, name):
        raise AssertionError(f"the argument checks must not reach the model ({name})")


def test_argument_rules_without_the_library():
    from surfh_amd.spectro_blind_rectangle import QuadCriterion_MRS_2D
    y = np.zeros(12)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="delta must be positive"):
            QuadCriterion_MRS_2D(1.0, y, _NoModel(), 1.0, delta=bad)
    with pytest.raises(ValueError, match="gradient must be 'separated'"):
        QuadCriterion_MRS_2D(1.0, y, _NoModel(), 1.0, gradient="joint", delta=0.1)
    q = QuadCriterion_MRS_2D(1.0, y, _NoModel(), 1.0, delta=0.1)
    assert q.delta == 0.1 and QuadCriterion_MRS_2D(1.0, y, _NoModel(), 1.0).delta is None
    with pytest.raises(ValueError, match="lcg minimises quadratic criteria only"):
        q.run_method("lcg", 3)
    # the same wording as the fusion criterion's
    from surfh_amd.fusion import QuadCriterion_MRS
    with pytest.raises(ValueError, match="lcg minimises quadratic criteria only"):
        QuadCriterion_MRS(1.0, y, _FusionModel(), 1.0, delta=0.1).run_method("lcg", 3)


class _FusionModel:
    ishape, oshape = (2, 8, 8), (12,)
