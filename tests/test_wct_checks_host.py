"""The checks of tests/test_gpu_wct_paths.py catch plausible faults of the Hessian kernel that a whole-array ``rel`` of ``expsol``
at the usual mu = 0.7 does not.  No GPU: the faults are seeded into the float64 oracle's own Hessian at ``dense_prime`` (planar
arrays, T = 5) and ``h2_T8_LP384`` (300 planes, T = 8) and run through the numpy stand-ins for ``fwadj`` and ``expsol`` of
tests/wct_cases.py; the measures are asserted on both sides of the project's gate TOL = 1e-5.  The reference-only precondition
of the ``expsol`` check and the conditioning the cases are built for are asserted here too."""
import numpy as np
import pytest

import wct_cases as W
from helpers import TOL, local_errs, max_err, rel

MAP_AXES = dict(template=0, alpha=1, beta=2)
HESS_AXES = dict(k_alpha=0, k_beta=1)
SEEDED = ("dense_prime", "h2_T8_LP384")


def worst(e):
    return max(v for k, v in e.items() if not k.endswith("_at"))


def hessian_check(hth, ref):
    """Check 1: the worst local measure over the (t, u) blocks, and whether the array is mirrored bit for bit."""
    T = ref.shape[0]
    w = max(worst(local_errs(hth[t, u], ref[t, u], HESS_AXES)) for t in range(T) for u in range(T))
    return w, bool(np.array_equal(hth, hth.transpose(1, 0, 2, 3)))


def faults(c):
    """name -> the oracle's Hessian with one fault of the kernel seeded."""
    T, L = c.specs.shape
    hb = c.shape[1] // 2 + 1
    out = {}
    out["imaginary_part_dropped"] = W.hessian(c.specs, c.wo.otf.real)            # as a wrong planar offset would do
    if L > 256:
        out["planes_from_256_left_out"] = W.hessian(c.specs[:, :256], c.wo.otf[:256])    # no second stride of the l loop
    h = c.hth.copy()
    h[T - 1, 0] = 0.0                                                             # one (t, u) entry not mirrored
    out["entry_not_mirrored"] = h
    h = c.hth.copy()
    h[:, :, :, hb - 1] = h[:, :, :, hb - 2]                                       # the last k_beta column holds its neighbour's values
    out["k_beta_column_shifted"] = h
    return out


@pytest.mark.parametrize("name", list(W.CASES))
def test_reference_alone(name):
    """What the GPU tests take for granted: the restated solve is the oracle's, fp32 inputs alone stay a factor 10 under the gate
    for every mu, and mu = 1e-3 gives systems on which the Hessian decides while mu = 0.7 does not."""
    c = W.case(name)
    reg = c.reg()
    for mu in (0.7, W.MU_SMALL, "list"):
        assert max_err(c.solve(mu), c.expsol(mu)) < 1e-13
        pre = c.precondition(mu)
        print(name, "mu", mu, f"fp32 inputs move the solve by {pre:.1e}")
        assert pre < TOL / 10, (name, mu, pre)
    if name in W.JOINT:
        assert c.precondition(0.7, "joint") < TOL / 10
    for kind in c.x:
        assert max_err(W.apply_hessian(c.hth, c.x[kind], c.shape), c.fwadj(kind)) < 1e-13
    med7, _ = c.condition(0.7)
    med3, max3 = c.condition(W.MU_SMALL)
    print(name, f"condition numbers: median {med7:.2f} at mu = 0.7; median {med3:.2f}, max {max3:.1e} at mu = 1e-3")
    assert med7 < 1.02
    assert reg[0, 0] < 1e-20                                   # the prior is blind to the mean: mu cannot mend a singular Hessian there
    if c.T > 1:
        assert max3 > 100
    tiles = W.otf_tiles(c.wo.otf)
    assert (0 < tiles[0] < tiles[1]) if c.lists else tiles[0] == tiles[1], tiles


@pytest.mark.parametrize("T8", [False, True])
@pytest.mark.parametrize("name", W.SINGULAR)
def test_singular_spectra_need_a_ridge(name, T8):
    """With linearly dependent spectra the zero frequency is singular whatever mu is (|D(0)|^2 = 0), so fp32 inputs move the
    float64 solve without bound; with |D(f)|^2 + 10 the precondition holds."""
    c = W.Case(name, specs=W.two_equal, T=8) if T8 else W.Case(name, specs=W.sum_of_first_two)
    assert np.linalg.cond(c.hth[:, :, 0, 0]) > 1e12
    pre = c.precondition(0.7, ridge=W.RIDGE)
    print(name, c.T, f"with the ridge fp32 inputs move the solve by {pre:.1e}, condition number up to {c.condition(0.7, W.RIDGE)[1]:.1e}")
    assert pre < TOL / 10


@pytest.mark.parametrize("name", SEEDED)
def test_seeded_hessian_faults(name):
    """Worst local measure of every check on the faulty Hessian, computed here (bound 1e-5):

                                                 check 1   check 2 (uniform, zero mean)   check 3 (mu = 1e-3, mu = 0.7; its rel)
        dense_prime  imaginary part dropped      2.1e-03   1.7e-04  1.7e-03               2.4e-01  3.9e-04  1.5e-04
        dense_prime  entry not mirrored          1.0e+00   7.2e-02  1.1e-01               4.0e+00  2.6e-01  7.6e-02
        dense_prime  k_beta column shifted       1.3e-04   5.0e-07  1.2e-05               8.2e-04  1.2e-08  4.3e-09
        h2_T8_LP384  imaginary part dropped      2.4e-03   1.9e-04  1.9e-03               2.6e-01  8.9e-04  2.2e-04
        h2_T8_LP384  planes from 256 left out    9.7e-01   6.2e-01  5.5e-01               5.6e+02  6.0e+02  2.2e+02
        h2_T8_LP384  entry not mirrored          1.0e+00   6.7e-02  1.2e-01               6.0e+00  4.3e-01  7.9e-02
        h2_T8_LP384  k_beta column shifted       1.8e-04   6.0e-07  1.4e-05               1.7e-03  3.4e-08  1.3e-08

    Check 1 and the mu = 1e-3 run see every fault, by a factor 10 at least.  The shifted column lies where the OTF is small and
    the prior large: ``expsol`` at mu = 0.7 passes it by three decades on every measure, and ``fwadj`` of the uniform maps passes
    it too -- that is why the Hessian is read out and why the solve is run where the Hessian decides."""
    c = W.case(name)
    reg = c.reg()
    ok1, sym = hessian_check(c.hth, c.hth)
    assert ok1 == 0.0 and sym
    for fault, h in faults(c).items():
        c1, mirrored = hessian_check(h, c.hth)
        c2 = {k: worst(local_errs(W.apply_hessian(h, c.x[k], c.shape), c.fwadj(k), MAP_AXES)) for k in c.x}
        c3 = {mu: worst(local_errs(W.solve_hessian(h, c.rhs, mu, reg, c.shape), c.expsol(mu), MAP_AXES)) for mu in (W.MU_SMALL, 0.7)}
        r07 = rel(W.solve_hessian(h, c.rhs, 0.7, reg, c.shape), c.expsol(0.7))
        print(f"{name:12s} {fault:26s} check 1 {c1:.1e}  check 2 {c2['uniform']:.1e} (uniform) {c2['zero_mean']:.1e} (zero mean)  "
              f"check 3 {c3[W.MU_SMALL]:.1e} (mu = 1e-3) {c3[0.7]:.1e} (mu = 0.7; rel {r07:.1e})")
        assert c1 > 10 * TOL and c3[W.MU_SMALL] > 10 * TOL, (fault, c1, c3)
        assert mirrored == (fault != "entry_not_mirrored")
        if fault == "k_beta_column_shifted":
            assert c3[0.7] < TOL / 100 and r07 < TOL / 100 and c2["uniform"] < TOL, (c3, r07, c2)
        else:
            assert c2["uniform"] > 10 * TOL and c2["zero_mean"] > 10 * TOL, (fault, c2)
