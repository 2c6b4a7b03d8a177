"""The transform passes of the fused forward and the adjoint's pass in front of the fused tail run over ``Leff`` planes -- the
owned planes rounded up to 32 -- instead of the plane pitch ``LP`` (owned planes rounded up to 128); ``SURFH_LAMBDA_TRIM=0``
restores ``LP`` (plan_internal.h, dft_h2.h ``Nv``).  On the small spectral-domain-capable problem of the suite (``dist_worker.small_problem(128)``:
128 x 128 maps, two channels) with its wavelength axis cut so that the plan owns

* 33 planes:  Leff  64 < LP 128  -- the only chunk of 128 planes is partial, every k_beta has padding tiles;
* 129 planes: Leff 160 < LP 256  -- one whole chunk and a partial one;
* 128 planes: Leff 128 = LP 128  -- the control with nothing to trim.

(``IFU.wslice`` excludes the last in-range plane of the axis, so an axis of n + 1 planes gives n owned ones.)

Forward and exact adjoint against the float64 oracle at the tolerance of test_gpu_parity.py (1e-5 relative L2), the dot test
with float64-accumulated inner products at < 1e-6 (non-negative vectors: the strict ratio; zero-mean vectors: against the natural
scale |u||Av|, as test_gpu_parity.test_dottest), eight CG iterations with the switch on and off whose r.r traces agree to 1e-6
relative, and the planes >= Leff of the blurred cube and of the adjoint's accumulator exactly zero after a forward and an adjoint.
The trimmed passes drop only tiles whose inputs are exact zeros and whose outputs nobody reads, so beyond what the issue asks the
two settings must give the same bits."""
import os

import numpy as np
import pytest

from helpers import TOL, rel

pytestmark = pytest.mark.gpu

OWNED = (33, 129, 128)
N_PIX = 128


def _problem(owned):
    from dist_worker import small_problem
    from surfh_amd import synth
    prob = dict(small_problem(N_PIX))
    wav = np.linspace(7.40, 7.90, owned + 1)
    prob.update(wavel=wav, templates=synth.templates(len(wav)),
                sotf=synth.ir2fr(synth.gaussian_psf(wav, synth.STEP), (N_PIX, N_PIX)))
    return prob


def _model(prob, trim):
    from surfh_amd.models import spectroSigRLSCT
    old = os.environ.get("SURFH_LAMBDA_TRIM")
    os.environ["SURFH_LAMBDA_TRIM"] = "1" if trim else "0"         # read at plan creation
    try:
        return spectroSigRLSCT(prob["sotf"], prob["templates"], prob["alpha_axis"], prob["beta_axis"], prob["wavel"], prob["ifus"],
                               prob["step_deg"], prob["pointings"])
    finally:
        if old is None:
            os.environ.pop("SURFH_LAMBDA_TRIM")
        else:
            os.environ["SURFH_LAMBDA_TRIM"] = old


@pytest.fixture(scope="module", params=OWNED, ids=[f"{n}_planes" for n in OWNED])
def case(request):
    """The problem, its float64 oracle with one forward and one adjoint (computed once), and the default plan."""
    from dist_worker import OracleBackedModel
    owned = request.param
    prob = _problem(owned)
    om = OracleBackedModel(prob, prob["ifus"], prob["pointings"]).om
    u = np.random.default_rng(1).standard_normal(om.osize)
    ref = dict(fwd=om.forward(prob["maps"]), adj=om.adjoint(u))
    m = _model(prob, True)
    try:
        yield dict(owned=owned, prob=prob, om=om, u=u, ref=ref, m=m)
    finally:
        m.close()


def test_extents(case):
    m, owned = case["m"], case["owned"]
    leff, lp, lown = (int(v) for v in m.debug_buffer("trim")[:3])
    print(f"owned {lown}, Leff {leff}, LP {lp}")
    assert m.spec_supported()                                       # the fused passes are what is trimmed
    assert lown == owned
    assert (leff, lp) == ((owned + 31) // 32 * 32, (owned + 127) // 128 * 128)
    assert (leff < lp) == (owned != 128)


def test_forward_and_adjoint_vs_oracle(case):
    m, prob, ref = case["m"], case["prob"], case["ref"]
    e = dict(fwd=rel(m.forward(prob["maps"]), ref["fwd"]), adj=rel(m.adjoint(case["u"]), ref["adj"]))
    print(f"{case['owned']} planes: {e}")
    assert e["fwd"] < TOL and e["adj"] < TOL, e


def test_dot_test(case):
    m = case["m"]
    rng = np.random.default_rng(11)
    ngaps, pgaps = [], []
    for _ in range(3):
        v, u = rng.standard_normal(m.isize), rng.standard_normal(m.osize)
        av = np.asarray(m.matvec(v), dtype=np.float64)
        l, r = float(np.vdot(np.asarray(m.rmatvec(u), dtype=np.float64), v)), float(np.vdot(u, av))
        ngaps.append(abs(l - r) / (np.linalg.norm(u) * np.linalg.norm(av)))
        v, u = rng.random(m.isize), rng.random(m.osize)            # no cancellation in <u, A v>: the strict ratio
        l, r = float(np.vdot(m.rmatvec(u), v)), float(np.vdot(u, m.matvec(v)))
        pgaps.append(abs(l - r) / abs(r))
    print(f"{case['owned']} planes: dot test, zero-mean (normalised) {ngaps}, non-negative {pgaps}")
    assert max(ngaps) < 1e-6 and max(pgaps) < 1e-6


def test_padding_planes_stay_zero(case):
    m, prob = case["m"], case["prob"]
    leff, lp = (int(v) for v in m.debug_buffer("trim")[:2])
    m.forward(prob["maps"])
    m.adjoint(case["u"])
    cube, acc = m.debug_buffer("blurred"), m.debug_buffer("gcube")      # [beta][alpha][LP]
    assert cube.shape[-1] == lp and acc.shape[-1] == lp
    assert cube[..., :leff].any() and acc[..., :leff].any()
    assert not cube[..., leff:].any() and not acc[..., leff:].any()


def test_cg_with_the_switch_on_and_off(case):
    m, prob = case["m"], case["prob"]
    y = case["ref"]["fwd"] + np.random.default_rng(2).standard_normal(case["ref"]["fwd"].shape) * 1e-2 * np.sqrt(np.mean(case["ref"]["fwd"] ** 2))
    kw = dict(mu=1.0, mu_reg=50.0, x0=None, max_iter=8, tol=0.0)    # the weights the suite solves this problem with
    x1, g1, n1 = m.cg(y, **kw)
    m0 = _model(prob, False)
    try:
        leff0, lp0 = (int(v) for v in m0.debug_buffer("trim")[:2])
        assert leff0 == lp0                                         # the switch restores LP
        x0, g0, n0 = m0.cg(y, **kw)
        same = np.array_equal(np.asarray(m0.forward(prob["maps"])), np.asarray(m.forward(prob["maps"]))) and \
            np.array_equal(np.asarray(m0.adjoint(case["u"])), np.asarray(m.adjoint(case["u"])))
    finally:
        m0.close()
    g1, g0 = np.asarray(g1, dtype=np.float64), np.asarray(g0, dtype=np.float64)
    d = float(np.max(np.abs(g1 - g0) / g0))
    print(f"{case['owned']} planes: r.r on {g1.ravel()}, off {g0.ravel()}, largest relative difference {d:.2e}; same operator bits {same}")
    assert n1 == n0 == 8 and g1.shape == g0.shape == (9,) + g1.shape[1:]
    assert d <= 1e-6
    assert same and np.array_equal(g1, g0) and np.array_equal(x1, x0)
