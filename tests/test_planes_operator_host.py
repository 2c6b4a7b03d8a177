"""The teeth of tests/planes_operator_cases.py, without a GPU.  The folded form of the plane-wise normal operator -- what the
device-resident CG computes on its fused routes, q = irfft2(mu conj(H) rfft2(g) + mu_reg |D|^2 rfft2(v)) with g the adjoint's
accumulated cube and |D|^2 = 4 sin^2(pi k / N) per axis -- is restated in float64 with switchable faults, each the kind of error a
fused kernel can make on one branch only:

  nyquist   the prior of the Nyquist column (k_beta = Nb / 2) dropped
  add_w     the product loader's prior weight not divided by mu: q = mu (A^T W A v + mu_reg D^T D v)
  mu_skip   mu applied only where the prior weight is non-zero in fp32 (a defect the device code had: surfh_amd/csrc/plan_solvers.hip,
            pn_normal)
  lane      the prior taken from the plane in the neighbouring lane (l ^ 1)
  tile      the planes of the last 128-wavelength super-tile not written

Without a fault the restatement agrees with the direct reference (``planes_operator_cases.reference``) to 1e-12 on every per-plane
measure, at even and odd shapes; every fault exceeds TOL on a per-plane measure of a listed case; and the whole-array ``rel`` --
what the plane-wise tests held the operator to -- passes some of them (RECORDED, computed here)."""
import ctypes as C

import numpy as np
import pytest

import planes_operator_cases as oc
from helpers import TOL, rel
from oracle import surfh_oracle as orc

FAULTS = ("nyquist", "add_w", "mu_skip", "lane", "tile")
CASES = [(name, Lc, w, mu, mur) for name, Lc in (("h2_even", 3), ("h2_even", 130), ("h2_odd", 3)) for w in oc.WEIGHTS for mu, mur in oc.PAIRS]


def dsq(n, k):
    return 4.0 * np.sin(np.pi * np.asarray(k) / n) ** 2


_cube = {}


def accumulated(name, Lc, weights):
    """g: the adjoint's cube before its OTF product, from the checker built on an OTF of ones"""
    key = (name, Lc, weights)
    if key not in _cube:
        c = oc.problem(name, Lc)
        bo = oc.oracle(name, Lc)
        ones = orc.BlurredOracle(np.ones_like(c["sotf"]), c["alpha_axis"], c["beta_axis"], c["spec"], c["step_deg"], c["pointings"])
        y = bo.forward(np.asarray(oc.vector(name, Lc)[0], dtype=np.float64))
        if weights == "weighted":
            y = y * np.asarray(oc.data_weights(name, Lc), dtype=np.float64)
        _cube[key] = ones.adjoint(y)
    return _cube[key]


def folded(name, Lc, weights, mu, mu_reg, fault=None):
    c = oc.problem(name, Lc)
    Na, Nb = c["imshape"]
    v = np.asarray(oc.vector(name, Lc)[0], dtype=np.float64)
    G, V, H = orc.dft(accumulated(name, Lc, weights)), orc.dft(v), c["sotf"]
    d2 = dsq(Na, np.arange(Na))[:, None] + dsq(Nb, np.arange(Nb // 2 + 1))[None, :]
    if fault == "nyquist" and Nb % 2 == 0:
        d2[:, Nb // 2] = 0.0
    if fault == "lane":
        V = np.stack([V[l ^ 1] if (l ^ 1) < Lc else np.zeros_like(V[0]) for l in range(Lc)])
    data, prior = np.conj(H) * G, d2[None] * V
    if fault == "add_w":
        spec = mu * (data + mu_reg * prior)
    elif fault == "mu_skip" and np.float32(mu_reg) == 0:
        spec = data + mu_reg * prior
    else:
        spec = mu * data + mu_reg * prior
    q = orc.idft(spec, (Na, Nb))
    if fault == "tile":
        q[128 * ((Lc - 1) // 128):] = 0.0
    return q


def local_worst(q, ref):
    """the worst per-plane measure; infinite where the all-zero plane did not come back zero"""
    return max(v for v, _, _ in oc.worst(oc.plane_errs(q, ref)).values())


@pytest.mark.parametrize("name,Lc", [("h2_even", 3), ("h2_odd", 3), ("h2_even", 130)])
def test_the_folded_form_is_the_operator(name, Lc):
    for w in oc.WEIGHTS:
        for mu, mur in oc.PAIRS:
            ref = oc.reference(name, Lc, False, w, mu, mur)
            e = oc.check_planes(folded(name, Lc, w, mu, mur), ref, f"{name} Lc {Lc} {w} mu {mu} mu_reg {mur}", tol=1e-12)
            assert not ref[oc.ZERO_PLANE].any() and ref[0].any()
            assert set(e) == set(oc.MEASURES)


# fault -> the listed cases it shows in (a per-plane measure above TOL), and how many of those the whole-array rel passes
# (computed here).  At these sizes rel sees every gross fault, as one figure without a place; it passes the lane fault under
# mu_reg = 1e-50 at Lc = 130, which only the all-zero plane shows: its neighbour's prior makes it 1e-50 times something instead of
# exactly 0 (at Lc = 3 the all-zero plane's neighbour is a padding plane and planes 0 and 1, swapped, lose nothing at 1e-50).
RECORDED = {"nyquist": (16, 0), "add_w": (18, 0), "mu_skip": (12, 0), "lane": (26, 2), "tile": (36, 0)}


def test_every_fault_is_caught_and_rel_misses_some():
    seen = {}
    for fault in FAULTS:
        caught, missed = [], []
        for case in CASES:
            name, Lc, w, mu, mur = case
            ref = oc.reference(name, Lc, False, w, mu, mur)
            if not ref.any():
                continue
            q = folded(name, Lc, w, mu, mur, fault)
            if local_worst(q, ref) > TOL:
                caught.append(case)
                if rel(q, ref) < TOL:
                    missed.append(case)
        print(fault, len(caught), "cases caught;", len(missed), "of them pass the whole-array rel:", missed)
        assert caught, f"{fault}: no listed case shows it"
        seen[fault] = (len(caught), len(missed))
    assert seen == RECORDED
    assert any(m for _, m in seen.values())          # the gap the per-plane measures close


def test_check_planes_names_the_plane_the_measure_and_the_index():
    name, Lc = "h2_odd", 3
    ref = oc.reference(name, Lc, False, "none", 1.3, 0.07)
    a = ref.copy()
    a[1, 40, 17] *= 1.0 + 1e-2
    with pytest.raises(AssertionError, match=r"plane 1: .*max "):
        oc.check_planes(a, ref, "seeded")
    a = ref.copy()
    a[0, 11] *= 1.0 + 1e-3                            # one row of plane 0, whatever the plane's scale beside the others
    with pytest.raises(AssertionError, match=r"plane 0: .*row .* at row 11"):
        oc.check_planes(a, ref, "seeded")
    a = ref.copy()
    a[oc.ZERO_PLANE, 3, 3] = 1e-30                    # the all-zero plane has to stay exactly zero
    with pytest.raises(AssertionError, match=f"plane {oc.ZERO_PLANE}: the reference is zero, 1 elements are not"):
        oc.check_planes(a, ref, "seeded")
    # a faint plane beside bright ones: 1e-3 of it is far below the whole array's gate and 100 times the plane's own
    ref130 = oc.reference("h2_even", 130, False, "none", 1.3, 0.07)
    norms = np.linalg.norm(ref130.reshape(130, -1), axis=1)
    faint = int(np.argmin(np.where(norms > 0, norms, np.inf)))
    a = ref130.copy()
    a[faint] *= 1.0 + 1e-3
    assert rel(a, ref130) < 0.01 * TOL
    with pytest.raises(AssertionError, match=f"plane {faint}: rel "):
        oc.check_planes(a, ref130, "seeded")
    # routes that transform the planes (l, l ^ 1) together get no other bound: over_tol names the planes that miss TOL, pair_bound
    # says how far a plane is from its own gate plus PAIR_LEAK of its partner
    assert oc.paired("h2_ct") and oc.paired("ct_ct") and oc.paired("ct_ct_own_products") and not oc.paired("ct_h2") and not oc.paired("h2_even")
    assert all(oc.PLANES[n] == (3, 4) for n in oc.ROUTES if oc.paired(n)) and oc.ZERO_PLANE ^ 1 == 3
    ref4 = oc.reference("h2_ct", 4, False, "none", 1.3, 0.07)
    peak = np.max(np.abs(ref4.reshape(4, -1)), axis=1)
    faint, bright = (0, 1) if peak[0] < peak[1] else (1, 0)
    a = ref4.copy()
    a[faint] += 1e-7 * ref4[bright]                    # the separation's residue: above TOL of the faint plane, inside the pair's bound
    a[oc.ZERO_PLANE] = 1e-7 * ref4[3]
    over, _ = oc.over_tol(a, ref4)
    assert set(over) == ({oc.ZERO_PLANE, faint} if peak[bright] > 150 * peak[faint] else {oc.ZERO_PLANE}) and "reference is zero" in over[oc.ZERO_PLANE]
    assert oc.pair_bound(a, ref4)[0] < 1.0
    a[oc.ZERO_PLANE] = 1e-6 * ref4[3]                  # ten times that: no longer what the pairing explains
    assert oc.pair_bound(a, ref4) == (pytest.approx(1e-6 / oc.PAIR_LEAK), oc.ZERO_PLANE)
    a = ref.copy()
    a[1, 5, 5] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        oc.check_planes(a, ref, "seeded")


def test_the_routes_the_cases_name_are_the_ones_plan_creation_decides():
    from surfh_amd import _lib
    L = _lib.load()
    out = (C.c_int64 * 8)()
    for name, (shape, env, want) in oc.ROUTES.items():
        for Lc in oc.PLANES[name]:
            for scan in (0, 1, 2):                   # a plan without templates scans nothing: the outcome must not matter
                _lib.check(L.surfh_route_decide(shape[0], shape[1], 0, oc.pitch(Lc), 0, 0, 1, oc.switch_mask(env), scan, out))
                assert (out[0], out[1], out[3]) == want, (name, Lc, list(out))
                assert out[2] == 0 and out[4] == 0       # no mix loader, no fused tail without templates
    assert {r[2] for r in oc.ROUTES.values()} >= {(oc.H2, oc.H2, 0), (oc.H2, oc.CT, 0), (oc.CT, oc.H2, 1), (oc.CT, oc.CT, 1), (oc.DENSE, oc.DENSE, 0),
                                                   (oc.CT, oc.CT, 0)}
