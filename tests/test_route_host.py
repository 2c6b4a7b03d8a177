"""The route of a plan -- which transform kernels run and which fusions ride on them -- decided on the CPU: surfh_route_decide
calls the function plan creation calls (decide_route, surfh_amd/csrc/plan.hip), so what a shape, a configuration and the eight
switches lead to can be read without building a plan.  tests/test_gpu_op_routes.py holds every built plan to this function.

(a) anchors: the routes the GPU suite has asserted plan by plan (``dims(m, "dft")``, ``spec_supported()``) since before the
    function existed;
(b) every switch flips the fields it names and no other;
(c) invariants over a sweep of shapes, template counts and verification plans."""
import ctypes as C

import pytest

DENSE, H2, CT = 0, 1, 2
NONE, LISTS, LISTS_RANGES = 0, 1, 2
FIELDS = ("ax_a", "ax_b", "mix", "prod", "fused_tail", "support", "tpl_spectral", "spec_calls")
SWITCHES = ("SURFH_DFT_H2", "SURFH_DFT_CT", "SURFH_DFT_DENSE", "SURFH_NO_FUSED_MIX", "SURFH_ADJ_FUSED", "SURFH_OTF_PROD",
            "SURFH_OTF_SUPPORT", "SURFH_OTF_RANGES")
DEFAULTS = 0b11110011


def bit(name):
    return 1 << SWITCHES.index(name)


@pytest.fixture(scope="module")
def decide():
    from surfh_amd import _lib
    L = _lib.load()
    out = (C.c_int64 * 8)()

    def call(na, nb, T, lp=128, verify=0, exact=0, sotf=1, switches=DEFAULTS, scan=LISTS_RANGES):
        _lib.check(L.surfh_route_decide(na, nb, T, lp, verify, exact, sotf, switches, scan, out))
        return dict(zip(FIELDS, (int(v) for v in out)))
    return call


def dft(r):
    """What ``surfh_debug_dims(plan, "dft")`` reports of a route."""
    return (r["ax_a"], r["ax_b"], int(r["ax_a"] != DENSE), r["fused_tail"])


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
def test_anchors(decide):
    mid = decide(128, 128, 4, lp=512)                           # problems.two_channel_mid
    assert dft(mid) == (H2, H2, 1, 1) and mid["spec_calls"] and mid["mix"] and mid["support"] == LISTS_RANGES
    ct300 = decide(300, 300, 4)                                 # dist_worker.small_problem(300)
    assert dft(ct300)[:3] == (CT, CT, 1) and ct300["spec_calls"] and not ct300["fused_tail"]
    assert dft(decide(300, 64, 4)) == (CT, H2, 1, 0)            # mixed_300x64
    c1 = decide(64, 64, 4)                                      # problems.config1
    assert dft(c1) == (H2, H2, 1, 0) and not c1["spec_calls"] and c1["support"] == NONE
    small = decide(127, 48, 4)                                  # test_gpu_spec_vectors.spec_problem("A")
    assert dft(small) == (H2, H2, 1, 1) and small["spec_calls"]
    planar = dict(zip(FIELDS, (DENSE, DENSE, 0, 0, 0, NONE, 0, 0)))
    assert decide(64, 64, 4, switches=DEFAULTS | bit("SURFH_DFT_DENSE")) == planar
    assert decide(64, 64, 4, verify=1) == planar and decide(128, 128, 4, lp=512, verify=1) == planar
    # plane-wise plans (test_gpu_op_routes.py: blurred_96 on dft_h2 with its own product kernels, blurred_300 on the product loader)
    assert dft(decide(96, 96, 0))[:3] == (H2, H2, 1) and not decide(96, 96, 0)["prod"]
    assert dft(decide(300, 300, 0))[:3] == (CT, CT, 1) and decide(300, 300, 0)["prod"]
    with pytest.raises(RuntimeError, match="surfh_route_decide"):
        decide(1, 64, 4)
    with pytest.raises(RuntimeError, match="surfh_route_decide"):
        decide(64, 64, 4, lp=100)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
MID, CT300, PLANES300 = (128, 128, 4, 512), (300, 300, 4, 128), (300, 300, 0, 128)
# (inputs, switch, its non-default value) -> the fields that change, with their new values
FLIPS = [
    (MID, "SURFH_DFT_H2", 0, dict(ax_a=CT, ax_b=CT, fused_tail=0)),                       # 128 = 2 x 64: dft_ct, its lists, no fused tail
    (MID, "SURFH_DFT_CT", 0, {}),                                                         # no axis of this plan is on dft_ct
    (MID, "SURFH_DFT_DENSE", 1, dict(ax_a=DENSE, ax_b=DENSE, mix=0, fused_tail=0, support=NONE, tpl_spectral=0, spec_calls=0)),
    (MID, "SURFH_NO_FUSED_MIX", 1, dict(mix=0, support=NONE, spec_calls=0)),              # the lists serve the mix loader; the tail stays fused
    (MID, "SURFH_ADJ_FUSED", 0, dict(fused_tail=0, support=NONE, spec_calls=0)),          # dft_h2's lists ride on the fused tail
    (MID, "SURFH_OTF_PROD", 0, {}),                                                       # plane-wise plans only
    (MID, "SURFH_OTF_SUPPORT", 0, dict(support=NONE)),
    (MID, "SURFH_OTF_RANGES", 0, dict(support=LISTS)),
    (CT300, "SURFH_DFT_H2", 0, {}),
    (CT300, "SURFH_DFT_CT", 0, dict(ax_a=DENSE, ax_b=DENSE, mix=0, support=NONE, tpl_spectral=0, spec_calls=0)),
    (CT300, "SURFH_DFT_DENSE", 1, dict(ax_a=DENSE, ax_b=DENSE, mix=0, support=NONE, tpl_spectral=0, spec_calls=0)),
    (CT300, "SURFH_NO_FUSED_MIX", 1, dict(mix=0, support=NONE, spec_calls=0)),
    (CT300, "SURFH_ADJ_FUSED", 0, {}),                                                    # dft_h2's tail
    (CT300, "SURFH_OTF_PROD", 0, {}),
    (CT300, "SURFH_OTF_SUPPORT", 0, dict(support=NONE)),
    (CT300, "SURFH_OTF_RANGES", 0, dict(support=NONE)),                                   # dft_ct: the k-ranges with the lists, or neither
    (PLANES300, "SURFH_OTF_PROD", 0, dict(prod=0)),
    (PLANES300, "SURFH_DFT_CT", 0, dict(ax_a=DENSE, ax_b=DENSE, prod=0, tpl_spectral=0)),
]


@pytest.mark.parametrize("inputs,switch,value,changes", FLIPS, ids=[f"{'x'.join(map(str, f[0][:3]))}-{f[1]}={f[2]}" for f in FLIPS])
def test_a_switch_flips_the_fields_it_names_and_no_other(decide, inputs, switch, value, changes):
    na, nb, T, lp = inputs
    base = decide(na, nb, T, lp=lp)
    mask = (DEFAULTS | bit(switch)) if value else (DEFAULTS & ~bit(switch))
    assert mask != DEFAULTS
    # the scan reports ranges only where they were asked for
    got = decide(na, nb, T, lp=lp, switches=mask, scan=LISTS_RANGES if mask & bit("SURFH_OTF_RANGES") else LISTS)
    assert all(base[k] != v for k, v in changes.items()), (base, changes)
    assert got == {**base, **changes}


def test_exact_2_and_a_missing_otf_keep_the_whole_spectrum(decide):
    for na, nb, T, lp in (MID, CT300):
        base = decide(na, nb, T, lp=lp)
        assert base["support"] == LISTS_RANGES
        for kw in (dict(exact=2), dict(exact=3), dict(sotf=0), dict(scan=NONE)):
            assert decide(na, nb, T, lp=lp, **kw) == {**base, "support": NONE}, kw
        assert decide(na, nb, T, lp=lp, exact=1) == base                 # bit 0 concerns the spectral-blur GEMMs


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
SIZES = list(range(2, 131)) + list(range(137, 601, 7))


def check_invariants(r, na, nb, T, verify, exact, mask):
    ilv = r["ax_a"] != DENSE
    assert ilv == (r["ax_b"] != DENSE)                                   # interleaved iff neither axis is DENSE
    if r["fused_tail"]:
        assert r["ax_a"] == r["ax_b"] == H2 and 1 <= T <= 4 and 127 <= na <= 255
    if r["prod"]:
        assert T == 0 and r["ax_a"] == CT
    if r["support"] != NONE:
        assert r["mix"] and not exact & 2
    if r["mix"]:
        assert ilv and 1 <= T <= 4
    if r["spec_calls"]:
        assert r["mix"]
    assert bool(r["tpl_spectral"]) == (ilv and T <= 4)
    if verify or mask & bit("SURFH_DFT_DENSE"):
        assert list(r.values()) == [DENSE, DENSE, 0, 0, 0, NONE, 0, 0]


def test_invariants_over_the_sweep(decide):
    seen = set()
    for T in (0, 1, 4, 5, 8):
        for verify in (0, 1):
            for na in SIZES:
                for nb in SIZES:
                    r = decide(na, nb, T, verify=verify)
                    check_invariants(r, na, nb, T, verify, 0, DEFAULTS)
                    seen.add(tuple(r.values()))
    assert len(seen) > 8, seen                                           # the sweep meets routes of every kind


def test_invariants_under_every_switch(decide):
    for sw in SWITCHES:
        mask = DEFAULTS ^ bit(sw)
        for T in (0, 1, 4, 5, 8):
            for exact in (0, 2):
                for n in SIZES[::3]:
                    for nb in (n, 64, 300):
                        check_invariants(decide(n, nb, T, exact=exact, switches=mask), n, nb, T, 0, exact, mask)
