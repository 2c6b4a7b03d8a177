"""The imager operator on the device bin by bin and at its edge shapes (tests/imager_cases.py; its teeth:
tests/test_imager_cases_host.py): G against float64 inside the derived ``g_bound`` with exact zeros in the padding bins; forward,
adjoint and both fwadj element by element (``helpers.local_errs``, every measure at the project's TOL) on broadband OTFs; the
identities that hold bit for bit whatever the shape; the transform temporary the imager shares with the plan's own operator,
through F > T, F = 16, F = 1 after it and the detach; and one joint solve with more filters than templates.  Every measured value
goes to the parity log.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import imager_cases as ic
import imager_oracle as io
import problems
import weights_oracle as wo
from helpers import TOL, build_model, local_errs, rel
from oracle import surfh_oracle as orc
from surfh_amd import _lib, imager
from surfh_amd.imager import ImagerModel
from test_gpu_imager import CG_GRADNORM_TOL, CG_ITERATE_TOL, MU, MU_IM, MUR, NIT, _gap, _max_rel, _set_data
from test_gpu_parity import note

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("name,i", ic.CASES, ids=ic.IDS)
_plans = {}


def dims(m, which):
    d = (C.c_int64 * 4)()
    assert m._L.surfh_debug_dims(m._plan, which.encode(), d) == 0
    return tuple(int(v) for v in d)


def make_plan(name):
    from surfh_amd.mixing import Model_WCT
    p = ic.plan(name)
    m = Model_WCT(p["psf"], p["tpl"], p["shape"], p["pce"])
    assert dims(m, "dft")[:2] == p["axes"], (name, dims(m, "dft"))          # the route the case names is the one the plan holds
    return m


def plan(name):
    """One plan per name for the whole module"""
    if name not in _plans:
        _plans[name] = make_plan(name)
    return _plans[name]


@pytest.fixture(scope="module", autouse=True)
def close_plans():
    yield
    for m in _plans.values():
        m.close()
    _plans.clear()


def attach(m, name, i):
    c = ic.case(name, i)
    dev = ImagerModel(m, c["filters"], decim=c["d"])
    if c["own"] is not None:
        dev.sotf = np.ascontiguousarray(c["own"], dtype=np.complex128)
    dev.attach()
    assert dev.oshape == c["im"].oshape and m._L.surfh_imager_osize(m._plan) == c["im"].osize
    return dev, c


def detach(m):
    _lib.check(m._L.surfh_set_imager(m._plan, None))
    m._imager = None
    assert m._L.surfh_imager_osize(m._plan) == 0


def no_data(m):
    _lib.check(m._L.surfh_set_imager_data(m._plan, None, None, 0.0))


def device_g(m):
    """The plan's G [(f, t)][2][KAP][KBP]"""
    shape = dims(m, "imager_g")
    out = np.empty(int(np.prod(shape)), dtype=np.float32)
    assert m._L.surfh_debug_copy(m._plan, b"imager_g", _lib.fptr(out), out.size) == out.size
    return out.reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def where_differ(a, b):
    k = np.argwhere(bits(a) != bits(b))
    return f"{len(k)} elements differ, the first at {k[:4].tolist()}"


# ---- 1. G bin by bin -------------------------------------------------------------------------------------------------------------------
def check_g(m, name, i, tag=""):
    c = ic.case(name, i)
    (Na, Nb), nkb = c["imshape"], c["imshape"][1] // 2 + 1
    g = device_g(m)
    assert g.shape[:2] == (c["F"] * c["T"], 2) and g.shape[2] >= Na and g.shape[3] >= nkb
    assert not g[:, :, Na:, :].any() and not g[:, :, :, nkb:].any(), "padding bins of G are not zero"
    worst, at = ic.g_excess(g[:, :, :Na, :nkb], name, i)
    note("imager_edges_g", case=c["id"] + tag, worst_over_bound=worst, pair=at[0], part=at[1], k_alpha=at[2], k_beta=at[3])
    print(f"{c['id']}{tag}: G at {worst:.3f} of its bound, component {at}")
    assert worst <= 1.0, f"{c['id']}: |g - G| is {worst:.3g} times its bound at (pair, part, k_alpha, k_beta) = {at}"
    return g


@CASES
def test_g_bin_by_bin(name, i):
    m = plan(name)
    attach(m, name, i)
    check_g(m, name, i)


def test_ragged_chunks_give_one_g(monkeypatch):
    """Lc = 150 streamed as 128 + 22, 96 + 54 and 32 x 4 + 22 planes: "one order however the planes are split" -- the same bits;
    and the filters that are one at a single plane leave G = tpl[t, l] sotf[l] rounded once."""
    name = "ragged_own_otf"
    m, c = plan(name), ic.case(name)
    got = {}
    for chunk in ic.CHUNKS:
        with monkeypatch.context() as mp:
            if chunk is None:
                mp.delenv("SURFH_IMAGER_CHUNK", raising=False)
            else:
                mp.setenv("SURFH_IMAGER_CHUNK", chunk)
            attach(m, name, 0)
        got[chunk] = check_g(m, name, 0, tag=f"-chunk{chunk}")
    for chunk in ic.CHUNKS[1:]:
        assert same_bits(got[None], got[chunk]), f"chunk {chunk}: " + where_differ(got[None], got[chunk])
    (Na, Nb), nkb, T = c["imshape"], c["imshape"][1] // 2 + 1, c["T"]
    g = got[None].reshape(c["F"], T, 2, *got[None].shape[2:])[:, :, :, :Na, :nkb]
    for f, l in ((0, 0), (1, c["Lc"] - 1)):
        want = c["tpl"][:, l, None, None] * c["own"][l][None]                           # fp32 times fp32: exact in float64
        want = np.stack([want.real, want.imag], axis=1).astype(np.float32)
        assert np.array_equal(g[f], want), f"filter {f} (plane {l}): {np.count_nonzero(g[f] != want)} components are not the product rounded once"


# ---- 2. the operator element by element ----------------------------------------------------------------------------------------------
def run_operator(m, dev, c):
    """forward(x), adjoint(u), fwadj(x) without and with the weights"""
    no_data(m)
    out = dict(forward=dev.forward(c["x"]), adjoint=dev.adjoint(c["u"]), fwadj=dev.fwadj(c["x"]))
    _set_data(m, np.zeros(c["im"].oshape), c["w"], 0.0)                   # the weights of fwadj; mu = 0: no term
    out["fwadj_weighted"] = dev.fwadj(c["x"])
    no_data(m)
    return out


def check_operator(m, dev, name, i, tag=""):
    c, want = ic.case(name, i), ic.outputs(name, i)
    got = run_operator(m, dev, c)
    over = {}
    for what, ref in want.items():
        assert got[what].shape == ref.shape and np.isfinite(got[what]).all()
        e = local_errs(got[what], ref, ic.axes_of(what))
        note("imager_edges_operator", case=c["id"] + tag, output=what, **e)
        print(f"{c['id']}{tag} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items() if not k.endswith("_at")))
        over.update({(what, k): (v, e.get(k + "_at")) for k, v in e.items() if not k.endswith("_at") and not v < TOL})
    gap = _gap(c["u"], got["forward"], got["adjoint"], c["x"])
    note("imager_edges_dot", case=c["id"] + tag, dot_gap=gap)
    assert not over, f"{c['id']}: (output, measure) -> (value, index) above {TOL:g}: {over}"
    assert gap < 1e-6
    return got


@CASES
def test_operator_element_by_element(name, i):
    m = plan(name)
    dev, _ = attach(m, name, i)
    check_operator(m, dev, name, i)


# ---- 3. identities without a tolerance -----------------------------------------------------------------------------------------------
def check_identities(m, dev, name, i):
    c = ic.case(name, i)
    a, b = run_operator(m, dev, c), run_operator(m, dev, c)
    for what in a:                                                          # (d) each call repeated gives the same bits
        assert same_bits(a[what], b[what]), f"{c['id']} {what} twice: " + where_differ(a[what], b[what])
    y32 = a["forward"].astype(np.float32)
    assert np.array_equal(y32, a["forward"])
    # (a) the window kernel forms each tile's sum in the sample kernel's order and writes what spread copies
    composed = dev.adjoint(y32)
    assert same_bits(a["fwadj"], composed), f"{c['id']}: fwadj(x) against adjoint(forward(x)): " + where_differ(a["fwadj"], composed)
    # (b) with weights: the product w * y in fp32, a weight of zero a select
    w32 = c["w"].astype(np.float32)
    wy = np.where(w32 > 0, w32 * y32, np.float32(0)).astype(np.float32)
    composed = dev.adjoint(wy)
    assert same_bits(a["fwadj_weighted"], composed), f"{c['id']}: weighted fwadj(x) against adjoint(w forward(x)): " + \
        where_differ(a["fwadj_weighted"], composed)
    # (c) the adjoint of zero is zero
    zero = dev.adjoint(np.zeros(c["im"].oshape))
    assert not zero.any(), f"{c['id']}: adjoint(0) has {np.count_nonzero(zero)} non-zero elements"


@CASES
def test_identities_bit_for_bit(name, i):
    m = plan(name)
    dev, _ = attach(m, name, i)
    check_identities(m, dev, name, i)


# ---- 4. the transform temporary the imager shares with the plan's operator ------------------------------------------------------------
@pytest.mark.parametrize("name", ["h2_T1", "wide_beta"])
def test_shared_temporary_through_attach_and_detach(name):
    """A fresh plan holds ycol_maps for max(T, 1) planes; the first attachment has F > T and makes it F planes.  The plan's own
    forward and adjoint give the same bits before, after, after an attachment with F = 1 and after the detach; the imager that
    follows the larger one passes the checks above."""
    p = ic.plan(name)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((p["T"],) + p["shape"]).astype(np.float32)
    cube = rng.standard_normal((p["Lc"],) + p["shape"]).astype(np.float32)
    m = make_plan(name)
    try:
        def own():
            return m.forward(x), m.adjoint(cube)
        want = own()
        assert all(np.isfinite(a).all() and a.any() for a in want)

        def unchanged(when):
            for what, a, b in zip(("forward", "adjoint"), own(), want):
                assert same_bits(a, b), f"{name}: the plan's {what} {when}: " + where_differ(a, b)
        F0 = p["attach"][0][0]
        assert F0 > p["T"]
        dev, c = attach(m, name, 0)
        unchanged(f"after attaching F = {F0}")
        first = run_operator(m, dev, c)
        unchanged(f"after applying the imager with F = {F0}")
        if name == "h2_T1":                                     # F = 1 after F = 16, on the buffers the larger one left
            dev1, c1 = attach(m, name, 1)
            assert c1["F"] == 1
            check_g(m, name, 1, tag="-after-F16")
            check_operator(m, dev1, name, 1, tag="-after-F16")
            check_identities(m, dev1, name, 1)
        else:
            c1 = ic.case(name, 1)
            dev1 = ImagerModel(m, c1["filters"][:1], decim=c1["d"]).attach()
            ref = io.ImagerOracle(c1["sotf"], c1["tpl"], c1["filters"][:1], c1["d"], c1["imshape"])
            e = local_errs(dev1.forward(c1["x"]), ref.forward(c1["x"]), ic.FORWARD_AXES)
            assert all(v < TOL for k, v in e.items() if not k.endswith("_at")), e
        unchanged("after attaching F = 1")
        dev, c = attach(m, name, 0)                             # and the larger one again: the bits of its first attachment
        again = run_operator(m, dev, c)
        for what in first:
            assert same_bits(first[what], again[what]), f"{name} {what} re-attached: " + where_differ(first[what], again[what])
        detach(m)
        unchanged("after the detach")
    finally:
        m.close()


# ---- 5. one solver with more filters than templates -----------------------------------------------------------------------------------
def test_cg_with_more_filters_than_templates():
    """The joint problem of tests/test_gpu_imager.py (config1, T = 4) with five filters, d = 3 and weights on both instruments, at
    the bounds of test_cg_matches_joint_oracle: a NaN under every zero weight."""
    cfg = problems.config1()
    om = problems.oracle_model(cfg, box="direct")
    N, d = cfg["N"], 3
    filters = imager.synthetic_filters(cfg["wavel"], 5)
    assert filters.shape[0] > cfg["templates"].shape[0] == 4
    im = io.ImagerOracle(cfg["sotf"], cfg["templates"], filters, d, (N, N), fast=True)
    p = wo.standard(cfg, om)
    yi = im.forward(cfg["maps"])
    y_im = yi + np.random.default_rng(2).standard_normal(yi.shape) * 1e-2 * np.sqrt(np.mean(yi ** 2))
    rng = np.random.default_rng(6)
    w_im = np.exp(rng.uniform(np.log(0.5), np.log(2.0), yi.shape))
    w_im[rng.random(yi.shape) < 0.12] = 0.0
    j = io.Joint(om, im, MU, MU_IM, p["w"], w_im)
    y_im_nan = np.where(w_im == 0, np.nan, y_im)
    y_nan = np.where(p["masked"], np.nan, p["y"])
    ref = orc.lcg(j, j.data(y_nan, y_im_nan), MU, MUR, np.zeros(om.ishape), tol=1e-12, max_iter=NIT)
    gr = np.array(ref["grad_norm"])
    m = build_model(cfg)
    try:
        m.set_imager(ImagerModel(m, filters, decim=d))
        x, gn, n = m.cg(y_nan, mu=MU, mu_reg=MUR, max_iter=NIT, tol=1e-12, weights=p["w"], imager=(y_im_nan, MU_IM, w_im))
        plain = m.cg(y_nan, mu=MU, mu_reg=MUR, max_iter=NIT, tol=1e-12, weights=p["w"])[0]
    finally:
        m.close()
    e, ge = rel(x, ref["x"]), _max_rel(gn[:10], gr[:10])
    note("imager_edges_cg_F5_T4", err_x=e, err_gradnorm_first10=ge, moved_by_the_term=rel(x, plain))
    print(f"cg, F = 5 > T = 4: iterate {e:.2e}, first ten r.r {ge:.2e}, the term moves the iterate by {rel(x, plain):.2e}")
    assert np.isfinite(x).all() and n == NIT and len(gn) == NIT + 1
    assert ge < CG_GRADNORM_TOL and e < CG_ITERATE_TOL
