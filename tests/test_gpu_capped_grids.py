"""The capped-grid kernels past their launch caps and chunk seams on the device (needs an MI355X): the robust data term from
16-, 8- and 4-byte aligned pointers, po_data, the maps' Huber kernels across a template boundary on their second trip, and the
cube's Huber kernels with several planes per chunk, uneven chunks and a second trip over the pixels.  Sizes, inputs, float64
expectations and the check functions: tests/capped_cases.py; that every size is in the regime it is named for, and that the
checks reject the faults of those regimes: tests/test_capped_grid_host.py (no GPU).  The CG vector kernels and nn_project take
their sizes from the same module in test_gpu_local_parity.py and test_gpu_nonneg.py.

Every case compares with float64 element by element, per template / per plane, checks the reductions, requires the same bits
from a second call and writes what it measured to the parity log."""
import time

import numpy as np
import pytest

import capped_cases as cc
import posterior_oracle as pso
from helpers import build_model, max_err, rel
from oracle import surfh_oracle as orc
from surfh_amd import potentials as P
from test_gpu_parity import note

pytestmark = pytest.mark.gpu
GUARD = 123.0


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0")


def _dev_off(a, off, fill=GUARD):
    """``a`` on the device ``off`` floats into a buffer of guard values; returns (buffer, view of the n floats)"""
    import torch
    n = a.size
    b = torch.full((n + off + 8,), fill, dtype=torch.float32, device="cuda:0")
    b[off: off + n] = _dev(a.ravel())
    return b, b[off: off + n]


def _guards_intact(buf, off, n):
    h = buf.cpu().numpy()
    return bool(np.all(h[:off] == GUARD) and np.all(h[off + n:] == GUARD))


@pytest.fixture(scope="module")
def old_plan():
    """The 5 x 72 x 77 plan of the earlier kernel-level tests: the flat-vector kernels run on any plan, and the bounds that
    are taken from the device's own error are taken here, not on the shapes under test."""
    m = build_model(pso.rect_problem(*cc.MAPS_OLD[1:], cc.MAPS_OLD[0]))
    yield m
    m.close()


def prior_add_bound(m):
    """ten times the error prior_add shows against NumPy on this plan's maps (test_gpu_nonneg.py, test_gpu_posterior.py)"""
    import torch
    rng = np.random.default_rng(40 + m.ishape[0])
    er, ec = (rng.standard_normal(m.ishape).astype(np.float32) for _ in range(2))
    q_t = _dev(ec)
    m.prior_add_dev(_dev(er), q_t, 9.0)
    torch.cuda.synchronize()
    er64 = er.astype(np.float64)
    bound = 10 * max_err(q_t.cpu().numpy(), ec.astype(np.float64) + 9.0 * (orc.diff_r_t(orc.diff_r(er64)) + orc.diff_c_t(orc.diff_c(er64))))
    assert 0 < bound < 1e-5
    return bound


# ---- robust_data, robust_curv ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off,V", cc.ROBUST_CALLS)
def test_robust_kernels_past_the_cap(old_plan, n, off, V):
    """2048 blocks of V floats a thread and a second trip: aligned (V = 4, three blocks on the second trip, a tail of 3), two
    floats off (V = 2, a tail of 1), one float off (V = 1).  The 1e-6 gates of test_gpu_robust.py on v, sum phi and the
    curvature, the count within the samples at the knee (at most 10; none with these seeds); and the sums of the second trip
    and of the tail on their own, as differences against calls on the first k samples (capped_cases.segment_sums)."""
    import torch
    m, c = old_plan, cc.robust_case(n)
    (_, y_t), (_, u_t), (_, w_t), (_, p0_t), (_, p1_t) = (_dev_off(c[k], off) for k in ("y", "u", "w", "p0", "p1"))
    assert all(t.data_ptr() % 16 == 4 * off for t in (y_t, u_t, w_t, p0_t, p1_t))
    runs = []
    for _ in range(2):
        vbuf, v_t = _dev_off(np.full(n, 7.0, dtype=np.float32), off)
        sums = m.robust_data_dev(y_t, u_t, w_t, v_t, n, cc.DD)
        curv = m.robust_curv_dev(y_t, u_t, w_t, p0_t, p1_t, n, cc.DD)
        torch.cuda.synchronize()
        assert _guards_intact(vbuf, off, n)
        runs.append((v_t.cpu().numpy(), sums, curv))
    prefix = []
    for k in cc.robust_prefixes(n, V):
        _, s_t = _dev_off(np.zeros(n, dtype=np.float32), off)
        prefix.append((k, m.robust_data_dev(y_t, u_t, w_t, s_t, k, cc.DD), m.robust_curv_dev(y_t, u_t, w_t, p0_t, p1_t, k, cc.DD)))
    e = cc.check_robust(c, *runs[0], prefix)
    print(f"robust n = {n} off = {off} V = {V}:", e)
    note("capped_robust", n=n, off=off, V=V, **e)
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])


# ---- po_data ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", cc.PO_VARIANTS)
def test_po_data_past_the_cap(old_plan, variant):
    """1 049 353 samples on 4096 blocks: a ragged second trip.  A sample of weight 0 keeps its bits -- a finite value, a NaN, a NaN
    with a payload -- and every other one is within the prior_add-derived bound of test_gpu_posterior.py; without weights too."""
    import torch
    m, c = old_plan, cc.po_case()
    bound = prior_add_bound(m)
    y, w = cc.po_inputs(c, variant)
    n = c["n"]
    outs = []
    for _ in range(2):
        buf, out_t = _dev_off(np.full(n, 7.0, dtype=np.float32), 0)
        m.po_data_dev(_dev(y), None if w is None else _dev(w), _dev(c["eps"]), out_t, n, cc.PO_MU)
        torch.cuda.synchronize()
        assert _guards_intact(buf, 0, n)
        outs.append(out_t.cpu().numpy())
    e = cc.check_po(c, variant, outs[0], bound)
    print(f"po_data n = {n} {variant}: {e:.2e} (bound {bound:.2e})")
    note("capped_po_data", n=n, variant=variant, err=e, bound=bound)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---- huber_grad, huber_curv on the maps -------------------------------------------------------------------------------------------------
def _maps_outputs(m, c):
    from test_gpu_potentials import _maps_outputs as run
    return run(m, c["kind"], c["x"], c["g0"], c["p0"], c["p1"], cc.COEF, cc.DELTA)


def test_map_kernels_past_the_cap(old_plan):
    """5 x 120 x 141 = 84 600 entries on 256 blocks: the second trip runs from inside template 3 into template 4.  Every
    potential; the rule of test_gpu_potentials.test_map_kernels_match_numpy -- ten times the Huber gradient's own error, taken on
    the 5 x 72 x 77 plan -- on the gradient (whole, worst template, worst element), sum phi and the curvature block."""
    old = cc.maps_case(cc.MAPS_OLD)
    bound = 10 * rel(_maps_outputs(old_plan, old)[0], old["grad"])
    assert 1e-9 < bound < 1e-5
    m = build_model(pso.rect_problem(*cc.MAPS_SHAPE[1:], cc.MAPS_SHAPE[0]))
    try:
        assert tuple(m.ishape) == cc.MAPS_SHAPE
        for kind in P.NAMES:
            c = cc.maps_case(cc.MAPS_SHAPE, kind)
            out, val, curv = _maps_outputs(m, c)
            out2, val2, curv2 = _maps_outputs(m, c)
            e = cc.check_maps(c, out, val, curv, bound)
            print(f"maps {cc.MAPS_SHAPE} {kind}: bound {bound:.2e}", e)
            note("capped_huber_maps", shape=list(cc.MAPS_SHAPE), kind=kind, bound=bound, **e)
            assert np.array_equal(out, out2) and val == val2 and np.array_equal(curv, curv2)
        assert m.get_potential("spatial") == "huber"
    finally:
        m.close()


# ---- huber_vox_grad, huber_vox_curv -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cc.VOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cube_kernels_past_one_plane_per_chunk(shape):
    """50 x 128 x 128 (32 chunks of 1 and 2 planes), 37 x 160 x 205 (a ragged last tile, 15 chunks of 2 and 3 planes) and
    3 x 728 x 728 (2071 tiles on 2048 blocks: one chunk of all planes, 23 blocks on a second trip over the pixels), on
    template-free plans; the Huber pair and the two mixed pairs.  The 1e-6 gates of test_gpu_vox._check_kernels on the gradient
    (whole, worst plane, worst element), the two sums of phi and the two curvature blocks."""
    from test_gpu_potentials import _plane_model, _vox_outputs
    t0 = time.perf_counter()
    m = _plane_model(*shape)
    t_plan = time.perf_counter() - t0
    try:
        assert tuple(m.ishape) == shape
        t0 = time.perf_counter()
        for ks, kl in cc.VOX_PAIRS:
            c = cc.vox_case(shape, ks, kl)
            args = (m, ks, kl, c["x"], c["g0"], c["p0"], c["p1"], cc.VOX["cs"], cc.VOX["ds"], cc.VOX["cl"], cc.VOX["dl"])
            out, vals, curv = _vox_outputs(*args)
            out2, vals2, curv2 = _vox_outputs(*args)
            e = cc.check_vox(c, out, vals, curv)
            print(f"cube {shape} ({ks}, {kl}):", e)
            note("capped_huber_vox", shape=list(shape), ks=ks, kl=kl, plan_seconds=t_plan, **e)
            assert np.array_equal(out, out2) and tuple(vals) == tuple(vals2) and np.array_equal(curv, curv2)
        print(f"cube {shape}: plan built in {t_plan:.1f} s, the three pairs checked in {time.perf_counter() - t0:.1f} s")
        assert [m.get_potential(s) for s in P.SLOTS] == ["huber"] * 3
    finally:
        m.close()
