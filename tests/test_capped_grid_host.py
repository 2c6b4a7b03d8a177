"""The capped-grid kernels past their launch caps and chunk seams, the part that needs no GPU (tests/capped_cases.py):

(a) through surfh_launch_geometry -- the library's own launch functions -- every new size is in the regime it is named for, and
    every kernel-level size the suite had before is in none of them (which is why the new sizes exist);
(b) the wavelength chunks of the cube's Huber kernels cover every plane exactly once on both sides of the 2048-block cap;
(c) the check functions have teeth: the float64 restatements of the kernels' loop structure, rounded to fp32, pass them, and
    every fault of that structure in capped_cases.FAULTS is rejected (each rejection is printed)."""
import numpy as np
import pytest

import capped_cases as cc
from capped_cases import TPB, geometry
from helpers import rel

f32 = np.float32


# ---- (a) geometry -----------------------------------------------------------------------------------------------------------------
def test_block_size_and_unknown_names():
    for k in (1, 2, 7):                                         # one more block for one more float: 256 threads a block
        assert geometry("cg_axpy", k * TPB)[0] == k and geometry("cg_axpy", k * TPB + 1)[0] == k + 1
        assert geometry("dot", k * TPB + 1)[0] == geometry("po_data", k * TPB + 1)[0] == geometry("robust", k * TPB + 1, 1)[0] == k + 1
        assert geometry("nn_project", k * TPB + 1, 0)[0] == geometry("huber_maps", 1, 1, k * TPB + 1)[0] == k + 1
        assert geometry("huber_vox", 1, 1, k * TPB + 1)[:2] == (k + 1, 1)
    for bad in (("no_such_kernel", 5), ("dot", 0), ("robust", 100, 3), ("huber_vox", 3, 0, 4), ("huber_maps", 1, 70000, 70000)):
        with pytest.raises(RuntimeError, match="surfh_launch_geometry"):
            geometry(*bad)


def test_new_sizes_are_past_the_caps_and_old_ones_are_not():
    # CG vectors: the dot kernels (512 blocks), the direction kernel that sums their partials, the 2048-block kernels
    assert geometry("dot", 131072) == (512, 1, 512, 1)
    assert geometry("dot", 131073) == (512, 1, 512, 2) and geometry("cg_dir_parts", 131073)[:3] == (513, 1, 512)
    assert geometry("cg_axpy", 131073)[3] == 1 and geometry("cg_axpy", 524288)[3] == 1
    assert geometry("dot", 600001) == (512, 1, 512, 5) and 600001 % (512 * TPB) not in (0, 512 * TPB - 1)       # a ragged fifth trip
    assert geometry("cg_axpy", 600001) == (2048, 1, 0, 2) and geometry("cg_dir_parts", 600001) == (2048, 1, 512, 2)
    assert 0 < 600001 - 2048 * TPB < 2048 * TPB and (600001 - 2048 * TPB) % TPB                                 # ... and second
    for n in cc.CG_OLD:
        g = geometry("cg_dir_parts", n)
        assert geometry("dot", n)[3] == 1 and geometry("cg_axpy", n)[3] == 1 and g[0] == g[2] and g[3] == 1, n
    # robust: V floats a thread; 2 100 227 puts three blocks on a second trip and leaves a tail of 3
    for n, off, V in cc.ROBUST_CALLS:
        grid, _, parts, trips = geometry("robust", n, V)
        assert (grid, parts, trips) == (2048, 2048, 2) and (n - n % V) // V > grid * TPB and n % V == (3, 1, 0)[(4, 2, 1).index(V)]
        assert off * 4 % 16 == (0, 8, 4)[(4, 2, 1).index(V)]                     # the widest access that offset allows
        assert cc.robust_prefixes(n, V) == [k for k in (2048 * TPB * V, n - n % V) if k != n]
    n = cc.ROBUST_CALLS[0][0]
    assert -(-(n // 4 - 2048 * TPB) // TPB) == 3
    assert all(geometry("robust", 100003, V)[3] == 1 for V in (4, 2, 1))
    # nn_project: 256 blocks
    (nv, _), (ns, _) = cc.NN_CALLS
    assert geometry("nn_project", nv, 1) == (256, 1, 256, 2) and nv % 4 == 3 and geometry("nn_project", ns, 0) == (256, 1, 256, 2)
    assert nv // 4 == 256 * TPB + 300 and ns == 256 * TPB + 300
    for (n, off) in cc.NN_OLD:
        assert geometry("nn_project", n, int(off == 0))[3] == 1
    # po_data: 4096 blocks
    assert geometry("po_data", cc.PO_N) == (4096, 1, 0, 2) and cc.PO_N % TPB and geometry("po_data", cc.PO_OLD)[3] == 1
    # maps Huber: 256 blocks; the second trip begins inside template 3 and ends in template 4
    T, na, nb = cc.MAPS_SHAPE
    assert geometry("huber_maps", T, na, nb) == (256, 1, 256, 2) and T * na * nb == 84600
    assert (256 * TPB) // (na * nb) == 3 and (256 * TPB) % (na * nb) and T == 5
    assert geometry("huber_maps", *cc.MAPS_OLD)[3] == 1
    # the cube: chunks of more than one plane, uneven chunks, the pixel stride
    want = ((64, 32), (129, 15), (2048, 1))
    for shape, sizes, (gx, gy) in zip(cc.VOX_SHAPES, cc.VOX_CHUNK_SIZES, want):
        g = geometry("huber_vox", *shape)
        assert g[:3] == (gx, gy, gx * gy) and g[3] == max(sizes), (shape, g)
        assert {l1 - l0 for l0, l1 in cc.chunks(shape[0], gy)} == sizes
    na, nb = cc.VOX_SHAPES[1][1:]
    assert (na * nb) % TPB and -(-na * nb // TPB) == 129                          # a ragged last tile
    na, nb = cc.VOX_SHAPES[2][1:]
    assert na * nb > 524288 and -(-na * nb // TPB) - 2048 == 23                   # 23 blocks on a second pixel trip
    for shape in cc.VOX_OLD:
        g = geometry("huber_vox", *shape)
        assert g[3] == 1 and g[1] == shape[0] and g[0] * TPB >= shape[1] * shape[2], shape
    assert geometry("huber_vox", 1024, 251, 251) == (247, 8, 1976, 128)          # config 2: what production runs


# ---- (b) chunk coverage -------------------------------------------------------------------------------------------------------------
def test_chunks_cover_every_plane_once():
    seen = set()
    for na, nb in ((1, 1), (16, 16), (72, 77), (128, 128), (160, 205), (251, 251), (501, 501), (724, 724), (1024, 511), (1024, 512),
                   (257, 2040), (728, 728), (1500, 1500)):
        tiles = -(-na * nb // TPB)
        for Lc in range(1, 71):
            gx, gy, parts, most = geometry("huber_vox", Lc, na, nb)
            assert gx == min(tiles, 2048) and 1 <= gy <= Lc and gx * gy <= 2048 and parts == gx * gy
            ch = cc.chunks(Lc, gy)
            cover = np.zeros(Lc, dtype=int)
            for l0, l1 in ch:
                assert l1 > l0                                   # no empty chunk: every block has a plane to start from
                cover[l0:l1] += 1
            assert np.all(cover == 1) and ch[0][0] == 0 and ch[-1][1] == Lc and max(l1 - l0 for l0, l1 in ch) == most
            seen.add((tiles > 2048, tiles == 2048, gy < Lc))
    assert {(True, False, True), (False, True, True), (False, False, True), (False, False, False)} <= seen      # both sides of the cap


# ---- (c) teeth ----------------------------------------------------------------------------------------------------------------------
def rejected(label, check, *args):
    """``check(*args)`` has to fail an assertion"""
    try:
        check(*args)
    except AssertionError as e:
        print(f"rejected: {label}: {' '.join(str(e).split())[:110]}")
        return
    pytest.fail(f"{label}: the fault passed its check")


def rounding_bound(want):
    """ten times the error of rounding the float64 expectation to fp32: the least a device-derived bound of this suite can be"""
    return 10 * rel(want.astype(f32), want)


def test_cube_march_faults_are_rejected():
    shape = cc.VOX_SHAPES[1]                                    # chunks of 2 and 3 planes
    for ks, kl in cc.VOX_PAIRS:
        c = cc.vox_case(shape, ks, kl)
        e = cc.check_vox(c, *cc.vox_restated(c))
        assert max(e["grad"], e["plane"], e["element"]) < 2e-7 and max(e["phi_s"], e["phi_l"], e["curv_s"], e["curv_l"]) < 1e-12, e
    c = cc.vox_case(shape)
    for fault in ("vprev_dropped", "c_stuck", "halo_again"):
        out, vals, curv = cc.vox_restated(c, fault)
        rejected(f"cube {shape} {fault}", cc.check_vox, c, out, vals, curv)
    # each output on its own: the gradient's carry is seen in the array, the curvature kernel's in its sums only
    clean = cc.vox_restated(c)
    stuck = cc.vox_restated(c, "c_stuck")
    rejected(f"cube {shape} c_stuck, curvature sums alone", cc.check_vox, c, clean[0], clean[1], stuck[2])
    rejected(f"cube {shape} c_stuck, gradient alone", cc.check_vox, c, stuck[0], clean[1], clean[2])
    c = cc.vox_case(cc.VOX_SHAPES[0])                           # chunks of 1 and 2 planes
    cc.check_vox(c, *cc.vox_restated(c))
    rejected(f"cube {cc.VOX_SHAPES[0]} vprev_dropped", cc.check_vox, c, *cc.vox_restated(c, "vprev_dropped"))


def test_cube_pixel_stride_fault_is_rejected():
    c = cc.vox_case(cc.VOX_SHAPES[2])                           # 2071 tiles on 2048 blocks
    clean = cc.vox_restated(c)
    cc.check_vox(c, *clean)
    bad = cc.vox_restated(c, "beyond_cap")
    rejected("cube 3 x 728 x 728 beyond_cap", cc.check_vox, c, *bad)
    rejected("cube 3 x 728 x 728 beyond_cap, sums alone", cc.check_vox, c, clean[0], bad[1], bad[2])
    assert rel(bad[0], c["grad"]) > 1e-2 and 23 * TPB / (728 * 728) < 0.012      # 1.1 % of the pixels: a falling criterion would not tell


def test_maps_faults_are_rejected():
    old = cc.maps_case(cc.MAPS_OLD)
    bound = rounding_bound(old["grad"])
    assert 1e-9 < bound < 1e-5
    for kind in cc.P.NAMES:
        c = cc.maps_case(cc.MAPS_SHAPE, kind)
        cc.check_maps(c, *cc.maps_restated(c), bound)
        for fault in ("stale_base", "beyond_cap"):
            out, val, curv = cc.maps_restated(c, fault)
            rejected(f"maps {kind} {fault}", cc.check_maps, c, out, val, curv, 0.99e-5)          # at the widest bound the rule admits
    c = cc.maps_case()
    clean, bad = cc.maps_restated(c), cc.maps_restated(c, "stale_base")
    rejected("maps stale_base, sums alone", cc.check_maps, c, clean[0], bad[1], bad[2], 0.99e-5)
    # only template 4 is wrong: the whole-array figure is diluted, the per-template one is not
    assert np.array_equal(bad[0][:4], clean[0][:4]) and not np.array_equal(bad[0][4], clean[0][4])


def test_robust_faults_are_rejected():
    for n, off, V in cc.ROBUST_CALLS:
        c = cc.robust_case(n)
        ks = cc.robust_prefixes(n, V)

        def outputs(fault):
            v, sums, curv = cc.robust_restated(c, V, fault)
            short = {k: cc.robust_case_prefix(c, k) for k in ks}
            pre = [(k,) + cc.robust_restated(short[k], V, fault if fault == "beyond_cap" else None)[1:] for k in ks]
            return v, sums, curv, pre
        clean = outputs(None)
        e = cc.check_robust(c, *clean)
        assert e["v"] < 1e-7 and e["phi"] < 1e-14 and all(v < 1e-9 for k, v in e.items() if "_from_" in k), e
        for fault in ("beyond_cap",) + (("no_tail",) if n % V else ()):
            bad = outputs(fault)
            rejected(f"robust n = {n} V = {V} {fault}", cc.check_robust, c, *bad)
            rejected(f"robust n = {n} V = {V} {fault}, sums alone", cc.check_robust, c, clean[0], *bad[1:])
            if fault == "no_tail":                  # by the segment sums alone, whatever the three values of the tail weigh
                k = n - n % V
                rejected(f"robust n = {n} V = {V} no_tail, segment sums alone", cc.segment_sums, bad[1][0], bad[3][-1][1][0], c["phi"], k, "sum phi")
                rejected(f"robust n = {n} V = {V} no_tail, segment curvature alone", cc.segment_sums, bad[2], bad[3][-1][2], c["curv"], k, "curv")


def test_nn_project_faults_are_rejected():
    for (n, off), vec in zip(cc.NN_CALLS, (1, 0)):
        c = cc.nn_case(n)
        for mode in cc.NN_MODES:
            want = {"r": c["rn"], "dv": c["dv"], "plain": c["rn"]}[mode]
            assert cc.check_nn(c, mode, *cc.nn_restated(c, mode, vec), rounding_bound(want)) < 1e-7
            for fault in ("beyond_cap",) + (("no_tail",) if vec else ()):
                rejected(f"nn_project n = {n} {mode} {fault}", cc.check_nn, c, mode, *cc.nn_restated(c, mode, vec, fault), 0.99e-5)
        # the sums alone, the tail of three: 1e-5 of the sums against the 1e-12 they are held to
        gz, gu, gw, _ = cc.nn_restated(c, "r", vec)
        if vec:
            rejected(f"nn_project n = {n} no_tail, sums alone", cc.check_nn, c, "r", gz, gu, gw, cc.nn_restated(c, "r", vec, "no_tail")[3], 0.99e-5)


def test_po_data_faults_are_rejected():
    c = cc.po_case()
    first = geometry("po_data", c["n"])[0] * TPB
    for variant in cc.PO_VARIANTS:
        y, w = cc.po_inputs(c, variant)
        want = cc.po_want(c, variant)
        live = np.isfinite(want)
        got = np.where(live, want, 0.0).astype(f32)
        got.view(np.uint32)[~live] = y.view(np.uint32)[~live]
        assert cc.check_po(c, variant, got, rounding_bound(want[live])) < 1e-7
        bad = got.copy()
        bad[first:] = 123.0
        rejected(f"po_data {variant} beyond_cap", cc.check_po, c, variant, bad, 0.99e-5)
        if variant == "nan":                                    # a payload that did not pass through
            bad = got.copy()
            bad[np.flatnonzero(c["dead"])[-2:]] = np.nan
            rejected("po_data NaN payload lost beyond the cap", cc.check_po, c, variant, bad, 0.99e-5)


def test_cg_faults_are_rejected():
    # the axpy kernels past 2048 blocks, the dot kernels past 512
    n = cc.CG_SIZES[1]
    x, r, d, q, b = cc.cg_vectors(n, 200 + n)
    b64, q64 = b.astype(np.float64), q.astype(np.float64)
    res = (b64 - q64).astype(f32)
    cc.within(res, b64 - q64, cc.EPS * np.abs(b64 - q64), "residual")
    bad = res.copy()
    bad[geometry("cg_axpy", n)[0] * TPB:] = 7.0
    rejected(f"residual n = {n} beyond_cap", cc.within, bad, b64 - q64, cc.EPS * np.abs(b64 - q64), "residual")
    grid = geometry("dot", n)[0]
    terms = d.astype(np.float64) * q64
    assert cc.check_dot(float(cc.block_partials(terms, grid).sum()), d, q) < 1e-15
    rejected(f"dot n = {n} beyond_cap", cc.check_dot, float(terms[:grid * TPB].sum()), d, q)
    rejected(f"dot n = {n} last element of the ragged trip skipped", cc.check_dot, float(terms[:-1].sum()), d, q)
    # the direction kernel at 513 blocks: it has to add the 512 partials of the step kernel, not one per block of its own
    n = cc.CG_SIZES[0]
    x, r, d, q, b = cc.cg_vectors(n, 300 + n)
    grid_dir, _, parts, _ = geometry("cg_dir_parts", n)
    assert (grid_dir, parts) == (513, 512) and parts == geometry("dot", n)[0]
    r64, d64 = r.astype(np.float64), d.astype(np.float64)
    rr_old = float(r64 @ r64)
    step = f32(rr_old / float(d64 @ q.astype(np.float64)))
    r1 = (r - step * q).astype(f32)
    r1_64 = r1.astype(np.float64)
    buf = np.full(2 * parts, 0.0)
    buf[parts:] = cc.block_partials(d64 * d64, parts)           # stale entries: an earlier product's partials behind the live ones
    buf[:parts] = cc.block_partials(r1_64 * r1_64, parts)

    def check_dir(nsum):
        rr = float(buf[:nsum].sum())
        own = float(r1_64 @ r1_64)
        assert abs(rr - own) <= 1e-14 * own, ("r.r against the stored residual", rr, own)
        beta = rr / rr_old
        d1 = (r1 + f32(beta) * d).astype(f32)
        cc.within(d1, r1_64 + (own / rr_old) * d64, cc.AXPY * (np.abs(r1_64) + np.abs(own / rr_old * d64)), "direction")
    check_dir(parts)
    rejected(f"cg_dir_parts n = {n} grid_count_partials", check_dir, grid_dir)
    # ... the direction itself would show it too: beta is off by one block's share of r.r, 2e-3, against 4 EPS
    d1 = (r1 + f32(float(buf[:grid_dir].sum()) / rr_old) * d).astype(f32)
    want = r1_64 + float(buf[:parts].sum()) / rr_old * d64
    rejected(f"cg_dir_parts n = {n} grid_count_partials, direction alone", cc.within, d1, want, cc.AXPY * (np.abs(r1_64) + np.abs(want - r1_64)),
             "direction")
