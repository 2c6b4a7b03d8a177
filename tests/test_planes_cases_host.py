"""The vector kernels of the plane-wise CG and 3MG loops, the part that needs no GPU (tests/planes_cases.py).

Every kernel is restated in numpy fp32 (sums in float64, as the kernels keep them), walking the data as the kernel does: a plane-major
kernel deals element i of a plane to thread i % 256 on trip i // 256; a wavelength-innermost one deals the pixels to 128 slices
[npix k / 128, npix (k + 1) / 128), four sub-threads per wavelength walking a slice with stride 4; a transpose moves 32 x 32 tiles.

(a) the restatements pass every check at every shape -- the float64 expectations alone stay inside every bound, without any
    device (numpy rounds every product and sum, the worst case the bounds are derived for);
(b) the checks have teeth: every fault of ``FAULTS`` is rejected at the shapes listed for it (each rejection is printed)."""
import numpy as np
import pytest

import planes_cases as pc
from planes_cases import PN_SPLIT, TPB, f32

FAULTS = ("clamp_am", "clamp_ap", "clamp_bm", "clamp_bp", "nap_swapped", "seam_plus", "seam_minus", "neighbour_scalar", "nonzero_step",
          "pad_written", "update_r_ignored", "tile_31", "l0_ignored")


def _thread_sums(terms):
    """[L, npix] float64 terms -> per plane: every thread adds its trips, a wave its 64 threads, the block its 4 waves"""
    L, npix = terms.shape
    trips = -(-npix // TPB)
    t = np.zeros((L, trips * TPB))
    t[:, :npix] = terms
    return t.reshape(L, trips, TPB).sum(axis=1).reshape(L, TPB // 64, 64).sum(axis=2).sum(axis=1)


def _scalar(num, den, fault):
    """fp32 of num / den, 0 under a zero denominator"""
    s = pc.ratio(num, den)
    if fault == "nonzero_step":
        s = np.where(np.asarray(den) == 0, 1.0, s)
    if fault == "neighbour_scalar":
        s = np.roll(s, 1)
    return s.astype(f32)


def _pn_chunks(Na, Nb, NAP, fault):
    """the rows (b NAP + a of [Nb NAP][LP]) of every (slice, sub-thread), in the kernel's order"""
    npix = Na * Nb
    for k in range(PN_SPLIT):
        p0, p1 = npix * k // PN_SPLIT, npix * (k + 1) // PN_SPLIT
        if fault == "seam_plus":
            p1 = min(p1 + 1, npix)
        elif fault == "seam_minus" and k < PN_SPLIT - 1:
            p1 = max(p1 - 1, p0)
        for sub in range(TPB // 64):
            pix = np.arange(p0 + sub, p1, TPB // 64)
            if pix.size:
                b, a = pix // Na, pix % Na
                yield b, a, (b * Na + a if fault == "nap_swapped" else b * NAP + a)


def restated(fault=None):
    """``launch`` of planes_cases.call: the kernels in numpy, in place"""
    def launch(which, ext, v, sc_in, so, mu_reg, update_r):
        if which in ("dot", "cg_step", "cg_dir", "mmmg_dir", "mmmg_step"):
            L, npix = ext
            a = [u[:L * npix].reshape(L, npix) for u in v]                    # views: the kernels work in place
            if which == "dot":
                so[:] = _thread_sums(pc.f64(a[0]) * pc.f64(a[1]))
            elif which == "cg_step":
                x, r, d, q = a
                step = _scalar(sc_in[0], sc_in[1], fault)[:, None]
                x += step * d
                if update_r or fault == "update_r_ignored":
                    r -= step * q
                if update_r:
                    so[:] = _thread_sums(pc.f64(r) ** 2)
            elif which == "cg_dir":
                d, r = a
                d[:] = r + _scalar(sc_in[0], sc_in[1], fault)[:, None] * d
                so[:] = sc_in[0]
            elif which == "mmmg_dir":
                d, r, m, qm = a
                s = [_thread_sums(pc.f64(u) * pc.f64(w)) for u, w in ((r, r), (r, qm), (m, qm))]
                beta = np.where(s[2] > 0, -pc.ratio(s[1], s[2]), 1.0 if fault == "nonzero_step" else 0.0)
                if fault == "neighbour_scalar":
                    beta = np.roll(beta, 1)
                d[:] = r + beta.astype(f32)[:, None] * m
                so[0], so[1] = s[0], s[2]
            else:
                x, r, d, m, qm, qd = a
                s = np.stack([_thread_sums(pc.f64(u) * pc.f64(w)) for u, w in ((d, qd), (d, qm), (d, r), (m, r))], axis=1)
                step = np.array([pc.mm_step2(s[l], sc_in[l]) for l in range(L)])
                if fault == "neighbour_scalar":
                    step = np.roll(step, 1, axis=0)
                if fault == "nonzero_step":
                    step[(step == 0).all(axis=1)] = 1.0
                f0, f1 = step[:, :1].astype(f32), step[:, 1:].astype(f32)
                mv, qv = f0 * d + f1 * m, f0 * qd + f1 * qm
                x += mv
                m[:], qm[:] = mv, qv
                if update_r or fault == "update_r_ignored":
                    r -= qv
            if fault == "pad_written":
                v[0][L * npix] = 1.0
            return
        Na, Nb, NAP, LP, Lc, l0 = ext
        if which in ("to_lam_inner", "from_lam_inner"):
            edge = 31 if fault == "tile_31" else 32
            cube = v[0 if which == "to_lam_inner" else 1][:(l0 + Lc + 1) * Na * Nb].reshape(l0 + Lc + 1, Na, Nb)
            lam = v[1 if which == "to_lam_inner" else 0][:Nb * NAP * LP].reshape(Nb, NAP, LP)
            off = 0 if fault == "l0_ignored" else l0
            for bx in range(0, Nb, 32):
                for ly in range(0, Lc, 32):
                    bs, ls = slice(bx, min(bx + edge, Nb)), slice(ly, min(ly + edge, Lc))
                    cs = slice(off + ls.start, off + ls.stop)
                    if which == "to_lam_inner":
                        lam[bs, :Na, ls] = np.transpose(cube[cs, :, bs], (2, 1, 0))
                    else:
                        cube[cs, :, bs] = np.transpose(lam[bs, :Na, ls], (2, 1, 0))
            if fault == "pad_written" and Lc < LP and which == "to_lam_inner":
                lam[:, :Na, Lc] = 1.0
            return
        a = [u[:Nb * NAP * LP].reshape(Nb * NAP, LP) for u in v]
        part = np.zeros(LP)
        if which == "pn_dot":
            for _, _, rows in _pn_chunks(Na, Nb, NAP, fault):
                part += (pc.f64(a[0][rows]) * pc.f64(a[1][rows])).sum(axis=0)
            so[:] = part
        elif which == "pn_prior_dot":
            d, q = a
            mu = f32(mu_reg)
            row = (lambda b, aa: b * Na + aa) if fault == "nap_swapped" else (lambda b, aa: b * NAP + aa)
            for b, aa, rows in _pn_chunks(Na, Nb, NAP, fault):
                dv, qv = d[rows], q[rows]
                if mu != 0:
                    am = np.where(aa > 0, aa - 1, aa if fault == "clamp_am" else Na - 1)
                    ap = np.where(aa + 1 < Na, aa + 1, aa if fault == "clamp_ap" else 0)
                    bm = np.where(b > 0, b - 1, b if fault == "clamp_bm" else Nb - 1)
                    bp = np.where(b + 1 < Nb, b + 1, b if fault == "clamp_bp" else 0)
                    lap = (f32(2) * dv - d[row(b, am)] - d[row(b, ap)]) + (f32(2) * dv - d[row(bm, aa)] - d[row(bp, aa)])
                    qv = qv + mu * lap
                    q[rows] = qv
                part += (pc.f64(dv) * pc.f64(qv)).sum(axis=0)
            so[:] = part
        elif which == "pn_step":
            x, r, d, q = a
            step = _scalar(sc_in[0], sc_in[1], fault)
            for _, _, rows in _pn_chunks(Na, Nb, NAP, fault):
                x[rows] += step * d[rows]
                if update_r or fault == "update_r_ignored":
                    r[rows] -= step * q[rows]
                if update_r:
                    part += (pc.f64(r[rows]) ** 2).sum(axis=0)
            if update_r:
                so[:] = part
            if fault == "pad_written" and Lc < LP:
                x.reshape(Nb, NAP, LP)[:, :Na, Lc] = 1.0
        else:
            assert which == "pn_dir", which
            d, r = a
            beta = _scalar(sc_in[0], sc_in[1], fault)
            for _, _, rows in _pn_chunks(Na, Nb, NAP, fault):
                d[rows] = r[rows] + beta * d[rows]
    return launch


def rejected(label, run, *args, **kw):
    try:
        run(*args, **kw)
    except AssertionError as e:
        print(f"rejected: {label}: {' '.join(str(e).split())[:120]}")
        return
    pytest.fail(f"{label}: the fault passed its check")


# ---- (a) the restatements pass -------------------------------------------------------------------------------------------------------
def _worst(acc, e):
    for k, v in e.items():
        acc[k] = max(acc.get(k, 0.0), v)


def test_plane_major_restatements_pass():
    go = restated()
    worst = {name: {} for name in ("dot", "cg_step", "cg_dir", "mmmg_dir", "mmmg_step")}
    for L in pc.PM_L:
        for npix in pc.PM_NPIX:
            c = pc.pm_case(L, npix)
            _worst(worst["dot"], pc.run_pm_dot(c, go))
            _worst(worst["cg_dir"], pc.run_pm_dir(c, go))
            for kw in ({}, dict(first=True), dict(neg=True)):
                _worst(worst["mmmg_dir"], pc.run_mmmg_dir(c, go, **kw))
            for update_r in (1, 0):
                _worst(worst["cg_step"], pc.run_pm_step(c, go, update_r))
                for kw in ({}, dict(first=True), dict(neg=True)):
                    _worst(worst["mmmg_step"], pc.run_mmmg_step(c, go, update_r, **kw))
    print("plane-major restatements, worst error in units of each bound:", worst)
    assert all(v <= 1.0 for e in worst.values() for v in e.values())
    assert max(worst["mmmg_step"][k] for k in ("m", "qm")) < 0.75 and max(worst["mmmg_step"][k] for k in ("x", "r")) < 0.75


def test_pn_restatements_pass():
    go = restated()
    worst = {name: {} for name in ("pn_dot", "pn_prior_dot", "pn_step", "pn_dir")}
    for shape in pc.PN_SHAPES:
        c = pc.pn_case(shape)
        _worst(worst["pn_dot"], pc.run_pn_dot(c, go))
        _worst(worst["pn_dir"], pc.run_pn_dir(c, go))
        for mu_reg in pc.MU_REGS + (0.0,):
            _worst(worst["pn_prior_dot"], pc.run_pn_prior_dot(c, go, mu_reg))
        for update_r in (1, 0):
            _worst(worst["pn_step"], pc.run_pn_step(c, go, update_r))
    print("wavelength-innermost restatements, worst error in units of each bound:", worst)
    assert all(v <= 1.0 for e in worst.values() for v in e.values())
    assert worst["pn_prior_dot"]["q"] < 0.6                  # seven roundings never line up: half of the bound is left


def test_transpose_restatements_pass():
    go = restated()
    for case in pc.TR_CASES:
        pc.run_transposes(pc.tr_case(*case), go)


def test_slices_cover_every_pixel_once():
    for Na, Nb, NAP, _, _ in pc.PN_SHAPES:
        rows = np.concatenate([r for _, _, r in _pn_chunks(Na, Nb, NAP, None)])
        want = (np.arange(Nb)[:, None] * NAP + np.arange(Na)[None, :]).ravel()
        assert np.array_equal(np.sort(rows), want)
    sizes = lambda npix: {npix * (k + 1) // PN_SPLIT - npix * k // PN_SPLIT for k in range(PN_SPLIT)}  # noqa: E731
    assert sizes(15) == {0, 1} and sizes(143) == {1, 2} and sizes(667) == {5, 6}                 # 5, 6 > 4 sub-threads: a second trip


# ---- (b) teeth -------------------------------------------------------------------------------------------------------------------------
def test_every_fault_is_rejected():
    seen = set()

    def bad(fault, label, run, c, *args, **kw):
        rejected(f"{fault}: {label}", run, c, restated(fault), *args, **kw)
        seen.add(fault)

    mid, big = pc.pn_case(pc.PN_SHAPES[5]), pc.pn_case(pc.PN_SHAPES[6])
    for fault in ("clamp_am", "clamp_ap", "clamp_bm", "clamp_bp"):
        for mu_reg in pc.MU_REGS:
            bad(fault, f"pn_prior_dot {mid['shape']} mu_reg {mu_reg}", pc.run_pn_prior_dot, mid, mu_reg)
    bad("clamp_am", "pn_prior_dot, Na = 2", pc.run_pn_prior_dot, pc.pn_case(pc.PN_SHAPES[3]), 0.05)    # 2d - 2d' against d - d'
    bad("clamp_bp", "pn_prior_dot, Nb = 2", pc.run_pn_prior_dot, pc.pn_case(pc.PN_SHAPES[2]), 0.05)
    for c in (pc.pn_case(pc.PN_SHAPES[4]), mid, big):
        bad("nap_swapped", f"pn_step {c['shape']}", pc.run_pn_step, c)
        bad("nap_swapped", f"pn_dot {c['shape']}", pc.run_pn_dot, c)
        bad("nap_swapped", f"pn_prior_dot {c['shape']}", pc.run_pn_prior_dot, c, 0.05)
        bad("nap_swapped", f"pn_dir {c['shape']}", pc.run_pn_dir, c)
        for fault in ("seam_plus", "seam_minus"):
            bad(fault, f"pn_step {c['shape']}", pc.run_pn_step, c)
            bad(fault, f"pn_step, x alone {c['shape']}", pc.run_pn_step, c, 0)
            bad(fault, f"pn_dot {c['shape']}", pc.run_pn_dot, c)
            bad(fault, f"pn_prior_dot {c['shape']}", pc.run_pn_prior_dot, c, 3.7)
            bad(fault, f"pn_dir {c['shape']}", pc.run_pn_dir, c)
    pm = pc.pm_case(3, 257)
    for fault in ("neighbour_scalar", "nonzero_step"):
        bad(fault, "cg_step 3 x 257", pc.run_pm_step, pm)
        bad(fault, "cg_dir 3 x 257", pc.run_pm_dir, pm)
        bad(fault, "mmmg_dir 3 x 257", pc.run_mmmg_dir, pm, neg=(fault == "nonzero_step"))
        bad(fault, "mmmg_step 3 x 257", pc.run_mmmg_step, pm, neg=(fault == "nonzero_step"))
        bad(fault, f"pn_step {mid['shape']}", pc.run_pn_step, mid)
        bad(fault, f"pn_dir {mid['shape']}", pc.run_pn_dir, mid)
    bad("neighbour_scalar", "pn_step (2, 2, 64, 64, 64)", pc.run_pn_step, pc.pn_case(pc.PN_SHAPES[3]))
    bad("pad_written", f"pn_step {mid['shape']}", pc.run_pn_step, mid)
    bad("pad_written", "cg_step 1 x 255", pc.run_pm_step, pc.pm_case(1, 255))
    bad("pad_written", "to_lam_inner L = 31", pc.run_transposes, pc.tr_case(31, 33, 3, 2))
    bad("update_r_ignored", "cg_step 3 x 257", pc.run_pm_step, pm, 0)
    bad("update_r_ignored", "mmmg_step 3 x 257", pc.run_mmmg_step, pm, 0)
    bad("update_r_ignored", f"pn_step {mid['shape']}", pc.run_pn_step, mid, 0)
    for case in ((33, 1, 1, 0), (1, 33, 3, 0), (70, 31, 1, 2), (31, 33, 3, 2)):
        bad("tile_31", f"transposes {case}", pc.run_transposes, pc.tr_case(*case))
    for case in ((1, 1, 1, 2), (33, 31, 3, 2), (70, 33, 1, 2)):
        bad("l0_ignored", f"transposes {case}", pc.run_transposes, pc.tr_case(*case))
    assert seen == set(FAULTS)


def test_clamped_neighbour_is_far_outside():
    """the fault the fused stencil is most likely to have sits some 1e6 bound units out: no marginal case"""
    c = pc.pn_case(pc.PN_SHAPES[5])
    Na, Nb, NAP, LP, Lc = c["shape"]
    v = [pc.pn_buf(c, c["d"], "in"), pc.pn_buf(c, c["q"], "acc")]
    clean = [u.copy() for u in v]
    restated()("pn_prior_dot", c["ext"], clean, None, np.zeros(LP), 0.05, 1)
    worst = 0.0
    for fault in ("clamp_am", "clamp_ap", "clamp_bm", "clamp_bp"):
        got = [u.copy() for u in v]
        restated(fault)("pn_prior_dot", c["ext"], got, None, np.zeros(LP), 0.05, 1)
        diff = np.abs(pc.f64(got[1]) - pc.f64(clean[1]))[:Nb * NAP * LP].reshape(Nb, NAP, LP)[c["inside"]]
        scale = pc.PRIOR * np.abs(pc.f64(c["q"]))[c["inside"]]
        worst = max(worst, float(np.max(diff[scale > 0] / scale[scale > 0])))
        assert np.max(diff) > 1e4 * pc.PRIOR, fault
    print(f"clamped neighbours: up to {worst:.1e} times 8 EPS |q|")
