"""The vector kernels of the plane-wise CG and 3MG loops, element by element: the shapes, the inputs, the float64 expectations and
the check functions shared by tests/test_planes_cases_host.py (no GPU) and tests/test_gpu_planes_kernels.py.

Every ``run_*`` function builds the buffers of one kernel call (inputs, guards), hands them to ``launch(which, ext, vectors, sc_in,
sc_out, mu_reg, update_r)`` -- which works in place: the GPU test uploads, calls ``planes_cg_dev`` (surfh_debug_planes_cg, the
launchers the solvers call) and downloads; the host test runs an fp32 numpy restatement, clean or with a fault injected -- twice
on fresh copies, and asserts: the same bits both times, ``const`` inputs back bit for bit, guards untouched, the bounds below.  It
returns the measured errors in units of their bounds.

Shapes: the smallest at which a kernel can go wrong.  Plane-major kernels run one workgroup of 256 threads per plane: npix on both
sides of 256, a ragged fifth trip (1101), one plane and three.  The wavelength-innermost ("pn") kernels deal the Na Nb pixels to
128 slices [npix k / 128, npix (k + 1) / 128) which four sub-threads walk with stride 4, 64 wavelengths to a block: fewer pixels
than slices, slices of 1 or 2, slices of 5 or 6 (a second trip), one and two blocks of wavelengths, the degenerate stencils
Na, Nb = 1, 2.  The transposes move 32 x 32 tiles: 31, 33 and 70 on both tile axes.

What lies outside a < Na, l < Lc, and a tail behind every array, is the guard value where a kernel writes the array and zero where
it only reads it, as the solver keeps its padding; both must come back bit for bit.  The pn kernels run over all LP wavelengths:
padding wavelengths of the pixels inside hold the guard in x and q (x + 0 * 0 and q + mu_reg * 0 give the guard back) and zero in
r and d, whose sums must come out as exactly 0.  With three planes (and from three wavelengths on) one is all zero in r, d, q, m,
qm and must keep still, and another is handed a zero denominator over live vectors.  The 3MG kernels also run on their first
iteration (m = Qm = 0) and with Qm (mmmg_dir) or Qd (mmmg_step) negated: no curvature over live vectors, beta = 0 and the step (0, 0).

Bounds, all from fp32 arithmetic (EPS = 2^-24; fused multiply-adds drop roundings, so they only lower the errors):
  SUMS      the kernels add exact float64 products of fp32 values: 1e-14 of sum |a||b| (capped_cases.check_dot; the summation depth
            is at most 5 trips + 8 + 4 < 23).  A sum returned beside a stored fp32 vector is held to the float64 sum of what was stored.
            r.Qm of mmmg_dir and the four sums of mmmg_step never leave their kernel: they are held through beta and the step,
            whose bounds leave them no more room (an error of EPS of a sum moves the scaled term of every element by a quarter of AXPY).
  AXPY      x + s d, r - s q, r + beta d, r + beta m with s, beta formed in float64 from the float64 sums: AXPY (|a| + |s b|)
            (capped_cases.AXPY: the scalar's rounding to fp32, the product, the sum, second order).  A zero denominator, and
            m.Qm <= 0 in mmmg_dir, give exactly 0: the output equals the other operand bit for bit.
  MM_MOVE   mv = s0 d + s1 m (and qv on qd, qm) with (s0, s1) from surfh_mm_step2 on the float64 sums: two scalar roundings, two
            products, one sum -- each term carries at most three roundings: 4 EPS (|s0 d| + |s1 m|) with the second order.
  MM_AXPY   x + mv, r - qv: one more rounding on the sum, which is at most |x| + |mv|: 6 EPS (|x| + |s0 d| + |s1 m|) (r: |r|, qd, qm).
  PRIOR     q + mu_reg ((2d - d_a- - d_a+) + (2d - d_b- - d_b+)): two doublings are exact; four subtractions, the sum of the
            halves, the product, the final sum -- seven roundings -- and mu_reg's conversion to fp32:
            8 EPS (|q| + mu_reg (4 |d| + sum |neighbours|)).
  transposes are copies: bit for bit."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from capped_cases import AXPY, EPS, cg_vectors, check_dot, within

f32 = np.float32
TPB, PN_SPLIT = 256, 128
GUARD, GUARD64, TAIL = f32(-77.25), -5.5, 37
MM_MOVE, MM_AXPY, PRIOR = 4 * EPS, 6 * EPS, 8 * EPS
MU_REGS = (0.05, 3.7)

PM_NPIX, PM_L = (1, 255, 256, 257, 1101), (1, 3)
PN_SHAPES = ((1, 1, 64, 64, 64), (2, 1, 64, 64, 1), (1, 2, 64, 64, 3), (2, 2, 64, 64, 64), (3, 5, 64, 64, 64), (13, 11, 64, 128, 70),
             (23, 29, 64, 128, 128))                                        # (Na, Nb, NAP, LP, Lc)
TR_CASES = tuple((L, nb, na, l0) for L in (1, 31, 33, 70) for nb in (1, 31, 33) for na in (1, 3) for l0 in (0, 2))
TR_NAP = 64


def tr_lp(L):
    return 64 if L <= 64 else 128


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ratio(num, den):
    """num / den in float64, exactly 0 under a zero denominator"""
    num, den = np.atleast_1d(f64(num)), np.atleast_1d(f64(den))
    out = np.zeros_like(num)
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def dot_ok(got, a, b, what):
    """capped_cases.check_dot; vectors without a non-zero product give exactly 0"""
    a, b = f64(a).ravel(), f64(b).ravel()
    if not np.any(a * b):
        assert got == 0.0, f"{what}: {got!r} from vectors whose products are all zero"
        return 0.0
    try:
        return check_dot(float(got), a, b) / 1e-14
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def units(got, want, scale, what):
    """capped_cases.within on the flattened arrays; returns the worst error in units of the bound"""
    got, want, scale = got.ravel(), f64(want).ravel(), f64(scale).ravel()
    within(got, want, scale, what)
    nz = scale > 0
    return float(np.max(np.abs(f64(got) - want)[nz] / scale[nz])) if nz.any() else 0.0


def still(got, before, where, what):
    """bit for bit inside ``where`` (a boolean array or slice)"""
    g, b = bits(got)[where], bits(before)[where]
    bad = np.flatnonzero((g != b).ravel())
    assert bad.size == 0, f"{what}: {bad.size} elements changed, the first at {bad[0]} of the selection: {got[where].ravel()[bad[0]]!r}"


def buf(a, fill=0.0):
    """the flat buffer of an array and a tail of ``fill`` behind it"""
    return np.concatenate([np.ascontiguousarray(a, dtype=f32).ravel(), np.full(TAIL, fill, dtype=f32)])


def call(launch, which, ext, vecs, const=(), sc_in=None, sc_out=None, mu_reg=0.0, update_r=1):
    """two launches on fresh copies: the same bits, the ``const`` vectors and every tail as they went in; (vectors, sc_out)"""
    runs = []
    for _ in range(2):
        v = [a.copy() for a in vecs]
        so = None if sc_out is None else sc_out.copy()
        launch(which, ext, v, None if sc_in is None else np.ascontiguousarray(sc_in, dtype=np.float64), so, float(mu_reg), int(update_r))
        runs.append((v, so))
    (v1, s1), (v2, s2) = runs
    for i, (a, b) in enumerate(zip(v1, v2)):
        assert same_bits(a, b), f"{which}: vector {i} differs between two calls"
    assert s1 is None or same_bits(s1, s2), f"{which}: the sums differ between two calls: {s1} {s2}"
    for i, a in enumerate(v1):
        still(a, vecs[i], slice(None) if i in const else slice(a.size - TAIL, None), f"{which}: {'const vector' if i in const else 'tail of vector'} {i}")
    return v1, s1


def mm_step2(v, mqm):
    """(s0, s1) of surfh_mm_step2 on the float64 sums v = (d.Qd, d.Qm, d.r, m.r)"""
    from surfh_amd import _lib
    out = (ctypes.c_double * 2)()
    _lib.check(_lib.load().surfh_mm_step2(float(v[0]), float(v[1]), float(mqm), float(v[2]), float(v[3]), out))
    return out[0], out[1]


def rowdot(a, b):
    return np.sum(f64(a).reshape(a.shape[0], -1) * f64(b).reshape(b.shape[0], -1), axis=1)


def frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return kw


# ---- plane-major kernels: arrays [L][npix] -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pm_case(L, npix):
    """x, r, d, q (d.q > 0), b, m, qm (m.Qm > 0) and the float64 sums.  L = 3: plane 1 is all zero in r, d, q, m, qm; plane 2 is handed
    a zero denominator (d.q in cg_step, the old r.r in cg_dir) over live vectors."""
    seed = 500 + 7 * npix + L
    x, r, d, q, b = (v.reshape(L, npix) for v in cg_vectors(L * npix, seed))
    rng = np.random.default_rng(seed + 1)
    m = rng.standard_normal((L, npix)).astype(f32)
    qm = ((0.5 + rng.random((L, npix))) * m + 0.1 * rng.standard_normal((L, npix))).astype(f32)
    if L == 3:
        for v in (r, d, q, m, qm):
            v[1] = 0.0
    rr, dq, old = rowdot(r, r), rowdot(d, q), rowdot(b, b)
    if L == 3:
        dq[2], old[1], old[2] = 0.0, 0.0, 0.0
    return frozen(L=L, npix=npix, x=x, r=r, d=d, q=q, m=m, qm=qm, rr=rr, dq=dq, old=old, mqm=rowdot(m, qm),
                  zero=[1] if L == 3 else [], noden=[2] if L == 3 else [])


def _body(v, c):
    return v[:c["L"] * c["npix"]].reshape(c["L"], c["npix"])


def run_pm_dot(c, launch):
    L, ext = c["L"], (c["L"], c["npix"])
    _, out = call(launch, "dot", ext, [buf(c["d"]), buf(c["q"])], const=(0, 1), sc_out=np.full(L, GUARD64))
    e = max(dot_ok(out[l], c["d"][l], c["q"][l], f"d.q of plane {l}") for l in range(L))
    for l in c["zero"]:
        assert out[l] == 0.0
    return dict(dq=e)


def run_pm_step(c, launch, update_r=1):
    L, ext = c["L"], (c["L"], c["npix"])
    vecs = [buf(c["x"], GUARD), buf(c["r"], GUARD), buf(c["d"]), buf(c["q"])]
    (x1, r1, _, _), rrn = call(launch, "cg_step", ext, vecs, const=(2, 3) if update_r else (1, 2, 3), sc_in=np.stack([c["rr"], c["dq"]]),
                               sc_out=np.full(L, GUARD64), update_r=update_r)
    x1, r1 = _body(x1, c), _body(r1, c)
    s = ratio(c["rr"], c["dq"])[:, None]
    x, r, d, q = (f64(c[k]) for k in "xrdq")
    e = dict(x=units(x1, x + s * d, AXPY * (np.abs(x) + np.abs(s * d)), "x + s d"))
    for l in c["zero"] + c["noden"]:                     # a zero step: nothing moves
        still(x1, c["x"], l, f"x of plane {l} under a zero step")
        still(r1, c["r"], l, f"r of plane {l} under a zero step")
    if update_r:
        e["r"] = units(r1, r - s * q, AXPY * (np.abs(r) + np.abs(s * q)), "r - s q")
        e["rrn"] = max(dot_ok(rrn[l], r1[l], r1[l], f"r.r of plane {l} against the stored residual") for l in range(L))
    else:
        assert np.all(rrn == GUARD64), f"update_r = 0 wrote r.r: {rrn}"
    return e


def run_pm_dir(c, launch):
    L, ext = c["L"], (c["L"], c["npix"])
    (d1, _), rr = call(launch, "cg_dir", ext, [buf(c["d"], GUARD), buf(c["r"])], const=(1,), sc_in=np.stack([c["rr"], c["old"]]),
                       sc_out=np.full(L, GUARD64))
    d1 = _body(d1, c)
    beta = ratio(c["rr"], c["old"])[:, None]
    r, d = f64(c["r"]), f64(c["d"])
    e = dict(d=units(d1, r + beta * d, AXPY * (np.abs(r) + np.abs(beta * d)), "r + beta d"))
    assert same_bits(rr, c["rr"]), f"rr <- rr': {rr} from {c['rr']}"
    for l in c["zero"] + c["noden"]:
        assert np.array_equal(d1[l], c["r"][l]), f"plane {l}: beta = 0 has to give d = r"
    return e


def run_mmmg_dir(c, launch, first=False, neg=False):
    """``first``: the first iteration, m = Qm = 0; ``neg``: Qm negated, m.Qm < 0 over live vectors.  Both give d = r bit for bit"""
    L, ext = c["L"], (c["L"], c["npix"])
    m, qm = (np.zeros_like(c[k]) if first else c[k] for k in ("m", "qm"))
    if neg:
        qm = -qm
    (d1, _, _, _), out = call(launch, "mmmg_dir", ext, [buf(c["d"], GUARD), buf(c["r"]), buf(m), buf(qm)], const=(1, 2, 3),
                              sc_out=np.full((2, L), GUARD64))
    d1 = _body(d1, c)
    e = dict(rr=max(dot_ok(out[0, l], c["r"][l], c["r"][l], f"r.r of plane {l}") for l in range(L)),
             mqm=max(dot_ok(out[1, l], m[l], qm[l], f"m.Qm of plane {l}") for l in range(L)))
    mqm = rowdot(m, qm)
    beta = np.where(mqm > 0, -ratio(rowdot(c["r"], qm), mqm), 0.0)[:, None]
    r, m64 = f64(c["r"]), f64(m)
    e["d"] = units(d1, r + beta * m64, AXPY * (np.abs(r) + np.abs(beta * m64)), "r + beta m")
    for l in range(L):
        if beta[l, 0] == 0.0:
            assert np.array_equal(d1[l], c["r"][l]), f"plane {l}: beta = 0 has to give d = r"
    assert not (first or neg) or (np.array_equal(d1, c["r"]) and not beta.any())
    return e


def run_mmmg_step(c, launch, update_r=1, first=False, neg=False):
    """d, qd: the case's d, q.  ``first``: m = Qm = 0 and m.Qm = 0, the step is (d.r / d.Qd, 0); ``neg``: Qd negated, no curvature
    along d over live vectors, the step is (0, 0) and nothing moves"""
    L, ext = c["L"], (c["L"], c["npix"])
    c = dict(c, q=-c["q"]) if neg else c
    m, qm = (np.zeros_like(c[k]) if first else c[k] for k in ("m", "qm"))
    mqm = rowdot(m, qm)
    vecs = [buf(c["x"], GUARD), buf(c["r"], GUARD), buf(c["d"]), buf(m, GUARD), buf(qm, GUARD), buf(c["q"])]
    (x1, r1, _, m1, qm1, _), _ = call(launch, "mmmg_step", ext, vecs, const=(2, 5) if update_r else (1, 2, 5), sc_in=mqm, update_r=update_r)
    x1, r1, m1, qm1 = (_body(v, c) for v in (x1, r1, m1, qm1))
    sums = np.stack([rowdot(c["d"], c["q"]), rowdot(c["d"], qm), rowdot(c["d"], c["r"]), rowdot(m, c["r"])], axis=1)
    step = np.array([mm_step2(sums[l], mqm[l]) for l in range(L)])
    if first:
        assert np.all(step[:, 1] == 0.0) and np.array_equal(step[:, 0], ratio(sums[:, 2], sums[:, 0]))
    s0, s1 = step[:, :1], step[:, 1:]
    x, r, d, qd, m64, qm64 = (f64(v) for v in (c["x"], c["r"], c["d"], c["q"], m, qm))
    mv, qv = s0 * d + s1 * m64, s0 * qd + s1 * qm64
    amv, aqv = np.abs(s0 * d) + np.abs(s1 * m64), np.abs(s0 * qd) + np.abs(s1 * qm64)
    e = dict(m=units(m1, mv, MM_MOVE * amv, "s0 d + s1 m"), qm=units(qm1, qv, MM_MOVE * aqv, "s0 Qd + s1 Qm"),
             x=units(x1, x + mv, MM_AXPY * (np.abs(x) + amv), "x + mv"))
    if update_r:
        e["r"] = units(r1, r - qv, MM_AXPY * (np.abs(r) + aqv), "r - qv")
    assert not neg or not step.any()
    for l in range(L):                                   # no curvature: the plane keeps still
        if l in c["zero"]:
            assert tuple(step[l]) == (0.0, 0.0) and not r1[l].any()
        if tuple(step[l]) == (0.0, 0.0):
            still(x1, c["x"], l, f"x of the plane {l} without curvature")
            still(r1, c["r"], l, f"r of the plane {l} without curvature")
            assert not m1[l].any() and not qm1[l].any()
    return e


# ---- wavelength-innermost kernels: arrays [Nb][NAP][LP] ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pn_case(shape):
    """x, r, d, q, b inside a < Na, l < Lc (zero elsewhere) and the float64 sums per wavelength [LP].  From three wavelengths on,
    wavelength Lc // 2 is all zero in r, d, q and wavelength Lc - 1 is handed a zero denominator over live vectors."""
    Na, Nb, NAP, LP, Lc = shape
    vs = [np.zeros((Nb, NAP, LP), dtype=f32) for _ in range(5)]
    for v, src in zip(vs, cg_vectors(Nb * Na * Lc, 700 + Na + 31 * Nb + Lc)):
        v[:, :Na, :Lc] = src.reshape(Nb, Na, Lc)
    x, r, d, q, b = vs
    zero, noden = ([Lc // 2], [Lc - 1]) if Lc >= 3 else ([], [])
    for v in (r, d, q):
        v[:, :, zero] = 0.0
    lamdot = lambda u, v: np.einsum("bal,bal->l", f64(u), f64(v))  # noqa: E731
    rr, dq, old = lamdot(r, r), lamdot(d, q), lamdot(b, b)
    dq[noden], old[zero], old[noden] = 0.0, 0.0, 0.0
    inside = np.zeros((Nb, NAP, LP), dtype=bool)
    inside[:, :Na, :Lc] = True
    return frozen(shape=shape, ext=(Na, Nb, NAP, LP, Lc, 0), x=x, r=r, d=d, q=q, rr=rr, dq=dq, old=old, zero=zero, noden=noden, inside=inside,
                  lamdot=lamdot)


def pn_buf(c, a, role):
    """"in": as it is (zero padding); "acc" (x, q): the guard everywhere outside; "rw" (r, d): the guard at a >= Na, zero in the padding
    wavelengths of the pixels inside"""
    Na = c["shape"][0]
    a = a.copy()
    if role == "acc":
        a[~c["inside"]] = GUARD
    elif role == "rw":
        a[:, Na:, :] = GUARD
    return buf(a, GUARD if role != "in" else 0.0)


def _pn_body(v, c):
    Na, Nb, NAP, LP, Lc = c["shape"]
    return v[:Nb * NAP * LP].reshape(Nb, NAP, LP)


def _pn_outside(c, got, before, what):
    still(_pn_body(got, c), _pn_body(before, c), ~c["inside"], f"{what} outside a < Na, l < Lc")


def _pn_sums(c, out, a, b, what):
    Lc, LP = c["shape"][4], c["shape"][3]
    assert np.all(out[Lc:] == 0.0), f"{what}: padding wavelengths {np.flatnonzero(out[Lc:] != 0.0) + Lc} are not 0"
    return max(dot_ok(out[l], a[:, :, l], b[:, :, l], f"{what} of wavelength {l}") for l in range(Lc))


def run_pn_dot(c, launch):
    LP = c["shape"][3]
    _, out = call(launch, "pn_dot", c["ext"], [pn_buf(c, c["d"], "in"), pn_buf(c, c["q"], "in")], const=(0, 1), sc_out=np.full(LP, GUARD64))
    return dict(dq=_pn_sums(c, out, c["d"], c["q"], "d.q"))


def run_pn_prior_dot(c, launch, mu_reg):
    Na, Nb, NAP, LP, Lc = c["shape"]
    vecs = [pn_buf(c, c["d"], "in"), pn_buf(c, c["q"], "acc")]
    (_, q1), out = call(launch, "pn_prior_dot", c["ext"], vecs, const=(0,) if mu_reg else (0, 1), sc_out=np.full(LP, GUARD64), mu_reg=mu_reg)
    _pn_outside(c, q1, vecs[1], "q")
    q1 = _pn_body(q1, c)
    d, q = f64(c["d"][:, :Na]), f64(c["q"][:, :Na])
    nb = [np.roll(d, 1, axis=1), np.roll(d, -1, axis=1), np.roll(d, 1, axis=0), np.roll(d, -1, axis=0)]      # a-, a+, b-, b+, circular
    want = q + mu_reg * ((2 * d - nb[0] - nb[1]) + (2 * d - nb[2] - nb[3]))
    scale = PRIOR * (np.abs(q) + mu_reg * (4 * np.abs(d) + sum(np.abs(v) for v in nb)))
    live = (slice(None), slice(0, Na), slice(0, Lc))
    e = dict(q=units(q1[live], want[:, :, :Lc], scale[:, :, :Lc], f"q + mu_reg Lap d, [b][a][l] of {(Nb, Na, Lc)}"))
    q_stored = np.where(c["inside"], q1, 0.0)
    e["dq"] = _pn_sums(c, out, c["d"], q_stored, "d.q against the stored q")
    return e


def run_pn_step(c, launch, update_r=1):
    LP = c["shape"][3]
    vecs = [pn_buf(c, c["x"], "acc"), pn_buf(c, c["r"], "rw"), pn_buf(c, c["d"], "in"), pn_buf(c, c["q"], "in")]
    (x1, r1, _, _), rrn = call(launch, "pn_step", c["ext"], vecs, const=(2, 3) if update_r else (1, 2, 3), sc_in=np.stack([c["rr"], c["dq"]]),
                               sc_out=np.full(LP, GUARD64), update_r=update_r)
    _pn_outside(c, x1, vecs[0], "x")
    _pn_outside(c, r1, vecs[1], "r")
    x1, r1 = _pn_body(x1, c), _pn_body(r1, c)
    s = ratio(c["rr"], c["dq"])
    x, r, d, q = (f64(c[k]) for k in "xrdq")
    ins = c["inside"]
    e = dict(x=units(x1[ins], (x + s * d)[ins], (AXPY * (np.abs(x) + np.abs(s * d)))[ins], "x + s d (inside, flattened)"))
    for l in c["zero"] + c["noden"]:
        still(x1[:, :, l], c["x"][:, :, l], ins[:, :, l], f"x of wavelength {l} under a zero step")
        still(r1[:, :, l], c["r"][:, :, l], ins[:, :, l], f"r of wavelength {l} under a zero step")
    if update_r:
        e["r"] = units(r1[ins], (r - s * q)[ins], (AXPY * (np.abs(r) + np.abs(s * q)))[ins], "r - s q (inside, flattened)")
        r_stored = np.where(ins, r1, 0.0)
        e["rrn"] = _pn_sums(c, rrn, r_stored, r_stored, "r.r against the stored residual")
    else:
        assert np.all(rrn == GUARD64), "update_r = 0 wrote r.r"
    return e


def run_pn_dir(c, launch):
    vecs = [pn_buf(c, c["d"], "rw"), pn_buf(c, c["r"], "in")]
    (d1, _), _ = call(launch, "pn_dir", c["ext"], vecs, const=(1,), sc_in=np.stack([c["rr"], c["old"]]))
    _pn_outside(c, d1, vecs[0], "d")
    d1 = _pn_body(d1, c)
    beta = ratio(c["rr"], c["old"])
    r, d, ins = f64(c["r"]), f64(c["d"]), c["inside"]
    e = dict(d=units(d1[ins], (r + beta * d)[ins], (AXPY * (np.abs(r) + np.abs(beta * d)))[ins], "r + beta d (inside, flattened)"))
    for l in c["zero"] + c["noden"]:
        assert np.array_equal(d1[:, :, l][ins[:, :, l]], c["r"][:, :, l][ins[:, :, l]]), f"wavelength {l}: beta = 0 has to give d = r"
    return e


# ---- the transposes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tr_case(L, nb, na, l0):
    """cube [l0 + L + 1][na][nb] (a plane behind the L moved ones) and its wavelength-innermost image [nb][TR_NAP][LP]"""
    LP = tr_lp(L)
    rng = np.random.default_rng(40 + L + 100 * nb + 7 * na + l0)
    cube = rng.standard_normal((l0 + L + 1, na, nb)).astype(f32)
    lam = rng.standard_normal((nb, TR_NAP, LP)).astype(f32)
    return frozen(ext=(na, nb, TR_NAP, LP, L, l0), L=L, nb=nb, na=na, l0=l0, LP=LP, cube=cube, lam=lam)


def run_transposes(c, launch):
    L, nb, na, l0, LP = c["L"], c["nb"], c["na"], c["l0"], c["LP"]
    moved = c["cube"][l0:l0 + L]
    dst = np.full((nb, TR_NAP, LP), GUARD)
    (_, lam1), _ = call(launch, "to_lam_inner", c["ext"], [buf(c["cube"]), buf(dst, GUARD)], const=(0,))
    want = dst.astype(f32)
    want[:, :na, :L] = np.transpose(moved, (2, 1, 0))
    assert same_bits(lam1, buf(want, GUARD)), f"to_lam_inner: {np.flatnonzero(bits(lam1) != bits(buf(want, GUARD)))[:4]} differ"
    back = np.full(c["cube"].shape, GUARD)
    (_, cube1), _ = call(launch, "from_lam_inner", c["ext"], [lam1, buf(back, GUARD)], const=(0,))
    want = back.astype(f32)
    want[l0:l0 + L] = moved                                                   # the round trip is the identity on the L planes from l0
    assert same_bits(cube1, buf(want, GUARD)), f"round trip: {np.flatnonzero(bits(cube1) != bits(buf(want, GUARD)))[:4]} differ"
    # the way back alone, from an array that is no image of a cube
    (_, cube2), _ = call(launch, "from_lam_inner", c["ext"], [buf(c["lam"]), buf(back, GUARD)], const=(0,))
    want[l0:l0 + L] = np.transpose(c["lam"][:, :na, :L], (2, 1, 0))
    assert same_bits(cube2, buf(want, GUARD)), f"from_lam_inner: {np.flatnonzero(bits(cube2) != bits(buf(want, GUARD)))[:4]} differ"
    return dict(exact=0.0)
