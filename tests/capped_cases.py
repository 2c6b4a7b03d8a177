"""The capped-grid kernels past their launch caps and chunk seams: the sizes, the inputs, float64 restatements of the kernels'
loop structure and the check functions shared by tests/test_capped_grid_host.py (no GPU) and the GPU tests
(tests/test_gpu_capped_grids.py and the parametrisations of test_gpu_local_parity.py, test_gpu_robust.py, test_gpu_nonneg.py).

Every bandwidth-bound kernel of the solvers launches at most ``cap`` blocks of 256 threads and covers the rest of its vector with
a grid-stride loop; the cube's Huber kernels (csrc/huber_vox.hip) march chunks of planes with values carried in registers.  The
sizes below are the smallest that leave the single-trip, one-plane-per-chunk regime; ``geometry`` asks the library itself
(surfh_launch_geometry, which calls the functions the launchers call) so that the host test can assert the regime of every size.

A check function takes a case (inputs and float64 expectations, computed once and cached) and what a kernel returned, asserts
the bounds and returns the measured errors.  The GPU tests hand it the device's output, the host test the float64 restatement
rounded to fp32 -- clean, and with a fault of the loop structure injected (``FAULTS``), which every check has to reject.

Bounds.  None is new: the element-wise ``within`` bounds of the CG kernels, 1e-14 of sum |a||b| for the float64 dot products
(depth of the summation at most trips + 18: 23 * 2^-53 = 2.6e-15 at n = 600 001), the 1e-6 gates of test_gpu_robust.py and of
test_gpu_vox._check_kernels, ten times the Huber gradient's own error for the maps (test_gpu_potentials.py), the rules of
test_gpu_nonneg.test_project_kernel_matches_numpy.  One check is added, ``segment_sums``: the float64 sums of a call on the first
k elements are subtracted from those of the whole call.  Both calls take the same path (same pointers, k a multiple of the
vector width) and compute the same fp32 terms for the first k elements, so the difference is the float64 sum of the terms of
[k, n) up to the rounding of two float64 summations, 2 * 23 * 2^-53 < 1e-14 of the whole sum; those terms have the kernel's fp32
error, the 1e-6 gate.  Without it a reduction that skipped the n % V floats behind the last vector is judged at the gate itself
(three terms of two million are 1.4e-6 of the sum on average) and passes or fails with the three values the seed put there."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import posterior_oracle as pso
import robust_oracle as ro
import vox_oracle as vo
from helpers import max_err, rel, slice_err
from oracle import surfh_oracle as orc
from surfh_amd import potentials as P

TPB = 256                                    # threads of a block, every kernel here (asserted through the hook by the host test)
GATE = 1e-6                                  # the kernel-level gate of test_gpu_robust.py and test_gpu_vox._check_kernels

# ---- the sizes --------------------------------------------------------------------------------------------------------------
CG_OLD = (1, 255, 1101, 3840, 100003)        # the kernel-level sizes before these tests: all single-trip
CG_SIZES = (131073, 600001)                  # second trip of the dot kernels and 513 blocks over 512 partials; ragged 2nd / 5th trips
ROBUST_CALLS = ((2100227, 0, 4), (1050003, 2, 2), (525001, 1, 1))      # (n, offset of every pointer in floats, V)
NN_CALLS = ((263347, 0), (65836, 1))         # (n, offset in floats): the 16-byte path with a tail of 3, the scalar path
NN_OLD = ((27720, 0), (5123, 1))
PO_N, PO_OLD = 1049353, 5123
MAPS_SHAPE, MAPS_OLD = (5, 120, 141), (5, 72, 77)
VOX_SHAPES = ((50, 128, 128), (37, 160, 205), (3, 728, 728))
VOX_CHUNK_SIZES = ({1, 2}, {2, 3}, {3})      # planes per chunk of the three shapes
VOX_OLD = ((1, 72, 77), (2, 72, 77), (5, 72, 77), (32, 48, 48))
VOX_PAIRS = (("huber", "huber"), ("hyperbolic", "hebert_leahy"), ("hebert_leahy", "hyperbolic"))


def geometry(which, a, b=0, c=0):
    """(grid x, grid y, partial sums the consumer adds, most loop trips of one thread) from the library's own launch functions."""
    from surfh_amd import _lib
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().surfh_launch_geometry(which.encode(), int(a), int(b), int(c), out))
    return tuple(int(v) for v in out)


def chunks(Lc, C):
    """the planes [l0, l1) of every wavelength chunk of huber_vox.hip"""
    return [(Lc * c // C, Lc * (c + 1) // C) for c in range(C)]


def block_partials(terms, grid):
    """per-block float64 sums of a grid-stride loop over ``terms``: element e belongs to block (e // 256) % grid"""
    return np.bincount((np.arange(terms.size) // TPB) % grid, weights=terms, minlength=grid)


# ---- CG vectors (moved here from test_gpu_local_parity.py, which imports them back) --------------------------------------------
EPS = 2.0 ** -24          # unit roundoff of fp32
# x + s d evaluated in fp32 from fp32 x, d and a float64 s: s rounded to fp32, the product, the sum (or one fused rounding) --
# three roundings of at most EPS each, relative to |x| + |s d|; 4 EPS covers their second-order terms
AXPY = 4 * EPS


def cg_vectors(n, seed):
    rng = np.random.default_rng(seed)
    x, r, d = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    q = ((0.5 + rng.random(n)) * d + 0.1 * rng.standard_normal(n)).astype(np.float32)      # d.q > 0, as under a positive operator
    b = rng.standard_normal(n).astype(np.float32)
    return x, r, d, q, b


def within(got, want, scale, what):
    """|got - want| <= scale element-wise (float64 ``want``); the failure names the worst element."""
    d = np.abs(got.astype(np.float64) - want) - scale
    k = int(np.argmax(d))
    assert d[k] <= 0, f"{what}: element {k} is {got[k]!r}, float64 gives {want[k]!r}, allowed {scale[k]:.3e}"


def check_dot(got, a, b):
    """a float64 sum of exact products: within 1e-14 of sum |a||b|; returns the error on that scale"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    scale = float(np.abs(a) @ np.abs(b))
    e = abs(got - float(a @ b)) / scale
    assert e <= 1e-14, (got, float(a @ b), e)
    return e


# ---- robust data term (the arrays of test_gpu_robust.test_kernels_match_numpy, which takes them from here) ---------------------------
DD = ro.DATA_DELTA


def robust_arrays(n):
    """u, w (a fifth of the samples masked), y with scaled residuals on both sides of the knee and NaN where masked, p0, p1"""
    rng = np.random.default_rng(100 + n)
    u = rng.standard_normal(n).astype(np.float32)
    w = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n)).astype(np.float32)
    w[rng.random(n) < 0.2] = 0.0
    if n == 1:
        w[:] = 1.5
    t0 = 2 * DD * rng.standard_normal(n)                                      # scaled residuals on both sides of the threshold
    if n == 1:
        t0[:] = 2.5 * DD
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(w > 0, u + t0 / np.sqrt(w), np.nan).astype(np.float32)   # NaN where the weight is 0
    p0, p1 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    return u, w, y, p0, p1


def robust_terms(y, u, w, p0, p1, delta=DD):
    """per sample in float64: keep, t, v, phi, beyond, and the three curvature terms [3, n]"""
    keep = w > 0
    w64, a, b = w.astype(np.float64), p0.astype(np.float64), p1.astype(np.float64)
    t = np.where(keep, np.sqrt(w64) * (np.where(keep, y, 0.0).astype(np.float64) - u), 0.0)
    ww = w64 * np.where(keep, ro.weight(t, delta), 0.0)
    return dict(keep=keep, t=t, v=np.sqrt(w64) * ro.dphi(t, delta), phi=ro.phi(t, delta), beyond=(np.abs(t) > delta).astype(np.float64),
                curv=np.stack([ww * a * a, ww * a * b, ww * b * b]), near=np.abs(np.abs(t) - delta) < 1e-6 * delta)


@functools.lru_cache(maxsize=None)
def robust_case(n):
    u, w, y, p0, p1 = robust_arrays(n)
    c = dict(n=n, u=u, w=w, y=y, p0=p0, p1=p1, **robust_terms(y, u, w, p0, p1))
    c["share"] = float(np.mean(np.abs(c["t"][c["keep"]]) > DD))
    return c


def robust_case_prefix(c, k):
    """the case of a call on the first k samples"""
    return {key: (k if key == "n" else v[..., :k] if isinstance(v, np.ndarray) else v) for key, v in c.items()}


def robust_prefixes(n, V):
    """lengths of the shorter calls of ``segment_sums``: the first trip of the capped grid alone, and all but the n % V last floats"""
    grid = geometry("robust", n, V)[0]
    return sorted({grid * TPB * V, n - n % V} - {n})


def segment_sums(whole, part, want_terms, k, what):
    """``whole`` - ``part`` (float64 sums of a call on n and on its first k elements) against the float64 sum of the terms of
    [k, n): within GATE of the largest segment sum plus the rounding of the two summations (module docstring)."""
    whole, part = np.atleast_1d(np.asarray(whole, dtype=np.float64)), np.atleast_1d(np.asarray(part, dtype=np.float64))
    want = np.atleast_2d(want_terms)[:, k:].sum(axis=1)
    assert np.max(np.abs(want)) > 0, (what, k, "an empty segment proves nothing")
    err = np.abs((whole - part) - want)
    allowed = GATE * np.max(np.abs(want)) + 1e-14 * np.abs(whole)
    assert np.all(err <= allowed), (what, k, whole - part, want, err, allowed)
    return float(np.max(err) / np.max(np.abs(want)))


def check_robust(c, v, sums, curv, prefix=()):
    """v [n] fp32, sums = (sum phi, count), curv [3] of one call; ``prefix``: (k, sums, curv) of calls on the first k samples"""
    keep, n = c["keep"], c["n"]
    near = int(np.sum(c["near"]))
    assert near <= 10 and 0.1 < c["share"] < 0.9
    assert v.shape == (n,) and np.all(np.isfinite(v)) and np.all(v[~keep] == 0.0)
    want_s, want_c = np.array([c["phi"].sum(), c["beyond"].sum()]), c["curv"].sum(axis=1)
    e = dict(v=float(np.max(np.abs(v - c["v"])) / np.max(np.abs(c["v"]))), phi=abs(sums[0] - want_s[0]) / want_s[0],
             curv=float(np.max(np.abs(curv - want_c)) / np.max(np.abs(want_c))), count_off=abs(sums[1] - want_s[1]), near=near)
    assert e["v"] < GATE and e["phi"] < GATE and e["curv"] < GATE and e["count_off"] <= near, e
    for k, s_k, c_k in prefix:
        e[f"phi_from_{k}"] = segment_sums(sums[0], s_k[0], c["phi"], k, "sum phi")
        e[f"curv_from_{k}"] = segment_sums(curv, c_k, c["curv"], k, "curvature")
        assert abs((sums[1] - s_k[1]) - c["beyond"][k:].sum()) <= int(np.sum(c["near"][k:])), ("count", k)
    return e


def robust_restated(c, V, fault=None):
    """What robust_data_kernel<V> and robust_curv_kernel<V> leave for the case, from the float64 terms: (v fp32 over a fill of 7,
    (sum phi, count), curv [3]).  Faults: "beyond_cap" (nothing past the first trip of the grid), "no_tail" (the n % V last
    floats skipped)."""
    n = c["n"]
    done = np.ones(n, dtype=bool)
    if fault == "beyond_cap":
        done[geometry("robust", n, V)[0] * TPB * V:] = False
    elif fault == "no_tail":
        assert n % V
        done[n - n % V:] = False
    else:
        assert fault is None
    v = np.where(done, c["v"], 7.0).astype(np.float32)
    return v, (float(c["phi"][done].sum()), float(c["beyond"][done].sum())), c["curv"][:, done].sum(axis=1)


# ---- nn_project (the arrays and the reference of test_gpu_nonneg.py, which imports them back) -----------------------------------
NN_RHO = 3e2
NN_MODES = ("r", "dv", "plain")


def kernel_arrays(n, seed):
    """x, u, z, r of both signs with, scattered over the vector: x + u exactly 0, +0 and -0 in every combination, denormal x + u of
    both signs (from denormal terms and as the difference of normal ones)."""
    rng = np.random.default_rng(seed)
    x, u, r = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    z = np.maximum(rng.standard_normal(n), 0.0).astype(np.float32)
    k = np.arange(n)
    u[k % 11 == 0] = -x[k % 11 == 0]                                   # x + u = 0 exactly
    for j, (a, b) in enumerate([(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)]):
        x[k % 53 == j], u[k % 53 == j] = a, b
    for j, (a, b) in enumerate([(1e-40, 0.0), (-1e-40, 0.0), (3e-39, -1e-39), (1.0 + 2.0 ** -23, -1.0), (-1.0 - 2.0 ** -23, 1.0)]):
        x[k % 59 == j + 5], u[k % 59 == j + 5] = a, b
    x[k % 61 == 7], u[k % 61 == 7] = np.float32(1.1754944e-38), np.float32(-1.1754942e-38)       # normal terms, denormal sum
    return x, u, z, (3e2 * r).astype(np.float32)


def project_ref(x, u, z, r, rho):
    """float32 where the kernel is exact (z', u'), float64 elsewhere."""
    t = x + u                                                          # float32
    zn = np.where(t > 0, t, np.float32(0.0)).astype(np.float32)
    un = (t - zn).astype(np.float32)
    d = lambda a: a.astype(np.float64)  # noqa: E731
    dv = rho * ((d(zn) - d(un)) - (d(z) - d(u)))
    return zn, un, dv, d(r) + dv


@functools.lru_cache(maxsize=None)
def nn_case(n):
    x, u, z, r = kernel_arrays(n, 7)
    zn, un, dv, rn = project_ref(x, u, z, r, NN_RHO)
    return dict(n=n, x=x, u=u, z=z, r=r, zn=zn, un=un, dv=dv, rn=rn)


def check_nn(c, mode, gz, gu, gw, sums, bound):
    """The rules of test_gpu_nonneg.test_project_kernel_matches_numpy: z', u' and the count exact, no set sign bit, the float64 sums
    to 1e-12, r / dv under ``bound`` (ten times prior_add's error there); returns the error of r / dv (0.0 in the plain mode)."""
    n, x, z, zn, un = c["n"], c["x"], c["z"], c["zn"], c["un"]
    d = lambda a: a.astype(np.float64)  # noqa: E731
    assert np.sum(zn == 0) > n // 4 and np.sum(zn > 0) > n // 4 and np.any((zn > 0) & (zn < 1.1754944e-38))
    assert not np.any(np.signbit(gz))
    assert np.array_equal(gz, zn) and np.array_equal(gu, un)
    assert sums[2] == float(np.sum(zn == 0))
    assert abs(sums[0] - np.sum((d(x) - d(zn)) ** 2)) <= 1e-12 * np.sum((d(x) - d(zn)) ** 2)
    assert abs(sums[1] - np.sum((d(zn) - d(z)) ** 2)) <= 1e-12 * np.sum((d(zn) - d(z)) ** 2)
    if mode == "plain":
        assert np.all(gw == 0.0) and sums[3] == 0.0
        return 0.0
    want = c["rn"] if mode == "r" else c["dv"]
    e = max_err(gw, want)
    assert e < bound, (mode, e, bound)
    if mode == "r":
        assert abs(sums[3] - np.sum(d(gw) ** 2)) <= 1e-12 * np.sum(d(gw) ** 2)
    else:
        assert sums[3] == 0.0
    return e


def nn_restated(c, mode, vec, fault=None):
    """nn_project_kernel's outputs for the case: (z', u', w, sums [4]); ``vec``: the 16-byte path.  Faults as in robust_restated."""
    n = c["n"]
    d = lambda a: a.astype(np.float64)  # noqa: E731
    done = np.ones(n, dtype=bool)
    if fault == "beyond_cap":
        done[geometry("nn_project", n, vec)[0] * TPB * (4 if vec else 1):] = False
    elif fault == "no_tail":
        assert vec and n % 4
        done[n - n % 4:] = False
    else:
        assert fault is None
    gz, gu = np.where(done, c["zn"], c["z"]), np.where(done, c["un"], c["u"])
    w0 = c["r"] if mode == "r" else np.zeros(n, dtype=np.float32)
    gw = w0 if mode == "plain" else np.where(done, c["rn"] if mode == "r" else c["dv"], w0).astype(np.float32)
    sums = np.array([np.sum((d(c["x"]) - d(c["zn"]))[done] ** 2), np.sum((d(c["zn"]) - d(c["z"]))[done] ** 2), float(np.sum(c["zn"][done] == 0)),
                     np.sum(d(gw)[done] ** 2) if mode == "r" else 0.0])
    return gz, gu, gw, sums


# ---- po_data ------------------------------------------------------------------------------------------------------------------
PO_MU = 4.0
PO_VARIANTS = ("zeros", "nan", "plain")      # weights that hold zeros under finite data, NaN (with payloads) at weight 0, no weights


@functools.lru_cache(maxsize=None)
def po_case(n=PO_N):
    """the vectors of test_gpu_posterior's detector check at n floats: y, w with a twentieth of the samples dead, eps"""
    rng = np.random.default_rng(60)
    y = (3.0 * rng.standard_normal(n)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32)
    dead = rng.random(n) < 0.05
    w[dead] = 0.0
    ynan = y.copy()
    ynan[dead] = np.nan
    ynan.view(np.uint32)[np.flatnonzero(dead)[::2]] = 0x7FC12345       # NaNs with a payload: the bits pass through
    eps = rng.standard_normal(n).astype(np.float32)
    return dict(n=n, y=y, ynan=ynan, w=w, dead=dead, eps=eps)


def po_inputs(c, variant):
    """(y, w or None) of a variant"""
    return (c["ynan"] if variant == "nan" else c["y"]), (None if variant == "plain" else c["w"])


def po_want(c, variant):
    y, w = po_inputs(c, variant)
    return pso.perturb_data(y.astype(np.float64), None if w is None else w.astype(np.float64), c["eps"].astype(np.float64), PO_MU)


def check_po(c, variant, got, bound):
    """a dead sample keeps the bits of y, every other is finite and within ``bound`` (prior_add's, as test_gpu_posterior.py) of
    float64 on the scale of the largest; a factor sqrt(mu) amiss is far outside.  Returns the error."""
    y, w = po_inputs(c, variant)
    live = np.ones(c["n"], dtype=bool) if w is None else ~c["dead"]
    assert got.shape == (c["n"],) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32)[~live], y.view(np.uint32)[~live]) and np.all(np.isfinite(got[live]))
    want = po_want(c, variant)
    e = max_err(got[live], want[live])
    assert e < bound, (variant, e, bound)
    w64 = None if w is None else w.astype(np.float64)
    assert max_err(got[live], pso.perturb_data(y.astype(np.float64), w64, c["eps"].astype(np.float64), PO_MU ** 2)[live]) > 1e-2
    return e


# ---- the Huber priors: arrays and float64 expectations (moved here from test_gpu_potentials.py, which imports them back) ---------
DELTA, COEF, TINY, HUGE = 0.3, 0.7, 1e-20, 1e5
SPAT = ((orc.diff_r, orc.diff_r_t), (orc.diff_c, orc.diff_c_t))


def pot_arrays(shape, seed, even_only=False):
    """x with differences on both sides of DELTA (``even_only``: weights below 1 in the even planes only), g0, p0, p1 -- and the
    overflow array: constant 8 x 8 blocks of height 0 .. 3e5"""
    rng = np.random.default_rng(seed)
    scale = 2 * DELTA
    if even_only:
        scale = np.where(np.arange(shape[0]) % 2 == 0, 2 * DELTA, 0.02 * DELTA)[:, None, None]
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    g0, p0, p1 = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    blocks = rng.integers(0, 4, size=(shape[0], -(-shape[1] // 8), -(-shape[2] // 8))).astype(np.float32)
    xo = (HUGE * np.kron(blocks, np.ones((1, 8, 8), dtype=np.float32)))[:, :shape[1], :shape[2]]
    return x, g0, p0, p1, np.ascontiguousarray(xo)


def spat_want(x, g0, a, b, coef, delta, kind):
    """per plane: g0 + coef sum_k D_k^T phi'(D_k x), sum_k sum phi, and the curvature block [L, 3] in float64"""
    x, a, b = (v.astype(np.float64) for v in (x, a, b))
    grad = g0.astype(np.float64) + coef * sum(dt(P.dphi(d(x), delta, kind)) for d, dt in SPAT)
    val = sum(np.sum(P.phi(d(x), delta, kind), axis=(1, 2)) for d, _ in SPAT)
    curv = np.stack([sum(np.sum(P.weight(d(x), delta, kind) * d(u) * d(v), axis=(1, 2)) for d, _ in SPAT)
                     for u, v in ((a, a), (a, b), (b, b))], axis=1)
    return grad, val, curv


def spec_want(x, a, b, coef, delta, kind):
    x, a, b = (v.astype(np.float64) for v in (x, a, b))
    if x.shape[0] == 1:
        return np.zeros_like(x), 0.0, np.zeros(3)
    grad = coef * vo.diff_l_t(P.dphi(vo.diff_l(x), delta, kind))
    w = P.weight(vo.diff_l(x), delta, kind)
    return grad, float(np.sum(P.phi(vo.diff_l(x), delta, kind))), np.array([np.sum(w * vo.diff_l(u) * vo.diff_l(v))
                                                                             for u, v in ((a, a), (a, b), (b, b))])


def curv_err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# ---- maps: huber_grad_kernel, huber_curv_kernel -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def maps_case(shape=MAPS_SHAPE, kind="huber"):
    x, g0, p0, p1, _ = pot_arrays(shape, 10 + shape[0])
    grad, val, curv = spat_want(x, g0, p0, p1, COEF, DELTA, kind)
    return dict(shape=shape, kind=kind, x=x, g0=g0, p0=p0, p1=p1, grad=grad, val=float(val.sum()), curv=curv.sum(axis=0))


def check_maps(c, out, val, curv, bound):
    """the measures of test_gpu_potentials.test_map_kernels_match_numpy and the worst template and element, all under ``bound``
    (ten times the Huber gradient's own error on the 5 x 72 x 77 plan, inside (1e-9, 1e-5))"""
    assert 1e-9 < bound < 1e-5 and out.shape == c["shape"] and np.isfinite(out).all()
    e = dict(grad=rel(out, c["grad"]), template=slice_err(out, c["grad"], 0)[0], element=max_err(out, c["grad"]),
             phi=abs(val - c["val"]) / c["val"], curv=curv_err(curv, c["curv"]))
    assert max(e.values()) < bound, (c["kind"], e, bound)
    return e


def maps_restated(c, fault=None):
    """huber_grad_kernel and huber_curv_kernel element by element as the kernels index them (flat e -> template base, pixel,
    circular neighbours): (out fp32, sum phi, curv [3]).  Faults: "beyond_cap"; "stale_base": an element of the last template on
    the second trip takes the base of the template the trip began in."""
    T, na, nb = c["shape"]
    kind, npix, n = c["kind"], na * nb, T * na * nb
    first = geometry("huber_maps", T, na, nb)[0] * TPB
    e = np.arange(n)
    t, p = e // npix, e % npix
    if fault == "stale_base":
        assert first < n and first // npix < T - 1
        t = np.where((e >= first) & (t == T - 1), first // npix, t)
    base, i, j = t * npix, p // nb, p % nb
    nbr = dict(c=p, im=np.where(i == 0, na - 1, i - 1) * nb + j, ip=np.where(i == na - 1, 0, i + 1) * nb + j,
               jm=i * nb + np.where(j == 0, nb - 1, j - 1), jp=i * nb + np.where(j == nb - 1, 0, j + 1))
    at = lambda v, k: v.astype(np.float64).ravel()[base + nbr[k]]  # noqa: E731
    x = c["x"]
    cc = at(x, "c")
    ur, uc, urn, ucn = at(x, "im") - cc, at(x, "jm") - cc, cc - at(x, "ip"), cc - at(x, "jp")
    dphi = lambda u: P.dphi(u, DELTA, kind)  # noqa: E731
    out = c["g0"].astype(np.float64).ravel() + COEF * ((dphi(urn) - dphi(ur)) + (dphi(ucn) - dphi(uc)))
    phi = P.phi(ur, DELTA, kind) + P.phi(uc, DELTA, kind)
    wr, wc = P.weight(ur, DELTA, kind), P.weight(uc, DELTA, kind)
    d = {k: (at(c[k], "im") - at(c[k], "c"), at(c[k], "jm") - at(c[k], "c")) for k in ("p0", "p1")}
    curv = np.stack([wr * d[u][0] * d[v][0] + wc * d[u][1] * d[v][1] for u, v in (("p0", "p0"), ("p0", "p1"), ("p1", "p1"))])
    done = np.ones(n, dtype=bool)
    if fault == "beyond_cap":
        done[first:] = False
    else:
        assert fault in (None, "stale_base")
    out = np.where(done, out, c["g0"].ravel()).astype(np.float32).reshape(c["shape"])
    return out, float(phi[done].sum()), curv[:, done].sum(axis=1)


# ---- cube: huber_vox_grad_kernel, huber_vox_curv_kernel ---------------------------------------------------------------------------
VOX = dict(cs=0.7, ds=0.3, cl=0.4, dl=0.4)           # the coefficients and thresholds of test_gpu_vox._check_kernels


def vox_arrays(shape, ds, seed):
    """the arrays of test_gpu_vox._check_kernels: x with differences on both sides of both thresholds, g0, p0, p1"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 2 * ds).astype(np.float32)
    g0, p0, p1 = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    return x, g0, p0, p1


@functools.lru_cache(maxsize=None)
def vox_arrays_of(shape):
    return vox_arrays(shape, VOX["ds"], 70 + shape[0])


@functools.lru_cache(maxsize=None)
def vox_case(shape, ks="huber", kl="huber"):
    x, g0, p0, p1 = vox_arrays_of(shape)
    wg, wv, wc = spat_want(x, g0, p0, p1, VOX["cs"], VOX["ds"], ks)
    lg, lv, lc = spec_want(x, p0, p1, VOX["cl"], VOX["dl"], kl)
    x64 = x.astype(np.float64)
    shares = (float(np.mean(np.abs(np.concatenate([d(x64).ravel() for d, _ in SPAT])) > VOX["ds"])),
              float(np.mean(np.abs(vo.diff_l(x64)) > VOX["dl"])))
    return dict(shape=shape, ks=ks, kl=kl, x=x, g0=g0, p0=p0, p1=p1, grad=wg + lg, vals=np.array([wv.sum(), lv]),
                curv=np.stack([wc.sum(axis=0), lc]), shares=shares)


def check_vox(c, out, vals, curv):
    """the 1e-6 gates of test_gpu_vox._check_kernels on the gradient, the two sums of phi and the two curvature blocks, and the
    same gate on the worst plane and the worst element; the corners of the first and the last plane entry by entry, as there"""
    Lc, Na, Nb = c["shape"]
    want = c["grad"]
    assert all(0.1 < s < 0.9 for s in c["shares"]), c["shares"]
    assert out.shape == c["shape"] and np.isfinite(out).all() and np.asarray(curv).shape == (2, 3)
    plane, at = slice_err(out, want, 0)
    e = dict(grad=rel(out, want), plane=plane, plane_at=at, element=max_err(out, want),
             phi_s=abs(vals[0] - c["vals"][0]) / c["vals"][0], phi_l=abs(vals[1] - c["vals"][1]) / c["vals"][1],
             curv_s=curv_err(curv[0], c["curv"][0]), curv_l=curv_err(curv[1], c["curv"][1]))
    assert max(v for k, v in e.items() if k != "plane_at") < GATE, e
    for l in (0, Lc - 1):
        for idx in [(l, 0, 0), (l, Na - 1, 0), (l, 0, Nb - 1), (l, Na - 1, Nb - 1)]:
            assert abs(out[idx] - want[idx]) < 1e-5 * (1 + abs(want[idx]))
    return e


def vox_restated(c, fault=None):
    """The march of huber_vox.hip in float64, plane by plane inside every chunk with the carried values as the kernels carry them
    (grad: the centre c, phi' of the difference behind it vprev; curv: the centres of x, p0, p1): (out fp32, vals [2], curv
    [2, 3]).  Faults: "vprev_dropped" (0 carried into the interior planes of a chunk), "c_stuck" (the centres not advanced),
    "halo_again" (the halo plane's term added on the interior planes too), "beyond_cap" (no second trip over the pixels)."""
    assert fault in (None, "vprev_dropped", "c_stuck", "halo_again", "beyond_cap")
    Lc, Na, Nb = c["shape"]
    ks, kl, cs, ds, cl, dl = c["ks"], c["kl"], VOX["cs"], VOX["ds"], VOX["cl"], VOX["dl"]
    gx, gy, _, _ = geometry("huber_vox", Lc, Na, Nb)
    x, g0, a, b = (c[k].astype(np.float64) for k in ("x", "g0", "p0", "p1"))
    done = np.ones(Na * Nb, dtype=bool)
    if fault == "beyond_cap":
        assert gx * TPB < Na * Nb
        done[gx * TPB:] = False
    done = done.reshape(Na, Nb)
    up, lf = (lambda v: np.roll(v, 1, 0)), (lambda v: np.roll(v, 1, 1))           # v[i-1][j], v[i][j-1]
    dn, rt = (lambda v: np.roll(v, -1, 0)), (lambda v: np.roll(v, -1, 1))
    out, vals, curv = g0.copy(), np.zeros(2), np.zeros((2, 3))
    for l0, l1 in chunks(Lc, gy):
        # the gradient kernel
        cen = x[l0]
        halo = P.dphi(cen - x[l0 - 1], dl, kl) if l0 > 0 else np.zeros((Na, Nb))
        vprev = halo
        for l in range(l0, l1):
            pl = x[l]
            nxt, vown = np.zeros((Na, Nb)), np.zeros((Na, Nb))
            if l < Lc - 1:
                nxt = x[l + 1]
                vown = P.dphi(nxt - cen, dl, kl)
                vals[1] += np.sum(P.phi(nxt - cen, dl, kl)[done])
            ur, uc, urn, ucn = up(pl) - cen, lf(pl) - cen, cen - dn(pl), cen - rt(pl)
            pgs = (P.dphi(urn, ds, ks) - P.dphi(ur, ds, ks)) + (P.dphi(ucn, ds, ks) - P.dphi(uc, ds, ks))
            g = g0[l] + cs * pgs + cl * (vprev - vown)
            if fault == "halo_again" and l > l0:
                g = g + cl * halo
            out[l] = np.where(done, g, g0[l])
            vals[0] += np.sum((P.phi(ur, ds, ks) + P.phi(uc, ds, ks))[done])
            vprev = np.zeros((Na, Nb)) if fault == "vprev_dropped" else vown
            if fault != "c_stuck":
                cen = nxt
        # the curvature kernel
        cen, ac, bc = x[l0], a[l0], b[l0]
        for l in range(l0, l1):
            wr, wc = P.weight(up(x[l]) - cen, ds, ks), P.weight(lf(x[l]) - cen, ds, ks)
            ar, acl, br, bcl = up(a[l]) - ac, lf(a[l]) - ac, up(b[l]) - bc, lf(b[l]) - bc
            curv[0] += [np.sum((wr * ar * ar + wc * acl * acl)[done]), np.sum((wr * ar * br + wc * acl * bcl)[done]),
                        np.sum((wr * br * br + wc * bcl * bcl)[done])]
            cn, an, bn = np.zeros((Na, Nb)), np.zeros((Na, Nb)), np.zeros((Na, Nb))
            if l < Lc - 1:
                cn, an, bn = x[l + 1], a[l + 1], b[l + 1]
                wl, al, bl = P.weight(cn - cen, dl, kl), an - ac, bn - bc
                curv[1] += [np.sum((wl * al * al)[done]), np.sum((wl * al * bl)[done]), np.sum((wl * bl * bl)[done])]
            if fault != "c_stuck":
                cen, ac, bc = cn, an, bn
    return out.astype(np.float32), vals, curv


FAULTS = ("vprev_dropped", "c_stuck", "halo_again", "beyond_cap", "no_tail", "grid_count_partials", "stale_base")
