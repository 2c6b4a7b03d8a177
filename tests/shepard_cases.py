"""Edge cases of the Shepard resampler's cell list (surfh_amd/csrc/shepard.hip) and a NumPy restatement of its layout.

``layout`` restates k_seg_setup and k_bin: the cell grid of one segment (``nx``, ``ny``, ``h``, the number of times ``h``
doubled) and the cell of every sample.  It is a model of the layout only, there to prove on the CPU that a case reaches
the branch it is named for; expected values come from shepard_oracle (replica, neighbour_mask, checker) and from the
reference's outputs in tests/golden/shepard_edges.npz (tests/golden/make_golden_shepard_edges.py runs the reference on
``fixture_cases``).

A case is a dict: ``a``, ``l``, ``v`` (float32 samples), ``ga``, ``gl`` (float32 2-D query meshes of one shape), ``p``,
``alpha``, ``cutoff``, ``eps``, ``ares``, ``lres``."""
from __future__ import annotations

import os

import numpy as np

import shepard_oracle as so

f32, f64 = np.float32, np.float64
GOLDEN_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shepard_edges.npz")
SORT_MAX = 64                        # shepard.hip: cells longer than this are sorted by k_long_sort
PAR = ("p", "alpha", "cutoff", "eps", "ares", "lres")
STACK_SIZES = (64, 65, 200, 1500, 4096)
# seeds of the stacks' values: of a short stack's 20 test permutations a quarter may leave the float32 sum's bits alone
# (a few large values dominate it), so the seeds are the first from 300 + n on at which all 20 change them
STACK_SEEDS = {64: 366, 65: 365, 200: 501, 1500: 1800, 4096: 4396}
LATTICE_CUTOFFS = (1.0, 1.000001, 1.0000011, 1.4142135, 1.4142147, 2.0, 2.0000012)
# the neighbour-count sets of lattice_cutoffs: d + eps <= cutoff decides by one ulp between 1.000001 and 1.0000011
# (d = 1), between 1.4142135 and 1.4142147 (d = sqrt 2) and between 2.0 and 2.0000012 (d = 2)
LATTICE_COUNTS = ({0, 1}, {0, 1}, {0, 1, 3, 4, 5}, {0, 1, 3, 4, 5}, {1, 2, 3, 4, 6, 9}, {1, 2, 3, 4, 6, 9},
                  {1, 3, 4, 6, 8, 9, 11, 12, 13})


def layout(a, l, ares, lres, cutoff):
    """k_seg_setup and k_bin of one segment: dict with nx, ny, h, doublings, cx, cy (per sample, -1: not binned),
    occupancy (per cell, row-major [ny, nx]) and n_binned."""
    a, l = np.asarray(a, f32).ravel(), np.asarray(l, f32).ravel()
    ok = np.isfinite(a) & np.isfinite(l)
    ia, il = abs(f64(so.inv_res(ares))), abs(f64(so.inv_res(lres)))
    cx = np.full(a.size, -1, np.int64)
    cy = np.full(a.size, -1, np.int64)
    r = dict(nx=0, ny=0, h=0.0, doublings=0, cx=cx, cy=cy, occupancy=np.zeros((0, 0), np.int64), n_binned=0)
    nv = int(ok.sum())
    if nv == 0 or not (np.isfinite(ia) and np.isfinite(il)):
        return r
    af, lf = a[ok].astype(f64), l[ok].astype(f64)
    a0, l0 = af.min(), lf.min()
    sx, sy = (af.max() - a0) * ia, (lf.max() - l0) * il
    h = max(f64(f32(cutoff)), 1e-30) * (1.0 + 1.0 / 64)
    cap = 4.0 * nv + 1024.0
    n = 0
    while (np.floor(sx / h) + 1.0) * (np.floor(sy / h) + 1.0) > cap:
        h *= 2.0
        n += 1
    nx, ny = int(np.floor(sx / h)) + 1, int(np.floor(sy / h)) + 1
    cx[ok] = np.clip(np.floor((af - a0) * ia / h), 0, nx - 1).astype(np.int64)
    cy[ok] = np.clip(np.floor((lf - l0) * il / h), 0, ny - 1).astype(np.int64)
    occ = np.bincount(cy[ok] * nx + cx[ok], minlength=nx * ny).reshape(ny, nx)
    r.update(nx=nx, ny=ny, h=h, doublings=n, occupancy=occ, n_binned=nv)
    return r


def _case(a, l, v, ga, gl, p=2.0, alpha=2.0, cutoff=1.0, eps=1e-6, ares=1.0, lres=1.0):
    ga, gl = np.asarray(ga, f32), np.asarray(gl, f32)
    if ga.ndim == 1:
        ga, gl = ga[None, :], gl[None, :]
    c = lambda x: np.ascontiguousarray(np.asarray(x, f32).ravel())  # noqa: E731
    return dict(a=c(a), l=c(l), v=c(v), ga=np.ascontiguousarray(ga), gl=np.ascontiguousarray(gl), p=float(p),
                alpha=float(alpha), cutoff=float(f32(cutoff)), eps=float(eps), ares=float(ares), lres=float(lres))


def wide_values(rng, n):
    """Values over seven decades: a float32 sum of them depends on the order of the additions."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(f32)


CLUSTERS = ((0.0, 0.0), (5000.0, 7000.0), (0.0, 7000.0))


def sparse_clusters(variant="cutoff1"):
    """Three clusters of 20 samples, 3 units wide, in a 5003 x 7003 box: the cell side doubles until the grid fits the
    cap of 4 nv + 1024 cells.  ``cutoff1``: cutoff 1, 120 query points over and just outside two clusters;
    ``cutoff1e-3``: cutoff 1e-3 (one float32 ulp is 4.9e-4 at 7000), query points next to samples; ``two``: two
    samples at opposite corners."""
    rng = np.random.default_rng(101)
    if variant == "two":
        a, l = np.array([0.25, 5000.5]), np.array([0.75, 7001.25])
        v = np.array([3.0, -0.125])
        th = rng.uniform(0, 2 * np.pi, 24)
        r = np.concatenate([rng.uniform(0, 0.9, 16), rng.uniform(1.2, 4.0, 8)])
        k = np.arange(24) % 2
        return _case(a, l, v, a[k] + r * np.cos(th), l[k] + r * np.sin(th))
    a = np.concatenate([cx + rng.uniform(0, 3, 20) for cx, _ in CLUSTERS])
    l = np.concatenate([cy + rng.uniform(0, 3, 20) for _, cy in CLUSTERS])
    v = rng.standard_normal(60)
    if variant == "cutoff1":
        qa = np.concatenate([cx + rng.uniform(-1, 4, 60) for cx, _ in CLUSTERS[:2]])
        ql = np.concatenate([cy + rng.uniform(-1, 4, 60) for _, cy in CLUSTERS[:2]])
        return _case(a, l, v, qa, ql)
    assert variant == "cutoff1e-3"
    k = np.arange(120) % 60
    th = rng.uniform(0, 2 * np.pi, 120)
    r = np.where(np.arange(120) < 84, 2.5e-4, 3e-3)       # 84 points a quarter of a cutoff from a sample, 36 three cutoffs
    return _case(a, l, v, a[k] + r * np.cos(th), l[k] + r * np.sin(th), cutoff=1e-3)


def dense_cells(grid=False):
    """300 samples in [0, 3]^2 at cutoff 2: 2 x 2 cells of side 2.03, the first of them far longer than SORT_MAX.  64 query points in the square
    (``grid``: the 8 x 8 grid of the separable axes ``ga[0]``, ``gl[:, 0]``)."""
    rng = np.random.default_rng(202)
    a, l, v = rng.uniform(0, 3, 300), rng.uniform(0, 3, 300), wide_values(rng, 300)
    if grid:
        ga, gl = np.meshgrid(np.linspace(0.1, 2.9, 8), np.linspace(0.05, 2.95, 8))
    else:
        ga, gl = rng.uniform(0, 3, 64), rng.uniform(0, 3, 64)
    return _case(a, l, v, ga, gl, cutoff=2.0)


def coincident_stack(n):
    """``n`` samples at one point and 8 more than 3 cutoffs away, spread through the input; one query at the point.
    Every weight is (float) exp((float)(-2 (1e-6)^2)) = 1, so out = (float32 sum of v in kernel order) / n."""
    rng = np.random.default_rng(STACK_SEEDS[n])
    at = np.sort(rng.choice(n + 8, 8, replace=False))
    at[0], at[-1] = 0, n + 7                              # the input begins and ends with a far sample
    far = np.zeros(n + 8, bool)
    far[at] = True
    a, l = np.full(n + 8, 1.5), np.full(n + 8, 2.5)
    th = np.arange(8) * (2 * np.pi / 8)
    a[far], l[far] = 1.5 + (4.0 + np.arange(8)) * np.cos(th), 2.5 + (4.0 + np.arange(8)) * np.sin(th)
    v = wide_values(rng, n + 8)
    c = _case(a, l, v, [1.5], [2.5])
    c["stack"] = ~far
    return c


def stack_expected(c):
    """The float32 sequential sum of the stack's values in input order, divided by their number."""
    v = c["v"][c["stack"]]
    return f32(np.add.accumulate(v, dtype=f32)[-1] / f32(v.size))


def _triples(x):
    x = np.asarray(x, f32)
    return np.stack([np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))], axis=1).ravel()


# cell_edges variants: (cutoff, the neighbouring cutoff its counts are compared with, epsilon)
EDGE_VARIANTS = {"c1_eps0": (1.0, float(np.nextafter(f32(1), f32(2))), 0.0),
                 "c1up_eps0": (float(np.nextafter(f32(1), f32(2))), 1.0, 0.0),
                 "c1": (1.0, 1.000001, 1e-6),
                 "c2": (2.0, 2.0000012, 1e-6),
                 "sky": (2.0, 2.25, 1e-6)}           # one float32 ulp of alpha is 0.16 pixel there: no one-ulp straddle
SKY = dict(a0=83.8221, ares=4.7e-5, l0=4.9, lres=8e-4)


def cell_edges(variant):
    """Samples at float32(j h), j = 0..5, and its two float32 neighbours along one axis (at float32(j h) along the
    other), h = float32(cutoff) (1 + 1/64) the cell side: k_bin's floor decides between two cells within one ulp.
    Query points at the samples, one cutoff away along alpha, along lambda and along the diagonal, and seven cutoffs
    away (no neighbour).  ``sky``: the
    same in the fixture's absolute coordinates (alpha = 83.8221 + x * 4.7e-5, lambda = 4.9 + y * 8e-4)."""
    cutoff, _, eps = EDGE_VARIANTS[variant]
    h = f64(f32(cutoff)) * (1.0 + 1.0 / 64)
    j = np.arange(6) * h
    if variant == "sky":
        xs, ys = f32(SKY["a0"] + j * SKY["ares"]), f32(SKY["l0"] + j * SKY["lres"])
        sa, sl, ares, lres = cutoff * SKY["ares"], cutoff * SKY["lres"], SKY["ares"], SKY["lres"]
    else:
        xs = ys = j.astype(f32)
        sa = sl = f64(f32(cutoff))
        ares = lres = 1.0
    pts = [(x, y) for x in _triples(xs) for y in ys] + [(x, y) for x in xs for y in _triples(ys)]
    pts = np.unique(np.array(pts, f32), axis=0)
    a, l = pts[:, 0], pts[:, 1]
    v = np.random.default_rng(404).standard_normal(a.size)
    s = np.sqrt(0.5)
    qa = np.concatenate([a, f32(a.astype(f64) + sa), a, f32(a.astype(f64) + s * sa), f32(a.astype(f64) + 7 * sa)])
    ql = np.concatenate([l, l, f32(l.astype(f64) + sl), f32(l.astype(f64) + s * sl), l])
    c = _case(a, l, v, qa.reshape(5, -1), ql.reshape(5, -1), cutoff=cutoff, eps=eps, ares=ares, lres=lres)
    c["xs"] = np.asarray(xs, f32)
    return c


def lattice_cutoffs(cutoff):
    """Samples on the 7 x 7 integer lattice, query points on the 9 x 9 lattice from -1 to 7: every distance is 0, 1,
    sqrt 2, 2, ... and the cutoffs of LATTICE_CUTOFFS straddle d + eps at 1, sqrt 2 and 2 by one float32 ulp."""
    a, l = (m.ravel() for m in np.meshgrid(np.arange(7.0), np.arange(7.0)))
    v = np.random.default_rng(505).standard_normal(49)
    ga, gl = np.meshgrid(np.arange(-1.0, 8.0), np.arange(-1.0, 8.0))
    return _case(a, l, v, ga, gl, cutoff=cutoff)


STRIP_SAMPLES = 132000


def wide_strip():
    """A strip of 2^19 cells along alpha (cutoff 1, epsilon 0, all lambdas 0): the one shape at which a float32 cell
    coordinate is wrong by more than the 1/64 of slack in the cell side.  Beyond 2^19 units a float32 holds sixteenths;
    with h = 65/64 the sample at x = (65 t + 32) / 16 lies at x / h = 4 t + 2 - 2/65, in cell 4 t + 1, 1/32 of a unit
    below the edge, but the float32 quotient rounds to 4 t + 2.  The query point at x - 1 (d = 1 <= cutoff) lies in
    cell 4 t, so a sample binned into cell 4 t + 2 is out of its reach.  The cap of 4 nv + 1024 cells asks for 131 000
    filler samples, far more than the other cases hold; ``near`` marks the samples within 3 units of a query point
    (the others are no one's neighbour), which is all a brute-force check needs.  ``crafted``: the samples at the edges."""
    rng = np.random.default_rng(808)
    t = 131100 + 7 * np.arange(40)
    xs = (65.0 * t + 32.0) / 16.0                         # exact in float32
    fill = np.sort(rng.uniform(0, xs.max() + 2, STRIP_SAMPLES - 40)).astype(f32)
    fill[0] = 0.0                                         # the origin of the cell grid
    a = np.concatenate([fill, xs])
    order = rng.permutation(a.size)
    a = a[order]
    v = rng.standard_normal(a.size)
    qa = np.concatenate([xs - 1.0, xs, xs + 1.0, xs - 2.0])
    c = _case(a, np.zeros(a.size), v, qa.reshape(4, -1), np.zeros((4, 40)), eps=0.0)
    assert np.array_equal(c["ga"][1], xs)                 # float32 holds every crafted coordinate
    c["crafted"] = np.isin(c["a"], xs.astype(f32))
    q = np.sort(c["ga"].ravel().astype(f64))
    k = np.clip(np.searchsorted(q, c["a"].astype(f64)), 1, q.size - 1)
    c["near"] = np.minimum(np.abs(c["a"] - q[k - 1]), np.abs(c["a"] - q[k])) <= 3.0
    return c


def _fixture_case(z0, i):
    c = so.kernel_cases(z0)[i]
    return _case(c["a"], c["l"], c["v"], c["ga"], c["gl"], p=c["p"], cutoff=c["cutoff"], ares=c["ares"], lres=c["lres"])


def non_finite(z0, everything=False):
    """Case 0 of shepard.npz with 10 % of the sample alphas NaN, 5 % of the lambdas +inf and 5 % -inf, 5 % of the
    values NaN at finite coordinates, one value +inf and four query points NaN / +-inf.  ``everything``: no sample
    has two finite coordinates."""
    c = _fixture_case(z0, 0)
    rng = np.random.default_rng(606)
    n = c["a"].size
    pick = rng.permutation(n)
    c["a"][pick[:n // 10]] = np.nan
    c["l"][pick[n // 10:n // 10 + n // 20]] = np.inf
    c["l"][pick[n // 10 + n // 20:n // 5]] = -np.inf
    c["v"][pick[n // 5:n // 5 + n // 20]] = np.nan
    # +inf goes to a sample that some query point sees without a NaN value beside it, so that an infinite output exists
    m = so.neighbour_mask(c["a"], c["l"], c["ga"], c["gl"], c["ares"], c["lres"], c["cutoff"], c["eps"])
    clean = m[~(m & np.isnan(c["v"])[None, :]).any(axis=1)].any(axis=0)
    c["v"][next(k for k in pick[n // 5 + n // 20:] if clean[k])] = np.inf
    if everything:
        c["a"][pick[n // 5::2]] = np.nan
        c["l"][pick[n // 5 + 1::2]] = -np.inf
    ga, gl = c["ga"].ravel(), c["gl"].ravel()
    q = rng.choice(ga.size, 4, replace=False)
    ga[q[0]], gl[q[1]], ga[q[2]], gl[q[3]] = np.nan, np.inf, -np.inf, np.nan
    return c


PARAMETER_GRID = {f"p{p}_alpha{al}_eps{e}": (p, al, e) for p in (0.5, 3.0) for al in (0.5, 8.0) for e in (0.0, 1e-3)}
PARAMETER_VARIANTS = tuple(PARAMETER_GRID) + ("negative_ares", "anisotropic")


def parameters(z0, variant):
    """The samples and mesh of shepard.npz's case 0 with p in {0.5, 3}, alpha in {0.5, 8} and epsilon in {0, 1e-3}
    (at epsilon = 0 two query points are moved onto samples: log(0) in the weight), with alpha_res = -1, and with
    alpha_res = 0.7, lambda_res = 2.1."""
    c = _fixture_case(z0, 0)
    if variant == "negative_ares":
        c["ares"] = -1.0
    elif variant == "anisotropic":
        c["ares"], c["lres"] = 0.7, 2.1
    else:
        p, al, e = PARAMETER_GRID[variant]
        c.update(p=p, alpha=al, eps=e)
        if e == 0.0:
            c["ga"][3, 4], c["gl"][3, 4] = c["a"][17], c["l"][17]
            c["ga"][7, 9], c["gl"][7, 9] = c["a"][230], c["l"][230]
    return c


def fixture_cases(z0):
    """name -> case: what tests/golden/make_golden_shepard_edges.py runs the reference on."""
    d = {"non_finite": non_finite(z0), "non_finite_all": non_finite(z0, everything=True)}
    d.update({f"parameters_{k}": parameters(z0, k) for k in PARAMETER_VARIANTS})
    d.update({f"lattice_cutoffs_{i}": lattice_cutoffs(c) for i, c in enumerate(LATTICE_CUTOFFS)})
    d.update({f"cell_edges_{k}": cell_edges(k) for k in EDGE_VARIANTS})
    d.update({f"sparse_clusters_{k}": sparse_clusters(k) for k in ("cutoff1", "cutoff1e-3", "two")})
    d["dense_cells"] = dense_cells()
    return d


def load_reference(z, name):
    """The case ``name`` as stored in shepard_edges.npz, with the reference's output under ``out``."""
    c = {k: z[f"{name}__{k}"] for k in ("a", "l", "v", "ga", "gl", "out")}
    c.update({k: float(x) for k, x in zip(PAR, z[f"{name}__par"])})
    return c


# ragged_batch: 40 separable segments; the first, the last and two adjacent ones are the empty kinds
RAGGED_KINDS = ("no_samples", "no_columns", "no_rows", "one_sample", "dense", "sparse", "fixture2")


def ragged_batch(z0):
    """[(kind, (a, l, v, q_alpha axis, q_lambda axis, ares, lres))] of 40 segments for shepard_segments(p=2,
    pixel_cutoff=2)."""
    rng = np.random.default_rng(707)
    five = lambda: (rng.uniform(0, 3, 5), rng.uniform(0, 3, 5), rng.standard_normal(5))  # noqa: E731
    e = np.zeros(0)

    def make(kind):
        if kind == "no_samples":
            return (e, e, e, np.linspace(0, 3, 4), np.linspace(0, 2, 3), 1.0, 1.0)
        if kind == "no_columns":
            return five() + (e, np.linspace(0, 3, 4), 1.0, 1.0)
        if kind == "no_rows":
            return five() + (np.linspace(0, 3, 4), e, 1.0, 1.0)
        if kind == "one_sample":
            x, y = rng.uniform(0, 3, 2)
            return (np.array([x]), np.array([y]), np.array([2.5]), np.array([x - 3, x - 1, x, x + 0.5, x + 2.5]),
                    np.array([y - 1.5, y, y + 2.5]), 1.0, 1.0)
        if kind == "dense":
            c = dense_cells(grid=True)
            return (c["a"], c["l"], c["v"], c["ga"][0], c["gl"][:, 0], 1.0, 1.0)
        if kind == "sparse":
            c = sparse_clusters()
            return (c["a"], c["l"], c["v"], np.linspace(-1, 4, 10), np.linspace(6999, 7004, 12), 1.0, 1.0)
        c = _fixture_case(z0, 2)
        return (c["a"], c["l"], c["v"], c["ga"][0], c["gl"][:, 0], c["ares"], c["lres"])

    kinds = list(rng.choice(RAGGED_KINDS, 40))
    kinds[0], kinds[39], kinds[19], kinds[20] = "no_samples", "no_rows", "no_columns", "no_samples"
    for k, kind in zip((3, 8, 13, 25, 30, 33, 36), RAGGED_KINDS):      # every kind at least once
        kinds[k] = kind
    return [(str(k), tuple(np.asarray(x, f32) if i < 5 else x for i, x in enumerate(make(k)))) for k in kinds]
