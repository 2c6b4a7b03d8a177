"""The edge cases of tests/shepard_cases.py on the CPU: the layout restatement shows that each case reaches the branch of
the cell list it is named for, the float32 replica and the float64 checker agree with the reference's kernel on them
(tests/golden/shepard_edges.npz), and the reference's own neighbour counts keep the GPU tests from being vacuous.

Where the reference surprised: a NaN or infinite value spoils only the query points that have it within the cutoff
(the replica's matrix product spread it to every point; it now sums over the neighbours only), a sample with a
non-finite coordinate is no one's neighbour, a non-finite query point is 0, and at epsilon = 0 a query point on a
sample gets weight exp(-alpha * 0) = 1 from it for every p > 0.  No case made the reference raise.  No GPU."""
import numpy as np
import pytest

import shepard_cases as sc
import shepard_oracle as so

f32 = np.float32


@pytest.fixture(scope="module")
def z0():
    return np.load(so.GOLDEN)


@pytest.fixture(scope="module")
def z():
    return np.load(sc.GOLDEN_EDGES)


@pytest.fixture(scope="module")
def cases(z0):
    return sc.fixture_cases(z0)


NAMES = list(sc.fixture_cases(np.load(so.GOLDEN)))


def _layout(c):
    return sc.layout(c["a"], c["l"], c["ares"], c["lres"], c["cutoff"])


def _counts(c, cutoff=None):
    return so.neighbour_mask(c["a"], c["l"], c["ga"], c["gl"], c["ares"], c["lres"],
                             c["cutoff"] if cutoff is None else cutoff, c["eps"]).sum(axis=1)


def test_fixture_holds_the_cases(z, cases):
    """shepard_edges.npz is what make_golden_shepard_edges.py writes for today's case builders: arrays only, every
    case, the builders' inputs bit for bit."""
    import os
    assert os.path.getsize(sc.GOLDEN_EDGES) < os.path.getsize(so.GOLDEN)
    assert list(z["names"]) == NAMES and len(z["raised"]) == 0
    assert all(z[k].dtype != object for k in z.files)
    for name, c in cases.items():
        r = sc.load_reference(z, name)
        for k in ("a", "l", "v", "ga", "gl"):
            assert r[k].dtype == np.float32 and np.array_equal(r[k], c[k], equal_nan=True), (name, k)
        assert [r[k] for k in sc.PAR] == [c[k] for k in sc.PAR], name
        assert r["out"].shape == c["ga"].shape and r["out"].dtype == np.float32


@pytest.mark.parametrize("name", NAMES)
def test_replica_and_checker_match_reference_kernel(z, cases, name):
    c, ref = cases[name], sc.load_reference(z, name)["out"].ravel().astype(np.float64)
    args = (c["a"], c["l"], c["v"], c["ga"], c["gl"])
    out, n = so.replica(*args, c["p"], c["cutoff"], c["ares"], c["lres"], alpha=c["alpha"], epsilon=c["eps"])
    mask = so.neighbour_mask(c["a"], c["l"], c["ga"], c["gl"], c["ares"], c["lres"], c["cutoff"], c["eps"])
    chk = so.checker(*args, mask, c["p"], c["cutoff"], c["ares"], c["lres"], alpha=c["alpha"], epsilon=c["eps"])
    fin = np.isfinite(ref)
    for got in (out, chk):                               # NaN and inf exactly where the reference has them
        assert np.array_equal(got[~fin], ref[~fin], equal_nan=True) and np.isfinite(got[fin]).all()
    scale = np.abs(c["v"][np.isfinite(c["v"])]).max()
    assert np.max(np.abs(out[fin] - ref[fin]), initial=0.0) <= 1e-6 * scale
    assert np.max(np.abs(chk[fin] - ref[fin]), initial=0.0) <= 1e-6 * scale
    if np.isfinite(c["v"]).all():
        assert np.array_equal(ref == 0, n == 0)          # exactly the points without a neighbour are 0
    else:
        assert np.all(ref[n == 0] == 0)


@pytest.mark.parametrize("variant", ["cutoff1", "cutoff1e-3", "two"])
def test_sparse_clusters_coarsen_the_cells(variant):
    c = sc.sparse_clusters(variant)
    lay = _layout(c)
    # 5003 x 7003 units at h0 = cutoff * 65/64 against a cap of 4 nv + 1024 cells
    assert lay["doublings"] == {"cutoff1": 8, "cutoff1e-3": 18, "two": 8}[variant]
    assert (lay["nx"], lay["ny"]) == {"cutoff1": (20, 27), "cutoff1e-3": (19, 27), "two": (20, 27)}[variant]
    assert lay["nx"] * lay["ny"] <= 4 * c["a"].size + 1024 and lay["n_binned"] == c["a"].size
    n = _counts(c)
    assert np.mean(n > 0) >= 0.5 and np.mean(n == 0) >= 0.1
    if variant == "cutoff1":
        assert c["ga"].size == 120 and n.max() >= 8


def test_dense_cells_are_long():
    c = sc.dense_cells()
    lay = _layout(c)
    assert (lay["nx"], lay["ny"], lay["doublings"]) == (2, 2, 0) and lay["occupancy"].max() > 2 * sc.SORT_MAX
    assert 0 < lay["occupancy"].min() <= sc.SORT_MAX     # a long cell next to three short ones: both sorts in one call
    assert np.mean(_counts(c) > 0) >= 0.5
    g = sc.dense_cells(grid=True)
    assert np.array_equal(g["a"], c["a"]) and np.array_equal(g["v"], c["v"]) and g["ga"].shape == (8, 8)
    assert np.array_equal(g["ga"], np.meshgrid(g["ga"][0], g["gl"][:, 0])[0])


@pytest.mark.parametrize("n", sc.STACK_SIZES)
def test_coincident_stack(n):
    c = sc.coincident_stack(n)
    lay = _layout(c)
    assert lay["occupancy"].max() == n and c["stack"].sum() == n
    assert (lay["occupancy"].max() > sc.SORT_MAX) == (n != 64)      # 64 is the longest cell of the short path
    assert not c["stack"][0] and not c["stack"][-1] and np.sort(lay["occupancy"].ravel())[-2] <= 8
    # each weight of the stack is float32(1), and nothing else is within the cutoff
    dist = so.pair_distance(c["a"], c["l"], c["ga"], c["gl"], 1.0, 1.0)[0]
    assert np.array_equal(dist <= 1.0, c["stack"]) and dist[~c["stack"]].min() > 3.0
    df = dist[c["stack"]].astype(f32).astype(np.float64)
    w = np.exp((-2.0 * np.exp(2.0 * np.log(df))).astype(f32).astype(np.float64)).astype(f32)
    assert w.dtype == f32 and np.all(w == f32(1)) and np.all(df == np.float64(f32(1e-6)))
    out, cnt = so.replica(c["a"], c["l"], c["v"], c["ga"], c["gl"], 2.0, 1.0, 1.0, 1.0)
    want = sc.stack_expected(c)
    assert cnt[0] == n and abs(out[0] - want) <= 1e-6 * np.abs(c["v"]).max()
    # the order of the additions shows in the bits
    v = c["v"][c["stack"]]
    s0 = np.add.accumulate(v, dtype=f32)[-1]
    rng = np.random.default_rng(n)
    for _ in range(20):
        assert np.add.accumulate(v[rng.permutation(n)], dtype=f32)[-1] != s0


@pytest.mark.parametrize("variant", list(sc.EDGE_VARIANTS))
def test_cell_edges_sit_on_the_edges(variant):
    c = sc.cell_edges(variant)
    lay = _layout(c)
    assert lay["doublings"] == 0 and (lay["nx"], lay["ny"]) == (6, 6)
    # some float32(j h) and its two float32 neighbours fall into different cells
    split = 0
    for x in c["xs"][1:]:
        lo, hi = np.nextafter(x, f32(-np.inf)), np.nextafter(x, f32(np.inf))
        cx = {int(lay["cx"][np.nonzero(c["a"] == t)[0][0]]) for t in (lo, x, hi)}
        split += len(cx) > 1
    assert split >= 1
    n = _counts(c)
    assert np.mean(n > 0) >= 0.5 and np.mean(n == 0) >= 0.1
    # the decision at the cutoff is live: the neighbouring cutoff changes counts
    assert np.any(n != _counts(c, sc.EDGE_VARIANTS[variant][1]))


def test_wide_strip_needs_double_cell_coordinates():
    c = sc.wide_strip()
    lay = _layout(c)
    assert lay["doublings"] == 0 and lay["ny"] == 1 and 2 ** 19 < lay["nx"] <= 4 * c["a"].size + 1024
    assert c["crafted"].sum() == 40 and c["near"][c["crafted"]].all() and c["near"].sum() < 2000
    # the float32 quotient puts each crafted sample one cell too high ...
    cx = lay["cx"][c["crafted"]]
    cx32 = np.floor(c["a"][c["crafted"]] / f32(lay["h"])).astype(np.int64)
    assert f32(lay["h"]) == lay["h"] and np.array_equal(cx32, cx + 1)
    # ... which is two cells above the query point one cutoff below it, its neighbour by d = 1 <= cutoff
    fx = np.floor(c["ga"][0].astype(np.float64) / lay["h"]).astype(np.int64)
    assert np.array_equal(np.sort(cx) - fx, np.full(40, 1))
    d = so.pair_distance(np.sort(c["a"][c["crafted"]]), np.zeros(40), c["ga"][0], np.zeros(40), 1.0, 1.0, 0.0)
    assert np.all(np.diag(d) == 1.0)
    # the samples more than 3 units from every query point are no one's neighbour: the rest decide the counts
    n = so.neighbour_mask(c["a"][c["near"]], c["l"][c["near"]], c["ga"], c["gl"], 1.0, 1.0, 1.0, 0.0).sum(axis=1)
    n = n.reshape(4, 40)
    assert np.all(n[0] >= 1) and np.all(n[1] >= 1) and np.mean(n == 0) >= 0.1


def test_lattice_cutoffs_straddle_the_distances():
    sets = []
    for cut, want in zip(sc.LATTICE_CUTOFFS, sc.LATTICE_COUNTS):
        c = sc.lattice_cutoffs(cut)
        n = _counts(c)
        assert set(n.tolist()) == want, cut
        assert _layout(c)["doublings"] == 0
        sets.append(want)
    changes = [a != b for a, b in zip(sets, sets[1:])]
    assert changes == [False, True, False, True, False, True]


def test_non_finite_case(z0):
    c, e = sc.non_finite(z0), sc.non_finite(z0, everything=True)
    n = c["a"].size
    lay = _layout(c)
    assert np.isnan(c["a"]).sum() == n // 10 and np.isposinf(c["l"]).sum() == np.isneginf(c["l"]).sum() == n // 20
    assert lay["n_binned"] == n - n // 5 and (lay["cx"] < 0).sum() == n // 5 and lay["nx"] > 0
    ok = np.isfinite(c["a"]) & np.isfinite(c["l"])
    assert np.isnan(c["v"][ok]).sum() == n // 20 and np.isposinf(c["v"][ok]).sum() == 1
    assert (~(np.isfinite(c["ga"]) & np.isfinite(c["gl"]))).sum() == 4
    le = _layout(e)
    assert (le["nx"], le["ny"], le["n_binned"]) == (0, 0, 0)


def test_parameter_variants(z0):
    seen = set()
    for k in sc.PARAMETER_VARIANTS:
        c = sc.parameters(z0, k)
        seen.add((c["p"], c["alpha"], c["eps"], c["ares"], c["lres"]))
        if c["eps"] == 0.0 and k in sc.PARAMETER_GRID:      # two query points on samples: d + eps = 0
            d = so.pair_distance(c["a"], c["l"], c["ga"], c["gl"], c["ares"], c["lres"], 0.0)
            assert (d.min(axis=1) == 0).sum() == 2
    assert len(seen) == 10 and (2.0, 2.0, 1e-6, -1.0, 1.0) in seen and (2.0, 2.0, 1e-6, 0.7, 2.1) in seen
    assert {s[:3] for s in seen if s[3:] == (1.0, 1.0)} == {(p, a, e) for p in (0.5, 3.0) for a in (0.5, 8.0)
                                                             for e in (0.0, 1e-3)}


def test_ragged_batch_layout(z0):
    segs = sc.ragged_batch(z0)
    kinds = [k for k, _ in segs]
    empty = ("no_samples", "no_columns", "no_rows")
    assert len(segs) == 40 and set(kinds) == set(sc.RAGGED_KINDS)
    assert kinds[0] in empty and kinds[-1] in empty and kinds[19] in empty and kinds[20] in empty
    for kind, s in segs:
        assert all(np.asarray(x).dtype == np.float32 for x in s[:5])
        if kind == "dense":
            assert sc.layout(s[0], s[1], s[5], s[6], 2.0)["occupancy"].max() > sc.SORT_MAX
        if kind == "sparse":
            assert sc.layout(s[0], s[1], s[5], s[6], 2.0)["doublings"] >= 1
        if kind == "no_samples":
            assert s[0].size == 0 and (s[4].size, s[3].size) == (3, 4)
        if kind == "no_columns":
            assert s[0].size == 5 and (s[4].size, s[3].size) == (4, 0)
        if kind == "no_rows":
            assert s[0].size == 5 and (s[4].size, s[3].size) == (0, 4)
