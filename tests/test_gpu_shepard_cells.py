"""The cell list of the GPU Shepard resampler (surfh_amd/csrc/shepard.hip) on the branches that the fixture of
test_gpu_shepard.py does not reach: a coarsened cell grid, cells longer than SORT_MAX, non-finite samples and query
points, empty segments inside a batch, parameters outside the fixture's, device pointers with a caller's stream, and
the cutoff decision within one ulp of a cell edge.  The cases are those of tests/shepard_cases.py (shown on the CPU to
reach their branch by test_shepard_cases_host.py); expected values are the reference's own outputs in
tests/golden/shepard_edges.npz, the float32 replica's neighbour counts and the float64 checker.

NaN values: the reference gives NaN exactly at the query points that have a NaN sample value within the cutoff, +-inf
or NaN where an infinite one is; the kernel is held to the same places."""
import ctypes as C

import numpy as np
import pytest

import shepard_cases as sc
import shepard_oracle as so
from surfh_amd import _lib
from surfh_amd import preprocessing as P

pytestmark = pytest.mark.gpu
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


@pytest.fixture(scope="module")
def ragged(z0):
    """The 40 segments, their batched result and, per segment, the replica's counts and the float64 checker."""
    segs = sc.ragged_batch(z0)
    res, cnt = P.shepard_segments([s for _, s in segs], p=2.0, pixel_cutoff=2.0, neighbours=True)
    want = []
    for _, (a, l, v, qa, ql, ares, lres) in segs:
        ga, gl = np.meshgrid(qa, ql)
        _, n = so.replica(a, l, v, ga, gl, 2.0, 2.0, ares, lres)
        m = so.neighbour_mask(a, l, ga, gl, ares, lres, 2.0)
        want.append((n.reshape(ga.shape), so.checker(a, l, v, ga, gl, m, 2.0, 2.0, ares, lres).reshape(ga.shape)))
    return dict(segs=segs, res=res, cnt=cnt, want=want)


NAMES = list(sc.fixture_cases(np.load(so.GOLDEN)))


def _note(name, **kw):
    from test_gpu_parity import note
    print(name, kw)
    note(name, **kw)


def _run(c):
    return P.exponential_modified_shepard(c["a"], c["l"], c["v"], c["ga"], c["gl"], p=c["p"], alpha=c["alpha"],
                                          pixel_cutoff=c["cutoff"], alpha_res=c["ares"], lambda_res=c["lres"],
                                          epsilon=c["eps"], return_neighbours=True)


@pytest.mark.parametrize("name", NAMES)
def test_counts_and_values_match_reference(z, cases, name):
    c, ref = cases[name], sc.load_reference(z, name)["out"]
    out, nbr = _run(c)
    assert out.shape == ref.shape and out.dtype == np.float32
    _, n = so.replica(c["a"], c["l"], c["v"], c["ga"], c["gl"], c["p"], c["cutoff"], c["ares"], c["lres"],
                      alpha=c["alpha"], epsilon=c["eps"])
    fin = np.isfinite(ref)
    scale = float(np.abs(c["v"][np.isfinite(c["v"])]).max())
    err = float(np.max(np.abs(out[fin] - ref[fin]), initial=0.0)) / scale
    _note("shepard_cells", case=name, err_over_max_v=err, neighbours=[int(n.min()), int(n.max())],
          non_finite_outputs=int((~fin).sum()), count_mismatches=int(np.sum(nbr.ravel() != n)))
    assert np.array_equal(nbr.ravel(), n)
    assert np.array_equal(out[~fin], ref[~fin], equal_nan=True) and np.isfinite(out[fin]).all()
    assert err <= 1e-5


def test_wide_strip_keeps_neighbours_across_cell_edges():
    """2^19 cells in a row: a cell coordinate computed in float32 would put the samples just below a cell edge one cell
    too high, out of reach of the query point one cutoff below them.  No fixture entry (132 000 samples): the float32
    replica's counts and the float64 checker over the samples within 3 units of a query point."""
    c = sc.wide_strip()
    out, nbr = _run(c)
    s = c["near"]
    args = (c["a"][s], c["l"][s], c["v"][s], c["ga"], c["gl"])
    _, n = so.replica(*args, 2.0, 1.0, 1.0, 1.0, epsilon=0.0)
    m = so.neighbour_mask(c["a"][s], c["l"][s], c["ga"], c["gl"], 1.0, 1.0, 1.0, 0.0)
    chk = so.checker(*args, m, 2.0, 1.0, 1.0, 1.0, epsilon=0.0)
    err = float(np.max(np.abs(out.ravel() - chk))) / float(np.abs(c["v"]).max())
    _note("shepard_cells", case="wide_strip", err_over_max_v=err, neighbours=[int(n.min()), int(n.max())],
          count_mismatches=int(np.sum(nbr.ravel() != n)))
    assert np.array_equal(nbr.ravel(), n)
    assert err <= 1e-5


@pytest.mark.parametrize("n", sc.STACK_SIZES)
def test_full_cell_sums_in_input_order(n):
    """Every weight of the stack is float32(1): the output is the float32 sequential sum of the values in the kernel's
    order over n, so it equals NumPy's sum in input order bit for bit only if the cell is in input order."""
    c = sc.coincident_stack(n)
    out, nbr = _run(c)
    want = sc.stack_expected(c)
    print(f"stack of {n}: out {out[0, 0]!r}, input-order sum / n {want!r}")
    assert nbr[0, 0] == n
    assert out[0, 0].tobytes() == want.tobytes()


def test_long_cells_repeat_bit_for_bit():
    c = sc.dense_cells()
    runs = [_run(c) for _ in range(5)]
    rng = np.random.default_rng(11)
    front = (rng.uniform(0, 3, 100), rng.uniform(0, 3, 100), rng.standard_normal(100), np.zeros((1, 7)),
             np.ones((1, 7)), 1.0, 1.0)              # 100 samples in front: the dense samples straddle other blocks
    res, cnt = P.shepard_segments([front, (c["a"], c["l"], c["v"], c["ga"], c["gl"], 1.0, 1.0)], p=2.0, pixel_cutoff=2.0,
                                  separable=False, neighbours=True)
    runs.append((res[1], cnt[1]))
    for out, nbr in runs[1:]:
        assert np.array_equal(out, runs[0][0]) and np.array_equal(nbr, runs[0][1])


def test_ragged_batch_counts_and_values(ragged):
    worst = 0.0
    for (kind, s), out, nbr, (n, chk) in zip(ragged["segs"], ragged["res"], ragged["cnt"], ragged["want"]):
        assert out.shape == (s[4].size, s[3].size) == nbr.shape and out.dtype == np.float32 and nbr.dtype == np.int32
        assert np.array_equal(nbr, n), kind
        if s[0].size == 0:
            assert out.size == 12 and not out.any() and not nbr.any()
            continue
        err = float(np.max(np.abs(out - chk), initial=0.0)) / float(np.abs(s[2]).max())
        worst = max(worst, err)
        assert err <= 1e-5, kind
    _note("shepard_cells", case="ragged_batch", err_over_max_v=worst)


def test_ragged_batch_equals_single_calls(ragged):
    for (kind, s), out, nbr in zip(ragged["segs"], ragged["res"], ragged["cnt"]):
        one, n1 = P.shepard_segments([s], p=2.0, pixel_cutoff=2.0, neighbours=True)
        assert one[0].shape == out.shape and n1[0].shape == nbr.shape
        assert np.array_equal(one[0], out) and np.array_equal(n1[0], nbr), kind


def test_ragged_batch_with_explicit_meshes(ragged):
    segs = [s[:3] + tuple(np.meshgrid(s[3], s[4])) + s[5:] for _, s in ragged["segs"]]
    res, cnt = P.shepard_segments(segs, p=2.0, pixel_cutoff=2.0, separable=False, neighbours=True)
    for out, nbr, out0, nbr0 in zip(res, cnt, ragged["res"], ragged["cnt"]):
        assert out.shape == out0.shape and np.array_equal(out, out0) and np.array_equal(nbr, nbr0)


def test_all_non_finite_segment_in_a_batch(z0, cases):
    """A segment without a finite sample (nx = 0) between two populated ones: zeros, and the others as on their own."""
    c, e = cases["non_finite"], cases["non_finite_all"]
    seg = lambda k: (k["a"], k["l"], k["v"], k["ga"], k["gl"], k["ares"], k["lres"])  # noqa: E731
    res, cnt = P.shepard_segments([seg(c), seg(e), seg(c)], p=2.0, pixel_cutoff=1.0, separable=False, neighbours=True)
    out, nbr = _run(c)
    assert not res[1].any() and not cnt[1].any() and res[1].shape == e["ga"].shape
    for k in (0, 2):
        assert np.array_equal(res[k], out, equal_nan=True) and np.array_equal(cnt[k], nbr)


# ---- the C entry point with device pointers ----------------------------------------------------------------------------
def _pack(segs, separable):
    """Concatenated float32 arrays and the offset / size tables of surfh_shepard for ``segs``."""
    cat = lambda i: np.ascontiguousarray(np.concatenate([np.asarray(s[i], f32).ravel() for s in segs]))  # noqa: E731
    off = np.zeros(len(segs) + 1, np.int64)
    off[1:] = np.cumsum([np.asarray(s[0]).size for s in segs])
    if separable:
        na = np.array([np.asarray(s[3]).size for s in segs], np.int32)
        nl = np.array([np.asarray(s[4]).size for s in segs], np.int32)
    else:
        na = np.array([np.asarray(s[3]).size for s in segs], np.int32)
        nl = np.ones(len(segs), np.int32)
    ia = np.array([P._inv_res(s[5]) for s in segs], f32)
    il = np.array([P._inv_res(s[6]) for s in segs], f32)
    return dict(off=off, a=cat(0), l=cat(1), v=cat(2), qa=cat(3), ql=cat(4), na=na, nl=nl, ia=ia, il=il,
                n_q=int(np.sum(na.astype(np.int64) * nl)), separable=1 if separable else 0, n_seg=len(segs))


def _call(L, k, a, l, v, qa, ql, out, nbr, device, stream=None, ms=None, off=None, na=None, nl=None, cutoff=2.0):
    ip = lambda x: x.ctypes.data_as(_lib.c_int32_p)  # noqa: E731
    off = k["off"] if off is None else off
    return L.surfh_shepard(k["n_seg"], off.ctypes.data_as(C.POINTER(C.c_int64)), a, l, v,
                           ip(k["na"] if na is None else na), ip(k["nl"] if nl is None else nl), k["separable"], qa, ql,
                           _lib.fptr(k["ia"]), _lib.fptr(k["il"]), 2.0, 2.0, cutoff, 1e-6, out, nbr, device, stream,
                           None if ms is None else C.byref(ms))


def _host_ptr(x):
    return x.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("which", ["fixture_case_4", "ragged_batch"])
def test_device_pointers_on_a_callers_stream(z0, which):
    import torch
    L = _lib.load()
    if which == "fixture_case_4":
        c = so.kernel_cases(z0)[4]
        k = _pack([(c["a"], c["l"], c["v"], c["ga"], c["gl"], c["ares"], c["lres"])], False)
    else:
        k = _pack([s for _, s in sc.ragged_batch(z0)], True)
    n_q = k["n_q"]
    out_h, nbr_h = np.full(n_q, -7.0, f32), np.full(n_q, -7, np.int32)
    rc = _call(L, k, *(_host_ptr(k[x]) for x in ("a", "l", "v", "qa", "ql")), _host_ptr(out_h), _host_ptr(nbr_h), 0)
    assert rc == 0, L.surfh_shepard_last_error()

    dev = {x: torch.as_tensor(k[x], device="cuda:0") for x in ("a", "l", "v", "qa", "ql")}
    out_d = torch.full((n_q,), -7.0, dtype=torch.float32, device="cuda:0")
    nbr_d = torch.full((n_q,), -7, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    torch.cuda.synchronize()
    ms = C.c_float(0.0)
    rc = _call(L, k, *(dev[x].data_ptr() for x in ("a", "l", "v", "qa", "ql")), out_d.data_ptr(), nbr_d.data_ptr(), 1,
               stream.cuda_stream, ms)
    assert rc == 0, L.surfh_shepard_last_error()
    stream.synchronize()
    got, cnt = out_d.cpu().numpy(), nbr_d.cpu().numpy()
    print(f"{which}: device-pointer call, kernels {ms.value:.3f} ms")
    assert np.array_equal(got, out_h) and np.array_equal(cnt, nbr_h) and ms.value > 0
    assert (nbr_h >= 0).all() and nbr_h.max() > 0
    # without a neighbour array: the same values, and the earlier counts are left alone
    out_d.fill_(-7.0)
    torch.cuda.synchronize()
    rc = _call(L, k, *(dev[x].data_ptr() for x in ("a", "l", "v", "qa", "ql")), out_d.data_ptr(), None, 1,
               stream.cuda_stream)
    assert rc == 0, L.surfh_shepard_last_error()
    stream.synchronize()
    assert np.array_equal(out_d.cpu().numpy(), out_h) and np.array_equal(nbr_d.cpu().numpy(), nbr_h)


def test_argument_errors_are_rejected_on_the_host():
    """Each of these returns non-zero with a message before anything is allocated or launched: the output arrays keep
    their fill."""
    L = _lib.load()
    rng = np.random.default_rng(5)
    segs = [(rng.uniform(0, 3, 6), rng.uniform(0, 3, 6), rng.standard_normal(6), np.linspace(0, 3, 4),
             np.linspace(0, 3, 3), 1.0, 1.0) for _ in range(3)]
    k = _pack(segs, True)
    out, nbr = np.full(k["n_q"], -7.0, f32), np.full(k["n_q"], -7, np.int32)
    ptrs = [_host_ptr(k[x]) for x in ("a", "l", "v", "qa", "ql")]

    def rejected(word, **kw):
        p = list(ptrs)
        if kw.pop("null_samples", False):
            p[0] = None
        rc = _call(L, k, *p, _host_ptr(out), _host_ptr(nbr), 0, **kw)
        msg = L.surfh_shepard_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)
        assert np.all(out == -7.0) and np.all(nbr == -7)

    assert _call(L, k, *ptrs, _host_ptr(out), _host_ptr(nbr), 0) == 0 and np.all(nbr >= 0)     # the call itself is valid
    out[:], nbr[:] = -7.0, -7
    rejected("pt_off[0]", off=k["off"] + 1)
    rejected("non-decreasing", off=np.array([0, 12, 6, 18], np.int64))
    rejected("negative grid size", na=np.array([4, -4, 4], np.int32))
    rejected("negative grid size", nl=np.array([3, 3, -1], np.int32))
    rejected("null sample array", null_samples=True)
