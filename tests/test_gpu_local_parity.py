"""Parity of the operator chain element by element (needs an MI355X).

tests/test_gpu_parity.py holds every stage to one figure, the relative L2 error of the whole array.  Here the same outputs are
held to the local measures of tests/helpers.py -- the worst element (``max_err``) and the worst slice along every axis
(``slice_err``, no slice left out) -- at the project's gate TOL = 1e-5, on the problems of tests/problems.py that reach, at
48 x 48 pixels, the code paths otherwise taken by the full-size configs only: channel windows and detector axes longer than
1024 (``long_windows``), three channels in an order that keeps the exact-range accumulator and in one that forces the cleared
cube with chunk masks (``three_channels``), one channel more than a grouped adjoint GEMM takes (``five_channels``).  Every
measured value goes to the parity log (test_gpu_parity.note); tests/test_local_metrics_host.py shows, without a GPU, which
faults these measures catch and ``rel`` does not.

The GEMM element-wise measure max_ij |C - ref|_ij / (|A| |B|)_ij is held to 5e-6: DESIGN 4.4's worst case of the far K-step
class (4e-6) plus the three-product part (1e-6).  The CG vector kernels are held to what fp32 arithmetic on the given fp32
vectors can differ from the float64 result (bounds derived where they are used)."""
import ctypes
import functools

import numpy as np
import pytest

import problems
from capped_cases import AXPY, CG_OLD, CG_SIZES, EPS, cg_vectors, within
from helpers import TOL, build_model, local_errs, rel, slice_err
from oracle import surfh_oracle as orc
from test_gpu_parity import note, oracle_xs

pytestmark = pytest.mark.gpu

FWD_AXES = dict(row=(0, 1, 3), lam=2)                  # a channel's data as (P, S, Ldet, a)
MAP_AXES = dict(template=0, alpha=1, beta=2)           # the adjoint's maps (T, alpha, beta)
GEMM_ELEMENT_TOL = 5e-6

MAKERS = {"config1": problems.config1, "two_channel_small": problems.two_channel_small, "two_channel_mid": problems.two_channel_mid,
          "long_windows": problems.long_windows, "three_channels_ABC": lambda: problems.three_channels("ABC"),
          "three_channels_ACB": lambda: problems.three_channels("ACB"), "five_channels": problems.five_channels}


def check_local(name, a, ref, axes, tol=TOL, **tags):
    """Log the local measures of ``a`` against ``ref`` and hold every one of them to ``tol``; a failure names the worst slice."""
    e = local_errs(a, ref, axes)
    note(name, **tags, **e)
    print(name, tags, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in e.items()})
    bad = [f"{k} = {e[k]:.3e}" + (f" at index {e[k + '_at']}" if k + "_at" in e else "")
           for k in e if not k.endswith("_at") and not e[k] < tol]
    assert not bad, f"{name} {tags}: " + "; ".join(bad) + f" (bound {tol:g})"
    return e


class Refs:
    """A problem with the float64 oracle's outputs, each computed once and never changed."""

    def __init__(self, name):
        self.name = name
        self.cfg = MAKERS[name]()
        self.om = problems.oracle_model(self.cfg, box="direct")
        rng = np.random.default_rng(77)
        self.u = dict(uniform=rng.random(self.om.osize), normal=rng.standard_normal(self.om.osize))

    @functools.cached_property
    def fwd(self):
        st = {}
        y = self.om.forward(self.cfg["maps"], stages=st)
        self.blurred = st["blurred"]
        return y

    @functools.lru_cache(maxsize=None)
    def adj(self, kind):
        return self.om.adjoint(self.u[kind])

    @functools.lru_cache(maxsize=None)
    def adj_ref(self, kind):
        return self.om.adjoint_ref(self.u[kind])

    def channel(self, y, k):
        om = self.om
        return np.asarray(y)[om._idx[k]:om._idx[k + 1]].reshape(om.channels[k].oshape)


@functools.lru_cache(maxsize=None)
def refs(name):
    return Refs(name)


@pytest.fixture(scope="module", params=list(MAKERS))
def case(request):
    """One plan per problem for all the tests of the module."""
    r = refs(request.param)
    m = build_model(r.cfg)
    yield r, m
    m.close()


@pytest.fixture(scope="module")
def long_plan():
    r = refs("long_windows")
    m = build_model(r.cfg)
    yield r, m
    m.close()


def check_forward(name, r, y, **tags):
    for k in range(len(r.om.channels)):
        check_local(name, r.channel(y, k), r.channel(r.fwd, k), FWD_AXES, case=r.name, channel=k, **tags)


def adjoint_profile(m, u):
    m.profile_reset()
    m.profile_enable(True)
    try:
        a = m.adjoint(u)
        prof = m.profile()
    finally:
        m.profile_enable(False)
    return a, {k: v[0] for k, v in prof.items()}


# ---- the operator on every problem --------------------------------------------------------------------------------------------
def test_forward(case):
    r, m = case
    check_forward("local_forward", r, m.forward(r.cfg["maps"]))


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_adjoint_exact(case, kind):
    r, m = case
    check_local("local_adjoint", m.adjoint(r.u[kind]), r.adj(kind), MAP_AXES, case=r.name, data=kind)


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_adjoint_ref(case, kind):
    r, m = case
    check_local("local_adjoint_ref", m.adjoint_ref(r.u[kind]), r.adj_ref(kind), MAP_AXES, case=r.name, data=kind)


def test_adjoint_twice_then_zeros(case):
    """The accumulator carries no state on either path (dedicated accumulator with exact ranges, or cleared cube with masks): the
    second call with other data meets the same bounds, and zero data give exactly zero."""
    r, m = case
    m.adjoint(1e3 * r.u["normal"])
    check_local("local_adjoint_second_call", m.adjoint(r.u["uniform"]), r.adj("uniform"), MAP_AXES, case=r.name)
    assert np.all(m.adjoint(np.zeros(m.osize)) == 0)
    check_local("local_adjoint_after_zeros", m.adjoint(r.u["normal"]), r.adj("normal"), MAP_AXES, case=r.name)


def test_paths_taken(case):
    """Each problem is on the path its name says: the accumulator's clearing pass ran (or not), the grouped adjoint GEMM went out
    in the expected number of launches, the long windows have a second 1024-plane chunk."""
    r, m = case
    _, prof = adjoint_profile(m, r.u["uniform"])
    nch = len(r.om.channels)
    info = [[int(v) for v in m.debug_buffer(f"xsinfo:{k}")] for k in range(nch)]
    note("local_paths", case=r.name, profile=prof, xsinfo=info, ksteps=[int(v) for v in m.debug_buffer("ksteps")])
    print(r.name, prof, info)
    cleared = prof.get("fill_zero", 0)
    # only the two-piece overlap falls back to the cleared cube and the chunk masks; every other problem, long_windows included,
    # keeps the dedicated accumulator with exact ranges, where the masks are not read (test_kernel_path_switches clears on purpose)
    assert cleared == (1 if r.name == "three_channels_ACB" else 0), prof
    assert prof["gemm_wblur_adj"] == (nch + 3) // 4, prof                      # a launch takes at most GEMM_GROUP_MAX = 4 channels
    assert prof["spmm_scatter_adj"] == nch, prof
    if r.name == "five_channels":
        assert prof["gemm_wblur_adj"] == 2                                     # five channels do not fit one launch: a second one goes out
    if r.name == "long_windows":
        assert all(i[0] > 1024 and i[3] > 1024 for i in info), info            # LinP and Lin: two chunks in the grids, two scale segments
        assert all(c.oshape[2] > 1024 for c in r.om.channels)
    else:
        assert all(i[0] <= 1024 for i in info), info


# ---- stages of the forward chain on the long windows --------------------------------------------------------------------------
def device_blurred(r, m):
    N = r.cfg["N"]
    lo, hi = int(m.debug_buffer("info")[0]), int(m.debug_buffer("info")[1])
    return m.debug_buffer("blurred").transpose(2, 1, 0)[: hi - lo, :N, :N], lo, hi     # device layout is [beta][alpha][lambda]


def xs_by_segment(m, k, ref_xs):
    """The device's GEMM operand of channel ``k`` and the reference [(l, b'), (p, s, a)], both as (row, b', chunk, 1024): the
    slices (row, b', chunk) are the segments that carry one block scale each."""
    LinP, shift, nbs, Lin = (int(v) for v in m.debug_buffer(f"xsinfo:{k}"))
    ref = ref_xs.reshape(Lin, nbs, -1).transpose(2, 1, 0)
    xs = m.debug_buffer(f"xs:{k}")[: ref.shape[0]]                              # device layout [(p,s,a)][b'][LinP]
    nchunk = (LinP + 1023) // 1024
    full = np.zeros(ref.shape[:2] + (nchunk * 1024,))
    full[:, :, shift: shift + Lin] = ref
    dev = np.zeros_like(full)
    dev[:, :, :LinP] = xs
    # the gather moves whole groups of four planes from a start aligned to four: up to three planes on either side of the window
    # ride along (their columns of the response are zero); the padding behind them stays zero
    end = (shift + Lin + 3) // 4 * 4
    assert shift < 4 and not dev[:, :, end:].any()
    dev[:, :, :shift] = 0.0
    dev[:, :, shift + Lin: end] = 0.0
    return dev.reshape(ref.shape[:2] + (nchunk, 1024)), full.reshape(ref.shape[:2] + (nchunk, 1024))


def test_stage_blurred_cube_per_plane(long_plan):
    r, m = long_plan
    m.forward(r.cfg["maps"])
    r.fwd
    b, lo, hi = device_blurred(r, m)
    check_local("local_blurred", b, r.blurred[lo:hi], dict(plane=0, alpha=1, beta=2), case=r.name)


def test_stage_gemm_operand_per_segment(long_plan):
    r, m = long_plan
    m.forward(r.cfg["maps"])
    r.fwd
    for k, tab in enumerate(r.om.channels):
        dev, ref = xs_by_segment(m, k, oracle_xs(r.om, tab, r.blurred))
        assert dev.shape[2] == 2
        check_local("local_xs", dev, ref, dict(segment=(0, 1, 2), row=0), case=r.name, channel=k)


# ---- the A/B switches where long windows and many channels change what they do ------------------------------------------------
def plan_groups(m):
    """Workgroups of the grouped gather and of the grouped scatter tables over all channels (0: row by row)."""
    dims = (ctypes.c_int64 * 4)()
    assert m._L.surfh_debug_dims(m._plan, b"groups", dims) == 0
    return int(dims[0]), int(dims[1])


@pytest.mark.parametrize("name", ["long_windows", "five_channels"])
@pytest.mark.parametrize("env", [{"SURFH_GATHER_GROUPED": "0"}, {"SURFH_SCATTER_GROUPED": "0"}, {"SURFH_GEMM_GROUPED": "0"},
                                 {"SURFH_WBLUR_FAR": "0"}, {"SURFH_SCATTER_RMW_ALL": "1"}, {"SURFH_ADJ_CLEAR": "1"},
                                 {"SURFH_ADJ_CLEAR": "1", "SURFH_SCATTER_RMW_ALL": "1"},
                                 {"SURFH_ADJ_CLEAR": "1", "SURFH_SCATTER_GROUPED": "0"}],
                         ids=["gather_row_by_row", "scatter_row_by_row", "adjoint_gemms_one_by_one", "gemm_three_products_everywhere",
                              "scatter_rmw_switch_on_exact_ranges", "cleared_cube_chunk_masks", "cleared_cube_rmw_everywhere",
                              "cleared_cube_chunk_masks_row_by_row"])
def test_kernel_path_switches(name, env, monkeypatch):
    """Every switch alone, and the cleared-cube path in its three forms.  By default both problems keep the dedicated accumulator
    with exact ranges, where the scatter kernels never read the chunk masks: SURFH_SCATTER_RMW_ALL=1 alone must then change
    nothing (asserted bit for bit -- a read-modify-write of the never-cleared accumulator would add up from call to call).
    SURFH_ADJ_CLEAR=1 puts the plan on the cleared cube, where the masks decide: on long_windows every scatter row of the second
    channel has two mask bits that differ (overlap in chunk 0 only), read by the grouped and by the row-by-row kernel; with
    SURFH_SCATTER_RMW_ALL=1 on top every row read-modify-writes."""
    r = refs(name)
    default = {}
    if env == {"SURFH_SCATTER_RMW_ALL": "1"}:
        m = build_model(r.cfg)
        try:
            default = dict(a=m.adjoint(r.u["normal"]), a2=m.adjoint(r.u["uniform"]))
        finally:
            m.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                               # read at plan creation
    m = build_model(r.cfg)
    try:
        y = m.forward(r.cfg["maps"])
        a, prof = adjoint_profile(m, r.u["normal"])
        a2 = m.adjoint(r.u["uniform"])
        ks = [int(v) for v in m.debug_buffer("ksteps")]
        groups = plan_groups(m)
        zero = m.adjoint(np.zeros(m.osize))
    finally:
        m.close()
    assert not zero.any()
    tag = "+".join(f"{k}={v}" for k, v in env.items())
    check_forward("local_switch_forward", r, y, env=tag)
    check_local("local_switch_adjoint", a, r.adj("normal"), MAP_AXES, case=name, env=tag, data="normal")
    check_local("local_switch_adjoint", a2, r.adj("uniform"), MAP_AXES, case=name, env=tag, data="uniform")
    nch = len(r.om.channels)
    if "SURFH_GEMM_GROUPED" in env:
        assert prof["gemm_wblur_adj"] == nch, prof
    else:
        assert prof["gemm_wblur_adj"] == (nch + 3) // 4, prof
    if "SURFH_WBLUR_FAR" in env:
        assert ks[1] == 0 and ks[3] == 0, ks
    else:
        assert ks[1] > 0, ks
    # the switch did what its name says
    assert (groups[0] == 0) == ("SURFH_GATHER_GROUPED" in env), groups
    assert (groups[1] == 0) == ("SURFH_SCATTER_GROUPED" in env), groups
    assert prof.get("fill_zero", 0) == (1 if "SURFH_ADJ_CLEAR" in env else 0), prof
    if default:
        assert np.array_equal(a, default["a"]) and np.array_equal(a2, default["a2"])


# ---- one hot detector row, one hot map pixel -----------------------------------------------------------------------------------
def own_norm_errs(a, ref, axes):
    """|a_s - ref_s| / |ref_s| of every slice, each against its OWN norm (the measure of the GEMM selftest's hot-row case): a
    slice 1e6 brighter than the others sets no floor for them.  Slices whose reference is zero must be zero."""
    axes = tuple(axes)
    lead = tuple(ref.shape[ax] for ax in axes)
    d = np.moveaxis(a - ref, axes, range(len(axes))).reshape(int(np.prod(lead)), -1)
    rr = np.moveaxis(ref, axes, range(len(axes))).reshape(d.shape)
    nr, nd = np.linalg.norm(rr, axis=1), np.linalg.norm(d, axis=1)
    assert not nd[nr == 0].any(), "a slice that must be zero is not"
    e = np.where(nr > 0, nd / np.where(nr > 0, nr, 1.0), 0.0)
    k = int(np.argmax(e))
    return float(e[k]), tuple(int(i) for i in np.unravel_index(k, lead)), e.reshape(lead)


def test_hot_detector_row(long_plan):
    """One (p, s, a) row of the data 1e6 times brighter: the adjoint GEMM's operand has one scale per row, so the rows beside it
    keep their precision.  Seen in the accumulated cube before the transforms mix the pixels: every pixel, the ones the hot row
    never reaches included, within TOL of ITS OWN norm; and the maps, where the hot row's strip dominates, within TOL on every
    local measure."""
    r, m = long_plan
    om = r.om
    u = r.u["uniform"].copy()
    hot = r.channel(u, 0)                                                       # a view: (P, S, Ldet, a)
    hot[1, 1, :, 2] *= 1e6
    st = {}
    ref = om.adjoint(u, stages=st)
    a = m.adjoint(u)
    N = r.cfg["N"]
    lo, hi = int(m.debug_buffer("info")[0]), int(m.debug_buffer("info")[1])
    g = m.debug_buffer("gcube").transpose(2, 1, 0)[: hi - lo, :N, :N].astype(np.float64)
    gref = st["global_cube"][lo:hi]
    e, at, per_pixel = own_norm_errs(g, gref, (1, 2))
    pix_norm = np.linalg.norm(gref, axis=0)
    faint = (pix_norm > 0) & (pix_norm < 1e-3 * pix_norm.max())                 # pixels the hot row does not reach
    assert faint.sum() > 100 and (pix_norm >= 1e-3 * pix_norm.max()).sum() >= 4
    note("local_hot_row", case=r.name, worst_pixel=e, at=at, worst_faint_pixel=float(per_pixel[faint].max()), faint_pixels=int(faint.sum()))
    print(f"hot detector row: worst pixel of the accumulated cube {e:.2e} at {at}, worst faint pixel {per_pixel[faint].max():.2e}")
    assert e < TOL, (e, at)
    check_local("local_hot_row_maps", a, ref, MAP_AXES, case=r.name)


def test_hot_map_pixel(long_plan):
    """One pixel of one map 1e6 times brighter: the gather writes the forward GEMM's operand with one block scale per (row,
    1024-plane segment of one beta column), so the segments beside the hot ones keep their precision.  The operand is compared
    with the oracle's gather of the DEVICE's blurred cube (the fp32 transforms before it spread their rounding of the hot pixel
    over the whole plane, as any fp32 transform does): every segment within TOL of ITS OWN norm; and the data against the oracle
    on every local measure."""
    r, m = long_plan
    maps = r.cfg["maps"].copy()
    maps[1, 20, 27] *= 1e6
    y = m.forward(maps)
    b, lo, hi = device_blurred(r, m)
    cube = np.zeros(r.om.cube_shape)
    cube[lo:hi] = b
    worst = {}
    for k, tab in enumerate(r.om.channels):
        dev, ref = xs_by_segment(m, k, oracle_xs(r.om, tab, cube))
        seg = np.linalg.norm(ref, axis=3)
        e, at, _ = own_norm_errs(dev, ref, (0, 1, 2))
        worst[k] = (e, at, float(seg[seg > 0].min() / seg.max()))
        print(f"hot map pixel, channel {k}: worst segment {e:.2e} at {at}, faintest / brightest segment {worst[k][2]:.1e}")
    note("local_hot_pixel_xs", case=r.name, worst={str(k): list(v[:2]) for k, v in worst.items()}, spread={str(k): v[2] for k, v in worst.items()})
    yref = r.om.forward(maps)
    rows = {}
    for k, tab in enumerate(r.om.channels):
        check_local("local_hot_pixel_forward", r.channel(y, k), r.channel(yref, k), FWD_AXES, case=r.name, channel=k)
        # ... and through the forward GEMM: every (p, s, a) row of the data within TOL of ITS OWN norm of the oracle's channel
        # applied to the device's blurred cube, the rows that look away from the hot pixel included
        ydev = orc.channel_forward(tab, cube, "direct").reshape(tab.oshape)
        e, at, per_row = own_norm_errs(r.channel(y, k), ydev, (0, 1, 3))
        nrm = np.linalg.norm(ydev, axis=2)
        rows[k] = (e, at, float(nrm.min() / nrm.max()))
        print(f"hot map pixel, channel {k}: worst data row {e:.2e} at {at}, faintest / brightest row {rows[k][2]:.1e}")
    note("local_hot_pixel_rows", case=r.name, worst={str(k): list(v[:2]) for k, v in rows.items()}, spread={str(k): v[2] for k, v in rows.items()})
    assert all(v[0] < TOL for v in worst.values()), worst
    assert all(v[0] < TOL for v in rows.values()), rows


# ---- the two-piece fp16 GEMM, element by element -------------------------------------------------------------------------------
def response_like(nout, Lin, ncol):
    """sinc^2 around a diagonal, rows normalised, ``ncol`` beta columns side by side: [nout][ncol * Lin]."""
    lo, li = np.arange(nout)[:, None], np.arange(Lin)[None, :]
    cols = []
    for c in range(ncol):
        w = np.sinc((li - (lo * (Lin / nout) + 3.0 * c)) / 2.3) ** 2
        cols.append(w / w.sum(axis=1, keepdims=True))
    return np.concatenate(cols, axis=1)


def gemm_cases():
    rng = np.random.default_rng(41)
    # ragged M (1664 = 6.5 tiles) with split K, and three K slabs: operands without structure, magnitudes over 12 decades
    for (M, N, K, sk) in [(1664, 1408, 2112, 2), (384, 640, 1056, 3)]:
        A = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-6, 6, (M, K)))).astype(np.float32)
        B = rng.standard_normal((K, N)).astype(np.float32) + np.arange(N, dtype=np.float32)[None, :] * 0.02
        yield f"plain_{M}x{N}x{K}_sk{sk}", "1", None, A, B, sk, False
    # K-step classes, split K dividing both lists; zero-mean and non-negative data
    M, N, Lin, ncol, sk = 384, 1408, 1152, 3, 2
    B = np.ascontiguousarray(response_like(N, Lin, ncol).T).astype(np.float32)
    for data, A in (("nonneg", rng.random((M, ncol * Lin)) * 50 + 1), ("randn", rng.standard_normal((M, ncol * Lin)))):
        yield f"klist_{data}_{M}x{N}x{ncol * Lin}_sk{sk}", "2", None, A.astype(np.float32), B, sk, True
    # the adjoint's tile shape (GemmArgs::permP) with a last group of missing columns: 5 = 4 + 1
    M, Ldet, Lin, ncol = 128, 640, 768, 5
    Wt = np.ascontiguousarray(response_like(Ldet, Lin, ncol)).astype(np.float32)
    yield f"perm_{M}x{ncol * Lin}x{Ldet}", "2", Lin, (rng.random((M, Ldet)) * 50 + 1).astype(np.float32), Wt, 1, True


@pytest.mark.parametrize("case_id", range(5))
def test_gemm_selftest_element_wise(case_id, monkeypatch):
    from surfh_amd import _lib
    L = _lib.load()
    name, mode, perm, A, B, sk, want_far = list(gemm_cases())[case_id]
    M, K = A.shape
    N = B.shape[1]
    monkeypatch.setenv("SURFH_SELFTEST_F16X2", mode)
    if perm:
        monkeypatch.setenv("SURFH_SELFTEST_PERM", str(perm))
    Cg = np.empty((M, N), dtype=np.float32)
    _lib.check(L.surfh_gemm_selftest(0, M, N, K, sk, _lib.fptr(A), _lib.fptr(B), _lib.fptr(Cg)))
    ks = (ctypes.c_int64 * 2)()
    L.surfh_gemm_selftest_ksteps(ks)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref, mag = A64 @ B64, np.abs(A64) @ np.abs(B64)
    assert mag.min() > 0

    def measures(C):
        el = np.abs(C - ref) / mag
        k = int(np.argmax(el))
        out = dict(element=float(el.flat[k]), element_at=[int(i) for i in np.unravel_index(k, el.shape)], rel=rel(C, ref))
        out["row"], out["row_at"] = slice_err(C, ref, 0)
        out["col"], out["col_at"] = slice_err(C, ref, 1)
        return out
    e = measures(Cg)
    f32 = measures(A @ B)                                                       # the same product in plain fp32, for scale
    note("local_gemm", shape=name, near=int(ks[0]), far=int(ks[1]), **e, **{"fp32_" + k: v for k, v in f32.items()})
    print(name, "near/far K steps", list(ks), {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in e.items()},
          "plain fp32:", f"element {f32['element']:.2e} row {f32['row']:.2e} col {f32['col']:.2e}")
    if mode == "2":
        assert (ks[1] > ks[0]) == want_far, list(ks)
    assert e["element"] < GEMM_ELEMENT_TOL, (name, e["element"], e["element_at"])
    assert e["row"] < TOL and e["col"] < TOL, (name, e)


# ---- the 2-D transforms at the boundary shapes of test_gpu_dft.py ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(251, 251), (255, 40), (33, 254), (256, 256), (300, 64), (501, 256), (257, 64), (20, 48)])
def test_transforms_local(shape):
    from test_gpu_dft import build, np_adjoint, np_forward
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    L, T = 130, 3
    m, sotf, specs = build(shape, L, T, rng)
    maps = rng.random((T,) + shape)
    cube = rng.standard_normal((L,) + shape)
    try:
        yf, ya = m.forward(maps), m.adjoint(cube)
    finally:
        m.close()
    axes = dict(plane=0, alpha=1, beta=2)
    check_local("local_dft_forward", yf, np_forward(sotf, specs, maps), axes, shape=list(shape))
    check_local("local_dft_adjoint", ya, np_adjoint(sotf, specs, cube), axes, shape=list(shape))


# ---- the CG vector kernels against float64 numpy -------------------------------------------------------------------------------
# EPS (the unit roundoff of fp32), the AXPY bound, the vectors and the element-wise comparison: tests/capped_cases.py, which
# also names the regime every n below is in (tests/test_capped_grid_host.py asserts it)


@pytest.fixture(scope="module")
def vec_plan():
    m = build_model(problems.config1())
    yield m
    m.close()


def dev(*arrays):
    import torch
    return [torch.as_tensor(a.copy(), device="cuda:0") for a in arrays]


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("n", CG_OLD + CG_SIZES)
def test_cg_vector_kernels(vec_plan, n):
    """single lane, partial block, an odd detector-axis length, config 1's osize, several blocks with a tail; past the launch
    caps: the first element of the dot kernels' second trip, ragged second (2048 blocks) and fifth (512 blocks) trips"""
    m = vec_plan
    x, r, d, q, b = cg_vectors(n, 200 + n)
    x64, r64, d64, q64, b64 = (v.astype(np.float64) for v in (x, r, d, q, b))
    # dot
    xt, rt, dt, qt, bt = dev(x, r, d, q, b)
    dot_errs = []
    for a_t, b_t, want in ((dt, qt, d64 @ q64), (rt, rt, r64 @ r64), (xt, bt, x64 @ b64)):
        got = m.dot_dev(a_t, b_t, n)
        scale = float(np.abs(host(a_t).astype(np.float64)) @ np.abs(host(b_t).astype(np.float64)))
        dot_errs.append(abs(got - want) / scale)
        assert abs(got - want) <= 1e-6 * abs(want) and abs(got - want) <= 1e-14 * scale, (n, got, want)      # fp64 sums of exact products
        assert m.dot_dev(a_t, b_t, n) == got                                       # a fixed order: the same bits again
    note("local_cg_dot", n=n, err_of_sum_abs=dot_errs)
    # residual: one fp32 subtraction
    out = dev(np.full(n, 7.0, dtype=np.float32))[0]
    m.residual_dev(out, bt, qt, n)
    within(host(out), b64 - q64, EPS * np.abs(b64 - q64), "residual")
    # step: x += s d, r -= s q with s = rr / d.q; returns the new r.r
    rr = float(r64 @ r64)
    s = rr / float(d64 @ q64)
    rr1 = m.cg_step_dev(xt, rt, dt, qt, n, rr)
    x1, r1 = host(xt), host(rt)
    within(x1, x64 + s * d64, AXPY * (np.abs(x64) + np.abs(s * d64)), "step x")
    rn64 = r64 - s * q64
    er = AXPY * (np.abs(r64) + np.abs(s * q64))
    within(r1, rn64, er, "step r")
    assert np.array_equal(host(dt), d) and np.array_equal(host(qt), q)
    want_rr = float(rn64 @ rn64)
    bound_rr = float(2 * np.abs(rn64) @ er + er @ er) + 1e-14 * want_rr            # r.r of elements each within `er` of rn64
    own_rr = float(r1.astype(np.float64) @ r1.astype(np.float64))
    note("local_cg_step", n=n, rr_err=abs(rr1 - want_rr) / want_rr, rr_bound=bound_rr / want_rr, rr_vs_own_r=abs(rr1 - own_rr) / own_rr)
    assert abs(rr1 - want_rr) <= bound_rr, (n, rr1, want_rr, bound_rr)
    assert abs(rr1 - want_rr) <= 1e-6 * want_rr, (n, rr1, want_rr)                 # the readable gate, as for the dot product
    assert abs(rr1 - own_rr) <= 1e-14 * own_rr, (n, rr1, own_rr)                   # the fp64 sum of the stored fp32 residual
    # direction: d = r + beta d
    beta = rr1 / rr
    m.cg_dir_dev(dt, rt, n, beta)
    d1 = host(dt)
    r1_64 = r1.astype(np.float64)
    within(d1, r1_64 + beta * d64, AXPY * (np.abs(r1_64) + np.abs(beta * d64)), "direction")
    # the fused call: the same bits as step + direction
    xf, rf, df, qf = dev(x, r, d, q)
    rrf = m.cg_iter_dev(xf, rf, df, qf, n, rr)
    assert rrf == rr1 and np.array_equal(host(xf), x1) and np.array_equal(host(rf), r1) and np.array_equal(host(df), d1)


@pytest.mark.parametrize("n", CG_OLD + CG_SIZES)
def test_cg_nosync_sequence(vec_plan, n):
    """The device-resident scalars: two iterations and one residual refresh without a host synchronisation leave the vectors of
    the synchronous calls, bit for bit, and a trace equal to the scalars those calls returned.  From n = 131 073 on the
    direction kernel runs more blocks than it sums partials (513 over 512)."""
    m = vec_plan
    x, r, d, q, b = cg_vectors(n, 300 + n)
    rng = np.random.default_rng(400 + n)
    q2 = ((0.5 + rng.random(n)) * d + 0.1 * rng.standard_normal(n)).astype(np.float32)
    # synchronous: r.r, two fused iterations
    xs, rs, ds, qs, q2s, bs = dev(x, r, d, q, q2, b)
    rr0 = m.dot_dev(rs, rs, n)
    rr1 = m.cg_iter_dev(xs, rs, ds, qs, n, rr0)
    rr2 = m.cg_iter_dev(xs, rs, ds, q2s, n, rr1)
    x2, r2, d2 = host(xs).copy(), host(rs).copy(), host(ds).copy()
    # ... and the refresh iteration from float64: x += (rr / d.q) d; r = b - q; rr' = r.r; d = r + (rr' / rr) d
    d2_64, x2_64 = d2.astype(np.float64), x2.astype(np.float64)
    s3 = rr2 / float(d2_64 @ q.astype(np.float64))
    r3_64 = b.astype(np.float64) - q2.astype(np.float64)
    # device-resident
    xn, rn, dn, qn, q2n, bn = dev(x, r, d, q, q2, b)
    m.cg_begin_dev(rn, n)
    m.cg_iter_nosync_dev(xn, rn, dn, qn, n)
    m.cg_iter_nosync_dev(xn, rn, dn, q2n, n)
    tr = m.cg_trace()
    assert np.array_equal(tr, np.array([rr0, rr1, rr2])), (tr, rr0, rr1, rr2)
    assert np.array_equal(host(xn), x2) and np.array_equal(host(rn), r2) and np.array_equal(host(dn), d2)
    m.cg_xupdate_nosync_dev(xn, dn, qn, n)
    m.cg_refresh_nosync_dev(rn, bn, q2n, dn, n)
    tr = m.cg_trace()
    assert len(tr) == 4 and np.array_equal(tr[:3], np.array([rr0, rr1, rr2]))
    within(host(xn), x2_64 + s3 * d2_64, AXPY * (np.abs(x2_64) + np.abs(s3 * d2_64)), "refresh x")
    r3 = host(rn)
    within(r3, r3_64, EPS * np.abs(r3_64), "refresh r")
    own = float(r3.astype(np.float64) @ r3.astype(np.float64))
    note("local_cg_nosync", n=n, refresh_rr_vs_own_r=abs(tr[3] - own) / own)
    assert abs(tr[3] - own) <= 1e-14 * own
    beta = tr[3] / rr2
    within(host(dn), r3.astype(np.float64) + beta * d2_64, AXPY * (np.abs(r3.astype(np.float64)) + np.abs(beta * d2_64)), "refresh d")
