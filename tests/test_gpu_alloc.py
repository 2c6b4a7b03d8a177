"""Device memory is owned, balanced and all-or-nothing (surfh_amd/csrc/dev_buf.h), stated as equalities of the allocator's own
counters: ``surfh_debug_alloc_count`` (live, total) and ``surfh_debug_alloc_fail`` (refuse the k-th allocation from now on, once).

1. every kind of plan, the masked mixing table and the two plan-less entry points give back exactly what they took;
2. every lazily allocated set is allocated once: the second call of an entry leaves ``live`` where the first left it (so NnScope
   and every call-scoped temporary return what they took), and closing the plan returns to the start;
3. a refused allocation -- each one a call makes, in turn, on a fresh plan -- is an error return that names the allocation and
   leaves nothing behind.  The failed call is never repeated on the same plan here: what a retry finds is proved on the host
   (tests/native/dev_buf_test.cpp), where a wrong answer is an assertion and not a launch on a null pointer.

``surfh_wct_expsol`` runs on the channel-less Model_WCT plan, not on config1: config1's channel window is planes [0, 127) of
128, and the closed-form solve refuses a plan that does not own every plane before it allocates anything.
Needs a real MI355X (`-m gpu`)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import problems
from helpers import build_model, make_ifu
from oracle import surfh_oracle as orc
from surfh_amd import _lib

pytestmark = pytest.mark.gpu

MU, MU_REG = 1.3, 5e3
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def counts():
    live, total = C.c_int64(), C.c_int64()
    _lib.load().surfh_debug_alloc_count(C.byref(live), C.byref(total))
    return live.value, total.value


def live():
    return counts()[0]


def arm(k):
    _lib.load().surfh_debug_alloc_fail(int(k))


@pytest.fixture(autouse=True)
def disarmed():
    yield
    arm(0)


# ---- plans built again and again: the problem (host work) once, the plan every time ------------------------------------------
_cfgs = {}


def _cfg(name):
    if name not in _cfgs:
        _cfgs[name] = getattr(problems, name)()
    return _cfgs[name]


def c1():
    return build_model(_cfg("config1"))


def mid():
    return build_model(_cfg("two_channel_mid"))


def blurred_96():
    """tests/test_gpu_variants.blurred_case(L=5, N=96) without its oracle"""
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    N, s = 96, problems.STEP_DEG
    if "blurred_96" not in _cfgs:
        ax = orc.synthetic_axes(N, s)
        spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
        _cfgs["blurred_96"] = (orc.ir2fr(orc.gaussian_psf(np.linspace(7.0, 8.2, 5), problems.STEP), (N, N)), ax, make_ifu(spec))
    sotf, ax, ifu = _cfgs["blurred_96"]
    pts = [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s)]
    return MRSBlurred(sotf, ax, ax, ifu, s, instru.CoordList([instru.Coord(a, b) for a, b in pts]))


def wct():
    """a channel-less Model_WCT plan, 16 x 12, with the spectra and PSFs of tests/wct_cases.py"""
    import wct_cases
    from surfh_amd.mixing import Model_WCT
    L, T, shape = 24, 3, (16, 12)
    return Model_WCT(wct_cases.noisy_psfs(shape, L, np.random.default_rng(5)), wct_cases.bump_spectra(T, L), shape, np.ones(L))


# ---- 1. balance ------------------------------------------------------------------------------------------------------------------
from test_gpu_op_routes import PLANS  # noqa: E402  (the eleven plan kinds, with their creation-time environment)


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_gives_back_what_it_took(name, monkeypatch):
    env, make, _ = PLANS[name]
    base = live()
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        m = make()
    built = live()
    rng = np.random.default_rng(1)
    m.forward(rng.random(m.ishape))
    m.adjoint(rng.standard_normal(m.oshape))
    print(f"{name}: {built - base} buffers after create, {live() - base} after one forward and one adjoint")
    assert built > base
    m.close()
    assert live() == base


def test_wct_plan_gives_back_what_it_took():
    base = live()
    m = wct()
    rng = np.random.default_rng(2)
    m.forward(rng.random(m.ishape))
    m.adjoint(rng.standard_normal(m.oshape))
    assert live() > base
    m.close()
    assert live() == base


def _mixing_st():
    from surfh_amd.mixing import MixingST
    src = open(os.path.join(G, "make_golden.py")).read()
    ns = {}
    exec(src[src.index("def mixing_st_inputs"):src.index("def mixing_st():")], {"np": np}, ns)
    tpl, (na, nb), L, sel, fast, maps, cube = ns["mixing_st_inputs"]()
    return MixingST(tpl, np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), sel, fast), maps, cube


def test_mixing_table_gives_back_what_it_took():
    base = live()
    m, maps, cube = _mixing_st()
    m.forward(maps), m.adjoint(cube), m.fwadj(maps)
    assert live() == base + 8                   # the table's eight buffers, TST among them
    m.close()
    assert live() == base


def test_planless_calls_give_back_what_they_took():
    import shepard_oracle as so
    from surfh_amd import preprocessing as P
    from surfh_amd import templates as T
    base, t0 = counts()
    c = so.kernel_cases(np.load(so.GOLDEN))[0]
    P.exponential_modified_shepard(c["a"], c["l"], c["v"], c["ga"], c["gl"], p=c["p"], alpha=2.0, pixel_cutoff=c["cutoff"],
                                   alpha_res=c["ares"], lambda_res=c["lres"], return_neighbours=True)
    l1, t1 = counts()
    assert l1 == base and t1 > t0
    z = np.load(os.path.join(G, "templates.npz"))
    T.median_filter_spectral(z["med0_in"], int(z["med0_size"]), str(z["med0_mode"]))
    l2, t2 = counts()
    assert l2 == base and t2 == t1 + 2


# ---- 2. and 3.: the entries ------------------------------------------------------------------------------------------------------
_inputs = {}


def _in(m, key):
    """fixed inputs, drawn once per plan shape"""
    k = (key, m.isize, m.osize)
    if k not in _inputs:
        rng = np.random.default_rng(7)
        _inputs[k] = dict(y=rng.random(m.osize), x=rng.random(m.ishape), w=0.5 + rng.random(m.osize))
    return _inputs[k]


def e_cg(m):
    m.cg(_in(m, "c1")["y"], mu=MU, mu_reg=MU_REG, max_iter=1)


def e_mmmg(m):
    m.mmmg(_in(m, "c1")["y"], mu=MU, mu_reg=MU_REG, max_iter=1)


def e_mmmg_huber(m):
    m.mmmg(_in(m, "c1")["y"], mu=MU, mu_reg=MU_REG, max_iter=1, delta=0.1)


def e_mmmg_robust(m):
    m.mmmg(_in(m, "c1")["y"], mu=MU, mu_reg=MU_REG, max_iter=1, data_delta=3.0)


def e_cg_sample(m):
    m.sample_posterior(_in(m, "c1")["y"], mu=MU, mu_reg=MU_REG, n_samples=2, seed=11, max_iter=1)


def e_cg_templates(m):
    d = _in(m, "c1")
    m.cg_templates(d["y"], d["x"], mu=MU, mu_spec=0.5, max_iter=1)


def e_cg_nonneg(m):
    m.cg_nonneg(_in(m, "c1")["y"], mu=MU, mu_reg=MU_REG, rho=2.0, outer=1, inner=1)


def e_data_weights(m):
    m.set_data_weights(_in(m, "c1")["w"])
    m.set_data_weights(None)


def e_imager(m):
    from surfh_amd.imager import ImagerModel
    rng = np.random.default_rng(3)
    im = ImagerModel(m, 0.1 + rng.random((2, m.cube_shape[0])), decim=2)
    m.set_imager(im)                            # config1 does not own every plane: the streamed set-up, with its own temporaries
    m.set_imager_data(rng.random(im.oshape), 0.7, weights=0.5 + rng.random(im.oshape))
    m.set_imager_data(None)
    m.set_imager(None)


def e_wct_expsol(m):
    from surfh_amd.mixing import regularisation_freq
    rng = np.random.default_rng(4)
    data, mu, reg = rng.standard_normal(m.oshape), np.full(m.n_spec, 0.5), regularisation_freq(m.shape_target) + 10.0
    m.expsol(data, mu, reg)
    m.set_specs(1.0 + rng.random((m.n_spec, m.n_lamb)))        # drops the Hessian: the next call builds it again
    m.expsol(data, mu, reg)


def e_cg_planes(m):
    m.cg(_in(m, "b96")["y"], mu=MU, mu_reg=0.07, max_iter=1)


def e_cg_planes_dev(m):
    import torch
    d = _in(m, "b96")
    y = torch.as_tensor(np.asarray(d["y"], dtype=np.float32).ravel(), device="cuda:0")
    x = torch.as_tensor(np.asarray(d["x"], dtype=np.float32).ravel(), device="cuda:0")
    torch.cuda.synchronize()
    m.cg_begin_dev(y, x, MU, 0.07)
    m.cg_step_dev(1, 50)
    m.cg_rr()
    torch.cuda.synchronize()


def e_huber_planes(m):
    m.mmmg(_in(m, "b96")["y"], mu=MU, mu_reg=0.07, max_iter=1, delta=0.1)


ENTRIES = {
    "cg": (c1, e_cg), "mmmg": (c1, e_mmmg), "mmmg_huber": (c1, e_mmmg_huber), "mmmg_robust": (c1, e_mmmg_robust),
    "cg_sample": (c1, e_cg_sample), "cg_templates": (c1, e_cg_templates), "cg_nonneg": (c1, e_cg_nonneg),
    "data_weights": (c1, e_data_weights), "imager": (c1, e_imager), "wct_expsol": (wct, e_wct_expsol),
    "cg_planes": (blurred_96, e_cg_planes), "cg_planes_dev": (blurred_96, e_cg_planes_dev), "huber_planes": (blurred_96, e_huber_planes),
}


@pytest.mark.parametrize("make", [c1, wct, blurred_96], ids=lambda f: f.__name__)
def test_lazy_sets_are_allocated_once(make):
    base = live()
    m = make()
    for name, (mk, call) in ENTRIES.items():
        if mk is not make:
            continue
        before, t0 = counts()
        call(m)
        first, t1 = counts()
        call(m)
        second, t2 = counts()
        print(f"{name}: first call {t1 - t0} allocations, {first - before} kept; second call {t2 - t1} allocations, {second - first} kept")
        assert second == first, name
        assert t2 - t1 <= t1 - t0, name
    m.close()
    assert live() == base


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refused_allocation_leaves_nothing_behind(name):
    make, call = ENTRIES[name]
    base = live()
    twin = make()
    t0 = counts()[1]
    call(twin)
    n = counts()[1] - t0
    twin.close()
    assert live() == base and n >= 1
    t = time.time()
    for k in range(1, n + 1):
        m = make()
        arm(k)
        with pytest.raises(Exception, match="hipMalloc") as ei:
            call(m)
        assert isinstance(ei.value, (RuntimeError, ValueError, np.linalg.LinAlgError)), ei.value
        arm(0)
        m.close()
        assert live() == base, (name, k)
    print(f"{name}: {n} allocations, each refused in turn on a fresh plan, {time.time() - t:.2f} s")


# (builder, last k, allocations of one build).  Measured on an MI355X: config1 65 allocations, one build 0.01 s, all 65 refused
# builds 0.37 s; blurred_96 44, 0.00 s, 0.18 s; two_channel_mid 111, 0.19 s, all 111 refused builds 12.1 s (each one repeats the
# host-side table construction in Python, 0.1 s) -- too long, so mid takes every k up to the first channel's last allocation,
# k = 57 (5.5 s): 26 before the channels (sotf, templates, 6 + 6 DFT matrices, the LDS image, 4 OTF-support lists and
# ycol_mix, adjmix_part, 6 work buffers), then the channel's 31 (gather table 4 + its groups 5, scatter table 4, reference
# table 4, W, Wt, Xs, ymat, W16, Wt16, amax, pmax, ymat16, Xs16, bscale, klF, klA, Cpart).  The count is asserted, so that a
# change of plan creation has the figure derived again.
CREATE = {"config1": (c1, None, 65), "two_channel_mid": (mid, 57, 111), "blurred_96": (blurred_96, None, 44)}


@pytest.mark.parametrize("name", list(CREATE))
def test_refused_allocation_in_plan_create(name):
    make, last_k, n_expected = CREATE[name]
    base, t0 = counts()
    t = time.time()
    m = make()
    dt = time.time() - t
    n = counts()[1] - t0
    m.close()
    assert live() == base and n == n_expected
    t = time.time()
    ks = range(1, (last_k or n) + 1)
    for k in ks:
        arm(k)
        with pytest.raises(ValueError, match="hipMalloc"):
            make()
        arm(0)
        assert live() == base, (name, k)
    print(f"{name}: one build {dt:.2f} s and {n} allocations; k = 1..{ks[-1]} refused in {time.time() - t:.2f} s")
