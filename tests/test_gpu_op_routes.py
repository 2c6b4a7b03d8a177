"""Which launches an operator call makes: every route through forward_dev, adjoint_dev, adjoint_tail and template_tail
(surfh_amd/csrc/plan_ops.hip), pinned as the ordered {stage: launches} mapping of ``model.profile()``.

Every launch on these paths sits inside a profile bracket, and the profile lists the stages by name, so the mapping of one call
names its head (where the operand comes from: pixels, the caller's scaled half spectra, spectra already in
``mhat``, plane-wise vectors in either layout), its tail (pixels, scaled half spectra with mu and the prior folded in, the
template transpose, plane-wise with or without the folded prior) and everything between.  The tables below are recorded runs: they
are the specification of which route a call takes, and a change of how the operators are told their mode (``OpCall``,
plan_internal.h) must leave them as they are.  Each row asserts the property of its plan that puts it on its route, so that a row
cannot quietly test another one, and that the route the plan holds (``surfh_debug_dims(plan, "route" / "route2")``) is the one
``surfh_route_decide`` -- the host-only call of the function plan creation calls, tests/test_route_host.py -- gives for the
plan's shape, switches and scan outcome.  Needs a real MI355X (`-m gpu`)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import problems
from helpers import build_model

pytestmark = pytest.mark.gpu

MU, MU_REG = 1.3, 5e3             # fusion calls
PL_MU, PL_MU_REG = 1.3, 0.07      # plane-wise calls


def dims(m, which):
    d = (C.c_int64 * 4)()
    assert m._L.surfh_debug_dims(m._plan, which.encode(), d) == 0
    return tuple(int(v) for v in d)


# ---- the plans: name -> (environment at plan creation, builder, precondition) --------------------------------------------------
def _mid():
    return build_model(problems.two_channel_mid())


def _ct300():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from dist_worker import small_problem
    from surfh_amd.models import spectroSigRLSCT
    prob = small_problem(300)
    return spectroSigRLSCT(prob["sotf"], prob["templates"], prob["alpha_axis"], prob["beta_axis"], prob["wavel"], prob["ifus"],
                           prob["step_deg"], prob["pointings"])


def _mixed():
    from test_gpu_variants import _variant_problem
    return build_model(_variant_problem(300, 64, 4))


def _c1(**kw):
    return build_model(problems.config1(), **kw)


def _disjoint_planes():
    cfg = dict(problems.two_channel_disjoint())
    cfg["templates"] = None
    return build_model(cfg)


def _blurred(N):
    from test_gpu_variants import blurred_case
    return blurred_case(L=5, N=N)[2]


def _spectral_small():
    from test_gpu_spec_vectors import spec_problem
    return build_model(spec_problem("A"), with_ref=False)


def _blurred_exact2():
    """blurred_case(L=5, N=300) of test_gpu_variants.py with surfh_config.exact = 2."""
    from surfh_amd import instru
    from surfh_amd.spectro_blind_rectangle import MRSBlurred
    from oracle import surfh_oracle as orc
    from helpers import make_ifu
    N, s = 300, problems.STEP_DEG
    ax = orc.synthetic_axes(N, s)
    spec = orc.ChannelSpec(1.0 / 3600, 1.2 / 3600, (0.0, 0.0), 0.0, 0.196, 12, 3000.0, np.linspace(7, 8, 10), "R")
    sotf = orc.ir2fr(orc.gaussian_psf(np.linspace(7.0, 8.2, 5), problems.STEP), (N, N))
    pts = [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s)]
    return MRSBlurred(sotf, ax, ax, make_ifu(spec), s, instru.CoordList([instru.Coord(a, b) for a, b in pts]), exact=2)


def _spectral_small_exact2():
    from test_gpu_spec_vectors import spec_problem
    return build_model(spec_problem("A"), with_ref=False, exact=2)


def _is_mid(m):
    assert dims(m, "dft") == (1, 1, 1, 1) and m.spec_supported()       # dft_h2 on both axes, the fused adjoint tail
    assert len(m.channels) == 2 and dims(m, "groups")[1] > 0            # two channels (grouped GEMM), grouped scatter
    assert dims(m, "otf")[0] < dims(m, "otf")[1]                        # OTF-support lists


def _is_ct300(m):
    assert dims(m, "dft")[:3] == (2, 2, 1) and m.spec_supported()       # dft_ct on both axes


def _is_mixed(m):
    assert dims(m, "dft") == (2, 1, 1, 0)                               # dft_ct along alpha, dft_h2 along beta


def _is_c1(m):
    assert dims(m, "dft") == (1, 1, 1, 0) and not m.spec_supported()    # interleaved passes, no fused tail
    assert m.ishape[0] == 4


def _is_planar(m):
    assert dims(m, "dft")[2] == 0 and dims(m, "spec")[0] == 2           # planar arrays: the dense products
    assert not m.spec_supported()


def _is_disjoint_planes(m):
    lo, hi, lown, nseg = dims(m, "info")
    assert nseg == 2 and lown < m.ishape[0] == 160 and m.templates is None   # two plane segments, planes no channel observes


def _is_blurred_h2(m):
    assert dims(m, "dft")[:3] == (1, 1, 1) and m.n_planes == 5


def _is_blurred_ct(m):
    assert dims(m, "dft")[:3] == (2, 2, 1) and m.n_planes == 5


def _is_spectral_small(m):
    assert dims(m, "dft") == (1, 1, 1, 1) and m.spec_supported() and m.ishape == (4, 127, 48)


def _whole_spectrum(m):
    assert dims(m, "otf")[0] in (0, dims(m, "otf")[1])                  # no super-tile of the OTF is dropped


def _is_mid_whole_spectrum(m):
    assert dims(m, "dft") == (1, 1, 1, 1) and m.spec_supported()        # SURFH_OTF_SUPPORT=0: the fused passes over every tile
    _whole_spectrum(m)


def _is_mid_lists_only(m):
    _is_mid(m)                                                          # SURFH_OTF_RANGES=0: the lists stay, the k-ranges go
    assert route(m)[5] == 1


def _is_mid_tail_separate(m):
    assert dims(m, "dft") == (1, 1, 1, 0) and not m.spec_supported()    # SURFH_ADJ_FUSED=0: no fused tail, so no lists either
    _whole_spectrum(m)


def _is_mid_unfused_mix(m):
    assert dims(m, "dft") == (1, 1, 1, 1) and not m.spec_supported()    # SURFH_NO_FUSED_MIX=1: the tail stays fused, the mix does not
    _whole_spectrum(m)


def _is_mid_on_ct(m):
    assert dims(m, "dft") == (2, 2, 1, 0) and m.spec_supported()        # SURFH_DFT_H2=0: 128 = 2 x 64 on dft_ct
    assert dims(m, "otf")[0] < dims(m, "otf")[1]


def _is_ct300_lists_only(m):
    _is_ct300(m)
    assert dims(m, "otf")[0] < dims(m, "otf")[1] and route(m)[5] == 0   # dft_ct takes its k-ranges with the lists, or neither


def _is_ct300_whole_spectrum(m):
    _is_ct300(m)
    _whole_spectrum(m)


def _is_mixed_planar(m):
    _is_planar(m)                                                       # SURFH_DFT_CT=0: 300 loses its kernel, the plan goes planar
    assert m.ishape == (4, 300, 64)


def _is_blurred_ct_exact2(m):
    _is_blurred_ct(m)                                                   # exact = 2 concerns the OTF's support: nothing for T = 0
    assert route(m)[3] == 1


def _is_spectral_small_exact2(m):
    assert dims(m, "dft") == (1, 1, 1, 1) and m.spec_supported() and m.ishape == (4, 127, 48)
    _whole_spectrum(m)


PLANS = {
    "mid": ({}, _mid, _is_mid),
    "ct300": ({}, _ct300, _is_ct300),
    "mixed_300x64": ({}, _mixed, _is_mixed),
    "config1": ({}, _c1, _is_c1),
    "config1_dense": ({"SURFH_DFT_DENSE": "1"}, _c1, _is_planar),
    "config1_verify": ({}, lambda: _c1(verify=True), _is_planar),
    "disjoint_planes": ({}, _disjoint_planes, _is_disjoint_planes),
    "blurred_96": ({}, lambda: _blurred(96), _is_blurred_h2),
    "blurred_300": ({}, lambda: _blurred(300), _is_blurred_ct),
    "blurred_300_own_products": ({"SURFH_OTF_PROD": "0"}, lambda: _blurred(300), _is_blurred_ct),
    "spectral_small": ({}, _spectral_small, _is_spectral_small),
    # the switch plans (every switch that feeds the route, on a plan where it changes the route)
    "mid_whole_spectrum": ({"SURFH_OTF_SUPPORT": "0"}, _mid, _is_mid_whole_spectrum),
    "mid_lists_only": ({"SURFH_OTF_RANGES": "0"}, _mid, _is_mid_lists_only),
    "mid_tail_separate": ({"SURFH_ADJ_FUSED": "0"}, _mid, _is_mid_tail_separate),
    "mid_unfused_mix": ({"SURFH_NO_FUSED_MIX": "1"}, _mid, _is_mid_unfused_mix),
    "mid_on_dft_ct": ({"SURFH_DFT_H2": "0"}, _mid, _is_mid_on_ct),
    "ct300_lists_only": ({"SURFH_OTF_RANGES": "0"}, _ct300, _is_ct300_lists_only),
    "ct300_whole_spectrum": ({"SURFH_OTF_SUPPORT": "0"}, _ct300, _is_ct300_whole_spectrum),
    "mixed_300x64_no_dft_ct": ({"SURFH_DFT_CT": "0"}, _mixed, _is_mixed_planar),
    "blurred_300_exact2": ({}, _blurred_exact2, _is_blurred_ct_exact2),
    "spectral_small_exact2": ({}, _spectral_small_exact2, _is_spectral_small_exact2),
}
CONFIG = {"config1_verify": dict(verify=1), "blurred_300_exact2": dict(exact=2), "spectral_small_exact2": dict(exact=2)}

# ---- the route: what the plan holds against what the host-only decision gives for the plan's shape, switches and scan outcome ---
SWITCHES = ("SURFH_DFT_H2", "SURFH_DFT_CT", "SURFH_DFT_DENSE", "SURFH_NO_FUSED_MIX", "SURFH_ADJ_FUSED", "SURFH_OTF_PROD",
            "SURFH_OTF_SUPPORT", "SURFH_OTF_RANGES")                   # bit i of the mask: switch i is on
SWITCH_DEFAULTS = 0b11110011


def route(m):
    """(axis alpha, axis beta, mix loader, product loader, fused tail, support, spectral template tail, spectral-domain calls)"""
    return dims(m, "route") + dims(m, "route2")


def check_route(name, m):
    env = PLANS[name][0]
    mask = SWITCH_DEFAULTS
    for i, k in enumerate(SWITCHES):
        if k in env:
            mask = (mask | 1 << i) if env[k] == "1" else (mask & ~(1 << i))
    planes = getattr(m, "templates", None) is None
    otf = dims(m, "otf")
    scan = 0 if otf[0] in (0, otf[1]) else (2 if mask & 1 << 7 else 1)
    cfg = CONFIG.get(name, {})
    out = (C.c_int64 * 8)()
    assert m._L.surfh_route_decide(m.ishape[-2], m.ishape[-1], 0 if planes else m.ishape[0], dims(m, "trim")[1], cfg.get("verify", 0),
                                   cfg.get("exact", 0), 1, mask, scan, out) == 0
    assert route(m) == tuple(int(v) for v in out), (name, route(m), tuple(out))
_plans = {}


def plan(name, monkeypatch):
    """One plan per name for the whole module; the switches read at plan creation are set around the build only."""
    if name not in _plans:
        env, make, _ = PLANS[name]
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            _plans[name] = make()
    return _plans[name]


@pytest.fixture(scope="module", autouse=True)
def close_plans():
    yield
    for m in _plans.values():
        m.close()
    _plans.clear()


# ---- the calls: inputs first (fixed seeds), then the profile on, then the one call under test; each returns its outputs -------
def start(m):
    m.profile_reset()
    m.profile_enable(True)


def _rng(m):
    return np.random.default_rng(m.isize % 9973)


def forward(m):
    x = _rng(m).random(m.ishape)
    start(m)
    return [m.forward(x)]


def adjoint(m):
    u = _rng(m).standard_normal(m.oshape)
    start(m)
    return [m.adjoint(u)]


def adjoint_ref(m):
    u = _rng(m).standard_normal(m.oshape)
    start(m)
    return [m.adjoint_ref(u)]


def fwadj(m):
    x = _rng(m).random(m.ishape)
    start(m)
    return [m.fwadj(x)]


def _dev(a):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel()), device="cuda:0")
    torch.cuda.synchronize()
    return t


def _host(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _spectra(m):
    import torch
    xt = torch.zeros(m.spec_size, dtype=torch.float32, device="cuda:0")
    m.to_spec_dev(_dev(_rng(m).standard_normal(m.ishape)), xt)
    torch.cuda.synchronize()
    return xt


def forward_spec(m):
    import torch
    xt, y = _spectra(m), torch.empty(m.osize, dtype=torch.float32, device="cuda:0")
    start(m)
    m.forward_spec_dev(xt, y)
    return _host(y)


def adjoint_spec(m, with_dt):
    import torch
    xt, y = _spectra(m), _dev(_rng(m).standard_normal(m.osize))
    qt = torch.empty_like(xt)
    start(m)
    if with_dt:
        m.adjoint_spec_dev(y, qt, MU, dt_t=xt, mu_reg=MU_REG)
    else:
        m.adjoint_spec_dev(y, qt, MU)
    return _host(qt)


def normal_spec(m, mu_reg):
    import torch
    xt = _spectra(m)
    qt = torch.empty_like(xt)
    start(m)
    m.normal_spec_dev(xt, qt, MU, mu_reg)
    return _host(qt)


def adjoint_templates(m):
    rng = _rng(m)
    u, maps = rng.standard_normal(m.osize), rng.random(m.ishape)
    start(m)
    return [m.adjoint_templates(u, maps)]


def cg_templates(m):
    rng = _rng(m)
    y, maps = rng.random(m.osize), rng.random(m.ishape)
    start(m)
    s, gn, nit = m.cg_templates(y, maps, mu=MU, mu_spec=0.5, max_iter=1)
    assert nit == 1
    return [s, gn]


def cg_nonneg(m):
    rng = _rng(m)
    y, x0 = rng.random(m.osize), rng.standard_normal(m.ishape)
    start(m)
    res = m.cg_nonneg(y, mu=MU, mu_reg=MU_REG, rho=2.0, x0=x0, outer=1, inner=1)
    assert res.nit == 1
    return [res.x, res.grad_norm]


def cg_sample(m):
    """The point estimate, then the draws: 2, the fewest the Python layer takes, of one iteration each."""
    y = _rng(m).random(m.osize)
    start(m)
    res = m.sample_posterior(y, mu=MU, mu_reg=MU_REG, n_samples=2, seed=11, max_iter=1)
    return [res.x_map, res.mean, res.cov]


def planes_cg(m, native, mu_reg, monkeypatch):
    """surfh_cg_planes_begin_dev and one iteration of _step_dev; SURFH_PLANES_NATIVE is read by the begin call."""
    monkeypatch.setenv("SURFH_PLANES_NATIVE", native)
    rng = _rng(m)
    y, x = _dev(rng.random(m.osize)), _dev(rng.random(m.ishape))
    start(m)
    m.cg_begin_dev(y, x, PL_MU, mu_reg)
    m.cg_step_dev(1, 50)
    rr = m.cg_rr()
    return _host(x) + [rr]


ROWS = {}
for _p in ("mid", "ct300"):
    ROWS.update({
        f"{_p}-forward": (_p, forward), f"{_p}-adjoint": (_p, adjoint), f"{_p}-adjoint_ref": (_p, adjoint_ref), f"{_p}-fwadj": (_p, fwadj),
        f"{_p}-forward_spec": (_p, forward_spec),
        f"{_p}-adjoint_spec": (_p, lambda m: adjoint_spec(m, False)), f"{_p}-adjoint_spec_prior": (_p, lambda m: adjoint_spec(m, True)),
        f"{_p}-normal_spec": (_p, lambda m: normal_spec(m, 0.0)), f"{_p}-normal_spec_prior": (_p, lambda m: normal_spec(m, MU_REG)),
    })
ROWS.update({
    "mid-adjoint_templates": ("mid", adjoint_templates), "mid-cg_templates": ("mid", cg_templates), "mid-cg_sample": ("mid", cg_sample),
    "mixed_300x64-forward": ("mixed_300x64", forward), "mixed_300x64-adjoint": ("mixed_300x64", adjoint),
    "disjoint_planes-forward": ("disjoint_planes", forward), "disjoint_planes-adjoint": ("disjoint_planes", adjoint),
    "disjoint_planes-fwadj": ("disjoint_planes", fwadj),
    "spectral_small-cg_nonneg": ("spectral_small", cg_nonneg),
})
for _p in ("mid_whole_spectrum", "mid_lists_only", "mid_on_dft_ct", "ct300_lists_only", "ct300_whole_spectrum", "spectral_small_exact2"):
    ROWS.update({f"{_p}-forward": (_p, forward), f"{_p}-adjoint": (_p, adjoint), f"{_p}-fwadj": (_p, fwadj),
                 f"{_p}-normal_spec_prior": (_p, lambda m: normal_spec(m, MU_REG))})
for _p in ("mid_tail_separate", "mid_unfused_mix", "mixed_300x64_no_dft_ct"):
    ROWS.update({f"{_p}-forward": (_p, forward), f"{_p}-adjoint": (_p, adjoint), f"{_p}-fwadj": (_p, fwadj)})
for _p in ("config1", "config1_dense", "config1_verify"):
    ROWS.update({f"{_p}-forward": (_p, forward), f"{_p}-adjoint": (_p, adjoint), f"{_p}-adjoint_ref": (_p, adjoint_ref), f"{_p}-fwadj": (_p, fwadj),
                 f"{_p}-adjoint_templates": (_p, adjoint_templates), f"{_p}-cg_templates": (_p, cg_templates)})
for _p in ("blurred_96", "blurred_300", "blurred_300_own_products", "blurred_300_exact2"):
    ROWS.update({f"{_p}-forward": (_p, forward), f"{_p}-adjoint": (_p, adjoint)})
    for _native in ("1", "0") if _p != "blurred_300_exact2" else ("1",):
        for _tag, _mur in (("", 0.0), ("_prior", PL_MU_REG)):
            ROWS[f"{_p}-planes_cg_native{_native}{_tag}"] = (_p, lambda m, mp, n=_native, r=_mur: planes_cg(m, n, r, mp))


def run_row(row, monkeypatch):
    """The ordered [(stage, launches)] of the row's call, and the call's outputs."""
    name, call = ROWS[row]
    m = plan(name, monkeypatch)
    PLANS[name][2](m)
    check_route(name, m)
    try:
        out = call(m, monkeypatch) if "planes_cg" in row else call(m)
        prof = m.profile()
    finally:
        m.profile_enable(False)
    return [(k, int(v[0])) for k, v in prof.items()], out


EXPECTED = {
    "mid-forward": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid-adjoint": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid-adjoint_ref": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "fill_zero": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "spmm_degrid_ref": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid-fwadj": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "mid-forward_spec": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_wblur_fwd": 2, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid-adjoint_spec": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 2, "ymat_from_y": 2},
    "mid-adjoint_spec_prior": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 2, "ymat_from_y": 2},
    "mid-normal_spec": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "mid-normal_spec_prior": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "ct300-forward": {"dft_ct_cols_inv_mix": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "ct300-adjoint": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "ct300-adjoint_ref": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "fill_zero": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_degrid_ref": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "ct300-fwadj": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "ct300-forward_spec": {"dft_ct_cols_inv_mix": 1, "dft_ct_rows_inv": 1, "gemm_wblur_fwd": 2, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "ct300-adjoint_spec": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "ymat_from_y": 2},
    "ct300-adjoint_spec_prior": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "ymat_from_y": 2},
    "ct300-normal_spec": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "ct300-normal_spec_prior": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "mid-adjoint_templates": {"dft_h2_cols_fwd": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_adj": 1, "pad_planes": 1, "spmm_scatter_adj": 2, "tplgrad_spec": 1, "ymat_from_y": 2},
    "mid-cg_templates": {"dft_h2_cols_fwd": 4, "dft_h2_cols_inv_mix": 3, "dft_h2_rows_fwd": 4, "dft_h2_rows_inv": 3, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_adj": 4, "gemm_wblur_fwd": 6, "pad_planes": 1, "spmm_gather_fwd": 6, "spmm_scatter_adj": 8, "tpl_pack": 3, "tpl_prior_add": 3, "tplgrad_spec": 4, "ymat16_from_cpart": 6, "ymat_from_y": 2},
    "mid-cg_sample": {"dft_h2_cols_fwd_adjmix": 9, "dft_h2_cols_inv_mix": 6, "dft_h2_rows_fwd": 9, "dft_h2_rows_inv": 6, "gemm_dft_cols_fwd_maps": 2, "gemm_dft_cols_inv_maps": 3, "gemm_dft_rows_fwd_maps": 2, "gemm_dft_rows_inv_maps": 3, "gemm_wblur_adj": 9, "gemm_wblur_fwd": 12, "po_data": 2, "po_moments": 3, "po_prior": 2, "po_randn": 6, "spmm_gather_fwd": 12, "spmm_scatter_adj": 18, "ymat16_from_cpart": 12, "ymat_from_y": 6},
    "mixed_300x64-forward": {"dft_ct_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "spmm_gather_fwd": 1, "y_from_cpart": 1},
    "mixed_300x64-adjoint": {"dft_ct_cols_fwd": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "disjoint_planes-forward": {"cube_transpose": 1, "dft_h2_cols_fwd": 1, "dft_h2_cols_inv": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_fwd": 2, "specmix_fwd": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "disjoint_planes-adjoint": {"cube_transpose": 1, "dft_h2_cols_fwd": 1, "dft_h2_cols_inv": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "ymat_from_y": 2},
    "disjoint_planes-fwadj": {"cube_transpose": 2, "dft_h2_cols_fwd": 2, "dft_h2_cols_inv": 2, "dft_h2_rows_fwd": 2, "dft_h2_rows_inv": 2, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "specmix_adj": 1, "specmix_fwd": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "spectral_small-cg_nonneg": {"dft_h2_cols_fwd_adjmix": 3, "dft_h2_cols_inv_mix": 2, "dft_h2_rows_fwd": 3, "dft_h2_rows_inv": 2, "gemm_dft_cols_fwd_maps": 3, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 3, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 3, "gemm_wblur_fwd": 2, "nn_project": 1, "nn_spec": 3, "spmm_gather_fwd": 2, "spmm_scatter_adj": 3, "ymat16_from_cpart": 2, "ymat_from_y": 1},
    "config1-forward": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "spmm_gather_fwd": 1, "y_from_cpart": 1},
    "config1-adjoint": {"dft_h2_cols_fwd": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "config1-adjoint_ref": {"dft_h2_cols_fwd": 1, "dft_h2_rows_fwd": 1, "fill_zero": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_degrid_ref": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "config1-fwadj": {"dft_h2_cols_fwd": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_adj": 1, "spmm_gather_fwd": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat16_from_cpart": 1},
    "config1-adjoint_templates": {"dft_h2_cols_fwd": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_adj": 1, "pad_planes": 1, "spmm_scatter_adj": 1, "tplgrad_spec": 1, "ymat_from_y": 1},
    "config1-cg_templates": {"dft_h2_cols_fwd": 4, "dft_h2_cols_inv_mix": 3, "dft_h2_rows_fwd": 4, "dft_h2_rows_inv": 3, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_adj": 4, "gemm_wblur_fwd": 3, "pad_planes": 1, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "tpl_pack": 3, "tpl_prior_add": 3, "tplgrad_spec": 4, "ymat16_from_cpart": 3, "ymat_from_y": 1},
    "config1_dense-forward": {"gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "y_from_cpart": 1},
    "config1_dense-adjoint": {"gemm_dft_cols_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "config1_dense-adjoint_ref": {"fill_zero": 1, "gemm_dft_cols_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_degrid_ref": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "config1_dense-fwadj": {"gemm_dft_cols_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_adj": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat16_from_cpart": 1},
    "config1_dense-adjoint_templates": {"gemm_dft_cols_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_wblur_adj": 1, "otf_conj_mul": 1, "pad_planes": 1, "spmm_scatter_adj": 1, "tplgrad_pix": 1, "ymat_from_y": 1},
    "config1_dense-cg_templates": {"gemm_dft_cols_fwd": 4, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 7, "gemm_dft_rows_fwd": 4, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 7, "gemm_wblur_adj": 4, "gemm_wblur_fwd": 3, "otf_conj_mul": 4, "pad_planes": 1, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "tpl_pack": 3, "tpl_prior_add": 3, "tplgrad_pix": 4, "ymat16_from_cpart": 3, "ymat_from_y": 1},
    "config1_verify-forward": {"gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "y_from_cpart": 1},
    "config1_verify-adjoint": {"fill_zero": 1, "gemm_dft_cols_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "config1_verify-adjoint_ref": {"fill_zero": 1, "gemm_dft_cols_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_degrid_ref": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "config1_verify-fwadj": {"fill_zero": 1, "gemm_dft_cols_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_adj": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "y_from_cpart": 1, "ymat_from_y": 1},
    "config1_verify-adjoint_templates": {"fill_zero": 1, "gemm_dft_cols_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_wblur_adj": 1, "otf_conj_mul": 1, "pad_planes": 1, "spmm_scatter_adj": 1, "tplgrad_pix": 1, "ymat_from_y": 1},
    "config1_verify-cg_templates": {"fill_zero": 4, "gemm_dft_cols_fwd": 4, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 7, "gemm_dft_rows_fwd": 4, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 7, "gemm_wblur_adj": 4, "gemm_wblur_fwd": 3, "otf_conj_mul": 4, "pad_planes": 1, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "tpl_pack": 3, "tpl_prior_add": 3, "tplgrad_pix": 4, "y_from_cpart": 3, "ymat_from_y": 4},
    "blurred_96-forward": {"cube_transpose": 1, "dft_h2_cols_fwd": 1, "dft_h2_cols_inv": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "y_transpose": 1},
    "blurred_96-adjoint": {"cube_transpose": 1, "dft_h2_cols_fwd": 1, "dft_h2_cols_inv": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "y_transpose": 1},
    "blurred_96-planes_cg_native1": {"dft_h2_cols_fwd": 7, "dft_h2_cols_inv": 7, "dft_h2_rows_fwd": 7, "dft_h2_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "scale": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_96-planes_cg_native1_prior": {"dft_h2_cols_fwd": 7, "dft_h2_cols_inv": 7, "dft_h2_rows_fwd": 7, "dft_h2_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_96-planes_cg_native0": {"cube_transpose": 7, "dft_h2_cols_fwd": 7, "dft_h2_cols_inv": 7, "dft_h2_rows_fwd": 7, "dft_h2_rows_inv": 7, "scale": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_96-planes_cg_native0_prior": {"cube_transpose": 7, "dft_h2_cols_fwd": 7, "dft_h2_cols_inv": 7, "dft_h2_rows_fwd": 7, "dft_h2_rows_inv": 7, "prior_add": 3, "scale": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300-forward": {"cube_transpose": 1, "dft_ct_cols_fwd": 1, "dft_ct_cols_inv_prod": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "spmm_gather_fwd": 1, "y_transpose": 1},
    "blurred_300-adjoint": {"cube_transpose": 1, "dft_ct_cols_fwd": 1, "dft_ct_cols_inv_prod": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "spmm_scatter_adj": 1, "y_transpose": 1},
    "blurred_300-planes_cg_native1": {"dft_ct_cols_fwd": 7, "dft_ct_cols_inv_prod": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300-planes_cg_native1_prior": {"dft_ct_cols_fwd": 7, "dft_ct_cols_inv_prod": 4, "dft_ct_cols_inv_prodadd": 3, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300-planes_cg_native0": {"cube_transpose": 7, "dft_ct_cols_fwd": 7, "dft_ct_cols_inv_prod": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "scale": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300-planes_cg_native0_prior": {"cube_transpose": 7, "dft_ct_cols_fwd": 7, "dft_ct_cols_inv_prod": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "prior_add": 3, "scale": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300_own_products-forward": {"cube_transpose": 1, "dft_ct_cols_fwd": 1, "dft_ct_cols_inv": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "y_transpose": 1},
    "blurred_300_own_products-adjoint": {"cube_transpose": 1, "dft_ct_cols_fwd": 1, "dft_ct_cols_inv": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "y_transpose": 1},
    "blurred_300_own_products-planes_cg_native1": {"dft_ct_cols_fwd": 7, "dft_ct_cols_inv": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "scale": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300_own_products-planes_cg_native1_prior": {"dft_ct_cols_fwd": 7, "dft_ct_cols_inv": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300_own_products-planes_cg_native0": {"cube_transpose": 7, "dft_ct_cols_fwd": 7, "dft_ct_cols_inv": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "scale": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300_own_products-planes_cg_native0_prior": {"cube_transpose": 7, "dft_ct_cols_fwd": 7, "dft_ct_cols_inv": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "prior_add": 3, "scale": 3, "specmix_adj": 4, "specmix_fwd": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    # the switch plans
    "mid_whole_spectrum-forward": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid_whole_spectrum-adjoint": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid_whole_spectrum-fwadj": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "mid_whole_spectrum-normal_spec_prior": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "mid_lists_only-forward": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid_lists_only-adjoint": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid_lists_only-fwadj": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "mid_lists_only-normal_spec_prior": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "mid_on_dft_ct-forward": {"dft_ct_cols_inv_mix": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid_on_dft_ct-adjoint": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid_on_dft_ct-fwadj": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "mid_on_dft_ct-normal_spec_prior": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "ct300_lists_only-forward": {"dft_ct_cols_inv_mix": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "ct300_lists_only-adjoint": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "ct300_lists_only-fwadj": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "ct300_lists_only-normal_spec_prior": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "ct300_whole_spectrum-forward": {"dft_ct_cols_inv_mix": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "ct300_whole_spectrum-adjoint": {"dft_ct_cols_fwd": 1, "dft_ct_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "ct300_whole_spectrum-fwadj": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "ct300_whole_spectrum-normal_spec_prior": {"dft_ct_cols_fwd": 1, "dft_ct_cols_inv_mix": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "ymat16_from_cpart": 2},
    "spectral_small_exact2-forward": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "spmm_gather_fwd": 1, "y_from_cpart": 1},
    "spectral_small_exact2-adjoint": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "spectral_small_exact2-fwadj": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "spmm_gather_fwd": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat16_from_cpart": 1},
    "spectral_small_exact2-normal_spec_prior": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 1, "spmm_gather_fwd": 1, "spmm_scatter_adj": 1, "ymat16_from_cpart": 1},
    "mid_tail_separate-forward": {"dft_h2_cols_inv_mix": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid_tail_separate-adjoint": {"dft_h2_cols_fwd": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid_tail_separate-fwadj": {"dft_h2_cols_fwd": 1, "dft_h2_cols_inv_mix": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_adj": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "mid_unfused_mix-forward": {"dft_h2_cols_inv": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_fwd": 1, "spmm_gather_fwd": 2, "y_from_cpart": 2},
    "mid_unfused_mix-adjoint": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_rows_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat_from_y": 2},
    "mid_unfused_mix-fwadj": {"dft_h2_cols_fwd_adjmix": 1, "dft_h2_cols_inv": 1, "dft_h2_rows_fwd": 1, "dft_h2_rows_inv": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 2, "pad_planes": 1, "specmix_fwd": 1, "spmm_gather_fwd": 2, "spmm_scatter_adj": 2, "unpad_planes": 1, "ymat16_from_cpart": 2},
    "mixed_300x64_no_dft_ct-forward": {"gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "y_from_cpart": 1},
    "mixed_300x64_no_dft_ct-adjoint": {"gemm_dft_cols_fwd": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "specmix_adj": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat_from_y": 1},
    "mixed_300x64_no_dft_ct-fwadj": {"gemm_dft_cols_fwd": 1, "gemm_dft_cols_fwd_maps": 1, "gemm_dft_cols_inv": 1, "gemm_dft_cols_inv_maps": 1, "gemm_dft_rows_fwd": 1, "gemm_dft_rows_fwd_maps": 1, "gemm_dft_rows_inv": 1, "gemm_dft_rows_inv_maps": 1, "gemm_wblur_adj": 1, "gemm_wblur_fwd": 1, "pad_planes": 1, "specmix_adj": 1, "specmix_fwd": 1, "spmm_gather_fwd": 1, "spmm_scatter_adj": 1, "unpad_planes": 1, "ymat16_from_cpart": 1},
    "blurred_300_exact2-forward": {"cube_transpose": 1, "dft_ct_cols_fwd": 1, "dft_ct_cols_inv_prod": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "spmm_gather_fwd": 1, "y_transpose": 1},
    "blurred_300_exact2-adjoint": {"cube_transpose": 1, "dft_ct_cols_fwd": 1, "dft_ct_cols_inv_prod": 1, "dft_ct_rows_fwd": 1, "dft_ct_rows_inv": 1, "spmm_scatter_adj": 1, "y_transpose": 1},
    "blurred_300_exact2-planes_cg_native1": {"dft_ct_cols_fwd": 7, "dft_ct_cols_inv_prod": 7, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
    "blurred_300_exact2-planes_cg_native1_prior": {"dft_ct_cols_fwd": 7, "dft_ct_cols_inv_prod": 4, "dft_ct_cols_inv_prodadd": 3, "dft_ct_rows_fwd": 7, "dft_ct_rows_inv": 7, "pn_dir": 1, "pn_prior_dot": 3, "spmm_gather_fwd": 3, "spmm_scatter_adj": 4, "y_transpose": 7},
}


@pytest.mark.parametrize("row", list(ROWS))
def test_launches_of_the_route(row, monkeypatch):
    got, _ = run_row(row, monkeypatch)
    print(row, got)
    assert got == list(EXPECTED[row].items())
