"""The solver's Fourier-domain vectors bin by bin against float64 (needs an MI355X).

The exported CG keeps x, r, d, q, b as scaled half spectra of the maps (include/surfh_amd.h,
surfh_normal_spec_dev and friends).  tests/test_gpu_spectral.py holds that basis against its map-domain twin on the GPU, with
whole-array figures on square images.  Here every spectral call is held against tests/spec_oracle.py -- the layout, the
self / pair factor, zero padding, the prior's diagonal -- with the local measures of tests/helpers.py at TOL = 1e-5 (worst
element, worst template, re / im part, k_alpha row and k_beta column), on the smallest rectangular shapes that reach each branch:

    A (127,  48) T = 4  dft_h2 + fused adjoint tail: first admissible Na, odd Na; even Nb with the Nyquist column kb = 24
    B (128,  51) T = 1  dft_h2 + fused tail: Na equal to its padding; odd Nb (no Nyquist column); T = 1 (the reducer's t < T)
    C (255,  40) T = 3  dft_h2 + fused tail: last admissible Na; 21 columns of KBP = 64
    D (200, 254) T = 4  dft_h2 + fused tail: 128 columns = KBP (no column padding); Nyquist at kb = 127
    E (258,  48) T = 4  Na on dft_ct (3 x 86), Nb on dft_h2: mixed plan
    F ( 48, 260) T = 2  Na on dft_h2 below 127, Nb on dft_ct (4 x 65): no fused tail; even dft_ct axis, Nyquist kb = 130 of 192
    G (260, 267) T = 4  both axes on dft_ct (4 x 65, 3 x 89): OTF-support lists; odd Nb

Each problem is a config-1-like single channel with a small field of view (three slits, two to four dither points) so that it
fits a 40-pixel axis.  The prior's diagonal is held per bin to 1e-6 of itself: 4 sinpif(k / N)^2 takes about ten roundings of
2^-24 from the argument to the product (6e-7); 2 - 2 cospif(2 k / N) cancels at low k and misses the bound by one to two decades
(tests/test_spec_host.py shows both on the CPU).  Measured on an MI355X: 1e-5 to 2.6e-4 with the cosine form (every case, both
kernels), 1.9e-7 to 2.8e-7 with prior_eig.h's dsq.  Every measured value goes to the parity log (test_gpu_parity.note)."""
import ctypes
import functools

import numpy as np
import pytest

import problems
import spec_oracle as so
from helpers import build_model, rel
from oracle import surfh_oracle as orc
from test_gpu_local_parity import FWD_AXES, MAP_AXES, check_local
from test_gpu_parity import note
from weights_oracle import Weighted, wdata

pytestmark = pytest.mark.gpu

SPEC_AXES = dict(template=0, part=1, ka=2, kb=3)        # a vector's valid bins as (T, re / im, ka, kb)
PRIOR_TOL = 1e-6                                        # per bin, relative to the eigenvalue (module docstring)
MU_REG = 5e3

# name: (Na, Nb, T, Lc, fov_alpha ["], fov_beta ["], dither points, (kernel of alpha, kernel of beta, interleaved, fused tail))
CASES = {
    "A": (127, 48, 4, 128, 0.50, 0.55, 4, (1, 1, 1, 1)),
    "B": (128, 51, 1, 96, 0.50, 0.55, 2, (1, 1, 1, 1)),
    "C": (255, 40, 3, 96, 0.55, 0.50, 3, (1, 1, 1, 1)),
    "D": (200, 254, 4, 96, 0.50, 0.55, 2, (1, 1, 1, 1)),
    "E": (258, 48, 4, 96, 0.50, 0.55, 2, (2, 1, 1, 0)),
    "F": (48, 260, 2, 96, 0.50, 0.55, 3, (1, 2, 1, 0)),
    "G": (260, 267, 4, 96, 0.50, 0.55, 2, (2, 2, 1, 0)),
}


def spec_problem(name):
    """A single three-slit channel (config 1's instrument constants) on an Na x Nb image with T of the synthetic templates."""
    Na, Nb, T, Lc, fa, fb, nd, _ = CASES[name]
    rng = np.random.default_rng(1000 + ord(name))
    wav = np.linspace(7.50, 7.70, Lc)
    spec = orc.ChannelSpec(fa / 3600, fb / 3600, (0.0, 0.0), 8.2, 0.196, 3, 3050.0, np.linspace(7.53, 7.67, 40), "S1")
    return dict(N=Na, Lc=Lc, alpha_axis=orc.synthetic_axes(Na, problems.STEP_DEG), beta_axis=orc.synthetic_axes(Nb, problems.STEP_DEG),
                wavel=wav, specs=[spec], templates=orc.synthetic_templates(Lc)[:T],
                sotf=orc.ir2fr(orc.gaussian_psf(wav, problems.STEP), (Na, Nb)),
                pointings=[orc.dither4(spec.det_pix_size, spec.beta_width / spec.n_slit)[:nd]],
                maps=rng.random((T, Na, Nb)), step_deg=problems.STEP_DEG)


class SpecRefs:
    """A case with the float64 oracle's vectors, each computed once and never changed.  The test inputs are float32 values, so the
    device and the oracle start from the same numbers."""

    def __init__(self, name):
        self.name = name
        self.Na, self.Nb, self.T = CASES[name][:3]
        self.dft = CASES[name][7]
        self.cfg = spec_problem(name)
        self.om = problems.oracle_model(self.cfg, box="direct")
        self.KAP, self.KBP = so.pads(self.Na, self.Nb)
        self.hb = self.Nb // 2 + 1
        self.vshape = (self.T, 2, self.KAP, self.KBP)
        self.valid = np.broadcast_to(so.valid_mask(self.Na, self.Nb, self.KAP, self.KBP), self.vshape)
        rng = np.random.default_rng(2000 + ord(name))
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        self.x = f32(rng.standard_normal(self.om.ishape))           # white maps: every row and column of the spectrum at its own scale
        self.maps = f32(self.cfg["maps"])                           # uniform maps: the DC bin about 250 times the rest
        self.y = f32(rng.standard_normal(self.om.osize))
        self.x0 = f32(0.5 * rng.random(self.om.ishape))
        self.eig = np.zeros(self.vshape)
        self.eig[:, :, :self.Na, :self.hb] = so.prior_eig(self.Na, self.Nb)

    def spec(self, x):
        return so.to_spec(x, self.KAP, self.KBP)

    def bins(self, v):
        """The valid bins of a vector [T][2][KAP][KBP] as (T, 2, Na, hb)."""
        return np.asarray(v).reshape(self.vshape)[:, :, :self.Na, :self.hb]

    @functools.cached_property
    def fwd(self):
        return self.om.forward(self.maps)

    @functools.cached_property
    def adj(self):
        return self.om.adjoint(self.y)

    @functools.cached_property
    def normal(self):
        return so.normal(self.om, self.x, 1.0, MU_REG, self.KAP, self.KBP)

    @functools.cached_property
    def data(self):
        """Noisy data of the uniform maps, as test_gpu_parity.test_cg_matches_oracle_lcg makes them."""
        y = self.fwd
        return y + np.random.default_rng(1).standard_normal(y.size) * 1e-2 * np.sqrt(np.mean(y ** 2))

    @functools.cached_property
    def weights(self):
        """Inverse variances with a block of zeros (one slit's samples at ten detector wavelengths, every pointing)."""
        w = np.exp(np.random.default_rng(3).uniform(np.log(0.5), np.log(2.0), self.om.channels[0].oshape))
        w[:, 1, 10:20, :] = 0.0
        return w.ravel()

    @functools.lru_cache(maxsize=None)
    def cg(self, weighted=False):
        if weighted:
            return orc.lcg(Weighted(self.om, self.weights), wdata(self.weights, self.data), 1.0, MU_REG, self.x0, tol=1e-12, max_iter=5)
        return orc.lcg(self.om, self.data, 1.0, MU_REG, self.x0, tol=1e-12, max_iter=5)


@functools.lru_cache(maxsize=None)
def refs(name):
    return SpecRefs(name)


def debug_dims(m, which):
    dims = (ctypes.c_int64 * 4)()
    assert m._L.surfh_debug_dims(m._plan, which.encode(), dims) == 0
    return tuple(int(v) for v in dims)


class Dev:
    """Device vectors of a case: float32 tensors in, host arrays out, the plan's stream and torch's kept in step."""

    def __init__(self, r, m):
        import torch
        self.torch, self.r, self.m = torch, r, m
        self.n = m.spec_size

    def put(self, a):
        t = self.torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel()), device="cuda:0")
        self.torch.cuda.synchronize()
        return t

    def poisoned(self, n=None):
        t = self.torch.full((self.n if n is None else n,), float("nan"), dtype=self.torch.float32, device="cuda:0")
        self.torch.cuda.synchronize()
        return t

    def get(self, t, shape=None):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().reshape(self.r.vshape if shape is None else shape)

    def ones_on_valid(self):
        return self.put(self.r.valid.astype(np.float32))


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    """One plan and one oracle model per case for all the tests of the module."""
    r = refs(request.param)
    m = build_model(r.cfg)
    yield r, m, Dev(r, m)
    m.close()


def check_vector(name, r, v, ref, **tags):
    """A device vector against the oracle's: padding exactly zero, the valid bins on every local measure at TOL."""
    v = np.asarray(v).reshape(r.vshape)
    assert not v[~r.valid].any(), f"{name} {tags}: {np.count_nonzero(v[~r.valid])} non-zero padding entries"
    return check_local(name, r.bins(v), r.bins(ref), SPEC_AXES, case=r.name, **tags)


def check_prior_diagonal(name, r, w, mu_reg, **tags):
    """``w`` [T][2][KAP][KBP]: mu_reg times the device's diagonal, one value per entry.  Every valid bin within PRIOR_TOL of its
    eigenvalue, bin (0, 0) and the padding exactly zero."""
    w = np.asarray(w, dtype=np.float64).reshape(r.vshape)
    ref = mu_reg * r.eig
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(ref > 0, np.abs(w - ref) / ref, 0.0)
    e[~np.isfinite(w)] = np.inf
    at = tuple(int(i) for i in np.unravel_index(int(np.argmax(e)), e.shape))
    low = float(np.max(e[:, :, [1, r.Na - 1], 0]))                      # the bins next to DC along alpha: where the cos form cancels most
    note(name, case=r.name, worst=float(e.max()), worst_at=list(at), lowest_alpha_bins=low, **tags)
    print(name, r.name, tags, f"worst {e.max():.2e} at (t, part, ka, kb) = {at}; bins (1, 0) and (Na - 1, 0): {low:.2e}")
    assert not w[:, :, 0, 0].any(), "bin (0, 0) of the prior's diagonal must be exactly zero"
    assert not w[~r.valid].any(), "padding of the prior's diagonal must be exactly zero"
    assert e.max() <= PRIOR_TOL, f"{name} {r.name}: per-bin error {e.max():.3e} at (t, part, ka, kb) = {at} (bound {PRIOR_TOL:g})"


# ---- the plan is the one the table says --------------------------------------------------------------------------------------
def test_path_and_layout(case):
    r, m, d = case
    dft, otf = debug_dims(m, "dft"), debug_dims(m, "otf")[:2]
    note("spec_path", case=r.name, dft=list(dft), otf=list(otf), spec_size=int(m.spec_size))
    print(r.name, "dft", dft, "otf", otf, "spec_size", m.spec_size)
    assert m.spec_supported()
    assert m.spec_size == 2 * r.T * r.KAP * r.KBP
    assert dft == r.dft, (r.name, dft)
    if r.name in "EF":
        assert 0 < otf[0] == otf[1]                              # one axis on each kernel: no OTF-support lists
    else:
        assert 0 < otf[0] < otf[1]                               # some, not all, super-tiles inside the OTF's support: the lists are on


# ---- a. maps -> vector ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "uniform"])
def test_to_spec(case, kind):
    r, m, d = case
    x = r.x if kind == "normal" else r.maps
    xd, out = d.put(x), d.poisoned()
    m.to_spec_dev(xd, out)
    v = d.get(out).copy()
    check_vector("spec_to_spec", r, v, r.spec(x), data=kind)
    out2 = d.poisoned()
    m.to_spec_dev(xd, out2)
    assert np.array_equal(d.get(out2), v)


# ---- b. vector -> maps ---------------------------------------------------------------------------------------------------------
def test_from_spec(case):
    r, m, d = case
    back = d.poisoned(m.isize)
    m.from_spec_dev(d.put(r.spec(r.x)), back)
    check_local("spec_from_spec", d.get(back, m.ishape), r.x, MAP_AXES, case=r.name)


# ---- c. forward from a vector --------------------------------------------------------------------------------------------------
def test_forward_spec(case):
    r, m, d = case
    y = d.poisoned(m.osize)
    m.forward_spec_dev(d.put(r.spec(r.maps)), y)
    ch = r.om.channels[0]
    check_local("spec_forward", d.get(y, ch.oshape), r.fwd.reshape(ch.oshape), FWD_AXES, case=r.name)


# ---- d. adjoint into a vector --------------------------------------------------------------------------------------------------
def test_adjoint_spec(case):
    r, m, d = case
    yd, qt = d.put(r.y), d.poisoned()
    m.adjoint_spec_dev(yd, qt, mu=0.37)
    v = d.get(qt).copy()
    # the columns beyond the OTF's support fall under the same measures: about zero, not what the buffers held before
    check_vector("spec_adjoint", r, v, r.spec(0.37 * r.adj))
    qt2 = d.poisoned()
    m.adjoint_spec_dev(yd, qt2, mu=0.37)
    assert np.array_equal(d.get(qt2), v)


# ---- e. the fused prior alone --------------------------------------------------------------------------------------------------
def test_fused_prior_diagonal(case):
    """Zero data and a vector of ones: the data term is exactly zero, what the adjoint's last kernel writes is mu_reg times the
    prior's diagonal, bins outside the OTF's support included."""
    r, m, d = case
    qt = d.poisoned()
    m.adjoint_spec_dev(d.put(np.zeros(m.osize)), qt, mu=1.0, dt_t=d.ones_on_valid(), mu_reg=3.0)
    check_prior_diagonal("spec_prior_fused", r, d.get(qt), 3.0)


# ---- f. the prior as its own kernel --------------------------------------------------------------------------------------------
def test_prior_spec_add(case):
    r, m, d = case
    ones = d.ones_on_valid()
    q = d.put(np.zeros(r.vshape))
    m.prior_spec_add_dev(ones, q, 3.0)
    inc = d.get(q).copy()
    check_prior_diagonal("spec_prior_add", r, inc, 3.0)
    # onto a vector that holds something, padding included: the increment times 1 is exact, so the sum is the fp32 sum of the two
    # (whether the kernel multiplies and adds or fuses them), and the padding is not touched
    q0 = np.random.default_rng(5).standard_normal(r.vshape).astype(np.float32)
    q = d.put(q0)
    m.prior_spec_add_dev(ones, q, 3.0)
    got = d.get(q)
    assert np.array_equal(got[~r.valid], q0[~r.valid])
    assert np.array_equal(got[r.valid], (q0 + inc)[r.valid])


# ---- g. fused against split, and against float64 -------------------------------------------------------------------------------
def test_normal_fused_against_split(case):
    """normal_spec_dev with the prior folded in (one GPU) against normal_spec_dev + prior_spec_add_dev (the multi-rank form, the
    all-reduce of q between them): kernels.h promises the same arithmetic."""
    r, m, d = case
    dt = d.put(r.spec(r.x))
    q1, q2 = d.poisoned(), d.poisoned()
    m.normal_spec_dev(dt, q1, 1.0, MU_REG)
    m.normal_spec_dev(dt, q2, 1.0, 0.0)
    m.prior_spec_add_dev(dt, q2, MU_REG)
    v1, v2 = d.get(q1).astype(np.float64), d.get(q2).astype(np.float64)
    gap = float(np.max(np.abs(v1 - v2)) / np.max(np.abs(v1)))
    note("spec_fused_vs_split", case=r.name, gap=gap)
    print(r.name, f"fused against split: {gap:.2e}")
    assert gap <= 1e-6
    assert not v2[~r.valid].any()
    check_vector("spec_normal", r, v1, r.normal)


# ---- h. no state left behind ---------------------------------------------------------------------------------------------------
def test_no_state_left_behind(case):
    r, m, d = case
    a0, f0 = m.adjoint(r.y), m.forward(r.maps)
    dt, q, y = d.put(r.spec(r.x)), d.poisoned(), d.poisoned(m.osize)
    m.normal_spec_dev(dt, q, 2.0, MU_REG)
    m.forward_spec_dev(dt, y)
    m.adjoint_spec_dev(d.put(r.y), q, mu=0.37, dt_t=dt, mu_reg=3.0)
    d.get(q)
    assert np.array_equal(m.adjoint(r.y), a0) and np.array_equal(m.forward(r.maps), f0)


# ---- i. five CG iterations -----------------------------------------------------------------------------------------------------
def cg_against(name, r, got, ref, tol_x, tol_rr, **tags):
    x, gn, nit = got
    gr = np.asarray(ref["grad_norm"])
    e_x, e_rr = rel(x, ref["x"]), np.abs(np.asarray(gn) - gr) / gr
    note(name, case=r.name, err_x=e_x, err_rr=[float(v) for v in e_rr], **tags)
    print(name, r.name, tags, f"x {e_x:.2e}; r.r", " ".join(f"{v:.1e}" for v in e_rr))
    assert nit == 5 and len(gn) == 6
    assert e_x < tol_x and np.all(e_rr < tol_rr), (e_x, e_rr)


def test_cg_five_iterations(case, monkeypatch):
    """The exported solver on the spectral loop from a non-zero start, at the bounds of test_gpu_parity.test_cg_matches_oracle_lcg
    (3e-3 on the iterate, 2e-4 on every r.r); on C with inverse-variance weights and a block of zeros as well."""
    r, m, d = case
    kw = dict(mu=1.0, mu_reg=MU_REG, x0=r.x0, max_iter=5, tol=1e-12)
    got = m.cg(r.data, **kw)
    cg_against("spec_cg", r, got, r.cg(), 3e-3, 2e-4)
    if r.name == "C":
        cg_against("spec_cg_weighted", r, m.cg(r.data, weights=r.weights, **kw), r.cg(True), 3e-3, 2e-4)
    if r.name in ("A", "F"):
        # the same solve on the maps, at the bounds tests/test_gpu_spectral.py uses at N = 300 for iterations that early
        monkeypatch.setenv("SURFH_SPECTRAL_CG", "0")
        m2 = build_model(r.cfg)
        try:
            xm, gm, _ = m2.cg(r.data, **kw)
        finally:
            m2.close()
        e_it, e_x = np.abs(np.asarray(got[1]) - gm) / gm, rel(got[0], xm)
        note("spec_cg_vs_maps", case=r.name, err_x=e_x, err_rr=[float(v) for v in e_it])
        print(r.name, "spectral against map-domain loop:", " ".join(f"{v:.1e}" for v in e_it), f"; x {e_x:.2e}")
        assert np.max(e_it[:4]) < 1e-4 and np.max(e_it) < 1e-2 and e_x < 5e-3


# ---- errors --------------------------------------------------------------------------------------------------------------------
def spectral_calls(m, d, n):
    dt, q, y, x = d.put(np.zeros(n)), d.put(np.zeros(n)), d.put(np.zeros(m.osize)), d.put(np.zeros(m.isize))
    return dict(to_spec=lambda: m.to_spec_dev(x, q), from_spec=lambda: m.from_spec_dev(dt, x),
                forward_spec=lambda: m.forward_spec_dev(dt, y), adjoint_spec=lambda: m.adjoint_spec_dev(y, q, 1.0),
                adjoint_spec_prior=lambda: m.adjoint_spec_dev(y, q, 1.0, dt, 3.0), normal_spec=lambda: m.normal_spec_dev(dt, q, 1.0, 0.0),
                normal_spec_prior=lambda: m.normal_spec_dev(dt, q, 1.0, 3.0), prior_spec_add=lambda: m.prior_spec_add_dev(dt, q, 3.0))


def test_unsupported_plan_refuses_every_spectral_call():
    """Config 1 (64 x 64: dft_h2 without the fused adjoint tail) has no spectral-domain calls: each of them is an error."""
    cfg = problems.config1()
    m = build_model(cfg)
    try:
        assert not m.spec_supported()
        for name, call in spectral_calls(m, Dev(None, m), m.spec_size).items():
            with pytest.raises(RuntimeError):
                call()
    finally:
        m.close()


def test_joint_prior_refuses_the_spectral_prior():
    """The spectral prior is the separated first differences.  Under the joint Laplacian the calls that would apply it are errors,
    the data half still works, and cg runs on the maps and matches the float64 oracle with that prior."""
    r = refs("A")
    m = build_model(r.cfg)
    d = Dev(r, m)
    try:
        dt, q_sep, q_joint = d.put(r.spec(r.x)), d.poisoned(), d.poisoned()
        m.normal_spec_dev(dt, q_sep, 1.0, 0.0)
        v_sep = d.get(q_sep).copy()
        m.set_prior("joint")
        try:
            assert not m.spec_supported()
            calls = spectral_calls(m, d, m.spec_size)
            for name in ("adjoint_spec_prior", "normal_spec_prior", "prior_spec_add"):
                with pytest.raises(RuntimeError):
                    calls[name]()
            m.normal_spec_dev(dt, q_joint, 1.0, 0.0)
            assert np.array_equal(d.get(q_joint), v_sep)
            reg = orc.reg_freq((r.Na, r.Nb), "joint")[None]

            def q_of(v):
                return r.om.adjoint(r.om.forward(v)) + MU_REG * np.fft.irfft2(reg * np.fft.rfft2(v, norm="ortho"), s=(r.Na, r.Nb), norm="ortho")
            ref = so.lcg(q_of, r.om.adjoint(r.data), r.x0, 5)
            cg_against("spec_cg_joint_prior", r, m.cg(r.data, mu=1.0, mu_reg=MU_REG, x0=r.x0, max_iter=5, tol=1e-12), ref, 3e-3, 2e-4)
        finally:
            m.set_prior("separated")
        assert m.spec_supported()
        m.normal_spec_dev(dt, q_joint, 1.0, MU_REG)
        check_vector("spec_normal_after_joint", r, d.get(q_joint), r.normal)
    finally:
        m.close()
