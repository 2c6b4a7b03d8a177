"""Inputs and float64 references of the Model_WCT path tests (tests/test_gpu_wct_paths.py, tests/test_wct_checks_host.py).

A case is (shape, L, T) with the transform path the plan must take: ``dft`` = (kernel of the alpha axis, kernel of the beta
axis, interleaved complex arrays, fused adjoint tail) with 0 = dense, 1 = dft_h2, 2 = dft_ct, and ``lists`` = OTF support
lists in use (None: decided by the OTF, see ``otf_tiles``).  Everything here is numpy float64; nothing needs a GPU."""
import functools

import numpy as np

from helpers import max_err
from oracle import surfh_oracle as orc

# id: (shape, L, T, dft, lists, psf)
CASES = {
    "h2_control": ((40, 36), 24, 3, (1, 1, 1, 0), False, "noisy"),            # the golden's shape: dft_h2, separate reduction
    "h2_fused_first": ((127, 40), 130, 4, (1, 1, 1, 1), False, "noisy"),      # fused tail at the first admissible Na, LP 256
    "h2_fused_last_T1": ((255, 33), 24, 1, (1, 1, 1, 1), False, "noisy"),     # fused tail at the last Na, Nb at the kernel's lower limit
    "h2_T5": ((127, 40), 130, 5, (1, 1, 1, 0), False, "noisy"),               # T > 4 takes the separate reduction
    "h2_T8_LP384": ((128, 64), 300, 8, (1, 1, 1, 0), False, "noisy"),         # Na equal to its padding, second stride of the Hessian's l loop
    "ct_mixed": ((300, 64), 130, 4, (2, 1, 1, 0), False, "noisy"),            # one axis on dft_ct, no lists
    "ct_lists": ((256, 256), 24, 3, (2, 2, 1, 0), None, "noisy"),             # both axes on dft_ct, T <= 4: the lists follow the OTF
    "ct_T8": ((256, 256), 24, 8, (2, 2, 1, 0), False, "noisy"),               # dft_ct, T > 4: no lists
    "dense_prime": ((257, 64), 130, 5, (0, 0, 0, 0), False, "noisy"),         # planar arrays
    "dense_short_T8": ((20, 48), 24, 8, (0, 0, 0, 0), False, "noisy"),        # planar arrays, smallest PL
    "band_limited": ((251, 130), 140, 3, (1, 1, 1, 1), True, "clean"),        # fused tail with 0 < otf[0] < otf[1]
    "ct_band_limited": ((256, 256), 24, 3, (2, 2, 1, 0), True, "clean"),      # both axes on dft_ct with lists that drop tiles
}
JOINT = ("h2_fused_first", "dense_prime")             # cases that also run gradient="joint"
SINGULAR = ("h2_fused_first", "ct_lists", "dense_prime")
MU_SMALL = 1e-3
RIDGE = 10.0          # added to |D(f)|^2 where the spectra are linearly dependent: the prior alone is zero at the zero frequency


def bump_spectra(T, L):
    """T Gaussian bumps along lambda plus a floor: the T x T systems stay well conditioned for every T up to 8."""
    l, t = np.arange(L)[None, :], np.arange(T)[:, None]
    return 0.05 + np.exp(-0.5 * ((l - (t + 0.5) * L / T) / (0.35 * L / T)) ** 2)


def noisy_psfs(shape, L, rng):
    """As tests/test_gpu_dft.build: not symmetric, so the OTF is complex."""
    hs, ws = min(15, shape[0]), min(13, shape[1])
    yy, xx = np.mgrid[0:hs, 0:ws]
    sig = np.linspace(1.0, 3.0, L)
    psfs = np.exp(-((yy - hs // 2) ** 2 + (xx - ws // 2) ** 2)[None] / (2.0 * sig[:, None, None] ** 2))
    psfs = psfs * (1.0 + 0.1 * rng.standard_normal(psfs.shape))
    return psfs / psfs.sum(axis=(1, 2), keepdims=True)


def clean_psfs(L, sig=(5.0, 2.5)):
    """The clean 81 x 81 Gaussians of test_gpu_dft.test_otf_support_lists: a band-limited OTF."""
    yy, xx = np.mgrid[0:81, 0:81]
    s = np.linspace(sig[0], sig[1], L)
    psfs = np.exp(-((yy - 40) ** 2 + (xx - 40) ** 2)[None] / (2.0 * s[:, None, None] ** 2))
    return psfs / psfs.sum(axis=(1, 2), keepdims=True)


def otf_tiles(otf):
    """(super-tiles kept, all super-tiles) by the plan's rule: a (k_beta, 128-wavelength chunk) tile is kept when some plane of
    the chunk has, at that k_beta or a higher one, an entry above 2^-24 of the plane's peak."""
    L, _, nkb = otf.shape
    nch = (L + 127) // 128
    m2 = np.abs(otf) ** 2
    km = m2.max(axis=1)                                                       # [L][k_beta]
    over = km > km.max(axis=1, keepdims=True) * 2.0 ** -48
    last = np.where(over.any(axis=1), nkb - 1 - np.argmax(over[:, ::-1], axis=1), -1)
    bmax = [last[j * 128:(j + 1) * 128].max() for j in range(nch)]
    return int(sum(b + 1 for b in bmax)), nkb * nch


def hessian(specs, otf):
    """einsum("tl,ul,lij->tuij", specs, specs, |otf|^2) as one matrix product."""
    T, L = specs.shape
    ss = (specs[:, None, :] * specs[None, :, :]).reshape(T * T, L)
    return (ss @ (np.abs(otf) ** 2).reshape(L, -1)).reshape((T, T) + otf.shape[1:])


def apply_hessian(hth, x, shape):
    """The numpy stand-in for fwadj: idft(hth dft(x))."""
    return orc.idft(np.einsum("tuij,uij->tij", hth, orc.dft(np.asarray(x, dtype=np.float64))), shape)


def solve_hessian(hth, b, mu, reg, shape, fp32=False):
    """The numpy stand-in for expsol: (hth + diag(mu) reg) x = b per frequency, b the half spectra [T][Na][Nb/2+1] of H^T y.
    ``fp32``: the Hessian and the right-hand side each rounded once to fp32 before the float64 solve."""
    T = hth.shape[0]
    mu = np.ones(T) * mu if np.isscalar(mu) else np.asarray(mu, dtype=np.float64)
    if fp32:
        hth = hth.astype(np.float32).astype(np.float64)
        b = b.astype(np.complex64).astype(np.complex128)
    A = np.moveaxis(hth, (0, 1), (-2, -1)) + reg[:, :, None, None] * np.diag(mu)[None, None]
    xf = np.linalg.solve(A, np.moveaxis(b, 0, -1)[..., None])[..., 0]
    return orc.idft(np.moveaxis(xf, -1, 0), shape)


class Case:
    """Inputs of one case and the oracle's outputs, each computed once and never changed."""

    def __init__(self, name, specs=None, T=None):
        self.name = name
        self.shape, self.L, T0, self.dft, self.lists, kind = CASES[name]
        self.T = T or T0
        rng = np.random.default_rng(sum(map(ord, name)))
        self.psfs = noisy_psfs(self.shape, self.L, rng) if kind == "noisy" else clean_psfs(self.L)
        self.pce = 0.5 + rng.random(self.L)
        self.specs = bump_spectra(self.T, self.L) if specs is None else specs(bump_spectra(self.T, self.L))
        self.wo = orc.WCTOracle(self.psfs, self.specs, self.shape, self.pce)
        self.x = dict(uniform=rng.random(self.wo.ishape), zero_mean=rng.standard_normal(self.wo.ishape))
        self.cube = rng.standard_normal(self.wo.oshape)
        self.maps = rng.random(self.wo.ishape)

    @functools.cached_property
    def data(self):
        """A cube the model explains up to 1 % noise: the closed form then returns maps of the scale of ``maps``."""
        y = self.wo.forward(self.maps)
        return y + 0.01 * np.abs(y).max() * np.random.default_rng(9).standard_normal(y.shape)

    @functools.cached_property
    def hth(self):
        return hessian(self.specs, self.wo.otf)

    @functools.cached_property
    def rhs(self):
        return orc.dft(self.wo.adjoint(self.data))

    @functools.lru_cache(maxsize=None)
    def fwadj(self, kind):
        return self.wo.fwadj(self.x[kind])

    def mu(self, mu):
        """``mu``: a number, or "list" for geomspace(1e-3, 10, T)."""
        return np.geomspace(1e-3, 10, self.T) if mu == "list" else mu

    def reg(self, gradient="separated", ridge=0.0):
        return orc.reg_freq(self.shape, gradient) + ridge

    @functools.lru_cache(maxsize=None)
    def expsol(self, mu, gradient="separated"):
        return self.wo.expsol(self.data, self.mu(mu), gradient)

    @functools.lru_cache(maxsize=None)
    def solve(self, mu, gradient="separated", ridge=0.0, fp32=False):
        """WCTOracle.expsol restated with the prior's |D(f)|^2 as an argument (equal to it to 1e-14 where ridge = 0:
        tests/test_wct_checks_host.py)."""
        return solve_hessian(self.hth, self.rhs, self.mu(mu), self.reg(gradient, ridge), self.shape, fp32)

    def precondition(self, mu, gradient="separated", ridge=0.0):
        """Worst element by which the float64 solve moves when its Hessian and right-hand side are rounded once to fp32: what
        no fp32 kernel can avoid.  From the reference alone."""
        return max_err(self.solve(mu, gradient, ridge, True), self.solve(mu, gradient, ridge))

    def condition(self, mu, ridge=0.0):
        """Median and largest 2-norm condition number of the T x T systems over the frequencies."""
        m = np.ones(self.T) * self.mu(mu)
        A = np.moveaxis(self.hth, (0, 1), (-2, -1)) + self.reg(ridge=ridge)[:, :, None, None] * np.diag(m)[None, None]
        c = np.linalg.cond(A)
        return float(np.median(c)), float(c.max())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def sum_of_first_two(specs):
    specs = specs.copy()
    specs[-1] = specs[0] + specs[1]
    return specs


def two_equal(specs):
    specs = specs.copy()
    specs[5] = specs[2]
    return specs
