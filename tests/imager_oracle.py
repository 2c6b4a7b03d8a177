"""Float64 restatement of the imager operator (include/surfh_amd.h: surfh_set_imager), written from its definition:

    cube[l]  = sum_t tpl[t,l] x[t]
    blur[l]  = irfft2(rfft2(cube[l], norm="ortho") * sotf[l], s=(Na, Nb), norm="ortho")          (spectroModel.py:166)
    z[f]     = sum_l wf[f,l] blur[l]
    y_im[f,a,b] = sum_{i<d, j<d} z[f, a d + i, b d + j],   a < Na // d, b < Nb // d

``ImagerOracle`` evaluates it plane by plane (``forward``), its exact transpose (``adjoint``), the weighted normal operator
(``fwadj``), and the same operator through G[f,t,k] = sum_l wf[f,l] tpl[t,l] sotf[l,k] (``forward_g`` / ``adjoint_g``; ``fast=True``
makes these the ones ``forward`` / ``adjoint`` run, for the solver tests).  The transpose is exact for OTFs of real point-spread
functions (what ``ir2fr`` gives), the only ones the spectrometer's own adjoint is exact for.

``Joint`` stacks a spectrometer oracle and the imager into one least-squares problem, the way ``weights_oracle.Weighted`` folds
the weights in:   mu |y - A x|^2_W + mu_im |y_im - A_im x|^2_Wim  =  mu |y~ - A~ x|^2   with
A~ = [W^1/2 A ; (mu_im / mu)^1/2 Wim^1/2 A_im],  y~ likewise (``Joint.data``), so the unchanged ``orc.lcg``, ``orc.mmmg``,
``huber_oracle.mmmg`` and ``orc.crit_val`` minimise and evaluate the joint criterion."""
from __future__ import annotations

import numpy as np

import problems  # noqa: F401  (puts the repository root on sys.path for `oracle`)


def sample(z, d):
    """[F, Na, Nb] -> [F, Na // d, Nb // d]: sums over whole d x d tiles, the rest is not observed."""
    F, Na, Nb = z.shape
    na, nb = Na // d, Nb // d
    return z[:, :na * d, :nb * d].reshape(F, na, d, nb, d).sum(axis=(2, 4))


def spread(y, d, imshape):
    """The transpose of ``sample``."""
    F, na, nb = y.shape
    z = np.zeros((F,) + tuple(imshape))
    z[:, :na * d, :nb * d] = np.repeat(np.repeat(y, d, axis=1), d, axis=2)
    return z


def build_g(sotf, tpl, filters):
    """G [F, T, Na, Nb//2+1] complex128."""
    return np.einsum("fl,tl,lab->ftab", filters, tpl, sotf)


class ImagerOracle:
    def __init__(self, sotf, tpl, filters, d, imshape, fast=False):
        self.sotf = np.asarray(sotf, dtype=np.complex128)
        self.tpl = np.asarray(tpl, dtype=np.float64)
        self.wf = np.atleast_2d(np.asarray(filters, dtype=np.float64))
        self.d, self.imshape = int(d), tuple(imshape)
        self.ishape = (self.tpl.shape[0],) + self.imshape
        self.oshape = (self.wf.shape[0], self.imshape[0] // self.d, self.imshape[1] // self.d)
        self.G = build_g(self.sotf, self.tpl, self.wf)
        if fast:
            self.forward, self.adjoint = self.forward_g, self.adjoint_g

    @property
    def isize(self):
        return int(np.prod(self.ishape))

    @property
    def osize(self):
        return int(np.prod(self.oshape))

    def _blur(self, cube, otf):
        return np.fft.irfft2(np.fft.rfft2(cube, norm="ortho") * otf, s=self.imshape, norm="ortho")

    def forward(self, x):
        cube = np.einsum("tl,tab->lab", self.tpl, np.asarray(x, dtype=np.float64).reshape(self.ishape))
        return sample(np.einsum("fl,lab->fab", self.wf, self._blur(cube, self.sotf)), self.d)

    def adjoint(self, y):
        z = spread(np.asarray(y, dtype=np.float64).reshape(self.oshape), self.d, self.imshape)
        cube = self._blur(np.einsum("fl,fab->lab", self.wf, z), np.conj(self.sotf))
        return np.einsum("tl,lab->tab", self.tpl, cube)

    def forward_g(self, x):
        xh = np.fft.rfft2(np.asarray(x, dtype=np.float64).reshape(self.ishape), norm="ortho")
        z = np.fft.irfft2(np.einsum("ftab,tab->fab", self.G, xh), s=self.imshape, norm="ortho")
        return sample(z, self.d)

    def adjoint_g(self, y):
        zh = np.fft.rfft2(spread(np.asarray(y, dtype=np.float64).reshape(self.oshape), self.d, self.imshape), norm="ortho")
        return np.fft.irfft2(np.einsum("ftab,fab->tab", np.conj(self.G), zh), s=self.imshape, norm="ortho")

    def fwadj(self, x, w=None):
        y = self.forward(x)
        if w is not None:
            w = np.asarray(w, dtype=np.float64).reshape(self.oshape)
            y = np.where(w > 0, w * y, 0.0)
        return self.adjoint(y)


class Joint:
    """[W^1/2 A ; (mu_im / mu)^1/2 Wim^1/2 A_im] as one operator on the maps (``w`` / ``w_im`` None: 1)."""

    def __init__(self, op, im, mu, mu_im, w=None, w_im=None):
        self.op, self.im = op, im
        self.ishape = tuple(op.ishape)
        self.n_s, self.n_i = int(np.prod(op.oshape)), im.osize
        self.oshape = (self.n_s + self.n_i,)
        self.sw = None if w is None else np.sqrt(np.asarray(w, dtype=np.float64).ravel())
        wi = np.ones(self.n_i) if w_im is None else np.asarray(w_im, dtype=np.float64).ravel()
        self.swi = np.sqrt(mu_im / mu * wi)

    @property
    def isize(self):
        return int(np.prod(self.ishape))

    @property
    def osize(self):
        return self.oshape[0]

    def forward(self, x):
        a = np.asarray(self.op.forward(x)).ravel()
        if self.sw is not None:
            a = self.sw * a
        return np.concatenate([a, self.swi * self.im.forward(x).ravel()])

    def adjoint(self, y):
        y = np.asarray(y, dtype=np.float64).ravel()
        ys = y[:self.n_s] if self.sw is None else self.sw * y[:self.n_s]
        return self.op.adjoint(ys.reshape(self.op.oshape)) + self.im.adjoint(self.swi * y[self.n_s:])

    def matvec(self, x):
        return self.forward(x.reshape(self.ishape)).ravel()

    def rmatvec(self, y):
        return self.adjoint(y).ravel()

    def data(self, y, y_im):
        """y~: a sample of weight 0 contributes 0 whatever it holds (a select: 0 * NaN is NaN)."""
        y = np.asarray(y, dtype=np.float64).ravel()
        if self.sw is not None:
            y = np.where(self.sw > 0, self.sw * np.where(self.sw > 0, y, 0.0), 0.0)
        yi = np.asarray(y_im, dtype=np.float64).ravel()
        return np.concatenate([y, np.where(self.swi > 0, self.swi * np.where(self.swi > 0, yi, 0.0), 0.0)])


def gaussian_psfs(sigmas, support):
    """Normalised Gaussian point-spread functions [L, support, support] of the given widths (pixels)."""
    yy, xx = np.mgrid[0:support, 0:support]
    c = support // 2
    sig = np.asarray(sigmas, dtype=np.float64)
    psf = np.exp(-((yy - c) ** 2 + (xx - c) ** 2)[None] / (2.0 * sig[:, None, None] ** 2))
    return psf / psf.sum(axis=(1, 2), keepdims=True)


def gaussian_sotf(sigmas, imshape, support=21):
    """Their OTFs [L, Na, Nb//2+1], through ``orc.ir2fr``."""
    from oracle import surfh_oracle as orc
    return orc.ir2fr(gaussian_psfs(sigmas, support), tuple(imshape))


def case(Na=40, Nb=45, Lc=24, T=3, F=2, d=4, seed=5):
    """The stand-alone problem of the tests: seeded templates > 0, Gaussian OTFs, two overlapping smooth filters, maps, a detector
    vector and a weight vector with zeros."""
    rng = np.random.default_rng(seed)
    tpl = rng.random((T, Lc)) + 0.1
    psf = gaussian_psfs(np.linspace(1.0, 2.5, Lc), 21)
    sotf = gaussian_sotf(np.linspace(1.0, 2.5, Lc), (Na, Nb), support=21)
    l = np.arange(Lc)
    filters = np.array([np.exp(-0.5 * ((l - c) / (Lc / 6.0)) ** 2) for c in np.linspace(Lc / 4.0, 3 * Lc / 4.0, F)])
    filters /= filters.sum(axis=1, keepdims=True)
    im = ImagerOracle(sotf, tpl, filters, d, (Na, Nb))
    x = rng.standard_normal(im.ishape)
    u = rng.standard_normal(im.oshape)
    w = np.exp(rng.uniform(np.log(0.5), np.log(2.0), im.oshape))
    w[rng.random(im.oshape) < 0.15] = 0.0
    return dict(im=im, tpl=tpl, psf=psf, sotf=sotf, filters=filters, x=x, u=u, w=w, d=d, imshape=(Na, Nb), Lc=Lc)
