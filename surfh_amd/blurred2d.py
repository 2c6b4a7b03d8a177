"""What the two 2-D deconvolution operators ``MRSBlurred`` share (the reference's surfh/Models/spectro_blind_rectangle.py and
surfh/Models/spectro_blind.py: their slit geometry, ``get_slit_slices`` and ``get_slit_weights`` are identical), and their
evaluation by the HIP library: one beta-sum channel (no spectral blur) whose gridding is given as bilinear taps.

    y[p, s, a] = sum_beta  w_s[beta] * boxsum_alpha(G_p C x)[alpha0 + a*srf, beta]

The variants differ only in G_p, the gridding of pointing p: an integer crop (``spectro_blind_rectangle.MRSBlurred``) or
bilinear interpolation at the rotated local grid (``spectro_blind.MRSBlurred``), and in their host-side quick-look
``data_to_img``.  Both are written as (i0, i1, y0, y1) tables for ``surfh_channel_desc``; the library builds the gather, its
exact transpose and, when the ``gt_*`` tables are given, the reference's interpolating back-projection from them.

``sotf`` may be ``[N_alpha, N_beta/2+1]`` (the reference's single image) or ``[L, N_alpha, N_beta/2+1]``: the L wavelength
planes are independent problems evaluated as one batch; ``forward`` then maps ``[L, N_alpha, N_beta] -> [L, P*S*alpha_out]``.
"""
from __future__ import annotations

import ctypes as C
from math import ceil, floor

import numpy as np

from . import _lib, instru
from ._lib import dev_ptr
from .linop import LinOp
from .plan_owner import PlanOwner
from . import potentials as _pot
from .nonneg import NonnegResult, check_nonneg_args, result_from_planes_trace
from .weights import DataWeights, check_data_weights


PLANE_COUPLINGS = ("none", "isotropic")


def plane_coupling_code(coupling) -> int:
    """The code of a plane-wise prior coupling, "none" or "isotropic".  ``ValueError`` for "vector" -- it would tie the independent
    planes together (one trace, one stopping test: a different solver) -- and for anything that is no coupling at all."""
    code = _pot.coupling_code(coupling)
    if _pot.COUPLING_NAMES[code] not in PLANE_COUPLINGS:
        raise ValueError(f"coupling {_pot.COUPLING_NAMES[code]!r} would tie the independent planes together; the plane-wise solver "
                         f"takes one of {', '.join(PLANE_COUPLINGS)}")
    return code


def per_plane(value, n_planes: int, what: str) -> np.ndarray:
    """``value`` (a number, or an array ``[n_planes]``) as a contiguous float64 array ``[n_planes]``; ``ValueError`` on another
    shape."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.size != n_planes):
        raise ValueError(f"{what} has shape {a.shape}, expected a number or [{n_planes}]")
    return np.ascontiguousarray(np.broadcast_to(a, (n_planes,)))


def plane_prior_args(n_planes: int, mu_reg, delta, coupling="none"):
    """The argument rules of the plane-wise priors, checked before any library call.  Returns ``(mu_reg, delta, code, extended)``:
    ``extended`` False -- numbers and no coupling, the arguments of the scalar entry points, returned as they came (the library
    checks them) -- or True: ``mu_reg`` and ``delta`` float64 arrays ``[n_planes]`` for the ``_ex`` entry points, every delta positive
    and every mu_reg >= 0."""
    code = plane_coupling_code(coupling)
    _pot.need_delta_coupling(code, delta)
    if delta is None:
        if np.ndim(mu_reg) > 0:
            raise ValueError("a per-plane mu_reg needs delta: the quadratic solvers take one mu_reg for all planes")
        return mu_reg, None, code, False
    if code == 0 and np.ndim(mu_reg) == 0 and np.ndim(delta) == 0:
        return mu_reg, delta, code, False
    r, d = per_plane(mu_reg, n_planes, "mu_reg"), per_plane(delta, n_planes, "delta")
    if not np.all(d > 0.0):
        raise ValueError(f"delta must be positive, not {delta!r}")
    if not np.all(r >= 0.0):
        raise ValueError(f"mu_reg must be >= 0, not {mu_reg!r}")
    return r, d, code, True


class Blurred2D(DataWeights, _pot.Potentials, PlanOwner, LinOp):
    def __init__(self, sotf, alpha_axis, beta_axis, instr: instru.IFU, step_degree: float, pointings: instru.CoordList):
        self.sotf = sotf
        self.alpha_axis = np.asarray(alpha_axis, dtype=np.float64)
        self.beta_axis = np.asarray(beta_axis, dtype=np.float64)
        self.step_degree = step_degree
        self.instr = instr                    # not pixelised, as in the reference (:38-39)
        self.pointings = pointings
        self.srf = instru.get_srf([instr.det_pix_size], step_degree * 3600)[0]
        self.local_alpha_axis, self.local_beta_axis = instr.fov.local_coords(step_degree, 5 * step_degree, 5 * step_degree)
        self.local_im_shape = (len(self.local_alpha_axis), len(self.local_beta_axis))
        self.imshape = (len(self.alpha_axis), len(self.beta_axis))
        self.slices_shape = (len(pointings), instr.n_slit, ceil(self.npix_slit_alpha_width / self.srf))
        sotf_c = np.ascontiguousarray(sotf, dtype=np.complex128)
        self.batched = sotf_c.ndim == 3
        if not self.batched:
            sotf_c = sotf_c[None]
        self.n_planes = sotf_c.shape[0]
        if sotf_c.shape[1:] != (self.imshape[0], self.imshape[1] // 2 + 1):
            raise ValueError(f"sotf plane shape {sotf_c.shape[1:]} does not match the image {self.imshape}")
        self._sotf_c = sotf_c
        n_out = int(np.prod(self.slices_shape))
        super().__init__(ishape=((self.n_planes,) if self.batched else ()) + self.imshape,
                         oshape=((self.n_planes, n_out) if self.batched else (n_out,)))

    def _slit_tables(self):
        """Slit windows (one alpha window, ``npix_slit_beta_width`` columns each) and their beta weights [S, nbs]."""
        S = self.instr.n_slit
        slices = [self.get_slit_slices(s) for s in range(S)]
        nbs = self.npix_slit_beta_width
        a0, a1 = slices[0][0].start, slices[0][0].stop
        weights = np.empty((S, nbs))
        for s, sl in enumerate(slices):
            if (sl[0].start, sl[0].stop) != (a0, a1) or sl[1].stop - sl[1].start != nbs:
                raise ValueError(f"slit {s}: window {sl} differs from slit 0 / npix_slit_beta_width={nbs}")
            weights[s] = self.get_slit_weights(s, sl)[0][0]
        return slices, weights

    def _set_tables(self, slices, weights, i0, i1, y0, y1, gt=None):
        """Host tables of the channel: gridding taps ``(i0, i1, y0, y1)`` [P, na*nb]; ``gt`` = (gt_i0, gt_i1, gt_y0, gt_y1,
        gt_inside) [P, Na*Nb] adds the reference's back-projection (``surfh_adjoint_ref``)."""
        self._tab = dict(slices=slices, alpha0=slices[0][0].start, n_alpha_slit=slices[0][0].stop - slices[0][0].start,
                         slit_beta0=np.ascontiguousarray([sl[1].start for sl in slices], dtype=np.int32),
                         slit_weights=np.ascontiguousarray(weights), i0=i0, i1=i1, y0=y0, y1=y1)
        if gt is not None:
            self._tab.update({k: np.ascontiguousarray(a, dtype=t) for k, a, t in
                              zip(("gt_i0", "gt_i1", "gt_y0", "gt_y1", "gt_inside"), gt,
                                  (np.int32, np.int32, np.float64, np.float64, np.uint8))})

    def _create_plan(self, device=0, stream=None, exact=0):
        """One beta-sum channel on the tables of ``_set_tables``; ``exact``: ``surfh_config.exact``."""
        t = self._tab
        na, nb = self.local_im_shape
        d = _lib.ChannelDesc()
        d.wslice_start, d.wslice_stop = 0, self.n_planes
        d.n_pointings, d.n_slit, d.n_lambda_out = len(self.pointings), self.instr.n_slit, self.n_planes
        d.n_alpha_out, d.srf = self.slices_shape[2], self.srf
        d.na, d.nb, d.alpha0, d.n_alpha_slit, d.n_beta_slit = na, nb, t["alpha0"], t["n_alpha_slit"], self.npix_slit_beta_width
        d.slit_beta0, d.slit_weights = _lib.iptr(t["slit_beta0"]), _lib.dptr(t["slit_weights"])
        d.grid_i0, d.grid_i1, d.grid_y0, d.grid_y1 = _lib.iptr(t["i0"]), _lib.iptr(t["i1"]), _lib.dptr(t["y0"]), _lib.dptr(t["y1"])
        d.wpsf = None                                # beta-sum mode (no spectral blur)
        if "gt_i0" in t:
            d.gt_i0, d.gt_i1, d.gt_y0, d.gt_y1 = _lib.iptr(t["gt_i0"]), _lib.iptr(t["gt_i1"]), _lib.dptr(t["gt_y0"]), _lib.dptr(t["gt_y1"])
            d.gt_inside = _lib.u8ptr(t["gt_inside"])
        cfg = _lib.Config()
        cfg.n_alpha, cfg.n_beta, cfg.n_lambda, cfg.n_templates = self.imshape[0], self.imshape[1], self.n_planes, 0
        cfg.templates = None
        cfg.sotf = self._sotf_c.view(np.float64).ctypes.data_as(_lib.c_double_p)
        cfg.n_channels, cfg.channels = 1, C.pointer(d)
        cfg.device, cfg.stream, cfg.split_k_forward = device, (C.c_void_p(stream) if stream else None), 0
        cfg.exact = int(exact)
        L = _lib.load()
        plan = C.c_void_p()
        _lib.check(L.surfh_plan_create(C.byref(cfg), C.byref(plan)), ValueError)
        self._L, self._plan = L, plan
        del self._sotf_c                             # the plan holds its own copy
        assert L.surfh_isize(plan) == self.isize and L.surfh_osize(plan) == self.osize

    # ---- geometry (same rules as the reference classes) ---------------------------------------------
    @property
    def npix_slit_alpha_width(self) -> int:
        step = self.local_alpha_axis[1] - self.local_alpha_axis[0]
        half = self.instr.fov.alpha_width / 2 / step
        return int(ceil(half)) - int(floor(-half))

    @property
    def slit_beta_width(self):
        return self.instr.fov.beta_width / self.instr.n_slit

    @property
    def npix_slit_beta_width(self) -> int:
        return int(ceil(self.slit_beta_width / (self.beta_axis[1] - self.beta_axis[0])))

    def slit_local_fov(self, slit_idx: int):
        return self.instr.slit_fov[slit_idx].local + self.instr.slit_shift[slit_idx]

    def get_slit_slices(self, slit_idx: int):
        """Beta trimming only: the alpha-length rule of Slicer is commented out here (:122-149)."""
        lf = self.slit_local_fov(slit_idx)
        sa, sb = lf.to_slices(self.local_alpha_axis, self.local_beta_axis)
        if sb.stop - sb.start > self.npix_slit_beta_width:
            far_end = abs(self.local_beta_axis[sb.stop] - lf.beta_end)
            far_start = abs(self.local_beta_axis[sb.start] - lf.beta_start)
            sb = slice(sb.start, sb.stop - 1) if far_end > far_start else slice(sb.start + 1, sb.stop)
        return sa, sb

    def get_slit_weights(self, slit_idx: int, slices):
        sa, sb = slices
        lf = self.slit_local_fov(slit_idx)
        db = self.local_beta_axis[1] - self.local_beta_axis[0]
        sel = self.local_beta_axis[sb]
        w = np.ones((sa.stop - sa.start, sb.stop - sb.start))
        if sel[0] - db / 2 < lf.beta_start:
            w[:, 0] = 1 - abs(sel[0] - db / 2 - lf.beta_start) / db
        if sel[-1] + db / 2 > lf.beta_end:
            w[:, -1] = 1 - abs(sel[-1] + db / 2 - lf.beta_end) / db
        assert np.all((0 <= w) & (w <= 1))
        if slit_idx > 0 and self.get_slit_slices(slit_idx - 1)[1].stop - 1 != sb.start:
            w[:, 0] = 1
        # the reference bounds this test by npix_slit_beta_width, not n_slit (:167): kept, including
        # its IndexError when there are fewer slits than beta columns
        if slit_idx < self.npix_slit_beta_width - 1:
            if sb.stop - 1 != self.get_slit_slices(slit_idx + 1)[1].start:
                w[:, -1] = 1
        return w[np.newaxis, ...]

    def _d2i_local(self, d, p, scale):
        """The local image of ``data_to_img`` for pointing p: every sample / ``scale`` spread over its slit's beta columns, put
        back on the local grid (slit windows with their beta-edge weights), summed over the srf-row window (the transposed
        box), values below 1 zeroed and local columns 5 / 153 overwritten by their neighbours 6 / 152 as the reference does
        (so the local grid needs >= 154 columns, as there)."""
        na, nb = self.local_im_shape
        nbs, n_out = self.npix_slit_beta_width, self.slices_shape[2]
        local = np.zeros((na, nb))
        for s in range(self.instr.n_slit):
            sl = self.get_slit_slices(s)
            w = self.get_slit_weights(s, sl)[0]
            bts = np.zeros((sl[0].stop - sl[0].start, sl[1].stop - sl[1].start))
            bts[: n_out * self.srf: self.srf, :] = np.repeat(d[p, s][:, None], nbs, axis=1) / scale
            local[sl[0], sl[1]] += bts * w
        st = sum(np.roll(local, j, axis=0) for j in range(self.srf))      # transpose of the circular srf-row window sum
        st[st < 1] = 0
        st[:, 5] = st[:, 6]
        st[:, 153] = st[:, 152]
        return st

    def _d2i_data(self, data):
        if self.batched:
            raise ValueError("data_to_img is defined for a single image")
        if self.local_im_shape[1] < 154:
            raise IndexError(f"data_to_img patches local columns 5 and 153: the local grid has {self.local_im_shape[1]} columns")
        return np.asarray(data, dtype=np.float64).reshape(self.slices_shape)

    # ---- operator -------------------------------------------------------------------------------------
    def forward(self, x):
        return self._host(self._L.surfh_forward, x, self.isize, self.oshape)

    def adjoint(self, data):
        return self._host(self._L.surfh_adjoint, data, self.osize, self.ishape)

    # ---- solver: regularised least squares by CG, one independent 2-D problem per plane -------------------
    def cg(self, data, mu=1.0, mu_reg=0.0, x0=None, max_iter=10, tol=1e-12, refresh=50, callback=None, weights=None):
        """Device-resident linear CG on  mu |y - A x|^2 + mu_reg (|Dr x|^2 + |Dc x|^2)  (criterion_2D.py:60-250 with
        `qmm.lcg` restated).  Batched model: every plane is its own problem with its own step sizes; returns
        ``(x, grad_norm, nit)`` with ``grad_norm`` of shape ``[nit+1]`` (single image) or ``[nit+1, n_planes]``.
        ``callback(it, grad_norm, x)`` as for ``spectroSigRLSCT.cg``.  ``weights``: data weights in the layout of ``data`` for this
        solve only, data term mu (y - A x)^T diag(w) (y - A x) (``set_data_weights``); None: the model's own state."""
        with self.installed_weights(weights):
            return _lib.solve(self, self._L.surfh_cg_planes_cb, data, mu, mu_reg, x0, max_iter, tol, refresh, callback,
                              planes=self.n_planes, squeeze=not self.batched)

    # ---- per-pixel uncertainty of what cg returns: perturbation-optimisation sampling, plane by plane (surfh_amd/posterior.py) ----
    def sample_posterior(self, data, mu=1.0, mu_reg=0.0, n_samples=16, seed=0, x0=None, max_iter=10, tol=1e-12, refresh=50,
                         weights=None, perturbations=None, callback=None):
        """Per-pixel uncertainty of the images ``cg`` returns.  The criterion of ``cg`` is, plane by plane, the negative log of a
        Gaussian posterior ``p(x_l | y_l) ~ exp(-x_l^T Q_l x_l / 2 + b_l^T x_l)``, ``Q_l = mu A_l^T W_l A_l + mu_reg (Dr^T Dr + Dc^T Dc)``,
        ``b_l = mu A_l^T W_l y_l`` -- a statistical statement once ``weights = 1 / sigma^2`` (``mu = 1``).  Runs ``cg`` (same
        arguments, same bits), then ``n_samples`` perturbed solves ``Q_l e_l = b~_l - b_l`` from zero (``b~ ~ N(b, Q)``,
        ``x~ = x_map + e``) with the same ``max_iter``, ``tol`` and ``refresh``, and returns a ``posterior.PlanesPosteriorResult``:
        ``x_map``, ``mean``, ``var``, ``std``, ``nit``, ``grad_norm``, ``rr_first``, ``rr_last``, ``n_samples`` (include/surfh_amd.h:
        surfh_cg_planes_sample).  The noise is generated on the device, in the registers of the kernels that use it: beside the
        solver's vectors a run holds two float32 and two float64 vectors of the planes' size.

        A sample is exact only if its solve converges: where ``rr_last`` is not small against ``rr_first`` the plane's ``std`` is a
        lower bound.  A plane whose ``rr_first`` is exactly 0 -- no data weight and ``mu_reg = 0`` -- has no proper posterior and
        reports ``var = std = +inf``, not 0.

        ``seed``: the counter-based generator's 64-bit key; the same seed gives the same bits, whatever ran before.  ``weights``:
        as in ``cg``.  ``perturbations=(eps_y [K, osize], eps_r [K, isize], eps_c [K, isize])``: the standard normal vectors of
        every draw instead of the generator's (what makes a float64 comparison possible; ``eps_r`` / ``eps_c`` may be None with
        ``mu_reg = 0``).  ``callback(k, rr, x)``: every finished sample -- its index, the r.r trace of its solve (``[nit_k+1,
        n_planes]``) and ``x~``; a truthy return stops the run with an error.  ``ValueError``: ``mu`` not finite and > 0,
        ``mu_reg`` not one finite number >= 0, ``n_samples < 2``, ``max_iter < 0``, arrays of the wrong size."""
        from . import posterior
        return posterior.sample_posterior_planes(self, data, mu, mu_reg, n_samples, seed, x0, max_iter, tol, refresh, weights,
                                                 perturbations, callback)

    def po_planes_dev(self, which, out_t, shape=None, n_out=0, seed=0, sample=0, mu=1.0, mu_reg=0.0, w_t=None):
        """Diagnostic: one fused perturbation kernel of ``sample_posterior`` into the device tensor ``out_t`` (or a raw address), on
        explicit extents whatever the model's own: ``which="eta"`` with ``shape=(L, na, nb)``, ``which="data"`` with ``n_out``
        floats and the weights ``w_t`` (None: 1).  Synchronises.  (include/surfh_amd.h: surfh_debug_po_planes)"""
        L, na, nb = (int(v) for v in (shape if shape is not None else (1, 1, 1)))
        _lib.check(self._L.surfh_debug_po_planes(self._plan, which.encode(), L, na, nb, int(n_out), _lib.seed64(seed), int(sample),
                                                 float(mu), float(mu_reg), dev_ptr(w_t), dev_ptr(out_t)), ValueError)

    # ---- the same criterion under x >= 0: ADMM around the CG above, plane by plane (surfh_amd/nonneg.py) ----------
    def nonneg_rho(self, mu=1.0, mu_reg=0.0, seed=0, weights=None):
        """The default penalties of ``cg_nonneg``: per plane ``v_l^T Q_l v_l / v_l^T v_l`` for one standard normal probe ``v``
        (``default_rng(seed)``, drawn in the model's input shape), ``Q_l = mu A_l^T W_l A_l + mu_reg (Dr^T Dr + Dc^T Dc)`` -- the mean
        eigenvalue of every plane's operator from one batched forward application.  ``weights`` as in ``cg`` (None: the model's
        own).  Returns ``[n_planes]``, a float for a single image."""
        v = np.random.default_rng(seed).standard_normal(self.ishape)
        av = np.asarray(self.forward(v), dtype=np.float64).reshape(self.n_planes, -1)
        w = self.data_weights if weights is None else check_data_weights(weights, self.osize)
        sq = av * av if w is None else np.where(w.reshape(av.shape) > 0, w.reshape(av.shape).astype(np.float64) * av * av, 0.0)
        vp = v.reshape((self.n_planes,) + self.imshape)
        prior = np.sum((vp - np.roll(vp, 1, axis=1)) ** 2 + (vp - np.roll(vp, 1, axis=2)) ** 2, axis=(1, 2)) if mu_reg else 0.0
        rho = (mu * np.sum(sq, axis=1) + mu_reg * prior) / np.sum(vp * vp, axis=(1, 2))
        return rho if self.batched else float(rho[0])

    def cg_nonneg(self, data, mu=1.0, mu_reg=0.0, rho=None, x0=None, outer=30, inner=10, tol=0.0, refresh=10, weights=None) -> NonnegResult:
        """The images of ``cg`` under ``x >= 0``: every plane its own problem ``min x_l^T Q_l x_l / 2 - b_l^T x_l, x_l >= 0`` with its
        own penalty, step sizes, trace and stopping test (include/surfh_amd.h: surfh_cg_planes_nonneg).  ``outer`` ADMM iterations
        of ``inner`` CG iterations each, from ``x0`` (None: zeros); the carried residual is recomputed every ``refresh`` outer
        iterations (0: never).  ``rho``: None (``nonneg_rho(mu, mu_reg, weights=weights)``), a number (every plane) or ``[n_planes]``.
        Returns a ``NonnegResult`` whose traces are ``[nit+1, n_planes]`` (``[nit+1]`` for a single image, as ``cg``'s
        ``grad_norm``) and whose ``rho`` is the array used (a float for a single image).  Stops early once every plane has
        ``max(rho_l primal_l, dual_l) < Na Nb tol``; the planes that met the test earlier keep iterating until then.
        ``ValueError`` for a bad argument."""
        if rho is not None:
            rho = np.asarray(rho, dtype=np.float64)
            if rho.ndim > 1 or (rho.ndim == 1 and rho.size != self.n_planes):
                raise ValueError(f"cg_nonneg: rho has shape {rho.shape}, expected a number or [{self.n_planes}]")
        for r in ([None] if rho is None else np.atleast_1d(rho)):
            check_nonneg_args(r, outer, inner, refresh)
        y = _lib.f32_vec(data, self.osize, f"data have {np.size(data)} elements, expected {self.osize}")
        x0a = _lib.f32_vec(x0, self.isize, f"x0 has {np.size(x0)} elements, expected {self.isize}", optional=True)
        if rho is None:
            rho = self.nonneg_rho(mu, mu_reg, weights=weights)
        rho = np.ascontiguousarray(np.broadcast_to(np.asarray(rho, dtype=np.float64), (self.n_planes,)))
        with self.installed_weights(weights):
            x, trace, nit = _lib._solve_nonneg(self, self._L.surfh_cg_planes_nonneg, y, (mu, mu_reg, _lib.dptr(rho)), x0a, outer, inner,
                                               tol, refresh, planes=self.n_planes)
        return result_from_planes_trace(x, trace, rho, nit, squeeze=not self.batched)

    def nn_project_planes_dev(self, x_t, z_t, u_t, r_t, n_planes: int, npix: int, rho) -> np.ndarray:
        """The projection / dual update of one outer iteration on device tensors ``[n_planes, npix]`` (or raw device addresses),
        in place in ``z_t``, ``u_t`` and ``r_t`` (include/surfh_amd.h: surfh_nn_project_planes_dev); ``rho`` ``[n_planes]``.
        Returns ``[4, n_planes]``: ``|x - z'|^2, |z' - z|^2, #{z' == 0}, r.r`` per plane (synchronises)."""
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        if rho.shape != (int(n_planes),):
            raise ValueError(f"rho has shape {rho.shape}, expected ({int(n_planes)},)")
        sums = np.zeros((4, int(n_planes)), dtype=np.float64)
        _lib.check(self._L.surfh_nn_project_planes_dev(self._plan, dev_ptr(x_t), dev_ptr(z_t), dev_ptr(u_t), dev_ptr(r_t), int(n_planes),
                                                       int(npix), _lib.dptr(rho), _lib.dptr(sums)), ValueError)
        return sums

    # the same loop on device tensors (torch), no host synchronisation inside: see include/surfh_amd.h
    def cg_begin_dev(self, y_t, x_t, mu=1.0, mu_reg=0.0, weights=None):
        """``x_t`` [n_planes, Na, Nb] float32 on the plan's device: the start, then the current iterate (updated in place).
        ``weights`` (a host array): installed with ``set_data_weights`` before the loop begins and left in the plan, since the
        ``cg_step_dev`` calls that follow apply them; None: the model's own state."""
        if weights is not None:
            self.set_data_weights(weights)
        _lib.check(self._L.surfh_cg_planes_begin_dev(self._plan, dev_ptr(y_t), float(mu), float(mu_reg), dev_ptr(x_t)))

    def cg_step_dev(self, iters=1, refresh=50):
        _lib.check(self._L.surfh_cg_planes_step_dev(self._plan, int(iters), int(refresh)))

    def cg_rr(self):
        out = np.zeros(self.n_planes, dtype=np.float64)
        _lib.check(self._L.surfh_cg_planes_rr(self._plan, _lib.dptr(out)))
        return out

    last_prior_values = None            # per-plane prior values of the last mmmg(delta=...) result (None after a quadratic run)

    def mmmg(self, data, mu=1.0, mu_reg=0.0, x0=None, max_iter=10, tol=1e-12, refresh=50, callback=None, delta=None, weights=None,
             potential="huber", coupling="none"):
        """Device-resident 3MG on the same criterion (`qmm.mmmg` restated for quadratic objectives) -- what the 2-D
        deconvolution driver's ``method = "qmm"`` runs (scripts/deconvolution_mrs_noRotation.py:199-212).  Same returns as
        ``cg`` except that ``grad_norm`` holds |grad| (not squared).  ``weights`` as in ``cg``.
        ``delta`` (a number): the priors are Huber potentials of threshold ``delta`` on the separated circular differences
        (criterion_2D.py imports qmm's ``Huber`` for this), every plane minimising its own
        mu |y - A x|^2 / 2 + mu_reg sum_k sum phi(D_k x)  (include/surfh_amd.h: surfh_mmmg_huber_planes); same returns, and the
        prior values sum_k sum phi(D_k x_l) of the returned iterate are left in ``self.last_prior_values`` ([n_planes]).
        ``potential``: the potential under ``delta`` for this call, "huber" (the default), "hyperbolic" or "hebert_leahy"
        (``surfh_amd.potentials``); ``ValueError`` for another one than Huber without ``delta``.
        With ``delta``, ``mu_reg`` and ``delta`` may each be an array ``[n_planes]``, every plane its own weight and threshold (a
        cube's flux changes by orders of magnitude along the wavelength); the planes stay independent, plane l of such a run is
        bit for bit plane l of the run on the numbers ``mu_reg[l]``, ``delta[l]`` that takes as many iterations.
        ``coupling`` (with ``delta``): "none" (the default: one potential per difference) or "isotropic" -- one potential per
        pixel on sqrt(u_r^2 + u_c^2), total variation under Huber's phi: an edge pays the same at every angle to the pixel grid.
        ``delta`` is then the threshold on that magnitude (sqrt(2) times larger for comparable behaviour) and
        ``last_prior_values`` holds sum phi(m), ``potentials.prior_value(x_l[None], delta, potential, "isotropic")``.  It is an
        argument of this call, not the plan's slot (``set_prior_coupling`` is the maps' and is refused here while it is set).
        ``ValueError``: a coupling without ``delta``, "vector" (it would tie the planes together), an array of another length, and
        on arrays or under a coupling a ``delta`` that is not positive or a negative ``mu_reg`` (numbers without a coupling are
        checked by the library, as before).  (include/surfh_amd.h: surfh_mmmg_huber_planes_ex)"""
        self.last_prior_values = None
        _pot.need_delta(potential, delta, "delta")
        mu_reg, delta, code, extended = plane_prior_args(self.n_planes, mu_reg, delta, coupling)
        with _pot.installed(self, spatial=potential), self.installed_weights(weights):
            if delta is None:
                return _lib.solve(self, self._L.surfh_mmmg_planes_cb, data, mu, mu_reg, x0, max_iter, tol, refresh, callback,
                                  planes=self.n_planes, squeeze=not self.batched)
            x, gn, nit, self.last_prior_values = _lib.solve_huber_planes(self, data, mu, mu_reg, delta, x0, max_iter, tol, refresh, callback,
                                                                         self.n_planes, not self.batched, code if extended else None)
            return x, gn, nit

    def huber_planes_prior_dev(self, x_t, g_t, mu_reg, delta, coupling="none"):
        """g_t += mu_reg sum_k D_k^T phi'(D_k x_t) on device tensors [n_planes, Na, Nb] (float32, contiguous); returns
        (|g_l|^2 of the result, sum_k sum phi(D_k x_l)), each [n_planes]: the gradient pass of ``mmmg(delta=...)`` alone.
        ``mu_reg``, ``delta`` (numbers or ``[n_planes]``) and ``coupling`` as in ``mmmg``; under "isotropic"
        g_t += mu_reg sum_k D_k^T (w(m) D_k x_t) and the values are sum phi(m)."""
        mu_reg, delta, code, extended = plane_prior_args(self.n_planes, mu_reg, delta, coupling)
        sq, val = np.zeros(self.n_planes), np.zeros(self.n_planes)
        fn, prior = _lib.planes_entry("surfh_huber_planes_prior_dev", code if extended else None, mu_reg, delta)
        _lib.check(fn(self._plan, dev_ptr(x_t), dev_ptr(g_t), *prior, _lib.dptr(sq), _lib.dptr(val)))
        return sq, val

    def huber_planes_curv_dev(self, x_t, p0_t, p1_t, delta, coupling="none") -> np.ndarray:
        """[n_planes, 3]: sum_k sum w(D_k x_l) (D_k p0_l)^2, (D_k p0_l)(D_k p1_l), (D_k p1_l)^2, the prior block of the majorant;
        ``delta`` (a number or ``[n_planes]``) and ``coupling`` as in ``mmmg`` (under "isotropic" w = w(m) for both differences)."""
        _, delta, code, extended = plane_prior_args(self.n_planes, 0.0, delta, coupling)
        out = np.zeros((3, self.n_planes))
        fn, prior = _lib.planes_entry("surfh_huber_planes_curv_dev", code if extended else None, delta)
        _lib.check(fn(self._plan, dev_ptr(x_t), dev_ptr(p0_t), dev_ptr(p1_t), *prior, _lib.dptr(out)))
        return np.ascontiguousarray(out.T)

    def planes_passes_dev(self, x_t, g_t, p0_t, p1_t, mu_reg, delta, potential="huber", coupling="none"):
        """Diagnostic: the two passes in one call on device arrays of any shape ``[L, Na, Nb]`` (every extent >= 1, whatever the
        model's own shape), under an explicit potential and coupling, ``mu_reg`` and ``delta`` numbers or ``[L]``; the plan's
        state is not consulted.  g_t += mu_reg_l sum_k D_k^T (w D_k x_t).  Returns (g.g, prior values, curvature blocks), shapes
        ``[L]``, ``[L]``, ``[L, 3]`` (synchronises).  (include/surfh_amd.h: surfh_debug_planes_passes)"""
        L, na, nb = (int(v) for v in x_t.shape)
        code = plane_coupling_code(coupling)
        r, d = per_plane(mu_reg, L, "mu_reg"), per_plane(delta, L, "delta")
        out = np.zeros((5, L), dtype=np.float64)
        _lib.check(self._L.surfh_debug_planes_passes(self._plan, L, na, nb, _pot.kind_code(potential), code, dev_ptr(x_t),
                                                     dev_ptr(g_t), dev_ptr(p0_t), dev_ptr(p1_t),
                                                     _lib.dptr(r), _lib.dptr(d), _lib.dptr(out)))
        return out[0].copy(), out[1].copy(), np.ascontiguousarray(out[2:].T)

    def planes_cg_dev(self, which, ext, vectors, sc_in=None, sc_out=None, mu_reg=0.0, update_r=1):
        """Diagnostic: one vector kernel of the plane-wise CG / 3MG loops on device tensors of explicit extents ``ext`` (``(L, npix)``
        or ``(Na, Nb, NAP, LP, L, l0)``), through the solvers' launcher; the plan's state is not consulted.  ``vectors``: the
        kernel's device tensors in its order, ``sc_in`` the rows of float64 scalars it reads, ``sc_out`` the rows it writes
        (filled in place, entries it leaves alone unchanged; returned).  Synchronises.
        (include/surfh_amd.h: surfh_debug_planes_cg)"""
        e = np.zeros(6, dtype=np.int64)
        e[:len(ext)] = ext
        ptrs = [dev_ptr(t) for t in vectors] + [None] * (6 - len(vectors))
        sc_in = None if sc_in is None else np.ascontiguousarray(sc_in, dtype=np.float64)
        if sc_out is not None and not (isinstance(sc_out, np.ndarray) and sc_out.dtype == np.float64 and sc_out.flags.c_contiguous):
            raise ValueError("sc_out must be a contiguous float64 array (it is filled in place)")
        _lib.check(self._L.surfh_debug_planes_cg(self._plan, which.encode(), e.ctypes.data_as(C.POINTER(C.c_int64)), *ptrs, float(mu_reg),
                                                 int(update_r), None if sc_in is None else _lib.dptr(sc_in),
                                                 None if sc_out is None else _lib.dptr(sc_out)))
        return sc_out

    def planes_normal_dev(self, v_t, q_t, mu=1.0, mu_reg=0.0, raw_t=None) -> np.ndarray:
        """Diagnostic: one application of the normal operator of the device-resident loop (``cg_begin_dev`` / ``cg_step_dev`` on
        wavelength-innermost vectors) on device tensors ``[n_planes, Na, Nb]`` (float32, contiguous):
        q_t = mu A^T W A v_t + mu_reg (Dr^T Dr + Dc^T Dc) v_t on the plan's route, with the model's data weights.  Returns
        ``v_l . q_l`` per plane ``[n_planes]``, the sums the operator leaves for the step.  ``raw_t``: a device tensor of the padded
        vector's size (``surfh_debug_dims(plan, "blurred")``) that receives it as the loop holds it.  Synchronises; a loop begun with
        ``cg_begin_dev`` has to be begun again afterwards.  (include/surfh_amd.h: surfh_debug_planes_normal)"""
        dq = np.zeros(self.n_planes, dtype=np.float64)
        _lib.check(self._L.surfh_debug_planes_normal(self._plan, dev_ptr(v_t), dev_ptr(q_t), float(mu), float(mu_reg), _lib.dptr(dq),
                                                     None if raw_t is None else dev_ptr(raw_t)))
        return dq
