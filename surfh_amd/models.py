"""``spectroSigRLSCT``: the reference's multi-channel multi-observation MRS operator
(surfh/Models/spectroModel.py:39-185) with the same constructor and methods, evaluated by
the HIP library through the C ABI (include/surfh_amd.h).

    y = Sigma R L S C T x      (operator chain documented at spectroModel.py:25-38)

``forward`` / ``adjoint`` take and return NumPy arrays (float64 out, for drop-in use with
a CPU solver); ``*_dev`` variants take device pointers / torch tensors and are
asynchronous on the plan's stream.  ``adjoint`` is the exact transpose of ``forward``
(what CG and the dot-test need); ``adjoint_ref`` reproduces the reference's
interpolating ``gridding_t`` (spectroModelChannel.py:180-199).
"""
from __future__ import annotations

import ctypes as C
from math import ceil
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, instru
from ._lib import dev_ptr
from .geometry import ChannelGeometry
from .linop import LinOp
from .plan_owner import PlanOwner
from . import potentials as _pot
from .weights import DataWeights
from .spectra import TemplateOps
from .nonneg import NonnegOps


class Channel(ChannelGeometry):
    """One channel of the model, as ``model.channels[k]`` (surfh.Models.spectroModelChannel.Channel): the geometry
    plus the reference's slice <-> cube projections its drivers use to look at data and to initialise
    (scripts/fusion/*.py).  Each projection is the library's own gather / GEMM / scatter chain on the GPU, run on a
    small single-channel plane-wise plan built on first use with the variant tables of ``ChannelGeometry``."""
    device = 0

    def _aux(self, key, wavel_axis, pointings, **opts):
        cache = self.__dict__.setdefault("_aux_ops", {})
        if key not in cache:
            cache[key] = spectroSigRLSCT(None, None, self.alpha_axis, self.beta_axis, wavel_axis, [self.raw_instr],
                                         self.step_degree, [instru.CoordList(pointings)], device=self.device,
                                         gridding=self.gridding_mode, channel_opts=opts)
        return cache[key]

    def close(self):
        for op in self.__dict__.pop("_aux_ops", {}).values():
            op.close()

    def sliceToCube(self, data):
        """spectroModelChannel.py:266-301: the data of pointing 0 back in the cube -- every detector sample goes to the
        wavelength plane where its spectral response peaks (``wpsf_dirac``), then the reference's adjoint chain
        (slit weights, transposed box sum, interpolating ``gridding_t``).  Returns [len(wavelength_axis), Na, Nb]."""
        if self.lam_slice is not None:
            raise ValueError("sliceToCube is defined on a whole channel, not on a lambda part")
        op = self._aux("s2c", self.global_wavelength_axis, [self.raw_pointings[0]], psf_type="dirac")
        y0 = np.asarray(data, dtype=np.float64).reshape(self.oshape)[0]
        return op.adjoint_ref(y0)

    def realData_cubeToSlice(self, cube):
        """spectroModelChannel.py:303-309: a cube on the detector's wavelength axis -> [n_slit, L, n_alpha_out]:
        gridding at pointing (0, 0), slit windows with their edge weights, plain alpha decimation, sum over beta."""
        cube = np.asarray(cube)
        if cube.shape != (self.oshape[2],) + self.imshape:
            raise ValueError(f"cube shape {cube.shape} != {(self.oshape[2],) + self.imshape}")
        op = self._aux("c2s", np.asarray(self.raw_instr.wavel_axis, dtype=np.float64), [instru.Coord(0, 0)],
                       beta_sum=True, full_window=True, box=(1, 0))
        L, (S, A) = self.oshape[2], (self.oshape[1], self.oshape[3])
        return op.forward(cube).reshape(L, S, A).transpose(1, 0, 2).copy()          # the plan's beta-sum output is [l][s][a]

    def realData_sliceToCube(self, slices, cube_dim):
        """spectroModelChannel.py:311-336: slit values spread evenly over the slit's beta columns, zero-stuffed along
        alpha, correlated with the box kernel (``_otf_sr.conj()``, no ``decalf``) and back-interpolated at pointing (0, 0)."""
        cube_dim = tuple(int(v) for v in cube_dim)
        if cube_dim != (self.oshape[2],) + self.imshape:
            raise ValueError(f"cube_dim {cube_dim} != {(self.oshape[2],) + self.imshape}")
        op = self._aux("s2c_rd", np.asarray(self.raw_instr.wavel_axis, dtype=np.float64), [instru.Coord(0, 0)],
                       beta_sum=True, full_window=True, box=(self.srf, -int((self.srf - 1) / 2)))
        s = np.asarray(slices, dtype=np.float64).reshape(self.oshape[1:]) / self.slicer.npix_slit_beta_width
        return op.adjoint_ref(np.ascontiguousarray(s.transpose(1, 0, 2)))


class _InstalledImager:
    def __init__(self, model, imager):
        self.model, self.args = model, None
        if imager is not None:
            from .imager import check_imager_data
            if model._imager is None:
                raise ValueError("imager=(y_im, mu_imager[, w_im]) needs an attached imager: set_imager(...) first")
            if not 2 <= len(imager) <= 3:
                raise ValueError("imager must be (y_im, mu_imager) or (y_im, mu_imager, w_im)")
            check_imager_data(imager[0], imager[1], imager[2] if len(imager) == 3 else None, model._imager.osize)
            self.args = (imager[0], imager[1], imager[2] if len(imager) == 3 else None)

    def __enter__(self):
        if self.args is not None:
            self.held = self.model._imager_data
            self.model.set_imager_data(*self.args)

    def __exit__(self, *exc):
        if self.args is not None:                    # back to what the model held, as installed_weights does: cleared if nothing
            if self.held is None:
                self.model.set_imager_data(None)
            else:
                y, mu, w = self.held
                self.model.set_imager_data(y, mu, w)
        return False


class spectroSigRLSCT(DataWeights, TemplateOps, NonnegOps, _pot.Potentials, PlanOwner, LinOp):
    huber_prior_value = None            # prior value of the last mmmg(delta=...) result (set by mmmg)
    huber_prior_values = None           # (spatial, spectral) prior values of the last mmmg_vox result
    robust_weights = None               # omega(t) [osize] of the last mmmg / mmmg_vox result under data_delta (else None)
    robust_data_value = None            # sum phi(t) of that result
    robust_n_beyond = None              # number of its samples with |t| > data_delta

    def __init__(self, sotf, templates, alpha_axis, beta_axis, wavelength_axis, instrs: List[instru.IFU],
                 step_degree: float, pointings: Sequence[instru.CoordList], *, device: int = 0,
                 channels: Optional[Sequence[int]] = None, with_ref: bool = True, stream: Optional[int] = None,
                 split_k_forward: int = 0, gridding: str = "bilinear", lam_slices=None, channel_opts: Optional[dict] = None,
                 verify: bool = False, exact: int = 0):
        """``exact``: ``surfh_config.exact`` -- 1: all three fp16 products on every K step of the spectral-blur GEMMs, 2: whole
        spectrum in the transform passes, 3: both (the production kernels without their two bounded approximations).
        ``sotf=None`` (plane-wise plans only, ``templates=None``) means no spatial blur; ``channel_opts`` are the
        ``ChannelGeometry`` variants of the slice <-> cube projections (see ``Channel`` below).  ``verify=True`` builds the
        verification plan (include/surfh_amd.h ``surfh_config.verify``): the same operator with every long sum accumulated in
        float64 -- slow; what the strict dot test with zero-mean test vectors runs on."""
        self.sotf = sotf
        self.alpha_axis = np.asarray(alpha_axis, dtype=np.float64)
        self.beta_axis = np.asarray(beta_axis, dtype=np.float64)
        self.wavelength_axis = np.asarray(wavelength_axis, dtype=np.float64)
        self.step_degree = step_degree
        self.templates = None if templates is None else np.ascontiguousarray(templates, dtype=np.float64)
        self.lmm = self.templates is not None
        self.pointings = pointings
        self.instrs = [i.pix(step_degree) for i in instrs]
        self.srfs = instru.get_srf([i.det_pix_size for i in instrs], step_degree * 3600)
        # every channel's geometry is known to every rank; `channels` selects the ones this plan owns
        self.all_channels = [Channel(ins, self.alpha_axis, self.beta_axis, self.wavelength_axis, srf,
                                     pointings[k], step_degree, gridding=gridding,
                                     lam_slice=None if lam_slices is None else lam_slices[k], **(channel_opts or {}))
                             for k, (srf, ins) in enumerate(zip(self.srfs, instrs))]
        for c in self.all_channels:
            c.device = device
        self.owned = list(range(len(instrs))) if channels is None else [int(c) for c in channels]
        self.channels = [self.all_channels[k] for k in self.owned]
        self.list_wslice = [c.wslice for c in self.channels]
        self.instrs_oshape = [c.oshape for c in self.channels]
        self._idx = np.cumsum([0] + [int(np.prod(s)) for s in self.instrs_oshape])
        self.full_idx = np.cumsum([0] + [int(np.prod(c.oshape)) for c in self.all_channels])
        self.imshape = (len(self.alpha_axis), len(self.beta_axis))
        self.cube_shape = (len(self.wavelength_axis),) + self.imshape
        lead = self.templates.shape[0] if self.lmm else len(self.wavelength_axis)
        super().__init__(ishape=(lead,) + self.imshape, oshape=(int(self._idx[-1]),))

        nkb = self.imshape[1] // 2 + 1
        if sotf is None and self.lmm:
            raise ValueError("sotf=None (no spatial blur) is only defined without templates")
        sotf_c = None if sotf is None else np.ascontiguousarray(sotf, dtype=np.complex128)
        if sotf_c is not None and sotf_c.shape != (self.cube_shape[0], self.imshape[0], nkb):
            raise ValueError(f"sotf shape {sotf_c.shape} != {(self.cube_shape[0], self.imshape[0], nkb)}")
        if self.lmm and self.templates.shape[1] != self.cube_shape[0]:
            raise ValueError("templates must be [T, len(wavelength_axis)]")

        L = _lib.load()
        self._keep = []          # keeps the table arrays alive during plan creation
        descs = (_lib.ChannelDesc * len(self.channels))()
        for d, ch in zip(descs, self.channels):
            t = ch.tables(with_ref=with_ref)   # raises ValueError like the reference if the FoV leaves the cube
            self._keep.append(t)
            for k in ("wslice_start", "wslice_stop", "n_pointings", "n_slit", "n_lambda_out", "n_alpha_out", "srf",
                      "na", "nb", "alpha0", "n_alpha_slit", "n_beta_slit"):
                setattr(d, k, t[k])
            d.slit_beta0 = _lib.iptr(t["slit_beta0"])
            d.slit_weights = _lib.dptr(t["slit_weights"])
            d.grid_i0, d.grid_i1 = _lib.iptr(t["grid_i0"]), _lib.iptr(t["grid_i1"])
            d.grid_y0, d.grid_y1 = _lib.dptr(t["grid_y0"]), _lib.dptr(t["grid_y1"])
            d.wpsf = None if t["wpsf"] is None else _lib.dptr(t["wpsf"])
            d.box_len, d.box_shift = t["box_len"], t["box_shift"]
            if with_ref:
                d.gt_i0, d.gt_i1 = _lib.iptr(t["gt_i0"]), _lib.iptr(t["gt_i1"])
                d.gt_y0, d.gt_y1 = _lib.dptr(t["gt_y0"]), _lib.dptr(t["gt_y1"])
                d.gt_inside = _lib.u8ptr(t["gt_inside"])
        cfg = _lib.Config()
        cfg.n_alpha, cfg.n_beta, cfg.n_lambda = self.imshape[0], self.imshape[1], self.cube_shape[0]
        cfg.n_templates = self.templates.shape[0] if self.lmm else 0
        cfg.templates = _lib.dptr(self.templates) if self.lmm else None
        cfg.sotf = None if sotf_c is None else sotf_c.view(np.float64).ctypes.data_as(_lib.c_double_p)
        cfg.n_channels = len(self.channels)
        cfg.channels = descs
        cfg.device = device
        cfg.stream = C.c_void_p(stream) if stream else None
        cfg.split_k_forward = split_k_forward
        cfg.verify = 1 if verify else 0
        cfg.exact = int(exact)
        plan = C.c_void_p()
        _lib.check(L.surfh_plan_create(C.byref(cfg), C.byref(plan)), ValueError)
        self._L, self._plan = L, plan
        self._keep = []
        assert L.surfh_isize(plan) == self.isize and L.surfh_osize(plan) == self.osize
        self.device = device

    # ---- life cycle -----------------------------------------------------------------------
    def close(self):
        for c in getattr(self, "all_channels", []):         # the channels' auxiliary plans first
            c.close()
        super().close()

    @property
    def alpha_step(self) -> float:
        return self.alpha_axis[1] - self.alpha_axis[0]

    @property
    def beta_step(self) -> float:
        return self.beta_axis[1] - self.beta_axis[0]

    # ---- host-array API (reference calling convention) --------------------------------------
    def forward(self, maps):
        return self._host(self._L.surfh_forward, maps, self.isize, self.oshape)

    def adjoint(self, inarray):
        return self._host(self._L.surfh_adjoint, inarray, self.osize, self.ishape)

    def adjoint_ref(self, inarray):
        return self._host(self._L.surfh_adjoint_ref, inarray, self.osize, self.ishape)

    def fwadj(self, x):
        return self._host(self._L.surfh_fwadj, x, self.isize, self.ishape)

    # ---- device-pointer API (asynchronous on self.stream; forward_dev ... fwadj_dev: PlanOwner) ------
    def normal_dev(self, d_t, q_t, mu: float = 1.0):
        _lib.check(self._L.surfh_normal_dev(self._plan, dev_ptr(d_t), dev_ptr(q_t), float(mu)))

    # ---- the same with the solver's vectors in the Fourier domain of the maps (include/surfh_amd.h: surfh_normal_spec_dev) ----
    def spec_supported(self) -> bool:
        return bool(self._L.surfh_spec_supported(self._plan))

    @property
    def spec_size(self) -> int:
        return int(self._L.surfh_spec_size(self._plan))

    def to_spec_dev(self, x_t, xt_t):
        _lib.check(self._L.surfh_to_spec_dev(self._plan, dev_ptr(x_t), dev_ptr(xt_t)))

    def from_spec_dev(self, xt_t, x_t):
        _lib.check(self._L.surfh_from_spec_dev(self._plan, dev_ptr(xt_t), dev_ptr(x_t)))

    def forward_spec_dev(self, dt_t, y_t):
        _lib.check(self._L.surfh_forward_spec_dev(self._plan, dev_ptr(dt_t), dev_ptr(y_t)))

    def adjoint_spec_dev(self, y_t, qt_t, mu: float = 1.0, dt_t=None, mu_reg: float = 0.0):
        _lib.check(self._L.surfh_adjoint_spec_dev(self._plan, dev_ptr(y_t), dev_ptr(qt_t), float(mu), dev_ptr(dt_t),
                                                  float(mu_reg)))

    def normal_spec_dev(self, dt_t, qt_t, mu: float = 1.0, mu_reg: float = 0.0):
        _lib.check(self._L.surfh_normal_spec_dev(self._plan, dev_ptr(dt_t), dev_ptr(qt_t), float(mu), float(mu_reg)))

    def prior_spec_add_dev(self, dt_t, qt_t, mu_reg: float):
        _lib.check(self._L.surfh_prior_spec_add_dev(self._plan, dev_ptr(dt_t), dev_ptr(qt_t), float(mu_reg)))

    def prior_add_dev(self, d_t, q_t, mu_reg: float):
        _lib.check(self._L.surfh_prior_add_dev(self._plan, dev_ptr(d_t), dev_ptr(q_t), float(mu_reg)))

    def dot_dev(self, a_t, b_t, n: int) -> float:
        out = C.c_double()
        _lib.check(self._L.surfh_dot_dev(self._plan, dev_ptr(a_t), dev_ptr(b_t), int(n), C.byref(out)))
        return out.value

    def cg_step_dev(self, x_t, r_t, d_t, q_t, n: int, rr: float) -> float:
        out = C.c_double()
        _lib.check(self._L.surfh_cg_step_dev(self._plan, dev_ptr(x_t), dev_ptr(r_t), dev_ptr(d_t), dev_ptr(q_t), int(n), float(rr),
                                             C.byref(out)))
        return out.value

    def cg_iter_dev(self, x_t, r_t, d_t, q_t, n: int, rr: float) -> float:
        """cg_step_dev + cg_dir_dev with one host synchronisation; returns the new r.r."""
        out = C.c_double()
        _lib.check(self._L.surfh_cg_iter_dev(self._plan, dev_ptr(x_t), dev_ptr(r_t), dev_ptr(d_t), dev_ptr(q_t), int(n), float(rr), C.byref(out)))
        return out.value

    def cg_dir_dev(self, d_t, r_t, n: int, beta: float):
        _lib.check(self._L.surfh_cg_dir_dev(self._plan, dev_ptr(d_t), dev_ptr(r_t), int(n), float(beta)))

    # device-resident CG scalars: nothing below synchronises with the host (include/surfh_amd.h)
    def cg_begin_dev(self, r_t, n: int):
        _lib.check(self._L.surfh_cg_begin_dev(self._plan, dev_ptr(r_t), int(n)))

    def cg_iter_nosync_dev(self, x_t, r_t, d_t, q_t, n: int):
        _lib.check(self._L.surfh_cg_iter_nosync_dev(self._plan, dev_ptr(x_t), dev_ptr(r_t), dev_ptr(d_t), dev_ptr(q_t), int(n)))

    def cg_xupdate_nosync_dev(self, x_t, d_t, q_t, n: int):
        _lib.check(self._L.surfh_cg_xupdate_nosync_dev(self._plan, dev_ptr(x_t), dev_ptr(d_t), dev_ptr(q_t), int(n)))

    def cg_refresh_nosync_dev(self, r_t, b_t, q_t, d_t, n: int):
        _lib.check(self._L.surfh_cg_refresh_nosync_dev(self._plan, dev_ptr(r_t), dev_ptr(b_t), dev_ptr(q_t), dev_ptr(d_t), int(n)))

    def cg_trace(self, cap: int = 1 << 16) -> np.ndarray:
        """r.r of every iterate since ``cg_begin_dev`` (synchronises the plan's stream)."""
        out = np.zeros(cap, dtype=np.float64)
        n = self._L.surfh_cg_trace(self._plan, _lib.dptr(out), int(cap))
        if n < 0:
            raise RuntimeError("surfh_cg_trace failed")
        return out[:n].copy()

    def residual_dev(self, r_t, b_t, q_t, n: int):
        _lib.check(self._L.surfh_residual_dev(self._plan, dev_ptr(r_t), dev_ptr(b_t), dev_ptr(q_t), int(n)))

    def set_prior(self, gradient: str = "separated"):
        """The regulariser of ``cg`` / ``mmmg`` / ``prior_add_dev``: "separated" (NpDiff_r / NpDiff_c, the default) or "joint"
        (the Laplacian of Difference_Operator_Joint) -- ``QuadCriterion_MRS(gradient=...)``, fusion_CT.py:98-106."""
        if gradient not in ("separated", "joint"):
            raise ValueError(f"gradient must be 'separated' or 'joint', not {gradient!r}")
        _lib.check(self._L.surfh_set_prior(self._plan, 1 if gradient == "joint" else 0))
        self._prior = gradient

    def get_prior(self) -> str:
        """The regulariser ``set_prior`` selected last ("separated" on a new model)."""
        return getattr(self, "_prior", "separated")

    # ---- the imager data term (surfh_amd.imager; include/surfh_amd.h: surfh_set_imager) ----------------------------------------
    _imager = None
    _imager_data = None

    def set_imager(self, imager_model=None):
        """Attach ``imager_model`` (an ``ImagerModel`` built on this model) to the plan, or detach with ``None``.  Attaching or
        detaching clears the imager data."""
        if imager_model is None:
            _lib.check(self._L.surfh_set_imager(self._plan, None))
            self._imager = None
        else:
            if imager_model.model is not self:
                raise ValueError("the ImagerModel was built on another model")
            imager_model.attach()
        self._imager_data = None

    @property
    def imager(self):
        return self._imager

    def set_imager_data(self, y_im=None, mu_imager=0.0, weights=None):
        """The imager's data term ``mu_imager (y_im - A_im x)^T W_im (y_im - A_im x) / 2`` of ``cg``, ``mmmg`` and
        ``mmmg(delta=...)``: plan state until cleared with ``y_im=None``.  ``weights`` ``[F, Na//d, Nb//d]`` follow the rules of
        the data weights (weight 0 takes the sample out, NaN included).  ``mu_imager = 0`` switches the term off."""
        from .imager import check_imager_data
        if self._imager is None:
            raise ValueError("no imager is attached: set_imager(ImagerModel(model, filters, ...)) first")
        if y_im is None:
            _lib.check(self._L.surfh_set_imager_data(self._plan, None, None, 0.0))
            self._imager_data = None
            return
        y, w, mu = check_imager_data(y_im, mu_imager, weights, self._imager.osize)
        _lib.check(self._L.surfh_set_imager_data(self._plan, _lib.fptr(y), None if w is None else _lib.fptr(w), mu), ValueError)
        self._imager_data = (y, mu, w)

    @property
    def imager_data(self):
        """``(y_im, mu_imager, w_im)`` as set last (float32 vectors, w_im None without weights), or None."""
        return self._imager_data

    def has_imager_term(self) -> bool:
        return bool(self._L.surfh_has_imager_term(self._plan))

    def installed_imager(self, imager):
        """``with model.installed_imager((y_im, mu_imager[, w_im])):`` -- the data are set for the solves inside and cleared
        afterwards (data set earlier with ``set_imager_data`` are put back instead, the way ``installed_weights`` puts the model's
        weights back); ``None`` leaves the plan's state alone.  The arguments are checked before any library call."""
        return _InstalledImager(self, imager)

    def _refuse_imager(self, what, imager=None):
        if imager is not None or self._imager_data is not None and self._imager_data[1] > 0:
            raise ValueError(f"{what} does not carry the imager data term: clear it (set_imager_data(None)), or use cg / mmmg")

    # ---- solver on one GPU ------------------------------------------------------------------
    def cg(self, data, mu=1.0, mu_reg=0.0, x0=None, max_iter=10, tol=1e-12, refresh=50, callback=None, weights=None,
           data_delta=None, imager=None):
        """Device-resident linear CG (qmm.lcg restated).  ``callback(it, grad_norm, x)`` -- the per-iteration callback
        of ``qmm.lcg`` (fusion_CT.py:194-225) -- receives the 1-based iteration, the grad_norm trace so far and the
        current iterate ``[T,Na,Nb]``; it may call ``forward`` / ``adjoint`` on this model; a truthy return stops.
        ``weights``: data weights ``[osize]`` for this solve only, data term mu (y - A x)^T diag(w) (y - A x) (``set_data_weights``;
        what the model held is put back afterwards); None: the model's own state.  ``data_delta`` must stay None: the robust
        data term of ``mmmg`` is not quadratic.  ``imager=(y_im, mu_imager[, w_im])``: the imager's data term for this solve
        (``set_imager_data``; cleared afterwards, or, where ``set_imager_data`` had set a term before, that one put back) -- the
        loop then runs on the maps, not on their spectra."""
        if data_delta is not None:
            raise ValueError("cg minimises quadratic criteria only: a robust data term (data_delta) needs mmmg")
        with_imager = self.installed_imager(imager)             # checked here, before any library call
        with self.installed_weights(weights), with_imager:
            return _lib.solve(self, self._L.surfh_cg_cb, data, mu, mu_reg, x0, max_iter, tol, refresh, callback)

    # ---- posterior sampling (surfh_amd.posterior; include/surfh_amd.h: surfh_cg_sample) ------------------------------------------
    def sample_posterior(self, data, mu=1.0, mu_reg=0.0, n_samples=16, seed=0, x0=None, max_iter=10, tol=1e-12, refresh=50,
                         weights=None, perturbations=None, callback=None):
        """Per-pixel uncertainty of the maps ``cg`` returns.  The criterion of ``cg`` is the negative log of the Gaussian posterior
        ``p(x | y) ~ exp(-x^T Q x / 2 + b^T x)``, ``Q = mu A^T W A + mu_reg (Dr^T Dr + Dc^T Dc)``, ``b = mu A^T W y``: the precision
        is ``Q`` as ``cg`` defines it, a statistical statement once ``weights = 1 / sigma^2`` (``mu = 1``).  Runs ``cg`` (same
        arguments, same bits), then ``n_samples`` perturbed solves ``Q x~ = b~``, ``b~ ~ N(b, Q)`` -- each as the solve of its deviation
        ``Q e = b~ - b`` from zero, ``x~ = x_map + e`` -- with the same ``max_iter``, ``tol`` and ``refresh``, and returns a ``PosteriorResult``: ``x_map``, ``mean``, ``cov``
        ``[T, T, Na, Nb]``, ``std``, ``nit``, ``grad_norm`` (of the unperturbed solve) and ``rr_worst``, the largest final r.r over
        the sample solves.  A sample is exact only if its solve converges: CG stopped at ``max_iter`` leaves the slowly converging
        directions under-dispersed and ``std`` is then a lower bound -- compare ``rr_worst`` with the ``rr[0]`` the callback sees.

        ``seed``: the counter-based generator's 64-bit key; the same seed gives the same bits, whatever ran before.
        ``weights``: as in ``cg``.  ``perturbations=(eps_y [K, osize], eps_r [K, isize], eps_c [K, isize])``: the standard normal
        vectors of every draw instead of the generator's (what makes a float64 comparison possible).
        ``callback(k, rr, x)``: every finished sample -- its index, the r.r trace of its solve, ``x~`` ``[T, Na, Nb]``; a truthy
        return aborts the run (``RuntimeError``).  ``ValueError`` for a model without templates, the joint prior, an active
        imager term, ``mu <= 0``, ``mu_reg < 0`` and ``n_samples < 2``."""
        from . import posterior
        return posterior.sample_posterior(self, data, mu, mu_reg, n_samples, seed, x0, max_iter, tol, refresh, weights, perturbations,
                                          callback)

    def cube_std(self, cov, planes=None):
        """``sqrt(s_lambda^T Sigma s_lambda)`` per pixel: the standard deviation of the cube's ``planes`` (None: all) under the
        maps' covariance ``cov`` ``[T, T, Na, Nb]`` of ``sample_posterior`` (NumPy, on the host)."""
        from . import posterior
        return posterior.cube_std(cov, self.templates, planes)

    def randn_dev(self, out_t, n: int, seed: int = 0, stream: int = 0, sample: int = 0):
        """``n`` standard normals of (seed, stream, sample, element index) into a device tensor (include/surfh_amd.h: surfh_randn_dev)."""
        _lib.check(self._L.surfh_randn_dev(self._plan, dev_ptr(out_t), int(n), _lib.seed64(seed), int(stream), int(sample)))

    def po_data_dev(self, y_t, w_t, eps_t, out_t, n: int, mu: float):
        """out = y + eps / sqrt(mu w) where w > 0 (``w_t=None``: 1), the bits of y elsewhere; device vectors of ``n`` floats."""
        _lib.check(self._L.surfh_po_data_dev(self._plan, dev_ptr(y_t), dev_ptr(w_t), dev_ptr(eps_t), int(n), float(mu),
                                             dev_ptr(out_t)))

    def po_prior_dev(self, er_t, ec_t, out_t, mu_reg: float):
        """out = sqrt(mu_reg) (Dr^T eps_r + Dc^T eps_c) on device maps ``[T, Na, Nb]``."""
        _lib.check(self._L.surfh_po_prior_dev(self._plan, dev_ptr(er_t), dev_ptr(ec_t), float(mu_reg), dev_ptr(out_t)))

    def mmmg(self, data, mu=1.0, mu_reg=0.0, x0=None, max_iter=10, tol=1e-12, refresh=50, callback=None, delta=None, weights=None,
             data_delta=None, potential="huber", data_potential="huber", imager=None, coupling="none"):
        """Device-resident 3MG (qmm.mmmg restated for quadratic objectives; the reference's ``method='mmmg'``,
        fusion_CT.py:194-198).  Same arguments as ``cg``; ``grad_norm`` holds |grad| (not squared) of every iterate.

        ``delta`` (a number): the spatial priors are Huber potentials of threshold ``delta`` on the separated circular
        differences instead (qmm.Huber, the reference's lmm_reconstruction, algorithms.py:73-106) and the criterion is
        ``mu |y - A x|^2 / 2 + mu_reg sum_k sum phi(D_k x)`` (include/surfh_amd.h: surfh_mmmg_huber); the prior value of the
        returned iterate is left in ``self.huber_prior_value`` (None after a quadratic run, and before any run).  qmm is not
        available to pin this restatement against.  ``None`` runs the quadratic solver above.  ``weights`` as in ``cg``.

        ``data_delta`` (a number): the data term is robust, ``mu sum_i phi_data_delta(t_i)`` with ``t_i = sqrt(w_i) (y_i - (A x)_i)``
        (qmm.Objective with a Huber loss; include/surfh_amd.h: surfh_mmmg_robust) -- with ``weights = 1 / sigma^2`` the threshold is
        in units of sigma, 3 say, and samples further off (cosmic-ray hits, warm pixels no flag marks) pull linearly instead of
        quadratically.  The priors stay what ``delta`` says (``None``: quadratic, on the separated differences).  Afterwards
        ``self.robust_weights`` holds ``omega(t) = phi'(t) / t`` ``[osize]`` of the returned iterate (1 inside the threshold, below 1
        beyond, 0 where the weight is 0), ``self.robust_data_value`` ``sum phi(t)`` and ``self.robust_n_beyond`` the number of
        samples beyond; all three are None after any other run.  ``None`` runs exactly the solvers above.

        ``potential`` / ``data_potential``: the potential of the priors under ``delta`` and of the data term under ``data_delta``
        for this call -- "huber" (the default), "hyperbolic" or "hebert_leahy" (``surfh_amd.potentials``); the plan's slots are put
        back afterwards.  ``ValueError`` for another potential than Huber without its threshold.  ``robust_n_beyond`` counts the
        samples past the knee, |t| > data_delta, whatever the potential.

        ``imager=(y_im, mu_imager[, w_im])``: the imager's data term for this solve, as in ``cg``; not with ``data_delta``
        (``ValueError`` before the library is reached).

        ``coupling``: which differences share one potential under ``delta``, for this call -- "none" (the default: each its own),
        "isotropic" (the row and the column difference of a pixel, ``phi(sqrt(u_r^2 + u_c^2))``) or "vector" (those of all ``T``
        maps at a pixel, ``phi(sqrt(sum_t u_r^2 + u_c^2))``: edges co-locate across maps); ``surfh_amd.potentials``.  ``delta`` is
        then the threshold on the **group magnitude**: for comparable behaviour it grows like ``sqrt(2)``, and like
        ``sqrt(2 T)`` for "vector".  It composes with ``potential``, ``data_delta``, ``weights`` and ``imager``; the plan's
        coupling (``set_prior_coupling``) is put back afterwards.  ``ValueError`` for a coupling without ``delta`` and on a model
        whose prior is the joint Laplacian (``set_prior('joint')``)."""
        _pot.need_delta(potential, delta, "delta")
        _pot.need_delta_coupling(coupling, delta)
        if _pot.coupling_code(coupling) != 0 and self.get_prior() != "separated":
            raise ValueError("a prior coupling groups the separated differences: set_prior('separated')")
        _pot.need_delta(data_potential, data_delta, "data_delta")
        if data_delta is not None:
            self._refuse_imager("the robust data term (data_delta)", imager)
        with_imager = self.installed_imager(imager)             # checked here, before any library call
        with_coupling = _pot.installed_coupling(self, coupling if delta is not None else None)
        with _pot.installed(self, spatial=potential, data=data_potential), with_coupling, with_imager:
            return self._mmmg(data, mu, mu_reg, x0, max_iter, tol, refresh, callback, delta, weights, data_delta)

    def _mmmg(self, data, mu, mu_reg, x0, max_iter, tol, refresh, callback, delta, weights, data_delta):
        self.huber_prior_value = None
        self.robust_weights = self.robust_data_value = self.robust_n_beyond = None
        if data_delta is not None and self.get_prior() != "separated":
            raise ValueError("the robust data term (data_delta) comes with priors on the separated differences: set_prior('separated')")
        with self.installed_weights(weights):
            if data_delta is not None:
                x, gn, nit, vals, omega = _lib.solve_robust(self, data, mu, data_delta, mu_reg, float("inf") if delta is None else delta,
                                                            x0, max_iter, tol, refresh, callback)
                self.robust_data_value, self.robust_n_beyond, self.robust_weights = vals[0], int(round(vals[1])), omega
                if delta is not None:
                    self.huber_prior_value = vals[2]
                return x, gn, nit
            if delta is None:
                return _lib.solve(self, self._L.surfh_mmmg, data, mu, mu_reg, x0, max_iter, tol, refresh, callback)
            x, gn, nit, self.huber_prior_value = _lib.solve_huber(self, data, mu, mu_reg, delta, x0, max_iter, tol, refresh, callback)
        return x, gn, nit

    def huber_curv_dev(self, x_t, p0_t, p1_t, delta: float) -> np.ndarray:
        """sum_k sum w(D_k x) (D_k p0)^2, (D_k p0)(D_k p1), (D_k p1)^2 on device maps: the prior block of the Huber majorant.
        Under a coupling of the plan (``set_prior_coupling``) w is the weight of the difference's group, w(m), and ``delta`` the
        threshold on the group magnitude m."""
        out = np.zeros(3, dtype=np.float64)
        _lib.check(self._L.surfh_huber_curv_dev(self._plan, dev_ptr(x_t), dev_ptr(p0_t), dev_ptr(p1_t), float(delta), _lib.dptr(out)))
        return out

    def robust_data_dev(self, y_t, u_t, w_t, v_t, n: int, data_delta: float):
        """v = sqrt(w) phi'(t), t = sqrt(w) (y - u), on device vectors of ``n`` floats (``w_t=None``: every weight 1; a weight of 0
        takes its sample out whatever y holds); returns (sum phi(t), number of |t| > data_delta) (synchronises)."""
        out = np.zeros(2, dtype=np.float64)
        _lib.check(self._L.surfh_robust_data_dev(self._plan, dev_ptr(y_t), dev_ptr(u_t), dev_ptr(w_t), int(n),
                                                 float(data_delta), dev_ptr(v_t), _lib.dptr(out)))
        return float(out[0]), int(round(out[1]))

    def robust_curv_dev(self, y_t, u_t, w_t, p0_t, p1_t, n: int, data_delta: float) -> np.ndarray:
        """sum w omega(t) p0^2, p0 p1, p1^2 on device vectors of ``n`` floats: the data block of the robust majorant."""
        out = np.zeros(3, dtype=np.float64)
        _lib.check(self._L.surfh_robust_curv_dev(self._plan, dev_ptr(y_t), dev_ptr(u_t), dev_ptr(w_t), dev_ptr(p0_t),
                                                 dev_ptr(p1_t), int(n), float(data_delta), _lib.dptr(out)))
        return out

    def huber_prior_dev(self, x_t, g_t, mu_reg: float, delta: float) -> float:
        """g += mu_reg sum_k D_k^T phi'(D_k x) on device maps [T, Na, Nb]; returns sum_k sum phi(D_k x) (synchronises).  Under a
        coupling of the plan (``set_prior_coupling``): g += mu_reg sum_k D_k^T (w(m) D_k x), returns sum phi(m) over the groups,
        ``delta`` the threshold on the group magnitude m (``potentials.group_magnitude``)."""
        out = C.c_double()
        _lib.check(self._L.surfh_huber_prior_dev(self._plan, dev_ptr(x_t), dev_ptr(g_t), float(mu_reg), float(delta), C.byref(out)))
        return out.value

    def prior_passes_dev(self, x_t, g_t, p0_t, p1_t, mu_reg: float, delta: float, potential="huber", coupling="none"):
        """Diagnostic: ``huber_prior_dev`` and ``huber_curv_dev`` in one call on device arrays of any shape ``[T, Na, Nb]`` (every
        extent >= 1, whatever the model's own shape), under an explicit potential and coupling; the plan's state is not consulted.
        Returns (g.g, prior value, curvature block [3]) (synchronises)."""
        T, na, nb = (int(v) for v in x_t.shape)
        out = np.zeros(5, dtype=np.float64)
        _lib.check(self._L.surfh_debug_prior_passes(self._plan, T, na, nb, _pot.kind_code(potential), _pot.coupling_code(coupling),
                                                    dev_ptr(x_t), dev_ptr(g_t), dev_ptr(p0_t), dev_ptr(p1_t), float(mu_reg), float(delta),
                                                    _lib.dptr(out)))
        return float(out[0]), float(out[1]), out[2:].copy()

    # ---- the cube itself under Huber priors (models without templates) -----------------------
    def mmmg_vox(self, data, mu=1.0, spat_reg=1.0, spat_delta=1.0, spec_reg=1.0, spec_delta=1.0, x0=None, max_iter=10, tol=1e-12,
                 refresh=50, callback=None, weights=None, data_delta=None, spat_potential="huber", spec_potential="huber",
                 data_potential="huber"):
        """3MG on the cube ``[Lc, Na, Nb]`` with Huber priors on its row, column and wavelength differences (the reference's
        vox_reconstruction, algorithms.py:27-71; include/surfh_amd.h: surfh_mmmg_huber_vox):

            mu |y - A x|^2 / 2 + spat_reg sum_{k in r,c} sum phi_spat_delta(D_k x) + spec_reg sum phi_spec_delta(D_l x)

        ``D_r`` / ``D_c`` circular inside every plane, ``D_l x = x[l+1] - x[l]`` open along wavelength (``Lc - 1`` planes).  The
        reference's legacy ``Spectro`` model is ``(alpha, beta, lambda)``, hence its ``Diff(0) / Diff(1) / Diff(2)``; the cube
        here is ``[lambda][alpha][beta]``.  Needs a model built with ``templates=None``.  Returns ``(x, grad_norm, nit)`` as
        ``mmmg`` and leaves ``self.huber_prior_values = (spatial, spectral)``.  A delta of ``inf`` makes its term quadratic, a
        weight of 0 switches it off.  qmm and aljabr are not available to pin the restatement or the border conventions.
        ``weights``: data weights for this solve, as in ``cg`` (the data term is then ``mu (y - A x)^T W (y - A x) / 2``).
        ``data_delta``: the robust data term of ``mmmg`` (include/surfh_amd.h: surfh_mmmg_robust_vox), with the same diagnostics
        left in ``self.robust_weights``, ``self.robust_data_value`` and ``self.robust_n_beyond``; ``None``: the solver above.
        ``spat_potential`` / ``spec_potential`` / ``data_potential``: the potential of the in-plane families, of the wavelength
        family and of the data term for this call, as ``mmmg``'s (a data potential other than Huber needs ``data_delta``)."""
        _pot.need_delta(data_potential, data_delta, "data_delta")
        self._refuse_imager("mmmg_vox")
        with _pot.installed(self, spatial=spat_potential, spectral=spec_potential, data=data_potential):
            return self._mmmg_vox(data, mu, spat_reg, spat_delta, spec_reg, spec_delta, x0, max_iter, tol, refresh, callback, weights,
                                  data_delta)

    def _mmmg_vox(self, data, mu, spat_reg, spat_delta, spec_reg, spec_delta, x0, max_iter, tol, refresh, callback, weights,
                  data_delta):
        self.huber_prior_values = None
        self.robust_weights = self.robust_data_value = self.robust_n_beyond = None
        if self.lmm:
            raise ValueError("mmmg_vox reconstructs the cube itself: build the model with templates=None "
                             "(mmmg(delta=...) is the solver of a template model)")
        with self.installed_weights(weights):
            if data_delta is not None:
                x, gn, nit, vals, omega = _lib.solve_robust_vox(self, data, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta,
                                                                x0, max_iter, tol, refresh, callback)
                self.robust_data_value, self.robust_n_beyond, self.robust_weights = vals[0], int(round(vals[1])), omega
                self.huber_prior_values = (vals[2], vals[3])
                return x, gn, nit
            x, gn, nit, self.huber_prior_values = _lib.solve_huber_vox(self, data, mu, spat_reg, spat_delta, spec_reg, spec_delta, x0,
                                                                       max_iter, tol, refresh, callback)
        return x, gn, nit

    def huber_vox_prior_dev(self, x_t, g_t, spat_reg: float, spat_delta: float, spec_reg: float, spec_delta: float):
        """g += spat_reg sum_k D_k^T phi'(D_k x) + spec_reg D_l^T phi'(D_l x) on device cubes [Lc, Na, Nb]; returns the spatial
        and the spectral sum of phi (synchronises)."""
        out = np.zeros(2, dtype=np.float64)
        _lib.check(self._L.surfh_huber_vox_prior_dev(self._plan, dev_ptr(x_t), dev_ptr(g_t), float(spat_reg), float(spat_delta),
                                                     float(spec_reg), float(spec_delta), _lib.dptr(out)))
        return float(out[0]), float(out[1])

    def huber_vox_curv_dev(self, x_t, p0_t, p1_t, spat_delta: float, spec_delta: float) -> np.ndarray:
        """[2, 3]: sum w (D p0)^2, (D p0)(D p1), (D p1)^2 under the spatial weights (row 0: rows and columns together) and under
        the spectral weights (row 1), on device cubes: the prior blocks of the majorant before spat_reg / spec_reg."""
        out = np.zeros(6, dtype=np.float64)
        _lib.check(self._L.surfh_huber_vox_curv_dev(self._plan, dev_ptr(x_t), dev_ptr(p0_t), dev_ptr(p1_t), float(spat_delta),
                                                    float(spec_delta), _lib.dptr(out)))
        return out.reshape(2, 3)

    # ---- helpers the reference's drivers call -----------------------------------------------
    def cubeTomaps(self, cube):
        """lmm_cube2maps (spectroModel.py:187-188, jax_utils.py:18-26) on the device."""
        cube = np.ascontiguousarray(np.asarray(cube, dtype=np.float32))
        tpl = np.ascontiguousarray(self.templates, dtype=np.float64)
        if cube.shape != (tpl.shape[1], self.ishape[-2], self.ishape[-1]):
            raise ValueError(f"cube shape {cube.shape} != {(tpl.shape[1], self.ishape[-2], self.ishape[-1])}")
        out = np.empty((tpl.shape[0],) + cube.shape[1:], dtype=np.float32)
        _lib.check(self._L.surfh_cube_to_maps(self._plan, _lib.dptr(tpl), tpl.shape[0], tpl.shape[1], _lib.fptr(cube), _lib.fptr(out)))
        return out.astype(np.float64)

    def mapsToCube(self, maps):
        """lmm_maps2cube (spectroModel.py:190-198, jax_utils.py:10-16) on the device."""
        tpl = np.ascontiguousarray(self.templates, dtype=np.float64)
        maps = np.ascontiguousarray(np.asarray(maps, dtype=np.float32).reshape((tpl.shape[0],) + tuple(self.ishape[-2:])))
        out = np.empty((tpl.shape[1],) + maps.shape[1:], dtype=np.float32)
        _lib.check(self._L.surfh_maps_to_cube(self._plan, _lib.dptr(tpl), tpl.shape[0], tpl.shape[1], _lib.fptr(maps), _lib.fptr(out)))
        return out.astype(np.float64)

    def real_data_janskySR_to_jansky(self, data):
        """Jy/sr -> Jy normalisation of slit data (spectroModel.py:225-239)."""
        out = np.zeros_like(data)
        for k, ch in enumerate(self.channels):
            d = np.array(data[self._idx[k]: self._idx[k + 1]]).reshape(self.instrs_oshape[k])
            for s in range(self.instrs_oshape[k][1]):
                sl = ch.slicer.get_slit_slices(s)
                w = ch.slicer.get_slit_weights(s, sl)
                d[:, s, :, :] = d[:, s, :, :] * np.sum(w[0, 0, :]) * self.srfs[self.owned[k]]
            out[self._idx[k]: self._idx[k + 1]] = d.ravel()
        return out

    # ---- instrumentation (profile_*: PlanOwner) ------------------------------------------------
    def debug_buffer(self, which: str) -> np.ndarray:
        dims = (C.c_int64 * 4)()
        _lib.check(self._L.surfh_debug_dims(self._plan, which.encode(), dims))
        shape = tuple(int(d) for d in dims)
        if which in ("info", "range", "ksteps", "otf", "trim") or which.startswith("xsinfo:"):
            return np.array(shape)
        while len(shape) > 1 and shape[-1] == 1:
            shape = shape[:-1]
        out = np.empty(int(np.prod(shape)), dtype=np.float32)
        n = self._L.surfh_debug_copy(self._plan, which.encode(), _lib.fptr(out), out.size)
        if n < 0:
            raise RuntimeError(self._L.surfh_last_error().decode())
        return out.reshape(shape)
