"""``MRSBlurred``: the 2-D, no-rotation operator of the reference's deconvolution path
(surfh/Models/spectro_blind_rectangle.py:27-332, driver scripts/deconvolution_mrs_noRotation.py:170-212)
evaluated by the HIP library.

    y[p, s, a] = sum_beta  w_s[beta] * boxsum_alpha(crop_p(C x))[alpha0 + a*srf, beta]

C = 2-D OTF multiply, crop = integer-shift gridding (:286-307), box-sum = srf consecutive alpha rows
(:201-204), slit window with beta-edge weights, alpha decimation and beta sum (:206-208).  The crop is
exactly transposable, so ``adjoint`` is both the exact transpose and the reference's adjoint (:212-237).

The slit geometry, the plan and the solvers are shared with the rotated-field variant ``spectro_blind.MRSBlurred``
(``blurred2d.Blurred2D``); ``instr.fov.angle`` is not used here, as in the reference class.

``sotf`` may be ``[N_alpha, N_beta/2+1]`` (the reference's single image) or
``[L, N_alpha, N_beta/2+1]``: the L wavelength planes are independent problems evaluated as one batch
(BASELINE.json configs[4]); ``forward`` then maps ``[L, N_alpha, N_beta] -> [L, P*S*alpha_out]``.
"""
from __future__ import annotations

import numpy as np

from . import instru
from .blurred2d import Blurred2D, plane_coupling_code
from .potentials import COUPLING_NAMES, kind_name, need_delta, need_delta_coupling, phi as potential_phi, prior_value
from .weights import check_data_weights, weighted_sq_residual


class MRSBlurred(Blurred2D):
    """The field of view's angle is not used: like the reference class, the gridding is an axis-aligned crop whatever
    ``instr.fov.angle`` is (a rotated field of view is ``spectro_blind.MRSBlurred``)."""

    def __init__(self, sotf, alpha_axis, beta_axis, instr: instru.IFU, step_degree: float,
                 pointings: instru.CoordList, *, device: int = 0, stream=None, exact: int = 0):
        super().__init__(sotf, alpha_axis, beta_axis, instr, step_degree, pointings)
        slices, weights = self._slit_tables()
        na, nb = self.local_im_shape
        P = len(pointings)
        i0 = np.empty((P, na * nb), dtype=np.int32)
        i1 = np.empty_like(i0)
        y0 = np.empty((P, na * nb), dtype=np.float64)
        y1 = np.empty_like(y0)
        self.crops = []
        for p, pt in enumerate(pointings):          # integer crop (:286-307) written as degenerate bilinear taps
            ia = int(np.abs(self.alpha_axis - pt.alpha).argmin())
            ib = int(np.abs(self.beta_axis - pt.beta).argmin())
            sa, sb = ia - na // 2, ib - nb // 2
            if sa < 0 or sb < 0 or sa + na > self.imshape[0] or sb + nb > self.imshape[1] or na % 2 == 0 or nb % 2 == 0:
                raise ValueError(f"pointing {p}: the {na}x{nb} field of view does not fit in the {self.imshape} image")
            self.crops.append((sa, sa + na, sb, sb + nb))
            ra = np.repeat(np.arange(sa, sa + na), nb)
            rb = np.tile(np.arange(sb, sb + nb), na)
            la, lb = np.minimum(ra, self.imshape[0] - 2), np.minimum(rb, self.imshape[1] - 2)
            i0[p], i1[p], y0[p], y1[p] = la, lb, ra - la, rb - lb
        self._set_tables(slices, weights, i0, i1, y0, y1)
        self._create_plan(device, stream, exact)

    def data_to_img(self, data):
        """The reference's quick-look back-projection of slit data (spectro_blind_rectangle.py:240-283; the reference's scripts
        call the rotated class's variant, ``spectro_blind.MRSBlurred.data_to_img``): every sample spread evenly over its slit's
        beta columns, put back on the local grid (slit windows with their beta-edge weights), summed over the srf-row window
        (the transposed box), values below 1 zeroed and local columns 5 / 153 overwritten by their neighbours 6 / 152 as the
        reference does (so the local grid needs >= 154 columns, as there), placed in the image at each pointing.  Returns
        ``(weighted_mean, global_img)``: the mean over the pointings that cover a pixel (0 where none does; the reference
        leaves those entries uninitialised) and the plain sum.  Host NumPy: a plotting aid on one image, not part of the
        operator."""
        d = self._d2i_data(data)
        cum = np.zeros((len(self.crops),) + self.imshape)
        for p, (a0, a1, b0, b1) in enumerate(self.crops):
            cum[p, a0:a1, b0:b1] = self._d2i_local(d, p, self.npix_slit_beta_width)
        valid = np.sum(cum != 0, axis=0)
        total = np.sum(cum, axis=0)
        return np.divide(total, valid, out=np.zeros(self.imshape), where=valid != 0), total


class QuadCriterion_MRS_2D:
    """The reference's 2-D criterion (surfh/Simulation/criterion_2D.py:66-250): same constructor, ``run_method('lcg' | 'mmmg')``
    and ``get_crit_val``, on ``MRSBlurred`` (one image, or a stack of independent images solved together)."""

    def __init__(self, mu_spectro, y_spectro, model_spectro, mu_reg, printing=False, gradient="separated", weights=None, delta=None,
                 potential="huber", coupling="none"):
        """``weights`` (not in criterion_2D.py): per-sample data weights in the layout of ``y_spectro``, data term
        mu (y - A x)^T diag(w) (y - A x) / 2 (``MRSBlurred.set_data_weights``); data of weight 0 are ignored whatever they hold.
        ``None``: the weights the model holds, if any.
        ``delta`` (criterion_2D.py imports qmm's ``Huber`` beside ``mmmg`` and never builds it): Huber potentials of threshold
        ``delta`` on the separated differences, criterion mu |y - A x|^2 / 2 + mu_reg sum_k sum phi(D_k x) per plane
        (include/surfh_amd.h: surfh_mmmg_huber_planes), as ``fusion.QuadCriterion_MRS``; only a method other than ``"lcg"``
        minimises it.  ``None``: the quadratic criterion.
        ``potential``: the potential under ``delta``, "huber" (the default), "hyperbolic" or "hebert_leahy"
        (``surfh_amd.potentials``); another one than Huber needs ``delta``.
        ``coupling``: "none" (the default) or "isotropic", one potential per pixel on sqrt((Dr x)^2 + (Dc x)^2) with ``delta`` the
        threshold on that magnitude (``MRSBlurred.mmmg``); it needs ``delta``, and "vector" is refused."""
        assert isinstance(mu_reg, (float, int, list, np.ndarray))
        self.potential = kind_name(potential)
        need_delta(potential, delta, "delta")
        self.coupling = COUPLING_NAMES[plane_coupling_code(coupling)]
        need_delta_coupling(self.coupling, delta)
        if delta is not None:
            if gradient != "separated":
                raise ValueError("the Huber prior (delta) acts on the separated differences: gradient must be 'separated'")
            delta = float(delta)
            if not delta > 0.0:
                raise ValueError(f"delta must be positive, not {delta!r}")
        self.delta = delta
        if gradient != "separated":
            raise NotImplementedError("only the separated first-difference priors (NpDiff_r / NpDiff_c) are built")
        self.mu_spectro, self.y_spectro, self.model_spectro, self.mu_reg = mu_spectro, y_spectro, model_spectro, mu_reg
        self.shape_of_output = tuple(model_spectro.ishape)
        self.printing, self.gradient, self.it = printing, gradient, 1
        self.L_crit_val = []
        self.weights = None if weights is None else check_data_weights(weights, model_spectro.osize)

    def run_method(self, method="lcg", maximum_iterations=10, tolerance=1e-12, calc_crit=False, perf_crit=None, value_init=0.5):
        assert isinstance(self.mu_reg, (int, float))             # criterion_2D.py:115
        if self.delta is not None and method == "lcg":
            raise ValueError("lcg minimises quadratic criteria only: a Huber prior (delta) needs method='mmmg'")
        solver = self.model_spectro.cg if method == "lcg" else self.model_spectro.mmmg       # criterion_2D.py:190-193
        init = np.ones(self.shape_of_output) * value_init if isinstance(value_init, (int, float)) else value_init
        assert tuple(np.shape(init)) == self.shape_of_output
        import time
        from .fusion import OptimizeResult
        self.L_crit_val = []
        self.it = 1

        # the four callback modes of criterion_2D.py:163-225 (the same as fusion_CT.py:163-225, see QuadCriterion_MRS.run_method)
        def record_crit(x):
            crit_val = self.get_crit_val(x)
            self.L_crit_val.append(crit_val)
            print(f"Criterion value = {crit_val}\n")

        def print_last_grad_norm(it, gn, x):
            print(f"Iteration n°{self.it}, Grad norm = {np.max(np.atleast_1d(gn[-1]))}")
            self.it = self.it + 1

        def print_last_grad_norm_and_crit(it, gn, x):
            print_last_grad_norm(it, gn, x)
            if self.it % 5 == 2:
                record_crit(x)

        if calc_crit and perf_crit is None:
            print(f"{method} : Criterion calculated at each iteration!")
            callback = lambda it, gn, x: record_crit(x)      # noqa: E731
        elif not calc_crit and perf_crit is not None:
            print(f"{method} : perf_crit calculated at each iteration!")
            callback = print_last_grad_norm
        elif calc_crit and perf_crit is not None:
            print(f"{method} : criterion and gradient printed at each iteration!")
            callback = print_last_grad_norm_and_crit
        else:
            callback = None
        t0 = time.time()
        kw = {} if self.delta is None else {"delta": self.delta}
        if self.potential != "huber":
            kw["potential"] = self.potential
        if self.coupling != "none":
            kw["coupling"] = self.coupling
        if self.weights is not None:
            kw["weights"] = self.weights
        x, gn, nit = solver(self.y_spectro, mu=self.mu_spectro, mu_reg=self.mu_reg, x0=init,
                            max_iter=maximum_iterations, tol=tolerance, callback=callback, **kw)
        last = np.max(np.atleast_1d(gn[-1]))
        last = np.sqrt(last) if method == "lcg" else last           # lcg traces r.r, mmmg |grad|
        res = OptimizeResult(x=x.ravel(), grad_norm=list(gn), nit=nit,
                             success=bool(last < np.prod(self.shape_of_output[-2:]) * tolerance), time=time.time() - t0)
        if self.printing:
            print(f"Total time needed for {method} :", round(res.time, 3))
        return res

    def sample(self, n_samples=16, seed=0, maximum_iterations=10, tolerance=1e-12, value_init=0.5, perturbations=None, callback=None):
        """Posterior samples of this criterion read as a Gaussian log-density (not in criterion_2D.py): forwards to
        ``model_spectro.sample_posterior`` with this criterion's data, weights and hyper-parameters and ``run_method``'s start, and
        returns its ``PlanesPosteriorResult`` (``x_map`` is what ``run_method("lcg", maximum_iterations)`` returns).
        ``ValueError`` for a criterion with a Huber prior (``delta``): its posterior is not Gaussian."""
        assert isinstance(self.mu_reg, (int, float))
        if self.delta is not None:
            raise ValueError("sample: the posterior of a Huber prior (delta) is not Gaussian")
        init = np.ones(self.shape_of_output) * value_init if isinstance(value_init, (int, float)) else value_init
        assert tuple(np.shape(init)) == self.shape_of_output
        return self.model_spectro.sample_posterior(self.y_spectro, mu=self.mu_spectro, mu_reg=self.mu_reg, n_samples=n_samples, seed=seed,
                                                   x0=init, max_iter=maximum_iterations, tol=tolerance, weights=self.weights,
                                                   perturbations=perturbations, callback=callback)

    def get_crit_val(self, x_hat):
        """(mu |y - A x|^2 + mu_reg (|Dr x|^2 + |Dc x|^2)) / 2   (criterion_2D.py:252-275), summed over the planes; with ``delta``
        mu |y - A x|^2 / 2 + mu_reg sum phi(Dr x) + phi(Dc x), phi the criterion's potential (Huber by default); under a coupling
        mu_reg ``potentials.prior_value`` of the planes, sum phi(sqrt((Dr x)^2 + (Dc x)^2)).  Under data weights (this criterion's,
        else the model's) |y - A x|^2 is sum w (y - A x)^2 over the samples with w > 0."""
        x_hat = np.asarray(x_hat).reshape(self.shape_of_output)
        w = self.weights if self.weights is not None else getattr(self.model_spectro, "data_weights", None)
        data = self.mu_spectro * weighted_sq_residual(self.y_spectro, self.model_spectro.forward(x_hat), w)
        dr = np.roll(x_hat, 1, axis=-2) - x_hat
        dc = np.roll(x_hat, 1, axis=-1) - x_hat
        if self.delta is not None and self.coupling != "none":
            planes = x_hat.reshape((-1,) + x_hat.shape[-2:])
            return data / 2 + self.mu_reg * prior_value(planes, self.delta, self.potential, self.coupling)
        if self.delta is not None:
            return data / 2 + self.mu_reg * (potential_phi(dr, self.delta, self.potential).sum() +
                                             potential_phi(dc, self.delta, self.potential).sum())
        return (data + self.mu_reg * np.sum(dr ** 2 + dc ** 2)) / 2
