#!/usr/bin/env python
"""2-D deconvolution of MRS slit data with the no-rotation operator ``MRSBlurred`` on MI355X -- the run of the reference's
``scripts/simulate_deconvolution_mrs_rectangle.py:100-188`` (and ``scripts/deconvolution_mrs_noRotation.py:100-212``):

    mixed_maps = (0.4 m0 + 0.5 m1 + 0.4 m2 + 0.3 m3) * 1e4          one image from four abundance maps      (:135)
    model      = MRSBlurred(sotf, alpha_axis, beta_axis, ch1c, step, 4 pointings)                           (:137-167)
    data       = model.forward(fliplr(mixed_maps))                                                          (:169)
    criterion  = QuadCriterion_MRS_2D(mu_spectro=1, data, model, mu_reg=5, gradient="separated")            (:190-196)
    result     = criterion.run_method("lcg", 600, perf_crit=1, calc_crit=True, value_init=0)                (:198)

The reference reads its maps, PSF and pointings from the author's disk; here they are synthetic (random maps, the Gaussian
PSF of surfh/ToolsDir/utils.py:40-50 at the chosen wavelength, the 1C field of view without rotation, four integer-pixel
pointings) or come from ``--input`` (an .npz with ``maps [4,N,N]``, ``psf [n,n]`` and optionally ``pointings [P,2]`` in
degrees).  ``--planes L`` solves L wavelength planes at once (BASELINE.json configs[4]).  Results: ``res_x.npy``,
``criterion.npy``, ``data.npy`` under ``--out``.

``--angle DEG`` (nonzero) runs the reference scripts' actual operator, the rotated-field ``spectro_blind.MRSBlurred``
(scripts/simulate_deconvolution_mrs_rectangle.py:125-155, scripts/deconvolution_mrs_single_wavelength.py:119-155: the 1C field
of view at ``8.2 - rotation_ref`` degrees, bilinear gridding, so ``--input`` pointings may be fractional); the solver uses the
exact transpose of that operator.  ``--data_to_img`` also writes the quick-look back-projection ``data_to_img`` of the data
(``adj_mean.npy``, ``adj.npy``, deconvolution_mrs_single_wavelength.py:159) and of the result's forward (``adj_mean_fit.npy``,
``adj_fit.npy``, :194), single image only.

``--delta D`` (not in the reference, whose criterion_2D.py imports qmm's ``Huber`` without building it): edge-preserving Huber
priors of threshold D on the row and column differences, minimised by 3MG (``-m`` anything but ``lcg``); the results then go to
``<--out>_huber_<D>``.  ``--potential`` (with ``--delta``) replaces Huber's potential by ``hyperbolic`` or ``hebert_leahy``
(surfh_amd/potentials.py); the results then go to ``<--out>_<kind>_<D>``.  ``--coupling isotropic`` (with ``--delta``) gives a
pixel's row and column difference one potential, on sqrt(u_r^2 + u_c^2) -- isotropic total variation under Huber's potential, D then
the threshold on that magnitude; the directory gains ``_cpl_isotropic``.  ``none`` (the default) keeps today's prior and directory.

``--nonneg`` (with ``-m lcg``; not in the reference either): the same quadratic criterion under ``x >= 0``, every plane its own
problem, by ``MRSBlurred.cg_nonneg`` (ADMM around the CG, surfh_amd/nonneg.py) from ``--value_init``: ``--outer`` outer iterations
(default ``-ni``) of ``--inner`` CG iterations (default 10), penalties ``--rho`` (default: estimated per plane).  The results go to
``<--out>_nn``: the files above, ``criterion.npy`` holding the criterion at the start and at the result, plus ``nn_trace.npy``
``[outer iterations run + 1, 4, planes]``: ``|x - z|``, ``rho |z - z_previous|``, ``|r|``, ``#{z == 0}`` per plane.  Works with
``--angle``.

``--samples K --sample_seed S`` (with ``-m lcg``; not in the reference): per-pixel uncertainty of the result by
``MRSBlurred.sample_posterior`` -- the CG solve, then K perturbed solves with as many iterations (perturbation-optimisation sampling,
surfh_amd/posterior.py; ``--seed`` stays the data's seed).  The results go to ``<--out>_po_<K>``: the files above (``res_x.npy`` the
point estimate), plus ``res_mean.npy`` and ``res_std.npy`` in its shape and ``po_trace.npy`` ``[2, planes]``: per plane the largest
first and the largest final r.r of the sample solves (``rr_first``, ``rr_last``).  Works with ``--angle``.
"""
from __future__ import annotations

import os
import sys
import time

import click
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP = 0.025                       # arcsec per pixel (simulate_deconvolution_mrs_rectangle.py:66)


def build_problem(npix: int, planes: int, seed: int, inp: str | None, angle: float = 0.0):
    from surfh_amd import instru, synth
    step_deg = STEP / 3600
    wl_1c = synth.band_wavelengths("1c")
    rng = np.random.default_rng(seed)
    if inp:
        z = np.load(inp)
        maps = np.asarray(z["maps"], dtype=np.float64)
        npix = maps.shape[-1]
        psf = np.asarray(z["psf"], dtype=np.float64)
        psfs = np.broadcast_to(psf / psf.sum(), (planes,) + psf.shape)
        pts = [tuple(p) for p in z["pointings"]] if "pointings" in z.files else None
    else:
        maps = rng.random((4, npix, npix))
        lam = wl_1c[100] if planes == 1 else np.linspace(wl_1c[100], wl_1c[100] + 0.05, planes)   # instr_wavelength[100] (:73)
        psfs = synth.gaussian_psf(np.atleast_1d(lam), STEP)
        pts = None
    if pts is None:
        s = step_deg
        pts = [(0.0, 0.0), (2 * s, -3 * s), (-4 * s, 1 * s), (3 * s, 5 * s)]
    mixed = (0.4 * maps[0] + 0.5 * maps[1] + 0.4 * maps[2] + 0.3 * maps[3]) * 10000          # :135
    ax = synth.axes(npix, step_deg)
    ch1c = instru.IFU(fov=instru.FOV(3.2 / 3600, 3.7 / 3600, origin=instru.Coord(0, 0), angle=angle), det_pix_size=0.196,
                      n_slit=21, w_blur=instru.SpectralBlur(float(np.mean([3100, 3610]))), pce=None, wavel_axis=wl_1c, name="1C")
    sotf = synth.ir2fr(psfs, (npix, npix))
    if planes == 1:
        sotf = sotf[0]
    truth = np.fliplr(mixed)                                                                  # :169
    if planes > 1:
        truth = np.stack([truth * (1.0 + 0.1 * k / planes) for k in range(planes)])
    return dict(sotf=sotf, alpha_axis=ax, beta_axis=ax.copy(), ifu=ch1c, step_deg=step_deg,
                pointings=instru.CoordList([instru.Coord(a, b) for a, b in pts]), truth=truth)


def result_dir(out, delta, potential="huber", coupling="none"):
    """<out>_huber_<delta> as before; another potential puts its name in Huber's place, a coupling appends _cpl_<coupling>"""
    name = f"{out}_{potential}_{delta:g}"
    return name if coupling == "none" else f"{name}_cpl_{coupling}"


def samples_dir(out, samples):
    """<out>_po_<K>"""
    return f"{out}_po_{samples}"


@click.command()
@click.option("-np", "--npix", default=251, type=int, help="image size (the reference's maps are 251 x 251)")
@click.option("-hp", "--hyper_parameter", default=5.0, type=float, help="mu_reg (reference: 5)")
@click.option("-ni", "--niter", default=600, type=int, help="iterations (reference: 600)")
@click.option("-m", "--method", default="lcg", type=str, help="'lcg' or anything else for 3MG (criterion_2D.py:190-193)")
@click.option("-vi", "--value_init", default=0.0, type=float)
@click.option("--planes", default=1, type=int, help="wavelength planes solved at once (independent 2-D problems)")
@click.option("--input", "inp", default=None, type=str, help=".npz with maps, psf[, pointings]")
@click.option("--out", default="deconvolution_results", type=str)
@click.option("--quiet", is_flag=True, help="no per-iteration prints (the reference prints every iteration)")
@click.option("--seed", default=19940407, type=int)
@click.option("--device", default=0, type=int)
@click.option("--angle", default=0.0, type=float,
              help="field-of-view angle in degrees; nonzero: the rotated-field operator spectro_blind.MRSBlurred (reference: 8.2)")
@click.option("--data_to_img", is_flag=True, help="also write data_to_img of the data and of the result's forward")
@click.option("--delta", default=None, type=float,
              help="Huber threshold of the priors (needs -m other than lcg); results go to <out>_huber_<delta>")
@click.option("--potential", default="huber", type=click.Choice(["huber", "hyperbolic", "hebert_leahy"]),
              help="potential of the priors under --delta; other than huber: results go to <out>_<potential>_<delta>")
@click.option("--coupling", default="none", type=click.Choice(["none", "isotropic"]),
              help="coupling of a pixel's row and column difference under --delta (isotropic: total variation); "
                   "other than none: results go to <out>_<potential>_<delta>_cpl_<coupling>")
@click.option("--nonneg", is_flag=True, default=False,
              help="solve under x >= 0 (ADMM around the CG, -m lcg); results go to <out>_nn, with nn_trace.npy")
@click.option("--rho", default=None, type=float, help="ADMM penalty of every plane (--nonneg); default: estimated per plane")
@click.option("--outer", default=None, type=int, help="outer iterations (--nonneg); default: -ni")
@click.option("--inner", default=None, type=int, help="CG iterations per outer iteration (--nonneg); default: 10")
@click.option("--samples", default=None, type=int,
              help="posterior samples for a per-pixel error bar (-m lcg, at least 2); results go to <out>_po_<samples>")
@click.option("--sample_seed", default=0, type=int, help="key of the sampler's generator (--samples); --seed is the data's")
def main(npix, hyper_parameter, niter, method, value_init, planes, inp, out, quiet, seed, device, angle, data_to_img, delta,
         potential="huber", coupling="none", nonneg=False, rho=None, outer=None, inner=None, samples=None, sample_seed=0):
    if samples is not None:
        if method != "lcg":
            raise click.UsageError("--samples draws from the Gaussian posterior of the quadratic criterion: use it with -m lcg, not qmm / 3MG")
        if delta is not None:
            raise click.UsageError("--samples: the posterior of a Huber prior (--delta) is not Gaussian")
        if nonneg:
            raise click.UsageError("--samples: the posterior under --nonneg is not Gaussian")
        if samples < 2:
            raise click.UsageError(f"--samples: a standard deviation needs at least 2 samples, not {samples}")
    if nonneg:
        if method != "lcg":
            raise click.UsageError("--nonneg runs ADMM around the linear CG; use it with -m lcg")
        if delta is not None:
            raise click.UsageError("--nonneg constrains the quadratic criterion: no --delta")
        if rho is not None and not (np.isfinite(rho) and rho > 0):
            raise click.BadParameter(f"must be finite and > 0, not {rho}", param_hint="--rho")
        if inner is not None and inner < 1:
            raise click.BadParameter(f"at least one CG iteration, not {inner}", param_hint="--inner")
        if outer is not None and outer < 1:
            raise click.BadParameter(f"at least one outer iteration, not {outer}", param_hint="--outer")
        out = out + "_nn"
    elif rho is not None or outer is not None or inner is not None:
        raise click.UsageError("--rho, --outer and --inner belong to --nonneg")
    if potential != "huber" and delta is None:
        raise click.UsageError("--potential needs --delta: a potential of the quadratic prior means nothing")
    if coupling != "none" and delta is None:
        raise click.UsageError("--coupling needs --delta: a coupling of the quadratic prior means nothing")
    if delta is not None:
        if method == "lcg":
            raise ValueError("lcg minimises quadratic criteria only: a Huber prior (delta) needs method='mmmg'")
        out = result_dir(out, delta, potential, coupling)
    if samples is not None:
        out = samples_dir(out, samples)
    if angle:
        from surfh_amd.spectro_blind import MRSBlurred, QuadCriterion_MRS_2D
    else:
        from surfh_amd.spectro_blind_rectangle import MRSBlurred, QuadCriterion_MRS_2D
    if data_to_img and planes != 1:
        raise click.UsageError("--data_to_img is defined for a single image (--planes 1)")
    prob = build_problem(npix, planes, seed, inp, angle)
    model = MRSBlurred(prob["sotf"], prob["alpha_axis"], prob["beta_axis"], prob["ifu"], prob["step_deg"], prob["pointings"],
                       device=device)
    simulated_data = model.forward(prob["truth"])
    crit = QuadCriterion_MRS_2D(mu_spectro=1, y_spectro=np.copy(simulated_data), model_spectro=model, mu_reg=hyper_parameter,
                                printing=True, gradient="separated", delta=delta, potential=potential, coupling=coupling)
    t0 = time.time()
    nn = po = None
    if samples is not None:
        from surfh_amd.fusion import OptimizeResult
        po = crit.sample(n_samples=samples, seed=sample_seed, maximum_iterations=niter, value_init=value_init)
        res = OptimizeResult(x=po.x_map.ravel(), grad_norm=list(po.grad_norm), nit=po.nit, success=True, time=time.time() - t0)
        crit.L_crit_val = [crit.get_crit_val(np.full(model.ishape, value_init)), crit.get_crit_val(po.x_map)]
        if not quiet:
            first, last = np.atleast_1d(po.rr_first), np.atleast_1d(po.rr_last)
            print(f"{samples} samples: median std {np.median(po.std):.4e}, worst final r.r / first r.r over the planes = "
                  f"{np.max(last / np.where(first > 0, first, 1.0)):.3e}")
    elif nonneg:
        from surfh_amd.fusion import OptimizeResult
        x0 = np.full(model.ishape, value_init)
        nn = model.cg_nonneg(np.copy(simulated_data), mu=1, mu_reg=hyper_parameter, rho=rho, x0=x0, outer=outer or niter, inner=inner or 10)
        res = OptimizeResult(x=nn.x.ravel(), grad_norm=list(nn.grad_norm), nit=nn.nit, success=True, time=time.time() - t0)
        crit.L_crit_val = [crit.get_crit_val(x0), crit.get_crit_val(nn.x)]
        if not quiet:
            for k in range(nn.nit + 1):
                print(f"Outer iteration n°{k}: |x - z| = {np.max(nn.primal[k]):.4e}, rho |z - z_prev| = {np.max(nn.dual[k]):.4e}, "
                      f"|r| = {np.max(nn.grad_norm[k]):.4e}, entries at zero = {int(np.sum(nn.n_active[k]))}")
    elif quiet:
        res = crit.run_method(method, niter, value_init=value_init)
        crit.L_crit_val = [crit.get_crit_val(np.full(model.ishape, value_init)), crit.get_crit_val(res.x)]
    else:
        res = crit.run_method(method, niter, perf_crit=1, calc_crit=True, value_init=value_init)
    dt = time.time() - t0
    x = np.asarray(res.x).reshape(model.ishape)
    err = float(np.linalg.norm(x - prob["truth"]) / np.linalg.norm(prob["truth"]))
    print(f"{method}: {res.nit} iterations in {dt:.2f} s ({res.nit / dt:.1f} it/s incl. callbacks), relative error to the truth {err:.3e}, "
          f"criterion {crit.L_crit_val[0]:.6e} -> {crit.L_crit_val[-1]:.6e}")
    os.makedirs(out, exist_ok=True)
    np.save(os.path.join(out, "res_x.npy"), x)
    np.save(os.path.join(out, "criterion.npy"), np.asarray(crit.L_crit_val))
    np.save(os.path.join(out, "data.npy"), simulated_data)
    if po is not None:
        np.save(os.path.join(out, "res_mean.npy"), po.mean)
        np.save(os.path.join(out, "res_std.npy"), po.std)
        np.save(os.path.join(out, "po_trace.npy"), np.stack([np.atleast_1d(po.rr_first), np.atleast_1d(po.rr_last)]))
    if nn is not None:
        tr = np.stack([nn.primal, nn.dual, nn.grad_norm, nn.n_active.astype(np.float64)], axis=1)
        np.save(os.path.join(out, "nn_trace.npy"), tr.reshape(nn.nit + 1, 4, planes))
    if data_to_img:
        for suffix, d in (("", simulated_data), ("_fit", model.forward(x))):
            adj_mean, adj = model.data_to_img(np.copy(d))
            np.save(os.path.join(out, f"adj_mean{suffix}.npy"), adj_mean)
            np.save(os.path.join(out, f"adj{suffix}.npy"), adj)
    model.close()


if __name__ == "__main__":
    main()
