"""MRS fusion driver on MI355X -- same command line, same result files as the reference's driver
(scripts/main_fusion.py:160-274 of sidiso/surfh), with the HIP operator and the device-resident CG behind it.

    python scripts/main_fusion.py -fd <fusion_dir> -np 501 -hp 5e3 -ni 50 -nt 4 -m lcg
    python scripts/main_fusion.py --synthetic config2 -hp 5e3 -ni 50         # no input files needed
    python scripts/main_fusion.py --synthetic small --voxel -m mmmg -hp 40 --delta 0.005 --spec_reg 20 --spec_delta 0.01
    python scripts/main_fusion.py -fd <fusion_dir> -hp 5e3 -ni 50 --mask_nan --weights inv_variance.npy
    python scripts/main_fusion.py -fd <fusion_dir> -hp 5e3 -ni 50 -m mmmg --weights inv_variance.npy --data_delta 3
    python scripts/main_fusion.py --synthetic small -m mmmg -hp 5e3 --delta 0.1 --potential hebert_leahy

Inputs under ``fusion_dir`` (reference layout, main_fusion.py:65-75): ``Templates/`` (wavelength axis + NMF templates,
.npy), ``PSF/`` (PSF stack, .npy), ``Filtered_slices/`` (one FITS file per band and pointing) -> results in
``Results/<method>_MC_<channels>_MO_4_Temp_<T>_nit_<niter>_mu_<mu>_SD_<scale>/``: ``res_x.npy`` (abundance maps),
``res_cube.npy`` (``mapsToCube`` of them), ``criterion.npy`` (criterion trace, fusion_CT.py:163-175,242-265).  ``--voxel`` reconstructs the cube itself instead (no
templates, Huber priors on its row, column and wavelength differences: the reference's vox_reconstruction,
surfh/ToolsDir/algorithms.py:27-71) and writes ``res_cube.npy`` and ``criterion.npy`` under ``..._vox/``.

``--weights FILE.npy`` gives every detector sample a weight in the data term (``[osize]``, the layout of the data: an inverse
variance, a 0/1 mask of bad pixels), ``--mask_nan`` gives the samples that are NaN or Inf weight 0 -- the reference's real-data
scripts overwrite them with 0 and fit the model to those zeros (scripts/fusion/fusion_real_data.py:175-177).  Either flag adds
``_wgt`` to the result directory's name and ``weights.npy`` to its files; without them nothing changes.

``--data_delta D`` (``--method mmmg`` only) makes the data term robust: Huber's potential of threshold ``D`` on the residuals
scaled by the square root of their weights, so that with inverse-variance weights ``D`` counts sigmas.  Outliers no flag marks
(cosmic-ray hits, warm pixels) then pull linearly instead of quadratically.  The result directory's name gains ``_rob_<D>`` and its
files ``robust_weights.npy``, the weights ``[osize]`` in (0, 1] the last iterate gave every sample (0 where masked).

``--potential`` / ``--data_potential`` (``--method mmmg`` only) and ``--spec_potential`` (``--voxel``) choose the potential under
``--delta``, ``--data_delta`` and ``--spec_delta``: ``huber`` (the default), ``hyperbolic`` or ``hebert_leahy``
(surfh_amd/potentials.py).  With another potential than Huber the directory's ``_huber_<D>`` becomes ``_<kind>_<D>``, its
``_rob_<D>`` ``_rob_<kind>_<D>``, and a voxel-wise run under another spectral potential gains ``_spec_<kind>``.
``--coupling isotropic|vector`` (``--method mmmg --delta D``, not with ``--voxel``) lets the row and column difference of a
pixel, or those of all maps at a pixel, share one potential; ``D`` is then the threshold on the group magnitude and the
directory gains ``_cpl_<coupling>`` behind the threshold.  ``none`` (the default) keeps today's prior and directory.

``--refine_templates K --mu_spec M [--tpl_iter n]`` (``--method lcg`` only) refines the spectra as well: K rounds of ``-ni`` CG
iterations on the maps and ``n`` (default 10) on the templates, under the first-difference prior of weight ``M`` along the wavelength
(surfh_amd/fusion.py: refine_templates).  Results go under ``..._tpl_<K>/``: ``res_x.npy``, ``res_templates.npy``,
``templates_start.npy`` and the joint criterion after every half-step in ``criterion.npy``.  Spectral features narrower than the
detector's wavelength sampling are not recovered: the data do not hold them.

The FITS reader needs astropy (FITS I/O is outside the hot path and not rebuilt here); when it is not importable the
same arrays may be given as ``Filtered_slices/<band>_<k>.npz`` with fields ``data`` (raveled ``[Ldet, S, a_out]`` as in
the FITS primary HDU), ``PA_V3``, ``TARG_RA``, ``TARG_DEC``.  ``--synthetic`` builds one of the benchmark problems
(surfh_amd/synth.py), simulates the slit data with the operator and runs the same reconstruction.
"""
import logging as log
import os
import pathlib
import sys

import click
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from surfh_amd import instru, synth                                   # noqa: E402
from surfh_amd.fusion import QuadCriterion_MRS, weights_from_data     # noqa: E402
from surfh_amd.weights import check_data_weights                      # noqa: E402
from surfh_amd.potentials import COUPLING_NAMES as COUPLINGS           # noqa: E402
from surfh_amd.potentials import NAMES as POTENTIALS                  # noqa: E402
from surfh_amd.models import spectroSigRLSCT                          # noqa: E402

LIST_CHAN = ['1a', '1b', '1c', '2a', '2b', '2c', '3a', '3b', '3c', '4a', '4b', '4c']

def initialize_parameters(fusion_dir_path):
    """Paths and the spatial step (main_fusion.py:65-78)."""
    paths = {
        'psf_dir': os.path.join(fusion_dir_path, 'PSF/'),
        'template_dir': os.path.join(fusion_dir_path, 'Templates/'),
        'save_filter_corrected_dir': os.path.join(fusion_dir_path, 'Filtered_slices/'),
        'result_path': os.path.join(fusion_dir_path, 'Results/'),
        'mask_path': os.path.join(fusion_dir_path, 'Masks/')
    }
    step = 0.025  # arcsec
    return paths, step, step / 3600.0


def load_simulation_data(paths, step, step_angle, npix, n_templates, with_templates=True):
    """Axes, templates and OTF (main_fusion.py:80-101).  `with_templates=False` (a voxel-wise run) reads the wavelength axis only:
    `n_templates` then just names the file the axis comes from, and None is returned for the templates."""
    imshape = (npix, npix)
    origin_alpha_axis = synth.axes(npix, step_angle)
    origin_beta_axis = synth.axes(npix, step_angle)
    if n_templates not in (4, 6):
        raise NameError("No corresponding Templates name")
    tag = f'orion_1ABC_2ABC_3ABC_4ABC_{n_templates}_templates_SS4.npy'
    wavel_axis = np.load(os.path.join(paths['template_dir'], 'wavel_axis_' + tag))
    templates = np.load(os.path.join(paths['template_dir'], 'nmf_' + tag)) if with_templates else None
    spsf = np.load(os.path.join(paths['psf_dir'], 'psfs_pixscale0.025_npix_501_fov12.525_chan_1ABC_2ABC_3ABC_4ABC_SS4.npy'))
    sotf = synth.ir2fr(spsf, imshape)
    if templates is not None:
        templates = templates / 10e3
    return origin_alpha_axis, origin_beta_axis, wavel_axis, templates, sotf


def load_data(list_chan, save_filter_corrected_dir):
    """Slit data, pointing targets and roll angle per band (main_fusion.py:30-63)."""
    data_dict = {'data': {c: [] for c in list_chan}, 'target': {c: [] for c in list_chan},
                 'rotation': {c: 0. for c in list_chan}}
    try:
        from astropy.io import fits
    except ImportError:
        fits = None
    for file in sorted(os.listdir(save_filter_corrected_dir)):
        for chan in list_chan:
            if chan not in file:
                continue
            n_slit, n_det = synth.BANDS[chan][0], synth.BANDS[chan][6][2]
            full = os.path.join(save_filter_corrected_dir, file)
            if file.endswith('.npz'):
                z = np.load(full)
                data, pa, ra, dec = z['data'], float(z['PA_V3']), float(z['TARG_RA']), float(z['TARG_DEC'])
            elif fits is not None:
                with fits.open(full) as hdul:
                    h = hdul[0].header
                    data, pa, ra, dec = hdul[0].data, h['PA_V3'], h['TARG_RA'], h['TARG_DEC']
            else:
                raise RuntimeError(f"{file}: reading FITS needs astropy, which is not installed; "
                                   "provide <band>_<k>.npz files instead (see the module docstring)")
            # the primary HDU is [Ldet, S, a_out] raveled (a_out = 19 / 24 / 24 / 27 for channels 1-4); the model's
            # channel output is [S, Ldet, a_out] per pointing
            ndata = np.asarray(data).reshape(n_det, n_slit, -1).transpose(1, 0, 2)
            data_dict['data'][chan].append(ndata)
            data_dict['target'][chan].append((ra, dec))
            data_dict['rotation'][chan] = pa
    return data_dict


def create_instruments(data_dict, list_chan=LIST_CHAN):
    """One IFU per band with the constants of main_fusion.py:107-136 (held in surfh_amd.synth.BANDS)."""
    return {chan: synth.band_ifu(chan, angle=-data_dict['rotation'][chan]) for chan in list_chan}


def create_model(sotf, templates, origin_alpha_axis, origin_beta_axis, wavel_axis, instruments, step_angle, data_dict,
                 device=0):
    """main_fusion.py:138-158: pointings from the FITS targets, axes recentred on the third 2A pointing."""
    main_pointing = instru.Coord(0, 0)
    pointings = []
    for chan in instruments.keys():
        pointing_chan = [main_pointing + instru.Coord(ra, dec) for ra, dec in data_dict['target'][chan]]
        pointings.append(instru.CoordList(pointing_chan).pix(step_angle))
    ref = data_dict['target']['2a'][2] if len(data_dict['target'].get('2a', [])) > 2 else (0.0, 0.0)
    return spectroSigRLSCT(sotf=sotf, templates=templates, alpha_axis=origin_alpha_axis + ref[0],
                           beta_axis=origin_beta_axis + ref[1], wavelength_axis=wavel_axis,
                           instrs=list(instruments.values()), step_degree=step_angle, pointings=pointings, device=device)


def result_dir_name(method, n_channels, n_templates, niter, hyper_parameter, scale_data, delta=None, voxel=False, weighted=False,
                    data_delta=None, potential='huber', data_potential='huber', spec_potential='huber', imager=0, samples=0,
                    refine=0, nonneg=False, coupling='none'):
    """main_fusion.py:182; with a Huber threshold `delta` (not in the reference) `_huber_<delta>` is appended, `_vox` for a
    voxel-wise reconstruction, `_wgt` for a run under data weights, and `_rob_<data_delta>` for a robust data term.  Another
    potential than Huber puts its name in Huber's place (`_<kind>_<delta>`, `_rob_<kind>_<data_delta>`; `_spec_<kind>` for the
    spectral prior of a voxel-wise run); with Huber the names are unchanged.  A prior coupling other than `none` appends
    `_cpl_<coupling>` behind the threshold.  `_img_<F>` follows for a run with an imager
    data term of F filters, `_po_<K>` for a run that draws K posterior samples, `_tpl_<K>` for K rounds of template refinement,
    `_nn` last for a non-negative run (--nonneg)."""
    name = f'{method}_MC_{n_channels}_MO_4_Temp_{n_templates}_nit_{str(niter)}_mu_{str("{:.2e}".format(hyper_parameter))}_SD_{scale_data}'
    if delta is not None:
        name += f'_{potential}_{delta:.2e}'
        if coupling != 'none':
            name += f'_cpl_{coupling}'
    if voxel:
        name += '_vox'
        if spec_potential != 'huber':
            name += f'_spec_{spec_potential}'
    if weighted:
        name += '_wgt'
    if data_delta is not None:
        name += f'_rob_{data_delta:g}' if data_potential == 'huber' else f'_rob_{data_potential}_{data_delta:g}'
    if imager:
        name += f'_img_{imager}'
    if samples:
        name += f'_po_{samples}'
    if refine:
        name += f'_tpl_{refine}'
    if nonneg:
        name += '_nn'
    return name + '/'


def data_weights(ndata, weights_file=None, mask_nan=False):
    """The data and their weights as the two flags ask: (ndata, None) without either; `--weights` loads `[osize]` weights
    (ValueError unless finite and >= 0); `--mask_nan` gives the samples that are not finite weight 0 and the datum 0
    (`weights_from_data`), on top of the loaded weights if both are given."""
    if not weights_file and not mask_nan:
        return ndata, None
    w = np.ones(ndata.size) if not weights_file else check_data_weights(np.load(weights_file), ndata.size).astype(np.float64)
    if mask_nan:
        ndata, keep = weights_from_data(ndata)
        w = w * keep.ravel()
    return ndata, w


def voxel_reconstruction(spectro_model, ndata, result_path, spat_reg, spat_th, spec_reg, spec_th, niter, method, scale_data,
                         weights=None, data_delta=None, potential='huber', data_potential='huber', spec_potential='huber'):
    """The cube itself by vox_reconstruction (surfh_amd/algorithms.py): res_cube.npy [Lc, N, N], and in criterion.npy the
    criterion at the start and after iterations 1, 6, 11, ... -- the trace `reconstruction_method` writes (perf_crit = 1)."""
    from surfh_amd.algorithms import vox_criterion, vox_reconstruction
    path = pathlib.Path(result_path) / result_dir_name(method, len(spectro_model.instrs), 0, niter, spat_reg, scale_data, spat_th,
                                                       voxel=True, weighted=weights is not None, data_delta=data_delta,
                                                       potential=potential, data_potential=data_potential,
                                                       spec_potential=spec_potential)
    pots = dict(spat_potential=potential, spec_potential=spec_potential, data_potential=data_potential)
    path.mkdir(parents=True, exist_ok=True)
    init = spectro_model.adjoint(ndata if weights is None else np.where(weights > 0, weights * np.where(weights > 0, ndata, 0.), 0.))
    crit = [vox_criterion(ndata, spectro_model, init, spat_reg, spat_th, spec_reg, spec_th, weights=weights, data_th=data_delta,
                          **pots)]

    def trace(it, grad_norm, x):
        if it % 5 == 1:
            crit.append(vox_criterion(ndata, spectro_model, x, spat_reg, spat_th, spec_reg, spec_th, weights=weights,
                                      data_th=data_delta, **pots))
            print(f"iteration {it}: criterion {crit[-1]:.6e}, |grad| {grad_norm[-1]:.3e}")
        return False

    res = vox_reconstruction(ndata, spectro_model, spat_reg=spat_reg, spat_th=spat_th, spec_reg=spec_reg, spec_th=spec_th, init=init,
                             max_iter=niter, callback=trace, weights=weights, data_th=data_delta, **pots)
    print(f"voxel-wise 3MG: {res.nit} iterations, criterion {crit[0]:.6e} -> {crit[-1]:.6e}")
    print(f"Results save in {path}")
    np.save(path / 'res_cube.npy', res.x.reshape(spectro_model.ishape))
    np.save(path / 'criterion.npy', np.array(crit))
    if weights is not None:
        np.save(path / 'weights.npy', weights)
    if data_delta is not None:
        np.save(path / 'robust_weights.npy', spectro_model.robust_weights)
    return res, path


def reconstruction_method(spectro_model, ndata, templates, result_path, hyper_parameter, niter, method, scale_data,
                          checkpoint_every=0, resume=None, delta=None, weights=None, data_delta=None, potential='huber',
                          data_potential='huber', imager=None, samples=0, seed=0, coupling='none'):
    """main_fusion.py:162-206: regularised least squares by CG, then the three result files.  Not in the reference:
    `checkpoint_every` > 0 writes the iterate to checkpoint.npz in the result directory every that many iterations,
    `resume` (such a file) warm-starts from it and runs the iterations that are left; `delta` replaces the quadratic
    priors by Huber potentials of that threshold (3MG only); `weights` `[osize]` weigh the samples of the data term and are
    stored beside the results as weights.npy; `data_delta` makes the data term robust (3MG only) and stores the last iterate's
    robustness weights as robust_weights.npy; `potential` / `data_potential` name the potential under `delta` / `data_delta`;
    `coupling` names the differences that share one potential under `delta` (`surfh_amd.potentials`);
    `imager` = (ImagerModel, y_im, mu_imager) adds the imager data term and stores y_im as y_imager.npy; `samples` = K > 0 (lcg
    only) draws K posterior samples under `seed` after the solve, each a CG solve of `niter` iterations for its deviation from res_x, and
    stores their mean, per-pixel standard deviation and covariance [T, T, N, N] as res_mean.npy, res_std.npy and res_cov.npy."""
    value_init = 0
    path = pathlib.Path(result_path) / result_dir_name(method, len(spectro_model.instrs), templates.shape[0], niter,
                                                       hyper_parameter, scale_data, delta, weighted=weights is not None,
                                                       data_delta=data_delta, potential=potential, data_potential=data_potential,
                                                       imager=imager[0].oshape[0] if imager else 0, samples=samples,
                                                       coupling=coupling)
    path.mkdir(parents=True, exist_ok=True)
    im_kw = dict(model_imager=imager[0], y_imager=imager[1], mu_imager=imager[2]) if imager else {}
    crit = QuadCriterion_MRS(mu_spectro=1, y_spectro=np.copy(ndata), model_spectro=spectro_model,
                             mu_reg=hyper_parameter, printing=True, gradient="separated", delta=delta, weights=weights,
                             data_delta=data_delta, potential=potential, data_potential=data_potential, coupling=coupling,
                             **im_kw)
    if resume:
        from surfh_amd.fusion import load_checkpoint
        x_saved, it_done, _ = load_checkpoint(resume)
        value_init = np.asarray(x_saved, dtype=np.float64).reshape(crit.shape_of_output)
        print(f"Resuming from {resume}: {it_done} iterations done, {max(niter - it_done, 0)} to go")
        niter = max(niter - it_done, 0)
    ck = (path / 'checkpoint.npz', checkpoint_every) if checkpoint_every and checkpoint_every > 0 else None
    res = crit.run_method(method, niter, perf_crit=1, calc_crit=True, value_init=value_init, checkpoint=ck)
    y_cube = spectro_model.mapsToCube(res.x)
    print(f"Results save in {path}")
    np.save(path / 'res_x.npy', res.x)
    np.save(path / 'res_cube.npy', y_cube)
    np.save(path / 'criterion.npy', crit.L_crit_val)
    if weights is not None:
        np.save(path / 'weights.npy', weights)
    if data_delta is not None:
        np.save(path / 'robust_weights.npy', spectro_model.robust_weights)
    if imager:
        np.save(path / 'y_imager.npy', imager[1])
    if samples:
        po = crit.sample(n_samples=samples, seed=seed, maximum_iterations=niter, value_init=value_init)
        print(f"{samples} posterior samples: worst final r.r {po.rr_worst:.3e} (unperturbed solve: {po.grad_norm[0]:.3e} -> "
              f"{po.grad_norm[-1]:.3e}); the standard deviation is a lower bound where the solves have not converged")
        np.save(path / 'res_mean.npy', po.mean)
        np.save(path / 'res_std.npy', po.std)
        np.save(path / 'res_cov.npy', po.cov)
    return res, path


def template_refinement(spectro_model, ndata, templates, result_path, hyper_parameter, niter, method, scale_data, rounds, mu_spec,
                        tpl_iter, weights=None, nonneg=False, rho=None, inner=10):
    """`rounds` rounds of (`niter` CG iterations on the maps, `tpl_iter` on the spectra) by surfh_amd.fusion.refine_templates, data
    weight 1: res_x.npy (maps), res_templates.npy and templates_start.npy [T, Lc], and in criterion.npy the joint criterion at the
    start and after every half-step.  Features narrower than the detector's wavelength sampling stay what the start had.
    `nonneg`: both half-steps under their constraint (`niter` / `tpl_iter` outer iterations of `inner` CG iterations, penalty `rho`
    or the estimate); the criterion trace may then rise between entries."""
    from surfh_amd.fusion import refine_templates
    path = pathlib.Path(result_path) / result_dir_name(method, len(spectro_model.instrs), templates.shape[0], niter, hyper_parameter,
                                                       scale_data, weighted=weights is not None, refine=rounds, nonneg=nonneg)
    path.mkdir(parents=True, exist_ok=True)
    res = refine_templates(spectro_model, ndata, 1., hyper_parameter, mu_spec, rounds, niter, tpl_iter, weights=weights,
                           **(dict(nonneg=True, rho=rho, inner=inner) if nonneg else {}))
    for k, j in enumerate(res.criterion):
        print(f"half-step {k}: joint criterion {j:.6e}")
    print(f"Results save in {path}")
    np.save(path / 'res_x.npy', res.x)
    np.save(path / 'res_templates.npy', res.templates)
    np.save(path / 'templates_start.npy', res.templates_start)
    np.save(path / 'criterion.npy', res.criterion)
    if weights is not None:
        np.save(path / 'weights.npy', weights)
    return res, path


def nonneg_reconstruction(spectro_model, ndata, templates, result_path, hyper_parameter, outer, inner, rho, method, scale_data,
                          weights=None):
    """The maps under x >= 0 by `cg_nonneg` (surfh_amd/nonneg.py), data weight 1, from zero: res_x.npy, res_cube.npy, and in
    nn_trace.npy one row per outer iteration (and one for the start): |x - z|, rho |z - z_previous|, |r|, #{z == 0}."""
    path = pathlib.Path(result_path) / result_dir_name(method, len(spectro_model.instrs), templates.shape[0], outer, hyper_parameter,
                                                       scale_data, weighted=weights is not None, nonneg=True)
    path.mkdir(parents=True, exist_ok=True)
    res = spectro_model.cg_nonneg(ndata, mu=1., mu_reg=hyper_parameter, rho=rho, outer=outer, inner=inner, weights=weights)
    print(f"non-negative lcg: rho {res.rho:.3e}, {res.nit} outer iterations of {inner}; primal {res.primal[-1]:.3e}, dual "
          f"{res.dual[-1]:.3e}, {res.n_active[-1]} of {res.x.size} entries at zero")
    print(f"Results save in {path}")
    np.save(path / 'res_x.npy', res.x)
    np.save(path / 'res_cube.npy', spectro_model.mapsToCube(res.x))
    np.save(path / 'nn_trace.npy', np.stack([res.primal, res.dual, res.grad_norm, res.n_active.astype(np.float64)], axis=1))
    if weights is not None:
        np.save(path / 'weights.npy', weights)
    return res, path


def synthetic_problem(name, npix):
    """One of the benchmark problems + simulated data  y = A maps + noise  (SURVEY.md 8d)."""
    if name == 'small':
        prob = synth.problem(['2a'], 256, (7.41, 8.87), n_pix=npix)
    elif name in ('config2', 'config3', 'config4'):
        prob = getattr(synth, name)(n_pix=npix)
    else:
        raise click.BadParameter(f"unknown synthetic problem {name!r} (small, config2, config3, config4)")
    return prob


@click.command()
@click.option('-fd', '--fusion_dir', default='/home/nmonnier/Data/JWST/Orion_bar/Fusion/', type=str, help='Fusion directory')
@click.option('-np', '--npix', default=501, type=int, help='Number of pixels')
@click.option('-hp', '--hyper_parameter', default=1., type=float, help='Hyperparameter value')
@click.option('-ni', '--niter', default=5, type=int, help='Number of iteration.')
@click.option('-nt', '--n_templates', default=4, type=int, help='Number of Templates.')
@click.option('-sd', '--scale_data', default=False, type=bool, help='Scale data from Jy  to Jy/str.')
@click.option('-m', '--method', default='lcg', type=str, help='Method used (default = lcg).')
@click.option('-v', '--verbose', default=True, type=bool, help='Verbose.')
@click.option('--synthetic', default=None, type=str,
              help='Run on a synthetic benchmark problem (small, config2, config3, config4) instead of fusion_dir inputs; '
                   'results go to <fusion_dir>/Results/.')
@click.option('--device', default=0, type=int, help='GPU index.')
@click.option('--checkpoint_every', default=0, type=int, help='Write the iterate to checkpoint.npz every that many iterations (0: never).')
@click.option('--resume', default=None, type=str, help='checkpoint.npz of an interrupted run to warm-start from.')
@click.option('--delta', default=None, type=float,
              help='Huber threshold of the spatial priors (edge-preserving; needs --method mmmg). Default: quadratic priors.')
@click.option('--voxel', is_flag=True, default=False,
              help='Reconstruct the cube itself, without templates (needs --method mmmg): -hp and --delta weigh and threshold the '
                   'spatial differences (--delta defaults to 1), --spec_reg and --spec_delta the spectral ones.')
@click.option('--spec_reg', default=1., type=float, help='Weight of the spectral Huber prior (--voxel).')
@click.option('--spec_delta', default=1., type=float, help='Huber threshold of the spectral differences (--voxel).')
@click.option('--weights', 'weights_file', default=None, type=str,
              help='.npy file of per-sample data weights [osize] (inverse variance, 0/1 mask), finite and >= 0.')
@click.option('--mask_nan', is_flag=True, default=False, help='Give the data samples that are NaN or Inf weight 0.')
@click.option('--data_delta', default=None, type=float,
              help='Huber threshold of a robust data term, in units of the weighted residual (sigmas under inverse-variance '
                   'weights); needs --method mmmg. Default: quadratic data term.')
@click.option('--potential', default='huber', type=click.Choice(POTENTIALS),
              help='Potential of the spatial priors under --delta (needs --method mmmg and --delta).')
@click.option('--data_potential', default='huber', type=click.Choice(POTENTIALS),
              help='Potential of the robust data term under --data_delta (needs --method mmmg and --data_delta).')
@click.option('--spec_potential', default='huber', type=click.Choice(POTENTIALS),
              help='Potential of the spectral prior under --spec_delta (--voxel).')
@click.option('--coupling', default='none', type=click.Choice(COUPLINGS),
              help='Differences that share one potential under --delta: none (each its own), isotropic (row and column of a '
                   'pixel) or vector (those of all maps at a pixel); needs --method mmmg and --delta, not with --voxel. --delta is '
                   'then the threshold on the group magnitude.')
@click.option('--imager', 'imager_filters', default=0, type=int,
              help='Add the data term of a synthetic imager with that many Gaussian filters tiling the wavelength axis (1..16; '
                   'needs --synthetic). Default: none.')
@click.option('--mu_imager', default=1., type=float, help='Weight of the imager data term (--imager).')
@click.option('--imager_decim', default=1, type=int, help='Cube pixels per imager pixel along each axis (--imager).')
@click.option('--samples', default=0, type=int,
              help='Draw that many posterior samples after the solve (needs --method lcg; at least 2) and store their mean, '
                   'standard deviation and covariance per pixel. Default: none.')
@click.option('--seed', default=None, type=int, help='Seed of the posterior samples (--samples). Default: 0.')
@click.option('--refine_templates', 'refine_rounds', default=0, type=int,
              help='Refine the templates too: that many rounds of (-ni CG iterations on the maps, --tpl_iter on the spectra); '
                   'needs --method lcg. Default: the templates stay as given.')
@click.option('--mu_spec', default=None, type=float, help='Weight of the first-difference prior along the wavelength of the spectra '
                                                          '(--refine_templates). Default: 0.')
@click.option('--tpl_iter', default=None, type=int, help='CG iterations of a template half-step (--refine_templates). Default: 10.')
@click.option('--nonneg', is_flag=True, default=False,
              help='Keep the maps non-negative (ADMM around the CG; needs --method lcg), and with --refine_templates the spectra too: '
                   '-ni and --tpl_iter then count outer iterations. Results go to a directory ending in _nn.')
@click.option('--rho', default=None, type=float, help='ADMM penalty (--nonneg). Default: estimated, the mean eigenvalue of the operator.')
@click.option('--outer', default=None, type=int, help='Outer iterations (--nonneg without --refine_templates). Default: -ni.')
@click.option('--inner', default=None, type=int, help='CG iterations per outer iteration (--nonneg). Default: 10.')
def main(fusion_dir, npix, hyper_parameter, niter, n_templates, scale_data, method, verbose, synthetic, device, checkpoint_every=0,
         resume=None, delta=None, voxel=False, spec_reg=1., spec_delta=1., weights_file=None, mask_nan=False, data_delta=None,
         potential='huber', data_potential='huber', spec_potential='huber', imager_filters=0, mu_imager=1., imager_decim=1,
         samples=0, seed=None, refine_rounds=0, mu_spec=None, tpl_iter=None, nonneg=False, rho=None, outer=None, inner=None,
         coupling='none'):
    if nonneg:
        if method != 'lcg':
            raise click.UsageError('--nonneg runs ADMM around the linear CG; use it with --method lcg')
        if voxel or imager_filters or samples or delta is not None or data_delta is not None or checkpoint_every or resume:
            raise click.UsageError('--nonneg constrains the quadratic criterion on the maps (and the spectra) alone: no --voxel, '
                                   '--imager, --samples, --delta, --data_delta or checkpoints')
        if rho is not None and not (rho > 0 and np.isfinite(rho)):
            raise click.BadParameter(f'must be finite and > 0, not {rho}', param_hint='--rho')
        if inner is not None and inner < 1:
            raise click.BadParameter(f'at least one CG iteration, not {inner}', param_hint='--inner')
        if outer is not None and refine_rounds:
            raise click.UsageError('--outer: with --refine_templates, -ni and --tpl_iter count the outer iterations')
        if outer is not None and outer < 1:
            raise click.BadParameter(f'at least one outer iteration, not {outer}', param_hint='--outer')
    elif rho is not None or outer is not None or inner is not None:
        raise click.UsageError('--rho, --outer and --inner belong to --nonneg')
    if refine_rounds:
        if refine_rounds < 1:
            raise click.BadParameter(f'at least one round, not {refine_rounds}', param_hint='--refine_templates')
        if method != 'lcg':
            raise click.UsageError('--refine_templates alternates two linear CG solves; use it with --method lcg')
        if voxel or imager_filters or samples or delta is not None or data_delta is not None or checkpoint_every or resume:
            raise click.UsageError('--refine_templates runs the quadratic criterion on the maps and the spectra alone: no --voxel, '
                                   '--imager, --samples, --delta, --data_delta or checkpoints')
        if mu_spec is not None and not (mu_spec >= 0 and np.isfinite(mu_spec)):
            raise click.BadParameter(f'must be finite and >= 0, not {mu_spec}', param_hint='--mu_spec')
        if tpl_iter is not None and tpl_iter < 1:
            raise click.BadParameter(f'at least one iteration, not {tpl_iter}', param_hint='--tpl_iter')
    elif mu_spec is not None or tpl_iter is not None:
        raise click.UsageError('--mu_spec and --tpl_iter belong to --refine_templates')
    if samples:
        if method != 'lcg':
            raise click.UsageError('--samples draws from the Gaussian posterior of the quadratic criterion; use it with --method lcg')
        if samples < 2:
            raise click.BadParameter(f'a covariance needs at least 2 samples, not {samples}', param_hint='--samples')
        if voxel or imager_filters:
            raise click.UsageError('--samples: the sampler carries neither the voxel-wise solver (--voxel) nor the imager data term (--imager)')
        if seed is not None and seed < 0:
            raise click.BadParameter(f'must be >= 0, not {seed}', param_hint='--seed')
    elif seed is not None:
        raise click.UsageError('--seed belongs to --samples')
    if imager_filters:
        if not 1 <= imager_filters <= 16:
            raise click.BadParameter(f'1 to 16 filters, not {imager_filters}', param_hint='--imager')
        if data_delta is not None:
            raise click.UsageError('--imager: the robust data term (--data_delta) does not carry the imager data term')
        if voxel:
            raise click.UsageError('--imager: the voxel-wise solver (--voxel) does not carry the imager data term')
        if not synthetic:
            raise click.UsageError('--imager simulates the imager data: use it with --synthetic')
        if not (mu_imager >= 0 and np.isfinite(mu_imager)):
            raise click.BadParameter(f'must be finite and >= 0, not {mu_imager}', param_hint='--mu_imager')
        if not 1 <= imager_decim <= npix:
            raise click.BadParameter(f'must be in 1..{npix}, not {imager_decim}', param_hint='--imager_decim')
    elif mu_imager != 1. or imager_decim != 1:
        raise click.UsageError('--mu_imager and --imager_decim belong to --imager')
    if (potential != 'huber' or data_potential != 'huber') and method != 'mmmg':
        raise click.UsageError('--potential and --data_potential choose a non-quadratic term; use them with --method mmmg')
    if coupling != 'none':
        if method != 'mmmg':
            raise click.UsageError('--coupling groups the differences of a non-quadratic prior; use it with --method mmmg and --delta')
        if voxel:
            raise click.UsageError('--coupling acts on the maps: the voxel-wise solver (--voxel) does not carry it')
        if delta is None:
            raise click.UsageError('--coupling needs --delta: a coupling of the quadratic prior means nothing')
    if potential != 'huber' and delta is None and not voxel:
        raise click.UsageError('--potential needs --delta: a potential of the quadratic prior means nothing')
    if data_potential != 'huber' and data_delta is None:
        raise click.UsageError('--data_potential needs --data_delta: a potential of the quadratic data term means nothing')
    if spec_potential != 'huber' and not voxel:
        raise click.UsageError('--spec_potential is the potential of the spectral prior of a voxel-wise run; use it with --voxel')
    if data_delta is not None and method != 'mmmg':
        raise click.UsageError('--data_delta (robust data term) is not quadratic; use it with --method mmmg')
    if data_delta is not None and not data_delta > 0:
        raise click.BadParameter(f'must be positive, not {data_delta}', param_hint='--data_delta')
    if voxel and method == 'lcg':
        raise click.BadParameter('the voxel-wise criterion is not quadratic; use --method mmmg with --voxel', param_hint='--voxel')
    if voxel and not spec_delta > 0:
        raise click.BadParameter(f'must be positive, not {spec_delta}', param_hint='--spec_delta')
    if voxel and (checkpoint_every or resume):
        raise click.BadParameter('checkpoints are not written for voxel-wise runs', param_hint='--voxel')
    if delta is not None and method == 'lcg':
        raise click.BadParameter('lcg minimises quadratic criteria only; use --method mmmg with --delta', param_hint='--delta')
    if delta is not None and not delta > 0:
        raise click.BadParameter(f'must be positive, not {delta}', param_hint='--delta')
    print('options:', dict(fusion_dir=fusion_dir, npix=npix, hyper_parameter=hyper_parameter, niter=niter,
                           n_templates=n_templates, scale_data=scale_data, method=method, synthetic=synthetic, device=device,
                           delta=delta))
    if verbose:
        log.basicConfig(format="%(levelname)s: %(message)s", level=log.INFO)

    log.info('Initialize basic path parameters')
    paths, step, step_angle = initialize_parameters(fusion_dir)

    if synthetic:
        log.info(f'Build the synthetic problem {synthetic}')
        prob = synthetic_problem(synthetic, npix)
        templates = None if voxel else prob['templates']
        truth = np.tensordot(prob['templates'].T, prob['maps'], 1) if voxel else prob['maps']      # cube = sum_t tpl[t] maps[t]
        model = spectroSigRLSCT(prob['sotf'], templates, prob['alpha_axis'], prob['beta_axis'], prob['wavel'],
                                prob['ifus'], prob['step_deg'], prob['pointings'], device=device)
        y = model.forward(truth)
        rng = np.random.default_rng(1)               # the run's noise seed: the spectrometer's draw first, then the imager's
        ndata = y + rng.standard_normal(y.shape) * 1e-2 * np.sqrt(np.mean(y ** 2))
        imager = None
        if imager_filters:
            from surfh_amd.imager import ImagerModel, synthetic_filters
            im_model = ImagerModel(model, synthetic_filters(prob['wavel'], imager_filters), decim=imager_decim)
            model.set_imager(im_model)
            y_im = im_model.forward(truth)
            imager = (im_model, y_im + rng.standard_normal(y_im.shape) * 1e-2 * np.sqrt(np.mean(y_im ** 2)), mu_imager)
    else:
        log.info('Load simulation data')
        origin_alpha_axis, origin_beta_axis, wavel_axis, templates, sotf = load_simulation_data(paths, step, step_angle, npix, n_templates,
                                                                                                with_templates=not voxel)
        log.info('Load MRS data')
        data_dict = load_data(LIST_CHAN, paths["save_filter_corrected_dir"])
        log.info('Create instruments and spectro models')
        instruments = create_instruments(data_dict)
        model = create_model(sotf, templates, origin_alpha_axis, origin_beta_axis, wavel_axis, instruments, step_angle,
                             data_dict, device=device)
        ndata = np.concatenate([np.array(data_dict['data'][chan]).ravel() for chan in LIST_CHAN])

    try:
        ndata, weights = data_weights(ndata, weights_file, mask_nan)
    except ValueError as e:
        raise click.BadParameter(str(e), param_hint='--weights')
    if weights is not None:
        log.info(f'Data weights: {int(np.sum(weights == 0))} of {weights.size} samples masked')

    if scale_data:
        log.info('Data scaling enable')
        ndata = model.real_data_janskySR_to_jansky(ndata)

    log.info(f'Start {method} algorithm')
    if voxel:
        voxel_reconstruction(model, ndata, paths["result_path"], hyper_parameter, 1. if delta is None else delta, spec_reg, spec_delta,
                             niter, method, scale_data, weights=weights, data_delta=data_delta, potential=potential,
                             data_potential=data_potential, spec_potential=spec_potential)
        model.close()
        return
    if refine_rounds:
        template_refinement(model, ndata, templates, paths["result_path"], hyper_parameter, niter, method, scale_data, refine_rounds,
                            mu_spec or 0., tpl_iter or 10, weights=weights, nonneg=nonneg, rho=rho, inner=inner or 10)
        model.close()
        return
    if nonneg:
        nonneg_reconstruction(model, ndata, templates, paths["result_path"], hyper_parameter, outer or niter, inner or 10, rho, method,
                              scale_data, weights=weights)
        model.close()
        return
    reconstruction_method(model, ndata, templates, paths["result_path"], hyper_parameter, niter, method, scale_data,
                          checkpoint_every=checkpoint_every, resume=resume, delta=delta, weights=weights, data_delta=data_delta,
                          potential=potential, data_potential=data_potential, imager=imager if synthetic else None, samples=samples,
                          coupling=coupling,
                          seed=seed or 0)
    model.close()


if __name__ == '__main__':
    main()
