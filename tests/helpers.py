"""Build the product model (surfh_amd) from a tests/problems.py config."""
import numpy as np

from surfh_amd import instru
from surfh_amd.models import spectroSigRLSCT


def make_ifu(spec):
    return instru.IFU(fov=instru.FOV(spec.alpha_width, spec.beta_width,
                                     origin=instru.Coord(spec.origin[0], spec.origin[1]), angle=spec.angle),
                      det_pix_size=spec.det_pix_size, n_slit=spec.n_slit,
                      w_blur=instru.SpectralBlur(spec.grating_resolution), pce=None,
                      wavel_axis=spec.wavel_axis, name=spec.name)


def make_pointings(cfg):
    return [instru.CoordList([instru.Coord(a, b) for a, b in pts]) for pts in cfg["pointings"]]


def build_model(cfg, **kw):
    return spectroSigRLSCT(cfg["sotf"], cfg["templates"], cfg["alpha_axis"], cfg["beta_axis"], cfg["wavel"],
                           [make_ifu(s) for s in cfg["specs"]], cfg["step_deg"], make_pointings(cfg), **kw)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) /
                 np.linalg.norm(np.asarray(b, dtype=np.float64)))


# ---- local error measures: what the whole-array figure above averages away (tests/test_local_metrics_host.py) -------------
TOL = 1e-5                   # the project's parity gate; every local measure is held to it as well


def max_err(a, ref):
    """max |a - ref| / max |ref|: the worst element against the array's largest value."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


def slice_err(a, ref, axis):
    """The worst slice along ``axis`` (one axis or a tuple of axes, whose index combinations are the slices) and its index:
    |a_s - ref_s| / max(|ref_s|, |ref| sqrt(n_s / n)), L2 norms.  The floor is the array's average slice norm: a slice that is
    almost empty (a map row outside every field of view) is judged against the array's scale, so no slice is left out."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    axes = tuple(ax % ref.ndim for ax in ((axis,) if np.isscalar(axis) else axis))
    lead = tuple(ref.shape[ax] for ax in axes)
    d = np.moveaxis(a - ref, axes, range(len(axes))).reshape(int(np.prod(lead)), -1)
    r = np.moveaxis(ref, axes, range(len(axes))).reshape(d.shape)
    floor = np.linalg.norm(r) * np.sqrt(r.shape[1] / r.size)
    e = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(r, axis=1), floor)
    k = int(np.argmax(e))
    idx = tuple(int(i) for i in np.unravel_index(k, lead))
    return float(e[k]), (idx[0] if np.isscalar(axis) else idx)


def local_errs(a, ref, axes):
    """{"rel", "max", and for every name in ``axes`` (name -> axis or tuple of axes) the worst slice "<name>" and its index
    "<name>_at"}."""
    out = dict(rel=rel(a, ref), max=max_err(a, ref))
    for name, ax in axes.items():
        out[name], out[name + "_at"] = slice_err(a, ref, ax)
    return out
