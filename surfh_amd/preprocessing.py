"""Distortion correction of MRS detector exposures (surfh/Preprocessing/distorsion_correction.py and the slit order of
scripts/correction_mrs_data.py:149-192): label the slits on the detector, sort them by centroid, and resample each slit's
scattered (alpha, lambda, intensity) samples onto the channel's regular lambda x alpha_out grid with the exponential
modified-Shepard kernel (surfh/ToolsDir/shepard_interpolation.pyx:78-141).  The output, [n_slit, L, n_alpha_out], is what
``Channel.realData_sliceToCube`` takes.

The resampling runs on the GPU (``surfh_shepard`` in include/surfh_amd.h): every slit of an exposure in one launch, a cell
list in place of the reference's all-pairs loop, and the reference's float32 arithmetic, so that each sample is used or
left out exactly as the reference decides.  Labelling and sorting are host-side NumPy / SciPy."""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import _lib

__all__ = ["exponential_modified_shepard", "shepard_segments", "generate_label_image", "sort_labels_by_centroid",
           "mrs_slices_distrorsion_correction", "reorder_corrected_slices", "slices_to_payload", "SLIT_ORDER"]


def _inv_res(res) -> np.float32:
    """The reference's ``inv = 1 / res``: res arrives as a C float, 1.0 / res is a double division stored as float."""
    return np.float32(1.0 / np.float64(np.float32(res)))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel())


def shepard_segments(segments, p: float = 2.0, alpha: float = 2.0, pixel_cutoff: float = 1.0, epsilon: float = 1e-6,
                     separable: bool = True, neighbours: bool = False, timing: bool = False):
    """Resample several independent segments in one GPU launch.

    ``segments``: a sequence of ``(alpha_coord, lambda_coord, values, q_alpha, q_lambda, alpha_res, lambda_res)``.  With
    ``separable`` the query points of a segment are the grid ``np.meshgrid(q_alpha, q_lambda)`` (output
    [len(q_lambda), len(q_alpha)]); otherwise ``q_alpha`` / ``q_lambda`` are explicit coordinates of one shape, which
    is the output's shape.  Every coordinate is cast to float32, as the reference does.

    Returns the list of float32 outputs, then (if asked) the list of per-point neighbour counts and the device time in
    milliseconds of the kernels."""
    L = _lib.load()
    segs = list(segments)
    if not segs:
        raise ValueError("no segment")
    pa, pl, pv, qa, ql, shapes = [], [], [], [], [], []
    n_pt = np.zeros(len(segs) + 1, dtype=np.int64)
    na = np.zeros(len(segs), dtype=np.int32)
    nl = np.zeros(len(segs), dtype=np.int32)
    ia = np.zeros(len(segs), dtype=np.float32)
    il = np.zeros(len(segs), dtype=np.float32)
    for s, (a, l, v, ga, gl, ares, lres) in enumerate(segs):
        a, l, v = _f32(a), _f32(l), _f32(v)
        if not (a.size == l.size == v.size):
            raise ValueError(f"segment {s}: alpha / lambda / values sizes differ ({a.size}, {l.size}, {v.size})")
        if separable:
            ga, gl = _f32(ga), _f32(gl)
            shapes.append((gl.size, ga.size))
            nl[s], na[s] = gl.size, ga.size
        else:
            ga_, gl_ = np.asarray(ga), np.asarray(gl)
            if ga_.shape != gl_.shape:
                raise ValueError(f"segment {s}: query meshes differ in shape ({ga_.shape} vs {gl_.shape})")
            shapes.append(ga_.shape)
            ga, gl = _f32(ga_), _f32(gl_)
            na[s], nl[s] = ga.size, 1
        pa.append(a); pl.append(l); pv.append(v); qa.append(ga); ql.append(gl)
        n_pt[s + 1] = n_pt[s] + a.size
        ia[s], il[s] = _inv_res(ares), _inv_res(lres)
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros(0, np.float32)  # noqa: E731
    pa, pl, pv, qa, ql = cat(pa), cat(pl), cat(pv), cat(qa), cat(ql)
    n_out = int(np.sum(na.astype(np.int64) * nl))
    out = np.zeros(max(n_out, 1), dtype=np.float32)
    nbr = np.zeros(max(n_out, 1), dtype=np.int32) if neighbours else None
    ms = C.c_float(0.0)
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.surfh_shepard(len(segs), n_pt.ctypes.data_as(C.POINTER(C.c_int64)), vp(pa), vp(pl), vp(pv),
                         na.ctypes.data_as(_lib.c_int32_p), nl.ctypes.data_as(_lib.c_int32_p), 1 if separable else 0,
                         vp(qa), vp(ql), _lib.fptr(ia), _lib.fptr(il), float(p), float(alpha), float(pixel_cutoff),
                         float(epsilon), vp(out), vp(nbr), 0, None, C.byref(ms) if timing else None)
    if rc != 0:
        raise RuntimeError(L.surfh_shepard_last_error().decode("utf-8", "replace"))
    res, cnt, o = [], [], 0
    for shp in shapes:
        n = int(np.prod(shp))
        res.append(out[o:o + n].reshape(shp).copy())
        if neighbours:
            cnt.append(nbr[o:o + n].reshape(shp).copy())
        o += n
    ret = (res,)
    if neighbours:
        ret += (cnt,)
    if timing:
        ret += (float(ms.value),)
    return ret if len(ret) > 1 else res


def exponential_modified_shepard(alpha_coord, lambda_coord, values, alpha_mesh, lambda_mesh, p=2., alpha=2.0,
                                 pixel_cutoff=1, alpha_res=1.0, lambda_res=1.0, epsilon=1e-6, return_neighbours=False):
    """shepard_interpolation.pyx:78-141 on the GPU: the interpolated values at every point of the (arbitrary, same-shape)
    2-D meshes, float32.  With ``return_neighbours`` also the number of samples within the cutoff of each point."""
    am, lm = np.asarray(alpha_mesh), np.asarray(lambda_mesh)
    if am.ndim != 2 or am.shape != lm.shape:
        raise ValueError(f"alpha_mesh and lambda_mesh must be 2-D arrays of one shape ({am.shape} vs {lm.shape})")
    r = shepard_segments([(alpha_coord, lambda_coord, values, am, lm, alpha_res, lambda_res)], p=p, alpha=alpha,
                         pixel_cutoff=pixel_cutoff, epsilon=epsilon, separable=False, neighbours=return_neighbours)
    if return_neighbours:
        return r[0][0], r[1][0]
    return r[0]


def generate_label_image(binary_grid) -> np.ndarray:
    """Connected components of the non-zero pixels (distorsion_correction.py:26-33, ``skimage.measure.label``): full
    8-connectivity, background 0, labels 1..n in raster order of their first pixel."""
    from scipy import ndimage
    lab, _ = ndimage.label(np.asarray(binary_grid) != 0, structure=np.ones((3, 3), dtype=bool))
    return lab.astype(np.int64)


def sort_labels_by_centroid(label_image) -> np.ndarray:
    """Renumber the labels 1..n by the column of their centroid (distorsion_correction.py:36-52)."""
    lab = np.asarray(label_image)
    n = int(lab.max()) if lab.size else 0
    if n < 1:
        return np.zeros_like(lab)
    flat = np.clip(lab, 0, None).ravel()
    cols = np.broadcast_to(np.arange(lab.shape[1], dtype=np.float64), lab.shape).ravel()
    with np.errstate(invalid="ignore", divide="ignore"):     # the column of scipy.ndimage.center_of_mass(lab, lab, 1..n)
        centroid_col = np.bincount(flat, cols, n + 1)[1:] / np.bincount(flat, None, n + 1)[1:]
    sorted_labels = np.argsort(centroid_col) + 1
    lut = np.zeros(n + 1, dtype=lab.dtype)
    lut[sorted_labels] = np.arange(1, n + 1, dtype=lab.dtype)
    return lut[lab]


def mrs_slices_distrorsion_correction(model_channel, sorted_labeled_image, detector2world, data, chan_wavelength, mode,
                                      recenter: bool = False, return_info: bool = False):
    """distorsion_correction.py:108-178: one slit per label 1..n-1 of ``sorted_labeled_image`` resampled onto
    lambda = ``chan_wavelength`` x ``model_channel.oshape[-1]`` alpha points spanning the slit; returns
    ``[oshape[1], L, oshape[-1]]`` (float64, zero where no slit was written).

    ``detector2world``: ``f(columns, rows) -> (alpha, beta, lam)`` as in the reference, or a tuple of precomputed
    ``(alpha, beta, lam)`` arrays in detector layout.  ``mode`` 0 skips a slit that reaches beyond
    ``max(chan_wavelength) + 1``, mode 1 one that reaches below ``min(chan_wavelength) - 1``; a skipped slit takes no
    output row.  Samples whose intensity is NaN are dropped, but the alpha grid spans all of the slit's pixels.  As the
    reference, every coordinate goes to the kernel in float32 (absolute sky coordinates included); ``recenter=True``
    subtracts each slit's alpha-grid centre in float64 first, which the reference does not do.

    With ``return_info`` also a dict: ``labels`` (the labels written, in output order), ``skipped`` (labels skipped)
    and ``kernel_ms`` (device time of the resampling)."""
    lab = np.asarray(sorted_labeled_image)
    data = np.asarray(data)
    if lab.ndim != 2 or data.shape != lab.shape:
        raise ValueError(f"data {data.shape} and label image {lab.shape} must be 2-D arrays of one shape")
    oshape = tuple(int(v) for v in model_channel.oshape)
    n_slit, n_lam, n_alpha = oshape[-3], oshape[-2], oshape[-1]
    cw = np.asarray(chan_wavelength, dtype=np.float64).ravel()
    if cw.size != n_lam:
        raise ValueError(f"chan_wavelength has {cw.size} samples, the channel's slices {n_lam}")
    if callable(detector2world):
        world = detector2world
    else:
        try:
            tab = [np.asarray(t) for t in detector2world]
        except TypeError:
            raise ValueError("detector2world must be a callable or an (alpha, beta, lam) tuple of arrays") from None
        if len(tab) != 3 or any(t.shape != lab.shape for t in tab):
            raise ValueError(f"detector2world arrays must be (alpha, beta, lam) of the label image's shape {lab.shape}")

        def world(cols, rows):
            return tuple(t[rows, cols] for t in tab)

    # pixels of every label, in the raster order of np.where(labels == slit)
    flat = lab.ravel()
    order = np.argsort(flat, kind="stable")
    bounds = np.searchsorted(flat[order], np.arange(flat.max() + 2 if flat.size else 1))
    n_labels = len(np.unique(lab))
    segs, used, skipped = [], [], []
    for slit in range(1, n_labels):
        pix = order[bounds[slit]:bounds[slit + 1]] if slit + 1 < len(bounds) else order[:0]
        rows, cols = np.divmod(pix, lab.shape[1])
        alpha, _, lam = (np.asarray(t, dtype=np.float64) for t in world(cols, rows))
        if mode == 0 and np.any(lam > np.max(cw) + 1):
            skipped.append(slit)
            continue
        if mode == 1 and np.any(lam < np.min(cw) - 1):
            skipped.append(slit)
            continue
        if len(used) >= n_slit:
            raise ValueError(f"more slits on the detector than the channel's {n_slit} (label {slit})")
        intensity = data[rows, cols]
        valid = ~np.isnan(intensity)
        ga = np.linspace(np.min(alpha), np.max(alpha), n_alpha)
        alpha_res = (np.max(ga) - np.min(ga)) / n_alpha
        lambda_res = (np.max(cw) - np.min(cw)) / n_lam
        av = alpha[valid]
        if recenter:
            c = 0.5 * (ga[0] + ga[-1])
            av, ga = av - c, ga - c
        segs.append((av, lam[valid], intensity[valid], ga, cw, alpha_res, lambda_res))
        used.append(slit)
    corrected = np.zeros(oshape[1:])
    ms = 0.0
    if segs:
        res, ms = shepard_segments(segs, p=2, alpha=2.0, pixel_cutoff=2, timing=True)
        for i, r in enumerate(res):
            corrected[i] = r
    if return_info:
        return corrected, {"labels": used, "skipped": skipped, "kernel_ms": ms}
    return corrected


# the reference driver's slit permutation per channel (scripts/correction_mrs_data.py:149-185): the centroid-sorted slit
# i goes to row order[i], then the rows are rolled by `roll`
SLIT_ORDER = {
    1: ([0, 11, 1, 12, 2, 13, 3, 14, 4, 15, 5, 16, 6, 17, 7, 18, 8, 19, 9, 20, 10], 10),
    2: ([8, 0, 9, 1, 10, 2, 11, 3, 12, 4, 13, 5, 14, 6, 15, 7, 16], 9),
    3: ([0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15], 0),
    4: ([0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11], 0),
}


def _channel_number(chan) -> int:
    s = str(chan).lower()
    for c in s.replace("ch", " ").split():
        if c[:1].isdigit():
            return int(c[0])
    raise ValueError(f"unknown channel {chan!r}")


def reorder_corrected_slices(slices, chan) -> np.ndarray:
    """Put centroid-sorted corrected slices into the model's slit order (scripts/correction_mrs_data.py:149-185).
    ``chan``: '1A', 'ch2-long', 3, ...  Channels 1 and 2 are rolled by 10 and 9 rows after the permutation.

    The reference's ch2 branch then also builds ``[sorted_data[:, i*24:(i+1)*24] for i in range(17)]`` (:168), a list
    that its next line (the ``transpose`` of :192) cannot take; that step is not reproduced."""
    slices = np.asarray(slices)
    order, roll = SLIT_ORDER[_channel_number(chan)]
    if slices.shape[0] > len(order):
        raise ValueError(f"{slices.shape[0]} slices for a channel of {len(order)} slits")
    out = np.zeros_like(slices)
    for i in range(slices.shape[0]):
        out[order[i]] = slices[i]
    return np.roll(out, roll, 0) if roll else out


def slices_to_payload(sorted_slices) -> np.ndarray:
    """[n_slit, L, n_alpha] -> [L, n_slit * n_alpha], the 2-D image the reference driver writes
    (scripts/correction_mrs_data.py:192)."""
    s = np.asarray(sorted_slices)
    return s.transpose(1, 0, 2).reshape(s.shape[1], s.shape[2] * s.shape[0])
