"""ctypes binding of the C ABI in include/surfh_amd.h (libsurfh_amd.so, built in-tree by
``__graft_entry__.build()``).  There is no CPU fallback: if the library is missing or a
call fails, an exception is raised."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsurfh_amd.so")

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
# int cb(void *user, int32_t it, const double *grad_norm, const float *x)   (include/surfh_amd.h:surfh_cg_callback)
CG_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, c_double_p, c_float_p)
c_uint8_p = C.POINTER(C.c_uint8)
# int cb(void *user, int32_t sample, int32_t nit, const double *rr, const float *x)   (include/surfh_amd.h:surfh_sample_callback)
SAMPLE_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, c_double_p, c_float_p)


class ChannelDesc(C.Structure):
    _fields_ = [
        ("wslice_start", C.c_int32), ("wslice_stop", C.c_int32),
        ("n_pointings", C.c_int32), ("n_slit", C.c_int32), ("n_lambda_out", C.c_int32),
        ("n_alpha_out", C.c_int32), ("srf", C.c_int32), ("na", C.c_int32), ("nb", C.c_int32),
        ("alpha0", C.c_int32), ("n_alpha_slit", C.c_int32), ("n_beta_slit", C.c_int32),
        ("slit_beta0", c_int32_p), ("slit_weights", c_double_p),
        ("grid_i0", c_int32_p), ("grid_i1", c_int32_p), ("grid_y0", c_double_p), ("grid_y1", c_double_p),
        ("wpsf", c_double_p),
        ("gt_i0", c_int32_p), ("gt_i1", c_int32_p), ("gt_y0", c_double_p), ("gt_y1", c_double_p),
        ("gt_inside", c_uint8_p),
        ("box_len", C.c_int32), ("box_shift", C.c_int32),
    ]


class Config(C.Structure):
    _fields_ = [
        ("n_alpha", C.c_int32), ("n_beta", C.c_int32), ("n_lambda", C.c_int32), ("n_templates", C.c_int32),
        ("templates", c_double_p), ("sotf", c_double_p),
        ("n_channels", C.c_int32), ("channels", C.POINTER(ChannelDesc)),
        ("device", C.c_int32), ("stream", C.c_void_p), ("split_k_forward", C.c_int32), ("verify", C.c_int32),
        ("exact", C.c_int32),
    ]


class ImagerDesc(C.Structure):
    _fields_ = [("n_filters", C.c_int32), ("filters", c_double_p), ("decim", C.c_int32), ("sotf", c_double_p)]


EXPORTS = [
    "surfh_last_error", "surfh_version", "surfh_plan_create", "surfh_plan_destroy", "surfh_isize", "surfh_osize",
    "surfh_stream", "surfh_forward", "surfh_adjoint", "surfh_adjoint_ref", "surfh_fwadj", "surfh_forward_dev",
    "surfh_adjoint_dev", "surfh_adjoint_ref_dev", "surfh_fwadj_dev", "surfh_wct_forward", "surfh_wct_adjoint",
    "surfh_wct_fwadj", "surfh_wct_expsol", "surfh_tst_create", "surfh_tst_destroy", "surfh_tst_forward",
    "surfh_tst_adjoint", "surfh_tst_fwadj", "surfh_tst_last_error", "surfh_cg", "surfh_cg_cb", "surfh_mmmg", "surfh_mmmg_huber", "surfh_huber_prior_dev", "surfh_huber_curv_dev", "surfh_mmmg_huber_vox", "surfh_huber_vox_prior_dev", "surfh_huber_vox_curv_dev", "surfh_mmmg_robust", "surfh_mmmg_robust_vox", "surfh_robust_data_dev", "surfh_robust_curv_dev", "surfh_mmmg_huber_planes", "surfh_huber_planes_prior_dev", "surfh_huber_planes_curv_dev", "surfh_cg_planes", "surfh_mmmg_planes", "surfh_cg_planes_cb", "surfh_mmmg_planes_cb", "surfh_cg_planes_begin_dev", "surfh_cg_planes_step_dev", "surfh_cg_planes_rr", "surfh_maps_to_cube", "surfh_cube_to_maps", "surfh_normal_dev",
    "surfh_prior_add_dev", "surfh_spec_supported", "surfh_spec_size", "surfh_to_spec_dev", "surfh_from_spec_dev", "surfh_forward_spec_dev",
    "surfh_adjoint_spec_dev", "surfh_normal_spec_dev", "surfh_prior_spec_add_dev", "surfh_set_prior", "surfh_set_potential", "surfh_get_potential", "surfh_set_prior_coupling", "surfh_get_prior_coupling", "surfh_set_data_weights", "surfh_set_data_weights_dev", "surfh_has_data_weights", "surfh_set_imager", "surfh_imager_osize", "surfh_imager_forward", "surfh_imager_adjoint", "surfh_imager_forward_dev", "surfh_imager_adjoint_dev", "surfh_imager_fwadj", "surfh_set_imager_data", "surfh_has_imager_term", "surfh_dot_dev", "surfh_cg_step_dev", "surfh_cg_dir_dev", "surfh_cg_iter_dev", "surfh_residual_dev",
    "surfh_randn_dev", "surfh_po_data_dev", "surfh_po_prior_dev", "surfh_po_moments", "surfh_po_rhs", "surfh_cg_sample",
    "surfh_cg_planes_sample", "surfh_po_planes_rhs", "surfh_po_planes_moments", "surfh_debug_po_planes",
    "surfh_cg_begin_dev", "surfh_cg_iter_nosync_dev", "surfh_cg_xupdate_nosync_dev", "surfh_cg_refresh_nosync_dev", "surfh_cg_trace",
    "surfh_profile_enable", "surfh_profile_filter", "surfh_profile_count", "surfh_profile_get", "surfh_profile_reset", "surfh_debug_copy",
    "surfh_debug_dims", "surfh_gemm_selftest", "surfh_gemm_selftest_ksteps", "surfh_gemm_selftest_ms", "surfh_klist_classify", "surfh_launch_geometry", "surfh_route_decide", "surfh_mm_step2",
    "surfh_debug_alloc_count", "surfh_debug_alloc_fail", "surfh_debug_prior_passes",
    "surfh_mmmg_huber_planes_ex", "surfh_huber_planes_prior_dev_ex", "surfh_huber_planes_curv_dev_ex", "surfh_debug_planes_passes",
    "surfh_debug_planes_cg", "surfh_debug_planes_normal",
    "surfh_shepard", "surfh_shepard_last_error", "surfh_spectral_median", "surfh_nmf_cd", "surfh_templates_last_error",
    "surfh_set_templates", "surfh_get_templates", "surfh_forward_templates", "surfh_adjoint_templates", "surfh_forward_templates_dev",
    "surfh_adjoint_templates_dev", "surfh_cg_templates", "surfh_cg_templates_cb", "surfh_joint_criterion",
    "surfh_cg_nonneg", "surfh_cg_templates_nonneg", "surfh_nn_project_dev", "surfh_cg_planes_nonneg", "surfh_nn_project_planes_dev",
]

_lib = None


def load():
    """Load libsurfh_amd.so and declare the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP path has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    tail = [c_float_p, C.c_int32, C.c_double, C.c_int32, c_float_p, c_double_p, c_int32_p]     # x0, max_iter, tol, refresh, x, grad_norm, nit
    admm = [c_float_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, c_float_p, c_double_p, c_int32_p]  # start, outer, inner, tol, refresh, out, trace, nit
    cb = [CG_CALLBACK, vp]                                                                       # callback, user
    L.surfh_last_error.restype = C.c_char_p
    L.surfh_version.restype = C.c_int
    L.surfh_plan_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.surfh_plan_destroy.argtypes = [vp]
    L.surfh_isize.argtypes = [vp]; L.surfh_isize.restype = C.c_int64
    L.surfh_osize.argtypes = [vp]; L.surfh_osize.restype = C.c_int64
    L.surfh_stream.argtypes = [vp]; L.surfh_stream.restype = vp
    for n in ("surfh_forward", "surfh_adjoint", "surfh_adjoint_ref", "surfh_fwadj", "surfh_wct_forward", "surfh_wct_adjoint",
              "surfh_wct_fwadj"):
        getattr(L, n).argtypes = [vp, c_float_p, c_float_p]
    for n in ("surfh_forward_dev", "surfh_adjoint_dev", "surfh_adjoint_ref_dev", "surfh_fwadj_dev"):
        getattr(L, n).argtypes = [vp, vp, vp]
    L.surfh_cg.argtypes = [vp, c_float_p, C.c_double, C.c_double] + tail
    L.surfh_tst_create.argtypes = [C.c_int32] * 4 + [c_double_p, c_int32_p, C.c_int64, c_float_p, C.c_int32, C.POINTER(vp)]
    L.surfh_tst_destroy.argtypes = [vp]
    for n in ("surfh_tst_forward", "surfh_tst_adjoint", "surfh_tst_fwadj"):
        getattr(L, n).argtypes = [vp, c_float_p, c_float_p]
    L.surfh_tst_last_error.restype = C.c_char_p
    L.surfh_wct_expsol.argtypes = [vp, c_float_p, c_double_p, c_double_p, c_float_p]
    L.surfh_cg_planes.argtypes = L.surfh_cg.argtypes
    L.surfh_cg_cb.argtypes = L.surfh_cg.argtypes + cb
    L.surfh_mmmg.argtypes = L.surfh_cg_cb.argtypes
    L.surfh_randn_dev.argtypes = [vp, vp, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.surfh_po_data_dev.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_double, vp]
    L.surfh_po_prior_dev.argtypes = [vp, vp, vp, C.c_double, vp]
    L.surfh_po_moments.argtypes = [C.c_int32, C.c_int64, c_float_p, c_float_p, C.c_int32, c_double_p, c_double_p, C.c_int32]
    L.surfh_po_rhs.argtypes = [vp, c_float_p, C.c_double, C.c_double, C.c_uint64, C.c_int32, c_float_p, c_float_p]
    L.surfh_cg_sample.argtypes = [vp, c_float_p, C.c_double, C.c_double, c_float_p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                  C.c_uint64, c_float_p, c_float_p, c_float_p, c_float_p, c_double_p, c_double_p, c_double_p,
                                  c_int32_p, c_double_p, SAMPLE_CALLBACK, vp]
    L.surfh_cg_planes_sample.argtypes = L.surfh_cg_sample.argtypes[:-3] + [c_double_p, c_double_p, SAMPLE_CALLBACK, vp]  # rr_first, rr_last
    L.surfh_po_planes_rhs.argtypes = L.surfh_po_rhs.argtypes
    L.surfh_po_planes_moments.argtypes = L.surfh_po_moments.argtypes
    L.surfh_debug_po_planes.argtypes = [vp, C.c_char_p] + [C.c_int32] * 3 + [C.c_int64, C.c_uint64, C.c_int32, C.c_double, C.c_double, vp, vp]
    L.surfh_mmmg_huber.argtypes = [vp, c_float_p] + [C.c_double] * 3 + tail + [c_double_p] + cb
    L.surfh_huber_prior_dev.argtypes = [vp, vp, vp, C.c_double, C.c_double, c_double_p]
    L.surfh_huber_curv_dev.argtypes = [vp, vp, vp, vp, C.c_double, c_double_p]
    L.surfh_mmmg_huber_vox.argtypes = [vp, c_float_p] + [C.c_double] * 5 + tail + [c_double_p] + cb
    L.surfh_huber_vox_prior_dev.argtypes = [vp, vp, vp] + [C.c_double] * 4 + [c_double_p]
    L.surfh_huber_vox_curv_dev.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, c_double_p]
    L.surfh_mmmg_robust.argtypes = [vp, c_float_p] + [C.c_double] * 4 + tail + [c_double_p, c_float_p] + cb
    L.surfh_mmmg_robust_vox.argtypes = [vp, c_float_p] + [C.c_double] * 6 + tail + [c_double_p, c_float_p] + cb
    L.surfh_robust_data_dev.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_double, vp, c_double_p]
    L.surfh_robust_curv_dev.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_double, c_double_p]
    L.surfh_mmmg_huber_planes.argtypes = L.surfh_mmmg_huber.argtypes
    L.surfh_huber_planes_prior_dev.argtypes = [vp, vp, vp, C.c_double, C.c_double, c_double_p, c_double_p]
    L.surfh_huber_planes_curv_dev.argtypes = [vp, vp, vp, vp, C.c_double, c_double_p]
    L.surfh_mmmg_huber_planes_ex.argtypes = [vp, c_float_p, C.c_double, c_double_p, c_double_p, C.c_int32] + tail + [c_double_p] + cb
    L.surfh_huber_planes_prior_dev_ex.argtypes = [vp, vp, vp, c_double_p, c_double_p, C.c_int32, c_double_p, c_double_p]
    L.surfh_huber_planes_curv_dev_ex.argtypes = [vp, vp, vp, vp, c_double_p, C.c_int32, c_double_p]
    L.surfh_debug_planes_passes.argtypes = [vp] + [C.c_int32] * 5 + [vp] * 4 + [c_double_p, c_double_p, c_double_p]
    L.surfh_debug_planes_cg.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)] + [vp] * 6 + [C.c_double, C.c_int32, c_double_p, c_double_p]
    L.surfh_debug_planes_normal.argtypes = [vp, vp, vp, C.c_double, C.c_double, c_double_p, vp]
    L.surfh_mmmg_planes.argtypes = L.surfh_cg_planes.argtypes
    L.surfh_cg_planes_begin_dev.argtypes = [vp, vp, C.c_double, C.c_double, vp]
    L.surfh_cg_planes_step_dev.argtypes = [vp, C.c_int32, C.c_int32]
    L.surfh_cg_planes_rr.argtypes = [vp, c_double_p]
    L.surfh_cg_planes_cb.argtypes = L.surfh_cg_cb.argtypes
    L.surfh_mmmg_planes_cb.argtypes = L.surfh_cg_cb.argtypes
    L.surfh_maps_to_cube.argtypes = [vp, c_double_p, C.c_int32, C.c_int32, c_float_p, c_float_p]
    L.surfh_cube_to_maps.argtypes = [vp, c_double_p, C.c_int32, C.c_int32, c_float_p, c_float_p]
    L.surfh_normal_dev.argtypes = [vp, vp, vp, C.c_double]
    L.surfh_prior_add_dev.argtypes = [vp, vp, vp, C.c_double]
    L.surfh_spec_supported.argtypes = [vp]
    L.surfh_spec_size.argtypes = [vp]
    L.surfh_spec_size.restype = C.c_int64
    L.surfh_to_spec_dev.argtypes = [vp, vp, vp]
    L.surfh_from_spec_dev.argtypes = [vp, vp, vp]
    L.surfh_forward_spec_dev.argtypes = [vp, vp, vp]
    L.surfh_adjoint_spec_dev.argtypes = [vp, vp, vp, C.c_double, vp, C.c_double]
    L.surfh_normal_spec_dev.argtypes = [vp, vp, vp, C.c_double, C.c_double]
    L.surfh_prior_spec_add_dev.argtypes = [vp, vp, vp, C.c_double]
    L.surfh_set_prior.argtypes = [vp, C.c_int32]
    L.surfh_set_potential.argtypes = [vp, C.c_int32, C.c_int32]
    L.surfh_get_potential.argtypes = [vp, C.c_int32]
    L.surfh_set_prior_coupling.argtypes = [vp, C.c_int32]
    L.surfh_debug_prior_passes.argtypes = [vp] + [C.c_int32] * 5 + [vp] * 4 + [C.c_double, C.c_double, c_double_p]
    L.surfh_get_prior_coupling.argtypes = [vp, c_int32_p]
    L.surfh_set_data_weights.argtypes = [vp, c_float_p]
    L.surfh_set_data_weights_dev.argtypes = [vp, vp]
    L.surfh_has_data_weights.argtypes = [vp]
    L.surfh_set_imager.argtypes = [vp, C.POINTER(ImagerDesc)]
    L.surfh_imager_osize.argtypes = [vp]
    L.surfh_has_imager_term.argtypes = [vp]
    for n in ("surfh_imager_forward", "surfh_imager_adjoint", "surfh_imager_fwadj"):
        getattr(L, n).argtypes = [vp, c_float_p, c_float_p]
    for n in ("surfh_imager_forward_dev", "surfh_imager_adjoint_dev"):
        getattr(L, n).argtypes = [vp, vp, vp]
    L.surfh_set_imager_data.argtypes = [vp, c_float_p, c_float_p, C.c_double]
    L.surfh_dot_dev.argtypes = [vp, vp, vp, C.c_int64, c_double_p]
    L.surfh_cg_step_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_double, c_double_p]
    L.surfh_cg_dir_dev.argtypes = [vp, vp, vp, C.c_int64, C.c_double]
    L.surfh_cg_iter_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_double, c_double_p]
    L.surfh_residual_dev.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.surfh_cg_begin_dev.argtypes = [vp, vp, C.c_int64]
    L.surfh_cg_iter_nosync_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int64]
    L.surfh_cg_xupdate_nosync_dev.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.surfh_cg_refresh_nosync_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int64]
    L.surfh_cg_trace.argtypes = [vp, c_double_p, C.c_int32]; L.surfh_cg_trace.restype = C.c_int32
    L.surfh_profile_enable.argtypes = [vp, C.c_int32]
    L.surfh_profile_filter.argtypes = [vp, C.c_char_p]
    L.surfh_profile_count.argtypes = [vp]; L.surfh_profile_count.restype = C.c_int32
    L.surfh_profile_get.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), c_double_p]
    L.surfh_profile_reset.argtypes = [vp]
    L.surfh_debug_copy.argtypes = [vp, C.c_char_p, c_float_p, C.c_int64]; L.surfh_debug_copy.restype = C.c_int64
    L.surfh_debug_dims.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.surfh_gemm_selftest.argtypes = [C.c_int32] * 5 + [c_float_p, c_float_p, c_float_p]
    L.surfh_gemm_selftest_ksteps.argtypes = [C.POINTER(C.c_int64)]
    L.surfh_gemm_selftest_ms.argtypes = [c_double_p]
    L.surfh_klist_classify.argtypes = [c_float_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64]
    L.surfh_klist_classify.restype = C.c_int32
    L.surfh_launch_geometry.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    L.surfh_route_decide.argtypes = [C.c_int32] * 3 + [C.c_int64] + [C.c_int32] * 3 + [C.c_uint32, C.c_int32, C.POINTER(C.c_int64)]
    L.surfh_mm_step2.argtypes = [C.c_double] * 5 + [c_double_p]
    L.surfh_debug_alloc_count.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.surfh_debug_alloc_count.restype = None
    L.surfh_debug_alloc_fail.argtypes = [C.c_int64]
    L.surfh_debug_alloc_fail.restype = None
    L.surfh_shepard.argtypes = [C.c_int32, C.POINTER(C.c_int64), vp, vp, vp, c_int32_p, c_int32_p, C.c_int32, vp, vp,
                                c_float_p, c_float_p, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, C.c_int32, vp,
                                c_float_p]
    L.surfh_shepard_last_error.restype = C.c_char_p
    L.surfh_spectral_median.argtypes = [c_float_p, c_float_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    L.surfh_nmf_cd.argtypes = [c_float_p, C.c_int64, C.c_int64, C.c_int32, c_int32_p, c_float_p, c_float_p, C.c_int32,
                               C.c_double, c_int32_p, c_double_p, c_double_p, c_double_p, C.c_int32, c_float_p]
    L.surfh_templates_last_error.restype = C.c_char_p
    L.surfh_set_templates.argtypes = [vp, c_double_p]
    L.surfh_get_templates.argtypes = [vp, c_double_p]
    L.surfh_forward_templates.argtypes = [vp, c_float_p, c_double_p, c_float_p]
    L.surfh_adjoint_templates.argtypes = [vp, c_float_p, c_float_p, c_float_p]
    for n in ("surfh_forward_templates_dev", "surfh_adjoint_templates_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp]
    L.surfh_cg_templates.argtypes = [vp, c_float_p, c_float_p, C.c_double, C.c_double] + tail
    L.surfh_cg_templates_cb.argtypes = L.surfh_cg_templates.argtypes + cb
    L.surfh_joint_criterion.argtypes = [vp, c_float_p, c_float_p, C.c_double, C.c_double, C.c_double, c_double_p]
    L.surfh_cg_nonneg.argtypes = [vp, c_float_p, C.c_double, C.c_double, C.c_double] + admm
    L.surfh_cg_templates_nonneg.argtypes = [vp, c_float_p, c_float_p, C.c_double, C.c_double, C.c_double] + admm
    L.surfh_nn_project_dev.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_double, c_double_p]
    L.surfh_cg_planes_nonneg.argtypes = [vp, c_float_p, C.c_double, C.c_double, c_double_p] + admm
    L.surfh_nn_project_planes_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int64, c_double_p, c_double_p]
    _lib = L
    return L


def check(rc: int, exc=RuntimeError):
    if rc != 0:
        raise exc(load().surfh_last_error().decode("utf-8", "replace"))


def fptr(a: np.ndarray):
    return a.ctypes.data_as(c_float_p)


def dptr(a: np.ndarray):
    return a.ctypes.data_as(c_double_p)


def iptr(a: np.ndarray):
    return a.ctypes.data_as(c_int32_p)


def u8ptr(a: np.ndarray):
    return a.ctypes.data_as(c_uint8_p)


# ---- marshalling: what every wrapper hands to a ``float *``, a ``void *`` or a ``uint64_t`` ---------------------------------------
def f32_vec(a, n, message, optional=False):
    """``a`` as the flat contiguous float32 vector a ``float *`` argument takes (``a`` itself where it already is one, a copy
    otherwise); ``ValueError(message)`` unless it has ``n`` elements.  ``optional``: ``None`` passes through (``x0``, ``s0``)."""
    if a is None and optional:
        return None
    v = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    if v.size != n:
        raise ValueError(message)
    return v


def opt_fptr(a):
    return None if a is None else fptr(a)


def dev_ptr(t):
    """The ``void *`` of a device argument: a tensor (anything with a ``data_ptr`` method), a raw address (``int``), or ``None`` (NULL)."""
    if t is None:
        return None
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def seed64(seed):
    """A Python integer as the generator's 64-bit key (its low 64 bits)."""
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


def host_call(fn, plan, x, nin, shape_out):
    """``fn(plan, in, out)`` on host arrays: ``x`` (``nin`` elements) in, float64 ``shape_out`` out."""
    a = f32_vec(x, nin, f"input has {np.size(x)} elements, expected {nin}")
    out = np.empty(int(np.prod(shape_out)), dtype=np.float32)
    check(fn(plan, fptr(a), fptr(out)))
    return out.astype(np.float64).reshape(shape_out)


# ---- callbacks ------------------------------------------------------------------------------------------------------------------
def trampoline(cbtype, callback, convert):
    """The C callable of a Python ``callback`` (``cbtype``: ``CG_CALLBACK`` or ``SAMPLE_CALLBACK``; the NULL callback for ``None``) and
    ``finish(rc, exc)``, to be called with the entry point's return code once it has returned.  The callback runs as
    ``callback(*convert(*raw))``, ``raw`` the C arguments after ``user``; a truthy return gives the library 1 (stop).  An exception
    in the callback (or in ``convert``) never unwinds through the C frame: it is held, the library is told to stop, and ``finish``
    raises it -- before it looks at the return code, which it turns into ``exc`` through ``check``."""
    held = []

    def tramp(_user, *raw):
        try:
            return 1 if callback(*convert(*raw)) else 0
        except BaseException as e:
            held.append(e)
            return 1

    def finish(rc, exc=RuntimeError):
        if held:
            raise held[0]
        check(rc, exc)

    return (cbtype(tramp) if callback is not None else cbtype()), finish


def iterate_args(size, shape, planes=1, squeeze=True):
    """The ``convert`` of both callback types, ``(it, trace, x)`` and ``(sample, nit, trace, x)`` -> ``(it or sample, trace, x)``:
    copies of the trace so far (``[n+1, planes]`` for the count ``n`` in front of it, ``[n+1]`` when ``squeeze``) and of the
    iterate (``size`` floats) as float64 ``shape``."""
    def convert(*raw):
        t = np.ctypeslib.as_array(raw[-2], shape=(raw[-3] + 1, planes)).copy()
        x = np.ctypeslib.as_array(raw[-1], shape=(size,)).astype(np.float64).reshape(shape)
        return raw[0], (t[:, 0] if squeeze else t), x

    return convert


# ---- host-buffer solvers --------------------------------------------------------------------------------------------------------
def _solve(model, fn, data, lead, x0, max_iter, tol, refresh, outs, callback, planes=1, squeeze=True, size=None, shape=None,
           exc=RuntimeError):
    """Run one host-buffer solver of the C ABI on ``model``'s plan:
    ``fn(plan, y, *lead, x0, max_iter, tol, refresh, x, grad_norm, nit, *outs, callback, NULL)``, ``lead`` the solver's leading
    arguments (numbers: weights, thresholds; ctypes values pass as they are) and ``outs`` its further out-buffers.  The iterate has
    ``size`` elements and comes back as ``shape`` (default: ``model.isize``, ``model.ishape``).  ``grad_norm`` has one column per
    plane, or is ``[nit+1]`` when ``squeeze`` (a single image).  A failure of the library raises ``exc``.  Returns
    ``(x, grad_norm, nit)``."""
    size, shape = (model.isize, model.ishape) if size is None else (size, shape)
    y = f32_vec(data, model.osize, "data size mismatch")
    x0a = f32_vec(x0, size, "x0 size mismatch", optional=True)
    x = np.empty(size, dtype=np.float32)
    gn = np.zeros((max_iter + 1, planes), dtype=np.float64)
    nit = C.c_int32()
    cb, finish = trampoline(CG_CALLBACK, callback, iterate_args(size, shape, planes, squeeze))
    lead = [v if isinstance(v, (C._Pointer, C._SimpleCData)) else float(v) for v in lead]       # ctypes arguments pass as they are
    finish(fn(model._plan, fptr(y), *lead, opt_fptr(x0a), int(max_iter), float(tol), int(refresh), fptr(x), dptr(gn), C.byref(nit),
              *outs, cb, None), exc)
    gn = gn[: nit.value + 1]
    return x.astype(np.float64).reshape(shape), (gn[:, 0] if squeeze else gn).copy(), nit.value


def _solve_nonneg(model, fn, data, lead, start, outer, inner, tol, refresh, size=None, shape=None, planes=None):
    """Run one ADMM solver of the C ABI on ``model``'s plan:
    ``fn(plan, y, *lead, start, outer, inner, tol, refresh, out, trace, nit)``, ``lead`` as in ``_solve`` (the penalty last: a number,
    or the pointer to one per plane), ``start`` optional.  The trace is ``[outer+1, 4]``, or ``[outer+1, 4, planes]`` for the
    plane-wise solver.  A failure of the library raises ``ValueError``.  Returns ``(out, trace, nit)``, the trace whole."""
    size, shape = (model.isize, model.ishape) if size is None else (size, shape)
    y = f32_vec(data, model.osize, "data size mismatch")
    s = f32_vec(start, size, "x0 size mismatch", optional=True)
    out = np.empty(size, dtype=np.float32)
    trace = np.zeros((int(outer) + 1, 4) + (() if planes is None else (planes,)), dtype=np.float64)
    nit = C.c_int32()
    lead = [v if isinstance(v, (C._Pointer, C._SimpleCData)) else float(v) for v in lead]
    check(fn(model._plan, fptr(y), *lead, opt_fptr(s), int(outer), int(inner), float(tol), int(refresh), fptr(out), dptr(trace),
             C.byref(nit)), ValueError)
    return out.astype(np.float64).reshape(shape), trace, nit.value


def solve(model, fn, data, mu, mu_reg, x0, max_iter, tol, refresh, callback, planes=1, squeeze=True):
    """``surfh_cg_cb``, ``surfh_mmmg``, ``surfh_cg_planes_cb`` or ``surfh_mmmg_planes_cb`` (``fn``).  Returns ``(x, grad_norm, nit)``."""
    return _solve(model, fn, data, (mu, mu_reg), x0, max_iter, tol, refresh, (), callback, planes, squeeze)


def solve_huber(model, data, mu, mu_reg, delta, x0, max_iter, tol, refresh, callback):
    """``surfh_mmmg_huber``.  Returns ``(x, grad_norm, nit, prior_value)``, prior_value = sum_k sum phi(D_k x) of the returned
    iterate."""
    pv = (C.c_double * 1)()
    return _solve(model, load().surfh_mmmg_huber, data, (mu, mu_reg, delta), x0, max_iter, tol, refresh, (pv,), callback) + (pv[0],)


def planes_entry(name, coupling, *values):
    """The entry point of a plane-wise prior call and its prior arguments.  ``coupling`` None: the scalar entry point ``name``, the
    ``values`` (``mu_reg``, ``delta``) as numbers, left to the library to check.  A coupling code (0 or 1): ``name + "_ex"``, the values
    float64 arrays ``[planes]`` (checked by ``blurred2d.plane_prior_args``), then the code."""
    if coupling is None:
        return getattr(load(), name), tuple(float(v) for v in values)
    return getattr(load(), name + "_ex"), tuple(dptr(v) for v in values) + (C.c_int32(int(coupling)),)


def solve_huber_planes(model, data, mu, mu_reg, delta, x0, max_iter, tol, refresh, callback, planes, squeeze, coupling=None):
    """``surfh_mmmg_huber_planes``, or with ``coupling`` (the code, 0 or 1) ``surfh_mmmg_huber_planes_ex`` on ``mu_reg`` and ``delta``
    float64 arrays ``[planes]``.  Returns ``(x, grad_norm, nit, prior_values)``, prior_values[l] = sum_k sum phi(D_k x_l) of the
    returned iterate (sum phi over the groups of the coupling)."""
    fn, prior = planes_entry("surfh_mmmg_huber_planes", coupling, mu_reg, delta)
    pv = np.zeros(planes, dtype=np.float64)
    return _solve(model, fn, data, (mu,) + prior, x0, max_iter, tol, refresh, (dptr(pv),), callback, planes, squeeze) + (pv,)


def solve_huber_planes_ex(model, data, mu, mu_reg, delta, coupling, x0, max_iter, tol, refresh, callback, planes, squeeze):
    """``solve_huber_planes`` with its ``coupling`` in the place it has in ``surfh_mmmg_huber_planes_ex``."""
    return solve_huber_planes(model, data, mu, mu_reg, delta, x0, max_iter, tol, refresh, callback, planes, squeeze, int(coupling))


def solve_huber_vox(model, data, mu, spat_reg, spat_delta, spec_reg, spec_delta, x0, max_iter, tol, refresh, callback):
    """``surfh_mmmg_huber_vox`` (a plan without templates).  Returns ``(x, grad_norm, nit, (spatial, spectral))``, the two sums
    of phi at the returned iterate."""
    pv = (C.c_double * 2)()
    return _solve(model, load().surfh_mmmg_huber_vox, data, (mu, spat_reg, spat_delta, spec_reg, spec_delta), x0, max_iter, tol,
                  refresh, (pv,), callback) + (tuple(pv),)


def solve_robust(model, data, mu, data_delta, mu_reg, delta, x0, max_iter, tol, refresh, callback):
    """``surfh_mmmg_robust``.  Returns ``(x, grad_norm, nit, values, omega)``: values = (sum phi(t), number of |t| > data_delta,
    prior value) and omega ``[osize]`` the robustness weights, at the returned iterate."""
    vals, omega = (C.c_double * 3)(), np.zeros(model.osize, dtype=np.float32)
    return _solve(model, load().surfh_mmmg_robust, data, (mu, data_delta, mu_reg, delta), x0, max_iter, tol, refresh,
                  (vals, fptr(omega)), callback) + (tuple(vals), omega)


def solve_robust_vox(model, data, mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta, x0, max_iter, tol, refresh, callback):
    """``surfh_mmmg_robust_vox`` (a plan without templates).  Returns ``(x, grad_norm, nit, values, omega)``, values =
    (sum phi(t), number of |t| > data_delta, spatial prior value, spectral prior value)."""
    vals, omega = (C.c_double * 4)(), np.zeros(model.osize, dtype=np.float32)
    return _solve(model, load().surfh_mmmg_robust_vox, data, (mu, data_delta, spat_reg, spat_delta, spec_reg, spec_delta), x0, max_iter,
                  tol, refresh, (vals, fptr(omega)), callback) + (tuple(vals), omega)
