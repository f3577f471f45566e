"""ctypes binding of ``libpdsc.so`` (the C ABI declared in ``include/pdsc.h``).

The library is built in-tree by ``make -C pointdsc_amd/csrc`` (or
``__graft_entry__.build()``).  There is no fallback: if the library is missing
or cannot be loaded, every entry point raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# PDSC_LIB_VARIANT=<v> loads libpdsc_<v>.so (an A/B build of the same sources,
# `make -C pointdsc_amd/csrc variant V=<v> VFLAGS=...`; measurement only)
_VARIANT = os.environ.get("PDSC_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, f"libpdsc_{_VARIANT}.so" if _VARIANT else "libpdsc.so")

c_int32, c_size_t, c_float, c_double = ctypes.c_int32, ctypes.c_size_t, ctypes.c_float, ctypes.c_double
vp = ctypes.c_void_p


class PdscConfig(ctypes.Structure):
    """``struct pdsc_config`` (include/pdsc.h)."""
    _fields_ = [
        ("in_dim", c_int32),
        ("num_layers", c_int32),
        ("num_channels", c_int32),
        ("num_iterations", c_int32),
        ("k", c_int32),
        ("ratio", c_double),
        ("inlier_threshold", c_float),
        ("nms_radius", c_float),
        ("refine_threshold", c_float),
        ("precision", c_int32),
    ]


# enum pdsc_precision (include/pdsc.h)
PRECISIONS = {"h3": 0, "f32": 1}


def precision_code(precision) -> int:
    """'h3' (default: 3 fp16 MFMA products per fp32 product) or 'f32' (exact fp32 MFMA)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
    return PRECISIONS[precision]


CFG = ctypes.POINTER(PdscConfig)


class PdscForwardDebug(ctypes.Structure):
    """``struct pdsc_forward_debug`` (include/pdsc.h): optional stage outputs."""
    _fields_ = [("conf", vp), ("seeds", vp), ("knn", vp), ("weights", vp), ("trans_pre_refine", vp)]


class PdscIcpResult(ctypes.Structure):
    """``struct pdsc_icp_result`` (include/pdsc.h): 152 bytes of device memory."""
    _fields_ = [("trans", c_double * 16), ("fitness", c_double), ("inlier_rmse", c_double), ("iterations", c_int32),
                ("n_corr", c_int32)]


class PdscRansacResult(ctypes.Structure):
    """``struct pdsc_ransac_result`` (include/pdsc.h): 160 bytes of device memory."""
    _fields_ = [("trans", c_double * 16), ("fitness", c_double), ("inlier_rmse", c_double), ("n_inliers", c_int32),
                ("iterations", c_int32), ("best", c_int32), ("n_validated", c_int32)]


class PdscRansacDebug(ctypes.Structure):
    """``struct pdsc_ransac_debug`` (include/pdsc.h): optional per-hypothesis outputs."""
    _fields_ = [("samples", vp), ("count", vp), ("sumsq", vp), ("trans", vp)]


class PdscGpfDebug(ctypes.Structure):
    """``struct pdsc_gpf_debug`` (include/pdsc.h): optional outputs of pdsc_gpf_select."""
    _fields_ = [("cell", vp), ("max_per_quad", vp), ("per_quad", vp), ("height", vp)]


class PdscCliqueResult(ctypes.Structure):
    """``struct pdsc_clique_result`` (include/pdsc.h): 24 bytes of device memory."""
    _fields_ = [("size", c_int32), ("exact", c_int32), ("heuristic_size", c_int32), ("roots_incomplete", c_int32),
                ("nodes", ctypes.c_int64)]


class PdscGncInfo(ctypes.Structure):
    """``struct pdsc_gnc_info`` (include/pdsc.h): 24 bytes of device memory."""
    _fields_ = [("iterations", c_int32), ("stop_reason", c_int32), ("cost", c_double), ("mu", c_double)]


class PdscTeaserResult(ctypes.Structure):
    """``struct pdsc_teaser_result`` (include/pdsc.h): 160 bytes of device memory."""
    _fields_ = [("trans", c_double * 16), ("valid", c_int32), ("clique_size", c_int32), ("clique_exact", c_int32),
                ("roots_incomplete", c_int32), ("gnc_iterations", c_int32), ("n_rotation_inliers", c_int32),
                ("n_translation_inliers", c_int32), ("reserved", c_int32)]


class PdscGcLabelDebug(ctypes.Structure):
    """``struct pdsc_gc_label_debug`` (include/pdsc.h): optional outputs of pdsc_gc_label."""
    _fields_ = [("d2", vp), ("m_star", vp), ("energy", vp), ("energy_gap", vp)]


class PdscGcRansacResult(ctypes.Structure):
    """``struct pdsc_gc_ransac_result`` (include/pdsc.h): 160 bytes of device memory."""
    _fields_ = [("trans", c_double * 16), ("score", c_double), ("n_inliers", c_int32), ("iterations", c_int32),
                ("best", c_int32), ("lo_runs", c_int32), ("lo_steps", c_int32), ("n_cells", c_int32)]


class PdscGcRansacDebug(ctypes.Structure):
    """``struct pdsc_gc_ransac_debug`` (include/pdsc.h): optional per-hypothesis outputs."""
    _fields_ = [("samples", vp), ("count", vp), ("score", vp), ("trans", vp)]


class PdscInformationResult(ctypes.Structure):
    """``struct pdsc_information_result`` (include/pdsc.h): 296 bytes of device memory."""
    _fields_ = [("info", c_double * 36), ("n_corr", c_int32), ("pad", c_int32)]


class PdscPoseGraphOptions(ctypes.Structure):
    """``struct pdsc_pose_graph_options`` (include/pdsc.h): a host struct."""
    _fields_ = [("max_correspondence_distance", c_double), ("edge_prune_threshold", c_double),
                ("preference_loop_closure", c_double), ("reference_node", c_int32), ("pad", c_int32)]


class PdscPoseGraphCriteria(ctypes.Structure):
    """``struct pdsc_pose_graph_criteria`` (include/pdsc.h): a host struct; open3d's defaults."""
    _fields_ = [("max_iteration", c_int32), ("max_iteration_lm", c_int32), ("min_relative_increment", c_double),
                ("min_relative_residual_increment", c_double), ("min_right_term", c_double),
                ("min_residual", c_double)]


class PdscPoseGraphResult(ctypes.Structure):
    """``struct pdsc_pose_graph_result`` (include/pdsc.h): 48 bytes of device memory."""
    _fields_ = [("objective", c_double * 2), ("mu", c_double * 2), ("iterations", c_int32 * 2),
                ("edges_kept", c_int32), ("solver_failed", c_int32)]


class PdscRgbdOdometryOptions(ctypes.Structure):
    """``struct pdsc_rgbd_odometry_options`` (include/pdsc.h): a host struct; open3d's OdometryOption."""
    _fields_ = [("max_depth_diff", c_double), ("min_depth", c_double), ("max_depth", c_double),
                ("iterations", c_int32 * 3), ("pad", c_int32)]


class PdscRgbdOdometryStatus(ctypes.Structure):
    """``struct pdsc_rgbd_odometry_status`` (include/pdsc.h): 16 bytes of device memory per pair."""
    _fields_ = [("success", c_int32), ("n_corr_last", c_int32), ("iterations_run", c_int32), ("pad", c_int32)]


class PdscFcgfDebug(ctypes.Structure):
    """``struct pdsc_fcgf_debug`` (include/pdsc.h): optional taps of pdsc_fcgf_forward."""
    _fields_ = [("block1", vp), ("block2", vp), ("block3", vp), ("block4", vp), ("block4_tr", vp), ("block3_tr", vp),
                ("block2_tr", vp), ("conv1_tr", vp), ("coords2", vp), ("coords4", vp), ("coords8", vp), ("counts", vp)]


# enum pdsc_edge_mode (include/pdsc.h)
EDGE_MODES = {"squared": 0, "length": 1}


# name -> (restype, argtypes)
_PROTOS = {
    "pdsc_version": (ctypes.c_char_p, []),
    "pdsc_last_error": (ctypes.c_char_p, []),
    "pdsc_param_count": (c_int32, [CFG]),
    "pdsc_param_name": (ctypes.c_char_p, [CFG, c_int32]),
    "pdsc_packed_weights_floats": (c_size_t, [CFG]),
    "pdsc_pack_weights": (c_int32, [CFG, ctypes.POINTER(vp), vp, vp]),
    "pdsc_compat_f32": (c_int32, [vp, vp, c_int32, c_int32, vp, vp, vp]),
    "pdsc_compat_packed_floats": (c_size_t, [c_int32]),
    "pdsc_compat_packed_f32": (c_int32, [vp, vp, c_int32, c_int32, vp, vp, vp]),
    "pdsc_encoder_workspace_bytes": (c_size_t, [CFG, c_int32, c_int32]),
    "pdsc_encoder_f32": (c_int32, [CFG, vp, vp, vp, c_int32, c_int32, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_attention_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "pdsc_attention_f32": (c_int32, [vp, vp, vp, vp, c_int32, c_int32, c_int32, c_int32, vp, vp, c_size_t, vp]),
    "pdsc_attention_lse_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "pdsc_attention_lse_f32": (c_int32, [vp, vp, vp, vp, c_int32, c_int32, c_int32, vp, vp, vp, c_size_t, vp]),
    "pdsc_attention_backward_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "pdsc_attention_backward_f32": (c_int32, [vp, vp, vp, vp, vp, vp, vp, c_int32, c_int32, c_int32, vp, vp, vp, vp,
                                              c_size_t, vp]),
    "pdsc_sm_loss_fused_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "pdsc_sm_loss_fused_f32": (c_int32, [vp, vp, vp, c_int32, c_int32, c_int32, c_int32, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_attention_layout": (c_int32, [c_int32, c_int32, c_int32, ctypes.POINTER(c_int32),
                                        ctypes.POINTER(c_int32)]),
    "pdsc_encoder_plan": (c_int32, [c_int32, c_int32, c_int32, ctypes.POINTER(c_int32)]),
    "pdsc_encoder_plan_vfold": (c_int32, [c_int32, c_int32, c_int32, ctypes.POINTER(c_int32)]),
    "pdsc_launch_plan": (c_int32, [CFG, c_int32, c_int32, ctypes.POINTER(c_int32), c_int32]),
    "pdsc_packed_block": (c_int32, [CFG, c_int32, c_int32, ctypes.POINTER(c_size_t)]),
    "pdsc_attention_timing": (c_int32, [ctypes.POINTER(vp), ctypes.POINTER(vp), c_int32, ctypes.POINTER(c_int32)]),
    "pdsc_forward_timing": (c_int32, [ctypes.POINTER(vp), c_int32, ctypes.POINTER(c_int32)]),
    "pdsc_diag_qkv_delay": (c_int32, [c_int32]),
    "pdsc_pick_seeds": (c_int32, [vp, vp, c_int32, c_int32, c_float, c_int32, vp, vp, vp]),
    "pdsc_seed_knn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "pdsc_seed_knn": (c_int32, [vp, vp, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, vp, vp, c_size_t,
                                vp]),
    "pdsc_nsm_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "pdsc_nsm_weights": (c_int32, [vp, vp, vp, vp, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                   vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_rigid_transform_3d": (c_int32, [vp, vp, vp, c_int32, c_int32, vp, vp]),
    "pdsc_seed_hypotheses_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_seed_hypotheses": (c_int32, [vp, vp, vp, vp, c_int32, c_int32, c_int32, c_int32, c_float,
                                       vp, vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_post_refine": (c_int32, [vp, vp, vp, c_int32, c_int32, c_float, vp]),
    "pdsc_mutual_nn_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_mutual_nn": (c_int32, [vp, vp, c_int32, c_int32, c_int32, vp, vp, vp, c_size_t, vp]),
    "pdsc_build_correspondences": (c_int32, [vp, vp, vp, vp, c_int32, c_int32, c_int32, c_int32, vp, c_double,
                                             vp, vp, vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_spectral_matching_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_spectral_matching": (c_int32, [vp, vp, vp, c_int32, c_double, c_double, c_int32, vp, vp, vp, vp,
                                         c_size_t, vp]),
    "pdsc_sm_compat": (c_int32, [vp, c_int32, c_double, vp, vp]),
    "pdsc_sm_matvec": (c_int32, [vp, vp, c_int32, vp, vp]),
    "pdsc_forward_workspace_bytes": (c_size_t, [CFG, c_int32, c_int32]),
    "pdsc_forward_testing": (c_int32, [CFG, vp, vp, vp, vp, c_int32, c_int32, vp, vp, vp, vp, vp,
                                       c_size_t, vp]),
    "pdsc_forward_testing_debug": (c_int32, [CFG, vp, vp, vp, vp, c_int32, c_int32, vp, vp,
                                             ctypes.POINTER(PdscForwardDebug), vp, c_size_t, vp]),
    "pdsc_forward_testing_ragged": (c_int32, [CFG, vp, vp, vp, vp, c_int32, c_int32, ctypes.POINTER(c_int32), vp, vp,
                                              ctypes.POINTER(PdscForwardDebug), vp, c_size_t, vp]),
    "pdsc_ply_read_xyz": (c_int32, [ctypes.c_char_p, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "pdsc_radius_knn_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_radius_knn": (c_int32, [vp, c_int32, c_float, c_int32, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_estimate_normals_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_estimate_normals": (c_int32, [vp, c_int32, c_float, c_int32, c_int32, vp, vp, vp, c_size_t, vp]),
    "pdsc_voxel_down_sample_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_voxel_down_sample": (c_int32, [vp, vp, c_int32, c_float, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_compute_fpfh_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_compute_fpfh": (c_int32, [vp, vp, c_int32, c_float, c_int32, vp, vp, vp, c_size_t, vp]),
    "pdsc_icp_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_icp_point_to_point": (c_int32, [vp, c_int32, vp, c_int32, vp, c_double, c_int32, c_double, c_double, vp, vp,
                                          vp, vp, c_size_t, vp]),
    "pdsc_ransac_round": (c_int32, []),
    "pdsc_ransac_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_ransac_correspondence": (c_int32, [vp, vp, c_int32, c_double, c_int32, c_double, c_int32, c_double,
                                             ctypes.c_uint64, c_int32, vp, vp, vp, ctypes.POINTER(PdscRansacDebug),
                                             vp, c_size_t, vp]),
    "pdsc_nn2_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_nn2": (c_int32, [vp, vp, c_int32, c_int32, c_int32, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_nn2_split": (c_int32, [vp, vp, c_int32, c_int32, c_int32, c_int32, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_match_ratio": (c_int32, [vp, vp, c_int32, c_int32, c_int32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pdsc_gpf_select_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_gpf_select": (c_int32, [vp, vp, vp, c_int32, c_int32, c_double, vp, vp, vp, ctypes.POINTER(PdscGpfDebug),
                                  vp, c_size_t, vp]),
    "pdsc_refit_inliers": (c_int32, [vp, vp, vp, c_int32, c_double, vp, vp, vp, vp, vp]),
    "pdsc_consistency_graph": (c_int32, [vp, c_int32, c_double, c_int32, vp, vp, vp]),
    "pdsc_max_clique_depth": (c_int32, []),
    "pdsc_max_clique_default_budget": (ctypes.c_int64, []),
    "pdsc_max_clique_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_max_clique": (c_int32, [vp, c_int32, ctypes.c_int64, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_greedy_clique": (c_int32, [vp, c_int32, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_gnc_tls_rotation": (c_int32, [vp, vp, c_int32, c_double, c_double, c_int32, c_double, vp, vp, vp, vp, vp]),
    "pdsc_tls_translation_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_tls_translation": (c_int32, [vp, vp, c_int32, c_double, vp, vp, vp, c_size_t, vp]),
    "pdsc_teaser_solve_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_teaser_solve": (c_int32, [vp, vp, c_int32, c_double, c_double, c_int32, c_double, ctypes.c_int64, vp, vp,
                                    vp, vp, c_size_t, vp]),
    "pdsc_gc_cell_bound": (c_int32, [c_int32]),
    "pdsc_gc_grid_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_gc_grid": (c_int32, [vp, vp, c_int32, c_int32, vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_gc_label_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_gc_label": (c_int32, [vp, vp, vp, c_int32, vp, vp, vp, c_double, c_double, vp, vp,
                                ctypes.POINTER(PdscGcLabelDebug), vp, c_size_t, vp]),
    "pdsc_gc_ransac_round": (c_int32, []),
    "pdsc_gc_ransac_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_gc_ransac": (c_int32, [vp, vp, c_int32, c_double, c_double, c_int32, c_int32, c_double, ctypes.c_uint64,
                                 c_int32, vp, vp, vp, ctypes.POINTER(PdscGcRansacDebug), vp, c_size_t, vp]),
    "pdsc_information_matrix_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_information_matrix": (c_int32, [vp, c_int32, vp, c_int32, vp, c_double, vp, vp, vp, c_size_t, vp]),
    "pdsc_pose_graph_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_pose_graph_optimize": (c_int32, [vp, c_int32, vp, vp, vp, vp, vp, c_int32, vp, vp, vp, vp, vp, vp, c_size_t,
                                           vp]),
    "pdsc_pose_graph_linearize": (c_int32, [vp, c_int32, vp, vp, vp, vp, vp, c_int32, vp, c_double, c_int32, vp, vp,
                                            vp, vp, vp, c_size_t, vp]),
    "pdsc_rgbd_odometry_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "pdsc_rgbd_odometry": (c_int32, [vp, vp, c_int32, c_int32, c_int32, c_double, c_double, c_double, c_double, vp, vp,
                                     c_int32, vp, vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_rgbd_odometry_linearize": (c_int32, [vp, vp, c_int32, c_int32, c_int32, c_double, c_double, c_double,
                                               c_double, vp, vp, c_int32, vp, vp, c_int32, vp, vp, vp, vp, c_size_t,
                                               vp]),
    "pdsc_rgbd_odometry_pyramid": (c_int32, [vp, vp, c_int32, c_int32, c_int32, c_double, c_double, c_int32, vp, vp, vp,
                                             vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_rgbd_from_color_and_depth": (c_int32, [vp, vp, c_int32, c_int32, c_int32, c_double, c_double, vp, vp, vp]),
    "pdsc_tsdf_workspace_bytes": (c_size_t, [c_int32]),
    "pdsc_tsdf_reset": (c_int32, [c_int32, vp, c_size_t, vp]),
    "pdsc_tsdf_integrate": (c_int32, [vp, vp, c_int32, c_int32, c_double, c_double, c_double, c_double, vp, c_double,
                                      c_double, c_int32, vp, c_size_t, vp]),
    "pdsc_tsdf_read_blocks": (c_int32, [c_int32, c_int32, vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_tsdf_write_blocks": (c_int32, [vp, c_int32, vp, vp, vp, c_int32, vp, c_size_t, vp]),
    "pdsc_tsdf_count_surface_points": (c_int32, [c_int32, vp, vp, c_size_t, vp]),
    "pdsc_tsdf_emit_surface_points": (c_int32, [c_double, c_int32, vp, vp, ctypes.c_int64, vp, c_size_t, vp]),
    "pdsc_fcgf_param_floats": (c_size_t, [c_int32, c_int32]),
    "pdsc_fcgf_packed_floats": (c_size_t, [c_int32, c_int32]),
    "pdsc_fcgf_pack_weights": (c_int32, [vp, c_int32, c_int32, vp, vp]),
    "pdsc_fcgf_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "pdsc_fcgf_quantize": (c_int32, [vp, c_int32, vp, c_int32, c_float, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_fcgf_forward": (c_int32, [vp, c_int32, c_int32, c_int32, vp, vp, c_int32, vp, ctypes.POINTER(PdscFcgfDebug),
                                    vp, c_size_t, vp]),
    "pdsc_forward_training_workspace_bytes": (c_size_t, [CFG, c_int32, c_int32]),
    "pdsc_range_status": (c_int32, [vp, c_int32, ctypes.POINTER(c_int32), vp]),
    "pdsc_range_poll": (c_int32, [vp, c_int32, vp]),
    "pdsc_forward_training": (c_int32, [CFG, vp, vp, vp, vp, c_int32, c_int32, vp, vp, vp, vp, vp, c_size_t, vp]),
    "pdsc_spectral_matching_loss_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "pdsc_spectral_matching_loss": (c_int32, [vp, vp, c_int32, c_int32, c_int32, vp, vp, c_size_t, vp]),
}

EXPORTS = tuple(_PROTOS)

_lib = None
_lock = threading.Lock()


def load():
    """Load libpdsc.so once; raise RuntimeError (no fallback) if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"pointdsc_amd: HIP library {LIB_PATH} is missing; build it with "
                    "`make -C pointdsc_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`. "
                    "There is no CPU fallback.")
            try:
                lib = ctypes.CDLL(LIB_PATH)
            except OSError as e:
                raise RuntimeError(f"pointdsc_amd: cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in _PROTOS.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            _lib = lib
    return _lib


def check(status: int, what: str):
    if status != 0:
        msg = load().pdsc_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")


def make_config(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, k=40, ratio=0.1,
                inlier_threshold=0.10, nms_radius=0.10, precision="h3") -> PdscConfig:
    """Build ``pdsc_config``; the refine threshold follows models/PointDSC.py:415-418."""
    refine = 0.10 if inlier_threshold == 0.10 else 1.2
    return PdscConfig(int(in_dim), int(num_layers), int(num_channels), int(num_iterations), int(k),
                      float(ratio), float(inlier_threshold), float(nms_radius), float(refine),
                      precision_code(precision))
