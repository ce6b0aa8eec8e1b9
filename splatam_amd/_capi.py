"""ctypes view of the C ABI in include/splat_hip.h (libsplat_hip.so).

The library is the product: there is NO fallback.  ``lib()`` raises if the
shared object has not been built (``python -m splatam_amd.build`` or
``__graft_entry__.build()``), and every rasterizer entry point goes through it.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SPLAT_HIP_LIB: developer override, A/B timing of two builds in one process launch each: scripts/ab_lib.sh)
LIB_PATH = os.environ.get("SPLAT_HIP_LIB") or os.path.join(_HERE, "lib", "libsplat_hip.so")

SPLAT_TILE = 16
SPLAT_MAX_CHANNELS = 8
SPLAT_GRAD_STRIDE = 16
SPLAT_COUNTER_STRIDE = 32
SPLAT_GROUP_TILES = 2
ABI_VERSION = 17
SPLAT_DEPTH_U16, SPLAT_DEPTH_F32 = 0, 1
SPLAT_VIEW_COLOR, SPLAT_VIEW_DEPTH, SPLAT_VIEW_SILHOUETTE = 0, 1, 2

_fp = C.c_void_p  # device pointers travel as integers


class SplatCamera(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32),
                ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("bg", _fp), ("scale_modifier", C.c_float),
                ("viewmatrix", _fp), ("projmatrix", _fp),
                ("sh_degree", C.c_int32), ("campos", _fp), ("prefiltered", C.c_int32)]


class SplatGaussians(C.Structure):
    _fields_ = [("P", C.c_int32), ("channels", C.c_int32),
                ("means3D", _fp), ("opacities", _fp), ("colors_precomp", _fp),
                ("scales", _fp), ("rotations", _fp), ("cov3D_precomp", _fp),
                ("shs", _fp), ("sh_coeffs", C.c_int32)]


class SplatState(C.Structure):
    _fields_ = [("depth", _fp), ("xy", _fp), ("conic_opacity", _fp), ("rect", _fp), ("radii", _fp),
                ("rgb", _fp), ("clamped", _fp),
                ("tile_count", _fp), ("tile_base", _fp), ("tile_cursor", _fp),
                ("keys", _fp), ("point_list", _fp), ("capacity", C.c_int64), ("tile_recs", _fp), ("keys_alt", _fp), ("long_base", _fp), ("long_items", _fp),
                ("group_count", _fp), ("group_recs", _fp),
                ("max_list_hint", C.c_int32), ("order_hint", C.c_int32), ("sub_bins", C.c_int32), ("tile_stride", C.c_int32),
                ("group_stride", C.c_int32), ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32),
                ("tile_work", _fp), ("tile_order", _fp),
                ("final_T", _fp), ("n_contrib", _fp), ("status", _fp), ("status_host", _fp), ("accum_to_zero", _fp)]


class SplatGrads(C.Structure):
    _fields_ = [("dL_dcolor", _fp), ("accum", _fp), ("dL_dmeans3D", _fp), ("dL_dmeans2D", _fp),
                ("dL_dcolors", _fp), ("dL_dopacities", _fp), ("dL_dscales", _fp), ("dL_drotations", _fp),
                ("dL_dcov3D", _fp), ("dL_dshs", _fp), ("flags", C.c_int32)]


class SplatMap(C.Structure):
    _fields_ = [("P", C.c_int32), ("isotropic", C.c_int32),
                ("means3D", _fp), ("rgb_colors", _fp), ("unnorm_rotations", _fp), ("logit_opacities", _fp),
                ("log_scales", _fp), ("cam_unnorm_rots", _fp), ("cam_trans", _fp), ("num_frames", C.c_int32)]


class SplatFrameData(C.Structure):
    _fields_ = [("im", _fp), ("depth", _fp), ("w2c", _fp), ("time_idx", C.c_int32)]


class SplatLossConfig(C.Structure):
    _fields_ = [("tracking", C.c_int32), ("camera_grad", C.c_int32), ("gaussians_grad", C.c_int32),
                ("use_sil_for_loss", C.c_int32), ("sil_thres", C.c_float), ("use_l1", C.c_int32),
                ("ignore_outlier_depth_loss", C.c_int32), ("w_im", C.c_float), ("w_depth", C.c_float),
                ("defer_finish", C.c_int32), ("fused_composite", C.c_int32)]


class SplatLossConfigEx(C.Structure):       # (added within ABI 17: the loss of the refinement script, include/splat_hip.h)
    _fields_ = [("base", SplatLossConfig), ("loss_mode", C.c_int32), ("reserved", C.c_int32 * 3)]


class SplatIterWorkspace(C.Structure):
    _fields_ = [("st", SplatState), ("feat8", _fp), ("out6", _fp), ("dL_dout6", _fp), ("accum", _fp),
                ("ssim_maps", _fp), ("sums", _fp), ("max_2D_radius", _fp),
                ("d_means3D", _fp), ("d_rgb_colors", _fp), ("d_unnorm_rotations", _fp), ("d_logit_opacities", _fp),
                ("d_log_scales", _fp), ("d_cam", _fp), ("outlier_err", _fp), ("outlier_scratch", _fp)]


class SplatAdamMap(C.Structure):
    _fields_ = [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("one_minus_beta1", C.c_float),
                ("one_minus_beta2", C.c_float), ("bc2_sqrt", C.c_float * 5),
                ("step_size", C.c_float * 5), ("grad", _fp * 5), ("exp_avg", _fp * 5), ("exp_avg_sq", _fp * 5), ("gate", _fp)]


class SplatMapStore(C.Structure):
    _fields_ = [("map", SplatMap), ("capacity", C.c_int32), ("exp_avg", _fp * 5), ("exp_avg_sq", _fp * 5),
                ("max_2D_radius", _fp), ("means2D_gradient_accum", _fp), ("denom", _fp), ("timestep", _fp), ("counts", _fp)]


class SplatAddArgs(C.Structure):
    _fields_ = [("mode", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("im", _fp), ("depth", _fp), ("out6", _fp),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("sil_thres", C.c_float),
                ("time_idx", C.c_int32), ("w2c", _fp), ("err", _fp), ("scratch", _fp)]


class SplatPruneArgs(C.Structure):
    _fields_ = [("removal_opacity_threshold", C.c_float), ("remove_big", C.c_int32), ("big_scale", C.c_float),
                ("to_remove", _fp), ("flags", _fp), ("stage", _fp), ("scratch", _fp)]


class SplatDensifyArgs(C.Structure):
    _fields_ = [("mode", C.c_int32), ("grad_thresh", C.c_float), ("small_scale", C.c_float), ("rows_with_grad", C.c_int32),
                ("num_to_split_into", C.c_int32), ("samples", _fp), ("flags", _fp), ("scratch", _fp)]


class SplatPoseAdam(C.Structure):
    _fields_ = [("state", _fp), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("bc2_sqrt", C.c_float),
                ("step_size_rot", C.c_float), ("step_size_trans", C.c_float)]


class SplatArrayInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("bytes", C.c_size_t), ("offset", C.c_size_t), ("zero_init", C.c_int32)]


class SplatEvalConfig(C.Structure):
    _fields_ = [("sil_thres", C.c_float), ("sil_mask", C.c_int32), ("ms_ssim", C.c_int32), ("holes", C.c_int32)]


class SplatEvalWorkspace(C.Structure):
    _fields_ = [("pyramid", _fp), ("sums", _fp)]


class SplatViewArgs(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("near_z", C.c_double), ("far_z", C.c_double),
                ("w2c_in", _fp), ("cam_unnorm_rots", _fp), ("cam_trans", _fp), ("first_w2c", _fp),
                ("num_frames", C.c_int32), ("time_idx", C.c_int32), ("offset", C.POINTER(C.c_double)),
                ("w2c", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("campos", _fp),
                ("out6", _fp), ("mode", C.c_int32), ("bg", C.c_float * 3), ("vmin", C.c_float), ("vmax", C.c_float),
                ("lut", _fp), ("rgb8", _fp), ("points", _fp), ("colors", _fp)]


class SplatTsdfVolume(C.Structure):        # (added within ABI 17: the mesh layer, csrc/tsdf.hip)
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel", C.c_float), ("trunc", C.c_float),
                ("tsdf", _fp), ("weight", _fp), ("r", _fp), ("g", _fp), ("b", _fp)]


class SplatTsdfView(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("sil_thres", C.c_float), ("depth_max", C.c_float), ("weight_max", C.c_float),
                ("out6", _fp), ("w2c", _fp), ("skip", _fp), ("skipped", _fp)]


class SplatTsdfSparse(C.Structure):        # (added within ABI 17: the sparse volume, csrc/tsdf_sparse.hip)
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel", C.c_float), ("trunc", C.c_float),
                ("brick", C.c_int32 * 3), ("slots", C.c_int32), ("directory", _fp), ("brick_of_slot", _fp),
                ("tsdf", _fp), ("weight", _fp), ("r", _fp), ("g", _fp), ("b", _fp)]


class SplatNnGrid(C.Structure):            # (added within ABI 17: the mesh score layer, csrc/meshscore.hip)
    _fields_ = [("lo", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_int32 * 3), ("count", C.c_int32), ("records", _fp), ("start", _fp)]


class SplatMeshView(C.Structure):          # (added within ABI 17: the mesh render layer, csrc/meshrender.hip)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near_z", C.c_float), ("w2c", _fp)]


class SplatMeshShade(C.Structure):         # (added within ABI 17: the mesh shade layer, csrc/meshshade.hip)
    _fields_ = [("mode", C.c_int32), ("samples", C.c_int32), ("smooth", C.c_int32), ("normal_frame", C.c_int32), ("bg", C.c_float * 3),
                ("albedo", C.c_float * 3), ("ambient", C.c_float), ("vmin", C.c_float), ("vmax", C.c_float), ("lut", _fp)]


class SplatViewOverlay(C.Structure):       # (added within ABI 17: the view overlay, csrc/viewoverlay.hip)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near_z", C.c_float), ("w2c", _fp), ("keys", _fp)]


class SplatViewRun(C.Structure):
    _fields_ = [("num_frames", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("w2c_all", _fp),
                ("cam_unnorm_rots", _fp), ("cam_trans", _fp), ("first_w2c", _fp), ("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("scale", C.c_double),
                ("frusta", C.c_int32), ("fixed_color", C.c_int32), ("color", C.c_uint8 * 4), ("segments", _fp), ("colors", _fp)]


class SplatViewOverlayFinish(C.Structure):
    _fields_ = [("depth", _fp), ("occlude", C.c_int32), ("fill", C.c_int32), ("rgb_colors", _fp), ("num_rows", C.c_int32),
                ("segment_colors", _fp), ("num_segments", C.c_int32), ("bg", C.c_float * 3), ("rgb8", _fp)]


class SplatLpipsWorkspace(C.Structure):    # (added within ABI 17: LPIPS from caller-supplied weights, csrc/lpips.hip)
    _fields_ = [("input", _fp), ("taps", _fp * 5), ("pooled", _fp * 2), ("partials", _fp), ("width", C.c_int32), ("height", C.c_int32)]


MIRRORED_STRUCTS = (SplatCamera, SplatGaussians, SplatState, SplatGrads, SplatMap, SplatFrameData, SplatLossConfig, SplatLossConfigEx,
                    SplatIterWorkspace, SplatAdamMap, SplatMapStore, SplatAddArgs, SplatPruneArgs, SplatDensifyArgs, SplatPoseAdam, SplatArrayInfo,
                    SplatEvalConfig, SplatEvalWorkspace, SplatViewArgs, SplatTsdfVolume, SplatTsdfView, SplatNnGrid, SplatMeshView, SplatLpipsWorkspace,
                    SplatTsdfSparse, SplatMeshShade, SplatViewOverlay, SplatViewRun, SplatViewOverlayFinish)


SPLAT_ADD_VALID_DEPTH = 0
SPLAT_ADD_NON_PRESENCE = 1
SPLAT_DENSIFY_CLONE = 0
SPLAT_DENSIFY_SPLIT = 1
SPLAT_LOSS_SPLATAM, SPLAT_LOSS_GS = 0, 1
SPLAT_ITER_SUMS = 32
SPLAT_ITER_SUM_COPIES = 64
SPLAT_POSE_STATE = 24
SPLAT_ITER_DCAM = 32
SPLAT_SLAB_ALIGN = 256
SPLAT_LAYOUT_SH, SPLAT_LAYOUT_LONG_LISTS, SPLAT_LAYOUT_BACKWARD, SPLAT_LAYOUT_SSIM, SPLAT_LAYOUT_OUTLIER = 1, 2, 4, 8, 16
SPLAT_LAYOUT_GROUPS, SPLAT_LAYOUT_TILE_ORDER, SPLAT_LAYOUT_RECS = 32, 64, 128
SPLAT_GRADS_UPSTREAM_SCALE, SPLAT_GRADS_POISON_IF_FLAGGED, SPLAT_GRADS_ACCUM_ZEROED = 1, 2, 4
SPLAT_LAYOUT_MAX_ARRAYS = 48
SPLAT_STATUS_INSTANCES, SPLAT_STATUS_OVERFLOW, SPLAT_STATUS_LONGEST, SPLAT_STATUS_STALE_HINT = 0, 1, 2, 3
SPLAT_REPORT_DROT, SPLAT_REPORT_DTRANS, SPLAT_REPORT_LOSS, SPLAT_REPORT_SUMS = 0, 4, 7, 8
SPLAT_REPORT_FLAG, SPLAT_REPORT_MEDIAN, SPLAT_REPORT_DEPTH_TERM, SPLAT_REPORT_IM_TERM = 12, 13, 14, 15
SPLAT_REPORT_STATUS, SPLAT_REPORT_FLAGGED, SPLAT_REPORT_SKIPPED = 16, 20, 21
SPLAT_EVAL_ROW, SPLAT_EVAL_LEVELS, SPLAT_EVAL_SUMS, SPLAT_EVAL_LAYOUT_MS_SSIM = 8, 5, 40, 1
SPLAT_NN_MAX_CELLS, SPLAT_NN_REDUCE_ROWS = 1 << 21, 256
SPLAT_MESH_COMPARE_ROWS, SPLAT_MESH_COMPARE_PARTIALS = 256, 6 * 256
SPLAT_ICP_STATE, SPLAT_ICP_ROWS, SPLAT_ICP_SUMS = 24, 256, 17      # (added within ABI 17: the ICP layer, csrc/icp.hip)
SPLAT_MESH_AREA_BITS, SPLAT_MESH_AREA_BAD = 40, 1 << 62            # (added within ABI 17: the mesh cleaning layer, csrc/meshclean.hip)
SPLAT_MESH_KEY_HIGHEST, SPLAT_MESH_KEY_LOWEST = 2 ** 31 - 1, -2 ** 31
SPLAT_MESH_SIMPLIFY_SUMS, SPLAT_MESH_SIMPLIFY_MEAN, SPLAT_MESH_SIMPLIFY_QUADRIC = 16, 0, 1      # (added within ABI 17: csrc/meshsimplify.hip)
SPLAT_MESH_SHADE_COLOR, SPLAT_MESH_SHADE_SHADED, SPLAT_MESH_SHADE_SHADED_COLOR, SPLAT_MESH_SHADE_NORMAL, SPLAT_MESH_SHADE_DEPTH = 0, 1, 2, 3, 4
SPLAT_ICP_ITERATION, SPLAT_ICP_STATUS, SPLAT_ICP_FITNESS, SPLAT_ICP_RMSE = 16, 17, 18, 19
SPLAT_ICP_PREV_FITNESS, SPLAT_ICP_PREV_RMSE, SPLAT_ICP_COUNT, SPLAT_ICP_POINTS = 20, 21, 22, 23
SPLAT_EVAL_PSNR, SPLAT_EVAL_DEPTH_RMSE, SPLAT_EVAL_DEPTH_L1, SPLAT_EVAL_MS_SSIM, SPLAT_EVAL_VALID, SPLAT_EVAL_FLAGGED, SPLAT_EVAL_HOLES = 0, 1, 2, 3, 4, 5, 6
SPLAT_VIEW_MAX_POINT_SIZE, SPLAT_VIEW_MAX_LINE_WIDTH, SPLAT_VIEW_FRUSTUM_SEGMENTS = 8, 4, 8      # (added within ABI 17: csrc/viewoverlay.hip)
SPLAT_EVAL_LPIPS, SPLAT_LPIPS_LAYERS, SPLAT_LPIPS_MIN_SIZE = 7, 5, 31      # (added within ABI 17: csrc/lpips.hip)


def lists_sorted_by_composite(max_list_hint: int) -> bool:
    """The library's test (splat_device.h): lists known to be at most this long are sorted by the composite kernel itself."""
    return 0 < max_list_hint and max_list_hint + max_list_hint // 4 <= 1024


# staged records handed from the forward to the backward composite (SplatState.tile_recs) pay where a tile's list is several
# 255-entry batches long and cost where it is one (profiles/r06_experiments.md 2): they are bound for lists longer than this
RECS_MIN_LIST = 400

EXPORTS = (
    "splat_error_string", "splat_abi_version", "splat_sizeof", "splat_num_tiles",
    "splat_preprocess_forward", "splat_bin_forward", "splat_render_forward", "splat_forward",
    "splat_render_backward", "splat_preprocess_backward", "splat_backward",
    "splat_mark_visible", "splat_same_geometry", "splat_time_kernel", "splat_debug_option", "splat_debug_stamps",
    "splat_iter_loss_backward", "splat_iter_adam_map", "splat_iter_adam_pose", "splat_iter_time_kernel",
    "splat_iter_tracking_step", "splat_iter_mapping_step", "splat_iter_finish", "splat_iter_fold_sums", "splat_iter_render", "splat_map_scratch_words", "splat_map_row_floats", "splat_map_add_new_gaussians", "splat_map_prune",
    "splat_iter_means2d_accumulate", "splat_map_densify_select", "splat_map_duplicate",
    "splat_workspace_bytes", "splat_state_layout", "splat_state_bind", "splat_iter_workspace_layout", "splat_iter_workspace_bind",
    "splat_iter_workspace_bytes",
    "splat_eval_workspace_layout", "splat_eval_workspace_bind", "splat_eval_metrics", "splat_iter_eval",
    "splat_frame_prepare", "splat_frame_ingest", "splat_frame_ingest_planes",
    "splat_view_camera", "splat_view_finish",
    "splat_view_run_segments", "splat_view_overlay_clear", "splat_view_points", "splat_view_segments", "splat_view_overlay_finish",
    "splat_iter_loss_backward_ex", "splat_iter_mapping_step_ex",
    "splat_tsdf_bytes", "splat_tsdf_reset", "splat_tsdf_integrate", "splat_tsdf_triangles", "splat_tsdf_vertices",
    "splat_tsdf_sparse_brick_shape", "splat_tsdf_sparse_bytes", "splat_tsdf_sparse_mark", "splat_tsdf_sparse_reset_slots",
    "splat_tsdf_sparse_integrate", "splat_tsdf_sparse_triangles", "splat_tsdf_sparse_vertices",
    "splat_tsdf_cubes", "splat_tsdf_sparse_cubes", "splat_tsdf_cubes_table",
    "splat_mesh_areas", "splat_mesh_sample", "splat_nn_cell_keys", "splat_nn_cell_starts", "splat_nn_query", "splat_nn_reduce",
    "splat_mesh_depth", "splat_mesh_seen", "splat_mesh_depth_compare",
    "splat_mesh_vertex_normals", "splat_mesh_visibility", "splat_mesh_shade",
    "splat_icp_transform", "splat_icp_accumulate", "splat_icp_solve",
    "splat_mesh_components", "splat_mesh_component_stats",
    "splat_mesh_simplify_keys", "splat_mesh_simplify_vertices", "splat_mesh_simplify_quadrics", "splat_mesh_simplify_place",
    "splat_mesh_simplify_faces",
    "splat_lpips_weight_floats", "splat_lpips_pack_floats", "splat_lpips_tap_size", "splat_lpips_workspace_layout", "splat_lpips_workspace_bind",
    "splat_lpips_pack", "splat_lpips_conv", "splat_lpips_planes", "splat_lpips_images",
)

_lib = None


def lib():
    """Load libsplat_hip.so (after torch, so that it binds to the HIP runtime
    torch already loaded) and type its entry points."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP rasterizer has not been built. "
            "Run `python -m splatam_amd.build` (needs hipcc); there is no CPU fallback.")
    import torch  # noqa: F401  (loads libamdhip64 first)
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise RuntimeError(f"{LIB_PATH} does not export {name}")
    L.splat_error_string.restype = C.c_char_p
    L.splat_error_string.argtypes = [C.c_int]
    L.splat_abi_version.restype = C.c_int
    L.splat_num_tiles.restype = C.c_size_t
    L.splat_num_tiles.argtypes = [C.c_int32, C.c_int32]
    cam, g, st, gr = C.POINTER(SplatCamera), C.POINTER(SplatGaussians), C.POINTER(SplatState), C.POINTER(SplatGrads)
    for name, args in (
        ("splat_preprocess_forward", [cam, g, st, _fp]),
        ("splat_bin_forward", [cam, g, st, _fp]),
        ("splat_render_forward", [cam, g, st, _fp, _fp, _fp]),
        ("splat_forward", [cam, g, st, _fp, _fp, _fp]),
        ("splat_render_backward", [cam, g, st, gr, _fp]),
        ("splat_preprocess_backward", [cam, g, st, gr, _fp]),
        ("splat_backward", [cam, g, st, gr, _fp]),
        ("splat_mark_visible", [C.c_int32, _fp, _fp, _fp, _fp]),
        ("splat_same_geometry", [C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
        ("splat_time_kernel", [C.c_int, C.c_int, cam, g, st, gr, _fp, _fp, _fp, C.POINTER(C.c_float)]),
    ):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    L.splat_iter_loss_backward.restype = C.c_int
    L.splat_iter_loss_backward.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatLossConfig),
                                           C.POINTER(SplatIterWorkspace), _fp]
    L.splat_iter_adam_map.restype = C.c_int
    L.splat_iter_adam_map.argtypes = [C.POINTER(SplatMap), C.POINTER(SplatAdamMap), _fp]
    L.splat_iter_adam_pose.restype = C.c_int
    L.splat_iter_adam_pose.argtypes = [C.POINTER(SplatMap), C.c_int32, _fp, _fp, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_float, _fp]
    L.splat_iter_time_kernel.restype = C.c_int
    L.splat_iter_time_kernel.argtypes = [C.c_int, C.c_int, cam, C.c_int32, C.POINTER(SplatIterWorkspace), _fp, C.POINTER(C.c_float)]
    L.splat_iter_tracking_step.restype = C.c_int
    L.splat_iter_tracking_step.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatLossConfig),
                                           C.POINTER(SplatIterWorkspace), C.POINTER(SplatPoseAdam), _fp]
    L.splat_iter_mapping_step.restype = C.c_int
    L.splat_iter_mapping_step.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatLossConfig),
                                          C.POINTER(SplatIterWorkspace), C.POINTER(SplatAdamMap), _fp]
    L.splat_iter_loss_backward_ex.restype = C.c_int
    L.splat_iter_loss_backward_ex.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatLossConfigEx),
                                              C.POINTER(SplatIterWorkspace), _fp]
    L.splat_iter_mapping_step_ex.restype = C.c_int
    L.splat_iter_mapping_step_ex.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatLossConfigEx),
                                             C.POINTER(SplatIterWorkspace), C.POINTER(SplatAdamMap), _fp]
    L.splat_iter_finish.restype = C.c_int
    L.splat_iter_finish.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatLossConfig),
                                    C.POINTER(SplatIterWorkspace), C.POINTER(SplatPoseAdam), _fp]
    L.splat_iter_fold_sums.restype = C.c_int
    L.splat_iter_fold_sums.argtypes = [_fp, _fp]
    L.splat_iter_render.restype = C.c_int
    L.splat_iter_render.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatIterWorkspace), _fp]
    L.splat_map_scratch_words.restype = C.c_size_t
    L.splat_map_scratch_words.argtypes = [C.c_int64]
    L.splat_map_row_floats.restype = C.c_int32
    L.splat_map_row_floats.argtypes = [C.POINTER(SplatMapStore)]
    L.splat_map_add_new_gaussians.restype = C.c_int
    L.splat_map_add_new_gaussians.argtypes = [C.POINTER(SplatMapStore), C.POINTER(SplatAddArgs), _fp]
    L.splat_map_prune.restype = C.c_int
    L.splat_map_prune.argtypes = [C.POINTER(SplatMapStore), C.POINTER(SplatPruneArgs), _fp]
    L.splat_iter_means2d_accumulate.restype = C.c_int
    L.splat_iter_means2d_accumulate.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatIterWorkspace), _fp, _fp, _fp, _fp]
    for name in ("splat_map_densify_select", "splat_map_duplicate"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SplatMapStore), C.POINTER(SplatDensifyArgs), _fp]
    info = C.POINTER(SplatArrayInfo)
    L.splat_workspace_bytes.restype = C.c_size_t
    L.splat_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    L.splat_state_layout.restype = C.c_int
    L.splat_state_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, info, C.c_int32, C.POINTER(C.c_size_t)]
    L.splat_state_bind.restype = C.c_int
    L.splat_state_bind.argtypes = [st, gr, _fp, info, C.c_int32, C.c_int32, C.c_int64]
    L.splat_iter_workspace_layout.restype = C.c_int
    L.splat_iter_workspace_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, info, C.c_int32, C.POINTER(C.c_size_t)]
    L.splat_iter_workspace_bind.restype = C.c_int
    L.splat_iter_workspace_bind.argtypes = [C.POINTER(SplatIterWorkspace), _fp, info, C.c_int32, C.c_int64, C.c_int32]
    L.splat_iter_workspace_bytes.restype = C.c_size_t
    L.splat_iter_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]
    L.splat_eval_workspace_layout.restype = C.c_int
    L.splat_eval_workspace_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, info, C.c_int32, C.POINTER(C.c_size_t)]
    L.splat_eval_workspace_bind.restype = C.c_int
    L.splat_eval_workspace_bind.argtypes = [C.POINTER(SplatEvalWorkspace), _fp, info, C.c_int32]
    L.splat_eval_metrics.restype = C.c_int
    L.splat_eval_metrics.argtypes = [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, C.POINTER(SplatEvalConfig), C.POINTER(SplatEvalWorkspace), _fp, _fp]
    L.splat_iter_eval.restype = C.c_int
    L.splat_iter_eval.argtypes = [cam, C.POINTER(SplatMap), C.POINTER(SplatFrameData), C.POINTER(SplatEvalConfig),
                                  C.POINTER(SplatIterWorkspace), C.POINTER(SplatEvalWorkspace), _fp, _fp]
    L.splat_frame_prepare.restype = C.c_int
    L.splat_frame_prepare.argtypes = [C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp]
    L.splat_frame_ingest.restype = C.c_int
    L.splat_frame_ingest.argtypes = [C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, C.c_double, C.c_int32, C.c_int32, _fp, _fp, _fp]
    L.splat_frame_ingest_planes.restype = C.c_int
    L.splat_frame_ingest_planes.argtypes = [C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                            _fp, _fp, _fp]
    for name in ("splat_view_camera", "splat_view_finish"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SplatViewArgs), _fp]
    overlay = C.POINTER(SplatViewOverlay)
    for name, args in (("splat_view_run_segments", [C.POINTER(SplatViewRun), _fp]), ("splat_view_overlay_clear", [overlay, _fp]),
                       ("splat_view_points", [overlay, _fp, C.c_int32, C.c_int32, _fp]),
                       ("splat_view_segments", [overlay, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
                       ("splat_view_overlay_finish", [overlay, C.POINTER(SplatViewOverlayFinish), _fp])):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    vol =C.POINTER(SplatTsdfVolume)
    L.splat_tsdf_bytes.restype = C.c_size_t
    L.splat_tsdf_bytes.argtypes = [vol]
    L.splat_tsdf_reset.restype = C.c_int
    L.splat_tsdf_reset.argtypes = [vol, _fp]
    L.splat_tsdf_integrate.restype = C.c_int
    L.splat_tsdf_integrate.argtypes = [vol, C.POINTER(SplatTsdfView), _fp]
    L.splat_tsdf_triangles.restype = C.c_int
    L.splat_tsdf_triangles.argtypes = [vol, C.c_float, _fp, C.c_int64, _fp, _fp]
    L.splat_tsdf_cubes.restype = C.c_int
    L.splat_tsdf_cubes.argtypes = [vol, C.c_float, _fp, C.c_int64, _fp, _fp]
    L.splat_tsdf_cubes_table.restype = C.c_int
    L.splat_tsdf_cubes_table.argtypes = [_fp]
    L.splat_tsdf_vertices.restype = C.c_int
    L.splat_tsdf_vertices.argtypes = [vol, _fp, C.c_int64, _fp, _fp, _fp]
    sparse = C.POINTER(SplatTsdfSparse)
    L.splat_tsdf_sparse_brick_shape.restype = C.c_int
    L.splat_tsdf_sparse_brick_shape.argtypes = [C.c_int, C.POINTER(C.c_int32)]
    L.splat_tsdf_sparse_bytes.restype = C.c_size_t
    L.splat_tsdf_sparse_bytes.argtypes = [sparse]
    for name, args in (("splat_tsdf_sparse_mark", [sparse, C.POINTER(SplatTsdfView), _fp, _fp]),
                       ("splat_tsdf_sparse_reset_slots", [sparse, C.c_int64, C.c_int64, _fp]),
                       ("splat_tsdf_sparse_integrate", [sparse, C.POINTER(SplatTsdfView), _fp]),
                       ("splat_tsdf_sparse_triangles", [sparse, C.c_float, _fp, C.c_int64, _fp, _fp]),
                       ("splat_tsdf_sparse_cubes", [sparse, C.c_float, _fp, C.c_int64, _fp, _fp]),
                       ("splat_tsdf_sparse_vertices", [sparse, _fp, C.c_int64, _fp, _fp, _fp])):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    nn = C.POINTER(SplatNnGrid)
    for name, args in (
        ("splat_mesh_areas", [_fp, C.c_int32, _fp, C.c_int32, _fp, _fp]),
        ("splat_mesh_sample", [_fp, C.c_int32, _fp, C.c_int32, _fp, C.c_uint64, C.c_int64, _fp, _fp, _fp]),
        ("splat_nn_cell_keys", [nn, _fp, C.c_int64, _fp, _fp]),
        ("splat_nn_cell_starts", [nn, _fp, _fp, _fp, _fp, _fp, _fp]),
        ("splat_nn_query", [nn, _fp, _fp, C.c_int64, _fp, _fp, _fp, _fp]),
        ("splat_nn_reduce", [_fp, C.c_int64, C.c_double, _fp, _fp, _fp]),
    ):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    for name, args in (
        ("splat_mesh_depth", [_fp, C.c_int32, _fp, C.c_int32, C.POINTER(SplatMeshView), _fp, _fp]),
        ("splat_mesh_seen", [_fp, C.c_int32, C.POINTER(SplatMeshView), _fp, C.c_int32, C.c_int32, _fp, C.c_float, _fp, _fp]),
        ("splat_mesh_depth_compare", [_fp, _fp, C.c_int64, _fp, _fp, _fp]),
        ("splat_mesh_vertex_normals", [_fp, C.c_int32, _fp, C.c_int32, _fp, _fp, _fp]),
        ("splat_mesh_visibility", [_fp, C.c_int32, _fp, C.c_int32, C.POINTER(SplatMeshView), _fp, _fp]),
        ("splat_mesh_shade", [_fp, C.c_int32, _fp, C.c_int32, _fp, _fp, C.POINTER(SplatMeshView), _fp, C.POINTER(SplatMeshShade), _fp, _fp, _fp,
                              _fp, _fp]),
    ):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    for name, args in (
        ("splat_mesh_components", [_fp, C.c_int32, C.c_int32, _fp, _fp]),
        ("splat_mesh_component_stats", [_fp, C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
        ("splat_mesh_simplify_keys", [_fp, C.c_int32, C.c_double, _fp, _fp]),
        ("splat_mesh_simplify_vertices", [_fp, _fp, C.c_int32, _fp, C.c_double, _fp, _fp, _fp]),
        ("splat_mesh_simplify_quadrics", [_fp, C.c_int32, _fp, C.c_int32, _fp, C.c_double, _fp, _fp, _fp]),
        ("splat_mesh_simplify_place", [_fp, _fp, _fp, C.c_int32, C.c_double, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp]),
        ("splat_mesh_simplify_faces", [_fp, C.c_int32, C.c_int32, _fp, _fp, _fp]),
    ):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    for name, args in (
        ("splat_icp_transform", [_fp, C.c_int64, _fp, _fp, _fp]),
        ("splat_icp_accumulate", [_fp, _fp, C.c_int64, _fp, _fp, C.c_int64, C.c_double, C.POINTER(C.c_double), _fp, _fp, _fp]),
        ("splat_icp_solve", [_fp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double), _fp, _fp, _fp]),
    ):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    lp = C.POINTER(SplatLpipsWorkspace)
    for name in ("splat_lpips_weight_floats", "splat_lpips_pack_floats"):
        f = getattr(L, name)
        f.restype = C.c_size_t
        f.argtypes = []
    L.splat_lpips_tap_size.restype = C.c_int32
    L.splat_lpips_tap_size.argtypes = [C.c_int32, C.c_int32]
    for name, args in (
        ("splat_lpips_workspace_layout", [C.c_int32, C.c_int32, info, C.c_int32, C.POINTER(C.c_size_t)]),
        ("splat_lpips_workspace_bind", [lp, _fp, info, C.c_int32, C.c_int32, C.c_int32]),
        ("splat_lpips_pack", [_fp, _fp, _fp]),
        ("splat_lpips_conv", [C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp]),
        ("splat_lpips_planes", [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, C.c_float, C.c_int32, _fp, lp, _fp, _fp]),
        ("splat_lpips_images", [C.c_int32, C.c_int32, _fp, _fp, _fp, lp, _fp, _fp]),
    ):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    L.splat_debug_option.restype = C.c_int
    L.splat_debug_option.argtypes = [C.c_int, C.c_int]
    L.splat_debug_stamps.restype = C.c_int
    L.splat_debug_stamps.argtypes = [_fp]
    if hasattr(L, "splat_selftest"):
        L.splat_selftest.restype = C.c_int
        L.splat_selftest.argtypes = [C.c_int, _fp, _fp, C.c_int, _fp]
    if L.splat_abi_version() != ABI_VERSION:
        raise RuntimeError(f"ABI mismatch: library {L.splat_abi_version()} vs binding {ABI_VERSION}")
    L.splat_sizeof.restype = C.c_size_t
    L.splat_sizeof.argtypes = [C.c_char_p]
    for cls in MIRRORED_STRUCTS:        # the hand-written mirrors against the compiled layout
        if L.splat_sizeof(cls.__name__.encode()) != C.sizeof(cls):
            raise RuntimeError(f"struct layout mismatch: {cls.__name__} is {L.splat_sizeof(cls.__name__.encode())} bytes in the library, "
                               f"{C.sizeof(cls)} in the binding")
    _lib = L
    return L


class Layout:
    """A scratch layout as the library describes it (include/splat_hip.h, "Scratch layouts"): ``arrays`` (the C table, for
    splat_*_bind), ``n``, ``total`` bytes of the slab, and by field name ``bytes`` / ``offset`` / ``zero_init``."""

    def __init__(self, arrays, n, total):
        self.arrays, self.n, self.total = arrays, n, total
        self.names = [arrays[i].name.decode() for i in range(n)]
        self.bytes = {self.names[i]: int(arrays[i].bytes) for i in range(n)}
        self.offset = {self.names[i]: int(arrays[i].offset) for i in range(n)}
        self.zero_init = {self.names[i]: bool(arrays[i].zero_init) for i in range(n)}


_state_layouts: dict = {}


def state_layout(P, width, height, sub_bins, capacity, flags):
    """(memoised: the drop-in path asks twice per rasterizer call, and a layout is a pure function of its arguments)"""
    key = (P, width, height, sub_bins, capacity, flags)
    hit = _state_layouts.get(key)
    if hit is None:
        if len(_state_layouts) > 256:
            _state_layouts.clear()
        hit = _state_layouts[key] = _state_layout(*key)
    return hit


def _state_layout(P, width, height, sub_bins, capacity, flags):
    arrays = (SplatArrayInfo * SPLAT_LAYOUT_MAX_ARRAYS)()
    total = C.c_size_t(0)
    n = lib().splat_state_layout(P, width, height, sub_bins, capacity, flags, arrays, SPLAT_LAYOUT_MAX_ARRAYS, C.byref(total))
    if n < 0 or n > SPLAT_LAYOUT_MAX_ARRAYS:
        raise RuntimeError(f"splat_state_layout({P}, {width}, {height}, {sub_bins}, {capacity}, {flags}) failed: {n}")
    return Layout(arrays, n, int(total.value))


def iter_workspace_layout(P, width, height, capacity, group_stride, flags):
    arrays = (SplatArrayInfo * SPLAT_LAYOUT_MAX_ARRAYS)()
    total = C.c_size_t(0)
    n = lib().splat_iter_workspace_layout(P, width, height, capacity, group_stride, flags, arrays, SPLAT_LAYOUT_MAX_ARRAYS, C.byref(total))
    if n < 0 or n > SPLAT_LAYOUT_MAX_ARRAYS:
        raise RuntimeError(f"splat_iter_workspace_layout({P}, {width}, {height}, {capacity}, {group_stride}, {flags}) failed: {n}")
    return Layout(arrays, n, int(total.value))


def eval_workspace_layout(width, height, ms_ssim=True):
    """The evaluation's scratch (SplatEvalWorkspace): ``pyramid`` (with MS-SSIM) and ``sums``.  Raises for a frame MS-SSIM cannot
    take (min(width, height) <= 160: four poolings must leave room for the 11-tap window)."""
    arrays = (SplatArrayInfo * 4)()
    total = C.c_size_t(0)
    n = lib().splat_eval_workspace_layout(int(width), int(height), SPLAT_EVAL_LAYOUT_MS_SSIM if ms_ssim else 0, arrays, 4, C.byref(total))
    if n < 0 or n > 4:
        raise RuntimeError(f"splat_eval_workspace_layout({width}, {height}, ms_ssim={bool(ms_ssim)}) failed: "
                           f"{lib().splat_error_string(-n).decode()} (MS-SSIM needs min(width, height) > 160)")
    return Layout(arrays, n, int(total.value))


def lpips_workspace_layout(width, height):
    """LPIPS' scratch for an image size (SplatLpipsWorkspace): the transformed input, the five taps, the two pooled maps and the
    distance's partials (the packed network is size-independent and lives beside the workspaces).  Raises for an extent under SPLAT_LPIPS_MIN_SIZE."""
    arrays = (SplatArrayInfo * 16)()
    total = C.c_size_t(0)
    n = lib().splat_lpips_workspace_layout(int(width), int(height), arrays, 16, C.byref(total))
    if n < 0 or n > 16:
        raise RuntimeError(f"splat_lpips_workspace_layout({width}, {height}) failed: LPIPS needs images of at least "
                           f"{SPLAT_LPIPS_MIN_SIZE} x {SPLAT_LPIPS_MIN_SIZE} pixels")
    return Layout(arrays, n, int(total.value))


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib().splat_error_string(rc).decode()} (code {rc})")
