"""ctypes binding of libfreesplat_hip.so (C ABI: the headers under include/, one record each in HEADERS, EXTENSION_HEADERS or
ADDON_HEADERS below).

The product path has NO fallback: if the HIP library is missing or a call fails this module
raises.  `build()` compiles the library in-tree with hipcc for gfx950.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple

_PKG = os.path.dirname(os.path.abspath(__file__))
# FREESPLAT_LIB: an alternative build of the same library (A/B measurements of kernel variants inside one GPU session)
LIB_PATH = os.environ.get("FREESPLAT_LIB") or os.path.join(_PKG, "libfreesplat_hip.so")
_lib = None


class FreeSplatHipError(RuntimeError):
    pass


class RasterDims(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("sh_degree", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("flags", C.c_int32)]


ABI_VERSION = 9
LOSS_API_VERSION = 1
OPTIM_API_VERSION = 1
DENSITY_API_VERSION = 1
DEPTHLOSS_API_VERSION = 1
NORMALS_API_VERSION = 1
EXPOSURE_API_VERSION = 1
MVDEPTH_API_VERSION = 1
TRANSFORM_API_VERSION = 1
POSE_API_VERSION = 1
TSDF_API_VERSION = 1
RAYCAST_API_VERSION = 1
GEOMETRY_API_VERSION = 1

RASTER_TILE_CULL = 1
RASTER_SH_FP16 = 2
RASTER_SH_CHANNEL_MAJOR = 4
RASTER_COV_FULL = 8
RASTER_FAST_EXP = 16
RASTER_NO_BACKWARD_STATE = 32
RASTER_DETERMINISTIC = 64
RASTER_SCALE_ROT = 128

SSIM_SKIMAGE = 1
SSIM_3DGS = 2

DEPTH_LOSS_LOG_L1 = 1
DEPTH_LOSS_L1 = 2
DEPTH_LOSS_MAX_SCALES = 6

MVDEPTH_MAX_SOURCES = 16

TRANSFORM_TABLE_FLOATS = 100
TRANSFORM_S, TRANSFORM_R, TRANSFORM_T, TRANSFORM_Q, TRANSFORM_D1, TRANSFORM_D2, TRANSFORM_D3 = 0, 1, 10, 13, 17, 26, 51
TRANSFORM_SH_CHANNEL_MAJOR = 1
TRANSFORM_SH_TRANSPOSE = 2
TRANSFORM_QUAT_XYZW = 4
TRANSFORM_COV_FULL = 8

SIM3_MAX_ROWS = 64
SIM3_TANGENT_DIM = 7
SIM3_SH_GENERATOR_DOUBLES = 83

TSDF_MAX_VIEWS = 64
TSDF_BRICK = (32, 8, 4)      # grid points (x, y, z) one workgroup of fs_tsdf_integrate owns
TSDF_MESH_RUN = 256          # consecutive cubes one workgroup of the extraction owns
TSDF_NO_BRICK_SKIP = 1

RAYCAST_TILE = 16            # pixels (x and y) one workgroup of fs_tsdf_raycast owns
RAYCAST_MAX_REFINE = 32
RAYCAST_MAX_STEPS = 1 << 20

NN_MAX_SIDE = 1024           # cells per side of a nearest-neighbour grid
NN_MAX_CELLS = 1 << 24
NN_MAX_THRESHOLDS = 8
NN_SUM_FIELDS = 3 + NN_MAX_THRESHOLDS
NN_SUM_FINITE, NN_SUM_WITHIN, NN_SUM_DIST, NN_SUM_TAU = 0, 1, 2, 3


def build(force: bool = False) -> str:
    """Compile every HIP translation unit under csrc/ for gfx950 into libfreesplat_hip.so."""
    csrc = os.path.join(_PKG, "csrc")
    args = ["make", "-C", csrc, "-j8"]
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_VP = C.c_void_p

# the tables: name -> (restype, argtypes)
SIGNATURES = {
    "fs_version": (C.c_char_p, []),
    "fs_abi_version": (C.c_int, []),
    "fs_last_error": (C.c_char_p, []),
    "fs_profile_enable": (C.c_int, [C.c_int]),
    "fs_profile_collect": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "fs_profile_stage_name": (C.c_char_p, [C.c_int]),
    "fs_raster_buffer_sizes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_size_t)]),
    "fs_raster_forward": (C.c_int, [C.POINTER(RasterDims)] + [_VP] * 15 + [C.c_int64] + [_VP] * 6),
    "fs_raster_backward": (C.c_int, [C.POINTER(RasterDims)] + [_VP] * 24 + [C.c_int, _VP]),
    "fs_raster_backward_alpha": (C.c_int, [C.POINTER(RasterDims)] + [_VP] * 25 + [C.c_int, _VP]),
    "fs_raster_cov3d_from_scale_rot": (C.c_int, [C.c_int32, _VP, _VP, _VP]),
    "fs_raster_backward_scratch_bytes": (C.c_size_t, [C.POINTER(RasterDims), C.c_int32, C.c_int32, C.c_int64]),
    "fs_cost_volume_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "fs_cost_volume_forward": (C.c_int, [C.c_int32] * 6 + [_VP] * 6 + [C.c_int64] * 3 + [_VP] * 9),
    "fs_cost_volume_forward_layout": (C.c_int, [C.c_int32] * 6 + [_VP] * 6 + [C.c_int64] * 3 + [_VP] * 8 + [C.c_int32, _VP]),
    "fs_cost_volume_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 6),
    "fs_cost_volume_backward_workspace_bytes_for": (C.c_size_t, [C.c_int32] * 6 + [C.c_int64]),
    "fs_cost_volume_backward": (C.c_int, [C.c_int32] * 6 + [_VP] * 6 + [C.c_int64] * 3 + [_VP] * 16),
    "fs_cost_volume_depth_planes": (C.c_int, [C.c_int32] + [_VP] * 5),
    "fs_cost_volume_saved_bytes": (C.c_size_t, [C.c_int32] * 5),
    "fs_cost_volume_forward_train": (C.c_int, [C.c_int32] * 6 + [_VP] * 6 + [C.c_int64] * 3 + [_VP] * 10),
    "fs_cost_volume_backward_train": (C.c_int, [C.c_int32] * 6 + [_VP] * 6 + [C.c_int64] * 3 + [_VP] * 17),
    "fs_cost_volume_backward_det_bytes": (C.c_size_t, [C.c_int32] * 6),
    "fs_cost_volume_backward_det": (C.c_int, [C.c_int32] * 6 + [_VP] * 6 + [C.c_int64] * 3 + [_VP] * 18),
    "fs_unproject_forward": (C.c_int, [C.c_int32] * 3 + [_VP] * 5),
    "fs_unproject_backward": (C.c_int, [C.c_int32] * 3 + [_VP] * 5),
    "fs_gaussian_head_forward": (C.c_int, [C.c_int64] + [_VP] * 4 + [C.c_int64, _VP, C.c_float, C.c_float] + [_VP] * 5),
    "fs_gaussian_head_backward": (C.c_int, [C.c_int64] + [_VP] * 4 + [C.c_int64, _VP, C.c_float, C.c_float] + [_VP] * 8),
    "fs_gaussian_head_forward_sh": (C.c_int, [C.c_int64, C.c_int32] + [_VP] * 4 + [C.c_int64, _VP, C.c_float, C.c_float]
                                    + [_VP] * 5),
    "fs_gaussian_head_backward_sh": (C.c_int, [C.c_int64, C.c_int32] + [_VP] * 4 + [C.c_int64, _VP, C.c_float, C.c_float]
                                     + [_VP] * 8),
    "fs_latents_pack_forward": (C.c_int, [C.c_int32, C.c_int64, C.c_int32] + [_VP] * 5),
    "fs_latents_pack_backward": (C.c_int, [C.c_int32, C.c_int64, C.c_int32] + [_VP] * 5),
    "fs_ptf_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_ptf_match": (C.c_int, [C.c_int32] * 3 + [_VP] * 4 + [C.c_float] + [_VP] * 7),
    "fs_ptf_gru_inputs": (C.c_int, [C.c_int32] + [_VP] * 10),
    "fs_ptf_write_state": (C.c_int, [C.c_int32] * 3 + [_VP] * 24),
    "fs_ptf_gru_table_rows": (C.c_int32, []),
    "fs_ptf_gru_forward": (C.c_int, [C.c_int32] + [_VP] * 4),
    "fs_ptf_gru_table_t_rows": (C.c_int32, []),
    "fs_ptf_gru_stream_rows": (C.c_int32, []),
    "fs_ptf_gru_stream_layout": (C.c_int32, []),
    "fs_ptf_gru_table_layout": (C.c_int32, []),
    "fs_ptf_gru_stream_chunk_rows": (C.c_int32, []),
    "fs_ptf_gru_side_cols": (C.c_int32, []),
    "fs_ptf_gru_backward": (C.c_int, [C.c_int32] + [_VP] * 7),
    "fs_ptf_gru_backward_saved": (C.c_int, [C.c_int32] + [_VP] * 7),
    "fs_ptf_gru_act_cols": (C.c_int32, []),
    "fs_ptf_gru_stream_t_rows": (C.c_int32, []),
    "fs_ptf_gru_grad_floats": (C.c_int32, []),
    "fs_ptf_gru_weight_grads_bytes": (C.c_size_t, [C.c_int32]),
    "fs_ptf_gru_weight_grads": (C.c_int, [C.c_int32] + [_VP] * 5),
    "fs_raster_forward_views": (C.c_int, [C.POINTER(RasterDims), C.c_int32] + [_VP] * 15 + [C.POINTER(C.c_size_t), C.c_int64]
                                + [_VP] * 5 + [C.c_int32, C.POINTER(C.c_void_p), _VP]),
    "fs_raster_backward_views": (C.c_int, [C.POINTER(RasterDims), C.c_int32] + [_VP] * 15 + [C.POINTER(C.c_size_t)] + [_VP] * 9
                                 + [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), _VP]),
    "fs_raster_backward_views_rows": (C.c_int, [C.POINTER(RasterDims), C.c_int32] + [_VP] * 15 + [C.POINTER(C.c_size_t)] + [_VP] * 9
                                      + [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), _VP, C.c_int32, C.c_int32, C.c_int32]),
    "fs_raster_backward_views_alpha": (C.c_int, [C.POINTER(RasterDims), C.c_int32] + [_VP] * 15 + [C.POINTER(C.c_size_t)]
                                       + [_VP] * 10 + [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), _VP]),
    "fs_raster_backward_views_rows_alpha": (C.c_int, [C.POINTER(RasterDims), C.c_int32] + [_VP] * 15 + [C.POINTER(C.c_size_t)]
                                            + [_VP] * 10 + [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), _VP, C.c_int32,
                                                            C.c_int32, C.c_int32]),
    "fs_ptf_fold_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_ptf_fold_step": (C.c_int, [C.c_int32, _VP, C.c_int32, C.c_int32] + [_VP] * 14 + [C.c_float] + [_VP] * 10),
    "fs_ptf_fold_step_save": (C.c_int, [C.c_int32, _VP, C.c_int32, C.c_int32] + [_VP] * 14 + [C.c_float] + [_VP] * 13),
    "fs_ptf_fold_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_ptf_fold": (C.c_int, [C.c_int32] * 3 + [_VP] * 8 + [C.c_float] + [_VP] * 2 + [C.POINTER(C.c_void_p)] * 2 + [_VP] * 2),
    "fs_ptf_cameras": (C.c_int, [C.c_int32] * 3 + [_VP] * 5),
    "fs_ptf_fold_step_lists": (C.c_int, [C.c_int32] * 3 + [_VP, C.POINTER(C.c_void_p)]),
    "fs_ptf_write_state_backward": (C.c_int, [C.c_int32] * 3 + [_VP] * 12 + [C.POINTER(C.c_void_p)] * 2 + [_VP] * 6),
    "fs_ptf_gru_inputs_backward": (C.c_int, [C.c_int32] + [_VP] * 14),
    "fs_ptf_backward_det_bytes": (C.c_size_t, [C.c_int32] * 2),
    "fs_ptf_write_state_backward_det": (C.c_int, [C.c_int32] * 3 + [_VP] * 12 + [C.POINTER(C.c_void_p)] * 2 + [_VP] * 5
                                        + [C.c_int32, _VP, _VP]),
    "fs_ptf_gru_inputs_backward_det": (C.c_int, [C.c_int32] + [_VP] * 13 + [C.c_int32, _VP, _VP]),
    "fs_frame_views": (C.c_int, [C.c_int32] + [_VP] * 4 + [C.c_int32] + [_VP] * 6),
    "fs_invert_4x4": (C.c_int, [C.c_int32, _VP, _VP, _VP]),
    "fs_depth_tail_forward": (C.c_int, [C.c_int32] * 4 + [_VP] * 2 + [C.c_int32] + [_VP] * 7),
    "fs_depth_tail_backward": (C.c_int, [C.c_int32] * 4 + [_VP] * 2 + [C.c_int32] + [_VP] * 13),
    "fs_depth_tail_backward_det": (C.c_int, [C.c_int32] * 4 + [_VP] * 2 + [C.c_int32] + [_VP] * 11),
    "fs_image_metrics_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "fs_image_metrics": (C.c_int, [C.c_int32] * 4 + [_VP] * 7),
    "fs_depth_metrics_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "fs_depth_metrics": (C.c_int, [C.c_int32, C.c_int64, _VP, _VP, C.c_float, _VP, _VP, _VP]),
    "fs_lpips_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "fs_lpips_saved_bytes": (C.c_size_t, [C.c_int32] * 4),
    "fs_lpips_layer_forward": (C.c_int, [_VP] * 3 + [C.c_int32] * 4 + [_VP] * 4),
    "fs_lpips_layer_backward": (C.c_int, [_VP] * 5 + [C.c_int32] * 4 + [_VP] * 3),
    "fs_lpips_prepare_forward": (C.c_int, [_VP] * 4 + [C.c_int32] * 5 + [_VP] * 2),
    "fs_lpips_prepare_backward": (C.c_int, [_VP] * 2 + [C.c_int32] * 5 + [_VP] * 3),
    "fs_skip_latents_saved_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_skip_latents_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_skip_latents_forward": (C.c_int, [C.c_int32] * 6 + [_VP] * 8),
    "fs_skip_latents_backward": (C.c_int, [C.c_int32] * 6 + [_VP] * 9),
    "fs_raster_scratch_slots": (C.c_int, [C.c_int32, C.c_int32]),
    "fs_raster_tile_ranges": (_VP, [_VP, C.c_int32, C.c_int32]),
    "fs_raster_point_list": (_VP, [_VP, C.c_int32, C.c_int32]),
    "fs_raster_geom_records": (_VP, [_VP]),
    "fs_raster_final_T": (_VP, [_VP]),
    "fs_raster_n_contrib": (_VP, [_VP, C.c_int32, C.c_int32]),
}

LOSS_SIGNATURES = {
    "fs_loss_api_version": (C.c_int, []),
    "fs_ssim_loss_saved_bytes": (C.c_size_t, [C.c_int32] * 5),
    "fs_ssim_loss_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "fs_ssim_loss_forward": (C.c_int, [C.c_int32] * 5 + [_VP] * 7),
    "fs_ssim_loss_backward": (C.c_int, [C.c_int32] * 5 + [_VP] * 8),
}


_PP = C.POINTER(C.c_void_p)
OPTIM_SIGNATURES = {
    "fs_optim_api_version": (C.c_int, []),
    "fs_gaussian_activate": (C.c_int, [C.c_int32] + [_VP] * 5),
    "fs_gaussian_adam_step": (C.c_int, [C.c_int32, C.c_int32] + [_PP] * 4 + [_VP] * 3 + [C.c_double] * 3 + [_VP] * 3),
}

DENSITY_SIGNATURES = {
    "fs_density_api_version": (C.c_int, []),
    "fs_density_accumulate": (C.c_int, [C.c_int32] + [_VP] * 6),
    "fs_density_plan_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "fs_density_plan": (C.c_int, [C.c_int32] + [_VP] * 5 + [C.c_float] * 6 + [_VP] * 6),
    "fs_density_apply": (C.c_int, [C.c_int32] * 3 + [_VP] + [_PP] * 6 + [_VP] * 2 + [C.c_uint32, _VP]),
    "fs_density_reset_opacity": (C.c_int, [C.c_int32, C.c_double] + [_VP] * 5),
}

DEPTHLOSS_SIGNATURES = {
    "fs_depthloss_api_version": (C.c_int, []),
    "fs_depth_loss_saved_bytes": (C.c_size_t, [C.c_int32] * 4),
    "fs_depth_loss_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "fs_depth_loss_forward": (C.c_int, [C.c_int32] * 5 + [_VP] * 3 + [C.c_float] * 3 + [_VP] * 7),
    "fs_depth_loss_backward": (C.c_int, [C.c_int32] * 5 + [_VP] * 3 + [C.c_float] * 3 + [_VP] * 7),
}

NORMALS_SIGNATURES = {
    "fs_normals_api_version": (C.c_int, []),
    "fs_normals_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_depth_normals_forward": (C.c_int, [C.c_int32] * 3 + [_VP] * 3 + [C.c_float] * 4 + [_VP] * 2),
    "fs_depth_normals_backward": (C.c_int, [C.c_int32] * 3 + [_VP] * 3 + [C.c_float] * 4 + [_VP] * 4),
    "fs_normals_loss_forward": (C.c_int, [C.c_int32] * 3 + [_VP] * 5 + [C.c_float] * 4 + [_VP] * 4),
    "fs_normals_loss_backward": (C.c_int, [C.c_int32] * 3 + [_VP] * 5 + [C.c_float] * 4 + [_VP] * 4),
}

EXPOSURE_SIGNATURES = {
    "fs_exposure_api_version": (C.c_int, []),
    "fs_exposure_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_exposure_apply_forward": (C.c_int, [C.c_int32] * 4 + [_VP] * 5),
    "fs_exposure_apply_backward": (C.c_int, [C.c_int32] * 4 + [_VP] * 8),
    "fs_exposure_fit": (C.c_int, [C.c_int32] * 4 + [_VP] * 4 + [C.c_double] + [_VP] * 5),
}

MVDEPTH_SIGNATURES = {
    "fs_mvdepth_api_version": (C.c_int, []),
    "fs_mvdepth_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "fs_mv_depth_forward": (C.c_int, [C.c_int32] * 7 + [_VP] * 6 + [C.c_float] * 4 + [_VP] * 5),
    "fs_mv_depth_backward": (C.c_int, [C.c_int32] * 7 + [_VP] * 6 + [C.c_float] * 4 + [_VP] * 4),
    "fs_si_depth_forward": (C.c_int, [C.c_int32] * 3 + [_VP] * 3 + [C.c_float] * 3 + [_VP] * 5),
    "fs_si_depth_backward": (C.c_int, [C.c_int32] * 3 + [_VP] * 3 + [C.c_float] * 3 + [_VP] * 5),
}

TRANSFORM_SIGNATURES = {
    "fs_transform_api_version": (C.c_int, []),
    "fs_transform_prepare": (C.c_int, [C.c_int32] + [_VP] * 3),
    "fs_sh_rotate": (C.c_int, [C.c_int32] * 4 + [_VP] * 5),
    "fs_gaussians_transform_forward": (C.c_int, [C.c_int32] * 4 + [_VP] * 13),
    "fs_gaussians_transform_backward": (C.c_int, [C.c_int32] * 4 + [_VP] * 13),
}

POSE_SIGNATURES = {
    "fs_pose_api_version": (C.c_int, []),
    "fs_sim3_tangent_scratch_bytes": (C.c_size_t, [C.c_int32] * 2),
    "fs_sim3_sh_generators": (C.c_int, [C.POINTER(C.c_double)]),
    "fs_sim3_tangent": (C.c_int, [C.c_int32] * 4 + [_VP] * 13 + [C.c_size_t, _VP]),
}

TSDF_SIGNATURES = {
    "fs_tsdf_api_version": (C.c_int, []),
    "fs_tsdf_integrate": (C.c_int, [C.c_int32] * 3 + [C.c_float] * 6 + [_VP] * 3 + [C.c_int32] * 3 + [_VP] * 5 + [C.c_float] * 5
                          + [C.c_int32, _VP]),
    "fs_tsdf_mt_table": (C.c_int, [C.POINTER(C.c_uint8)]),
    "fs_tsdf_mesh_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "fs_tsdf_mesh_plan": (C.c_int, [C.c_int32] * 3 + [_VP] * 2 + [C.c_float] + [_VP] * 3),
    "fs_tsdf_mesh_emit": (C.c_int, [C.c_int32] * 3 + [C.c_float] * 4 + [_VP] * 3 + [C.c_float, _VP, C.c_int64] + [_VP] * 3),
}

RAYCAST_SIGNATURES = {
    "fs_raycast_api_version": (C.c_int, []),
    "fs_tsdf_raycast": (C.c_int, [C.c_int32] * 3 + [C.c_float] * 5 + [_VP] * 3 + [C.c_int32] * 3 + [_VP] * 2 + [C.c_float] * 5
                        + [C.c_int32] * 2 + [_VP] * 5),
}

GEOMETRY_SIGNATURES = {
    "fs_geometry_api_version": (C.c_int, []),
    "fs_nn_grid_keys": (C.c_int, [C.c_int32, _VP] + [C.c_float] * 4 + [C.c_int32] * 3 + [_VP, _VP]),
    "fs_nn_grid_gather": (C.c_int, [C.c_int32] + [_VP] * 4),
    "fs_nn_query_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "fs_nn_query": (C.c_int, [C.c_int32, _VP, _VP, C.c_int32, _VP, _VP] + [C.c_float] * 4 + [C.c_int32] * 3
                    + [C.c_float, C.c_int32, C.POINTER(C.c_float)] + [_VP] * 5),
}


class Header(NamedTuple):
    file: str          # under include/
    macro: str         # the header's revision macro
    version_fn: str    # the entry point that returns the library's value of it
    revision: int      # what this binding expects
    label: str         # how lib()'s mismatch message names it
    signatures: dict


# One record per header under include/ and nothing else to keep in step: a table lists every symbol its header declares and
# no other table's, and lib() binds and checks whatever is listed here (tests/test_abi.py holds every record to its header
# and to the built library).
HEADERS = (
    Header("freesplat_amd.h", "FS_ABI_VERSION", "fs_abi_version", ABI_VERSION, "ABI", SIGNATURES),
    Header("freesplat_amd_loss.h", "FS_LOSS_API_VERSION", "fs_loss_api_version", LOSS_API_VERSION, "loss API", LOSS_SIGNATURES),
    Header("freesplat_amd_optim.h", "FS_OPTIM_API_VERSION", "fs_optim_api_version", OPTIM_API_VERSION, "optimizer API",
           OPTIM_SIGNATURES),
    Header("freesplat_amd_density.h", "FS_DENSITY_API_VERSION", "fs_density_api_version", DENSITY_API_VERSION, "density API",
           DENSITY_SIGNATURES),
    Header("freesplat_amd_depthloss.h", "FS_DEPTHLOSS_API_VERSION", "fs_depthloss_api_version", DEPTHLOSS_API_VERSION,
           "depth-loss API", DEPTHLOSS_SIGNATURES),
    Header("freesplat_amd_normals.h", "FS_NORMALS_API_VERSION", "fs_normals_api_version", NORMALS_API_VERSION, "normals API",
           NORMALS_SIGNATURES),
    Header("freesplat_amd_exposure.h", "FS_EXPOSURE_API_VERSION", "fs_exposure_api_version", EXPOSURE_API_VERSION, "exposure API",
           EXPOSURE_SIGNATURES),
    Header("freesplat_amd_mvdepth.h", "FS_MVDEPTH_API_VERSION", "fs_mvdepth_api_version", MVDEPTH_API_VERSION,
           "multi-view depth API", MVDEPTH_SIGNATURES),
    Header("freesplat_amd_transform.h", "FS_TRANSFORM_API_VERSION", "fs_transform_api_version", TRANSFORM_API_VERSION,
           "transform API", TRANSFORM_SIGNATURES),
    Header("freesplat_amd_pose.h", "FS_POSE_API_VERSION", "fs_pose_api_version", POSE_API_VERSION, "pose API", POSE_SIGNATURES),
    Header("freesplat_amd_tsdf.h", "FS_TSDF_API_VERSION", "fs_tsdf_api_version", TSDF_API_VERSION, "TSDF API", TSDF_SIGNATURES),
)

# Headers added after those eleven: include/freesplat_ext_<x>.h, the same records, bound and checked by lib() after HEADERS.
# (The eleven above, their table sizes and their revisions are pinned by tests/test_abi.py, a file that does not change;
# tests/test_abi_extensions.py holds every record here to its header and to the built library in the same way.)
EXTENSION_HEADERS = (
    Header("freesplat_ext_raycast.h", "FS_RAYCAST_API_VERSION", "fs_raycast_api_version", RAYCAST_API_VERSION, "ray-cast API",
           RAYCAST_SIGNATURES),
)

# Headers added from now on: include/ext/<name>.h (`file` is relative to include/), the same records, bound and checked by lib()
# after the two tuples above.  Those two are CLOSED: tests/test_abi.py and tests/test_abi_extensions.py pin their files, counts,
# table sizes and revisions literally, and a test file does not change.  This tuple is open: tests/test_abi_addons.py is
# parametrised over it and builds what it expects from each record's own fields, so a further record needs no edit to any test.
ADDON_HEADERS = (
    Header("ext/geometry.h", "FS_GEOMETRY_API_VERSION", "fs_geometry_api_version", GEOMETRY_API_VERSION, "geometry API",
           GEOMETRY_SIGNATURES),
)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FreeSplatHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). freesplat_amd has no CPU / eager fallback.")
        # torch first: it brings its own HIP runtime (libamdhip64 of its ROCm build), and the library must resolve its HIP
        # symbols to THAT copy -- loaded the other way round (this library first, as a bare `build(); smoke()` in one
        # process did) the system runtime is initialised beside torch's and every launch fails with "no ROCm-capable
        # device is detected"
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for h in HEADERS + EXTENSION_HEADERS + ADDON_HEADERS:
            for name, (res, args) in h.signatures.items():
                fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            got = getattr(L, h.version_fn)()
            if got != h.revision:
                raise FreeSplatHipError(f"{LIB_PATH} has {h.label} revision {got}, this binding expects {h.revision} "
                                        f"(include/{h.file} {h.macro}): rebuild the library")
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().fs_last_error().decode(errors="replace")
        raise FreeSplatHipError(f"{what} failed with status {status} {msg}")


def call(name: str, *args) -> None:
    """One status-returning entry point with exactly `args`; a non-zero status raises with the library's last error."""
    check(getattr(lib(), name)(*args), name)


def launch(name: str, *args) -> None:
    """call() of an entry point whose last argument is the stream: torch's current one."""
    check(getattr(lib(), name)(*args, current_stream()), name)


def ptr(t):
    """Device pointer of a torch tensor (or None).  The tensor must stay referenced until the library call that
    receives the pointer has returned (queued its launches): never write ptr(t.contiguous()) for more than one
    argument of a call -- a temporary freed between two conversions hands its block to the next one."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def profile_stage_names() -> list:
    L = lib()
    names = []
    while True:
        s = L.fs_profile_stage_name(len(names))
        if s is None:
            return names
        names.append(s.decode())


def profile_enable(on, stages=None) -> None:
    """on=False: off.  on=True: time every stage, or only the named `stages` (each timed launch costs two event
    records on the stream, so a throughput measurement should time as little as it needs)."""
    mask = 0
    if on:
        names = profile_stage_names()
        mask = -1 if stages is None else sum(1 << names.index(s) for s in stages)
    call("fs_profile_enable", mask)


def profile_collect() -> dict:
    """{stage name: (total ms, launches)} of the launches recorded since the last collect."""
    names = profile_stage_names()
    n = len(names)
    ms = (C.c_float * n)()
    cnt = (C.c_int32 * n)()
    call("fs_profile_collect", n, ms, cnt)
    return {names[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}
