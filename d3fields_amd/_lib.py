"""ctypes binding of libd3fields_hip.so (the C ABI declared in include/d3fields_hip.h).

There is deliberately no fallback: if the shared library cannot be loaded, or a call returns
an error status, an exception is raised.  Nothing in this package computes the field query on
the CPU or through torch ops.
"""
import ctypes
import functools
import os

import torch

from . import build as _build

ABI_VERSION = 16

# status codes (include/d3fields_hip.h)
OK = 0
ERR_INVALID_ARG, ERR_BAD_SHAPE, ERR_BAD_DTYPE, ERR_BAD_LAYOUT, ERR_HIP, ERR_WORKSPACE = -1, -2, -3, -4, -5, -6
FLAG_FINITE_MAPS = 1
FLAG_UNORDERED_POINTS = 2
FLAG_REFERENCE_ROUNDING = 4
FLAG_REUSE_POINT_ORDER = 8
FLAG_LOCAL_POINTS = 128
# D3F_PLAN_*: the planner's thresholds (csrc/d3f_plan.h defines its own from the same macros) that decide whether those two flags are honoured
PLAN_SMALL_BATCH, PLAN_WINDOW_CLOUD_MIN, PLAN_CACHE_RESIDENT_BYTES, PLAN_INFINITY_CACHE_BYTES = 65536, 262144, 64 << 20, 256 << 20
PROBE_WORDS = 40
TUNE_XCD_REMAP, TUNE_NO_REORDER, TUNE_FORCE_REORDER = 1 << 12, 1 << 13, 1 << 14
TUNE_DIRECT_GATHER = 1 << 4
TUNE_NO_WINDOW_GATE, TUNE_WINDOW_SIDE = 1 << 5, 1 << 6
GATE_SAMPLES, GATE_MIN_FIT = 128, 96
CHECK_WORDS_ARE_ZERO = 1
TRACK_STALL_SENTINEL = 0x57A11ED
MAX_VIEWS = 64
MAX_MAPS = 8
MAX_PROJECTION = 64
MAX_MOMENT_CHANNELS = 2048
VOLUME_MAX_CHANNELS = 4096
RAYCAST_MAX_STEPS = 65536
EDT_MAX_EXTENT = 16384
SEGMENT_CUT_CORNERS = 1
PEAKS_MAX_RADIUS = 8
ALIGN_ROW_DOUBLES, ALIGN_STATE_DOUBLES = 32, 96
ALIGN_RUNNING, ALIGN_CONVERGED, ALIGN_STALLED, ALIGN_NO_GRADIENT, ALIGN_FAILED = 0, 1, 2, 3, 4
ALIGN_CHUNK = 256
CONSENSUS_MAX_POINTS, CONSENSUS_MAX_CANDIDATES, CONSENSUS_MAX_SURVIVORS = 64, 8, 1 << 16
POOL_MEAN, POOL_VOTES = 0, 1
POOL_CHUNK = 256
POOL_MAX_VOTE_CHANNELS = 256
LINK_L2, LINK_COSINE, LINK_ARGMAX = 0, 1, 2
LINK_TILE = (4, 4, 16)
FLOW_MAX_RADIUS = 4
MOTION_OK, MOTION_THINNED, MOTION_TOO_FEW = 0, 1, 2
MOTION_MAX_FITS = 8
MOTION_SUM_DOUBLES, MOTION_POSE_DOUBLES = 16, 15
WARP_MAX_PARTS = 4096
KERNEL_NAME_MAX = 80
GAUSSIAN_MAX_RADIUS = 64
DTYPE_F32 = 0
DTYPE_F16 = 1
DIST_L2, DIST_SQUARE = 0, 1
SIM_DIST, SIM_EXP, SIM_SOFTMAX_DIM0 = 0, 1, 2

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_u32 = ctypes.c_uint32
_f32 = ctypes.c_float
_f64 = ctypes.c_double


class Views(ctypes.Structure):
    """struct d3f_views"""
    _fields_ = [("V", _i32), ("H", _i32), ("W", _i32), ("depth", _vp), ("K", _vp), ("pose", _vp), ("depth_nonfinite", _vp)]


class ChannelMap(ctypes.Structure):
    """struct d3f_channel_map"""
    _fields_ = [("data", _vp), ("fh", _i32), ("fw", _i32), ("C", _i32), ("dtype", _i32),
                ("stride_v", _i64), ("stride_y", _i64), ("stride_x", _i64), ("nonfinite", _vp)]


def channel_map(t, nonfinite=None):
    """The d3f_channel_map of a (V,h,w,C) tensor, or of a (V,H,W) depth tensor as a map of one float32 channel; `nonfinite`: the address
    of its d3f_map_check word.  Describes the tensor as it is: whether the library can read that is readable_layout(t)."""
    if t.dim() == 3:
        return ChannelMap(t.data_ptr(), t.shape[1], t.shape[2], 1, DTYPE_F32, t.stride(0), t.stride(1), max(t.stride(2), 1), nonfinite)
    return ChannelMap(t.data_ptr(), t.shape[1], t.shape[2], t.shape[3], DTYPE_F16 if t.dtype == torch.float16 else DTYPE_F32,
                      t.stride(0), t.stride(1), t.stride(2), nonfinite)


def readable_layout(t):
    """Can the library read `t` where it lies?  A map: float32 or float16, channels adjacent, texels >= C apart in x; depth: float32; no negative stride."""
    if t.dim() == 3:
        ok = t.dtype == torch.float32 and t.stride(2) >= 1
    else:
        ok = t.dtype in (torch.float32, torch.float16) and t.stride(3) == 1 and t.stride(2) >= t.shape[3]
    return ok and min(t.stride()) >= 0


class Grid(ctypes.Structure):
    """struct d3f_grid"""
    _fields_ = [("x", _vp), ("y", _vp), ("z", _vp), ("nx", _i32), ("ny", _i32), ("nz", _i32), ("reserved", _i32)]


class Volume(ctypes.Structure):
    """struct d3f_volume"""
    _fields_ = [("nx", _i32), ("ny", _i32), ("nz", _i32), ("origin", _f32 * 3), ("step", _f32), ("reserved", _i32),
                ("dist", _vp), ("valid", _vp), ("cell_valid", _vp)]


class VolumeSet(ctypes.Structure):
    """struct d3f_volume_set"""
    _fields_ = [("data", _vp), ("C", _i32), ("reserved", _i32), ("stride_voxel", _i64), ("fill", _vp)]


class Band(ctypes.Structure):
    """struct d3f_band"""
    _fields_ = [("slot", _vp), ("cell_band", _vp), ("n_rows", _i64)]


class WarpSelect(ctypes.Structure):
    """struct d3f_warp_select (host memory)"""
    _fields_ = [("vol", Volume), ("owner", _vp), ("pose", _vp), ("K", _i32), ("reserved", _i32), ("out_source", _vp), ("out_dist", _vp), ("out_valid", _vp),
                ("out_boxes", _vp)]


class WarpRows(ctypes.Structure):
    """struct d3f_warp_rows (host memory)"""
    _fields_ = [("vol", Volume), ("band", ctypes.POINTER(Band)), ("sets", ctypes.POINTER(VolumeSet)), ("n_sets", _i32), ("K", _i32), ("source", _vp), ("pose", _vp),
                ("voxels", _vp), ("m", _i64), ("out_sets", ctypes.POINTER(_vp)), ("out_known", _vp)]


class MergeSelect(ctypes.Structure):
    """struct d3f_merge_select (host memory; include/d3fields_hip_ext.h)"""
    _fields_ = [("nx", _i32), ("ny", _i32), ("nz", _i32), ("reserved", _i32), ("dist_a", _vp), ("valid_a", _vp), ("weight_a", _vp), ("dist_b", _vp), ("valid_b", _vp),
                ("weight_b", _vp), ("weight_a_all", _f32), ("weight_b_all", _f32), ("w_max", _f32), ("gap", _f32), ("out_dist", _vp), ("out_weight", _vp),
                ("out_beta", _vp), ("out_valid", _vp), ("out_kind", _vp)]


class MergeRows(ctypes.Structure):
    """struct d3f_merge_rows (host memory; include/d3fields_hip_ext.h)"""
    _fields_ = [("nx", _i32), ("ny", _i32), ("nz", _i32), ("n_sets", _i32), ("band_a", ctypes.POINTER(Band)), ("band_b", ctypes.POINTER(Band)),
                ("sets_a", ctypes.POINTER(VolumeSet)), ("sets_b", ctypes.POINTER(VolumeSet)), ("kind", _vp), ("beta", _vp), ("voxels", _vp), ("m", _i64),
                ("out_sets", ctypes.POINTER(_vp)), ("out_known", _vp), ("reserved", _i64)]


class CoarsenSelect(ctypes.Structure):
    """struct d3f_coarsen_select (host memory; include/d3fields_hip_pyramid.h)"""
    _fields_ = [("nx", _i32), ("ny", _i32), ("nz", _i32), ("min_children", _i32), ("dist", _vp), ("valid", _vp), ("out_dist", _vp), ("out_valid", _vp),
                ("out_children", _vp), ("reserved", _i64)]


class CoarsenRows(ctypes.Structure):
    """struct d3f_coarsen_rows (host memory; include/d3fields_hip_pyramid.h)"""
    _fields_ = [("nx", _i32), ("ny", _i32), ("nz", _i32), ("n_sets", _i32), ("band", ctypes.POINTER(Band)), ("sets", ctypes.POINTER(VolumeSet)), ("children", _vp),
                ("voxels", _vp), ("m", _i64), ("out_sets", ctypes.POINTER(_vp)), ("out_known", _vp), ("reserved", _i64)]


class FlowSeeded(ctypes.Structure):
    """struct d3f_flow_seeded (host memory; include/d3fields_hip_pyramid.h)"""
    _fields_ = [("site_a", _vp), ("slot_a", _vp), ("set_a", ctypes.POINTER(VolumeSet)), ("site_b", _vp), ("slot_b", _vp), ("set_b", ctypes.POINTER(VolumeSet)),
                ("seed", _vp), ("nx", _i32), ("ny", _i32), ("nz", _i32), ("radius", _i32), ("max_cost2", _f32), ("reserved", _i32), ("out_target", _vp),
                ("out_cost", _vp), ("out_axis_cost", _vp)]


class Pinhole(ctypes.Structure):
    """struct d3f_pinhole (host memory)"""
    _fields_ = [("K", _f32 * 9), ("pose", _f32 * 12), ("H", _i32), ("W", _i32)]


class TrackState(ctypes.Structure):
    """struct d3f_track_state"""
    _fields_ = [("t", _vp), ("w", _vp), ("adam_m", _vp), ("adam_v", _vp), ("step", _vp), ("out_pts", _vp), ("loss", _vp), ("scratch", _vp)]


class EvalPlan(ctypes.Structure):
    """struct d3f_eval_plan"""
    _fields_ = [("tile_points", _i32), ("reorder", _i32), ("lds_bytes", _i32), ("reserved", _i32), ("workgroups", _i64),
                ("vector_floats", _i32 * MAX_MAPS), ("lanes_per_point", _i32 * MAX_MAPS),
                ("vectors_per_lane", _i32 * MAX_MAPS), ("staged", _i32 * MAX_MAPS), ("gated_window", _i32), ("reserved2", _i32), ("family", _i32), ("reserved3", _i32),
                ("kernel", ctypes.c_char * KERNEL_NAME_MAX), ("window_kernel", ctypes.c_char * KERNEL_NAME_MAX)]


# name -> (restype, argtypes); every symbol include/d3fields_hip.h declares
SIGNATURES = {
    "d3f_abi_version": (ctypes.c_int, []),
    "d3f_version": (ctypes.c_char_p, []),
    "d3f_last_error": (ctypes.c_char_p, []),
    "d3f_build_has_experiments": (ctypes.c_int, []),
    "d3f_eval": (ctypes.c_int, [ctypes.POINTER(Views), _vp, _i64, ctypes.POINTER(ChannelMap), _i32, _f32, _u32,
                                _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _i64, _vp]),
    "d3f_map_check": (ctypes.c_int, [ctypes.POINTER(ChannelMap), _i32, _vp, _vp]),
    "d3f_map_check_many": (ctypes.c_int, [ctypes.POINTER(ChannelMap), ctypes.POINTER(_i32), _i32, ctypes.POINTER(_vp), _u32, _vp]),
    "d3f_project_maps": (ctypes.c_int, [ctypes.POINTER(ChannelMap), _i32, _vp, _i32, _vp, _vp]),
    "d3f_row_moments_workspace_bytes": (_i64, [_i64, _i32]),
    "d3f_row_moments": (ctypes.c_int, [_vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "d3f_eval_workspace_bytes": (_i64, [_i64]),
    "d3f_eval_dist_workspace_bytes": (_i64, [ctypes.POINTER(Views), _i64]),
    "d3f_eval_gate_offset": (_i64, [_i64]),
    "d3f_plan_family_name": (ctypes.c_char_p, [_i32]),
    "d3f_plan_family_takes": (ctypes.c_char_p, [_i32]),
    "d3f_profile_next_eval": (None, [_vp, _vp]),
    "d3f_eval_plan_query": (ctypes.c_int, [ctypes.POINTER(Views), _i64, ctypes.POINTER(ChannelMap), _i32, _u32, _i32, _i32,
                                           ctypes.POINTER(EvalPlan)]),
    "d3f_eval_grid": (ctypes.c_int, [ctypes.POINTER(Views), ctypes.POINTER(Grid), ctypes.POINTER(ChannelMap), _i32, _f32, _u32,
                                     _vp, _vp, ctypes.POINTER(_vp), _vp]),
    "d3f_eval_lattice": (ctypes.c_int, [ctypes.POINTER(Views), _vp, _i32, _i32, _i32, ctypes.POINTER(ChannelMap), _i32, _f32, _u32,
                                        _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]),
    "d3f_eval_plan_query_lattice": (ctypes.c_int, [ctypes.POINTER(Views), _i32, _i32, _i32, ctypes.POINTER(ChannelMap), _i32, _u32, _i32,
                                                   ctypes.POINTER(EvalPlan)]),
    "d3f_lattice_probe": (ctypes.c_int, [_vp, _i64, _vp, _vp]),
    "d3f_grid_shell_workspace_bytes": (_i64, [ctypes.POINTER(Grid)]),
    "d3f_grid_shell": (ctypes.c_int, [ctypes.POINTER(Views), ctypes.POINTER(Grid), _f32, _f32, _i64, _vp, _vp, _vp, _i64, _vp]),
    "d3f_mesh_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "d3f_mesh_count": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _i64, _vp]),
    "d3f_mesh_extract": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "d3f_volume_gaussian_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "d3f_volume_gaussian": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _f32, _vp, _i64, _vp]),
    "d3f_volume_cell_valid": (ctypes.c_int, [ctypes.POINTER(Volume), _vp, _vp]),
    "d3f_volume_sample": (ctypes.c_int, [ctypes.POINTER(Volume), _vp, _i64, ctypes.POINTER(VolumeSet), _i32, _vp, _vp, ctypes.POINTER(_vp), _vp]),
    "d3f_volume_sample_backward": (ctypes.c_int, [ctypes.POINTER(Volume), _vp, _i64, ctypes.POINTER(VolumeSet), _i32, _vp, ctypes.POINTER(_vp),
                                                  _vp, _vp]),
    "d3f_band_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "d3f_band_mark": (ctypes.c_int, [ctypes.POINTER(Volume), _f32, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "d3f_band_sample": (ctypes.c_int, [ctypes.POINTER(Volume), ctypes.POINTER(Band), _vp, _i64, ctypes.POINTER(VolumeSet), _i32, _vp, _vp, _vp,
                                       ctypes.POINTER(_vp), _vp]),
    "d3f_band_sample_backward": (ctypes.c_int, [ctypes.POINTER(Volume), ctypes.POINTER(Band), _vp, _i64, ctypes.POINTER(VolumeSet), _i32, _vp,
                                                ctypes.POINTER(_vp), _vp, _vp]),
    "d3f_volume_edt_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "d3f_volume_edt": (ctypes.c_int, [_vp, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "d3f_volume_components_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "d3f_volume_components": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "d3f_volume_components_linked": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "d3f_volume_links": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, ctypes.POINTER(VolumeSet), _i32, _f32, _i32, _vp, _vp]),
    "d3f_volume_flow": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(VolumeSet), _vp, _vp, ctypes.POINTER(VolumeSet), _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp,
                                       _vp]),
    "d3f_part_motion_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i64]),
    "d3f_part_motion": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _f64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _i64, _vp]),
    "d3f_volume_warp_select": (ctypes.c_int, [ctypes.POINTER(WarpSelect), _vp]),
    "d3f_volume_warp_rows": (ctypes.c_int, [ctypes.POINTER(WarpRows), _vp]),
    "d3f_volume_pool_workspace_bytes":(_i64, [_i32, _i32, _i32, _i32, _i64, _i64]),
    "d3f_volume_pool": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, ctypes.POINTER(VolumeSet), _i32, ctypes.POINTER(_i32), _i64, _vp, _vp, _vp,
                                       ctypes.POINTER(_vp), _vp, _i64, _vp]),
    "d3f_volume_geodesic_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "d3f_volume_geodesic_init": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _i64, _vp]),
    "d3f_volume_geodesic_relax": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, ctypes.POINTER(_i32), _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "d3f_volume_geodesic_finish": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, ctypes.POINTER(_i32), _f32, _vp, _vp, _vp, _vp]),
    "d3f_volume_follow": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "d3f_volume_segments": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i64, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "d3f_path_shorten": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _u32, _vp, _vp, _vp, _vp]),
    "d3f_volume_peaks": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _i64, _i32, _f32, _vp, _i64, _vp, _vp, _i64, _vp]),
    "d3f_volume_align_workspace_bytes": (_i64, [_i64, _i64]),
    "d3f_volume_align_centroid": (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "d3f_volume_align_accumulate": (ctypes.c_int, [ctypes.POINTER(Volume), ctypes.POINTER(Band), ctypes.POINTER(VolumeSet), _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   _i64, _i64, _f32, _f32, _f32, _vp, _vp, _i64, _vp]),
    "d3f_volume_align_step": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _i32, _f64, _f64, _vp, _vp, _vp, _vp]),
    "d3f_pose_consensus_workspace_bytes": (_i64, [_i32, _i32, _i64, _i64]),
    "d3f_pose_consensus_score": (ctypes.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _f32, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "d3f_pose_consensus_select": (ctypes.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _f32, _f64, _f64, _f64, _vp, _i32, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp,
                                                 _vp, _i64, _vp]),
    "d3f_pose_refit": (ctypes.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _f32, _vp, _vp, _vp, _vp]),
    "d3f_volume_raycast": (ctypes.c_int, [ctypes.POINTER(Volume), _vp, _vp, _i64, ctypes.POINTER(Pinhole), _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "d3f_fps_workspace_bytes": (_i64, [_i64]),
    "d3f_fps_pixels_workspace_bytes": (_i64, [_i64]),
    "d3f_farthest_point_sampling": (ctypes.c_int, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    "d3f_backproject_workspace_bytes": (_i64, [_i32, _i32]),
    "d3f_backproject_view": (ctypes.c_int, [_vp, _vp, _i32, _i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), _i64, _vp, _vp, _vp, _vp, _vp]),
    "d3f_pcd_nearest": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "d3f_pcd_to_index": (ctypes.c_int, [_vp, _i64, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.POINTER(_i32), _vp, _vp, _vp]),
    "d3f_vox_iou_workspace_bytes": (_i64, [_i64, _i64]),
    "d3f_vox_idx_iou": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "d3f_erode": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "d3f_compose_labels": (ctypes.c_int, [_vp, _i32, _i64, _vp, _vp, _vp]),
    "d3f_voxel_downsample_workspace_bytes": (_i64, [_i64]),
    "d3f_voxel_downsample": (ctypes.c_int, [_vp, _vp, _i64, ctypes.c_double, _vp, _vp, _vp, _vp, _i64, _vp]),
    "d3f_mask_gate": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i32, _i32, _f32, _f32, _vp, _vp]),
    "d3f_nonzero_pixels": (ctypes.c_int, [_vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp]),
    "d3f_fps_pixels": (ctypes.c_int, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    "d3f_eval_backward": (ctypes.c_int, [ctypes.POINTER(Views), _vp, _i64, ctypes.POINTER(ChannelMap), _i32, _f32,
                                         _vp, ctypes.POINTER(_vp), _vp, _vp]),
    "d3f_eval_dist_backward": (ctypes.c_int, [ctypes.POINTER(Views), _vp, _i64, _vp, _vp, _vp]),
    "d3f_eval_dist": (ctypes.c_int, [ctypes.POINTER(Views), _vp, _i64, _vp, _vp, _vp]),
    "d3f_onehot2instance": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "d3f_instance2onehot": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "d3f_softmax_workspace_bytes": (_i64, [_i64, _i64]),
    "d3f_similarity_to_target": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i64, _i64, _i64, _vp, _f32, _i32, _i32,
                                                _vp, _vp, _i64, _vp]),
    "d3f_pairwise_similarity": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _i64,
                                               _vp]),
    "d3f_pairwise_topk_workspace_bytes": (_i64, [_i64, _i64]),
    "d3f_pairwise_similarity_topk": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i32, _f32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64,
                                                    _vp]),
    "d3f_topk_smallest": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    "d3f_topk_merge": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp]),
    "d3f_pairwise_softmax_local": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i32, _f32, _i32, _i64, _vp, _vp, _vp, _i64,
                                                  _vp]),
    "d3f_point_order_locality": (ctypes.c_int, [_vp, _i64, _vp, _vp]),
    "d3f_points_probe": (ctypes.c_int, [_vp, _i64, _vp, _vp]),
    "d3f_rigid_transform": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "d3f_track_loss_grad": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp, _vp]),
    "d3f_track_step_scratch_bytes": (_i64, [_i32, _i32]),
    "d3f_track_step": (ctypes.c_int, [ctypes.POINTER(Views), ctypes.POINTER(ChannelMap), _vp, _i32, _i32, _vp, _f32, _f32, _f32, _f32, _f32,
                                      _f32, _f32, ctypes.POINTER(TrackState), _vp]),
    "d3f_track_run": (ctypes.c_int, [ctypes.POINTER(Views), ctypes.POINTER(ChannelMap), _vp, _i32, _i32, _vp, _f32, _f32, _f32, _f32, _f32,
                                     _f32, _f32, _i32, ctypes.POINTER(TrackState), _vp]),
    "d3f_track_run_max_keypoints": (_i32, []),
    "d3f_track_stall_word": (_i64, [_i32, _i32]),
    "d3f_rigid_update": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _vp]),
    "d3f_softmax_merge": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "d3f_softmax_apply": (ctypes.c_int, [_vp, _i64, _i64, _f32, _vp, _vp]),
}

# the entry points whose declaration ends in `void *stream` (names without their d3f_ prefix): on() fills that argument in
STREAMED = frozenset("d3f_" + n for n in """
    eval map_check map_check_many project_maps row_moments eval_grid eval_lattice lattice_probe grid_shell mesh_count mesh_extract volume_gaussian
    volume_cell_valid volume_sample volume_sample_backward band_mark band_sample band_sample_backward volume_edt volume_components volume_components_linked
    volume_links volume_flow part_motion volume_warp_select volume_warp_rows volume_pool volume_geodesic_init volume_geodesic_relax volume_geodesic_finish
    volume_follow volume_segments path_shorten volume_peaks volume_align_centroid volume_align_accumulate volume_align_step pose_consensus_score
    pose_consensus_select pose_refit volume_raycast farthest_point_sampling backproject_view pcd_nearest pcd_to_index vox_idx_iou erode compose_labels
    voxel_downsample mask_gate nonzero_pixels fps_pixels eval_backward eval_dist_backward eval_dist onehot2instance instance2onehot similarity_to_target
    pairwise_similarity pairwise_similarity_topk topk_smallest topk_merge pairwise_softmax_local point_order_locality points_probe rigid_transform
    track_loss_grad track_step track_run rigid_update softmax_merge softmax_apply
""".split())
# the others that return a status; everything else returns a value
STATUS = STREAMED | {"d3f_eval_plan_query", "d3f_eval_plan_query_lattice"}

# The entry points added after ABI 16's main table, declared by include/d3fields_hip_ext.h and exported by the same library.  The main header and
# the three tables above are closed (host tests pin their counts); what is added since goes here, in the same (restype, argtypes) form.
EXT_SIGNATURES = {
    "d3f_volume_merge_select": (ctypes.c_int, [ctypes.POINTER(MergeSelect), _vp]),
    "d3f_volume_merge_rows": (ctypes.c_int, [ctypes.POINTER(MergeRows), _vp]),
}
# ... whose declaration ends in `void *stream`
EXT_STREAMED = frozenset(["d3f_volume_merge_select", "d3f_volume_merge_rows"])
MERGE_NONE, MERGE_KEEP, MERGE_NEW, MERGE_BLEND, MERGE_RESET = 0, 1, 2, 3, 4

# The extension header is closed as well (a host test pins it to the merge pair).  From here on a feature brings a header of its own and ONE
# entry here: header file name -> (signatures in the (restype, argtypes) form, the names whose declaration ends in `void *stream`).  load(),
# on.__getattr__ and on._call treat every entry as they treat EXT_*, and tests/test_pyramid_host.py checks each header against its own table.
FEATURE_TABLES = {
    "d3fields_hip_pyramid.h": ({
        "d3f_volume_coarsen_select": (ctypes.c_int, [ctypes.POINTER(CoarsenSelect), _vp]),
        "d3f_volume_coarsen_rows": (ctypes.c_int, [ctypes.POINTER(CoarsenRows), _vp]),
        "d3f_volume_flow_seeded": (ctypes.c_int, [ctypes.POINTER(FlowSeeded), _vp]),
    }, frozenset(["d3f_volume_coarsen_select", "d3f_volume_coarsen_rows", "d3f_volume_flow_seeded"])),
}
FLOW_SEED_MAX = 16384


def _feature(name):
    """(restype, argtypes, streamed) of an entry point of FEATURE_TABLES, or None"""
    for signatures, streamed in FEATURE_TABLES.values():
        if name in signatures:
            return signatures[name] + (name in streamed,)
    return None


_lib = None


class D3FError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libd3fields_hip: status %d: %s" % (code, text))
        self.code = code


def library_path():
    return _build.LIB_PATH


def load():
    """Loads (building first if the .so is absent and hipcc exists) and type-annotates the ABI."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if _build.is_stale():
        # missing, or built from other sources than the ones in the tree (content fingerprint, not mtimes):
        # rebuild -- raises if hipcc is unavailable, so a stale library is never loaded silently
        try:
            _build.build_library()
        except (RuntimeError, OSError) as exc:
            raise ImportError("libd3fields_hip.so is %s and hipcc is not available to build it: %s"
                              % ("missing" if not os.path.exists(path) else "out of date with csrc/", exc))
    lib = ctypes.CDLL(path)
    features = [item for signatures, _ in FEATURE_TABLES.values() for item in signatures.items()]
    for name, (res, args) in list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) + features:
        fn = getattr(lib, name)     # AttributeError if the .so lacks a declared symbol (of any header)
        fn.restype = res
        fn.argtypes = args
    got = lib.d3f_abi_version()
    if got != ABI_VERSION:
        raise ImportError("libd3fields_hip ABI %d != binding ABI %d; rebuild with python -m d3fields_amd.build --force"
                          % (got, ABI_VERSION))
    _lib = lib
    return lib


def check(code):
    if code != OK:
        raise D3FError(code, load().d3f_last_error().decode("utf-8", "replace"))


def ptr(t):
    """Device (or host) address of a torch tensor as c_void_p; None -> NULL."""
    return _vp(t.data_ptr()) if t is not None else _vp(None)


def current_stream_handle(device):
    return _vp(torch.cuda.current_stream(device).cuda_stream)


class on:
    """Calls into the library on one device, on its current stream:

        with _lib.on(dev) as q:
            ws, ws_bytes = q.workspace("d3f_volume_edt_workspace_bytes", nx, ny, nz)
            q.d3f_volume_edt(site, nx, ny, nz, step, max_d2, d2, nearest, dist, ws, ws_bytes)

    Entering sets the device and reads its current stream once; every call in the block shares that stream, and the entry points in
    STREAMED receive it as their last argument.  A tensor goes in as its address, a Structure by reference, everything else (None, ctypes
    arrays and pointers, numbers, host addresses) as it is.  A tensor that is not on the device is refused before anything is launched;
    converting and checking the arguments touches no GPU state.  A status other than OK raises D3FError."""

    def __init__(self, device, lib=None):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = load() if lib is None else lib

    def __enter__(self):
        self._guard = torch.cuda.device(self.device)
        self._guard.__enter__()
        self.stream = current_stream_handle(self.device)
        return self

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)

    def __getattr__(self, name):
        if name not in SIGNATURES and name not in EXT_SIGNATURES and _feature(name) is None:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, *args):
        conv = []
        for a in args:
            if isinstance(a, torch.Tensor):
                if not a.is_cuda or a.device != self.device:     # (host memory goes in as a ctypes array or an address, never as a tensor)
                    raise RuntimeError("%s: argument %d is a tensor on %s; this call runs on %s" % (name, len(conv), a.device, self.device))
                a = _vp(a.data_ptr())
            elif isinstance(a, ctypes.Structure):
                a = ctypes.byref(a)
            conv.append(a)
        feature = _feature(name)
        if name in STREAMED or name in EXT_STREAMED or (feature is not None and feature[2]):
            conv.append(self.stream)
        out = getattr(self.lib, name)(*conv)
        if name in STATUS or (name in EXT_SIGNATURES and EXT_SIGNATURES[name][0] is ctypes.c_int) or (feature is not None and feature[0] is ctypes.c_int):
            return check(out)
        return out

    def workspace(self, size_fn, *args):
        """(uint8 tensor on the device, the byte count size_fn(*args) gave): at least 16 bytes are allocated, so that the address is never
        NULL -- the library refuses a NULL workspace even where it needs no bytes"""
        nbytes = int(self._call(size_fn, *args))
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device), nbytes
