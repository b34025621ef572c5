"""ctypes binding of include/zly.h (libzly.so) for tests, bench.py and smoke().

Plumbing only: every call goes straight through the C ABI.  There is no Python or CPU fallback:
if the HIP extension is missing, or no HIP device is visible, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libzly.so")
DEFAULT_WEIGHTS = os.path.join(_HERE, "_build", "yolov8n_synth.zlyw")

OK = 0
ERR_INVALID_ARGUMENT = 2
ERR_NOT_INITIALIZED = 3
ERR_INFERENCE = 200
ERR_MODEL_NOT_FOUND = 201
ERR_MODEL_LOAD = 202
ERR_INVALID_INPUT = 203
ERR_SYSTEM = 300
PENDING = 1
DTYPE_FP32, DTYPE_BF16 = 0, 1
SLAB_OVERFLOW = 1
FLAG_DUMP_LOGITS = 1
FLAG_NO_FUSION = 2
FLAG_NO_HEAD_TENSOR = 4
FLAG_ASYNC_NMS = 8
FLAG_SINGLE_CHAIN = 16
FLAG_LETTERBOX = 32          # per-engine resize mode: aspect-preserving bilinear letterbox (include/zly.h), boxes normalised to the request frame
LETTERBOX_MAX_DIM = 16384    # largest request side (and model side) of a letterbox engine
FLAG_AREA = 64               # per-engine resize filter: the exact area average over every source pixel (include/zly.h); combines with FLAG_LETTERBOX
AREA_MAX_DIM = 16384         # largest request side (and model side) of an area engine
# pixel formats of a request frame (include/zly.h ZLY_PIX_*): packed BGR, 8-bit YUV 4:2:0 (limited range) converted in the front kernel, or
# packed RGB / BGRA / RGBA (the fourth byte is never interpreted) fetched in the front kernel as the BGR frame of their B, G, R bytes
PIX_BGR, PIX_NV12_BT601, PIX_I420_BT601, PIX_NV12_BT709, PIX_I420_BT709 = 0, 1, 2, 3, 4
PIX_RGB, PIX_BGRA, PIX_RGBA = 16, 17, 18
PIX_YUY2_BT601, PIX_UYVY_BT601, PIX_YUY2_BT709, PIX_UYVY_BT709 = 10, 11, 12, 13      # packed YUV 4:2:2 (capture cards, UVC devices): 1-D u8 buffers of 2wh bytes, w even
MERGE_IOU, MERGE_IOS = 0, 1          # zly_merge_config.metric (include/zly.h "Tiles")
MERGE_MAX_CANDIDATES = 4096          # tiles of a group x max_dets may not exceed it
SURFACE_MAX_RECTS = 1024             # rectangles per surface_update / detect_delta call (include/zly.h "Resident surfaces")
SURFACE_ALIGN = 256                  # the store's slot stride is a multiple of it
SURFACE_MAX_MOVES = 1024             # moves per surface_move call
CHIP_BGR8, CHIP_RGB_F32 = 0, 1      # zly_chip_config.layout (include/zly.h "Chips")
CHIPS_SRC_SLABS, CHIPS_SRC_MERGED = 0, 1     # which engine-owned slab buffer a chips call reads when it is given none
_PACKED_BPP = {PIX_BGR: 3, PIX_RGB: 3, PIX_BGRA: 4, PIX_RGBA: 4}

# every symbol include/zly.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    "zly_default_config", "zly_create", "zly_destroy", "zly_last_error", "zly_version",
    "zly_detect", "zly_detect_batch", "zly_submit", "zly_submit_try", "zly_poll", "zly_wait", "zly_detect_device", "zly_slab_bytes", "zly_read_slabs", "zly_sync", "zly_join",
    "zly_frame_bytes", "zly_letterbox_geometry", "zly_detect_fmt", "zly_detect_batch_fmt", "zly_submit_fmt", "zly_submit_try_fmt", "zly_detect_device_fmt", "zly_preprocess_fmt",
    "zly_preprocess", "zly_forward", "zly_head_tensor", "zly_postprocess", "zly_debug_tap",
    "zly_view_bytes", "zly_view_tight", "zly_view_crop", "zly_detect_view", "zly_detect_batch_view", "zly_submit_view", "zly_submit_try_view",
    "zly_detect_device_view", "zly_preprocess_view",
    "zly_default_track_config", "zly_track_enable", "zly_track_reset", "zly_track_state_at", "zly_track_slabs", "zly_submit_view_tracked", "zly_submit_try_view_tracked",
    "zly_default_track_motion_config", "zly_track_motion_enable", "zly_track_read",
    "zly_default_merge_config", "zly_merge_slabs", "zly_read_merged", "zly_tile_grid", "zly_detect_tiled",
    "zly_surfaces_enable", "zly_surface_define", "zly_surface_update", "zly_surface_read", "zly_detect_surfaces", "zly_detect_delta",
    "zly_surface_moves_enable", "zly_surface_move",
    "zly_default_zoom_config", "zly_zoom_enable", "zly_detect_device_zoom", "zly_detect_surfaces_zoom", "zly_zoom_plan", "zly_zoom_read_plan",
    "zly_default_chip_config", "zly_chips_enable", "zly_chip_layout", "zly_chips_device_view", "zly_chips_surfaces", "zly_read_chips",
    "zly_default_change_config", "zly_change_enable", "zly_change_layout", "zly_change_device_view", "zly_change_surfaces", "zly_change_read", "zly_change_reset",
    "zly_zoom_use_change",
    "zly_default_camera_config", "zly_camera_enable", "zly_camera_layout", "zly_camera_device_view", "zly_camera_surfaces", "zly_camera_read", "zly_camera_reset",
    "zly_camera_apply_tracks",
    "zly_num_classes", "zly_weights_fp8", "zly_num_anchors", "zly_num_ops", "zly_op_info_at", "zly_launch_info_at", "zly_op_kernel_name", "zly_profile_ops", "zly_get_stats",
]

DET_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("confidence", "<f4"),
                      ("class_id", "<i4"), ("track_id", "<u4"), ("pad_", "<u4"), ("timestamp", "<u8")])
assert DET_DTYPE.itemsize == 40
SLAB_HDR_DTYPE = np.dtype([("n_kept", "<i4"), ("n_candidates", "<i4"), ("flags", "<u4"), ("frame_tag", "<u4")])
# zly_track: one live slot of a stream's track table (zly_track_read)
TRACK_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("vx", "<f4"), ("vy", "<f4"),
                        ("class_id", "<i4"), ("id", "<u4"), ("hits", "<u4"), ("last_seen", "<u4")])
assert TRACK_DTYPE.itemsize == 40
# zly_zoom_region: one planned region of a frame (zly_zoom_plan, zly_zoom_read_plan); slot = -1, track_id = 0: a fallback
ZOOM_REGION_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("slot", "<i4"), ("track_id", "<u4")])
assert ZOOM_REGION_DTYPE.itemsize == 24
# zly_chip_header / zly_chip_rec: the head of a chip slab and one chip's record (zly_read_chips)
CHIP_HDR_DTYPE = np.dtype([("n_chips", "<i4"), ("n_eligible", "<i4"), ("frame_tag", "<u4"), ("flags", "<u4")])
assert CHIP_HDR_DTYPE.itemsize == 16
CHIP_REC_DTYPE = np.dtype([("det", "<i4"), ("class_id", "<i4"), ("track_id", "<u4"), ("confidence", "<f4"),
                           ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4")])
assert CHIP_REC_DTYPE.itemsize == 32
# zly_change_header / zly_change_peak: the head of a stream's change record and one peak (zly_change_read)
CHANGE_FIRST, CHANGE_GLOBAL, CHANGE_MAX_CELLS = 1, 2, 8192
CHANGE_HDR_DTYPE = np.dtype([("n_cells", "<i4"), ("n_active", "<i4"), ("n_peaks", "<i4"), ("flags", "<u4"), ("gw", "<i4"), ("gh", "<i4"), ("step", "<u4"), ("pad", "<u4")])
CHANGE_PEAK_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("activity", "<u4"), ("pad", "<u4")])
assert CHANGE_HDR_DTYPE.itemsize == 32 and CHANGE_PEAK_DTYPE.itemsize == 32
# zly_camera_header: the head of a stream's camera motion record (zly_camera_read); the SAD table, u64 [17 * 17], lies behind it
CAMERA_FIRST, CAMERA_LOST, CAMERA_CLIPPED, CAMERA_MAX_RADIUS, CAMERA_SAD_ROOM = 1, 2, 4, 8, 289
CAMERA_HDR_DTYPE = np.dtype([("flags", "<u4"), ("step", "<u4"), ("gw", "<i4"), ("gh", "<i4"), ("dx", "<i4"), ("dy", "<i4"), ("fx", "<i4"), ("fy", "<i4"),
                             ("sx_q4", "<i4"), ("sy_q4", "<i4"), ("n_lost", "<u4"), ("n_applied", "<u4"), ("sad_min", "<u8"), ("sad_zero", "<u8"),
                             ("pend_x_q4", "<i8"), ("pend_y_q4", "<i8"), ("pad", "<u4", (4,))])
assert CAMERA_HDR_DTYPE.itemsize == 96


class Config(C.Structure):
    _fields_ = [("weights_path", C.c_char_p), ("model_w", C.c_int32), ("model_h", C.c_int32),
                ("conf_thr", C.c_float), ("iou_thr", C.c_float), ("max_batch", C.c_int32),
                ("max_dets", C.c_int32), ("device", C.c_int32), ("dtype", C.c_int32),
                ("warmup_runs", C.c_int32), ("use_graph", C.c_int32), ("flags", C.c_int32)]


class FrameView(C.Structure):
    """zly_frame_view: where a request's samples lie inside a larger buffer (offsets from the buffer base, row pitches)"""
    _fields_ = [("fmt", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("pad_", C.c_int32),
                ("off", C.c_uint64 * 3), ("pitch", C.c_int32 * 3), ("pad2_", C.c_int32)]


class TrackConfig(C.Structure):
    """zly_track_config"""
    _fields_ = [("max_streams", C.c_int32), ("max_tracks", C.c_int32), ("match_iou", C.c_float), ("max_lost", C.c_int32)]


class TrackState(C.Structure):
    """zly_track_state"""
    _fields_ = [("frame_no", C.c_uint32), ("next_id", C.c_uint32), ("n_live", C.c_int32), ("evictions", C.c_uint32)]


class TrackMotionConfig(C.Structure):
    """zly_track_motion_config"""
    _fields_ = [("beta", C.c_float), ("v_max", C.c_float)]


class Track(C.Structure):
    """zly_track (TRACK_DTYPE is its numpy twin)"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float), ("vx", C.c_float), ("vy", C.c_float),
                ("class_id", C.c_int32), ("id", C.c_uint32), ("hits", C.c_uint32), ("last_seen", C.c_uint32)]


class Tile(C.Structure):
    """zly_tile: the rectangle (x0, y0, w, h) of a W x H surface that a slab's boxes are fractions of, and the group it is merged in (-1 = none)"""
    _fields_ = [("group", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("W", C.c_int32), ("H", C.c_int32)]


class MergeConfig(C.Structure):
    """zly_merge_config"""
    _fields_ = [("metric", C.c_int32), ("thr", C.c_float)]


class SurfaceRect(C.Structure):
    """zly_surface_rect: where a rectangle's first pixel lies in which resident surface (its size and format are its source view's)"""
    _fields_ = [("surface", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32)]


class SurfaceMove(C.Structure):
    """struct zly_surface_move: the w x h block at (sx, sy) of a resident surface now lies at (dx, dy)"""
    _fields_ = [("surface", C.c_int32), ("sx", C.c_int32), ("sy", C.c_int32), ("dx", C.c_int32), ("dy", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class Roi(C.Structure):
    """zly_roi"""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class ZoomConfig(C.Structure):
    """zly_zoom_config"""
    _fields_ = [("regions", C.c_int32), ("region_w", C.c_int32), ("region_h", C.c_int32), ("max_age", C.c_int32), ("class_id", C.c_int32)]


class ChangeConfig(C.Structure):
    """zly_change_config"""
    _fields_ = [("cell", C.c_int32), ("threshold_q4", C.c_int32), ("max_active_permille", C.c_int32), ("max_peaks", C.c_int32), ("window_w", C.c_int32),
                ("window_h", C.c_int32)]


class CameraConfig(C.Structure):
    """zly_camera_config"""
    _fields_ = [("cell", C.c_int32), ("radius", C.c_int32), ("max_residual_q4", C.c_int32)]


class ChipConfig(C.Structure):
    """zly_chip_config"""
    _fields_ = [("chip_w", C.c_int32), ("chip_h", C.c_int32), ("max_chips", C.c_int32), ("class_id", C.c_int32), ("scale", C.c_float), ("layout", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("inference_count", C.c_uint64), ("inference_errors", C.c_uint64),
                ("total_preprocess_ms", C.c_double), ("total_forward_ms", C.c_double),
                ("total_postprocess_ms", C.c_double), ("last_detect_ms", C.c_double),
                ("sampled_frames", C.c_uint64), ("sampled_preprocess_ms", C.c_double), ("sampled_forward_ms", C.c_double),
                ("sampled_postprocess_ms", C.c_double), ("batches", C.c_uint64), ("graph_replays", C.c_uint64), ("eager_batches", C.c_uint64)]


class OpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kind", C.c_int32), ("pad_", C.c_int32),
                ("flops_per_frame", C.c_double), ("bytes_per_frame", C.c_double)]


class LaunchInfo(C.Structure):
    _fields_ = [("covered_by", C.c_int32), ("n_ops", C.c_int32), ("flops_per_frame", C.c_double),
                ("bytes_unfused_per_frame", C.c_double), ("bytes_fused_per_frame", C.c_double), ("weight_bytes", C.c_double)]


class ZlyError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"zly error {code}: {msg}")
        self.code = code
        self.message = msg


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Loads libzly.so and declares the prototypes.  Raises if the extension has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ZLY_LIB") or LIB_PATH          # ZLY_LIB: A/B two builds on one box (dev aid)
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not found: build the HIP extension first (make, or __graft_entry__.build())")
    lib = C.CDLL(p)
    vp, i32, u32, f32, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_size_t
    pi32 = C.POINTER(C.c_int32)
    lib.zly_default_config.argtypes = [C.POINTER(Config)]; lib.zly_default_config.restype = None
    lib.zly_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]; lib.zly_create.restype = i32
    lib.zly_destroy.argtypes = [vp]; lib.zly_destroy.restype = i32
    lib.zly_last_error.argtypes = []; lib.zly_last_error.restype = C.c_char_p
    lib.zly_version.argtypes = []; lib.zly_version.restype = C.c_char_p
    lib.zly_detect.argtypes = [vp, vp, sz, i32, i32, vp, i32, pi32]; lib.zly_detect.restype = i32
    lib.zly_detect_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), pi32, pi32, vp, i32, pi32]; lib.zly_detect_batch.restype = i32
    lib.zly_submit.argtypes = [vp, vp, sz, i32, i32, C.POINTER(C.c_uint64)]; lib.zly_submit.restype = i32
    lib.zly_submit_try.argtypes = [vp, vp, sz, i32, i32, C.POINTER(C.c_uint64)]; lib.zly_submit_try.restype = i32
    lib.zly_poll.argtypes = [vp, C.c_uint64]; lib.zly_poll.restype = i32
    lib.zly_wait.argtypes = [vp, C.c_uint64, vp, i32, pi32]; lib.zly_wait.restype = i32
    lib.zly_detect_device.argtypes = [vp, i32, vp, i32, i32, vp, u32, vp]; lib.zly_detect_device.restype = i32
    lib.zly_slab_bytes.argtypes = [vp]; lib.zly_slab_bytes.restype = sz
    lib.zly_read_slabs.argtypes = [vp, i32, vp]; lib.zly_read_slabs.restype = i32
    lib.zly_sync.argtypes = [vp]; lib.zly_sync.restype = i32
    lib.zly_join.argtypes = [vp, vp, i32]; lib.zly_join.restype = i32
    lib.zly_preprocess.argtypes = [vp, vp, sz, i32, i32, vp]; lib.zly_preprocess.restype = i32
    lib.zly_frame_bytes.argtypes = [i32, i32, i32]; lib.zly_frame_bytes.restype = sz
    lib.zly_letterbox_geometry.argtypes = [i32, i32, i32, i32, pi32, pi32, pi32, pi32]; lib.zly_letterbox_geometry.restype = i32
    lib.zly_detect_fmt.argtypes = [vp, i32, vp, sz, i32, i32, vp, i32, pi32]; lib.zly_detect_fmt.restype = i32
    lib.zly_detect_batch_fmt.argtypes = [vp, i32, pi32, C.POINTER(vp), C.POINTER(sz), pi32, pi32, vp, i32, pi32]; lib.zly_detect_batch_fmt.restype = i32
    lib.zly_submit_fmt.argtypes = [vp, i32, vp, sz, i32, i32, C.POINTER(C.c_uint64)]; lib.zly_submit_fmt.restype = i32
    lib.zly_submit_try_fmt.argtypes = [vp, i32, vp, sz, i32, i32, C.POINTER(C.c_uint64)]; lib.zly_submit_try_fmt.restype = i32
    lib.zly_detect_device_fmt.argtypes = [vp, i32, i32, vp, i32, i32, vp, u32, vp]; lib.zly_detect_device_fmt.restype = i32
    lib.zly_preprocess_fmt.argtypes = [vp, i32, vp, sz, i32, i32, vp]; lib.zly_preprocess_fmt.restype = i32
    pv = C.POINTER(FrameView)
    lib.zly_view_bytes.argtypes = [pv]; lib.zly_view_bytes.restype = sz
    lib.zly_view_tight.argtypes = [i32, i32, i32, pv]; lib.zly_view_tight.restype = i32
    lib.zly_view_crop.argtypes = [pv, i32, i32, i32, i32, pv]; lib.zly_view_crop.restype = i32
    lib.zly_detect_view.argtypes = [vp, vp, sz, pv, vp, i32, pi32]; lib.zly_detect_view.restype = i32
    lib.zly_detect_batch_view.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), pv, vp, i32, pi32]; lib.zly_detect_batch_view.restype = i32
    lib.zly_submit_view.argtypes = [vp, vp, sz, pv, C.POINTER(C.c_uint64)]; lib.zly_submit_view.restype = i32
    lib.zly_submit_try_view.argtypes = [vp, vp, sz, pv, C.POINTER(C.c_uint64)]; lib.zly_submit_try_view.restype = i32
    lib.zly_detect_device_view.argtypes = [vp, i32, vp, sz, pv, vp, u32, vp]; lib.zly_detect_device_view.restype = i32
    lib.zly_preprocess_view.argtypes = [vp, vp, sz, pv, vp]; lib.zly_preprocess_view.restype = i32
    lib.zly_default_track_config.argtypes = [C.POINTER(TrackConfig)]; lib.zly_default_track_config.restype = None
    lib.zly_track_enable.argtypes = [vp, C.POINTER(TrackConfig)]; lib.zly_track_enable.restype = i32
    lib.zly_track_reset.argtypes = [vp, i32, u32]; lib.zly_track_reset.restype = i32
    lib.zly_track_state_at.argtypes = [vp, i32, C.POINTER(TrackState)]; lib.zly_track_state_at.restype = i32
    lib.zly_track_slabs.argtypes = [vp, i32, pi32, vp, vp]; lib.zly_track_slabs.restype = i32
    lib.zly_submit_view_tracked.argtypes = [vp, vp, sz, pv, i32, C.POINTER(C.c_uint64)]; lib.zly_submit_view_tracked.restype = i32
    lib.zly_submit_try_view_tracked.argtypes = [vp, vp, sz, pv, i32, C.POINTER(C.c_uint64)]; lib.zly_submit_try_view_tracked.restype = i32
    lib.zly_default_track_motion_config.argtypes = [C.POINTER(TrackMotionConfig)]; lib.zly_default_track_motion_config.restype = None
    lib.zly_track_motion_enable.argtypes = [vp, C.POINTER(TrackMotionConfig)]; lib.zly_track_motion_enable.restype = i32
    lib.zly_track_read.argtypes = [vp, i32, vp, i32, pi32]; lib.zly_track_read.restype = i32
    lib.zly_default_merge_config.argtypes = [C.POINTER(MergeConfig)]; lib.zly_default_merge_config.restype = None
    lib.zly_merge_slabs.argtypes = [vp, i32, C.POINTER(Tile), i32, C.POINTER(MergeConfig), vp, vp, u32, vp]; lib.zly_merge_slabs.restype = i32
    lib.zly_read_merged.argtypes = [vp, i32, vp]; lib.zly_read_merged.restype = i32
    lib.zly_tile_grid.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(Tile), i32, pi32]; lib.zly_tile_grid.restype = i32
    lib.zly_detect_tiled.argtypes = [vp, vp, sz, pv, i32, C.POINTER(Tile), C.POINTER(MergeConfig), vp, i32, pi32]; lib.zly_detect_tiled.restype = i32
    lib.zly_surfaces_enable.argtypes = [vp, i32, sz]; lib.zly_surfaces_enable.restype = i32
    lib.zly_surface_define.argtypes = [vp, i32, i32, i32, i32]; lib.zly_surface_define.restype = i32
    lib.zly_surface_update.argtypes = [vp, i32, C.POINTER(SurfaceRect), C.POINTER(vp), C.POINTER(sz), pv]; lib.zly_surface_update.restype = i32
    lib.zly_surface_read.argtypes = [vp, i32, vp, sz]; lib.zly_surface_read.restype = i32
    lib.zly_detect_surfaces.argtypes = [vp, i32, pi32, C.POINTER(Roi), vp, u32, vp]; lib.zly_detect_surfaces.restype = i32
    lib.zly_detect_delta.argtypes = [vp, i32, C.POINTER(SurfaceRect), C.POINTER(vp), C.POINTER(sz), pv, i32, pi32, vp, i32, pi32]; lib.zly_detect_delta.restype = i32
    lib.zly_surface_moves_enable.argtypes = [vp, sz]; lib.zly_surface_moves_enable.restype = i32
    lib.zly_surface_move.argtypes = [vp, i32, C.POINTER(SurfaceMove)]; lib.zly_surface_move.restype = i32
    lib.zly_default_zoom_config.argtypes = [vp, C.POINTER(ZoomConfig)]; lib.zly_default_zoom_config.restype = None
    lib.zly_zoom_enable.argtypes = [vp, C.POINTER(ZoomConfig)]; lib.zly_zoom_enable.restype = i32
    lib.zly_detect_device_zoom.argtypes = [vp, i32, vp, sz, pv, pi32, C.POINTER(MergeConfig), vp, u32, vp]; lib.zly_detect_device_zoom.restype = i32
    lib.zly_detect_surfaces_zoom.argtypes = [vp, i32, pi32, pi32, C.POINTER(MergeConfig), vp, u32, vp]; lib.zly_detect_surfaces_zoom.restype = i32
    lib.zly_zoom_plan.argtypes = [vp, i32, pi32, pi32, pi32, vp]; lib.zly_zoom_plan.restype = i32
    lib.zly_zoom_read_plan.argtypes = [vp, i32, vp]; lib.zly_zoom_read_plan.restype = i32
    psz = C.POINTER(sz)
    lib.zly_default_chip_config.argtypes = [vp, C.POINTER(ChipConfig)]; lib.zly_default_chip_config.restype = None
    lib.zly_chips_enable.argtypes = [vp, C.POINTER(ChipConfig)]; lib.zly_chips_enable.restype = i32
    lib.zly_chip_layout.argtypes = [vp, psz, psz, psz]; lib.zly_chip_layout.restype = i32
    lib.zly_chips_device_view.argtypes = [vp, i32, vp, sz, pv, vp, i32, vp, vp]; lib.zly_chips_device_view.restype = i32
    lib.zly_chips_surfaces.argtypes = [vp, i32, pi32, vp, i32, vp, vp]; lib.zly_chips_surfaces.restype = i32
    lib.zly_read_chips.argtypes = [vp, i32, vp]; lib.zly_read_chips.restype = i32
    lib.zly_default_change_config.argtypes = [vp, C.POINTER(ChangeConfig)]; lib.zly_default_change_config.restype = None
    lib.zly_change_enable.argtypes = [vp, C.POINTER(ChangeConfig), i32]; lib.zly_change_enable.restype = i32
    lib.zly_change_layout.argtypes = [vp, psz, psz, psz]; lib.zly_change_layout.restype = i32
    lib.zly_change_device_view.argtypes = [vp, i32, vp, sz, pv, pi32, vp]; lib.zly_change_device_view.restype = i32
    lib.zly_change_surfaces.argtypes = [vp, i32, pi32, pi32, vp]; lib.zly_change_surfaces.restype = i32
    lib.zly_change_read.argtypes = [vp, i32, vp, sz]; lib.zly_change_read.restype = i32
    lib.zly_change_reset.argtypes = [vp, i32]; lib.zly_change_reset.restype = i32
    lib.zly_zoom_use_change.argtypes = [vp, i32]; lib.zly_zoom_use_change.restype = i32
    lib.zly_default_camera_config.argtypes = [C.POINTER(CameraConfig)]; lib.zly_default_camera_config.restype = None
    lib.zly_camera_enable.argtypes = [vp, C.POINTER(CameraConfig), i32]; lib.zly_camera_enable.restype = i32
    lib.zly_camera_layout.argtypes = [vp, psz, psz, psz]; lib.zly_camera_layout.restype = i32
    lib.zly_camera_device_view.argtypes = [vp, i32, vp, sz, pv, pi32, vp]; lib.zly_camera_device_view.restype = i32
    lib.zly_camera_surfaces.argtypes = [vp, i32, pi32, pi32, vp]; lib.zly_camera_surfaces.restype = i32
    lib.zly_camera_read.argtypes = [vp, i32, vp, sz]; lib.zly_camera_read.restype = i32
    lib.zly_camera_reset.argtypes = [vp, i32]; lib.zly_camera_reset.restype = i32
    lib.zly_camera_apply_tracks.argtypes = [vp, i32, pi32, vp]; lib.zly_camera_apply_tracks.restype = i32
    lib.zly_forward.argtypes = [vp, i32, vp, vp]; lib.zly_forward.restype = i32
    lib.zly_head_tensor.argtypes = [vp, i32, vp]; lib.zly_head_tensor.restype = i32
    lib.zly_postprocess.argtypes = [vp, vp, i32, i32, i32, i32, f32, f32, vp, i32, pi32, pi32]; lib.zly_postprocess.restype = i32
    lib.zly_debug_tap.argtypes = [vp, C.c_char_p, i32, vp, sz, pi32, pi32, pi32]; lib.zly_debug_tap.restype = i32
    lib.zly_num_classes.argtypes = [vp]; lib.zly_num_classes.restype = i32
    lib.zly_num_anchors.argtypes = [vp]; lib.zly_num_anchors.restype = i32
    lib.zly_weights_fp8.argtypes = [vp]; lib.zly_weights_fp8.restype = i32
    lib.zly_num_ops.argtypes = [vp]; lib.zly_num_ops.restype = i32
    lib.zly_op_info_at.argtypes = [vp, i32, C.POINTER(OpInfo)]; lib.zly_op_info_at.restype = i32
    lib.zly_launch_info_at.argtypes = [vp, i32, i32, C.POINTER(LaunchInfo)]; lib.zly_launch_info_at.restype = i32
    lib.zly_op_kernel_name.argtypes = [vp, i32, i32, C.c_char_p, sz]; lib.zly_op_kernel_name.restype = i32
    lib.zly_profile_ops.argtypes = [vp, i32, vp, i32, i32, i32, vp]; lib.zly_profile_ops.restype = i32
    lib.zly_get_stats.argtypes = [vp, C.POINTER(Stats)]; lib.zly_get_stats.restype = i32
    if path is None:
        _lib = lib
    return lib


def frame_bytes(fmt: int, w: int, h: int) -> int:
    """bytes of one w x h frame of format fmt (PIX_*): 3wh for BGR / RGB, 4wh for BGRA / RGBA, 3wh/2 for YUV 4:2:0, 2wh for packed 4:2:2; 0 for an unknown format or invalid sizes (host only)"""
    return int(load_library().zly_frame_bytes(fmt, w, h))


def letterbox_geometry(w: int, h: int, model_w: int, model_h: int) -> Tuple[int, int, int, int]:
    """(nw, nh, pad_x, pad_y): where a w x h request lands in the model_w x model_h tensor of a FLAG_LETTERBOX engine (host only)"""
    lib = load_library()
    o = [C.c_int32() for _ in range(4)]
    _check(lib, lib.zly_letterbox_geometry(w, h, model_w, model_h, *[C.byref(x) for x in o]))
    return tuple(int(x.value) for x in o)


def view_tight(fmt: int, w: int, h: int) -> FrameView:
    """the view of a tight w x h frame of format fmt (host only)"""
    lib = load_library()
    v = FrameView()
    _check(lib, lib.zly_view_tight(fmt, w, h, C.byref(v)))
    return v


def view_crop(surface: FrameView, x0: int, y0: int, w: int, h: int) -> FrameView:
    """the view of the rectangle (x0, y0, w, h) of a view; crops compose (host only)"""
    lib = load_library()
    v = FrameView()
    _check(lib, lib.zly_view_crop(C.byref(surface), x0, y0, w, h, C.byref(v)))
    return v


def view_bytes(v: FrameView) -> int:
    """the smallest buffer that holds the view; 0 for an invalid view (host only)"""
    return int(load_library().zly_view_bytes(C.byref(v)))


def tile(x0: int, y0: int, w: int, h: int, W: int, H: int, group: int = 0) -> Tile:
    return Tile(group, x0, y0, w, h, W, H)


def tile_grid(W: int, H: int, tile_w: int, tile_h: int, overlap_x: int = 0, overlap_y: int = 0, even: bool = False) -> List[Tile]:
    """the row-major tiles of a W x H surface (zly_tile_grid; host only): every tile full-sized, the last of an axis shifted back"""
    lib = load_library()
    n = C.c_int32(0)
    _check(lib, lib.zly_tile_grid(W, H, tile_w, tile_h, overlap_x, overlap_y, 1 if even else 0, None, 0, C.byref(n)))
    out = (Tile * max(n.value, 1))()
    _check(lib, lib.zly_tile_grid(W, H, tile_w, tile_h, overlap_x, overlap_y, 1 if even else 0, out, n.value, C.byref(n)))
    return [Tile(t.group, t.x0, t.y0, t.w, t.h, t.W, t.H) for t in out[:n.value]]


def merge_config(metric: Optional[int] = None, thr: Optional[float] = None) -> MergeConfig:
    """zly_default_merge_config (IoS at 0.5) with the given fields replaced"""
    c = MergeConfig()
    load_library().zly_default_merge_config(C.byref(c))
    if metric is not None:
        c.metric = metric
    if thr is not None:
        c.thr = thr
    return c


def _dims(frame: np.ndarray, fmt: int, w: Optional[int], h: Optional[int]) -> Tuple[int, int]:
    """(w, h) of a request: packed frames carry them in their shape ([h][w][3] for BGR / RGB, [h][w][4] for BGRA / RGBA); a YUV frame, or a
    packed one given as a flat u8 buffer, needs explicit w, h"""
    if fmt in _PACKED_BPP and frame.ndim == 3:
        if frame.shape[2] != _PACKED_BPP[fmt]:
            raise ValueError(f"a frame of format {fmt} is [h][w][{_PACKED_BPP[fmt]}], got shape {frame.shape}")
        return (w if w is not None else frame.shape[1]), (h if h is not None else frame.shape[0])
    if w is None or h is None:
        raise ValueError("a YUV frame (1-D u8 buffer) needs explicit w and h")
    return w, h


def _check(lib, rc: int):
    if rc != OK:
        raise ZlyError(rc, (lib.zly_last_error() or b"").decode(errors="replace"))


class Engine:
    """Thin object wrapper over a zly_engine handle."""

    def __init__(self, weights: Optional[str] = None, model_w: int = 416, model_h: int = 416, conf_thr: float = 0.5,
                 iou_thr: float = 0.45, max_batch: int = 1, max_dets: int = 64, device: int = 0,
                 dtype: int = DTYPE_BF16, warmup_runs: int = 1, use_graph: bool = True, flags: int = 0):
        self.lib = load_library()
        cfg = Config()
        self.lib.zly_default_config(C.byref(cfg))
        self._wpath = (weights or DEFAULT_WEIGHTS).encode()
        cfg.weights_path = self._wpath
        cfg.model_w, cfg.model_h = model_w, model_h
        cfg.conf_thr, cfg.iou_thr = conf_thr, iou_thr
        cfg.max_batch, cfg.max_dets, cfg.device, cfg.dtype = max_batch, max_dets, device, dtype
        cfg.warmup_runs, cfg.use_graph = warmup_runs, 1 if use_graph else 0
        cfg.flags = flags
        self.cfg = cfg
        h = C.c_void_p()
        _check(self.lib, self.lib.zly_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.model_w, self.model_h, self.max_batch, self.max_dets = model_w, model_h, max_batch, max_dets
        self.zoom_regions = 0             # K, once zoom_enable has been called
        self.nc = self.lib.zly_num_classes(h)
        self.weights_fp8 = bool(self.lib.zly_weights_fp8(h))
        self.N = self.lib.zly_num_anchors(h)
        self.slab_bytes = int(self.lib.zly_slab_bytes(h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.zly_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- whole path --------------------------------------------------------------------------------
    def detect(self, frame: np.ndarray, cap: Optional[int] = None, nbytes: Optional[int] = None,
               w: Optional[int] = None, h: Optional[int] = None, fmt: int = PIX_BGR) -> Tuple[np.ndarray, int]:
        """frame: u8 [h][w][3] BGR, or (fmt = PIX_NV12_* / PIX_I420_*) a 1-D u8 YUV 4:2:0 buffer with explicit w, h.
        -> (detections[min(n,cap)], n)."""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        if fmt == PIX_BGR:
            hh, ww = (frame.shape[0], frame.shape[1]) if frame.ndim == 3 else (h, w)
            ww = w if w is not None else ww
            hh = h if h is not None else hh
        else:
            ww, hh = _dims(frame, fmt, w, h)
        cap = cap or self.max_dets
        out = np.zeros(cap, dtype=DET_DTYPE)
        n = C.c_int32(0)
        nb = frame.nbytes if nbytes is None else nbytes
        if fmt == PIX_BGR:
            _check(self.lib, self.lib.zly_detect(self.h, frame.ctypes.data, nb, ww, hh, out.ctypes.data, cap, C.byref(n)))
        else:
            _check(self.lib, self.lib.zly_detect_fmt(self.h, fmt, frame.ctypes.data, nb, ww, hh, out.ctypes.data, cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    def detect_batch(self, frames: Sequence[np.ndarray], cap: Optional[int] = None, fmt=None,
                     ws: Optional[Sequence[int]] = None, hs: Optional[Sequence[int]] = None) -> List[Tuple[np.ndarray, int]]:
        """fmt: None (all BGR), one PIX_* for every frame, or a list with one per frame (formats may mix);
        ws / hs: the sizes of the YUV frames (BGR frames carry theirs in their shape)"""
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        n = len(frames)
        cap = cap or self.max_dets
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        nbytes = (C.c_size_t * n)(*[f.nbytes for f in frames])
        out = np.zeros((n, cap), dtype=DET_DTYPE)
        n_out = (C.c_int32 * n)()
        if fmt is None:
            cws = (C.c_int32 * n)(*[f.shape[1] for f in frames])
            chs = (C.c_int32 * n)(*[f.shape[0] for f in frames])
            _check(self.lib, self.lib.zly_detect_batch(self.h, n, ptrs, nbytes, cws, chs, out.ctypes.data, cap, n_out))
        else:
            fl = [fmt] * n if isinstance(fmt, int) else list(fmt)
            dims = [_dims(f, fl[i], None if ws is None else ws[i], None if hs is None else hs[i]) for i, f in enumerate(frames)]
            cws = (C.c_int32 * n)(*[d[0] for d in dims])
            chs = (C.c_int32 * n)(*[d[1] for d in dims])
            cfm = (C.c_int32 * n)(*fl)
            _check(self.lib, self.lib.zly_detect_batch_fmt(self.h, n, cfm, ptrs, nbytes, cws, chs, out.ctypes.data, cap, n_out))
        return [(out[i, :min(n_out[i], cap)], int(n_out[i])) for i in range(n)]

    def detect_view(self, buf: np.ndarray, view: FrameView, cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
        """buf: the caller's whole u8 buffer (a surface); view: where the request lies in it"""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        cap = cap or self.max_dets
        out = np.zeros(cap, dtype=DET_DTYPE)
        n = C.c_int32(0)
        _check(self.lib, self.lib.zly_detect_view(self.h, buf.ctypes.data, buf.nbytes, C.byref(view), out.ctypes.data, cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    def detect_batch_view(self, bufs: Sequence[np.ndarray], views: Sequence[FrameView], cap: Optional[int] = None) -> List[Tuple[np.ndarray, int]]:
        bufs = [np.ascontiguousarray(b, dtype=np.uint8) for b in bufs]
        n = len(bufs)
        cap = cap or self.max_dets
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        nbytes = (C.c_size_t * n)(*[b.nbytes for b in bufs])
        cv = (FrameView * n)(*views)
        out = np.zeros((n, cap), dtype=DET_DTYPE)
        n_out = (C.c_int32 * n)()
        _check(self.lib, self.lib.zly_detect_batch_view(self.h, n, ptrs, nbytes, cv, out.ctypes.data, cap, n_out))
        return [(out[i, :min(n_out[i], cap)], int(n_out[i])) for i in range(n)]

    # -- asynchronous, pipelined host-to-host path ---------------------------------------------------
    def submit_view(self, buf: np.ndarray, view: FrameView) -> int:
        """copies the view's rows into the engine's pinned staging ring (on this thread) and returns a ticket"""
        t = C.c_uint64(0)
        _check(self.lib, self.lib.zly_submit_view(self.h, buf.ctypes.data, buf.nbytes, C.byref(view), C.byref(t)))
        return t.value

    def submit_view_tracked(self, buf: np.ndarray, view: FrameView, stream: int) -> int:
        """submit_view plus the frame's stream index (-1 = untracked): its detections come back with track ids"""
        t = C.c_uint64(0)
        _check(self.lib, self.lib.zly_submit_view_tracked(self.h, buf.ctypes.data, buf.nbytes, C.byref(view), stream, C.byref(t)))
        return t.value

    # -- tracking (include/zly.h "tracking") ------------------------------------------------------------
    def track_enable(self, max_streams: Optional[int] = None, max_tracks: Optional[int] = None, match_iou: Optional[float] = None,
                     max_lost: Optional[int] = None):
        """once per engine, before the first tracked call; arguments left out keep zly_default_track_config's values"""
        c = TrackConfig()
        self.lib.zly_default_track_config(C.byref(c))
        if max_streams is not None:
            c.max_streams = max_streams
        if max_tracks is not None:
            c.max_tracks = max_tracks
        if match_iou is not None:
            c.match_iou = match_iou
        if max_lost is not None:
            c.max_lost = max_lost
        _check(self.lib, self.lib.zly_track_enable(self.h, C.byref(c)))

    def track_reset(self, stream: int = -1, first_id: int = 0):
        _check(self.lib, self.lib.zly_track_reset(self.h, stream, first_id))

    def track_state(self, stream: int) -> dict:
        s = TrackState()
        _check(self.lib, self.lib.zly_track_state_at(self.h, stream, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in TrackState._fields_}

    def track_motion_enable(self, beta: Optional[float] = None, v_max: Optional[float] = None):
        """once per engine, after track_enable: every tracked call from then on runs the constant-velocity motion step; arguments left out keep
        zly_default_track_motion_config's values"""
        c = TrackMotionConfig()
        self.lib.zly_default_track_motion_config(C.byref(c))
        if beta is not None:
            c.beta = beta
        if v_max is not None:
            c.v_max = v_max
        _check(self.lib, self.lib.zly_track_motion_enable(self.h, C.byref(c)))

    def track_read(self, stream: int) -> np.ndarray:
        """the stream's live slots in ascending slot order, as TRACK_DTYPE records (vx, vy, hits = 0 on an engine without the motion model)"""
        out = np.zeros(64, dtype=TRACK_DTYPE)
        n = C.c_int32(0)
        _check(self.lib, self.lib.zly_track_read(self.h, stream, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value].copy()

    def track_slabs(self, streams: Sequence[int], d_slabs_ptr: int = 0, stream: int = 0):
        """tracks, in place, the len(streams) slabs of the most recent detect_device* call (d_slabs_ptr = 0: the engine's own buffer); -1 = untouched"""
        n = len(streams)
        cs = (C.c_int32 * n)(*streams)
        _check(self.lib, self.lib.zly_track_slabs(self.h, n, cs, d_slabs_ptr or None, stream or None))

    # -- tiles (include/zly.h "Tiles") ------------------------------------------------------------------
    def merge_slabs(self, tiles: Sequence[Tile], n_groups: int = 1, metric: Optional[int] = None, thr: Optional[float] = None, d_slabs_ptr: int = 0,
                    d_out_ptr: int = 0, tag0: int = 0, stream: int = 0):
        """merges the len(tiles) slabs of the most recent detect_device* call (d_slabs_ptr = 0: the engine's own buffer) into n_groups slabs at
        d_out_ptr (0: the engine-owned merge buffer, read with read_merged); enqueued, not synchronised"""
        n = len(tiles)
        ct = (Tile * n)(*tiles)
        c = merge_config(metric, thr)
        _check(self.lib, self.lib.zly_merge_slabs(self.h, n, ct, n_groups, C.byref(c), d_slabs_ptr or None, d_out_ptr or None, tag0, stream or None))

    def read_merged(self, n_groups: int = 1) -> List[Tuple[np.ndarray, np.ndarray]]:
        raw = np.zeros(n_groups * self.slab_bytes, dtype=np.uint8)
        _check(self.lib, self.lib.zly_read_merged(self.h, n_groups, raw.ctypes.data))
        return parse_slabs(raw, n_groups, self.max_dets)

    def detect_tiled(self, buf: np.ndarray, surface: FrameView, tiles: Sequence[Tile], metric: Optional[int] = None, thr: Optional[float] = None,
                     cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
        """buf: the surface in host memory, uploaded once; tiles: rectangles of it, detected in one call and merged as one group
        -> (detections[min(n, cap)] in surface fractions, n)"""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        cap = cap or self.max_dets
        n_t = len(tiles)
        ct = (Tile * n_t)(*tiles)
        c = merge_config(metric, thr)
        out = np.zeros(cap, dtype=DET_DTYPE)
        n = C.c_int32(0)
        _check(self.lib, self.lib.zly_detect_tiled(self.h, buf.ctypes.data, buf.nbytes, C.byref(surface), n_t, ct, C.byref(c), out.ctypes.data, cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    # -- resident surfaces (include/zly.h "Resident surfaces") ---------------------------------------------
    def surfaces_enable(self, max_surfaces: int, max_bytes_each: int):
        """once per engine: one HBM store of max_surfaces slots"""
        _check(self.lib, self.lib.zly_surfaces_enable(self.h, max_surfaces, max_bytes_each))

    def surface_define(self, s: int, fmt: int, w: int, h: int):
        """slot s now holds a tight w x h frame of format fmt and is not valid until a rectangle covers it whole"""
        _check(self.lib, self.lib.zly_surface_define(self.h, s, fmt, w, h))

    @staticmethod
    def _rect_args(rects):
        """rects: (surface, x0, y0, buf, view) each -- view (a FrameView) says where the rectangle's samples lie in the host u8 array buf"""
        n = len(rects)
        bufs = [np.ascontiguousarray(r[3], dtype=np.uint8) for r in rects]
        cr = (SurfaceRect * max(n, 1))(*[SurfaceRect(r[0], r[1], r[2]) for r in rects])
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        nbytes = (C.c_size_t * max(n, 1))(*[b.nbytes for b in bufs])
        cv = (FrameView * max(n, 1))(*[r[4] for r in rects])
        return n, cr, ptrs, nbytes, cv, bufs

    def surface_update(self, rects):
        """writes the rectangles into the store: one staged upload, one kernel launch; enqueued, not synchronised"""
        n, cr, ptrs, nbytes, cv, _keep = self._rect_args(rects)
        _check(self.lib, self.lib.zly_surface_update(self.h, n, cr, ptrs, nbytes, cv))

    def surface_read(self, s: int, nbytes: int) -> np.ndarray:
        """the slot's current bytes (synchronises)"""
        out = np.zeros(nbytes, dtype=np.uint8)
        _check(self.lib, self.lib.zly_surface_read(self.h, s, out.ctypes.data, out.nbytes))
        return out

    def detect_surfaces(self, surfaces: Sequence[int], rois=None, d_slabs_ptr: int = 0, tag0: int = 0, stream: int = 0):
        """the device path on resident surfaces; rois: None or one (x0, y0, w, h) per surface"""
        n = len(surfaces)
        cs = (C.c_int32 * n)(*surfaces)
        cr = None if rois is None else (Roi * n)(*[Roi(*r) for r in rois])
        _check(self.lib, self.lib.zly_detect_surfaces(self.h, n, cs, cr, d_slabs_ptr or None, tag0, stream or None))

    def detect_delta(self, rects, surfaces: Sequence[int], cap: Optional[int] = None) -> List[Tuple[np.ndarray, int]]:
        """surface_update(rects), then the named surfaces detected whole and read back (synchronous)"""
        nr, cr, ptrs, nbytes, cv, _keep = self._rect_args(rects)
        n = len(surfaces)
        cs = (C.c_int32 * n)(*surfaces)
        cap = cap or self.max_dets
        out = np.zeros((n, cap), dtype=DET_DTYPE)
        n_out = (C.c_int32 * n)()
        _check(self.lib, self.lib.zly_detect_delta(self.h, nr, cr, ptrs, nbytes, cv, n, cs, out.ctypes.data, cap, n_out))
        return [(out[i, :min(n_out[i], cap)], int(n_out[i])) for i in range(n)]

    def surface_moves_enable(self, scratch_bytes: int = 0):
        """once per engine, after surfaces_enable: the bounce buffer of surface_move (0: one slot stride)"""
        _check(self.lib, self.lib.zly_surface_moves_enable(self.h, scratch_bytes))

    def surface_move(self, moves):
        """moves: (surface, sx, sy, dx, dy, w, h) each, applied in order inside the store (memmove semantics); enqueued, not synchronised"""
        n = len(moves)
        cm = (SurfaceMove * max(n, 1))(*[SurfaceMove(*m) for m in moves])
        _check(self.lib, self.lib.zly_surface_move(self.h, n, cm))

    # -- zoom regions (include/zly.h "Zoom regions") ---------------------------------------------------------
    def zoom_enable(self, regions: Optional[int] = None, region_w: Optional[int] = None, region_h: Optional[int] = None, max_age: Optional[int] = None,
                    class_id: Optional[int] = None):
        """once per engine, after track_enable; arguments left out keep zly_default_zoom_config's values (3 regions of the model's size, max_age 2, any class)"""
        c = ZoomConfig()
        self.lib.zly_default_zoom_config(self.h, C.byref(c))
        for name, v in (("regions", regions), ("region_w", region_w), ("region_h", region_h), ("max_age", max_age), ("class_id", class_id)):
            if v is not None:
                setattr(c, name, v)
        _check(self.lib, self.lib.zly_zoom_enable(self.h, C.byref(c)))
        self.zoom_regions = c.regions

    def detect_device_zoom(self, d_base_ptr: int, buf_bytes: int, surface_views: Sequence[FrameView], streams: Sequence[int], metric: Optional[int] = None,
                           thr: Optional[float] = None, d_out_ptr: int = 0, tag0: int = 0, stream: int = 0):
        """one frame per surface view of the device buffer: the whole surface and its planned regions detected in one batch, merged (d_out_ptr = 0: the
        engine-owned merge buffer, read with read_merged) and tracked with streams[i]; enqueued, not synchronised"""
        n = len(surface_views)
        cv = (FrameView * n)(*surface_views)
        cs = (C.c_int32 * len(streams))(*streams)
        c = merge_config(metric, thr)
        _check(self.lib, self.lib.zly_detect_device_zoom(self.h, n, d_base_ptr or None, buf_bytes, cv, cs, C.byref(c), d_out_ptr or None, tag0, stream or None))

    def detect_surfaces_zoom(self, surfaces: Sequence[int], streams: Sequence[int], metric: Optional[int] = None, thr: Optional[float] = None,
                             d_out_ptr: int = 0, tag0: int = 0, stream: int = 0):
        """detect_device_zoom on resident surfaces"""
        n = len(surfaces)
        cf = (C.c_int32 * n)(*surfaces)
        cs = (C.c_int32 * len(streams))(*streams)
        c = merge_config(metric, thr)
        _check(self.lib, self.lib.zly_detect_surfaces_zoom(self.h, n, cf, cs, C.byref(c), d_out_ptr or None, tag0, stream or None))

    def zoom_plan(self, sizes: Sequence[Tuple[int, int]], streams: Sequence[int]) -> np.ndarray:
        """the plan kernel alone (synchronous): sizes[i] = (W, H) of the frame of streams[i] -> ZOOM_REGION_DTYPE[len(sizes)][K]"""
        n = len(sizes)
        cw = (C.c_int32 * n)(*[s[0] for s in sizes])
        ch = (C.c_int32 * n)(*[s[1] for s in sizes])
        cs = (C.c_int32 * n)(*streams)
        out = np.zeros((n, max(self.zoom_regions, 1)), dtype=ZOOM_REGION_DTYPE)
        _check(self.lib, self.lib.zly_zoom_plan(self.h, n, cw, ch, cs, out.ctypes.data))
        return out

    def zoom_read_plan(self, n: int) -> np.ndarray:
        """the regions of the most recent zoom call of n frames (synchronises) -> ZOOM_REGION_DTYPE[n][K]"""
        out = np.zeros((n, max(self.zoom_regions, 1)), dtype=ZOOM_REGION_DTYPE)
        _check(self.lib, self.lib.zly_zoom_read_plan(self.h, n, out.ctypes.data))
        return out

    # -- chips (include/zly.h "Chips") -----------------------------------------------------------------------
    def chips_enable(self, chip_w: Optional[int] = None, chip_h: Optional[int] = None, max_chips: Optional[int] = None, class_id: Optional[int] = None,
                     scale: Optional[float] = None, layout: Optional[int] = None):
        """once per engine; arguments left out keep zly_default_chip_config's values (64 x 64 BGR8 chips, min(max_dets, 16) per frame, any class, scale 1.25)"""
        c = ChipConfig()
        self.lib.zly_default_chip_config(self.h, C.byref(c))
        for name, v in (("chip_w", chip_w), ("chip_h", chip_h), ("max_chips", max_chips), ("class_id", class_id), ("scale", scale), ("layout", layout)):
            if v is not None:
                setattr(c, name, v)
        _check(self.lib, self.lib.zly_chips_enable(self.h, C.byref(c)))
        self.chip_cfg = c

    def chip_layout(self) -> Tuple[int, int, int]:
        """(bytes of a chip slab, offset of chip 0 in it, bytes from one chip to the next)"""
        o = [C.c_size_t() for _ in range(3)]
        _check(self.lib, self.lib.zly_chip_layout(self.h, *[C.byref(x) for x in o]))
        return tuple(int(x.value) for x in o)

    def chips_device_view(self, d_base_ptr: int, buf_bytes: int, views: Sequence[FrameView], d_slabs_ptr: int = 0, source: int = CHIPS_SRC_SLABS,
                          d_chips_ptr: int = 0, stream: int = 0):
        """chip slab i from view i of the device buffer with the boxes of slab i (d_slabs_ptr = 0: the engine-owned buffer `source` names;
        d_chips_ptr = 0: the engine-owned chip slabs, read with read_chips); enqueued, not synchronised"""
        n = len(views)
        cv = (FrameView * max(n, 1))(*views)
        _check(self.lib, self.lib.zly_chips_device_view(self.h, n, d_base_ptr or None, buf_bytes, cv, d_slabs_ptr or None, source, d_chips_ptr or None, stream or None))

    def chips_surfaces(self, surfaces: Sequence[int], d_slabs_ptr: int = 0, source: int = CHIPS_SRC_SLABS, d_chips_ptr: int = 0, stream: int = 0):
        """chips_device_view on resident surfaces, whole"""
        n = len(surfaces)
        cs = (C.c_int32 * max(n, 1))(*surfaces)
        _check(self.lib, self.lib.zly_chips_surfaces(self.h, n, cs, d_slabs_ptr or None, source, d_chips_ptr or None, stream or None))

    def read_chips(self, n: int) -> np.ndarray:
        """the first n chip slabs of the engine-owned buffer (synchronises) -> u8 [n][slab_bytes]; parse_chip_slab takes one apart"""
        sb = self.chip_layout()[0]
        raw = np.zeros((n, sb), dtype=np.uint8)
        _check(self.lib, self.lib.zly_read_chips(self.h, n, raw.ctypes.data))
        return raw

    # -- change map (include/zly.h "Change map") -------------------------------------------------------------
    def change_enable(self, max_streams: int = 8, cell: Optional[int] = None, threshold_q4: Optional[int] = None, max_active_permille: Optional[int] = None,
                      max_peaks: Optional[int] = None, window_w: Optional[int] = None, window_h: Optional[int] = None):
        """once per engine; arguments left out keep zly_default_change_config's values (cells of 32, 2 luma levels per pixel, 25 % of the cells, 3 peaks,
        windows of the model's size)"""
        c = ChangeConfig()
        self.lib.zly_default_change_config(self.h, C.byref(c))
        for name, v in (("cell", cell), ("threshold_q4", threshold_q4), ("max_active_permille", max_active_permille), ("max_peaks", max_peaks),
                        ("window_w", window_w), ("window_h", window_h)):
            if v is not None:
                setattr(c, name, v)
        _check(self.lib, self.lib.zly_change_enable(self.h, C.byref(c), max_streams))
        self.change_cfg = c

    def change_layout(self) -> Tuple[int, int, int]:
        """(bytes of a stream's change record, offset of the peaks in it, offset of the activity grid)"""
        o = [C.c_size_t() for _ in range(3)]
        _check(self.lib, self.lib.zly_change_layout(self.h, *[C.byref(x) for x in o]))
        return tuple(int(x.value) for x in o)

    def change_device_view(self, d_base_ptr: int, buf_bytes: int, views: Sequence[FrameView], streams: Sequence[int], stream: int = 0):
        """view i of the device buffer is the next frame of streams[i]; enqueued, not synchronised"""
        n = len(views)
        cv = (FrameView * max(n, 1))(*views)
        cs = (C.c_int32 * max(len(streams), 1))(*streams)
        _check(self.lib, self.lib.zly_change_device_view(self.h, n, d_base_ptr or None, buf_bytes, cv, cs, stream or None))

    def change_surfaces(self, surfaces: Sequence[int], streams: Sequence[int], stream: int = 0):
        """change_device_view on resident surfaces, whole"""
        n = len(surfaces)
        cf = (C.c_int32 * max(n, 1))(*surfaces)
        cs = (C.c_int32 * max(len(streams), 1))(*streams)
        _check(self.lib, self.lib.zly_change_surfaces(self.h, n, cf, cs, stream or None))

    def change_read(self, stream: int) -> np.ndarray:
        """the stream's whole record (synchronises) -> u8 [rec_bytes]; parse_change_record takes it apart"""
        raw = np.zeros(self.change_layout()[0], dtype=np.uint8)
        _check(self.lib, self.lib.zly_change_read(self.h, stream, raw.ctypes.data, raw.nbytes))
        return raw

    def change_reset(self, stream: int = -1):
        """the stream (-1: every stream) has no previous grid; enqueued"""
        _check(self.lib, self.lib.zly_change_reset(self.h, stream))

    def zoom_use_change(self, on: bool = True):
        """zoom calls fill their fallback regions from the change map"""
        _check(self.lib, self.lib.zly_zoom_use_change(self.h, 1 if on else 0))

    # -- camera motion (include/zly.h "Camera motion") ------------------------------------------------------
    def camera_enable(self, max_streams: int = 8, cell: Optional[int] = None, radius: Optional[int] = None, max_residual_q4: Optional[int] = None):
        """once per engine; arguments left out keep zly_default_camera_config's values (cells of 16, a radius of 4 cells, 4 luma levels per pixel)"""
        c = CameraConfig()
        self.lib.zly_default_camera_config(C.byref(c))
        for name, v in (("cell", cell), ("radius", radius), ("max_residual_q4", max_residual_q4)):
            if v is not None:
                setattr(c, name, v)
        _check(self.lib, self.lib.zly_camera_enable(self.h, C.byref(c), max_streams))
        self.camera_cfg = c

    def camera_layout(self) -> Tuple[int, int, int]:
        """(bytes of a stream's camera record, offset of the SAD table in it, the table's room in entries)"""
        o = [C.c_size_t() for _ in range(3)]
        _check(self.lib, self.lib.zly_camera_layout(self.h, *[C.byref(x) for x in o]))
        return tuple(int(x.value) for x in o)

    def camera_device_view(self, d_base_ptr: int, buf_bytes: int, views: Sequence[FrameView], streams: Sequence[int], stream: int = 0):
        """view i of the device buffer is the next frame of streams[i]: its shift against the stream's previous frame; enqueued, not synchronised"""
        n = len(views)
        cv = (FrameView * max(n, 1))(*views)
        cs = (C.c_int32 * max(len(streams), 1))(*streams)
        _check(self.lib, self.lib.zly_camera_device_view(self.h, n, d_base_ptr or None, buf_bytes, cv, cs, stream or None))

    def camera_surfaces(self, surfaces: Sequence[int], streams: Sequence[int], stream: int = 0):
        """camera_device_view on resident surfaces, whole"""
        n = len(surfaces)
        cf = (C.c_int32 * max(n, 1))(*surfaces)
        cs = (C.c_int32 * max(len(streams), 1))(*streams)
        _check(self.lib, self.lib.zly_camera_surfaces(self.h, n, cf, cs, stream or None))

    def camera_read(self, stream: int) -> np.ndarray:
        """the stream's whole record (synchronises) -> u8 [rec_bytes]; parse_camera_record takes it apart"""
        raw = np.zeros(self.camera_layout()[0], dtype=np.uint8)
        _check(self.lib, self.lib.zly_camera_read(self.h, stream, raw.ctypes.data, raw.nbytes))
        return raw

    def camera_reset(self, stream: int = -1):
        """the stream (-1: every stream) has no previous grid and no pending shift; enqueued"""
        _check(self.lib, self.lib.zly_camera_reset(self.h, stream))

    def camera_apply_tracks(self, streams: Sequence[int], stream: int = 0):
        """moves the live tracks of the named streams by their pending shifts, which become 0; enqueued, not synchronised"""
        n = len(streams)
        cs = (C.c_int32 * max(n, 1))(*streams)
        _check(self.lib, self.lib.zly_camera_apply_tracks(self.h, n, cs, stream or None))

    def submit(self, frame: np.ndarray, nbytes: Optional[int] = None, fmt: int = PIX_BGR,
               w: Optional[int] = None, h: Optional[int] = None) -> int:
        """copies the frame into the engine's pinned staging ring (on this thread) and returns a ticket"""
        t = C.c_uint64(0)
        if fmt == PIX_BGR:
            _check(self.lib, self.lib.zly_submit(self.h, frame.ctypes.data, frame.nbytes if nbytes is None else nbytes,
                                                 frame.shape[1], frame.shape[0], C.byref(t)))
        else:
            ww, hh = _dims(frame, fmt, w, h)
            _check(self.lib, self.lib.zly_submit_fmt(self.h, fmt, frame.ctypes.data, frame.nbytes if nbytes is None else nbytes,
                                                     ww, hh, C.byref(t)))
        return t.value

    def poll(self, ticket: int) -> bool:
        rc = self.lib.zly_poll(self.h, ticket)
        if rc not in (OK, PENDING):
            _check(self.lib, rc)
        return rc == OK

    def wait(self, ticket: int, cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
        cap = cap or self.max_dets
        out = np.zeros(cap, dtype=DET_DTYPE)
        n = C.c_int32(0)
        _check(self.lib, self.lib.zly_wait(self.h, ticket, out.ctypes.data, cap, C.byref(n)))
        return out[:min(n.value, cap)], n.value

    def detect_device(self, d_frames_ptr: int, n: int, w: int, h: int, d_slabs_ptr: int = 0, tag0: int = 0, stream: int = 0,
                      fmt: int = PIX_BGR):
        """n frames of format fmt in device memory, frame_bytes(fmt, w, h) apart"""
        if fmt == PIX_BGR:
            _check(self.lib, self.lib.zly_detect_device(self.h, n, d_frames_ptr, w, h, d_slabs_ptr or None, tag0, stream or None))
        else:
            _check(self.lib, self.lib.zly_detect_device_fmt(self.h, fmt, n, d_frames_ptr, w, h, d_slabs_ptr or None, tag0, stream or None))

    def detect_device_view(self, d_base_ptr: int, buf_bytes: int, views: Sequence[FrameView], d_slabs_ptr: int = 0, tag0: int = 0, stream: int = 0):
        """len(views) frame views of one device buffer of buf_bytes at d_base_ptr: sizes, formats, pitches and offsets per frame"""
        n = len(views)
        cv = (FrameView * n)(*views)
        _check(self.lib, self.lib.zly_detect_device_view(self.h, n, d_base_ptr, buf_bytes, cv, d_slabs_ptr or None, tag0, stream or None))

    def sync(self):
        _check(self.lib, self.lib.zly_sync(self.h))

    def join(self, stream: int = 0, lag: int = 0):
        """FLAG_ASYNC_NMS: make `stream` wait (on the device) for the NMS of every call so far but the last `lag`"""
        _check(self.lib, self.lib.zly_join(self.h, stream or None, lag))

    def read_slabs(self, n: int) -> List[Tuple[np.ndarray, np.ndarray]]:
        raw = np.zeros(n * self.slab_bytes, dtype=np.uint8)
        _check(self.lib, self.lib.zly_read_slabs(self.h, n, raw.ctypes.data))
        return parse_slabs(raw, n, self.max_dets)

    # -- stage level -------------------------------------------------------------------------------
    def preprocess(self, frame: np.ndarray, nbytes: Optional[int] = None, w: Optional[int] = None, h: Optional[int] = None,
                   fmt: int = PIX_BGR) -> np.ndarray:
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        out = np.zeros((3, self.model_h, self.model_w), dtype=np.float32)
        nb = frame.nbytes if nbytes is None else nbytes
        if fmt == PIX_BGR:
            hh = h if h is not None else frame.shape[0]
            ww = w if w is not None else frame.shape[1]
            _check(self.lib, self.lib.zly_preprocess(self.h, frame.ctypes.data, nb, ww, hh, out.ctypes.data))
        else:
            ww, hh = _dims(frame, fmt, w, h)
            _check(self.lib, self.lib.zly_preprocess_fmt(self.h, fmt, frame.ctypes.data, nb, ww, hh, out.ctypes.data))
        return out

    def preprocess_view(self, buf: np.ndarray, view: FrameView) -> np.ndarray:
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        out = np.zeros((3, self.model_h, self.model_w), dtype=np.float32)
        _check(self.lib, self.lib.zly_preprocess_view(self.h, buf.ctypes.data, buf.nbytes, C.byref(view), out.ctypes.data))
        return out

    def forward(self, images_nchw: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(images_nchw, dtype=np.float32)
        n = x.shape[0]
        out = np.zeros((n, 4 + self.nc, self.N), dtype=np.float32)
        _check(self.lib, self.lib.zly_forward(self.h, n, x.ctypes.data, out.ctypes.data))
        return out

    def head_tensor(self, idx: int = 0) -> np.ndarray:
        out = np.zeros((4 + self.nc, self.N), dtype=np.float32)
        _check(self.lib, self.lib.zly_head_tensor(self.h, idx, out.ctypes.data))
        return out

    def postprocess(self, head: np.ndarray, img_w: int, img_h: int, conf_thr: float = 0.5, iou_thr: float = 0.45,
                    cap: Optional[int] = None) -> Tuple[np.ndarray, int, int]:
        head = np.ascontiguousarray(head, dtype=np.float32)
        ncls, nbox = head.shape[0] - 4, head.shape[1]
        cap = cap or max(nbox, 1)
        out = np.zeros(cap, dtype=DET_DTYPE)
        n, nc = C.c_int32(0), C.c_int32(0)
        _check(self.lib, self.lib.zly_postprocess(self.h, head.ctypes.data, ncls, nbox, img_w, img_h, conf_thr, iou_thr,
                                                  out.ctypes.data, cap, C.byref(n), C.byref(nc)))
        return out[:min(n.value, cap)], n.value, nc.value

    def tap(self, name: str, idx: int = 0) -> np.ndarray:
        cap = 4 * 1024 * 1024
        buf = np.zeros(cap, dtype=np.float32)
        c, h, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(self.lib, self.lib.zly_debug_tap(self.h, name.encode(), idx, buf.ctypes.data, cap, C.byref(c), C.byref(h), C.byref(w)))
        return buf[:c.value * h.value * w.value].reshape(c.value, h.value, w.value).copy()

    # -- introspection -----------------------------------------------------------------------------
    def ops(self) -> List[dict]:
        out = []
        for i in range(self.lib.zly_num_ops(self.h)):
            info = OpInfo()
            _check(self.lib, self.lib.zly_op_info_at(self.h, i, C.byref(info)))
            out.append(dict(name=info.name.decode(), kind=info.kind, flops=info.flops_per_frame, bytes=info.bytes_per_frame))
        return out

    def launches(self, n: int) -> List[dict]:
        """launch groups at batch size n: one record per op (covered_by != index: the op runs inside another op's launch)"""
        out = []
        for i in range(self.lib.zly_num_ops(self.h)):
            li = LaunchInfo()
            _check(self.lib, self.lib.zly_launch_info_at(self.h, i, n, C.byref(li)))
            out.append({k: getattr(li, k) for k, _ in LaunchInfo._fields_})
        return out

    def op_kernels(self, n: int) -> List[str]:
        """kernel (and tile shape) every op launches at batch size n"""
        out = []
        buf = C.create_string_buffer(96)
        for i in range(self.lib.zly_num_ops(self.h)):
            _check(self.lib, self.lib.zly_op_kernel_name(self.h, i, n, buf, 96))
            out.append(buf.value.decode())
        return out

    def profile_ops(self, d_frames_ptr: int, n: int, w: int, h: int, reps: int = 5) -> np.ndarray:
        ms = np.zeros(self.lib.zly_num_ops(self.h), dtype=np.float32)
        _check(self.lib, self.lib.zly_profile_ops(self.h, n, d_frames_ptr, w, h, reps, ms.ctypes.data))
        return ms

    def stats(self) -> dict:
        s = Stats()
        _check(self.lib, self.lib.zly_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}


def parse_slabs(raw: np.ndarray, n: int, cap: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """raw u8 [n * slab_bytes] -> [(header record, detections[min(n_kept, cap)])]."""
    sb = SLAB_HDR_DTYPE.itemsize + cap * DET_DTYPE.itemsize
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(n, sb)
    out = []
    for i in range(n):
        hdr = raw[i, :SLAB_HDR_DTYPE.itemsize].view(SLAB_HDR_DTYPE)[0]
        dets = raw[i, SLAB_HDR_DTYPE.itemsize:].view(DET_DTYPE)
        out.append((hdr, dets[:min(int(hdr["n_kept"]), cap)].copy()))
    return out


def parse_chip_slab(raw: np.ndarray, chip_w: int, chip_h: int, max_chips: int, layout: int, pixels_off: int, chip_stride: int):
    """one chip slab (u8 [slab_bytes]) -> (header record, records[n_chips], chips[n_chips]): chips are u8 [chip_h][chip_w][3] B, G, R for CHIP_BGR8
    and float32 [3][chip_h][chip_w] R, G, B planes for CHIP_RGB_F32"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    hdr = raw[:CHIP_HDR_DTYPE.itemsize].view(CHIP_HDR_DTYPE)[0]
    n = int(hdr["n_chips"])
    recs = raw[CHIP_HDR_DTYPE.itemsize:CHIP_HDR_DTYPE.itemsize + max_chips * CHIP_REC_DTYPE.itemsize].view(CHIP_REC_DTYPE)[:n].copy()
    chips = []
    for j in range(n):
        o = pixels_off + j * chip_stride
        if layout == CHIP_RGB_F32:
            chips.append(raw[o:o + chip_w * chip_h * 12].view(np.float32).reshape(3, chip_h, chip_w).copy())
        else:
            chips.append(raw[o:o + chip_w * chip_h * 3].reshape(chip_h, chip_w, 3).copy())
    return hdr, recs, chips


def parse_change_record(raw: np.ndarray, max_peaks: int):
    """one stream's change record (u8 [rec_bytes]) -> (header record, peaks[n_peaks], activity u32 [gh][gw])"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    hdr = raw[:CHANGE_HDR_DTYPE.itemsize].view(CHANGE_HDR_DTYPE)[0]
    po = CHANGE_HDR_DTYPE.itemsize
    ao = po + max_peaks * CHANGE_PEAK_DTYPE.itemsize
    peaks = raw[po:ao].view(CHANGE_PEAK_DTYPE)[:int(hdr["n_peaks"])].copy()
    act = raw[ao:ao + 4 * int(hdr["n_cells"])].view(np.uint32).reshape(int(hdr["gh"]), int(hdr["gw"])).copy()
    return hdr, peaks, act


def parse_camera_record(raw: np.ndarray, radius: int):
    """one stream's camera motion record (u8 [rec_bytes]) -> (header record, SAD table u64 [2R+1][2R+1], rows dy = -R..R, columns dx = -R..R)"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    hdr = raw[:CAMERA_HDR_DTYPE.itemsize].view(CAMERA_HDR_DTYPE)[0]
    side = 2 * radius + 1
    so = CAMERA_HDR_DTYPE.itemsize
    return hdr, raw[so:so + 8 * side * side].view(np.uint64).reshape(side, side).copy()
