"""The one ctypes binding of libpvnet_vote.so (C ABI: include/pvnet_vote.h, include/pvnet_nn.h) and of the side libraries beside it, each
with a header, a prototype table and an ABI version of its own: ``SIDE_LIBRARIES`` has one row per library (name -> path, version,
table; ``pvnet_amd.build.SIDE_LIBRARIES`` holds the same names' build facts) and ``load_<name>_library()`` loads one.

Owns what the Python front end mirrors of that ABI, each stated once: the library paths and the release / development choice, loading
and the ABI-version check, the prototype of EVERY exported function (``PROTOTYPES``, applied once per loaded library), the image of
``PvnetVoteLayout``, the error codes and the header's constants.  ``voting``, ``pnp``, ``evaluation`` and ``distributed`` take them from
here; tests/test_abi_mirror.py holds every row against the two headers.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpvnet_vote.so")          # release build: the tuning knobs are constants
DEV_LIB_PATH = os.path.join(_HERE, "libpvnet_vote_dev.so")  # development build (-DPVNET_DEV): PVNET_* environment knobs + every kernel variant
# the knobs of the development build (vote_host.hip, load_tuning): with one of them in the environment the Python front end loads
# libpvnet_vote_dev.so instead of the release library -- the knob tests, the fuzz matrix and the tuning tools work through that
TUNING_KNOBS = ("PVNET_SCORE_MODE", "PVNET_SCORE_WGS_PER_CU", "PVNET_SCORE_HPL", "PVNET_SCORE_CHUNK", "PVNET_COMPACT_KG",
                "PVNET_SCORE_XCD", "PVNET_SCORE_ATOMIC", "PVNET_SCORE_LDS_KB", "PVNET_SCORE_ACC", "PVNET_EXACT_FOLD",
                "PVNET_SCORE_RUNS", "PVNET_SCORE_CULL", "PVNET_CULL_Q_MILLI", "PVNET_DEV_STAGES")

# ---- the header's constants (PVNET_<name>; PVNET_VOTE_ABI_VERSION is ABI_VERSION) --------------------------------------------------
ABI_VERSION = 9
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3
MASK_U8, MASK_I16, MASK_I32, MASK_I64, MASK_F32, MASK_LOGITS_F32 = 0, 1, 2, 3, 4, 5
F_LITERAL = 1
F_NO_REFINE = 2
F_VERTEX_F16, F_VERTEX_BF16, F_LOGITS_F16, F_LOGITS_BF16 = 4, 8, 16, 32
F_APPROX = 64        # the round-1/2 "fast" mode: matrix-pipe scoring without the rounding-band re-evaluation
F_BAND_STATS = 128   # development aid: count the re-evaluated cells / literal tests (exact mode)
F_CONCURRENT = 256   # hint: other batches are in flight on other streams (see voting.concurrent_hint)
F_CULL_ALL, F_CULL_NONE = 512, 1024   # exact mode: disc-cull every key-point / none (default: K3 selects per image on the device)
S_SKIPPED, S_SINGULAR, S_NO_INLIER, S_OVERFLOW = 1, 2, 4, 8
NUM_STAGES = 6
STAGE_NAMES = ("mask_bits", "subsample", "compact", "hypotheses", "score", "select_refine")
POSE_W_NONE, POSE_W_EXPLICIT, POSE_W_COV_F32 = 0, 1, 2
METRIC_SYM_PROJECTION = 1


class Layout(C.Structure):
    """ctypes image of ``PvnetVoteLayout`` (include/pvnet_vote.h)."""
    _fields_ = [(n, C.c_int32) for n in ("b", "h", "w", "vn", "hn", "cap", "words", "chunk", "max_chunks", "hpl",
                                          "hgroups", "hn_pad")] + \
               [(n, C.c_size_t) for n in ("off_ctrl", "off_bits", "off_pix", "off_rec", "off_hyp",
                                          "off_partial", "off_counts", "off_win", "off_seg", "off_items", "off_hypb",
                                          "total_bytes")] + \
               [("nseg", C.c_int32), ("wg_g", C.c_int32), ("wg_s", C.c_int32), ("reserved_", C.c_int32), ("cull", C.c_int32)] + \
               [(n, C.c_size_t) for n in ("off_perm", "off_hyps", "off_cnts", "off_hypc")]


# ---- the prototype of every function the two headers declare: name -> (restype, argtypes) -------------------------------------------
_int, _size, _ptr, _f32 = C.c_int, C.c_size_t, C.c_void_p, C.c_float
_i64p = C.POINTER(C.c_int64)   # stride arrays
# the 22 arguments of pvnet_vote_v3: mask part (3), field part (2), sizes (5), thresholds (3), seed, image offset, idxs, flags, out,
# status, workspace + bytes, stream
_V3 = [_ptr, _int, _i64p, _ptr, _i64p] + [_int] * 5 + [_f32, _int, _int, C.c_uint64, _int, _ptr, C.c_uint32, _ptr, _ptr, _ptr, _size,
                                                        _ptr]
_WS_TAIL = [_int] * 6 + [_ptr, _size, _ptr]   # b, h, w, vn, hn, max_num, workspace, bytes, stream (the epilogues of a completed call)
_OP_GENERATE = [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _ptr]
_OP_VOTE = [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _f32, _ptr]
PROTOTYPES = {
    "pvnet_vote_abi_version": (_int, []),
    "pvnet_vote_build_info": (C.c_char_p, []),
    "pvnet_vote_tuning_reload": (None, []),
    "pvnet_vote_layout": (_int, [_int] * 6 + [C.POINTER(Layout)]),
    "pvnet_vote_workspace_bytes": (_size, [_int] * 6),
    "pvnet_vote_v3": (_int, _V3),
    "pvnet_vote_v3_logits": (_int, [_ptr, _i64p, _int, _ptr, _i64p] + _V3[5:]),
    # pvnet_vote_v3 without its mask part, src_div behind b: the layer from its second kernel on, over a workspace the caller filled
    "pvnet_vote_v3_prepared": (_int, _V3[3:6] + [_int] + _V3[6:]),
    "pvnet_vote_v3_profiled": (_int, _V3 + [C.POINTER(_f32)]),
    "pvnet_vote_v3_stage_repeat": (_int, _V3 + [_int, _int, C.POINTER(_f32)]),
    "pvnet_vote_band_margin": (_int, [_f32, _ptr] + _WS_TAIL),
    "pvnet_vote_confidence": (_int, [_ptr, _f32, _ptr, C.c_uint32] + _WS_TAIL),
    "pvnet_vote_distribution": (_int, [_ptr, _ptr] + _WS_TAIL),
    "pvnet_motion_workspace_bytes": (_size, [_int] * 4),
    "pvnet_motion_voting": (_int, [_ptr, _int, _i64p, _ptr, _i64p] + [_int] * 4 + [_ptr, _ptr, _size, _ptr]),
    "pvnet_motion_voting_typed": (_int, [_ptr, _int, _i64p, _ptr, _i64p] + [_int] * 4 + [C.c_uint32, _ptr, _ptr, _size, _ptr]),
    "pvnet_generate_hypothesis": (_int, _OP_GENERATE),
    "pvnet_voting_for_hypothesis": (_int, _OP_VOTE),
    "pvnet_generate_hypothesis_vanishing_point": (_int, _OP_GENERATE),
    "pvnet_voting_for_hypothesis_vanishing_point": (_int, _OP_VOTE),
    "pvnet_pose_solve": (_int, [_ptr, _int, _i64p, _ptr, _ptr, _int, _ptr] + [_int] * 4 + [_ptr] * 4),
    "pvnet_pose_metrics_workspace_bytes": (_size, [_int] * 3),
    "pvnet_pose_metrics": (_int, [_ptr, _ptr, _int] + [_ptr] * 4 + [_int, _int, _ptr, _ptr, _int, _int, _int, C.POINTER(C.c_double)] +
                           [_ptr] * 4 + [_size, _ptr]),
    "pvnet_nearest_workspace_bytes": (_size, [_int, _int]),
    "pvnet_nearest_point_idx": (_int, [_ptr, _ptr, _ptr] + [_int] * 5 + [_ptr, _size, _ptr]),
    "pvnet_rccl_load": (_int, [C.c_char_p]),
    "pvnet_rccl_unique_id": (_int, [_ptr]),
    "pvnet_rccl_comm_init": (_int, [C.POINTER(_ptr), _int, _ptr, _int]),
    "pvnet_rccl_comm_ranks": (_int, [_ptr, C.POINTER(_int)]),
    "pvnet_rccl_comm_destroy": (_int, [_ptr]),
    "pvnet_vote_allgather": (_int, [_ptr, _ptr, _size, _ptr, _ptr]),
}

# ---- libpvnet_head.so (include/pvnet_head.h): a library and a table of its own, bound once like the one above ----------------------
HEAD_LIB_PATH = os.path.join(_HERE, "libpvnet_head.so")
HEAD_ABI_VERSION = 1
HEAD_F_VERTEX_F16, HEAD_F_VERTEX_BF16, HEAD_F_LOGITS_F16, HEAD_F_LOGITS_BF16 = 1, 2, 4, 8
HEAD_F_NT_NONE, HEAD_F_NT_ALL = 16, 32   # measurement aids: which loads are non-temporal (default: targets, weights and mask)
HEAD_S_BAD_LABEL = 1
HEAD_PROTOTYPES = {
    "pvnet_head_abi_version": (_int, []),
    "pvnet_head_metrics_workspace_bytes": (_size, [_int] * 3),
    # seg_pred + strides + classes, vertex_pred + strides, target + strides, weights + strides, mask + dtype + strides, b, h, w, vn,
    # sigma, flags, losses, counts, status, workspace + bytes, stream
    "pvnet_head_metrics": (_int, [_ptr, _i64p, _int, _ptr, _i64p, _ptr, _i64p, _ptr, _i64p, _ptr, _int, _i64p] + [_int] * 4 +
                           [C.c_double, C.c_uint32, _ptr, _ptr, _ptr, _ptr, _size, _ptr]),
}

# ---- libpvnet_train.so (include/pvnet_train.h): the head losses' backward; it takes the HEAD_F_* flags and HEAD_S_* bits above -----
TRAIN_LIB_PATH = os.path.join(_HERE, "libpvnet_train.so")
TRAIN_ABI_VERSION = 1
TRAIN_PROTOTYPES = {
    "pvnet_train_abi_version": (_int, []),
    "pvnet_head_grad_workspace_bytes": (_size, [_int] * 3),
    # the forward's inputs as pvnet_head_metrics takes them (through flags), then upstream, grad_seg + strides, grad_vertex + strides,
    # status, workspace + bytes, stream
    "pvnet_head_grad": (_int, HEAD_PROTOTYPES["pvnet_head_metrics"][1][:18] + [_ptr, _ptr, _i64p, _ptr, _i64p, _ptr, _ptr, _size, _ptr]),
}

# ---- libpvnet_targets.so (include/pvnet_targets.h): the targets from the key-points and the head fused with them; it takes the
# HEAD_F_* flags and HEAD_S_* bits above and adds one flag ----------------------------------------------------------------------------
TARGETS_LIB_PATH = os.path.join(_HERE, "libpvnet_targets.so")
TARGETS_ABI_VERSION = 1
TARGETS_F_MOTION = 64   # the reference's use_motion=True: targets are not normalised
_f32p, _f64p = _ptr, _ptr   # hcoords [b,vn,3] float64, weight_scale [b] float32 (device pointers)
# seg_pred + strides + classes, vertex_pred + strides, hcoords, weight_scale, mask + dtype + strides, b, h, w, vn, sigma, flags
_KP_HEAD = [_ptr, _i64p, _int, _ptr, _i64p, _f64p, _f32p, _ptr, _int, _i64p] + [_int] * 4 + [C.c_double, C.c_uint32]
TARGETS_PROTOTYPES = {
    "pvnet_targets_abi_version": (_int, []),
    # mask + dtype + strides, hcoords, weight_scale, b, h, w, vn, flags, vertex + strides, vertex_weights + strides, stream
    "pvnet_vertex_targets": (_int, [_ptr, _int, _i64p, _f64p, _f32p] + [_int] * 4 + [C.c_uint32, _ptr, _i64p, _ptr, _i64p, _ptr]),
    "pvnet_head_metrics_kp_workspace_bytes": (_size, [_int] * 3),
    # ..., losses, counts, status, workspace + bytes, stream
    "pvnet_head_metrics_kp": (_int, _KP_HEAD + [_ptr, _ptr, _ptr, _ptr, _size, _ptr]),
    "pvnet_head_grad_kp_workspace_bytes": (_size, [_int] * 3),
    # ..., upstream, grad_seg + strides, grad_vertex + strides, status, workspace + bytes, stream
    "pvnet_head_grad_kp": (_int, _KP_HEAD + [_ptr, _ptr, _i64p, _ptr, _i64p, _ptr, _ptr, _size, _ptr]),
}

# ---- libpvnet_class_targets.so (include/pvnet_class_targets.h): the same for label images -- hcoords [b,nk,vn,3] and weight_scale
# [b,nk] per class, picked by the pixel's label; it takes the HEAD_F_* flags, TARGETS_F_MOTION and the HEAD_S_* bits above ----------------
CLASS_TARGETS_LIB_PATH = os.path.join(_HERE, "libpvnet_class_targets.so")
CLASS_TARGETS_ABI_VERSION = 1
CLASS_TARGETS_MAX_CLASSES = 64   # classes including the background (CLASSES_MAX below, by value)
CLASS_TARGETS_MAX_TABLE = 1024   # (classes - 1) * vn, at most
CLASS_TARGETS_PROTOTYPES = {
    "pvnet_class_targets_abi_version": (_int, []),
    # pvnet_vertex_targets' arguments with class_num behind weight_scale
    "pvnet_vertex_targets_classes": (_int, [_ptr, _int, _i64p, _f64p, _f32p] + [_int] * 5 + [C.c_uint32, _ptr, _i64p, _ptr, _i64p, _ptr]),
    "pvnet_head_metrics_ckp_workspace_bytes": (_size, [_int] * 3),
    "pvnet_head_metrics_ckp": (_int, list(TARGETS_PROTOTYPES["pvnet_head_metrics_kp"][1])),
    "pvnet_head_grad_ckp_workspace_bytes": (_size, [_int] * 3),
    "pvnet_head_grad_ckp": (_int, list(TARGETS_PROTOTYPES["pvnet_head_grad_kp"][1])),
}

# ---- libpvnet_augment.so (include/pvnet_augment.h): the augmentation of a training batch; it takes the MASK_* codes and E_* above ---
AUGMENT_LIB_PATH = os.path.join(_HERE, "libpvnet_augment.so")
AUGMENT_ABI_VERSION = 1
AUGMENT_F_MASK, AUGMENT_F_ROTATION, AUGMENT_F_CROP, AUGMENT_F_FLIP, AUGMENT_F_USE_MASK_OUT = 1, 2, 4, 8, 16
AUGMENT_OUT_F32, AUGMENT_OUT_BF16, AUGMENT_OUT_F16 = 0, 1, 2
AUGMENT_S_RANGE, AUGMENT_S_EMPTIED, AUGMENT_S_DEGENERATE, AUGMENT_S_NO_FOREGROUND = 1, 2, 4, 8
AUGMENT_UNIFORMS = 14


class AugmentConfigStruct(C.Structure):
    """ctypes image of ``PvnetAugmentConfig`` (include/pvnet_augment.h)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32)] + \
               [(n, C.c_double) for n in ("min_mask", "max_mask", "overlap_ratio", "resize_hmin", "resize_hmax", "resize_wmin",
                                          "resize_wmax")] + [("mean", C.c_float * 3), ("std", C.c_float * 3)]


_cfgp = C.POINTER(AugmentConfigStruct)
AUGMENT_PROTOTYPES = {
    "pvnet_augment_abi_version": (_int, []),
    "pvnet_augment_workspace_bytes": (_size, [_int]),
    # rgb + strides, mask + dtype + strides, hcoords, uniforms, b, h, w, vn, height, width, cfg, seed, image + dtype, mask_out + dtype,
    # hcoords_out, status, workspace + bytes, stream
    "pvnet_augment": (_int, [_ptr, _i64p, _ptr, _int, _i64p, _ptr, _ptr] + [_int] * 6 + [_cfgp, C.c_uint64, _ptr, _int, _ptr, _int, _ptr,
                             _ptr, _ptr, _size, _ptr]),
    # rgb + strides, b, h, w, cfg, image + dtype, stream
    "pvnet_normalize": (_int, [_ptr, _i64p, _int, _int, _int, _cfgp, _ptr, _int, _ptr]),
}

# ---- libpvnet_color.so (include/pvnet_color.h): the colour jitter, alone or fused behind the augmentation; it takes the MASK_* codes,
# the AUGMENT_OUT_* codes, AugmentConfigStruct and E_* above ---------------------------------------------------------------------------
COLOR_LIB_PATH = os.path.join(_HERE, "libpvnet_color.so")
COLOR_ABI_VERSION = 1
COLOR_UNIFORMS = 5
COLOR_STEP_B, COLOR_STEP_C, COLOR_STEP_S, COLOR_STEP_H = 0, 1, 2, 3


class ColorConfigStruct(C.Structure):
    """ctypes image of ``PvnetColorConfig`` (include/pvnet_color.h)."""
    _fields_ = [(n, C.c_double) for n in ("brightness", "contrast", "saturation", "hue")] + [("mean", C.c_float * 3), ("std", C.c_float * 3)]


_ccfgp = C.POINTER(ColorConfigStruct)
COLOR_PROTOTYPES = {
    "pvnet_color_abi_version": (_int, []),
    "pvnet_color_workspace_bytes": (_size, [_int] * 3),
    # rgb + strides, uniforms, b, h, w, cfg, mask + dtype + strides, maskmul, image + dtype, workspace + bytes, stream
    "pvnet_color_jitter": (_int, [_ptr, _i64p, _ptr, _int, _int, _int, _ccfgp, _ptr, _int, _i64p, _ptr, _ptr, _int, _ptr, _size, _ptr]),
    # pvnet_augment's arguments through seed, then jitter, jitter_uniforms, then pvnet_augment's from image on
    "pvnet_augment_jitter": (_int, AUGMENT_PROTOTYPES["pvnet_augment"][1][:15] + [_ccfgp, _ptr] + AUGMENT_PROTOTYPES["pvnet_augment"][1][15:]),
}

# ---- libpvnet_classes.so (include/pvnet_classes.h): the voting layer's first kernel for a mask of class labels; it takes the MASK_*
# codes and E_* above and fills the workspace pvnet_vote_v3_prepared runs on ------------------------------------------------------------
CLASSES_LIB_PATH = os.path.join(_HERE, "libpvnet_classes.so")
CLASSES_ABI_VERSION = 1
CLASSES_MAX = 64   # classes including the background
CLASSES_LOGITS_F32, CLASSES_LOGITS_F16, CLASSES_LOGITS_BF16 = 0, 1, 2
# source + type + strides, num_classes, b, h, w, max_num, seed, image_base, bits, seg0, cum, stream
_CLASS_SPLIT = [_ptr, _int, _i64p] + [_int] * 5 + [C.c_uint64, _int, _ptr, _ptr, _ptr, _ptr]
CLASSES_PROTOTYPES = {
    "pvnet_classes_abi_version": (_int, []),
    "pvnet_class_split": (_int, _CLASS_SPLIT),
    "pvnet_class_split_logits": (_int, _CLASS_SPLIT),
}

# ---- libpvnet_raster.so (include/pvnet_raster.h): poses and meshes -> silhouettes and label images; it takes E_* above ---------------
RASTER_LIB_PATH = os.path.join(_HERE, "libpvnet_raster.so")
RASTER_ABI_VERSION = 1
RASTER_LANE_PIXELS = 64      # pixels of a triangle's box a single lane walks; larger boxes take the cooperative path
RASTER_MAX_INSTANCES, RASTER_MAX_MESHES, RASTER_MAX_IMAGES, RASTER_MAX_SIDE = 768, 64, 65535, 32768
RASTER_S_NONFINITE, RASTER_S_BEHIND, RASTER_S_BADFACE = 1, 2, 4
_i32p = C.POINTER(C.c_int32)   # host arrays: offsets, mesh ids, image ids, labels
RASTER_PROTOTYPES = {
    "pvnet_raster_abi_version": (_int, []),
    "pvnet_raster_workspace_bytes": (_size, [_int] * 6),   # q, P, T, b, h, w
    # tri, n, tn, h, w, mask_out, status_out, workspace + bytes, stream
    "pvnet_raster_triangles": (_int, [_ptr] + [_int] * 4 + [_ptr, _ptr, _ptr, _size, _ptr]),
    # vertices, faces, vertex_offset, face_offset (host), M, P, T, q, mesh_id (host), poses, K, k_per_instance, image_id, label (host),
    # order, b, h, w, out, tri_out, status_out, workspace + bytes, stream
    "pvnet_render": (_int, [_ptr, _ptr, _i32p, _i32p] + [_int] * 4 + [_i32p, _ptr, _ptr, _int, _i32p, _i32p, _ptr] + [_int] * 3 +
                     [_ptr, _ptr, _ptr, _ptr, _size, _ptr]),
}

# ---- libpvnet_depth.so (include/pvnet_depth.h): poses and meshes -> depth, occlusion-correct labels, visible pixel counts -------------
DEPTH_LIB_PATH = os.path.join(_HERE, "libpvnet_depth.so")
DEPTH_ABI_VERSION = 1
DEPTH_LANE_PIXELS = 64       # as RASTER_LANE_PIXELS
DEPTH_MAX_INSTANCES, DEPTH_MAX_MESHES, DEPTH_MAX_IMAGES, DEPTH_MAX_SIDE = 768, 64, 65535, 32768   # the limits of pvnet_render
DEPTH_S_NONFINITE, DEPTH_S_BEHIND, DEPTH_S_BADFACE = 1, 2, 4
DEPTH_PROTOTYPES = {
    "pvnet_depth_abi_version": (_int, []),
    "pvnet_depth_workspace_bytes": (_size, [_int] * 6),   # q, P, T, b, h, w
    # vertices, faces, vertex_offset, face_offset (host), M, P, T, q, mesh_id (host), poses, K, k_per_instance, image_id, label (host),
    # b, h, w, far, depth_out, label_out, visible_out, status_out, workspace + bytes, stream
    "pvnet_render_depth": (_int, [_ptr, _ptr, _i32p, _i32p] + [_int] * 4 + [_i32p, _ptr, _ptr, _int, _i32p, _i32p] + [_int] * 3 +
                           [_f32, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr]),
}

# ---- libpvnet_shade.so (include/pvnet_shade.h): poses and coloured meshes -> shaded images over a background, with depth's outputs -----
SHADE_LIB_PATH = os.path.join(_HERE, "libpvnet_shade.so")
SHADE_ABI_VERSION = 1
SHADE_LANE_PIXELS = 64       # as DEPTH_LANE_PIXELS
SHADE_MAX_INSTANCES, SHADE_MAX_MESHES, SHADE_MAX_IMAGES, SHADE_MAX_SIDE = 768, 64, 65535, 32768   # the limits of pvnet_render_depth
SHADE_MAX_FACES = 1 << 22    # faces of one mesh: the face index has 22 bits of the z-buffer's word
SHADE_S_NONFINITE, SHADE_S_BEHIND, SHADE_S_BADFACE = 1, 2, 4
SHADE_NONE, SHADE_FLAT, SHADE_PHONG = 0, 1, 2
_u8p = C.POINTER(C.c_uint8)   # host array: the background colour
SHADE_PROTOTYPES = {
    "pvnet_shade_abi_version": (_int, []),
    "pvnet_shade_workspace_bytes": (_size, [_int] * 6),   # q, P, T, b, h, w
    # pvnet_render_depth's arguments through far, then colors, normals, shading, ambient, bg_color (host), bg_image, rgb_out, then
    # depth_out, label_out, visible_out, status_out, workspace + bytes, stream
    "pvnet_render_color": (_int, DEPTH_PROTOTYPES["pvnet_render_depth"][1][:18] + [_ptr, _ptr, _int, _f32, _u8p, _ptr, _ptr] +
                           DEPTH_PROTOTYPES["pvnet_render_depth"][1][18:]),
}

# ---- libpvnet_poses.so (include/pvnet_poses.h): the pose solve behind the per-class vote -- one pose per (image, class) in one launch,
# absent classes gated by the vote's status; it takes E_* and S_SKIPPED above, and its weight kinds are POSE_W_* ---------------------------
POSES_LIB_PATH = os.path.join(_HERE, "libpvnet_poses.so")
POSES_ABI_VERSION = 1
POSES_W_NONE, POSES_W_EXPLICIT, POSES_W_COV_F32 = 0, 1, 2
assert (POSES_W_NONE, POSES_W_EXPLICIT, POSES_W_COV_F32) == (POSE_W_NONE, POSE_W_EXPLICIT, POSE_W_COV_F32)
POSES_MAX_PN, POSES_MAX_CLASSES, POSES_MAX_ITEMS = 64, 63, 178956970
POSES_ABSENT = -3   # status of an item whose vote was skipped: zeros returned
POSES_PROTOTYPES = {
    "pvnet_poses_abi_version": (_int, []),
    # pts2d + float64? + strides[4], pts3d, weights + kind, K + per image?, vote_status, b, nk, pn, max_iterations, rt, poses, status,
    # stream
    "pvnet_pose_solve_classes": (_int, [_ptr, _int, _i64p, _ptr, _ptr, _int, _ptr, _int, _ptr] + [_int] * 4 + [_ptr] * 4),
}

# ---- libpvnet_decoder.so (include/pvnet_decoder.h): a decoder stage in one launch -- upsample, concat, 3 x 3 convolution, LeakyReLU; it
# takes E_* above ----------------------------------------------------------------------------------------------------------------------------
DECODER_LIB_PATH = os.path.join(_HERE, "libpvnet_decoder.so")
DECODER_ABI_VERSION = 1
DECODER_SKIP = 64              # channels of skip
DECODER_T_F32, DECODER_T_F16, DECODER_T_BF16 = 0, 1, 2
DECODER_F_PACKED = 1           # w is the bfloat16 fragment-order image of the weights
DECODER_SHAPES = ((64, 64, 32), (128, 64, 64))   # (cl, cs, co): conv2s and conv4s of Resnet18_8s
DECODER_PROTOTYPES = {
    "pvnet_decoder_abi_version": (_int, []),
    # lo + type + strides, skip + type + strides, w, bias, b, hin, win, h, w_, cl, cs, co, flags, out + type, stream
    "pvnet_decoder_stage": (_int, [_ptr, _int, _i64p, _ptr, _int, _i64p, _ptr, _ptr] + [_int] * 8 + [C.c_uint32, _ptr, _int, _ptr]),
}

# ---- libpvnet_tail.so (include/pvnet_tail.h): the network's tail in one launch -- upsample, concat, 3 x 3 and 1 x 1 convolution; it takes
# E_* above --------------------------------------------------------------------------------------------------------------------------------
TAIL_LIB_PATH = os.path.join(_HERE, "libpvnet_tail.so")
TAIL_ABI_VERSION = 1
TAIL_WIDTH, TAIL_MAX_COUT = 32, 32
TAIL_T_F32, TAIL_T_F16, TAIL_T_BF16 = 0, 1, 2
TAIL_BF16, TAIL_F32 = 0, 1     # precision
TAIL_F_RAW = 1
TAIL_PROTOTYPES = {
    "pvnet_tail_abi_version": (_int, []),
    # fm + type + strides, image + type + strides, w1, b1, w2, b2, b, hin, win, h, w, feat, raw, cout, precision, flags, out + type, stream
    "pvnet_tail_forward": (_int, [_ptr, _int, _i64p, _ptr, _int, _i64p, _ptr, _ptr, _ptr, _ptr] + [_int] * 9 + [C.c_uint32, _ptr, _int, _ptr]),
}

# ---- libpvnet_stem.so (include/pvnet_stem.h): the network's stem in one launch -- 7 x 7 stride-2 convolution, ReLU, 3 x 3 stride-2
# max-pool; it takes E_* above ----------------------------------------------------------------------------------------------------------------
STEM_LIB_PATH = os.path.join(_HERE, "libpvnet_stem.so")
STEM_ABI_VERSION = 1
STEM_CIN, STEM_COUT = 3, 64
STEM_T_F32, STEM_T_F16, STEM_T_BF16 = 0, 1, 2
STEM_PROTOTYPES = {
    "pvnet_stem_abi_version": (_int, []),
    # image + type + strides, w, bias, b, h, w_, x2s, pooled, out type, stream
    "pvnet_stem_forward": (_int, [_ptr, _int, _i64p, _ptr, _ptr, _int, _int, _int, _ptr, _ptr, _int, _ptr]),
}

# ---- libpvnet_texture.so (include/pvnet_texture.h): pvnet_render_color with UV-mapped textures; a mesh without one is shaded as there ----
TEXTURE_LIB_PATH = os.path.join(_HERE, "libpvnet_texture.so")
TEXTURE_ABI_VERSION = 1
TEXTURE_LANE_PIXELS = 64     # as SHADE_LANE_PIXELS
TEXTURE_MAX_INSTANCES, TEXTURE_MAX_MESHES, TEXTURE_MAX_IMAGES, TEXTURE_MAX_IMAGE_SIDE = 768, 64, 65535, 32768   # pvnet_render_color's
TEXTURE_MAX_FACES = 1 << 22  # as SHADE_MAX_FACES
TEXTURE_MAX_SIDE = 16384     # texels along one side of one texture; the table holds fewer than 2^31 texels
TEXTURE_S_NONFINITE, TEXTURE_S_BEHIND, TEXTURE_S_BADFACE = 1, 2, 4
TEXTURE_SHADING_NONE, TEXTURE_SHADING_FLAT, TEXTURE_SHADING_PHONG = 0, 1, 2
TEXTURE_NEAREST, TEXTURE_BILINEAR = 0, 1
_i64p = C.POINTER(C.c_int64)  # host array: the texel offsets
TEXTURE_PROTOTYPES = {
    "pvnet_texture_abi_version": (_int, []),
    "pvnet_texture_workspace_bytes": (_size, [_int] * 6),   # q, P, T, b, h, w
    # pvnet_render_color's arguments through normals, then uv, texels, tex_offset, tex_h, tex_w (host), filter, then its from shading on
    "pvnet_render_textured": (_int, SHADE_PROTOTYPES["pvnet_render_color"][1][:20] + [_ptr, _ptr, _i64p, _i32p, _i32p, _int] +
                              SHADE_PROTOTYPES["pvnet_render_color"][1][20:]),
}

# ---- libpvnet_trunk.so (include/pvnet_trunk.h): a 3 x 3 convolution of the residual trunk in one launch -- one or two inputs, BatchNorm
# folded in, residual and activation on its own accumulators; it takes E_* above -----------------------------------------------------------
TRUNK_LIB_PATH = os.path.join(_HERE, "libpvnet_trunk.so")
TRUNK_ABI_VERSION = 1
TRUNK_MAX_WIDTH = 512          # c1 + c2 and co, at most; each a multiple of 32
TRUNK_CO_GROUP = 128           # output channels of a workgroup
TRUNK_T_F32, TRUNK_T_F16, TRUNK_T_BF16 = 0, 1, 2
assert ((TAIL_T_F32, TAIL_T_F16, TAIL_T_BF16) == (DECODER_T_F32, DECODER_T_F16, DECODER_T_BF16) == (STEM_T_F32, STEM_T_F16, STEM_T_BF16)
        == (TRUNK_T_F32, TRUNK_T_F16, TRUNK_T_BF16)), "the four network libraries share one map of type codes (pvnet_amd/_net.py)"
TRUNK_ACT_NONE, TRUNK_ACT_RELU, TRUNK_ACT_LEAKY = 0, 1, 2
TRUNK_GEOMETRIES = ((1, 1), (2, 1), (1, 2), (1, 4))   # (stride, dilation)
TRUNK_PROTOTYPES = {
    "pvnet_trunk_abi_version": (_int, []),
    # src1 + type + strides, src2 + type + strides, res + type + strides, w, bias, b, h, w_, c1, c2, co, stride, dilation, act,
    # out + type, stream
    "pvnet_conv3x3_fused": (_int, [_ptr, _int, _i64p] * 3 + [_ptr, _ptr] + [_int] * 9 + [_ptr, _int, _ptr]),
}


class SideLibrary(NamedTuple):
    path: str
    abi_version: int      # what pvnet_<name>_abi_version() must answer (PVNET_<NAME>_ABI_VERSION of include/pvnet_<name>.h)
    prototypes: dict      # name -> (restype, argtypes) of every function that header declares


# one row per side library, under the name pvnet_amd.build.SIDE_LIBRARIES builds it by; read when a library is loaded
SIDE_LIBRARIES = {
    "head": SideLibrary(HEAD_LIB_PATH, HEAD_ABI_VERSION, HEAD_PROTOTYPES),
    "train": SideLibrary(TRAIN_LIB_PATH, TRAIN_ABI_VERSION, TRAIN_PROTOTYPES),
    "targets": SideLibrary(TARGETS_LIB_PATH, TARGETS_ABI_VERSION, TARGETS_PROTOTYPES),
    "class_targets": SideLibrary(CLASS_TARGETS_LIB_PATH, CLASS_TARGETS_ABI_VERSION, CLASS_TARGETS_PROTOTYPES),
    "augment": SideLibrary(AUGMENT_LIB_PATH, AUGMENT_ABI_VERSION, AUGMENT_PROTOTYPES),
    "color": SideLibrary(COLOR_LIB_PATH, COLOR_ABI_VERSION, COLOR_PROTOTYPES),
    "classes": SideLibrary(CLASSES_LIB_PATH, CLASSES_ABI_VERSION, CLASSES_PROTOTYPES),
    "raster": SideLibrary(RASTER_LIB_PATH, RASTER_ABI_VERSION, RASTER_PROTOTYPES),
    "depth": SideLibrary(DEPTH_LIB_PATH, DEPTH_ABI_VERSION, DEPTH_PROTOTYPES),
    "shade": SideLibrary(SHADE_LIB_PATH, SHADE_ABI_VERSION, SHADE_PROTOTYPES),
    "poses": SideLibrary(POSES_LIB_PATH, POSES_ABI_VERSION, POSES_PROTOTYPES),
    "trunk": SideLibrary(TRUNK_LIB_PATH, TRUNK_ABI_VERSION, TRUNK_PROTOTYPES),
    "stem": SideLibrary(STEM_LIB_PATH, STEM_ABI_VERSION, STEM_PROTOTYPES),
    "decoder": SideLibrary(DECODER_LIB_PATH, DECODER_ABI_VERSION, DECODER_PROTOTYPES),
    "tail": SideLibrary(TAIL_LIB_PATH, TAIL_ABI_VERSION, TAIL_PROTOTYPES),
    "texture": SideLibrary(TEXTURE_LIB_PATH, TEXTURE_ABI_VERSION, TEXTURE_PROTOTYPES),
}

_lib = None
_libs = {}        # path -> loaded vote library
_side_libs = {}   # name -> loaded side library


def _wanted_library() -> str:
    if os.environ.get("PVNET_VOTE_LIB"):   # development aid: an experimental build of the same ABI
        return os.environ["PVNET_VOTE_LIB"]
    return DEV_LIB_PATH if any(os.environ.get(k) not in (None, "") for k in TUNING_KNOBS) else LIB_PATH


def load_library() -> C.CDLL:
    """dlopen the in-tree HIP library; loud failure if it has not been built (python -m pvnet_amd.build).  The release library unless
    a tuning knob is set in the environment (see TUNING_KNOBS; `reload_tuning()` re-decides after the environment changed)."""
    global _lib
    if _lib is not None:
        return _lib
    _lib = _load(_wanted_library())
    return _lib


def _bound(lib_path: str, prototypes: dict) -> C.CDLL:
    """dlopen a library and give every function of its table its prototype; loud failure if it has not been built"""
    if not os.path.exists(lib_path):
        raise RuntimeError(f"pvnet_amd: HIP library {lib_path} is missing -- build it with "
                           f"`python -m pvnet_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    lib = C.CDLL(lib_path)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def _load(lib_path: str) -> C.CDLL:
    if lib_path not in _libs:
        lib = _bound(lib_path, PROTOTYPES)
        if lib.pvnet_vote_abi_version() != ABI_VERSION:
            raise RuntimeError("pvnet_amd: libpvnet_vote.so ABI version mismatch; rebuild it")
        _libs[lib_path] = lib
    return _libs[lib_path]


def _load_side(name: str) -> C.CDLL:
    """dlopen one of SIDE_LIBRARIES, bind its table, check its ABI version -- once"""
    if name not in _side_libs:
        path, version, prototypes = SIDE_LIBRARIES[name]
        lib = _bound(path, prototypes)
        if getattr(lib, f"pvnet_{name}_abi_version")() != version:
            raise RuntimeError(f"pvnet_amd: libpvnet_{name}.so ABI version mismatch; rebuild it")
        _side_libs[name] = lib
    return _side_libs[name]


# the public spelling, one per row of SIDE_LIBRARIES: loud failure if the library has not been built.  There is no CPU fallback.
load_head_library = functools.partial(_load_side, "head")
load_train_library = functools.partial(_load_side, "train")
load_targets_library = functools.partial(_load_side, "targets")
load_class_targets_library = functools.partial(_load_side, "class_targets")
load_augment_library = functools.partial(_load_side, "augment")
load_color_library = functools.partial(_load_side, "color")
load_classes_library = functools.partial(_load_side, "classes")
load_raster_library = functools.partial(_load_side, "raster")
load_depth_library = functools.partial(_load_side, "depth")
load_shade_library = functools.partial(_load_side, "shade")
load_poses_library = functools.partial(_load_side, "poses")
load_stem_library = functools.partial(_load_side, "stem")
load_decoder_library = functools.partial(_load_side, "decoder")
load_tail_library = functools.partial(_load_side, "tail")
load_texture_library = functools.partial(_load_side, "texture")
load_trunk_library = functools.partial(_load_side, "trunk")


def reload_tuning():
    """the PVNET_* tuning environment changed: pick the library again (release without knobs, the development build with) and have
    the development build re-read them (it reads them once, at its first call; the release build's knobs are constants)."""
    global _lib
    _lib = _load(_wanted_library())
    _lib.pvnet_vote_tuning_reload()


_ERROR_NAMES = {E_BADARG: "PVNET_E_BADARG", E_WORKSPACE: "PVNET_E_WORKSPACE", E_UNSUPPORTED: "PVNET_E_UNSUPPORTED"}


def _check(rc: int, what: str):
    if rc == 0:
        return
    raise RuntimeError(f"{what} failed: {_ERROR_NAMES.get(rc, 'hipError_t ' + str(rc))}")


def vote_layout(b, h, w, vn, hn, max_num) -> Layout:
    L = Layout()
    _check(load_library().pvnet_vote_layout(b, h, w, vn, hn, max_num, C.byref(L)), "pvnet_vote_layout")
    return L
