"""ctypes binding of libposegen_hip.so (include/posegen_hip.h, include/posegen_gan.h, include/posegen_generator.h,
include/posegen_regressor.h, include/posegen_optim.h).

north_star asks for a "thin C-ABI cffi layer"; cffi is not installed in the build
image (and cannot be: no network), so the same C ABI is bound with ctypes from the
standard library.  Nothing here computes: it declares prototypes, loads the library
and turns negative return codes into exceptions.  There is NO CPU fallback -- if
the library is missing every entry point raises `HipLibraryError`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libposegen_hip.so")

PG_OK, PG_EINVAL, PG_ENOMEM, PG_EHIP, PG_ESTATE = 0, -1, -2, -3, -4
PG_FLAG_LINDISP = 1
PG_FLAG_STAGE_ONE_LAUNCH = 256
PG_ACT_RELU, PG_ACT_SOFTPLUS = 0, 1
PG_COMP_PLAIN, PG_COMP_IS_ONLY, PG_COMP_MERGED = 0, 1, 2
PG_ABI_VERSION = 11
PG_METRICS_BG = 1
PG_POSE_ALIGN_NONE, PG_POSE_ALIGN_SCALE, PG_POSE_ALIGN_BEST, PG_POSE_ALIGN_ROTATION = 0, 1, 2, 3
PG_POSE_LOSS_MPJPE, PG_POSE_LOSS_NORM_MATCHED = 0, 1
PG_TRAIN_LOSS_MSE, PG_TRAIN_LOSS_L1, PG_TRAIN_LOSS_HUBER = 0, 1, 2
PG_TRAIN_REG_NONE, PG_TRAIN_REG_BCE, PG_TRAIN_REG_L1, PG_TRAIN_REG_MSE = 0, 1, 2, 3
PG_GRAD_NORMS_MAX = 256


class HipLibraryError(RuntimeError):
    """libposegen_hip.so is missing or unusable (no CPU fallback exists)."""


class PgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"posegen_hip error {code}: {msg}")
        self.code = code


class PgConfig(C.Structure):
    _fields_ = [("n_joints", C.c_int32), ("multires", C.c_int32), ("multires_views", C.c_int32),
                ("multires_bones", C.c_int32), ("net_depth", C.c_int32), ("net_width", C.c_int32),
                ("skip_layer", C.c_int32), ("view_width", C.c_int32), ("framecode_ch", C.c_int32),
                ("n_framecodes", C.c_int32), ("chunk", C.c_int32), ("precision", C.c_int32),
                ("cutoff_dist", C.c_float), ("density_scale", C.c_float), ("rgb_eps", C.c_float),
                ("softplus_shift", C.c_float), ("density_act", C.c_int32), ("single_net", C.c_int32)]


_FP = C.c_void_p  # device float*


class PgTrainDraws(C.Structure):
    """pg_train_draws: the caller's random numbers of one training-mode call."""
    _fields_ = [(k, _FP) for k in ("t_rand", "u_rand", "noise0", "noise1", "ray_noise")]


class PgNetParams(C.Structure):
    """pg_net_params: device pointers of one net's 24 tensors (+ frame codes with the mean row appended)."""
    _fields_ = [("w", _FP * 24), ("codes", _FP), ("n_codes", C.c_int32)]


class PgNetGrads(C.Structure):
    _fields_ = [("w", _FP * 24), ("codes", _FP)]


class PgImageBank(C.Structure):
    """pg_image_bank: the device arrays a training batch is gathered from (bkgd_idxs: host)."""
    _fields_ = [("imgs", C.c_void_p), ("masks", C.c_void_p), ("bkgds", C.c_void_p), ("bkgd_idxs", C.POINTER(C.c_int32)),
                ("c2ws", _FP), ("focals", _FP), ("centers", _FP), ("F", C.c_int64), ("P", C.c_int64), ("n_bkgd", C.c_int64),
                ("n_cam", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("mask_img", C.c_int32)]


PG_SCENE_MAX_PEOPLE = 8


class PgScenePerson(C.Structure):
    """pg_scene_person: one person of a pg_render_scene call (skts, cyl: device pointers; the rest host data)."""
    _fields_ = [("subject", C.c_int32), ("box", C.c_int32 * 4), ("skts", _FP), ("cyl", _FP), ("cam", C.c_float)]


class PgBodyModel(C.Structure):
    """pg_body_model: the device arrays of one SMPL body (blend, skin, rest_joints) and its joint tree."""
    _fields_ = [("V", C.c_int32), ("NB", C.c_int32), ("blend", _FP), ("skin", _FP), ("rest_joints", C.c_void_p),
                ("parents", C.c_int32 * 24)]


class PgCropItem(C.Structure):
    """pg_crop_item: one (image, crop box) item of a pg_regressor_input call (offset: bytes into the pixel buffer)."""
    _fields_ = [("offset", C.c_int64)] + [(k, C.c_int32) for k in ("H", "W", "x0", "y0", "x1", "y1")]


class PgOutputs(C.Structure):
    _fields_ = [(k, _FP) for k in ("rgb_map", "disp_map", "acc_map", "alpha", "rgb0", "disp0", "acc0",
                                   "alpha0", "near_far", "z_coarse", "z_fine", "raw_coarse", "raw_fine",
                                   "weights0")]


PG_DISC_MAX_PATHS, PG_DISC_MAX_POINTS, PG_DISC_LAYERS = 8, 24, 5


class PgDiscPath(C.Structure):
    """pg_disc_path (include/posegen_gan.h): one five-layer path over the rows sel[:n_sel] of a pose"""
    _fields_ = [("n_sel", C.c_int32), ("sel", C.c_int32 * PG_DISC_MAX_POINTS), ("width", C.c_int32), ("mid", C.c_int32)]


class PgDiscSpec(C.Structure):
    _fields_ = [("n_paths", C.c_int32), ("n_points", C.c_int32), ("point_dim", C.c_int32), ("path", PgDiscPath * PG_DISC_MAX_PATHS),
                ("slope", C.c_float)]


class PgDiscParams(C.Structure):
    """pg_disc_params / pg_disc_grads: per path five weight and five bias device pointers, where torch keeps them"""
    _fields_ = [("w", (_FP * PG_DISC_LAYERS) * PG_DISC_MAX_PATHS), ("b", (_FP * PG_DISC_LAYERS) * PG_DISC_MAX_PATHS)]


PG_GEN_MAX_TRUNKS, PG_GEN_MAX_STAGES, PG_GEN_MAX_LAYERS, PG_GEN_MAX_DIM, PG_GEN_MAX_ROWS, PG_GEN_MAX_JOINTS = 4, 4, 9, 512, 1048576, 64


class PgGenTrunk(C.Structure):
    """pg_gen_trunk (include/posegen_generator.h): nz -> width, then n_stages blocks of two width -> width layers"""
    _fields_ = [("nz", C.c_int32), ("width", C.c_int32), ("n_stages", C.c_int32)]


class PgGenSpec(C.Structure):
    _fields_ = [("n_trunks", C.c_int32), ("trunk", PgGenTrunk * PG_GEN_MAX_TRUNKS), ("slope", C.c_float), ("eps", C.c_float),
                ("momentum", C.c_float)]


_GEN_TABLE = (_FP * PG_GEN_MAX_LAYERS) * PG_GEN_MAX_TRUNKS


class PgGenParams(C.Structure):
    """pg_gen_params: per trunk and layer the device pointers of the Linear's and the BatchNorm1d's tensors, where torch keeps them"""
    _fields_ = [(k, _GEN_TABLE) for k in ("w", "b", "gamma", "beta", "running_mean", "running_var")]


class PgGenGrads(C.Structure):
    _fields_ = [(k, _GEN_TABLE) for k in ("w", "b", "gamma", "beta")]


_GEN_PTRS = _FP * PG_GEN_MAX_TRUNKS          # a host array of per-trunk device pointers (noise, d_out)

# every symbol include/posegen_hip.h declares: (restype, argtypes)
PROTOTYPES = {
    "pg_abi_version": (C.c_int, []),
    "pg_create": (C.c_int, [C.POINTER(PgConfig), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "pg_destroy": (None, [C.c_void_p]),
    "pg_last_error": (C.c_char_p, [C.c_void_p]),
    "pg_load_weights": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int]),
    "pg_set_embedder": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_float]),
    "pg_set_framecodes": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "pg_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_set_far_skip": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_set_empty_skip": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_debug_wave_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pg_set_onchip": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_load_weights_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int]),
    "pg_set_train_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_render_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, C.c_int64, _FP, C.c_int64, _FP,
                                 C.c_int, C.c_int, C.c_int, C.POINTER(PgOutputs)]),
    "pg_calibrate_mfma": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pg_render_rays_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, C.c_int64, _FP, C.c_int64, _FP,
                                       C.c_int, C.c_int, C.c_int, C.POINTER(PgTrainDraws), C.POINTER(PgOutputs)]),
    "pg_stage_sample_coarse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, C.c_int64, C.c_int,
                                         C.c_int, _FP, _FP]),
    "pg_stage_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, _FP, _FP, _FP,
                                C.c_int64, _FP, _FP, _FP, C.c_int]),
    "pg_stage_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP,
                                     _FP, _FP, C.c_int, _FP]),
    "pg_stage_sample_coarse_draws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, C.c_int64, C.c_int,
                                               C.c_int, _FP, _FP, _FP]),
    "pg_stage_composite_form": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, _FP, _FP, _FP, _FP, _FP,
                                          _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, C.c_int, _FP, _FP]),
    "pg_stage_composite_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "pg_stage_merged_composite_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, _FP, _FP, _FP, _FP, _FP,
                                                _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "pg_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pg_profile_read_aux": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pg_debug_pack": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int32)]),
    "pg_render_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.POINTER(C.c_int), C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_float,
                                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "pg_pose_kinematics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_double),
                                     C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pg_query_density": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pg_debug_pack_map": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "pg_debug_widen_views": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "pg_debug_pack_vy": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_int64, C.POINTER(C.c_int64)]),
    "pg_device_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pg_query": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pg_device_count": (C.c_int, [C.c_void_p]),
    "pg_pose_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double,
                                C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p]),
    "pg_render_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                   C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pg_render_frame_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(C.c_int), C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pg_compose_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pg_stage_frame_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_int), C.c_float, C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_void_p,
                                      C.c_void_p]),
    "pg_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, C.c_int64, _FP, C.c_int64, _FP, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(PgTrainDraws), C.POINTER(PgNetParams), C.POINTER(PgNetParams), C.POINTER(PgOutputs),
                                   C.POINTER(C.c_int64)]),
    "pg_train_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, _FP, _FP, C.POINTER(PgNetGrads), C.POINTER(PgNetGrads)]),
    "pg_train_backward_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, _FP, _FP, C.POINTER(PgNetGrads),
                                         C.POINTER(PgNetGrads), _FP, C.c_int64]),
    "pg_poseopt_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, _FP, C.c_int64, C.POINTER(C.c_int32), C.c_int64,
                                     C.POINTER(C.c_int32), _FP, _FP, _FP, _FP]),
    "pg_poseopt_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, _FP, C.c_int64, C.POINTER(C.c_int32), C.c_int64,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), _FP, _FP, _FP, _FP, _FP, _FP]),
    "pg_set_subject_count": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_subject_count": (C.c_int, [C.c_void_p]),
    "pg_select_subject": (C.c_int, [C.c_void_p, C.c_int]),
    "pg_subject_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pg_render_frames_subjects": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                            C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pg_grid_density": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_float), C.c_void_p, C.c_int64,
                                  C.c_void_p]),
    "pg_mesh_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pg_mesh_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                               C.c_void_p, C.c_int64, C.c_int64]),
    "pg_pixel_index_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "pg_pixel_index_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "pg_batch_sample_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int64,
                                         C.POINTER(C.c_int32), C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "pg_batch_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgImageBank), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64,
                                  C.c_int, C.c_void_p, _FP, _FP, _FP, _FP, _FP, _FP]),
    "pg_regressor_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(PgCropItem), C.c_int32, C.c_int32,
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), _FP]),
    "pg_frame_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgImageBank), C.c_int32, C.POINTER(C.c_int32), _FP, C.c_int,
                                   C.c_void_p]),
    "pg_frame_metrics_val": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgImageBank), C.c_int32, C.POINTER(C.c_int32), _FP, C.c_int32,
                                       C.c_int32, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "pg_pose_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_double), C.c_int, C.c_void_p, _FP, _FP, C.c_void_p]),
    "pg_smpl_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgBodyModel), C.c_int64, _FP, C.c_int64, _FP, C.c_int, _FP, C.c_int,
                                  _FP, _FP, _FP]),
    "pg_smpl_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgBodyModel), C.c_int64, _FP, C.c_int64, _FP, C.c_int, _FP, C.c_int,
                                   _FP, _FP, _FP, _FP, _FP, _FP]),
    "pg_vertex_errors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, C.c_void_p, C.c_void_p]),
    "pg_pose_kinematics_rot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "pg_pose_kinematics_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), _FP,
                                         C.c_void_p]),
    "pg_pose_kinematics_rot_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, C.POINTER(C.c_double), C.POINTER(C.c_int32), _FP, _FP]),
    "pg_pose_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _FP, _FP, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                               C.c_double, C.c_double, C.c_void_p, C.c_void_p, _FP, _FP]),
    "pg_train_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, _FP, _FP, _FP, _FP, C.c_double, _FP, C.c_int, C.c_double, C.c_int,
                                C.c_double, C.c_int, C.c_double, C.c_void_p, _FP, _FP, _FP, _FP]),
    "pg_pose_reg_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _FP, _FP, C.c_int64, _FP, _FP, C.POINTER(C.c_int32), C.c_double,
                                   C.c_double, C.c_double, _FP, _FP, _FP, _FP, _FP, C.c_double, C.c_void_p, _FP, _FP]),
    "pg_grad_norms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]),
    "pg_plan_frames": (C.c_int, [C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                 C.POINTER(C.c_int)]),
    "pg_render_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                  C.c_float, C.c_int, C.POINTER(PgScenePerson), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "pg_stage_scene_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p, _FP, _FP, _FP, _FP, _FP]),
}

# every symbol include/posegen_gan.h declares (the second public header: PROTOTYPES stays the table of posegen_hip.h alone, which
# its tests compare with that header symbol for symbol); bound by load_library and called through `call` like the others
GAN_PROTOTYPES = {
    "pg_disc_tape_floats": (C.c_int, [C.POINTER(PgDiscSpec), C.c_int64, C.POINTER(C.c_int64)]),
    "pg_disc_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgDiscSpec), C.POINTER(PgDiscParams), _FP, C.c_int64, _FP, _FP]),
    "pg_disc_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgDiscSpec), C.POINTER(PgDiscParams), _FP, C.c_int64, _FP, _FP, _FP,
                                   C.POINTER(PgDiscParams)]),
    "pg_disc_loss": (C.c_int, [C.c_void_p, C.c_void_p, _FP, C.c_int64, C.c_float, C.c_double, C.c_void_p, _FP]),
    "pg_pool_exchange": (C.c_int, [C.c_void_p, C.c_void_p, _FP, C.c_int64, C.c_int32, C.c_int64, _FP, C.c_int64, C.c_void_p, C.c_void_p,
                                   _FP]),
}

# every symbol include/posegen_generator.h declares (the third public header), bound and called like the others
GENERATOR_PROTOTYPES = {
    "pg_gen_tape_size": (C.c_int, [C.POINTER(PgGenSpec), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pg_gen_trunk_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgGenSpec), C.POINTER(PgGenParams), C.POINTER(_FP), C.c_int64,
                                       C.c_int32, _FP, C.c_void_p]),
    "pg_gen_trunk_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgGenSpec), C.POINTER(PgGenParams), C.POINTER(_FP), C.c_int64,
                                        C.c_int32, _FP, C.c_void_p, C.POINTER(_FP), C.POINTER(PgGenGrads)]),
    "pg_gen_ba_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgGenSpec), C.c_int32, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP,
                                         _FP]),
    "pg_gen_ba_head_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgGenSpec), C.c_int32, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP,
                                          _FP, _FP, _FP]),
    "pg_gen_rt_head": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgGenSpec), C.c_int32, C.c_int32, _FP, C.c_int64, C.c_int32, _FP, _FP,
                                 _FP, _FP, _FP, _FP, _FP]),
}

PG_HMR_MAX_FEAT, PG_HMR_MAX_HIDDEN, PG_HMR_MAX_JOINTS, PG_HMR_MAX_SHAPE, PG_HMR_MAX_CAM, PG_HMR_MAX_ITER, PG_HMR_MAX_ROWS = 4096, 2048, 64, 64, 16, 8, 1048576
HMR_TENSORS = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "decpose_w", "decpose_b", "decshape_w", "decshape_b", "deccam_w", "deccam_b")


class PgHmrSpec(C.Structure):
    """pg_hmr_spec (include/posegen_regressor.h): the widths of the regression head, its rounds and nn.Dropout's p"""
    _fields_ = [(k, C.c_int32) for k in ("n_feat", "n_hidden", "n_joints", "n_shape", "n_cam", "n_iter")] + [("p_drop", C.c_float)]


class PgHmrParams(C.Structure):
    """pg_hmr_params: the device pointers of the five nn.Linears' tensors, where torch keeps them"""
    _fields_ = [(k, _FP) for k in HMR_TENSORS]


class PgHmrGrads(C.Structure):
    _fields_ = [(k, _FP) for k in HMR_TENSORS]


# every symbol include/posegen_regressor.h declares (the fourth public header), bound and called like the others
REGRESSOR_PROTOTYPES = {
    "pg_hmr_tape_size": (C.c_int, [C.POINTER(PgHmrSpec), C.c_int64, C.POINTER(C.c_int64)]),
    "pg_hmr_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgHmrSpec), C.POINTER(PgHmrParams), _FP, _FP, C.c_int32, C.c_void_p,
                                      C.c_int64, _FP, _FP, _FP, _FP]),
    "pg_hmr_head_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PgHmrSpec), C.POINTER(PgHmrParams), _FP, C.c_void_p, C.c_int64, _FP,
                                       _FP, _FP, _FP, C.POINTER(PgHmrGrads), _FP, _FP]),
}

PG_ADAM_MAX_TENSORS, PG_ADAM_MAX_GROUPS, PG_ADAM_SEGMENT, PG_ADAM_NO_CLIP = 4096, 64, 16384, -1.0


class PgAdamGroup(C.Structure):
    """pg_adam_group (include/posegen_optim.h): torch.optim.Adam's hyperparameters of one param_group"""
    _fields_ = [(k, C.c_double) for k in ("lr", "beta1", "beta2", "eps", "weight_decay")]


class PgAdamTensor(C.Structure):
    """pg_adam_tensor: one parameter's device pointers, its element count, its group and the step being taken"""
    _fields_ = [(k, C.c_void_p) for k in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("count", C.c_int64), ("group", C.c_int32), ("step", C.c_int32)]


# every symbol include/posegen_optim.h declares (the fifth public header), bound and called like the others
OPTIM_PROTOTYPES = {
    "pg_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PgAdamTensor), C.c_int, C.POINTER(PgAdamGroup), C.c_double, C.c_int,
                               C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load (once) and type the shared library; raises HipLibraryError if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("POSEGEN_HIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise HipLibraryError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C posegen_amd/csrc` (there is no CPU fallback for the render path)")
    try:
        lib = C.CDLL(p)
    except OSError as e:  # pragma: no cover - depends on the box
        raise HipLibraryError(f"cannot load {p}: {e}") from e
    for name, (res, args) in (list(PROTOTYPES.items()) + list(GAN_PROTOTYPES.items()) + list(GENERATOR_PROTOTYPES.items()) + list(REGRESSOR_PROTOTYPES.items())
                               + list(OPTIM_PROTOTYPES.items())):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{p} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.pg_abi_version() != PG_ABI_VERSION:
        raise HipLibraryError(f"{p}: ABI version {lib.pg_abi_version()} != {PG_ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def check(lib: C.CDLL, handle, rc: int):
    if rc != PG_OK:
        msg = lib.pg_last_error(handle)
        raise PgError(rc, msg.decode() if msg else "unknown error")


def ptr(t):
    """a tensor's device pointer as the c_void_p an entry point takes; None stays None (NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def call(renderer, name: str, *args):
    """The stream-taking entry point `name` on `renderer`'s handle and current stream: tensors among `args` go as their pointers,
    everything else as given; a negative return code raises (`renderer._check`).  No device guard is entered: the caller's covers
    its allocations as well."""
    fn = getattr(renderer.lib, name)
    return renderer._check(fn(renderer.handle, renderer._stream(), *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args]))


def device_of(renderer, who: str, what: str) -> torch.device:
    """The renderer's device, which must be a HIP one; `what` ends the refusal's "not on a HIP device" clause in the caller's words."""
    device = torch.device(getattr(renderer, "device", "cpu"))
    if device.type != "cuda":
        raise NotImplementedError(f"{who}: the renderer is on {device}, not on a HIP device{what} there is no CPU path")
    return device
