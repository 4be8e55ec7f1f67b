"""ctypes binding of libnnue_hip.so (C ABI: include/nnue_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every wrapper checks
device / dtype / contiguity / shapes on the host, then passes raw pointers.  There is no
fallback of any kind: if the library is missing or a tensor is not on the GPU the call raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libnnue_hip.so"
ABI_VERSION = 39

_c_int, _c_i64, _c_f, _c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class NnueBuckets(ctypes.Structure):
    """struct nnue_buckets of include/nnue_hip.h (read on the host by the *_bucketed entry points)."""
    _fields_ = [("K", ctypes.c_int32), ("bucket", _c_p), ("rows", _c_p), ("tile_bucket", _c_p), ("seg", _c_p),
                ("tiles", ctypes.c_int32)]


_c_bk = ctypes.POINTER(NnueBuckets)


class NnueClsRider(ctypes.Structure):
    """struct nnue_cls_rider of include/nnue_hip.h: the arguments of the classifier's small-gradient tile family when it rides
    in nnue_ftm_backward's launch (opaque; filled by nnue_classifier_train_rider)."""
    _fields_ = [("opaque", ctypes.c_ubyte * 256)]


_c_rider = ctypes.POINTER(NnueClsRider)

# name -> (restype, argtypes); mirrors include/nnue_hip.h one to one
SIGNATURES = {
    "nnue_hip_abi_version": (_c_int, []),
    "nnue_hip_last_error": (ctypes.c_char_p, []),
    "nnue_conv3x3_forward": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "nnue_conv3x3_backward_input": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_sparse_values": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_sparse_values_backward": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_binarize_features": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int,
                                        _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p]),
    "nnue_act_to_padded": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ste_conv_backward_scratch": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ste_conv_backward_chunks": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ste_conv_backward": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int,
                                        _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "nnue_ft_prepare": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p]),
    "nnue_ft_forward": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_ft_backward_weight": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ft_backward_values": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int,
                                         _c_p, _c_int, _c_p]),
    "nnue_ftb_supported": (_c_int, [_c_int]),
    "nnue_ftb_list_tiles": (_c_int, [_c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_ftb_scratch": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_binarize_bits": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_int, _c_p, _c_int,
                                    _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p]),
    "nnue_ftb_forward": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_ftb_backward_weight": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p,
                                          _c_p, _c_i64, _c_p]),
    "nnue_ftb_backward_values": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_ftm_supported": (_c_int, [_c_int, _c_int, _c_int]),
    "nnue_ftm_scratch": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_binarize": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_conv_binarize": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_conv_binarize_patches": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p,
                                                _c_p]),
    "nnue_ste_conv_backward_patches": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "nnue_ftm_forward": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_ftm_forward_grouping": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_int,
                                           _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_forward_l1_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_forward_l1": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ftm_forward_l1_planes_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_forward_planes_bytes": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_conv_binarize_planes": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_int, _c_int, _c_p, _c_i64,
                                               _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_forward_l1_planes": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ftm_backward_weight": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ftm_backward_values": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_ftm_backward_values_scratch": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_backward_values_ws": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_ftm_backward_cw_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_backward_sq_count": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_backward_ste_chunks": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_backward_ste_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_backward": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                                   _c_p, _c_p, _c_int, _c_p, _c_p, _c_rider, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int,
                                   _c_p, _c_i64, _c_p]),
    "nnue_ftm_value_planes_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_value_planes_bytes": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_conv_binarize_value_planes": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_int, _c_int, _c_p,
                                                     _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_backward_planes": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                                          _c_p, _c_p, _c_int, _c_p, _c_p, _c_rider, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int,
                                          _c_p, _c_i64, _c_p, _c_i64, _c_p]),
    "nnue_ftm_backward_bucketed": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                                            _c_p, _c_p, _c_int, _c_p, _c_p, _c_int, _c_p, _c_int, _c_rider, _c_p, _c_p, _c_p,
                                            _c_p, _c_int, _c_int, _c_int, _c_p, _c_i64, _c_p]),
    "nnue_classifier_train_rider": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                                             _c_p, _c_p, _c_p, _c_i64, _c_bk, _c_rider]),
    "nnue_classifier_train_dz1_grouped_offset": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_train_x_grouped_offset": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_scratch": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_forward": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f,
                                         _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                                         _c_p, _c_i64, _c_p]),
    "nnue_classifier_backward": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_f, _c_p, _c_p, _c_p,
                                          _c_int, _c_int, _c_int, _c_int, _c_int,
                                          _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_classifier_train_scratch": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_train_dz1_offset": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_train_fused_tail_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_train_step": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_f,
                                            _c_int, _c_int, _c_int, _c_int, _c_int,
                                            _c_p, _c_p, _c_p, _c_p, _c_p,
                                            _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "nnue_bucket_tile_count": (_c_int, [_c_int, _c_int]),
    "nnue_bucket_group": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_classifier_scratch_bucketed": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_train_scratch_bucketed": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_classifier_forward_bucketed": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f,
                                                  _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                                                  _c_p, _c_i64, _c_bk, _c_p]),
    "nnue_classifier_backward_bucketed": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_f, _c_p, _c_p, _c_p,
                                                   _c_int, _c_int, _c_int, _c_int, _c_int,
                                                   _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_bk, _c_p]),
    "nnue_classifier_train_step_bucketed": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_f,
                                                     _c_int, _c_int, _c_int, _c_int, _c_int,
                                                     _c_p, _c_p, _c_p, _c_p, _c_p,
                                                     _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_bk, _c_p]),
    "nnue_cross_entropy": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_f, _c_p, _c_p, _c_p, _c_p]),
    "nnue_cross_entropy_soft": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_f, _c_int, _c_int, _c_f, _c_p, _c_p, _c_p, _c_p]),
    "nnue_classifier_train_step_soft": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_f,
                                                 _c_int, _c_int, _c_int, _c_int, _c_int,
                                                 _c_p, _c_p, _c_p, _c_p, _c_p,
                                                 _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int,
                                                 _c_p, _c_p, _c_f, _c_p]),
    "nnue_classifier_train_step_soft_bucketed": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_f,
                                                          _c_int, _c_int, _c_int, _c_int, _c_int,
                                                          _c_p, _c_p, _c_p, _c_p, _c_p,
                                                          _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int,
                                                          _c_p, _c_p, _c_f, _c_bk, _c_p]),
    "nnue_cross_entropy_distill": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_f, _c_int, _c_int, _c_f, _c_p, _c_p, _c_p, _c_p, _c_f, _c_f, _c_p]),
    "nnue_classifier_train_step_distill": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_f,
                                                    _c_int, _c_int, _c_int, _c_int, _c_int,
                                                    _c_p, _c_p, _c_p, _c_p, _c_p,
                                                    _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int,
                                                    _c_p, _c_p, _c_f, _c_p, _c_f, _c_f, _c_p]),
    "nnue_classifier_train_step_distill_bucketed": (_c_int, [_c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_f,
                                                             _c_int, _c_int, _c_int, _c_int, _c_int,
                                                             _c_p, _c_p, _c_p, _c_p, _c_p,
                                                             _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int,
                                                             _c_p, _c_p, _c_f, _c_p, _c_f, _c_f, _c_bk, _c_p]),
    "nnue_mix_batch": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_f, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_confusion_accumulate": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_p, _c_p]),
    "nnue_load_batch": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_i64, _c_int, ctypes.c_uint64, ctypes.c_uint64,
                                 _c_p, _c_p, _c_p]),
    "nnue_load_batch_policy": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, ctypes.c_uint64,
                                        ctypes.c_uint64, _c_p, _c_p, _c_p, _c_p]),
    "nnue_load_batch_params_count": (_c_int, []),
    "nnue_engine_scratch": (_c_i64, [_c_p, _c_int]),
    "nnue_engine_evaluate_logits": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_engine_stream_state_bytes": (_c_i64, [_c_p, _c_int]),
    "nnue_engine_stream_step": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_engine_evaluate_logits_stacks": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64,
                                                    _c_p]),
    "nnue_engine_stream_step_stacks": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p,
                                                _c_p, _c_p, _c_i64, _c_p]),
    "nnue_engine_stream_update": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_i64, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p,
                                           _c_p, _c_p, _c_p, _c_p]),
    "nnue_engine_matrix_supported": (_c_int, [_c_p, _c_int, _c_int]),
    "nnue_engine_table_planes_bytes": (_c_i64, [_c_p, _c_int]),
    "nnue_engine_matrix_scratch": (_c_i64, [_c_p, _c_int, _c_int]),
    "nnue_engine_pack_table": (_c_int, [_c_p, _c_int, _c_p, _c_i64, _c_p, _c_p]),
    "nnue_engine_evaluate_logits_matrix": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                                                    _c_p, _c_p, _c_i64, _c_p]),
    "nnue_engine_evaluate_logits_u8": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_engine_evaluate_logits_matrix_u8": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p,
                                                       _c_p, _c_i64, _c_p]),
    "nnue_engine_stream_step_u8": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p,
                                            _c_i64, _c_p]),
    "nnue_engine_stream_step_u8_regions": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_i64,
                                                    _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_engine_quantize_model": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int,
                                            _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p]),
    "nnue_sgd_scratch": (_c_i64, [_c_i64]),
    "nnue_multi_optim_scratch": (_c_i64, [_c_p, _c_int]),
    "nnue_multi_sgd_step": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_p, _c_i64, _c_p, _c_p]),
    "nnue_multi_adam_step": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_p,
                                      _c_i64, _c_p, _c_p]),
    "nnue_adam_step": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                _c_p, _c_p, _c_i64, _c_p, _c_p]),
    "nnue_sgd_step": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f, _c_int,
                               _c_p, _c_p, _c_i64, _c_p, _c_int, _c_int, _c_p, _c_p, _c_p, _c_int, _c_i64, _c_i64, _c_p, _c_int, _c_p, _c_p]),
    "nnue_lr_schedule_step": (_c_int, [_c_p, _c_i64, _c_p, _c_p, _c_p]),
    "nnue_ftm_uses_bf16": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_sqnorm_partials": (_c_int, [_c_p, _c_i64, _c_p, _c_int, _c_p]),
    "nnue_dp_factor_chunk_bytes": (_c_i64, [_c_int, _c_int, _c_int, _c_i64]),
    "nnue_dp_factor_offset": (_c_i64, [_c_int, _c_int, _c_int, _c_int, _c_i64]),
    "nnue_dp_factor_pack": (_c_int, [_c_p, _c_p, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "nnue_dp_factor_unpack": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_gram_sq_count": (_c_i64, [_c_int, _c_int]),
    "nnue_ftm_gram_scratch": (_c_i64, [_c_int, _c_int, _c_int]),
    "nnue_ftm_gram_sqnorm": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ftm_gram_sqnorm_tail": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nnue_ftm_backward_tail_rows": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "nnue_ftm_backward_weight_update": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_f, _c_f, _c_f, _c_f,
                                                 _c_int, _c_p, _c_p]),
    "nnue_ftm_update_forward_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "nnue_ftm_backward_weight_update_forward": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_f, _c_f, _c_f, _c_f,
                                                         _c_int, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_adam_step_ext": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                    _c_p, _c_p, _c_i64, _c_p, _c_int, _c_i64, _c_i64, _c_p, _c_int, _c_p, _c_p]),
    "nnue_ftm_backward_weight_update_adam": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p,
                                                      _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_p, _c_p]),
    "nnue_ftm_backward_weight_update_forward_adam": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p,
                                                              _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_p,
                                                              _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    # the weight clip (include/nnue_hip.h, "weight clip"): the optimizer entry points with the clamp in their update launch
    "nnue_sgd_step_clip": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_int,
                                    _c_int, _c_p, _c_p, _c_p, _c_int, _c_i64, _c_i64, _c_p, _c_int, _c_p, _c_f, _c_p, _c_int, _c_p]),
    "nnue_adam_step_clip": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                     _c_p, _c_p, _c_i64, _c_p, _c_f, _c_p, _c_int, _c_p]),
    "nnue_adam_step_ext_clip": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                         _c_p, _c_p, _c_i64, _c_p, _c_int, _c_i64, _c_i64, _c_p, _c_int, _c_p, _c_f, _c_p, _c_int, _c_p]),
    "nnue_ftm_backward_weight_update_clip": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_f, _c_f, _c_f, _c_f,
                                                      _c_int, _c_f, _c_p, _c_p]),
    "nnue_ftm_backward_weight_update_forward_clip": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_f, _c_f, _c_f,
                                                              _c_f, _c_int, _c_f, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_ftm_backward_weight_update_adam_clip": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p,
                                                           _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_p, _c_p]),
    "nnue_ftm_backward_weight_update_forward_adam_clip": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p,
                                                                   _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_p,
                                                                   _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "nnue_multi_sgd_step_clip": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p, _c_p, _c_i64, _c_p,
                                          _c_p]),
    "nnue_multi_adam_step_clip": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_f, _c_p,
                                           _c_p, _c_i64, _c_p, _c_p]),
    # the weight average (include/nnue_hip.h, "weight average"): the stand-alone pass, and the _clip entry points with the average
    # (ema, ema_omd, ema_omd_dev -- the multi-tensor forms: ema[], ema_omd[]) in front of the stream
    "nnue_ema_update": (_c_int, [_c_p, _c_p, _c_i64, _c_f, _c_p, _c_p]),
}
# the optimizer updates that have a _clip and an _ema sibling with one bound and one average (the multi-tensor forms take lists)
_UPDATE_ENTRY_POINTS = ("nnue_sgd_step", "nnue_adam_step", "nnue_adam_step_ext", "nnue_ftm_backward_weight_update",
                        "nnue_ftm_backward_weight_update_forward", "nnue_ftm_backward_weight_update_adam",
                        "nnue_ftm_backward_weight_update_forward_adam")
_MULTI_UPDATE_ENTRY_POINTS = ("nnue_multi_sgd_step", "nnue_multi_adam_step")  # (timed under their own names: not in _TIMED_AS)
for _name in _UPDATE_ENTRY_POINTS:
    _res, _args = SIGNATURES[_name + "_clip"]
    SIGNATURES[_name + "_ema"] = (_res, _args[:-1] + [_c_p, _c_f, _c_p, _c_p])
for _name in _MULTI_UPDATE_ENTRY_POINTS:
    _res, _args = SIGNATURES[_name + "_clip"]
    SIGNATURES[_name + "_ema"] = (_res, _args[:-1] + [_c_p, _c_p, _c_p])

_lib: Optional[ctypes.CDLL] = None


class NnueHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Loads the library (once).  Raises loudly if it was not built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NnueHipError(
            f"{LIB_PATH} is missing: build it with `python nnue-vision_amd/csrc/build.py` "
            "(or __graft_entry__.build()).  There is no CPU or eager fallback.")
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    got = lib.nnue_hip_abi_version()
    if got != ABI_VERSION:
        raise NnueHipError(f"libnnue_hip.so ABI {got} != binding ABI {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


_recording: Optional[list] = None  # when a list: every C call is also appended as (name, fn, args-without-stream)


class record_calls:
    """Context manager: collects the raw C calls made by the wrappers so that a fixed kernel sequence
    can later be replayed with no Python between launches (``run_plan``) -- eagerly or under hipGraph
    capture.  The last argument of every launching entry point is the stream; it is re-read at replay."""

    def __enter__(self):
        global _recording
        self.prev, _recording = _recording, []
        self.calls = _recording
        return self.calls

    def __exit__(self, *exc):
        global _recording
        _recording = self.prev
        return False


_timing: Optional[dict] = None  # when a dict {entry point: list}: direct calls of those entry points are bracketed with events


class time_calls:
    """Context manager: like ``run_plan(..., timers)`` for calls made directly through the wrappers (the exchange-and-update
    tail of a data-parallel step is not a recorded plan): (start, end) events on the current stream around each named call."""

    def __init__(self, timers):
        self.timers = timers

    def __enter__(self):
        global _timing
        self.prev, _timing = _timing, self.timers
        return self.timers

    def __exit__(self, *exc):
        global _timing
        _timing = self.prev
        return False


# entry points timed under the name of the call they replace (a caller's timer keys name the plain forms)
_TIMED_AS = {**{_name + _suffix: _name for _suffix in ("_ema", "_clip") for _name in _UPDATE_ENTRY_POINTS},
             "nnue_ftm_conv_binarize_planes": "nnue_ftm_conv_binarize", "nnue_ftm_forward_l1_planes": "nnue_ftm_forward_l1",
             "nnue_ftm_conv_binarize_value_planes": "nnue_ftm_conv_binarize", "nnue_ftm_backward_planes": "nnue_ftm_backward",
             "nnue_classifier_train_step_soft": "nnue_classifier_train_step",
             "nnue_classifier_train_step_soft_bucketed": "nnue_classifier_train_step_bucketed",
             "nnue_classifier_train_step_distill": "nnue_classifier_train_step",
             "nnue_classifier_train_step_distill_bucketed": "nnue_classifier_train_step_bucketed"}


def _call(name: str, *args) -> None:
    lib = load()
    fn = getattr(lib, name)
    key = _TIMED_AS.get(name, name)
    if _timing is not None and key in _timing:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = fn(*args)
        t1.record()
        _timing[key].append((t0, t1))
    else:
        rc = fn(*args)
    if rc != 0:
        raise NnueHipError(f"{name} failed (code {rc}): {lib.nnue_hip_last_error().decode()}")
    if _recording is not None:
        _recording.append((name, fn, args[:-1]))


def run_plan(plan, stream_ptr: int, timers=None) -> None:
    """Replays recorded calls on `stream_ptr`.  timers: {entry-point name: list} -- a (start, end) pair of
    torch events is recorded around each matching call on the current stream and appended to the list."""
    for name, fn, args in plan:
        key = _TIMED_AS.get(name, name)
        if timers is not None and key in timers:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rc = fn(*args, stream_ptr)
            t1.record()
            timers[key].append((t0, t1))
        else:
            rc = fn(*args, stream_ptr)
        if rc != 0:
            raise NnueHipError(f"{name} failed (code {rc}): {load().nnue_hip_last_error().decode()}")


def retarget_plan(plan, pointers, structs=None):
    """`plan` with other buffers behind its calls: an integer argument that is a key of `pointers` ({address: address}) becomes
    the value; a ctypes pointer whose target's address is a key of `structs` ({address: ctypes pointer}) becomes the value;
    everything else passes through.  The plan itself is never modified, and comes back as it is when nothing was replaced."""
    if not pointers and not structs:
        return plan

    def sub(a):
        if isinstance(a, int):
            return pointers.get(a, a) if pointers else a
        if structs and isinstance(a, ctypes._Pointer) and a:
            return structs.get(ctypes.addressof(a.contents), a)
        return a
    out = [(name, fn, tuple(sub(a) for a in args)) for name, fn, args in plan]
    return plan if out == plan else out  # (ctypes pointers and functions compare by identity)


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _need(t: torch.Tensor, dtype, what: str, shape: Optional[Tuple[int, ...]] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise NnueHipError(f"{what}: tensor is on {t.device}; the NNUE hot path runs on the GPU only "
                           "(no CPU fallback in this build)")
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


# ---------------------------------------------------------------------------- the FeatureTransformer kernel families
# Three kernel families run the FeatureTransformer on the binary map.  Each keeps one batch's active features in its own class
# (FT_FAMILIES: "mfma" FeatureMatrix, "bits" FeatureBits, "list" ActList) and the three classes have the same members, thin
# calls of the module-level ftm_* / ftb_* / ft_* functions, so a consumer picks the class once (ft_path) and never asks again:
#   family, n (int32 [B]: active positions per sample), empty(batch, positions, num_rows, l1, device)
#   binarize(conv_out, thr, stages=3)   stage 1: what the forward and the value gradient read; stage 2: what only the weight
#       gradient reads, the bit family's transposed masks (the other two leave everything in stage 1: stages=2 launches nothing)
#   front(images, conv_w, thr, stride, conv_out, patches=None)   images -> conv_out and stage 1, in the family's own launches
#   forward(weight, bias, out=None, group=None)   group (a BucketPlan): the launch(es) also form the bucket grouping from n
#   backward_weight(d_out, d_weight=None, d_bias=None, want_weight=True, want_bias=True), backward_values(d_out, weight, dst=None)
def _gather_front(self, images, conv_w, thr, stride: int, conv_out, patches=None):
    """front() of the two gather families: the conv launch, then the first stage of their own binarise launch."""
    conv3x3_forward(images, conv_w, stride, out=conv_out)
    self.binarize(conv_out, thr, stages=1)


@dataclass
class ActList:
    """Active-feature list + transposed coefficients (layout: include/nnue_hip.h)."""
    rows: torch.Tensor   # int32 [B, cap]
    pos: torch.Tensor    # int32 [B, cap]
    coef: torch.Tensor   # float32 [B, cap]
    n: torch.Tensor      # int32 [B]
    coefT: torch.Tensor  # float32 [F, ldb]
    cap: int
    ldb: int
    family = "list"

    batch = property(lambda self: self.n.shape[0])
    num_rows = property(lambda self: self.coefT.shape[0])

    @staticmethod
    def empty(batch: int, positions: int, num_rows: int, l1, device=None) -> "ActList":
        # l1 is not used (the lists do not depend on the table's width); the form without it, empty(batch, cap, num_rows, device), works too
        cap, ldb, device = positions, round_up(batch, 64), l1 if device is None else device
        i32 = dict(dtype=torch.int32, device=device)
        return ActList(torch.empty((batch, cap), **i32), torch.empty((batch, cap), **i32),
                       torch.empty((batch, cap), dtype=torch.float32, device=device),
                       torch.empty((batch,), **i32),
                       torch.empty((num_rows, ldb), dtype=torch.float32, device=device), cap, ldb)

    def binarize(self, conv_out, thr, stages: int = 3) -> "ActList":
        return binarize_features(conv_out, thr, self.num_rows, act=self) if stages & 1 else self

    def forward(self, weight, bias, out=None, group=None):
        if group is not None:  # (the gather kernels have no workgroup to spare for it: a launch ahead of theirs)
            bucket_group(self.n, self.cap, group.K, plan=group)
        return ft_forward(weight, bias, self, out=out)

    def backward_weight(self, d_out, d_weight=None, d_bias=None, want_weight: bool = True, want_bias: bool = True):
        return ft_backward_weight(d_out, self, self.num_rows, d_weight, d_bias, want_weight, want_bias)

    def backward_values(self, d_out, weight, dst=None):
        return ft_backward_values(d_out, weight, self, self.cap, dst=dst)

    front = _gather_front


# ---------------------------------------------------------------------------- front end
def conv_out_hw(h: int, w: int, stride: int) -> Tuple[int, int]:
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def conv3x3_forward(images: torch.Tensor, weight: torch.Tensor, stride: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images: expected [B,3,H,W], got {tuple(images.shape)}")
    images = _need(images, torch.float32, "images")
    b, _, h, w = images.shape
    fps = weight.shape[0]
    weight = _need(weight, torch.float32, "conv weight", (fps, 3, 3, 3))
    gh, gw = conv_out_hw(h, w, stride)
    if out is None:
        out = torch.empty((b, fps, gh, gw), dtype=torch.float32, device=images.device)
    else:
        _need(out, torch.float32, "conv_out", (b, fps, gh, gw))
    _call("nnue_conv3x3_forward", images.data_ptr(), weight.data_ptr(), out.data_ptr(), b, h, w, fps, stride,
          _stream(images))
    return out


def conv3x3_backward_input(d_conv_out: torch.Tensor, weight: torch.Tensor, image_shape, stride: int) -> torch.Tensor:
    """d(images) of the 3x3 / pad 1 conv: [B,3,H,W] from d_conv_out [B,fps,Gh,Gw]."""
    b, _, h, w = image_shape
    fps = weight.shape[0]
    gh, gw = conv_out_hw(h, w, stride)
    d_conv_out = _need(d_conv_out, torch.float32, "d_conv_out", (b, fps, gh, gw))
    weight = _need(weight, torch.float32, "conv weight", (fps, 3, 3, 3))
    d_images = torch.empty((b, 3, h, w), dtype=torch.float32, device=d_conv_out.device)
    _call("nnue_conv3x3_backward_input", d_conv_out.data_ptr(), weight.data_ptr(), b, h, w, fps, int(stride), d_images.data_ptr(),
          _stream(d_conv_out))
    return d_images


def sparse_values(flat_map: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """val[b,i] = map[b, idx[b,i]] (0 where idx < 0); map float32 [B,P], idx int64 [B,M]."""
    flat_map = _need(flat_map, torch.float32, "feature map")
    idx = _need(idx, torch.int64, "feature indices")
    b, p = flat_map.shape
    val = torch.empty(idx.shape, dtype=torch.float32, device=flat_map.device)
    _call("nnue_sparse_values", flat_map.data_ptr(), idx.data_ptr(), b, p, idx.shape[1], val.data_ptr(), _stream(flat_map))
    return val


def sparse_values_backward(d_val: torch.Tensor, idx: torch.Tensor, positions: int) -> torch.Tensor:
    d_val = _need(d_val, torch.float32, "d_val")
    idx = _need(idx, torch.int64, "feature indices", tuple(d_val.shape))
    b, m = idx.shape
    d_map = torch.empty((b, positions), dtype=torch.float32, device=d_val.device)
    _call("nnue_sparse_values_backward", d_val.data_ptr(), idx.data_ptr(), b, positions, m, d_map.data_ptr(), _stream(d_val))
    return d_map


def binarize_features(conv_out: torch.Tensor, thr: torch.Tensor, num_rows: int,
                      act: Optional[ActList] = None) -> ActList:
    conv_out = _need(conv_out, torch.float32, "conv_out")
    if conv_out.dim() != 4:
        raise ValueError(f"conv_out: expected [B,fps,Gh,Gw], got {tuple(conv_out.shape)}")
    b, fps, gh, gw = conv_out.shape
    thr = _need(thr.reshape(-1), torch.float32, "threshold", (fps,))
    cap = fps * gh * gw
    if act is None:
        act = ActList.empty(b, cap, num_rows, 0, conv_out.device)
    elif act.cap != cap or act.batch != b or act.coefT.shape != (num_rows, act.ldb):
        raise ValueError("binarize_features: act list does not match the map")
    _call("nnue_binarize_features", conv_out.data_ptr(), thr.data_ptr(), b, fps, gh, gw, num_rows,
          act.rows.data_ptr(), act.pos.data_ptr(), act.coef.data_ptr(), act.n.data_ptr(),
          act.coefT.data_ptr(), act.ldb, _stream(conv_out))
    return act


def act_to_padded(act: ActList, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    b = act.batch
    idx = torch.empty((b, width), dtype=torch.int64, device=act.n.device)
    val = torch.empty((b, width), dtype=torch.float32, device=act.n.device)
    _call("nnue_act_to_padded", act.pos.data_ptr(), act.coef.data_ptr(), act.n.data_ptr(), act.cap, b, width,
          idx.data_ptr(), val.data_ptr(), _stream(act.n))
    return idx, val


def _ste_outputs(b: int, fps: int, gh: int, gw: int, dev, d_thr, d_weight, scratch):
    """The two results and the scratch of the STE backward's two forms, allocated where the caller gave none."""
    if d_thr is None:
        d_thr = torch.empty((fps,), dtype=torch.float32, device=dev)
    if d_weight is None:
        d_weight = torch.empty((fps, 3, 3, 3), dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = torch.empty((load().nnue_ste_conv_backward_scratch(b, fps, gh, gw),), dtype=torch.uint8, device=dev)
    return d_thr, d_weight, scratch


def ste_conv_backward(images, conv_out, thr, d_conv_out, stride: int,
                      d_thr: Optional[torch.Tensor] = None, d_weight: Optional[torch.Tensor] = None,
                      scratch: Optional[torch.Tensor] = None, stages: int = 3):
    """stages=1 leaves the per-workgroup partials at the start of `scratch` (finish with stages=2 or hand them to
    sgd_step(ste=...), whose norm launch then carries the second stage)."""
    images = _need(images, torch.float32, "images")
    b, _, h, w = images.shape
    fps = conv_out.shape[1]
    gh, gw = conv_out_hw(h, w, stride)
    conv_out = _need(conv_out, torch.float32, "conv_out", (b, fps, gh, gw))
    d_conv_out = _need(d_conv_out, torch.float32, "d_conv_out").view(b, fps, gh, gw)
    thr = _need(thr.reshape(-1), torch.float32, "threshold", (fps,))
    d_thr, d_weight, scratch = _ste_outputs(b, fps, gh, gw, images.device, d_thr, d_weight, scratch)
    _call("nnue_ste_conv_backward", images.data_ptr(), conv_out.data_ptr(), thr.data_ptr(), d_conv_out.data_ptr(),
          b, h, w, fps, stride, d_thr.data_ptr(), d_weight.data_ptr(), scratch.data_ptr(), scratch.numel(), int(stages),
          _stream(images))
    return d_thr, d_weight


def ste_conv_backward_patches(patches, conv_out, thr, d_conv_out, gh: int, gw: int,
                              d_thr: Optional[torch.Tensor] = None, d_weight: Optional[torch.Tensor] = None,
                              scratch: Optional[torch.Tensor] = None, stages: int = 3):
    """ste_conv_backward from the im2col form ftm_conv_binarize(patches=...) left in place of the images; bitwise the same
    d_thr / d_weight / partials."""
    b, fps = conv_out.shape[:2]
    conv_out = _need(conv_out, torch.float32, "conv_out", (b, fps, gh, gw))
    patches = _need(patches, torch.float32, "patches", (27, b * gh * gw))
    d_conv_out = _need(d_conv_out, torch.float32, "d_conv_out").view(b, fps, gh, gw)
    thr = _need(thr.reshape(-1), torch.float32, "threshold", (fps,))
    d_thr, d_weight, scratch = _ste_outputs(b, fps, gh, gw, patches.device, d_thr, d_weight, scratch)
    _call("nnue_ste_conv_backward_patches", patches.data_ptr(), conv_out.data_ptr(), thr.data_ptr(), d_conv_out.data_ptr(), b, fps, gh, gw,
          d_thr.data_ptr(), d_weight.data_ptr(), scratch.data_ptr(), scratch.numel(), int(stages), _stream(patches))
    return d_thr, d_weight


def ste_conv_backward_chunks(b: int, fps: int, gh: int, gw: int) -> int:
    """Partials per output a stages=1 call leaves in its scratch."""
    return int(load().nnue_ste_conv_backward_chunks(b, fps, gh, gw))


# ---------------------------------------------------------------------------- FeatureTransformer
def ft_prepare(idx: torch.Tensor, val: torch.Tensor, num_rows: int) -> ActList:
    if idx.dim() != 2 or idx.shape != val.shape:
        raise ValueError(f"feature_indices / feature_values: expected matching [B,M], got "
                         f"{tuple(idx.shape)} and {tuple(val.shape)}")
    idx = _need(idx, torch.int64, "feature_indices")
    val = _need(val, torch.float32, "feature_values")
    b, m = idx.shape
    act = ActList.empty(b, m, num_rows, 0, idx.device)
    _call("nnue_ft_prepare", idx.data_ptr(), val.data_ptr(), b, m, num_rows, act.rows.data_ptr(), act.pos.data_ptr(),
          act.coef.data_ptr(), act.n.data_ptr(), act.coefT.data_ptr(), act.ldb, _stream(idx))
    return act


def ft_forward(weight: torch.Tensor, bias: torch.Tensor, act: ActList,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    weight = _need(weight, torch.float32, "input.weight")
    f, l1 = weight.shape
    bias = _need(bias, torch.float32, "input.bias", (l1,))
    if act.coefT.shape[0] != f:
        raise ValueError("ft_forward: act list was built for a different table")
    if out is None:
        out = torch.empty((act.batch, l1), dtype=torch.float32, device=weight.device)
    _call("nnue_ft_forward", weight.data_ptr(), bias.data_ptr(), act.rows.data_ptr(), act.coef.data_ptr(),
          act.n.data_ptr(), act.cap, act.batch, f, l1, out.data_ptr(), _stream(weight))
    return out


def ft_backward_weight(d_out: torch.Tensor, act: ActList, num_rows: int,
                       d_weight: Optional[torch.Tensor] = None, d_bias: Optional[torch.Tensor] = None,
                       want_weight: bool = True, want_bias: bool = True):
    d_out = _need(d_out, torch.float32, "d_out")
    b, l1 = d_out.shape
    if b != act.batch or act.coefT.shape[0] != num_rows:
        raise ValueError("ft_backward_weight: act list does not match d_out / table")
    if want_weight and d_weight is None:
        d_weight = torch.empty((num_rows, l1), dtype=torch.float32, device=d_out.device)
    if want_bias and d_bias is None:
        d_bias = torch.empty((l1,), dtype=torch.float32, device=d_out.device)
    _call("nnue_ft_backward_weight", d_out.data_ptr(), act.coefT.data_ptr(), act.ldb, b, num_rows, l1,
          _ptr(d_weight if want_weight else None), _ptr(d_bias if want_bias else None), _stream(d_out))
    return d_weight, d_bias


def ft_backward_values(d_out: torch.Tensor, weight: torch.Tensor, act: ActList, dst_ld: int,
                       dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    d_out = _need(d_out, torch.float32, "d_out")
    weight = _need(weight, torch.float32, "input.weight")
    b, l1 = d_out.shape
    f = weight.shape[0]
    if weight.shape[1] != l1 or b != act.batch:
        raise ValueError("ft_backward_values: shape mismatch")
    if dst is None:
        dst = torch.empty((b, dst_ld), dtype=torch.float32, device=d_out.device)
    elif dst.numel() != b * dst_ld:
        raise ValueError("ft_backward_values: dst has the wrong size")
    _call("nnue_ft_backward_values", d_out.data_ptr(), weight.data_ptr(), act.rows.data_ptr(), act.pos.data_ptr(),
          act.n.data_ptr(), act.cap, b, f, l1, dst.data_ptr(), dst_ld, _stream(d_out))
    return dst


# ---------------------------------------------------------------------------- FeatureTransformer, binary features
@dataclass
class FeatureBits:
    """Bit-mask + tile-list form of the active features of one batch (layout: include/nnue_hip.h)."""
    maskW: torch.Tensor  # int64 [B, pw64]           position bits per sample
    maskT: torch.Tensor  # int64 [F+1, bw64]         sample bits per table row (+ bias row)
    sink: torch.Tensor   # float32 [B]               active ids >= F-1
    n: torch.Tensor      # int32 [B]                 active positions
    tlW: torch.Tensor    # int16 [B, tiles_fwd, 128] LDS offsets of the rows to add per sample and table tile
    tcW: torch.Tensor    # uint8 [B, tiles_fwd]
    tlT: torch.Tensor    # int16 [F+1, tiles_bwd, 128] LDS offsets of the samples to add per output row and batch tile
    tcT: torch.Tensor    # uint8 [F+1, tiles_bwd]
    scratch: torch.Tensor  # uint8, split-slab workspace of the gather kernels
    positions: int       # P = fps*Gh*Gw
    num_rows: int        # F
    family = "bits"

    @property
    def batch(self) -> int:
        return self.n.shape[0]

    def binarize(self, conv_out, thr, stages: int = 3) -> "FeatureBits":
        return binarize_bits(conv_out, thr, self.num_rows, 0, bits=self, stages=stages)  # (l1 only sizes a new object's scratch)

    def forward(self, weight, bias, out=None, group=None):
        if group is not None:  # (as ActList.forward)
            bucket_group(self.n, self.positions, group.K, plan=group)
        return ftb_forward(weight, bias, self, out=out)

    def backward_weight(self, d_out, d_weight=None, d_bias=None, want_weight: bool = True, want_bias: bool = True):
        return ftb_backward_weight(d_out, self, d_weight, d_bias, want_weight, want_bias)

    def backward_values(self, d_out, weight, dst=None):
        return ftb_backward_values(d_out, weight, self, dst=dst)

    front = _gather_front

    @staticmethod
    def empty(batch: int, positions: int, num_rows: int, l1: int, device) -> "FeatureBits":
        pw64, bw64 = round_up(round_up(positions, 64) // 64, 2), round_up(round_up(batch, 64) // 64, 2)
        tf, tb = ctypes.c_int(), ctypes.c_int()
        if load().nnue_ftb_list_tiles(batch, num_rows, positions, ctypes.byref(tf), ctypes.byref(tb)) != 0:
            raise ValueError("FeatureBits: sizes must be positive")
        u8 = dict(dtype=torch.uint8, device=device)
        return FeatureBits(torch.empty((batch, pw64), dtype=torch.int64, device=device),
                           torch.empty((num_rows + 1, bw64), dtype=torch.int64, device=device),
                           torch.empty((batch,), dtype=torch.float32, device=device),
                           torch.empty((batch,), dtype=torch.int32, device=device),
                           torch.empty((batch, tf.value, 128), dtype=torch.int16, device=device), torch.empty((batch, tf.value), **u8),
                           torch.empty((num_rows + 1, tb.value, 128), dtype=torch.int16, device=device), torch.empty((num_rows + 1, tb.value), **u8),
                           torch.empty((max(16, int(load().nnue_ftb_scratch(batch, num_rows, positions, l1))),), **u8),
                           positions, num_rows)


def ftb_supported(l1: int) -> bool:
    return bool(load().nnue_ftb_supported(int(l1)))


def ft_path(num_rows: int, positions: int, l1: int, batch: int = 1, mode: Optional[str] = None) -> str:
    """Which FeatureTransformer kernels the fused path uses for the binary map: "mfma" | "bits" | "list" (a key of FT_FAMILIES).

    "mfma" = dense f32-MFMA products over the float {0,1} map (fastest at the reference's ~43 % density and still
    ahead at 1 %); "bits" = tile-list kernels that stage table tiles in LDS once per sample tile; "list" = id-list
    gather kernels (any shape).  mode = "mfma" | "bits" | "list" forces one where the shape allows it; "auto" takes the first of
    mfma, bits, list that supports the shape.  mode=None reads NNUE_FT_PATH (default "auto"): a given mode wins over it."""
    if mode is None:
        mode = os.environ.get("NNUE_FT_PATH", "auto")
    # the product kernels address every operand with 32-bit byte offsets (batch-sized ones included)
    fits = (batch + 256) * positions * 4 < 2 ** 31 and (batch + 256) * l1 * 4 < 2 ** 31
    can_mfma, can_bits = fits and ftm_supported(num_rows, positions, l1), ftb_supported(l1)
    if mode == "list":
        return "list"
    if mode == "bits":
        return "bits" if can_bits else "list"
    if can_mfma:
        return "mfma"
    return "bits" if can_bits else "list"


def binarize_bits(conv_out: torch.Tensor, thr: torch.Tensor, num_rows: int, l1: int,
                  bits: Optional[FeatureBits] = None, stages: int = 3) -> FeatureBits:
    conv_out = _need(conv_out, torch.float32, "conv_out")
    if conv_out.dim() != 4:
        raise ValueError(f"conv_out: expected [B,fps,Gh,Gw], got {tuple(conv_out.shape)}")
    b, fps, gh, gw = conv_out.shape
    thr = _need(thr.reshape(-1), torch.float32, "threshold", (fps,))
    if bits is None:
        bits = FeatureBits.empty(b, fps * gh * gw, num_rows, l1, conv_out.device)
    elif bits.batch != b or bits.positions != fps * gh * gw or bits.num_rows != num_rows:
        raise ValueError("binarize_bits: bit buffers do not match the map")
    _call("nnue_binarize_bits", conv_out.data_ptr(), thr.data_ptr(), b, fps, gh, gw, num_rows, bits.maskW.data_ptr(),
          bits.maskW.shape[1], bits.maskT.data_ptr(), bits.maskT.shape[1], bits.sink.data_ptr(), bits.n.data_ptr(),
          bits.tlW.data_ptr(), bits.tcW.data_ptr(), bits.tlT.data_ptr(), bits.tcT.data_ptr(), int(stages), _stream(conv_out))
    return bits


def ftb_forward(weight: torch.Tensor, bias: torch.Tensor, bits: FeatureBits, out: Optional[torch.Tensor] = None):
    weight = _need(weight, torch.float32, "input.weight")
    f, l1 = weight.shape
    bias = _need(bias, torch.float32, "input.bias", (l1,))
    if f != bits.num_rows:
        raise ValueError("ftb_forward: bits were built for a different table")
    if out is None:
        out = torch.empty((bits.batch, l1), dtype=torch.float32, device=weight.device)
    _call("nnue_ftb_forward", weight.data_ptr(), bias.data_ptr(), bits.tlW.data_ptr(), bits.tcW.data_ptr(),
          bits.sink.data_ptr(), bits.batch, f, bits.positions, l1, out.data_ptr(), bits.scratch.data_ptr(),
          bits.scratch.numel(), _stream(weight))
    return out


def ftb_backward_weight(d_out: torch.Tensor, bits: FeatureBits, d_weight: Optional[torch.Tensor] = None,
                        d_bias: Optional[torch.Tensor] = None, want_weight: bool = True, want_bias: bool = True):
    d_out = _need(d_out, torch.float32, "d_out")
    b, l1 = d_out.shape
    if b != bits.batch:
        raise ValueError("ftb_backward_weight: bits do not match d_out")
    if want_weight and d_weight is None:
        d_weight = torch.empty((bits.num_rows, l1), dtype=torch.float32, device=d_out.device)
    if want_bias and d_bias is None:
        d_bias = torch.empty((l1,), dtype=torch.float32, device=d_out.device)
    _call("nnue_ftb_backward_weight", d_out.data_ptr(), bits.tlT.data_ptr(), bits.tcT.data_ptr(), bits.sink.data_ptr(),
          b, bits.num_rows, bits.positions, l1, _ptr(d_weight if want_weight else None),
          _ptr(d_bias if want_bias else None), bits.scratch.data_ptr(), bits.scratch.numel(), _stream(d_out))
    return d_weight, d_bias


def ftb_backward_values(d_out: torch.Tensor, weight: torch.Tensor, bits: FeatureBits,
                        dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    d_out = _need(d_out, torch.float32, "d_out")
    weight = _need(weight, torch.float32, "input.weight")
    b, l1 = d_out.shape
    if weight.shape != (bits.num_rows, l1) or b != bits.batch:
        raise ValueError("ftb_backward_values: shape mismatch")
    if dst is None:
        dst = torch.empty((b, bits.positions), dtype=torch.float32, device=d_out.device)
    elif dst.numel() != b * bits.positions:
        raise ValueError("ftb_backward_values: dst has the wrong size")
    _call("nnue_ftb_backward_values", d_out.data_ptr(), weight.data_ptr(), bits.maskW.data_ptr(), bits.maskW.shape[1],
          b, bits.num_rows, bits.positions, l1, dst.data_ptr(), _stream(d_out))
    return dst


# ---------------------------------------------------------------------------- FeatureTransformer, dense MFMA form
def ftm_supported(num_rows: int, positions: int, l1: int) -> bool:
    return bool(load().nnue_ftm_supported(int(num_rows), int(positions), int(l1)))


def ftm_scratch_bytes(b: int, num_rows: int, positions: int, l1: int) -> int:
    return int(load().nnue_ftm_scratch(int(b), int(num_rows), int(positions), int(l1)))


class FeatureMatrix:
    """The binary map of one batch as a byte {0,1} matrix (layout: include/nnue_hip.h, nnue_ftm_*)."""
    bits: torch.Tensor     # uint8 [B, P]
    n: torch.Tensor        # int32 [B]    active positions
    sink: torch.Tensor     # float32 [B]  active positions >= F-1
    scratch: torch.Tensor  # uint8, split-K slabs of the forward
    positions: int
    num_rows: int
    family = "mfma"

    def __init__(self, bits, n, sink, scratch, positions, num_rows):
        self.bits, self.n, self.sink, self.scratch, self.positions, self.num_rows = bits, n, sink, scratch, positions, num_rows

    @property
    def batch(self) -> int:
        return self.n.shape[0]

    @staticmethod
    def empty(batch: int, positions: int, num_rows: int, l1: int, device) -> "FeatureMatrix":
        return FeatureMatrix(torch.empty((batch, positions), dtype=torch.uint8, device=device),
                             torch.empty((batch,), dtype=torch.int32, device=device),
                             torch.empty((batch,), dtype=torch.float32, device=device),
                             torch.empty((max(16, ftm_scratch_bytes(batch, num_rows, positions, l1)),), dtype=torch.uint8, device=device),
                             positions, num_rows)

    def binarize(self, conv_out, thr, stages: int = 3) -> "FeatureMatrix":  # (l1 = 0 here and in front: it only sizes a new object's scratch)
        return ftm_binarize(conv_out, thr, self.num_rows, 0, fm=self) if stages & 1 else self

    def front(self, images, conv_w, thr, stride: int, conv_out, patches=None):
        """conv + map + counts in ONE launch; patches: it also leaves the images' im2col form."""
        ftm_conv_binarize(images, conv_w, thr, stride, self.num_rows, 0, conv_out=conv_out, fm=self, patches=patches)

    def forward(self, weight, bias, out=None, group=None):
        return ftm_forward(weight, bias, self, out=out, group=group)  # (the grouping rides in the launch)

    def backward_weight(self, d_out, d_weight=None, d_bias=None, want_weight: bool = True, want_bias: bool = True):
        return ftm_backward_weight(d_out, self, d_weight, d_bias, want_weight, want_bias)

    def backward_values(self, d_out, weight, dst=None):
        return ftm_backward_values(d_out, weight, self, dst=dst)


FT_FAMILIES = {"mfma": FeatureMatrix, "bits": FeatureBits, "list": ActList}  # ft_path's answer -> the family's class


def ftm_binarize(conv_out: torch.Tensor, thr: torch.Tensor, num_rows: int, l1: int,
                 fm: Optional[FeatureMatrix] = None) -> FeatureMatrix:
    conv_out = _need(conv_out, torch.float32, "conv_out")
    if conv_out.dim() != 4:
        raise ValueError(f"conv_out: expected [B,fps,Gh,Gw], got {tuple(conv_out.shape)}")
    b, fps, gh, gw = conv_out.shape
    thr = _need(thr.reshape(-1), torch.float32, "threshold", (fps,))
    if fm is None:
        fm = FeatureMatrix.empty(b, fps * gh * gw, num_rows, l1, conv_out.device)
    elif fm.batch != b or fm.positions != fps * gh * gw or fm.num_rows != num_rows:
        raise ValueError("ftm_binarize: buffers do not match the map")
    _call("nnue_ftm_binarize", conv_out.data_ptr(), thr.data_ptr(), b, fps, gh, gw, int(num_rows), fm.bits.data_ptr(),
          fm.n.data_ptr(), fm.sink.data_ptr(), _stream(conv_out))
    return fm


def _conv_front(who: str, images, weight, thr, stride: int, num_rows: int, l1: int, conv_out, fm):
    """What the one-launch conv + map forms share: images, conv weight and thresholds checked, conv_out and the map checked or
    allocated.  Returns (images, weight, thr, (b, h, w, fps, gh, gw), conv_out, fm)."""
    images = _need(images, torch.float32, "images")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images: expected [B,3,H,W], got {tuple(images.shape)}")
    b, _, h, w = images.shape
    weight = _need(weight, torch.float32, "conv.weight")
    fps = weight.shape[0]
    if tuple(weight.shape) != (fps, 3, 3, 3):
        raise ValueError("conv.weight: expected [fps,3,3,3]")
    thr = _need(thr.reshape(-1), torch.float32, "threshold", (fps,))
    gh, gw = conv_out_hw(h, w, stride)
    if conv_out is None:
        conv_out = torch.empty((b, fps, gh, gw), dtype=torch.float32, device=images.device)
    elif tuple(conv_out.shape) != (b, fps, gh, gw):
        raise ValueError(f"{who}: conv_out has the wrong shape")
    if fm is None:
        fm = FeatureMatrix.empty(b, fps * gh * gw, num_rows, l1, images.device)
    elif fm.batch != b or fm.positions != fps * gh * gw or fm.num_rows != num_rows:
        raise ValueError(f"{who}: buffers do not match the map")
    return images, weight, thr, (b, h, w, fps, gh, gw), conv_out, fm


def ftm_conv_binarize(images: torch.Tensor, weight: torch.Tensor, thr: torch.Tensor, stride: int, num_rows: int, l1: int,
                      conv_out: Optional[torch.Tensor] = None, fm: Optional[FeatureMatrix] = None,
                      patches: Optional[torch.Tensor] = None):
    """conv3x3_forward + ftm_binarize in one launch; returns (conv_out, fm), bitwise the two separate calls.
    patches (float32 [27, B*Gh*Gw]): the launch also leaves the im2col form of the images (ste_conv_backward_patches reads
    it)."""
    images, weight, thr, (b, h, w, fps, gh, gw), conv_out, fm = _conv_front("ftm_conv_binarize", images, weight, thr, stride, num_rows, l1,
                                                                            conv_out, fm)
    if patches is not None:
        patches = _need(patches, torch.float32, "patches", (27, b * gh * gw))
        _call("nnue_ftm_conv_binarize_patches", images.data_ptr(), weight.data_ptr(), thr.data_ptr(), b, h, w, fps, int(stride), int(num_rows),
              patches.data_ptr(), conv_out.data_ptr(), fm.bits.data_ptr(), fm.n.data_ptr(), fm.sink.data_ptr(), _stream(images))
        return conv_out, fm
    _call("nnue_ftm_conv_binarize", images.data_ptr(), weight.data_ptr(), thr.data_ptr(), b, h, w, fps, int(stride), int(num_rows),
          conv_out.data_ptr(), fm.bits.data_ptr(), fm.n.data_ptr(), fm.sink.data_ptr(), _stream(images))
    return conv_out, fm


def ftm_forward(weight: torch.Tensor, bias: torch.Tensor, fm: FeatureMatrix, out: Optional[torch.Tensor] = None,
                group=None) -> torch.Tensor:
    """group (a BucketPlan): the bucket grouping of this batch (from fm.n) rides in the launch as one extra workgroup."""
    weight = _need(weight, torch.float32, "input.weight")
    f, l1 = weight.shape
    bias = _need(bias, torch.float32, "input.bias", (l1,))
    if f != fm.num_rows:
        raise ValueError("ftm_forward: the map was built for a different table")
    if out is None:
        out = torch.empty((fm.batch, l1), dtype=torch.float32, device=weight.device)
    args = (fm.bits.data_ptr(), fm.sink.data_ptr(), weight.data_ptr(), bias.data_ptr(), fm.batch, f,
            fm.positions, l1, out.data_ptr(), fm.scratch.data_ptr(), fm.scratch.numel())
    if group is None:
        _call("nnue_ftm_forward", *args, _stream(weight))
    else:
        if group.batch != fm.batch:
            raise ValueError("ftm_forward: the bucket plan was built for another batch size")
        _call("nnue_ftm_forward_grouping", *args, fm.n.data_ptr(), group.K, group.bucket.data_ptr(), group.rows.data_ptr(),
              group.tile_bucket.data_ptr(), group.seg.data_ptr(), _stream(weight))
    return out


def ftm_forward_l1_supported(batch: int, num_rows: int, positions: int, l1: int, l2: int) -> bool:
    return bool(load().nnue_ftm_forward_l1_supported(int(batch), int(num_rows), int(positions), int(l1), int(l2)))


def _forward_l1_operands(who: str, weight, bias, fm: FeatureMatrix, w1, part, out):
    """What the two fused-forward forms share: table, bias, w1 and the slab buffer checked, the output allocated where none is
    given.  Returns (weight, bias, w1, (f, l1, l2), out)."""
    weight = _need(weight, torch.float32, "input.weight")
    f, l1 = weight.shape
    bias = _need(bias, torch.float32, "input.bias", (l1,))
    l2 = w1.shape[0]
    w1 = _need(w1, torch.float32, "classifier.0.weight", (l2, l1))
    if f != fm.num_rows:
        raise ValueError(f"{who}: the map was built for a different table")
    if not part.is_cuda or part.numel() * part.element_size() < (l1 // 64) * fm.batch * l2 * 4:
        raise ValueError(f"{who}: part buffer too small for [L1/64][B][L2] floats")
    if out is None:
        out = torch.empty((fm.batch, l1), dtype=torch.float32, device=weight.device)
    return weight, bias, w1, (f, l1, l2), out


def ftm_forward_l1(weight: torch.Tensor, bias: torch.Tensor, fm: FeatureMatrix, w1: torch.Tensor, part: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ftm_forward + the classifier's layer-1 slabs part[L1/64][B][L2] (written at the start of `part`, the
    classifier's scratch buffer; consumed by classifier_train_step(phases | 8))."""
    weight, bias, w1, (f, l1, l2), out = _forward_l1_operands("ftm_forward_l1", weight, bias, fm, w1, part, out)
    _call("nnue_ftm_forward_l1", fm.bits.data_ptr(), fm.sink.data_ptr(), weight.data_ptr(), bias.data_ptr(), w1.data_ptr(),
          fm.batch, f, fm.positions, l1, l2, out.data_ptr(), part.data_ptr(), _stream(weight))
    return out


def ftm_forward_l1_planes_supported(batch: int, num_rows: int, positions: int, l1: int, l2: int) -> bool:
    return bool(load().nnue_ftm_forward_l1_planes_supported(int(batch), int(num_rows), int(positions), int(l1), int(l2)))


def ftm_forward_planes_bytes(batch: int, num_rows: int, positions: int, l1: int) -> int:
    return int(load().nnue_ftm_forward_planes_bytes(int(batch), int(num_rows), int(positions), int(l1)))


def ftm_conv_binarize_planes(images: torch.Tensor, weight: torch.Tensor, thr: torch.Tensor, stride: int, table: torch.Tensor, l2: int,
                             planes: torch.Tensor, conv_out: Optional[torch.Tensor] = None, fm: Optional[FeatureMatrix] = None,
                             val_planes: Optional[torch.Tensor] = None):
    """ftm_conv_binarize whose launch also leaves `table` (input.weight) as the bf16 planes ftm_forward_l1_planes reads
    (`planes`: a uint8 buffer of ftm_forward_planes_bytes); returns (conv_out, fm), bitwise ftm_conv_binarize's.
    val_planes (a uint8 buffer of ftm_value_planes_bytes; shapes: ftm_value_planes_supported): the launch also leaves the planes
    ftm_backward(val_planes=...) reads."""
    table = _need(table, torch.float32, "input.weight")
    f, l1 = table.shape
    if planes is not None or val_planes is None:  # (planes=None with val_planes: the value planes alone)
        planes = _need(planes, torch.uint8, "planes")
    images, weight, thr, (b, h, w, fps, gh, gw), conv_out, fm = _conv_front("ftm_conv_binarize_planes", images, weight, thr, stride, f, l1,
                                                                            conv_out, fm)
    if val_planes is not None:
        val_planes = _need(val_planes, torch.uint8, "val_planes")
        _call("nnue_ftm_conv_binarize_value_planes", images.data_ptr(), weight.data_ptr(), thr.data_ptr(), b, h, w, fps, int(stride), f,
              table.data_ptr(), l1, int(l2), _ptr(planes), planes.numel() if planes is not None else 0, val_planes.data_ptr(), val_planes.numel(),
              conv_out.data_ptr(), fm.bits.data_ptr(), fm.n.data_ptr(), fm.sink.data_ptr(), _stream(images))
        return conv_out, fm
    _call("nnue_ftm_conv_binarize_planes", images.data_ptr(), weight.data_ptr(), thr.data_ptr(), b, h, w, fps, int(stride), f,
          table.data_ptr(), l1, int(l2), planes.data_ptr(), planes.numel(), conv_out.data_ptr(), fm.bits.data_ptr(), fm.n.data_ptr(),
          fm.sink.data_ptr(), _stream(images))
    return conv_out, fm


def ftm_forward_l1_planes(weight: torch.Tensor, bias: torch.Tensor, fm: FeatureMatrix, planes: torch.Tensor, w1: torch.Tensor,
                          part: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ftm_forward_l1 reading the planes ftm_conv_binarize_planes wrote from `weight` (bitwise its 32-row bf16 form)."""
    planes = _need(planes, torch.uint8, "planes")
    weight, bias, w1, (f, l1, l2), out = _forward_l1_operands("ftm_forward_l1_planes", weight, bias, fm, w1, part, out)
    _call("nnue_ftm_forward_l1_planes", fm.bits.data_ptr(), fm.sink.data_ptr(), planes.data_ptr(), planes.numel(), weight.data_ptr(),
          bias.data_ptr(), w1.data_ptr(), fm.batch, f, fm.positions, l1, l2, out.data_ptr(), part.data_ptr(), _stream(weight))
    return out


def ftm_backward_weight(d_out: torch.Tensor, fm: FeatureMatrix, d_weight: Optional[torch.Tensor] = None,
                        d_bias: Optional[torch.Tensor] = None, want_weight: bool = True, want_bias: bool = True):
    d_out = _need(d_out, torch.float32, "d_out")
    if d_out.dim() != 2 or d_out.shape[0] != fm.batch:
        raise ValueError("ftm_backward_weight: d_out does not match the map")
    l1 = d_out.shape[1]
    if want_weight and d_weight is None:
        d_weight = torch.empty((fm.num_rows, l1), dtype=torch.float32, device=d_out.device)
    if want_bias and d_bias is None:
        d_bias = torch.empty((l1,), dtype=torch.float32, device=d_out.device)
    _call("nnue_ftm_backward_weight", fm.bits.data_ptr(), fm.sink.data_ptr(), d_out.data_ptr(), fm.batch, fm.num_rows,
          fm.positions, l1, _ptr(d_weight if want_weight else None), _ptr(d_bias if want_bias else None), _stream(d_out))
    return d_weight, d_bias


def ftm_backward_values(d_out: torch.Tensor, weight: torch.Tensor, fm: FeatureMatrix,
                        dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    d_out = _need(d_out, torch.float32, "d_out")
    weight = _need(weight, torch.float32, "input.weight")
    b, l1 = d_out.shape
    if tuple(weight.shape) != (fm.num_rows, l1) or b != fm.batch:
        raise ValueError("ftm_backward_values: shape mismatch")
    if dst is None:
        dst = torch.empty((b, fm.positions), dtype=torch.float32, device=d_out.device)
    elif dst.numel() != b * fm.positions:
        raise ValueError("ftm_backward_values: dst has the wrong size")
    # the workspace-taking name (no shape needs a workspace): the name the value gradient is timed by
    _call("nnue_ftm_backward_values_ws", fm.bits.data_ptr(), d_out.data_ptr(), weight.data_ptr(), b, fm.num_rows, fm.positions,
          l1, dst.data_ptr(), None, 0, _stream(d_out))
    return dst


def ftm_backward_sq_count(b: int, f: int, p: int, l1: int) -> int:
    """Floats ftm_backward's sq_partial receives (one sum of squares per weight-gradient tile); 0 = not available."""
    return int(load().nnue_ftm_backward_sq_count(b, f, p, l1))


def ftm_backward_cw_supported(b: int, f: int, p: int, l1: int, l2: int) -> bool:
    """Shapes whose merged backward launch can also carry the classifier's first-layer weight gradient."""
    return bool(load().nnue_ftm_backward_cw_supported(b, f, p, l1, l2))


def ftm_value_planes_supported(b: int, f: int, p: int, l1: int, h: int, w: int, stride: int) -> bool:
    """Shapes whose merged backward reads the table's value planes (ftm_backward(val_planes=...)); NNUE_FTM_VAL_PLANES=0: none."""
    return bool(load().nnue_ftm_value_planes_supported(int(b), int(f), int(p), int(l1), int(h), int(w), int(stride)))


def ftm_value_planes_bytes(b: int, f: int, p: int, l1: int) -> int:
    return int(load().nnue_ftm_value_planes_bytes(int(b), int(f), int(p), int(l1)))


def ftm_backward_ste_chunks(b: int, f: int, p: int, l1: int, h: int, w: int, stride: int) -> int:
    """Runs of STE partials the merged backward's value tiles leave for this shape (ftm_backward(ste=...)); 0: not taken."""
    return int(load().nnue_ftm_backward_ste_chunks(b, f, p, l1, h, w, stride))


def ftm_backward(d_out: torch.Tensor, weight: torch.Tensor, fm: FeatureMatrix, d_weight: Optional[torch.Tensor] = None,
                 d_bias: Optional[torch.Tensor] = None, dst: Optional[torch.Tensor] = None, ft: Optional[torch.Tensor] = None,
                 d_z1: Optional[torch.Tensor] = None, d_w1: Optional[torch.Tensor] = None,
                 sq_partial: Optional[torch.Tensor] = None, buckets=None, small: Optional["NnueClsRider"] = None, ste=None,
                 val_planes: Optional[torch.Tensor] = None):
    """(d_weight, d_bias, d_conv_out) in one launch; bitwise the results of ftm_backward_weight + ftm_backward_values.
    ste = (images [B, 3, H, W], conv_out, thr, stride, partial[, patches]): the value tiles also leave stage 1 of ste_conv_backward
    as [fps * 28][ftm_backward_ste_chunks(...)] floats in `partial` (its second stage: sgd_step(ste=...)); with the im2col
    `patches` [27, B * Gh * Gw] (ftm_conv_binarize(patches=...)) the pixel terms are read from them (the same bits);
    d_conv_out is then stored only when `dst` is given (the third result is None otherwise).
    small (classifier_train_rider(...)): the classifier's small gradients + mean loss run as one more tile family of the launch.
    With ft [B, L1], d_z1 [B, L2] and d_w1 [L2, L1] the launch also writes d_w1 = d_z1^T l0 (the pairwise block of ft).
    buckets (a BucketPlan): d_w1 [K, L2, L1]; ft / d_z1 are then the GROUPED-row copies [tiles*16, .] the bucketed
    classifier step left in its scratch.
    val_planes (with ste, no buckets): the planes ftm_conv_binarize_planes(val_planes=...) wrote from `weight` this step; where
    ftm_value_planes_supported says yes the value tiles read them (six bf16 plane products) instead of the table."""
    d_out = _need(d_out, torch.float32, "d_out")
    weight = _need(weight, torch.float32, "input.weight")
    b, l1 = d_out.shape
    if weight.shape != (fm.num_rows, l1) or b != fm.batch:
        raise ValueError("ftm_backward: shape mismatch")
    if d_weight is None:
        d_weight = torch.empty((fm.num_rows, l1), dtype=torch.float32, device=d_out.device)
    if d_bias is None:
        d_bias = torch.empty((l1,), dtype=torch.float32, device=d_out.device)
    if dst is None and ste is None:
        dst = torch.empty((b, fm.positions), dtype=torch.float32, device=d_out.device)
    elif dst is not None and dst.numel() != b * fm.positions:
        raise ValueError("ftm_backward: dst has the wrong size")
    ste_args = (None, None, None, None, 0, 0, 0, None, 0)
    if ste is not None:
        images, conv_out, thr, stride, part = ste[:5]
        patches = ste[5] if len(ste) > 5 else None
        images = _need(images, torch.float32, "images")
        conv_out = _need(conv_out, torch.float32, "conv_out")
        thr = _need(thr, torch.float32, "visual_threshold")
        if images.dim() != 4 or images.shape[:2] != (b, 3) or conv_out.numel() != b * fm.positions or part.device != d_out.device:
            raise ValueError("ftm_backward: STE operands have the wrong shape")
        h, w = images.shape[2], images.shape[3]
        if patches is not None:
            gh, gw = conv_out_hw(h, w, stride)
            patches = _need(patches, torch.float32, "patches", (27, b * gh * gw))
        ste_args = (images.data_ptr(), _ptr(patches), conv_out.data_ptr(), thr.data_ptr(), h, w, int(stride), part.data_ptr(),
                    part.numel() * part.element_size())
    l2 = 0
    rows = b if buckets is None else buckets.tiles * 16
    if d_w1 is not None:
        ft = _need(ft, torch.float32, "ft")
        d_z1 = _need(d_z1, torch.float32, "d_z1")
        l2 = d_w1.shape[-2]
        want = (l2, l1) if buckets is None else (buckets.K, l2, l1)
        if ft.shape != (rows, l1) or d_z1.numel() != rows * l2 or tuple(d_w1.shape) != want or not d_w1.is_contiguous():
            raise ValueError("ftm_backward: ft / d_z1 / d_w1 shape mismatch")
    args = (fm.bits.data_ptr(), fm.sink.data_ptr(), d_out.data_ptr(), weight.data_ptr(), b, fm.num_rows,
            fm.positions, l1, d_weight.data_ptr(), d_bias.data_ptr(), _ptr(dst),
            _ptr(ft if d_w1 is not None else None), _ptr(d_z1 if d_w1 is not None else None), l2, _ptr(d_w1), _ptr(sq_partial))
    rider = ctypes.pointer(small) if small is not None else None
    if val_planes is not None:
        if buckets is not None:
            raise ValueError("ftm_backward: the value planes have no bucketed form")
        val_planes = _need(val_planes, torch.uint8, "val_planes")
        _call("nnue_ftm_backward_planes", *args, rider, *ste_args, val_planes.data_ptr(), val_planes.numel(), _stream(d_out))
    elif buckets is None:
        _call("nnue_ftm_backward", *args, rider, *ste_args, _stream(d_out))
    else:
        _call("nnue_ftm_backward_bucketed", *args, buckets.K, buckets.seg.data_ptr(), rows, rider, *ste_args, _stream(d_out))
    return d_weight, d_bias, dst


def classifier_train_rider(pairwise: bool, b: int, l1: int, l2: int, l3: int, c: int, h1, h2, sample_loss, loss, grads, scratch,
                           buckets: Optional["BucketPlan"] = None) -> "NnueClsRider":
    """Arguments of the small-gradient tile family for ftm_backward(small=...) when classifier_train_step runs with phases bit 32.
    grads: the six classifier gradients (d_w1, d_b1, d_w2, d_b2, d_w3, d_b3) as classifier_train_step takes them.  The returned
    struct lives on the host and holds device pointers: keep it alive as long as a recorded plan refers to it."""
    out = NnueClsRider()
    _, d_b1, d_w2, d_b2, d_w3, d_b3 = grads
    rc = load().nnue_classifier_train_rider(int(bool(pairwise)), b, l1, l2, l3, c, h1.data_ptr(), h2.data_ptr(), sample_loss.data_ptr(),
                                            loss.data_ptr(), d_b1.data_ptr(), d_w2.data_ptr(), d_b2.data_ptr(), d_w3.data_ptr(),
                                            d_b3.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                            buckets.ref if buckets is not None else None, ctypes.byref(out))
    if rc != 0:
        raise NnueHipError(f"nnue_classifier_train_rider failed (code {rc}): {load().nnue_hip_last_error().decode()}")
    return out


# ---------------------------------------------------------------------------- bucketed layer stacks
class BucketPlan:
    """Per-batch bucket assignment + grouping (struct nnue_buckets): which of the K layer stacks each sample uses and
    the bucket-homogeneous 16-row tiles the first-layer MFMA kernels walk.  Buffers are static (hipGraph-friendly);
    ``bucket_group`` refills them from the active-feature counts of a batch."""

    def __init__(self, batch: int, buckets: int, device):
        self.batch, self.K = int(batch), int(buckets)
        self.tiles = int(load().nnue_bucket_tile_count(self.batch, self.K))
        i32 = dict(dtype=torch.int32, device=device)
        self.bucket = torch.zeros((self.batch,), **i32)
        self.rows = torch.full((self.tiles * 16,), -1, **i32)
        self.tile_bucket = torch.full((self.tiles,), -1, **i32)
        self.seg = torch.zeros((self.K + 1,), **i32)
        self.cstruct = NnueBuckets(self.K, self.bucket.data_ptr(), self.rows.data_ptr(), self.tile_bucket.data_ptr(),
                                   self.seg.data_ptr(), self.tiles)

    @property
    def ref(self):
        return ctypes.byref(self.cstruct)


def bucket_group(n: torch.Tensor, positions: int, buckets: int, plan: Optional[BucketPlan] = None) -> BucketPlan:
    """bucket[b] = min(K-1, n[b]*K // (positions+1)) and the grouping; positions == 0: n holds the bucket ids themselves."""
    n = _need(n, torch.int32, "active-feature counts")
    b = n.numel()
    if plan is None:
        plan = BucketPlan(b, buckets, n.device)
    elif plan.batch != b or plan.K != buckets:
        raise ValueError("bucket_group: plan was built for another batch size / bucket count")
    _call("nnue_bucket_group", n.data_ptr(), b, int(positions), int(buckets), plan.bucket.data_ptr(), plan.rows.data_ptr(),
          plan.tile_bucket.data_ptr(), plan.seg.data_ptr(), _stream(n))
    return plan


# ---------------------------------------------------------------------------- classifier
def classifier_scratch_bytes(b: int, l1: int, l2: int, l3: int, buckets: int = 1) -> int:
    return int(load().nnue_classifier_scratch_bucketed(b, l1, l2, l3, buckets))


def _cls_shapes(w1, b1, w2, b2, w3, b3, l1: int, buckets: Optional[BucketPlan]):
    """Checks the six (possibly stacked) tensors; returns them contiguous with (l2, l3, c, K)."""
    k = buckets.K if buckets is not None else 1
    lead = (k,) if w1.dim() == 3 else ()
    if (w1.dim() == 3) != (buckets is not None) or (lead and w1.shape[0] != k):
        raise ValueError("stacked [K, out, in] classifier weights need a BucketPlan with the same K (and vice versa)")
    l2, l3, c = w1.shape[-2], w2.shape[-2], w3.shape[-2]
    w1 = _need(w1, torch.float32, "classifier.0.weight", (*lead, l2, l1))
    w2 = _need(w2, torch.float32, "classifier.2.weight", (*lead, l3, l2))
    w3 = _need(w3, torch.float32, "classifier.4.weight", (*lead, c, l3))
    if b1 is not None:
        b1 = _need(b1, torch.float32, "classifier.0.bias", (*lead, l2))
        b2 = _need(b2, torch.float32, "classifier.2.bias", (*lead, l3))
        b3 = _need(b3, torch.float32, "classifier.4.bias", (*lead, c))
    return w1, b1, w2, b2, w3, b3, l2, l3, c, k


def classifier_forward(x, pairwise: bool, w1, b1, w2, b2, w3, b3, clip: float = 0.0,
                       scratch: Optional[torch.Tensor] = None, out=None, buckets: Optional[BucketPlan] = None):
    x = _need(x, torch.float32, "classifier input")
    if x.dim() != 2:
        raise ValueError(f"classifier input: expected [B,L1], got {tuple(x.shape)}")
    b, l1 = x.shape
    w1, b1, w2, b2, w3, b3, l2, l3, c, k = _cls_shapes(w1, b1, w2, b2, w3, b3, l1, buckets)
    dev = x.device
    if scratch is None:
        scratch = torch.empty((classifier_scratch_bytes(b, l1, l2, l3, k),), dtype=torch.uint8, device=dev)
    if out is None:
        h1 = torch.empty((b, l2), dtype=torch.float32, device=dev)
        h2 = torch.empty((b, l3), dtype=torch.float32, device=dev)
        logits = torch.empty((b, c), dtype=torch.float32, device=dev)
    else:
        h1, h2, logits = out
    args = (x.data_ptr(), int(bool(pairwise)), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
            b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), float(clip), b, l1, l2, l3, c, h1.data_ptr(), h2.data_ptr(),
            logits.data_ptr(), scratch.data_ptr(), scratch.numel())
    if buckets is None:
        _call("nnue_classifier_forward", *args, _stream(x))
    else:
        _call("nnue_classifier_forward_bucketed", *args, buckets.ref, _stream(x))
    return h1, h2, logits


def classifier_backward(x, pairwise: bool, w1, w2, w3, h1, h2, d_logits, clip: float = 0.0,
                        want_dx: bool = True, scratch: Optional[torch.Tensor] = None, grads=None, d_x=None,
                        buckets: Optional[BucketPlan] = None):
    x = _need(x, torch.float32, "classifier input")
    b, l1 = x.shape
    w1, _, w2, _, w3, _, l2, l3, c, k = _cls_shapes(w1, None, w2, None, w3, None, l1, buckets)
    h1 = _need(h1, torch.float32, "h1", (b, l2))
    h2 = _need(h2, torch.float32, "h2", (b, l3))
    d_logits = _need(d_logits, torch.float32, "d_logits", (b, c))
    dev = x.device
    lead = (k,) if buckets is not None else ()
    if scratch is None:
        scratch = torch.empty((classifier_scratch_bytes(b, l1, l2, l3, k),), dtype=torch.uint8, device=dev)
    if grads is None:
        mk = lambda *s: torch.empty((*lead, *s), dtype=torch.float32, device=dev)  # noqa: E731
        grads = (mk(l2, l1), mk(l2), mk(l3, l2), mk(l3), mk(c, l3), mk(c))
    if want_dx and d_x is None:
        d_x = torch.empty((b, l1), dtype=torch.float32, device=dev)
    args = (x.data_ptr(), int(bool(pairwise)), w1.data_ptr(), w2.data_ptr(), w3.data_ptr(),
            float(clip), h1.data_ptr(), h2.data_ptr(), d_logits.data_ptr(), b, l1, l2, l3, c,
            _ptr(d_x if want_dx else None), *[g.data_ptr() for g in grads], scratch.data_ptr(), scratch.numel())
    if buckets is None:
        _call("nnue_classifier_backward", *args, _stream(x))
    else:
        _call("nnue_classifier_backward_bucketed", *args, buckets.ref, _stream(x))
    return (d_x if want_dx else None), grads


def classifier_train_scratch_bytes(b: int, l1: int, l2: int, l3: int, c: int, buckets: int = 1) -> int:
    return int(load().nnue_classifier_train_scratch_bucketed(b, l1, l2, l3, c, buckets))


def classifier_train_dz1_offset(b: int, l1: int, l2: int, l3: int, c: int, pairwise: bool) -> int:
    """Byte offset of d_z1 [B, L2] inside the classifier's training scratch (valid after phase 1)."""
    return int(load().nnue_classifier_train_dz1_offset(b, l1, l2, l3, c, int(bool(pairwise))))


def classifier_train_fused_tail_supported(b: int, l1: int, l2: int, l3: int, c: int, buckets: int = 1, pairwise: bool = True) -> bool:
    """Whether classifier_train_step accepts phases 123 (59 with the per-sample tail inside the d_x launch) at this shape."""
    return bool(load().nnue_classifier_train_fused_tail_supported(int(b), int(l1), int(l2), int(l3), int(c), int(buckets),
                                                                  int(bool(pairwise))))


def classifier_train_grouped_offsets(b: int, l1: int, l2: int, l3: int, c: int, buckets: int):
    """Byte offsets of (d_z1 grouped [tiles*16, L2], x grouped [tiles*16, L1]) inside the bucketed training scratch."""
    lib = load()
    return (int(lib.nnue_classifier_train_dz1_grouped_offset(b, l1, l2, l3, c, buckets)),
            int(lib.nnue_classifier_train_x_grouped_offset(b, l1, l2, l3, c, buckets)))


# the bits of classifier_train_step's ``phases`` (include/nnue_hip.h, nnue_classifier_train_step)
CLS_PHASE_DX = 1         # activations, per-sample losses and d_x
CLS_PHASE_SMALL = 2      # the mean loss and the six weight/bias gradients (needs CLS_PHASE_DX on the same scratch)
CLS_DW1_BESIDE_DX = 4    # the first-layer weight product shares the d_x launch; the CLS_PHASE_SMALL call only sums its slabs
CLS_L1_SLABS_GIVEN = 8   # the layer-1 slabs are at the start of scratch already (ftm_forward_l1's epilogue)
CLS_DW1_RIDES = 16       # d_w1 is left to ftm_backward's rider (not with CLS_DW1_BESIDE_DX)
CLS_SMALL_RIDE = 32      # ... and so are the small gradients and the mean loss (ftm_backward's `small`)
CLS_TAIL_IN_DX = 64      # the per-sample tail runs inside the d_x launch (only on top of all of 1 | 2 | 8 | 16 | 32)


def classifier_train_step(x, pairwise: bool, w1, b1, w2, b2, w3, b3, labels, grad_scale: float = 1.0, clip: float = 0.0,
                          want_dx: bool = True, scratch: Optional[torch.Tensor] = None, out=None, loss_out=None,
                          grads=None, d_x=None, phases: int = 3, buckets: Optional[BucketPlan] = None, soft=None,
                          distill=None):
    """Forward + mean cross-entropy + backward of the classifier block in one C call.
    soft = (labels_b int64 [B] or None, lam float32 [B] or None, eps): the soft-target entry points (include/nnue_hip.h,
    "soft targets") -- a second label and a weight per sample, label smoothing eps; None: the plain ones.
    distill = (teacher float32 [B, C] or None, alpha, T): the distillation entry points -- (1 - alpha) times the soft loss plus
    alpha T^2 KL(teacher at T || student at T); beside ``soft`` or alone (one label per sample, eps 0).  teacher may be None
    only with alpha == 0, which is the soft call.  ValueError before any call for alpha outside [0, 1] or T not finite and > 0.
    Returns (h1, h2, logits), (sample_loss, loss), d_x, grads."""
    if distill is not None:
        distill = (distill[0], *check_distill(distill[1], distill[2]))
    x = _need(x, torch.float32, "classifier input")
    b, l1 = x.shape
    w1, b1, w2, b2, w3, b3, l2, l3, c, k = _cls_shapes(w1, b1, w2, b2, w3, b3, l1, buckets)
    labels = _need(labels, torch.int64, "labels", (b,))
    dev = x.device
    lead = (k,) if buckets is not None else ()
    mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    if scratch is None:
        scratch = torch.empty((classifier_train_scratch_bytes(b, l1, l2, l3, c, k),), dtype=torch.uint8, device=dev)
    h1, h2, logits = out if out is not None else (mk(b, l2), mk(b, l3), mk(b, c))
    sample_loss, loss = loss_out if loss_out is not None else (mk(b), mk())
    if grads is None:
        grads = (mk(*lead, l2, l1), mk(*lead, l2), mk(*lead, l3, l2), mk(*lead, l3), mk(*lead, c, l3), mk(*lead, c))
    if want_dx and d_x is None:
        d_x = mk(b, l1)
    args = (x.data_ptr(), int(bool(pairwise)), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
            b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), float(clip), labels.data_ptr(), float(grad_scale), b, l1, l2, l3, c,
            h1.data_ptr(), h2.data_ptr(), logits.data_ptr(), sample_loss.data_ptr(), loss.data_ptr(),
            _ptr(d_x if want_dx else None), *[g.data_ptr() for g in grads], scratch.data_ptr(), scratch.numel(), int(phases))
    if distill is not None and soft is None:
        soft = (None, None, 0.0)
    if soft is not None:
        labels_b, lam, eps = soft
        if labels_b is not None:
            labels_b = _need(labels_b, torch.int64, "labels_b", (b,))
        if lam is not None:
            lam = _need(lam, torch.float32, "lam", (b,))
        args += (_ptr(labels_b), _ptr(lam), float(eps))
    if distill is not None:
        teacher, alpha, temperature = distill
        if teacher is not None:
            teacher = _need(teacher, torch.float32, "teacher logits", (b, c))
        elif alpha > 0.0:
            raise ValueError("distill: alpha > 0 needs teacher logits")
        args += (_ptr(teacher), alpha, temperature)
    form = "_distill" if distill is not None else "_soft" if soft is not None else ""
    if buckets is None:
        _call(f"nnue_classifier_train_step{form}", *args, _stream(x))
    else:
        _call(f"nnue_classifier_train_step{form}_bucketed", *args, buckets.ref, _stream(x))
    return (h1, h2, logits), (sample_loss, loss), (d_x if want_dx else None), grads


# ---------------------------------------------------------------------------- loss + step tail
def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, grad_scale: float = 1.0, want_grad: bool = True,
                  out=None):
    logits = _need(logits, torch.float32, "logits")
    b, c = logits.shape
    labels = _need(labels, torch.int64, "labels", (b,))
    dev = logits.device
    if out is None:
        sample_loss = torch.empty((b,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d_logits = torch.empty((b, c), dtype=torch.float32, device=dev) if want_grad else None
    else:
        sample_loss, loss, d_logits = out
    _call("nnue_cross_entropy", logits.data_ptr(), labels.data_ptr(), b, c, float(grad_scale), sample_loss.data_ptr(),
          loss.data_ptr(), _ptr(d_logits), _stream(logits))
    return sample_loss, loss, d_logits


def cross_entropy_soft(logits: torch.Tensor, labels: torch.Tensor, labels_b: Optional[torch.Tensor] = None,
                       lam: Optional[torch.Tensor] = None, eps: float = 0.0, grad_scale: float = 1.0, want_grad: bool = True, out=None):
    """cross_entropy on soft targets (include/nnue_hip.h, "soft targets"): lam CE(z, labels) + (1 - lam) CE(z, labels_b), each with
    label_smoothing = eps.  labels_b = lam = None: one label per sample."""
    logits = _need(logits, torch.float32, "logits")
    b, c = logits.shape
    labels = _need(labels, torch.int64, "labels", (b,))
    if labels_b is not None:
        labels_b = _need(labels_b, torch.int64, "labels_b", (b,))
    if lam is not None:
        lam = _need(lam, torch.float32, "lam", (b,))
    dev = logits.device
    if out is None:
        sample_loss = torch.empty((b,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d_logits = torch.empty((b, c), dtype=torch.float32, device=dev) if want_grad else None
    else:
        sample_loss, loss, d_logits = out
    _call("nnue_cross_entropy_soft", logits.data_ptr(), labels.data_ptr(), _ptr(labels_b), _ptr(lam), float(eps), b, c, float(grad_scale),
          sample_loss.data_ptr(), loss.data_ptr(), _ptr(d_logits), _stream(logits))
    return sample_loss, loss, d_logits


def check_distill(alpha, temperature):
    """(alpha, T) of a distillation call as floats; ValueError unless alpha lies in [0, 1] and T is finite and positive (what
    the C entry points refuse with NNUE_E_ARG)."""
    alpha, temperature = float(alpha), float(temperature)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"distill alpha = {alpha} must lie in [0, 1]")
    if not (0.0 < temperature < float("inf")):
        raise ValueError(f"distill temperature = {temperature} must be finite and positive")
    return alpha, temperature


def cross_entropy_distill(logits: torch.Tensor, labels: torch.Tensor, teacher: Optional[torch.Tensor], alpha: float,
                          temperature: float = 1.0, labels_b: Optional[torch.Tensor] = None, lam: Optional[torch.Tensor] = None,
                          eps: float = 0.0, grad_scale: float = 1.0, want_grad: bool = True, out=None):
    """cross_entropy_soft with a teacher (include/nnue_hip.h, "soft targets"): (1 - alpha) times the soft loss plus
    alpha T^2 KL(softmax(teacher / T) || softmax(logits / T)).  teacher float32 [B, C]; None only with alpha == 0."""
    alpha, temperature = check_distill(alpha, temperature)
    logits = _need(logits, torch.float32, "logits")
    b, c = logits.shape
    labels = _need(labels, torch.int64, "labels", (b,))
    if labels_b is not None:
        labels_b = _need(labels_b, torch.int64, "labels_b", (b,))
    if lam is not None:
        lam = _need(lam, torch.float32, "lam", (b,))
    if teacher is not None:
        teacher = _need(teacher, torch.float32, "teacher logits", (b, c))
    elif alpha > 0.0:
        raise ValueError("cross_entropy_distill: alpha > 0 needs teacher logits")
    dev = logits.device
    if out is None:
        sample_loss = torch.empty((b,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d_logits = torch.empty((b, c), dtype=torch.float32, device=dev) if want_grad else None
    else:
        sample_loss, loss, d_logits = out
    _call("nnue_cross_entropy_distill", logits.data_ptr(), labels.data_ptr(), _ptr(labels_b), _ptr(lam), float(eps), b, c, float(grad_scale),
          sample_loss.data_ptr(), loss.data_ptr(), _ptr(d_logits), _ptr(teacher), alpha, temperature, _stream(logits))
    return sample_loss, loss, d_logits


def confusion_accumulate(logits: torch.Tensor, labels: torch.Tensor, confusion: Optional[torch.Tensor] = None) -> torch.Tensor:
    """confusion[truth, pred] += 1 for every row of the batch (int64 [K, K], K = C or 2 when C == 1)."""
    logits = _need(logits, torch.float32, "logits")
    b, c = logits.shape
    labels = _need(labels, torch.int64, "labels", (b,))
    k = 2 if c == 1 else c
    if confusion is None:
        confusion = torch.zeros((k, k), dtype=torch.int64, device=logits.device)
    else:
        _need(confusion, torch.int64, "confusion", (k, k))
    _call("nnue_confusion_accumulate", logits.data_ptr(), labels.data_ptr(), b, c, confusion.data_ptr(), _stream(logits))
    return confusion


def sgd_scratch_bytes(count: int) -> int:
    return int(load().nnue_sgd_scratch(count))


def sqnorm_partials(grads: torch.Tensor, partial: torch.Tensor) -> torch.Tensor:
    """partial[i] = block partial sums of grads^2 (their sum is ||grads||^2); fixed order."""
    grads = _need(grads, torch.float32, "gradient shard")
    _need(partial, torch.float32, "partials")
    _call("nnue_sqnorm_partials", grads.data_ptr(), grads.numel(), partial.data_ptr(), partial.numel(), _stream(grads))
    return partial


def ftm_gram_scratch(fm: "FeatureMatrix") -> int:
    """Floats of scratch ftm_gram_sqnorm needs for this map."""
    return int(load().nnue_ftm_gram_scratch(fm.bits.shape[0], fm.num_rows, fm.positions))


def ftm_gram_sqnorm(fm: "FeatureMatrix", d_out: torch.Tensor, gram: torch.Tensor, sq_partial: torch.Tensor,
                    tail=None) -> torch.Tensor:
    """Partial sums of ||A^T d_out||_F^2 over the table rows the map reaches, from two B x B Gram matrices.  ``gram``:
    ``ftm_gram_scratch(fm)`` floats of scratch; its first B*B hold A A^T afterwards.  tail = (d_weight, d_bias): the workgroups of
    ftm_backward_tail_rows ride in the first launch (same results, one launch fewer)."""
    d_out = _need(d_out, torch.float32, "d_out")
    b, l1 = d_out.shape
    _need(gram, torch.float32, "gram scratch", (ftm_gram_scratch(fm),))
    _need(sq_partial, torch.float32, "gram partials", (int(load().nnue_ftm_gram_sq_count(b, l1)),))
    if tail is not None:
        d_weight, d_bias = tail
        _call("nnue_ftm_gram_sqnorm_tail", fm.bits.data_ptr(), fm.sink.data_ptr(), d_out.data_ptr(), b, fm.num_rows, fm.positions, l1,
              gram.data_ptr(), sq_partial.data_ptr(), d_weight.data_ptr(), d_bias.data_ptr(), _stream(d_out))
        return sq_partial
    _call("nnue_ftm_gram_sqnorm", fm.bits.data_ptr(), d_out.data_ptr(), b, fm.num_rows, fm.positions, l1, gram.data_ptr(),
          sq_partial.data_ptr(), _stream(d_out))
    return sq_partial


def ftm_backward_tail_rows(d_out: torch.Tensor, fm: "FeatureMatrix", d_weight: torch.Tensor, d_bias: torch.Tensor) -> None:
    d_out = _need(d_out, torch.float32, "d_out")
    b, l1 = d_out.shape
    _call("nnue_ftm_backward_tail_rows", fm.sink.data_ptr(), d_out.data_ptr(), b, fm.num_rows, fm.positions, l1, d_weight.data_ptr(),
          d_bias.data_ptr(), _stream(d_out))


def _ftm_weight_update(name: str, d_out, fm, weight, coef, lr_dev, scalars, momentum_rows=None, adam=None, nxt=None,
                       weight_clip: float = 0.0, ema: Optional["WeightAverage"] = None) -> None:
    """The one body of ftm_backward_weight_update{,_forward}{,_adam}; `name`: the public function, "nnue_" + name its C entry
    point.  scalars: the optimizer's C arguments between the state pointers and lr_dev; adam = (exp_avg_rows, exp_avg_sq_rows,
    step_counter), else SGD on momentum_rows; nxt = (fm_next, bias, out_next): the pass also forms that map's forward.
    weight_clip > 0: the ``_clip`` sibling of the entry point, which clamps the new table elements (include/nnue_hip.h, "weight
    clip"); 0 is the plain entry point.
    ema (a WeightAverage over the rows that match `weight`): the ``_ema`` sibling, which also moves the average of every table
    element it stores (include/nnue_hip.h, "weight average"), in the fused pass (nxt) as in the product's epilogue."""
    weight_clip = checked_weight_clip(weight_clip)
    ema_args = ()
    if ema is not None:
        _need(ema.ema, torch.float32, "average's rows", tuple(weight.shape))
        name, scalars = name + "_ema", (*scalars, weight_clip)
        ema_args = ema.args()
    elif weight_clip > 0.0:
        name, scalars = name + "_clip", (*scalars, weight_clip)
    d_out = _need(d_out, torch.float32, "d_out")
    b, l1 = d_out.shape
    weight = _need(weight, torch.float32, "input.weight", (fm.num_rows, l1))
    if nxt is not None:
        fm_next, bias, out_next = nxt
        bias = _need(bias, torch.float32, "input.bias", (l1,))
        out_next = _need(out_next, torch.float32, "out_next", (fm_next.batch, l1))
    if adam is not None:
        _need(adam[0], torch.float32, "exp_avg rows")
        _need(adam[1], torch.float32, "exp_avg_sq rows")
    _need(coef, torch.float32, "clip coefficient")
    if adam is not None:
        _need(adam[2], torch.int32, "step counter", (1,))
        state = (adam[0].data_ptr(), adam[1].data_ptr(), coef.data_ptr(), adam[2].data_ptr())
    else:
        state = (_ptr(momentum_rows), coef.data_ptr())
    forward = ()
    if nxt is not None:
        if fm.batch != b or fm_next.positions != fm.positions or fm_next.num_rows != fm.num_rows:
            raise ValueError(f"{name}: the maps do not match d_out / each other")
        forward = (fm_next.bits.data_ptr(), fm_next.sink.data_ptr(), fm_next.batch, bias.data_ptr(), out_next.data_ptr(),
                   fm_next.scratch.data_ptr(), fm_next.scratch.numel())
    _call("nnue_" + name, fm.bits.data_ptr(), d_out.data_ptr(), b, fm.num_rows, fm.positions, l1, weight.data_ptr(), *state, *scalars,
          _ptr(lr_dev), *forward, *ema_args, _stream(d_out))


def ftm_backward_weight_update(d_out: torch.Tensor, fm: "FeatureMatrix", weight: torch.Tensor, momentum_rows: Optional[torch.Tensor],
                               coef: torch.Tensor, lr: float, momentum: float, weight_decay: float, grad_scale: float,
                               first_step: bool, lr_dev: Optional[torch.Tensor] = None, weight_clip: float = 0.0,
                               ema: Optional["WeightAverage"] = None) -> None:
    """weight rows [0, direct) <- SGD update with d_W = A^T d_out formed and consumed in the product's epilogue.
    lr_dev (device float32 scalar): the learning rate is read from it instead of `lr`.  weight_clip, ema: see _ftm_weight_update."""
    _ftm_weight_update("ftm_backward_weight_update", d_out, fm, weight, coef, lr_dev, momentum_rows=momentum_rows, weight_clip=weight_clip, ema=ema,
                       scalars=(float(lr), float(momentum), float(weight_decay), float(grad_scale), int(bool(first_step))))


def ftm_update_forward_supported(batch: int, num_rows: int, positions: int, l1: int, batch_next: Optional[int] = None) -> bool:
    """batch: rows of the gradient's factors (the global batch under the factor exchange); batch_next: rows of the next map."""
    return bool(load().nnue_ftm_update_forward_supported(int(batch), int(batch if batch_next is None else batch_next), int(num_rows),
                                                         int(positions), int(l1)))


def ftm_backward_weight_update_forward(d_out: torch.Tensor, fm: "FeatureMatrix", weight: torch.Tensor,
                                       momentum_rows: Optional[torch.Tensor], coef: torch.Tensor, lr: float, momentum: float,
                                       weight_decay: float, grad_scale: float, first_step: bool, fm_next: "FeatureMatrix",
                                       bias: torch.Tensor, out_next: torch.Tensor, lr_dev: Optional[torch.Tensor] = None,
                                       weight_clip: float = 0.0, ema: Optional["WeightAverage"] = None) -> None:
    """ftm_backward_weight_update(d_out, fm, ...) and ftm_forward(weight, bias, fm_next, out=out_next) in one pass over the
    table (bitwise the two calls).  `bias` and table row F-1 must already be updated (sgd_step).  weight_clip: the forward
    contracts the clamped table (see _ftm_weight_update)."""
    _ftm_weight_update("ftm_backward_weight_update_forward", d_out, fm, weight, coef, lr_dev, momentum_rows=momentum_rows, weight_clip=weight_clip, ema=ema,
                       nxt=(fm_next, bias, out_next), scalars=(float(lr), float(momentum), float(weight_decay), float(grad_scale), int(bool(first_step))))


def ftm_backward_weight_update_adam(d_out: torch.Tensor, fm: "FeatureMatrix", weight: torch.Tensor, exp_avg_rows: torch.Tensor,
                                    exp_avg_sq_rows: torch.Tensor, coef: torch.Tensor, step_counter: torch.Tensor, lr: float,
                                    betas, eps: float, weight_decay: float, grad_scale: float,
                                    lr_dev: Optional[torch.Tensor] = None, weight_clip: float = 0.0,
                                    ema: Optional["WeightAverage"] = None) -> None:
    """weight rows [0, direct) and the matching moment rows <- Adam update with d_W = A^T d_out formed and consumed in the
    product's epilogue.  ``step_counter`` (device int32) is read, not advanced: adam_step(ext_applied_elsewhere=True) of the
    same step advances it and leaves ``coef``."""
    _ftm_weight_update("ftm_backward_weight_update_adam", d_out, fm, weight, coef, lr_dev, adam=(exp_avg_rows, exp_avg_sq_rows, step_counter),
                       weight_clip=weight_clip, ema=ema,
                       scalars=(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale)))


def ftm_backward_weight_update_forward_adam(d_out: torch.Tensor, fm: "FeatureMatrix", weight: torch.Tensor, exp_avg_rows: torch.Tensor,
                                            exp_avg_sq_rows: torch.Tensor, coef: torch.Tensor, step_counter: torch.Tensor, lr: float,
                                            betas, eps: float, weight_decay: float, grad_scale: float, fm_next: "FeatureMatrix",
                                            bias: torch.Tensor, out_next: torch.Tensor, lr_dev: Optional[torch.Tensor] = None,
                                            weight_clip: float = 0.0, ema: Optional["WeightAverage"] = None) -> None:
    """ftm_backward_weight_update_adam(d_out, fm, ...) and ftm_forward(weight, bias, fm_next, out=out_next) in one pass over the
    table (bitwise the two calls).  `bias` and table row F-1 must already be updated (adam_step)."""
    _ftm_weight_update("ftm_backward_weight_update_forward_adam", d_out, fm, weight, coef, lr_dev,
                       adam=(exp_avg_rows, exp_avg_sq_rows, step_counter), nxt=(fm_next, bias, out_next), weight_clip=weight_clip, ema=ema,
                       scalars=(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale)))


class FactorExchange:
    """Buffers of the factor exchange (include/nnue_hip.h, nnue_dp_factor_*): ``chunks`` uint8 [world][chunk_bytes] is the
    all-gather's receive buffer, ``own`` this rank's slice of it (sent in place); ``d_ft`` / ``sink`` are float views of the
    own chunk that the step's kernels write directly; ``g_*`` the global factors every rank rebuilds after the gather."""

    def __init__(self, world: int, rank: int, batch: int, positions: int, num_rows: int, l1: int, head: int, tail_lo: int,
                 tail: int, device):
        L = load()
        self.world, self.rank, self.batch, self.positions, self.l1 = world, rank, batch, positions, l1
        self.head, self.tail_lo, self.tail = int(head), int(tail_lo), int(tail)
        small = self.head + self.tail
        self.chunk_bytes = int(L.nnue_dp_factor_chunk_bytes(batch, positions, l1, small))
        if self.chunk_bytes <= 0 or self.chunk_bytes % 16:
            raise NnueHipError("nnue_dp_factor_chunk_bytes: unusable shape")
        self.chunks = torch.zeros((world, self.chunk_bytes), dtype=torch.uint8, device=device)
        self.own = self.chunks[rank]
        off = [int(L.nnue_dp_factor_offset(w, batch, positions, l1, small)) for w in range(4)]
        self.d_ft = self.own[off[0]:off[0] + batch * l1 * 4].view(torch.float32).view(batch, l1)
        self.sink = self.own[off[1]:off[1] + batch * 4].view(torch.float32)
        rows = world * batch
        self.g_dft = torch.empty((rows, l1), dtype=torch.float32, device=device)
        # the global map as a FeatureMatrix: what nnue_ftm_gram_sqnorm / nnue_ftm_backward_weight_update take (no forward scratch)
        self.g_fm = FeatureMatrix(torch.empty((rows, positions), dtype=torch.uint8, device=device),
                                  torch.zeros((rows,), dtype=torch.int32, device=device),
                                  torch.empty((rows,), dtype=torch.float32, device=device),
                                  torch.empty((16,), dtype=torch.uint8, device=device), positions, num_rows)

    def pack(self, fm: "FeatureMatrix", flat_grads: torch.Tensor) -> None:
        """own chunk <- map bits + the small gradients (d_ft and sink are already there)."""
        _call("nnue_dp_factor_pack", fm.bits.data_ptr(), flat_grads.data_ptr(), self.head, self.tail_lo, self.tail, self.batch,
              self.positions, self.l1, self.own.data_ptr(), _stream(flat_grads))

    def unpack(self, flat_grads: torch.Tensor) -> None:
        """gathered chunks -> global factors; flat_grads' small parts <- their sum over the ranks (rank order)."""
        _call("nnue_dp_factor_unpack", self.chunks.data_ptr(), self.world, self.batch, self.positions, self.l1, self.head, self.tail_lo,
              self.tail, self.g_fm.bits.data_ptr(), self.g_fm.sink.data_ptr(), self.g_dft.data_ptr(), flat_grads.data_ptr(),
              _stream(flat_grads))


def checked_weight_clip(value) -> float:
    """The weight clip's bound as a float: 0 (off) or a finite positive number; ValueError otherwise."""
    value = float(value)
    if not 0.0 <= value < float("inf"):  # (NaN fails the comparison)
        raise ValueError(f"weight_clip = {value} must be finite and not negative")
    return value


class WeightClip:
    """The weight clip of a flat buffer (include/nnue_hip.h, "weight clip"): the bound and up to four half-open element ranges
    [(lo, hi), ...] of the buffer, as sgd_step / adam_step take it (``clip=``).  ``array`` is the host array the C call reads;
    a recorded plan holds this object's array, which keeps it alive."""

    def __init__(self, bound: float, ranges):
        self.bound = checked_weight_clip(bound)
        self.ranges = [(int(lo), int(hi)) for lo, hi in ranges if int(lo) < int(hi)]
        if len(self.ranges) > 4 or any(lo < 0 for lo, _ in self.ranges):
            raise ValueError(f"a weight clip takes at most four ranges of non-negative indices, got {self.ranges}")
        self.array = (ctypes.c_int64 * (2 * max(1, len(self.ranges))))(*[x for r in self.ranges for x in r])

    @property
    def on(self) -> bool:
        return self.bound > 0.0 and bool(self.ranges)

    def window(self, lo: int, hi: int) -> "WeightClip":
        """The clip of the slice [lo, hi) of the buffer: the ranges intersected with it, in the slice's own indices (the sharded
        update's call covers one shard)."""
        return WeightClip(self.bound, [(max(a, lo) - lo, min(b, hi) - lo) for a, b in self.ranges])

    def args(self):
        return (self.bound, self.array, len(self.ranges))


def checked_ema_decay(value) -> float:
    """The weight average's decay as a float: 0 (off) or a number in (0, 1); ValueError otherwise."""
    value = float(value)
    if not 0.0 <= value < 1.0:  # (NaN fails the comparison)
        raise ValueError(f"ema_decay = {value} must be 0 (off) or lie in (0, 1)")
    return value


def ema_omd(decay: float) -> float:
    """The rate the kernels take for `decay` (include/nnue_hip.h, "weight average"): float32(1 - float64(decay))."""
    return float(torch.tensor(1.0 - float(decay), dtype=torch.float64).to(torch.float32))


EMA_WARMUP_MAX = 1 << 24  # entries of a warm-up table (64 MB): decays up to 1 - 5.4e-7


def ema_warmup_table(decay: float) -> torch.Tensor:
    """The rates of a warmed-up average as a per-step table (float32, CPU) for nnue_lr_schedule_step: step t, counted from 0,
    uses omd_t = float32(1 - decay_t) with decay_t = min(decay, (1 + t) / (10 + t)) in float64; the table ends at the first t
    at which the decay itself is reached, which every later step then uses (the schedule launch clamps its position)."""
    decay = checked_ema_decay(decay)
    if decay == 0.0:
        raise ValueError("a warm-up needs ema_decay > 0")
    n = 1
    if decay > 0.1:  # (1 + t) / (10 + t) >= decay  <=>  t >= (10 decay - 1) / (1 - decay)
        n = int((10.0 * decay - 1.0) / (1.0 - decay)) + 2
    if n > EMA_WARMUP_MAX:
        raise ValueError(f"ema_warmup with ema_decay = {decay} needs a table of {n} steps (at most {EMA_WARMUP_MAX})")
    t = torch.arange(n, dtype=torch.float64)
    decay_t = torch.clamp((1.0 + t) / (10.0 + t), max=decay)
    return (1.0 - decay_t).to(torch.float32)


class WeightAverage:
    """The weight average as the optimizer calls take it (``ema=``; include/nnue_hip.h, "weight average"): the average's
    buffer, laid out like the parameters the call updates, its rate omd = float32(1 - decay), and optionally the device float32
    scalar that replaces the rate (as lr_dev replaces lr)."""

    def __init__(self, ema: torch.Tensor, omd: float, omd_dev: Optional[torch.Tensor] = None):
        self.ema = _need(ema, torch.float32, "weight average")
        self.omd = float(omd)
        if omd_dev is None and not 0.0 < self.omd <= 1.0:
            raise ValueError(f"the weight average's rate omd = {self.omd} must lie in (0, 1]")
        if omd_dev is not None:
            _need(omd_dev, torch.float32, "weight average's rate", (1,))
        self.omd_dev = omd_dev

    def window(self, lo: int, hi: int) -> "WeightAverage":
        """The average of the slice [lo, hi) of the buffer (the sharded update's shard)."""
        return WeightAverage(self.ema[lo:hi], self.omd, self.omd_dev)

    def args(self):
        return (self.ema.data_ptr(), self.omd, _ptr(self.omd_dev))


def ema_update(ema: torch.Tensor, params: torch.Tensor, omd: float, omd_dev: Optional[torch.Tensor] = None) -> None:
    """ema <- fmaf(omd, params - ema, ema), element by element: the stand-alone pass of the weight average (nnue_ema_update).
    Contiguous float32 tensors of one shape, any 4-byte-aligned views; omd_dev (device float32 scalar) replaces omd."""
    _need(ema, torch.float32, "weight average")
    _need(params, torch.float32, "params", tuple(ema.shape))
    if not ema.is_contiguous() or not params.is_contiguous():
        raise ValueError("ema_update: both tensors must be contiguous (the average is written in place)")
    if omd_dev is not None:
        _need(omd_dev, torch.float32, "weight average's rate", (1,))
    _call("nnue_ema_update", ema.data_ptr(), params.data_ptr(), ema.numel(), float(omd), _ptr(omd_dev), _stream(ema))


def _clip_ema_args(clip: Optional[WeightClip], ema: Optional[WeightAverage], shape):
    """(entry-point suffix, arguments between lr_dev and the stream) of a flat optimizer call."""
    clipped = clip is not None and clip.on
    if ema is not None:
        _need(ema.ema, torch.float32, "weight average", shape)
        return "_ema", (*(clip.args() if clipped else (0.0, None, 0)), *ema.args())
    return ("_clip", clip.args()) if clipped else ("", ())


def sgd_step(params: torch.Tensor, grads: torch.Tensor, momentum_buf: Optional[torch.Tensor], lr: float,
             momentum: float, weight_decay: float, max_norm: float, grad_scale: float, first_step: bool,
             norm_out: Optional[torch.Tensor], scratch: torch.Tensor, ste=None, ext=None,
             coef_out: Optional[torch.Tensor] = None, ext_applied_elsewhere: bool = False,
             lr_dev: Optional[torch.Tensor] = None, clip: Optional[WeightClip] = None,
             ema: Optional[WeightAverage] = None) -> None:
    """ste = (partial scratch of ste_conv_backward(stages=1), chunks, fps, d_thr, d_weight): the deferred second stage
    runs inside the norm launch; d_thr / d_weight must be the first elements of `grads`.  lr_dev (device float32 scalar): the
    learning rate is read from it instead of `lr` (changes between steps need no re-recording / re-capture).  clip (a
    WeightClip that is ``on``): nnue_sgd_step_clip, which clamps the updated elements of its ranges; None or off: nnue_sgd_step.
    ema (a WeightAverage laid out like params): nnue_sgd_step_ema, which also moves the average of every element it stores."""
    params = _need(params, torch.float32, "flat params")
    grads = _need(grads, torch.float32, "flat grads", tuple(params.shape))
    if momentum_buf is not None:
        _need(momentum_buf, torch.float32, "momentum buffer", tuple(params.shape))
    if ste is not None:
        part, chunks, fps, d_thr, d_weight = ste
        ste_args = (part.data_ptr(), int(chunks), int(fps), d_thr.data_ptr(), d_weight.data_ptr())
    else:
        ste_args = (None, 0, 0, None, None)
    # ext = (partials, lo, hi): a producer's sums of squares for grads[lo:hi] (e.g. ftm_backward(sq_partial=...))
    ext_args = (ext[0].data_ptr(), ext[0].numel(), int(ext[1]), int(ext[2])) if ext is not None else (None, 0, 0, 0)
    suffix, tail = _clip_ema_args(clip, ema, tuple(params.shape))
    _call("nnue_sgd_step" + suffix, params.data_ptr(), grads.data_ptr(), _ptr(momentum_buf), params.numel(), float(lr),
          float(momentum), float(weight_decay), float(max_norm), float(grad_scale), int(bool(first_step)),
          _ptr(norm_out), scratch.data_ptr(), scratch.numel(), *ste_args, *ext_args, _ptr(coef_out), int(bool(ext_applied_elsewhere)),
          _ptr(lr_dev), *tail, _stream(params))


def lr_schedule_step(table: torch.Tensor, position: torch.Tensor, lr_out: torch.Tensor) -> None:
    """lr_out[0] <- table[clamp(position[0], 0, n-1)], then position[0] += 1 (saturating): one optimizer step of a tabulated
    learning-rate schedule, on the device -- recorded into plans and captured into graphs like every other call."""
    table = _need(table, torch.float32, "schedule table")
    if table.dim() != 1 or table.numel() < 1:
        raise ValueError(f"schedule table: expected a 1-D tensor of at least one value, got shape {tuple(table.shape)}")
    _need(position, torch.int32, "schedule position", (1,))
    _need(lr_out, torch.float32, "learning rate", (1,))
    _call("nnue_lr_schedule_step", table.data_ptr(), table.numel(), position.data_ptr(), lr_out.data_ptr(), _stream(table))


def adam_step(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
              step_counter: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
              max_norm: float = 0.0, grad_scale: float = 1.0, norm_out: Optional[torch.Tensor] = None,
              scratch: Optional[torch.Tensor] = None, lr_dev: Optional[torch.Tensor] = None, ext=None,
              coef_out: Optional[torch.Tensor] = None, ext_applied_elsewhere: bool = False,
              clip: Optional[WeightClip] = None, ema: Optional[WeightAverage] = None) -> None:
    """ext / coef_out / ext_applied_elsewhere as in sgd_step (nnue_adam_step_ext): ext = (partials, lo, hi), a producer's sums of
    squares for grads[lo:hi]; with ext_applied_elsewhere that range of params and moments is left to the producer.  clip as in
    sgd_step: the ``_clip`` sibling of whichever of the two entry points the call takes; ema as in sgd_step: its ``_ema`` sibling."""
    params = _need(params, torch.float32, "flat params")
    shape = tuple(params.shape)
    grads = _need(grads, torch.float32, "flat grads", shape)
    _need(exp_avg, torch.float32, "exp_avg", shape)
    _need(exp_avg_sq, torch.float32, "exp_avg_sq", shape)
    _need(step_counter, torch.int32, "step counter", (1,))
    if scratch is None:
        scratch = torch.empty((sgd_scratch_bytes(params.numel()),), dtype=torch.uint8, device=params.device)
    suffix, clip_args = _clip_ema_args(clip, ema, shape)
    if ext is not None or coef_out is not None or ext_applied_elsewhere:
        ext_args = (ext[0].data_ptr(), ext[0].numel(), int(ext[1]), int(ext[2])) if ext is not None else (None, 0, 0, 0)
        _call("nnue_adam_step_ext" + suffix, params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
              step_counter.data_ptr(), params.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
              float(max_norm), float(grad_scale), _ptr(norm_out), scratch.data_ptr(), scratch.numel(), *ext_args, _ptr(coef_out),
              int(bool(ext_applied_elsewhere)), _ptr(lr_dev), *clip_args, _stream(params))
        return
    _call("nnue_adam_step" + suffix, params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
          step_counter.data_ptr(), params.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
          float(max_norm), float(grad_scale), _ptr(norm_out), scratch.data_ptr(), scratch.numel(), _ptr(lr_dev), *clip_args, _stream(params))


def load_batch(images_u8: torch.Tensor, labels_all: torch.Tensor, indices: torch.Tensor, augment: bool, seed: int, step: int,
               out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None):
    """uint8 [N,H,W,3] dataset + indices [B] -> normalised float32 [B,3,H,W] (+ light augmentation) and labels [B]."""
    images_u8 = _need(images_u8, torch.uint8, "dataset images")
    if images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError(f"dataset images: expected uint8 [N,H,W,3], got {tuple(images_u8.shape)}")
    n, h, w, _ = images_u8.shape
    labels_all = _need(labels_all, torch.int64, "dataset labels", (n,))
    indices = _need(indices, torch.int64, "indices")
    b = indices.numel()
    if out is None:
        out = torch.empty((b, 3, h, w), dtype=torch.float32, device=images_u8.device)
    elif tuple(out.shape) != (b, 3, h, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("load_batch: out must be a contiguous float32 [B,3,H,W] tensor")
    if labels_out is None:
        labels_out = torch.empty((b,), dtype=torch.int64, device=images_u8.device)
    _call("nnue_load_batch", images_u8.data_ptr(), labels_all.data_ptr(), indices.data_ptr(), b, h, w, n, int(bool(augment)),
          int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), out.data_ptr(), labels_out.data_ptr(), _stream(images_u8))
    return out, labels_out


LOAD_POLICIES = {"none": 0, "light": 1, "medium": 2}  # nnue_load_batch_policy's policy argument


def load_batch_policy(images_u8: torch.Tensor, labels_all: torch.Tensor, indices: torch.Tensor, policy: int, seed: int, step: int,
                      out_hw: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                      labels_out: Optional[torch.Tensor] = None, params_out: Optional[torch.Tensor] = None):
    """uint8 [N,H,W,3] dataset + indices [B] -> augmented (policy 0 none / 1 light / 2 medium), resized to out_hw and normalised
    float32 [B,3,Ho,Wo] and labels [B]; params_out (float32 [B, load_batch_params_count()]) receives what was drawn."""
    images_u8 = _need(images_u8, torch.uint8, "dataset images")
    if images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError(f"dataset images: expected uint8 [N,H,W,3], got {tuple(images_u8.shape)}")
    n, h, w, _ = images_u8.shape
    ho, wo = (h, w) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    labels_all = _need(labels_all, torch.int64, "dataset labels", (n,))
    indices = _need(indices, torch.int64, "indices")
    b = indices.numel()
    if out is None:
        out = torch.empty((b, 3, max(ho, 0), max(wo, 0)), dtype=torch.float32, device=images_u8.device)
    elif tuple(out.shape) != (b, 3, ho, wo) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("load_batch_policy: out must be a contiguous float32 [B,3,Ho,Wo] tensor")
    if labels_out is None:
        labels_out = torch.empty((b,), dtype=torch.int64, device=images_u8.device)
    if params_out is not None:
        params_out = _need(params_out, torch.float32, "params_out", (b, load_batch_params_count()))
        if not params_out.is_contiguous():
            raise ValueError("load_batch_policy: params_out must be contiguous (it is written in place)")
    _call("nnue_load_batch_policy", images_u8.data_ptr(), labels_all.data_ptr(), indices.data_ptr(), b, h, w, n, ho, wo, int(policy),
          int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), out.data_ptr(), labels_out.data_ptr(), _ptr(params_out),
          _stream(images_u8))
    return out, labels_out


def load_batch_params_count() -> int:
    return int(load().nnue_load_batch_params_count())


MIX_MODES = {"none": 0, "mixup": 1, "cutmix": 2}  # nnue_mix_batch's mode argument


def mix_batch(images: torch.Tensor, labels: torch.Tensor, mode: int, lam: float = 1.0, box=(0, 0, 0, 0),
              labels_b_out: Optional[torch.Tensor] = None, lam_out: Optional[torch.Tensor] = None):
    """Batch-level mixing IN PLACE on float32 [B,3,H,W]: sample i with B-1-i; mode 0 none / 1 mixup (weight lam) / 2 CutMix (the
    samples swap the pixels of box = (y0, x0, hh, hw)).  Returns (labels_b [B] = labels reversed, lam [B]): the ``soft`` inputs of
    classifier_train_step beside ``labels``."""
    images = _need(images, torch.float32, "images")
    if images.dim() != 4 or images.shape[1] != 3 or not images.is_contiguous():
        raise ValueError(f"mix_batch: images must be a contiguous float32 [B,3,H,W] tensor, got {tuple(images.shape)}")
    b, _, h, w = images.shape
    labels = _need(labels, torch.int64, "labels", (b,))
    if labels_b_out is None:
        labels_b_out = torch.empty((b,), dtype=torch.int64, device=images.device)
    else:
        labels_b_out = _need(labels_b_out, torch.int64, "labels_b_out", (b,))
    if lam_out is None:
        lam_out = torch.empty((b,), dtype=torch.float32, device=images.device)
    else:
        lam_out = _need(lam_out, torch.float32, "lam_out", (b,))
    if labels_b_out.data_ptr() == labels.data_ptr():
        raise ValueError("mix_batch: labels_b_out must not be labels (a pair reads both labels and writes both)")
    y0, x0, hh, hw = (int(v) for v in box)
    _call("nnue_mix_batch", images.data_ptr(), labels.data_ptr(), b, h, w, int(mode), float(lam), y0, x0, hh, hw,
          labels_b_out.data_ptr(), lam_out.data_ptr(), _stream(images))
    return labels_b_out, lam_out
