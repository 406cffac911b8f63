"""ctypes binding of libp2w_gfx950.so (C ABI: include/p2w.h).

The library is the product path: there is no CPU or eager-PyTorch fallback, so a
missing library is a hard error naming the build command.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libp2w_gfx950.so")

_vp, _i32, _f32, _sz = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


class Epilogue(C.Structure):
    _fields_ = [("bias", _vp), ("sc0", _vp), ("sh0", _vp), ("sc1", _vp), ("sh1", _vp), ("residual", _vp),
                ("ldr", _i32), ("relu0", _i32), ("relu1", _i32), ("relu2", _i32), ("relu_final", _i32), ("range", _vp),
                ("interp", _vp), ("interp_rows", _i32)]


class BnStage(C.Structure):                                     # include/p2w.h p2w_bn_stage
    _fields_ = [("dw_w", _vp), ("dw_b", _vp), ("gamma", _vp), ("beta", _vp), ("running_mean", _vp), ("running_var", _vp),
                ("momentum", C.c_double), ("eps", C.c_double), ("relu", _i32)]


class OptimTensor(C.Structure):                                 # include/p2w.h p2w_optim_tensor (a HOST array of device pointers)
    _fields_ = [("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("n", C.c_int64)]


class OptimHyper(C.Structure):                                  # include/p2w.h p2w_optim_hyper
    _fields_ = [(k, C.c_double) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm", "growth_factor", "backoff_factor")] + \
               [("growth_interval", _i32), ("scaling", _i32)]


class OptimState(C.Structure):                                  # include/p2w.h p2w_optim_state (the 80-byte DEVICE record)
    _fields_ = [("sumsq", C.c_double), ("norm", _f32), ("coef", _f32), ("inv_scale", _f32), ("scale", _f32), ("found_inf", _i32),
                ("growth_tracker", _i32), ("t", C.c_int64), ("skipped", C.c_int64), ("decay", _f32), ("omb1", _f32), ("beta2", _f32),
                ("omb2", _f32), ("step_size", _f32), ("rsb2", _f32), ("eps", _f32), ("reserved", _i32)]


# name -> (restype, argtypes); must list every symbol declared in include/p2w.h
SEARCH_X_INDEX_IN_W, SEARCH_Q_ROW_IN_W, SEARCH_BOX = 1, 2, 4   # include/p2w.h P2W_SEARCH_*
PREC_F16X3, PREC_F16, PREC_BF16 = 0, 1, 2                      # include/p2w.h P2W_PREC_*
PREC_OF = {"f16x3": PREC_F16X3, "fp16": PREC_F16, "bf16": PREC_BF16}
GEMM_TILE_128, GEMM_TILE_256, GEMM_GENERIC_EPI, GEMM_ORDER_ROWS, GEMM_ORDER_COLS, GEMM_RESIDUAL_H = 1, 2, 4, 8, 16, 32   # P2W_GEMM_*
GEMM_STREAMK, GEMM_NO_STREAMK = 64, 128
SA_ITEM_256, SA_ITEM_128, SA_PACK8 = 1, 2, 4                                                       # P2W_SA_*
CLUSTER_LINK, CLUSTER_COMPRESS, CLUSTER_NUMBER, CLUSTER_ALL = 1, 2, 4, 7                           # P2W_CLUSTER_*
MAX_K_WIDE = 100                                                                                   # P2W_MAX_K_WIDE
EVAL_CHUNK, EVAL_MAX_CLASSES = 4096, 8                                                             # P2W_EVAL_*
LOSS_CHUNK = 4096                                                                                  # P2W_LOSS_CHUNK
EDGE_CHUNK = 1024                                                                                  # P2W_EDGE_CHUNK
BN_GROUP = 16                                                                                      # P2W_BN_GROUP
BN_CHAIN_MAX, BN_CHAIN_ROWS = 3, 32                                                                # P2W_BN_CHAIN_*
FEED_CHUNK, FEED_STREAM = 256, 0x50325746                                                          # P2W_FEED_*
SAMPLE_STREAM, SAMPLE_TILE, SAMPLE_N_MAX = 0x50325753, 1024, 1 << 24                               # P2W_SAMPLE_*
CAP_STREAM, CAP_N_MAX, CAP_S_MAX, CAP_OUT_MAX = 0x50325743, 1 << 30, 1 << 20, 1 << 38                  # P2W_CAP_*
OPTIM_CHUNK, OPTIM_GROUP, OPTIM_MAX_TENSORS = 4096, 32, 4096                                       # P2W_OPTIM_*
F32, F16, BF16 = 0, 1, 2                                                                           # P2W_F32, P2W_F16, P2W_BF16

SIGNATURES = {
    "p2w_version": (_i32, []),
    "p2w_strerror": (C.c_char_p, [_i32]),
    "p2w_pack_xyzr": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "p2w_voxel_sample_ws_bytes": (_sz, [_i32]),
    "p2w_voxel_sample": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_voxel_sample_table_ws_bytes": (_sz, [_i32, C.c_int64]),
    "p2w_voxel_sample_table": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64,
                                      _vp, _sz, _vp]),
    "p2w_voxel_sample_table_prepare": (_i32, [_vp, _sz, _vp]),
    "p2w_voxel_sample_table_prepared": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64,
                                               _vp, _sz, _vp]),
    "p2w_knn_grid_indexed": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "p2w_ball_query_grid_indexed": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.c_double, _i32, _vp, _vp, _i32, _vp]),
    "p2w_knn_hint2": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "p2w_knn_grid": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "p2w_ball_query_grid": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.c_double, _i32, _vp, _vp, _i32, _vp]),
    "p2w_index_records": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "p2w_voxel_grid": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "p2w_consecutive_cluster": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_level_gather": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "p2w_ball_query": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, C.c_double, _i32, _vp, _vp, _vp, _i32, _vp]),
    "p2w_knn": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "p2w_morton_order_ws_bytes": (_sz, [_i32]),
    "p2w_morton_order": (_i32, [_vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_cells_nd": (_i32, [_vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "p2w_sort_pairs_u64_ws_bytes": (_sz, [_i32]),
    "p2w_sort_pairs_u64": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "p2w_key_runs_ws_bytes": (_sz, [_i32]),
    "p2w_key_runs": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_knn_refine_f64": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "p2w_cell_starts_ws_bytes": (_sz, [C.c_int64]),
    "p2w_cell_starts": (_i32, [_vp, _i32, C.c_int64, _vp, _vp, _sz, _vp]),
    "p2w_vote": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _f32, _vp, _vp, _vp]),
    "p2w_euclid_cluster_ws_bytes": (_sz, [C.c_int64]),
    "p2w_euclid_cluster": (_i32, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_double, C.c_int64, C.c_int64, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_knn_wide_f64": (_i32, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _i32, C.c_double, _vp, _vp]),
    "p2w_pathlen_grow_ws_bytes": (_sz, [C.c_int64]),
    "p2w_pathlen_grow": (_i32, [_vp, _vp, C.c_int64, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp, C.c_int64, _vp, _vp,
                                _vp, _sz, _vp]),
    "p2w_pathlen_sssp_ws_bytes": (_sz, [C.c_int64, C.c_int64]),
    "p2w_pathlen_sssp": (_i32, [_vp, _vp, C.c_int64, C.c_int64, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_pathlen_weights": (_i32, [_vp, _vp, C.c_int64, _vp, _vp]),
    "p2w_confusion_ws_bytes": (_sz, [C.c_int64, _i32, _i32]),
    "p2w_confusion": (_i32, [_vp, _vp, _vp, _vp, C.c_int64, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_poly1_focal_ws_bytes": (_sz, [C.c_int64]),
    "p2w_poly1_focal": (_i32, [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp,
                               _vp, _sz, _vp]),
    "p2w_train_feed_ws_size": (_sz, [C.c_int64, _i32]),
    "p2w_train_feed": (_i32, [_vp, _vp, _vp, C.c_int64, _i32, _vp, _vp, _i32, C.c_int64, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_random_subset_ws_size": (_sz, [C.c_int64]),
    "p2w_random_subset": (_i32, [C.c_int64, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_cap_subset_ws_size": (_sz, [C.c_int64, C.c_int64]),
    "p2w_cap_subset": (_i32, [C.c_int64, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp,
                              _sz, _vp]),
    "p2w_clip_adamw_ws_size": (_sz, [_vp, _i32]),
    "p2w_clip_adamw": (_i32, [C.POINTER(OptimTensor), _i32, C.POINTER(OptimHyper), _vp, _vp, _sz, _vp]),
    "p2w_tile_bbox": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "p2w_tile_bbox_count": (_i32, [_i32, _i32]),
    "p2w_stem": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "p2w_packed_dims": (None, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "p2w_gemm": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, C.POINTER(Epilogue), _vp, _i32, _vp]),
    "p2w_sa_conv": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp,
                           _vp, _i32, _vp]),
    "p2w_packed_dims_h": (_i32, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "p2w_gemm_h2": (_i32, [_i32, _vp, _i32, _vp, _f32, _i32, _i32, _i32, C.POINTER(Epilogue), _vp, _i32, _vp, _i32, _i32, _vp]),
    "p2w_gemm_h2_sk_ws_bytes": (_sz, []),
    "p2w_gemm_h2_sk": (_i32, [_i32, _vp, _i32, _vp, _f32, _i32, _i32, _i32, C.POINTER(Epilogue), _vp, _i32, _vp, _i32, _vp, _sz, _i32, _vp]),
    "p2w_gemm_h2_rowdot_ws_bytes": (_sz, [_i32, _i32]),
    "p2w_gemm_h2_rowdot": (_i32, [_i32, _vp, _i32, _vp, _f32, _i32, _i32, _i32, C.POINTER(Epilogue), _vp, _f32, _vp, _vp, _sz, _i32, _vp]),
    "p2w_sa_conv_h_ws_bytes": (_sz, [_i32, _i32]),
    "p2w_sa_conv_h": (_i32, [_i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _f32, _i32, _i32, _vp, _vp,
                             _vp, _vp, _i32, _vp, _i32, _vp, _sz, _i32, _vp]),
    "p2w_stem_h2": (_i32, [_i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "p2w_stem_h2_indexed": (_i32, [_i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "p2w_sa_conv_h_rows": (_i32, [_i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _f32, _i32, _i32, _vp, _vp,
                                  _vp, _vp, _i32, _vp, _i32, _vp, _sz, _i32, _vp, _vp, _vp]),
    "p2w_interp_concat_h2": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp]),
    "p2w_interp_weights": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "p2w_concat_xyz_h2": (_i32, [_i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp]),
    "p2w_interp_concat": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp]),
    "p2w_concat_xyz": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _vp]),
    "p2w_segment_max": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _vp]),
    "p2w_rowdot": (_i32, [_vp, _i32, _i32, _vp, _f32, _i32, _vp, _vp]),
    "p2w_fill_batch_nbr": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "p2w_segment_max_arg": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "p2w_segment_max_bwd": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp]),
    "p2w_interp_bwd_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "p2w_interp_bwd": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _sz, _vp]),
    "p2w_edge_l1": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "p2w_edge_l1_bwd_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "p2w_edge_l1_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_relu_bn_max_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "p2w_relu_bn_max": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                               _vp]),
    "p2w_relu_bn_max_bwd": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_chain_ws_size": (_sz, [_i32, _i32, _i32]),
    "p2w_bn_chain": (_i32, [_vp, _i32, _vp, _i32, C.POINTER(BnStage), _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_chain_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, C.POINTER(BnStage), _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp,
                                _vp, _vp, _vp, _sz, _vp]),
    "p2w_relu_bn_ws_size": (_sz, [_i32, _i32]),
    "p2w_relu_bn": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_relu_bn_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_interp_add_relu": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "p2w_interp_add_relu_bwd_ws_size": (_sz, [_i32, _i32, _i32]),
    "p2w_interp_add_relu_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _sz, _vp]),
    "p2w_bn_relu_rowdot_ws_size": (_sz, [_i32, _i32]),
    "p2w_bn_relu_rowdot": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_relu_rowdot_bwd": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_chain_io": (_i32, [_vp, _i32, _i32, _vp, _i32, C.POINTER(BnStage), _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_chain_bwd_io": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, C.POINTER(BnStage), _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp,
                                   _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_relu_bn_io": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz,
                              _vp]),
    "p2w_relu_bn_bwd_io": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_relu_rowdot_io": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp,
                                     _sz, _vp]),
    "p2w_bn_relu_rowdot_bwd_io": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz,
                                         _vp]),
    "p2w_segment_max_arg_io": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "p2w_segment_max_bwd_io": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "p2w_relu_bn_max_io": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _sz, _vp]),
    "p2w_relu_bn_max_bwd_io": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz,
                                      _vp]),
    "p2w_edge_l1_io": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp]),
    "p2w_edge_l1_bwd_io": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "p2w_bn_relu_rowdot_bf16": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp, _sz,
                                       _vp]),
    "p2w_bn_relu_rowdot_bwd_bf16": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "p2w_segment_max_arg_bf16": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "p2w_segment_max_bwd_bf16": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raise loudly when the library is not built."""
    global _lib
    if _lib is None:
        from . import build as _build
        if _build._stale():  # missing, or built from other sources than the ones in the tree
            try:
                _build.build()
            except Exception as e:  # no hipcc, compile error, read-only tree ...
                raise RuntimeError(
                    f"{LIB_PATH} is missing or stale and could not be rebuilt ({e}). The HIP extension is the "
                    "only compute path (no CPU fallback). Build it with `python -m pointstowood_amd.build`.") from e
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError = symbol missing from the build
            fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = lib().p2w_strerror(code).decode()
        raise RuntimeError(f"{what or 'p2w'} failed: {msg} (code {code})")


def ws_bytes(name: str, *args) -> int:
    """Workspace size of entry point ``name``: ``p2w_<name>_ws_bytes`` or, where the header calls the query that, ``p2w_<name>_ws_size``
    (no entry point has both); 0 is the library's answer to sizes it refuses."""
    symbol = f"p2w_{name}_ws_bytes"
    if symbol not in SIGNATURES:
        symbol = f"p2w_{name}_ws_size"
    need = int(getattr(lib(), symbol)(*args))
    if need == 0:
        raise RuntimeError(f"{symbol}({', '.join(map(str, args))}) failed")
    return need


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """Raw handle of torch's current HIP stream.  Through torch._C directly when it is there: ``torch.cuda.current_stream()``
    builds a Stream object behind several device-index lookups (8 us per call, 0.45 ms of host time per forward - a third of it;
    small batches are paced by the host)."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def stage_timer(on: bool):
    """(mark, ms) of a ``stats=`` run: ``mark()`` records an event on the current stream (nothing when ``on`` is false), ``ms()``
    waits for the last one and returns the GPU milliseconds between consecutive marks."""
    events = []

    def mark():
        if on:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()

    def ms():
        events[-1].synchronize()
        return [a.elapsed_time(b) for a, b in zip(events[:-1], events[1:])]
    return mark, ms


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("pointstowood_amd operators need tensors on an MI355X (cuda) device; "
                               "there is no CPU fallback")


def aligned16(t):
    """Kernels that read 16 bytes at a time need their arrays on a 16-byte boundary: a view that starts inside its storage
    (``x[1:]``) is copied."""
    return t.clone() if t.data_ptr() % 16 else t


def packed_dims(n: int, k: int, prec: int | None = None):
    """(N_pad, K_pad) of a packed weight: fp32 / f16x3 pad K to 32, the single-plane H precisions to 64."""
    a, b = _i32(), _i32()
    if prec is None:
        lib().p2w_packed_dims(n, k, C.byref(a), C.byref(b))
    else:
        check(lib().p2w_packed_dims_h(prec, n, k, C.byref(a), C.byref(b)), "p2w_packed_dims_h")
    return a.value, b.value
