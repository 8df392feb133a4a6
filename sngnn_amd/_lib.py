"""ctypes binding of ``libsngnn_hip.so`` (the C ABI declared in include/sngnn_hip.h).

The product path has NO fallback: if the shared library is missing or a call
fails, an exception is raised.  (The CPU oracle under ``oracle/`` is test
infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os

import torch
from torch import Tensor

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SNGNN_LIB_PATH: an experimental build of the same library for an A/B measurement; the product is the in-tree file)
LIB_PATH = os.environ.get("SNGNN_LIB_PATH") or os.path.join(_HERE, "libsngnn_hip.so")

OK, EINVAL, ERANGE, EHIP, ENOMEM = 0, -1, -2, -3, -4
DTYPE_F16, DTYPE_BF16 = 1, 2          # SNGNN_DTYPE_*: storage types of the half path's rows
UNSELECTED = -4.0
LOOPS_REPLACE = 2      # SNGNN_LOOPS_REPLACE: drop the original loops, then append one per node
MAX_CHANNELS = 512
TWO_HOP_HASH_MAX = 1024    # SNGNN_TWO_HOP_HASH_MAX: the widest candidate bound the two-hop build keeps in an LDS table
SPARSE_COSINE_HASH_MAX = 2048    # SNGNN_SPARSE_COSINE_HASH_MAX: the same bound for the sparse cosine's LDS tables

_vp, _i64, _i32, _f32, _f64 = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double

# name -> (restype, argtypes); mirrors include/sngnn_hip.h one to one
SIGNATURES = {
    "sngnn_last_error": (C.c_char_p, []), "sngnn_build_info": (C.c_char_p, []),
    "sngnn_graph_create": (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, C.POINTER(_vp)]),
    "sngnn_graph_create_partition": (_i32, [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, C.POINTER(_vp)]),
    "sngnn_graph_destroy": (None, [_vp]),
    "sngnn_graph_num_nodes": (_i64, [_vp]), "sngnn_graph_num_total_nodes": (_i64, [_vp]),
    "sngnn_graph_row_offset": (_i64, [_vp]), "sngnn_graph_num_edges": (_i64, [_vp]),
    "sngnn_graph_max_in_degree": (_i64, [_vp]), "sngnn_graph_src_min": (_i64, [_vp]),
    "sngnn_graph_num_fused_nodes": (_i64, [_vp]), "sngnn_graph_workspace_bytes": (_i64, [_vp, _i32]),
    "sngnn_graph_copy_array": (_i32, [_vp, _i32, _vp]),
    "sngnn_graph_array_dev": (_vp, [_vp, _i32]), "sngnn_graph_array_len": (_i64, [_vp, _i32]),
    "sngnn_agg_forward": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_normalize_rows": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp]), "sngnn_filter_row_bytes": (_i64, [_i32]),
    "sngnn_normalize_rows_filter": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_agg_forward_prepared": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_agg_forward_epilogue": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_agg_forward_prepared_epilogue": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_filter_enable": (_i32, [_i32]), "sngnn_filter_wanted": (_i32, [_vp, _i32, _i32, _f32]),
    "sngnn_agg_forward_rows": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_tuning_set": (_i32, [_i32, _i32]), "sngnn_last_forward_finalize_workgroups": (_i32, []),
    "sngnn_filter_pair_scores": (_i32, [_vp, _i32, _vp, _vp, _i64, _vp, _vp]),
    "sngnn_agg_forward_normalized": (_i32, [_vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_agg_backward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_agg_backward_topk": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_agg_kept_bits_supported": (_i32, [_vp, _i32, _i32]), "sngnn_agg_head_supported": (_i32, [_vp, _i32, _i32]),
    "sngnn_agg_head_workspace_bytes": (_i64, [_vp]), "sngnn_graph_kept_bits_bytes": (_i64, [_vp]),
    "sngnn_agg_backward_bits": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_agg_forward_half": (_i32, [_vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_agg_backward_half": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_attn_forward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_attn_backward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_signed_forward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_signed_backward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_attn_forward_half": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_attn_backward_half": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_signed_forward_half": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_signed_backward_half": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_blend_workspace_bytes": (_i64, []), "sngnn_blend_forward": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "sngnn_blend_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_blend_forward_epilogue": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "sngnn_blend_backward_epilogue": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _f32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_ggcn_transition_workspace_bytes": (_i64, []),
    "sngnn_ggcn_transition_forward": (_i32, [_vp, _vp, _vp, _vp, _f32, _i32, _i64, _vp, _vp]),
    "sngnn_ggcn_transition_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_bn_train_workspace_bytes": (_i64, [_i32]),
    "sngnn_bn_train_forward": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _f32, _vp, _f32] + [_vp] * 5),
    "sngnn_bn_train_backward": (_i32, [_vp, _vp, _vp, _i64, _i32] + [_vp] * 4 + [_f32, _vp, _f32] + [_vp] * 6),
    "sngnn_bn_post_forward": (_i32, [_vp, _i64, _i32, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _f32, _vp, _f32] + [_vp] * 5),
    "sngnn_bn_post_backward": (_i32, [_vp, _vp, _i64, _i32] + [_vp] * 5 + [_f32, _vp, _f32] + [_vp] * 5),
    "sngnn_knn_workspace_bytes": (_i64, [_i64, _i32]), "sngnn_knn_query_workspace_bytes": (_i64, [_i64, _i64, _i32]), "sngnn_knn_graph_route": (_i32, [_i64]), "sngnn_cosine_threshold_workspace_bytes": (_i64, [_i64, _i64]),
    "sngnn_knn_graph": (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]), "sngnn_knn_query": (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp]), "sngnn_knn_graph_half": (_i32, [_vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]), "sngnn_knn_query_half": (_i32, [_vp, _i64, _vp, _i32, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    "sngnn_cosine_threshold_count": (_i32, [_vp, _i64, _vp, _i64, _i64, _f32, _i64, _vp, _vp, _vp]), "sngnn_cosine_threshold_fill": (_i32, [_vp, _i64, _vp, _i64, _i64, _f32, _i64, _vp, _i64, _vp, _vp, _vp, _vp]), "sngnn_cosine_threshold_count_half": (_i32, [_vp, _i64, _vp, _i32, _i64, _i64, _f32, _i64, _vp, _vp, _vp]), "sngnn_cosine_threshold_fill_half": (_i32, [_vp, _i64, _vp, _i32, _i64, _i64, _f32, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "sngnn_gather_sum_rows": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]), "sngnn_scatter_sum_rows": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_weighted_gather_sum_rows": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]), "sngnn_weighted_scatter_sum_rows": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_pair_dot_rows": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "sngnn_prop_dinv": (_i32, [_vp, _vp, _vp]), "sngnn_prop_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "sngnn_prop_gpr_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_prop_gpr_backward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_prop_appnp": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_gat_workspace_bytes": (_i64, [_vp, _i32, _i32]), "sngnn_gat_scores": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "sngnn_gat_forward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "sngnn_gat_backward": (_i32, [_vp] * 9 + [_i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "sngnn_wrgat_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "sngnn_wrgat_forward": (_i32, [_vp, _vp, _i64, _vp, _i64] + [_vp] * 4 + [_i32, _i32, _f32, _i32] + [_vp] * 5),
    "sngnn_wrgat_backward": (_i32, [_vp] * 4 + [_i64] + [_vp] * 6 + [_i32, _i32, _f32, _i32, _vp, _i64, _vp, _i64] + [_vp] * 4),
    "sngnn_acm_workspace_bytes": (_i64, [_vp, _i32]),
    "sngnn_acm_forward": (_i32, [_vp] * 6 + [_i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_acm_backward": (_i32, [_vp] * 9 + [_i32, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_gcn2_workspace_bytes": (_i64, [_vp, _i32]),
    "sngnn_gcn2_hop": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32, _i32, _i32, _vp, _vp, _vp]),
    "sngnn_gcn2_map": (_i32, [_vp, _vp, _f32, _f32, _i64, _i32, _i32] + [_vp] * 6),
    "sngnn_gcn_workspace_bytes": (_i64, [_vp, _i32]), "sngnn_gcn_hop": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "sngnn_gcn_bias_grad": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "sngnn_two_hop_workspace_bytes": (_i64, [_vp]), "sngnn_two_hop_count": (_i32, [_vp, _vp, _vp, _vp]),
    "sngnn_two_hop_fill": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "sngnn_h2gcn_dinv": (_i32, [_vp, _vp, _vp]), "sngnn_h2gcn_workspace_bytes": (_i64, [_vp, _i32]),
    "sngnn_h2gcn_hop": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_glognn_gram_workspace_bytes": (_i64, [_i32]), "sngnn_glognn_gram": (_i32, [_vp, _vp, _f64, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_glognn_solve": (_i32, [_vp, _vp, _f64, _f64, _f64, _i32] + [_vp] * 6),
    "sngnn_glognn_solve_backward": (_i32, [_vp, _vp, _f64, _f64] + [_vp] * 4 + [_f64] * 3 + [_i32] + [_vp] * 4),
    "sngnn_glognn_workspace_bytes": (_i64, [_vp, _i32, _i32]), "sngnn_glognn_forward": (_i32, [_vp] * 5 + [_i32, _f64, _f64, _i32] + [_vp] * 4),
    "sngnn_glognn_backward": (_i32, [_vp] * 6 + [_i32, _f64, _f64, _i32] + [_vp] * 5),
    "sngnn_linkx_join_supported": (_i32, [_i32]), "sngnn_linkx_join_forward": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "sngnn_linkx_join_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_jk_max_forward": (_i32, [_vp, _i32, _i64, _i32, _vp, _vp, _vp]), "sngnn_jk_max_backward": (_i32, [_vp, _vp, _i32, _i64, _i32, _vp, _vp]),
    "sngnn_profile_enable": (_i32, [_i32]),
    "sngnn_profile_last_forward": (_i32, [C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32)]),
    "sngnn_gather_floor_workspace_bytes": (_i64, []), "sngnn_gather_floor": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "sngnn_adj_linear_forward": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]), "sngnn_adj_linear_backward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_head_workspace_bytes": (_i64, [_i64]),
    "sngnn_head_nll": (_i32, [_vp, _vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    "sngnn_head_nll2": (_i32, [_vp, _vp, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp]),
    "sngnn_head_nll_blend_supported": (_i32, [_i32]),
    "sngnn_head_nll_blend": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_linear_forward": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "sngnn_linear_forward_masked": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _f32, _vp, _vp]),
    "sngnn_epilogue_backward": (_i32, [_vp, _vp, _f32, _i64, _vp, _vp]), "sngnn_linear_normalized_supported": (_i32, [_i64, _i32, _i32]),
    "sngnn_linear_forward_normalized": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_linear_wgrad_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "sngnn_linear_wgrad": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_cosine_dense": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "sngnn_cosine_class_sums": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp]),
    "sngnn_cosine_hist_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "sngnn_cosine_hist": (_i32, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp]), "sngnn_cosine_scan_half_supported": (_i32, [_i64, _i32]), "sngnn_cosine_hist_half": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_edge_cosine": (_i32, [_vp, _i64, _i64, _vp, _i64, _vp, _vp]), "sngnn_segment_mean": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "sngnn_sparse_pair_dot": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "sngnn_sparse_cosine_count_workspace_bytes": (_i64, [_i64, _i64]), "sngnn_sparse_cosine_fill_workspace_bytes": (_i64, [_i64, _i64]),
    "sngnn_sparse_cosine_hist_workspace_bytes": (_i64, [_i64, _i64, _i32]), "sngnn_sparse_cosine_topk_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "sngnn_sparse_cosine_count": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "sngnn_sparse_cosine_fill": (_i32, [_vp] * 6 + [_i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "sngnn_sparse_cosine_hist": (_i32, [_vp] * 6 + [_i64, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _vp]), "sngnn_sparse_cosine_topk": (_i32, [_vp] * 6 + [_i64, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "sngnn_replica_unpack": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "sngnn_replica_wgrad_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "sngnn_replica_wgrad": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "sngnn_replica_head_workspace_bytes": (_i64, [_i32]),
    "sngnn_replica_head_nll": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "sngnn_replica_blend_workspace_bytes": (_i64, [_i32]),
    "sngnn_replica_blend_forward": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "sngnn_replica_blend_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
}

# the one status entry that ends in a c_void_p which is NOT the stream (a host buffer): it stays on ``check``; every
# other c_int entry whose last argument is a c_void_p takes the stream there and is entered through ``call``
STREAMLESS = ("sngnn_graph_copy_array",)


class Epilogue(C.Structure):
    """``sngnn_epilogue_t`` (include/sngnn_hip.h)."""
    _fields_ = [("bias", C.c_void_p), ("keep", C.c_void_p), ("keep_scale", C.c_float), ("relu", C.c_int),
                ("seed", C.c_void_p), ("p", C.c_float), ("kept_bits", C.c_void_p),
                ("head_y", C.c_void_p), ("head_sel", C.c_void_p), ("head_sets", C.c_int), ("head_out_mode", C.c_int),
                ("head_n_a", C.c_int64), ("head_n_b", C.c_int64), ("head_metrics", C.c_void_p),
                ("head_workspace", C.c_void_p), ("no_filter", C.c_int)]


class GcnHop(C.Structure):
    """``sngnn_gcn_hop_t`` (include/sngnn_hip.h)."""
    _fields_ = [("src", C.c_void_p), ("ld_src", C.c_int64), ("W", C.c_int), ("W0", C.c_int),
                ("dst0", C.c_void_p), ("ld0", C.c_int64), ("dst1", C.c_void_p), ("ld1", C.c_int64),
                ("pass_src", C.c_void_p), ("ld_ps", C.c_int64), ("pass_dst", C.c_void_p), ("ld_pd", C.c_int64),
                ("Wp", C.c_int), ("relu", C.c_int), ("bias", C.c_void_p), ("rm", C.c_void_p), ("invstd", C.c_void_p),
                ("gamma", C.c_void_p), ("beta_bn", C.c_void_p)]


class H2gcnHop(C.Structure):
    """``sngnn_h2gcn_hop_t`` (include/sngnn_hip.h)."""
    _fields_ = [("src", C.c_void_p), ("ld_src", C.c_int64), ("dst", C.c_void_p), ("ld_dst", C.c_int64), ("W", C.c_int),
                ("rm", C.c_void_p), ("invstd", C.c_void_p), ("gamma", C.c_void_p), ("beta_bn", C.c_void_p)]


_lib = None
_entries = {}        # name -> bound function of every entry ``call`` may enter (filled by load)


class SngnnError(RuntimeError):
    pass


def load():
    """Load the library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SngnnError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` or `make -C sngnn_amd/csrc` (there is no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
            if res is _i32 and args and args[-1] is _vp and name not in STREAMLESS:
                _entries[name] = fn
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().sngnn_last_error().decode("utf-8", "replace")
        exc = ValueError if rc in (EINVAL, ERANGE) else SngnnError
        raise exc(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device/host pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


_guard, _current_stream = torch.cuda.device, torch.cuda.current_stream


def _ordinal(device):
    """``device``'s index where it has one: handed an int, torch's device guard and stream lookup skip their
    parsing of a ``torch.device`` (about 2 us of host time each, per call)."""
    idx = getattr(device, "index", None)
    return device if idx is None else idx


def stream(device) -> int:
    return _current_stream(_ordinal(device)).cuda_stream


def _entry(name):
    load()          # (fills _entries on first use)
    if name not in _entries:
        raise SngnnError(f"{name} is not a status entry that takes the stream last")
    return _entries[name]


def call(name, device, *args):
    """Enter the stream-taking, status-returning C entry ``name`` on ``device``'s current stream: tensors go in
    as their ``data_ptr()`` (and must be contiguous - the kernels index dense rows), None and everything else
    (ints, floats, ``ctypes.byref``, graph handles) as they are; the stream is appended.  Only enqueues."""
    try:
        fn = _entries[name]
    except KeyError:
        fn = _entry(name)
    ptrs = []
    add = ptrs.append
    for a in args:
        if type(a) is Tensor or isinstance(a, Tensor):
            if not a.is_contiguous():
                raise ValueError(f"{name}: argument {len(ptrs) + 1} must be a contiguous tensor, got shape "
                                 f"{tuple(a.shape)} with strides {a.stride()}")
            a = a.data_ptr()
        add(a)
    idx = _ordinal(device)
    with _guard(idx):
        rc = fn(*ptrs, _current_stream(idx).cuda_stream)
    if rc != 0:
        check(rc, name)


_ws_cache = {}          # (purpose, device, stream) -> every buffer handed out for it, the live one last


def workspace(key, nbytes, device):
    """Grow-only scratch per (purpose, device, stream) for the entries whose ``*_workspace_bytes`` depends on the call.
    Lifetime rule: a buffer handed out once is never released while the process lives - a captured epoch launches on
    its address.  One that is outgrown stays in its slot's list, behind a new one of at least twice its size."""
    held = _ws_cache.setdefault((key, str(device), stream(device) if torch.device(device).type == "cuda" else None), [])
    if not held or held[-1].numel() < nbytes:
        held.append(torch.empty(max(int(nbytes), 256, 2 * held[-1].numel() if held else 0), dtype=torch.uint8, device=device))
    return held[-1]
