"""ctypes binding of libdrin_hip.so (include/drin_hip.h).

This is the same stub a maintainer of the reference would add to call the library from
`drin/model.py`.  The library is loaded from the package directory
(in-tree build, `python -m drin_amd.build`); if it is missing the import of the HIP path
fails loudly - there is no CPU or PyTorch fallback in the product.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRIN_LIB_PATH: another build of the same library (the sanitizer build of `python -m drin_amd.build --asan-host`)
LIB_PATH = os.environ.get("DRIN_LIB_PATH") or os.path.join(_HERE, "libdrin_hip.so")
MAX_LAYERS = 8
ABI_VERSION = 12

OK, E_SHAPE, E_NULL, E_ALIGN, E_WORKSPACE, E_HIP, E_UNSUPPORTED, E_INDEX = 0, -1, -2, -3, -4, -5, -6, -7
TOPK_SLICE, TOPK_MAX_K = 4096, 256                                         # DRIN_TOPK_SLICE; k of the cosine top-k
POOL_AVG, POOL_MAX = 0, 1                                                  # drin_entity_pooling
ENTITY_POOLINGS = {"avg": POOL_AVG, "max": POOL_MAX}                       # common/args.py entity_final_pooling -> its id
PREC_F32, PREC_BF16X3, PREC_BF16X3_ALL, PREC_BF16X3_IF16 = 0, 1, 3, 5     # (2 and 4: removed with ABI 6 - outside the 1e-4 bar)
ROW_ACT = {"none": 0, "relu": 1, "gelu": 2}                               # drin_row_activation (drin_act_dropout_*)
FEAT_F32, FEAT_BF16 = 0, 1
CACHE_F32, CACHE_MIXED_F16 = 0, 1                                      # drin_cache_format
WIDTH_NOT_BUILT, WIDTH_TINY, WIDTH_GUARDED, WIDTH_EXACT = 0, 1, 2, 3      # drin_width_band
WIDTH_BANDS = {WIDTH_NOT_BUILT: "not-built", WIDTH_TINY: "tiny", WIDTH_GUARDED: "guarded", WIDTH_EXACT: "exact"}
# drin_width_family (the last one answers with V, the register slots of k_layernorm_gelu_bwd<V>)
WIDTH_FAMILIES = {"entity_stream": 0, "pair_rows": 1, "cache_rows": 2, "cache_pack": 3, "cached_pairs": 4, "ln_backward": 5}
CACHE_FORMATS = {"f32": CACHE_F32, "mixed_f16": CACHE_MIXED_F16}
ACTIVATIONS = {"gelu": 1, "sigmoid": 2, "relu": 3, "tanh": 4, "silu": 5}   # drin_activation

fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int64)


class DrinConfigC(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("num_candidates", C.c_int32), ("embed_dim", C.c_int32), ("image_dim", C.c_int32),
        ("mention_tokens", C.c_int32), ("image_regions", C.c_int32), ("mention_objects", C.c_int32),
        ("entity_objects", C.c_int32), ("entity_tokens", C.c_int32), ("mention_object_inner", C.c_int32),
        ("entity_image_inner", C.c_int32), ("entity_object_inner", C.c_int32), ("num_layers", C.c_int32),
        ("dynamic_edges", C.c_int32), ("edge_enabled", C.c_float * 4), ("layer_norm_eps", C.c_float),
        ("cosine_eps", C.c_float), ("miei_eps", C.c_float), ("clip_scale", C.c_float), ("precision", C.c_int32),
        ("num_entities", C.c_int32), ("vector_edges", C.c_int32), ("feature_dtype", C.c_int32),
        ("vertex_activation", C.c_int32), ("edge_activation", C.c_int32), ("cache_format", C.c_int32),
    ]


class DrinBatchC(C.Structure):
    _fields_ = [
        ("mention_text", C.c_void_p), ("mention_start", C.c_void_p), ("mention_end", C.c_void_p),
        ("mention_image", C.c_void_p), ("mention_object", C.c_void_p), ("mention_object_score", C.c_void_p),
        ("entity_text", C.c_void_p), ("entity_text_mask", C.c_void_p), ("entity_image", C.c_void_p),
        ("entity_object", C.c_void_p), ("entity_object_score", C.c_void_p), ("miet_similarity", C.c_void_p),
        ("mtei_similarity", C.c_void_p), ("entity_index", C.c_void_p), ("entity_text_cls", C.c_void_p),
        ("index_status", C.c_void_p),
    ]


class DrinLayerParamsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_h", "b_h", "w_u", "b_u", "w_v", "b_v", "ln_weight", "ln_bias", "w_m", "b_m")]


class DrinParamsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "w_mention_text", "b_mention_text", "w_entity_text", "b_entity_text",
        "w_mention_image", "b_mention_image", "w_entity_image", "b_entity_image")] + [("layer", DrinLayerParamsC * MAX_LAYERS)]


class DrinParamGradsC(C.Structure):  # same shape as DrinParamsC, mutable pointers
    _fields_ = DrinParamsC._fields_


class DrinInputGradsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "mention_text", "mention_image", "mention_object", "mention_object_score", "entity_text", "entity_text_cls",
        "entity_image", "entity_object", "entity_object_score", "miet_similarity", "mtei_similarity", "scratch")] + [
        ("scratch_bytes", C.c_size_t)]


class DrinMelhiConfigC(C.Structure):
    _fields_ = [("batch", C.c_int32), ("num_candidates", C.c_int32), ("embed_dim", C.c_int32), ("image_dim", C.c_int32),
                ("mention_tokens", C.c_int32), ("image_regions", C.c_int32), ("precision", C.c_int32),
                ("cosine_eps", C.c_float), ("thres_tmim", C.c_float), ("thres_imie", C.c_float)]


class DrinMelhiBatchC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "mention_feature", "mention_mask", "start", "end", "mention_image", "entity_feature", "entity_image")]


MELHI_PARAMS = ("w_image_map_text", "b_image_map_text", "w_ih", "w_hh", "b_ih", "b_hh", "w_mention_final_map",
                "b_mention_final_map", "w_entity_final_map", "b_entity_final_map")


class DrinMelhiParamsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MELHI_PARAMS]


class DrinMelhiParamGradsC(C.Structure):  # same shape, mutable pointers
    _fields_ = DrinMelhiParamsC._fields_


class DrinGhmfcConfigC(C.Structure):
    _fields_ = [("batch", C.c_int32), ("num_candidates", C.c_int32), ("embed_dim", C.c_int32), ("image_dim", C.c_int32),
                ("mention_tokens", C.c_int32), ("image_regions", C.c_int32), ("num_heads", C.c_int32),
                ("entity_tokens", C.c_int32), ("precision", C.c_int32), ("layer_norm_eps", C.c_float), ("cosine_eps", C.c_float)]


class DrinGhmfcBatchC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("mention_feature", "mention_mask", "mention_image", "entity_feature", "entity_mask")]


GHMFC_CROSS_PARAMS = ("a2b_wq", "a2b_wk", "a2b_wv", "a2b_in_bias", "a2b_wo", "a2b_bo", "a2b_ffn_w", "a2b_ffn_b", "b2a_in_w",
                      "b2a_in_bias", "b2a_wo", "b2a_bo", "b2a_ffn_w", "b2a_ffn_b", "ln0_w", "ln0_b", "ln1_w", "ln1_b", "ln2_w",
                      "ln2_b", "ln3_w", "ln3_b")


class DrinGhmfcCrossParamsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in GHMFC_CROSS_PARAMS]


class DrinGhmfcParamsC(C.Structure):   # the 52 state-dict tensors, in state-dict order
    _fields_ = [("t2v", DrinGhmfcCrossParamsC), ("v2t", DrinGhmfcCrossParamsC)] + [(n, C.c_void_p) for n in (
        "w_text_linear", "b_text_linear", "w_image_linear", "b_image_linear", "w_score_linear", "b_score_linear", "w_entity",
        "b_entity")]


class DrinGhmfcTableC(C.Structure):    # drin_ghmfc_table: the table form of drin_ghmfc_forward, with the struct's own size
    _fields_ = [("size", C.c_size_t), ("text", C.c_void_p), ("mask", C.c_void_p), ("num_entities", C.c_int64),
                ("entity_tokens", C.c_int32), ("candidates", C.c_void_p), ("index_status", C.c_void_p), ("rows", C.c_void_p)]


class DrinTopkTermC(C.Structure):     # drin_topk_term: one cosine of drin_table_topk_sum's sum
    _fields_ = [("x", C.c_void_p), ("rows", C.c_void_p), ("row_inv_norms", C.c_void_p), ("width", C.c_int32), ("weight", C.c_float)]


TOPK_MAX_TERMS = 4                                                         # DRIN_TOPK_MAX_TERMS
TOPK_COSINE, TOPK_RATIO = 0, 1                                             # drin_topk_form.form


class DrinTopkFormC(C.Structure):     # drin_topk_form: the form of one term of drin_table_topk_sum_forms' sum
    _fields_ = [("form", C.c_int32), ("x_mass", C.c_void_p), ("row_mass", C.c_void_p), ("eps", C.c_float)]


class DrinGemmRouteC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("launches", "family", "bm", "bn", "w_planes", "a_lo", "f16", "persist", "indexed", "accumulate",
                                         "ksplit", "splits")] + [(n, C.c_int64) for n in ("tiles", "whole_tiles", "tile0", "work_items")]


class DrinGemmProbeArgsC(C.Structure):   # drin_gemm_probe: a test and tuning entry, no stability promise beyond struct_size
    _fields_ = [("struct_size", C.c_size_t), ("op", C.c_int32), ("precision", C.c_int32), ("accumulate", C.c_int32),
                ("row_tile_wgs", C.c_int32), ("row_tile_begin", C.c_int64), ("row_tile_end", C.c_int64), ("a", C.c_void_p),
                ("a_lo", C.c_void_p), ("lda", C.c_int64), ("b", C.c_void_p), ("b_hi", C.c_void_p), ("b_lo", C.c_void_p),
                ("ldb", C.c_int64), ("bias", C.c_void_p), ("y", C.c_void_p), ("ldy", C.c_int64), ("rows", C.c_int64),
                ("n_out", C.c_int32), ("k", C.c_int32), ("scratch", C.c_void_p), ("scratch_floats", C.c_size_t),
                ("a_index", C.c_void_p), ("row_scale", C.c_void_p), ("b_scale", C.c_void_p), ("route", DrinGemmRouteC)]


class DrinWgradProductC(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("lddy", C.c_int64), ("x", C.c_void_p), ("ldx", C.c_int64), ("x_index", C.c_void_p), ("dw", C.c_void_p),
                ("lddw", C.c_int64), ("db", C.c_void_p), ("rows", C.c_int64), ("n_out", C.c_int32), ("k", C.c_int32)]


class DrinWgradProductRouteC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kernel", "slices", "in_place", "db_rode", "db_slices", "launch")] + [("rows_per_slice", C.c_int64)]


WGRAD_PROBE_MAX, WGRAD_ROUTE_LAUNCHES = 16, 8


class DrinWgradRouteC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("gemm_launches", "colsum_launches", "sum_launches", "reduce_launches", "sum_dsts", "sum_segs",
                                         "nn_family", "nn_bm", "nn_bn", "nn_splits", "nn_wt_form", "nn_accumulate")] + [
        ("grid", C.c_int64 * WGRAD_ROUTE_LAUNCHES), ("product", DrinWgradProductRouteC * WGRAD_PROBE_MAX)]


class DrinWgradProbeArgsC(C.Structure):   # drin_wgrad_probe: a test and tuning entry, no stability promise beyond struct_size
    _fields_ = [("struct_size", C.c_size_t), ("op", C.c_int32), ("precision", C.c_int32), ("staged", C.c_int32), ("n_products", C.c_int32),
                ("layers_done_after", C.c_int32), ("accumulate", C.c_int32), ("wt_form", C.c_int32), ("reserved", C.c_int32),
                ("scratch", C.c_void_p), ("scratch_floats", C.c_size_t), ("wt", C.c_void_p), ("wt_floats", C.c_size_t),
                ("product", DrinWgradProductC * WGRAD_PROBE_MAX), ("route", DrinWgradRouteC)]


WGRAD_TN_GROUP, WGRAD_TN_F32_GROUP, WGRAD_TN, WGRAD_COLSUM_BATCH, WGRAD_PASS, WGRAD_NN = range(1, 7)
WGRAD_KERNEL = {0: "none", 1: "tn_bf16x3", 2: "tn_f32_small", 3: "tn_f32_large"}
WGRAD_WT_NONE, WGRAD_WT_F32_SCRATCH, WGRAD_WT_PLANES = range(3)
PROBE_GEMM_NT, PROBE_GEMM_NT_BF16X3, PROBE_GEMM_NT_BF16X3_P4, PROBE_GEMM_X3_PLANES, PROBE_GEMM_F16_PLANES, PROBE_TO_F16_SCALED = range(1, 7)
GEMM_FAMILY = {0: "none", 1: "bf16x3", 2: "bf16x3_p4", 3: "planes", 4: "planes_p4", 5: "f32", 6: "f32_gemv"}


MENTION_LINEAR, MENTION_ROWS = 0, 1                                    # drin_mention_encoder
REPR_AVG_EXTRACT, REPR_MAX_POOL = 0, 1                                 # drin_mention_repr
MENTION_REPR = {"avg extract": REPR_AVG_EXTRACT, "max pool": REPR_MAX_POOL}   # common/args.py:29's spellings


class DrinMentionHeadC(C.Structure):     # drin_mention_head: the settings of the *_head entry points, with the struct's own size
    _fields_ = [("struct_size", C.c_size_t), ("encoder", C.c_int32), ("representation", C.c_int32), ("encoded", C.c_void_p),
                ("max_index", C.c_void_p), ("grad_encoded", C.c_void_p)]


class DrinTraceC(C.Structure):
    _fields_ = [(n, C.c_void_p * (MAX_LAYERS + 1)) for n in (
        "mention_text_vertex", "mention_image_vertex", "entity_text_vertex", "entity_image_vertex", "edges")]


EXPORTS = {
    # name: (restype, argtypes)
    "drin_version": (C.c_int, []),
    "drin_last_error": (C.c_char_p, []),
    "drin_build_info": (C.c_char_p, []),
    "drin_default_config": (C.c_int, [C.POINTER(DrinConfigC)]),
    "drin_host_selftest": (C.c_int, []),
    "drin_workspace_bytes": (C.c_size_t, [C.POINTER(DrinConfigC), C.c_int]),
    "drin_edges_fwd": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_pool_fwd": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_linear_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_linear_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "drin_forward": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                               C.c_size_t, C.c_void_p, C.c_int, C.POINTER(DrinTraceC), C.c_void_p]),
    "drin_forward_staged": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_int, C.POINTER(DrinTraceC), C.c_void_p, C.c_void_p]),
    "drin_backward": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                C.c_size_t, C.c_void_p, C.POINTER(DrinParamGradsC), C.c_void_p]),
    "drin_backward_staged": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.POINTER(DrinParamGradsC), C.c_void_p, C.c_void_p]),
    "drin_backward_ex": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.POINTER(DrinParamGradsC), C.POINTER(DrinInputGradsC), C.c_void_p,
                                   C.c_void_p]),
    "drin_input_grad_scratch_bytes": (C.c_size_t, [C.POINTER(DrinConfigC)]),
    "drin_pool_bwd": (C.c_int, [C.POINTER(DrinConfigC), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_fused_supported": (C.c_int, [C.POINTER(DrinConfigC)]),
    "drin_indexed_supported": (C.c_int, [C.POINTER(DrinConfigC)]),
    "drin_width_class": (C.c_int, [C.POINTER(DrinConfigC), C.c_int]),
    "drin_prepared_bytes": (C.c_size_t, [C.POINTER(DrinConfigC)]),
    "drin_fused_workspace_bytes": (C.c_size_t, [C.POINTER(DrinConfigC)]),
    "drin_workgroups_per_mention": (C.c_int32, [C.POINTER(DrinConfigC), C.c_int32]),
    "drin_index_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "drin_image_contraction_passes": (C.c_int32, [C.POINTER(DrinConfigC), C.c_int32]),
    "drin_image_contraction_side_tiles": (C.c_int32, [C.POINTER(DrinConfigC), C.c_int32]),
    "drin_prepare": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinParamsC), C.c_void_p, C.c_size_t, C.c_void_p]),
    "drin_forward_prepared": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "drin_entity_cache_bytes": (C.c_size_t, [C.POINTER(DrinConfigC)]),
    "drin_entity_cache_build_workspace_bytes": (C.c_size_t, [C.POINTER(DrinConfigC)]),
    "drin_cached_workspace_bytes": (C.c_size_t, [C.POINTER(DrinConfigC)]),
    "drin_build_entity_cache": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "drin_forward_cached": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "drin_split_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "drin_linear_planes_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_gemm_probe": (C.c_int, [C.POINTER(DrinGemmProbeArgsC), C.c_void_p]),
    "drin_wgrad_probe": (C.c_int, [C.POINTER(DrinWgradProbeArgsC), C.c_void_p]),
    "drin_loss_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "drin_triplet_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_int32), C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "drin_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "drin_melhi_workspace_bytes": (C.c_size_t, [C.POINTER(DrinMelhiConfigC), C.c_int]),
    "drin_melhi_forward": (C.c_int, [C.POINTER(DrinMelhiConfigC), C.POINTER(DrinMelhiBatchC), C.POINTER(DrinMelhiParamsC), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "drin_melhi_backward": (C.c_int, [C.POINTER(DrinMelhiConfigC), C.POINTER(DrinMelhiBatchC), C.POINTER(DrinMelhiParamsC),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(DrinMelhiParamGradsC),
                                      C.c_void_p]),
    "drin_ghmfc_workspace_bytes": (C.c_size_t, [C.POINTER(DrinGhmfcConfigC)]),
    "drin_ghmfc_forward": (C.c_int, [C.POINTER(DrinGhmfcConfigC), C.POINTER(DrinGhmfcBatchC), C.POINTER(DrinGhmfcParamsC), C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_ghmfc_table_workspace_bytes": (C.c_size_t, [C.POINTER(DrinGhmfcConfigC), C.POINTER(DrinGhmfcTableC)]),
    "drin_ghmfc_forward_table": (C.c_int, [C.POINTER(DrinGhmfcConfigC), C.POINTER(DrinGhmfcBatchC), C.POINTER(DrinGhmfcParamsC),
                                           C.POINTER(DrinGhmfcTableC), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_ghmfc_entity_rows_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    # (text, mask, num_entities, entity_tokens, width, w_entity, b_entity, precision, rows, workspace, workspace_bytes, stream)
    "drin_ghmfc_entity_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # (text, mask, num_entities, entity_tokens, width, pooling, w_entity, b_entity, precision, rows, workspace, workspace_bytes, stream)
    "drin_ghmfc_entity_rows_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # the token pool with a pooling (POOL_AVG / POOL_MAX): (feat, mask, out, pairs, tokens, width, pooling, stream),
    # (text, mask, index, num_entities, out, pairs, tokens, width, pooling, index_status, stream)
    "drin_entity_token_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_entity_token_pool_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    # the indexed row operations: (table, index, num_entities, out, count, width, index_status, stream),
    # (text, mask, index, num_entities, out, pairs, tokens, width, index_status, stream),
    # (x, rows, index, num_entities, out, batch, num_candidates, width, eps, index_status, stream)
    "drin_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "drin_entity_token_mean_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p]),
    "drin_cosine_rows_indexed_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    # cosine top-k against the whole table: (rows, num_entities, width, eps, out, stream),
    # (block, ld, batch, cols, col_base, col_inv_norms, k, state_keys, state_rows, scratch, scratch_bytes, first, out_keys, out_rows, stream),
    # (batch, num_entities, width, k, chunk_entities),
    # (x, rows, row_inv_norms, num_entities, batch, width, k, cosine_eps, precision, chunk_entities, workspace, workspace_bytes,
    #  out_scores, out_rows, stream)
    "drin_row_inv_norms": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "drin_topk_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_table_topk_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64]),
    "drin_table_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                  C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # a sum of cosines against the tables (csrc/table_topk.hip):
    # (blocks, col_inv_norms, row_scales, weights, num_terms, ld, batch, cols, out, stream),
    # (terms, num_terms, batch, num_entities, k, chunk_entities),
    # (terms, num_terms, num_entities, batch, k, cosine_eps, precision, chunk_entities, workspace, workspace_bytes, out_scores, out_rows,
    #  stream)
    "drin_topk_combine": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.c_int32,
                                    C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "drin_table_topk_sum_workspace_bytes": (C.c_size_t, [C.POINTER(DrinTopkTermC), C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64]),
    "drin_table_topk_sum": (C.c_int, [C.POINTER(DrinTopkTermC), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int64,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # DRIN behind a first stage (csrc/cross_edges.hip, csrc/table_topk.hip):
    # (mention_clip_image, mention_clip_text, table_clip_text, table_clip_image, index, num_entities, batch, num_candidates, width,
    #  scale, eps, miet, mtei, index_status, stream), (scores, rows, batch, n, k, out_scores, out_rows, out_slots, stream)
    "drin_cross_modal_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the same against table rows stored as row_dtype (FEAT_F32 | FEAT_BF16): the old argument lists with
    # row_dtype behind the rows (the cross-modal edges: behind the two tables; the sum: a host int32 array behind `terms`), the
    # two workspace queries with (row_dtype | row_dtypes, ..., precision)
    "drin_row_inv_norms_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "drin_cosine_rows_indexed_fwd_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "drin_cross_modal_edges_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_table_topk_workspace_bytes_ex": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "drin_table_topk_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                     C.c_int32, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_table_topk_sum_workspace_bytes_ex": (C.c_size_t, [C.POINTER(DrinTopkTermC), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int64,
                                                            C.c_int32, C.c_int64, C.c_int32]),
    "drin_table_topk_sum_ex": (C.c_int, [C.POINTER(DrinTopkTermC), C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float,
                                         C.c_int32, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the image-image edge as a term, the RATIO form:
    # (obj, score, dtype, n, K, width, eps, out, mass, stream),
    # (x, x_mass, rows, row_mass, index, num_entities, out, batch, num_candidates, width, eps, index_status, stream),
    # drin_topk_combine's list with `forms` behind `weights`; drin_table_topk_sum(_workspace_bytes)_ex's lists with `forms` behind `row_dtypes`
    "drin_object_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "drin_ratio_rows_indexed_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "drin_topk_combine_forms": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_float),
                                          C.POINTER(DrinTopkFormC), C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "drin_table_topk_sum_forms_workspace_bytes": (C.c_size_t, [C.POINTER(DrinTopkTermC), C.POINTER(C.c_int32), C.POINTER(DrinTopkFormC),
                                                               C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32]),
    "drin_table_topk_sum_forms": (C.c_int, [C.POINTER(DrinTopkTermC), C.POINTER(C.c_int32), C.POINTER(DrinTopkFormC), C.c_int32, C.c_int64,
                                            C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "drin_rank_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drin_ghmfc_mention_forward_workspace_bytes": (C.c_size_t, [C.POINTER(DrinGhmfcConfigC)]),
    "drin_ghmfc_mention_forward": (C.c_int, [C.POINTER(DrinGhmfcConfigC), C.POINTER(DrinGhmfcBatchC), C.POINTER(DrinGhmfcParamsC), C.c_void_p,
                                             C.c_size_t, C.c_void_p, C.c_void_p]),
    "drin_attention": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_attention_train_fwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_attention_bwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p]),
    # (p, seed, call) follow the undropped entry points' arguments, ahead of the stream
    "drin_attention_dropout_fwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                             C.c_uint64, C.c_uint64, C.c_void_p]),
    "drin_attention_dropout_bwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_float, C.c_uint64, C.c_uint64, C.c_void_p]),
    "drin_attention_dropout_keep": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    # the matrix-core attention core (csrc/attention_mfma.hip): the dropout entry points' argument lists, p = 0 = no dropout
    "drin_attention_mfma_fwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                          C.c_uint64, C.c_uint64, C.c_void_p]),
    "drin_attention_mfma_bwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_float, C.c_uint64, C.c_uint64, C.c_void_p]),
    "drin_layernorm_res_train_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "drin_layernorm_res_bwd_scratch_floats": (C.c_size_t, [C.c_int64, C.c_int32]),
    "drin_layernorm_res_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_void_p]),
    "drin_seq_max_train_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_seq_max_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_gate_mix_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_gate_mix_bwd_scratch_floats": (C.c_size_t, [C.c_int32, C.c_int32]),
    "drin_gate_mix_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_cosine_rows_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "drin_cosine_rows_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "drin_entity_token_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_act_dropout_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_uint64,
                                       C.c_void_p]),
    "drin_act_dropout_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_uint64,
                                       C.c_uint64, C.c_void_p]),
    "drin_span_mean_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_span_mean_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_forward_staged_head": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_int, C.POINTER(DrinTraceC), C.c_void_p,
                                           C.POINTER(DrinMentionHeadC), C.c_void_p]),
    "drin_backward_head": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.POINTER(DrinParamGradsC), C.POINTER(DrinInputGradsC), C.c_void_p,
                                     C.POINTER(DrinMentionHeadC), C.c_void_p]),
    "drin_forward_prepared_head": (C.c_int, [C.POINTER(DrinConfigC), C.POINTER(DrinBatchC), C.POINTER(DrinParamsC), C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(DrinMentionHeadC), C.c_void_p]),
    # (raw, raw_dtype, encoded, start, end, representation, edge_row, vertex_row, max_index, batch, seq_len, width, stream)
    "drin_mention_rows_fwd": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    # (g_edge_row, g_vertex_row, start, end, max_index, representation, has_encoded, grad_raw, grad_encoded, batch, seq_len, width, stream)
    "drin_mention_rows_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    # gradient x input attribution (csrc/attribution_kernels.hip):
    # (tokens, token_dtype, mask, entity_index, num_entities, index_status, grad_pooled, out, pairs, T, width, stream),
    # (x, x_dtype, g, out, rows, width, stream)
    "drin_token_attribution": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "drin_rows_dot": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "drin_profile_begin": (C.c_int, [C.c_int]),
    "drin_profile_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "drin_kernel_class_name": (C.c_char_p, [C.c_int]),
}
KERNEL_CLASSES = 12


class DrinError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libdrin_hip status {status}: {message}")
        self.status = status


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every entry point of include/drin_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the DRIN HIP path has no fallback. Build it with `python -m drin_amd.build`."
        )
    # The library works on PyTorch's device pointers and streams, so it must run on the HIP runtime PyTorch runs on: torch
    # ships its own libamdhip64 and the library needs "libamdhip64.so.7" - whichever is in the process first serves both.
    # Loaded before torch, the library pulls /opt/rocm's copy in, torch then brings its own, and the library's calls fail
    # with "no ROCm-capable device is detected" (seen: __graft_entry__.build() followed by smoke() in one process).
    try:
        import torch  # noqa: F401
    except ImportError:  # a torch-free caller (examples/score_c_abi.cpp has no Python at all): the system runtime alone
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.drin_version() != ABI_VERSION:
        raise ImportError(f"libdrin_hip ABI {lib.drin_version()} != binding {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def profile_begin(max_launches: int = 65536) -> None:
    check(load().drin_profile_begin(max_launches))


def profile_end() -> dict:
    """{class name: (gpu milliseconds, launches)} since profile_begin (launches from every thread)."""
    ms = (C.c_double * KERNEL_CLASSES)()
    n = (C.c_int64 * KERNEL_CLASSES)()
    check(load().drin_profile_end(ms, n))
    lib = load()
    return {lib.drin_kernel_class_name(k).decode(): (ms[k], n[k]) for k in range(KERNEL_CLASSES)}


def check(status: int) -> None:
    if status != OK:
        raise DrinError(status, load().drin_last_error().decode())


# ---- what every torch caller of the entry points needs -------------------------------------------------------------
def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device) -> C.c_void_p:
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _scratch(pool: dict, device, stream_id: int, floats: int):
    """A float32 scratch buffer of `pool` (one dictionary per purpose: buffers of different pools never alias), one per
    (device, stream) and grown to the largest need seen: calls on one stream run in order, so they share it."""
    import torch
    buf = pool.get((device, stream_id))
    if buf is None or buf.numel() < floats:
        buf = pool[(device, stream_id)] = torch.empty(max(floats, 1), dtype=torch.float32, device=device)
    return buf
