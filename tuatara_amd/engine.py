"""ctypes binding of the C ABI in include/tuatara_hip.h (libtuatara_hip.so).

Thin by design: numpy arrays in, numpy arrays / python lists out; every compute call
runs the HIP engine.  There is no CPU fallback — loading fails loudly when the shared
library is missing and ``Engine(...)`` raises when no GPU is present.
"""
from __future__ import annotations

import collections.abc
import ctypes as C
import functools
import math
import os
import sys
from typing import List, Optional, Sequence

import numpy as np

_LIBPATH = os.environ.get("TUATARA_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libtuatara_hip.so")   # (TUATARA_LIB: another build of the same ABI, for same-box A/B timing)
_lib = None

PREC_BF16, PREC_F32, PREC_F16X4 = 0, 1, 2
CROP_BOUNDING, CROP_RECTIFIED = 0, 1
ORIENT_OFF, ORIENT_FLIP, ORIENT_QUARTER = 0, 1, 2


class Config(C.Structure):
    _fields_ = [("precision", C.c_int), ("device", C.c_int), ("canvas_size", C.c_int), ("mag_ratio", C.c_float),
                ("text_threshold", C.c_float), ("link_threshold", C.c_float), ("low_text", C.c_float), ("min_area", C.c_int),
                ("strict_crops", C.c_int), ("max_components", C.c_int), ("verbose", C.c_int), ("crop_mode", C.c_int),
                ("orient", C.c_int), ("orient_page", C.c_int), ("lines", C.c_int), ("chars", C.c_int), ("blocks", C.c_int),
                ("mixed_batches", C.c_int)]


class Page(C.Structure):
    """ttr_page: one page in device memory, u8 HWC 3 channels; row_stride in bytes, 0 = 3 * w"""
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("row_stride", C.c_int)]


class Region(C.Structure):
    """ttr_region: a quad tl, tr, br, bl in image pixels on page `page`, read under set `set` (-1 = the engine's own)"""
    _fields_ = [("quad", C.c_float * 8), ("page", C.c_int32), ("set", C.c_int32)]


# every symbol include/tuatara_hip.h declares: (name, restype, argtypes)
_VP, _I, _F = C.c_void_p, C.c_int, C.c_float
_PU8, _PF, _PI = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
SYMBOLS = [
    ("ttr_config_default", None, [C.POINTER(Config)]),
    ("ttr_create", _VP, [C.c_char_p, C.POINTER(Config)]),
    ("ttr_destroy", None, [_VP]),
    ("ttr_last_error", C.c_char_p, []),
    ("ttr_version", C.c_char_p, []),
    ("ttr_image_to_data", _I, [_VP, _PU8, _I, _I, _I, C.POINTER(_VP)]),
    ("ttr_pages_to_data_dev", _I, [_VP, _VP, _I, _I, _I, C.POINTER(_VP)]),
    ("ttr_stream_push", _I, [_VP, _VP, _I, _I, _I, C.POINTER(_VP), C.POINTER(C.c_int)]),
    ("ttr_stream_flush", _I, [_VP, C.POINTER(_VP), C.POINTER(C.c_int)]),
    ("ttr_images_to_data", _I, [_VP, C.POINTER(_VP), _PI, _PI, _PI, _I, C.POINTER(_VP)]),
    ("ttr_canvas_geometry", _I, [_VP, _I, _I, _PI, _PI, _PF]),
    ("ttr_pages_to_data_dev_v", _I, [_VP, C.POINTER(Page), _I, C.POINTER(_VP)]),
    ("ttr_stream_push_v", _I, [_VP, C.POINTER(Page), _I, C.POINTER(_VP), C.POINTER(C.c_int)]),
    ("ttr_last_images_batches", _I, [_VP, _PI, _I]),
    ("ttr_resize_canvas_batch", _I, [_VP, C.POINTER(_VP), _PI, _PI, _PI, _I, _PU8, C.c_size_t, _PI, _PI, _PF]),
    ("ttr_pack_crops_batch", _I, [_VP, C.POINTER(_VP), _PI, _PI, _PI, _I, _PF, _PI, _I, _I, _I, _PU8, _PF]),
    ("ttr_dbg_canvas_geometry", _I, [_I, _I, _I, _F, _PI, _PI, _PF, _PI, _PI]),
    ("ttr_dbg_launch_groups", _I, [_I] * 13 + [_PI, _PI, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("ttr_dbg_split_layer_check", _I, [_I] * 10 + [C.c_char_p, C.c_size_t]),
    ("ttr_dbg_last_groups", _I, [_VP, _PI, _PI]),
    ("ttr_dbg_last_heat", _I, [_VP, _PF, C.c_size_t]),
    ("ttr_dbg_scratch_table", _I, [C.c_char_p, C.c_size_t]),
    ("ttr_dbg_poison_scratch", C.c_int64, [_VP, _I, _I]),
    ("ttr_result_count", _I, [_VP]),
    ("ttr_result_text", C.c_char_p, [_VP, _I]),
    ("ttr_result_bbox", _PF, [_VP, _I]),
    ("ttr_result_ids", _PI, [_VP, _I]),
    ("ttr_result_quad", _PF, [_VP, _I]),
    ("ttr_result_quads", _PF, [_VP]),
    ("ttr_result_conf", _F, [_VP, _I]),
    ("ttr_result_prob", _PF, [_VP, _I]),
    ("ttr_result_confs", _PF, [_VP]),
    ("ttr_result_probs_all", _PF, [_VP]),
    ("ttr_result_orient", _I, [_VP, _I]),
    ("ttr_result_orients", _PI, [_VP]),
    ("ttr_result_orient_candidates", _I, [_VP]),
    ("ttr_result_orient_confs", _PF, [_VP]),
    ("ttr_result_page_orient", _I, [_VP]),
    ("ttr_results_gather_orient", _I, [C.POINTER(_VP), _I, _PI, _PF, _PI]),
    ("ttr_orient_select", _I, [_PF, _PI, _I, _I, _I, _PI, _PI]),
    ("ttr_result_line_count", _I, [_VP]),
    ("ttr_result_lines", _PI, [_VP]),
    ("ttr_result_words", _PI, [_VP]),
    ("ttr_result_reading_order", _PI, [_VP]),
    ("ttr_result_line_first", _PI, [_VP]),
    ("ttr_result_line_bboxes", _PF, [_VP]),
    ("ttr_result_line_text", _I, [_VP, _I, C.c_char_p, C.c_size_t]),
    ("ttr_result_page_text", _I, [_VP, C.c_char_p, C.c_size_t]),
    ("ttr_results_gather_lines", _I, [C.POINTER(_VP), _I, _PI, _PI, _PI, _PI, _PI, _PF]),
    ("ttr_lines_from_quads", _I, [_PF, _I, _PI, _PI, _PI]),
    ("ttr_group_lines", _I, [_VP, _PF, _PI, _I, _PI, _PI, _PI]),
    ("ttr_result_char_count", _I, [_VP, _I]),
    ("ttr_result_char_first", _PI, [_VP]),
    ("ttr_result_char_quads", _PF, [_VP]),
    ("ttr_result_char_bboxes", _PF, [_VP]),
    ("ttr_result_char_cuts", _PI, [_VP]),
    ("ttr_result_char_modes", _PI, [_VP]),
    ("ttr_result_char_profiles", _PU8, [_VP]),
    ("ttr_results_gather_chars", _I, [C.POINTER(_VP), _I, _PI, _PF, _PF, _PI, _PI, _PU8]),
    ("ttr_char_cuts_from_profile", _I, [_PU8, _I, _I, _PI, _PI]),
    ("ttr_chars_from_map", _I, [_PF, _I, _I, _F, _F, _PF, _PI, _PI, _I, _PI, _PI, _PU8]),
    ("ttr_char_quads_from_cuts", _I, [_PF, _I, _PI, _I, _PF, _PF]),
    ("ttr_char_cuts", _I, [_VP, _PF, _I, _I, _F, _F, _PF, _PI, _PI, _I, _PI, _PI, _PU8]),
    ("ttr_result_block_count", _I, [_VP]),
    ("ttr_result_block_mode", _I, [_VP]),
    ("ttr_result_line_blocks", _PI, [_VP]),
    ("ttr_result_line_pos", _PI, [_VP]),
    ("ttr_result_blocks", _PI, [_VP]),
    ("ttr_result_block_order", _PI, [_VP]),
    ("ttr_result_block_first", _PI, [_VP]),
    ("ttr_result_block_bboxes", _PF, [_VP]),
    ("ttr_result_block_text", _I, [_VP, _I, C.c_char_p, C.c_size_t]),
    ("ttr_result_page_text_blocks", _I, [_VP, C.c_char_p, C.c_size_t]),
    ("ttr_results_gather_blocks", _I, [C.POINTER(_VP), _I, _PI, _PI, _PI, _PI, _PI, _PI, _PI, _PF]),
    ("ttr_blocks_from_quads", _I, [_PF, _I, _PI, _PI, _PI, _PI, _PI, _PI, _PI]),
    ("ttr_group_blocks", _I, [_VP, _PF, _PI, _I, _PI, _PI, _PI, _PI, _PI, _PI, _PI]),
    ("ttr_result_free", None, [_VP]),
    ("ttr_result_bboxes", _PF, [_VP]),
    ("ttr_result_ids_all", _PI, [_VP]),
    ("ttr_result_texts", _I, [_VP, C.c_char_p, C.c_size_t]),
    ("ttr_results_gather", _I, [C.POINTER(_VP), _I, _PI, _PF, _PI, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ttr_results_gather_conf", _I, [C.POINTER(_VP), _I, _PF, _PF]),
    ("ttr_confidence_from_probs", _I, [_PI, _PF, _I, _PF, C.POINTER(C.c_int), _PF]),
    ("ttr_logits_confidence", _I, [_VP, _PF, _I, _PI, _PF, _PF]),
    ("ttr_charset_mask", _I, [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    ("ttr_engine_set_charset", _I, [_VP, C.c_char_p, C.c_char_p]),
    ("ttr_engine_get_charset", _I, [_VP, C.POINTER(C.c_uint32)]),
    ("ttr_logits_confidence_masked", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _PI, _PF, _PF]),
    ("ttr_region_from_rect", _I, [_I, _I, _I, _I, _PF]),
    ("ttr_region_geometry", _I, [_PF, _I, _I, C.POINTER(C.c_int64), _PF, C.POINTER(C.c_int)]),
    ("ttr_regions_to_data_dev", _I, [_VP, C.POINTER(Page), _I, C.POINTER(Region), _I, C.POINTER(C.c_uint32), _I, C.POINTER(_VP)]),
    ("ttr_image_regions_to_data", _I, [_VP, _PU8, _I, _I, _I, C.POINTER(Region), _I, C.POINTER(C.c_uint32), _I, C.POINTER(_VP)]),
    ("ttr_result_sets", _PI, [_VP]),
    ("ttr_pack_regions", _I, [_VP, _PU8, _I, _I, _I, _PF, _I, _PU8]),
    ("ttr_parseq_logits_sets", _I, [_VP, _PU8, _I, C.POINTER(C.c_uint32), _I, _PI, _PF, _PF, _PI]),
    ("ttr_logits_confidence_sets", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _I, _PI, _PI, _PF, _PF]),
    ("ttr_pattern_compile", _I, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(_VP)]),
    ("ttr_pattern_free", None, [_VP]),
    ("ttr_pattern_states", _I, [_VP]),
    ("ttr_pattern_min_length", _I, [_VP]),
    ("ttr_pattern_table", _I, [_VP, C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(_PU8), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("ttr_pattern_matches", _I, [_VP, C.c_char_p]),
    ("ttr_engine_set_pattern", _I, [_VP, C.c_char_p]),
    ("ttr_engine_get_pattern", C.c_char_p, [_VP]),
    ("ttr_regions_to_data_dev_p", _I, [_VP, C.POINTER(Page), _I, C.POINTER(Region), _I, C.POINTER(C.c_uint32), _I, C.POINTER(C.c_char_p), _I, _PI, C.POINTER(_VP)]),
    ("ttr_image_regions_to_data_p", _I, [_VP, _PU8, _I, _I, _I, C.POINTER(Region), _I, C.POINTER(C.c_uint32), _I, C.POINTER(C.c_char_p), _I, _PI, C.POINTER(_VP)]),
    ("ttr_parseq_logits_patterns", _I, [_VP, _PU8, _I, C.POINTER(C.c_uint32), _I, _PI, C.POINTER(C.c_char_p), _I, _PI, _PF, _PF, _PI]),
    ("ttr_logits_decode_patterns", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _I, _PI, C.POINTER(C.c_char_p), _I, _PI, _PI, _PF, _PF]),
    ("ttr_engine_set_pattern_decode", _I, [_VP, _I]),
    ("ttr_engine_pattern_decode", _I, [_VP]),
    ("ttr_result_pattern_logp", _PF, [_VP]),
    ("ttr_results_gather_pattern_logp", _I, [C.POINTER(_VP), _I, _PF]),
    ("ttr_logits_decode_patterns_best", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _I, _PI, C.POINTER(C.c_char_p), _I, _PI, _PI, _PF, _PF, _PF]),
    ("ttr_pattern_best_from_lp", _I, [_VP, _PF, _PI, _PI, _PF]),
    ("ttr_engine_set_alternatives", _I, [_VP, _I]),
    ("ttr_engine_alternatives", _I, [_VP]),
    ("ttr_result_alt_k", _I, [_VP]),
    ("ttr_result_alt_ids", _PI, [_VP, _I]),
    ("ttr_result_alt_probs", _PF, [_VP, _I]),
    ("ttr_result_alt_ids_all", _PI, [_VP]),
    ("ttr_result_alt_probs_all", _PF, [_VP]),
    ("ttr_results_gather_alts", _I, [C.POINTER(_VP), _I, _PI, _PF]),
    ("ttr_logits_alternatives", _I, [_VP, _PF, _I, _I, C.POINTER(C.c_uint32), _I, _PI, _PI, _PF]),
    ("ttr_nbest_from_alts", _I, [_PI, _PF, _I, _I, C.c_char_p, C.c_size_t, _PF, C.POINTER(C.c_size_t)]),
    ("ttr_engine_set_lexicon", _I, [_VP, C.POINTER(C.c_char_p), _I, _I]),
    ("ttr_engine_lexicon_size", _I, [_VP]),
    ("ttr_engine_lexicon_m", _I, [_VP]),
    ("ttr_engine_lexicon_word", C.c_char_p, [_VP, _I]),
    ("ttr_result_lex_m", _I, [_VP]),
    ("ttr_result_lex_idx", _PI, [_VP, _I]),
    ("ttr_result_lex_logp", _PF, [_VP, _I]),
    ("ttr_result_lex_idx_all", _PI, [_VP]),
    ("ttr_result_lex_logp_all", _PF, [_VP]),
    ("ttr_lexicon_encode", _I, [C.POINTER(C.c_char_p), _I, _PU8]),
    ("ttr_logits_lexicon", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _I, _PI, _PI, _PF]),
    ("ttr_engine_set_lexicon_fuzzy", _I, [_VP, _I, C.c_float]),
    ("ttr_engine_lexicon_fuzzy", _I, [_VP, _PI, _PF]),
    ("ttr_result_lex_band", _I, [_VP]),
    ("ttr_result_lex_edits", _PI, [_VP, _I]),
    ("ttr_result_lex_edits_all", _PI, [_VP]),
    ("ttr_lexicon_fuzzy_from_lp", _I, [_PF, _PU8, _I, _I, C.c_float, _PF, _PI]),
    ("ttr_logits_lexicon_fuzzy", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _I, _PI, _I, C.c_float, _PI, _PF, _PI]),
    ("ttr_debug_lexicon_tables", _I, [_VP, _PF, _I, C.POINTER(C.c_uint32), _I, _PI, _PF]),
    ("ttr_craft_heatmap", _I, [_VP, _PU8, _I, _I, _PF]),
    ("ttr_ccl_boxes", _I, [_VP, _PF, _I, _I, _PF, _I, _PI]),
    ("ttr_resize_canvas", _I, [_VP, _PU8, _I, _I, _I, _PU8, C.c_size_t, _PI, _PI, _PF]),
    ("ttr_pack_crops", _I, [_VP, _PU8, _I, _I, _I, _PF, _I, _F, _PU8, _PF]),
    ("ttr_pack_crops_rectified", _I, [_VP, _PU8, _I, _I, _I, _PF, _I, _F, _PU8, _PF]),
    ("ttr_pack_crops_oriented", _I, [_VP, _PU8, _I, _I, _I, _PF, _I, _F, _I, _I, _PU8, _PF]),
    ("ttr_parseq_logits", _I, [_VP, _PU8, _I, _PF, _PF, _PI]),
    ("ttr_decode_ids", _I, [_PI, _I, C.c_char_p]),
    ("ttr_engine_set_tuning", _I, [_VP, C.c_char_p, _I]),
    ("ttr_dbg_conv", _I, [_VP, _PF, _I, _PF, _I, _I, _I, _I, _I, _I, _I, _I, _PF, _PF, _I, _I, _PF]),
    ("ttr_dbg_min_area_rect", _I, [_PF, _I, _PF]),
    ("ttr_dbg_tcp_share", _I, [_I, _I, C.c_char_p, _I, _VP, C.c_size_t]),
    ("ttr_dbg_component_rect", _I, [_I, _I, _I, _I, _I, _PI, _I, _I, _PF]),
    ("ttr_dbg_box_geometry", _I, [_PF, _F, _PF, _PI, _PF]),
    ("ttr_dbg_deskew", _I, [_PF, _PF, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    ("ttr_dbg_orient_quad", _I, [_PF, _I, _I, _I, _I, _PF, C.POINTER(C.c_int64)]),
    ("ttr_dev_alloc", _VP, [C.c_size_t]),
    ("ttr_dev_free", None, [_VP]),
    ("ttr_dev_upload", _I, [_VP, _VP, C.c_size_t]),
    ("ttr_dev_download", _I, [_VP, _VP, C.c_size_t]),
    ("ttr_dev_sync", _I, [_VP]),
    ("ttr_last_stage_ms", _I, [_VP, _PF]),
    ("ttr_set_profiling", _I, [_VP, _I]),
    ("ttr_dbg_conv_pool", _I, [_VP, _PF, _I, _I, _I, _I, _I, _PF, _PF, _I, _I, _I, _PF, _PF]),
    ("ttr_dbg_split_gemm", _I, [_VP, _PF, _I, _I, _PF, _PF, _I, _I, _I, _I, _PF, _I, _PF]),
    ("ttr_dbg_split_planes", _I, [_VP, _PF, _I, _I, _I, _I, _I, C.POINTER(C.c_uint16), _PI]),
    ("ttr_dbg_layernorm_planes", _I, [_VP, _PF, _I, _I, _PF, _PF, _F, _I, _I, C.POINTER(C.c_uint16)]),
    ("ttr_dbg_ln_linear", _I, [_VP, _PF, _I, _PF, _PF, _F, _PF, _PF, _I, _I, _PF]),
    ("ttr_dbg_craft_taps", _I, [_VP, _PU8, _I, _I, _I, _PF]),
    ("ttr_dbg_craft_tap_count", _I, [_VP]),
    ("ttr_dbg_craft_tap_info", _I, [_VP, _I, C.c_char_p, C.c_size_t, _PI]),
    ("ttr_dbg_craft_tap_read", _I, [_VP, _I, _PF]),
    ("ttr_dbg_craft_fold_tap_count", _I, [_VP]),
    ("ttr_dbg_craft_fold_tap_info", _I, [_VP, _I, C.c_char_p, C.c_size_t, _PI]),
    ("ttr_dbg_craft_fold_tap_read", _I, [_VP, _I, _PF]),
    ("ttr_set_gemm_config", None, [_I]),
    ("ttr_set_decoder_mode", None, [_I]),
    ("ttr_set_tuning", _I, [C.c_char_p, _I]),
    ("ttr_last_host_us", None, [_VP, _PF]),
    ("ttr_dbg_attn_enc", _I, [_VP, _PF, _I, _PF]),
    ("ttr_dbg_cross_attn", _I, [_VP, _PF, _PF, _I, _I, _PF]),
    ("ttr_dbg_dec_self_attn", _I, [_VP, _PF, _PF, _PI, _I, _I, _I, _I, _PF]),
    ("ttr_dbg_qkv_attn", _I, [_VP, _PF, _I, _PF, _PF, _PF]),
    ("ttr_dbg_mlp", _I, [_VP, _PF, _I, _PF, _PF, C.c_float, _PF, _PF, _PF, _PF, _PF, _PF, _PF, _PF, _PF, _PF, _PF]),
    ("ttr_dbg_dec_stamps", _I, [C.POINTER(C.c_ulonglong)]),
    ("ttr_dbg_dec_stamps_ext", _I, [C.POINTER(C.c_ulonglong), _I]),
    ("ttr_bench_conv", _I, [_VP, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _PF]),
    ("ttr_get_profile", _I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    ("ttr_get_profile_kinds", _I, [_VP, C.c_char_p, C.c_size_t]),
    ("ttr_comm_unique_id", _I, [_VP]),
    ("ttr_comm_create", _VP, [_VP, _I, _I, _VP]),
    ("ttr_comm_create_tcp", _VP, [_VP, _I, _I, C.c_char_p, _I]),
    ("ttr_comm_create_socket", _VP, [_VP, _I, _I, C.c_char_p, _I]),
    ("ttr_comm_transport", C.c_char_p, [_VP]),
    ("ttr_comm_describe", _I, [_VP, C.c_char_p, C.c_size_t]),
    ("ttr_comm_destroy", None, [_VP]),
    ("ttr_comm_rank", _I, [_VP]),
    ("ttr_comm_world", _I, [_VP]),
    ("ttr_engine_attach_comm", _I, [_VP, _VP]),
    ("ttr_last_gathered", _I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int), _PI, C.c_size_t, _PI, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ttr_last_gathered_conf", _I, [_VP, _PF, C.c_size_t, _PF, C.c_size_t]),
    ("ttr_comm_allgather_host", _I, [_VP, _VP, C.c_size_t, _VP]),
    ("ttr_gather_layout", _I, [_PI, _I, _I, C.POINTER(C.c_int), _PI, C.POINTER(C.c_int64)]),
    ("ttr_pages_to_data_dev_sharded", _I, [_VP, _VP, _I, _I, _I, C.POINTER(_VP)]),
    ("ttr_engine_set_wide", _I, [_VP, _F]),
    ("ttr_engine_wide", _F, [_VP]),
    ("ttr_result_piece_first", _PI, [_VP]),
    ("ttr_result_piece_ids", _PI, [_VP]),
    ("ttr_result_piece_probs", _PF, [_VP]),
    ("ttr_result_piece_confs", _PF, [_VP]),
    ("ttr_result_piece_quads", _PF, [_VP]),
    ("ttr_result_piece_cuts", _PI, [_VP]),
    ("ttr_results_gather_pieces", _I, [C.POINTER(_VP), _I, _PI, _PI, _PF, _PF, _PF, _PI]),
    ("ttr_wide_plan", _I, [_PF, _F, C.POINTER(C.c_int64)]),
    ("ttr_wide_profile", _I, [_PU8, _I, _I, _I, C.POINTER(C.c_int64), _I, C.POINTER(C.c_uint16)]),
    ("ttr_wide_cuts_from_profile", _I, [C.POINTER(C.c_uint16), _I, _PI]),
    ("ttr_wide_piece_coef", _I, [C.POINTER(C.c_int64), _I, _I, C.POINTER(C.c_int64)]),
    ("ttr_wide_piece_quads", _I, [_PF, _PI, _I, _PF]),
    ("ttr_wide_cuts", _I, [_VP, _PU8, _I, _I, _I, _PF, _I, _F, _I, _PI, _PI, C.POINTER(C.c_uint16), C.POINTER(C.c_int64)]),
    ("ttr_engine_set_curved", _I, [_VP, _I]),
    ("ttr_engine_curved", _I, [_VP]),
    ("ttr_result_curved", _PI, [_VP]),
    ("ttr_result_outlines", _PF, [_VP]),
    ("ttr_result_spine_knots", C.POINTER(C.c_int64), [_VP]),
    ("ttr_results_gather_curved", _I, [C.POINTER(_VP), _I, _PI, _PF, C.POINTER(C.c_int64)]),
    ("ttr_curve_frame", _I, [_PF, C.POINTER(C.c_int64)]),
    ("ttr_curve_columns", _I, [_PU8, _I, _I, _I, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _PI]),
    ("ttr_curve_knots", _I, [_PU8, _I, _I, _I, C.POINTER(C.c_int64), _PI, _PI, _PI, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("ttr_curve_crop", _I, [_PU8, _I, _I, _I, C.POINTER(C.c_int64), _PU8]),
    ("ttr_curve_outline", _I, [_PF, _I, C.POINTER(C.c_int64), _PF]),
    ("ttr_curve_crops", _I, [_VP, _PU8, _I, _I, _I, _PF, _I, _I, _PI, _PI, _PI, C.POINTER(C.c_int64), _PU8]),
    ("ttr_engine_set_tables", _I, [_VP, _I, _I]),
    ("ttr_engine_tables", _I, [_VP, _PI]),
    ("ttr_result_table_mode", _I, [_VP]),
    ("ttr_result_ruling_count", _I, [_VP]),
    ("ttr_result_rulings", _PI, [_VP]),
    ("ttr_result_table_count", _I, [_VP]),
    ("ttr_result_tables", _PI, [_VP]),
    ("ttr_result_table_lines", _PI, [_VP, _PI]),
    ("ttr_result_cell_count", _I, [_VP]),
    ("ttr_result_cells", _PI, [_VP]),
    ("ttr_result_item_table", _PI, [_VP]),
    ("ttr_result_item_cell", _PI, [_VP]),
    ("ttr_result_cell_text", _I, [_VP, _I, C.c_char_p, _I]),
    ("ttr_results_gather_tables", _I, [C.POINTER(_VP), _I, _PI, _PI]),
    ("ttr_tables_from_page", _I, [_PU8, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI, _PI, _PI, _PI, _PI]),
    ("ttr_tables_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI, _PI, _PI, _PI, _PI]),
    ("ttr_dbg_tables", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_uint64), _PI, _PI, _PI]),
    ("ttr_engine_set_deskew", _I, [_VP, _I, _I, _I]),
    ("ttr_engine_deskew", _I, [_VP, _PI, _PI]),
    ("ttr_result_skew", _I, [_VP, C.c_void_p]),
    ("ttr_result_to_page", _I, [_VP, _PF, _I, _PF]),
    ("ttr_skew_to_page", _I, [C.c_void_p, _PF, _I, _PF]),
    ("ttr_results_gather_skew", _I, [C.POINTER(_VP), _I, C.c_void_p]),
    ("ttr_deskew_from_page", _I, [_PU8, _I, _I, _I, _I, _I, _I, _PU8, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("ttr_deskew_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _PU8, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("ttr_dbg_deskew_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _I, _I, _PU8, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("ttr_engine_set_ink", _I, [_VP, _I, _I, _I]),
    ("ttr_engine_ink", _I, [_VP, _PI, _PI]),
    ("ttr_result_ink", _I, [_VP, C.c_void_p]),
    ("ttr_results_gather_ink", _I, [C.POINTER(_VP), _I, C.c_void_p]),
    ("ttr_ink_from_page", _I, [_PU8, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
    ("ttr_ink_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
    ("ttr_dbg_ink_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
    ("ttr_engine_set_marks", _I, [_VP, _I, _I, _I, _I]),
    ("ttr_engine_marks", _I, [_VP, _PI, _PI, _PI]),
    ("ttr_result_mark_mode", _I, [_VP]),
    ("ttr_result_mark_count", _I, [_VP]),
    ("ttr_result_marks", _PI, [_VP]),
    ("ttr_result_item_mark", _PI, [_VP]),
    ("ttr_results_gather_marks", _I, [C.POINTER(_VP), _I, _PI]),
    ("ttr_marks_from_page", _I, [_PU8, _I, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI]),
    ("ttr_marks_from_page_ink", _I, [_PU8, _I, _I, _I, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI]),
    ("ttr_marks_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI]),
    ("ttr_dbg_marks", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _I, _I, _I, _PI, _PI, _PI, _PI]),
    ("ttr_engine_set_barcodes", _I, [_VP, _I, _I, _I]),
    ("ttr_engine_barcodes", _I, [_VP, _PI, _PI]),
    ("ttr_result_barcode_mode", _I, [_VP]),
    ("ttr_result_barcode_count", _I, [_VP]),
    ("ttr_result_barcodes", _PI, [_VP]),
    ("ttr_result_item_barcode", _PI, [_VP]),
    ("ttr_results_gather_barcodes", _I, [C.POINTER(_VP), _I, _PI]),
    ("ttr_barcodes_from_page", _I, [_PU8, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI, _PI, _PI]),
    ("ttr_barcodes_from_page_ink", _I, [_PU8, _I, _I, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI]),
    ("ttr_barcodes_page", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI]),
    ("ttr_dbg_barcodes", _I, [_VP, _PU8, _I, _I, _I, _I, _I, _I, _I, _I, _PI, _PI, _PI]),
    ("ttr_dbg_page_ink_passes", C.c_int64, [_VP]),
    ("ttr_tables_from_page_ink", _I, [_PU8, _I, _I, _I, _I, _I, _I, _I, _PF, _I, _PI, _PI, _PI, _PI, _PI, _PI, _PI, _PI]),
    ("ttr_deskew_from_page_ink", _I, [_PU8, _I, _I, _I, _I, _I, _I, _I, _I, _PU8, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("ttr_engine_set_tiled", _I, [_VP, _I]),
    ("ttr_engine_tiled", _I, [_VP]),
    ("ttr_result_tiles", _I, [_VP]),
    ("ttr_tile_plan", _I, [_I, _I, _I, _I, _F] + [_PI] * 10),
    ("ttr_stitch_tiles", _I, [_PF, _I, _I, _I, _PI, _PI, _I, _I, _I, _I, _PF]),
    ("ttr_stitch_heat", _I, [_VP, _PF, _I, _I, _I, _PI, _PI, _I, _I, _I, _I, _PF]),
    ("ttr_craft_heatmap_tiled", _I, [_VP, _PU8, _I, _I, _I, _I, _PF, C.c_size_t, _PI, _PI]),
    ("ttr_tile_canvases", _I, [_VP, _PU8, _I, _I, _I, _I, _PU8, C.c_size_t]),
]


def lib_path() -> str:
    return _LIBPATH


def load():
    """Load libtuatara_hip.so (no GPU needed for loading)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise RuntimeError(f"{_LIBPATH} is missing: run `python -m tuatara_amd.build` (or __graft_entry__.build()) first")
        # PyTorch's ROCm wheel carries its own HIP runtime.  If torch is imported AFTER this library (which links the system
        # runtime) has been loaded, the process ends up with two runtimes and the one that initialises second sees no device
        # ("no HIP device available").  Imported first, torch's copy is the one both use.  A Python process that loads the
        # engine may import torch later (the oracle, torch.distributed), so: torch first, where it is installed
        # (TUATARA_PRELOAD_TORCH=0 turns this off; the C++ callers - pytuatara, ocr_cli - never see torch).
        if "torch" not in sys.modules and os.environ.get("TUATARA_PRELOAD_TORCH", "1") != "0":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = C.CDLL(_LIBPATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _u8(a):
    return a.ctypes.data_as(_PU8)


def _f(a):
    return a.ctypes.data_as(_PF)


def _i(a):
    return a.ctypes.data_as(_PI)


class EngineError(RuntimeError):
    pass


def decode_ids(ids: Sequence[int]) -> str:
    a = np.ascontiguousarray(ids, dtype=np.int32)
    buf = C.create_string_buffer(len(a) + 2)
    load().ttr_decode_ids(_i(a), len(a), buf)
    return buf.value.decode("latin1")


def min_area_rect(points) -> np.ndarray:
    """Engine host geometry (no GPU): cv::minAreaRect stand-in."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(5, np.float32)
    load().ttr_dbg_min_area_rect(_f(pts), len(pts), _f(out))
    return out


def component_rect(area: int, x0: int, y0: int, x1: int, y1: int, rows: np.ndarray, H: int, W: int):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros(5, np.float32)
    ok = load().ttr_dbg_component_rect(area, x0, y0, x1, y1, _i(rows), H, W, _f(out))
    return out if ok == 1 else None


def box_geometry(rect5, ratio: float):
    r = np.ascontiguousarray(rect5, dtype=np.float32)
    adj, xywh, bbox = np.zeros(5, np.float32), np.zeros(4, np.int32), np.zeros(4, np.float32)
    load().ttr_dbg_box_geometry(_f(r), C.c_float(ratio), _f(adj), _i(xywh), _f(bbox))
    return adj, tuple(int(v) for v in xywh), [float(v) for v in bbox]


def deskew(rect5):
    """Engine host geometry (no GPU): the rectified-crop rule on one rect {cx,cy,w,h,angle} in image pixels (ttr_dbg_deskew) ->
    (kind, quad f32 [4,2] tl/tr/br/bl, coef f64 [6] {X0,Ax,Bx,Y0,Ay,By}, fixed int64 [6] in units of 2^-16 px)."""
    r = np.ascontiguousarray(rect5, dtype=np.float32)
    quad, coef, fixed = np.zeros(8, np.float32), np.zeros(6, np.float64), np.zeros(6, np.int64)
    kind = load().ttr_dbg_deskew(_f(r), _f(quad), coef.ctypes.data_as(C.POINTER(C.c_double)), fixed.ctypes.data_as(C.POINTER(C.c_int64)))
    if kind < 0:
        raise EngineError(load().ttr_last_error().decode())
    return kind, quad.reshape(4, 2), coef, fixed


def orient_quad(rect5, h: int, w: int, crop_mode: int, turn: int):
    """Engine host geometry (no GPU): a word's quad turned by `turn` quarter turns and its fixed-point coefficients, as the engine forms its
    twin crops (ttr_dbg_orient_quad) -> (quad f32 [4,2] = Q_t, fixed int64 [6])."""
    r = np.ascontiguousarray(rect5, dtype=np.float32)
    quad, fixed = np.zeros(8, np.float32), np.zeros(6, np.int64)
    if load().ttr_dbg_orient_quad(_f(r), int(h), int(w), int(crop_mode), int(turn), _f(quad), fixed.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise EngineError(load().ttr_last_error().decode())
    return quad.reshape(4, 2), fixed


def canvas_geometry(h: int, w: int, canvas_size: int = 1024, mag_ratio: float = 1.0):
    """The detector canvas of an h x w page on the host (ttr_dbg_canvas_geometry, no GPU; DESIGN.md "Mixed-size batches") ->
    (H, W, ratio, target_h, target_w): the page scaled by ratio to target_h x target_w, each side rounded up to a multiple of 32."""
    H, W, th, tw, ratio = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
    if load().ttr_dbg_canvas_geometry(int(h), int(w), int(canvas_size), float(mag_ratio), C.byref(H), C.byref(W), C.byref(ratio), C.byref(th), C.byref(tw)) != 0:
        raise EngineError("ttr_dbg_canvas_geometry: h and w must be positive")
    return H.value, W.value, ratio.value, th.value, tw.value


OFFSET_WINDOW = (1 << 31) - 1              # most bytes a tensor the f16x4 kernels address with 32-bit buffer offsets may hold


def launch_groups(H: int, W: int, n_pages: int, n_crops: int, craft_group: int = 16, first_fused: int = 1, craft_products: int = 3, up_commute: int = 1,
                  enc_chunk: int = 0, enc_fc2_pairs: int = 1, qkv_attn_split: int = 1, enc_ln_pairs: int = 1, sp_hidden16: int = 0):
    """The f16x4 engine's launch groups on the host (ttr_dbg_launch_groups, no GPU; DESIGN.md "Launch groups") for a batch of n_pages canvases of H x W and
    n_crops crops under the tuning values given -> (pages per CRAFT group, crops per encoder group, bytes per page, bytes per crop of the widest tensor)."""
    gp, ge, bp, bc = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    rc = load().ttr_dbg_launch_groups(int(H), int(W), int(n_pages), int(n_crops), int(craft_group), int(first_fused), int(craft_products), int(up_commute),
                                      int(enc_chunk), int(enc_fc2_pairs), int(qkv_attn_split), int(enc_ln_pairs), int(sp_hidden16),
                                      C.byref(gp), C.byref(ge), C.byref(bp), C.byref(bc))
    if rc != 0:
        raise EngineError("ttr_dbg_launch_groups: H and W must be positive multiples of 32, the counts and craft_group at least 1")
    return gp.value, ge.value, bp.value, bc.value


def split_layer_check(kernel: str, B: int, H: int, W: int, C0: int, Cout: int, ks: int = 3, products: int = 3, out_planes: int = 2, pooled: bool = False):
    """The shape check of an f16x4 layer launcher on the host (ttr_dbg_split_layer_check, no GPU, nothing is launched): kernel "conv3p", "gemm2" or "conv3p_first" (conv1_1 fused in front) ->
    None when the launcher takes the layer, else its reason."""
    text = C.create_string_buffer(256)
    rc = load().ttr_dbg_split_layer_check({"conv3p": 0, "gemm2": 1, "conv3p_first": 2}[kernel], int(B), int(H), int(W), int(C0), int(Cout), int(ks), int(products), int(out_planes),
                                          int(bool(pooled)), text, 256)
    if rc < 0:
        raise EngineError("ttr_dbg_split_layer_check: bad arguments")
    return text.value.decode() if rc else None


def scratch_table():
    """The engine's device buffers as engine.h classifies them (ttr_dbg_scratch_table, no GPU) -> a list of (name, class, kind, note): class "scratch" /
    "kept", kind "f32" / "f16" / "u8" / "i32" / "addr"; a kept row's note is the contract that makes it so."""
    buf = C.create_string_buffer(1 << 16)
    n = load().ttr_dbg_scratch_table(buf, len(buf))
    if n < 0 or n >= len(buf):
        raise EngineError("ttr_dbg_scratch_table: the table does not fit the buffer")
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split(None, 3)
        rows.append((f[0], f[1], f[2], f[3] if len(f) > 3 else ""))
    return rows


def _host_images(images):
    """a list of host images [h, w, 3] u8 (C-contiguous rows: a view into a wider array keeps its row stride) -> ctypes pointer, h, w, stride arrays + keep-alives"""
    keep = []
    for im in images:
        a = np.asarray(im)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise EngineError("Input array should have 3 dimensions")
        if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
            a = np.ascontiguousarray(a)
        keep.append(a)
    n = len(keep)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in keep])
    hs = (C.c_int32 * n)(*[a.shape[0] for a in keep])
    ws = (C.c_int32 * n)(*[a.shape[1] for a in keep])
    st = (C.c_int32 * n)(*[a.strides[0] for a in keep])
    return ptrs, hs, ws, st, keep


def confidence_from_probs(ids, probs):
    """The confidence rule on the host (ttr_confidence_from_probs, no GPU): ids / probs of one row -> (char_conf f32 [len(text)], conf f32)."""
    ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
    probs = np.ascontiguousarray(probs, dtype=np.float32).ravel()
    if len(ids) != len(probs):
        raise ValueError("ids and probs differ in length")
    cc = np.zeros(max(len(ids), 1), np.float32)
    nc, conf = C.c_int(), C.c_float()
    if load().ttr_confidence_from_probs(_i(ids), _f(probs), len(ids), _f(cc), C.byref(nc), C.byref(conf)) < 0:
        raise EngineError("ttr_confidence_from_probs: bad arguments")
    return cc[:nc.value].copy(), np.float32(conf.value)


def _charlist(s):
    """A character list for the C ABI: None stays None; str travels as bytes (one byte per character where latin-1 can)."""
    if s is None or isinstance(s, bytes):
        return s
    try:
        return s.encode("latin1")
    except UnicodeEncodeError:
        return s.encode("utf-8")


def charset_mask(allow=None, deny=None) -> np.ndarray:
    """The class mask of a character set on the host (ttr_charset_mask, no GPU; DESIGN.md "Character sets"): uint32 [3], class c = bit c & 31 of
    word c >> 5.  Bit 0 (EOS) is always set; None or "" mean every character (allow) / none (deny).  A character that names no class ('~', a blank,
    non-ASCII) or a set that leaves only EOS raises EngineError."""
    m = (C.c_uint32 * 3)()
    if load().ttr_charset_mask(_charlist(allow), _charlist(deny), m) < 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    return np.array(list(m), dtype=np.uint32)


class Pattern:
    """A compiled pattern (ttr_pattern_compile, no GPU; DESIGN.md "Patterns"): .states - states of the minimal automaton, its DONE state not counted;
    .min_length - characters of the shortest member; .table() -> (delta uint16 [states + 1, 96], mind uint8 [states + 1], start, done); .matches(text) ->
    True / False, or None for a text that names no class somewhere."""

    def __init__(self, pattern, mask=None):
        self.lib = load()
        self.h = None
        self.pattern = pattern
        m = None if mask is None else (C.c_uint32 * 3)(*[int(v) for v in np.asarray(mask).ravel()[:3]])
        h = C.c_void_p()
        if self.lib.ttr_pattern_compile(_charlist(pattern), m, C.byref(h)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))
        self.h = h

    @property
    def states(self) -> int:
        return int(self.lib.ttr_pattern_states(self.h))

    @property
    def min_length(self) -> int:
        return int(self.lib.ttr_pattern_min_length(self.h))

    def table(self):
        d, m, s, e = C.POINTER(C.c_uint16)(), _PU8(), C.c_int(), C.c_int()
        rows = self.lib.ttr_pattern_table(self.h, C.byref(d), C.byref(m), C.byref(s), C.byref(e))
        return (np.ctypeslib.as_array(d, (rows, 96)).copy(), np.ctypeslib.as_array(m, (rows,)).copy(), s.value, e.value)

    def matches(self, text):
        r = self.lib.ttr_pattern_matches(self.h, _charlist(text))
        return None if r < 0 else bool(r)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ttr_pattern_free(self.h)
            self.h = None


def pattern_compile(pattern, mask=None) -> Pattern:
    """Compile a pattern under a class mask (charset_mask's form; None = every class) on the host.  EngineError for a refused pattern."""
    return Pattern(pattern, mask)


PATTERN_GREEDY, PATTERN_BEST = 0, 1


def pattern_best_from_lp(pattern, lp, mask=None):
    """The likeliest member of a pattern's language under a table lp f32 [26, 96] (ttr_pattern_best_from_lp, no GPU; DESIGN.md "Patterns", best mode):
    -> (path i32 [L] the classes, logp f32), or None when no member has a finite score.  `pattern`: a Pattern, or a string compiled under `mask`."""
    pat = pattern if isinstance(pattern, Pattern) else Pattern(pattern, mask)
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    if lp.shape != (26, 96):
        raise ValueError("lp is a [26, 96] table: row p = position p, column 0 = the end of the text")
    path, ln, logp = np.zeros(26, np.int32), C.c_int32(-1), C.c_float(0.0)
    rc = pat.lib.ttr_pattern_best_from_lp(pat.h, _f(lp), _i(path), C.cast(C.byref(ln), _PI), C.cast(C.byref(logp), _PF))
    if rc < 0:
        raise EngineError("ttr_pattern_best_from_lp: null argument")
    return None if rc else (path[:ln.value].copy(), np.float32(logp.value))


def _patterns_arg(patterns):
    """a list of pattern strings (or None) -> (char* array or None, n, keep-alive)"""
    if patterns is None or len(patterns) == 0:
        return None, 0, None
    enc = [_charlist(p) for p in patterns]
    return (C.c_char_p * len(enc))(*enc), len(enc), enc


def _pattern_rows(patterns):
    """a list parallel to the rows, None = no pattern of its own -> (distinct patterns, pattern_of i32 [n])"""
    distinct, of = [], np.full(len(patterns), -1, np.int32)
    for i, p in enumerate(patterns):
        if p is None:
            continue
        if p not in distinct:
            distinct.append(p)
        of[i] = distinct.index(p)
    return distinct, of


def region_from_rect(x0: int, y0: int, x1: int, y1: int) -> np.ndarray:
    """The pixel-edge quad of the pixels [x0, x1) x [y0, y1) (ttr_region_from_rect, no GPU): f32 [8] tl, tr, br, bl, pixel centres at integers."""
    q = np.zeros(8, np.float32)
    if load().ttr_region_from_rect(int(x0), int(y0), int(x1), int(y1), _f(q)) < 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    return q


def region_geometry(quad, h: int = 0, w: int = 0):
    """What a region call derives from one quad on the host (ttr_region_geometry, no GPU): (fixed int64 [6] - the sampler's coefficients in 2^-16 px -,
    bbox f32 [4], inside - every corner within the pixel edges of an h x w page).  EngineError for a coordinate that is not finite or has |x| >= 32768."""
    q = np.ascontiguousarray(quad, dtype=np.float32).ravel()
    if q.size != 8:
        raise ValueError("a quad is 8 floats (tl, tr, br, bl)")
    fixed, bbox, inside = np.zeros(6, np.int64), np.zeros(4, np.float32), C.c_int(0)
    if load().ttr_region_geometry(_f(q), int(h), int(w), fixed.ctypes.data_as(C.POINTER(C.c_int64)), _f(bbox), C.byref(inside)) < 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    return fixed, bbox, bool(inside.value)


def region_quad(region) -> np.ndarray:
    """A region as the C ABI takes it: an 8-float quad (or 4 x 2) stays, an (x0, y0, x1, y1) rectangle becomes its pixel-edge quad."""
    a = np.asarray(region, dtype=np.float64).ravel()
    if a.size == 8:
        return a.astype(np.float32)
    if a.size == 4:
        if not np.all(a == np.floor(a)):
            raise ValueError("a rectangle region is four integers (x0, y0, x1, y1)")
        return region_from_rect(*[int(v) for v in a])
    raise ValueError("a region is an 8-float quad (tl, tr, br, bl) or an (x0, y0, x1, y1) rectangle")


def charset_masks(charsets) -> np.ndarray:
    """A list of character sets -> uint32 [n, 3]: each entry an (allow, deny) pair (None or "" = every / no character) or a ready-made mask (3 words)."""
    out = np.zeros((len(charsets), 3), np.uint32)
    for i, cs in enumerate(charsets):
        if isinstance(cs, np.ndarray) or (len(cs) == 3 and all(isinstance(v, (int, np.integer)) for v in cs)):
            out[i] = np.asarray(cs, dtype=np.uint32).ravel()[:3]
        elif len(cs) == 2:
            out[i] = charset_mask(cs[0], cs[1])
        else:
            raise ValueError("a charset is an (allow, deny) pair or a mask of three words")
    return out


def _sets_arg(sets):
    """uint32 [n, 3] (or None) -> (pointer, n, keep-alive array)"""
    if sets is None or len(sets) == 0:
        return None, 0, None
    m = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1, 3)
    return m.ctypes.data_as(C.POINTER(C.c_uint32)), len(m), m


def orient_select(conf, ids, per_page: bool = False):
    """The orientation choice on the host (ttr_orient_select, no GPU): one page's conf f32 [n, k] and ids i32 [n, k, 26] of k candidate
    readings in ascending turn order (k = 2: turns 0, 2; k = 4: turns 0..3) -> (turns i32 [n] as 0..3, page turn)."""
    conf = np.ascontiguousarray(conf, dtype=np.float32)
    n, k = conf.shape
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(n, k, 26)
    turns, pt = np.zeros(max(n, 1), np.int32), C.c_int32()
    if load().ttr_orient_select(_f(conf), _i(ids), n, k, int(per_page), _i(turns), C.byref(pt)) != 0:
        raise EngineError("ttr_orient_select: bad arguments")
    return turns[:n].copy(), int(pt.value)


def lines_from_quads(quads):
    """The text-line rule on the host (ttr_lines_from_quads, no GPU; DESIGN.md "Text lines"): one page's quads f32 [n, 8] (tl, tr, br, bl) ->
    (line i32 [n] in line order, word i32 [n] the position inside the line, n_lines)."""
    q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    n = len(q)
    line, word, nl = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), C.c_int32()
    if load().ttr_lines_from_quads(_f(q), n, _i(line), _i(word), C.byref(nl)) != 0:
        raise EngineError("ttr_lines_from_quads: a coordinate is not finite or has |x| >= 32768")
    return line[:n].copy(), word[:n].copy(), int(nl.value)


def char_cuts_from_profile(q, K: int, qlow: int):
    """The cut rule on one profile (ttr_char_cuts_from_profile, no GPU; DESIGN.md "Character boxes"): q u8 [128], K characters (0..26),
    qlow = int(low_text * 255) -> (cuts i32 [27]: b[0..K] in 1/256 column, -1 beyond K; mode 0 uniform / 1 valley cuts)."""
    q = np.ascontiguousarray(q, dtype=np.uint8).reshape(128)
    cuts, mode = np.zeros(27, np.int32), C.c_int32()
    if load().ttr_char_cuts_from_profile(_u8(q), int(K), int(qlow), _i(cuts), C.byref(mode)) != 0:
        raise EngineError("ttr_char_cuts_from_profile: K must lie in 0..26")
    return cuts, int(mode.value)


def blocks_from_quads(quads):
    """The text-block rule on the host (ttr_blocks_from_quads, no GPU; DESIGN.md "Text blocks"): one page's quads f32 [n, 8] -> (line i32 [n],
    word i32 [n], n_lines, block i32 [n_lines] each line's block in reading order, pos i32 [n_lines] its position inside that block, n_blocks,
    mode: 1 ordered by the precedence relation, 0 more than 512 blocks, by key alone)."""
    q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    n = len(q)
    line, word, block, pos = (np.zeros(max(n, 1), np.int32) for _ in range(4))
    nl, nb, mode = C.c_int32(), C.c_int32(), C.c_int32()
    if load().ttr_blocks_from_quads(_f(q), n, _i(line), _i(word), C.byref(nl), _i(block), _i(pos), C.byref(nb), C.byref(mode)) != 0:
        raise EngineError("ttr_blocks_from_quads: a coordinate is not finite or has |x| >= 32768")
    m = int(nl.value)
    return line[:n].copy(), word[:n].copy(), m, block[:m].copy(), pos[:m].copy(), int(nb.value), int(mode.value)


def _chars_args(tnorm, quads, turns, nchars):
    t = np.ascontiguousarray(tnorm, dtype=np.float32)
    if t.ndim != 2:
        raise ValueError("tnorm must be a [H2, W2] plane")
    q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    n = len(q)
    tu = np.ascontiguousarray(turns, dtype=np.int32).reshape(-1)
    nc = np.ascontiguousarray(nchars, dtype=np.int32).reshape(-1)
    if len(tu) != n or len(nc) != n:
        raise ValueError("turns and nchars must hold one entry per quad")
    out = np.zeros((max(n, 1), 27), np.int32), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 128), np.uint8)
    return t, q, tu, nc, n, out


def chars_from_map(tnorm, ratio: float, low_text: float, quads, turns, nchars):
    """The character rule on the host (ttr_chars_from_map, no GPU; DESIGN.md "Character boxes"): one page's normalised region plane f32
    [H2, W2], its canvas ratio, n words as quads f32 [n, 8], turns i32 [n] and character counts i32 [n] ->
    (cuts i32 [n, 27], mode i32 [n], profile u8 [n, 128])."""
    t, q, tu, nc, n, (cuts, modes, prof) = _chars_args(tnorm, quads, turns, nchars)
    if load().ttr_chars_from_map(_f(t), t.shape[0], t.shape[1], float(ratio), float(low_text), _f(q), _i(tu), _i(nc), n, _i(cuts), _i(modes), _u8(prof)) != 0:
        raise EngineError("ttr_chars_from_map: a coordinate is not finite or has |x| >= 32768, or a turn, count or ratio is out of range")
    return cuts[:n].copy(), modes[:n].copy(), prof[:n].copy()


def char_quads_from_cuts(quad, turn: int, cuts, K: int):
    """One word's cells (ttr_char_quads_from_cuts): quad f32 [8], turn, cuts i32 [27], K -> (quads f32 [K, 8], bboxes f32 [K, 4])."""
    q = np.ascontiguousarray(quad, dtype=np.float32).reshape(8)
    c = np.ascontiguousarray(cuts, dtype=np.int32).reshape(27)
    oq, ob = np.zeros((max(K, 1), 8), np.float32), np.zeros((max(K, 1), 4), np.float32)
    if load().ttr_char_quads_from_cuts(_f(q), int(turn), _i(c), int(K), _f(oq), _f(ob)) != 0:
        raise EngineError("ttr_char_quads_from_cuts: bad arguments")
    return oq[:K].copy(), ob[:K].copy()


def nbest_from_alts(alt_ids, alt_prob, m: int):
    """The M best readings of one word from its alternatives (ttr_nbest_from_alts, no GPU, exact; DESIGN.md "Character alternatives"): alt_ids i32 [26, K]
    and alt_prob f32 [26, K] -> [(text, score f32), ...], at most m (1..64), by (score descending, rank tuple ascending).  Readings differ from the top
    reading by substitutions only; reading 0 is the item's (text, conf)."""
    ids = np.ascontiguousarray(alt_ids, dtype=np.int32)
    prob = np.ascontiguousarray(alt_prob, dtype=np.float32)
    if ids.ndim != 2 or ids.shape[0] != 26 or prob.shape != ids.shape:
        raise ValueError("alt_ids and alt_prob are [26, K] arrays")
    k = ids.shape[1]
    need = C.c_size_t()
    scores = np.zeros(max(int(m), 1), np.float32)
    n = load().ttr_nbest_from_alts(_i(ids), _f(prob), k, int(m), None, 0, _f(scores), C.byref(need))
    if n < 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    buf = C.create_string_buffer(max(need.value, 1))
    load().ttr_nbest_from_alts(_i(ids), _f(prob), k, int(m), buf, need.value, None, None)
    texts = buf.raw[:need.value].decode("latin1").split("\n")
    return [(texts[i], np.float32(scores[i])) for i in range(n)]


def _words_arg(words):
    """a word list -> (char* array, count, the bytes objects kept alive).  A str travels as _charlist sends it - latin1 where it can, else UTF-8 - so a
    character outside ASCII reaches the library as bytes that name no class and is refused there, naming the word.  An entry that cannot be encoded or
    holds a NUL (which would cut it short on the way) is refused here, likewise."""
    bs = []
    for i, w in enumerate(words):
        try:
            b = bytes(w) if isinstance(w, (bytes, bytearray)) else _charlist(str(w))
        except UnicodeEncodeError:
            raise EngineError(f"lexicon: word {i} cannot be encoded") from None
        if b"\0" in b:
            raise EngineError(f"lexicon: word {i} holds '\\x00', which names no recogniser class")
        bs.append(b)
    arr = (C.c_char_p * max(len(bs), 1))(*bs)
    return arr, len(bs), bs


def lexicon_encode(words) -> np.ndarray:
    """The 32-byte device records of a word list (ttr_lexicon_encode, no GPU; DESIGN.md "Lexicon matching"): u8 [n, 32] - byte 0 the length, bytes 1..L the
    classes, zeros behind.  Raises EngineError naming the first offending word's index."""
    arr, n, _keep = _words_arg(words)
    rec = np.zeros((max(n, 1), 32), np.uint8)
    if load().ttr_lexicon_encode(arr, n, _u8(rec)) != 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    return rec[:n]


def lexicon_matches(words, idx, logp) -> list:
    """one item's matches [(word, prob), ...]: the filled slots of idx / logp [M], prob = exp(logp) in float64"""
    return [(words[int(i)], float(np.exp(np.float64(l)))) for i, l in zip(idx, logp) if int(i) >= 0]


LEXICON_GAP = float(np.float32(-6.9077554))   # ln 1e-3: the default gap of fuzzy alignment, at band 1; neither has been tuned on documents


def lexicon_fuzzy_from_lp(lp, records, band: int, gap: float = LEXICON_GAP):
    """Fuzzy alignment of lexicon entries on the host (ttr_lexicon_fuzzy_from_lp, no GPU; DESIGN.md "Lexicon matching", Fuzzy alignment): one table lp f32
    [26, 96] and records u8 [n, 32] (lexicon_encode's) -> (logp f32 [n], edits i32 [n]) under a band 0..3 and a gap (finite, <= 0).  Raises EngineError for a
    band or gap out of range and for a record whose length byte is outside 1..25."""
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    if lp.shape != (26, 96):
        raise ValueError("lp is one crop's table, f32 [26, 96]")
    records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, 32)
    n = len(records)
    logp, edits = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
    if load().ttr_lexicon_fuzzy_from_lp(_f(lp), _u8(records) if n else _u8(np.zeros(32, np.uint8)), n, int(band), float(gap), _f(logp), _i(edits)) != 0:
        raise EngineError("lexicon_fuzzy_from_lp: the band must lie in 0..3, the gap be finite and <= 0, every record's length in 1..25")
    return logp[:n], edits[:n]


def _is_char(c: int) -> bool:
    return 1 <= c < 95 and c != 88


def char_alternatives(alt_ids, alt_prob) -> list:
    """One word's alternatives per character of its text: alt_ids i32 [26, K], alt_prob f32 [26, K] -> one list per character (the positions before the EOS
    whose slot-0 id is a character), holding (char, prob) over that position's character options - slots that are not -1, the EOS or id 88 - ranked by
    (prob descending, slot ascending)."""
    out = []
    for p in range(26):
        if int(alt_ids[p][0]) == 0:
            break
        if not _is_char(int(alt_ids[p][0])):
            continue
        slots = [j for j in range(len(alt_ids[p])) if _is_char(int(alt_ids[p][j]))]
        slots.sort(key=lambda j: -float(alt_prob[p][j]))          # (stable: ties keep slot order)
        out.append([(decode_ids([int(alt_ids[p][j])]), float(alt_prob[p][j])) for j in slots])
    return out


def _add_conf(d: dict, conf, prob) -> dict:
    """the conf=True keys of a result dict: "conf" (the kernel's word confidence) and "char_conf" (one probability per character of "text")"""
    d["conf"] = float(conf)
    d["char_conf"] = confidence_from_probs(d["ids"], prob)[0].tolist()
    return d


WIDE_DEFAULT = 8.0   # wide=True: the largest aspect a piece may have (DESIGN.md "Wide words": untuned on documents)


def _wide_arg(wide) -> float:
    """False / None / 0 -> 0.0 (off), True -> WIDE_DEFAULT, a number -> itself"""
    if wide is None or wide is False:
        return 0.0
    if wide is True:
        return WIDE_DEFAULT
    return float(wide)


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _u16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def _lib_check(rc):
    if rc < 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    return rc


TILED_DEFAULT = 128   # tiled=True: the tiles' overlap in pixels (DESIGN.md "Tiled pages": untuned on documents)


def _tiled_arg(tiled) -> int:
    """tiled=None / False / 0 -> 0 (off), True -> TILED_DEFAULT, else the overlap itself (the setter checks it)."""
    if tiled is None or tiled is False:
        return 0
    if tiled is True:
        return TILED_DEFAULT
    if isinstance(tiled, (int, np.integer)):
        return int(tiled)
    raise EngineError(f"tiled must be True, False or an overlap in pixels, got {tiled!r}")


class TilePlan:
    """ttr_tile_plan's answer for one page: ny x nx tiles at origins oy / ox (image pixels) with extents ey / ex on a shared canvas Hc x Wc; the page map is
    H2 x W2.  Tile (ty, tx) is the window [oy[ty], oy[ty] + ey[ty]) x [ox[tx], ox[tx] + ex[tx]); a page's tiles travel in (ty, tx) order."""
    __slots__ = ("ny", "nx", "oy", "ox", "ey", "ex", "Hc", "Wc", "H2", "W2")

    def __init__(self, ny, nx, oy, ox, ey, ex, Hc, Wc, H2, W2):
        self.ny, self.nx, self.oy, self.ox, self.ey, self.ex, self.Hc, self.Wc, self.H2, self.W2 = ny, nx, oy, ox, ey, ex, Hc, Wc, H2, W2

    @property
    def tiles(self) -> int:
        return self.ny * self.nx

    def __repr__(self):
        return f"TilePlan({self.ny} x {self.nx}, oy={self.oy}, ox={self.ox}, canvas={self.Hc} x {self.Wc}, map={self.H2} x {self.W2})"


def tile_plan(h: int, w: int, canvas_size: int = 1024, overlap: int = TILED_DEFAULT, mag_ratio: float = 1.0) -> TilePlan:
    """The tile plan of an h x w page on the host (ttr_tile_plan, no GPU; DESIGN.md "Tiled pages").  Raises EngineError with the rule's message."""
    v = [C.c_int() for _ in range(6)]
    a = [np.zeros(16, np.int32) for _ in range(4)]
    if load().ttr_tile_plan(int(h), int(w), int(canvas_size), int(overlap), float(mag_ratio), C.byref(v[0]), C.byref(v[1]), _i(a[0]), _i(a[1]), _i(a[2]), _i(a[3]),
                            C.byref(v[2]), C.byref(v[3]), C.byref(v[4]), C.byref(v[5])) != 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    ny, nx = v[0].value, v[1].value
    return TilePlan(ny, nx, a[0][:ny].tolist(), a[1][:nx].tolist(), a[2][:ny].tolist(), a[3][:nx].tolist(), v[2].value, v[3].value, v[4].value, v[5].value)


def _stitch_args(tiles, oy, ox, Hc, Wc, H2, W2):
    oy, ox = np.ascontiguousarray(oy, dtype=np.int32).ravel(), np.ascontiguousarray(ox, dtype=np.int32).ravel()
    ny, nx = len(oy), len(ox)
    t = np.ascontiguousarray(tiles, dtype=np.float32)
    if t.ndim == 4 and t.shape[1:] == (int(Hc) // 2, int(Wc) // 2, 2) and ny * nx and t.shape[0] % (ny * nx) == 0:
        t = t.reshape(t.shape[0] // (ny * nx), ny * nx, int(Hc) // 2, int(Wc) // 2, 2)
    elif not (t.ndim == 5 and t.shape[1:] == (ny * nx, int(Hc) // 2, int(Wc) // 2, 2)):
        raise EngineError(f"stitch: tiles must be f32 [pages * {ny * nx}, {int(Hc) // 2}, {int(Wc) // 2}, 2], got {t.shape}")
    pages = t.shape[0]
    if pages < 1 or int(H2) < 1 or int(W2) < 1 or int(H2) > 4096 or int(W2) > 4096:
        raise EngineError("stitch: bad sizes")
    return t, pages, ny, nx, oy, ox, np.zeros((pages, int(H2), int(W2), 2), np.float32)


def stitch_tiles(tiles, oy, ox, Hc: int, Wc: int, H2: int, W2: int):
    """ttr_stitch_tiles: the stitch on the host (no GPU; DESIGN.md "Tiled pages").  tiles f32 [pages * ny * nx, Hc / 2, Wc / 2, 2], a page's tiles in (ty, tx)
    order; oy / ox the origins in image pixels -> f32 [pages, H2, W2, 2].  Raises EngineError for origins the stitch cannot take."""
    t, pages, ny, nx, oy, ox, out = _stitch_args(tiles, oy, ox, Hc, Wc, H2, W2)
    if load().ttr_stitch_tiles(_f(t), pages, ny, nx, _i(oy), _i(ox), int(Hc), int(Wc), int(H2), int(W2), _f(out)) != 0:
        raise EngineError(load().ttr_last_error().decode("latin1"))
    return out


def wide_plan(quad, max_aspect: float):
    """The wide-word plan of one quad (ttr_wide_plan, no GPU; DESIGN.md "Wide words"): 8 floats tl, tr, br, bl -> (n, frame i64 [6]): n pieces (1 = not wide)
    and the frame {X0f, Axf, Bxf, Y0f, Ayf, Byf} in 2^-16 px over 128 n columns x 32 rows."""
    q = np.ascontiguousarray(quad, dtype=np.float32).reshape(8)
    frame = np.zeros(6, np.int64)
    n = _lib_check(load().ttr_wide_plan(_f(q), float(max_aspect), _i64(frame)))
    return int(n), frame


def wide_profile(image, frame, n: int) -> np.ndarray:
    """The contrast profile of a frame on a host image u8 [H, W, 3] (ttr_wide_profile, no GPU) -> u16 [128 n]."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image is [H, W, 3] u8")
    f = np.ascontiguousarray(frame, dtype=np.int64).reshape(6)
    q = np.zeros(128 * max(int(n), 1), np.uint16)
    _lib_check(load().ttr_wide_profile(_u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _i64(f), int(n), _u16(q)))
    return q


def wide_cuts_from_profile(q, n: int) -> np.ndarray:
    """The cuts of a profile u16 [128 n] (ttr_wide_cuts_from_profile, no GPU) -> i32 [17]: c_0 = 0 < ... < c_n = 128 n, -1 beyond n."""
    q = np.ascontiguousarray(q, dtype=np.uint16).ravel()
    if 1 <= int(n) <= 16 and len(q) < 128 * int(n):
        raise ValueError("the profile holds 128 n columns")
    cuts = np.full(17, -1, np.int32)
    _lib_check(load().ttr_wide_cuts_from_profile(_u16(q), int(n), _i(cuts)))
    return cuts


def wide_piece_coef(frame, c0: int, c1: int) -> np.ndarray:
    """The packer row of the piece over columns [c0, c1) of a frame (ttr_wide_piece_coef, no GPU) -> i64 [8] = {1, X0, Ax, Bx, Y0, Ay, By, 0}."""
    f = np.ascontiguousarray(frame, dtype=np.int64).reshape(6)
    row = np.zeros(8, np.int64)
    _lib_check(load().ttr_wide_piece_coef(_i64(f), int(c0), int(c1), _i64(row)))
    return row


def wide_piece_quads(quad, cuts, n: int) -> np.ndarray:
    """The n pieces' quads of a word's quad from its cuts (ttr_wide_piece_quads, no GPU) -> f32 [n, 8]."""
    q = np.ascontiguousarray(quad, dtype=np.float32).reshape(8)
    c = np.ascontiguousarray(cuts, dtype=np.int32).ravel()
    if 1 <= int(n) <= 16 and len(c) < int(n) + 1:
        raise ValueError("cuts holds n + 1 entries")
    out = np.zeros((max(int(n), 1), 8), np.float32)
    _lib_check(load().ttr_wide_piece_quads(_f(q), _i(c), int(n), _f(out)))
    return out[:int(n)]


def _curve_image(image) -> np.ndarray:
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image is [H, W, 3] u8")
    return image


def curve_frame(quad) -> np.ndarray:
    """The curved-word frame of one quad (ttr_curve_frame, no GPU; DESIGN.md "Curved words"): 8 floats tl, tr, br, bl -> i64 [6] = {X0, Ax, Bx, Y0, Ay, By} in
    2^-16 px over 128 columns x 64 rows."""
    q = np.ascontiguousarray(quad, dtype=np.float32).reshape(8)
    frame = np.zeros(6, np.int64)
    _lib_check(load().ttr_curve_frame(_f(q), _i64(frame)))
    return frame


def curve_columns(image, frame, knots=None) -> np.ndarray:
    """The column statistics of a frame on a host image u8 [H, W, 3] (ttr_curve_columns, no GPU) -> i32 [4, 128] = G | M | first | last; knots=None walks
    the frame's own columns (pass 1), a knot table i64 [9, 4] the columns of its band (pass 2)."""
    image = _curve_image(image)
    f = np.ascontiguousarray(frame, dtype=np.int64).reshape(6)
    t = None if knots is None else np.ascontiguousarray(knots, dtype=np.int64).reshape(36)
    stats = np.zeros((4, 128), np.int32)
    _lib_check(load().ttr_curve_columns(_u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _i64(f), None if t is None else _i64(t), _i(stats)))
    return stats


def curve_knots(image, frame) -> dict:
    """The whole rule on one frame (ttr_curve_knots, no GPU) -> {"flag", "hb" i32 [2], "spine" i32 [2, 9], "knots" i64 [9, 4], "knots1" i64 [9, 4]}."""
    image = _curve_image(image)
    f = np.ascontiguousarray(frame, dtype=np.int64).reshape(6)
    flag, hb, spine = np.zeros(1, np.int32), np.zeros(2, np.int32), np.zeros((2, 9), np.int32)
    knots, knots1 = np.zeros((9, 4), np.int64), np.zeros((9, 4), np.int64)
    _lib_check(load().ttr_curve_knots(_u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _i64(f), _i(flag), _i(hb), _i(spine), _i64(knots), _i64(knots1)))
    return {"flag": int(flag[0]), "hb": hb, "spine": spine, "knots": knots, "knots1": knots1}


def curve_crop(image, knots) -> np.ndarray:
    """The crop of a knot table i64 [9, 4] on a host image (ttr_curve_crop, no GPU) -> u8 [32, 128, 3]."""
    image = _curve_image(image)
    t = np.ascontiguousarray(knots, dtype=np.int64).reshape(36)
    crop = np.zeros((32, 128, 3), np.uint8)
    _lib_check(load().ttr_curve_crop(_u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _i64(t), _u8(crop)))
    return crop


def curve_outline(quad, flag: int, knots) -> np.ndarray:
    """The outline of a word (ttr_curve_outline, no GPU) -> f32 [18, 2]: the top edge left to right, then the bottom edge right to left."""
    q = np.ascontiguousarray(quad, dtype=np.float32).reshape(8)
    t = np.ascontiguousarray(knots, dtype=np.int64).reshape(36)
    out = np.zeros((18, 2), np.float32)
    _lib_check(load().ttr_curve_outline(_f(q), int(flag), _i64(t), _f(out)))
    return out


def _quad_pairs(q8) -> list:
    """8 floats tl, tr, br, bl -> [[x, y], ...] (4 pairs)"""
    q = [float(v) for v in q8]
    return [q[0:2], q[2:4], q[4:6], q[6:8]]


TABLES_MIN_LEN, TABLES_INK = 48, 128   # what tables=True means (DESIGN.md "Tables": neither value has been tuned on documents)


def _layer_arg(name, value, fields, defaults):
    """a page layer's setting as its tuple of ints: False / None / 0 -> off (0, then the other defaults); True -> the defaults; a tuple or list of as many values,
    or a bare first value, otherwise"""
    if value is None or value is False or (isinstance(value, int) and not isinstance(value, bool) and value == 0):
        return (0,) + tuple(defaults[1:])
    if value is True:
        return tuple(defaults)
    if isinstance(value, (tuple, list)) and len(value) == len(defaults):
        return tuple(int(v) for v in value)
    if isinstance(value, int):
        return (int(value),) + tuple(defaults[1:])
    raise EngineError(f"{name} must be False, True or ({fields})")


_tables_arg = functools.partial(_layer_arg, "tables", fields="min_len, ink", defaults=(TABLES_MIN_LEN, TABLES_INK))


def _page_image(image, row_stride=0):
    """the opening of the one-page calls: a host image u8 [H, W, 3] (row_stride: the bytes from row to row of a view into a wider buffer; 0 = packed, copied
    when it is not) -> the array, H, W and the stride in bytes"""
    image = np.asarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise RuntimeError("Input array should have 3 dimensions")
    if not row_stride:
        image = np.ascontiguousarray(image)
    return image, image.shape[0], image.shape[1], int(row_stride) or image.shape[1] * 3


def _page_entry(form, layer, head, ink, tail=(), engine=None):
    """The library call behind a layer's three one-page wrappers, and its parameter tuple: form "from_page" (the host rule; ink = the threshold), "from_page_ink"
    (the host rule under the local ink rule; ink = local_ink, True or (radius, drop, polarity), which goes behind the layer's other parameters) or "page" (the
    engine's stage call).  -> fn(image..., params..., outputs...), params"""
    sym = getattr(engine.lib if engine else load(), f"ttr_{layer}_{form}")
    params = head + tail + _local_ink_arg(ink) if form == "from_page_ink" else head + (ink,) + tail
    if engine:
        return (lambda *a: engine._check(sym(engine.h, *a))), params
    return (lambda *a: _lib_check(sym(*a))), params


def _tables_call(fn, params, image, quads, row_stride=0):
    """the shared body of tables_from_page and Engine.tables_page: fn(image..., params..., quads, outputs...) -> the dict both return"""
    image, h, w, stride = _page_image(image, row_stride)
    q = np.zeros((0, 8), np.float32) if quads is None else np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    nq, m = len(q), max(len(q), 1)
    mode, counts = np.zeros(1, np.int32), np.zeros(6, np.int32)
    rul, tab, lin, cel = np.zeros((512, 6), np.int32), np.zeros((32, 8), np.int32), np.zeros(32 * 130, np.int32), np.zeros((1024, 9), np.int32)
    it, ic = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
    fn(_u8(image), h, w, stride, *[int(v) for v in params], _f(q), nq, _i(mode), _i(counts), _i(rul), _i(tab), _i(lin), _i(cel), _i(it), _i(ic))
    return {"mode": int(mode[0]), "rulings": rul[:counts[0]].copy(), "tables": tab[:counts[1]].copy(), "lines": lin[:counts[3]].copy(), "cells": cel[:counts[2]].copy(),
            "item_table": it[:nq].copy(), "item_cell": ic[:nq].copy(), "runs": (int(counts[4]), int(counts[5]))}


MARKS_MIN_SIDE, MARKS_MAX_SIDE, MARKS_FILL, MARKS_INK = 10, 64, 24, 128   # what marks=True means (DESIGN.md "Selection marks": none of them has been tuned on documents)
MARK_FIELDS = ("x0", "y0", "x1", "y1", "ix0", "iy0", "ix1", "iy1", "inked", "area", "state", "label")


_marks_arg = functools.partial(_layer_arg, "marks", fields="min_side, max_side, fill, ink", defaults=(MARKS_MIN_SIDE, MARKS_MAX_SIDE, MARKS_FILL, MARKS_INK))


def _marks_call(fn, params, image, quads, row_stride=0):
    """the shared body of marks_from_page and Engine.marks_page: fn(image..., params..., quads, outputs...) -> the dict both return"""
    image, h, w, stride = _page_image(image, row_stride)
    q = np.zeros((0, 8), np.float32) if quads is None else np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    nq = len(q)
    mode, counts, marks, im = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros((512, 12), np.int32), np.full(max(nq, 1), -1, np.int32)
    fn(_u8(image), h, w, stride, *[int(v) for v in params], _f(q), nq, _i(mode), _i(counts), _i(marks), _i(im))
    return {"mode": int(mode[0]), "marks": marks[:counts[0]].copy(), "item_mark": im[:nq].copy(), "corners": int(counts[1]), "kept": int(counts[2])}


def marks_from_page(image, quads=None, min_side: int = MARKS_MIN_SIDE, max_side: int = MARKS_MAX_SIDE, fill: int = MARKS_FILL, ink: int = MARKS_INK,
                    row_stride: int = 0) -> dict:
    """The selection-marks rule on the host (ttr_marks_from_page, no GPU; DESIGN.md "Selection marks"): a host image u8 [H, W, 3] (row_stride: the bytes from
    row to row of a view into a wider buffer) and quads f32 [nq, 8] -> {"mode" (1, or -6 beyond 512 marks), "marks" i32 [n, 12] (MARK_FIELDS), "item_mark" i32
    [nq], "corners" (examined), "kept" (candidates, beyond 512 on a page of mode -6)}."""
    return _marks_call(*_page_entry("from_page", "marks", (min_side, max_side, fill), ink), image=image, quads=quads, row_stride=row_stride)


def marks_from_page_ink(image, quads=None, min_side: int = MARKS_MIN_SIDE, max_side: int = MARKS_MAX_SIDE, fill: int = MARKS_FILL, local_ink=True,
                        row_stride: int = 0) -> dict:
    """marks_from_page under the local ink rule (ttr_marks_from_page_ink): local_ink = True or (radius, drop, polarity) in the place of ink"""
    return _marks_call(*_page_entry("from_page_ink", "marks", (min_side, max_side, fill), local_ink), image=image, quads=quads, row_stride=row_stride)


def mark_dicts(marks, texts=None) -> list:
    """mark records i32 [n, 12] -> [{"box", "interior", "selected", "fill", "label", "text"}] (text: the label's, "" without one or without texts)"""
    out = []
    for m in np.asarray(marks, np.int32).reshape(-1, 12):
        lab = int(m[11])
        out.append({"box": [int(v) for v in m[0:4]], "interior": [int(v) for v in m[4:8]], "selected": bool(m[10]), "fill": float(m[8]) / float(m[9]),
                    "label": lab, "text": texts[lab] if texts is not None and lab >= 0 else ""})
    return out


BARCODES_MIN_LINES, BARCODES_INK, BARCODES_SYMBOLOGIES = 8, 128, 3   # what barcodes=True means (DESIGN.md "Barcodes": none of them has been tuned on documents)
BARCODE_FIELDS = ("x0", "y0", "x1", "y1", "symbology", "dir", "lines", "module64", "flags", "len")   # then two zeros and 48 bytes of text
BARCODE_SYMBOLOGIES = {1: "code128", 2: "code39"}
BARCODE_DIRECTIONS = ("left-to-right", "top-to-bottom", "right-to-left", "bottom-to-top")


_barcodes_arg = functools.partial(_layer_arg, "barcodes", fields="min_lines, ink, symbologies", defaults=(BARCODES_MIN_LINES, BARCODES_INK, BARCODES_SYMBOLOGIES))


def _barcodes_call(fn, params, image, quads, row_stride=0, raw=False):
    """the shared body of barcodes_from_page and Engine.barcodes_page: fn(image..., params..., quads, outputs...) -> the dict both return"""
    image, h, w, stride = _page_image(image, row_stride)
    q = np.zeros((0, 8), np.float32) if quads is None else np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    nq, lines = len(q), h + w
    mode, counts, recs, ib = np.zeros(1, np.int32), np.zeros(6, np.int32), np.zeros((64, 24), np.int32), np.full(max(nq, 1), -1, np.int32)
    extra = [np.zeros((lines, 2, 8, 20), np.int32), np.zeros((lines, 2, 4), np.int32)] if raw else []
    fn(_u8(image), h, w, stride, *[int(v) for v in params], _f(q), nq, _i(mode), _i(counts), _i(recs), _i(ib), *[_i(a) for a in extra])
    out = {"mode": int(mode[0]), "records": recs[:counts[0]].copy(), "item_barcode": ib[:nq].copy(), "counts": [int(v) for v in counts]}
    if raw:
        out["hits"], out["line_counts"] = extra
    out["barcodes"] = barcode_dicts(out["records"])
    return out


def barcodes_from_page(image, quads=None, min_lines: int = BARCODES_MIN_LINES, ink: int = BARCODES_INK, symbologies: int = BARCODES_SYMBOLOGIES, row_stride: int = 0,
                       raw: bool = False) -> dict:
    """The barcode rule on the host (ttr_barcodes_from_page, no GPU; DESIGN.md "Barcodes"): a host image u8 [H, W, 3] (row_stride: the bytes from row to row of
    a view into a wider buffer) and quads f32 [nq, 8] -> {"mode" (1, or -7 beyond 64 barcodes), "records" i32 [n, 24] (BARCODE_FIELDS, then the text),
    "barcodes" (barcode_dicts), "item_barcode" i32 [nq], "counts" [6] = barcodes, candidates examined, start patterns matched, hits kept, hits dropped, chains
    below min_lines}; raw adds "hits" i32 [H + W, 2, 8, 20] and "line_counts" i32 [H + W, 2, 4], the lines' raw hits."""
    fn, params = _page_entry("from_page", "barcodes", (min_lines,), ink, (symbologies,))
    return _barcodes_call(fn if raw else (lambda *a: fn(*a, None, None)), params, image, quads, row_stride, raw)


def barcodes_from_page_ink(image, quads=None, min_lines: int = BARCODES_MIN_LINES, symbologies: int = BARCODES_SYMBOLOGIES, local_ink=True, row_stride: int = 0) -> dict:
    """barcodes_from_page under the local ink rule (ttr_barcodes_from_page_ink): local_ink = True or (radius, drop, polarity) in the place of ink"""
    return _barcodes_call(*_page_entry("from_page_ink", "barcodes", (min_lines,), local_ink, (symbologies,)), image=image, quads=quads, row_stride=row_stride)


def barcode_dicts(records) -> list:
    """barcode records i32 [n, 24] -> [{"box", "symbology", "direction", "text", "data", "lines", "module", "gs1", "flags"}] (text: the data as latin-1)"""
    out = []
    for r in np.ascontiguousarray(records, np.int32).reshape(-1, 24):
        data = r[12:].tobytes()[:int(r[9])]
        out.append({"box": [int(v) for v in r[0:4]], "symbology": BARCODE_SYMBOLOGIES.get(int(r[4]), "?"), "direction": int(r[5]), "text": data.decode("latin1"),
                    "data": data, "lines": int(r[6]), "module": float(r[7]) / 64.0, "gs1": bool(r[8] & 1), "flags": int(r[8])})
    return out


DESKEW_MAX_SLOPE, DESKEW_GAIN, DESKEW_INK = 64, 288, 128   # what deskew=True means (DESIGN.md "Deskew": none of them has been tuned on documents)


class Skew(C.Structure):
    """ttr_skew: one page's skew record"""
    _fields_ = [("slope", C.c_int32), ("found", C.c_int32), ("C", C.c_int32), ("S", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("mode", C.c_int32),
                ("reserved", C.c_int32), ("score0", C.c_uint64), ("score_found", C.c_uint64)]


_deskew_arg = functools.partial(_layer_arg, "deskew", fields="max_slope, gain, ink", defaults=(DESKEW_MAX_SLOPE, DESKEW_GAIN, DESKEW_INK))


def _skew_dict(rec) -> dict:
    """a ttr_skew as the dict PageResult.skew carries: the record's fields and degrees = atan(slope / 512)"""
    d = {k: int(getattr(rec, k)) for k in ("slope", "found", "C", "S", "w", "h", "mode", "score0", "score_found")}
    d["degrees"] = math.degrees(math.atan(d["slope"] / 512.0))
    return d


def skew_to_page(skew: dict, points) -> np.ndarray:
    """the map back of a skew record (ttr_skew_to_page; DESIGN.md "Deskew", step 6): points [..., 2] of the upright page -> the caller's page, float32 of the
    double map.  skew: a dict with "C", "S", "w", "h" (PageResult.skew is one)."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    if p.shape[-1:] != (2,):
        raise EngineError("to_page takes points [..., 2]")
    rec = Skew(C=int(skew["C"]), S=int(skew["S"]), w=int(skew["w"]), h=int(skew["h"]))
    out = np.zeros_like(p)
    _lib_check(load().ttr_skew_to_page(C.addressof(rec), _f(p), p.size // 2, _f(out)))
    return out


def _deskew_call(fn, params, image, row_stride=0):
    """the shared body of deskew_from_page and Engine.deskew_page: fn(image..., params..., outputs...) (params: max_slope first) -> the dict both return"""
    image, h, w, stride = _page_image(image, row_stride)
    out, rec, scores = np.zeros((h, w, 3), np.uint8), Skew(), np.zeros(2 * max(int(params[0]), 0) + 1, np.uint64)
    fn(_u8(image), h, w, stride, *[int(v) for v in params], _u8(out), C.addressof(rec), scores.ctypes.data_as(C.POINTER(C.c_uint64)))
    return {"image": out, "skew": _skew_dict(rec), "scores": scores}


def deskew_from_page(image, max_slope: int = DESKEW_MAX_SLOPE, gain: int = DESKEW_GAIN, ink: int = DESKEW_INK, row_stride: int = 0) -> dict:
    """The deskew rule on the host (ttr_deskew_from_page, no GPU; DESIGN.md "Deskew"): a host image u8 [H, W, 3] (row_stride: the bytes from row to row of a view
    into a wider buffer) -> {"image" u8 [H, W, 3] the upright page, "skew" the record as PageResult.skew carries it, "scores" u64 [2 max_slope + 1]}."""
    return _deskew_call(*_page_entry("from_page", "deskew", (max_slope, gain), ink), image=image, row_stride=row_stride)


LOCAL_INK_RADIUS, LOCAL_INK_DROP, LOCAL_INK_POLARITY = 16, 38, 2   # what local_ink=True means (DESIGN.md "Local ink": none of them has been tuned on documents)
INK_DARK, INK_LIGHT, INK_AUTO = 0, 1, 2


class Ink(C.Structure):
    """ttr_ink: one page's local-ink record"""
    _fields_ = [("radius", C.c_int32), ("drop", C.c_int32), ("polarity", C.c_int32), ("inverted", C.c_int32), ("sum", C.c_uint64), ("w", C.c_int32), ("h", C.c_int32)]


_local_ink_arg = functools.partial(_layer_arg, "local_ink", fields="radius, drop, polarity", defaults=(LOCAL_INK_RADIUS, LOCAL_INK_DROP, LOCAL_INK_POLARITY))


def _ink_dict(rec) -> dict:
    """a ttr_ink as the dict PageResult.ink carries"""
    return {k: int(getattr(rec, k)) for k in ("radius", "drop", "polarity", "inverted", "sum", "w", "h")}


def _ink_call(fn, image, radius, drop, polarity, row_stride=0):
    """the shared body of ink_from_page and Engine.ink_page: fn(image..., outputs...) -> the dict both return"""
    image, h, w, stride = _page_image(image, row_stride)
    bits, bitsT, rec = np.zeros((h, (w + 63) // 64), np.uint64), np.zeros((w, (h + 63) // 64), np.uint64), Ink()
    u64 = C.POINTER(C.c_uint64)
    fn(_u8(image), h, w, stride, int(radius), int(drop), int(polarity), bits.ctypes.data_as(u64), bitsT.ctypes.data_as(u64), C.addressof(rec))
    return {"bits": bits, "bitsT": bitsT, "ink": _ink_dict(rec)}


def ink_from_page(image, radius: int = LOCAL_INK_RADIUS, drop: int = LOCAL_INK_DROP, polarity: int = LOCAL_INK_POLARITY, row_stride: int = 0) -> dict:
    """The local ink rule on the host (ttr_ink_from_page, no GPU; DESIGN.md "Local ink"): a host image u8 [H, W, 3] (row_stride: the bytes from row to row of a
    view into a wider buffer) -> {"bits" u64 [H, ceil(W / 64)] (bit x % 64 of word x / 64), "bitsT" u64 [W, ceil(H / 64)] the same bits along y, "ink" the
    record as PageResult.ink carries it}."""
    lib = load()

    def fn(*a):
        _lib_check(lib.ttr_ink_from_page(*a))
    return _ink_call(fn, image, radius, drop, polarity, row_stride)


def tables_from_page_ink(image, quads=None, min_len: int = TABLES_MIN_LEN, local_ink=True, row_stride: int = 0) -> dict:
    """tables_from_page under the local ink rule (ttr_tables_from_page_ink): local_ink = True or (radius, drop, polarity) in the place of ink"""
    return _tables_call(*_page_entry("from_page_ink", "tables", (min_len,), local_ink), image=image, quads=quads, row_stride=row_stride)


def deskew_from_page_ink(image, max_slope: int = DESKEW_MAX_SLOPE, gain: int = DESKEW_GAIN, local_ink=True, row_stride: int = 0) -> dict:
    """deskew_from_page under the local ink rule (ttr_deskew_from_page_ink): local_ink = True or (radius, drop, polarity) in the place of ink"""
    return _deskew_call(*_page_entry("from_page_ink", "deskew", (max_slope, gain), local_ink), image=image, row_stride=row_stride)


def table_line_lists(tables, lines) -> list:
    """the flat line values of a result split per table: [(row lines i32 [rows + 1], column lines i32 [cols + 1]), ...] in doubled px"""
    out, k = [], 0
    for t in np.asarray(tables).reshape(-1, 8):
        r, c = int(t[4]) + 1, int(t[5]) + 1
        out.append((np.asarray(lines[k:k + r]), np.asarray(lines[k + r:k + r + c])))
        k += r + c
    return out


def tables_from_page(image, quads=None, min_len: int = TABLES_MIN_LEN, ink: int = TABLES_INK, row_stride: int = 0) -> dict:
    """The tables rule on the host (ttr_tables_from_page, no GPU; DESIGN.md "Tables"): a host image u8 [H, W, 3] (row_stride: the bytes from row to row of a
    view into a wider buffer) and quads f32 [nq, 8] -> {"mode", "rulings" i32 [nr, 6], "tables" i32 [nt, 8], "lines" i32 (per table its row lines, then its
    column lines, doubled px), "cells" i32 [nc, 9], "item_table" i32 [nq], "item_cell" i32 [nq], "runs": (horizontal, vertical) run counts, 0 for a page beyond a cap}."""
    return _tables_call(*_page_entry("from_page", "tables", (min_len,), ink), image=image, quads=quads, row_stride=row_stride)


class PageResult(collections.abc.Sequence):
    """One page's words as the list of {"text", "bbox", "ids"} dicts pytuatara.image_to_data returns, materialised on access:
    the batch hand-over keeps the arrays the C ABI filled (`texts`, `bbox` f32 [n,4], `ids` i32 [n,26]; `quad` f32 [n,8] in the
    rectified crop mode, else None; `conf` f32 [n] and `prob` f32 [n,26] always) and builds dicts only for the items a caller touches.
    with_conf: the dicts carry "conf" and "char_conf" too (DESIGN.md "Recognition confidence").  Word orientation (orient != 0; DESIGN.md
    "Word orientation"): `orient` i32 [n] the chosen turns 0..3 (dicts gain "orient" in degrees), `orient_conf` f32 [n, K] every candidate's
    conf in ascending turn order, `page_orient` the page's turn; None / None / 0 when orientation is off.  Text lines (lines=True; DESIGN.md
    "Text lines"): `line` / `word` i32 [n] (dicts gain "line" and "word"), `order` i32 [n] the items in reading order, `line_first` i32
    [n_lines + 1] the lines' offsets into it, `line_bbox` f32 [n_lines, 4]; `lines` the list of {"text", "bbox", "items"} in reading order and
    `text` the page's text (words joined by ' ', lines by '\\n'); line is None, lines [] and text "" when lines are off.  Character boxes
    (chars=True; DESIGN.md "Character boxes"): `char_first` i32 [n + 1] the items' offsets into `char_quad` f32 [total, 8] and `char_bbox`
    f32 [total, 4], `char_cuts` i32 [n, 27], `char_mode` i32 [n], `char_profile` u8 [n, 128], `word_quad` f32 [n, 8] the words' own quads
    in every crop mode; dicts gain "chars", a list of {"char", "quad", "bbox"}; all None when chars are off.  Text blocks (blocks=True;
    DESIGN.md "Text blocks"): `block` i32 [n] each item's block (dicts gain "block"), `line_block` / `line_pos` i32 [n_lines] each line's block
    in reading order and its position in it, `block_order` i32 [n_lines] the lines in block reading order, `block_first` i32 [n_blocks + 1],
    `block_bbox` f32 [n_blocks, 4], `block_mode` (1: ordered by the precedence relation, 0: more than 512 blocks, by key alone); `blocks` the
    list of {"text", "bbox", "lines"} in reading order and `text_blocks` the page read block after block (lines joined by '\\n', blocks by a
    blank line); block is None, blocks [] and text_blocks "" when blocks are off.  Character alternatives (Engine.set_alternatives(K); DESIGN.md
    "Character alternatives"): `alt_ids` i32 [n, 26, K] the K best allowed classes of every position (-1 = none; slot 0 is `ids`) and `alt_prob` f32
    [n, 26, K] their probabilities (slot 0 is `prob`); dicts gain "alternatives", one list per character of "text" holding (char, prob) over that
    position's character options in rank order; nbest(i, m) reads item i's m likeliest whole words; both None when alternatives are off.  Lexicon
    matching (Engine.set_lexicon(words, m); DESIGN.md "Lexicon matching"): `lex_idx` i32 [n, M] the M best entries of the word list by (logp descending,
    index ascending), -1 = none, and `lex_logp` f32 [n, M] their log-probabilities (-inf = none); dicts gain "lexicon", [(word, prob), ...] with
    prob = exp(logp); both None when no lexicon is set.  Patterns in best mode (Engine.set_pattern(p, best=True); DESIGN.md "Patterns"): `pattern_logp` f32 [n]
    the log-probability of every item's reading, -inf for an item without a pattern (dicts gain "pattern_logp"); None in greedy mode, without a pattern, and for a page without items.  Wide words (Engine.set_wide(a); DESIGN.md "Wide words"): `piece_first` i32 [n + 1] the items' offsets
    into `piece_ids` i32 [P, 26], `piece_prob` f32 [P, 26], `piece_conf` f32 [P] and `piece_quad` f32 [P, 8] (an item that is not wide owns one piece, itself),
    `piece_cuts` i32 [n, 17] each item's cuts in columns of its frame; dicts gain "pieces", a list of {"text", "conf", "quad"}; all None when wide is off.
    Curved words (Engine.set_curved(True); DESIGN.md "Curved words"): `curved` i32 [n] (1 = the item's crop was straightened along its spine), `outline` f32
    [n, 18, 2] (the top edge left to right, then the bottom edge right to left) and `spine_knots` i64 [n, 9, 4] the knot tables; dicts gain "curved" and
    "outline"; all None when curved is off.  Tiled pages (Engine.set_tiled(O); DESIGN.md "Tiled pages"): `tiles` = the tiles the page's detector ran as,
    0 when tiling is off.  Tables (Engine.set_tables; DESIGN.md "Tables"): `table_mode` (1, or -(step) of the cap the page overflowed; 0 = off), `rulings` i32
    [nr, 6] (dir, x0, y0, x1, y1, table), `table_rects` i32 [nt, 8] (box, rows, cols, first cell, cell count), `table_lines` i32 (doubled px), `cells` i32
    [nc, 9] (table, row, col, rowspan, colspan, box), `item_table` / `item_cell` i32 [n] (dicts gain "table" and "cell", -1 = in no cell), `cell_texts`;
    `tables` the list of {"bbox", "rows", "cols", "cells": [{"row", "col", "rowspan", "colspan", "bbox", "items", "text"}]} and table_grid(t) its rows x cols
    strings; rulings is None, tables [] when tables are off and for a page without items.  Deskew (Engine.set_deskew; DESIGN.md "Deskew"): `skew` = the page's
    record {"slope", "found", "C", "S", "w", "h", "mode", "score0", "score_found", "degrees"} or None when the layer is off; every coordinate of the result is
    in the upright page's frame, to_page(points) maps points to the caller's page and every dict gains "quad_page".  Local ink (Engine.set_local_ink; DESIGN.md
    "Local ink"): `ink` = the page's record {"radius", "drop", "polarity", "inverted", "sum", "w", "h"} - the tables pass's when tables ran, else the deskew
    pass's - or None when no pass of the page ran under it.  Selection marks (Engine.set_marks; DESIGN.md "Selection marks"): `mark_mode` (1, or -6 beyond 512
    marks; 0 = off), `mark_recs` i32 [n, 12] (MARK_FIELDS) and `item_mark` i32 [items], None when off; `marks` the list of {"box", "interior", "selected",
    "fill", "label", "text"}; every dict gains "mark"; a page without items has its marks too."""
    __slots__ = ("skew", "quad_page", "ink", "mark_mode", "mark_recs", "item_mark", "barcode_mode", "barcode_recs", "item_barcode",
                 "table_mode", "rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell", "cell_texts",
                 "texts", "bbox", "ids", "quad", "conf", "prob", "with_conf", "orient", "orient_conf", "page_orient",
                 "line", "word", "order", "line_first", "line_bbox",
                 "char_first", "char_quad", "char_bbox", "char_cuts", "char_mode", "char_profile", "word_quad",
                 "block", "line_block", "line_pos", "block_order", "block_first", "block_bbox", "block_mode", "alt_ids", "alt_prob",
                 "lex_idx", "lex_logp", "lex_words", "lex_edits", "lex_band", "pattern_logp", "piece_first", "piece_ids", "piece_prob", "piece_conf", "piece_quad", "piece_cuts",
                 "curved", "outline", "spine_knots", "tiles")

    def __init__(self, texts, bbox, ids, quad=None, conf=None, prob=None, with_conf=False, orient=None, orient_conf=None, page_orient=0,
                 line=None, word=None, order=None, line_first=None, line_bbox=None,
                 char_first=None, char_quad=None, char_bbox=None, char_cuts=None, char_mode=None, char_profile=None, word_quad=None,
                 block=None, line_block=None, line_pos=None, block_order=None, block_first=None, block_bbox=None, block_mode=0,
                 alt_ids=None, alt_prob=None, lex_idx=None, lex_logp=None, lex_words=None, pattern_logp=None,
                 piece_first=None, piece_ids=None, piece_prob=None, piece_conf=None, piece_quad=None, piece_cuts=None,
                 curved=None, outline=None, spine_knots=None, lex_edits=None, lex_band=-1, tiles=0,
                 table_mode=0, rulings=None, table_rects=None, table_lines=None, cells=None, item_table=None, item_cell=None, cell_texts=None, skew=None, quad_page=None, ink=None,
                 mark_mode=0, mark_recs=None, item_mark=None, barcode_mode=0, barcode_recs=None, item_barcode=None):
        self.tiles = tiles
        # barcodes (Engine.set_barcodes; DESIGN.md "Barcodes"): barcode_mode 1, or -7 beyond 64 barcodes, 0 = off; barcode_recs i32 [n, 24] (BARCODE_FIELDS, then
        # the text), in the upright page's frame under deskew; item_barcode i32 [items] the barcode every item's centre lies in (-1 = none); None when off
        self.barcode_mode, self.barcode_recs, self.item_barcode = barcode_mode, barcode_recs, item_barcode
        # selection marks (Engine.set_marks; DESIGN.md "Selection marks"): mark_mode 1, or -6 beyond 512 marks, 0 = off; mark_recs i32 [n, 12] (MARK_FIELDS), in
        # the upright page's frame under deskew; item_mark i32 [items] the mark every item's centre lies in (-1 = none); None when marks are off
        self.mark_mode, self.mark_recs, self.item_mark = mark_mode, mark_recs, item_mark
        self.ink = ink
        self.skew, self.quad_page = skew, quad_page     # quad_page f32 [n, 8]: every quad on the caller's page (ttr_result_to_page), None without deskew or quads
        self.table_mode, self.rulings, self.table_rects, self.table_lines, self.cells = table_mode, rulings, table_rects, table_lines, cells
        self.item_table, self.item_cell, self.cell_texts = item_table, item_cell, cell_texts
        self.lex_edits, self.lex_band = lex_edits, lex_band
        self.curved, self.outline, self.spine_knots = curved, outline, spine_knots
        self.piece_first, self.piece_ids, self.piece_prob = piece_first, piece_ids, piece_prob
        self.piece_conf, self.piece_quad, self.piece_cuts = piece_conf, piece_quad, piece_cuts
        self.alt_ids, self.alt_prob = alt_ids, alt_prob
        self.lex_idx, self.lex_logp, self.lex_words = lex_idx, lex_logp, lex_words
        self.pattern_logp = pattern_logp
        self.block, self.line_block, self.line_pos, self.block_order = block, line_block, line_pos, block_order
        self.block_first, self.block_bbox, self.block_mode = block_first, block_bbox, block_mode
        self.char_first, self.char_quad, self.char_bbox = char_first, char_quad, char_bbox
        self.char_cuts, self.char_mode, self.char_profile, self.word_quad = char_cuts, char_mode, char_profile, word_quad
        self.line, self.word, self.order, self.line_first, self.line_bbox = line, word, order, line_first, line_bbox
        self.texts, self.bbox, self.ids, self.quad = texts, bbox, ids, quad
        n = len(texts)
        self.conf = conf if conf is not None else np.zeros(n, np.float32)
        self.prob = prob if prob is not None else np.zeros((n, 26), np.float32)
        self.with_conf = with_conf
        self.orient, self.orient_conf, self.page_orient = orient, orient_conf, page_orient

    def __len__(self):
        return len(self.texts)

    def __getitem__(self, j):
        if isinstance(j, slice):
            return [self[i] for i in range(*j.indices(len(self)))]
        if j < 0:
            j += len(self)
        if not 0 <= j < len(self):
            raise IndexError(j)
        d = {"text": self.texts[j], "bbox": self.bbox[j].tolist(), "ids": self.ids[j].tolist()}
        if self.quad is not None:
            d["quad"] = _quad_pairs(self.quad[j])
        if self.with_conf:
            _add_conf(d, self.conf[j], self.prob[j])
        if self.orient is not None:
            d["orient"] = 90 * int(self.orient[j])
        if self.line is not None:
            d["line"], d["word"] = int(self.line[j]), int(self.word[j])
        if self.block is not None:
            d["block"] = int(self.block[j])
        if self.char_first is not None:
            a, b = int(self.char_first[j]), int(self.char_first[j + 1])
            text = self.texts[j]
            d["chars"] = [{"char": text[k - a] if k - a < len(text) else "", "quad": _quad_pairs(self.char_quad[k]), "bbox": self.char_bbox[k].tolist()}
                          for k in range(a, b)]
        if self.alt_ids is not None:
            d["alternatives"] = char_alternatives(self.alt_ids[j], self.alt_prob[j])
        if self.lex_idx is not None:
            d["lexicon"] = lexicon_matches(self.lex_words, self.lex_idx[j], self.lex_logp[j])
            if self.lex_edits is not None:      # fuzzy alignment: each match's edits, beside the (word, prob) pairs
                d["lexicon_edits"] = [int(e) for i, e in zip(self.lex_idx[j], self.lex_edits[j]) if int(i) >= 0]
        if self.pattern_logp is not None:
            d["pattern_logp"] = float(self.pattern_logp[j])
        if self.piece_first is not None:
            d["pieces"] = self.pieces(j)
        if self.curved is not None:
            d["curved"], d["outline"] = int(self.curved[j]), self.outline[j].tolist()
        if self.item_table is not None:
            d["table"], d["cell"] = int(self.item_table[j]), int(self.item_cell[j])
        if self.item_mark is not None:
            d["mark"] = int(self.item_mark[j])
        if self.item_barcode is not None:
            d["barcode"] = int(self.item_barcode[j])
        if self.quad_page is not None:
            d["quad_page"] = _quad_pairs(self.quad_page[j])
        return d

    @property
    def marks(self) -> list:
        """the page's selection marks in (y, x) order: {"box": [x0, y0, x1, y1], "interior", "selected", "fill" (inked / area), "label" (an item or -1), "text"
        (the label's)}; [] when marks are off"""
        return [] if self.mark_recs is None else mark_dicts(self.mark_recs, self.texts)

    @property
    def barcodes(self) -> list:
        """the page's barcodes in (y0, x0, dir) order: {"box": [x0, y0, x1, y1], "symbology" ("code128" | "code39"), "direction" (0 left to right, 1 top to
        bottom, 2 right to left, 3 bottom to top), "text", "data" (bytes), "lines", "module" (px), "gs1", "flags"}; [] when barcodes are off"""
        return [] if self.barcode_recs is None else barcode_dicts(self.barcode_recs)

    def to_page(self, points) -> np.ndarray:
        """points [..., 2] of this result's frame -> the caller's page (the identity when deskew is off), float32"""
        if self.skew is None:
            return np.asarray(points, dtype=np.float32).copy()
        return skew_to_page(self.skew, points)

    @property
    def tables(self) -> list:
        """the page's tables in order: {"bbox": [x0, y0, x1, y1], "rows", "cols", "cells": [{"row", "col", "rowspan", "colspan", "bbox", "items", "text"}]}"""
        if self.table_rects is None:
            return []
        out = []
        for t in self.table_rects:
            cells = []
            for c in range(int(t[6]), int(t[6]) + int(t[7])):
                q = self.cells[c]
                cells.append({"row": int(q[1]), "col": int(q[2]), "rowspan": int(q[3]), "colspan": int(q[4]), "bbox": [int(v) for v in q[5:9]],
                              "items": [int(i) for i in np.nonzero(self.item_cell == c)[0]], "text": self.cell_texts[c]})
            out.append({"bbox": [int(v) for v in t[:4]], "rows": int(t[4]), "cols": int(t[5]), "cells": cells})
        return out

    def table_grid(self, t: int) -> list:
        """table t as rows x cols strings: a merged cell's text at its first base cell, "" at its others"""
        if self.table_rects is None or not 0 <= t < len(self.table_rects):
            raise EngineError("table_grid: no such table")
        T = self.table_rects[t]
        grid = [["" for _ in range(int(T[5]))] for _ in range(int(T[4]))]
        for c in range(int(T[6]), int(T[6]) + int(T[7])):
            grid[int(self.cells[c][1])][int(self.cells[c][2])] = self.cell_texts[c]
        return grid

    def pieces(self, j: int) -> list:
        """item j's pieces in order: [{"text", "conf", "quad"}, ...] (one, the item itself, when it is not wide)"""
        if self.piece_first is None:
            raise EngineError("pieces: the result carries no pieces (Engine.set_wide)")
        a, b = int(self.piece_first[j]), int(self.piece_first[j + 1])
        return [{"text": decode_ids(self.piece_ids[k]), "conf": float(self.piece_conf[k]), "quad": _quad_pairs(self.piece_quad[k])} for k in range(a, b)]

    def nbest(self, i: int, m: int) -> list:
        """item i's m likeliest readings [(text, score), ...] (nbest_from_alts); reading 0 is (text, conf)"""
        if self.alt_ids is None:
            raise EngineError("nbest: the result carries no alternatives (Engine.set_alternatives)")
        return nbest_from_alts(self.alt_ids[i], self.alt_prob[i], m)

    @property
    def lines(self) -> list:
        """the page's text lines in reading order: {"text": the words joined by ' ', "bbox": [x1, y1, x2, y2], "items": item indices in word order}"""
        if self.line is None:
            return []
        out = []
        for l in range(len(self.line_first) - 1):
            items = self.order[self.line_first[l]:self.line_first[l + 1]].tolist()
            out.append({"text": " ".join(self.texts[i] for i in items), "bbox": self.line_bbox[l].tolist(), "items": items})
        return out

    @property
    def text(self) -> str:
        """the page's text: its lines in reading order, joined by '\\n' ("" when lines are off)"""
        return "\n".join(ln["text"] for ln in self.lines)

    @property
    def blocks(self) -> list:
        """the page's text blocks in reading order: {"text": the block's lines joined by '\\n', "bbox": [x1, y1, x2, y2], "lines": line indices
        (into `lines`) in order}"""
        if self.block is None:
            return []
        lines, out = self.lines, []
        for b in range(len(self.block_first) - 1):
            members = self.block_order[self.block_first[b]:self.block_first[b + 1]].tolist()
            out.append({"text": "\n".join(lines[l]["text"] for l in members), "bbox": self.block_bbox[b].tolist(), "lines": members})
        return out

    @property
    def text_blocks(self) -> str:
        """the page's text read block after block, the blocks joined by a blank line ("" when blocks are off)"""
        return "\n\n".join(b["text"] for b in self.blocks)

    def __eq__(self, other):
        return list(self) == list(other)

    def __repr__(self):
        return repr(list(self))


class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.ptr = load().ttr_dev_alloc(nbytes)
        if not self.ptr:
            raise EngineError("device allocation failed")
        self.nbytes = nbytes

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        if load().ttr_dev_upload(self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) != 0:
            raise EngineError("upload failed")

    def free(self):
        if self.ptr:
            load().ttr_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    def __init__(self, weights_dir: str, precision: str = "f16x4", device: int = 0, strict_crops: bool = False, **overrides):
        self.lib = load()
        # A process that also uses torch's GPU runtime (bench.py, tuatara_amd/dist.py over RCCL) must let torch initialise FIRST:
        # the torch wheel bundles its own ROCm 7.0 HIP / HSA libraries, and they do not come up once the system ROCm 7.2 runtime the
        # engine links has claimed the device ("No HIP GPUs are available"); the other order works.  So if torch is already
        # imported, bring its runtime up before the engine's.
        _t = sys.modules.get("torch")
        if _t is not None and hasattr(_t, "cuda"):
            try:
                if _t.cuda.is_available():
                    _t.cuda.init()
            except Exception:
                pass
        cfg = Config()
        self.lib.ttr_config_default(C.byref(cfg))
        cfg.precision = (PREC_F32 if precision in ("f32", "fp32", PREC_F32) else
                         PREC_F16X4 if precision in ("f16x4", "split", PREC_F16X4) else PREC_BF16)
        cfg.device = device
        cfg.strict_crops = int(strict_crops)
        alts = int(overrides.pop("alts", 0) or 0)                                         # not a config field either: set_alternatives, below
        lexicon, lexicon_m = overrides.pop("lexicon", None), int(overrides.pop("lexicon_m", 1))   # nor these: set_lexicon, below
        lexicon_fuzzy, lexicon_gap = overrides.pop("lexicon_fuzzy", None), float(overrides.pop("lexicon_gap", LEXICON_GAP))   # nor these: set_lexicon_fuzzy, below
        pattern = overrides.pop("pattern", None)                                          # nor this: set_pattern, below
        pattern_best = bool(overrides.pop("pattern_best", False))                         # nor this: set_pattern_decode, below
        wide = _wide_arg(overrides.pop("wide", None))                                     # nor this: set_wide, below
        curved = bool(overrides.pop("curved", False))                                     # nor this: set_curved, below
        tiled = _tiled_arg(overrides.pop("tiled", None))                                  # nor this: set_tiled, below
        marks = _marks_arg(overrides.pop("marks", None))                                  # nor this: set_marks, below
        barcodes = _barcodes_arg(overrides.pop("barcodes", None))                         # nor this: set_barcodes, below
        tables = _tables_arg(overrides.pop("tables", None))                               # nor this: set_tables, below
        deskew = _deskew_arg(overrides.pop("deskew", None))                               # nor this: set_deskew, below
        local_ink = _local_ink_arg(overrides.pop("local_ink", None))                      # nor this: set_local_ink, below
        self._lex_words = []
        tuning = {k: overrides.pop(k) for k in list(overrides) if not hasattr(cfg, k)}     # not a config field: a tuning key (below)
        for k, v in overrides.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.h = self.lib.ttr_create(weights_dir.encode(), C.byref(cfg))
        if not self.h:
            raise EngineError(self.lib.ttr_last_error().decode())
        for k, v in tuning.items():
            if self.set_tuning(k, int(v)) != 0:
                raise EngineError(f"unknown engine option {k!r}")
        if alts:
            self.set_alternatives(alts)
        if lexicon is not None:
            self.set_lexicon(lexicon, lexicon_m)
        if lexicon_fuzzy is not None:
            self.set_lexicon_fuzzy(lexicon_fuzzy, lexicon_gap)
        if pattern_best:
            self.set_pattern_decode(PATTERN_BEST)
        if pattern:
            self.set_pattern(pattern)
        if wide:
            self.set_wide(wide)
        if curved:
            self.set_curved(True)
        if tiled:
            self.set_tiled(tiled)
        if tables[0]:
            self.set_tables(tables)
        if marks[0]:
            self.set_marks(marks)
        if barcodes[0]:
            self.set_barcodes(barcodes)
        if deskew[0]:
            self.set_deskew(deskew)
        if local_ink[0]:
            self.set_local_ink(local_ink)

    def _set_layer(self, setter, values):
        """a page layer's setter with its tuple of ints; the library's refusal (ASCII) as an EngineError"""
        if setter(self.h, *values) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    def _get_layer(self, getter, n: int):
        """a page layer's n values in force - the getter returns the first and writes the others - or None when the layer is off"""
        rest = [C.c_int() for _ in range(n - 1)]
        first = int(getter(self.h, *[C.byref(v) for v in rest]))
        return (first, *[int(v.value) for v in rest]) if first else None

    def set_local_ink(self, local_ink=True):
        """Take the ink bitmap of the engine's tables and deskew passes from the adaptive threshold (ttr_engine_set_ink; DESIGN.md "Local ink"): False / 0 = off,
        True = (16, 38, 2), else (radius, drop, polarity) with radius in 1..64 px, drop in 1..255 (1/256ths) and polarity 0 dark / 1 light / 2 auto (none of the
        defaults has been tuned on documents).  With neither tables nor deskew on nothing runs; the stage calls keep the fixed rule.  PageResult.ink carries the
        page's record.  Raises EngineError, and changes nothing, for other values and between a stream_push and its flush."""
        self._set_layer(self.lib.ttr_engine_set_ink, _local_ink_arg(local_ink))

    @property
    def local_ink(self):
        """(radius, drop, polarity) in force, or None when local ink is off"""
        return self._get_layer(self.lib.ttr_engine_ink, 3)

    @staticmethod
    def ink_from_page(image, radius: int = LOCAL_INK_RADIUS, drop: int = LOCAL_INK_DROP, polarity: int = LOCAL_INK_POLARITY, row_stride: int = 0) -> dict:
        """the module's ink_from_page: the local ink rule on the host, no GPU"""
        return ink_from_page(image, radius, drop, polarity, row_stride)

    def ink_page(self, image, radius: int = LOCAL_INK_RADIUS, drop: int = LOCAL_INK_DROP, polarity: int = LOCAL_INK_POLARITY, dev_offset: int = 0, dev_stride: int = 0) -> dict:
        """ttr_ink_page: ink_rows_kernel and ink_local_kernel on a host image u8 [H, W, 3], whatever the engine's setting -> the dict ink_from_page returns.
        dev_offset / dev_stride (ttr_dbg_ink_page): the image is placed dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 W)."""
        def fn(*a):
            if dev_offset or dev_stride:
                self._check(self.lib.ttr_dbg_ink_page(self.h, *a[:4], int(dev_offset), int(dev_stride), *a[4:]))
            else:
                self._check(self.lib.ttr_ink_page(self.h, *a))
        return _ink_call(fn, image, radius, drop, polarity)

    def set_deskew(self, deskew=True):
        """Estimate every page's skew on the GPU and read the page upright (ttr_engine_set_deskew; DESIGN.md "Deskew"): False / 0 = off, True = (64, 288, 128),
        else (max_slope, gain, ink) with max_slope in 1..128 (px per 512 px; 128 = 14 degrees), gain in 256..65535 (1/256ths) and ink in 1..255 (none of the
        defaults has been tuned on documents).  Results are those of the upright page, in its frame; PageResult.skew / to_page / "quad_page" lead back to the
        caller's.  Raises EngineError, and changes nothing, for other values, between a stream_push and its flush, and with a communicator attached."""
        self._set_layer(self.lib.ttr_engine_set_deskew, _deskew_arg(deskew))

    @property
    def deskew(self):
        """(max_slope, gain, ink) in force, or None when deskew is off"""
        return self._get_layer(self.lib.ttr_engine_deskew, 3)

    def deskew_page(self, image, max_slope: int = DESKEW_MAX_SLOPE, gain: int = DESKEW_GAIN, ink: int = DESKEW_INK, dev_offset: int = 0, dev_stride: int = 0) -> dict:
        """ttr_deskew_page: the pixel pass, deskew_score_kernel and deskew_rotate_kernel on a host image u8 [H, W, 3], whatever the engine's setting -> the dict
        deskew_from_page returns.  dev_offset / dev_stride (ttr_dbg_deskew_page): the image is placed dev_offset bytes into a device buffer with dev_stride
        bytes from row to row (0 = 3 W)."""
        def fn(*a):
            if dev_offset or dev_stride:
                self._check(self.lib.ttr_dbg_deskew_page(self.h, *a[:4], int(dev_offset), int(dev_stride), *a[4:]))
            else:
                self._check(self.lib.ttr_deskew_page(self.h, *a))
        return _deskew_call(fn, (max_slope, gain, ink), image)

    def set_tables(self, tables=True):
        """Find ruling lines, tables, their grids and merged cells in every page's pixels and give every item its cell (ttr_engine_set_tables; DESIGN.md
        "Tables"): False / 0 = off, True = (48, 128), else (min_len, ink) with min_len in 16..4096 and ink in 1..255 (neither default has been tuned on
        documents).  Items, order, boxes, text, ids and conf keep their bits.  Raises EngineError, and changes nothing, for other values, between a stream_push
        and its flush, and with a communicator attached."""
        self._set_layer(self.lib.ttr_engine_set_tables, _tables_arg(tables))

    @property
    def tables(self):
        """(min_len, ink) in force, or None when tables are off"""
        return self._get_layer(self.lib.ttr_engine_tables, 2)

    def set_marks(self, marks=True):
        """Find every page's checkboxes and their state and give every item its mark (ttr_engine_set_marks; DESIGN.md "Selection marks"): False / 0 = off,
        True = (10, 64, 24, 128), else (min_side 8..64, max_side min_side..128, fill 1..255, ink 1..255) or a bare min_side; none of the defaults has been
        tuned on documents.  Refused while batches stream and with a communicator attached."""
        self._set_layer(self.lib.ttr_engine_set_marks, _marks_arg(marks))

    @property
    def marks(self):
        """(min_side, max_side, fill, ink) in force, or None when marks are off"""
        return self._get_layer(self.lib.ttr_engine_marks, 4)

    def marks_page(self, image, quads=None, min_side: int = MARKS_MIN_SIDE, max_side: int = MARKS_MAX_SIDE, fill: int = MARKS_FILL, ink: int = MARKS_INK) -> dict:
        """ttr_marks_page: table_ink_kernel, mark_cand_kernel and mark_page_kernel on a host image u8 [H, W, 3] and host quads f32 [nq, 8], whatever the
        engine's setting -> the dict marks_from_page returns."""
        return _marks_call(*_page_entry("page", "marks", (min_side, max_side, fill), ink, engine=self), image=image, quads=quads)

    def marks_debug(self, image, min_side: int = MARKS_MIN_SIDE, max_side: int = MARKS_MAX_SIDE, fill: int = MARKS_FILL, ink: int = MARKS_INK, dev_offset: int = 0,
                    dev_stride: int = 0) -> dict:
        """ttr_dbg_marks: the corner count, the band counts i32 [ceil(H / 32), 2] (kept, corners) and the marks as the device formed them; the image is placed
        dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 W)"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape[:2]
        corners, mode, bands, marks = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(((h + 31) // 32, 2), np.int32), np.zeros((512, 12), np.int32)
        self._check(self.lib.ttr_dbg_marks(self.h, _u8(image), h, w, w * 3, int(dev_offset), int(dev_stride), int(min_side), int(max_side), int(fill), int(ink),
                                           _i(corners), _i(bands), _i(mode), _i(marks)))
        n = int(bands[:, 0].sum()) if mode[0] == 1 else 0
        return {"mode": int(mode[0]), "corners": int(corners[0]), "bands": bands, "marks": marks[:n].copy()}

    def set_barcodes(self, barcodes=True):
        """Read every page's Code 128 and Code 39 barcodes and give every item its barcode (ttr_engine_set_barcodes; DESIGN.md "Barcodes"): False / 0 = off,
        True = (8, 128, 3), else (min_lines 4..256, ink 1..255, symbologies 1..3: bit 0 Code 128, bit 1 Code 39) or a bare min_lines; none of the defaults has
        been tuned on documents.  Refused while batches stream and with a communicator attached."""
        self._set_layer(self.lib.ttr_engine_set_barcodes, _barcodes_arg(barcodes))

    @property
    def barcodes(self):
        """(min_lines, ink, symbologies) in force, or None when barcodes are off"""
        return self._get_layer(self.lib.ttr_engine_barcodes, 3)

    def barcodes_page(self, image, quads=None, min_lines: int = BARCODES_MIN_LINES, ink: int = BARCODES_INK, symbologies: int = BARCODES_SYMBOLOGIES) -> dict:
        """ttr_barcodes_page: table_ink_kernel, barcode_scan_kernel and barcode_page_kernel on a host image u8 [H, W, 3] and host quads f32 [nq, 8], whatever
        the engine's setting -> the dict barcodes_from_page returns."""
        return _barcodes_call(*_page_entry("page", "barcodes", (min_lines,), ink, (symbologies,), engine=self), image=image, quads=quads)

    def barcodes_debug(self, image, min_lines: int = BARCODES_MIN_LINES, ink: int = BARCODES_INK, symbologies: int = BARCODES_SYMBOLOGIES, dev_offset: int = 0,
                       dev_stride: int = 0) -> dict:
        """ttr_dbg_barcodes: the lines' raw hits i32 [H + W, 2, 8, 20], their counters i32 [H + W, 2, 4] (kept, dropped, candidates, starts) and the side block
        i32 [1544] as the device formed them; the image is placed dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 W)"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape[:2]
        hits, cnt, side = np.zeros((h + w, 2, 8, 20), np.int32), np.zeros((h + w, 2, 4), np.int32), np.zeros(8 + 64 * 24, np.int32)
        self._check(self.lib.ttr_dbg_barcodes(self.h, _u8(image), h, w, w * 3, int(dev_offset), int(dev_stride), int(min_lines), int(ink), int(symbologies),
                                              _i(hits), _i(cnt), _i(side)))
        return {"hits": hits, "line_counts": cnt, "side": side}

    def page_ink_passes(self) -> int:
        """ttr_dbg_page_ink_passes: the ink passes enqueued for the batches' page layers so far (tables and marks in one batch share one)"""
        return int(self.lib.ttr_dbg_page_ink_passes(self.h))

    def tables_page(self, image, quads=None, min_len: int = TABLES_MIN_LEN, ink: int = TABLES_INK) -> dict:
        """ttr_tables_page: table_ink_kernel and table_grid_kernel on a host image u8 [H, W, 3] and host quads f32 [nq, 8], whatever the engine's setting ->
        the dict tables_from_page returns."""
        return _tables_call(*_page_entry("page", "tables", (min_len,), ink, engine=self), image=image, quads=quads)

    def tables_debug(self, image, min_len: int = TABLES_MIN_LEN, ink: int = TABLES_INK, dev_offset: int = 0, dev_stride: int = 0) -> dict:
        """ttr_dbg_tables: the ink bitmap u64 [H, ceil(W / 64)] and the run lists i32 [n, 3] of both directions as the device formed them; the image is placed
        dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 W)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise RuntimeError("Input array should have 3 dimensions")
        h, w = image.shape[:2]
        bits, runs, nr, mode = np.zeros((h, (w + 63) // 64), np.uint64), np.zeros((2, 8192, 3), np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32)
        self._check(self.lib.ttr_dbg_tables(self.h, _u8(image), h, w, w * 3, int(dev_offset), int(dev_stride), int(min_len), int(ink),
                                            bits.ctypes.data_as(C.POINTER(C.c_uint64)), _i(runs), _i(nr), _i(mode)))
        return {"bits": bits, "runs_h": runs[0, :nr[0]].copy(), "runs_v": runs[1, :nr[1]].copy(), "mode": int(mode[0])}

    def set_tiled(self, overlap=True):
        """Read pages larger than the detector canvas at full size, as overlapping tiles whose heat maps are stitched into one page map (ttr_engine_set_tiled;
        DESIGN.md "Tiled pages"): 0 / False = off, True = TILED_DEFAULT (128), else the overlap in pixels - a multiple of 32 in [64, canvas_size / 4].  A page
        that fits one tile keeps every bit.  Raises EngineError, and changes nothing, for another value, on an engine whose mag_ratio is not 1.0, between a
        stream_push and its flush, and with a communicator attached."""
        if self.lib.ttr_engine_set_tiled(self.h, _tiled_arg(overlap)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def tiled(self) -> int:
        """the overlap in force (0 = off)"""
        return int(self.lib.ttr_engine_tiled(self.h))

    def tile_plan(self, h: int, w: int, overlap=None) -> TilePlan:
        """the tile plan this engine gives an h x w page under `overlap` (None: the engine's own, or TILED_DEFAULT when tiling is off)"""
        return tile_plan(h, w, self.cfg.canvas_size, self.tiled or TILED_DEFAULT if overlap is None else _tiled_arg(overlap), self.cfg.mag_ratio)

    def stitch_heat(self, tiles, oy, ox, Hc: int, Wc: int, H2: int, W2: int):
        """ttr_stitch_heat: engine.stitch_tiles through tile_stitch_kernel (one launch for all pages), bit for bit the host rule's result."""
        t, pages, ny, nx, oy, ox, out = _stitch_args(tiles, oy, ox, Hc, Wc, H2, W2)
        self._check(self.lib.ttr_stitch_heat(self.h, _f(t), pages, ny, nx, _i(oy), _i(ox), int(Hc), int(Wc), int(H2), int(W2), _f(out)))
        return out

    def craft_heatmap_tiled(self, image, overlap=True):
        """ttr_craft_heatmap_tiled: a host image u8 [H, W, 3] at full size under `overlap`, whatever the engine's setting -> the page map f32 [H2, W2, 2]."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise RuntimeError("Input array should have 3 dimensions")
        p = self.tile_plan(image.shape[0], image.shape[1], overlap)
        out = np.zeros((p.H2, p.W2, 2), np.float32)
        H2, W2 = C.c_int(), C.c_int()
        self._check(self.lib.ttr_craft_heatmap_tiled(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _tiled_arg(overlap), _f(out), out.size,
                                                     C.byref(H2), C.byref(W2)))
        return out

    def tile_canvases(self, image, overlap=True):
        """ttr_tile_canvases: the canvases of a host image's tiles as the detector gets them -> u8 [ny * nx, Hc, Wc, 3]."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise RuntimeError("Input array should have 3 dimensions")
        p = self.tile_plan(image.shape[0], image.shape[1], overlap)
        out = np.zeros((p.tiles, p.Hc, p.Wc, 3), np.uint8)
        self._check(self.lib.ttr_tile_canvases(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _tiled_arg(overlap), _u8(out), out.size))
        return out

    def set_curved(self, on=True):
        """Straighten the crops of words set on an arc along a spine found in the page's pixels (ttr_engine_set_curved; DESIGN.md "Curved words").  Every page
        and region call's PageResult then carries curved / outline / spine_knots, its dicts "curved" and "outline"; words that are not curved keep every bit.
        Raises EngineError, and changes nothing, between a stream_push and its flush, on an engine without crop_mode=1, and with orient, chars, wide words or
        a communicator."""
        if on not in (True, False, 0, 1):
            raise EngineError("set_curved: on must be True or False")
        if self.lib.ttr_engine_set_curved(self.h, int(bool(on))) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def curved(self) -> bool:
        return bool(self.lib.ttr_engine_curved(self.h))

    def curve_crops(self, image, quads, table: bool = False):
        """ttr_curve_crops: the kind-1 packer and curve_crop_kernel on a host image u8 [H, W, 3] and host quads f32 [nq, 8], whatever the engine's setting;
        table=True reads the page through the device page table -> (flag i32 [nq], hb i32 [nq, 2], spine i32 [nq, 2, 9], knots i64 [nq, 9, 4], crops u8
        [nq, 32, 128, 3])."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise RuntimeError("Input array should have 3 dimensions")
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
        nq, m = len(q), max(len(q), 1)
        flag, hb, spine = np.zeros(m, np.int32), np.zeros((m, 2), np.int32), np.zeros((m, 2, 9), np.int32)
        knots, crops = np.zeros((m, 9, 4), np.int64), np.zeros((m, 32, 128, 3), np.uint8)
        self._check(self.lib.ttr_curve_crops(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _f(q), nq, int(bool(table)),
                                             _i(flag), _i(hb), _i(spine), _i64(knots), _u8(crops)))
        return flag[:nq].copy(), hb[:nq].copy(), spine[:nq].copy(), knots[:nq].copy(), crops[:nq].copy()

    def set_wide(self, max_aspect=True):
        """Read words wider than max_aspect times their height in pieces cut at ink gaps (ttr_engine_set_wide; DESIGN.md "Wide words"): 0 / False = off, True
        = WIDE_DEFAULT (8.0), else a value in [2, 64].  Every page and region call's PageResult then carries piece_*, its dicts "pieces"; a wide item's text is
        its pieces' texts joined, its conf their product; words that are not wide keep every bit.  Raises EngineError, and changes nothing, for another value,
        between a stream_push and its flush, on an engine without crop_mode=1, and with orient, chars, alternatives, a lexicon, a pattern or a communicator."""
        if self.lib.ttr_engine_set_wide(self.h, _wide_arg(max_aspect)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def wide(self) -> float:
        """max_aspect in force (0.0 = off)"""
        return float(self.lib.ttr_engine_wide(self.h))

    def wide_cuts(self, image, quads, max_aspect: float = WIDE_DEFAULT, table: bool = False):
        """ttr_wide_cuts: wide_cut_kernel on a host image u8 [H, W, 3] and host quads f32 [nq, 8], whatever the engine's setting; table=True reads the page
        through the device page table -> (n i32 [nq], cuts i32 [nq, 17], profiles u16 [nq, 2048], coef i64 [nq, 16, 8])."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise RuntimeError("Input array should have 3 dimensions")
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
        nq = len(q)
        n, cuts = np.zeros(max(nq, 1), np.int32), np.full((max(nq, 1), 17), -1, np.int32)
        prof, coef = np.zeros((max(nq, 1), 2048), np.uint16), np.zeros((max(nq, 1), 16, 8), np.int64)
        self._check(self.lib.ttr_wide_cuts(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _f(q), nq, float(max_aspect), int(bool(table)),
                                           _i(n), _i(cuts), _u16(prof), _i64(coef)))
        return n[:nq].copy(), cuts[:nq].copy(), prof[:nq].copy(), coef[:nq].copy()

    def set_lexicon(self, words=None, m: int = 1):
        """The word list every read word is scored against (ttr_engine_set_lexicon; DESIGN.md "Lexicon matching"): words of 1..25 characters out of the
        recogniser's set (without ']' and the backslash), at most 2^20 of them, duplicates allowed; m = matches kept per item, 1..8.  None clears it.
        Every page call's PageResult then carries lex_idx / lex_logp and its dicts "lexicon"; every other field keeps its bits.  Raises EngineError, and
        changes nothing, for a bad word (naming its index), between a stream_push and its flush, on a bf16 engine and with orient set."""
        if words is None:
            rc = self.lib.ttr_engine_set_lexicon(self.h, None, 0, 0)
        else:
            words = list(words)
            arr, n, _keep = _words_arg(words)
            rc = self.lib.ttr_engine_set_lexicon(self.h, arr, n, int(m))
        if rc != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))
        self._lex_words = [] if words is None else [w.decode("latin1") if isinstance(w, bytes) else str(w) for w in words]

    def set_lexicon_fuzzy(self, band, gap: float = LEXICON_GAP):
        """Fuzzy alignment of the lexicon's entries (ttr_engine_set_lexicon_fuzzy; DESIGN.md "Lexicon matching", Fuzzy alignment): band 0..3 aligns every
        entry against the reading instead of indexing it - a dropped or an extra character costs `gap` (a log-probability, finite, <= 0; the default ln 1e-3
        at band 1 has not been tuned on documents) - and every PageResult then carries lex_edits beside lex_idx / lex_logp, its dicts "lexicon_edits".
        None or -1 switches it off.  It may be set with no lexicon in place and survives set_lexicon.  Raises EngineError, and changes nothing, for a band or
        gap out of range and between a stream_push and its flush."""
        if self.lib.ttr_engine_set_lexicon_fuzzy(self.h, -1 if band is None else int(band), float(gap)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def lexicon_fuzzy(self):
        """(band, gap) in force, None when fuzzy alignment is off"""
        b, g = C.c_int(-1), C.c_float(0.0)
        self.lib.ttr_engine_lexicon_fuzzy(self.h, C.byref(b), C.byref(g))
        return None if b.value < 0 else (int(b.value), float(g.value))

    @property
    def lexicon_size(self) -> int:
        """V in force (0 = no lexicon)"""
        return int(self.lib.ttr_engine_lexicon_size(self.h))

    @property
    def lexicon_m(self) -> int:
        """M in force (0 = no lexicon)"""
        return int(self.lib.ttr_engine_lexicon_m(self.h))

    def lexicon_word(self, idx: int):
        """entry idx as the engine holds it (ttr_engine_lexicon_word), None out of range"""
        w = self.lib.ttr_engine_lexicon_word(self.h, int(idx))
        return None if w is None else w.decode("latin1")

    def logits_lexicon(self, logits: np.ndarray, set_of=None, sets=None):
        """decode_conf_kernel and the lexicon scorer on host logits f32 [n, 26, 95] under the engine's lexicon (ttr_logits_lexicon) -> (idx i32 [n, M],
        logp f32 [n, M]).  sets None: every row under the engine's own set; else row i under sets[set_of[i]] (uint32 [m, 3] masks), -1 = the engine's own."""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 26, 95)
        n, M = len(logits), max(self.lexicon_m, 1)
        idx, logp = np.full((n, M), -1, np.int32), np.full((n, M), -np.inf, np.float32)
        sp, ns, _keep = _sets_arg(sets)
        so = None
        if sp is not None:
            if set_of is None:
                raise ValueError("sets need set_of, one entry per row")
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel()
            if len(so) != n:
                raise ValueError("set_of holds one entry per row")
        self._check(self.lib.ttr_logits_lexicon(self.h, _f(logits), n, sp, ns, _i(so) if so is not None else None, _i(idx), _f(logp)))
        return idx, logp

    def _rows_sets(self, n, set_of, sets):
        sp, ns, keep = _sets_arg(sets)
        so = None
        if sp is not None:
            if set_of is None:
                raise ValueError("sets need set_of, one entry per row")
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel()
            if len(so) != n:
                raise ValueError("set_of holds one entry per row")
        return sp, ns, so, keep

    def logits_lexicon_fuzzy(self, logits: np.ndarray, band: int, gap: float = LEXICON_GAP, set_of=None, sets=None):
        """logits_lexicon through the fuzzy scorer under (band, gap), whatever the engine's mode (ttr_logits_lexicon_fuzzy) -> (idx i32 [n, M], logp f32
        [n, M], edits i32 [n, M]; -1 / -inf / -1 in the empty slots)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 26, 95)
        n, M = len(logits), max(self.lexicon_m, 1)
        idx, logp, edits = np.full((n, M), -1, np.int32), np.full((n, M), -np.inf, np.float32), np.full((n, M), -1, np.int32)
        sp, ns, so, _keep = self._rows_sets(n, set_of, sets)
        self._check(self.lib.ttr_logits_lexicon_fuzzy(self.h, _f(logits), n, sp, ns, _i(so) if so is not None else None, int(band), float(gap), _i(idx), _f(logp),
                                                      _i(edits)))
        return idx, logp, edits

    def debug_lexicon_tables(self, logits: np.ndarray, set_of=None, sets=None) -> np.ndarray:
        """the lexicon's tables as the device forms them (ttr_debug_lexicon_tables): host logits f32 [n, 26, 95] -> lp f32 [n, 26, 96], column 95 -inf"""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 26, 95)
        n = len(logits)
        lp = np.zeros((n, 26, 96), np.float32)
        sp, ns, so, _keep = self._rows_sets(n, set_of, sets)
        self._check(self.lib.ttr_debug_lexicon_tables(self.h, _f(logits), n, sp, ns, _i(so) if so is not None else None, _f(lp)))
        return lp

    def set_alternatives(self, k: int):
        """K alternatives per character position, the winner included (ttr_engine_set_alternatives; DESIGN.md "Character alternatives"): 0 = off, or
        2..8.  Every page call's PageResult then carries alt_ids / alt_prob, its dicts "alternatives", and nbest() works; every other field keeps its
        bits.  Raises EngineError, and changes nothing, for another K, between a stream_push and its flush, on a bf16 engine and with orient set."""
        if self.lib.ttr_engine_set_alternatives(self.h, int(k)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def alternatives(self) -> int:
        """K in force (0 = off)"""
        return int(self.lib.ttr_engine_alternatives(self.h))

    def logits_alternatives(self, logits: np.ndarray, k: int, set_of=None, sets=None):
        """decode_conf_kernel and decode_alts_kernel on host logits f32 [n, 26, 95] (ttr_logits_alternatives) -> (alt_ids i32 [n, 26, k], alt_prob f32
        [n, 26, k]).  sets None: every row under the engine's own set; else row i under sets[set_of[i]] (uint32 [m, 3] masks), -1 = the engine's own."""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 26, 95)
        n = len(logits)
        ids, prob = np.zeros((n, 26, max(int(k), 1)), np.int32), np.zeros((n, 26, max(int(k), 1)), np.float32)
        sp, ns, _keep = _sets_arg(sets)
        so = None
        if sp is not None:
            if set_of is None:
                raise ValueError("sets need set_of, one entry per row")
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel()
            if len(so) != n:
                raise ValueError("set_of holds one entry per row")
        self._check(self.lib.ttr_logits_alternatives(self.h, _f(logits), n, int(k), sp, ns, _i(so) if so is not None else None, _i(ids), _f(prob)))
        return ids, prob

    def set_tuning(self, key, value: int) -> int:
        """Per-engine kernel-selection knob (ttr_engine_set_tuning); keys it does not know go to the process-wide diagnostics setter."""
        return self.lib.ttr_engine_set_tuning(self.h, key if isinstance(key, bytes) else key.encode(), int(value))

    def set_charset(self, allow=None, deny=None):
        """Restrict what the recogniser may emit (ttr_engine_set_charset; DESIGN.md "Character sets"): allow = the characters it may choose (None or
        "": all), deny = characters it may not (None or "": none).  set_charset() resets.  The set acts where each token is chosen - AR steps,
        refinement inputs, the final decode - on parseq_logits and every page call; prob / conf are over the allowed classes.  Raises EngineError,
        and keeps the previous set, on a character that names no class, between a stream_push and its flush, and on a bf16 engine."""
        if self.lib.ttr_engine_set_charset(self.h, _charlist(allow), _charlist(deny)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def charset(self) -> np.ndarray:
        """The class mask in force: uint32 [3] (charset_mask's form); all 95 bits set when there is no set."""
        m = (C.c_uint32 * 3)()
        self._check(self.lib.ttr_engine_get_charset(self.h, m))
        return np.array(list(m), dtype=np.uint32)

    def set_pattern(self, pattern=None, best=None):
        """Constrain every word to a regular expression (ttr_engine_set_pattern; DESIGN.md "Patterns"): the subset of Python's re that include/tuatara_hip.h
        lists, compiled under the engine's character set and recompiled when set_charset changes it.  set_pattern() resets.  Every returned text (of at most
        25 characters) then matches the pattern; prob / conf are over the choices it left open.  Raises EngineError, and changes nothing, on a bad pattern,
        between a stream_push and its flush, on a bf16 engine and with orient, alternatives or a lexicon set.  In sharded mode give every rank the same one.
        best: True / False also sets the decode mode (set_pattern_decode) - True reads every word as the likeliest member of the language; None keeps it."""
        before = self.pattern_decode
        if best is not None:                    # the mode first (it may refuse: bf16, streaming), put back if the pattern is refused
            self.set_pattern_decode(PATTERN_BEST if best else PATTERN_GREEDY)
        if self.lib.ttr_engine_set_pattern(self.h, _charlist(pattern)) != 0:
            err = self.lib.ttr_last_error().decode("latin1")
            self.lib.ttr_engine_set_pattern_decode(self.h, before)
            raise EngineError(err)

    def set_pattern_decode(self, mode):
        """The decode mode of patterns (ttr_engine_set_pattern_decode): PATTERN_GREEDY (0, the default) or PATTERN_BEST (1) - the final decode of every row that
        has a pattern returns the likeliest member of its language under the refined distributions, and page results carry pattern_logp.  Raises EngineError,
        and changes nothing, for another value, between a stream_push and its flush, and for best on a bf16 engine; without a pattern it has no effect."""
        if self.lib.ttr_engine_set_pattern_decode(self.h, int(mode)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode("latin1"))

    @property
    def pattern_decode(self):
        """The decode mode of patterns: PATTERN_GREEDY or PATTERN_BEST."""
        return int(self.lib.ttr_engine_pattern_decode(self.h))

    @property
    def pattern(self):
        """The pattern in force, None when there is none."""
        p = self.lib.ttr_engine_get_pattern(self.h)
        return p.decode("latin1") if p else None

    def logits_decode_patterns(self, logits: np.ndarray, patterns, pattern_of, set_of=None, sets=None, best=False):
        """decode_pat_kernel alone on host logits f32 [n, 26, 95] (ttr_logits_decode_patterns) -> (ids i32 [n, 26], prob f32 [n, 26], conf f32 [n]): row i
        decodes under patterns[pattern_of[i]] (-1: the engine's own pattern, or none) compiled under sets[set_of[i]] (set_of None: the engine's own set).
        best=True: decode_conf_kernel and pattern_best_kernel instead (ttr_logits_decode_patterns_best) -> (ids, prob, conf, logp f32 [n])."""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 26, 95)
        n = len(logits)
        ids, prob, conf = np.zeros((n, 26), np.int32), np.zeros((n, 26), np.float32), np.zeros(n, np.float32)
        po = np.ascontiguousarray(pattern_of, dtype=np.int32).ravel()
        if len(po) != n:
            raise ValueError("pattern_of holds one entry per row")
        so = None
        if set_of is not None:
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel()
            if len(so) != n:
                raise ValueError("set_of holds one entry per row")
        sp, ns, _keep = _sets_arg(sets)
        pp, npat, _keep2 = _patterns_arg(patterns)
        if best:
            logp = np.zeros(n, np.float32)
            self._check(self.lib.ttr_logits_decode_patterns_best(self.h, _f(logits), n, sp, ns, _i(so) if so is not None else None, pp, npat, _i(po), _i(ids), _f(prob),
                                                                 _f(conf), _f(logp)))
            return ids, prob, conf, logp
        self._check(self.lib.ttr_logits_decode_patterns(self.h, _f(logits), n, sp, ns, _i(so) if so is not None else None, pp, npat, _i(po), _i(ids), _f(prob), _f(conf)))
        return ids, prob, conf

    def close(self):
        if getattr(self, "h", None):
            self.lib.ttr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(self.lib.ttr_last_error().decode())

    @property
    def rectified(self) -> bool:
        """crop_mode = CROP_RECTIFIED: result dicts carry "quad" (4 [x, y] corners tl, tr, br, bl)"""
        return self.cfg.crop_mode == CROP_RECTIFIED

    @property
    def orienting(self) -> bool:
        """orient != ORIENT_OFF: result dicts carry "orient" (the chosen turn in degrees clockwise: 0, 90, 180 or 270)"""
        return self.cfg.orient != ORIENT_OFF

    @property
    def orient_candidates(self) -> int:
        """K, the candidate turns per word: 1 (off), 2 (ORIENT_FLIP: 0, 180) or 4 (ORIENT_QUARTER)"""
        return {ORIENT_FLIP: 2, ORIENT_QUARTER: 4}.get(self.cfg.orient, 1)

    @property
    def grouping_lines(self) -> bool:
        """lines=True: result dicts carry "line" and "word", PageResult.lines / .text are filled (DESIGN.md "Text lines")"""
        return self.cfg.lines != 0

    @property
    def cutting_chars(self) -> bool:
        """chars=True: result dicts carry "chars", PageResult.char_* are filled (DESIGN.md "Character boxes")"""
        return self.cfg.chars != 0

    @property
    def grouping_blocks(self) -> bool:
        """blocks=True: result dicts carry "block", PageResult.blocks / .text_blocks are filled (DESIGN.md "Text blocks")"""
        return self.cfg.blocks != 0

    def group_blocks(self, quads, first):
        """ttr_group_blocks: line_group_kernel and block_group_kernel on host quads f32 [N, 8] of several pages (page p owns rows [first[p],
        first[p + 1])), whatever the engine's config -> (line i32 [N], word i32 [N], n_lines i32 [pages], block i32 [N], pos i32 [N], n_blocks
        i32 [pages], mode i32 [pages]); block and pos are per line, within each page's range: entries [first[p], first[p] + n_lines[p]), -1
        behind them."""
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
        first = np.ascontiguousarray(first, dtype=np.int32)
        pages, N = len(first) - 1, len(q)
        if pages < 0 or (pages > 0 and int(first[-1]) != N) or (pages == 0 and N):
            raise ValueError("first must hold pages + 1 offsets ending at len(quads)")
        line, word, block, pos = (np.zeros(max(N, 1), np.int32) for _ in range(4))
        nl, nb, mode = (np.zeros(max(pages, 1), np.int32) for _ in range(3))
        self._check(self.lib.ttr_group_blocks(self.h, _f(q), _i(first), pages, _i(line), _i(word), _i(nl), _i(block), _i(pos), _i(nb), _i(mode)))
        return line[:N].copy(), word[:N].copy(), nl[:pages].copy(), block[:N].copy(), pos[:N].copy(), nb[:pages].copy(), mode[:pages].copy()

    def char_cuts(self, tnorm, ratio: float, low_text: float, quads, turns, nchars):
        """ttr_char_cuts: char_cut_kernel on a host region plane and host words, whatever the engine's `chars`; arguments and results as
        chars_from_map."""
        t, q, tu, nc, n, (cuts, modes, prof) = _chars_args(tnorm, quads, turns, nchars)
        self._check(self.lib.ttr_char_cuts(self.h, _f(t), t.shape[0], t.shape[1], float(ratio), float(low_text), _f(q), _i(tu), _i(nc), n, _i(cuts), _i(modes), _u8(prof)))
        return cuts[:n].copy(), modes[:n].copy(), prof[:n].copy()

    def group_lines(self, quads, first):
        """ttr_group_lines: line_group_kernel on host quads f32 [N, 8] of several pages (page p owns rows [first[p], first[p + 1])), whatever
        the engine's `lines` -> (line i32 [N], word i32 [N], n_lines i32 [pages])."""
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
        first = np.ascontiguousarray(first, dtype=np.int32)
        pages, N = len(first) - 1, len(q)
        if pages < 0 or (pages > 0 and int(first[-1]) != N) or (pages == 0 and N):
            raise ValueError("first must hold pages + 1 offsets ending at len(quads)")
        line, word, nl = np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int32), np.zeros(max(pages, 1), np.int32)
        self._check(self.lib.ttr_group_lines(self.h, _f(q), _i(first), pages, _i(line), _i(word), _i(nl)))
        return line[:N].copy(), word[:N].copy(), nl[:pages].copy()

    def _quads(self, r, n: int) -> np.ndarray:
        return np.ctypeslib.as_array(self.lib.ttr_result_quads(r), (n, 8)).copy() if n else np.zeros((0, 8), np.float32)

    def _take_records(self, r, c: int, one: str, many: str, width: int, keys) -> dict:
        """a result's records of one page layer (ttr_result_<one>_mode / _<one>_count / _<many> / _item_<one>) under the keys (mode, records i32 [n, width],
        items i32 [c], -1 without any); {} for a result the layer did not run for"""
        mode = int(getattr(self.lib, f"ttr_result_{one}_mode")(r))
        if not mode:
            return {}
        n = int(getattr(self.lib, f"ttr_result_{one}_count")(r))
        rp, ip = getattr(self.lib, f"ttr_result_{many}")(r), getattr(self.lib, f"ttr_result_item_{one}")(r)
        return {keys[0]: mode, keys[1]: np.ctypeslib.as_array(rp, (n, width)).copy() if rp and n else np.zeros((0, width), np.int32),
                keys[2]: np.ctypeslib.as_array(ip, (c,)).copy() if ip and c else np.full(c, -1, np.int32)}

    def _take_many(self, arr, n: int, conf: bool = False) -> List[List[dict]]:
        """A batch of ttr_results -> list (per page) of lists of {"text", "bbox", "ids"} (+ "conf", "char_conf" with conf): one gather call
        for the whole batch."""
        counts = np.zeros(n, np.int32)
        need = C.c_size_t()
        total = self.lib.ttr_results_gather(arr, n, _i(counts), None, None, None, 0, C.byref(need))
        bb = np.zeros((max(total, 1), 4), np.float32)
        ids = np.zeros((max(total, 1), 26), np.int32)
        buf = C.create_string_buffer(max(need.value, 1))
        self.lib.ttr_results_gather(arr, n, None, _f(bb), _i(ids), buf, need.value, None)
        texts = buf.raw[:need.value].decode("latin1").split("\n")
        cf = np.zeros(max(total, 1), np.float32)
        pr = np.zeros((max(total, 1), 26), np.float32)
        self.lib.ttr_results_gather_conf(arr, n, _f(cf), _f(pr))
        if self.orienting:                      # the chosen turns, every candidate's conf and the page turns, one call
            K = self.orient_candidates
            ot, oc, op = np.zeros(max(total, 1), np.int32), np.zeros((max(total, 1), K), np.float32), np.zeros(max(n, 1), np.int32)
            if self.lib.ttr_results_gather_orient(arr, n, _i(ot), _f(oc), _i(op)) < 0:
                raise EngineError("ttr_results_gather_orient: the results differ in their candidate count")
        if self.grouping_lines:                 # every page's lines, one call
            nl, ll, lw, lo = np.zeros(max(n, 1), np.int32), np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32)
            lf, lb = np.zeros(total + n + 1, np.int32), np.zeros((max(total, 1), 4), np.float32)
            if self.lib.ttr_results_gather_lines(arr, n, _i(nl), _i(ll), _i(lw), _i(lo), _i(lf), _f(lb)) < 0:
                raise EngineError("ttr_results_gather_lines: bad arguments")
        if self.cutting_chars:                  # every page's characters, one call
            ctot = self.lib.ttr_results_gather_chars(arr, n, None, None, None, None, None, None)
            if ctot < 0:
                raise EngineError("ttr_results_gather_chars: bad arguments")
            chf, chq, chb = np.zeros(total + n + 1, np.int32), np.zeros((max(ctot, 1), 8), np.float32), np.zeros((max(ctot, 1), 4), np.float32)
            chc, chm, chp = np.zeros((max(total, 1), 27), np.int32), np.zeros(max(total, 1), np.int32), np.zeros((max(total, 1), 128), np.uint8)
            self.lib.ttr_results_gather_chars(arr, n, _i(chf), _f(chq), _f(chb), _i(chc), _i(chm), _u8(chp))
        if self.grouping_blocks:                # every page's blocks, one call
            bn, bm, bi = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(total, 1), np.int32)
            bl, bp, bo = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32)
            bf, bbx = np.zeros(total + n + 1, np.int32), np.zeros((max(total, 1), 4), np.float32)
            if self.lib.ttr_results_gather_blocks(arr, n, _i(bn), _i(bm), _i(bi), _i(bl), _i(bp), _i(bo), _i(bf), _f(bbx)) < 0:
                raise EngineError("ttr_results_gather_blocks: bad arguments")
        K = self.alternatives if total else 0   # (the setter refuses while batches stream: every result in flight was made under the K in force)
        if K:                                   # every page's alternatives, one call
            ai, ap = np.zeros((max(total, 1), 26, K), np.int32), np.zeros((max(total, 1), 26, K), np.float32)
            if self.lib.ttr_results_gather_alts(arr, n, _i(ai), _f(ap)) < 0:
                raise EngineError("ttr_results_gather_alts: the results differ in K")
        ptot = self.lib.ttr_results_gather_pieces(arr, n, None, None, None, None, None, None) if total else 0   # wide words: every page's pieces, one call
        if ptot < 0:
            raise EngineError("ttr_results_gather_pieces: bad arguments")
        if ptot:
            pf, pi, pp = np.zeros(total + n + 1, np.int32), np.zeros((ptot, 26), np.int32), np.zeros((ptot, 26), np.float32)
            pc, pq, pcu = np.zeros(ptot, np.float32), np.zeros((ptot, 8), np.float32), np.full((max(total, 1), 17), -1, np.int32)
            self.lib.ttr_results_gather_pieces(arr, n, _i(pf), _i(pi), _f(pp), _f(pc), _f(pq), _i(pcu))
        with_curved = bool(total) and any(bool(self.lib.ttr_result_curved(arr[i])) for i in range(n))   # curved words: every page's flags, outlines and knots, one call
        if with_curved:
            cvf, cvo, cvk = np.zeros(total, np.int32), np.zeros((total, 18, 2), np.float32), np.zeros((total, 9, 4), np.int64)
            if self.lib.ttr_results_gather_curved(arr, n, _i(cvf), _f(cvo), _i64(cvk)) < 0:
                raise EngineError("ttr_results_gather_curved: bad arguments")
        skews = (Skew * max(n, 1))()            # deskew: every page's record, one call (zeroes where a result has none)
        self.lib.ttr_results_gather_skew(arr, n, C.addressof(skews))
        inks = (Ink * max(n, 1))()              # local ink: likewise
        self.lib.ttr_results_gather_ink(arr, n, C.addressof(inks))
        out, k, kl, kc, kbl, kb, kp = [], 0, 0, 0, 0, 0, 0
        for i in range(n):
            c = int(counts[i])
            lex = {}
            if ptot and self.lib.ttr_result_piece_first(arr[i]):
                first = pf[k + i:k + i + c + 1]
                m = int(first[-1])
                lex.update(piece_first=first, piece_ids=pi[kp:kp + m], piece_prob=pp[kp:kp + m], piece_conf=pc[kp:kp + m], piece_quad=pq[kp:kp + m], piece_cuts=pcu[k:k + c])
                kp += m
            if with_curved and self.lib.ttr_result_curved(arr[i]):
                lex.update(curved=cvf[k:k + c], outline=cvo[k:k + c], spine_knots=cvk[k:k + c])
            M = int(self.lib.ttr_result_lex_m(arr[i]))
            if M:                               # the page's matches (the setter refuses while batches stream: the word list is the one in force)
                li, ll = self.lib.ttr_result_lex_idx_all(arr[i]), self.lib.ttr_result_lex_logp_all(arr[i])
                lex.update(lex_idx=np.ctypeslib.as_array(li, (c, M)).copy() if li else np.zeros((0, M), np.int32),
                           lex_logp=np.ctypeslib.as_array(ll, (c, M)).copy() if ll else np.zeros((0, M), np.float32), lex_words=self._lex_words)
                band = int(self.lib.ttr_result_lex_band(arr[i]))
                if band >= 0:                   # fuzzy alignment: the matches' edits
                    le = self.lib.ttr_result_lex_edits_all(arr[i])
                    lex.update(lex_band=band, lex_edits=np.ctypeslib.as_array(le, (c, M)).copy() if le else np.zeros((0, M), np.int32))
            lex["tiles"] = int(self.lib.ttr_result_tiles(arr[i]))
            if self.lib.ttr_result_ink(arr[i], None):    # local ink: the page's record
                lex["ink"] = _ink_dict(inks[i])
            if self.lib.ttr_result_skew(arr[i], None):   # deskew: the page's record, and its quads on the caller's page
                lex["skew"] = _skew_dict(skews[i])
                if self.rectified:
                    q = self._quads(arr[i], c)
                    qp = np.zeros_like(q)
                    if c:
                        self._check(self.lib.ttr_result_to_page(arr[i], _f(q), 4 * c, _f(qp)))
                    lex["quad_page"] = qp
            if self.lib.ttr_result_item_table(arr[i]):   # tables: the page's rulings, tables, lines and cells, its items' cells and the cells' texts
                r = arr[i]
                nr_, nt_, nc_, nl_ = self.lib.ttr_result_ruling_count(r), self.lib.ttr_result_table_count(r), self.lib.ttr_result_cell_count(r), C.c_int()
                lp = self.lib.ttr_result_table_lines(r, C.byref(nl_))

                def view(ptr, shape):
                    return np.ctypeslib.as_array(ptr, shape).copy() if ptr and shape[0] else np.zeros(shape, np.int32)
                texts_c = []
                for cc in range(nc_):
                    need_c = self.lib.ttr_result_cell_text(r, cc, None, 0)
                    buf_c = C.create_string_buffer(max(need_c, 0) + 1)
                    self.lib.ttr_result_cell_text(r, cc, buf_c, need_c + 1)
                    texts_c.append(buf_c.value.decode("latin1"))
                lex.update(table_mode=int(self.lib.ttr_result_table_mode(r)), rulings=view(self.lib.ttr_result_rulings(r), (nr_, 6)),
                           table_rects=view(self.lib.ttr_result_tables(r), (nt_, 8)), table_lines=view(lp, (nl_.value,)),
                           cells=view(self.lib.ttr_result_cells(r), (nc_, 9)), item_table=view(self.lib.ttr_result_item_table(r), (c,)),
                           item_cell=view(self.lib.ttr_result_item_cell(r), (c,)), cell_texts=texts_c)
            # selection marks and barcodes: the page's records and its items' (there for a page without items too)
            lex.update(self._take_records(arr[i], c, "mark", "marks", 12, ("mark_mode", "mark_recs", "item_mark")))
            lex.update(self._take_records(arr[i], c, "barcode", "barcodes", 24, ("barcode_mode", "barcode_recs", "item_barcode")))
            pl = self.lib.ttr_result_pattern_logp(arr[i])
            if pl:                              # patterns in best mode: the page's log-probabilities
                lex["pattern_logp"] = np.ctypeslib.as_array(pl, (c,)).copy()
            orient = (ot[k:k + c], oc[k:k + c], int(op[i])) if self.orienting else (None, None, 0)
            lines = (None,) * 5
            if self.grouping_lines:
                m = int(nl[i])
                lines = (ll[k:k + c], lw[k:k + c], lo[k:k + c], lf[kl + i:kl + i + m + 1], lb[kl:kl + m])
                kl += m
            chars = (None,) * 7
            if self.cutting_chars:
                first = chf[k + i:k + i + c + 1]
                m = int(first[-1])
                chars = (first, chq[kc:kc + m], chb[kc:kc + m], chc[k:k + c], chm[k:k + c], chp[k:k + c], self._quads(arr[i], c))
                kc += m
            blocks = (None,) * 6 + (0,)
            if self.grouping_blocks and int(bn[i]) > 0:
                m, ml = int(bn[i]), int(nl[i])
                blocks = (bi[k:k + c], bl[kbl:kbl + ml], bp[kbl:kbl + ml], bo[kbl:kbl + ml], bf[kb + i:kb + i + m + 1], bbx[kb:kb + m], int(bm[i]))
                kbl += ml
                kb += m
            elif self.grouping_blocks:              # an empty page: no blocks
                blocks = (bi[k:k], bl[:0], bp[:0], bo[:0], np.zeros(1, np.int32), bbx[:0], 0)
            out.append(PageResult(texts[k:k + c], bb[k:k + c], ids[k:k + c], self._quads(arr[i], c) if self.rectified else None,
                                  cf[k:k + c], pr[k:k + c], conf, *orient, *lines, *chars, *blocks,
                                  alt_ids=ai[k:k + c] if K else None, alt_prob=ap[k:k + c] if K else None, **lex))
            k += c
            self.lib.ttr_result_free(arr[i])
        return out

    def _results(self, arr, n: int, keep: bool, conf: bool = False):
        """n ttr_results -> _take_many's pages (keep), else each page's word count; frees them either way."""
        if keep:
            return self._take_many(arr, n, conf)
        counts = []
        for i in range(n):
            counts.append(self.lib.ttr_result_count(arr[i]))
            self.lib.ttr_result_free(arr[i])
        return counts

    # ---- hot path
    def image_to_data(self, image: np.ndarray, conf: bool = False) -> List[dict]:
        """conf=True: every dict gains "conf" (the word's confidence, a probability) and "char_conf" (one probability per character of "text")."""
        if image.ndim != 3:
            raise RuntimeError("Input array should have 3 dimensions")          # bindings/python.cpp:15-17 of the reference
        if image.shape[2] != 3:
            raise RuntimeError("Input array should have 3 channels")            # the C ABI reads rows of 3 * w bytes
        image = np.ascontiguousarray(image, dtype=np.uint8)
        arr = (C.c_void_p * 1)()
        self._check(self.lib.ttr_image_to_data(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, arr))
        return list(self._take_many(arr, 1, conf)[0])

    def images_to_data(self, images, keep: bool = True, conf: bool = False):
        """image_to_data over a list of host images [H, W, 3] u8 of any sizes (ttr_images_to_data): one result list per image, input order.
        Engine(..., mixed_batches=True) batches images that share one detector canvas instead of one size (DESIGN.md "Mixed-size batches")."""
        arrs = []
        for im in images:
            a = np.asarray(im)
            if a.ndim != 3 or a.shape[2] != 3:
                raise EngineError("Input array should have 3 dimensions")
            arrs.append(np.ascontiguousarray(a, dtype=np.uint8))
        n = len(arrs)
        if n == 0:
            return []
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        hs = (C.c_int32 * n)(*[a.shape[0] for a in arrs])
        ws = (C.c_int32 * n)(*[a.shape[1] for a in arrs])
        out = (C.c_void_p * n)()
        rc = self.lib.ttr_images_to_data(self.h, ptrs, hs, ws, None, n, out)
        self.last_images_error = None
        if rc < 0:
            self._check(rc)
        if rc > 0:                              # rc images failed: their results are empty, the others delivered (include/tuatara_hip.h)
            self.last_images_error = self.lib.ttr_last_error().decode()
        return self._results(out, n, keep, conf)

    def pages_to_data_dev(self, d_pages, n: int, h: int, w: int, keep: bool = True, conf: bool = False):
        """d_pages: DeviceBuffer or raw device pointer holding [n][h][w][3] u8."""
        ptr = d_pages.ptr if isinstance(d_pages, DeviceBuffer) else d_pages
        arr = (C.c_void_p * n)()
        self._check(self.lib.ttr_pages_to_data_dev(self.h, ptr, n, h, w, arr))
        return self._results(arr, n, keep, conf)

    def stream_push(self, d_pages, n: int, h: int, w: int, keep: bool = True, max_batch: int = 0, conf: bool = False):
        """Streamed batches (ttr_stream_push): enqueue batch k+1, get batch k's results (an empty list on the first push).  The
        pages of a batch must stay alive until its results have come back."""
        ptr = d_pages.ptr if isinstance(d_pages, DeviceBuffer) else d_pages
        self._max_pushed = max(getattr(self, "_max_pushed", 1), n, max_batch)   # a returned batch is never larger than the largest pushed
        arr = (C.c_void_p * self._max_pushed)()
        n_prev = C.c_int(0)
        self._check(self.lib.ttr_stream_push(self.h, ptr, n, h, w, arr, C.byref(n_prev)))
        return self._results(arr, n_prev.value, keep, conf)

    def stream_flush(self, keep: bool = True, conf: bool = False):
        arr = (C.c_void_p * getattr(self, "_max_pushed", 1))()
        n_prev = C.c_int(0)
        self._check(self.lib.ttr_stream_flush(self.h, arr, C.byref(n_prev)))
        return self._results(arr, n_prev.value, keep, conf)

    def read_regions(self, pages_or_image, regions, charsets=None, patterns=None):
        """Read regions the caller already knows, each under its own character set, with no detector (DESIGN.md "Regions and per-row character sets").
        pages_or_image: one host image [H, W, 3] u8 (ttr_image_regions_to_data), or a list of device pages (ptr | DeviceBuffer, h, w[, row_stride]) of
        any sizes (ttr_regions_to_data_dev).  regions: a list of dicts {"quad": 8 floats | "rect": (x0, y0, x1, y1), "page": index (default 0), "set":
        index into charsets, or -1 / absent = the engine's own set}, or of bare quads / rectangles (page 0, the engine's set).  charsets: a list of
        (allow, deny) pairs or ready-made masks.  Returns, per page (for an image: that page alone), the regions in the caller's order as dicts {"text",
        "bbox", "ids", "quad", "conf", "prob", "set", "region"} - "quad" the caller's floats verbatim, "region" the index into `regions`; with set_alternatives(K) also "alt_ids",
        "alt_prob" ([26, K] arrays) and "alternatives", each region's under its own set; with set_lexicon also "lex_idx", "lex_logp" ([M] arrays) and "lexicon".
        patterns (DESIGN.md "Patterns"): a list parallel to `regions`, each entry the region's own pattern or None (the engine's own pattern, or none)."""
        pp, npat, po = None, 0, None
        if patterns is not None:
            if len(patterns) != len(regions):
                raise ValueError("patterns holds one entry per region (None = no pattern of its own)")
            distinct, po = _pattern_rows(patterns)
            pp, npat, _keep_p = _patterns_arg(distinct)
        regs = (Region * max(len(regions), 1))()
        for i, r in enumerate(regions):
            d = r if isinstance(r, dict) else {"quad" if np.asarray(r).size == 8 else "rect": r}
            if ("quad" in d) == ("rect" in d):
                raise ValueError(f"region {i}: give a quad or a rect")
            q = region_quad(d["quad"] if "quad" in d else d["rect"])
            regs[i] = Region((C.c_float * 8)(*[float(v) for v in q]), int(d.get("page", 0)), int(d.get("set", -1)))
        sp, ns, _keep = _sets_arg(charset_masks(charsets) if charsets is not None else None)
        single = isinstance(pages_or_image, np.ndarray)
        if single:
            image = np.ascontiguousarray(pages_or_image, dtype=np.uint8)
            if image.ndim != 3 or image.shape[2] != 3:
                raise RuntimeError("Input array should have 3 dimensions")
            n_pages = 1
            arr = (C.c_void_p * 1)()
            if po is not None:
                self._check(self.lib.ttr_image_regions_to_data_p(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, regs, len(regions), sp, ns, pp, npat, _i(po), arr))
            else:
                self._check(self.lib.ttr_image_regions_to_data(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, regs, len(regions), sp, ns, arr))
        else:
            n_pages = len(pages_or_image)
            arr = (C.c_void_p * max(n_pages, 1))()
            if po is not None:
                self._check(self.lib.ttr_regions_to_data_dev_p(self.h, self._page_array(pages_or_image), n_pages, regs, len(regions), sp, ns, pp, npat, _i(po), arr))
            else:
                self._check(self.lib.ttr_regions_to_data_dev(self.h, self._page_array(pages_or_image), n_pages, regs, len(regions), sp, ns, arr))
        where = [[i for i in range(len(regions)) if regs[i].page == p] for p in range(n_pages)]
        out = []
        for p in range(n_pages):
            c = self.lib.ttr_result_count(arr[p])
            sets = np.ctypeslib.as_array(self.lib.ttr_result_sets(arr[p]), (c,)).copy() if c else np.zeros(0, np.int32)
            quads = self._quads(arr[p], c)
            page = self._take_many((C.c_void_p * 1)(arr[p]), 1)[0]      # (frees the result)
            items = []
            for k in range(c):
                items.append({"text": page.texts[k], "bbox": page.bbox[k].tolist(), "ids": page.ids[k].tolist(), "quad": quads[k].tolist(),
                              "conf": float(page.conf[k]), "prob": page.prob[k].tolist(), "set": int(sets[k]), "region": where[p][k]})
                if page.alt_ids is not None:        # character alternatives: each region under its own set
                    items[-1].update({"alt_ids": page.alt_ids[k], "alt_prob": page.alt_prob[k], "alternatives": char_alternatives(page.alt_ids[k], page.alt_prob[k])})
                if page.piece_first is not None:    # wide words: each region's pieces under its own set
                    a, b = int(page.piece_first[k]), int(page.piece_first[k + 1])
                    items[-1].update({"pieces": page.pieces(k), "piece_ids": page.piece_ids[a:b], "piece_prob": page.piece_prob[a:b], "piece_conf": page.piece_conf[a:b],
                                      "piece_quad": page.piece_quad[a:b], "piece_cuts": page.piece_cuts[k]})
                if page.curved is not None:         # curved words: each region's flag, outline and knot table
                    items[-1].update({"curved": int(page.curved[k]), "outline": page.outline[k].tolist(), "spine_knots": page.spine_knots[k]})
                if page.lex_idx is not None:        # lexicon matching: each region under its own set
                    items[-1].update({"lex_idx": page.lex_idx[k], "lex_logp": page.lex_logp[k], "lexicon": lexicon_matches(page.lex_words, page.lex_idx[k], page.lex_logp[k])})
                    if page.lex_edits is not None:  # fuzzy alignment: likewise
                        items[-1].update({"lex_edits": page.lex_edits[k], "lexicon_edits": [int(e) for i, e in zip(page.lex_idx[k], page.lex_edits[k]) if int(i) >= 0]})
                if page.pattern_logp is not None:   # patterns in best mode: each region under its own pattern and set
                    items[-1]["pattern_logp"] = float(page.pattern_logp[k])
            out.append(items)
        return out[0] if single else out

    def pack_regions(self, image: np.ndarray, quads) -> np.ndarray:
        """ttr_pack_regions: the crops of caller-given quads f32 [n, 8] (tl, tr, br, bl in image pixels) on a host image -> u8 [n, 32, 128, 3]."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        quads = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
        n = len(quads)
        crops = np.zeros((n, 32, 128, 3), np.uint8)
        self._check(self.lib.ttr_pack_regions(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _f(quads), n, _u8(crops)))
        return crops

    def canvas_geometry(self, h: int, w: int):
        """ttr_canvas_geometry: the detector canvas this engine gives an h x w page -> (H, W, ratio).  Pages with equal (H, W) can share a batch."""
        H, W, ratio = C.c_int32(), C.c_int32(), C.c_float()
        self._check(self.lib.ttr_canvas_geometry(self.h, int(h), int(w), C.byref(H), C.byref(W), C.byref(ratio)))
        return H.value, W.value, ratio.value

    @staticmethod
    def _page_array(pages):
        """a list of (ptr | DeviceBuffer, h, w[, row_stride]) -> ttr_page array"""
        arr = (Page * max(len(pages), 1))()
        for i, p in enumerate(pages):
            d = p[0].ptr if isinstance(p[0], DeviceBuffer) else p[0]
            arr[i] = Page(d, int(p[1]), int(p[2]), int(p[3]) if len(p) > 3 else 0)
        return arr

    def pages_to_data_dev_v(self, pages, keep: bool = True, conf: bool = False):
        """ttr_pages_to_data_dev_v: a batch of device-resident pages of different sizes and row strides that share one canvas (DESIGN.md "Mixed-size
        batches"); pages: a list of (ptr | DeviceBuffer, h, w, row_stride), row_stride in bytes (0 or absent = 3 * w)."""
        n = len(pages)
        arr = (C.c_void_p * max(n, 1))()
        self._check(self.lib.ttr_pages_to_data_dev_v(self.h, self._page_array(pages), n, arr))
        return self._results(arr, n, keep, conf)

    def stream_push_v(self, pages, keep: bool = True, max_batch: int = 0, conf: bool = False):
        """ttr_stream_push_v: stream_push for such a batch; mixes freely with stream_push, the same stream_flush returns both kinds."""
        n = len(pages)
        self._max_pushed = max(getattr(self, "_max_pushed", 1), n, max_batch)
        arr = (C.c_void_p * self._max_pushed)()
        n_prev = C.c_int(0)
        self._check(self.lib.ttr_stream_push_v(self.h, self._page_array(pages), n, arr, C.byref(n_prev)))
        return self._results(arr, n_prev.value, keep, conf)

    def last_images_batches(self) -> List[int]:
        """ttr_last_images_batches: the pages per batch of the last images_to_data call, in run order."""
        n = self.lib.ttr_last_images_batches(self.h, None, 0)
        if n < 0:
            self._check(n)
        out = np.zeros(max(n, 1), np.int32)
        self.lib.ttr_last_images_batches(self.h, _i(out), n)
        return out[:n].tolist()

    def resize_canvas_batch(self, images):
        """ttr_resize_canvas_batch: host images of different sizes that share one canvas through ONE launch of resize_pad_pages_kernel ->
        (canvases u8 [n, H, W, 3], ratios f32 [n]).  A view into a wider array keeps its row stride on the device."""
        ptrs, hs, ws, st, keep = _host_images(images)
        n = len(keep)
        H, W, _ = self.canvas_geometry(keep[0].shape[0], keep[0].shape[1])
        buf = np.zeros((n, H, W, 3), np.uint8)
        ratios = np.zeros(n, np.float32)
        Ho, Wo = C.c_int32(), C.c_int32()
        self._check(self.lib.ttr_resize_canvas_batch(self.h, ptrs, hs, ws, st, n, _u8(buf), buf.nbytes, C.byref(Ho), C.byref(Wo), _f(ratios)))
        assert (Ho.value, Wo.value) == (H, W)
        return buf, ratios

    def pack_crops_batch(self, images, rects, page_of, crop_mode: int, turn: int):
        """ttr_pack_crops_batch: heat-map rects f32 [n, 5], rect i on page page_of[i] of `images` (different sizes, one canvas), through ONE launch of the
        table packer -> (crops u8 [n, 32, 128, 3], turned quads f32 [n, 4, 2]).  Crop i is pack_crops_oriented's on its page alone."""
        ptrs, hs, ws, st, keep = _host_images(images)
        rects = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 5)
        page_of = np.ascontiguousarray(page_of, dtype=np.int32).reshape(-1)
        n = len(rects)
        if len(page_of) != n:
            raise ValueError("page_of must hold one entry per rect")
        crops = np.zeros((n, 32, 128, 3), np.uint8)
        quads = np.zeros((n, 4, 2), np.float32)
        self._check(self.lib.ttr_pack_crops_batch(self.h, ptrs, hs, ws, st, len(keep), _f(rects), _i(page_of), n, int(crop_mode), int(turn), _u8(crops), _f(quads)))
        return crops, quads

    def last_groups(self):
        """(pages per CRAFT launch group of the last batch, crops per encoder group of the last recogniser pass); 0 = none yet."""
        gp, ge = C.c_int32(), C.c_int32()
        self._check(self.lib.ttr_dbg_last_groups(self.h, C.byref(gp), C.byref(ge)))
        return gp.value, ge.value

    def last_heat(self, n: int, H: int, W: int) -> np.ndarray:
        """The heat maps the detector left for the last batch of n pages on a canvas of H x W: f32 [n, H/2, W/2, 2] (ttr_dbg_last_heat)."""
        heat = np.zeros((n, H // 2, W // 2, 2), np.float32)
        self._check(self.lib.ttr_dbg_last_heat(self.h, _f(heat), heat.size))
        return heat

    def poison_scratch(self, pattern: int, also_kept_once: bool = False) -> int:
        """f16x4 engines, developer hook (ttr_dbg_poison_scratch): every allocated scratch buffer of the engine filled to its capacity with pattern
        0 (zeros) / 1 (quiet NaN) / 2 (large finite); integer buffers always with zeros.  also_kept_once poisons the two write-once float buffers too:
        close such an engine afterwards.  Returns the bytes filled."""
        n = self.lib.ttr_dbg_poison_scratch(self.h, int(pattern), int(bool(also_kept_once)))
        if n < 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        return int(n)

    def last_stage_ms(self):
        ms = (C.c_float * 4)()
        self.lib.ttr_last_stage_ms(self.h, ms)
        return dict(craft=ms[0], post=ms[1], pack=ms[2], parseq=ms[3])

    def dbg_attn_enc(self, qkv):
        """Encoder self-attention on qkv [N,128,1152] -> [N,128,384] (values rounded to the engine's type on the way in / out)."""
        qkv = np.ascontiguousarray(qkv, np.float32)
        N = qkv.shape[0]
        out = np.zeros((N, 128, 384), np.float32)
        self._check(self.lib.ttr_dbg_attn_enc(self.h, _f(qkv), N, _f(out)))
        return out

    def dbg_cross_attn(self, q, kvmem):
        """The decoder's cross-attention kernels on their own: q [N, R, 384], kvmem [N, 128, 768] (K | V) -> [N, R, 384] (split / fp32 engines)."""
        q = np.ascontiguousarray(q, np.float32); kvmem = np.ascontiguousarray(kvmem, np.float32)
        N, R = q.shape[0], q.shape[1]
        out = np.zeros((N, R, 384), np.float32)
        self._check(self.lib.ttr_dbg_cross_attn(self.h, _f(q), _f(kvmem), N, R, _f(out)))
        return out

    def dbg_dec_self_attn(self, q, kvcache, tokens, R: int, qi0: int, mode: int):
        """The decoder's self-attention kernel on its own: q [26, 384], kvcache [N, 26, 768] (K | V), tokens i32 [N, 26]; mode 0 = AR step qi0 (R = 1),
        mode 1 = refinement (R rows per crop) -> [N, R, 384] (split / fp32 engines; a row the kernel left out is NaN)."""
        q = np.ascontiguousarray(q, np.float32); kvcache = np.ascontiguousarray(kvcache, np.float32); tokens = np.ascontiguousarray(tokens, np.int32)
        N = kvcache.shape[0]
        if q.shape != (26, 384) or kvcache.shape != (N, 26, 768) or tokens.shape != (N, 26):
            raise ValueError("q [26, 384], kvcache [N, 26, 768], tokens [N, 26]")
        out = np.zeros((N, int(R), 384), np.float32)
        self._check(self.lib.ttr_dbg_dec_self_attn(self.h, _f(q), _f(kvcache), _i(tokens), N, int(R), int(qi0), int(mode), _f(out)))
        return out

    def dbg_qkv_attn(self, x, w, b):
        """qkv_attn.hip: x [N,128,384] (LayerNorm output), w [1152,384], b [1152] -> attention output [N,128,384]."""
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
        out = np.zeros((x.shape[0], 128, 384), np.float32)
        self._check(self.lib.ttr_dbg_qkv_attn(self.h, _f(x), x.shape[0], _f(w), _f(b), _f(out)))
        return out

    def dbg_mlp(self, x, ln_g, ln_b, w1, b1, w2, b2, nln_g=None, nln_b=None, eps=1e-6, att=None, wp=None, bp=None):
        """mlp_fused.hip on f32 rows x [M,384] -> (x_out f32 [M,384], LayerNorm_next(x_out) as f32 or None)."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x, ln_g, ln_b, w1, b1, w2, b2 = map(f, (x, ln_g, ln_b, w1, b1, w2, b2))
        M = x.shape[0]
        out = np.zeros((M, 384), np.float32)
        nout = np.zeros((M, 384), np.float32) if nln_g is not None else None
        ng, nb = (f(nln_g), f(nln_b)) if nln_g is not None else (None, None)
        self._check(self.lib.ttr_dbg_mlp(self.h, _f(x), M, _f(ln_g), _f(ln_b), eps, _f(w1), _f(b1), _f(w2), _f(b2),
                                         _f(ng) if ng is not None else None, _f(nb) if nb is not None else None, _f(out),
                                         _f(nout) if nout is not None else None,
                                         _f(f(att)) if att is not None else None, _f(f(wp)) if att is not None else None, _f(f(bp)) if att is not None else None))
        return out, nout

    def last_host_us(self):
        us = (C.c_float * 8)()
        self.lib.ttr_last_host_us(self.h, us)
        return [round(float(x), 1) for x in us]

    def set_profiling(self, on):
        """0 / False off, 1 / True CRAFT conv launches only, 2 every conv / GEMM launch."""
        self.lib.ttr_set_profiling(self.h, int(on))

    def get_profile(self):
        ms, fl, n = (C.c_double * 3)(), (C.c_double * 3)(), (C.c_longlong * 3)()
        self.lib.ttr_get_profile(self.h, ms, fl, n)
        return {"craft": dict(ms=ms[0], flops=fl[0], launches=n[0]), "parseq": dict(ms=ms[1], flops=fl[1], launches=n[1]),
                "parseq_ar": dict(ms=ms[2], flops=fl[2], launches=n[2])}

    def get_profile_kinds(self):
        """The timed launches by kernel kind: list of dicts {kind, stage, launches, ms, alg_flops, exec_flops} (ttr_get_profile_kinds)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        n = self.lib.ttr_get_profile_kinds(self.h, buf, len(buf))
        if n >= len(buf):                                   # the call returns the full length: come back with room for it
            buf = C.create_string_buffer(n + 1)
            n = self.lib.ttr_get_profile_kinds(self.h, buf, len(buf))
        if n < 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        return json.loads(buf.value.decode())

    # ---- stages
    def craft_heatmap(self, canvas: np.ndarray) -> np.ndarray:
        canvas = np.ascontiguousarray(canvas, dtype=np.uint8)
        H, W = canvas.shape[:2]
        heat = np.zeros((H // 2, W // 2, 2), np.float32)
        self._check(self.lib.ttr_craft_heatmap(self.h, _u8(canvas), H, W, _f(heat)))
        return heat

    def craft_taps(self, canvases: np.ndarray):
        """f16x4 engines, developer hook (ttr_dbg_craft_taps): one detector pass over canvases u8 [B, H, W, 3] (or [H, W, 3]) with the tap on ->
        (heat f32 [B, H/2, W/2, 2], records).  A record is a dict: layer, role (canvas / in0 / in1 / out / out_relu / out_pool / z / heat), kind (the
        kernel, on outputs), B, H, W, C (real channels), ld (row length in channels), form (0 fp32, 1 packed pairs, 2 pairs, 3 triples, 4 u8), index.
        craft_tap_read(index) fetches a tensor; the records hold until this engine's next detector pass."""
        canvases = np.ascontiguousarray(canvases, dtype=np.uint8)
        if canvases.ndim == 3:
            canvases = canvases[None]
        B, H, W = canvases.shape[:3]
        heat = np.zeros((B, H // 2, W // 2, 2), np.float32)
        n = self.lib.ttr_dbg_craft_taps(self.h, _u8(canvases), B, H, W, _f(heat))
        if n < 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        recs = []
        text, dims = C.create_string_buffer(512), np.zeros(7, np.int32)
        for i in range(n):
            self._check(self.lib.ttr_dbg_craft_tap_info(self.h, i, text, 512, _i(dims)))
            layer, role, kind = text.value.decode().split("\n")
            recs.append(dict(index=i, layer=layer, role=role, kind=kind, B=int(dims[0]), H=int(dims[1]), W=int(dims[2]), C=int(dims[3]), ld=int(dims[4]),
                             form=int(dims[5])))
        return heat, recs

    def craft_fold_taps(self):
        """The records of the folded upconv1.0 launches of the last craft_taps pass (tuning key fc7_fold on; empty with it off): layer "upconv1.0", roles in0
        (the 3x3 max-pool's output), in1 (relu5_3), z (the skip half's 1x1, fp32) and out.  craft_taps' own records are those of the three original layers,
        which a tapped pass runs beside the folded launches into workspaces nothing reads.  Read with craft_tap_read."""
        recs = []
        text, dims = C.create_string_buffer(512), np.zeros(7, np.int32)
        for i in range(max(0, self.lib.ttr_dbg_craft_fold_tap_count(self.h))):
            self._check(self.lib.ttr_dbg_craft_fold_tap_info(self.h, i, text, 512, _i(dims)))
            layer, role, kind = text.value.decode().split("\n")
            recs.append(dict(index=i, layer=layer, role=role, kind=kind, B=int(dims[0]), H=int(dims[1]), W=int(dims[2]), C=int(dims[3]), ld=int(dims[4]),
                             form=int(dims[5]), fold=True))
        return recs

    def craft_tap_read(self, rec) -> np.ndarray:
        """Tensor of a craft_taps (or craft_fold_taps) record joined to fp32 on the host, every step exact: f32 [B, H, W, ld], padding channels included."""
        out = np.zeros((rec["B"], rec["H"], rec["W"], rec["ld"]), np.float32)
        read = self.lib.ttr_dbg_craft_fold_tap_read if rec.get("fold") else self.lib.ttr_dbg_craft_tap_read
        self._check(read(self.h, rec["index"], _f(out)))
        return out

    def ccl_boxes(self, heat: np.ndarray, max_rects: int = 8192) -> np.ndarray:
        heat = np.ascontiguousarray(heat, dtype=np.float32)
        H2, W2 = heat.shape[:2]
        rects = np.zeros((max_rects, 5), np.float32)
        n = C.c_int32()
        self._check(self.lib.ttr_ccl_boxes(self.h, _f(heat), H2, W2, _f(rects), max_rects, C.byref(n)))
        return rects[: n.value].copy()

    def resize_canvas(self, image: np.ndarray):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        cap = 1056 * 1056 * 3 * 4
        buf = np.zeros(cap, np.uint8)
        H, W, ratio = C.c_int32(), C.c_int32(), C.c_float()
        self._check(self.lib.ttr_resize_canvas(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _u8(buf), cap,
                                               C.byref(H), C.byref(W), C.byref(ratio)))
        return buf[: H.value * W.value * 3].reshape(H.value, W.value, 3).copy(), ratio.value

    def pack_crops(self, image: np.ndarray, rects: np.ndarray, ratio: float):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rects = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 5)
        n = len(rects)
        crops = np.zeros((n, 32, 128, 3), np.uint8)
        boxes = np.zeros((n, 5), np.float32)
        self._check(self.lib.ttr_pack_crops(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _f(rects), n,
                                            C.c_float(ratio), _u8(crops), _f(boxes)))
        return crops, boxes

    def pack_crops_rectified(self, image: np.ndarray, rects: np.ndarray, ratio: float):
        """ttr_pack_crops_rectified: the crop_mode = CROP_RECTIFIED crops of heat-map rects -> (crops u8 [n,32,128,3], quads f32 [n,4,2])."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rects = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 5)
        n = len(rects)
        crops = np.zeros((n, 32, 128, 3), np.uint8)
        quads = np.zeros((n, 4, 2), np.float32)
        self._check(self.lib.ttr_pack_crops_rectified(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _f(rects), n,
                                                      C.c_float(ratio), _u8(crops), _f(quads)))
        return crops, quads

    def pack_crops_oriented(self, image: np.ndarray, rects: np.ndarray, ratio: float, crop_mode: int, turn: int):
        """ttr_pack_crops_oriented: the crops of heat-map rects read at `turn` quarter turns clockwise -> (crops u8 [n,32,128,3], turned quads
        f32 [n,4,2]).  Turn 0 is pack_crops (crop_mode 0) / pack_crops_rectified (crop_mode 1)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rects = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 5)
        n = len(rects)
        crops = np.zeros((n, 32, 128, 3), np.uint8)
        quads = np.zeros((n, 4, 2), np.float32)
        self._check(self.lib.ttr_pack_crops_oriented(self.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, _f(rects), n,
                                                     C.c_float(ratio), int(crop_mode), int(turn), _u8(crops), _f(quads)))
        return crops, quads

    def parseq_logits(self, crops: np.ndarray, want_ar: bool = False, set_of=None, sets=None, pattern_of=None, patterns=None):
        """set_of (i32 [n]) with sets (uint32 [k, 3] masks): crop i chooses under sets[set_of[i]], -1 = the engine's own set (ttr_parseq_logits_sets).
        pattern_of (i32 [n]) with patterns (strings): crop i reads under patterns[pattern_of[i]], -1 = the engine's own pattern or none (ttr_parseq_logits_patterns)."""
        crops = np.ascontiguousarray(crops, dtype=np.uint8)
        n = len(crops)
        logits = np.zeros((n, 26, 95), np.float32)
        ar = np.zeros((n, 26, 95), np.float32) if want_ar else None
        ids = np.zeros((n, 26), np.int32)
        if pattern_of is not None:
            po = np.ascontiguousarray(pattern_of, dtype=np.int32).ravel()
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel() if set_of is not None else None
            if len(po) != n or (so is not None and len(so) != n):
                raise ValueError("pattern_of and set_of hold one entry per crop")
            sp, ns, _keep = _sets_arg(sets)
            pp, npat, _keep2 = _patterns_arg(patterns)
            self._check(self.lib.ttr_parseq_logits_patterns(self.h, _u8(crops), n, sp, ns, _i(so) if so is not None else None, pp, npat, _i(po), _f(logits),
                                                            _f(ar) if want_ar else None, _i(ids)))
        elif set_of is not None:
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel()
            if len(so) != n:
                raise ValueError("set_of holds one entry per crop")
            sp, ns, _keep = _sets_arg(sets)
            self._check(self.lib.ttr_parseq_logits_sets(self.h, _u8(crops), n, sp, ns, _i(so), _f(logits), _f(ar) if want_ar else None, _i(ids)))
        else:
            self._check(self.lib.ttr_parseq_logits(self.h, _u8(crops), n, _f(logits), _f(ar) if want_ar else None, _i(ids)))
        return (logits, ar, ids) if want_ar else (logits, ids)

    def logits_confidence(self, logits: np.ndarray, mask=None, set_of=None, sets=None):
        """The recogniser's final decode on host logits f32 [n, 26, 95] (ttr_logits_confidence: decode_conf_kernel) -> (ids i32 [n, 26],
        prob f32 [n, 26], conf f32 [n]).  mask (uint32 [3], charset_mask's form): the decode among the allowed classes only
        (ttr_logits_confidence_masked); the engine's own set is not consulted either way.  set_of (i32 [n]) with sets (uint32 [k, 3]): row i
        decodes under sets[set_of[i]], -1 = the engine's own set (ttr_logits_confidence_sets)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 26, 95)
        n = len(logits)
        ids, prob, conf = np.zeros((n, 26), np.int32), np.zeros((n, 26), np.float32), np.zeros(n, np.float32)
        if set_of is not None:
            so = np.ascontiguousarray(set_of, dtype=np.int32).ravel()
            if len(so) != n:
                raise ValueError("set_of holds one entry per row")
            sp, ns, _keep = _sets_arg(sets)
            self._check(self.lib.ttr_logits_confidence_sets(self.h, _f(logits), n, sp, ns, _i(so), _i(ids), _f(prob), _f(conf)))
        elif mask is None:
            self._check(self.lib.ttr_logits_confidence(self.h, _f(logits), n, _i(ids), _f(prob), _f(conf)))
        else:
            m = (C.c_uint32 * 3)(*[int(v) for v in np.asarray(mask).ravel()[:3]])
            self._check(self.lib.ttr_logits_confidence_masked(self.h, _f(logits), n, m, _i(ids), _f(prob), _f(conf)))
        return ids, prob, conf

    def dbg_conv_pool(self, x0: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], ks: int, act: int = 0, pool_relu: bool = False,
                      want_full: bool = True):
        """bf16 engines: conv + fused 2x2 max-pool -> (full f32 [B,H,W,Cout] or None, pooled f32 [B,H/2,W/2,Cout])."""
        x0 = np.ascontiguousarray(x0, dtype=np.float32)
        B, H, W_, C0 = x0.shape
        w = np.ascontiguousarray(w, dtype=np.float32)
        Cout = w.shape[0]
        full = np.zeros((B, H, W_, Cout), np.float32) if want_full else None
        pool = np.zeros((B, H // 2, W_ // 2, Cout), np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
        self._check(self.lib.ttr_dbg_conv_pool(self.h, _f(x0), C0, B, H, W_, ks, _f(w), _f(b) if b is not None else None, Cout, act,
                                               int(pool_relu), _f(full) if want_full else None, _f(pool)))
        return full, pool

    def dbg_conv(self, x0: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], ks: int, dil: int = 1, act: int = 0,
                 x1: Optional[np.ndarray] = None, relu0: bool = False, relu1: bool = False) -> np.ndarray:
        """x0 f32 NHWC [B,H,W,C0], w f32 [Cout,ks,ks,C0+C1] -> f32 NHWC [B,H,W,Cout]."""
        x0 = np.ascontiguousarray(x0, dtype=np.float32)
        B, H, W_, C0 = x0.shape
        C1 = 0
        if x1 is not None:
            x1 = np.ascontiguousarray(x1, dtype=np.float32)
            C1 = x1.shape[-1]
        w = np.ascontiguousarray(w, dtype=np.float32)
        Cout = w.shape[0]
        out = np.zeros((B, H, W_, Cout), np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
        self._check(self.lib.ttr_dbg_conv(self.h, _f(x0), C0, _f(x1) if x1 is not None else None, C1, int(relu0), int(relu1), B, H, W_, ks, dil,
                                          _f(w), _f(b) if b is not None else None, Cout, act, _f(out)))
        return out

    def dbg_split_gemm(self, x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray] = None, np_products: int = 3, act: int = 0, out_planes: int = 0,
                       resid: Optional[np.ndarray] = None, cfg: int = 0) -> np.ndarray:
        """f16x4 engines: one split-operand linear, x f32 [M,K], w f32 [N,K] -> act(x w^T + bias (+ resid)) f32 [M,N] (tests)."""
        x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w, dtype=np.float32)
        M, K = x.shape
        N = w.shape[0]
        out = np.zeros((M, N), np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
        r = np.ascontiguousarray(resid, dtype=np.float32) if resid is not None else None
        self._check(self.lib.ttr_dbg_split_gemm(self.h, _f(x), M, K, _f(w), _f(b) if b is not None else None, N, np_products, act, out_planes,
                                                _f(r) if r is not None else None, cfg, _f(out)))
        return out

    def dbg_split_planes(self, x: np.ndarray, C_: int, planes: int = 3, relu: int = 0):
        """f16x4 engines: split_planes_kernel on host rows x f32 [M, ld] (the first C_ channels of each) -> (the f16 bit planes u16 [M, planes, C_] as the kernel
        wrote them, whether the launch's own range word tripped) (tests)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        M, ld = x.shape
        raw = np.zeros((M, int(planes), int(C_)), np.uint16)
        tripped = C.c_int32(0)
        self._check(self.lib.ttr_dbg_split_planes(self.h, _f(x), M, int(C_), ld, int(planes), int(relu), raw.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(tripped)))
        return raw, bool(tripped.value)

    def dbg_layernorm_planes(self, x: np.ndarray, gamma: np.ndarray, beta: np.ndarray, eps: float, planes: int = 3, tiled: int = 0) -> np.ndarray:
        """f16x4 engines: layernorm_planes_kernel on host rows x f32 [M, ld] (384 channels) -> the raw planes buffer u16 [M * planes * 384] in the kernel's own
        layout: rows [M][planes][384], or (tiled) [M / 8][plane][6 blocks of 64][8 rows][64] (tests)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        g = np.ascontiguousarray(gamma, dtype=np.float32); b = np.ascontiguousarray(beta, dtype=np.float32)
        if g.shape != (384,) or b.shape != (384,) or x.ndim != 2:
            raise ValueError("x [M, ld], gamma [384], beta [384]")
        M, ld = x.shape
        raw = np.zeros(M * int(planes) * 384, np.uint16)
        self._check(self.lib.ttr_dbg_layernorm_planes(self.h, _f(x), M, ld, _f(g), _f(b), float(eps), int(planes), int(tiled), raw.ctypes.data_as(C.POINTER(C.c_uint16))))
        return raw

    def dbg_ln_linear(self, x: np.ndarray, gamma: np.ndarray, beta: np.ndarray, eps: float, w: np.ndarray, bias: Optional[np.ndarray] = None,
                      fused: int = 0) -> np.ndarray:
        """f16x4 engines: the decoder's LayerNorm + linear pair, x f32 [M, 384], w f32 [N, 384] -> f32 [M, N]; fused = 0: the LayerNorm kernel then the skinny
        linear, 1: the skinny linear with the LayerNorm as its prologue (tests)."""
        x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w, dtype=np.float32)
        g = np.ascontiguousarray(gamma, dtype=np.float32); b = np.ascontiguousarray(beta, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != 384 or w.ndim != 2 or w.shape[1] != 384 or g.shape != (384,) or b.shape != (384,):
            raise ValueError("x [M, 384], w [N, 384], gamma [384], beta [384]")
        M, N = x.shape[0], w.shape[0]
        bs = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
        out = np.zeros((M, N), np.float32)
        self._check(self.lib.ttr_dbg_ln_linear(self.h, _f(x), M, _f(g), _f(b), float(eps), _f(w), _f(bs) if bs is not None else None, N, int(fused), _f(out)))
        return out


def gather_layout(counts: np.ndarray):
    """The framing of a gathered batch (ttr_gather_layout, host logic only): counts int32 [world, pages] -> (cap, total[world],
    first[world * pages + 1])."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    world, pages = counts.shape
    cap = C.c_int()
    total = np.zeros(world, np.int32)
    first = np.zeros(world * pages + 1, np.int64)
    if load().ttr_gather_layout(_i(counts), world, pages, C.byref(cap), _i(total), first.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise EngineError(load().ttr_last_error().decode())
    return cap.value, total, first


class Comm:
    """RCCL communicator pair of an engine (include/tuatara_hip.h, "multi-GPU"): one process per GPU.  `Comm(engine, rank, world,
    addr, port)`: rank 0 listens on addr:port and hands the NCCL ids to the others; `attach()` makes every batch of the engine
    all-gather its token ids on the engine's stream."""

    def __init__(self, engine: "Engine", rank: int, world: int, addr: str = "127.0.0.1", port: int = 29617, unique_id: Optional[bytes] = None,
                 transport: str = "rccl"):
        self.eng, self.lib = engine, engine.lib
        if transport == "socket":        # TCP through rank 0: ranks that share one GPU (tests), or where RCCL cannot initialise
            self.h = self.lib.ttr_comm_create_socket(engine.h, rank, world, addr.encode(), port)
        elif unique_id is not None:
            buf = C.create_string_buffer(unique_id, 256)
            self.h = self.lib.ttr_comm_create(engine.h, rank, world, buf)
        else:
            self.h = self.lib.ttr_comm_create_tcp(engine.h, rank, world, addr.encode(), port)
        if not self.h:
            raise EngineError(self.lib.ttr_last_error().decode())
        self.rank, self.world = rank, world

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(256)
        if load().ttr_comm_unique_id(buf) != 0:
            raise EngineError(load().ttr_last_error().decode())
        return buf.raw

    def attach(self, on: bool = True):
        if self.lib.ttr_engine_attach_comm(self.eng.h, self.h if on else None) != 0:
            raise EngineError(self.lib.ttr_last_error().decode())

    def allgather_host(self, mine: np.ndarray) -> np.ndarray:
        """Small host array of every rank, stacked by rank (collective; with an empty array: a barrier)."""
        mine = np.ascontiguousarray(mine)
        out = np.zeros((self.world,) + mine.shape, mine.dtype)
        if self.lib.ttr_comm_allgather_host(self.h, mine.ctypes.data_as(C.c_void_p), mine.nbytes, out.ctypes.data_as(C.c_void_p)) != 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        return out

    def barrier(self):
        self.allgather_host(np.zeros(1, np.int32))

    def describe(self) -> dict:
        """this rank's end of the communicator (ttr_comm_describe): rank, world, transport, RCCL version, HIP device, PCI bus id"""
        import json
        buf = C.create_string_buffer(512)
        if self.lib.ttr_comm_describe(self.h, buf, len(buf)) < 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        return json.loads(buf.value.decode())

    def describe_all(self) -> list:
        """every rank's describe(), by rank (collective)"""
        import json
        mine = np.zeros(512, np.uint8)
        raw = json.dumps(self.describe()).encode()[:511]
        mine[:len(raw)] = np.frombuffer(raw, np.uint8)
        return [json.loads(bytes(r).split(b"\0", 1)[0].decode()) for r in self.allgather_host(mine)]

    def last_gathered(self):
        """(counts int32 [world, pages], ids int32 [rows, 26]) of the batch whose results the engine returned last."""
        world, pages, need = C.c_int(), C.c_int(), C.c_size_t()
        self.lib.ttr_last_gathered(self.eng.h, C.byref(world), C.byref(pages), None, 0, None, 0, C.byref(need))
        counts = np.zeros((max(world.value, 0), max(pages.value, 0)), np.int32)
        ids = np.zeros((need.value // 26, 26), np.int32)
        self.lib.ttr_last_gathered(self.eng.h, None, None, _i(counts), counts.size, _i(ids), ids.size, None)
        return counts, ids

    def last_gathered_conf(self):
        """(conf f32 [rows], prob f32 [rows, 26]) of the same rows as last_gathered(), carried by the same collective."""
        rows = self.lib.ttr_last_gathered_conf(self.eng.h, None, 0, None, 0)
        if rows < 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        conf, prob = np.zeros(rows, np.float32), np.zeros((rows, 26), np.float32)
        self.lib.ttr_last_gathered_conf(self.eng.h, _f(conf), conf.size, _f(prob), prob.size)
        return conf, prob

    def pages_to_data_sharded(self, d_pages, n: int, h: int, w: int, conf: bool = False):
        """Latency mode (ttr_pages_to_data_dev_sharded): rank 0 passes the device pages, the others None."""
        ptr = d_pages.ptr if isinstance(d_pages, DeviceBuffer) else d_pages
        arr = (C.c_void_p * max(n, 1))()
        k = self.lib.ttr_pages_to_data_dev_sharded(self.h, ptr, n, h, w, arr)
        if k < 0:
            raise EngineError(self.lib.ttr_last_error().decode())
        return self.eng._take_many(arr, k, conf) if k else []

    def close(self):
        if getattr(self, "h", None):
            self.lib.ttr_comm_destroy(self.h)
            self.h = None
