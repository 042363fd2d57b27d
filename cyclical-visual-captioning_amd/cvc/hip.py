"""ctypes binding of libcvc_hip.so (include/cvc_hip.h) -- the only door between the host-side
module mirrors and the gfx950 kernels.

There is NO CPU fallback: if the library is missing or a tensor is not a contiguous fp32 CUDA
(ROCm) tensor, calls raise.  PyTorch is used for device memory and streams only; the pointers
handed over are raw `data_ptr()`s and the current HIP stream handle.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CVC_LIB: a variant library for A/B measurements -- tools/runs/build_variant.sh; the product loads the in-tree build)
LIB_PATH = os.environ.get("CVC_LIB") or os.path.join(_HERE, "lib", "libcvc_hip.so")

ATTN_ADDITIVE, ATTN_DOT = 0, 1


class AttnSet(C.Structure):
    _fields_ = [("proj", C.c_void_p), ("ctx", C.c_void_p), ("mask", C.c_void_p), ("frame_mask", C.c_void_p),
                ("scores", C.c_void_p), ("frame_masked", C.c_void_p), ("attn", C.c_void_p), ("ctx_out", C.c_void_p),
                ("n", C.c_int), ("stream", C.c_int)]


class GemmSeg(C.Structure):
    _fields_ = [("x", C.c_void_p), ("idx", C.c_void_p), ("w", C.c_void_p),
                ("k", C.c_int), ("ldx", C.c_int), ("ldw", C.c_int), ("relu", C.c_int)]


class NNSeg(C.Structure):
    _fields_ = [("w", C.c_void_p), ("dst", C.c_void_p), ("ldw", C.c_int), ("ncols", C.c_int), ("ld_dst", C.c_int)]


_P, _I, _F, _LL = C.c_void_p, C.c_int, C.c_float, C.c_longlong


class OptimSeg(C.Structure):
    """cvc_optim_seg (include/cvc_hip.h): one parameter of the fused clip + Adam / SGD / Adamax step"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_void_p), ("n", C.c_longlong),
                ("lr", C.c_float), ("weight_decay", C.c_float)]


class OptimChunk(C.Structure):
    _fields_ = [("seg", C.c_int), ("pad", C.c_int), ("start", C.c_longlong)]


class GskGroup(C.Structure):
    """cvc_gsk_group: one GEMM of a grouped stream-K launch (include/cvc_hip.h, "Grouped stream-K form")."""
    _fields_ = [("wp", C.c_void_p), ("w_blk_stride", C.c_longlong), ("xq", C.c_void_p), ("nblk", C.c_int), ("nchunk", C.c_int),
                ("skip_at", C.c_int), ("skip_n", C.c_int), ("slab", C.c_void_p), ("maxseg", C.c_int)]


class GskSegs(C.Structure):
    """cvc_gsk_segs: where a consumer finds one group's partial tiles."""
    _fields_ = [("slab", C.c_void_p), ("unit0", C.c_int), ("nchunk", C.c_int), ("U", C.c_int), ("maxseg", C.c_int)]


class DecodeDesc(C.Structure):
    """cvc_decode_desc of include/cvc_hip.h, field for field (tests/test_cabi.py compares the size with the C compiler's)."""
    _fields_ = (
        [(n, C.c_int) for n in ("B", "beam", "T", "N", "F", "R", "A", "E", "V", "unk_idx", "attn_kind")] +
        [("inv_temp", C.c_float)] +
        [(n, C.c_int) for n in ("stream_r", "stream_f", "path", "qsplit", "ks_gate", "ks_q", "ks_o", "ks_fc")] +
        [(n, C.c_void_p) for n in ("b_ih_att", "b_hh_att", "b_ih_lang", "b_hh_lang", "b_h", "w_a", "b_a", "b_o", "embed")] +
        [("w_fc", C.c_void_p), ("ld_w_fc", C.c_int)] +
        [(n, C.c_void_p) for n in ("w_att", "w_lang", "w_h", "w_o", "w_fc_frag")] +
        [(n, C.c_void_p) for n in ("fc", "conv", "pconv", "pool", "ppool", "mask")] +
        [(n, C.c_void_p) for n in ("words", "att_steps", "logprob", "score", "done", "parent")] +
        [(n, C.c_void_p) for n in ("gate_fc", "scores_r", "scores_f", "attn_f", "q", "q_parts", "top2_part")] +
        [("xa", C.c_void_p * 2), ("xl", C.c_void_p * 2), ("ca", C.c_void_p * 2), ("cl", C.c_void_p * 2), ("xa0_init", C.c_void_p)] +
        [(n, C.c_void_p) for n in ("xaf", "xlf", "xhf", "xff")] +
        [(n, C.c_longlong) for n in ("xaf_stride", "xlf_stride", "xhf_stride", "xff_stride")] +
        [(n, C.c_void_p) for n in ("parts_gate", "parts_o", "parts_fc", "logits")] +
        [(n, C.c_void_p) for n in ("h_att", "c_att", "h_lang", "c_lang", "c_att_prev", "c_lang_prev", "zero_state")] +
        [("beam_ws", C.c_void_p)] +
        [("gsk_nwg", C.c_int)] + [(n, C.c_void_p) for n in ("slab_att", "slab_lang", "slab_q", "slab_o", "emb_gate", "sel_counter")] +
        [("att_w_cached", C.c_int), ("lang_ksx", C.c_int), ("ksx_slab", C.c_void_p), ("ksx_flags", C.c_void_p)] +
        [("tail", C.c_int), ("tail_keys", C.c_void_p), ("tail_ms", C.c_void_p)])

class GradSrc(C.Structure):
    """cvc_grad_src: a gradient given as the sum of K-slice planes"""
    _fields_ = [("p", C.c_void_p), ("ld", C.c_longlong), ("plane_stride", C.c_longlong), ("nplanes", C.c_int)]


class PwBwdArgs(C.Structure):
    """cvc_pw_bwd_args of include/cvc_hip_blocks.h (one argument set of cvc_lstm_pointwise_bwd4_pair), field for field"""
    _fields_ = ([("d_h", GradSrc * 3), ("d_hd", C.c_void_p), ("rng_state", C.c_void_p), ("site", C.c_uint), ("p", C.c_float)] +
                [(n, C.c_void_p) for n in ("d_c", "gates", "c_prev", "c_new")] + [("M", C.c_int)] +
                [(n, C.c_void_p) for n in ("d_gates", "d_c_prev", "d_gates_q", "dg_sum")] + [("q_row0", C.c_int)])


class LstmStep(C.Structure):
    """cvc_lstm_step of include/cvc_hip.h ("Training loops driven from C"), field for field"""
    _fields_ = ([("wp", C.c_void_p), ("xq", C.c_void_p), ("K", C.c_int), ("M", C.c_int), ("R", C.c_int)] +
                [(n, C.c_void_p) for n in ("b_ih", "b_hh", "gate_pre", "row_bias", "row_index", "c_prev", "c_out", "gates_out", "h_out",
                                           "h_out2", "h_drop_out", "rng_state")] +
                [("site", C.c_uint), ("p", C.c_float), ("h_dst1_q", C.c_void_p), ("h_dst2_q", C.c_void_p), ("w_cached", C.c_int)])


class Constraint(C.Structure):
    """cvc_constraint of include/cvc_hip_blocks.h: the rules of cvc_constrained_select_parts (the two lists are device memory)."""
    _fields_ = [("no_repeat_ngram", C.c_int), ("no_immediate_repeat", C.c_int), ("min_len", C.c_int), ("nban", C.c_int),
                ("ban", C.c_void_p), ("bad_end", C.c_void_p), ("nbad", C.c_int)]


class EnsembleSrc(C.Structure):
    """cvc_ensemble_src of include/cvc_hip_blocks.h: one member's logits as a selection block takes them (device pointers)."""
    _fields_ = [("parts", C.c_void_p), ("nparts", C.c_int), ("part_stride", C.c_longlong), ("bias", C.c_void_p)]


ENSEMBLE_MAX = 8                 # CVC_ENSEMBLE_MAX


class TrainLoop(C.Structure):
    """cvc_train_loop of include/cvc_hip.h, field for field (tests/test_cabi.py compares the size with the C compiler's)."""
    _fields_ = (
        [(n, C.c_int) for n in ("kind", "B", "T", "R", "A", "N", "F", "attn_kind")] + [("inv_temp", C.c_float)] +
        [(n, C.c_void_p) for n in ("wp_att", "wp_lang", "b_ih_att", "b_hh_att", "b_ih_lang", "b_hh_lang", "w_ih_att", "w_hh_att",
                                   "w_ih_lang", "w_hh_lang")] +
        [("ld_ih_att", C.c_int), ("ld_ih_lang", C.c_int)] +
        [(n, C.c_void_p) for n in ("w_h", "b_h", "wp_h")] + [("q_split", C.c_int)] +
        [(n, C.c_void_p) for n in ("w_a", "b_a", "gpre_att", "row_bias", "row_index", "gpre_lang", "pool", "ppool", "conv",
                                   "pconv", "mask", "frame_mask", "rng_state")] +
        [("site0", C.c_uint), ("p", C.c_float)] +
        [(n, C.c_void_p) for n in ("out", "h_att", "h_att_prev", "h_lang_prev", "c_att", "c_lang", "g_att", "g_lang", "ctx", "q", "attn_r",
                                   "attn_f", "fm", "scores_ws")] +
        [("xa", C.c_void_p * 2), ("xl", C.c_void_p * 2)] +
        [(n, C.c_void_p) for n in ("d_out", "d_fm", "dg_att", "dg_lang", "dgsum_att", "dgsum_lang", "dq", "dwa_part", "ds_r", "ds_f", "d_pool", "d_ppool", "d_conv",
                                   "d_pconv", "bwd_ws", "d_ctx_all")])


# name -> argtypes, exactly the declarations of include/cvc_hip.h (tests/test_cabi.py checks both)
SIGNATURES = {
    "cvc_packed_lstm_step_fwd": [C.POINTER(LstmStep), _P],
    "cvc_attn_wsum_quad_rm": [C.POINTER(AttnSet), _I, _I, _I, _P, _P, _P],
    "cvc_attn_bwd_pair": [_I, C.POINTER(GradSrc), _P, _P, _F, C.POINTER(AttnSet), _I, C.POINTER(GradSrc), _I, _I, _I, _I, _P, _P, _P,
                          C.POINTER(_P), C.POINTER(_P), _P],
    "cvc_ctxfeat_bwd_steps": [_P, _P, _I, _I, _I, _I, _P, _P],
    "cvc_tile_gemm_big": [_I, _I],
    "cvc_tile_gemm_plan": [_I, _I, _I, _P, _P, _P],
    "cvc_dproj_bwd_steps": [_P, _LL, _LL, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "cvc_lstm_pointwise_bwd4": [C.POINTER(GradSrc), _P, _P, C.c_uint, _F, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P],
    "cvc_vocab_head_nll_fwd": [_P, _I, _LL, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _P],
    "cvc_scale_by_scalar": [_P, _P, _LL, _P, _P],
    "cvc_relu_dropout_fwd": [_P, _P, _LL, _I, _P, C.c_uint, _F, _P, _P],
    "cvc_relu_dropout_bwd": [_P, _P, _LL, _P, C.c_uint, _F, _P, _P],
    "cvc_bn_workspace": [_LL, _I],
    "cvc_bn_relu_train_fwd": [_P, _P, _P, _F, _F, _P, _P, _LL, _I, _P, _P, _P, _P, _P],
    "cvc_bn_relu_train_bwd": [_P, _P, _P, _P, _P, _P, _LL, _I, _P, _P, _P, _P, _P],
    "cvc_class_softmax_bwd": [_P, _P, _P, _P, _I, _I, _I, _P, _P],
    "cvc_layernorm_cat_bwd": [C.POINTER(_P), C.POINTER(_LL), C.POINTER(_I), _I, _LL, _F, _P, _LL, C.POINTER(_P), C.POINTER(_LL), _P],
    "cvc_bbox_overlaps_fwd": [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P],
    "cvc_label_glue_fwd": [_P, _P, _LL, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "cvc_attn_nll_fwd": [_P, _LL, _LL, _P, _LL, _LL, _P, _I, _I, _I, _P, _P, _P],
    "cvc_attn_nll_bwd": [_P, _LL, _LL, _P, _LL, _LL, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_train_loop_bwd_ws": [_I, _I, _I],
    "cvc_train_loop_fwd": [C.POINTER(TrainLoop), _P],
    "cvc_train_loop_bwd": [C.POINTER(TrainLoop), _P],
    "cvc_train_loops_bwd_joint": [C.POINTER(TrainLoop), C.POINTER(TrainLoop), _P],
    "cvc_stable_order": [_P, _I, _P, _P],
    "cvc_attn_weighted_rows": [_P, _P, _I, _I, _I, _I, _F, _P, _P],
    "cvc_col_sum": [_P, _LL, _I, _I, _P, _P, _P, _P],
    "cvc_col_sum_ws": [_I, _I],
    "cvc_train_loop_profile": [_I],
    "cvc_train_loop_profile_read": [C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _I],
    "cvc_attn_fwd": [_I, _P, _P, _P, _F, C.POINTER(AttnSet), _I, _I, _I, _I, _I, _P, _P],
    "cvc_attn_scores": [_I, _P, _P, _P, _F, C.POINTER(AttnSet), _I, _I, _I, _I, _P],
    "cvc_attn_scores_qparts": [_I, _P, _I, _P, _P, _P, _F, C.POINTER(AttnSet), _I, _I, _I, _I, _P],
    "cvc_linear_splitk_fwd": [C.POINTER(GemmSeg), _I, _P, _I, _I, _I, _P, _P],
    "cvc_linear_top2_fwd": [C.POINTER(GemmSeg), _I, _P, _I, _I, _P, _P, _P],
    "cvc_top2_final": [_P, _I, _I, _I, _P, _I, _P, _P, _I, _P, _I, _P],
    "cvc_attn_wsum_quad": [C.POINTER(AttnSet), _I, _I, _I, _I, _P, _P],
    "cvc_packed_lstm_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "cvc_packed_linear_fwd": [_P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P],
    "cvc_packed_lstm_wg_blocks": [_I],
    "cvc_packed_lstm_embgate_fwd": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "cvc_packed_lstm_embgate_ex_fwd": [_P, _LL, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P],
    "cvc_packed_linear_select_fwd": [_P, _P, _I, _P, _I, _I, _P, _P, _I, _P, _I, _P, _P],
    "cvc_gsk_plan": [C.POINTER(_I), C.POINTER(_I), _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)],
    "cvc_gsk_gemm": [C.POINTER(GskGroup), _I, _I, _P],
    "cvc_packed_lstm_late_fwd": [_P, _LL, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, C.POINTER(GskSegs), _P],
    "cvc_attn_scores_qslab": [_I, C.POINTER(GskSegs), _P, _P, _P, _F, C.POINTER(AttnSet), _I, _I, _I, _I, _P],
    "cvc_top2_slab": [C.POINTER(GskSegs), _P, _I, _I, _I, _P, _I, _P, _P, _I, _P, _I, _P],
    "cvc_packed_lstm_train_fwd": [_P, _P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_pack_lstm_weights": [_P, _I, _P, _I, _I, _P, _P],
    "cvc_pack_lstm_segs": [C.POINTER(_P), C.POINTER(_LL), C.POINTER(_I), _I, _I, _P, _P],
    "cvc_packed_lstm_train_pre_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_pack_quad_segs": [C.POINTER(_P), C.POINTER(_LL), C.POINTER(_I), _I, _I, _P, _P],
    "cvc_beam_backtrack": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "cvc_gru_seq_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P],
    "cvc_gru_seq_train_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P, _LL, _LL, _P],
    "cvc_lstm_pointwise_bwd4_pair": [C.POINTER(PwBwdArgs), C.POINTER(PwBwdArgs), _I, _P],
    "cvc_gru_persistent_halves": [_I],
    "cvc_gru_persistent_waves8": [_I],
    "cvc_gru_persistent_sync_words": [],
    "cvc_gru_seq_persistent_train_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P, _LL, _LL, _P, _P],
    "cvc_gru_seq_bwd_ksplit": [_I],
    "cvc_gru_bwd_persistent_sync_words": [],
    "cvc_gru_seq_bwd_persistent": [_P, _LL, _LL, _P, _LL, _LL, _P, _LL, _LL, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "cvc_linear_nn_planes_fwd": [_P, _I, _I, C.POINTER(NNSeg), _I, _I, _P, _P],
    "cvc_linear_nn_planes2_fwd": [_P, _P, _I, _I, _I, C.POINTER(NNSeg), _I, _I, _P, _I, _P],
    "cvc_gru_seq_bwd": [_P, _LL, _LL, _P, _LL, _LL, _P, _LL, _LL, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "cvc_gru_seq_persistent_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P, _P],
    # LSTM recurrence of the `bilstm` frame encoder (csrc/lstm_seq.hip; building blocks)
    "cvc_lstm_persistent_sync_words": [],
    "cvc_lstm_seq_persistent_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P, _P],
    "cvc_lstm_seq_persistent_train_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P, _LL, _LL, _P, _LL, _LL, _P, _P],
    "cvc_lstm_seq_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P],
    "cvc_lstm_seq_train_fwd": [_P, _P, _LL, _LL, _P, _P, _I, _I, _I, _I, _P, _P, _LL, _LL, _P, _LL, _LL, _P, _LL, _LL, _P],
    "cvc_lstm_seq_bwd_work": [_I, _I, _I],
    "cvc_lstm_seq_bwd": [_P, _LL, _LL, _P, _LL, _LL, _P, _LL, _LL, _P, _I, _I, _I, _I, _P, _P, _P],
    "cvc_packed_lstm_ks_slices": [_I, _I],
    "cvc_packed_lstm_ks_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _LL, _P],
    "cvc_packed_lstm_ksf_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_packed_lstm_ksx_local": [_I],
    "cvc_packed_lstm_ksx_fwd": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, C.c_uint, _P],
    "cvc_attn_wsum": [C.POINTER(AttnSet), _I, _I, _I, _I, _P, _P],
    "cvc_attn_bwd": [_I, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_linear_fwd": [C.POINTER(GemmSeg), _I, _P, _P, _I, _I, _P, _I, _P],
    "cvc_gemm_force_generic": [_I],
    "cvc_gemm_packed_split": [_I],
    "cvc_lstm_cell_fwd": [C.POINTER(GemmSeg), _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "cvc_lstm_pointwise_bwd": [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "cvc_lstm_pointwise_bwd3": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "cvc_linear_nn_fwd": [_P, _I, _I, C.POINTER(NNSeg), _I, _I, _P, _P],
    "cvc_pack_quad": [_P, _LL, _I, _I, _P, _P],
    "cvc_embed_relu_fwd": [_P, _P, _P, _I, _I, _P, _P],
    "cvc_embed_relu_bwd": [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P],
    "cvc_embed_relu_rng_fwd": [_P, _P, _P, C.c_uint, _F, _I, _I, _P, _P],
    "cvc_embed_relu_rng_bwd": [_P, _P, _P, _P, C.c_uint, _F, _P, _I, _I, _P, _P, _P],
    "cvc_dropout_rng": [_P, _LL, _P, C.c_uint, _F, _P, _P],
    "cvc_packed_lstm_train_drop_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, C.c_uint, _F, _P],
    "cvc_lstm_pointwise_bwd3_drop": [_P, _P, _P, _P, C.c_uint, _F, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "cvc_log_softmax_fwd": [_P, _I, _I, _P, _P],
    "cvc_log_softmax_bwd": [_P, _P, _I, _I, _P, _P],
    "cvc_nll_bwd": [_P, _P, _P, _I, _I, _P, _P],
    "cvc_top2_unk": [_P, _I, _I, _I, _P, _I, _P, _P],
    "cvc_nll_fwd": [_P, _P, _P, _I, _I, _P, _P],
    "cvc_vocab_nll_fwd": [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_bwd": [_P, _P, _P, _P, _P, _I, _I, _P, _P],
    "cvc_grounder_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "cvc_grounder_bwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "cvc_beam_select": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_beam_select_parts": [_P, _I, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "cvc_sample_select_parts": [_P, _I, _LL, _P, _I, _I, _I, _F, _P, _I, _P, _I, _P, _P],
    "cvc_sample_select_trunc_parts": [_P, _I, _LL, _P, _I, _I, _I, _F, _I, _F, _P, _I, _P, _I, _P, _P, _P, _P],
    "cvc_sample_advance": [_P, _P],
    # scheduled sampling: draw, coin, drawn-or-given word (csrc/mix.hip; building block)
    "cvc_mixed_select_parts": [_P, _I, _LL, _P, _I, _I, _I, _F, _P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P],
    "cvc_forced_select_parts": [_P, _I, _LL, _P, _I, _I, _P, _I, _P, _P, _P],
    "cvc_ensemble_logprobs": [C.POINTER(EnsembleSrc), _I, C.POINTER(_F), _I, _I, _I, _P, _I, _P],
    "cvc_ensemble_mix": [C.POINTER(_P), _I, C.POINTER(_F), _LL, _P, _P],
    "cvc_constrained_select_parts": [_P, _I, _LL, _P, _I, _I, _I, _F, _I, _F, _P, _I, _P, _I, _P, _P, _P, _P, _LL, C.POINTER(Constraint),
                                     _P, _P],
    "cvc_beam_select_hist_parts": [_P, _I, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _LL, C.POINTER(Constraint), _P, _P, _P, _P, _P,
                                   _P, _P],
    # diverse (group) beam search and the length-normalised final ranking (csrc/beam.hip; building blocks)
    "cvc_beam_select_groups_parts": [_P, _I, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _LL, C.POINTER(Constraint), _I, _F, _P, _P, _P,
                                     _P, _P, _P, _P],
    "cvc_beam_rank": [_P, _LL, _P, _I, _I, _I, _F, _P, _P, _P, _P],
    "cvc_beam_backtrack_from": [_P, _P, _P, _I, _I, _I, _I, _P, _LL, _P, _P, _P],
    # lexically constrained beam search: forced words per clip, banks, and its final ranking (csrc/beam.hip; building blocks)
    "cvc_beam_select_force_parts": [_P, _I, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _LL, C.POINTER(Constraint), _P, _I, _P, _P, _P,
                                    _P, _P, _P, _P, _P],
    "cvc_beam_rank_force": [_P, _LL, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P],
    # stochastic beam search: k distinct sampled captions per clip, in draw order (csrc/beam.hip; building block)
    "cvc_beam_select_stoch_parts": [_P, _I, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _LL, C.POINTER(Constraint), _F, _P, _P, _P,
                                    _P, _P, _P, _P, _P, _P, _P, _P, _P],
    # packed GEMMs with bf16-stored weights (the WB16 mode of csrc/gemm_packed.hip; building blocks)
    "cvc_packed_lstm_bf16w_fwd": [_P, _LL, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P],
    "cvc_packed_linear_bf16w_fwd": [_P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P],
    # greedy word choice without a selection launch (csrc/sel_keys.h; building blocks)
    "cvc_packed_linear_keys_fwd": [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P],
    "cvc_packed_lstm_embgate_keys_fwd": [_P, _LL, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _P],
    "cvc_keys_finalize": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    # self-critical training: CIDEr-D reward and per-token loss weights (csrc/cider.hip; building blocks)
    "cvc_cider_d": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _F, _F, _P, _P, _P],
    "cvc_scst_weights": [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P],
    # self-critical training without replacement: importance weights, per-row baseline, per-token weights (csrc/scst_wor.hip; building block)
    "cvc_scst_weights_wor": [_P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P],
    # token-overlap caption metrics: BLEU statistics, sentence BLEU, ROUGE-L (csrc/overlap.hip; building block)
    "cvc_caption_overlap": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    # consensus caption selection: pairwise CIDEr-D among a clip's candidates, pick and picked row (csrc/consensus.hip; building block)
    "cvc_consensus_cider": [_P, _P, _I, _I, _I, _P, _P, _I, _F, _F, _P, _P, _P, _P],
    "cvc_consensus_mix": [_P, _P, _P, _I, _I, _I, _P, _P, _I, _F, _F, _P, _P, _P, _P, _P, _P],
    # caption-set diversity: distinct n-grams, mBLEU statistics, distinct captions per clip (csrc/diversity.hip; building block)
    "cvc_caption_set_stats": [_P, _P, _I, _I, _I, _P, _P, _P, _P],
    # spectral caption-set diversity: similarity matrix, its eigenvalues, Self-CIDEr / LSA scores (csrc/spectrum.hip; building block)
    "cvc_caption_set_spectrum": [_P, _P, _I, _I, _I, _I, _P, _P, _I, _F, _P, _P, _P, _P, _P],
    # grounding F1 of generated captions: picks per object word and frame, per-class counters (csrc/grounding.hip; building block)
    "cvc_grounding_f1": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    # label smoothing in the vocabulary criterion: the fused head, the two-step form and its backward (csrc/vocab.hip; building blocks)
    "cvc_vocab_head_nll_ls_fwd": [_P, _I, _LL, _I, _P, _P, _P, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_ls_fwd": [_P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_ls_bwd": [_P, _P, _P, _P, _P, _I, _I, _F, _P, _P],
    # entropy regulariser in the vocabulary criterion: the same three forms with beta, the entropy weight and row_ent / ent_sum
    "cvc_vocab_head_nll_ent_fwd": [_P, _I, _LL, _I, _P, _P, _P, _P, _I, _I, _F, _F, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_ent_fwd": [_P, _P, _P, _P, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_ent_bwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _F, _P, _P],
    # word-level distillation in the vocabulary criterion: a dense teacher row (base, leading dimension, optional int32 row map, rows),
    # alpha and tau; row_kd / kd_sum beside the label-smoothing entries' outputs (csrc/distill.hip; building blocks)
    "cvc_vocab_head_nll_kd_fwd": [_P, _I, _LL, _I, _P, _P, _P, _P, _I, _P, _I, _I, _I, _F, _F, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_kd_fwd": [_P, _P, _P, _P, _I, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "cvc_vocab_nll_kd_bwd": [_P, _P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _F, _F, _P, _P],
    "cvc_gather_rows": [_P, _P, _I, _I, _I, _P, _P],
    "cvc_tile_rows_alloc": [_I],
    "cvc_tile_gemm_loaders": [_I],
    "cvc_tile_gemm": [_P, _P, _LL, _I, _I, _I, _I, _P, _I, _LL, _P],
    "cvc_tile_lstm_finish": [_P, _I, _LL, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _LL, _P, _LL, _P],
    "cvc_tile_lstm_finish_embgate": [_P, _I, _LL, _P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _P, _P, _P, _LL, _P, _LL, _P],
    "cvc_tile_linear_finish": [_P, _I, _LL, _I, _P, _P, _I, _I, _P, _I, _P],
    "cvc_tile_pack_rows": [_P, _I, _P, _I, _I, _I, _P, _LL, _P],
    "cvc_tile_pack_rows_any": [_P, _LL, _I, _I, _P, _LL, _P],
    "cvc_tile_pack_cols": [_P, _LL, _I, _I, _P, _LL, _P],
    "cvc_tile_reorder_pack": [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _LL, _P, _LL, _I, _I, _P],
    "cvc_attn_wsum_frag": [C.POINTER(AttnSet), _I, _I, _I, _I, _P, _LL, _P],
    "cvc_class_softmax_fwd": [_P, _LL, _P, _P, _I, _I, _I, _P, _P, _P],
    "cvc_layernorm_cat_fwd": [C.POINTER(_P), C.POINTER(_LL), C.POINTER(_I), _I, _LL, _F, _P, _LL, _P],
    "cvc_frame_embed_fwd": [_P, _P, _I, _P, _P, _I, _P, _P, _LL, _P, _P],
    "cvc_decode_plan_create": [C.POINTER(DecodeDesc), C.POINTER(C.c_void_p)],
    "cvc_decode_plan_destroy": [_P],
    "cvc_decode_plan_set_features": [_P, _P, _P, _P, _P, _P, _P],
    "cvc_decode_num_launches": [_P],
    "cvc_decode_greedy": [_P, _P],
    "cvc_decode_beam": [_P, _P],
    "cvc_optim_chunk_elems": [],
    "cvc_adam_clip_step": [_P, _I, _P, _I, _F, _F, _F, _F, _F, _I, _P, _P, _P, _P],
    "cvc_sgd_clip_step": [_P, _I, _P, _I, _F, _F, _F, _I, _P, _P, _P, _P],
    "cvc_adamax_clip_step": [_P, _I, _P, _I, _F, _F, _F, _F, _F, _I, _P, _P, _P, _P],
    # weight averaging inside the step: the plain entry's arguments, then ema (device pointer array), ema_state, decay, warmup
    "cvc_adam_clip_step_ema": [_P, _I, _P, _I, _F, _F, _F, _F, _F, _I, _P, _P, _P, _P, _P, _F, _I, _P],
    "cvc_sgd_clip_step_ema": [_P, _I, _P, _I, _F, _F, _F, _I, _P, _P, _P, _P, _P, _F, _I, _P],
    "cvc_adamax_clip_step_ema": [_P, _I, _P, _I, _F, _F, _F, _F, _F, _I, _P, _P, _P, _P, _P, _F, _I, _P],
    "cvc_ema_swap": [_P, _I, _P, _I, _P, _P],
    "cvc_comm_unique_id": [_P],
    "cvc_comm_init": [_I, _I, _P, C.POINTER(C.c_void_p)],
    "cvc_allreduce_grads": [_P, _P, _LL, _P],
    "cvc_comm_destroy": [_P],
}
_VOID_RETURN = {"cvc_decode_plan_destroy"}
# Building blocks (include/cvc_hip_blocks.h) and experimental forms (include/cvc_hip_experimental.h, only in a library built with
# CVC_EXPERIMENTAL=1) are NOT exported: they are bound through cvc_block("name").  Everything else in SIGNATURES is the exported
# drop-in ABI of include/cvc_hip.h.
BLOCKS = {
    "cvc_attn_scores", "cvc_attn_wsum", "cvc_attn_scores_qparts", "cvc_attn_wsum_quad", "cvc_attn_wsum_frag", "cvc_attn_wsum_quad_rm",
    "cvc_attn_bwd_pair", "cvc_ctxfeat_bwd_steps", "cvc_dproj_bwd_steps", "cvc_tile_gemm_big", "cvc_tile_gemm_plan", "cvc_linear_splitk_fwd", "cvc_linear_top2_fwd", "cvc_top2_final", "cvc_packed_lstm_fwd", "cvc_packed_linear_fwd",
    "cvc_packed_lstm_embgate_fwd", "cvc_packed_lstm_embgate_ex_fwd", "cvc_packed_lstm_late_fwd", "cvc_packed_lstm_train_fwd",
    "cvc_packed_lstm_train_pre_fwd", "cvc_packed_lstm_train_drop_fwd", "cvc_lstm_pointwise_bwd", "cvc_lstm_pointwise_bwd3",
    "cvc_lstm_pointwise_bwd3_drop", "cvc_pack_lstm_weights", "cvc_linear_nn_planes_fwd", "cvc_linear_nn_planes2_fwd", "cvc_gru_seq_train_fwd", "cvc_lstm_pointwise_bwd4_pair", "cvc_beam_select_parts", "cvc_sample_select_parts", "cvc_sample_select_trunc_parts", "cvc_sample_advance", "cvc_forced_select_parts", "cvc_constrained_select_parts", "cvc_beam_select_hist_parts", "cvc_beam_select_groups_parts", "cvc_beam_rank", "cvc_beam_select_force_parts", "cvc_beam_rank_force", "cvc_beam_select_stoch_parts", "cvc_beam_backtrack_from", "cvc_tile_lstm_finish",
    "cvc_tile_lstm_finish_embgate", "cvc_tile_reorder_pack", "cvc_decode_num_launches", "cvc_gemm_force_generic",
    "cvc_tile_gemm_loaders", "cvc_gru_persistent_waves8", "cvc_relu_dropout_fwd", "cvc_relu_dropout_bwd", "cvc_bn_workspace",
    "cvc_bn_relu_train_fwd", "cvc_bn_relu_train_bwd", "cvc_class_softmax_bwd", "cvc_layernorm_cat_bwd", "cvc_stable_order", "cvc_col_sum", "cvc_col_sum_ws", "cvc_attn_weighted_rows",
    "cvc_lstm_persistent_sync_words", "cvc_lstm_seq_persistent_fwd", "cvc_lstm_seq_persistent_train_fwd", "cvc_lstm_seq_fwd", "cvc_lstm_seq_train_fwd", "cvc_lstm_seq_bwd_work", "cvc_lstm_seq_bwd",
    "cvc_packed_lstm_bf16w_fwd", "cvc_packed_linear_bf16w_fwd",
    "cvc_packed_linear_keys_fwd", "cvc_packed_lstm_embgate_keys_fwd", "cvc_keys_finalize",
    "cvc_cider_d", "cvc_scst_weights", "cvc_scst_weights_wor", "cvc_mixed_select_parts", "cvc_caption_overlap", "cvc_consensus_cider", "cvc_consensus_mix",
    "cvc_caption_set_stats", "cvc_caption_set_spectrum", "cvc_grounding_f1", "cvc_vocab_head_nll_ls_fwd", "cvc_vocab_nll_ls_fwd", "cvc_vocab_nll_ls_bwd",
    "cvc_vocab_head_nll_ent_fwd", "cvc_vocab_nll_ent_fwd", "cvc_vocab_nll_ent_bwd", "cvc_ensemble_logprobs", "cvc_ensemble_mix",
    "cvc_vocab_head_nll_kd_fwd", "cvc_vocab_nll_kd_fwd", "cvc_vocab_nll_kd_bwd", "cvc_sgd_clip_step", "cvc_adamax_clip_step",
    "cvc_adam_clip_step_ema", "cvc_sgd_clip_step_ema", "cvc_adamax_clip_step_ema", "cvc_ema_swap"}
EXPERIMENTAL = {
    "cvc_gsk_plan", "cvc_gsk_gemm", "cvc_attn_scores_qslab", "cvc_top2_slab", "cvc_packed_lstm_ks_slices", "cvc_packed_lstm_ks_fwd",
    "cvc_packed_lstm_ksf_fwd", "cvc_packed_lstm_ksx_local", "cvc_packed_lstm_ksx_fwd", "cvc_packed_lstm_wg_blocks",
    "cvc_packed_linear_select_fwd", "cvc_gru_persistent_halves"}

_lib = None


def _missing(name):
    def fn(*_a, **_k):
        raise RuntimeError(f"{name} is an experimental form (include/cvc_hip_experimental.h): this libcvc_hip.so was built without "
                           "CVC_EXPERIMENTAL=1 (`CVC_EXPERIMENTAL=1 python cyclical-visual-captioning_amd/build_hip.py --force`)")
    return fn


def lib() -> C.CDLL:
    """Load libcvc_hip.so (built by build_hip.py / __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python cyclical-visual-captioning_amd/build_hip.py` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the caption-decode hot path.")
        l = C.CDLL(LIB_PATH)
        l.cvc_block.restype = C.c_void_p
        l.cvc_block.argtypes = [C.c_char_p]
        for name, argtypes in SIGNATURES.items():
            restype = None if name in _VOID_RETURN else (C.c_longlong if name in ("cvc_train_loop_bwd_ws", "cvc_bn_workspace", "cvc_col_sum_ws") else C.c_int)
            if name in BLOCKS or name in EXPERIMENTAL:
                addr = l.cvc_block(name.encode())
                if not addr:
                    if name in BLOCKS:
                        raise RuntimeError(f"{LIB_PATH}: building block {name} is not in the library's table (stale build?)")
                    setattr(l, name, _missing(name))
                    continue
                setattr(l, name, C.CFUNCTYPE(restype, *argtypes)(addr))
                continue
            fn = getattr(l, name)
            fn.argtypes = argtypes
            fn.restype = restype
        l.cvc_version.restype = C.c_char_p
        l.cvc_version.argtypes = []
        _lib = l
    return _lib


def experimental_built() -> bool:
    """was the loaded library built with CVC_EXPERIMENTAL=1?"""
    return b"+experimental" in lib().cvc_version()


def version() -> str:
    return lib().cvc_version().decode()


# --------------------------------------------------------------------------- weights generation
# Packed copies of parameters (the decode engine's weight packs, the encoder's GRU / dense-layer operands) are keyed on the
# parameters' (data_ptr, _version).  A fused optimizer kernel and a HIP-graph replay of the training step update parameters
# WITHOUT bumping _version, so every such cache also carries this process-wide generation; whoever updates weights behind
# autograd's back bumps it (Trainer after every optimizer step, the captioner's invalidate_decode_cache()).
_weights_generation = 0


def weights_generation() -> int:
    return _weights_generation


_warned = set()


def warn_once(key: str, msg: str):
    """One warning per process and reason: a path that leaves the HIP kernels for a library module says so (and why) once."""
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn("cvc: " + msg, RuntimeWarning, stacklevel=3)


def bump_weights_generation() -> int:
    global _weights_generation
    _weights_generation += 1
    return _weights_generation


# --------------------------------------------------------------------------- deferred error words (graph-captured training steps)
# The persistent GRU kernels (csrc/gru_persistent.hip, gru_bwd_persistent.hip) separate their time steps by a barrier in device
# memory with a BOUNDED spin: when a peer workgroup never arrives (the grid is not co-resident) the kernel raises an error word in
# its sync buffer instead of hanging the GPU, and its outputs are invalid.  Eagerly the caller reads that word on the host and
# repeats the layer in the per-step form -- a host read per layer, which nothing that is captured into a HIP graph can contain.
# Deferred mode keeps the verdict ON THE DEVICE: every launch ORs its error word into ONE status word (a stream operation), the
# optimizer pass reads it and leaves the parameters, moments and step counts untouched when it is set (cvc_adam_clip_step's `skip`),
# and the trainer reads it back together with the losses once per display interval, re-running the few steps it names on the
# per-step forms (cvc.trainer.Trainer.train).  A time-out therefore costs one re-run step, never a corrupted update.
_step_status: dict = {}
_deferred_status = None


def step_status(device) -> torch.Tensor:
    """the device's status word: int32[1], non-zero = some launch of the current step reported invalid outputs"""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _step_status.get(key)
    if t is None:
        t = _step_status[key] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
    return t


def defer_errors(status) -> None:
    """status = a step_status() tensor: error words are OR-ed into it from now on (no host reads); None: back to host reads"""
    global _deferred_status
    _deferred_status = status


def errors_deferred() -> bool:
    return _deferred_status is not None


def error_word_ok(word: torch.Tensor) -> bool:
    """`word`: a one-element int32 view of a launch's error word.  Deferred mode: OR it into the status word (stream operation,
    capturable) and report True -- the verdict is taken later; otherwise read it now (host sync)."""
    if _deferred_status is not None:
        _deferred_status.bitwise_or_(word)
        return True
    return int(word) == 0


# --------------------------------------------------------------------------- per-entry-point HIP-event timing (bench.py)
_raw_fns = {}
# entry points that launch nothing (sizes, switches, handles): an event pair around them would read as ~5 us of GPU time each
_HOST_ONLY = {"cvc_tile_gemm_big", "cvc_tile_rows_alloc", "cvc_tile_gemm_plan", "cvc_col_sum_ws", "cvc_train_loop_bwd_ws", "cvc_bn_workspace", "cvc_optim_chunk_elems", "cvc_version",
              "cvc_block", "cvc_gemm_packed_split", "cvc_gemm_force_generic", "cvc_tile_gemm_loaders", "cvc_gru_persistent_waves8",
              "cvc_lstm_persistent_sync_words", "cvc_lstm_seq_bwd_work",
              "cvc_decode_plan_create", "cvc_decode_plan_destroy", "cvc_decode_plan_set_features", "cvc_decode_num_launches",
              "cvc_train_loop_profile", "cvc_train_loop_profile_read", "cvc_comm_unique_id", "cvc_comm_init", "cvc_comm_destroy"}


TIMED_SHAPES: dict = {}      # enable_timers(): entry point -> the sizes of each of its launches (what bench.py prices a role's work with)
_SHAPE_ARGS = {
    "cvc_tile_gemm": lambda a: (int(a[3]), int(a[4]), int(a[5]), int(a[6])),            # (wb, xb, x_mblk_stride, K, M, N, ksplit, ...)
    "cvc_tile_pack_rows_any": lambda a: (int(a[2]), int(a[3])),                         # (x, ldx, M, K, ...)
    "cvc_tile_pack_cols": lambda a: (int(a[2]), int(a[3])),                             # (x, ldx, S, C, ...)
    "cvc_pack_lstm_segs": lambda a: (sum(int(a[2][i]) for i in range(int(a[3]))), int(a[4])),     # (ws, lds, widths, nseg, R, ...) -> (K, R)
    # (kind, q, w_a, inv_temp, proj, ctx, attn, d_ctx, d_fm, nclip, nq, n, A, R, d_scores, d_q, d_w_part, d_proj, d_ctxfeat)
    "cvc_attn_bwd": lambda a: (int(a[9]), int(a[10]), int(a[11]), int(a[12]), int(a[13]), bool(a[7]), bool(a[17]), bool(a[18])),
}


def enable_timers() -> dict:
    """Bracket every C-ABI launch with a HIP-event pair on the launch stream (torch's current stream, which is the stream
    handed to the entry point).  Returns the dict that fills up: entry-point name -> [(start_event, end_event)]; the (K, M, N) of
    every cvc_tile_gemm launch go to TIMED_SHAPES (what bench.py prices the dense products' roofline with).
    Measurement aid for bench.py (--mode train); the product path never enables it."""
    l = lib()
    timers: dict = {}
    TIMED_SHAPES.clear()
    if _raw_fns:
        disable_timers()
    for name in SIGNATURES:
        if name in _HOST_ONLY:
            continue
        raw = getattr(l, name)
        _raw_fns[name] = raw

        def timed(*args, _raw=raw, _name=name):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = _raw(*args)
            e1.record()
            timers.setdefault(_name, []).append((e0, e1))
            pick = _SHAPE_ARGS.get(_name)
            if pick is not None:
                TIMED_SHAPES.setdefault(_name, []).append(pick(args))
            return rc
        setattr(l, name, timed)
    return timers


def disable_timers():
    l = lib()
    for name, raw in _raw_fns.items():
        setattr(l, name, raw)
    _raw_fns.clear()


def _check(rc: int, name: str):
    if rc != 0:
        kind = {-1: "bad argument (size/alignment precondition)", -2: "dimension not covered by the kernel templates",
                -3: "librccl.so could not be opened"}.get(
            rc, f"hipError_t {rc}")
        raise RuntimeError(f"{name} failed: {kind}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Optional[torch.Tensor], dtype=torch.float32, name="tensor") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"cvc.hip: {name} must live on the GPU (no CPU fallback for the hot path)")
    if t.dtype != dtype:
        raise RuntimeError(f"cvc.hip: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"cvc.hip: {name} must be contiguous")
    return t.data_ptr()


def ensemble_log_weights(weights, M: int) -> np.ndarray:
    """The log-weights cvc_ensemble_logprobs / cvc_ensemble_mix take (fp32 [M]): None = uniform, else M finite numbers > 0,
    normalised in fp64 to sum to 1, the log rounded once to fp32.  Anything else raises RuntimeError."""
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or not 1 <= M <= ENSEMBLE_MAX:
        raise RuntimeError(f"ensemble_log_weights: an ensemble has 1 .. {ENSEMBLE_MAX} members, got {M!r}")
    if weights is None:
        w = np.ones(M, dtype=np.float64)
    else:
        try:
            w = np.array([float(v) for v in weights], dtype=np.float64)
        except (TypeError, ValueError):
            raise RuntimeError(f"ensemble_log_weights: the weights must be {M} numbers, got {weights!r}") from None
        if w.shape != (M,):
            raise RuntimeError(f"ensemble_log_weights: {M} members need {M} weights, got {len(w)}")
        if not np.all(np.isfinite(w)) or not np.all(w > 0):
            raise RuntimeError(f"ensemble_log_weights: every weight must be a finite number > 0, got {list(w)}")
    return np.log(w / w.sum()).astype(np.float32)


def _mask(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """bool / uint8 mask -> contiguous uint8 view (one byte per element)."""
    if t is None:
        return None
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).contiguous().view(torch.uint8)
    return t.contiguous()


def gsk_plan(ntile: Sequence[int], nchunk: Sequence[int], nwg: int) -> dict:
    """Host arithmetic of a grouped stream-K launch (cvc_gsk_plan): units per workgroup, each group's first unit and the
    segments per tile its slab must hold."""
    n = len(ntile)
    arr = lambda v: (C.c_int * n)(*[int(x) for x in v])
    U, unit0, maxseg = C.c_int(), (C.c_int * n)(), (C.c_int * n)()
    _check(lib().cvc_gsk_plan(arr(ntile), arr(nchunk), n, int(nwg), C.byref(U), unit0, maxseg), "cvc_gsk_plan")
    return dict(U=U.value, unit0=list(unit0), maxseg=list(maxseg), nwg=int(nwg))


# --------------------------------------------------------------------------- attention
def attn_fwd(kind: int, q: torch.Tensor, w_a: Optional[torch.Tensor], b_a: Optional[torch.Tensor], inv_temp: float,
             sets: Sequence[dict], nclip: int, nq: int, want_ctx: bool = True, want_sum: bool = False):
    """sets: dicts with proj [nclip,n,A], ctx [nclip,n,R], mask, frame_mask.  Returns
    ([(scores, frame_masked, attn, ctx_out)], ctx_sum)."""
    rows, A = q.shape
    assert rows == nclip * nq
    R = sets[0]["ctx"].shape[2]
    arr = (AttnSet * len(sets))()
    outs, keep = [], []
    for i, s in enumerate(sets):
        n = s["proj"].shape[1]
        assert s["proj"].shape == (nclip, n, A) and s["ctx"].shape == (nclip, n, R), (s["proj"].shape, s["ctx"].shape)
        m, fmk = _mask(s.get("mask")), _mask(s.get("frame_mask"))
        if m is not None:
            assert m.shape == (nclip, n)
        if fmk is not None:
            assert fmk.shape == (rows, n)
        scores = torch.empty(rows, n, device=q.device, dtype=torch.float32)
        attn = torch.empty_like(scores)
        fm = torch.empty_like(scores) if fmk is not None else None
        ctx_out = torch.empty(rows, R, device=q.device, dtype=torch.float32) if want_ctx else None
        arr[i] = AttnSet(_dev(s["proj"], name="proj"), _dev(s["ctx"], name="ctx"), _dev(m, torch.uint8), _dev(fmk, torch.uint8),
                         _dev(scores), _dev(fm), _dev(attn), _dev(ctx_out), n, 4 if s.get("sentinel") else 0)
        keep += [m, fmk]
        outs.append((scores, fm, attn, ctx_out))
    ctx_sum = torch.empty(rows, R, device=q.device, dtype=torch.float32) if want_sum else None
    _check(lib().cvc_attn_fwd(kind, _dev(q, name="q"), _dev(w_a), _dev(b_a), float(inv_temp), arr, len(sets), nclip, nq, A, R,
                              _dev(ctx_sum), _stream()), "cvc_attn_fwd")
    return outs, ctx_sum


def attn_bwd(kind: int, q, w_a, inv_temp: float, proj, ctx, attn, d_ctx, d_fm, nclip: int, nq: int,
             want_d_proj: bool, want_d_ctxfeat: bool, want_d_w: bool):
    rows, A = q.shape
    n, R = proj.shape[1], ctx.shape[2]
    d_scores = torch.empty(rows, n, device=q.device, dtype=torch.float32)
    d_q = torch.empty_like(q)
    d_w_part = torch.empty_like(q) if (want_d_w and kind == ATTN_ADDITIVE) else None
    d_proj = torch.zeros_like(proj) if want_d_proj else None
    d_ctxfeat = torch.zeros_like(ctx) if (want_d_ctxfeat and d_ctx is not None) else None
    _check(lib().cvc_attn_bwd(kind, _dev(q), _dev(w_a), float(inv_temp), _dev(proj), _dev(ctx), _dev(attn), _dev(d_ctx),
                              _dev(d_fm), nclip, nq, n, A, R, _dev(d_scores), _dev(d_q), _dev(d_w_part), _dev(d_proj),
                              _dev(d_ctxfeat), _stream()), "cvc_attn_bwd")
    return d_scores, d_q, d_w_part, d_proj, d_ctxfeat


# --------------------------------------------------------------------------- skinny GEMM / LSTM cell
def _segs(segs: Sequence[dict], M: int):
    """segs: dicts {x: [M,k] (or table with idx), w: [Nout, k] (a column slice is fine), idx, relu}."""
    arr = (GemmSeg * len(segs))()
    for i, s in enumerate(segs):
        x, w = s["x"], s["w"]
        k = w.shape[1]
        if x.stride(-1) != 1 or w.stride(-1) != 1:
            raise RuntimeError("cvc.hip: GEMM segments must have unit inner stride")
        idx = s.get("idx")
        if idx is None:
            assert x.shape[0] == M and x.shape[1] == k, (x.shape, M, k)
        else:
            assert idx.shape == (M,) and x.shape[1] == k
            _dev(idx, torch.int64, "idx")
        for t_ in (x, w):
            if not t_.is_cuda or t_.dtype != torch.float32:
                raise RuntimeError("cvc.hip: GEMM operands must be fp32 GPU tensors (no CPU fallback)")
        arr[i] = GemmSeg(x.data_ptr(), None if idx is None else idx.data_ptr(), w.data_ptr(), k, x.stride(0), w.stride(0),
                         1 if s.get("relu") else 0)
    return arr


def linear_fwd(segs: Sequence[dict], bias: Optional[torch.Tensor], M: int, Nout: int, bias2=None, out=None):
    dev = segs[0]["w"].device
    y = out if out is not None else torch.empty(M, Nout, device=dev, dtype=torch.float32)
    arr = _segs(segs, M)
    _check(lib().cvc_linear_fwd(arr, len(segs), _dev(bias), _dev(bias2), M, Nout, _dev(y), y.stride(0), _stream()),
           "cvc_linear_fwd")
    return y


_split_mode_cache = None


def gemm_packed_split(mode: int) -> int:
    """Packed decode GEMMs: 0 = plain fp32 MFMA, 1 = bf16x3-split products on the bf16 MFMA with 4 waves per
    workgroup, 2 = the same with 8 waves (two per SIMD).  -> previous setting.  A negative mode only queries (cached on the
    host: the backward pass asks once per LSTM step)."""
    global _split_mode_cache
    if mode < 0 and _split_mode_cache is not None:
        return _split_mode_cache
    prev = int(lib().cvc_gemm_packed_split(int(mode)))
    _split_mode_cache = prev if mode < 0 else (2 if mode > 2 else int(mode))
    return prev


def gemm_force_generic(on: bool) -> bool:
    return bool(lib().cvc_gemm_force_generic(1 if on else 0))


def lstm_cell_fwd(segs: Sequence[dict], b_ih, b_hh, c_prev, want_gates: bool = False, h_out=None, c_out=None,
                  gate_bias=None):
    M, R = c_prev.shape
    h = h_out if h_out is not None else torch.empty_like(c_prev)
    c = c_out if c_out is not None else torch.empty_like(c_prev)
    gates = torch.empty(M, 4 * R, device=c_prev.device, dtype=torch.float32) if want_gates else None
    arr = _segs(segs, M)
    _check(lib().cvc_lstm_cell_fwd(arr, len(segs), _dev(b_ih), _dev(b_hh), _dev(gate_bias), _dev(c_prev), M, R, _dev(h),
                                   _dev(c), _dev(gates), _stream()), "cvc_lstm_cell_fwd")
    return h, c, gates


# ---- training form of the packed gate GEMM: the weights are re-packed once per optimizer step, the cell's inputs per call
_train_generation = 0


def lstm_train_new_step() -> None:
    """Called by the model at the start of every training forward: the packed LSTM weights are rebuilt at their first use of
    the step whatever their autograd version says (a captured training step must contain the re-pack launch)."""
    global _train_generation
    _train_generation += 1
    _step_operands.clear()


# tile-GEMM operand packs of WEIGHTS (or column slices of them), shared by every product of one training step that reads the same
# weight the same way: the vocabulary head is multiplied in both loops and read again by both backward-data products, the embedding
# columns of the attention cell by both loops' hoisted products and both d_emb products.  Cleared at the start of every forward.
_step_operands = {}


def weight_operand(w: torch.Tensor, kmajor: bool = False) -> "TileOperand":
    key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()), bool(kmajor), _train_generation, w._version)
    op = _step_operands.get(key)
    if op is None:
        op = _step_operands[key] = TileOperand(w.detach(), kmajor)
    return op


def lstm_train_ok(M: int, R: int, widths: Sequence[int]) -> bool:
    return 1 <= M <= 64 and R % 8 == 0 and all(w % 4 == 0 and w >= 4 for w in widths) and sum(widths) % 32 == 0


def lstm_train_pack(w_ih: torch.Tensor, w_hh: torch.Tensor, cols: Optional[Sequence] = None) -> torch.Tensor:
    """Packed copy [R/8][K/4][32][4] of an LSTM cell's weights for cvc_packed_lstm_train_fwd: all of weight_ih, or only its
    column ranges `cols` = ((col0, width), ...) (the recurrent inputs of a hoisted cell), followed by weight_hh.  The packs live
    ON the weight tensor object (they die with it: no table keyed by addresses that a later tensor could reuse), one per `cols`,
    and are rebuilt when the step generation, either tensor's version counter or either address changed."""
    R = w_hh.shape[1]
    key = None if cols is None else tuple((int(c0), int(n)) for c0, n in cols)
    stamp = (_train_generation, w_ih._version, w_hh._version, w_ih.data_ptr(), w_hh.data_ptr(), tuple(w_ih.shape))
    packs = getattr(w_ih, "_cvc_train_packs", None)
    if packs is None:
        packs = w_ih._cvc_train_packs = {}
    ent = packs.get(key)
    if ent is not None and ent[1] == stamp:
        return ent[0]
    K_hh = w_hh.shape[1]
    ranges = [(0, w_ih.shape[1])] if key is None else list(key)
    K = sum(n for _, n in ranges) + K_hh
    shape = (R // 8, K // 4, 32, 4)
    wp = ent[0] if (ent is not None and tuple(ent[0].shape) == shape and ent[0].device == w_ih.device) else \
        torch.empty(*shape, device=w_ih.device, dtype=torch.float32)
    n = len(ranges) + 1
    ptrs = (_P * n)(*[w_ih.data_ptr() + 4 * c0 for c0, _ in ranges], w_hh.data_ptr())
    lds = (_LL * n)(*[w_ih.stride(0)] * len(ranges), w_hh.stride(0))
    ws = (_I * n)(*[nn_ for _, nn_ in ranges], K_hh)
    _check(lib().cvc_pack_lstm_segs(ptrs, lds, ws, n, R, _dev(wp), _stream()), "cvc_pack_lstm_segs")
    packs[key] = (wp, stamp)
    return wp


def linear_train_pack(w: torch.Tensor) -> torch.Tensor:
    """Packed copy [Nout/32][K/4][32][4] of a linear layer's weight [Nout, K] for cvc_packed_linear_fwd (the training loop's
    h2attn): lives on the weight tensor like the LSTM packs, rebuilt when the step generation / version / address changed."""
    n, k = w.shape
    assert n % 32 == 0 and k % 32 == 0
    stamp = (_train_generation, w._version, w.data_ptr(), (n, k))
    ent = getattr(w, "_cvc_linear_pack", None)
    if ent is not None and ent[1] == stamp:
        return ent[0]
    wp = ent[0] if (ent is not None and tuple(ent[0].shape) == (n // 32, k // 4, 32, 4) and ent[0].device == w.device) else \
        torch.empty(n // 32, k // 4, 32, 4, device=w.device, dtype=torch.float32)
    with torch.no_grad():
        wp.copy_(w.detach().view(n // 32, 32, k // 4, 4).permute(0, 2, 1, 3))       # one strided copy
    w._cvc_linear_pack = (wp, stamp)
    return wp


def pack_quad_segs(xs: Sequence[torch.Tensor]) -> torch.Tensor:
    """Row-major segments [M <= 64, k_s] -> one quad-layout operand [sum k_s / 4][64][4]."""
    n, M = len(xs), xs[0].shape[0]
    ptrs = (_P * n)(*[x.data_ptr() for x in xs])
    lds = (_LL * n)(*[x.stride(0) for x in xs])
    ws = (_I * n)(*[x.shape[1] for x in xs])
    xq = torch.empty(sum(x.shape[1] for x in xs) // 4, 64, 4, device=xs[0].device, dtype=torch.float32)
    _check(lib().cvc_pack_quad_segs(ptrs, lds, ws, n, M, _dev(xq), _stream()), "cvc_pack_quad_segs")
    return xq


def lstm_cell_train_fwd(xs: Sequence[torch.Tensor], h_prev, c_prev, wp, b_ih, b_hh, want_gates: bool = True, copies: int = 1,
                        gate_pre: Optional[torch.Tensor] = None, drop=None):
    """nn.LSTMCell forward on the packed gate GEMM (cvc_packed_lstm_train_fwd) from the pack `lstm_train_pack` built:
    -> h (a tuple of `copies` identical tensors when copies > 1), c, activated gates (or None).  gate_pre [M, 4R]: the
    contribution of input segments multiplied beforehand for all steps (hoisted cell); xs are then the remaining segments.
    drop = (rng_state, site, p): one more output tensor, nn.Dropout(h') with the in-kernel mask (copies <= 2 then):
    -> (h or tuple of h, h_dropped), c, gates."""
    M, R = c_prev.shape
    xq = pack_quad_segs([*xs, h_prev])
    c = torch.empty_like(c_prev)
    gates = torch.empty(M, 4 * R, device=c_prev.device, dtype=torch.float32) if want_gates else None
    if drop is not None:
        state, site, p = drop
        hs = [torch.empty_like(c_prev) for _ in range(max(1, min(2, copies)))]
        hd = torch.empty_like(c_prev)
        _check(lib().cvc_packed_lstm_train_drop_fwd(_dev(wp), _dev(xq), xq.shape[0] * 4, _dev(b_ih), _dev(b_hh), _dev(gate_pre),
                                                    _dev(c_prev), M, R, _dev(hs[0]), _dev(c), _dev(gates),
                                                    _dev(hs[1]) if len(hs) > 1 else None, _dev(hd), _rng_ptr(state), int(site),
                                                    float(p), _stream()), "cvc_packed_lstm_train_drop_fwd")
        return ((hs[0] if copies <= 1 else tuple(hs)), hd), c, gates
    hs = [torch.empty_like(c_prev) for _ in range(max(1, min(3, copies)))]
    tail = (_dev(c_prev), M, R, _dev(hs[0]), _dev(c), _dev(gates), _dev(hs[1]) if len(hs) > 1 else None,
            _dev(hs[2]) if len(hs) > 2 else None, _stream())
    if gate_pre is None:
        _check(lib().cvc_packed_lstm_train_fwd(_dev(wp), _dev(xq), xq.shape[0] * 4, _dev(b_ih), _dev(b_hh), *tail), "cvc_packed_lstm_train_fwd")
    else:
        _check(lib().cvc_packed_lstm_train_pre_fwd(_dev(wp), _dev(xq), xq.shape[0] * 4, _dev(b_ih), _dev(b_hh), _dev(gate_pre), *tail),
               "cvc_packed_lstm_train_pre_fwd")
    return (hs[0] if copies <= 1 else tuple(hs)), c, gates


def lstm_pointwise_bwd(d_h, d_c, gates, c_prev, c_new, want_quad=False, d_h2=None, d_h3=None, drop3=None):
    """-> d_gates [M,4R], d_c_prev [M,R] (+ d_gates in the quad layout [R][64][4] for linear_nn when asked).  d_h2, d_h3: the
    gradients of further copies of h' (summed with d_h inside the kernel).  drop3 = (rng_state, site, p): d_h3 is the gradient
    of the copy that left the cell through the fused dropout and takes that mask."""
    M, R = c_prev.shape
    d_gates = torch.empty_like(gates)
    d_c_prev = torch.empty_like(c_prev)
    d_gates_q = torch.empty(R, 64, 4, device=gates.device, dtype=torch.float32) if want_quad else None
    if drop3 is not None and d_h3 is not None:
        state, site, p = drop3
        _check(lib().cvc_lstm_pointwise_bwd3_drop(_dev(d_h), _dev(d_h2), _dev(d_h3), _rng_ptr(state), int(site), float(p), _dev(d_c),
                                                  _dev(gates), _dev(c_prev), _dev(c_new), M, R, _dev(d_gates), _dev(d_c_prev),
                                                  _dev(d_gates_q), _stream()), "cvc_lstm_pointwise_bwd3_drop")
        return (d_gates, d_c_prev, d_gates_q) if want_quad else (d_gates, d_c_prev)
    _check(lib().cvc_lstm_pointwise_bwd3(_dev(d_h), _dev(d_h2), _dev(d_h3), _dev(d_c), _dev(gates), _dev(c_prev), _dev(c_new), M, R,
                                         _dev(d_gates), _dev(d_c_prev), _dev(d_gates_q), _stream()), "cvc_lstm_pointwise_bwd3")
    return (d_gates, d_c_prev, d_gates_q) if want_quad else (d_gates, d_c_prev)


def linear_nn_ok(M, K, ranges):
    """Shapes cvc_linear_nn_fwd accepts (everything else keeps the library GEMM)."""
    return M <= 64 and K % 8 == 0 and all(
        n >= 4 and n % 4 == 0 and w.stride(0) % 4 == 0 and w.stride(1) == 1 and c0 % 4 == 0 and w.data_ptr() % 16 == 0
        for (w, c0, n) in ranges)


def pack_quad(x: torch.Tensor) -> torch.Tensor:
    """[M <= 64, K] row-major -> [K/4][64][4] (linear_nn's dY layout)."""
    M, K = x.shape
    xq = torch.empty(K // 4, 64, 4, device=x.device, dtype=torch.float32)
    _check(lib().cvc_pack_quad(_dev(x), x.stride(0), M, K, _dev(xq), _stream()), "cvc_pack_quad")
    return xq


def linear_nn(dy_q, M, K, ranges, ksplit=None):
    """dX_s[M, n_s] = dY[M, K] @ W_s[:, c0_s : c0_s + n_s] for every (W_s, c0_s, n_s) in `ranges`, one launch.
    dy_q: dY in the quad layout [K/4][64][4] (lstm_pointwise_bwd(want_quad=True))."""
    arr = (NNSeg * len(ranges))()
    outs, keep = [], []
    slabs = 0
    for i, (w, c0, n) in enumerate(ranges):
        assert w.shape[0] == K and w.is_cuda and w.dtype == torch.float32
        out = torch.empty(M, n, device=w.device, dtype=torch.float32)
        arr[i] = NNSeg(w.data_ptr() + 4 * c0, out.data_ptr(), w.stride(0), n, n)
        outs.append(out)
        slabs += (n + 127) // 128
    # K slices: one resident round of workgroups and >= 16 rows (two double groups) per wave in every slice -- a short K on few
    # column slabs (h2attn's backward) is a latency-bound launch that wants the whole chip, not long K loops
    if ksplit is None:
        # the split-product kernel holds one workgroup per CU (256 on the chip), the fp32-MFMA kernel two
        resident = 256 if gemm_packed_split(-1) != 0 else 512
        ksplit = max(1, min(K // 8 // 16, resident // slabs))
    ws = torch.empty(ksplit * M * slabs * 128, device=dy_q.device, dtype=torch.float32) if ksplit > 1 else None
    _check(lib().cvc_linear_nn_fwd(_dev(dy_q), K, M, arr, len(ranges), ksplit, _dev(ws), _stream()), "cvc_linear_nn_fwd")
    return outs


# --------------------------------------------------------------------------- embedding / vocabulary head
def embed_relu_fwd(table, idx, drop=None):
    M, E = idx.shape[0], table.shape[1]
    out = torch.empty(M, E, device=table.device, dtype=torch.float32)
    _check(lib().cvc_embed_relu_fwd(_dev(table), _dev(idx, torch.int64), _dev(drop), M, E, _dev(out), _stream()),
           "cvc_embed_relu_fwd")
    return out


def _rng_ptr(state: torch.Tensor):
    """device pointer of a dropout generator state (cvc/dropout.py: >= 3 int32 words {seed_lo, seed_hi, step})"""
    if not (state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= 3):
        raise RuntimeError("dropout generator state: contiguous int32 device tensor of >= 3 words")
    return state.data_ptr()


def embed_relu_rng_fwd(table, idx, state, site: int, p: float):
    """relu(table[idx]) * in-kernel keep-mask of (site, element index) (cvc_embed_relu_rng_fwd)"""
    M, E = idx.shape[0], table.shape[1]
    out = torch.empty(M, E, device=table.device, dtype=torch.float32)
    _check(lib().cvc_embed_relu_rng_fwd(_dev(table), _dev(idx, torch.int64), _rng_ptr(state), int(site), float(p), M, E, _dev(out),
                                        _stream()), "cvc_embed_relu_rng_fwd")
    return out


_order_cache = {}


def _embed_order(idx: torch.Tensor) -> torch.Tensor:
    """stable argsort of the word indices (rows grouped by word), cached for the step: loops A and C embed the same words"""
    key = (idx.data_ptr(), idx.numel(), idx._version, _train_generation)
    o = _order_cache.get(key)
    if o is None:
        if len(_order_cache) > 16:
            _order_cache.clear()
        o = _order_cache[key] = (stable_order(idx), idx)      # (idx kept alive: its address is the key)
    return o[0]


def stable_order(idx: torch.Tensor) -> torch.Tensor:
    """torch.argsort(idx, stable=True) for a 1-d int64 tensor (one launch, cvc_stable_order, up to 7168 keys)"""
    idx = idx.contiguous()
    if idx.dim() != 1 or idx.dtype != torch.int64 or not 1 <= idx.numel() <= 7168:
        return torch.argsort(idx, stable=True)
    order = torch.empty_like(idx)
    _check(lib().cvc_stable_order(_dev(idx, torch.int64), idx.numel(), _dev(order, torch.int64), _stream()), "cvc_stable_order")
    return order


def col_sum(x: torch.Tensor, out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [S, n] (unit inner stride) -> sum over rows [n], written to `out` (and `out2`) when given: bias gradients"""
    assert x.dim() == 2 and x.dtype == torch.float32
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    S, n = x.shape
    if out is None:
        out = torch.empty(n, device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == n and (out2 is None or (out2.is_contiguous() and out2.numel() == n))
    if not x.is_cuda:
        raise RuntimeError("cvc.hip: col_sum input must live on the GPU (no CPU fallback for the hot path)")
    nws = int(lib().cvc_col_sum_ws(S, n))
    ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
    _check(lib().cvc_col_sum(x.data_ptr(), x.stride(0), S, n, _dev(out), _dev(out2), _dev(ws), _stream()), "cvc_col_sum")
    return out


def embed_relu_rng_bwd(table, idx, state, site: int, p: float, d_out, d_table=None):
    """d_table given: ACCUMULATED into (several lookups of one table add up in one buffer)"""
    if d_table is None:
        d_table = torch.zeros_like(table)
    order = _embed_order(idx)
    ws = torch.empty(idx.shape[0], table.shape[1], device=table.device, dtype=torch.float32)
    _check(lib().cvc_embed_relu_rng_bwd(_dev(table), _dev(idx, torch.int64), _dev(order, torch.int64), _rng_ptr(state), int(site),
                                        float(p), _dev(d_out), idx.shape[0], table.shape[1], _dev(d_table), _dev(ws), _stream()),
           "cvc_embed_relu_rng_bwd")
    return d_table


def dropout_rng(x, state, site: int, p: float):
    """x * in-kernel keep-mask of (site, flat element index) (cvc_dropout_rng); its own backward on the gradient"""
    y = torch.empty_like(x)
    _check(lib().cvc_dropout_rng(_dev(x), x.numel(), _rng_ptr(state), int(site), float(p), _dev(y), _stream()), "cvc_dropout_rng")
    return y


def embed_relu_bwd(table, idx, drop, d_out, d_table=None):
    if d_table is None:
        d_table = torch.zeros_like(table)
    order = _embed_order(idx)                                    # rows grouped by word, original order inside a group
    ws = torch.empty(idx.shape[0], table.shape[1], device=table.device, dtype=torch.float32)
    _check(lib().cvc_embed_relu_bwd(_dev(table), _dev(idx, torch.int64), _dev(order, torch.int64), _dev(drop), _dev(d_out),
                                    idx.shape[0], table.shape[1], _dev(d_table), _dev(ws), _stream()), "cvc_embed_relu_bwd")
    return d_table


def log_softmax_fwd(logits, out=None):
    M, V = logits.shape
    out = out if out is not None else torch.empty_like(logits)
    _check(lib().cvc_log_softmax_fwd(_dev(logits), M, V, _dev(out), _stream()), "cvc_log_softmax_fwd")
    return out


def log_softmax_bwd(logp, d_logp):
    M, V = logp.shape
    d = torch.empty_like(logp)
    _check(lib().cvc_log_softmax_bwd(_dev(logp), _dev(d_logp), M, V, _dev(d), _stream()), "cvc_log_softmax_bwd")
    return d


def nll_bwd(target, w, g, V: int):
    M = target.shape[0]
    d = torch.empty(M, V, device=w.device, dtype=torch.float32)
    _check(lib().cvc_nll_bwd(_dev(target, torch.int64), _dev(w), _dev(g), M, V, _dev(d), _stream()), "cvc_nll_bwd")
    return d


def top2_unk(logits, unk_idx: int, word_out: torch.Tensor, word_stride: int = 1, logprob: Optional[torch.Tensor] = None):
    """word_out: int64 tensor whose element m*word_stride (from its data_ptr) receives row m's word."""
    M, V = logits.shape
    assert word_out.dtype == torch.int64 and word_out.is_cuda
    _check(lib().cvc_top2_unk(_dev(logits), M, V, int(unk_idx), word_out.data_ptr(), int(word_stride), _dev(logprob),
                              _stream()), "cvc_top2_unk")


def nll_fwd(logp, target, w):
    M, V = logp.shape
    loss = torch.zeros(1, device=logp.device, dtype=torch.float32)
    _check(lib().cvc_nll_fwd(_dev(logp), _dev(target, torch.int64), _dev(w), M, V, _dev(loss), _stream()), "cvc_nll_fwd")
    return loss


def vocab_nll_fwd(logits, target, w, want_argmax=True):
    """-> loss_sum [1], lse [M], argmax [M] int64 (or None)"""
    M, V = logits.shape
    dev = logits.device
    lse = torch.empty(M, device=dev, dtype=torch.float32)
    row_loss = torch.empty(M, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64) if want_argmax else None
    _check(lib().cvc_vocab_nll_fwd(_dev(logits), _dev(target, torch.int64), _dev(w), M, V, _dev(lse), _dev(amax, torch.int64),
                                   _dev(row_loss), _dev(loss), _stream()), "cvc_vocab_nll_fwd")
    return loss, lse, amax


def vocab_head_nll_fwd(parts, bias, target, w):
    """parts [ks, M, V]: the vocabulary head's K-slice slabs.  -> loss_sum [1], argmax [M], pre [M, V] (aliasing slab 0)"""
    ks, M, V = parts.shape
    dev = parts.device
    row_loss = torch.empty(M, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64)
    pre = parts[0]
    _check(lib().cvc_vocab_head_nll_fwd(_dev(parts), ks, M * V, V, _dev(bias), _dev(target, torch.int64), _dev(w), M, V, pre.data_ptr(), V,
                                        _dev(amax, torch.int64), _dev(row_loss), _dev(loss), _stream()), "cvc_vocab_head_nll_fwd")
    return loss, amax, pre


def check_label_smoothing(eps, what="label_smoothing") -> float:
    """eps as a float in [0, 1) -- the share of the target distribution spread uniformly over the vocabulary -- or ValueError (before
    any tensor is touched or kernel launched)"""
    try:
        e = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number in [0, 1), got {eps!r}") from None
    if not (0.0 <= e < 1.0):                 # (a NaN fails the comparison)
        raise ValueError(f"{what} must be in [0, 1), got {eps!r}")
    return e


def vocab_nll_ls_fwd(logits, target, w, eps: float, want_argmax=True):
    """vocab_nll_fwd with label smoothing eps -> loss_sum [1] (smoothed), lse [M], argmax [M] int64 (or None), nll_sum [1] (unsmoothed)"""
    eps = check_label_smoothing(eps)
    M, V = logits.shape
    dev = logits.device
    lse = torch.empty(M, device=dev, dtype=torch.float32)
    rows = torch.empty(2, M, device=dev, dtype=torch.float32)
    loss, nll = torch.empty(1, device=dev, dtype=torch.float32), torch.empty(1, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64) if want_argmax else None
    _check(lib().cvc_vocab_nll_ls_fwd(_dev(logits), _dev(target, torch.int64), _dev(w), M, V, eps, _dev(lse), _dev(amax, torch.int64),
                                      _dev(rows), _dev(loss), rows[1].data_ptr(), _dev(nll), _stream()), "cvc_vocab_nll_ls_fwd")
    return loss, lse, amax, nll


def vocab_head_nll_ls_fwd(parts, bias, target, w, eps: float):
    """vocab_head_nll_fwd with label smoothing eps -> loss_sum [1] (smoothed), argmax [M], pre [M, V] (aliasing slab 0; the
    smoothed loss's gradient), nll_sum [1] (unsmoothed)"""
    eps = check_label_smoothing(eps)
    ks, M, V = parts.shape
    dev = parts.device
    rows = torch.empty(2, M, device=dev, dtype=torch.float32)
    loss, nll = torch.empty(1, device=dev, dtype=torch.float32), torch.empty(1, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64)
    pre = parts[0]
    _check(lib().cvc_vocab_head_nll_ls_fwd(_dev(parts), ks, M * V, V, _dev(bias), _dev(target, torch.int64), _dev(w), M, V, eps,
                                           pre.data_ptr(), V, _dev(amax, torch.int64), _dev(rows), _dev(loss), rows[1].data_ptr(),
                                           _dev(nll), _stream()), "cvc_vocab_head_nll_ls_fwd")
    return loss, amax, pre, nll


def vocab_nll_ls_bwd(logits, lse, target, w, g, eps: float):
    eps = check_label_smoothing(eps)
    M, V = logits.shape
    d = torch.empty_like(logits)
    _check(lib().cvc_vocab_nll_ls_bwd(_dev(logits), _dev(lse), _dev(target, torch.int64), _dev(w), _dev(g), M, V, eps, _dev(d),
                                      _stream()), "cvc_vocab_nll_ls_bwd")
    return d


def check_entropy_beta(beta, what="entropy_beta") -> float:
    """beta as a finite float -- the coefficient of the entropy term -beta m H in the criterion (beta > 0 rewards entropy; 0 only
    reports it) -- or ValueError (before any tensor is touched or kernel launched)"""
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a finite number, got {beta!r}") from None
    if not math.isfinite(b):
        raise ValueError(f"{what} must be finite, got {beta!r}")
    return b


def _check_rows(what, M, **rows):
    for name, t in rows.items():
        if t.numel() != M:
            raise ValueError(f"{what}: {name} has {t.numel()} elements for {M} rows")


def vocab_nll_ent_fwd(logits, target, w, m, eps: float, beta: float, want_argmax=True):
    """vocab_nll_ls_fwd with the entropy term -beta m H -> loss_sum [1], lse [M], argmax [M] int64 (or None), nll_sum [1]
    (unsmoothed, without the entropy term), ent_sum [1] (sum_r m H), row_ent [M] (the backward's input)"""
    eps, beta = check_label_smoothing(eps), check_entropy_beta(beta)
    M, V = logits.shape
    _check_rows("vocab_nll_ent_fwd", M, target=target, w=w, m=m)
    dev = logits.device
    lse = torch.empty(M, device=dev, dtype=torch.float32)
    rows = torch.empty(6, M, device=dev, dtype=torch.float32)          # (loss, NLL, entropy; then the rows' fp32 remainders)
    sums = torch.empty(3, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64) if want_argmax else None
    _check(lib().cvc_vocab_nll_ent_fwd(_dev(logits), _dev(target, torch.int64), _dev(w), _dev(m), M, V, eps, beta, _dev(lse),
                                       _dev(amax, torch.int64), _dev(rows), _dev(sums), rows[1].data_ptr(), sums[1:].data_ptr(),
                                       rows[2].data_ptr(), sums[2:].data_ptr(), rows[3].data_ptr(), _stream()), "cvc_vocab_nll_ent_fwd")
    return sums[0:1], lse, amax, sums[1:2], sums[2:3], rows[2]


def vocab_head_nll_ent_fwd(parts, bias, target, w, m, eps: float, beta: float):
    """vocab_head_nll_ls_fwd with the entropy term -beta m H -> loss_sum [1], argmax [M], pre [M, V] (aliasing slab 0; the whole
    loss's gradient), nll_sum [1] (unsmoothed, without the entropy term), ent_sum [1] (sum_r m H)"""
    eps, beta = check_label_smoothing(eps), check_entropy_beta(beta)
    ks, M, V = parts.shape
    _check_rows("vocab_head_nll_ent_fwd", M, target=target, w=w, m=m)
    dev = parts.device
    rows = torch.empty(6, M, device=dev, dtype=torch.float32)          # (loss, NLL, entropy; then the rows' fp32 remainders)
    sums = torch.empty(3, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64)
    pre = parts[0]
    _check(lib().cvc_vocab_head_nll_ent_fwd(_dev(parts), ks, M * V, V, _dev(bias), _dev(target, torch.int64), _dev(w), _dev(m), M, V, eps,
                                            beta, pre.data_ptr(), V, _dev(amax, torch.int64), _dev(rows), _dev(sums), rows[1].data_ptr(),
                                            sums[1:].data_ptr(), rows[2].data_ptr(), sums[2:].data_ptr(), rows[3].data_ptr(), _stream()),
           "cvc_vocab_head_nll_ent_fwd")
    return sums[0:1], amax, pre, sums[1:2], sums[2:3]


def vocab_nll_ent_bwd(logits, lse, target, w, m, row_ent, g, eps: float, beta: float):
    eps, beta = check_label_smoothing(eps), check_entropy_beta(beta)
    M, V = logits.shape
    _check_rows("vocab_nll_ent_bwd", M, lse=lse, target=target, w=w, m=m, row_ent=row_ent)
    d = torch.empty_like(logits)
    _check(lib().cvc_vocab_nll_ent_bwd(_dev(logits), _dev(lse), _dev(target, torch.int64), _dev(w), _dev(m), _dev(row_ent), _dev(g), M, V,
                                       eps, beta, _dev(d), _stream()), "cvc_vocab_nll_ent_bwd")
    return d


def check_distill_scalars(alpha, tau, what="distill"):
    """(alpha, tau) as floats -- the soft loss's share in [0, 1] and the temperature, finite and > 0 -- or ValueError (before any tensor
    is touched or kernel launched)"""
    try:
        a, t = float(alpha), float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: alpha and tau must be numbers, got {alpha!r}, {tau!r}") from None
    if not (0.0 <= a <= 1.0):                # (a NaN fails the comparison)
        raise ValueError(f"{what}: alpha must be in [0, 1], got {alpha!r}")
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"{what}: tau (the temperature) must be finite and > 0, got {tau!r}")
    return a, t


def check_distill(distill, rows: int, V: int, what="distill"):
    """distill = (teacher_rows, alpha, tau[, row_map]) -> (teacher [R, V] fp32 contiguous, alpha, tau, row_map int32 [rows]
    or None), or ValueError.  teacher_rows: [R, V] or [T, R', V] (flattened, rows t * R' + r) log-scale scores; without a row map row m
    of the criterion takes teacher row m, so R >= rows"""
    if not isinstance(distill, (tuple, list)) or len(distill) not in (3, 4):
        raise ValueError(f"{what}: expected (teacher_rows, alpha, tau[, row_map]), got {type(distill).__name__}")
    alpha, tau = check_distill_scalars(distill[1], distill[2], what)
    t = distill[0]
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (2, 3) or t.shape[-1] != V:
        raise ValueError(f"{what}: teacher_rows must be an fp32 [rows, {V}] or [T, rows, {V}] tensor, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dim() == 3:
        t = t.reshape(-1, V)
    if not t.is_contiguous():
        t = t.contiguous()
    row_map = distill[3] if len(distill) == 4 else None
    if row_map is not None:
        if row_map.dtype != torch.int32 or row_map.numel() != rows:
            raise ValueError(f"{what}: row_map must be int32 with {rows} elements")
        row_map = row_map.contiguous()
    elif t.shape[0] < rows:
        raise ValueError(f"{what}: {t.shape[0]} teacher rows for {rows} rows of the criterion")
    return t, alpha, tau, row_map


def vocab_head_nll_kd_fwd(parts, bias, target, w, teacher, alpha: float, tau: float, row_map=None):
    """vocab_head_nll_ls_fwd against a dense teacher row (cvc_vocab_head_nll_kd_fwd): -> loss_sum [1] (mixed), argmax [M], pre [M, V]
    (aliasing slab 0; the mixed loss's gradient), nll_sum [1] (unmixed), kd_sum [1] (unmixed)"""
    alpha, tau = check_distill_scalars(alpha, tau)
    ks, M, V = parts.shape
    _check_rows("vocab_head_nll_kd_fwd", M, target=target, w=w)
    dev = parts.device
    rows = torch.empty(3, M, device=dev, dtype=torch.float32)
    sums = torch.empty(3, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64)
    pre = parts[0]
    _check(lib().cvc_vocab_head_nll_kd_fwd(_dev(parts), ks, M * V, V, _dev(bias), _dev(target, torch.int64), _dev(w), _dev(teacher),
                                           V, _dev(row_map, torch.int32), teacher.shape[0], M, V, alpha, tau, pre.data_ptr(), V,
                                           _dev(amax, torch.int64), _dev(rows), _dev(sums), rows[1].data_ptr(), sums[1:].data_ptr(),
                                           rows[2].data_ptr(), sums[2:].data_ptr(), _stream()), "cvc_vocab_head_nll_kd_fwd")
    return sums[0:1], amax, pre, sums[1:2], sums[2:3]


def vocab_nll_kd_fwd(logits, target, w, teacher, alpha: float, tau: float, row_map=None, want_argmax=True):
    """the two-step form on materialised logits -> loss_sum [1], stats [5, M] (the backward's input), argmax [M] int64 (or None),
    nll_sum [1], kd_sum [1]"""
    alpha, tau = check_distill_scalars(alpha, tau)
    M, V = logits.shape
    _check_rows("vocab_nll_kd_fwd", M, target=target, w=w)
    dev = logits.device
    stats = torch.empty(5, M, device=dev, dtype=torch.float32)
    rows = torch.empty(3, M, device=dev, dtype=torch.float32)
    sums = torch.empty(3, device=dev, dtype=torch.float32)
    amax = torch.empty(M, device=dev, dtype=torch.int64) if want_argmax else None
    _check(lib().cvc_vocab_nll_kd_fwd(_dev(logits), _dev(target, torch.int64), _dev(w), _dev(teacher), V,
                                      _dev(row_map, torch.int32), teacher.shape[0], M, V, alpha, tau, _dev(stats), _dev(amax, torch.int64),
                                      _dev(rows), _dev(sums), rows[1].data_ptr(), sums[1:].data_ptr(), rows[2].data_ptr(),
                                      sums[2:].data_ptr(), _stream()), "cvc_vocab_nll_kd_fwd")
    return sums[0:1], stats, amax, sums[1:2], sums[2:3]


def vocab_nll_kd_bwd(logits, stats, target, w, teacher, g, alpha: float, tau: float, row_map=None):
    alpha, tau = check_distill_scalars(alpha, tau)
    M, V = logits.shape
    _check_rows("vocab_nll_kd_bwd", M, target=target, w=w)
    d = torch.empty_like(logits)
    _check(lib().cvc_vocab_nll_kd_bwd(_dev(logits), _dev(stats), _dev(target, torch.int64), _dev(w), _dev(teacher), V,
                                      _dev(row_map, torch.int32), teacher.shape[0], _dev(g), M, V, alpha, tau, _dev(d), _stream()),
           "cvc_vocab_nll_kd_bwd")
    return d


def scale_by_scalar(x, g):
    """g[0] * x with g a device scalar tensor (no host read)"""
    y = torch.empty_like(x)
    _check(lib().cvc_scale_by_scalar(_dev(x), _dev(g), x.numel(), _dev(y), _stream()), "cvc_scale_by_scalar")
    return y


def vocab_nll_bwd(logits, lse, target, w, g):
    M, V = logits.shape
    d = torch.empty_like(logits)
    _check(lib().cvc_vocab_nll_bwd(_dev(logits), _dev(lse), _dev(target, torch.int64), _dev(w), _dev(g), M, V, _dev(d),
                                   _stream()), "cvc_vocab_nll_bwd")
    return d


def grounder_fwd(xt, feats, bias, mask):
    B, T, G = xt.shape
    N = feats.shape[1]
    out = torch.empty(B, T, N, device=xt.device, dtype=torch.float32)
    m = _mask(mask)
    _check(lib().cvc_grounder_fwd(_dev(xt), _dev(feats), _dev(bias), _dev(m, torch.uint8), B, T, N, G, _dev(out), _stream()),
           "cvc_grounder_fwd")
    return out


def grounder_bwd(d, xt, feats, want_xt: bool, want_feats: bool):
    B, T, G = xt.shape
    N = feats.shape[1]
    d_xt = torch.empty_like(xt) if want_xt else None
    d_feats = torch.empty_like(feats) if want_feats else None
    _check(lib().cvc_grounder_bwd(_dev(d), _dev(xt), _dev(feats), B, T, N, G, _dev(d_xt), _dev(d_feats), _stream()), "cvc_grounder_bwd")
    return d_xt, d_feats


def beam_select(logits, score_in, done_in, B: int, beam: int, unk_idx: int, first_step: bool):
    V = logits.shape[1]
    dev = logits.device
    parent = torch.empty(B * beam, dtype=torch.int64, device=dev)
    word = torch.empty(B * beam, dtype=torch.int64, device=dev)
    score = torch.empty(B * beam, dtype=torch.float32, device=dev)
    done = torch.empty(B * beam, dtype=torch.uint8, device=dev)
    ws = torch.empty(17 * B * beam, dtype=torch.float32, device=dev)
    _check(lib().cvc_beam_select(_dev(logits), _dev(score_in), _dev(done_in, torch.uint8), B, beam, V, int(unk_idx),
                                 1 if first_step else 0, parent.data_ptr(), word.data_ptr(), _dev(score),
                                 _dev(done, torch.uint8), _dev(ws), _stream()), "cvc_beam_select")
    return parent, word, score, done


def beam_select_parts(parts, bias, score_in, done_in, B: int, beam: int, unk_idx: int, first_step: bool):
    """beam_select over logits that still are the K-slice slabs [nparts, rows, V] of the vocabulary GEMM (+ bias [V]): summed while
    the rows are scanned, in the finishing pass's order (cvc_beam_select_parts)"""
    nparts, rows, V = parts.shape
    dev = parts.device
    parent = torch.empty(B * beam, dtype=torch.int64, device=dev)
    word = torch.empty(B * beam, dtype=torch.int64, device=dev)
    score = torch.empty(B * beam, dtype=torch.float32, device=dev)
    done = torch.empty(B * beam, dtype=torch.uint8, device=dev)
    ws = torch.empty(17 * B * beam, dtype=torch.float32, device=dev)
    _check(lib().cvc_beam_select_parts(_dev(parts), nparts, rows * V, _dev(bias), _dev(score_in), _dev(done_in, torch.uint8), B, beam, V,
                                       int(unk_idx), 1 if first_step else 0, parent.data_ptr(), word.data_ptr(), _dev(score),
                                       _dev(done, torch.uint8), _dev(ws), _stream()), "cvc_beam_select_parts")
    return parent, word, score, done


def gather_rows(src, parent, beam: int):
    rows, width = src.shape
    dst = torch.empty_like(src)
    _check(lib().cvc_gather_rows(_dev(src), _dev(parent, torch.int64), rows, beam, width, _dev(dst), _stream()),
           "cvc_gather_rows")
    return dst


# --------------------------------------------------------------------------- label glue / supervised attention criteria
def bbox_overlaps(rois: torch.Tensor, gt: torch.Tensor, frm_mask: torch.Tensor, pnt_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """IoU [B, N, K] of proposals [B, N, >= 4] vs ground-truth boxes [B, K, >= 4] (cvc_bbox_overlaps_fwd); frm_mask [B, N, K] and
    pnt_mask [B, N] (nullable) zero the overlap where set."""
    B, N, K = frm_mask.shape
    rois, gt = rois.contiguous(), gt.contiguous()
    fm = _mask(frm_mask)
    pm = None
    if pnt_mask is not None:       # [B, N], any row stride (the trainer's pnt_mask[:, 1:]): a byte view, no copy
        pm = pnt_mask.view(torch.uint8) if pnt_mask.dtype == torch.bool else (pnt_mask if pnt_mask.dtype == torch.uint8 else (pnt_mask != 0).view(torch.uint8))
        if pm.stride(1) != 1:
            pm = pm.contiguous()
    ov = torch.empty(B, N, K, device=rois.device, dtype=torch.float32)
    _check(lib().cvc_bbox_overlaps_fwd(_dev(rois), rois.shape[2], _dev(gt), gt.shape[2], _dev(fm, torch.uint8),
                                       None if pm is None else pm.data_ptr(), 0 if pm is None else pm.stride(0), B, N, K, _dev(ov),
                                       _stream()), "cvc_bbox_overlaps_fwd")
    return ov


def label_glue(ov: torch.Tensor, box_mask_kt: torch.Tensor, frm_mask: torch.Tensor, pnt_mask: torch.Tensor, want_steps: bool = True):
    """ov [B, N, K]; box_mask_kt: bool view [B, K, T] (any strides) of mask_boxes[:, 0, :, 1:T+1]; frm_mask [B, N, K]; pnt_mask
    [B, N + 1].  -> roi_labels [B, T, N] bool, frm_mask_output [B, T, N + 1] bool, step_fmask [T, B, N] bool (or None)."""
    B, N, K = ov.shape
    T = box_mask_kt.shape[2]
    bm = box_mask_kt if box_mask_kt.dtype == torch.uint8 else box_mask_kt.view(torch.uint8) if box_mask_kt.dtype == torch.bool else (box_mask_kt != 0).view(torch.uint8)
    fm, pm = _mask(frm_mask), _mask(pnt_mask)
    labels = torch.empty(B, T, N, device=ov.device, dtype=torch.uint8)
    fmo = torch.empty(B, T, N + 1, device=ov.device, dtype=torch.uint8)
    steps = torch.empty(T, B, N, device=ov.device, dtype=torch.uint8) if want_steps else None
    _check(lib().cvc_label_glue_fwd(_dev(ov), bm.data_ptr(), bm.stride(0), bm.stride(1), bm.stride(2), _dev(fm, torch.uint8),
                                    _dev(pm, torch.uint8), B, N, K, T, _dev(labels, torch.uint8), _dev(fmo, torch.uint8),
                                    _dev(steps, torch.uint8), _stream()), "cvc_label_glue_fwd")
    return labels.view(torch.bool), fmo.view(torch.bool), (None if steps is None else steps.view(torch.bool))


def attn_nll_fwd(x0: torch.Tensor, x1: Optional[torch.Tensor], target: torch.Tensor):
    """-> loss [2] (or [1]), workspace (kept for the backward)"""
    B, T, N = x0.shape
    for x in (x0, x1):
        if x is not None and not (x.is_cuda and x.dtype == torch.float32 and x.stride(2) == 1):
            raise RuntimeError("cvc.hip.attn_nll: fp32 GPU tensors with unit inner stride (no CPU fallback)")
    tg = _mask(target)
    ws = torch.empty(5 * B * T + 1, device=x0.device, dtype=torch.float32)
    loss = torch.empty(2 if x1 is not None else 1, device=x0.device, dtype=torch.float32)
    _check(lib().cvc_attn_nll_fwd(x0.data_ptr(), x0.stride(0), x0.stride(1), None if x1 is None else x1.data_ptr(),
                                  0 if x1 is None else x1.stride(0), 0 if x1 is None else x1.stride(1), _dev(tg, torch.uint8), B, T, N,
                                  _dev(ws), _dev(loss), _stream()), "cvc_attn_nll_fwd")
    return loss, ws, tg


def attn_nll_bwd(x0, x1, tg, ws, g0, g1, want0: bool, want1: bool):
    B, T, N = x0.shape
    d0 = torch.empty(B, T, N, device=x0.device, dtype=torch.float32) if want0 else None
    d1 = torch.empty(B, T, N, device=x0.device, dtype=torch.float32) if (want1 and x1 is not None) else None
    _check(lib().cvc_attn_nll_bwd(x0.data_ptr(), x0.stride(0), x0.stride(1), None if x1 is None else x1.data_ptr(),
                                  0 if x1 is None else x1.stride(0), 0 if x1 is None else x1.stride(1), _dev(tg, torch.uint8), B, T, N,
                                  _dev(ws), _dev(g0), _dev(g1), _dev(d0), _dev(d1), _stream()), "cvc_attn_nll_bwd")
    return d0, d1


# --------------------------------------------------------------------------- self-critical training (csrc/cider.hip)
def cider_d(cand: torch.Tensor, refs: torch.Tensor, nref: torch.Tensor, keys: torch.Tensor, idf: torch.Tensor, idf_unseen: float,
            sigma: float = 6.0, want_orders: bool = False):
    """cand [rows, T] int64; refs [clips, Rmax, T] int64 (rows % clips == 0: rows / clips samples per clip); nref [clips] int32; keys [G]
    int64 holding the table's unsigned 64-bit keys, idf [G].  -> reward [rows] (, per_order [rows, 4])."""
    if cand.dim() != 2 or refs.dim() != 3 or refs.shape[2] != cand.shape[1] or refs.shape[0] < 1 or cand.shape[0] % refs.shape[0] != 0 \
            or nref.numel() != refs.shape[0] or idf.numel() != keys.numel():
        raise RuntimeError(f"cvc.hip.cider_d: cand {tuple(cand.shape)}, refs {tuple(refs.shape)}, nref {tuple(nref.shape)}, keys "
                           f"{tuple(keys.shape)}, idf {tuple(idf.shape)} do not fit")
    rows, T = cand.shape
    clips, Rmax = refs.shape[0], refs.shape[1]
    G = int(keys.numel())
    reward = torch.empty(rows, device=cand.device, dtype=torch.float32)
    orders = torch.empty(rows, 4, device=cand.device, dtype=torch.float32) if want_orders else None
    _check(lib().cvc_cider_d(_dev(cand, torch.int64, "cand"), _dev(refs, torch.int64, "refs"), _dev(nref, torch.int32, "nref"), rows, T,
                             rows // clips, Rmax, _dev(keys, torch.int64, "keys") if G else None, _dev(idf, name="idf") if G else None, G,
                             float(idf_unseen), float(sigma), _dev(reward), _dev(orders), _stream()), "cvc_cider_d")
    return (reward, orders) if want_orders else reward


def scst_weights(reward: torch.Tensor, base: Optional[torch.Tensor], per_clip: int, cand: torch.Tensor, t_major: bool = False):
    """reward [rows], base [rows / per_clip] (per_clip == 1) or None, cand [rows, T] int64 -> adv [rows], w [rows, T] (t_major: [T, rows])"""
    rows, T = cand.shape
    if reward.numel() != rows or rows % int(per_clip) != 0 or (base is not None and base.numel() != rows // int(per_clip)):
        raise RuntimeError(f"cvc.hip.scst_weights: reward {tuple(reward.shape)}, base {None if base is None else tuple(base.shape)}, "
                           f"per_clip {per_clip}, cand {tuple(cand.shape)} do not fit")
    adv = torch.empty(rows, device=cand.device, dtype=torch.float32)
    w = torch.empty((T, rows) if t_major else (rows, T), device=cand.device, dtype=torch.float32)
    _check(lib().cvc_scst_weights(_dev(reward, name="reward"), _dev(base, name="base"), rows, int(per_clip), _dev(cand, torch.int64, "cand"),
                                  T, 1 if t_major else 0, _dev(adv), _dev(w), _stream()), "cvc_scst_weights")
    return adv, w


def scst_weights_wor(reward: torch.Tensor, logq: torch.Tensor, G: torch.Tensor, state: torch.Tensor, per_clip: int, cand: torch.Tensor,
                     t_major: bool = False, normalize: bool = True):
    """Self-critical weights of captions sampled without replacement (csrc/scst_wor.hip; the rule: include/cvc_hip_blocks.h).
    reward [rows] of the S = per_clip rollouts per clip; logq, G [rows / S, S + 1] the stochastic beam's sampling log-probs and
    perturbed keys (beam = S + 1: slot S is the threshold); state: the engine's generator words, int32 [4] (DecodeEngine.rng_state);
    cand [rows, T] int64 -> adv [rows], wgt [rows], est [rows / S], w [rows, T] (t_major: [T, rows])"""
    S = int(per_clip)
    if cand.dim() != 2 or S < 1 or reward.numel() != cand.shape[0] or cand.shape[0] % S != 0 or state.numel() != 4 \
            or logq.numel() != (cand.shape[0] // S) * (S + 1) or G.numel() != logq.numel():
        raise RuntimeError(f"cvc.hip.scst_weights_wor: reward {tuple(reward.shape)}, logq {tuple(logq.shape)}, G {tuple(G.shape)}, state "
                           f"{tuple(state.shape)}, per_clip {per_clip}, cand {tuple(cand.shape)} do not fit")
    rows, T = cand.shape
    dev = cand.device
    adv = torch.empty(rows, device=dev, dtype=torch.float32)
    wgt = torch.empty(rows, device=dev, dtype=torch.float32)
    est = torch.empty(rows // S, device=dev, dtype=torch.float32)
    w = torch.empty((T, rows) if t_major else (rows, T), device=dev, dtype=torch.float32)
    _check(lib().cvc_scst_weights_wor(_dev(reward, name="reward"), _dev(logq, name="logq"), _dev(G, name="G"),
                                      _dev(state, torch.int32, "state"), rows, S, _dev(cand, torch.int64, "cand"), T, 1 if t_major else 0,
                                      1 if normalize else 0, _dev(adv), _dev(wgt), _dev(est), _dev(w), _stream()), "cvc_scst_weights_wor")
    return adv, wgt, est, w


# --------------------------------------------------------------------------- token-overlap caption metrics (csrc/overlap.hip)
def caption_overlap(cand: torch.Tensor, refs: torch.Tensor, nref: torch.Tensor, per_clip: Optional[int] = None, want_lcs: bool = False):
    """cand [rows, T] int64; refs [clips, Rmax, T] int64 (per_clip = rows / clips consecutive candidates per clip); nref [clips] int32.
    -> stats [rows, 10] int32 (correct_1..4, guess_1..4, cand_len, ref_len), lcs [rows, Rmax] int32 or None, bleu [rows, 4], rouge [rows]"""
    if cand.dim() != 2 or refs.dim() != 3 or refs.shape[2] != cand.shape[1] or refs.shape[0] < 1 or nref.numel() != refs.shape[0]:
        raise RuntimeError(f"cvc.hip.caption_overlap: cand {tuple(cand.shape)}, refs {tuple(refs.shape)}, nref {tuple(nref.shape)} do not fit")
    rows, T = cand.shape
    clips, Rmax = refs.shape[0], refs.shape[1]
    per_clip = rows // clips if per_clip is None else int(per_clip)
    if per_clip < 1 or per_clip * clips != rows:
        raise RuntimeError(f"cvc.hip.caption_overlap: {rows} candidate rows are not {per_clip} per clip of {clips} clips")
    dev = cand.device
    stats = torch.empty(rows, 10, device=dev, dtype=torch.int32)
    lcs = torch.empty(rows, Rmax, device=dev, dtype=torch.int32) if want_lcs else None
    bleu = torch.empty(rows, 4, device=dev, dtype=torch.float32)
    rouge = torch.empty(rows, device=dev, dtype=torch.float32)
    _check(lib().cvc_caption_overlap(_dev(cand, torch.int64, "cand"), _dev(refs, torch.int64, "refs"), _dev(nref, torch.int32, "nref"),
                                     rows, T, per_clip, Rmax, _dev(stats, torch.int32), _dev(lcs, torch.int32), _dev(bleu), _dev(rouge),
                                     _stream()), "cvc_caption_overlap")
    return stats, lcs, bleu, rouge


# --------------------------------------------------------------------------- consensus caption selection (csrc/consensus.hip)
def consensus_cider(cand: torch.Tensor, per_clip: int, keys: torch.Tensor, idf: torch.Tensor, idf_unseen: float, sigma: float = 6.0,
                    live: Optional[torch.Tensor] = None):
    """cand [rows, T] int64, per_clip consecutive candidates per clip; keys [G] int64 holding the table's unsigned 64-bit keys, idf [G];
    live [rows] int32 or None (every row is live).  -> utility [rows] fp32 (CIDEr-D of the row against the clip's other live rows),
    pick [clips] int32 (the first live row with the largest utility), best [clips, T] int64 (that row)."""
    per_clip = int(per_clip)
    if cand.dim() != 2 or per_clip < 1 or cand.shape[0] < 1 or cand.shape[0] % per_clip != 0 or idf.numel() != keys.numel() \
            or (live is not None and live.numel() != cand.shape[0]):
        raise RuntimeError(f"cvc.hip.consensus_cider: cand {tuple(cand.shape)}, per_clip {per_clip}, live "
                           f"{None if live is None else tuple(live.shape)}, keys {tuple(keys.shape)}, idf {tuple(idf.shape)} do not fit")
    rows, T = cand.shape
    clips = rows // per_clip
    G = int(keys.numel())
    utility = torch.empty(rows, device=cand.device, dtype=torch.float32)
    pick = torch.empty(clips, device=cand.device, dtype=torch.int32)
    best = torch.empty(clips, T, device=cand.device, dtype=torch.int64)
    _check(lib().cvc_consensus_cider(_dev(cand, torch.int64, "cand"), _dev(live, torch.int32, "live"), rows, T, per_clip,
                                     _dev(keys, torch.int64, "keys") if G else None, _dev(idf, name="idf") if G else None, G,
                                     float(idf_unseen), float(sigma), _dev(utility), _dev(pick, torch.int32), _dev(best, torch.int64),
                                     _stream()), "cvc_consensus_cider")
    return utility, pick, best


# --------------------------------------------------------------------------- consensus under a utility mix (csrc/consensus_mix.hip)
CONSENSUS_METRICS = 6        # cider, bleu1..4, rougel: the order of cvc.metrics.REWARD_NAMES


def consensus_mix(cand: torch.Tensor, per_clip: int, coef, keys: Optional[torch.Tensor] = None, idf: Optional[torch.Tensor] = None,
                  idf_unseen: float = 0.0, sigma: float = 6.0, live: Optional[torch.Tensor] = None,
                  logw: Optional[torch.Tensor] = None, want_pairs: bool = False):
    """cand [rows, T] int64, per_clip consecutive candidates per clip; coef: six numbers >= 0 (cider, bleu1..4, rougel), not all 0;
    keys [G] int64 holding the table's unsigned 64-bit keys and idf [G] (needed with coef[0] > 0 only); live [rows] int32 or None (every
    row is live); logw [rows] fp32 log-weights or None (uniform).  -> utility [rows] fp32 (the weighted mean over the clip's other
    live rows j of sum_k coef[k] metric_k(row; j)), pick [clips] int32, best [clips, T] int64, pairs [clips, per_clip, per_clip, 6]
    fp32 (None unless want_pairs)."""
    per_clip = int(per_clip)
    coef = [float(c) for c in coef]
    if len(coef) != CONSENSUS_METRICS:
        raise RuntimeError(f"cvc.hip.consensus_mix: coef holds {len(coef)} numbers; it takes {CONSENSUS_METRICS} (cider, bleu1..4, rougel)")
    cider = coef[0] > 0.0
    if cider and (keys is None or idf is None):
        raise RuntimeError("cvc.hip.consensus_mix: a CIDEr coefficient needs the idf table (keys, idf)")
    if cand.dim() != 2 or per_clip < 1 or cand.shape[0] < 1 or cand.shape[0] % per_clip != 0 \
            or (live is not None and live.numel() != cand.shape[0]) or (logw is not None and logw.numel() != cand.shape[0]) \
            or (cider and idf.numel() != keys.numel()):
        raise RuntimeError(f"cvc.hip.consensus_mix: cand {tuple(cand.shape)}, per_clip {per_clip}, live "
                           f"{None if live is None else tuple(live.shape)}, logw {None if logw is None else tuple(logw.shape)}"
                           + (f", keys {tuple(keys.shape)}, idf {tuple(idf.shape)}" if cider else "") + " do not fit")
    rows, T = cand.shape
    clips = rows // per_clip
    G = int(keys.numel()) if cider else 0
    utility = torch.empty(rows, device=cand.device, dtype=torch.float32)
    pick = torch.empty(clips, device=cand.device, dtype=torch.int32)
    best = torch.empty(clips, T, device=cand.device, dtype=torch.int64)
    pairs = torch.empty(clips, per_clip, per_clip, CONSENSUS_METRICS, device=cand.device, dtype=torch.float32) if want_pairs else None
    c_coef = (C.c_float * CONSENSUS_METRICS)(*coef)          # read on the host before the launch
    _check(lib().cvc_consensus_mix(_dev(cand, torch.int64, "cand"), _dev(live, torch.int32, "live"), _dev(logw, name="logw"), rows, T,
                                   per_clip, _dev(keys, torch.int64, "keys") if G else None, _dev(idf, name="idf") if G else None, G,
                                   float(idf_unseen), float(sigma), C.addressof(c_coef), _dev(utility), _dev(pick, torch.int32),
                                   _dev(best, torch.int64), _dev(pairs), _stream()), "cvc_consensus_mix")
    return utility, pick, best, pairs


# --------------------------------------------------------------------------- caption-set diversity (csrc/diversity.hip)
def caption_set_stats(cand: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None):
    """cand [rows, T] int64, per_clip consecutive candidates per clip; live [rows] int32 or None (every row is live).
    -> set_stats [clips, 12] int32 (distinct_1..4, total_1..4, live, unique, scored, 0), mbleu_stats [rows, 10] int32 and mbleu
    [rows, 4] fp32 (the row against the clip's other live rows, caption_overlap's layout and bits)."""
    per_clip = int(per_clip)
    if cand.dim() != 2 or per_clip < 1 or cand.shape[0] < 1 or cand.shape[0] % per_clip != 0 \
            or (live is not None and live.numel() != cand.shape[0]):
        raise RuntimeError(f"cvc.hip.caption_set_stats: cand {tuple(cand.shape)}, per_clip {per_clip}, live "
                           f"{None if live is None else tuple(live.shape)} do not fit")
    rows, T = cand.shape
    set_stats = torch.empty(rows // per_clip, 12, device=cand.device, dtype=torch.int32)
    mbleu_stats = torch.empty(rows, 10, device=cand.device, dtype=torch.int32)
    mbleu = torch.empty(rows, 4, device=cand.device, dtype=torch.float32)
    _check(lib().cvc_caption_set_stats(_dev(cand, torch.int64, "cand"), _dev(live, torch.int32, "live"), rows, T, per_clip,
                                       _dev(set_stats, torch.int32), _dev(mbleu_stats, torch.int32), _dev(mbleu), _stream()),
           "cvc_caption_set_stats")
    return set_stats, mbleu_stats, mbleu


# --------------------------------------------------------------------------- spectral caption-set diversity (csrc/spectrum.hip)
SPECTRUM_MODES = {"cider": 0, "lsa": 1}
SPECTRUM_SLOTS = 32          # the padded side of gram and the length of lam, whatever per_clip is


def caption_set_spectrum(cand: torch.Tensor, per_clip: int, mode: str, keys: Optional[torch.Tensor] = None,
                         idf: Optional[torch.Tensor] = None, idf_unseen: float = 0.0, live: Optional[torch.Tensor] = None,
                         want_gram: bool = False):
    """cand [rows, T] int64, per_clip consecutive candidates per clip; mode "cider" (keys [G] int64 holding the table's unsigned 64-bit
    keys, idf [G], idf_unseen) or "lsa" (no table); live [rows] int32 or None (every row is live).
    -> gram [clips, 32, 32] fp32 (None unless want_gram), lam [clips, 32] fp64 (descending, zeros behind the m eigenvalues), score
    [clips, 2] fp32, info [clips, 2] int32 (m, sweeps or -1)."""
    per_clip = int(per_clip)
    if mode not in SPECTRUM_MODES:
        raise RuntimeError(f"cvc.hip.caption_set_spectrum: mode {mode!r}; it is one of {sorted(SPECTRUM_MODES)}")
    cider = mode == "cider"
    if cider and (keys is None or idf is None):
        raise RuntimeError("cvc.hip.caption_set_spectrum: mode 'cider' needs the idf table (keys, idf)")
    if cand.dim() != 2 or per_clip < 1 or cand.shape[0] < 1 or cand.shape[0] % per_clip != 0 \
            or (live is not None and live.numel() != cand.shape[0]) or (cider and idf.numel() != keys.numel()):
        raise RuntimeError(f"cvc.hip.caption_set_spectrum: cand {tuple(cand.shape)}, per_clip {per_clip}, live "
                           f"{None if live is None else tuple(live.shape)}"
                           + (f", keys {tuple(keys.shape)}, idf {tuple(idf.shape)}" if cider else "") + " do not fit")
    rows, T = cand.shape
    clips = rows // per_clip
    G = int(keys.numel()) if cider else 0
    gram = torch.empty(clips, SPECTRUM_SLOTS, SPECTRUM_SLOTS, device=cand.device, dtype=torch.float32) if want_gram else None
    lam = torch.empty(clips, SPECTRUM_SLOTS, device=cand.device, dtype=torch.float64)
    score = torch.empty(clips, 2, device=cand.device, dtype=torch.float32)
    info = torch.empty(clips, 2, device=cand.device, dtype=torch.int32)
    _check(lib().cvc_caption_set_spectrum(_dev(cand, torch.int64, "cand"), _dev(live, torch.int32, "live"), rows, T, per_clip,
                                          SPECTRUM_MODES[mode], _dev(keys, torch.int64, "keys") if G else None,
                                          _dev(idf, name="idf") if G else None, G, float(idf_unseen), _dev(gram),
                                          _dev(lam, torch.float64), _dev(score), _dev(info, torch.int32), _stream()),
           "cvc_caption_set_spectrum")
    return gram, lam, score, info


# --------------------------------------------------------------------------- grounding F1 of generated captions (csrc/grounding.hip)
def grounding_f1(seq: torch.Tensor, att: torch.Tensor, ppls: torch.Tensor, gt_bboxs: torch.Tensor, nbox: torch.Tensor,
                 word_cls: torch.Tensor, frames: int, table: torch.Tensor, per_clip: Optional[int] = None,
                 props_per_frame: Optional[int] = None):
    """seq [rows, T] int64; att [rows, T, P] fp32 over the clip's proposals (frame-major, P <= frames * props_per_frame: the trimmed
    axis; props_per_frame None: P / frames);
    ppls [clips, P, 7] fp32; gt_bboxs [clips, K, 6] fp32 (x1, y1, x2, y2, frame, class); nbox [clips] int32; word_cls [V] int32;
    table [C + 1, 6] int32, added to (per_clip = rows / clips consecutive rows per clip).
    -> pick [rows, T, frames] int32, counts [rows, 6] int32, f1 [rows] fp32"""
    frames = int(frames)
    if seq.dim() != 2 or att.dim() != 3 or ppls.dim() != 3 or gt_bboxs.dim() != 3 or word_cls.dim() != 1 or table.dim() != 2 \
            or att.shape[:2] != seq.shape or ppls.shape[0] < 1 or ppls.shape[1] != att.shape[2] or ppls.shape[2] != 7 \
            or gt_bboxs.shape[0] != ppls.shape[0] or gt_bboxs.shape[2] != 6 or nbox.numel() != ppls.shape[0] \
            or table.shape[0] < 2 or table.shape[1] != 6 or frames < 1:
        raise RuntimeError(f"cvc.hip.grounding_f1: seq {tuple(seq.shape)}, att {tuple(att.shape)}, ppls {tuple(ppls.shape)}, gt_bboxs "
                           f"{tuple(gt_bboxs.shape)}, nbox {tuple(nbox.shape)}, word_cls {tuple(word_cls.shape)}, table "
                           f"{tuple(table.shape)}, frames {frames} do not fit")
    rows, T = seq.shape
    clips, P, K = ppls.shape[0], ppls.shape[1], gt_bboxs.shape[1]
    per_clip = rows // clips if per_clip is None else int(per_clip)
    if per_clip < 1 or per_clip * clips != rows:
        raise RuntimeError(f"cvc.hip.grounding_f1: {rows} caption rows are not {per_clip} per clip of {clips} clips")
    if props_per_frame is None:   # an untrimmed axis: frames x Np slots exactly
        if P % frames != 0:
            raise RuntimeError(f"cvc.hip.grounding_f1: {P} proposal slots are not {frames} frames of equally many: a trimmed axis needs "
                               "props_per_frame")
        props_per_frame = P // frames
    Np = int(props_per_frame)
    if Np < 1 or P > frames * Np:
        raise RuntimeError(f"cvc.hip.grounding_f1: {P} proposal slots do not fit {frames} frames of {Np}")
    dev = seq.device
    pick = torch.empty(rows, T, frames, device=dev, dtype=torch.int32)
    counts = torch.empty(rows, 6, device=dev, dtype=torch.int32)
    f1 = torch.empty(rows, device=dev, dtype=torch.float32)
    _check(lib().cvc_grounding_f1(_dev(seq, torch.int64, "seq"), _dev(att, name="att"), _dev(ppls, name="ppls"),
                                  _dev(gt_bboxs, name="gt_bboxs"), _dev(nbox, torch.int32, "nbox"), _dev(word_cls, torch.int32, "word_cls"),
                                  rows, T, P, frames, Np, K, table.shape[0] - 1, int(word_cls.numel()), per_clip,
                                  _dev(pick, torch.int32), _dev(counts, torch.int32), _dev(f1), _dev(table, torch.int32, "table"),
                                  _stream()), "cvc_grounding_f1")
    return pick, counts, f1


# --------------------------------------------------------------------------- tile path (rows > 64), csrc/gemm_tile.hip
def tile_rows_alloc(M: int) -> int:
    return int(lib().cvc_tile_rows_alloc(int(M)))


def _frag_ptr(xb: torch.Tensor, k0: int = 0):
    """(address of k step k0/16 of row block 0, row-block stride in bf16 elements) of a fragment tensor
    [blocks][k steps][3][2][32][8] int16."""
    if not xb.is_cuda or xb.dtype != torch.int16 or not xb.is_contiguous() or xb.dim() != 6:
        raise RuntimeError("cvc.hip: activation / weight fragments must be a contiguous int16 GPU tensor [blk][kstep][3][2][32][8]")
    assert k0 % 16 == 0
    return xb.data_ptr() + (k0 // 16) * 3 * 1024, xb.shape[1] * 1536


def tile_gemm(wb: torch.Tensor, xb: torch.Tensor, k0: int, K: int, M: int, N: int, ksplit: int, parts: Optional[torch.Tensor] = None):
    """parts [ksplit, M, N] = per-K-slice partial products of x[:, k0:k0+K] @ W^T (wb packed for exactly these K columns)."""
    wp, _ = _frag_ptr(wb)
    assert wb.shape[1] == K // 16 and wb.shape[0] * 32 >= N and xb.shape[0] * 32 >= tile_rows_alloc(M)
    xp, xs = _frag_ptr(xb, k0)
    if parts is None:
        parts = torch.empty(ksplit, M, N, device=xb.device, dtype=torch.float32)
    _check(lib().cvc_tile_gemm(wp, xp, xs, K, M, N, ksplit, _dev(parts), N, M * N, _stream()), "cvc_tile_gemm")
    return parts


def tile_pack_rows(x: torch.Tensor, xb: torch.Tensor, k0: int = 0, idx: Optional[torch.Tensor] = None, relu: bool = False):
    M = x.shape[0] if idx is None else idx.shape[0]
    K = x.shape[1]
    xp, xs = _frag_ptr(xb, k0)
    _check(lib().cvc_tile_pack_rows(_dev(x), x.stride(0), _dev(idx, torch.int64), 1 if relu else 0, M, K, xp, xs, _stream()),
           "cvc_tile_pack_rows")
    return xb


class _FragPool:
    """Fragment buffers of TileOperand, reused across calls.  A buffer is keyed by everything that decides which of its bytes the
    packers never write (rows, K -> the zero padding of the last row blocks / k step), so the padding is cleared ONCE per buffer
    instead of by a fill launch per operand (27 per training step); buffers return to the pool when their operand dies.  All use is
    stream-ordered on the launch stream.  Buffers taken while a HIP graph is being captured stay with that capture."""

    def __init__(self):
        self.free = {}

    def take(self, rows: int, K: int, device):
        rows_alloc = max(tile_rows_alloc(rows), (rows + 127) // 128 * 128)
        key = (rows, K, str(device), torch.cuda.is_current_stream_capturing())
        lst = self.free.get(key)
        if lst:
            return lst.pop(), key
        frags = torch.empty(rows_alloc // 32, (K + 15) // 16, 3, 2, 32, 8, dtype=torch.int16, device=device)
        # padding must read as zero: only what the packer does not write completely is cleared -- the row blocks past the last
        # full one, and the last k step when K is not a multiple of 16 (the row packer writes whole quads, not whole k steps)
        if rows_alloc > rows:
            frags[rows // 32:].zero_()
        if K % 16 != 0:
            frags[:, -1].zero_()
        return frags, key

    def give(self, frags, key):
        lst = self.free.setdefault(key, [])
        if len(lst) < 8:
            lst.append(frags)


_FRAGS = _FragPool()


class TileOperand:
    """One operand of tile_mm, packed once into bf16 split-term fragments (reusable as either side of several products)."""

    def __init__(self, t: torch.Tensor, kmajor: bool = False):
        """t is [rows, K], or [K, rows] with kmajor (read as its transpose).  Unit inner stride; any sizes."""
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError("cvc.hip: tile_mm operands must be fp32 GPU tensors (no CPU fallback)")
        if t.dim() != 2:
            raise RuntimeError("cvc.hip: tile_mm operands are matrices")
        if t.stride(1) != 1:
            t = t.contiguous()
        self.rows, self.K = (t.shape[1], t.shape[0]) if kmajor else (t.shape[0], t.shape[1])
        self.frags, self._key = _FRAGS.take(self.rows, self.K, t.device)
        self.ptr, self.stride = _frag_ptr(self.frags)
        L = lib()
        if kmajor:
            _check(L.cvc_tile_pack_cols(t.data_ptr(), t.stride(0), self.K, self.rows, self.ptr, self.stride, _stream()), "cvc_tile_pack_cols")
        else:
            _check(L.cvc_tile_pack_rows_any(t.data_ptr(), t.stride(0), self.rows, self.K, self.ptr, self.stride, _stream()),
                   "cvc_tile_pack_rows_any")

    def __del__(self):
        try:
            _FRAGS.give(self.frags, self._key)
        except Exception:
            pass


@functools.lru_cache(maxsize=None)
def tile_gemm_plan(M: int, N: int, K: int):
    """(ksplit, rows per workgroup, workgroups) of the tile GEMM for an [M, K] x [N, K]^T product (cvc_tile_gemm_plan)"""
    ks, rows, wgs = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().cvc_tile_gemm_plan(int(M), int(N), int(K), C.addressof(ks), C.addressof(rows), C.addressof(wgs)), "cvc_tile_gemm_plan")
    return ks.value, rows.value, wgs.value


def tile_mm(a, b, a_kmajor: bool = False, b_kmajor: bool = False, out: Optional[torch.Tensor] = None, parts_only: bool = False,
            bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C[M, N] = sum_k A[m, k] B[n, k] on the tile GEMM (split products on the bf16 MFMA, fp32 accumulate, fp32-grade error):
    the dense products of the backward pass -- no library GEMM.  `a` is [M, K], or [K, M] with a_kmajor (read as its transpose);
    `b` is [N, K], or [K, N] with b_kmajor; either may be a TileOperand packed earlier (shared operands are packed once).
    out: [M, N] fp32 with unit inner stride and any row stride (a column block of a wider matrix: the weight-gradient products
    write their segment of weight_ih in place)."""
    A = a if isinstance(a, TileOperand) else TileOperand(a, a_kmajor)
    B = b if isinstance(b, TileOperand) else TileOperand(b, b_kmajor)
    assert A.K == B.K, (A.rows, A.K, B.rows, B.K)
    M, N, L, st = A.rows, B.rows, lib(), _stream()
    Kp = (A.K + 15) // 16 * 16
    ks = tile_gemm_plan(M, N, Kp)[0]               # chosen where the grid is chosen (csrc/gemm_tile.hip::cvc_tile_gemm_plan)
    if out is None:
        out = torch.empty(0 if parts_only else M, N, device=A.frags.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (M, N) and out.stride(1) == 1
              and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0):
        raise RuntimeError("cvc.hip.tile_mm: out must be an fp32 GPU [M, N] view with unit inner stride, 16-byte aligned rows")
    ldy = out.stride(0)
    if parts_only:          # the K-slice slabs themselves, for a consumer that sums them (cvc_vocab_head_nll_fwd)
        parts = torch.empty(ks, M, N, device=A.frags.device, dtype=torch.float32)
        _check(L.cvc_tile_gemm(B.ptr, A.ptr, A.stride, Kp, M, N, ks, parts.data_ptr(), N, M * N, st), "cvc_tile_gemm")
        return parts
    if ks == 1 and bias is None:
        _check(L.cvc_tile_gemm(B.ptr, A.ptr, A.stride, Kp, M, N, 1, out.data_ptr(), ldy, M * ldy, st), "cvc_tile_gemm")
        return out
    # bias [N]: added by the finishing pass (nn.Linear's epilogue), not by a framework add over the result
    parts = torch.empty(ks, M, N, device=out.device, dtype=torch.float32)
    _check(L.cvc_tile_gemm(B.ptr, A.ptr, A.stride, Kp, M, N, ks, parts.data_ptr(), N, M * N, st), "cvc_tile_gemm")
    _check(L.cvc_tile_linear_finish(parts.data_ptr(), ks, M * N, N, _dev(bias), None, M, N, out.data_ptr(), ldy, st), "cvc_tile_linear_finish")
    return out
