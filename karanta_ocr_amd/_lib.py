"""ctypes binding of libkaranta_hip.so (include/karanta_hip.h).

The product path has NO CPU fallback: if the shared library is missing or fails to load,
:func:`lib` raises :class:`KarantaHipError`.  `import torch` happens first on purpose — torch
ships its own libamdhip64.so.7 / librccl.so.1 and the extension must bind to the same runtime
instance so that torch's streams and device pointers are valid inside the library.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkaranta_hip.so")

c_p = C.c_void_p
i32, i64, f32 = C.c_int, C.c_int64, C.c_float


class KarantaHipError(RuntimeError):
    pass


# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "kr_version": [],
    "kr_last_error": [],
    "kr_device_info": [i32, C.c_char_p, C.POINTER(i32), C.POINTER(C.c_size_t)],
    "kr_set_device": [i32],
    "kr_stream_synchronize": [c_p],
    "kr_stream_create_cu_mask": [C.POINTER(c_p), i32],
    "kr_stream_create_cu_range": [C.POINTER(c_p), i32, i32],
    "kr_stream_destroy": [c_p],
    "kr_event_create": [C.POINTER(c_p)],
    "kr_event_destroy": [c_p],
    "kr_event_record": [c_p, c_p],
    "kr_event_synchronize": [c_p],
    "kr_stream_wait_event": [c_p, c_p],
    "kr_event_elapsed_ms": [c_p, c_p, C.POINTER(f32)],
    "kr_graph_begin_capture": [c_p],
    "kr_graph_end_capture": [c_p, C.POINTER(c_p)],
    "kr_graph_launch": [c_p, c_p],
    "kr_graph_destroy": [c_p],
    "kr_cast_pad_f32_bf16": [c_p, c_p, i64, i32, i32, c_p],
    "kr_layernorm": [c_p, c_p, c_p, c_p, i64, i32, f32, c_p],
    "kr_rmsnorm": [c_p, i64, c_p, c_p, i64, i32, f32, c_p],
    "kr_gemm_bf16": [c_p, i64, c_p, c_p, c_p, i64, c_p, i64, i64, i32, i32, i32, i32, c_p],
    "kr_decode_resnorm": [c_p, i64, c_p, i32, i32, c_p, i64, c_p, f32, c_p, i64, i32, i32, c_p],
    "kr_decode_resnorm32": [c_p, i64, c_p, i32, i32, c_p, i64, c_p, f32, c_p, i32, i32, i32, c_p],
    "kr_pack_rows32": [c_p, i64, i32, i32, c_p, c_p],
    "kr_linear_decode32": [i32, c_p, c_p],
    "kr_attn_decode_merge32": [c_p, c_p, i32, i32, i32, i32, c_p],
    "kr_attn_decode_merge16": [c_p, c_p, i32, i32, i32, i32, c_p],
    "kr_quantize_rows_fp8": [c_p, i64, c_p, i64, c_p, i64, i32, c_p],
    "kr_gemm_fp8a": [c_p, i64, c_p, c_p, c_p, c_p, c_p, i64, c_p, i64, i64, i32, i32, i32, c_p],
    "kr_gemm_bf16_ws": [c_p, i64, c_p, c_p, c_p, i64, c_p, i64, i64, i32, i32, i32, i32, c_p, C.c_size_t, c_p],
    "kr_gemv_bf16": [c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, i64, i32, i32, i32, i32, c_p, f32, c_p],
    "kr_qkv_prep": [c_p, i64, i32, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p, i64, c_p, i64, c_p, i64,
                    i32, i32, i32, c_p],
    "kr_rope2d_vision": [c_p, c_p, c_p, i64, i32, i32, i64, c_p],
    "kr_attn_varlen": [c_p, c_p, c_p, c_p, c_p, c_p, i32, i64, i32, i32, i32, i64, i64, f32, i32, c_p],
    "kr_attn_varlen_q": [c_p, c_p, c_p, c_p, c_p, c_p, i32, i64, i32, i32, i32, i64, i64, f32, i32, i32, c_p],
    "kr_embed_scatter": [c_p, c_p, c_p, c_p, i64, i32, c_p],
    "kr_mrope": [c_p, c_p, c_p, i64, i32, i32, i64, c_p],
    "kr_kv_append": [c_p, c_p, i64, c_p, c_p, c_p, c_p, i64, i32, i32, i32, i32, i32, c_p],
    "kr_decode_qkv_prep": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, c_p],
    "kr_attn_decode_gqa": [c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, i32, f32, c_p],
    "kr_argmax_embed": [c_p, i64, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, i32, i32, c_p],
    "kr_argmax": [c_p, i64, i32, c_p, i32, c_p],
    "kr_linear_decode": [i32, c_p, i64, c_p, c_p, c_p, f32, c_p, i64, c_p, c_p, i64, i32, i32, i32, i32, i32, i32, c_p, c_p,
                         c_p, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, c_p, c_p],
    "kr_linear_decode_wide": [i32, c_p, i64, c_p, c_p, c_p, f32, c_p, i64, c_p, c_p, i64, i32, i32, i32, i32, i32, c_p, c_p, c_p],
    "kr_image_resize_bicubic_u8": [c_p, i32, i32, c_p, i32, i32, c_p, c_p, c_p, i32, c_p, c_p, i32, c_p],
    "kr_image_normalize_patchify": [c_p, i32, i32, c_p, c_p, i32, i32, i32, c_p, c_p],
    "kr_linear_decode_wide_fp8": [i32, c_p, i64, c_p, c_p, c_p, c_p, f32, c_p, i64, c_p, c_p, i64, i32, i32, i32, i32, i32, c_p, c_p, c_p],
    "kr_linear_decode_narrow_fp8": [i32, c_p, i64, c_p, i32, c_p, i64, c_p, c_p, c_p, c_p, f32, c_p, i64, c_p, c_p, i64,
                                    i32, i32, i32, i32, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, c_p],
    "kr_fp8_to_bf16": [c_p, c_p, i64, c_p],
    "kr_gemm_fp8": [c_p, i64, c_p, c_p, c_p, c_p, i64, c_p, i64, i64, i32, i32, i32, c_p],
    "kr_gumbel_argmax": [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, c_p],
    "kr_gumbel_argmax_guided": [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, c_p, c_p, i32, i32, c_p],
    "kr_guide_build_masks": [c_p, c_p, i32, c_p, c_p, i32, c_p, i32, c_p, i32, c_p],
    "kr_sample_threshold": [c_p, i64, i32, c_p, c_p, c_p, i64, c_p, i32, c_p, c_p, i32, c_p, i32, c_p, i64, c_p, c_p, i32, c_p],
    "kr_gumbel_argmax_processed": [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, c_p, c_p, i32, i32, c_p, c_p, i64, c_p,
                                   i32, c_p, c_p],
    "kr_sample_threshold_rows": [c_p, i64, i32, c_p, c_p, c_p, i64, c_p, i32, c_p, c_p, i32, c_p, i32, c_p, i64, c_p, c_p, i32, c_p, c_p,
                                 c_p, i32, i32, c_p],
    "kr_gumbel_argmax_processed_rows": [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, c_p, c_p, i32, i32, c_p, c_p, i64, c_p,
                                        i32, c_p, c_p, c_p, c_p, i32, i32, c_p],
    "kr_sample_count": [c_p, c_p, c_p, i64, i32, i32, c_p],
    "kr_logits_adjust": [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p],
    "kr_logits_adjust_rows": [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p, i32, c_p],
    "kr_logits_restore": [c_p, i64, i32, c_p, c_p, c_p, i32, c_p],
    "kr_logits_restore_rows": [c_p, i64, i32, c_p, c_p, c_p, i32, c_p, i32, c_p],
    "kr_stop_tokens": [c_p, c_p, c_p, c_p, c_p, i32, i32, c_p],
    "kr_guide_advance": [c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, c_p],
    "kr_kv_fork": [c_p, c_p, i64, i64, i64, i64, i64, i64, i32, i32, i32, i32, i32, c_p, c_p],
    "kr_logprobs_topk": [c_p, i64, i32, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, c_p],
    "kr_linear_decode_narrow": [i32, c_p, i64, c_p, i32, c_p, i64, c_p, c_p, c_p, f32, c_p, i64, c_p, c_p, i64,
                                i32, i32, i32, i32, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, c_p],
    "kr_attn_decode_fused": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, f32, c_p],
    "kr_attn_decode_slots": [c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, f32, c_p],
    "kr_attn_decode_merge": [c_p, c_p, i32, i32, i32, i32, c_p],
    "kr_sample_greedy": [c_p, c_p, i32, c_p, i32, c_p, c_p, i32, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, i32, c_p],
    "kr_spec_propose": [c_p, c_p],
    "kr_spec_accept": [c_p, c_p, c_p, i32, c_p, c_p, i32, i32, c_p],
    "kr_spec_lookup": [c_p, c_p, c_p],
    "kr_spec_deal": [c_p, c_p, c_p, c_p],
    "kr_spec_accept_rows": [c_p, c_p, c_p, c_p, i32, c_p, c_p, i32, i32, c_p],
    "kr_spec_guide_trim": [c_p, c_p, c_p, c_p],
    "kr_spec_guide_rows": [c_p, c_p, c_p, c_p],
    "kr_spec_guide_advance": [c_p, c_p, c_p],
    "kr_spec_controls_trim": [c_p, c_p, c_p, c_p],
    "kr_spec_controls_rows": [c_p, c_p, c_p, c_p],
    "kr_spec_controls_count": [c_p, c_p, c_p],
    "kr_spec_mark": [c_p, c_p, c_p],
    "kr_logprobs_topk_rows": [c_p, c_p, c_p, c_p, i64, c_p],
    "kr_repeat_detect": [c_p, c_p],
    "kr_linear_decode32_rows": [i32, c_p, c_p, c_p],
    "kr_attn_decode_rows": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, f32, c_p],
    "kr_kv_quantize": [c_p, c_p, c_p, i32, i32, i32, i32, c_p, c_p, c_p],
    "kr_kv_absmax": [c_p, c_p, i32, i32, i32, i32, c_p, f32, f32, c_p, c_p, c_p],
    "kr_kv_fork8": [c_p, c_p, i64, i64, i64, i64, i64, i64, i32, i32, i32, i32, i32, c_p, c_p],
    "kr_attn_decode_slots_kv8": [c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, f32, c_p],
    "kr_attn_decode_rows_kv8": [c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, i32, f32, c_p],
    "kr_linear_decode_narrow_kv8": [c_p, i64, c_p, i32, c_p, i64, c_p, c_p, c_p, c_p, f32, i32, i32, i32, i32, c_p, i32, c_p, c_p,
                                    c_p, c_p, i32, i32, i32, c_p, c_p],
    "kr_linear_decode32_kv8": [c_p, c_p, c_p, c_p],
    "kr_comm_unique_id": [c_p],
    "kr_comm_init": [C.POINTER(c_p), i32, i32, c_p],
    "kr_comm_count": [c_p, C.POINTER(i32)],
    "kr_comm_destroy": [c_p],
    "kr_rccl_version": [C.POINTER(i32)],
    "kr_bcast_weights": [c_p, c_p, C.c_size_t, i32, c_p],
    "kr_selftest_mfma": [c_p],
    "kr_probe_launch_floor": [c_p, i32, i32, i32, C.POINTER(f32)],
    "kr_probe_stream_read": [c_p, C.c_size_t, i32, i32, c_p, C.POINTER(f32)],
    "kr_launch_null": [c_p],
}
_RESTYPES = {"kr_last_error": C.c_char_p}

# include/karanta_hip_experiments.h: exported only by -DKR_EXPERIMENTS builds (csrc/tools/build_variant.py, loaded through
# KARANTA_HIP_LIB); bound when present, absent from the shipped library
EXPERIMENT_SIGNATURES = {
    "kr_linear_decode_narrow_x32": [i32, c_p, i64, c_p, i32, c_p, i64, c_p, i64, c_p, c_p, c_p, c_p, f32, c_p, i64, c_p, c_p, i64,
                                    i32, i32, i32, i32, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p,
                                    c_p, C.c_size_t, i32, c_p],
    "kr_oproj_heads": [c_p, i32, c_p, c_p, c_p, i64, i32, i32, i32, c_p],
    "kr_linear_decode_wide_x32": [i32, c_p, i64, c_p, i64, c_p, c_p, c_p, f32, c_p, c_p, i64, i32, i32, i32, i32, i32, c_p, c_p, c_p],
    "kr_prefetch": [c_p, C.c_size_t, i32, c_p],
}


class NarrowOpts(C.Structure):
    """kr_narrow_opts (include/karanta_hip.h): the explicit per-launch options of kr_linear_decode_narrow*."""
    _fields_ = [("zero_ptr", c_p), ("zero_bytes", C.c_uint64), ("atomic_out", C.c_int32), ("part_rows", C.c_int32),
                ("w_resident", C.c_int32)]


class NarrowOptsXP(C.Structure):
    """kr_narrow_opts of a launch on a packed x operand (x_packed = 1).  The same 32 bytes as NarrowOpts, whose tail ctypes
    zero-fills: a launch on row-major x keeps the record it had before the field existed (tests/launch_trace.py lists a struct
    by its fields)."""
    _fields_ = NarrowOpts._fields_ + [("x_packed", C.c_int32)]


def narrow_opts(zero_ptr: int = 0, zero_bytes: int = 0, atomic_out: bool = False, part_rows: int = 0, w_resident: bool = False,
                x_packed: bool = False):
    """A kr_narrow_opts* for one launch (0 = NULL when every field is at its default).  The struct is read during the
    call only, so the temporary may die right after it."""
    if not (zero_bytes or atomic_out or part_rows or w_resident or x_packed):
        return None
    head = (zero_ptr or None, int(zero_bytes), 1 if atomic_out else 0, int(part_rows), 1 if w_resident else 0)
    return C.byref(NarrowOptsXP(*head, 1) if x_packed else NarrowOpts(*head))

class Dec32(C.Structure):
    """kr_dec32 (include/karanta_hip.h): the arguments of kr_linear_decode32."""
    _fields_ = [("xp", c_p), ("w_packed", c_p), ("w_scale", c_p), ("bias", c_p), ("residual", c_p), ("ldr", C.c_int64),
                ("out", c_p), ("out_f32", c_p), ("ldc", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("waves_ref", C.c_int32), ("ksplit", C.c_int32), ("atomic_out", C.c_int32), ("tiles_per_wg", C.c_int32),
                ("group_split", C.c_int32), ("reserved0", C.c_int32), ("zero_ptr", c_p), ("zero_bytes", C.c_uint64),
                ("cs_table", c_p), ("cs_stride", C.c_int32), ("prompt_len", c_p), ("ctx_len", c_p),
                ("q_out", c_p), ("kcache", c_p), ("vtcache", c_p), ("heads", C.c_int32), ("kv_heads", C.c_int32), ("s_max", C.c_int32)]


class Spec(C.Structure):
    """kr_spec (include/karanta_hip.h): the layout and the buffers of a speculative decode step."""
    _fields_ = [("slots", C.c_int32), ("k", C.c_int32), ("rows", C.c_int32), ("ngram_min", C.c_int32), ("ngram_max", C.c_int32),
                ("s_max", C.c_int32), ("prompt_ids", c_p), ("prompt_stride", C.c_int64), ("history", c_p), ("hist_stride", C.c_int32),
                ("hist_rows", C.c_int32), ("script", c_p), ("script_len", c_p), ("row_slot", c_p), ("ctx_len", c_p),
                ("prompt_len", c_p), ("finished", c_p), ("temperature", c_p), ("seed", c_p), ("n_draft", c_p), ("draft_tok", c_p),
                ("embed_table", c_p), ("d", C.c_int32), ("pad_id", C.c_int32), ("vocab", C.c_int32), ("x", c_p), ("ldx", C.c_int64),
                ("proposed", c_p), ("accepted", c_p)]


class SpecGuide(C.Structure):
    """kr_spec_guide (include/karanta_hip.h): the guides of a speculative step's rows and the scratch of its three launches."""
    _fields_ = [("guide_trans", c_p), ("guide_masks", c_p), ("guide_state", c_p), ("mask_words", C.c_int32), ("vocab_off", c_p),
                ("vocab_bytes", c_p), ("draft_state", c_p), ("ctx_before", c_p)]


class SpecControls(C.Structure):
    """kr_spec_controls (include/karanta_hip.h): the slots' adjustment tables and output counts, the rows' depths and the scratch of
    the three launches that let controlled requests take part in a speculative step."""
    _fields_ = [("adj_ids", c_p), ("adj_flag", c_p), ("adj_meta", c_p), ("counts", c_p), ("ld_counts", C.c_int64), ("depth", c_p),
                ("ctx_before", c_p)]


class SpecLogprobs(C.Structure):
    """kr_spec_logprobs (include/karanta_hip.h): the scratch and the history kr_logprobs_topk_rows records a speculative step's
    tokens into."""
    _fields_ = [("k_top", C.c_int32), ("n_part", C.c_int32), ("part_val", c_p), ("part_idx", c_p), ("part_ms", c_p), ("out_lp", c_p),
                ("out_idx", c_p), ("hist_len", C.c_int32), ("hist_batch", C.c_int32), ("k_stride", C.c_int32), ("ctx_before", c_p)]


REP_MAX_PERIOD = 1024                   # KR_REP_MAX_PERIOD


class Repeat(C.Structure):
    """kr_repeat (include/karanta_hip.h): the history and the per-slot state kr_repeat_detect walks."""
    _fields_ = [("slots", C.c_int32), ("history", c_p), ("hist_stride", C.c_int32), ("hist_rows", C.c_int32), ("ctx_len", c_p),
                ("prompt_len", c_p), ("finished", c_p), ("cfg", c_p), ("run", c_p), ("seen", c_p), ("rep_at", c_p),
                ("flags", C.c_int32)]


class Kv8(C.Structure):
    """kr_kv8 (include/karanta_hip.h): one layer of the fp8 KV cache and its [2][kv_heads] scales."""
    _fields_ = [("k", c_p), ("vt", c_p), ("scale", c_p)]


def kv8(k: int, vt: int, scale: int):
    """A kr_kv8* from three device addresses; read during the call only."""
    return C.byref(Kv8(k, vt, scale))


KVQ_MAX_ROWS = 32                       # KR_KVQ_MAX_ROWS


class KvqPlan(C.Structure):
    """kr_kvq_plan (include/karanta_hip.h): the (slot, prompt length) rows kr_kv_quantize converts."""
    _fields_ = [("n", C.c_int32), ("slot", C.c_int32 * KVQ_MAX_ROWS), ("len", C.c_int32 * KVQ_MAX_ROWS)]


def kvq_plan(rows):
    """A kr_kvq_plan* from [(slot, prompt length), ...]; too many rows are passed on as a count the library rejects."""
    p = KvqPlan()
    p.n = len(rows) if len(rows) <= KVQ_MAX_ROWS else -1
    for i, (slot, n) in enumerate(list(rows)[:KVQ_MAX_ROWS]):
        p.slot[i], p.len[i] = int(slot), int(n)
    return C.byref(p)


FORK_MAX_GROUPS = FORK_MAX_SLOTS = 32   # KR_FORK_MAX_GROUPS / KR_FORK_MAX_SLOTS


class ForkGroup(C.Structure):
    """kr_fork_group (include/karanta_hip.h)."""
    _fields_ = [("src", C.c_int32), ("n_tokens", C.c_int32), ("n_dst", C.c_int32), ("dst", C.c_int32 * FORK_MAX_SLOTS)]


class ForkPlan(C.Structure):
    """kr_fork_plan (include/karanta_hip.h): what kr_kv_fork copies."""
    _fields_ = [("n_groups", C.c_int32), ("groups", ForkGroup * FORK_MAX_GROUPS)]


def fork_plan(groups):
    """A kr_fork_plan* from [(source slot, n_tokens, [destination slots]), ...].  Like kr_narrow_opts it is read during the call
    only.  What the struct cannot hold (too many groups / destinations) is passed on as a count the library rejects."""
    p = ForkPlan()
    p.n_groups = len(groups) if len(groups) <= FORK_MAX_GROUPS else -1
    for g, (src, n_tokens, dst) in zip(p.groups, groups):
        g.src, g.n_tokens = int(src), int(n_tokens)
        g.n_dst = len(dst) if len(dst) <= FORK_MAX_SLOTS else -1
        for i, j in enumerate(list(dst)[:FORK_MAX_SLOTS]):
            g.dst[i] = int(j)
    return C.byref(p)


ABI_MAJOR = 5              # include/karanta_hip.h KR_ABI_VERSION / 100: the header this binding was written against
DEC_OUT_XP = 0x100         # KR_DEC_OUT_XP
DEC_OUT_XP16 = 0x200       # KR_DEC_OUT_XP16
ADJ_CAP = 320              # KR_ADJ_CAP: entries per row of the logit-adjustment tables (kr_logits_adjust)
EPI_NONE, EPI_QUICK_GELU, EPI_GELU_ERF, EPI_SILU_MUL, EPI_SILU_MUL8 = 0, 1, 2, 3, 4
DEC_PLAIN, DEC_SILU, DEC_ROPE_KV, DEC_ARGMAX, DEC_SILU8 = 0, 1, 2, 3, 4


class _Lib:
    def __init__(self, path: str):
        if not os.path.exists(path):
            raise KarantaHipError(
                f"{path} not found: build it with `python -m karanta_ocr_amd.build` "
                "(the MI355X engine has no CPU fallback)")
        import torch  # noqa: F401  (loads torch's libamdhip64 / librccl first; see module docstring)

        try:
            self._dll = C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError as e:  # pragma: no cover
            raise KarantaHipError(f"cannot load {path}: {e}") from e
        self.path = path
        for name, argtypes in SIGNATURES.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError as e:
                raise KarantaHipError(f"{path} does not export {name}") from e
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
            if name in ("kr_version", "kr_last_error"):
                setattr(self, name, fn)
            else:
                setattr(self, name, self._checked(name, fn))
        if self.kr_version() // 100 != ABI_MAJOR:
            raise KarantaHipError(f"{path} reports kr_version() = {self.kr_version()}, this binding is written against ABI major "
                                  f"{ABI_MAJOR} (include/karanta_hip.h): rebuild with `python -m karanta_ocr_amd.build`")
        self.experiments = hasattr(self._dll, "kr_oproj_heads")
        for name, argtypes in EXPERIMENT_SIGNATURES.items():
            if self.experiments:
                fn = getattr(self._dll, name)
                fn.argtypes, fn.restype = argtypes, C.c_int
                setattr(self, name, self._checked(name, fn))
            else:
                setattr(self, name, self._absent(name))

    @staticmethod
    def _absent(name):
        def call(*_):
            raise KarantaHipError(f"{name} is an experiment entry point (include/karanta_hip_experiments.h): this library was built "
                                  "without -DKR_EXPERIMENTS (csrc/tools/build_variant.py; load it through KARANTA_HIP_LIB)")
        call.__name__ = name
        return call

    def _checked(self, name, fn):
        def call(*args):
            rc = fn(*args)
            if rc != 0:
                msg = self._dll.kr_last_error()
                raise KarantaHipError(f"{name} -> {rc}: {msg.decode() if msg else ''}")
            return rc

        call.__name__ = name
        call.raw = fn
        return call


_LIB: Optional[_Lib] = None


def lib() -> _Lib:
    global _LIB
    if _LIB is None:
        _LIB = _Lib(os.environ.get("KARANTA_HIP_LIB", LIB_PATH))
    return _LIB


def ptr(t) -> int:
    """Device/host address of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()
