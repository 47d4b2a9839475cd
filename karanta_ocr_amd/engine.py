"""MI355X inference engine for the karanta OCR hot path: Qwen2-VL ViT -> scatter -> prefill ->
greedy decode, every arithmetic step a hand-written HIP kernel behind include/karanta_hip.h.

This is the thing the reference reaches over HTTP (``vllm serve``,
/root/reference/karanta/pipeline.py:707-742, :317-319) or through Hugging Face ``generate``
(/root/reference/karanta/training/test_trained_model.py:76-99).  PyTorch is used for device
memory and streams only; there is no torch arithmetic and no CPU fallback on this path.

Batching model: one `generate` call = one static batch of <= max_batch pages (one image +
prompt each, any mix of sizes); pages of different requests never interact.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import image_processing as IP
from . import positions as POS
from ._lib import (DEC_ARGMAX, DEC_OUT_XP, DEC_OUT_XP16, DEC_PLAIN, DEC_ROPE_KV, DEC_SILU8, Dec32, EPI_NONE, EPI_SILU_MUL8, KarantaHipError, lib,
                   narrow_opts, ptr)
from . import kv_cache
from .config import ModelConfig
from .kv_cache import KV_SCALES_FLAG_WINS   # noqa: F401  (cli.py takes it from here)
from .weights import KV_SCALE_RANGES, kv_cache_dtype_name
from .device_weights import DeviceWeights, _align, narrow_weight_bytes, plan_resident
from .request import GenerateResult, PageRequest, SpecConfig, children
from .sampler import DeviceGuide, Sampler
from .sampling import StepFeatures, has_penalties, spec_refusal
from .speculative import Speculator
from .vision import DevicePlan, VisionTower, device_plan

BF16 = torch.bfloat16
GEMM_SCRATCH_BYTES = 512 * 65536   # include/karanta_hip.h: KR_GEMM_SCRATCH_BYTES
FP8_ACT_DEFAULT = False            # fp8 engines: W8A8 prefill on by default? (measured error and speed)
# default-on switches of csrc/tools/experiment_engine.ExperimentEngine that select a superseded decode launch sequence
# Infinity-Cache residency of the <= 16-row narrow launches' weights (kr_narrow_opts.w_resident):
# (launch kind, us saved per MB of its weights kept resident, measured inside a replayed 2B / 8-row step), and the default budget.
# qkv: 12.3 us per step for 176 MB; o_proj (2.8 us for 132 MB) and down_proj (none) stayed inside the spread of three repeats
# and are left out (profiles/r05_ic_residency.txt).  192 MB: the smallest swept budget that holds qkv in all 28 layers of the 2B model.
IC_RESIDENT_GAINS: Tuple[Tuple[str, float], ...] = (("qkv", 0.07),)
IC_RESIDENT_MB = 192
# a launch is planned only if its expected saving reaches what two identical graphs differ by per launch in that sweep (3-4 us per
# step over 28 launches): the sub-MB matrices of the test-sized models keep their nontemporal loads
IC_RESIDENT_MIN_US = 0.1
SEQUENCE_SWITCHES = ("KARANTA_NARROW", "KARANTA_NARROW_O", "KARANTA_DEFER_DOWN", "KARANTA_WIDE", "KARANTA_ATOMIC_SLAB", "KARANTA_DEC32")

__all__ = ["Engine", "PageRequest", "SpecConfig", "DeviceWeights", "GenerateResult", "children", "SEQUENCE_SWITCHES", "DeviceGuide"]


@dataclass
class Admission:
    """One admission — a whole batch (`generate`) or new requests for some slots — from the host tables
    (Engine._prefill_prepare) over the sampling state (Engine.prefill) to the activation of its sequences (Engine._activate)."""
    B: int
    slots: List[int]
    whole_batch: bool
    lens: List[int]
    M: int
    src: np.ndarray          # int32 [M]: token id, or -(image row + 1)
    cos: np.ndarray          # fp32 [M, head_dim] M-RoPE tables of the prompts
    sin: np.ndarray
    deltas: np.ndarray       # int32 [max_batch]
    plan: POS.AttnPlan
    last_rows: np.ndarray    # int32 [B]: row of every prompt's last token
    cs: np.ndarray           # fp32 [B, max_new, head_dim] rotary table of the decode positions
    n_img: int
    # added by prefill: what the sampler keeps per sequence
    temps: Optional[np.ndarray] = None
    seeds: Optional[np.ndarray] = None
    guides: Optional[list] = None      # Sampler._guide_rows
    procs: Optional[list] = None       # Sampler._control_rows
    adjs: Optional[list] = None        # Sampler._adjust_rows
    reps: Optional[list] = None        # per sequence its RepetitionParams or None
    need: StepFeatures = StepFeatures()
    # parallel sampling: B / slots / lens / last_rows / cs count SEQUENCES (children); the prefill (M, src, cos, sin, plan) covers
    # every page once, in child 0's slot, and `forks` names what KVCache.fork copies afterwards
    n_pages: int = 0
    rows: list = field(default_factory=list)    # `children` of the admission's pages, made once per admission
    forks: list = field(default_factory=list)   # (source slot, prompt length, [sibling slots]) per page with n > 1
    kvq: list = field(default_factory=list)     # (slot, prompt length) per prefilled page: what the fp8 KV cache quantises

    def spans(self, width: int):
        """(first sequence, first slot, slots) of what an activation does per stretch of slots: a whole batch is ONE stretch of
        `width` slots from slot 0 (its sequences, or max_batch with the idle rows behind them); named slots go one by one, the
        others keep their state."""
        return [(0, 0, width)] if self.whole_batch else [(b, j, 1) for b, j in enumerate(self.slots)]

    def copies(self, rows: np.ndarray, width: int):
        """(first slot, host rows) of the copies that put one per-sequence field in place: `spans` of the field's `width` rows, a
        whole batch padded with zeros."""
        if self.whole_batch:
            rows = np.concatenate([rows[:self.B], np.zeros(width - self.B, rows.dtype)])
        return [(j, rows[b:b + n]) for b, j, n in self.spans(width)]


class Engine:
    def __init__(self, cfg: ModelConfig, device: str = "cuda:0", max_batch: int = 8, s_max: int = 4096,
                 max_patches: int = 8 * 5476, max_prompt_tokens: int = 8 * 2048, decode_splits: int = 16,
                 weight_dtype: str = "bf16", fp8_activations: Optional[bool] = None, admission_cus: Optional[int] = None,
                 speculative: Optional[SpecConfig] = None, ic_resident_mb: Optional[int] = None, kv_cache_dtype: str = "auto",
                 calculate_kv_scales: bool = False, kv_scale_ranges: Tuple[float, float] = KV_SCALE_RANGES):
        if not torch.cuda.is_available():
            raise KarantaHipError("no HIP device: the karanta MI355X engine has no CPU fallback")
        self.L = lib()
        self.cfg = cfg
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.s = self.stream.cuda_stream
        self.B = max_batch
        if max_batch > 32:
            raise KarantaHipError("max_batch > 32: the decode kernels take at most two 16-row column tiles")
        # a speculative step runs max_batch x (K + 1) rows through the packed 17..32-row family (never fewer than 17 rows: its
        # gate/up launch writes packed activations above 16 rows only); without `speculative` the rows are the slots.
        # (SpecConfig.rows; with shared rows at most 32 of them: the rows behind the slots' own are dealt per step)
        self.spec = speculative
        if speculative is not None:
            speculative.check(max_batch)
        self.K = int(speculative.num_tokens) if speculative is not None else 0
        self.rows = speculative.rows(max_batch) if speculative is not None else max_batch
        self.spec_steps = self.plain_steps = 0
        self._snap_counts = None
        self.s_max = _align(s_max, 64)
        self.max_patches = max_patches
        self.max_tokens = max_prompt_tokens
        self.n_split = decode_splits
        self._ignore_eos = self._freeze_finished = self._want_logits = False
        # _caps: the passes the current mode ALLOWS (begin_slots(sampling=, guided=); generate(): what its pages need);
        # _step: the passes the next decode step RUNS — in slot mode they follow the requests that are actually in the slots
        # (set_step_features), and an admission switches on what it needs (_admit_features)
        self._caps = self._step = StepFeatures()
        self._logprobs = None         # None or k: the decode graph records log-probabilities (kr_logprobs_topk)
        self._adm_stream = None                          # second stream of the overlapped admission (slot mode)
        # overlapped admissions run on a stream restricted to this many compute units (kr_stream_create_cu_mask), so the
        # decode graph on the main stream always finds free CUs beside the admission's long-running workgroups; 0 / None: an
        # ordinary second stream (round 1: no gain, the streams serialise).  KARANTA_ADMIT_CUS overrides.
        env_cus = os.environ.get("KARANTA_ADMIT_CUS")
        self.admission_cus = int(env_cus) if env_cus is not None else (int(admission_cus) if admission_cus else 0)
        self._adm_stream_handle = None
        # ... and, while an admission is in flight on it, the decode graph replays on a stream restricted to the OTHER compute units
        # (kr_stream_create_cu_range): disjoint sets, so neither side waits for a workgroup slot of the other.  Measured alone
        # (tools/decode_ab.py --cus): a 32-row step keeps 94 / 70 / 47 % of its speed on 75 / 50 / 25 % of the CUs.
        self.disjoint_decode = os.environ.get("KARANTA_DISJOINT_DECODE", "1") != "0"
        self._dec_stream, self._dec_stream_handle, self._adm_inflight = None, None, 0
        self.n_cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        self.persist_blocks = int(os.environ.get("KARANTA_PERSIST_BLOCKS", "512"))  # 2 persistent workgroups per CU (swept: 256..1024)
        self._refuse_retired_switches()
        v, t = cfg.vision, cfg.text
        # --kv-cache-dtype: "auto" = bfloat16; "fp8" = "fp8_e4m3": e4m3 codes with one f32 scale per (layer, K or V, kv head)
        self.kv_cache_dtype = kv_cache_dtype_name(kv_cache_dtype)
        self.kv8 = self.kv_cache_dtype == "fp8"
        if self.kv8 and t.head_dim != 128:
            raise KarantaHipError(f"kv_cache_dtype fp8 needs a text head_dim of 128, this model has {t.head_dim}: the fp8 cache's "
                                  "quantise, append and attention kernels are written for 128-byte K rows")
        # --calculate-kv-scales: the FIRST prefill writes the scale table from the absolute maxima of its own K / V:
        # scale = amax / range per (layer, K or V, kv head) (kv_cache.KVCacheFp8)
        self.calculate_kv_scales = bool(calculate_kv_scales)
        if self.calculate_kv_scales and not self.kv8:
            raise KarantaHipError("calculate_kv_scales: the KV cache is bfloat16, there are no scales to calculate "
                                  "(kv_cache_dtype=\"fp8\" quantises it)")
        self.kv_scale_ranges = tuple(float(r) for r in kv_scale_ranges)
        if len(self.kv_scale_ranges) != 2 or not all(np.isfinite(r) and r > 0 for r in self.kv_scale_ranges):
            raise KarantaHipError(f"kv_scale_ranges {kv_scale_ranges!r}: (K range, V range), finite and positive")
        if v.head_dim not in (80, 128) or t.head_dim != 128:
            raise KarantaHipError(f"unsupported head dims vit={v.head_dim} llm={t.head_dim}")
        self.w = DeviceWeights(cfg, self.device, weight_dtype)
        self.fp8 = weight_dtype == "fp8"
        self.set_resident_budget(IC_RESIDENT_MB if ic_resident_mb is None else ic_resident_mb)
        # fp8 engine: prefill GEMMs read the fp8 codes (kr_gemm_fp8); KARANTA_FP8_PREFILL=0: their dequantised bf16 copy
        self.fp8_prefill_gemm = os.environ.get("KARANTA_FP8_PREFILL", "1") == "1"
        # W8A8 prefill (fp8 engine): the activations entering the decoder's prefill GEMMs are quantised per token to e4m3
        # (kr_quantize_rows_fp8) and the products run on the fp8 matrix instruction (kr_gemm_fp8a) — what vLLM does for the
        # reference's OLMO_7B_0725_FP8.  Decode keeps bf16 activations (weight-only fp8).  KARANTA_FP8_ACT=0/1 overrides.
        env = os.environ.get("KARANTA_FP8_ACT")
        self.fp8_act = self.fp8 and self.fp8_prefill_gemm and (bool(fp8_activations) if fp8_activations is not None
                                                              else (env == "1" if env is not None else FP8_ACT_DEFAULT))
        self._graphs: Dict[Tuple[int, bool], int] = {}
        self._prof_on = False
        self._prof_events: List[Tuple[C.c_void_p, C.c_void_p]] = []
        self._prof_next = 0
        self._last_batch = max_batch
        self._alloc()

    def set_resident_budget(self, mb: int, gains: Optional[Sequence[Tuple[str, float]]] = None):
        """The (layer, kind) whose <= 16-row narrow launches load their weights with the default cache policy: up to `mb` MB of
        them stay in the Infinity Cache from one decode step to the next (device_weights.plan_resident).  gains: the planner's
        (kind, us per MB) list when it is not the measured one (tools, tests).  The policy is baked into captured decode
        graphs, so a call after construction drops them."""
        for g in getattr(self, "_graphs", {}).values():
            self.L.kr_graph_destroy(g)
        getattr(self, "_graphs", {}).clear()
        self.ic_resident_mb = int(mb)
        self.resident = plan_resident(narrow_weight_bytes(self.cfg, self.w.weight_dtype),
                                      IC_RESIDENT_GAINS if gains is None else gains, self.ic_resident_mb * 10 ** 6,
                                      IC_RESIDENT_MIN_US)

    def _refuse_retired_switches(self):
        if type(self) is Engine and any(os.environ.get(k, "0") not in ("", "0") for k in
                                        ("KARANTA_PREFETCH", "KARANTA_FAST_RESIDUAL", "KARANTA_ATTN_FUSED", "KARANTA_MERGE_IN_OPROJ")):
            raise KarantaHipError("KARANTA_PREFETCH / KARANTA_FAST_RESIDUAL / KARANTA_ATTN_FUSED / KARANTA_MERGE_IN_OPROJ are decode "
                                  "experiments: they run on csrc/tools/experiment_engine.ExperimentEngine with a -DKR_EXPERIMENTS "
                                  "library (csrc/tools/build_variant.py, KARANTA_HIP_LIB), not on the product engine")
        # the switches that used to select a superseded launch sequence: refused, not ignored (an A/B of two identical runs)
        if os.environ.get("KARANTA_RESNORM32_QKV", "1") != "1":
            raise KarantaHipError("KARANTA_RESNORM32_QKV is retired: the packed family with the fused row-major qkv launch was "
                                  "measured and dropped (profiles/r04_decode32_chains.txt)")
        moved = [k for k in SEQUENCE_SWITCHES if os.environ.get(k, "1") != "1"] + [k for k in ("KARANTA_RESNORM_QKV",) if k in os.environ]
        if type(self) is Engine and moved:
            raise KarantaHipError(" / ".join(moved) + ": superseded decode launch sequences run on csrc/tools/experiment_engine."
                                  "ExperimentEngine (csrc/tools/decode_ab.py builds it for such a variant), not on the product engine")

    # ------------------------------------------------------------------ buffers
    def _alloc(self):
        t, dev = self.cfg.text, self.device
        M, B, R = self.max_tokens, self.B, self.rows
        z = lambda *shape, dtype=BF16: torch.zeros(*shape, dtype=dtype, device=dev)
        self.vision = VisionTower(self)
        # decoder prefill
        self.p_x = z(M, t.hidden_size)
        self.p_h = z(M, t.hidden_size)
        self.p_qkv = z(M, t.qkv_dim)
        self.p_q = z(t.num_heads, M, t.head_dim)
        self.p_o = z(M, t.q_dim)
        self.p_act = z(M, t.intermediate_size)
        self.p_cos = z(M, t.head_dim, dtype=torch.float32)
        self.p_sin = z(M, t.head_dim, dtype=torch.float32)
        self.p_src = z(M, dtype=torch.int32)
        if self.fp8_act:   # W8A8 prefill: the quantised A operand (row stride = the widest K) and its per-token scales
            self.p_a8 = z(M, (max(t.intermediate_size, t.hidden_size, t.q_dim) + 15) // 16 * 16, dtype=torch.uint8)
            self.p_as = z(M, dtype=torch.float32)
        self.gemm_scratch = z(GEMM_SCRATCH_BYTES // 4, dtype=torch.float32)   # kr_gemm_bf16_ws (KR_GEMM_SCRATCH_BYTES)
        self.kv = kv_cache.make(self)     # the KV cache: storage, scales and the launches that depend on its dtype
        # decode state
        self.d_x = z(R, t.hidden_size)
        self.d_x2 = z(R, t.hidden_size)  # the other residual buffer (deferred split-K ping-pong)
        # down_proj slabs of the deferred split: [2][B][hidden]; > 16 rows with the group-split down_proj: two PAIRS (layer parity)
        self.d_part = z(4 if R > 16 else 2, R, t.hidden_size, dtype=torch.float32)
        # ONE-slab form of the deferred split: down_proj's two K ranges add into one f32 accumulator with float atomics
        # (a + b onto zero: order-free, reproducible); two accumulators alternate by layer parity, layer L's qkv launch
        # zeroes the one layer L's down_proj adds into.  d_part doubles as the pair.
        # down_proj at >= 192 weight tiles (7B widths) runs two tiles per workgroup (kr_decode.hip, launch_narrow_direct):
        # 8-wave workgroups with a 5-deep ring then beat 16-wave ones (7B step 2.992 -> 2.975 ms)
        if t.hidden_size // 16 >= 192:
            self.down_waves_small = 8
        self.d_qkv = z(B, t.qkv_dim)
        # batches above 16 rows keep the inputs of their decode linears in the PACKED layout of kr_linear_decode32 (32 row
        # slots whatever the batch): d_h (normalised rows of kr_decode_resnorm32), d_o (merged heads), d_act (SiLU * up)
        Bp = 32 if R > 16 else B
        self.d_h = z(Bp, t.hidden_size)
        self.d_q = z(R, t.num_heads, t.head_dim)
        self.d_o = z(Bp, t.q_dim)
        self.d_act = z(Bp, t.intermediate_size)
        self.d_logits = z(R, t.vocab_size, dtype=torch.float32)
        self.d_ws = z(R * t.num_heads * self.n_split * (t.head_dim + 4), dtype=torch.float32)
        # waves per workgroup of the narrow decode linears: enough waves that every wave still
        # streams >= 2 K-chunks, no cross-workgroup reduction (each fence/atomic hop costs microseconds)
        self.wv_qkv = self._waves(t.hidden_size // 64)
        self.wv_o = self._waves(t.q_dim // 64)
        self.wv_down = self._waves(t.intermediate_size // 64)
        self.wv_wide = 4
        for name in ("qkv", "o", "down", "wide"):  # tuning overrides (sweeps): KARANTA_WV_DOWN=8 ...
            v_ = os.environ.get("KARANTA_WV_" + name.upper())
            if v_:
                setattr(self, "wv_" + name, int(v_))
        # down_proj split over 2 workgroups per tile with the reduction deferred to the next layer's qkv prologue
        # (K = 1536 / 2048 / 3584 only)
        self.defer_down = t.hidden_size in (1536, 2048, 3584)
        # <= 16 rows at those widths: o_proj and down_proj read their x operand PACKED (the XP16 layout, kr_narrow_opts.x_packed:
        # whole cache lines instead of 16 rows x 64 B per wave instruction; same bits), written by
        # kr_attn_decode_merge16 and the gate/up launch with DEC_OUT_XP16.  Sized for 16 rows whatever the batch (8 row slots per
        # chunk up to 8 rows, 16 above: the launches of a step agree through their M); row slots >= B are never stored by that step
        # and never used: they hold the zeros of the allocation or an earlier step's finite values.
        self.narrow_xp = self.defer_down and self.narrow_mode and not self.kv8
        if self.narrow_xp:
            self.d_o_xp = z(16, t.q_dim)
            self.d_act_xp = z(16, t.intermediate_size)
        # gate/up and lm_head: one wave per 16-row tile (kr_linear_decode_wide) when K allows it
        self.wide_mode = t.hidden_size % 512 == 0 and t.hidden_size <= 4096
        self.wide_blocks = int(os.environ.get("KARANTA_WIDE_BLOCKS", "256"))
        self.wide_waves = int(os.environ.get("KARANTA_WIDE_WAVES", "0"))  # 0: ceil(tiles / blocks), at most 8
        self.wide_spread32 = os.environ.get("KARANTA_WIDE_SPREAD32", "1") == "1"   # > 16 rows: tiles dealt as at <= 16 rows (_wide_geometry)
        if R > 16 and not (self.wide_mode and t.intermediate_size % 64 == 0):
            raise KarantaHipError("max_batch > 16 needs the wide / narrow decode kernels (hidden_size % 512 == 0) and hidden_size <= 2048 or == 3584")
        # Above 16 rows the narrow linears (qkv behind kr_decode_resnorm32, o_proj, down_proj) run as the packed-activation
        # family (kr_linear_decode32) and the wide launches (gate/up, lm_head) hold two 16-row column tiles per weight
        # fragment, with all 32 normalised x rows in LDS — which fits up to hidden_size 2048 (Qwen2-VL-2B, Qwen2.5-VL-3B).
        # At the 7B width (32 x 3584 bf16 = 229 KB against 160 KB of LDS) they stage K in two halves (dec_wide_kh_kernel:
        # weights still read once): row_split.
        self.row_split = self.B > 16 and t.hidden_size > 2048
        self.family32, self.resnorm_qkv = self.B > 16, self.row_split     # what bench.py --full counts launches from
        self.group_split_down = int(os.environ.get("KARANTA_DOWN_GS", "1"))   # 0 off, 1 at 16-atom partitions (2B widths), 2 always
        if R > 16 and t.hidden_size > 2048 and t.hidden_size != 3584:
            raise KarantaHipError("max_batch > 16: hidden_size <= 2048 or == 3584 (the 7B width) only")
        if self.fp8 and not self.wide_mode:
            raise KarantaHipError("fp8 weights need the wide / narrow decode kernels: hidden_size % 512 == 0 and <= 4096")
        # one argmax partial per wave of the lm_head launch; the launch geometry depends on the row count (8 waves above
        # 16 rows), so the buffers are sized for the larger one and the sampler is told the launch's own count
        self.n_amax = (max(self._amax_parts(0), self._amax_parts(32)) if self.wide_mode
                       else (t.vocab_size // 16 + 1) // 2)
        self.d_amax_v = z(R, self.n_amax, dtype=torch.float32)
        self.d_amax_i = z(R, self.n_amax, dtype=torch.int32)
        # per-ROW state (prompt length, context, finished, temperature, seed): the slots' entries are in front — what every launch of
        # a plain step and the host read — and a speculative step writes the entries of its draft rows behind them
        self.d_plen = z(R, dtype=torch.int32)[:B]
        self.d_cs = None  # [B][max_new][128] rotary table of the decode positions, built per request
        self.d_ctx = z(R, dtype=torch.int32)[:B]
        self.d_delta = z(B, dtype=torch.int32)
        self.d_tok = z(B, dtype=torch.int32)
        self.d_fin = z(R, dtype=torch.int32)[:B]
        self._snap_ring, self._snap_next, self._snap_event, self._copy_stream = None, 0, None, None   # snapshot_slots()
        self._rep_read = np.full(B, -1, np.int64)     # slot_rep_at()
        self.d_temp = z(R, dtype=torch.float32)[:B]   # per-slot sampling temperature and seed
        self.d_seed = z(R, dtype=torch.int32)[:B]
        self.sampler = Sampler(self)
        self.speculator = Speculator(self) if self.spec is not None else None     # the speculative step: speculative.py
        self.max_new = 0          # size of the token history / rotary tables (only grows: graphs hold their addresses)
        self._req_max_new = 0     # what the current generate() / begin_slots() asked for (capacity checks use this)
        self.d_hist = None
        self.d_eos = torch.tensor(list(self.cfg.eos_token_ids), dtype=torch.int32, device=dev)
        self.d_invfreq = torch.from_numpy(POS.rope_inv_freq(t.head_dim, t.rope_theta)).to(dev)
        self.d_last = z(B, dtype=torch.int32)
        # per slot the hidden row of its prompt's last token (written at every admission) and, on the host, the length of the
        # prompt whose KV rows the slot holds: what admit_reuse starts a sequence from without ViT or prefill
        self.d_prompt_x = z(B, t.hidden_size)
        self._slot_plen = [0] * B
        self.pages_prefilled = self.sequences_started = self.sequences_forked = self.sequences_reused = 0
        torch.cuda.synchronize(dev)

    @staticmethod
    def _waves(nchunks: int) -> int:
        return 16 if nchunks >= 64 else 8 if nchunks >= 16 else 4

    # ------------------------------------------------------------------ KV cache: the component's public entries
    def set_kv_scales(self, k, v, source: str = "set_kv_scales"):
        """The scales of the fp8 KV cache: k and v are [L] or [L, KVH] arrays, a code stands for code x scale.  They apply to what
        enters the cache from now on: set them before the first admission."""
        self.kv.set_scales(k, v, source)

    def kv_scales(self) -> np.ndarray:
        """The [L, 2, KVH] scale table (K scales, then V scales, per layer) from its host mirror: what set_kv_scales put there, or
        what the calibrating admission calculated — as of the last admission whose stream has been waited for (generate, admit,
        admit_end), like kv_clamped.  `set_kv_scales(table[:, 0], table[:, 1])` on another engine pins it."""
        return self.kv.scales()

    @property
    def kv_scales_ready(self) -> bool:
        """calculate_kv_scales: the calibrating admission has run on the device and kv_scales() holds what it calculated.  A query
        of an event, no synchronisation."""
        return self.kv.scales_ready

    @property
    def kv_scales_calibrated(self) -> bool:
        """True once the calibrating admission has been launched."""
        return self.kv.calibrated

    @property
    def kv_clamped(self) -> int:
        """Elements the COMPLETED admissions clamped to +-448 x scale on their way into the fp8 cache (kr_kv_quantize's counter, as
        of the last admission whose stream has been waited for: generate, admit, admit_end).  No synchronisation here."""
        return self.kv.clamped

    @property
    def kv_scale_source(self) -> str:
        return self.kv.scale_source

    def kv_cache_bytes(self) -> int:
        return self.kv.nbytes()

    # the component's tensors under the names they had on the engine, read-only: what tests and operators' scripts inspect.
    # Properties, not attributes: the tensors have one holder (tests/launch_trace.py names pointers by it)
    kcache = property(lambda self: self.kv.kcache)
    vtcache = property(lambda self: self.kv.vtcache)
    d_kv_scale = property(lambda self: self.kv.d_kv_scale)
    d_kv_work = property(lambda self: self.kv.d_kv_work)

    def load_weights(self, weights: Dict[str, np.ndarray], log=None):
        self.w.load(weights)
        self.kv.load_scales(weights, log)

    # ------------------------------------------------------------------ small launch helpers
    def _gemm(self, A, W, C_, M, bias=None, res=None, epi=EPI_NONE, packed=False, w8=None, w_scale=None):
        N, K = W.shape
        if w8 is not None and self.fp8_act:
            # W8A8: per-token e4m3 codes of A (scale = max|row| / 448), both operands through v_mfma_f32_16x16x32_fp8_fp8
            ldq = self.p_a8.stride(0)
            self.L.kr_quantize_rows_fp8(ptr(A), A.stride(0), ptr(self.p_a8), ldq, ptr(self.p_as), M, K, self.s)
            self.L.kr_gemm_fp8a(ptr(self.p_a8), ldq, ptr(self.p_as), ptr(w8), ptr(w_scale), ptr(bias), ptr(res),
                                res.stride(0) if res is not None else 0, ptr(C_), C_.stride(0), M, N, K, epi, self.s)
            return
        if w8 is not None and self.fp8_prefill_gemm:
            # fp8 engine: the prefill streams the SAME e4m3 codes + row scales the decode kernels read (kr_gemm_fp8)
            self.L.kr_gemm_fp8(ptr(A), A.stride(0), ptr(w8), ptr(w_scale), ptr(bias), ptr(res),
                               res.stride(0) if res is not None else 0, ptr(C_), C_.stride(0), M, N, K, epi, self.s)
            return
        # split-K scratch of long-K tail rounds: the engine's own buffer (its GEMMs never run on two streams at once)
        self.L.kr_gemm_bf16_ws(ptr(A), A.stride(0), ptr(W), ptr(bias), ptr(res), res.stride(0) if res is not None else 0,
                               ptr(C_), C_.stride(0), M, N, K, epi, 1 if packed else 0, ptr(self.gemm_scratch),
                               self.gemm_scratch.numel() * 4, self.s)

    def _dec(self, mode, x, W, M, out=None, out_f32=None, norm_w=None, waves=4):
        """kr_linear_decode on packed weights: gate/up and lm_head at the widths without the wide kernels."""
        t = self.cfg.text
        N, K = W.shape
        o = out if out is not None else out_f32
        self.L.kr_linear_decode(mode, ptr(x), x.stride(0), ptr(W), 0, ptr(norm_w), t.rms_norm_eps, 0, 0, ptr(out), ptr(out_f32),
                                o.stride(0) if o is not None else 0, M, N, K, waves, self.persist_blocks, 1, 0, 0,
                                0, self.n_split, ptr(self.d_cs), self.max_new, ptr(self.d_plen),
                                ptr(self.d_ctx), ptr(self.d_q), 0, 0, t.num_heads, t.num_kv_heads, self.s_max,
                                ptr(self.d_amax_v), ptr(self.d_amax_i), self.s)

    def _dec_narrow(self, mode, x, W, M, out=None, out_f32=None, bias=None, norm_w=None, res=None, waves=8, ksplit=1,
                    part_in=None, x_out=None, kc=0, vc=0, w8=None, w_scale=None, zero=None, atomic_out=False,
                    resident=False, kv8=None, x_packed=False):
        """kr_linear_decode_narrow: one workgroup per tile (pair); ksplit > 1 = deferred split-K sums in out_f32.
        w8 / w_scale: the fp8 copy of W and its row scales (kr_linear_decode_narrow_fp8).  zero (an f32 tensor the launch
        also zeroes), atomic_out, resident (w_resident: the weights stay in the Infinity Cache), x_packed (x is a packed
        buffer, d_o_xp / d_act_xp): the launch's kr_narrow_opts.
        kc / vc (addresses) or kv8 (a kr_kv8*): the layer of the cache a qkv launch appends to, as `self.kv.qkv(i)` names it."""
        t = self.cfg.text
        N, K = W.shape
        o = out if out is not None else out_f32
        if kv8 is not None:     # the qkv launch into the fp8 cache (ROPE_KV8): same launch, the cache as a kr_kv8
            self.L.kr_linear_decode_narrow_kv8(
                ptr(x), x.stride(0), ptr(part_in), int(part_in.shape[0]) if part_in is not None else 0, ptr(x_out),
                x_out.stride(0) if x_out is not None else 0, ptr(w8 if w8 is not None else W), ptr(w_scale), ptr(bias), ptr(norm_w),
                t.rms_norm_eps, M, N, K, waves, ptr(self.d_cs), self.max_new, ptr(self.d_plen), ptr(self.d_ctx), ptr(self.d_q),
                kv8, t.num_heads, t.num_kv_heads, self.s_max,
                narrow_opts(ptr(zero), zero.numel() * 4 if zero is not None else 0, atomic_out, w_resident=resident), self.s)
            return
        head = (mode, ptr(x), x.stride(0), ptr(part_in), int(part_in.shape[0]) if part_in is not None else 0, ptr(x_out),
                x_out.stride(0) if x_out is not None else 0)
        args = (ptr(bias), ptr(norm_w), t.rms_norm_eps, ptr(res), res.stride(0) if res is not None else 0, ptr(out),
                ptr(out_f32), o.stride(-2) if o is not None else 0, M, N, K, waves, ksplit, ptr(self.d_cs), self.max_new,
                ptr(self.d_plen), ptr(self.d_ctx), ptr(self.d_q), kc, vc, t.num_heads, t.num_kv_heads, self.s_max,
                narrow_opts(ptr(zero), zero.numel() * 4 if zero is not None else 0, atomic_out, w_resident=resident,
                            x_packed=x_packed), self.s)
        if w8 is not None:
            self.L.kr_linear_decode_narrow_fp8(*head, ptr(w8), ptr(w_scale), *args)
        else:
            self.L.kr_linear_decode_narrow(*head, ptr(W), *args)

    def _dec32(self, mode, xp, W, M, waves_ref, out=None, out_f32=None, bias=None, res=None, ksplit=1, atomic_out=False, zero=None,
               kc=0, vc=0, w8=None, w_scale=None, tiles_per_wg=0, group_split=False, row_slot=None, kv8=None):
        """kr_linear_decode32: the decode linears of a 17..32-row batch on PACKED activations (xp: kr_pack_rows32 layout, written
        by kr_decode_resnorm32 / kr_attn_decode_merge32 / the gate/up launch with DEC_OUT_XP), with the K partition of the
        <= 16-row launch of the same layer (waves_ref, ksplit): row for row the bits that launch produces."""
        t = self.cfg.text
        N, K = W.shape
        o = out if out is not None else out_f32
        a = Dec32(ptr(xp), ptr(w8 if w8 is not None else W), ptr(w_scale), ptr(bias), ptr(res), res.stride(0) if res is not None else 0,
                  ptr(out), ptr(out_f32), o.stride(-2) if o is not None else 0, M, N, K, waves_ref, ksplit, 1 if atomic_out else 0,
                  tiles_per_wg, 1 if group_split else 0, 0, ptr(zero) if zero is not None else None,
                  zero.numel() * 4 if zero is not None else 0,
                  ptr(self.d_cs), self.max_new, ptr(self.d_plen), ptr(self.d_ctx), ptr(self.d_q), kc or None, vc or None,
                  t.num_heads, t.num_kv_heads, self.s_max)
        if kv8 is not None:   # the qkv launch into the fp8 cache (ROPE_KV8), with the row map of a speculative step or without
            self.L.kr_linear_decode32_kv8(C.byref(a), kv8, ptr(row_slot), self.s)
        elif row_slot is not None:    # speculative step: cache and rotary row by the row's slot (kr_linear_decode32_rows)
            self.L.kr_linear_decode32_rows(mode, C.byref(a), ptr(row_slot), self.s)
        else:
            self.L.kr_linear_decode32(mode, C.byref(a), self.s)

    # the shipped sequence; ExperimentEngine overrides these per instance; bench.py --full reads resnorm_qkv, family32,
    # resnorm32_qkv (the instance's wide_mode, defer_down, row_split, family32, resnorm_qkv follow from its config: _alloc)
    narrow_mode = narrow_o = atomic_slab = resnorm32_qkv = True

    down_waves_small = 16         # waves per down_proj workgroup at <= 16 rows (instance attribute for sweeps)
    down_gs_tiles = 0             # weight tiles per workgroup of the group-split down_proj (0: 4 at 8-atom partitions, else 2)
    o_waves = 8                   # waves per o_proj workgroup at <= 16 rows

    def _w8kw(self, name: str) -> dict:
        w8, sc = self._w8(name)
        return {} if w8 is None else {"w8": w8, "w_scale": sc}

    def _w8(self, name: str):
        """(fp8 codes, row scales) of a decoder Linear when the engine runs on fp8 weights, else (None, None)."""
        if self.fp8 and self.w.has(name + "8"):
            return self.w.view_u8(name + "8"), self.w.view_f32(name[:-1] + "s")
        return None, None

    def _wide_geometry(self, N: int, M: int = 0):
        """(workgroups, waves) of a wide launch.  No idle waves: W = tiles per CU (at most 8), then just enough
        workgroups for one tile per wave (gate/up of the 2B decoder: 1120 tiles = 224 workgroups x 5 waves);
        beyond that the waves loop over their tiles.  More than 16 rows: 8 waves, so that the branch-free prologue
        (4 rows per wave) stages all 32 rows — with 5 waves 12 rows went the slow way, behind the weight ring
        (gate/up at B = 32: 16.7 -> 14.7 us)."""
        tiles = N // 16
        if M > 16 and not self.wide_waves and self.wide_spread32:
            # r4: 8 waves stage the 32 rows, but the TILES are dealt as at <= 16 rows — to as many workgroups as there are compute
            # units to pull them (2B gate/up: 1120 tiles = 224 workgroups whose waves 0..4 own one tile each and waves 5..7 only
            # help with the prologue; 140 x 8 left 116 compute units without a weight stream)
            own = min(8, -(-tiles // self.wide_blocks))
            return min(self.wide_blocks, -(-tiles // own)), 8
        waves = self.wide_waves or (8 if M > 16 else min(8, -(-tiles // self.wide_blocks)))
        return min(self.wide_blocks, -(-tiles // waves)), waves

    def _amax_parts(self, M: int) -> int:
        """Argmax partials the lm_head launch writes per row at batch M (= its stride in d_amax_*): workgroups x waves."""
        wb, ww = self._wide_geometry(self.cfg.text.vocab_size, M)
        return wb * ww

    def _dec_wide(self, mode, x, W, M, out=None, out_f32=None, norm_w=None, w8=None, w_scale=None):
        """kr_linear_decode_wide: `wide_blocks` workgroups (one per CU), each wave an independent weight stream."""
        N, K = W.shape
        blocks, waves = self._wide_geometry(N, M)
        o = out if out is not None else out_f32
        tail = (0, ptr(norm_w), self.cfg.text.rms_norm_eps, 0, 0, ptr(out), ptr(out_f32), o.stride(0) if o is not None else 0,
                M, N, K, blocks, waves, ptr(self.d_amax_v), ptr(self.d_amax_i), self.s)
        if w8 is not None:
            self.L.kr_linear_decode_wide_fp8(mode, ptr(x), x.stride(0), ptr(w8), ptr(w_scale), *tail)
        else:
            self.L.kr_linear_decode_wide(mode, ptr(x), x.stride(0), ptr(W), *tail)

    def _h2d(self, dst: torch.Tensor, arr: np.ndarray):
        src = torch.from_numpy(np.ascontiguousarray(arr))
        dst.view(-1)[:src.numel()].copy_(src.view(-1), non_blocking=False)

    # ------------------------------------------------------------------ vision tower and guides: the components' public entries
    def patches_from_images(self, images, min_pixels: int = IP.MIN_PIXELS, max_pixels: int = IP.MAX_PIXELS_CLASS_DEFAULT, grids=None):
        return self.vision.patches_from_images(images, min_pixels, max_pixels, grids)

    def vit_forward(self, pixel_values, grids: Sequence[Sequence[int]]) -> torch.Tensor:
        return self.vision.vit_forward(pixel_values, grids)

    def set_vocab(self, token_bytes: Sequence[bytes]):
        self.sampler.set_vocab(token_bytes)

    def compile_guide(self, guide) -> DeviceGuide:
        return self.sampler.compile_guide(guide)

    def _attention(self, qkv, k_off, v_off, cos, sin, dp: DevicePlan, q, k, k_stride, vt, vt_stride, out, H, KVH, hd, causal):
        """Varlen attention of a fused [rows, q | k | v] buffer: kr_qkv_prep (rotary on q and k; q head-major, k rows and V^T
        blocks to where the plan says) then kr_attn_varlen_q over the plan's query blocks.  k / vt with their head strides: the
        ViT's scratch buffers, or a layer of the KV cache."""
        L, s = self.L, self.s
        L.kr_qkv_prep(ptr(qkv), qkv.shape[1], 0, k_off, v_off, ptr(cos), ptr(sin),
                      ptr(dp.blk_tok0), ptr(dp.blk_ntok), ptr(dp.blk_kr), ptr(dp.blk_vb), dp.n_blk,
                      ptr(q), q.stride(0), ptr(k), k_stride, ptr(vt), vt_stride, H, KVH, hd, s)
        L.kr_attn_varlen_q(ptr(q), ptr(k), ptr(vt), ptr(out), ptr(dp.qblk), ptr(dp.qlen), dp.host.qblk.shape[0], q.shape[1],
                           H, KVH, hd, k_stride, vt_stride, hd ** -0.5, 1 if causal else 0, dp.host.q_block, s)

    # ------------------------------------------------------------------ admission: host tables, prefill, slot state, first tokens
    def _ensure_history(self, max_new_tokens: int):
        """Token history, rotary table and (when asked for) log-prob history sized for max_new_tokens; their
        addresses are baked into captured graphs, so a reallocation drops the graphs."""
        max_new_tokens += self.K      # a speculative step may write K rows past what a plain step reaches
        grow = self.d_hist is None or self.max_new < max_new_tokens
        if grow:
            self.max_new = max_new_tokens
            self.d_hist = torch.zeros(max_new_tokens + 1, self.B, dtype=torch.int32, device=self.device)
            self.d_cs = torch.zeros(self.B, max_new_tokens, self.cfg.text.head_dim, dtype=torch.float32, device=self.device)
        grow = self.sampler.ensure_logprob_history(self.max_new + 1) or grow
        if grow:
            for g in self._graphs.values():
                self.L.kr_graph_destroy(g)
            self._graphs.clear()

    def _enter_mode(self, max_new_tokens: int, *, ignore_eos: bool, freeze_finished: bool, want_logits: bool, caps: StepFeatures,
                    step: StepFeatures, logprobs: Optional[int]):
        """The switches of a mode (generate(), slot mode, a tool's bare decode steps), THEN the history they size (log-probabilities
        get theirs only when asked for), THEN the budget the capacity checks use: in this order, or the history is smaller than
        the budget check assumes."""
        self._ignore_eos, self._freeze_finished, self._want_logits = bool(ignore_eos), bool(freeze_finished), bool(want_logits)
        self._caps, self._step = caps, step
        self._logprobs = None if logprobs is None else int(logprobs)
        self._ensure_history(max_new_tokens)
        self._req_max_new = int(max_new_tokens)

    def seq_room(self) -> int:
        """Cache rows one sequence may use: prompt + generated tokens (slot mode keeps the last row as the parking row)."""
        return self.s_max - (1 if self._freeze_finished else 0) - self.K     # (the draft rows' K/V land up to K rows ahead)

    def _prefill_prepare(self, pages: Sequence[PageRequest], n_image_tokens_total: Optional[int], slots: Optional[Sequence[int]] = None,
                         budgets: Optional[Sequence[int]] = None, rows: Optional[list] = None) -> Admission:
        """Host side of `prefill` (numpy only: token sources, M-RoPE tables of the prompt and of every decode position,
        the varlen attention plan).  `generate` runs it while the ViT launches are still executing.
        ``budgets``: per page, the number of tokens it may generate (slot mode: its max_tokens + the scheduler's chunk
        overshoot); default: the current request's max_new_tokens.  The bound is each page's OWN prompt + budget — not
        the engine-wide history size, which only grows.
        ``slots`` and ``budgets`` hold one entry per SEQUENCE (sum of the pages' n, `children` order); the prompt tables and the
        attention plan cover every page once, in the slot of its child 0.  ``n_image_tokens_total`` None (admit_reuse): nothing
        will be prefilled, so neither the image rows nor the prompt-token limit are checked.  ``rows``: `children(pages)` where the
        caller has made them already."""
        cfg, t = self.cfg, self.cfg.text
        rows = children(pages) if rows is None else rows
        ns = [int(getattr(p, "n", 1)) for p in pages]
        first = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)     # row of every page's child 0
        B = len(rows)
        whole_batch = slots is None
        slots = list(range(B)) if whole_batch else [int(j) for j in slots]
        if len(slots) != B or len(set(slots)) != B or min(slots) < 0 or max(slots) >= self.B:
            raise KarantaHipError(f"slots {slots} do not name {B} distinct slots below {self.B}")
        page_lens = [int(len(p.input_ids)) for p in pages]
        lens = [int(len(p.input_ids)) for p in rows]
        M = sum(page_lens)
        if n_image_tokens_total is not None and M > self.max_tokens:
            raise KarantaHipError(f"{M} prompt tokens > max_prompt_tokens {self.max_tokens}")
        if budgets is None:
            budgets = [self._req_max_new] * B
        if len(budgets) != B or max(budgets) > self.max_new - self.K:
            raise KarantaHipError(f"budgets {list(budgets)} do not fit {B} sequences / the history of {self.max_new - self.K} tokens")
        self._check_budgets(rows, budgets)
        src = np.empty(M, np.int32)
        cos = np.empty((M, t.head_dim), np.float32)
        sin = np.empty((M, t.head_dim), np.float32)
        deltas = np.zeros(self.B, np.int32)
        off, img_off = 0, 0
        for b, pg in enumerate(pages):
            ids = np.asarray(pg.input_ids).reshape(-1)
            is_img = ids == cfg.image_token_id
            k = int(is_img.sum())
            row = ids.astype(np.int64).copy()
            row[is_img] = -(np.arange(img_off, img_off + k) + 1)
            if row.max(initial=0) >= t.vocab_size:
                raise KarantaHipError("token id out of vocabulary")
            src[off:off + len(ids)] = row
            pos3, delta = POS.rope_index_one(ids, pg.grids, cfg.image_token_id, cfg.vision.spatial_merge_size)
            c, sn = POS.mrope_tables(pos3, t.head_dim, t.rope_theta, t.mrope_section)
            cos[off:off + len(ids)], sin[off:off + len(ids)] = c, sn
            deltas[first[b]:first[b + 1]] = delta
            off += len(ids)
            img_off += k
        if n_image_tokens_total is not None and img_off != n_image_tokens_total:
            raise KarantaHipError(f"Image features and image tokens do not match, tokens: {img_off}, "
                                  f"features: {n_image_tokens_total}")
        plan = POS.prefill_attn_plan(page_lens, [slots[f] for f in first[:-1]], t.num_kv_heads, self.s_max)
        last_rows = np.repeat(np.cumsum(page_lens) - 1, ns).astype(np.int32)
        # rotary table of every decode position of every sequence: pos = P + k + delta (all three
        # M-RoPE axes equal for generated text, TF:1124-1136), cos/sin rounded to bf16 (TF:169)
        kk = np.arange(self.max_new, dtype=np.int64)
        cs = np.zeros((B, self.max_new, t.head_dim), np.float32)
        for b in range(B):
            p1 = lens[b] + kk + int(deltas[b])
            c_, s_ = POS.mrope_tables(np.stack([p1, p1, p1]), t.head_dim, t.rope_theta, t.mrope_section)
            cs[b, :, : t.head_dim // 2], cs[b, :, t.head_dim // 2:] = c_[:, : t.head_dim // 2], s_[:, : t.head_dim // 2]
        forks = [(slots[first[i]], page_lens[i], slots[first[i] + 1:first[i + 1]]) for i in range(len(pages)) if ns[i] > 1]
        return Admission(B, slots, whole_batch, lens, M, src, cos, sin, deltas, plan, last_rows, cs, n_image_tokens_total,
                         n_pages=len(pages), rows=rows, forks=forks, kvq=[(slots[f], n) for f, n in zip(first[:-1], page_lens)])

    def _vit_and_prepare(self, pages: Sequence[PageRequest], pixel_values_device=None, slots: Optional[Sequence[int]] = None,
                         budgets: Optional[Sequence[int]] = None, rows: Optional[list] = None) -> Admission:
        """Front of every admission: the pages' images through the ViT (launches only), then the host tables of the prefill
        while those launches execute."""
        pix = self.vision._pixels_for(pages, pixel_values_device)
        n_img_tok = self.vit_forward(pix, [g for p in pages for g in p.grids]).shape[0] if pix is not None else 0
        return self._prefill_prepare(pages, n_img_tok, slots, budgets, rows)

    def prefill(self, pages: Sequence[PageRequest], n_image_tokens_total: int, slots: Optional[Sequence[int]] = None,
                defer_activation: bool = False, adm: Optional[Admission] = None) -> Admission:
        """embed+scatter, M-RoPE, 28 x decoder layer over the flattened prompts (causal varlen
        attention writing the KV cache), last-token logits -> first token.
        Leaves the decode state (d_x, d_ctx, d_delta, history row 0) ready.  Returns the admission's record (`lens`: the
        prompt lengths).  ``adm``: what `_prefill_prepare` made of these pages ahead of time.
        ``slots`` (slot scheduler): the cache / state slots the pages go to; only those slots' state is
        touched, the other sequences keep decoding from where they are.  ``defer_activation`` (overlapped
        admission): only the layers run here (they fill the slots' KV rows); `admit_end` activates the sequences (`_activate`) from the
        returned record on the decode stream."""
        t, L, s, w = self.cfg.text, self.L, self.s, self.w
        if adm is None or adm.n_img != n_image_tokens_total:
            adm = self._prefill_prepare(pages, n_image_tokens_total, slots)
        rows = adm.rows
        adm.need = self._admit_features(rows)
        M, d = adm.M, t.hidden_size
        with torch.cuda.stream(self.stream):
            self._h2d(self.p_src, adm.src)
            self._h2d(self.p_cos, adm.cos)
            self._h2d(self.p_sin, adm.sin)
            self.sampler._sampler_rows(adm, rows)
            if not defer_activation:
                self._activate(adm, tokens=False)
            self._h2d(self.d_last, adm.last_rows)
            dp = device_plan(adm.plan, self.device)
            L.kr_embed_scatter(ptr(self.p_src), ptr(w.view("llm.embed")), ptr(self.vision.img_embeds), ptr(self.p_x), M, d, s)
            for i in range(t.num_layers):
                p = f"llm.{i}."
                L.kr_rmsnorm(ptr(self.p_x), d, ptr(w.view(p + "ln1.w")), ptr(self.p_h), M, d, t.rms_norm_eps, s)
                self._gemm(self.p_h, w.view(p + "qkv.w"), self.p_qkv, M, bias=w.view(p + "qkv.b"), packed=True, **self._w8kw(p + "qkv.w"))
                kc, vc = self.kv.prefill_target(i)     # [max_batch, kv heads, ...]: the plan's rows count from slot 0
                self._attention(self.p_qkv, t.q_dim, t.q_dim + t.kv_dim, self.p_cos, self.p_sin, dp, self.p_q, kc, kc.stride(1),
                                vc, vc.stride(1), self.p_o, t.num_heads, t.num_kv_heads, t.head_dim, causal=True)
                self.kv.prefill_layer_done(i, adm)
                self._gemm(self.p_o, w.view(p + "o.w"), self.p_x, M, res=self.p_x, packed=True, **self._w8kw(p + "o.w"))
                L.kr_rmsnorm(ptr(self.p_x), d, ptr(w.view(p + "ln2.w")), ptr(self.p_h), M, d, t.rms_norm_eps, s)
                self._gemm(self.p_h, w.view(p + "gate_up.w"), self.p_act, M, epi=EPI_SILU_MUL8, packed=True, **self._w8kw(p + "gate_up.w"))
                self._gemm(self.p_act, w.view(p + "down.w"), self.p_x, M, res=self.p_x, packed=True, **self._w8kw(p + "down.w"))
            self.kv.prefill_done(adm)
            self.pages_prefilled += adm.n_pages
            if not defer_activation:
                self._fork(adm.forks)
                self._activate(adm, state=False)
        return adm

    def _fork(self, groups):
        """The prompt's KV rows of every (source slot, prompt length, [destination slots]), in one launch on the engine's current
        stream (KVCache.fork)."""
        if not groups:
            return
        self.kv.fork(groups)
        self.sequences_forked += sum(len(g[2]) for g in groups)

    def _admit_features(self, pages) -> StepFeatures:
        """What an admission's pages need: raises where the mode does not allow it, else the next steps carry it (from this
        admission on: its first token included).  Returns the need."""
        need = StepFeatures.of(pages)
        self.sampler.check_features(need)
        self._step |= need
        return need

    def _activate(self, a: Admission, src_of: Optional[Sequence[int]] = None, state: bool = True, tokens: bool = True):
        """Starts an admission's sequences in their slots, the same way whatever admitted them.
        `state`: the decode state, field by field from one list of (device field, host rows) — one copy per field for a whole
        batch, padded with zeros to max_batch rows; one-row copies into named slots, the others keep decoding — then the
        sampler's own fields (Sampler.write).
        `tokens`: every sequence's last prompt position -> its slot's x -> lm_head -> first token, the whole batch in one pass,
        named slots one by one.  The hidden row comes from the prefill just run (row d_last[b] of p_x; the children of a page read
        the same row), or with `src_of` (admit_reuse: per sequence the slot that holds its prompt) from what that prefill left
        in d_prompt_x — which every activation keeps per slot for exactly this.
        A non-deferred prefill writes the state before its layers and samples behind them; every other caller does both at once."""
        if state:
            lens = np.asarray(a.lens, np.int32)
            for j, n in zip(a.slots, a.lens):
                self._slot_plen[j] = int(n)
            self.sequences_started += a.B
            fields = ((self.d_delta, a.deltas), (self.d_ctx, lens - 1), (self.d_plen, lens),   # kr_sample_greedy adds 1 to ctx -> cached tokens
                      (self.d_temp, a.temps), (self.d_seed, a.seeds))
            for dst, rows in fields:
                for j, part in a.copies(rows, self.B):
                    self._h2d(dst[j:], part)
            for b, j, n in a.spans(a.B):
                self._h2d(self.d_cs[j:], a.cs[b:b + n])
            for _, j, n in a.spans(self.B):
                self.d_fin[j:j + n].zero_()
            if self.speculator is not None:
                self.speculator.write_prompts(a)
            self.sampler.write(a)
        if tokens:
            d = self.cfg.text.hidden_size
            for b, j, n in a.spans(a.B):
                if src_of is None:
                    self.L.kr_embed_scatter(ptr(self.d_last[b:]), ptr(self.p_x), 0, ptr(self.d_x[j:]), n, d, self.s)
                    self.L.kr_embed_scatter(ptr(self.d_last[b:]), ptr(self.p_x), 0, ptr(self.d_prompt_x[j:]), n, d, self.s)
                else:
                    if j != src_of[b]:
                        self.d_prompt_x[j].copy_(self.d_prompt_x[src_of[b]])
                    self.d_x[j].copy_(self.d_prompt_x[j])
                self._lm_head_and_sample(n, slot0=j)

    # ------------------------------------------------------------------ the step's tail: lm_head -> sampler passes -> tokens
    def _flags(self) -> int:
        """The flags word of kr_sample_greedy, of a speculative step's verification and of the sampler's passes."""
        return (1 if self._ignore_eos else 0) | (2 if self._freeze_finished else 0)

    def _lm_head(self, B: int, x, j: int = 0):
        """final RMSNorm (fused) -> lm_head with per-wave argmax partials over rows j .. j + B - 1 of x (TF:839, :1320-1323).
        Returns (the f32 logits where a later pass or the caller reads them, else None; the partials per row = the stride the
        launch wrote d_amax_* with)."""
        w, step = self.w, self._step
        logits = self.d_logits[j:] if (self._want_logits or step.sampling or step.processing or self._logprobs is not None) else None
        if self.wide_mode:
            self._dec_wide(DEC_ARGMAX, x[j:], w.view("llm.lm_head"), B, norm_w=w.view("llm.norm.w"), out_f32=logits)
        else:
            self._dec(DEC_ARGMAX, x[j:], w.view("llm.lm_head"), B, norm_w=w.view("llm.norm.w"), out_f32=logits,
                      waves=self.wv_wide)
        return logits, (self._amax_parts(B) if self.wide_mode else self.n_amax)

    def _lm_head_and_sample(self, B: int, x=None, slot0: int = 0):
        """lm_head -> the sampler's passes (Sampler.pre_token) -> greedy token over the argmax partials, bookkeeping and the next
        step's input embedding (generate(do_sample=False)) -> the passes behind the token (Sampler.post_token).
        x = the residual buffer holding the last layer's output (d_x unless the decode step ended on the
        other buffer); the next step's input embedding always goes to d_x."""
        t, w = self.cfg.text, self.w
        j = slot0  # rows j .. j+B-1 of every per-sequence array (the slot scheduler prefills single slots)
        logits, n_part = self._lm_head(B, self.d_x if x is None else x, j)
        flags = self._flags()
        n_part = self.sampler.pre_token(logits, n_part, B, j, flags)
        self.L.kr_sample_greedy(ptr(self.d_amax_v), ptr(self.d_amax_i), n_part, ptr(w.view("llm.embed")), t.hidden_size,
                                ptr(self.d_tok[j:]), ptr(self.d_hist[:, j:]), self.d_hist.stride(0), ptr(self.d_plen[j:]),
                                ptr(self.d_ctx[j:]), ptr(self.d_fin[j:]), ptr(self.d_eos), self.d_eos.numel(),
                                self.cfg.pad_token_id, flags, ptr(self.d_x[j:]), B, self.s)
        self.sampler.post_token(logits, B, j, flags)

    # ------------------------------------------------------------------ decode
    def _decode_step_launches(self, B: int):
        """One plain decode step over the B slots: the layers, then lm_head and the sampler."""
        self._lm_head_and_sample(B, self._layer_launches(B))

    def _gate_up(self, x, i: int, B: int, out_xp: bool = False, out_xp16: bool = False):
        """RMSNorm + gate/up + SiLU*mul of layer i over B rows of x into d_act; out_xp: in the packed layout kr_linear_decode32
        reads; out_xp16: into d_act_xp, in the packed layout the <= 16-row down_proj launch reads with x_packed."""
        w, p = self.w, f"llm.{i}."
        if self.wide_mode:
            self._dec_wide(DEC_SILU8 | (DEC_OUT_XP if out_xp else DEC_OUT_XP16 if out_xp16 else 0), x, w.view(p + "gate_up.w"), B,
                           out=self.d_act_xp if out_xp16 else self.d_act, norm_w=w.view(p + "ln2.w"), **self._w8kw(p + "gate_up.w"))
        else:
            self._dec(DEC_SILU8, x, w.view(p + "gate_up.w"), B, out=self.d_act, norm_w=w.view(p + "ln2.w"), waves=self.wv_wide)

    def _layer_launches(self, B: int, row_slot=None):
        """The layers of a decode step over B rows; returns the residual buffer that holds the last layer's output.  row_slot (a
        speculative step, B = self.rows): row r belongs to slot row_slot[r] — its K/V go to that slot's cache at the row's own
        position and its attention reads that cache (kr_linear_decode32_rows, KVCache.attention); the per-row state arrays are
        the slots' own, continued behind the slots.
        One decode step = 6 (<= 16 rows) or 7 (17..32 rows) launches per layer + 2 (Qwen2VLDecoderLayer TF:559-624, final norm
        TF:839, lm_head TF:1320-1323).
        <= 16 rows: [(x += down_proj sums) + RMSNorm + QKV + bias + M-RoPE + KV append] (kr_linear_decode_narrow) -> attention
        partials -> merge -> [o_proj + residual] (narrow) -> [RMSNorm + gate/up + SiLU*mul] (kr_linear_decode_wide) ->
        [down_proj (+ residual | deferred split-K sums)] (narrow).
        17..32 rows: the residual sum + RMSNorm are a launch of their own (kr_decode_resnorm32) and qkv, o_proj and down_proj
        read PACKED activations (kr_linear_decode32; written by kr_decode_resnorm32, kr_attn_decode_merge32 and gate/up with
        DEC_OUT_XP): same sums, row for row.  The superseded and the measured-and-not-adopted sequences (kr_linear_decode
        everywhere, two slabs, row-major launches above 16 rows, prefetch branches, fast-residual mode, in-launch merges)
        live in csrc/tools/experiment_engine.py."""
        t, L, w, s = self.cfg.text, self.L, self.w, self.s
        H, hd = t.num_heads, t.head_dim
        nl = t.num_layers
        big = B > 16                              # packed-activation family of 17..32-row batches
        xp16 = not big and self.narrow_xp         # <= 16 rows, production widths: o_proj / down_proj on packed x (one column tile)
        x, x_other = self.d_x, self.d_x2          # residual stream: swaps buffers at every deferred reduction
        pending = False                           # down_proj's split-K sums of the previous layer waiting in d_part
        # deferred split-K: down_proj's two K ranges add into one f32 accumulator; two accumulators alternate by layer parity
        slabs = self.d_part.view(-1)[: 2 * B * t.hidden_size].view(2, B, t.hidden_size)   # as down_proj packs them
        # > 16 rows, bf16 weights: down_proj's K ranges each in TWO workgroups (kr_dec32.group_split) adding into a slab per range;
        # the pair of a layer parity replaces the one slab, and kr_decode_resnorm32 adds x + (slab 0 + slab 1): the same bits
        # (measured, profiles/r04_down_group_split.txt: 2B / 32 rows 1.691 -> 1.678 ms per step; at the 7B width, where two tiles
        # per workgroup already share the x fragments, 3.968 -> 3.983: there it stays off unless KARANTA_DOWN_GS=2)
        gs = (big and self.defer_down and not self.fp8
              and (self.group_split_down == 2 or self.group_split_down == 1 and self.down_waves_small == 16)
              and (t.hidden_size // 16) % (4 if self.down_waves_small == 8 else 2) == 0)
        if gs:
            slabs = self.d_part.view(-1)[: 4 * B * t.hidden_size].view(2, 2, B, t.hidden_size)
        for i in range(nl):
            p = f"llm.{i}."
            defer = self.defer_down and i + 1 < nl
            # ---- 1. (x += down_proj sums of layer i - 1) -> RMSNorm -> QKV + bias + M-RoPE + KV append
            # this layer's down_proj will ADD into accumulator (i + 1) & 1: the qkv launch zeroes it (it was last read by
            # layer i - 1's qkv launch, which is complete)
            acc = slabs[(i + 1) & 1] if defer else None
            pin = (slabs[i & 1] if gs else slabs[i & 1:(i & 1) + 1]) if pending else None
            if big:
                # the residual sum + RMSNorm ONCE for the batch (bit-identical rows), then ONE qkv launch over all rows
                L.kr_decode_resnorm32(ptr(x), x.stride(0), ptr(pin), int(pin.shape[0]) if pending else 0, B, ptr(x_other),
                                      x_other.stride(0), ptr(w.view(p + "ln1.w")), t.rms_norm_eps, ptr(self.d_h), B, t.hidden_size,
                                      1 if (gs and pending) else 0, s)
                self._dec32(DEC_ROPE_KV, self.d_h, w.view(p + "qkv.w"), B, 8, bias=w.view(p + "qkv.b"), zero=acc,
                            row_slot=row_slot, **self.kv.qkv(i), **self._w8kw(p + "qkv.w"))
            else:
                self._dec_narrow(DEC_ROPE_KV, x, w.view(p + "qkv.w"), B, bias=w.view(p + "qkv.b"), norm_w=w.view(p + "ln1.w"),
                                 part_in=pin, x_out=x_other if pending else None, zero=acc,
                                 resident=(i, "qkv") in self.resident, **self.kv.qkv(i), **self._w8kw(p + "qkv.w"))
            if pending:
                x, x_other = x_other, x
            # ---- 2. split-KV attention partials, 3. their merge
            self.kv.attention(i, B, row_slot)
            if xp16:
                L.kr_attn_decode_merge16(ptr(self.d_ws), ptr(self.d_o_xp), B, H, hd, self.n_split, s)
            else:
                (L.kr_attn_decode_merge32 if big else L.kr_attn_decode_merge)(ptr(self.d_ws), ptr(self.d_o), B, H, hd, self.n_split, s)
            # ---- 4. o_proj + residual
            if big:
                self._dec32(DEC_PLAIN, self.d_o, w.view(p + "o.w"), B, self.o_waves, out=x, res=x, **self._w8kw(p + "o.w"))
            else:
                self._dec_narrow(DEC_PLAIN, self.d_o_xp if xp16 else self.d_o, w.view(p + "o.w"), B, out=x, res=x, waves=self.o_waves,
                                 resident=(i, "o") in self.resident, x_packed=xp16, **self._w8kw(p + "o.w"))
            # ---- 5. RMSNorm + gate/up + SiLU*mul (the kernel bench.py's roofline object is measured on)
            if self._prof_on:
                # [e0][e1] gate/up [e2]: the empty bracket e0..e1 measures what two back-to-back event
                # packets cost by themselves; it is subtracted from the bracket around the launch
                (e0, e1), (e2, _) = self._prof_event_pair(), self._prof_event_pair()
                L.kr_event_record(e0, s)
                L.kr_event_record(e1, s)
            self._gate_up(x, i, B, out_xp=big, out_xp16=xp16)
            if self._prof_on:
                L.kr_event_record(e2, s)
            # ---- 6. down_proj: two K ranges per tile whose sums the next layer's first launch adds to x (deferred split-K),
            # or (last layer / widths without the deferral) down_proj + residual
            down = dict(ksplit=2, out_f32=acc, atomic_out=True) if defer else dict(out=x, res=x)
            if gs and defer:
                self._dec32(DEC_PLAIN, self.d_act, w.view(p + "down.w"), B, self.down_waves_small, group_split=True,
                            tiles_per_wg=self.down_gs_tiles, **down)
            elif big:
                self._dec32(DEC_PLAIN, self.d_act, w.view(p + "down.w"), B, self.down_waves_small, **down, **self._w8kw(p + "down.w"))
            else:
                self._dec_narrow(DEC_PLAIN, self.d_act_xp if xp16 else self.d_act, w.view(p + "down.w"), B,
                                 waves=self.down_waves_small, **down, resident=(i, "down") in self.resident, x_packed=xp16,
                                 **self._w8kw(p + "down.w"))
            pending = defer
        return x

    # ------------------------------------------------------------------ speculative step: the component's public entries
    # SpecConfig's options as the slot scheduler (before it asks for a speculative chunk) and the tests read them
    share_rows = property(lambda self: self.spec is not None and bool(self.spec.share_rows))
    spec_guided = property(lambda self: self.spec is not None and bool(self.spec.guided))
    spec_controls = property(lambda self: self.spec is not None and bool(self.spec.controls))
    spec_logprobs = property(lambda self: self.spec is not None and bool(self.spec.logprobs))
    # the component's tensors that tools read off the engine, read-only: one holder each, as for the KV cache's
    d_spec_count = property(lambda self: self._need_speculator("d_spec_count").d_spec_count)
    d_row_slot = property(lambda self: self._need_speculator("d_row_slot").d_row_slot)

    def _need_speculator(self, who: str) -> Speculator:
        if self.speculator is None:
            raise KarantaHipError(who + ": the engine was built without speculative=SpecConfig(...)")
        return self.speculator

    def _spec_refusal(self) -> Optional[str]:
        """Why the next steps cannot be speculative (None: they can): sampling.spec_refusal."""
        return spec_refusal(self.spec, self._step, self._freeze_finished, self._logprobs is not None)

    def can_speculate(self) -> bool:
        """Whether decode_steps(speculative=True) would run with the passes the next steps carry."""
        return self._spec_refusal() is None

    def _spec_step_launches(self):
        self._need_speculator("speculative decode step refused").step_launches()

    def set_draft_script(self, slot: int, tokens: Optional[Sequence[int]]):
        self._need_speculator("set_draft_script").set_draft_script(slot, tokens)

    def spec_counts(self) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        return None if self.speculator is None else self.speculator.counts()

    def spec_counters(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._need_speculator("spec_counters").counters()

    # ------------------------------------------------------------------ live kernel timing (bench.py roofline)
    def _prof_event_pair(self):
        if self._prof_next == len(self._prof_events):
            e0, e1 = C.c_void_p(), C.c_void_p()
            self.L.kr_event_create(C.byref(e0))
            self.L.kr_event_create(C.byref(e1))
            self._prof_events.append((e0, e1))
        pair = self._prof_events[self._prof_next]
        self._prof_next += 1
        return pair

    def kernel_profile(self, reset: bool = True) -> Dict[str, float]:
        """Durations of the decode gate/up projection (the kernel that moves half of the decoder's bytes)
        measured with HIP events on the launch stream during the profiled eager steps.  Each sample is a HIP-event bracket around the one launch, minus an empty bracket
        (two events, nothing between) recorded right before it — the event packets' own cost.  Returns {launches, avg_us, min_us, bracket_us, null_bracket_us, bytes_per_launch}."""
        self.stream.synchronize()
        ms = C.c_float()
        vals, nulls = [], []
        ev = self._prof_events[: self._prof_next]
        for (e0, e1), (e2, _) in zip(ev[0::2], ev[1::2]):
            self.L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
            nulls.append(ms.value * 1e3)
            self.L.kr_event_elapsed_ms(e1, e2, C.byref(ms))
            vals.append(ms.value * 1e3)
        if reset:
            self._prof_next = 0
        t = self.cfg.text
        B = self._last_batch
        nbytes = 2 * (2 * t.intermediate_size * t.hidden_size + t.hidden_size + B * t.hidden_size + B * t.intermediate_size)
        raw = float(np.mean(vals)) if vals else 0.0
        null = float(np.mean(nulls)) if nulls else 0.0
        return {"launches": len(vals), "bracket_us": raw, "null_bracket_us": null, "avg_us": max(raw - null, 0.0),
                "min_us": float(np.min(vals) - null) if vals else 0.0, "bytes_per_launch": nbytes}

    def gate_up_chain_profile(self, B: int, reps: int = 8) -> Dict[str, float]:
        """Average launch duration of the decode gate/up kernel, HIP events on the launch stream around a replayed
        graph of reps x num_layers back-to-back launches, each on its own layer's weights (so no launch finds its
        weights in a cache: 28 x 55 MB against 32 MB of L2 and 256 MB of Infinity Cache).  The per-launch figure
        includes the dispatch gap between dependent launches, as a rocprofv3 kernel span in a graph replay does."""
        t, L = self.cfg.text, self.L
        e0, e1 = self._prof_event_pair()
        self._prof_next -= 1
        def chain(n):
            for _ in range(n):
                for i in range(t.num_layers):
                    self._gate_up(self.d_x, i, B)
        chain(1)                               # eager once (function attributes), then captured: a replayed
        self.stream.synchronize()              # graph issues the launches at the GPU's pace, not Python's
        g = C.c_void_p()
        L.kr_graph_begin_capture(self.s)
        try:
            chain(reps)
        finally:
            L.kr_graph_end_capture(self.s, C.byref(g))
        ms, best = C.c_float(), None
        for _ in range(3):
            L.kr_event_record(e0, self.s)
            L.kr_graph_launch(g, self.s)
            L.kr_event_record(e1, self.s)
            L.kr_event_synchronize(e1)
            L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
            best = ms.value if best is None else min(best, ms.value)
        L.kr_graph_destroy(g)
        ms.value = best
        n = reps * t.num_layers
        wbytes = 2 * t.intermediate_size * t.hidden_size * (1 if self.fp8 else 2) + (8 * t.intermediate_size if self.fp8 else 0)
        nbytes = wbytes + 2 * (t.hidden_size + B * t.hidden_size + B * t.intermediate_size)
        return {"launches": n, "avg_us": ms.value * 1e3 / n, "bytes_per_launch": nbytes}

    def _graph_key(self, B: int, spec: bool = False):
        return (B, self._ignore_eos, self._freeze_finished, self._logprobs, self._step, "spec" if spec else "plain")

    def _graph_for(self, B: int, spec: bool = False) -> int:
        key = self._graph_key(B, spec)
        assert not self._want_logits
        g = self._graphs.get(key)
        if g is None:
            L = self.L
            L.kr_graph_begin_capture(self.s)
            try:
                if spec:
                    self._spec_step_launches()
                else:
                    self._decode_step_launches(B)
            finally:
                ge = C.c_void_p()
                L.kr_graph_end_capture(self.s, C.byref(ge))
            g = ge.value
            self._graphs[key] = g
        return g

    # ------------------------------------------------------------------ public API
    def generate(self, pages: Sequence[PageRequest], max_new_tokens: int, ignore_eos: bool = False,
                 use_graph: bool = True, return_logits: bool = False, sync_every: int = 32,
                 pixel_values_device: Optional[torch.Tensor] = None, profile_every: int = 0,
                 force_tokens: Optional[np.ndarray] = None) -> GenerateResult:
        """Greedy generation for a static batch of pages (temperature 0 — the reference's
        ``build_page_query`` default, /root/reference/karanta/pipeline.py:166-171).

        ``pixel_values_device``: all pages' patches already resident in HBM (fp32 ``[n, 1176]``), used
        instead of the per-page host arrays.  ``profile_every`` > 0: every that many decode steps one
        step runs eagerly with HIP events around the dominant kernel (see :meth:`kernel_profile`).
        ``force_tokens`` (int [B, >= max_new_tokens - 1], eager path: a parity-test instrument): teacher forcing — after
        every sampling step the NEXT step's input embedding is replaced by that of the given token, while `tokens` /
        `logits` still report the engine's own argmax and logits.  With a reference's tokens as the forced sequence
        every step can be compared with the reference, also past a near-tie where free-running sequences part."""
        rows = children(pages)            # the batch's sequences: a page with n > 1 stands for n of them
        B = len(rows)
        if not 1 <= B <= self.B:
            raise KarantaHipError(f"batch {B} not in 1..{self.B}")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        t0 = time.perf_counter()
        if force_tokens is not None and any(has_penalties(p) for p in rows):
            raise KarantaHipError("force_tokens with repetition / frequency / presence penalties: the output counts would follow "
                                  "the engine's own tokens, not the forced ones")
        ks = [int(p.logprobs) for p in rows if getattr(p, "logprobs", None) is not None]
        if ks and not 0 <= max(ks) <= 20:
            raise KarantaHipError("logprobs must be in 0..20")
        self._last_batch = B
        need = StepFeatures.of(rows)
        self._enter_mode(max_new_tokens, ignore_eos=ignore_eos, freeze_finished=False, want_logits=return_logits, caps=need, step=need,
                         logprobs=max(ks) if ks else None)
        adm = self._vit_and_prepare(pages, pixel_values_device, rows=rows)
        self.stream.synchronize()
        t1 = time.perf_counter()
        lens = self.prefill(pages, adm.n_img, adm=adm).lens
        forced = None
        if force_tokens is not None:
            ft = np.asarray(force_tokens, np.int64)
            if ft.ndim != 2 or ft.shape[0] != B or ft.shape[1] < max_new_tokens - 1 or ft.min() < 0 or ft.max() >= self.cfg.text.vocab_size:
                raise KarantaHipError(f"force_tokens must be [B={B}, >= {max_new_tokens - 1}] token ids")
            forced = torch.from_numpy(np.ascontiguousarray(ft.T.astype(np.int32))).to(self.device)   # [steps, B]
            use_graph = False

        def force(k):     # the input of decode step k + 1 becomes the embedding of forced token k
            if forced is not None and k < forced.shape[0]:
                self.L.kr_embed_scatter(ptr(forced[k]), ptr(self.w.view("llm.embed")), 0, ptr(self.d_x), B,
                                        self.cfg.text.hidden_size, self.s)

        with torch.cuda.stream(self.stream):
            force(0)
        logits_steps = []
        if return_logits:
            self.stream.synchronize()
            logits_steps.append(self.d_logits[:B].float().cpu().numpy().copy())
        self.stream.synchronize()
        t2 = time.perf_counter()
        steps_done = 1
        with torch.cuda.stream(self.stream):
            want_graph = use_graph and not return_logits
            graph = self._graphs.get(self._graph_key(B)) if want_graph else None
            while steps_done < max_new_tokens:
                if graph is not None and profile_every and steps_done % profile_every == 0:
                    self._prof_on = True
                    self._decode_step_launches(B)
                    self._prof_on = False
                elif graph is not None:
                    self.L.kr_graph_launch(graph, self.s)
                else:
                    # eager step; the first one also sets per-kernel attributes, so capture only
                    # after it (no attribute calls inside a stream capture)
                    self._decode_step_launches(B)
                    force(steps_done)
                    if want_graph:
                        graph = self._graph_for(B)
                steps_done += 1
                if return_logits:
                    self.stream.synchronize()
                    logits_steps.append(self.d_logits[:B].float().cpu().numpy().copy())
                if not ignore_eos and steps_done % sync_every == 0:
                    self.stream.synchronize()
                    if bool(self.d_fin[:B].all().item()):
                        break
        self.stream.synchronize()
        t3 = time.perf_counter()
        hist = self.d_hist[:steps_done, :B].cpu().numpy().T  # [B, steps]
        toks, reasons, causes = [], [], []
        eos = set(int(e) for e in self.cfg.eos_token_ids)
        rep_at = self.sampler.d_rep_at[:B].cpu().numpy() if need.repetition else None
        for b in range(B):
            row = hist[b]
            cut, reason, cause = len(row), "length", None
            if not ignore_eos:       # a row's own stop ids end it as EOS does (kr_stop_tokens)
                hit = np.flatnonzero(np.isin(row, list(eos | set(int(x) for x in getattr(rows[b], "stop_token_ids", None) or ()))))
                if hit.size:
                    cut, reason = int(hit[0]) + 1, "stop"
                # the token the sequence repeats at is kept; an EOS or stop id at or before it wins (kr_repeat_detect)
                g = int(rep_at[b]) if rep_at is not None and getattr(rows[b], "repetition", None) is not None else -1
                if 0 <= g < len(row) and g + 1 < cut + (reason == "length"):
                    cut, reason, cause = g + 1, "length", "repetition"
            toks.append(row[:cut].astype(np.int64))
            reasons.append(reason)
            causes.append(cause)
        lps = None
        if self._logprobs is not None:
            lp = self.sampler.d_lp[:steps_done, :B].cpu().numpy()
            li = self.sampler.d_lpi[:steps_done, :B].cpu().numpy()
            lps = []
            for b, p in enumerate(rows):
                k = getattr(p, "logprobs", None)
                n = len(toks[b]) - (1 if reasons[b] == "stop" else 0)   # the EOS step records nothing
                lps.append(None if k is None else {"token": lp[:n, b, 0].copy(), "top": lp[:n, b, 1:1 + int(k)].copy(),
                                                   "top_ids": li[:n, b, :int(k)].astype(np.int64)})
        return GenerateResult(
            tokens=toks, finish_reasons=reasons, prompt_tokens=lens,
            timings={"vit_s": t1 - t0, "prefill_s": t2 - t1, "decode_s": t3 - t2, "total_s": t3 - t0,
                     "decode_steps": steps_done - 1},
            logits=np.stack(logits_steps, 1) if return_logits else None, logprobs=lps, stop_reasons=causes)

    # ------------------------------------------------------------------ slot scheduler API (continuous batching)
    # The decode graph always runs all `max_batch` slots; a slot whose sequence has finished idles in place
    # (kr_sample_greedy freeze bit) until `admit` prefills a new request into it.  See scheduler.SlotScheduler.
    def begin_slots(self, max_new_tokens: int, sampling: bool = False, guided: bool = False, logprobs: Optional[int] = None):
        """Enter slot mode: every slot idle, per-slot history / rotary tables sized for `max_new_tokens`.
        sampling=True: the decode graph carries the Gumbel-max pass, so requests may ask for temperature > 0.
        guided=True: that pass masks the logits of slots that carry a guide and their DFA state advances in the graph
        (needs set_vocab()).  logprobs=k: every step records log-probabilities of the token and of the k most probable."""
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if logprobs is not None and not 0 <= int(logprobs) <= 20:
            raise KarantaHipError("logprobs must be in 0..20")
        if guided and self.sampler.d_voc_off is None:
            raise KarantaHipError("guided decoding needs the vocabulary's byte strings: call Engine.set_vocab() first")
        # the sampling controls come with the sampling configuration; the steps carry each pass while a request needs it.  The
        # repetition pass chooses no token: every configuration allows it
        sampled = bool(sampling) or bool(guided)
        self._last_batch = self.B
        self._enter_mode(max_new_tokens, ignore_eos=False, freeze_finished=True, want_logits=False,
                         caps=StepFeatures(sampled, bool(guided), sampled, sampled, True), step=StepFeatures(), logprobs=logprobs)
        # a scheduler rebuilt after an exception may have left an overlapped admission in flight: without this the counter stays
        # above zero and every later decode_steps() replays the graph on the complement CU subset
        if self._adm_stream is not None:
            self._adm_stream.synchronize()
        self._adm_inflight = 0
        self._snap_event = self._snap_counts = None
        with torch.cuda.stream(self.stream):
            self.d_fin.fill_(1)
            self.d_temp.zero_()
            self.sampler.reset_slots()
            self.d_ctx.zero_()
            self.d_plen.zero_()
            self.d_x.zero_()
            if self.speculator is not None:
                self.speculator.reset_counters()
        self.spec_steps = self.plain_steps = 0
        self.stream.synchronize()

    def admit(self, pages: Sequence[PageRequest], slots: Sequence[int], budgets: Optional[Sequence[int]] = None) -> List[int]:
        """ViT + prefill of new requests into idle slots; their first token is sampled.  Returns prompt lengths.
        ``budgets``: tokens each page may generate before the host retires it (its max_tokens + the chunk overshoot)."""
        rows = children(pages)
        self._check_budgets(rows, budgets)       # before any launch: an oversized page fails the call, nothing ran
        adm = self._vit_and_prepare(pages, None, slots, budgets, rows)
        return self.prefill(pages, adm.n_img, slots=slots, adm=adm).lens

    def admit_reuse(self, pages: Sequence[PageRequest], srcs: Sequence[int], slots: Sequence[int],
                    budgets: Optional[Sequence[int]] = None) -> List[int]:
        """Start sequences from prompts that are already resident: pages[i] from the KV rows and the last-token hidden row that
        an earlier admission of the SAME prompt left in slot srcs[i] — no ViT, no prefill.  ``slots`` / ``budgets``: one entry per
        sequence as in `admit` (a page's n children consecutive).  A sequence whose slot is its source is re-activated in place;
        the others get the prompt's rows by one fork launch (the source may be decoding: its rows below the prompt length never
        change).  Runs on the decode stream only.  The caller vouches that srcs[i] holds this page's prompt; what the engine
        can check is its length.  Returns prompt lengths per sequence."""
        rows = children(pages)
        self._check_budgets(rows, budgets)
        srcs, slots = [int(j) for j in srcs], [int(j) for j in slots]
        if len(srcs) != len(pages) or any(not 0 <= j < self.B for j in srcs):
            raise KarantaHipError(f"srcs {srcs} do not name one slot below {self.B} per page")
        for p, j in zip(pages, srcs):
            if self._slot_plen[j] < 1 or self._slot_plen[j] != len(p.input_ids):
                raise KarantaHipError(f"slot {j} holds a prompt of {self._slot_plen[j]} tokens, the page has {len(p.input_ids)}")
        adm = self._prefill_prepare(pages, None, slots, budgets, rows)
        src_of = [j for p, j in zip(pages, srcs) for _ in range(int(getattr(p, "n", 1)))]
        if any(j != sj and j in srcs for j, sj in zip(slots, src_of)):
            raise KarantaHipError(f"slots {slots}: a destination is another page's source {srcs}")
        if len(set(srcs)) != len(srcs):
            raise KarantaHipError(f"srcs {srcs}: one call reuses a slot once (give the page n > 1)")
        groups = [(sj, len(p.input_ids), [j for j, s2 in zip(slots, src_of) if s2 == sj and j != sj]) for p, sj in zip(pages, srcs)]
        groups = [g for g in groups if g[2]]
        adm.need = self._admit_features(rows)
        with torch.cuda.stream(self.stream):
            self.sampler._sampler_rows(adm, rows)
            self._fork(groups)
            self._activate(adm, src_of=src_of)
        self.sequences_reused += len(rows)
        return adm.lens

    def _check_budgets(self, pages, budgets):
        room = self.seq_room()
        for i, p in enumerate(pages):
            bud = int(budgets[i]) if budgets is not None else self._req_max_new
            if len(p.input_ids) + bud > room:
                raise KarantaHipError(f"prompt {len(p.input_ids)} + max_new_tokens {bud} exceeds s_max {room}")

    # Overlapped admission (optional, SlotScheduler(overlap=True); measured: no gain on the ragged serving benchmark —
    # 6.56 vs 6.57 pages/s, with or without a high-priority decode stream: the ViT / prefill launches fill all 256 CUs
    # with long-running workgroups and the short decode launches wait for slots, so the two streams serialise in
    # practice).  ViT + prefill of the new requests run on a second stream while the decode graph keeps
    # stepping the other slots.  The target slots are first PARKED on the last cache row (their frozen per-step KV
    # write then cannot land inside the rows the prefill is filling); the slot state and the first sampling step are
    # applied on the decode stream once the admission stream has finished.
    def admit_begin(self, pages: Sequence[PageRequest], slots: Sequence[int], budgets: Optional[Sequence[int]] = None):
        rows = children(pages)
        self._check_budgets(rows, budgets)
        slots = [int(j) for j in slots]
        if self._adm_stream is None:
            if self.admission_cus > 0:
                h = C.c_void_p()
                self.L.kr_stream_create_cu_mask(C.byref(h), int(self.admission_cus))
                self._adm_stream_handle = h
                self._adm_stream = torch.cuda.ExternalStream(h.value, device=self.device)
            else:
                self._adm_stream = torch.cuda.Stream(device=self.device)
        park = np.asarray([self.s_max - 1], np.int32)
        with torch.cuda.stream(self.stream):
            for j in slots:
                self.d_fin[j:j + 1].fill_(1)
                self._h2d(self.d_ctx[j:j + 1], park)
                self._h2d(self.d_plen[j:j + 1], park)
            parked = torch.cuda.Event()
            parked.record(self.stream)
        self._adm_stream.wait_event(parked)
        main = (self.stream, self.s)
        self.stream, self.s = self._adm_stream, self._adm_stream.cuda_stream
        try:
            adm = self._vit_and_prepare(pages, None, slots, budgets, rows)
            rec = self.prefill(pages, adm.n_img, slots=slots, defer_activation=True, adm=adm)
            done = torch.cuda.Event()
            done.record(self._adm_stream)
        finally:
            self.stream, self.s = main
        self._adm_inflight += 1
        return {"done": done, "rec": rec}

    def admit_ready(self, handle) -> bool:
        return bool(handle["done"].query())

    def admit_end(self, handle) -> List[int]:
        """Activate the admitted slots on the decode stream (waits for the admission stream there, not on the host)."""
        rec: Admission = handle["rec"]
        self._adm_inflight = max(0, self._adm_inflight - 1)
        self.stream.wait_event(handle["done"])
        # the first tokens are sampled with the passes this admission needs, whatever set_step_features did since admit_begin
        self._step |= rec.need
        with torch.cuda.stream(self.stream):
            self._fork(rec.forks)         # on the decode stream: never beside the decode graph
            self._activate(rec)
        return rec.lens

    def set_step_features(self, sampling: bool, guided: bool, processing: bool = False, adjust: bool = False,
                          repetition: bool = False):
        """Slot mode: which passes the NEXT decode steps carry, within what begin_slots() allowed.  The scheduler calls it with what
        the requests in the slots need: a server that accepts guided / sampled requests runs the plain argmax graph (no f32 logits
        written and re-read, no DFA advance) while none is decoding — rows with temperature 0 and no guide get the same token from
        either graph.  An admission switches on what its pages need by itself (prefill, admit_end).
        processing: the sampling-control launches (top_k / top_p / min_p / penalties; needs_processing), same rules.
        adjust: the logit-adjustment launches (logit_bias / min_tokens / stop_token_ids; needs_adjust), same rules.
        repetition: the repetition pass (PageRequest.repetition), same rules."""
        self._step = StepFeatures(bool(sampling), bool(guided), bool(processing), bool(adjust), bool(repetition)) & self._caps

    def decode_steps(self, n: int, speculative: bool = False):
        """n decode steps over all slots (asynchronous on the engine's stream).  speculative=True: speculative steps (every slot
        advances by 1 .. K + 1 tokens per step, the same tokens as plain steps give); raises where the steps carry guided decoding
        (without SpecConfig(guided=True)), sampling controls or logit adjustments (without SpecConfig(controls=True)), or record
        log-probabilities (without SpecConfig(logprobs=True)).  While an admission is in flight on a CU-masked stream the captured graph replays on the complementary compute units (same kernels, same grids: the same tokens), ordered
        against the engine's stream by events on both sides."""
        spec = bool(speculative)
        if spec:
            why = self._spec_refusal()
            if why is not None:
                raise KarantaHipError("decode_steps(speculative=True): " + why)
            self.spec_steps += n
        else:
            self.plain_steps += n
        graph = self._graphs.get(self._graph_key(self.B, spec))
        self.last_decode_disjoint = False      # (observable for tests: which of the two paths the call took)
        if (graph is not None and self._adm_inflight > 0 and self.admission_cus > 0 and self.disjoint_decode
                and self.admission_cus < self.n_cus):
            self.last_decode_disjoint = True
            if self._dec_stream is None:
                h = C.c_void_p()
                self.L.kr_stream_create_cu_range(C.byref(h), int(self.admission_cus), int(self.n_cus - self.admission_cus))
                self._dec_stream_handle = h
                self._dec_stream = torch.cuda.ExternalStream(h.value, device=self.device)
            before = torch.cuda.Event()
            before.record(self.stream)
            self._dec_stream.wait_event(before)
            for _ in range(n):
                self.L.kr_graph_launch(graph, self._dec_stream.cuda_stream)
            after = torch.cuda.Event()
            after.record(self._dec_stream)
            self.stream.wait_event(after)
            return
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                graph = self._graphs.get(self._graph_key(self.B, spec))
                if graph is not None:
                    self.L.kr_graph_launch(graph, self.s)
                else:  # first step eager (kernel attributes), then captured
                    self._spec_step_launches() if spec else self._decode_step_launches(self.B)
                    self._graph_for(self.B, spec)

    def poll_slots(self):
        """(finished[B], generated[B]): device EOS flags and tokens generated so far per slot (synchronises)."""
        self.stream.synchronize()
        self._snap_event = self._snap_counts = None
        fin = self.d_fin.cpu().numpy().astype(bool)
        gen = (self.d_ctx.cpu().numpy() + 1 - self.d_plen.cpu().numpy()).astype(np.int64)
        self._rep_read = (self.sampler.d_rep_at.cpu().numpy().astype(np.int64) if self.sampler._rep_slots
                          else np.full(self.B, -1, np.int64))
        return fin, gen

    def slot_rep_at(self) -> np.ndarray:
        """Per slot the generated-token index its sequence repeats at (kr_repeat_detect; -1: none), as of the flags the host last
        read with poll_slots() / read_snapshot()."""
        return self._rep_read

    # poll_slots without draining the stream (SlotScheduler launch-ahead): the slot state as of THIS point of the engine's stream is
    # copied to pinned host memory behind an event; the scheduler queues the next decode chunk before it waits for that event, so
    # the GPU has work while the host harvests finished slots and prepares the next admission.
    def snapshot_slots(self):
        ring = self._snap_ring
        if ring is None:
            ring = self._snap_ring = [torch.empty(6 if self.spec is not None else 4, self.B, dtype=torch.int32).pin_memory()
                                      for _ in range(4)]      # the last row: rep_at, beside the finished flags it explains
        buf = ring[self._snap_next % len(ring)]
        self._snap_next += 1
        with torch.cuda.stream(self.stream):
            buf[0].copy_(self.d_fin, non_blocking=True)
            buf[1].copy_(self.d_ctx, non_blocking=True)
            buf[2].copy_(self.d_plen, non_blocking=True)
            if self.spec is not None:     # proposed / accepted drafts per slot as of this point: snap["buf"][3], [4]
                buf[3:5].copy_(self.speculator.d_spec_count, non_blocking=True)
            if self.sampler._rep_slots:   # (no slot carries the feature: no copy is queued)
                buf[-1].copy_(self.sampler.d_rep_at, non_blocking=True)
            else:
                buf[-1].fill_(-1)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return {"buf": buf, "event": ev}

    def read_snapshot(self, snap):
        """(finished[B], generated[B]) of a snapshot_slots() handle; waits for that point of the stream only.  Later slot_tokens /
        slot_logprobs reads run on a side stream ordered after the same point (history rows are append-only)."""
        snap["event"].synchronize()
        a = snap["buf"].numpy()
        fin = a[0].astype(bool)
        gen = (a[1].astype(np.int64) + 1 - a[2])
        self._snap_event = snap["event"]
        self._snap_counts = (a[3].astype(np.int64), a[4].astype(np.int64)) if a.shape[0] >= 6 else None
        self._rep_read = a[-1].astype(np.int64)
        return fin, gen

    def _host_copy(self, t: "torch.Tensor") -> np.ndarray:
        """Device -> host of a slot's history.  After read_snapshot(): on the copy stream, behind the snapshot's event, so that the
        read does not wait for the decode chunk already queued on the engine's stream."""
        if self._snap_event is None:
            return t.cpu().numpy()
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        self._copy_stream.wait_event(self._snap_event)
        with torch.cuda.stream(self._copy_stream):
            return t.cpu().numpy()

    def slot_tokens(self, slot: int, n: int) -> np.ndarray:
        return self._host_copy(self.d_hist[:n, slot]).astype(np.int64)

    def slot_logprobs(self, slot: int, n: int, k: int) -> Dict[str, np.ndarray]:
        """Log-probabilities of the first n generated tokens of a slot (begin_slots(logprobs=...))."""
        if self.sampler.d_lp is None or self._logprobs is None:
            raise KarantaHipError("log-probabilities were not recorded: begin_slots(logprobs=k)")
        k = min(int(k), int(self._logprobs))
        lp = self._host_copy(self.sampler.d_lp[:n, slot])
        return {"token": lp[:, 0].copy(), "top": lp[:, 1:1 + k].copy(),
                "top_ids": self._host_copy(self.sampler.d_lpi[:n, slot, :k]).astype(np.int64)}

    def retire(self, slot: int):
        """Host-side stop (length limit): the slot idles from the next step on."""
        with torch.cuda.stream(self.stream):
            self.d_fin[slot:slot + 1].fill_(1)

    def close(self):
        for g in self._graphs.values():
            self.L.kr_graph_destroy(g)
        self._graphs.clear()
        if self._adm_stream_handle is not None:
            torch.cuda.synchronize(self.device)
            self._adm_stream = None
            self.L.kr_stream_destroy(self._adm_stream_handle)
            self._adm_stream_handle = None
        if self._dec_stream_handle is not None:
            torch.cuda.synchronize(self.device)
            self._dec_stream = None
            self.L.kr_stream_destroy(self._dec_stream_handle)
            self._dec_stream_handle = None
