"""What a caller hands to the engine and gets back: plain data, importable without torch or the HIP library."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ._lib import KarantaHipError


REP_MAX_PERIOD = 1024      # KR_REP_MAX_PERIOD (include/karanta_hip.h)


@dataclass(frozen=True)
class RepetitionParams:
    """vLLM's repetition_detection: the sequence ends ("length", stop_reason "repetition") at the first generated token after which
    the last min_count x p tokens are min_count copies of one block of p tokens, min_pattern_size <= p <= max_pattern_size, and the
    repeated stretch is at least min_span tokens long (0: no such floor; it keeps dot leaders and table rules out without raising
    min_count for long blocks).  The rule reads the output alone (kr_repeat_detect, include/karanta_hip.h).  No field has a
    default: which values suit real pages is unmeasured."""
    max_pattern_size: int
    min_pattern_size: int
    min_count: int
    min_span: int = 0

    def __post_init__(self):
        for name in ("max_pattern_size", "min_pattern_size", "min_count", "min_span"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"repetition_detection: {name} must be an integer, got {v!r}")
        a, b, c, m = self.row()
        if not 1 <= a <= b:
            raise ValueError(f"repetition_detection: 1 <= min_pattern_size ({a}) <= max_pattern_size ({b}) must hold")
        if b > REP_MAX_PERIOD:
            raise ValueError(f"repetition_detection: max_pattern_size {b} is above {REP_MAX_PERIOD}")
        if c < 2:
            raise ValueError(f"repetition_detection: min_count must be at least 2, got {c}")
        if m < 0:
            raise ValueError(f"repetition_detection: min_span must not be negative, got {m}")
        if max(c, m) > 0x7FFFFFFF:      # the device row is int32
            raise ValueError("repetition_detection: min_count and min_span must fit 31 bits")

    def row(self):
        """The kr_repeat cfg row: (a, b, c, m)."""
        return int(self.min_pattern_size), int(self.max_pattern_size), int(self.min_count), int(self.min_span)


@dataclass
class PageRequest:
    """One page = one sequence: prompt token ids (image placeholders included) + its images."""
    input_ids: np.ndarray                      # int64 [P]
    pixel_values: Optional[np.ndarray] = None  # fp32 [n_patches, 1176] (all images concatenated)
    grids: List[Tuple[int, int, int]] = field(default_factory=list)
    temperature: float = 0.0                   # 0: greedy; > 0: Gumbel-max sampling (kr_gumbel_argmax)
    seed: int = 0                              # the sampler is counter-based: (seed, token index) fixes every draw
    images: Optional[List[Any]] = None         # instead of pixel_values: HWC uint8 RGB pages for the GPU front end
    #                                            (numpy arrays, or torch uint8 tensors already resident in HBM)
    guide: Any = None                          # guided.Guide / DeviceGuide: the output must match this pattern
    logprobs: Optional[int] = None             # None: off; k >= 0: log-prob of every token + the k most probable (<= 20)
    # vLLM's sampling controls (kr_sample_threshold / kr_gumbel_argmax_processed); the defaults are "off"
    top_k: int = 0                             # 0 or -1: off; k: keep the k largest scores (ties kept)
    top_p: float = 1.0                         # 1: off; keep the smallest top set whose probability reaches top_p
    min_p: float = 0.0                         # 0: off; keep p_i >= min_p * p_max
    repetition_penalty: float = 1.0            # 1: off; tokens of the prompt or the output so far: l > 0 ? l / r : l * r
    frequency_penalty: float = 0.0             # l -= frequency_penalty * (count in the output so far)
    presence_penalty: float = 0.0              # l -= presence_penalty * (count > 0)
    # vLLM's logit adjustments (kr_logits_adjust / kr_stop_tokens), applied before the penalties; the defaults are "off"
    logit_bias: Optional[Dict[int, float]] = None   # token id -> value added to its logit (fp32)
    min_tokens: int = 0                        # while fewer tokens are generated, EOS and the stop_token_ids cannot be chosen
    stop_token_ids: Tuple[int, ...] = ()       # a generated token among these ends the sequence as EOS does
    # parallel sampling (OpenAI's n): the page starts n sequences, exactly what n copies of it with seeds (seed + c) & 0xFFFFFFFF,
    # c = 0..n-1, start (vLLM's seeds for the children of a seeded request) — but its images go through the ViT once and its
    # prompt through the prefill once; the siblings' KV rows are copies of child 0's (kr_kv_fork)
    n: int = 1
    # runaway repetition (kr_repeat_detect): None = off.  It changes no token choice, only where the sequence ends
    repetition: Optional[RepetitionParams] = None


def children(pages) -> list:
    """The sequences a batch of pages starts, page-major with a page's children consecutive: the page itself for n = 1, else n
    copies with n = 1 and seeds (seed + c) & 0xFFFFFFFF.  This is the row order of every per-sequence list of the engine."""
    rows = []
    for p in pages:
        n = getattr(p, "n", 1)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise KarantaHipError(f"PageRequest.n must be an integer >= 1, not {n!r}")
        if n == 1:
            rows.append(p)
            continue
        for c in range(int(n)):
            ch = copy.copy(p)
            ch.n, ch.seed = 1, (int(getattr(p, "seed", 0) or 0) + c) & 0xFFFFFFFF
            rows.append(ch)
    return rows


@dataclass
class GenerateResult:
    """Per-sequence lists hold sum(n) entries: page-major, a page's n children consecutive (`children`)."""
    tokens: List[np.ndarray]          # per sequence: generated ids (EOS included, nothing after it)
    finish_reasons: List[str]         # "stop" | "length"
    prompt_tokens: List[int]
    timings: Dict[str, float]
    logits: Optional[np.ndarray] = None  # [B, steps, V] when return_logits
    logprobs: Optional[List[Optional[Dict[str, np.ndarray]]]] = None   # per page (None where not asked): "token" [n],
    #                                                                    "top_ids" [n, k], "top" [n, k]
    stop_reasons: Optional[List[Optional[str]]] = None   # per sequence: "repetition" where PageRequest.repetition ended it, else None


@dataclass(frozen=True)
class SpecConfig:
    """Prompt-lookup speculative decoding (vLLM's ngram method): per step and slot up to `num_tokens` draft tokens, copied from
    behind the latest earlier occurrence of the sequence's last ngram_max .. ngram_min tokens, are verified beside the slot's own
    row (kr_spec_propose / kr_spec_accept).  The tokens are those of the plain steps, whatever the temperature.
    share_rows: instead of num_tokens rows owned by every slot (max_batch x (num_tokens + 1) <= 32), the rows of a step that the slots
    do not take themselves are dealt per step to the slots whose lookup found drafts (kr_spec_lookup / kr_spec_deal /
    kr_spec_accept_rows): any max_batch up to 31.
    guided: steps that carry guided requests speculate too — the drafts of a guided slot are kept while its guide allows them and
    every draft row is masked with the DFA state behind its drafts (kr_spec_guide_trim / kr_spec_guide_rows /
    kr_spec_guide_advance).  Off, such steps are plain steps, as before the option existed.
    controls: steps that carry sampling controls (top_k, top_p, min_p, penalties) or logit adjustments (logit_bias, min_tokens,
    stop_token_ids) speculate too — a draft row runs the sampler's passes with its slot's parameters and the output counts behind
    its drafts, and a draft that is a stop entry of its slot ends the slot's drafts (kr_spec_controls_trim / kr_spec_controls_rows /
    kr_spec_controls_count, the _rows launches of the sampler).  Off, such steps are plain steps, as before the option existed.
    logprobs: steps that record log-probabilities (begin_slots(logprobs=k)) speculate too — every token a step emits gets the record
    the plain steps would have written, from the logits row that chose it (kr_spec_mark / kr_logits_restore_rows /
    kr_logprobs_topk_rows).  Off, such steps are plain steps, as before the option existed."""
    num_tokens: int = 3
    ngram_min: int = 2
    ngram_max: int = 4
    share_rows: bool = False
    guided: bool = False
    controls: bool = False
    logprobs: bool = False

    def rows(self, max_batch: int) -> int:
        """Rows of a speculative step: never fewer than 17 (the packed 17..32-row family)."""
        n = max(17, max_batch * (int(self.num_tokens) + 1))
        return min(32, n) if self.share_rows else n

    def check(self, max_batch: int):
        k = self.num_tokens
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise KarantaHipError(f"speculative: num_tokens {k!r} must be an integer >= 1")
        if not 1 <= int(self.ngram_min) <= int(self.ngram_max) <= 8:
            raise KarantaHipError(f"speculative: 1 <= ngram_min {self.ngram_min} <= ngram_max {self.ngram_max} <= 8")
        if not isinstance(self.guided, (bool, np.bool_)):
            raise KarantaHipError(f"speculative: guided {self.guided!r} must be True or False")
        if not isinstance(self.controls, (bool, np.bool_)):
            raise KarantaHipError(f"speculative: controls {self.controls!r} must be True or False")
        if not isinstance(self.logprobs, (bool, np.bool_)):
            raise KarantaHipError(f"speculative: logprobs {self.logprobs!r} must be True or False")
        if self.share_rows:
            if k > 31:
                raise KarantaHipError(f"speculative: num_tokens {k} > 31, the draft rows a 32-row decode step can hold")
            if not 1 <= max_batch <= 31:
                raise KarantaHipError(f"speculative: share_rows with max_batch {max_batch}: 1..31 slots — with 32 every row of a decode "
                                      "step is a slot's own, no row is spare for a draft")
        elif max_batch * (k + 1) > 32:
            raise KarantaHipError(f"speculative: max_batch {max_batch} x (num_tokens {k} + 1) = {max_batch * (k + 1)} rows > 32, the most "
                                  "one decode step takes")
