"""vLLM's sampling controls on a page: top_k, top_p, min_p and the repetition / frequency / presence penalties, and its logit
adjustments: logit_bias, min_tokens, stop_token_ids (kr_logits_adjust / kr_stop_tokens) and the `stop` strings of a request.

Host side only (no torch): the kr_sample_threshold params row of a page, whether a page uses any control, which passes the
decode steps of a set of pages carry (StepFeatures: Engine._lm_head_and_sample, SlotScheduler), and the request validation of
the server, which follows vLLM's SamplingParams checks.  The device semantics are documented in include/karanta_hip.h and DESIGN.md §5c.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._lib import ADJ_CAP          # KR_ADJ_CAP (include/karanta_hip.h): entries of a row's logit-adjustment table
from .request import RepetitionParams

# request field -> neutral value ("off")
NEUTRAL = {"top_k": 0, "top_p": 1.0, "min_p": 0.0, "repetition_penalty": 1.0, "frequency_penalty": 0.0,
           "presence_penalty": 0.0}


def sampling_params(p) -> np.ndarray:
    """The kr_sample_threshold params row of a page: [top_k, top_p, min_p, repetition, frequency, presence, 0, 0] (fp32;
    top_k of 0 or -1 is stored as 0 = off)."""
    g = lambda name: NEUTRAL[name] if getattr(p, name, None) is None else float(getattr(p, name))
    k = g("top_k")
    return np.asarray([k if k > 0 else 0.0, g("top_p"), g("min_p"), g("repetition_penalty"), g("frequency_penalty"),
                       g("presence_penalty"), 0.0, 0.0], np.float32)


def has_penalties(p) -> bool:
    sp = sampling_params(p)
    return bool(sp[3] != 1.0 or sp[4] != 0.0 or sp[5] != 0.0)


def needs_processing(p) -> bool:
    """Whether a page uses any of the sampling controls."""
    sp = sampling_params(p)
    return bool(sp[0] > 0 or sp[1] != 1.0 or sp[2] != 0.0 or has_penalties(p))


def temperature(p) -> float:
    """A page's sampling temperature; None, missing or 0 all mean greedy (0.0)."""
    return float(getattr(p, "temperature", 0.0) or 0.0)


MAX_STOP = 16          # stop_token_ids / stop strings a request may carry
BIAS_CLAMP = 100.0     # logit_bias values are clamped to [-100, 100] (OpenAI / vLLM)


def needs_adjust(p) -> bool:
    """Whether a page carries a logit adjustment: a logit_bias, min_tokens > 0 or stop_token_ids."""
    return bool(getattr(p, "logit_bias", None)) or int(getattr(p, "min_tokens", 0) or 0) > 0 or \
        len(getattr(p, "stop_token_ids", None) or ()) > 0


def adjust_table(p, eos_token_ids: Sequence[int], vocab_size: int) -> Optional[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """The kr_logits_adjust table of a page, every id once: (ids int32 [n], values fp32 [n], flags int32 [n], meta int32 [4] =
    {n, min_tokens, 0, 0}); None for a page without adjustments.  Stop entries (flag bit 0) are the page's stop_token_ids and,
    while min_tokens is on, the model's EOS ids (EOS itself ends a row in kr_sample_greedy; min_tokens has to mask it).
    Raises ValueError for an id outside the vocabulary or a table above ADJ_CAP."""
    if not needs_adjust(p):
        return None
    entries: Dict[int, list] = {}
    for k, v in (getattr(p, "logit_bias", None) or {}).items():
        entries[int(k)] = [float(v), 0]
    m = int(getattr(p, "min_tokens", 0) or 0)
    stops = [int(t) for t in getattr(p, "stop_token_ids", None) or ()] + ([int(e) for e in eos_token_ids] if m > 0 else [])
    for t in stops:
        entries.setdefault(t, [0.0, 0])[1] = 1
    if len(entries) > ADJ_CAP:
        raise ValueError(f"logit_bias + stop_token_ids + EOS ids name {len(entries)} tokens, at most {ADJ_CAP} fit")
    ids = np.fromiter(entries, np.int64, len(entries))
    if ids.size and (ids.min() < 0 or ids.max() >= vocab_size):
        raise ValueError(f"logit_bias / stop_token_ids: token id outside the vocabulary [0, {vocab_size})")
    vals = np.asarray([e[0] for e in entries.values()], np.float32)
    flags = np.asarray([e[1] for e in entries.values()], np.int32)
    return ids.astype(np.int32), vals, flags, np.asarray([len(entries), m, 0, 0], np.int32)


class _LogitPasses(NamedTuple):
    sampling: bool = False
    guided: bool = False
    processing: bool = False
    adjust: bool = False


class StepFeatures(_LogitPasses):
    """The optional passes of a decode step (part of Engine's graph key): `sampling` the Gumbel-max argmax, `guided` its
    guide mask and the DFA advance, `processing` the sampling-control launches, `adjust` the logit-adjustment launches
    (kr_logits_adjust / kr_stop_tokens / kr_logits_restore).  A guided row is masked in the sampling pass and an adjusted
    row's token is the argmax of that pass over the adjusted logits, so `guided` and `adjust` imply `sampling`.
    Those four work on the logits and are the tuple.  `repetition`, the repetition pass behind the token choice
    (kr_repeat_detect), touches no logit and implies nothing: it rides beside the tuple as an attribute, and equality and the hash
    (the graph key) take it in."""

    def __new__(cls, sampling: bool = False, guided: bool = False, processing: bool = False, adjust: bool = False,
                repetition: bool = False):
        self = super().__new__(cls, sampling, guided, processing, adjust)
        self.repetition = bool(repetition)
        return self

    def __eq__(self, other):
        same = tuple.__eq__(self, other)
        return same if same is NotImplemented else same and self.repetition == bool(getattr(other, "repetition", False))

    def __ne__(self, other):
        same = self.__eq__(other)
        return same if same is NotImplemented else not same

    def __hash__(self):
        return hash((tuple(self), self.repetition))

    def __repr__(self):
        return super().__repr__()[:-1] + f", repetition={self.repetition})"

    @classmethod
    def of(cls, pages: Iterable) -> "StepFeatures":
        """What a set of pages needs; the one place that decides it."""
        pages = list(pages)
        guided = any(getattr(p, "guide", None) is not None for p in pages)
        adjust = any(needs_adjust(p) for p in pages)
        return cls(guided or adjust or any(temperature(p) > 0 for p in pages), guided, any(needs_processing(p) for p in pages),
                   adjust, any(getattr(p, "repetition", None) is not None for p in pages))

    def __or__(self, other: "StepFeatures") -> "StepFeatures":
        return StepFeatures(*(a or b for a, b in zip(self, other)), repetition=self.repetition or other.repetition)

    def __and__(self, caps: "StepFeatures") -> "StepFeatures":
        """The clamp to what `caps` allows; a guided or adjusted row that stays so keeps the sampling pass it needs."""
        guided = self.guided and caps.guided
        adjust = self.adjust and caps.adjust
        return StepFeatures((self.sampling and caps.sampling) or guided or adjust, guided, self.processing and caps.processing,
                            adjust, self.repetition and caps.repetition)


def spec_refusal(spec, step: StepFeatures, slot_mode: bool, recording: bool) -> Optional[str]:
    """Why the steps that carry `step` cannot be speculative on an engine built with the SpecConfig `spec` (None: without one), in slot
    mode or not, recording log-probabilities or not; None: they can.  A draft row sees the logits of its own position only: the
    passes that carry state from token to token (the penalties' counts, min_tokens) or record per step (log-probabilities)
    would need that state per draft.  A guide's DFA state is had per draft (kr_spec_guide_*) where the engine was built with
    SpecConfig(guided=True), the sampler's counts and stop entries (kr_spec_controls_*, the _rows launches) where it was built
    with SpecConfig(controls=True), a record per emitted token (kr_logprobs_topk_rows) where it was built with
    SpecConfig(logprobs=True)."""
    if spec is None:
        return "the engine was built without speculative=SpecConfig(...)"
    if not slot_mode:
        return "speculative steps run in slot mode (begin_slots)"
    controlled = (step.processing or step.adjust) and not spec.controls
    if spec.guided:
        if controlled:
            return "the step carries sampling controls or logit adjustments"
    elif step.guided or controlled:
        return ("the step carries guided decoding, sampling controls or logit adjustments"
                + (" (guided requests speculate on an engine built with SpecConfig(guided=True))" if step.guided else ""))
    if recording and not spec.logprobs:
        return "log-probabilities are recorded"
    return None


REPETITION_KEYS = ("max_pattern_size", "min_pattern_size", "min_count", "min_span")


def parse_repetition_field(v: Any) -> Optional[RepetitionParams]:
    """`repetition_detection` of a request body, the server's --repetition-detection or LocalServer(repetition=...): an object
    with max_pattern_size, min_pattern_size, min_count and (optional, 0) min_span, all integers; None or False: off.  Raises
    ValueError with the message for the 400 answer: non-integers, a > b, b > 1024, c < 2, m < 0, unknown or missing keys."""
    if v is None or v is False:
        return None
    if isinstance(v, RepetitionParams):
        return v
    if not isinstance(v, dict):
        raise ValueError(f"repetition_detection must be an object, false or null, got {type(v).__name__}")
    unknown = sorted(k for k in v if k not in REPETITION_KEYS)
    if unknown:
        raise ValueError(f"repetition_detection: unknown key(s) {', '.join(map(repr, unknown))} (known: {', '.join(REPETITION_KEYS)})")
    missing = [k for k in REPETITION_KEYS[:3] if v.get(k) is None]
    if missing:
        raise ValueError(f"repetition_detection: {', '.join(missing)} must be given (the server ships no defaults)")
    kw = {k: _int_field(f"repetition_detection.{k}", v[k]) for k in REPETITION_KEYS if v.get(k) is not None}
    return RepetitionParams(**kw)


def parse_request_fields(req: Dict[str, Any]) -> Dict[str, Any]:
    """The six fields of an OpenAI / vLLM request body, validated as vLLM does; absent or null fields take the neutral
    value.  Raises ValueError with the message for the 400 answer."""
    out: Dict[str, Any] = {}
    for name, neutral in NEUTRAL.items():
        v = req.get(name)
        if v is None:
            out[name] = neutral
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name} must be a number, got {v!r}")
        if not math.isfinite(float(v)):
            raise ValueError(f"{name} must be finite, got {v!r}")
        if name == "top_k":
            if float(v) != int(v):
                raise ValueError(f"top_k must be an integer, got {v!r}")
            v = int(v)
            if v < -1:
                raise ValueError(f"top_k must be -1 (disable) or at least 1, got {v}")
            out[name] = 0 if v == -1 else v
            continue
        v = float(v)
        if name == "top_p" and not 0.0 < v <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {v}")
        if name == "min_p" and not 0.0 <= v <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {v}")
        if name == "repetition_penalty" and not v > 0.0:
            raise ValueError(f"repetition_penalty must be greater than zero, got {v}")
        if name in ("frequency_penalty", "presence_penalty") and not -2.0 <= v <= 2.0:
            raise ValueError(f"{name} must be in [-2, 2], got {v}")
        out[name] = v
    return out


def _int_field(name: str, v: Any) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)) or float(v) != int(v):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def parse_adjust_fields(req: Dict[str, Any], vocab_size: int, max_tokens: int, guided: bool = False,
                        eos_token_ids: Sequence[int] = ()) -> Dict[str, Any]:
    """`logit_bias`, `min_tokens`, `stop_token_ids`, `stop` and `include_stop_str_in_output` of an OpenAI / vLLM request body,
    validated as vLLM's OpenAI layer does; absent or null fields are off.  `guided`: the request carries a guide;
    `eos_token_ids`: the model's, which share the device table with the bias keys and stop ids while min_tokens is on.
    Raises ValueError with the message for the 400 answer."""
    out: Dict[str, Any] = {"logit_bias": None, "min_tokens": 0, "stop_token_ids": (), "stop": (),
                           "include_stop_str_in_output": False}
    lb = req.get("logit_bias")
    if lb is not None:
        if not isinstance(lb, dict):
            raise ValueError(f"logit_bias must be an object of token id -> bias, got {type(lb).__name__}")
        bias: Dict[int, float] = {}
        for k, v in lb.items():
            try:
                if isinstance(k, bool) or not isinstance(k, (int, str)):
                    raise ValueError
                tid = int(k)
            except ValueError:
                raise ValueError(f"logit_bias key {k!r} is not an integer token id") from None
            if not 0 <= tid < vocab_size:
                raise ValueError(f"logit_bias token id {tid} is outside the vocabulary [0, {vocab_size})")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
                raise ValueError(f"logit_bias value of token {tid} must be a finite number, got {v!r}")
            bias[tid] = min(BIAS_CLAMP, max(-BIAS_CLAMP, float(v)))
        out["logit_bias"] = bias or None
    mt = req.get("min_tokens")
    if mt is not None:
        m = _int_field("min_tokens", mt)
        if not 0 <= m <= int(max_tokens):
            raise ValueError(f"min_tokens must be in [0, max_tokens = {int(max_tokens)}], got {m}")
        if m > 0 and guided:
            raise ValueError("min_tokens > 0 cannot be combined with guided decoding: a guide state that allows only EOS "
                             "would leave no token")
        out["min_tokens"] = m
    st = req.get("stop_token_ids")
    if st is not None:
        if not isinstance(st, (list, tuple)):
            raise ValueError("stop_token_ids must be a list of token ids")
        if len(st) > MAX_STOP:
            raise ValueError(f"stop_token_ids holds {len(st)} ids, at most {MAX_STOP} are served")
        ids = tuple(_int_field("stop_token_ids entry", t) for t in st)
        if any(not 0 <= t < vocab_size for t in ids):
            raise ValueError(f"stop_token_ids: token id outside the vocabulary [0, {vocab_size})")
        out["stop_token_ids"] = ids
    sp = req.get("stop")
    if sp is not None:
        stops = [sp] if isinstance(sp, str) else sp
        if not isinstance(stops, (list, tuple)) or any(not isinstance(x, str) for x in stops):
            raise ValueError("stop must be a string or a list of strings")
        if len(stops) > MAX_STOP:
            raise ValueError(f"stop holds {len(stops)} strings, at most {MAX_STOP} are served")
        if any(x == "" for x in stops):
            raise ValueError("stop strings must not be empty")
        out["stop"] = tuple(stops)
    inc = req.get("include_stop_str_in_output")
    if inc is not None:
        if not isinstance(inc, bool):
            raise ValueError(f"include_stop_str_in_output must be a boolean, got {inc!r}")
        out["include_stop_str_in_output"] = inc
    n = len(set(out["logit_bias"] or ()) | set(out["stop_token_ids"]) | (set(int(e) for e in eos_token_ids) if out["min_tokens"] else set()))
    if n > ADJ_CAP:
        raise ValueError(f"logit_bias + stop_token_ids name {n} tokens, at most {ADJ_CAP} are served")
    return out


class StopStrings:
    """The `stop` strings of one request against its growing token list.  `check(tokens)` returns the number of tokens to keep
    — through the token that completed the earliest match (by start position; ties: the string listed first) — or None;
    after a match `text` is the message content: cut before the match, or after it with `include`.  Matches on bytes where
    the tokenizer gives every token's byte string (`token_bytes`: a stop string may end inside a token and span several),
    on `decode` otherwise.  Incremental: a call only scans what the tokens added since the last one can have completed."""

    def __init__(self, stops: Sequence[str], include: bool = False, token_bytes: Optional[Sequence[bytes]] = None, decode=None):
        if token_bytes is None and decode is None:
            raise ValueError("StopStrings needs token_bytes or decode")
        self.stops = [s.encode("utf-8") for s in stops] if token_bytes is not None else list(stops)
        self.include, self._tb, self._decode = bool(include), token_bytes, decode
        self._seen: list = []
        self._buf = b"" if token_bytes is not None else ""
        self._ends: list = []            # length of _buf after each token
        self.keep: Optional[int] = None
        self.text: Optional[str] = None

    def check(self, tokens) -> Optional[int]:
        toks = [int(t) for t in tokens]
        if self.keep is not None and toks[:self.keep] == self._seen[:self.keep]:
            return self.keep
        if toks[:len(self._seen)] != self._seen:       # not a continuation: start over
            self._seen, self._ends, self._buf, self.keep, self.text = [], [], self._buf[:0], None, None
        old = len(self._buf)
        for t in toks[len(self._seen):]:
            self._seen.append(t)
            if self._tb is not None:
                self._buf += self._tb[t] if 0 <= t < len(self._tb) else b""
            else:
                self._buf = self._decode(self._seen)
            self._ends.append(len(self._buf))
        best = None
        for s in self.stops:
            at = self._buf.find(s, max(0, old - len(s) + 1) if self._tb is not None else 0)   # decode may rewrite its tail
            if at >= 0 and (best is None or at < best[0]):
                best = (at, at + len(s))
        if best is None:
            return None
        self.keep = next(i for i, e in enumerate(self._ends) if e >= best[1]) + 1
        cut = self._buf[:best[1] if self.include else best[0]]
        self.text = cut.decode("utf-8", "replace") if isinstance(cut, bytes) else cut
        return self.keep

    __call__ = check
