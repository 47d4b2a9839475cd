"""vLLM's sampling controls on a page: top_k, top_p, min_p and the repetition / frequency / presence penalties.

Host side only (no torch): the kr_sample_threshold params row of a page, whether a page uses any control, which passes the
decode steps of a set of pages carry (StepFeatures: Engine._lm_head_and_sample, SlotScheduler), and the request validation of
the server, which follows vLLM's SamplingParams checks.  The device semantics are documented in include/karanta_hip.h and DESIGN.md §5c.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, NamedTuple

import numpy as np

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


class StepFeatures(NamedTuple):
    """The optional passes of a decode step (part of Engine's graph key): `sampling` the Gumbel-max argmax, `guided` its
    guide mask and the DFA advance, `processing` the sampling-control launches.  A guided row is masked in the sampling
    pass, so `guided` implies `sampling`."""
    sampling: bool = False
    guided: bool = False
    processing: bool = False

    @classmethod
    def of(cls, pages: Iterable) -> "StepFeatures":
        """What a set of pages needs; the one place that decides it."""
        pages = list(pages)
        guided = any(getattr(p, "guide", None) is not None for p in pages)
        return cls(guided or any(temperature(p) > 0 for p in pages), guided, any(needs_processing(p) for p in pages))

    def __or__(self, other: "StepFeatures") -> "StepFeatures":
        return StepFeatures(*(a or b for a, b in zip(self, other)))

    def __and__(self, caps: "StepFeatures") -> "StepFeatures":
        """The clamp to what `caps` allows; a guided row that stays guided keeps the sampling pass it is masked in."""
        guided = self.guided and caps.guided
        return StepFeatures((self.sampling and caps.sampling) or guided, guided, self.processing and caps.processing)


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
