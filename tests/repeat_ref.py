"""Numpy / plain-Python restatement of repetition detection (include/karanta_hip.h, kr_repeat); not a test module.

`first_repeat` is the rule as the header words it, by comparing blocks: no run counters, no state.  `Incremental` is the state
machine the kernel keeps per slot (run counters per period, `seen`, `rep_at`) fed with tokens in chunks of any size.
test_repeat_cpu.py checks the two against each other; the GPU tests check the kernel and the engine against both."""
from typing import Optional, Sequence

import numpy as np

MAX_PERIOD = 1024


def repeats_at(y: Sequence[int], g: int, a: int, b: int, c: int, m: int) -> bool:
    """Whether y[0..g] repeats at g: for some p in [a, b] the last L = max(c p, m) tokens exist and each of them but the first p
    equals the token p places before it — the last c p tokens are c copies of one block, the repeated stretch is >= m tokens long."""
    for p in range(a, b + 1):
        L = max(c * p, m)
        if L < p + 1 or g + 1 < L:       # (c >= 2 makes L >= 2 p: at least one comparison)
            continue
        seg = list(y[g + 1 - L:g + 1])
        if seg[p:] == seg[:-p]:
            return True
    return False


def first_repeat(y: Sequence[int], a: int, b: int, c: int, m: int = 0) -> Optional[int]:
    """The smallest g at which y repeats, or None."""
    assert 1 <= a <= b <= MAX_PERIOD and c >= 2 and m >= 0
    for g in range(len(y)):
        if repeats_at(y, g, a, b, c, m):
            return g
    return None


def cut(y: Sequence[int], params, stop_ids=()) -> tuple:
    """(tokens kept, finish_reason, stop_reason) of an undetected output y under `params` = (a, b, c, m) or None: the first stop id
    ends it as "stop" unless the sequence repeats before it."""
    y = [int(t) for t in y]
    e = next((i for i, t in enumerate(y) if t in set(stop_ids)), None)
    g = first_repeat(y if e is None else y[:e + 1], *params) if params is not None else None
    if g is not None and (e is None or g < e):
        return y[:g + 1], "length", "repetition"
    if e is not None:
        return y[:e + 1], "stop", None
    return y, "length", None


class Incremental:
    """One slot's state as kr_repeat_detect keeps it.  run[p - 1] belongs to period p and only periods a..b are ever written; it is
    NOT cleared by `admit` (token 0 does that), as on the device."""

    def __init__(self, a: int, b: int, c: int, m: int = 0, run: Optional[np.ndarray] = None):
        self.cfg = (a, b, c, m)
        self.run = np.zeros(MAX_PERIOD, np.int32) if run is None else np.array(run, np.int32)
        self.y: list = []
        self.seen, self.rep_at = 0, -1

    def admit(self, a: int, b: int, c: int, m: int = 0):
        self.cfg, self.y, self.seen, self.rep_at = (a, b, c, m), [], 0, -1

    def feed(self, tokens: Sequence[int]) -> int:
        """Append tokens (one decode step's worth) and walk them; returns rep_at.  After a hit nothing changes any more."""
        if self.rep_at >= 0:
            return self.rep_at
        self.y += [int(t) for t in tokens]
        a, b, c, m = self.cfg
        y, run = self.y, self.run.tolist()
        for g in range(self.seen, len(y)):
            hit = False
            for p in range(a, b + 1):
                run[p - 1] = run[p - 1] + 1 if g >= p and y[g] == y[g - p] else 0
                hit = hit or run[p - 1] >= max((c - 1) * p, m - p)
            self.seen = g + 1
            if hit:
                self.rep_at = g
                break
        self.run = np.asarray(run, np.int32)
        return self.rep_at
