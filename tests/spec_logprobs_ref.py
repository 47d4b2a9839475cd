"""Numpy statement of which tokens of a speculative decode step record log-probabilities, on which row and at which history index
(include/karanta_hip.h: kr_spec_mark, kr_logprobs_topk_rows); not a test module.  test_spec_logprobs_cpu.py checks it against a
token-by-token simulation of plain steps, test_gpu_spec_logprobs_kernels.py runs the kernels against it.

Written from the rule: a plain step records the token it appended at that token's history index unless the token finished the
sequence; a speculative step emitted e = ctx_len - ctx_before tokens, token j chosen on the row of draft j (j = 0: the slot's own)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np


def row_of(slot: int, j: int, slots: int, k: int, draft_row: Optional[np.ndarray]) -> int:
    """The row token j of `slot` was chosen on: the slot's own for j = 0; else row j * slots + slot of the static layout
    (draft_row None) or the row kr_spec_deal dealt draft j (draft_row [slots, k]; -1: none)."""
    if j == 0:
        return int(slot)
    if draft_row is None:
        return j * slots + int(slot)
    return int(np.asarray(draft_row).reshape(slots, k)[slot, j - 1])


def records(ctx_before, ctx_len, prompt_len, finished, k: int, rows: int, hist_len: int, draft_row=None,
            hist_rows: Optional[int] = None) -> List[Tuple[int, int, int, int]]:
    """(slot, j, row, h) of every record one step writes, given the slots' ctx_len before and after the step, their prompt lengths
    and their finished flags after it.  The token that finished a slot records nothing; nothing is written for an h outside
    [0, hist_len) (or at or past the token history's hist_rows) or for a row outside [0, rows)."""
    slots = len(ctx_len)
    out = []
    for s in range(slots):
        e = max(0, min(k + 1, int(ctx_len[s]) - int(ctx_before[s])))
        n_rec = e - (1 if finished[s] else 0)
        for j in range(n_rec):
            row = row_of(s, j, slots, k, draft_row)
            h = int(ctx_before[s]) + 1 + j - int(prompt_len[s])
            if not 0 <= row < rows or not 0 <= h < hist_len or (hist_rows is not None and h >= hist_rows):
                continue
            out.append((s, j, row, h))
    return out


def plain_records(truth, start: int, gen: int, stops) -> List[int]:
    """The history indices one-token steps record while a sequence grows from `start` to `gen` generated tokens: every token but
    one that is an EOS or stop id (it finishes the sequence, and nothing follows it)."""
    return [h for h in range(start, gen) if truth[h] not in stops]
