"""Numpy restatement of a speculative decode step with shared rows (include/karanta_hip.h: kr_spec_lookup, kr_spec_deal,
kr_spec_accept_rows); not a test module.  test_spec_deal_cpu.py checks it on hand-worked cases, test_gpu_spec_deal.py runs the kernels
and the engine against it.

Written from the rule, not from the kernel: the dealing below is the literal loop "for depth, for slot, take the next free row"."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import spec_ref as R


def lookup(prompts, hist, ctx, plen, fin, k, n_min, n_max, s_max, pad_id, vocab, scripts=None) -> Tuple[np.ndarray, np.ndarray]:
    """What kr_spec_lookup writes: (n_want [B], draft_tok [B, k]) — kr_spec_propose's n_draft and draft_tok, nothing else."""
    B = len(ctx)
    z = np.zeros(B)
    out = R.propose(prompts, hist, ctx, plen, fin, z, z, k, B * (k + 1), n_min, n_max, s_max, pad_id, vocab, scripts=scripts)
    return out["n_draft"], out["draft_tok"]


def deal_rows(n_want: Sequence[int], live: Sequence[bool], k: int, rows: int) -> np.ndarray:
    """draft_row [B, k]: rows B .. rows - 1 breadth first — for depth j = 1..k, for the slots in ascending order, a live slot with
    n_want >= j takes the next free row until none is left; -1 where the draft got none."""
    B = len(n_want)
    out = np.full((B, k), -1, np.int32)
    free = B
    for j in range(1, k + 1):
        for b in range(B):
            if live[b] and n_want[b] >= j and free < rows:
                out[b, j - 1] = free
                free += 1
    return out


def deal(n_want, draft_tok, ctx, plen, fin, temp, seed, k, rows, s_max, pad_id):
    """What kr_spec_deal writes.  ctx / plen / fin / temp / seed [B]: the slots' entries of the row arrays.  Returns a dict: n_draft
    [B], draft_row [B, k] and the row arrays [rows] (slot, ctx, plen, fin, temp, seed, tok) with the slots' own entries in front as
    given (tok = -1 there: the kernel does not write x of a slot's own row).  A row nobody was dealt is parked: slot 0, position
    s_max - 1, finished, the pad token."""
    B = len(ctx)
    out = {"slot": np.zeros(rows, np.int32), "ctx": np.full(rows, s_max - 1, np.int32), "plen": np.full(rows, s_max - 1, np.int32),
           "fin": np.ones(rows, np.int32), "temp": np.zeros(rows, np.float32), "seed": np.zeros(rows, np.uint32),
           "tok": np.full(rows, pad_id, np.int64)}
    out["slot"][:B] = np.arange(B)
    out["tok"][:B] = -1
    for name, src in (("ctx", ctx), ("plen", plen), ("fin", fin), ("temp", temp), ("seed", seed)):
        out[name][:B] = src
    out["draft_row"] = deal_rows(n_want, [not f for f in fin], k, rows)
    out["n_draft"] = (out["draft_row"] >= 0).sum(axis=1).astype(np.int32)
    for b in range(B):
        for j in range(1, k + 1):
            r = int(out["draft_row"][b, j - 1])
            if r < 0:
                continue
            out["slot"][r], out["plen"][r], out["temp"][r], out["seed"][r], out["fin"][r] = b, plen[b], temp[b], seed[b], 0
            out["ctx"][r] = min(int(ctx[b]) + j, s_max - 1)
            out["tok"][r] = int(draft_tok[b, j - 1])
    return out


def static_partials(amax_val: np.ndarray, amax_idx: np.ndarray, draft_row: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The partials [rows, n_part] of a shared-rows step in kr_spec_accept's static layout [B * (k + 1), n_part]: row j * B + b is
    the row draft j of slot b was dealt (zeros where it got none: kr_spec_accept does not look past n_draft)."""
    B, k = draft_row.shape
    val = np.zeros((B * (k + 1), amax_val.shape[1]), amax_val.dtype)
    idx = np.zeros((B * (k + 1), amax_idx.shape[1]), amax_idx.dtype)
    val[:B], idx[:B] = amax_val[:B], amax_idx[:B]
    for b in range(B):
        for j in range(1, k + 1):
            r = int(draft_row[b, j - 1])
            if r >= 0:
                val[j * B + b], idx[j * B + b] = amax_val[r], amax_idx[r]
    return val, idx


def accept_rows(amax_val, amax_idx, n_draft, draft_tok, draft_row, hist, ctx, plen, fin, eos, pad_id, flags, k):
    """What kr_spec_accept_rows does: kr_spec_accept (spec_ref.accept) on the rows the map names.  hist / ctx / fin are updated in
    place; returns (tokens_out [B], proposed [B], accepted [B]) of this step."""
    val, idx = static_partials(amax_val, amax_idx, np.asarray(draft_row).reshape(len(n_draft), k))
    return R.accept(val, idx, n_draft, draft_tok, hist, ctx, plen, fin, eos, pad_id, flags, k)


def simulate(prompts, scripts, truths, k: int, rows: int, steps: int, n_min: int = 2, n_max: int = 4, eos=(), start: int = 1,
             trace: Optional[list] = None) -> List[Tuple[int, int, int]]:
    """`steps` shared-rows steps over all slots: slot b's drafts come from scripts[b] (indexed by generated-token index) or, where
    that is None, from the lookup in prompts[b] + what it has generated, while the model's own continuation is truths[b]; `start`
    tokens are out already.  Per slot (generated, proposed, accepted) afterwards; proposed counts the drafts that were dealt a row.
    An emitted token in `eos` finishes the slot.  trace: a list that receives (n_want [B], n_draft [B]) per step."""
    B = len(truths)
    truths = [[int(t) for t in tr] for tr in truths]
    gen, prop, acc = [start] * B, [0] * B, [0] * B
    live = [not (start > 0 and tr[start - 1] in eos) for tr in truths]
    for _ in range(steps):
        drafts: List[List[int]] = []
        for b in range(B):
            if not live[b]:
                drafts.append([])
            elif scripts[b] is not None:
                drafts.append([int(t) for t in scripts[b][gen[b]:gen[b] + k]])
            else:
                drafts.append(R.lookup([int(t) for t in prompts[b]] + truths[b][:gen[b]], k, n_min, n_max))
        want = [len(d) for d in drafts]
        nd = (deal_rows(want, live, k, rows) >= 0).sum(axis=1)
        if trace is not None:
            trace.append((list(want), [int(n) for n in nd]))
        for b in range(B):
            if not live[b]:
                continue
            tr, g, e = truths[b], gen[b], 0
            for j in range(k + 1):
                if j > 0 and not (j <= nd[b] and drafts[b][j - 1] == tr[g + j - 1]):
                    break
                assert g + j < len(tr), "the recorded continuation is too short for this many steps"
                e += 1
                if tr[g + j] in eos:
                    live[b] = False
                    break
            acc[b] += sum(1 for j in range(min(e, int(nd[b]))) if drafts[b][j] == tr[g + j])
            prop[b] += int(nd[b])
            gen[b] = g + e
    return list(zip(gen, prop, acc))
