"""Numpy restatement of what lets requests with sampling controls and logit adjustments take part in a speculative decode step
(include/karanta_hip.h: kr_spec_controls_trim, kr_spec_controls_rows, kr_spec_controls_count, and the counts the row-mapped sampler
launches read); not a test module.  test_spec_controls_cpu.py checks it on hand-worked cases and in a closed loop against plain
controlled steps, test_gpu_spec_controls_kernels.py runs the kernels against it, test_gpu_spec_controls_engine.py compares the engine's
counters with `simulate`.

Written from the rules, not from the kernels.  A slot's adjustment table is the device's: ids / flags [B, CAP] and meta [B, 4] =
{n_entries, min_tokens, 0, 0}; a stop entry is an entry whose flag has bit 0 set."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


def stop_entries(ids, flags, meta, b: int) -> set:
    """The stop entries of slot b's table."""
    n = int(meta[b][0])
    return {int(ids[b][e]) for e in range(n) if int(flags[b][e]) & 1}


def trim(ids, flags, meta, fin, ctx, n_count, draft_tok, pad_id: int):
    """kr_spec_controls_trim.  ids / flags [B, CAP], meta [B, 4], fin / ctx / n_count [B], draft_tok [B, k].  Returns (n_count,
    draft_tok, ctx_before), the inputs untouched.  ctx_before = ctx, always.  A finished slot or one with an empty table keeps its
    count and its drafts.  Otherwise the count is cut to j - 1 at the first draft j that is a stop entry, and draft_tok at and beyond
    the new count is pad_id."""
    n_count, draft_tok = np.array(n_count, np.int32), np.array(draft_tok, np.int32)
    B, k = draft_tok.shape
    for b in range(B):
        if fin[b] or int(meta[b][0]) == 0:
            continue
        stops = stop_entries(ids, flags, meta, b)
        n = max(0, min(k, int(n_count[b])))
        for j in range(1, n + 1):
            if int(draft_tok[b, j - 1]) in stops:
                n_count[b] = j - 1
                draft_tok[b, j - 1:] = pad_id
                break
    return n_count, draft_tok, np.array(ctx, np.int32)


def depth_rows(fin_rows, n_draft, B: int, k: int, R: int, draft_row=None):
    """kr_spec_controls_rows.  fin_rows [R]: the per-row `finished`, the slots' entries in front; n_draft [B] as the trims (and the
    deal) left it; draft_row [B, k] or None for the static layout (draft j of a slot on row j * B + slot).  Returns (depth [R],
    fin_rows): depth is j for the row of draft (slot, j) with j <= n_draft[slot] and 0 for every other row; static layout only: a
    row (slot, j) with j > n_draft[slot] is finished."""
    depth, fin_rows = np.zeros(R, np.int32), np.array(fin_rows, np.int32)
    for b in range(B):
        for j in range(1, k + 1):
            r = j * B + b if draft_row is None else int(np.asarray(draft_row).reshape(B, k)[b, j - 1])
            if not B <= r < R:
                continue
            if j <= int(n_draft[b]):
                depth[r] = j
            elif draft_row is None:
                fin_rows[r] = 1
    return depth, fin_rows


def effective_counts(counts_slot, drafts: Sequence[int], depth: int) -> np.ndarray:
    """The output counts a row at `depth` sees: the slot's plus one for each of the drafts d_1..d_depth in front of it."""
    c = np.array(counts_slot, np.int32)
    for t in list(drafts)[:int(depth)]:
        c[int(t)] += 1
    return c


def count_update(counts, ctx_before, ctx, plen, hist, k: int, vocab: Optional[int] = None):
    """kr_spec_controls_count.  counts [B, V]; the slots' ctx_before / ctx / plen [B]; hist [T, B] as the verification left it.
    Returns counts with +1 for each of the e = ctx - ctx_before tokens the step emitted (0 <= e <= k + 1; generated-token indices
    ctx_before + 1 - plen ..), a finishing EOS or stop token included."""
    counts = np.array(counts, np.int32)
    V = counts.shape[1] if vocab is None else vocab
    for b in range(counts.shape[0]):
        e = max(0, min(k + 1, int(ctx[b]) - int(ctx_before[b])))
        for i in range(e):
            h = int(ctx_before[b]) + 1 - int(plen[b]) + i
            if 0 <= h < hist.shape[0]:
                t = int(hist[h, b])
                if 0 <= t < V:
                    counts[b, t] += 1
    return counts


def stop_tokens(tokens, ids, flags, meta, fin, flags_word: int = 2):
    """kr_stop_tokens: a live slot whose token is one of its stop entries finishes (in place on fin); bit 0 of the flags word:
    nothing finishes."""
    if flags_word & 1:
        return
    for b in range(len(tokens)):
        if not fin[b] and int(meta[b][0]) > 0 and int(tokens[b]) in stop_entries(ids, flags, meta, b):
            fin[b] = 1


def simulate(scripts, truths, stops: Sequence[set], k: int, steps: int, eos=(), rows: Optional[int] = None, start: int = 1,
             trace=None, depths: Optional[list] = None, trim: bool = True) -> List[Tuple[int, int, int]]:
    """`steps` controlled speculative steps over all slots: slot b's drafts come from scripts[b] (indexed by generated-token index)
    while the model's own — controlled — continuation is truths[b]; stops[b] is the set of the slot's stop entries.  The drafts of a
    step are cut in front of the first stop entry; rows: the shared-rows layout, where the cut counts are then dealt rows
    (spec_deal_ref.deal_rows), else every slot has its k rows.  An emitted token in `eos` or in the slot's stop entries finishes the
    slot.  Per slot (generated, proposed, accepted) afterwards.  trace receives (wanted [B], trimmed [B], n_draft [B]) per step;
    depths[b] receives, per step, the number of drafts of slot b that were accepted.  trim=False: what the counters would be if a
    drafted stop entry were verified and rejected like any wrong draft."""
    from tests import spec_deal_ref as D
    B = len(truths)
    truths = [[int(t) for t in tr] for tr in truths]
    gen, prop, acc = [start] * B, [0] * B, [0] * B
    ends = [set(int(e) for e in eos) | set(stops[b]) for b in range(B)]
    live = [not (start > 0 and tr[start - 1] in ends[b]) for b, tr in enumerate(truths)]
    for _ in range(steps):
        want, cut = [0] * B, [0] * B
        for b in range(B):
            if not live[b]:
                continue
            want[b] = cut[b] = max(0, min(k, len(scripts[b]) - gen[b]))
            for j in range(want[b]):
                if trim and int(scripts[b][gen[b] + j]) in stops[b]:
                    cut[b] = j
                    break
        nd = cut if rows is None else [int(n) for n in (D.deal_rows(cut, live, k, rows) >= 0).sum(axis=1)]
        if trace is not None:
            trace.append((list(want), list(cut), list(nd)))
        for b in range(B):
            if not live[b]:
                continue
            tr, sc, g, e = truths[b], scripts[b], gen[b], 0
            for j in range(k + 1):
                if j > 0 and not (j <= nd[b] and int(sc[g + j - 1]) == tr[g + j - 1]):
                    break
                assert g + j < len(tr), "the recorded continuation is too short for this many steps"
                e += 1
                if tr[g + j] in ends[b]:
                    live[b] = False
                    break
            a = sum(1 for j in range(min(e, nd[b])) if int(sc[g + j]) == tr[g + j])
            if depths is not None:
                depths[b].append(a)
            acc[b] += a
            prop[b] += nd[b]
            gen[b] = g + e
    return list(zip(gen, prop, acc))
