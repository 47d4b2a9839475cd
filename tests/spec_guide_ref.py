"""Numpy restatement of the three launches that let guided slots take part in a speculative decode step (include/karanta_hip.h:
kr_spec_guide_trim, kr_spec_guide_rows, kr_spec_guide_advance); not a test module.  test_spec_guide_cpu.py checks it on hand-worked
cases and in a closed loop against plain guided steps, test_gpu_spec_guide_kernels.py runs the kernels against it.

Written from the rules, not from the kernels: states move through guided.Guide.walk, and the allowed-token table is built here in
Python from Guide.trans / Guide.accept by kr_guide_build_masks' rule.  A slot's guide is an index into a list of patterns, 1-based
(0: the slot is unconstrained) — what the device arrays hold as table addresses."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from karanta_ocr_amd.guided import Guide, compile_regex

MULTI = [b"ab", b"abc", b"abc-", b"12;", b"bc", b"ca", b"-1", b"-12", b"2;", b"12", b"ab-", b"cab", b"a-", b"34;", b"ab-1", b"c-",
         b"bb", b"aa", b"00;", b"-0"]
SPECIAL, EOS = 256 + len(MULTI), 256 + len(MULTI) + 1      # the two ids without bytes; EOS is the one listed as such


def synthetic_vocab(size: int = 300) -> List[bytes]:
    """Ids 0..255: the single bytes; then MULTI's 2 to 4-byte strings; SPECIAL and EOS without bytes; three-byte fillers up to size."""
    tb = [bytes([i]) for i in range(256)] + list(MULTI) + [b"", b""]
    return tb + [b"z%02d" % i for i in range(size - len(tb))]


def build_mask(guide: Guide, token_bytes: Sequence[bytes], eos: Sequence[int]) -> np.ndarray:
    """[S, V] bool, kr_guide_build_masks' rule: in state s != 0 a token with bytes is allowed iff the walk over them stays alive; a
    token without bytes never — except the EOS ids, allowed exactly in the accepting states.  State 0 allows nothing."""
    S, V = guide.n_states, len(token_bytes)
    m = np.zeros((S, V), bool)
    for s in range(1, S):
        for t, b in enumerate(token_bytes):
            m[s, t] = len(b) > 0 and guide.walk(s, b) != 0
        for e in eos:
            m[s, e] = bool(guide.accept[s])
    return m


class Pattern:
    """A compiled pattern and its allowed-token table over one vocabulary."""

    def __init__(self, pattern: str, token_bytes: Sequence[bytes], eos: Sequence[int]):
        self.guide = compile_regex(pattern) if isinstance(pattern, str) else pattern
        self.mask = build_mask(self.guide, token_bytes, eos)
        self.start = int(self.guide.start)


def trim(pats: Sequence[Pattern], gid, gstate, fin, ctx, n_count, draft_tok, draft_state, pad_id: int, token_bytes):
    """kr_spec_guide_trim.  gid / gstate / fin / ctx [B]: the slots' entries; n_count [B]; draft_tok, draft_state [B, k].  Returns
    (n_count, draft_tok, draft_state, ctx_before), the inputs untouched.  ctx_before = ctx, always.  A finished or unconstrained
    slot keeps its count and its drafts.  Otherwise from st = gstate, for j = 1..n_count: draft j is kept iff the mask allows it in
    st; the first that is not cuts the count to j - 1; a kept draft moves st over its bytes and draft_state[j - 1] = st; a kept draft
    without bytes cuts the count to j.  draft_tok at and beyond the new count is pad_id."""
    n_count, draft_tok, draft_state = np.array(n_count, np.int32), np.array(draft_tok, np.int32), np.array(draft_state, np.int32)
    B, k = draft_tok.shape
    for b in range(B):
        if fin[b] or gid[b] == 0:
            continue
        p = pats[int(gid[b]) - 1]
        st, keep = int(gstate[b]), int(n_count[b])
        for j in range(1, int(n_count[b]) + 1):
            t = int(draft_tok[b, j - 1])
            if not (0 <= t < len(token_bytes)) or not p.mask[st, t]:
                keep = j - 1
                break
            st = p.guide.walk(st, token_bytes[t])
            draft_state[b, j - 1] = st
            if len(token_bytes[t]) == 0:
                keep = j
                break
        n_count[b] = keep
        draft_tok[b, keep:] = pad_id
    return n_count, draft_tok, draft_state, np.array(ctx, np.int32)


def rows(gid, gstate, fin, n_draft, draft_state, B: int, k: int, R: int, draft_row=None):
    """kr_spec_guide_rows.  gid / gstate / fin [R]: the per-row arrays, the slots' entries in front; n_draft [B] and draft_state
    [B, k] as the trim (and the deal) left them; draft_row [B, k] or None for the static layout (draft j of a slot on row
    j * B + slot).  Returns (gid, gstate, fin) with every row r >= B rewritten: the row of draft (slot, j), j <= n_draft[slot], of a
    guided slot carries the slot's guide and draft_state[slot, j - 1]; every other row zeros.  Static layout only: a row (slot, j)
    with j > n_draft[slot] is finished."""
    gid, gstate, fin = np.array(gid), np.array(gstate, np.int32), np.array(fin, np.int32)
    owner = {}
    for b in range(B):
        for j in range(1, k + 1):
            r = j * B + b if draft_row is None else int(np.asarray(draft_row).reshape(B, k)[b, j - 1])
            if B <= r < R:
                owner[r] = (b, j)
    for r in range(B, R):
        gid[r], gstate[r] = 0, 0
        if r not in owner:
            continue
        b, j = owner[r]
        if j <= int(n_draft[b]):
            if gid[b] != 0:
                gid[r], gstate[r] = gid[b], draft_state[b, j - 1]
        elif draft_row is None:
            fin[r] = 1
    return gid, gstate, fin


def advance(pats: Sequence[Pattern], gid, gstate, ctx_before, ctx, plen, fin, hist, token_bytes):
    """kr_spec_guide_advance.  The slots' entries [B]; hist [T, B] as the verification left it.  Returns gstate: per guided slot the
    state walked over the e = ctx - ctx_before tokens the step emitted (generated-token indices ctx_before + 1 - plen ..), except the
    last one where the slot is finished now (e > 0: this step finished it)."""
    gstate = np.array(gstate, np.int32)
    for b in range(len(gstate)):
        if gid[b] == 0:
            continue
        e = int(ctx[b]) - int(ctx_before[b])
        n = e - 1 if (e > 0 and fin[b]) else e
        st = int(gstate[b])
        for i in range(n):
            t = int(hist[int(ctx_before[b]) + 1 - int(plen[b]) + i, b])
            if 0 <= t < len(token_bytes):
                st = pats[int(gid[b]) - 1].guide.walk(st, token_bytes[t])
        gstate[b] = st
    return gstate


def allowed(pats: Sequence[Pattern], gid: int, state: int, vocab: int) -> Optional[np.ndarray]:
    """The token ids a row may choose: None where it is unconstrained."""
    return None if gid == 0 else np.flatnonzero(pats[int(gid) - 1].mask[int(state)][:vocab])


def plain_guided_step(tok: int, pats, gid, gstate, b: int, hist, ctx, plen, fin, eos, pad_id: int, flags: int, token_bytes):
    """One plain guided step of slot b with the chosen token `tok`, in place: kr_sample_greedy (spec_ref.greedy_step), then
    kr_guide_advance — a row that is finished afterwards keeps its state."""
    from tests import spec_ref as R
    R.greedy_step(tok, hist, b, ctx, plen, fin, eos, pad_id, flags)
    if gid[b] != 0 and not fin[b] and 0 <= tok < len(token_bytes):
        gstate[b] = pats[int(gid[b]) - 1].guide.walk(int(gstate[b]), token_bytes[tok])


def simulate(scripts, truths, pats: Sequence[Optional[Pattern]], token_bytes, k: int, steps: int, eos=(), rows: Optional[int] = None,
             start: int = 1, trace=None) -> List[Tuple[int, int, int]]:
    """`steps` guided speculative steps over all slots: slot b's drafts come from scripts[b] (indexed by generated-token index; []:
    none) while the model's own — guided — continuation is truths[b]; pats[b] is the slot's pattern or None.  The drafts of a step
    are cut where the guide forbids one and behind an allowed token without bytes; rows: the shared-rows layout, where the cut counts
    are then dealt rows (spec_deal_ref.deal_rows), else every slot has its k rows.  Per slot (generated, proposed, accepted)
    afterwards; an emitted token in `eos` finishes the slot.  trace receives (wanted [B], trimmed [B], n_draft [B]) per step."""
    from tests import spec_deal_ref as D
    B = len(truths)
    truths = [[int(t) for t in tr] for tr in truths]
    gen, prop, acc = [start] * B, [0] * B, [0] * B
    live = [not (start > 0 and tr[start - 1] in eos) for tr in truths]
    for _ in range(steps):
        want, cut = [0] * B, [0] * B
        for b in range(B):
            if not live[b]:
                continue
            want[b] = cut[b] = max(0, min(k, len(scripts[b]) - gen[b]))
            p = pats[b]
            if p is None:
                continue
            st = p.start
            for t in truths[b][:gen[b]]:
                st = p.guide.walk(st, token_bytes[t])
            for j in range(want[b]):
                t = int(scripts[b][gen[b] + j])
                if not p.mask[st, t]:
                    cut[b] = j
                    break
                st = p.guide.walk(st, token_bytes[t])
                if len(token_bytes[t]) == 0:
                    cut[b] = j + 1
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
                if tr[g + j] in eos:
                    live[b] = False
                    break
            acc[b] += sum(1 for j in range(min(e, nd[b])) if int(sc[g + j]) == tr[g + j])
            prop[b] += nd[b]
            gen[b] = g + e
    return list(zip(gen, prop, acc))
