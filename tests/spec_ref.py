"""Numpy restatement of the two ends of a speculative decode step (include/karanta_hip.h: kr_spec_propose, kr_spec_accept); not a
test module.  test_spec_ref_cpu.py checks it on hand-worked cases, test_gpu_spec_kernels.py runs the kernels against it.

Written from the rule, not from the kernel: the lookup below is the literal double loop over n and i."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


def lookup(seq: Sequence[int], k: int, n_min: int, n_max: int) -> List[int]:
    """The drafts for the sequence s[0..L): for n from n_max down to n_min (n <= L - 1) the matches are the i with
    i + n <= L - 1 and s[i..i+n) == s[L-n..L); the first n that has a match decides; among its matches the one maximising
    (min(k, L - i - n), i); the drafts are the tokens after it."""
    s = [int(x) for x in seq]
    L = len(s)
    for n in range(n_max, n_min - 1, -1):
        if n > L - 1:
            continue
        tail = s[L - n:]
        best = None
        for i in range(0, L - 1 - n + 1):
            if s[i:i + n] == tail:
                key = (min(k, L - i - n), i)
                if best is None or key > best:
                    best = key
        if best is not None:
            c, i = best
            return s[i + n:i + n + c]
    return []


def sequence(prompt: Sequence[int], hist_col: Sequence[int], ctx_len: int) -> List[int]:
    """s[0..ctx_len + 1): the prompt, then the slot's column of the token history."""
    plen = len(prompt)
    return [int(x) for x in prompt] + [int(x) for x in hist_col[:ctx_len + 1 - plen]]


def propose(prompts, hist, ctx, plen, fin, temp, seed, k, rows, n_min, n_max, s_max, pad_id, vocab, scripts=None):
    """What kr_spec_propose writes.  prompts: per slot the prompt ids; hist [T, B]; ctx / plen / fin / temp / seed [B] (the slots'
    entries of the row arrays); scripts: per slot None or the scripted continuation.  Returns a dict: n_draft [B], draft_tok [B, k],
    and the row arrays [rows] (slot, ctx, plen, fin, temp, seed, tok) with the slots' own entries in front as given (tok = -1 there:
    the kernel does not write x of a slot's own row)."""
    B = len(ctx)
    out = {"n_draft": np.zeros(B, np.int32), "draft_tok": np.full((B, k), pad_id, np.int32),
           "slot": np.arange(rows, dtype=np.int32) % B, "ctx": np.zeros(rows, np.int32), "plen": np.zeros(rows, np.int32),
           "fin": np.ones(rows, np.int32), "temp": np.zeros(rows, np.float32), "seed": np.zeros(rows, np.uint32),
           "tok": np.full(rows, -1, np.int64)}
    out["slot"][:B] = np.arange(B)
    for name, src in (("ctx", ctx), ("plen", plen), ("fin", fin), ("temp", temp), ("seed", seed)):
        out[name][:B] = src
    for b in range(B):
        drafts: List[int] = []
        if not fin[b]:
            sc = scripts[b] if scripts is not None else None
            if sc is not None:
                gen = int(ctx[b]) + 1 - int(plen[b])
                drafts = [int(x) for x in sc[gen:gen + k]]
            else:
                drafts = lookup(sequence(prompts[b][:plen[b]], hist[:, b], int(ctx[b])), k, n_min, n_max)
            drafts = drafts[:max(0, s_max - 1 - int(ctx[b]))]
            for j, t in enumerate(drafts):
                if t < 0 or t >= vocab:
                    drafts = drafts[:j]
                    break
        nd = len(drafts)
        out["n_draft"][b] = nd
        out["draft_tok"][b, :nd] = drafts
        for j in range(1, k + 1):
            r = j * B + b
            out["slot"][r], out["plen"][r], out["temp"][r], out["seed"][r] = b, plen[b], temp[b], seed[b]
            out["ctx"][r] = min(int(ctx[b]) + j, s_max - 1)
            active = (not fin[b]) and j <= nd
            out["fin"][r] = 0 if active else 1
            out["tok"][r] = drafts[j - 1] if active else pad_id
    for r in range(B * (k + 1), rows):      # rows past the layout: inactive rows of slot 0 parked on the last cache row
        out["slot"][r], out["ctx"][r], out["plen"][r], out["fin"][r], out["tok"][r] = 0, s_max - 1, s_max - 1, 1, pad_id
    return out


def greedy_step(tok: int, hist, b: int, ctx, plen, fin, eos, pad_id: int, flags: int) -> Optional[int]:
    """kr_sample_greedy for one slot and one step, in place on hist / ctx / fin: returns the token fed back (tokens_out)."""
    ignore_eos, freeze = bool(flags & 1), bool(flags & 2)
    was = bool(fin[b])
    if was and not ignore_eos:
        tok = pad_id
    if freeze and was and not ignore_eos:
        return tok
    ctx[b] += 1
    hist[ctx[b] - plen[b], b] = tok
    if not ignore_eos and not was and tok in eos:
        fin[b] = 1
    return tok


def argmax_partials(val: np.ndarray, idx: np.ndarray) -> int:
    """The final argmax over one row's partials: the largest value, ties to the lowest token index."""
    best = val.max()
    return int(idx[val == best].min())


def accept(amax_val, amax_idx, n_draft, draft_tok, hist, ctx, plen, fin, eos, pad_id, flags, k) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What kr_spec_accept does, as kr_sample_greedy applied token by token: amax_* [rows, n_part]; hist / ctx / fin (the slots'
    entries) are updated in place.  Returns (tokens_out [B], proposed [B], accepted [B]) of this step."""
    B = len(n_draft)
    tokens_out = np.zeros(B, np.int32)
    proposed, accepted = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        t = [argmax_partials(amax_val[j * B + b], amax_idx[j * B + b]) for j in range(k + 1)]
        if fin[b] and not (flags & 1):
            tokens_out[b] = greedy_step(t[0], hist, b, ctx, plen, fin, eos, pad_id, flags)
            continue
        nd = int(n_draft[b])
        emitted = []
        for j in range(k + 1):
            if j > 0 and not (j <= nd and int(draft_tok[b, j - 1]) == t[j - 1]):
                break
            tokens_out[b] = greedy_step(t[j], hist, b, ctx, plen, fin, eos, pad_id, flags)
            emitted.append(t[j])
            if fin[b] and not (flags & 1):
                break
        # a draft is accepted when it equals the token emitted at its position (draft j + 1 <-> t_j)
        proposed[b], accepted[b] = nd, sum(1 for j, tok in enumerate(emitted) if j < nd and int(draft_tok[b, j]) == tok)
    return tokens_out, proposed, accepted


def simulate(script: Sequence[int], truth: Sequence[int], k: int, steps: int, eos=(), start: int = 1, trace=None) -> Tuple[int, int, int]:
    """`steps` speculative steps on one slot whose drafts come from `script` while the model's own continuation is `truth` (both
    indexed by generated-token index; `start` tokens are out already): (generated, proposed, accepted) afterwards.  An emitted token
    in `eos` finishes the slot: later steps neither propose nor emit.  trace: a list that receives (n_draft, emitted) per live step."""
    gen, prop, acc, live = start, 0, 0, not (start > 0 and truth[start - 1] in eos)
    for _ in range(steps):
        if not live:
            continue
        nd = max(0, min(k, len(script) - gen))
        e = 0
        for j in range(k + 1):
            if j > 0 and not (j <= nd and script[gen + j - 1] == truth[gen + j - 1]):
                break
            assert gen + j < len(truth), "the recorded continuation is too short for this many steps"
            e += 1
            if truth[gen + j] in eos:
                live = False
                break
        acc += sum(1 for j in range(min(e, nd)) if script[gen + j] == truth[gen + j])
        prop, gen = prop + nd, gen + e
        if trace is not None:
            trace.append((nd, e))
    return gen, prop, acc
