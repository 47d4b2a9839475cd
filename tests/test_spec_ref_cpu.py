"""tests/spec_ref.py on hand-worked cases: the prompt-lookup rule, the row layout of a speculative step and the token-by-token
acceptance.  The GPU tests compare the kernels with these functions, so they are pinned here to answers worked out by hand."""
import numpy as np

from tests import spec_ref as R


def test_lookup_rule_by_hand():
    K = 3
    # no earlier occurrence of the last two tokens
    assert R.lookup([1, 2, 3, 4, 5, 6], K, 2, 4) == []
    # [7, 8] occurred at i = 1: the tokens behind it
    assert R.lookup([0, 7, 8, 9, 10, 11, 5, 7, 8], K, 2, 4) == [9, 10, 11]
    # the longest n wins although a shorter n has a later match: n = 3 matches at i = 0 only, n = 2 also at i = 5
    assert R.lookup([1, 2, 3, 40, 41, 2, 3, 50, 51, 1, 2, 3], K, 2, 3) == [40, 41, 2]
    # fallback from n_max to n_min: [9, 2, 3] never occurred, [2, 3] did
    assert R.lookup([1, 2, 3, 40, 41, 42, 9, 2, 3], K, 2, 3) == [40, 41, 42]
    # a truncated continuation loses to an earlier full one: [5, 6] at i = 0 (3 tokens follow) and at i = 5 (only 2 before the suffix ...
    s = [5, 6, 70, 71, 72, 5, 6, 80, 5, 6]
    # ... i = 5: L - i - n = 10 - 5 - 2 = 3 as well -> the tie on the count goes to the larger i
    assert R.lookup(s, K, 2, 2) == [80, 5, 6]
    # here the later match has one token only (count 1) and loses to the earlier full one
    assert R.lookup([5, 6, 70, 71, 72, 9, 5, 6, 5, 6], K, 2, 2) == [70, 71, 72]
    # the match may overlap the suffix: i + n <= L - 1 is the only bound ([4, 4] at i = 0 and i = 1 of [4, 4, 4])
    assert R.lookup([4, 4, 4], K, 2, 2) == [4]
    # L <= n_min: nothing to look up
    assert R.lookup([3, 3], K, 2, 4) == []
    assert R.lookup([3], K, 1, 4) == []
    # n_min = 1, L = 2
    assert R.lookup([3, 3], K, 1, 4) == [3]


def test_sequence_crosses_the_prompt_history_border():
    hist = np.asarray([[11, 0], [12, 0], [13, 0], [99, 0]])
    assert R.sequence([1, 2, 3], hist[:, 0], ctx_len=4) == [1, 2, 3, 11, 12]
    # suffix [3, 11] lies across the border; its earlier occurrence is inside the prompt
    assert R.lookup(R.sequence([3, 11, 50, 3], np.asarray([11, 7]), 4), 2, 2, 4) == [50, 3]


def test_propose_rows_by_hand():
    B, K, rows, s_max, pad, V = 2, 2, 8, 64, 0, 100
    prompts = [np.asarray([7, 8, 9, 7, 8]), np.asarray([1, 2, 3])]
    hist = np.zeros((8, B), np.int32)
    ctx, plen = np.asarray([4, 62]), np.asarray([5, 3])
    fin = np.asarray([0, 0])
    temp, seed = np.asarray([0.5, 0.0], np.float32), np.asarray([17, 3], np.uint32)
    # slot 0: s = [7, 8, 9, 7, 8] -> drafts [9, 7]; slot 1 scripted, generated = 60, room for no draft (ctx = s_max - 2 -> 1 draft)
    hist1 = np.zeros((70, B), np.int32)
    out = R.propose(prompts, hist1, ctx, plen, fin, temp, seed, K, rows, 2, 4, s_max, pad, V, scripts=[None, list(range(100))])
    assert out["n_draft"].tolist() == [2, 1]
    assert out["draft_tok"].tolist() == [[9, 7], [60, pad]]
    #        rows:  s0 s1 | j=1: s0 s1 | j=2: s0 s1 | past the layout
    assert out["slot"].tolist() == [0, 1, 0, 1, 0, 1, 0, 0]
    assert out["ctx"].tolist() == [4, 62, 5, 63, 6, 63, 63, 63]          # slot 1, j = 2: clamped to s_max - 1
    assert out["fin"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    assert out["tok"].tolist() == [-1, -1, 9, 60, 7, pad, pad, pad]
    assert out["plen"].tolist() == [5, 3, 5, 3, 5, 3, 63, 63]
    assert out["seed"].tolist() == [17, 3, 17, 3, 17, 3, 0, 0]
    # a finished slot proposes nothing; a parked slot (ctx = plen = s_max - 1, finished) gets the clamp on every row
    out = R.propose(prompts, hist1, np.asarray([4, 63]), np.asarray([5, 63]), np.asarray([1, 1]), temp, seed, K, rows, 2, 4, s_max, pad, V)
    assert out["n_draft"].tolist() == [0, 0] and out["fin"][B:].tolist() == [1] * 6
    assert out["ctx"].tolist() == [4, 63, 5, 63, 6, 63, 63, 63]


def partials(tokens, n_part=4, vocab=100):
    """amax partials [rows, n_part] whose final argmax is tokens[r]: the winner in a random part, a tie with a HIGHER index in another."""
    rows = len(tokens)
    val = np.full((rows, n_part), -5.0, np.float32)
    idx = np.tile(np.arange(n_part, dtype=np.int32) + 1, (rows, 1))
    for r, t in enumerate(tokens):
        val[r, (r + 1) % n_part], idx[r, (r + 1) % n_part] = 3.0, t
        val[r, (r + 2) % n_part], idx[r, (r + 2) % n_part] = 3.0, t + 1     # the tie goes to the lower index
    return val, idx


def test_accept_by_hand():
    B, K, pad, eos = 3, 2, 0, (50,)
    # rows j * B + b: slot 0 produces 10, 11, 12; slot 1 produces 20, 50 (EOS), 22; slot 2 is finished
    val, idx = partials([10, 20, 30, 11, 50, 31, 12, 22, 32])
    hist = np.full((12, B), -1, np.int32)
    ctx, plen, fin = np.asarray([6, 4, 9]), np.asarray([5, 4, 8]), np.asarray([0, 0, 1])
    n_draft = np.asarray([2, 2, 0])
    draft = np.asarray([[10, 99], [20, 50], [pad, pad]])     # slot 0: draft 2 is wrong; slot 1: both right, EOS at t_1
    tok, prop, acc = R.accept(val, idx, n_draft, draft, hist, ctx, plen, fin, eos, pad, 2, K)
    # slot 0: t_0 = 10 always; draft 1 = 10 = t_0 -> t_1 = 11; draft 2 = 99 != t_1 -> stop.  history rows ctx + 1 + j - plen = 2, 3
    assert hist[:, 0].tolist() == [-1, -1, 10, 11] + [-1] * 8 and ctx[0] == 8 and tok[0] == 11 and fin[0] == 0
    # slot 1: 20, then 50 = EOS: emitted, finishes the slot, t_2 is not emitted although draft 2 was right
    assert hist[:, 1].tolist() == [-1, 20, 50] + [-1] * 9 and ctx[1] == 6 and tok[1] == 50 and fin[1] == 1
    # slot 2: frozen
    assert (hist[:, 2] == -1).all() and ctx[2] == 9 and tok[2] == pad
    # accepted: slot 0's draft 1; slot 1's both drafts (the second IS the EOS that was emitted)
    assert prop.tolist() == [2, 2, 0] and acc.tolist() == [1, 2, 0]


def test_simulate_counts():
    truth = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    assert R.simulate(truth, truth, 3, 2) == (9, 6, 6)                    # 1 + 4 + 4 generated
    bad = list(truth)
    bad[2] = 99                                                            # draft for index 2 is wrong
    # step 1 (gen 1): drafts idx 1, 2, 3: idx 1 right, idx 2 wrong -> 2 emitted (1 accepted); step 2 (gen 3): all right -> 4
    assert R.simulate(bad, truth, 3, 2) == (7, 6, 4)
    assert R.simulate(truth, truth, 3, 5, eos=(8,)) == (4, 3, 3)           # 8 sits at index 3: drafted, emitted, then the slot idles
    assert R.simulate(truth[:3], truth, 3, 2) == (5, 2, 2)                 # the script runs out: 2 drafts (1 + 3 tokens), then none (+ 1)
