"""Speculative decoding for guided requests without a GPU: the numpy restatement of kr_spec_guide_trim / _rows / _advance
(tests/spec_guide_ref.py) on hand-worked cases and in a closed loop — a guided speculative step with arbitrary drafts leaves the
tokens, the DFA state, `finished` and the history that as many plain guided steps leave — the option's way through SpecConfig, the
command line and the slot scheduler, and the entry points' argument checks (host side: nothing launches)."""
import ctypes as C
import json
import zlib

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd._lib import KarantaHipError
from karanta_ocr_amd.request import SpecConfig
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy
from tests import spec_deal_ref as D
from tests import spec_guide_ref as G
from tests import spec_ref as R
from tests.test_spec_host_cpu import SCRIPT, FakeSpecEngine, Page

PATTERN = r"[a-f]{3}-[0-9]{2}(?:;[a-z ]{2,5})?"            # tests/test_gpu_spec_engine.py's
LONG = r"(?:[a-c]{2,3}-[0-9]{2};){1,4}"                    # holds K = 3 drafts many times over
TB = G.synthetic_vocab()
V, PAD = len(TB), 3
EOS, SPECIAL = G.EOS, G.SPECIAL
PATS = [G.Pattern(PATTERN, TB, (EOS,)), G.Pattern(LONG, TB, (EOS,))]


def tok(b: bytes) -> int:
    return TB.index(b)


def state(p: G.Pattern, text: bytes) -> int:
    return p.guide.walk(p.start, text)


# ----------------------------------------------------------------------------- the restatement, by hand
def test_the_mask_is_the_build_rule():
    p = PATS[0]
    s0, acc = p.start, state(p, b"abc-12")
    assert p.guide.accept[acc] and not p.guide.accept[s0]
    assert p.mask[s0, tok(b"a")] and p.mask[s0, tok(b"abc-")] and p.mask[s0, tok(b"ab")]
    assert not p.mask[s0, tok(b"-")] and not p.mask[s0, tok(b"ab-")] and not p.mask[s0, tok(b"12;")]
    assert p.mask[acc, EOS] and not p.mask[s0, EOS] and not p.mask[acc, SPECIAL] and not p.mask[s0, SPECIAL]
    assert not p.mask[0].any()


def trim1(gstate, drafts, n=None, gid=1, fin=0):
    """One slot, K = 3: (n_count, draft_tok, draft_state) after the trim."""
    k = 3
    d = np.full((1, k), PAD, np.int32)
    d[0, :len(drafts)] = drafts
    nc, dt, ds, cb = G.trim(PATS, [gid], [gstate], [fin], [41], [len(drafts) if n is None else n], d, np.full((1, k), -9), PAD, TB)
    assert cb.tolist() == [41]
    return int(nc[0]), dt[0].tolist(), ds[0].tolist()


def test_trim_by_hand():
    p = PATS[0]
    s0 = p.start
    a, b, c, dash, one = tok(b"a"), tok(b"b"), tok(b"c"), tok(b"-"), tok(b"1")
    # every draft allowed: the states behind them
    assert trim1(s0, [a, b, c]) == (3, [a, b, c], [state(p, b"a"), state(p, b"ab"), state(p, b"abc")])
    # forbidden at depth 1, 2, 3: the count is cut in front of it, the tokens from there on are the pad token
    assert trim1(s0, [dash, b, c]) == (0, [PAD] * 3, [-9] * 3)
    assert trim1(s0, [a, one, c]) == (1, [a, PAD, PAD], [state(p, b"a"), -9, -9])
    assert trim1(s0, [a, b, dash]) == (2, [a, b, PAD], [state(p, b"a"), state(p, b"ab"), -9])
    # a multi-byte draft that dies on its last byte ("ab-" wants a third letter), and one that lives
    assert trim1(s0, [tok(b"ab-"), a, a]) == (0, [PAD] * 3, [-9] * 3)
    assert trim1(s0, [tok(b"abc-"), tok(b"12;"), a]) == (3, [tok(b"abc-"), tok(b"12;"), a],
                                                       [state(p, b"abc-"), state(p, b"abc-12;"), state(p, b"abc-12;a")])
    # EOS: kept in an accepting state, where it ends the run; trimmed elsewhere.  A token without bytes that is no EOS: trimmed
    acc = state(p, b"abc-12")
    assert trim1(acc, [EOS, a, b]) == (1, [EOS, PAD, PAD], [acc, -9, -9])
    assert trim1(state(p, b"abc-1"), [tok(b"2"), EOS, a]) == (2, [tok(b"2"), EOS, PAD], [acc, acc, -9])
    assert trim1(s0, [a, EOS, b]) == (1, [a, PAD, PAD], [state(p, b"a"), -9, -9])
    assert trim1(acc, [SPECIAL, a, b]) == (0, [PAD] * 3, [-9] * 3)
    # fewer drafts than K; an unguided and a finished slot keep everything, forbidden tokens included
    assert trim1(s0, [a, b], n=2) == (2, [a, b, PAD], [state(p, b"a"), state(p, b"ab"), -9])
    assert trim1(s0, [dash, SPECIAL, EOS], gid=0) == (3, [dash, SPECIAL, EOS], [-9] * 3)
    assert trim1(s0, [dash, SPECIAL, EOS], fin=1) == (3, [dash, SPECIAL, EOS], [-9] * 3)


def test_rows_by_hand():
    B, k, Rr = 3, 2, 17
    gid = np.asarray([1, 0, 2] + [7] * (Rr - B))
    gstate = np.asarray([4, 5, 6] + [8] * (Rr - B), np.int32)
    fin = np.asarray([0, 0, 0] + [0] * (Rr - B), np.int32)
    ds = np.asarray([[11, 12], [21, 22], [31, 32]], np.int32)
    # static layout: row j * B + slot.  Slot 0 keeps one draft, slot 1 (unguided) two, slot 2 none
    g, s, f = G.rows(gid, gstate, fin, [1, 2, 0], ds, B, k, Rr)
    assert g[:B].tolist() == [1, 0, 2] and s[:B].tolist() == [4, 5, 6] and f[:B].tolist() == [0, 0, 0]
    assert g[B:].tolist() == [1, 0, 0, 0, 0, 0] + [0] * 8 and s[B:].tolist() == [11, 0, 0, 0, 0, 0] + [0] * 8
    assert f[B:].tolist() == [0, 0, 1, 1, 0, 1] + [0] * 8           # (rows past the layout are kr_spec_propose's alone)
    # the dealt map: slot 2's depth 1 on row 3, slot 0's depths on rows 5 and 4, nobody on the others; `finished` is the deal's
    row = np.asarray([[5, 4], [-1, -1], [3, -1]])
    g, s, f = G.rows(gid, gstate, fin, [2, 0, 1], ds, B, k, Rr, draft_row=row)
    assert g[B:].tolist() == [2, 1, 1] + [0] * 11 and s[B:].tolist() == [31, 12, 11] + [0] * 11 and not f.any()
    # a map that names a row beyond the dealt depth: zeros
    g, s, f = G.rows(gid, gstate, fin, [1, 0, 1], ds, B, k, Rr, draft_row=row)
    assert g[B:].tolist() == [2, 0, 1] + [0] * 11 and s[B:].tolist() == [31, 0, 11] + [0] * 11


def test_advance_by_hand():
    p = PATS[0]
    a, b, c = tok(b"a"), tok(b"b"), tok(b"c")
    plen = np.asarray([5, 5, 5, 5, 5])
    hist = np.full((12, 5), PAD, np.int32)
    # slot 0 emitted nothing (frozen), slot 1 one token, slot 2 K + 1 = 4 tokens, slot 3 ends on an EOS, slot 4 is unguided
    hist[2, 1] = c
    hist[0:4, 2] = [tok(b"abc-"), tok(b"1"), tok(b"2"), tok(b";")]
    hist[1:3, 3] = [tok(b"2"), EOS]
    before = np.asarray([7, 6, 4, 5, 5])
    ctx = np.asarray([7, 7, 8, 7, 9])
    fin = np.asarray([1, 0, 0, 1, 0])
    st = [state(p, b"abc-12"), state(p, b"ab"), p.start, state(p, b"abc-1"), 77]
    out = G.advance(PATS, [1, 1, 1, 1, 0], st, before, ctx, plen, fin, hist, TB)
    assert out.tolist() == [st[0], state(p, b"abc"), state(p, b"abc-12;"), state(p, b"abc-12"), 77]


# ----------------------------------------------------------------------------- the closed loop
def model(seq, allow) -> int:
    """The "model": any deterministic function of (sequence, allowed set); an empty allowed set gives the fallback EOS."""
    h = zlib.crc32(np.asarray(seq, np.int64).tobytes())
    if allow is None:
        return h % V
    return EOS if len(allow) == 0 else int(allow[h % len(allow)])


@pytest.mark.parametrize("B,K,rows,shared", [(5, 3, 20, False), (4, 1, 17, False), (3, 3, 17, True), (20, 3, 32, True)])
def test_a_guided_speculative_step_equals_as_many_plain_guided_steps(B, K, rows, shared):
    rng = np.random.default_rng(B * 100 + K)
    flags, T, steps = 2, 64, 10
    gid = np.asarray([(b % 3) for b in range(B)])                    # unguided, PATTERN, LONG in turn
    plen = np.asarray([4 + b % 5 for b in range(B)])
    prompts = [rng.integers(0, V, int(n)).tolist() for n in plen]
    # ---- the plain guided run: the truth, with the state and `finished` behind every generated token
    hist, ctx, fin = np.full((T, B), -1, np.int32), plen - 1, np.zeros(B, np.int32)
    gstate = np.asarray([PATS[g - 1].start if g else 0 for g in gid], np.int32)
    after = [{0: (int(gstate[b]), 0)} for b in range(B)]
    for _ in range(1 + steps * (K + 1)):
        for b in range(B):
            if fin[b]:
                continue
            seq = prompts[b] + hist[:ctx[b] + 1 - plen[b], b].tolist()
            t = model(seq, G.allowed(PATS, gid[b], gstate[b], V))
            G.plain_guided_step(t, PATS, gid, gstate, b, hist, ctx, plen, fin, (EOS,), PAD, flags, TB)
            after[b][int(ctx[b] + 1 - plen[b])] = (int(gstate[b]), int(fin[b]))
    truth, n_truth = hist, ctx + 1 - plen
    assert any(fin[b] for b in range(B) if gid[b]) or B < 5, "a guided slot should reach its forced EOS"
    # ---- the speculative run from the state behind the first token
    hist, ctx, fin = np.full((T, B), -1, np.int32), plen.copy(), np.zeros(B, np.int32)
    hist[0] = truth[0]
    g_rows, s_rows = np.zeros(rows, np.int64), np.zeros(rows, np.int32)
    g_rows[:B] = gid
    for b in range(B):
        s_rows[b], fin[b] = after[b][1]
    trimmed = accepted = 0
    for _ in range(steps):
        gen = ctx + 1 - plen
        draft = np.full((B, K), PAD, np.int32)
        n_count = np.zeros(B, np.int32)
        for b in range(B):
            if fin[b]:
                continue
            n_count[b] = rng.integers(0, K + 1)
            for j in range(int(n_count[b])):
                right = gen[b] + j < n_truth[b] and rng.random() < 0.75
                draft[b, j] = truth[gen[b] + j, b] if right else rng.choice([EOS, SPECIAL, tok(b"ab-"), tok(b"1"), tok(b"a"), tok(b"12;")])
        n0 = n_count.copy()
        n_count, draft, dstate, before = G.trim(PATS, g_rows[:B], s_rows[:B], fin, ctx, n_count, draft, np.full((B, K), -9), PAD, TB)
        trimmed += int((n0 - n_count).sum())
        assert (n_count[gid == 0] == n0[gid == 0]).all()
        fin_rows = np.ones(rows, np.int32)
        fin_rows[:B] = fin
        if shared:
            row = D.deal_rows(n_count, [not f for f in fin], K, rows)
            n_draft = (row >= 0).sum(axis=1).astype(np.int32)
            fin_rows[row[row >= 0]] = 0
        else:
            row, n_draft = None, n_count
            for b in range(B):
                fin_rows[[j * B + b for j in range(1, int(n0[b]) + 1)]] = 0        # kr_spec_propose ran before the trim
        g_rows, s_rows, fin_rows = G.rows(g_rows, s_rows, fin_rows, n_draft, dstate, B, K, rows, draft_row=row)
        # every live row chooses its token under its own guide entries; the other rows hold a token nobody may read
        idx = np.full((rows, 1), tok(b"a"), np.int32)
        for b in range(B):
            seq = prompts[b] + hist[:gen[b], b].tolist()
            for j in range(0, int(n_draft[b]) + 1):
                r = b if j == 0 else (j * B + b if row is None else int(row[b, j - 1]))
                assert fin_rows[r] == fin[b] if j == 0 else fin_rows[r] == 0
                idx[r, 0] = model(seq + draft[b, :j].tolist(), G.allowed(PATS, g_rows[r], s_rows[r], V))
        val = np.ones((rows, 1), np.float32)
        if shared:
            _, _, acc = D.accept_rows(val, idx, n_draft, draft, row, hist, ctx, plen, fin, (EOS,), PAD, flags, K)
        else:
            _, _, acc = R.accept(val, idx, n_draft, draft, hist, ctx, plen, fin, (EOS,), PAD, flags, K)
        accepted += int(acc.sum())
        s_rows[:B] = G.advance(PATS, g_rows[:B], s_rows[:B], before, ctx, plen, fin, hist, TB)
        for b in range(B):
            n = int(ctx[b] + 1 - plen[b])
            assert n >= gen[b] + (0 if after[b][int(gen[b])][1] else 1)
            np.testing.assert_array_equal(hist[:n, b], truth[:n, b], err_msg=f"slot {b}: tokens")
            assert (hist[n:, b] == -1).all(), f"slot {b}: history behind the emitted tokens"
            assert (int(s_rows[b]), int(fin[b])) == after[b][n], f"slot {b}: (state, finished) after {n} tokens"
    assert trimmed > 0 and accepted > 0


# ----------------------------------------------------------------------------- the option: SpecConfig, command line, scheduler
def test_spec_config_carries_the_option():
    assert SpecConfig().guided is False and SpecConfig(3, guided=True).guided is True
    assert SpecConfig(3, 2, 4, True, True) == SpecConfig(3, 2, 4, share_rows=True, guided=True)
    SpecConfig(3, guided=True).check(5)
    with pytest.raises(KarantaHipError, match="guided"):
        SpecConfig(3, guided="yes").check(5)


def spec_args(cfg, *more):
    return cli.parse_args(["serve", "/m", "--speculative-config", json.dumps(cfg), *more])


def test_cli_parses_guided():
    a = spec_args({"method": "ngram", "num_speculative_tokens": 3, "guided": True})
    assert a.speculative == (3, 2, 4) and a.speculative_guided is True and a.speculative_share_rows is False
    a = spec_args({"method": "ngram", "share_rows": True, "guided": True}, "--max-num-seqs", "20")
    assert a.speculative_guided is True and a.speculative_share_rows is True
    assert spec_args({"method": "ngram", "guided": False}).speculative_guided is False
    assert spec_args({"method": "ngram"}).speculative_guided is False
    assert cli.parse_args(["serve", "/m"]).speculative_guided is False
    assert cli.speculative_fields(json.dumps({"method": "ngram", "guided": True}), 8) == (3, 2, 4, False)     # four values, as before
    assert cli.speculative_guided(json.dumps({"method": "ngram", "guided": True})) is True


@pytest.mark.parametrize("value", [1, 0, "true", None, [True]])
def test_cli_refuses_a_guided_that_is_no_boolean(value, capsys):
    with pytest.raises(SystemExit):
        spec_args({"method": "ngram", "guided": value})
    assert "guided must be true or false" in capsys.readouterr().err


def test_bench_corpus_checks_the_key():
    from karanta_ocr_amd import bench_corpus
    with pytest.raises(SystemExit):
        bench_corpus.main(["--slots", "4", "--speculative-config", json.dumps({"method": "ngram", "guided": "on"})])


class GuidedSpecEngine(FakeSpecEngine):
    spec_guided = True


def test_the_scheduler_speculates_with_a_guided_request_in_a_slot():
    eng = GuidedSpecEngine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    res = sch.run([SlotRequest(Page([1], guide="[a-z]+"), 12), SlotRequest(Page([5]), 40)])
    assert [len(r.tokens) for r in res] == [12, 40]
    assert {k for k, _ in eng.log} == {"spec"} and sch.spec_steps > 0 and sch.plain_steps == 0


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.2), dict(logit_bias={3: 1.0}), dict(top_k=5)])
def test_other_per_token_state_still_forces_plain_chunks(kw):
    eng = GuidedSpecEngine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    res = sch.run([SlotRequest(Page([1], guide="[a-z]+", **kw), 6), SlotRequest(Page([5]), 40)])
    assert [len(r.tokens) for r in res] == [6, 40]
    kinds = [k for k, _ in eng.log]
    assert kinds.index("spec") >= 3


# ----------------------------------------------------------------------------- argument checks: KR_ERR_ARG, nothing launches
@pytest.fixture(scope="module")
def L():
    from karanta_ocr_amd import build
    from karanta_ocr_amd._lib import lib
    build.build(verbose=False)
    return lib()


def fake_args(**change):
    """kr_spec and kr_spec_guide whose pointers are non-null and never read: every call below must fail before its launch."""
    from karanta_ocr_amd._lib import Spec, SpecGuide
    p = 0x1000
    a = Spec(4, 3, 17, 2, 4, 64, p, 64, p, 4, 16, None, None, p, p, p, p, p, p, p, p, p, 64, PAD, V, p, 64, p, p)
    g = SpecGuide(p, p, p, 2 * ((V + 63) // 64), p, p, p, p)
    for k, v in change.items():
        setattr(a if hasattr(a, k) else g, k, v)
    return a, g


@pytest.mark.parametrize("change,why", [
    (dict(mask_words=9), "mask_words"), (dict(mask_words=0), "mask_words"), (dict(mask_words=-2), "mask_words"),
    (dict(mask_words=2), "mask_words"),                                    # even, but 64 bits do not cover the vocabulary
    (dict(guide_trans=None), "null"), (dict(guide_masks=None), "null"), (dict(guide_state=None), "null"), (dict(vocab_off=None), "null"),
    (dict(vocab_bytes=None), "null"), (dict(draft_state=None), "null"), (dict(ctx_before=None), "null"),
    (dict(rows=33), "rows"), (dict(k=0), "k="), (dict(slots=0), "slots"), (dict(ngram_max=9), "ngram"), (dict(draft_tok=None), "null"),
])
def test_entry_points_refuse_bad_arguments(L, change, why):
    a, g = fake_args(**change)
    with pytest.raises(KarantaHipError, match=why):
        L.kr_spec_guide_trim(C.byref(a), C.byref(g), 0x1000, 0)
    with pytest.raises(KarantaHipError, match=why):
        L.kr_spec_guide_rows(C.byref(a), C.byref(g), None, 0)
    with pytest.raises(KarantaHipError, match=why):
        L.kr_spec_guide_rows(C.byref(a), C.byref(g), 0x1000, 0)
    with pytest.raises(KarantaHipError, match=why):
        L.kr_spec_guide_advance(C.byref(a), C.byref(g), 0)


def test_entry_points_refuse_null_structs_and_layouts(L):
    a, g = fake_args()
    for call in (lambda x, y: L.kr_spec_guide_trim(x, y, 0x1000, 0), lambda x, y: L.kr_spec_guide_rows(x, y, None, 0),
                 lambda x, y: L.kr_spec_guide_advance(x, y, 0)):
        with pytest.raises(KarantaHipError, match="null"):
            call(None, C.byref(g))
        with pytest.raises(KarantaHipError, match="null"):
            call(C.byref(a), None)
    with pytest.raises(KarantaHipError, match="null n_count"):
        L.kr_spec_guide_trim(C.byref(a), C.byref(g), None, 0)
    # the static layout needs slots * (k + 1) rows; with a dealt map the same sizes are the shared layout's
    a, g = fake_args(slots=5)
    with pytest.raises(KarantaHipError, match="rows"):
        L.kr_spec_guide_rows(C.byref(a), C.byref(g), None, 0)
    assert L.kr_spec_guide_rows.raw(C.byref(a), C.byref(g), None, 0) == -1        # KR_ERR_ARG
