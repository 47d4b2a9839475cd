"""Speculative decoding under sampling controls and logit adjustments without a GPU: the numpy restatement of kr_spec_controls_trim /
_rows / _count and of the counts a draft row reads (tests/spec_controls_ref.py) on hand-worked cases and in a closed loop — a
controlled speculative step with arbitrary drafts leaves the tokens, the output counts, `finished` and the history that as many plain
controlled steps leave — the option's way through SpecConfig, the command line and the slot scheduler, and the argument checks of
the new entry points (host side: nothing launches).  (Fails on a tree without the feature: SpecConfig takes no `controls`.)"""
import ctypes as C
import json
import zlib

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd._lib import KarantaHipError
from karanta_ocr_amd.request import SpecConfig
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy
from tests import adjust_cases as A
from tests import sampling_ref as S
from tests import spec_controls_ref as X
from tests import spec_deal_ref as D
from tests import spec_ref as R
from tests.test_spec_host_cpu import SCRIPT, FakeSpecEngine, Page

V, PAD, EOS = 120, 3, 7


# ----------------------------------------------------------------------------- the restatement, by hand
def table1(entries, min_tokens=0):
    return A.tables(1, [(entries, min_tokens)])


def trim1(entries, drafts, n=None, fin=0, min_tokens=0):
    """One slot, K = 3: (n_count, draft_tok) after the trim."""
    ids, _, flags, meta = table1(entries, min_tokens)
    d = np.full((1, 3), PAD, np.int32)
    d[0, :len(drafts)] = drafts
    nc, dt, cb = X.trim(ids, flags, meta, [fin], [41], [len(drafts) if n is None else n], d, PAD)
    assert cb.tolist() == [41]
    return int(nc[0]), dt[0].tolist()


def test_trim_by_hand():
    stop = [(50, 0.0, 1), (60, 2.0, 1), (70, -5.0, 0)]          # two stop entries (one with a bias), one bias that is no stop
    assert trim1(stop, [10, 11, 12]) == (3, [10, 11, 12])
    # a stop id at every depth: the count is cut in front of it, the tokens from there on are the pad token
    assert trim1(stop, [50, 11, 12]) == (0, [PAD] * 3)
    assert trim1(stop, [10, 60, 12]) == (1, [10, PAD, PAD])
    assert trim1(stop, [10, 11, 50]) == (2, [10, 11, PAD])
    assert trim1(stop, [10, 60, 50]) == (1, [10, PAD, PAD])      # the first one decides
    # a biased token that is no stop entry stays; so does a stop id beyond the count
    assert trim1(stop, [70, 70, 70]) == (3, [70, 70, 70])
    assert trim1(stop, [10, 11, 50], n=2) == (2, [10, 11, 50])
    # min_tokens does not matter to the cut: the EOS of a slot with min_tokens is a stop entry, before and after the floor
    assert trim1([(EOS, 0.0, 1)], [10, EOS, 12], min_tokens=9) == (1, [10, PAD, PAD])
    # an unadjusted slot (empty table) and a finished slot keep everything
    assert trim1([], [50, EOS, 60]) == (3, [50, EOS, 60])
    assert trim1(stop, [50, 60, 70], fin=1) == (3, [50, 60, 70])


def test_depth_rows_by_hand():
    B, k, Rr = 3, 2, 17
    fin = np.zeros(Rr, np.int32)
    # static layout: row j * B + slot.  Slot 0 keeps one draft, slot 1 two, slot 2 none
    depth, f = X.depth_rows(fin, [1, 2, 0], B, k, Rr)
    assert depth.tolist() == [0, 0, 0, 1, 1, 0, 0, 2, 0] + [0] * 8
    assert f.tolist() == [0, 0, 0, 0, 0, 1, 1, 0, 1] + [0] * 8
    # the dealt map, not monotonic: slot 2's depth 1 on row 3, slot 0's depths on rows 5 and 4; `finished` is the deal's
    row = np.asarray([[5, 4], [-1, -1], [3, -1]])
    depth, f = X.depth_rows(fin, [2, 0, 1], B, k, Rr, draft_row=row)
    assert depth.tolist() == [0, 0, 0, 1, 2, 1] + [0] * 11 and not f.any()
    # a map that names a row beyond the dealt depth: depth 0
    depth, _ = X.depth_rows(fin, [1, 0, 1], B, k, Rr, draft_row=row)
    assert depth.tolist() == [0, 0, 0, 1, 0, 1] + [0] * 11


def test_effective_counts_and_count_update_by_hand():
    c = np.zeros(10, np.int32)
    c[4] = 2
    assert X.effective_counts(c, [4, 4, 9], 0).tolist() == c.tolist()
    assert X.effective_counts(c, [4, 4, 9], 2)[4] == 4 and X.effective_counts(c, [4, 4, 9], 2)[9] == 0
    assert X.effective_counts(c, [4, 4, 9], 3)[9] == 1 and c[4] == 2
    # slot 0 emitted nothing (frozen), slot 1 one token, slot 2 K + 1 = 4 tokens two of them equal, slot 3 ends on a stop id
    plen = np.asarray([5, 5, 5, 5])
    hist = np.full((12, 4), PAD, np.int32)
    hist[2, 1] = 8
    hist[0:4, 2] = [6, 1, 6, 2]
    hist[1:3, 3] = [9, 0]
    before, ctx = np.asarray([7, 6, 4, 5]), np.asarray([7, 7, 8, 7])
    out = X.count_update(np.zeros((4, 10), np.int32), before, ctx, plen, hist, 3)
    assert out[0].sum() == 0 and out[1].tolist() == [0] * 8 + [1, 0]
    assert out[2].tolist() == [0, 1, 1, 0, 0, 0, 2, 0, 0, 0] and out[3].tolist() == [1] + [0] * 8 + [1]


def test_simulate_cuts_at_stop_entries_and_frees_rows():
    truth = [[1, 2, 3, 4, 5, 6, 7, 8, 9]] * 2
    # slot 0's script is right but token 4 is its stop entry: drafts 2, 3 are taken, 4 is cut, the step emits 1 + 2 tokens, then
    # the model itself chooses 4 and the slot finishes; slot 1 has no stop entry and takes K + 1 tokens a step
    trace = []
    out = X.simulate(truth, truth, [{4}, set()], 3, 2, trace=trace)
    assert trace[0] == ([3, 3], [2, 3], [2, 3]) and out == [(4, 2, 2), (9, 6, 6)]
    # 20 slots on 32 rows: 12 rows; the slots want 3 each; slot 0's cut at depth 1 frees a row for depth 1 of another slot
    tr = [[1, 2, 3, 4, 5]] * 20
    full, cut = [], []
    X.simulate(tr, tr, [set()] * 20, 3, 1, rows=32, trace=full)
    X.simulate(tr, tr, [{2}] + [set()] * 19, 3, 1, rows=32, trace=cut)
    assert full[0][2] == [1] * 12 + [0] * 8 and cut[0][2] == [0] + [1] * 12 + [0] * 7


# ----------------------------------------------------------------------------- the closed loop
def logits_of(seq) -> np.ndarray:
    """The "model": fp32 logits that are a deterministic function of the sequence so far."""
    rng = np.random.default_rng(zlib.crc32(np.asarray(seq, np.int64).tobytes()))
    return (rng.standard_normal(V) * 3).astype(np.float32)


# (T, top_k, top_p, min_p, repetition, frequency, presence, bias, min_tokens, stop ids)
KINDS = [
    (1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, {}, 0, ()),                       # neutral sampled
    (0.9, 6, 1.0, 0.0, 1.0, 0.0, 0.0, {}, 0, ()),                       # top_k
    (1.0, 0, 0.8, 0.0, 1.3, 0.0, 0.0, {}, 0, ()),                       # top_p + repetition
    (0.0, 0, 1.0, 0.0, 1.0, 1.5, 0.5, {}, 0, ()),                       # greedy, frequency + presence
    (1.0, 0, 1.0, 0.05, 1.0, 0.0, 0.0, {EOS: 6.0}, 5, ()),              # an EOS that wants out, held back by min_tokens
    (0.8, 0, 1.0, 0.0, 1.0, 0.0, 0.0, {40: 5.0, 41: -100.0}, 0, (40, 55)),   # a favoured stop id
    (0.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, {}, 0, ()),                       # neutral greedy
    (1.1, 8, 0.9, 0.02, 1.2, 0.7, 0.3, {12: 3.0}, 3, (12,)),            # everything
]


class Slots:
    """The sampler state of B slots on the host, in the device's shapes."""

    def __init__(self, B, rng):
        self.B = B
        self.kind = [KINDS[b % len(KINDS)] for b in range(B)]
        self.plen = np.asarray([4 + b % 5 for b in range(B)])
        self.prompts = [rng.integers(0, V, int(n)).tolist() for n in self.plen]
        self.seed = [int(s) for s in rng.integers(0, 2 ** 32, B, dtype=np.uint64)]
        rows = []
        for k in self.kind:
            ent = {t: [v, 0] for t, v in k[7].items()}
            for t in list(k[9]) + ([EOS] if k[8] > 0 else []):
                ent.setdefault(t, [0.0, 0])[1] = 1
            rows.append(([(t, v, f) for t, (v, f) in ent.items()], k[8]))
        self.ids, self.vals, self.flags, self.meta = A.tables(B, rows)
        self.stops = [X.stop_entries(self.ids, self.flags, self.meta, b) for b in range(B)]

    def choose(self, b, seq, n, counts):
        """The token slot b chooses behind `seq` as its n-th generated token, with the output counts `counts`: kr_logits_adjust,
        then the sampler (tests/adjust_cases.adjust_ref, tests/sampling_ref.sample_step)."""
        T, top_k, top_p, min_p, rep, freq, pres = self.kind[b][:7]
        row = A.adjust_ref(logits_of(seq), self.ids[b], self.vals[b], self.flags[b], self.meta[b, 0], self.meta[b, 1], n)
        out = np.repeat(np.arange(V), counts)
        return S.sample_step(row, T, self.seed[b], n, self.prompts[b], out, V, None, top_k, top_p, min_p, rep, freq, pres)[0]


@pytest.mark.parametrize("B,K,rows,shared", [(8, 3, 32, False), (4, 1, 17, False), (3, 3, 17, True), (20, 3, 32, True)])
def test_a_controlled_speculative_step_equals_as_many_plain_controlled_steps(B, K, rows, shared):
    rng = np.random.default_rng(B * 100 + K)
    flags, T, steps = 2, 64, 9
    sl = Slots(B, rng)
    plen, prompts = sl.plen, sl.prompts
    # ---- the plain controlled run: the truth, with `finished` behind every generated token
    hist, ctx, fin = np.full((T, B), -1, np.int32), plen - 1, np.zeros(B, np.int32)
    counts = np.zeros((B, V), np.int32)
    after = [{0: 0} for _ in range(B)]
    for _ in range(1 + steps * (K + 1)):
        tok = np.full(B, PAD, np.int32)
        live = [not f for f in fin]
        for b in range(B):
            if fin[b]:
                continue
            n = int(ctx[b] + 1 - plen[b])
            t = sl.choose(b, prompts[b] + hist[:n, b].tolist(), n, counts[b])
            tok[b] = R.greedy_step(t, hist, b, ctx, plen, fin, (EOS,), PAD, flags)
        X.stop_tokens(tok, sl.ids, sl.flags, sl.meta, fin, flags)
        for b in range(B):
            if live[b]:
                counts[b, tok[b]] += 1           # kr_sample_count: live is taken before the token
                after[b][int(ctx[b] + 1 - plen[b])] = int(fin[b])
    truth, n_truth = hist, ctx + 1 - plen
    by_stop = [b for b in range(B) if fin[b] and int(truth[n_truth[b] - 1, b]) != EOS]
    by_eos = [b for b in range(B) if fin[b] and int(truth[n_truth[b] - 1, b]) == EOS]
    if B >= 8:
        assert by_stop and by_eos, "a slot should end on its stop id and one on the EOS min_tokens held back"
        for b in by_eos:
            assert n_truth[b] > sl.kind[b][8], "min_tokens holds the EOS back"
    # ---- the speculative run from the state behind the first token
    hist, ctx, fin = np.full((T, B), -1, np.int32), plen.copy(), np.zeros(B, np.int32)
    hist[0] = truth[0]
    counts = np.zeros((B, V), np.int32)
    for b in range(B):
        fin[b] = after[b][1]
        counts[b, truth[0, b]] += 1
    trimmed = accepted = deep = early_eos = 0
    for _ in range(steps):
        gen = ctx + 1 - plen
        draft = np.full((B, K), PAD, np.int32)
        n_count = np.zeros(B, np.int32)
        for b in range(B):
            if fin[b]:
                continue
            n_count[b] = rng.integers(0, K + 1)
            for j in range(int(n_count[b])):
                right = gen[b] + j < n_truth[b] and rng.random() < 0.7
                wrong = [EOS, int(rng.integers(0, V))] + sorted(sl.stops[b])
                draft[b, j] = truth[gen[b] + j, b] if right else wrong[int(rng.integers(0, len(wrong)))]
                early_eos += draft[b, j] == EOS and gen[b] + j < sl.kind[b][8]
        n0 = n_count.copy()
        n_count, draft, before = X.trim(sl.ids, sl.flags, sl.meta, fin, ctx, n_count, draft, PAD)
        trimmed += int((n0 - n_count).sum())
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
        depth, fin_rows = X.depth_rows(fin_rows, n_draft, B, K, rows, draft_row=row)
        assert (depth[:B] == 0).all() and int((depth > 0).sum()) == int(n_draft.sum())
        # every live row chooses its token with its slot's state behind its drafts; the other rows hold a token nobody may read
        idx = np.full((rows, 1), 1, np.int32)
        for b in range(B):
            seq = prompts[b] + hist[:gen[b], b].tolist()
            for j in range(0, int(n_draft[b]) + 1):
                r = b if j == 0 else (j * B + b if row is None else int(row[b, j - 1]))
                assert depth[r] == j and (fin_rows[r] == fin[b] if j == 0 else fin_rows[r] == 0)
                idx[r, 0] = sl.choose(b, seq + draft[b, :j].tolist(), int(gen[b]) + j, X.effective_counts(counts[b], draft[b], depth[r]))
        val = np.ones((rows, 1), np.float32)
        tok = np.zeros(B, np.int32)
        if shared:
            tok, _, acc = D.accept_rows(val, idx, n_draft, draft, row, hist, ctx, plen, fin, (EOS,), PAD, flags, K)
        else:
            tok, _, acc = R.accept(val, idx, n_draft, draft, hist, ctx, plen, fin, (EOS,), PAD, flags, K)
        accepted += int(acc.sum())
        deep += int((acc >= 2).sum())
        X.stop_tokens(tok, sl.ids, sl.flags, sl.meta, fin, flags)
        counts = X.count_update(counts, before, ctx, plen, hist, K)
        for b in range(B):
            n = int(ctx[b] + 1 - plen[b])
            assert n >= gen[b] + (0 if after[b][int(gen[b])] else 1)
            np.testing.assert_array_equal(hist[:n, b], truth[:n, b], err_msg=f"slot {b}: tokens")
            assert (hist[n:, b] == -1).all(), f"slot {b}: history behind the emitted tokens"
            assert int(fin[b]) == after[b][n], f"slot {b}: finished after {n} tokens"
            np.testing.assert_array_equal(counts[b], np.bincount(truth[:n, b], minlength=V), err_msg=f"slot {b}: counts")
    assert accepted > 0 and (K == 1 or deep > 0)
    if B >= 8:
        assert trimmed > 0 and early_eos > 0


def test_a_row_that_ignores_its_drafts_chooses_another_token():
    """The closed loop is decisive: with the slot's counts alone (no drafts added) some draft row's choice differs."""
    rng = np.random.default_rng(5)
    sl = Slots(8, rng)
    differs = 0
    for b in (2, 3, 7):                        # the slots with penalties
        for trial in range(6):
            seq = sl.prompts[b] + rng.integers(0, V, 6).tolist()
            # a draft repeated twice that is also the model's favourite behind it: the penalties have something to move
            hits = [t for t in range(V) if int(np.argmax(logits_of(seq + [t, t]))) == t]
            c = np.zeros(V, np.int32)
            for t in hits:
                differs += sl.choose(b, seq + [t, t], 8, X.effective_counts(c, [t, t], 2)) != sl.choose(b, seq + [t, t], 8, c)
    assert differs > 0


# ----------------------------------------------------------------------------- the option: SpecConfig, command line, scheduler
def test_spec_config_carries_the_option():
    assert SpecConfig().controls is False and SpecConfig(3, controls=True).controls is True
    assert SpecConfig(3, 2, 4, True, True, True) == SpecConfig(3, 2, 4, share_rows=True, guided=True, controls=True)
    SpecConfig(3, controls=True).check(5)
    SpecConfig(3, share_rows=True, guided=True, controls=True).check(24)
    with pytest.raises(KarantaHipError, match="controls"):
        SpecConfig(3, controls="yes").check(5)
    with pytest.raises(KarantaHipError, match="controls"):
        SpecConfig(3, controls=1).check(5)


def spec_args(cfg, *more):
    return cli.parse_args(["serve", "/m", "--speculative-config", json.dumps(cfg), *more])


def test_cli_parses_controls():
    a = spec_args({"method": "ngram", "num_speculative_tokens": 3, "controls": True})
    assert a.speculative == (3, 2, 4) and a.speculative_controls is True and a.speculative_guided is False
    a = spec_args({"method": "ngram", "share_rows": True, "guided": True, "controls": True}, "--max-num-seqs", "24")
    assert a.speculative_controls is True and a.speculative_guided is True and a.speculative_share_rows is True
    assert spec_args({"method": "ngram", "controls": False}).speculative_controls is False
    assert spec_args({"method": "ngram"}).speculative_controls is False
    assert cli.parse_args(["serve", "/m"]).speculative_controls is False
    assert cli.speculative_fields(json.dumps({"method": "ngram", "controls": True}), 8) == (3, 2, 4, False)     # four values, as before
    assert cli.speculative_controls(json.dumps({"method": "ngram", "controls": True})) is True
    assert cli.speculative_guided(json.dumps({"method": "ngram", "controls": True})) is False


@pytest.mark.parametrize("value", [1, 0, "true", None, [True]])
def test_cli_refuses_a_controls_that_is_no_boolean(value, capsys):
    with pytest.raises(SystemExit):
        spec_args({"method": "ngram", "controls": value})
    assert "controls must be true or false" in capsys.readouterr().err


def test_cli_still_refuses_log_probabilities(capsys):
    with pytest.raises(SystemExit):
        spec_args({"method": "ngram", "controls": True}, "--max-logprobs", "5")
    assert "--max-logprobs" in capsys.readouterr().err


def test_bench_corpus_checks_the_key():
    from karanta_ocr_amd import bench_corpus
    with pytest.raises(SystemExit):
        bench_corpus.main(["--slots", "4", "--speculative-config", json.dumps({"method": "ngram", "controls": "on"})])


class ControlsSpecEngine(FakeSpecEngine):
    spec_controls = True


class BothSpecEngine(FakeSpecEngine):
    spec_controls = spec_guided = True


TRAFFIC = [(dict(top_p=0.9), 6), ({}, 40), (dict(logit_bias={3: 1.0}), 9), (dict(repetition_penalty=1.2, stop_token_ids=(8,)), 5),
           (dict(min_tokens=2), 7), (dict(top_k=5, frequency_penalty=0.5), 8)]


def run_traffic(eng):
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    res = sch.run([SlotRequest(Page([1 if kw else 5], **kw), n, tag=i) for i, (kw, n) in enumerate(TRAFFIC)])
    assert [len(r.tokens) for r in res] == [n for _, n in TRAFFIC] and all(r.error is None for r in res)
    return sch, [k for k, _ in eng.log]


def test_the_scheduler_speculates_while_controlled_requests_come_and_go():
    sch, kinds = run_traffic(ControlsSpecEngine(2, SCRIPT, 3, lambda j, s: 3))
    assert set(kinds) == {"spec"} and sch.spec_steps > 0 and sch.plain_steps == 0


def test_without_the_option_the_same_traffic_runs_plain_chunks():
    sch, kinds = run_traffic(FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 3))
    # controlled requests pass through one of the two slots until the last of them has left: plain chunks; then the long one speculates
    n_plain = kinds.index("spec")
    assert n_plain >= 5 and set(kinds[n_plain:]) == {"spec"} and sch.plain_steps == 2 * n_plain


@pytest.mark.parametrize("engine,kw,spec", [
    (ControlsSpecEngine, dict(guide="[a-z]+", top_k=5), False),       # guided requests need SpecConfig(guided=True) as before
    (BothSpecEngine, dict(guide="[a-z]+", top_k=5, logit_bias={3: 1.0}), True),
    (ControlsSpecEngine, dict(logit_bias={3: 1.0}), True),
])
def test_the_two_options_are_independent(engine, kw, spec):
    eng = engine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    res = sch.run([SlotRequest(Page([1], **kw), 6), SlotRequest(Page([5]), 40)])
    assert [len(r.tokens) for r in res] == [6, 40]
    kinds = [k for k, _ in eng.log]
    assert (set(kinds) == {"spec"}) if spec else kinds.index("spec") >= 3


def test_log_probabilities_still_force_plain_chunks():
    eng = ControlsSpecEngine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=8, chunk=2, speculative=True)
    sch.logprobs = 2
    eng.slot_logprobs = lambda j, n, k: None
    sch.run([SlotRequest(Page([5], top_p=0.9), 8)])
    assert sch.spec_steps == 0 and sch.plain_steps > 0


# ----------------------------------------------------------------------------- argument checks: KR_ERR_ARG, nothing launches
@pytest.fixture(scope="module")
def L():
    from karanta_ocr_amd import build
    from karanta_ocr_amd._lib import lib
    build.build(verbose=False)
    return lib()


P = 0x1000          # a pointer that is not null and never read: every call below must fail before its launch


def fake_args(**change):
    from karanta_ocr_amd._lib import Spec, SpecControls
    a = Spec(4, 3, 17, 2, 4, 64, P, 64, P, 4, 16, None, None, P, P, P, P, P, P, P, P, P, 64, PAD, V, P, 64, P, P)
    c = SpecControls(P, P, P, P, V, P, P)
    for k, v in change.items():
        setattr(a if hasattr(a, k) else c, k, v)
    return a, c


@pytest.mark.parametrize("change,why", [
    (dict(adj_ids=None), "null"), (dict(adj_flag=None), "null"), (dict(adj_meta=None), "null"), (dict(counts=None), "null"),
    (dict(depth=None), "null"), (dict(ctx_before=None), "null"), (dict(ld_counts=V - 1), "ld_counts"), (dict(ld_counts=0), "ld_counts"),
    (dict(rows=33), "rows"), (dict(k=0), "k="), (dict(k=32), "k="), (dict(slots=0), "slots"), (dict(ngram_max=9), "ngram"),
    (dict(draft_tok=None), "null"), (dict(history=None), "null"), (dict(s_max=1), "s_max"), (dict(pad_id=V), "bad sizes"),
])
def test_the_three_launches_refuse_bad_arguments(L, change, why):
    a, c = fake_args(**change)
    for call in (lambda: L.kr_spec_controls_trim(C.byref(a), C.byref(c), P, 0), lambda: L.kr_spec_controls_rows(C.byref(a), C.byref(c), None, 0),
                 lambda: L.kr_spec_controls_rows(C.byref(a), C.byref(c), P, 0), lambda: L.kr_spec_controls_count(C.byref(a), C.byref(c), 0)):
        with pytest.raises(KarantaHipError, match=why):
            call()


def test_the_three_launches_refuse_null_structs_and_layouts(L):
    a, c = fake_args()
    for call in (lambda x, y: L.kr_spec_controls_trim(x, y, P, 0), lambda x, y: L.kr_spec_controls_rows(x, y, None, 0),
                 lambda x, y: L.kr_spec_controls_count(x, y, 0)):
        with pytest.raises(KarantaHipError, match="null"):
            call(None, C.byref(c))
        with pytest.raises(KarantaHipError, match="null"):
            call(C.byref(a), None)
    with pytest.raises(KarantaHipError, match="null n_count"):
        L.kr_spec_controls_trim(C.byref(a), C.byref(c), None, 0)
    # the static layout needs slots * (k + 1) rows; with a dealt map the same sizes are the shared layout's
    a, c = fake_args(slots=5)
    with pytest.raises(KarantaHipError, match="rows"):
        L.kr_spec_controls_rows(C.byref(a), C.byref(c), None, 0)
    assert L.kr_spec_controls_rows.raw(C.byref(a), C.byref(c), None, 0) == -1        # KR_ERR_ARG


def rows_calls(L, row_slot=P, depth=P, draft=P, k=3, slots=4, batch=17, vocab=V, ld=V):
    W = (V + 31) // 32
    return [
        lambda: L.kr_logits_adjust_rows(P, ld, vocab, P, P, P, P, P, P, P, batch, row_slot, slots, 0),
        lambda: L.kr_sample_threshold_rows(P, ld, vocab, P, P, P, V, P, W, None, None, 0, P, 2, P, V, P, P, batch, row_slot, depth, draft,
                                           k, slots, 0),
        lambda: L.kr_gumbel_argmax_processed_rows(P, ld, vocab, P, P, P, P, P, P, 8, batch, None, None, 0, 0, P, P, V, P, W, P, row_slot,
                                                  depth, draft, k, slots, 0),
    ]


@pytest.mark.parametrize("kw,why,which", [
    (dict(row_slot=None), "null", (0, 1, 2)), (dict(depth=None), "null", (1, 2)), (dict(draft=None), "null", (1, 2)),
    (dict(k=0), "k=", (1, 2)), (dict(k=32), "k=", (1, 2)), (dict(slots=0), "slots", (0, 1, 2)), (dict(slots=18), "slots", (0, 1, 2)),
    (dict(batch=33), "rows", (0, 1, 2)), (dict(batch=0), "bad sizes", (0, 1, 2)), (dict(ld=V - 1), "bad sizes", (0, 1, 2)),
    (dict(vocab=0), "bad sizes", (0, 1, 2)),
])
def test_the_row_mapped_launches_refuse_bad_arguments(L, kw, why, which):
    calls = rows_calls(L, **kw)
    for i in which:
        with pytest.raises(KarantaHipError, match=why):
            calls[i]()
