"""Speculative decoding with log-probabilities without a GPU: the rule of kr_logprobs_topk_rows — which tokens of a step record, on
which row and at which history index (tests/spec_logprobs_ref.py) — against a token-by-token simulation of plain steps built on
tests/spec_ref.simulate; the option's way through SpecConfig, the command line, the server's check and the slot scheduler; and the
argument checks of the three new entry points (host side: nothing launches).  (Fails on a tree without the feature: SpecConfig takes
no `logprobs`, the library exports none of the three.)"""
import ctypes as C
import json

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd._lib import KarantaHipError
from karanta_ocr_amd.request import SpecConfig
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy
from tests import spec_logprobs_ref as LR
from tests import spec_ref as R
from tests.test_spec_host_cpu import SCRIPT, FakeSpecEngine, Page

V, PAD = 120, 3


# ----------------------------------------------------------------------------- the rule, by hand
def test_records_by_hand():
    """K = 2, three slots in the static layout of a 17-row step: one token, three tokens the last of which finished the slot, a frozen
    slot."""
    got = LR.records(ctx_before=[10, 20, 30], ctx_len=[11, 23, 30], prompt_len=[8, 20, 5], finished=[0, 1, 1], k=2, rows=17, hist_len=40)
    assert got == [(0, 0, 0, 3), (1, 0, 1, 1), (1, 1, 4, 2)]
    # the same step under a dealt map: slot 1's drafts on rows 9 and 3; a draft without a row records nothing
    got = LR.records([10, 20, 30], [11, 23, 30], [8, 20, 5], [0, 0, 1], 2, 17, 40, draft_row=[[-1, -1], [9, 3], [-1, -1]])
    assert got == [(0, 0, 0, 3), (1, 0, 1, 1), (1, 1, 9, 2), (1, 2, 3, 3)]
    got = LR.records([10, 20, 30], [11, 23, 30], [8, 20, 5], [0, 0, 1], 2, 17, 40, draft_row=[[-1, -1], [9, -1], [-1, -1]])
    assert got == [(0, 0, 0, 3), (1, 0, 1, 1), (1, 1, 9, 2)]
    # the history ends: nothing at or past hist_len
    assert LR.records([10], [13], [8], [0], 2, 17, hist_len=5) == [(0, 0, 0, 3), (0, 1, 1, 4)]
    # a slot that finished on its only token records nothing
    assert LR.records([10], [11], [8], [1], 2, 17, 40) == []


# ----------------------------------------------------------------------------- closed loop against plain steps
@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("B,K", [(3, 2), (5, 3), (4, 1)])
def test_the_steps_record_what_plain_steps_record(B, K, seed):
    """Random continuations, drafts that are right up to a random point, EOS and stop ids at random places: over a run of speculative
    steps the rule records every (h, slot) exactly once, the ones one-token steps record, with the tokens of the history."""
    rng = np.random.default_rng(1000 * B + 10 * K + seed)
    T, steps, eos, stop = 64, 12, 7, 9             # T: past 1 + steps * (K + 1) tokens
    stops = {eos, stop}             # a stop id finishes a slot as an EOS does, and the controls' trim keeps it the last token of a step
    rows = max(17, B * (K + 1))
    seen = {}
    for s in range(B):
        truth = rng.integers(10, V, T).tolist()
        for pos in rng.choice(np.arange(2, T), 2, replace=False):
            if rng.random() < 0.6:
                truth[pos] = int(rng.choice([eos, stop]))
        script = list(truth)
        for pos in rng.choice(T, int(rng.integers(0, 12)), replace=False):
            script[pos] = 11 if script[pos] != 11 else 12
        plen, start = int(rng.integers(1, 9)), 1
        trace = []
        gen_end, _, _ = R.simulate(script, truth, K, steps, eos=stops, start=start, trace=trace)
        gen = start
        for nd, e in trace:
            ctx_before = plen + gen - 1
            fin = truth[gen + e - 1] in stops
            # one slot at a time through the rule, placed at column s of a B-slot step
            cb, cl, pl, fi = np.zeros(B, int), np.zeros(B, int), np.ones(B, int), np.ones(B, int)
            cb[s], cl[s], pl[s], fi[s] = ctx_before, ctx_before + e, plen, fin
            for slot, j, row, h in LR.records(cb, cl, pl, fi, K, rows, T):
                assert slot == s and row == (s if j == 0 else j * B + s) and j <= nd
                assert (h, s) not in seen, "a token recorded twice"
                seen[(h, s)] = truth[h]
            gen += e
        assert gen == gen_end
        want = LR.plain_records(truth, start, gen_end, stops)
        assert sorted(h for h, col in seen if col == s) == want
        assert all(seen[(h, s)] == truth[h] for h in want)
    assert seen


def test_a_finishing_token_is_the_only_one_left_out():
    truth, K = [20, 21, 22, 7, 30, 31], 3
    trace = []
    gen, _, _ = R.simulate(truth, truth, K, 3, eos={7}, start=1, trace=trace)
    assert trace == [(3, 3)] and gen == 4          # one step: tokens 1, 2 and the EOS at 3
    got = LR.records([4], [7], [4], [1], K, 17, 40)
    assert [h for _, _, _, h in got] == [1, 2] == LR.plain_records(truth, 1, gen, {7})


# ----------------------------------------------------------------------------- the option: SpecConfig, command line, server, scheduler
def test_spec_config_carries_the_option():
    assert SpecConfig().logprobs is False and SpecConfig(3, logprobs=True).logprobs is True
    assert SpecConfig(3, 2, 4, True, True, True, True) == SpecConfig(3, 2, 4, share_rows=True, guided=True, controls=True, logprobs=True)
    SpecConfig(3, logprobs=True).check(5)
    for bad in ("yes", 1, None):
        with pytest.raises(KarantaHipError, match="logprobs"):
            SpecConfig(3, logprobs=bad).check(5)


def spec_args(cfg, *more):
    return cli.parse_args(["serve", "/m", "--speculative-config", json.dumps(cfg), *more])


def test_cli_parses_logprobs():
    a = spec_args({"method": "ngram", "num_speculative_tokens": 3, "logprobs": True}, "--max-logprobs", "5")
    assert a.speculative == (3, 2, 4) and a.speculative_logprobs is True and a.max_logprobs == 5
    assert a.speculative_controls is False and a.speculative_guided is False
    a = spec_args({"method": "ngram", "share_rows": True, "guided": True, "controls": True, "logprobs": True}, "--max-num-seqs", "24",
                  "--max-logprobs", "20")
    assert a.speculative_logprobs and a.speculative_controls and a.speculative_guided and a.speculative_share_rows
    assert spec_args({"method": "ngram", "logprobs": True}).max_logprobs is None          # the key alone asks for no records
    assert spec_args({"method": "ngram", "logprobs": False}).speculative_logprobs is False
    assert spec_args({"method": "ngram"}).speculative_logprobs is False
    assert cli.parse_args(["serve", "/m"]).speculative_logprobs is False
    assert cli.speculative_fields(json.dumps({"method": "ngram", "logprobs": True}), 8) == (3, 2, 4, False)     # four values, as before
    assert cli.speculative_logprobs(json.dumps({"method": "ngram", "logprobs": True})) is True
    assert cli.speculative_controls(json.dumps({"method": "ngram", "logprobs": True})) is False


@pytest.mark.parametrize("value", [1, 0, "true", None, [True]])
def test_cli_refuses_a_logprobs_that_is_no_boolean(value, capsys):
    with pytest.raises(SystemExit):
        spec_args({"method": "ngram", "logprobs": value})
    assert "logprobs must be true or false" in capsys.readouterr().err


@pytest.mark.parametrize("cfg", [{"method": "ngram"}, {"method": "ngram", "logprobs": False},
                                 {"method": "ngram", "guided": True, "controls": True}])
def test_cli_still_refuses_max_logprobs_without_the_key(cfg, capsys):
    with pytest.raises(SystemExit):
        spec_args(cfg, "--max-logprobs", "5")
    assert "cannot be combined with --max-logprobs" in capsys.readouterr().err


def test_bench_corpus_checks_the_key():
    from karanta_ocr_amd import bench_corpus
    with pytest.raises(SystemExit):
        bench_corpus.main(["--slots", "4", "--speculative-config", json.dumps({"method": "ngram", "logprobs": "on"})])


def test_the_server_takes_max_logprobs_beside_speculation_on_such_an_engine_only():
    from karanta_ocr_amd.serving import LocalServer

    class Eng:
        K = 3

    class Rec(Eng):
        spec_logprobs = True

    with pytest.raises(ValueError, match="max_logprobs"):
        LocalServer(Eng(), None, continuous=True, speculative=True, max_logprobs=5)
    with pytest.raises(ValueError, match="continuous"):
        LocalServer(Rec(), None, continuous=False, speculative=True, max_logprobs=5)


class RecordingSpecEngine(FakeSpecEngine):
    spec_logprobs = True


def run_recording(eng):
    sch = SlotScheduler(eng, max_tokens_cap=8, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    sch.logprobs = 2                         # (the fake's begin_slots takes no logprobs: the scheduler's switch is set behind it)
    asked = []
    eng.slot_logprobs = lambda j, n, k: asked.append((j, n, k))
    res = sch.run([SlotRequest(Page([5], logprobs=2), 8), SlotRequest(Page([0], logprobs=1), 8)])
    return sch, res, asked


def test_spec_chunk_with_and_without_the_engines_flag():
    sch, res, asked = run_recording(RecordingSpecEngine(2, SCRIPT, 3, lambda j, s: 3))
    assert sch.spec_steps > 0 and sch.plain_steps == 0
    # [9] * 8 cut by max_tokens: 8 records; [1, 2, 3, 99] ends on the EOS: one record fewer than tokens
    assert [len(r.tokens) for r in res] == [8, 4] and sorted(asked) == [(0, 8, 2), (1, 3, 1)]
    sch, res, asked = run_recording(FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 3))
    assert sch.spec_steps == 0 and sch.plain_steps > 0
    assert [len(r.tokens) for r in res] == [8, 4] and sorted(asked) == [(0, 8, 2), (1, 3, 1)]


def test_spec_chunk_looks_at_nothing_else_of_the_scheduler():
    eng = RecordingSpecEngine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=8, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    assert sch._spec_chunk() is True
    sch.logprobs = 5
    assert sch._spec_chunk() is True
    eng.spec_logprobs = False
    assert sch._spec_chunk() is False
    sch.logprobs = None
    assert sch._spec_chunk() is True


# ----------------------------------------------------------------------------- argument checks: KR_ERR_ARG, nothing launches
@pytest.fixture(scope="module")
def L():
    from karanta_ocr_amd import build
    from karanta_ocr_amd._lib import lib
    build.build(verbose=False)
    return lib()


P = 0x1000          # a pointer that is not null and never read: every call below must fail before its launch


def fake_args(**change):
    from karanta_ocr_amd._lib import Spec, SpecLogprobs
    a = Spec(4, 3, 17, 2, 4, 64, P, 64, P, 4, 16, None, None, P, P, P, P, P, P, P, P, P, 64, PAD, V, P, 64, P, P)
    p = SpecLogprobs(5, 1, P, P, P, P, P, 16, 4, 20, P)
    for k, v in change.items():
        setattr(p if hasattr(p, k) else a, k, v)
    return a, p


@pytest.mark.parametrize("change,why", [
    (dict(part_val=None), "null"), (dict(part_idx=None), "null"), (dict(part_ms=None), "null"), (dict(out_lp=None), "null"),
    (dict(out_idx=None), "null"), (dict(ctx_before=None), "null"), (dict(k_top=-1), "k must be"), (dict(k_top=21), "k must be"),
    (dict(k_top=5, k_stride=4), "k must be"), (dict(n_part=0), "slice"), (dict(n_part=1025), "slice"), (dict(hist_len=0), "bad sizes"),
    (dict(hist_batch=3), "bad sizes"), (dict(rows=33), "rows"), (dict(k=0), "k="), (dict(k=32), "k="), (dict(slots=0), "slots"),
    (dict(ngram_max=9), "ngram"), (dict(history=None), "null"), (dict(finished=None), "null"), (dict(s_max=1), "s_max"),
    (dict(pad_id=V), "bad sizes"),
])
def test_logprobs_topk_rows_refuses_bad_arguments(L, change, why):
    a, p = fake_args(**change)
    for draft_row in (None, P):
        with pytest.raises(KarantaHipError, match=why):
            L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), draft_row, P, V, 0)
        assert L.kr_logprobs_topk_rows.raw(C.byref(a), C.byref(p), draft_row, P, V, 0) == -1        # KR_ERR_ARG


def test_logprobs_topk_rows_refuses_slices_tables_layouts_and_null_structs(L):
    a, p = fake_args(vocab=4097, n_part=1)
    with pytest.raises(KarantaHipError, match="slice"):             # ceil(vocab / n_part) <= 4096
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), None, P, 4097, 0)
    a, p = fake_args(n_part=1024, k_top=20)                         # 1024 * 20 * 8 bytes of candidates: past the merge's LDS
    with pytest.raises(KarantaHipError, match="LDS"):
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), None, P, V, 0)
    a, p = fake_args()
    with pytest.raises(KarantaHipError, match="bad sizes"):         # ld_logits below the vocabulary
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), None, P, V - 1, 0)
    with pytest.raises(KarantaHipError, match="null"):
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), None, None, V, 0)
    with pytest.raises(KarantaHipError, match="null"):
        L.kr_logprobs_topk_rows(None, C.byref(p), None, P, V, 0)
    with pytest.raises(KarantaHipError, match="null"):
        L.kr_logprobs_topk_rows(C.byref(a), None, None, P, V, 0)
    # the static layout needs slots * (k + 1) rows; with a dealt map the same sizes are the shared layout's: refused further on
    a, p = fake_args(slots=5, hist_stride=5, hist_batch=5, out_lp=None)
    with pytest.raises(KarantaHipError, match="rows"):
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), None, P, V, 0)
    with pytest.raises(KarantaHipError, match="null pointer"):
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), P, P, V, 0)


def test_spec_mark_and_restore_rows_refuse_bad_arguments(L):
    a, _ = fake_args()
    with pytest.raises(KarantaHipError, match="null ctx_before"):
        L.kr_spec_mark(C.byref(a), None, 0)
    with pytest.raises(KarantaHipError, match="null"):
        L.kr_spec_mark(None, P, 0)
    for change, why in ((dict(rows=33), "rows"), (dict(slots=0), "slots"), (dict(k=0), "k="), (dict(ctx_len=None), "null")):
        a, _ = fake_args(**change)
        with pytest.raises(KarantaHipError, match=why):
            L.kr_spec_mark(C.byref(a), P, 0)
    good = dict(logits=P, ld=V, vocab=V, ids=P, meta=P, saved=P, batch=17, row_slot=P, slots=4)
    for change, why in ((dict(logits=None), "null"), (dict(ids=None), "null"), (dict(meta=None), "null"), (dict(saved=None), "null"),
                        (dict(row_slot=None), "null"), (dict(ld=V - 1), "bad sizes"), (dict(vocab=0), "bad sizes"),
                        (dict(batch=0), "bad sizes"), (dict(batch=33), "rows"), (dict(slots=0), "slots"), (dict(slots=18), "slots")):
        kw = {**good, **change}
        args = (kw["logits"], kw["ld"], kw["vocab"], kw["ids"], kw["meta"], kw["saved"], kw["batch"], kw["row_slot"], kw["slots"], 0)
        with pytest.raises(KarantaHipError, match=why):
            L.kr_logits_restore_rows(*args)
        assert L.kr_logits_restore_rows.raw(*args) == -1
