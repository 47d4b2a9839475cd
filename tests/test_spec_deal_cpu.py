"""Shared draft rows without a GPU: the numpy restatement (tests/spec_deal_ref.py) on hand-worked cases, SpecConfig's and the command
line's share_rows, and the scheduler at 20 slots on a fake engine that deals a step's spare rows."""
import json

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd._lib import KarantaHipError
from karanta_ocr_amd.request import SpecConfig
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy
from tests import spec_deal_ref as D
from tests import spec_ref as R
from tests.test_spec_host_cpu import SCRIPT, FakeSpecEngine, Page, expect, spec_args

S_MAX, PAD = 64, 3


def dealt(n_want, rows, k=3, fin=None, ctx=None):
    B = len(n_want)
    fin = np.zeros(B, np.int32) if fin is None else np.asarray(fin, np.int32)
    ctx = np.full(B, 10, np.int32) if ctx is None else np.asarray(ctx, np.int32)
    tok = 100 + 10 * np.arange(B)[:, None] + np.arange(k)[None, :]            # draft j of slot b: 100 + 10 b + (j - 1)
    plen = np.full(B, 4, np.int32)
    out = D.deal(np.asarray(n_want), tok, ctx, plen, fin, np.linspace(0.1, 0.9, B).astype(np.float32), 50 + np.arange(B, dtype=np.uint32),
                 k, rows, S_MAX, PAD)
    # what holds in every case: the slots' own entries untouched, every other row either one draft's or parked
    assert out["slot"][:B].tolist() == list(range(B)) and (out["ctx"][:B] == ctx).all() and (out["fin"][:B] == fin).all()
    owned = {int(r) for r in out["draft_row"].ravel() if r >= 0}
    assert len(owned) == int((out["draft_row"] >= 0).sum()) and all(B <= r < rows for r in owned)
    for r in range(B, rows):
        if r not in owned:
            assert (out["slot"][r], out["ctx"][r], out["plen"][r], out["fin"][r], out["tok"][r]) == (0, S_MAX - 1, S_MAX - 1, 1, PAD)
            assert out["temp"][r] == 0 and out["seed"][r] == 0
    return out


# ----------------------------------------------------------------------------- the dealing rule
def test_everything_fits():
    out = dealt([3, 0, 2, 1, 0], 17)
    assert out["draft_row"].tolist() == [[5, 8, 10], [-1, -1, -1], [6, 9, -1], [7, -1, -1], [-1, -1, -1]]
    assert out["n_draft"].tolist() == [3, 0, 2, 1, 0]
    assert out["slot"][5:11].tolist() == [0, 2, 3, 0, 2, 0] and out["ctx"][5:11].tolist() == [11, 11, 11, 12, 12, 13]
    assert out["tok"][5:11].tolist() == [100, 120, 130, 101, 121, 102] and out["fin"][5:11].tolist() == [0] * 6
    assert out["seed"][5:11].tolist() == [50, 52, 53, 50, 52, 50] and out["plen"][5:11].tolist() == [4] * 6
    assert out["fin"][11:].tolist() == [1] * 6 and out["tok"][11:].tolist() == [PAD] * 6


def test_the_budget_ends_in_depth_one_so_slot_order_decides():
    out = dealt([2] * 20, 32, k=2)
    assert out["n_draft"].tolist() == [1] * 12 + [0] * 8
    assert out["draft_row"][:, 0].tolist() == list(range(20, 32)) + [-1] * 8 and (out["draft_row"][:, 1] == -1).all()
    assert out["slot"][20:].tolist() == list(range(12)) and out["fin"][20:].tolist() == [0] * 12


def test_the_budget_ends_in_the_middle_of_depth_two():
    out = dealt([3, 3, 3, 3], 10)
    assert out["draft_row"].tolist() == [[4, 8, -1], [5, 9, -1], [6, -1, -1], [7, -1, -1]]
    assert out["n_draft"].tolist() == [2, 2, 1, 1]
    assert out["ctx"][4:].tolist() == [11, 11, 11, 11, 12, 12] and out["tok"][4:].tolist() == [100, 110, 120, 130, 101, 111]


def test_finished_slots_and_slots_that_found_nothing_take_no_row():
    out = dealt([3, 3, 0, 1, 2], 17, fin=[1, 0, 0, 0, 1])
    assert out["draft_row"].tolist() == [[-1] * 3, [5, 7, 8], [-1] * 3, [6, -1, -1], [-1] * 3]
    assert out["n_draft"].tolist() == [0, 3, 0, 1, 0]
    assert out["slot"][5:9].tolist() == [1, 3, 1, 1] and out["fin"][9:].tolist() == [1] * 8


def test_one_spare_row_goes_to_the_first_slot_that_wants_one():
    want = [0] * 31
    want[2], want[7] = 2, 3
    out = dealt(want, 32)
    assert out["n_draft"].tolist() == [0, 0, 1] + [0] * 28
    assert out["draft_row"][2].tolist() == [31, -1, -1] and (np.delete(out["draft_row"], 2, axis=0) == -1).all()
    assert (out["slot"][31], out["ctx"][31], out["tok"][31], out["fin"][31]) == (2, 11, 120, 0)
    # nobody wants it: it is parked
    out = dealt([0] * 31, 32)
    assert (out["draft_row"] == -1).all() and out["fin"][31] == 1 and out["ctx"][31] == S_MAX - 1


def test_lookup_is_the_proposers_search_without_row_state():
    """n_want / draft_tok of scripted and looked-up slots, the s_max and vocabulary clamps, a finished slot."""
    prompts = [np.asarray(p, np.int32) for p in ([10, 11, 12, 13, 14, 15, 11, 12], [1, 2, 3], [1, 2, 3], [10, 11, 12, 13, 10, 11],
                                                 list(range(200, 260)) + [200, 201])]
    plen = np.asarray([len(p) for p in prompts], np.int32)
    hist = np.full((8, 5), -1, np.int32)
    hist[0, 1], hist[0, 2] = 4, 4
    ctx = plen - 1 + np.asarray([0, 1, 1, 0, 0])
    fin = np.asarray([0, 0, 0, 1, 0], np.int32)
    scripts = [None, [4, 8, 9, 7, 7], [4, 8, 999, 8], None, None]
    n_want, tok = D.lookup(prompts, hist, ctx, plen, fin, 3, 2, 4, S_MAX, PAD, 300, scripts)
    assert n_want.tolist() == [3, 3, 1, 0, 2]            # slot 4: ctx = s_max - 3, room for two
    assert tok.tolist() == [[13, 14, 15], [8, 9, 7], [8, PAD, PAD], [PAD] * 3, [202, 203, PAD]]


def test_accept_over_the_map_is_accept_on_the_rows_it_names():
    """Two slots, K = 2, 6 rows: slot 0 verifies depths 1 and 2 on rows 3 and 5, slot 1 depth 1 on row 4 (row 2 is parked)."""
    B, K, rows, n_part = 2, 2, 6, 4
    row_tok = {0: 10, 1: 20, 3: 11, 5: 12, 4: 99, 2: 77}                      # the model's token on every row
    val = np.zeros((rows, n_part), np.float32)
    idx = np.zeros((rows, n_part), np.int32)
    for r, t in row_tok.items():
        val[r, r % n_part], idx[r, r % n_part] = 3.0, t
    draft_row = np.asarray([[3, 5], [4, -1]], np.int32)
    draft_tok = np.asarray([[10, 11], [21, PAD]], np.int32)                    # slot 0: both right; slot 1: wrong
    hist = np.full((8, B), -1, np.int32)
    ctx, plen, fin = np.asarray([5, 6], np.int32), np.asarray([5, 6], np.int32), np.zeros(B, np.int32)
    tok, prop, acc = D.accept_rows(val, idx, np.asarray([2, 1]), draft_tok, draft_row, hist, ctx, plen, fin, (50,), PAD, 2, K)
    assert tok.tolist() == [12, 20] and ctx.tolist() == [8, 7] and prop.tolist() == [2, 1] and acc.tolist() == [2, 0]
    assert hist[1:4, 0].tolist() == [10, 11, 12] and hist[1:3, 1].tolist() == [20, -1]


def test_simulate_counts_dealt_drafts_only():
    """Three slots with full scripts, K = 2, 5 rows: two spare rows, so per step slots 0 and 1 verify one draft and slot 2 none,
    until slot 0 ends on its EOS and its row goes to slot 2."""
    truth = [[1, 2, 3, 9, 0, 0, 0], list(range(20, 40)), list(range(40, 60))]
    trace = []
    res = D.simulate([[5]] * 3, truth, truth, 2, 5, 3, eos=(9,), trace=trace)
    assert [nd for _, nd in trace] == [[1, 1, 0], [1, 1, 0], [0, 1, 1]]
    assert res == [(4, 2, 2), (7, 3, 3), (5, 1, 1)]
    # with rows for everything it is spec_ref.simulate slot by slot
    res = D.simulate([[5]] * 3, truth, truth, 2, 9, 3, eos=(9,))
    assert res == [R.simulate(t, t, 2, 3, eos=(9,)) for t in truth]


# ----------------------------------------------------------------------------- SpecConfig and the command line
def test_spec_config_share_rows():
    assert SpecConfig().share_rows is False and SpecConfig(3, 2, 4) == SpecConfig(3, 2, 4, False)
    shared = SpecConfig(3, share_rows=True)
    for B, rows in ((1, 17), (4, 17), (5, 20), (8, 32), (9, 32), (20, 32), (31, 32)):
        shared.check(B)
        assert shared.rows(B) == rows
    assert [SpecConfig(3).rows(B) for B in (1, 4, 5, 8)] == [17, 17, 20, 32]
    with pytest.raises(KarantaHipError, match="no row is spare"):
        shared.check(32)
    with pytest.raises(KarantaHipError, match="rows > 32"):
        SpecConfig(3).check(9)
    with pytest.raises(KarantaHipError, match="ngram_min"):
        SpecConfig(3, 3, 2, share_rows=True).check(20)


def test_cli_share_rows():
    cfg = {"method": "ngram", "num_speculative_tokens": 3, "share_rows": True}
    a = spec_args(cfg, "--max-num-seqs", "24")
    assert a.speculative == (3, 2, 4) and a.speculative_share_rows is True
    assert spec_args(cfg, "--max-num-seqs", "31").speculative_share_rows is True
    assert cli.speculative_fields(json.dumps(cfg), 24) == (3, 2, 4, True) and cli.speculative_config(json.dumps(cfg), 24) == (3, 2, 4)
    # without the key nothing changes
    a = spec_args({"method": "ngram"})
    assert a.speculative == (3, 2, 4) and a.speculative_share_rows is False
    assert cli.parse_args(["serve", "/m"]).speculative_share_rows is False
    a = spec_args({"method": "ngram", "share_rows": False})
    assert a.speculative == (3, 2, 4) and a.speculative_share_rows is False


@pytest.mark.parametrize("cfg,more,why", [
    ({"method": "ngram", "share_rows": True}, ["--max-num-seqs", "32"], "no row is spare"),
    ({"method": "ngram", "num_speculative_tokens": 3}, ["--max-num-seqs", "9"], "36 rows"),
    ({"method": "ngram", "share_rows": False}, ["--max-num-seqs", "9"], "36 rows"),
    ({"method": "ngram", "share_rows": 1}, [], "share_rows must be true or false"),
    ({"method": "ngram", "share_rows": True}, ["--max-logprobs", "5"], "cannot be combined with --max-logprobs"),
])
def test_cli_share_rows_refusals(cfg, more, why, capsys):
    import re
    with pytest.raises(SystemExit):
        spec_args(cfg, *more)
    assert re.search(why, capsys.readouterr().err)


def test_bench_corpus_takes_share_rows():
    from karanta_ocr_amd import bench_corpus
    with pytest.raises(SystemExit):      # 32 slots: refused with the reason, before anything is built
        bench_corpus.main(["--slots", "32", "--speculative-config", json.dumps({"method": "ngram", "share_rows": True})])


# ----------------------------------------------------------------------------- the scheduler at 20 slots
class FakeSharedEngine(FakeSpecEngine):
    """FakeSpecEngine whose speculative step has `rows` rows in all: every live slot wants K drafts, the rows - B spare ones are dealt
    (spec_deal_ref.deal_rows) and a slot emits 1 + min(dealt, accept(j, step)) tokens."""

    def __init__(self, n_slots, script, K, accept, rows=32):
        super().__init__(n_slots, script, K, accept)
        self.rows = rows

    def decode_steps(self, n, speculative=False):
        if not speculative:
            return super().decode_steps(n)
        self.log.append(("spec", n))
        for _ in range(n):
            self.step_no += 1
            live = [not f for f in self.fin]
            nd = (D.deal_rows([self.K] * self.B, live, self.K, self.rows) >= 0).sum(axis=1)
            assert nd.sum() == min(self.rows - self.B, self.K * sum(live))
            for j in range(self.B):
                if not live[j]:
                    continue
                self._emit(j)
                self.prop[j] += int(nd[j])
                for _ in range(min(int(nd[j]), self.accept(j, self.step_no))):
                    if not self._emit(j):
                        break
                    self.acc[j] += 1


@pytest.mark.parametrize("accept", [lambda j, s: 3, lambda j, s: (j + s) % 4])
def test_scheduler_at_twenty_slots_gives_the_right_lengths(accept):
    eng = FakeSharedEngine(20, SCRIPT, 3, accept)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=4, speculative=True, spec_policy=SpecPolicy(0.0))
    assert sch.over == 4 * 4 and eng.max_new == 50 + 16           # the overshoot stays chunk x (K + 1)
    reqs = [(k % 6, 5 + (7 * k) % 46) for k in range(50)]
    res = sch.run([SlotRequest(Page([k, 0]), mt, tag=i) for i, (k, mt) in enumerate(reqs)])
    for r, (k, mt) in zip(res, reqs):
        toks, reason = expect(k, mt)
        assert r.error is None and r.tokens.tolist() == toks and r.finish_reason == reason
    assert all(kind == "spec" for kind, _ in eng.log) and eng.max_hist <= 50 + 16
    assert (sch.spec_draft_tokens, sch.spec_accepted_tokens) == (int(eng.prop.sum()), int(eng.acc.sum()))
    assert 0 < int(eng.prop.sum()) <= 12 * sch.spec_steps          # never more than the 12 spare rows per step
