"""Host side of speculative decoding without a GPU: the policy as a pure rule, the scheduler's overshoot and choice of chunk kind
on a fake engine that advances a variable number of tokens per step, the command line's --speculative-config, and /metrics."""
import json
import types

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd.scheduler import SPEC_BREAK_EVEN, SlotRequest, SlotScheduler, SpecPolicy


# ----------------------------------------------------------------------------- policy
def test_policy_stays_speculative_at_and_above_the_break_even():
    p = SpecPolicy(break_even=0.5, window=4, probe_after=3)
    for _ in range(20):
        assert p.want()
        p.record(accepted=8, slot_steps=16)       # exactly 0.5 per slot-step
    assert p.rate() == 0.5


def test_policy_falls_back_to_plain_chunks_and_probes_again():
    p = SpecPolicy(break_even=0.5, window=4, probe_after=3)
    kinds = []
    for i in range(16):
        w = p.want()
        kinds.append(w)
        if w:
            p.record(accepted=1, slot_steps=16)   # 0.0625 per slot-step: far below
    # four speculative chunks fill the window, then three plain ones, then the probe: a fresh window of four
    assert kinds == [True] * 4 + [False] * 3 + [True] * 4 + [False] * 3 + [True] * 2


def test_policy_judges_the_window_not_the_first_chunk():
    p = SpecPolicy(break_even=0.5, window=4, probe_after=3)
    for acc in (0, 0, 0):
        assert p.want()
        p.record(acc, 8)
    assert p.want()                                # three bad chunks do not fill the window
    p.record(24, 8)                                # (0 + 0 + 0 + 24) / 32 = 0.75
    assert p.want() and p.rate() == 0.75
    p.record(0, 0)                                 # a chunk without live slots says nothing
    assert p.rate() == 0.75


def test_default_break_even_is_the_cited_ratio():
    assert SPEC_BREAK_EVEN == pytest.approx(1.68 / 1.15 - 1) and SpecPolicy().break_even == SPEC_BREAK_EVEN
    with pytest.raises(ValueError):
        SpecPolicy(window=0)


# ----------------------------------------------------------------------------- scheduler on a fake engine
class Page:
    def __init__(self, ids, **kw):
        self.input_ids = np.asarray(ids)
        self.pixel_values, self.grids = None, []
        for k, v in kw.items():
            setattr(self, k, v)


class FakeSpecEngine:
    """The Engine slot API with speculative steps: slot j's sequence is script[prompt[0]]; in a speculative step a live slot emits
    1 + accept(j, step) tokens (at most K + 1, nothing after an EOS) and K drafts count as proposed."""
    class cfg:
        eos_token_ids = (99,)

    def __init__(self, n_slots, script, K, accept, s_max=10 ** 6):
        self.B, self.script, self.K, self.accept, self.s_max = n_slots, script, K, accept, s_max
        self.log, self.max_hist = [], 0

    def seq_room(self):
        return self.s_max - 1 - self.K

    def can_speculate(self):
        return True

    def begin_slots(self, max_new, sampling=False):
        self.max_new = max_new
        self.seq, self.gen, self.fin = [None] * self.B, [0] * self.B, [True] * self.B
        self.hist = [[] for _ in range(self.B)]
        self.prop, self.acc = np.zeros(self.B, np.int64), np.zeros(self.B, np.int64)
        self.step_no = 0

    def admit(self, pages, slots, budgets=None):
        for p, j, bud in zip(pages, slots, budgets):
            assert self.fin[j] and bud <= self.max_new and len(p.input_ids) + bud <= self.seq_room()
            self.seq[j], self.hist[j], self.gen[j], self.fin[j] = list(self.script[int(p.input_ids[0])]), [], 0, False
            self.budget = getattr(self, "budget", {})
            self.budget[j] = bud
            self._emit(j)
        return [len(p.input_ids) for p in pages]

    def _emit(self, j):
        if self.fin[j]:
            return False
        tok = self.seq[j][self.gen[j]] if self.gen[j] < len(self.seq[j]) else 7
        assert self.gen[j] < self.budget[j], f"slot {j} ran past its budget of {self.budget[j]} tokens"
        self.hist[j].append(tok)
        self.gen[j] += 1
        self.max_hist = max(self.max_hist, self.gen[j])
        if tok == 99:
            self.fin[j] = True
        return True

    def decode_steps(self, n, speculative=False):
        self.log.append(("spec" if speculative else "plain", n))
        for _ in range(n):
            self.step_no += 1
            for j in range(self.B):
                if self.fin[j]:
                    continue
                self._emit(j)
                if speculative:
                    self.prop[j] += self.K
                    for _ in range(min(self.K, self.accept(j, self.step_no))):
                        if not self._emit(j):
                            break
                        self.acc[j] += 1

    def spec_counts(self):
        return self.prop.copy(), self.acc.copy()

    def poll_slots(self):
        return np.asarray(self.fin), np.asarray(self.gen)

    def slot_tokens(self, j, n):
        return np.asarray(self.hist[j][:n])

    def retire(self, j):
        self.fin[j] = True


SCRIPT = {0: [1, 2, 3, 99], 1: [5] * 60, 2: [99], 3: [4, 4, 99, 8, 8], 4: list(range(100, 140)) + [99], 5: [9] * 200}


def expect(k, max_tokens):
    seq = SCRIPT[k]
    out = []
    for t in seq + [7] * 300:
        out.append(t)
        if t == 99 or len(out) == max_tokens:
            break
    return out, "stop" if out[-1] == 99 else "length"


@pytest.mark.parametrize("accept", [lambda j, s: 3, lambda j, s: 0, lambda j, s: (j + s) % 4])
def test_results_do_not_depend_on_what_is_accepted(accept):
    """Token limits that fall inside accepted runs, EOS inside a run, and the overshoot: a slot never runs past its budget of
    max_tokens + chunk * (K + 1) tokens although a step emits up to K + 1."""
    eng = FakeSpecEngine(3, SCRIPT, 3, accept)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=4, speculative=True, spec_policy=SpecPolicy(0.0))
    assert sch.over == 4 * 4 and eng.max_new == 50 + 16
    reqs = [(0, 10), (1, 9), (2, 5), (3, 30), (4, 50), (5, 33), (1, 50), (5, 7)]
    res = sch.run([SlotRequest(Page([k, 0]), mt, tag=i) for i, (k, mt) in enumerate(reqs)])
    for r, (k, mt) in zip(res, reqs):
        toks, reason = expect(k, mt)
        assert r.error is None and r.tokens.tolist() == toks and r.finish_reason == reason
    assert all(kind == "spec" for kind, _ in eng.log) and sch.spec_steps == sch.steps and sch.plain_steps == 0
    assert eng.max_hist <= 50 + 16
    assert (sch.spec_draft_tokens, sch.spec_accepted_tokens) == (int(eng.prop.sum()), int(eng.acc.sum()))


def test_a_request_beyond_the_speculative_capacity_is_a_client_error():
    eng = FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 3, s_max=64)        # room 64 - 1 - 3 = 60
    sch = SlotScheduler(eng, max_tokens_cap=40, chunk=2, speculative=True)
    ok, bad = sch.run([SlotRequest(Page([5] * 12), 40), SlotRequest(Page([5] * 13), 40)])     # 12 + 40 + 8 = 60; 13 + 40 + 8 = 61
    assert ok.error is None and len(ok.tokens) == 40
    assert bad.status == 400 and "8 scheduler steps" in bad.error


def test_policy_drives_the_kind_of_chunk():
    """Acceptance below the break-even: after the window the chunks are plain, and the scheduler probes again after probe_after."""
    eng = FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 0)
    sch = SlotScheduler(eng, max_tokens_cap=200, chunk=2, speculative=True, spec_policy=SpecPolicy(0.5, window=3, probe_after=5))
    sch.run([SlotRequest(Page([5]), 60), SlotRequest(Page([5]), 60)])
    kinds = [k for k, _ in eng.log]
    assert kinds[:12] == ["spec"] * 3 + ["plain"] * 5 + ["spec"] * 3 + ["plain"]
    assert sch.spec_steps == 2 * kinds.count("spec") and sch.plain_steps == 2 * kinds.count("plain")
    # full acceptance: never leaves speculation
    eng = FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=200, chunk=2, speculative=True, spec_policy=SpecPolicy(0.5, window=3, probe_after=5))
    sch.run([SlotRequest(Page([5]), 150), SlotRequest(Page([5]), 150)])
    assert {k for k, _ in eng.log} == {"spec"} and sch.spec_policy.rate() == 3.0


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.2), dict(guide="[a-z]+"), dict(logit_bias={3: 1.0}), dict(top_k=5)])
def test_requests_that_need_per_token_state_run_plain_chunks(kw):
    eng = FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 3)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    # the special request is short: while it is in its slot every chunk is plain, afterwards the other request speculates
    res = sch.run([SlotRequest(Page([1], **kw), 6), SlotRequest(Page([5]), 40)])
    assert [len(r.tokens) for r in res] == [6, 40]
    kinds = [k for k, _ in eng.log]
    n_plain = kinds.index("spec")
    assert n_plain >= 3 and set(kinds[n_plain:]) == {"spec"}


def test_scheduler_refuses_speculation_without_a_speculative_engine():
    eng = FakeSpecEngine(2, SCRIPT, 0, lambda j, s: 0)
    with pytest.raises(ValueError, match="SpecConfig"):
        SlotScheduler(eng, max_tokens_cap=8, speculative=True)
    logged = SlotScheduler(FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 3), max_tokens_cap=8, chunk=2, speculative=True)
    logged.logprobs = 2                              # a scheduler that records log-probabilities never speculates
    logged.engine.slot_logprobs = lambda j, n, k: None
    logged.run([SlotRequest(Page([5]), 8)])
    assert logged.spec_steps == 0 and logged.plain_steps > 0


# ----------------------------------------------------------------------------- command line
def spec_args(cfg, *more):
    return cli.parse_args(["serve", "/m", "--speculative-config", json.dumps(cfg) if not isinstance(cfg, str) else cfg, *more])


def test_cli_parses_the_ngram_config():
    a = spec_args({"method": "ngram", "num_speculative_tokens": 3, "prompt_lookup_min": 2, "prompt_lookup_max": 4})
    assert a.speculative == (3, 2, 4) and "--speculative-config" not in a.ignored
    assert spec_args({"method": "ngram"}).speculative == (3, 2, 4)                                   # the defaults
    assert spec_args({"method": "ngram", "num_speculative_tokens": 1, "prompt_lookup_min": 5}, "--max-num-seqs", "16").speculative == (1, 5, 5)
    assert cli.parse_args(["serve", "/m"]).speculative is None


@pytest.mark.parametrize("cfg,more,why", [
    ({"method": "eagle", "num_speculative_tokens": 3}, [], "method 'eagle' is not supported"),
    ({"num_speculative_tokens": 3}, [], "method None is not supported"),
    ({"method": "ngram", "num_speculative_tokens": 4}, [], r"8 x \(num_speculative_tokens 4 \+ 1\) = 40 rows"),
    ({"method": "ngram", "num_speculative_tokens": 3}, ["--max-num-seqs", "9"], "36 rows"),
    ({"method": "ngram", "num_speculative_tokens": 0}, [], "num_speculative_tokens must be an integer >= 1"),
    ({"method": "ngram", "prompt_lookup_min": 3, "prompt_lookup_max": 2}, [], "prompt_lookup_min 3 <= prompt_lookup_max 2"),
    ({"method": "ngram", "prompt_lookup_max": 9}, [], "<= 8 does not hold"),
    ("{not json", [], "is not JSON"),
    ("[1]", [], "must be a JSON object"),
    ({"method": "ngram"}, ["--max-logprobs", "5"], "cannot be combined with --max-logprobs"),
    ({"method": "ngram"}, ["--static-batching"], "not with --static-batching"),
])
def test_cli_refuses_with_the_reason(cfg, more, why, capsys):
    import re
    with pytest.raises(SystemExit):
        spec_args(cfg, *more)
    assert re.search(why, capsys.readouterr().err)


def test_bench_corpus_takes_the_flag():
    from karanta_ocr_amd import bench_corpus
    with pytest.raises(SystemExit):
        bench_corpus.main(["--slots", "16", "--speculative-config", json.dumps({"method": "ngram", "num_speculative_tokens": 3})])


# ----------------------------------------------------------------------------- /metrics
def test_metrics_carry_the_speculative_counters():
    from karanta_ocr_amd.serving import LocalServer
    eng = FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 2)
    sch = SlotScheduler(eng, max_tokens_cap=50, chunk=2, speculative=True, spec_policy=SpecPolicy(0.0))
    sch.run([SlotRequest(Page([5]), 30), SlotRequest(Page([1], top_k=3), 10)])
    stats = LocalServer.scheduler_stats(types.SimpleNamespace(_sch=sch))
    assert stats["spec_decode_num_draft_tokens"] == int(eng.prop.sum()) > 0
    assert stats["spec_decode_num_accepted_tokens"] == int(eng.acc.sum()) > 0
    assert stats["spec_decode_steps"] == sch.spec_steps > 0 and stats["plain_decode_steps"] == sch.plain_steps > 0
    assert stats["decode_steps"] == sch.spec_steps + sch.plain_steps
    # a scheduler without speculation reports zeros under the same names
    plain = SlotScheduler(FakeSpecEngine(2, SCRIPT, 3, lambda j, s: 0), max_tokens_cap=8, chunk=2)
    plain.run([SlotRequest(Page([5]), 8)])
    stats = LocalServer.scheduler_stats(types.SimpleNamespace(_sch=plain))
    assert stats["spec_decode_num_draft_tokens"] == 0 and stats["spec_decode_steps"] == 0 and stats["plain_decode_steps"] == plain.steps
