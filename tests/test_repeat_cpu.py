"""Repetition detection without a GPU: the rule by its definition against the state machine the kernel keeps (tests/repeat_ref.py),
the guide patterns of tests/test_gpu_repeat_engine.py force their output, the request field, the slot scheduler on a fake engine
that follows kr_repeat_detect, the server's default and a request's override, the CLI flag."""
import itertools
import json
from types import SimpleNamespace

import numpy as np
import pytest

from karanta_ocr_amd import serving as S
from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.request import PageRequest, RepetitionParams
from karanta_ocr_amd.sampling import StepFeatures, parse_repetition_field
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
from tests import repeat_ref as R
from tests.spec_guide_ref import Pattern
from tests.test_scheduler_cpu import FakeEngine, Page

SMALL = [(1, 3, 2, 0), (1, 2, 3, 0), (2, 4, 2, 0), (1, 3, 2, 5), (2, 3, 3, 7)]


def walk(y, params, chunks):
    inc, at = R.Incremental(*params), 0
    for n in itertools.cycle(chunks):
        if at >= len(y):
            break
        inc.feed(y[at:at + n])
        at += n
    return inc


# ----------------------------------------------------------------------------- the rule
def test_hand_worked_cases():
    abc = [1, 2, 3] * 10
    assert R.first_repeat(abc, 2, 8, 5) == 14                       # five copies of a 3-token block: token 15
    assert R.first_repeat([9] * 6 + abc, 2, 8, 5) == 20
    assert R.first_repeat(abc, 2, 8, 5, m=20) == 19                 # min_span binds: 20 tokens of repetition (run 17 = 20 - 3)
    assert R.first_repeat(abc, 4, 5, 2) is None and R.first_repeat(abc, 4, 6, 2) == 11    # only through p = 6
    assert R.first_repeat([1, 2] * 10, 3, 4, 2) == 7                # a period-2 loop seen as period 4
    assert R.first_repeat([7] * 5, 1, 1, 5) == 4 and R.first_repeat([7] * 4, 1, 1, 5) is None
    broken = [1, 2, 3] * 3 + [1, 2, 0] + [1, 2, 3] * 6
    assert R.first_repeat(broken, 3, 3, 5) == 12 + 14 and R.first_repeat(broken[:26], 3, 3, 5) is None
    assert R.cut([5, 5, 5, 99, 5], (1, 1, 3, 0), stop_ids=(99,)) == ([5, 5, 5], "length", "repetition")
    assert R.cut([5, 5, 99, 5], (1, 1, 3, 0), stop_ids=(99,)) == ([5, 5, 99], "stop", None)
    assert R.cut([5, 5, 99], (1, 1, 2, 0), stop_ids=(99,)) == ([5, 5], "length", "repetition")
    assert R.cut([5, 99, 99], (1, 1, 2, 0), stop_ids=(99,)) == ([5, 99], "stop", None)      # an EOS at the index wins


def test_definition_and_state_machine_agree_on_every_binary_sequence():
    for params in SMALL:
        for bits in range(1 << 14):
            y = [(bits >> i) & 1 for i in range(14)]
            want = R.first_repeat(y, *params)
            inc = R.Incremental(*params)
            got = inc.feed(y)
            assert got == (-1 if want is None else want), (params, y)
            assert inc.seen == (14 if want is None else want + 1)


def planted(rng, n_free, block, copies, tail=0):
    return (rng.integers(0, 50, n_free).tolist() + rng.integers(0, 50, block).tolist() * copies + rng.integers(0, 50, tail).tolist())


@pytest.mark.parametrize("seed", range(6))
def test_planted_loops_and_chunkings(seed):
    rng = np.random.default_rng(seed)
    for _ in range(25):
        block, copies = int(rng.integers(1, 40)), int(rng.integers(2, 7))
        y = planted(rng, int(rng.integers(0, 30)), block, copies, int(rng.integers(0, 10)))
        a = int(rng.integers(1, block + 2))
        params = (a, a + int(rng.integers(0, 40)), int(rng.integers(2, 6)), int(rng.integers(0, 3)) * int(rng.integers(0, 60)))
        want = R.first_repeat(y, *params)
        one = walk(y, params, [1])
        assert one.rep_at == (-1 if want is None else want), (params, y)
        for chunks in ([2], [3], [4], [1, 4, 2, 3], [4, 1]):
            many = walk(y, params, chunks)
            assert (many.rep_at, many.seen) == (one.rep_at, one.seen), (params, chunks, y)
            np.testing.assert_array_equal(many.run, one.run)


def test_stale_counters_do_not_leak_into_the_next_sequence():
    inc = R.Incremental(1, 8, 5)
    inc.feed([1, 2, 3] * 4 + [1, 2])                # one short of the trigger
    assert inc.rep_at == -1 and inc.run[2] == 11
    inc.admit(1, 8, 5)                              # run is left as it is
    y = [3, 1, 2] + [4, 5] * 6
    assert inc.feed(y) == R.first_repeat(y, 1, 8, 5) == 3 + 10 - 1


# ----------------------------------------------------------------------------- the engine tests' patterns force their output
CFG = CONFIGS["tiny-w512"]
FORCED = {r"(?:abc){40}": b"abc" * 40, r"hello (?:abc){40}": b"hello " + b"abc" * 40, r"x{100}": b"x" * 100,
          r"(?:abcdefg){20}": b"abcdefg" * 20, r"abcdefghijklmnopqrstuvwxyz0123456789": b"abcdefghijklmnopqrstuvwxyz0123456789"}


@pytest.mark.parametrize("text", sorted(FORCED))
def test_every_state_of_the_forcing_patterns_allows_one_token(text):
    tb = S.ByteTokenizer(CFG).token_bytes()
    eos = tuple(int(e) for e in CFG.eos_token_ids)
    p = Pattern(text, tb, eos)
    st = p.start
    for ch in FORCED[text]:
        assert np.flatnonzero(p.mask[st]).tolist() == [ch], (text, st)
        st = p.guide.walk(st, bytes([ch]))
        assert st != 0
    assert p.guide.accept[st] and sorted(np.flatnonzero(p.mask[st]).tolist()) == sorted(set(eos))
    assert p.guide.n_states <= len(FORCED[text]) + 2        # the walk saw them all: start .. accept (+ the dead state)


# ----------------------------------------------------------------------------- the request field
GOOD = {"max_pattern_size": 8, "min_pattern_size": 2, "min_count": 5}


def test_field_parsing():
    assert parse_repetition_field(None) is None and parse_repetition_field(False) is None
    assert parse_repetition_field(GOOD) == RepetitionParams(8, 2, 5, 0) and parse_repetition_field(GOOD).row() == (2, 8, 5, 0)
    assert parse_repetition_field({**GOOD, "min_span": 30}).row() == (2, 8, 5, 30)
    assert parse_repetition_field({**GOOD, "max_pattern_size": 1024.0}).row() == (2, 1024, 5, 0)      # 1024.0 is an integer, as for top_k
    assert parse_repetition_field({"max_pattern_size": 1, "min_pattern_size": 1, "min_count": 2}).row() == (1, 1, 2, 0)
    for bad in ({**GOOD, "max_pattern_size": 8.5}, {**GOOD, "min_count": "5"}, {**GOOD, "min_span": True},
                {**GOOD, "min_pattern_size": 9}, {**GOOD, "min_pattern_size": 0}, {**GOOD, "max_pattern_size": 1025},
                {**GOOD, "min_count": 1}, {**GOOD, "min_span": -1}, {**GOOD, "window": 3}, {"max_pattern_size": 8}, {}, True, 5, "on",
                [2, 8, 5]):
        with pytest.raises(ValueError, match="repetition_detection"):
            parse_repetition_field(bad)
    with pytest.raises(ValueError):
        RepetitionParams(8, 2, 1)
    assert not StepFeatures.of([PageRequest(np.zeros(3, np.int64))]).repetition
    f = StepFeatures.of([PageRequest(np.zeros(3, np.int64), repetition=RepetitionParams(8, 2, 5))])
    assert f.repetition and f == StepFeatures(repetition=True) and f != StepFeatures() and not f.sampling
    assert (f | StepFeatures(True)).repetition and not (f & StepFeatures(True, True, True, True)).repetition
    assert len({StepFeatures(), StepFeatures(repetition=True)}) == 2        # the graph key tells them apart


def test_frontend_400s_and_parses():
    fe = S.ChatFrontend(CFG, S.ByteTokenizer(CFG))
    msg = [{"role": "user", "content": "x"}]
    p = fe.parse({"messages": msg})
    assert p.repetition is None and not p.repetition_set
    p = fe.parse({"messages": msg, "repetition_detection": GOOD})
    assert p.repetition == RepetitionParams(8, 2, 5) and p.repetition_set
    for off in (None, False):
        p = fe.parse({"messages": msg, "repetition_detection": off})
        assert p.repetition is None and p.repetition_set
    with pytest.raises(S.BadRequest, match="min_count"):
        fe.parse({"messages": msg, "repetition_detection": {**GOOD, "min_count": 1}})


# ----------------------------------------------------------------------------- the scheduler, on a fake engine that keeps kr_repeat_detect's state
class RepFake(FakeEngine):
    """test_scheduler_cpu's engine with the repetition pass: per slot the state machine of tests/repeat_ref.py behind every token."""

    def begin_slots(self, max_new, **kw):
        super().begin_slots(max_new)
        self.inc = [None] * self.B
        self.features = []

    def set_step_features(self, sampling, guided, processing=False, adjust=False, repetition=False):
        self.features.append(bool(repetition))

    def admit(self, pages, slots):
        for p, j in zip(pages, slots):
            r = getattr(p, "repetition", None)
            self.inc[j] = None if r is None else R.Incremental(*r.row())
        return super().admit(pages, slots)

    def _emit(self, j):
        if self.fin[j]:
            return
        super()._emit(j)
        if self.inc[j] is not None and not self.fin[j] and self.inc[j].feed(self.hist[j][-1:]) >= 0:     # an EOS row is left alone
            self.fin[j] = True

    def slot_rep_at(self):
        return np.asarray([-1 if i is None else i.rep_at for i in self.inc])


LOOPS = {0: [1, 2, 3, 99], 1: [5] * 40, 2: [4, 5, 6] * 20, 3: [7, 7, 7, 99, 7, 7], 4: [7, 7, 99, 7], 5: [1, 2] + [8, 9] * 30}
P3 = RepetitionParams(3, 1, 3)        # three copies of a block of 1..3 tokens


def test_scheduler_cuts_at_the_repeat_and_counts():
    eng = RepFake(2, LOOPS)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=4, launch_ahead=False)
    pages = [Page([k]) for k in range(6)] + [Page([1])]
    for p in pages[1:6]:
        p.repetition = P3
    res = sch.run([SlotRequest(p, 50, tag=k) for k, p in enumerate(pages)])
    got = [(r.tokens.tolist(), r.finish_reason, r.stop_reason) for r in res]
    assert got.pop() == ([5] * 40 + [7] * 10, "length", None)       # the same script without the feature runs to its limit
    want = [R.cut(LOOPS[k], None if k == 0 else P3.row(), stop_ids=(99,)) for k in range(6)]
    assert got[0] == ([1, 2, 3, 99], "stop", None)
    assert got[1] == ([5, 5, 5], "length", "repetition") and got[2] == ([4, 5, 6] * 3, "length", "repetition")
    assert got[3] == ([7, 7, 7], "length", "repetition")            # the repeat comes before the EOS
    assert got[4] == ([7, 7, 99], "stop", None)                     # the EOS sits where the third copy would: "stop"
    assert got[5] == ([1, 2] + [8, 9] * 3, "length", "repetition")
    assert [(list(w[0]), w[1], w[2]) for w in want] == got
    assert sch.repetition_stops == 4 and sch.repetition_tokens_cut == sum(50 - len(g[0]) for g in got if g[2])
    assert eng.features[0] is True and eng.features[-1] is False and sch.idle      # the pass leaves with the last such request


def test_max_tokens_before_the_repeat_is_a_plain_length():
    eng = RepFake(1, LOOPS)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=4, launch_ahead=False)
    page = Page([2])
    page.repetition = P3
    (r,) = sch.run([SlotRequest(page, 8)])                           # one short of token 9
    assert (r.tokens.tolist(), r.finish_reason, r.stop_reason) == ([4, 5, 6, 4, 5, 6, 4, 5], "length", None)
    assert sch.repetition_stops == 0 and sch.repetition_tokens_cut == 0


def test_scheduler_default_and_the_requests_that_opt_out():
    eng = RepFake(2, LOOPS)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=4, launch_ahead=False, repetition=P3)
    own = Page([1])
    own.repetition = RepetitionParams(1, 1, 6)
    res = sch.run([SlotRequest(Page([1]), 20, tag="default"), SlotRequest(Page([1]), 20, tag="off", repetition_off=True),
                   SlotRequest(own, 20, tag="own")])
    assert [(len(r.tokens), r.stop_reason) for r in res] == [(3, "repetition"), (20, None), (6, "repetition")]
    assert all(r.finish_reason == "length" for r in res)


def test_scheduler_without_the_feature_asks_the_engine_nothing():
    eng = RepFake(2, LOOPS)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=4, launch_ahead=False)
    res = sch.run([SlotRequest(Page([1]), 20), SlotRequest(Page([0]), 20)])
    assert [len(r.tokens) for r in res] == [20, 4] and all(r.stop_reason is None for r in res) and eng.features == []


# ----------------------------------------------------------------------------- the server: default, override, stop_reason, metrics
class LoopEngine:
    """Static batches: every page emits its prompt's last byte forever; a page with `repetition` is cut by the reference."""
    B = 4
    cfg = CFG

    def generate(self, pages, max_new_tokens, **kw):
        toks, reasons, why = [], [], []
        for p in pages:
            r = getattr(p, "repetition", None)
            t, reason, cause = R.cut([int(p.input_ids[-1])] * max_new_tokens, None if r is None else r.row())
            toks.append(np.asarray(t, np.int64)); reasons.append(reason); why.append(cause)
        return SimpleNamespace(tokens=toks, finish_reasons=reasons, prompt_tokens=[len(p.input_ids) for p in pages], stop_reasons=why)


@pytest.mark.parametrize("greedy", [False, True])
def test_server_default_override_and_stop_reason(greedy):
    mk = lambda **kw: S.LocalServer(LoopEngine(), S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None,
                                    honor_temperature=not greedy, **kw)
    ask = lambda srv, **kw: srv.chat_completions({"messages": [{"role": "user", "content": "x"}], "max_tokens": 30, **kw})[1]["choices"][0]
    srv = mk()
    try:
        c = ask(srv)
        assert c["finish_reason"] == "length" and c["stop_reason"] is None
        c = ask(srv, repetition_detection={"max_pattern_size": 2, "min_pattern_size": 1, "min_count": 4})
        assert (c["finish_reason"], c["stop_reason"]) == ("length", "repetition")
        status, body = srv.chat_completions({"messages": [{"role": "user", "content": "x"}], "repetition_detection": {**GOOD, "min_count": 1}})
        assert status == 400 and "min_count" in body["error"]["message"]
    finally:
        srv.close()
    srv = mk(repetition={"max_pattern_size": 1, "min_pattern_size": 1, "min_count": 7})
    try:
        status, body = srv.chat_completions({"messages": [{"role": "user", "content": "x"}], "max_tokens": 30})
        assert body["choices"][0]["stop_reason"] == "repetition" and body["usage"]["completion_tokens"] == 7
        assert ask(srv, repetition_detection=False)["stop_reason"] is None
        assert ask(srv, repetition_detection=None)["stop_reason"] is None
        status, body = srv.chat_completions({"messages": [{"role": "user", "content": "x"}], "max_tokens": 30,
                                             "repetition_detection": {"max_pattern_size": 1, "min_pattern_size": 1, "min_count": 3}})
        assert body["usage"]["completion_tokens"] == 3 and body["choices"][0]["stop_reason"] == "repetition"
    finally:
        srv.close()
    with pytest.raises(ValueError, match="repetition_detection"):
        mk(repetition={"max_pattern_size": 1})


def test_continuous_server_metrics_and_client_result():
    from karanta_ocr_amd.clients import VLLMClient

    class Slots(RepFake):
        cfg = SimpleNamespace(eos_token_ids=(99,), text=CFG.text, pad_token_id=CFG.pad_token_id, image_token_id=CFG.image_token_id,
                              vision=CFG.vision, vision_start_token_id=CFG.vision_start_token_id, vision_end_token_id=CFG.vision_end_token_id)

        def admit(self, pages, slots):
            self.script = {int(p.input_ids[0]): [65] * 100 for p in pages}
            return super().admit(pages, slots)

    srv = S.LocalServer(Slots(2, {}), S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, continuous=True,
                        max_tokens_cap=64, repetition=RepetitionParams(1, 1, 5))
    S.register_local_server(8771, srv)
    try:
        r = VLLMClient(port=8771).generate([{"role": "user", "content": "x"}], max_tokens=40)
        assert (r["text"], r["finish_reason"], r["stop_reason"]) == ("AAAAA", "length", "repetition")
        assert r["usage"]["completion_tokens"] == 5
        r = VLLMClient(port=8771).generate([{"role": "user", "content": "x"}], max_tokens=9, repetition_detection=False)
        assert r["finish_reason"] == "length" and "stop_reason" not in r and r["usage"]["completion_tokens"] == 9
        m = srv.metrics()[1]["scheduler"]
        assert m["repetition_stops"] == 1 and m["repetition_tokens_cut"] == 35
    finally:
        S.unregister_local_server(8771)
        srv.close()


# ----------------------------------------------------------------------------- the CLI flag
def test_cli_flag():
    from karanta_ocr_amd import cli
    args = cli.parse_args(["serve", "/m", "--repetition-detection", json.dumps({**GOOD, "min_span": 40})])
    assert args.repetition == RepetitionParams(8, 2, 5, 40)
    assert cli.parse_args(["serve", "/m"]).repetition is None
    for bad in ("{not json", "[1, 2]", json.dumps({**GOOD, "min_count": 1}), json.dumps({"max_pattern_size": 4})):
        with pytest.raises(ValueError):
            cli.repetition_config(bad)
        with pytest.raises(SystemExit):
            cli.parse_args(["serve", "/m", "--repetition-detection", bad])
