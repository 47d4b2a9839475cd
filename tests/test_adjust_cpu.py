"""logit_bias / min_tokens / stop_token_ids / stop on the host (no GPU): request validation as vLLM's OpenAI layer does it, the
StepFeatures algebra with `adjust`, the device table of a page, the stop-string matcher on the byte tokenizer, the slot scheduler
with a stop string next to a plain request, the server surface, and the seeds of the GPU sampler-integration cases."""
from types import SimpleNamespace

import numpy as np
import pytest

from karanta_ocr_amd import serving as S
from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.sampling import (ADJ_CAP, StepFeatures, StopStrings, adjust_table, needs_adjust, parse_adjust_fields)
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
from tests import adjust_cases as A

CFG = CONFIGS["tiny"]
V = CFG.text.vocab_size
EOS = CFG.eos_token_ids


def parse(req, max_tokens=16, **kw):
    return parse_adjust_fields(req, V, max_tokens, **kw)


# ----------------------------------------------------------------------------- validation
def test_absent_and_null_fields_are_off():
    off = {"logit_bias": None, "min_tokens": 0, "stop_token_ids": (), "stop": (), "include_stop_str_in_output": False}
    assert parse({}) == off
    assert parse({k: None for k in off}) == off
    assert parse({"logit_bias": {}, "stop_token_ids": [], "stop": []}) == off


def test_logit_bias_keys_and_values():
    assert parse({"logit_bias": {"12": 1.5, 7: -3}})["logit_bias"] == {12: 1.5, 7: -3.0}
    assert parse({"logit_bias": {"0": 250, str(V - 1): -1e9}})["logit_bias"] == {0: 100.0, V - 1: -100.0}    # clamped
    for bad in ({"x": 1.0}, {"1.5": 1.0}, {str(V): 1.0}, {"-1": 1.0}, {"3": "1"}, {"3": None}, {"3": float("nan")},
                {"3": float("inf")}, {"3": True}, [1, 2], "7"):
        with pytest.raises(ValueError, match="logit_bias"):
            parse({"logit_bias": bad})


def test_min_tokens_bounds_and_guides():
    assert parse({"min_tokens": 0})["min_tokens"] == 0
    assert parse({"min_tokens": 16})["min_tokens"] == 16          # == max_tokens
    assert parse({"min_tokens": 3.0})["min_tokens"] == 3
    for bad in (17, -1, 2.5, "3", True):
        with pytest.raises(ValueError, match="min_tokens"):
            parse({"min_tokens": bad})
    with pytest.raises(ValueError, match="guided"):
        parse({"min_tokens": 1}, guided=True)
    assert parse({"min_tokens": 0, "logit_bias": {"1": 1}}, guided=True)["min_tokens"] == 0     # a guide alone is fine


def test_stop_token_ids_and_stop_strings():
    assert parse({"stop_token_ids": list(range(16))})["stop_token_ids"] == tuple(range(16))
    for bad in (list(range(17)), [V], [-1], [1.5], ["1"], 5, [True]):
        with pytest.raises(ValueError, match="stop_token_ids"):
            parse({"stop_token_ids": bad})
    assert parse({"stop": "END"})["stop"] == ("END",)
    assert parse({"stop": ["a", "bc"], "include_stop_str_in_output": True}) == dict(
        parse({}), stop=("a", "bc"), include_stop_str_in_output=True)
    for bad in ("", ["ok", ""], [1], 7, ["s"] * 17):
        with pytest.raises(ValueError, match="stop"):
            parse({"stop": bad})
    assert len(parse({"stop": ["s%d" % i for i in range(16)]})["stop"]) == 16
    with pytest.raises(ValueError, match="include_stop_str_in_output"):
        parse({"include_stop_str_in_output": "yes"})


def test_table_one_entry_over_the_cap():
    stops = list(range(400, 416))
    fits = {str(i): 1.0 for i in range(ADJ_CAP - 16)}
    assert len(parse({"logit_bias": fits, "stop_token_ids": stops})["logit_bias"]) == ADJ_CAP - 16
    over = dict(fits, **{str(ADJ_CAP - 16): 1.0})
    with pytest.raises(ValueError, match=str(ADJ_CAP)):
        parse({"logit_bias": over, "stop_token_ids": stops})
    # a stop id that is also a bias key shares its entry; the EOS ids join the table only with min_tokens
    assert parse({"logit_bias": over, "stop_token_ids": stops[:15] + [0]})
    with pytest.raises(ValueError, match=str(ADJ_CAP)):
        parse({"logit_bias": fits, "stop_token_ids": stops, "min_tokens": 1}, eos_token_ids=EOS)
    page = SimpleNamespace(logit_bias={i: 1.0 for i in range(ADJ_CAP - 15)}, stop_token_ids=tuple(stops), min_tokens=0)
    with pytest.raises(ValueError, match=str(ADJ_CAP)):
        adjust_table(page, EOS, V)


def test_frontend_parse_answers_400_and_fills_the_request():
    fe = S.ChatFrontend(CFG, S.ByteTokenizer(CFG))
    msg = [{"role": "user", "content": "x"}]
    q = fe.parse({"messages": msg, "max_tokens": 8, "logit_bias": {"65": 250}, "min_tokens": 2, "stop_token_ids": [66],
                  "stop": "zz", "include_stop_str_in_output": True})
    assert (q.logit_bias, q.min_tokens, q.stop_token_ids, q.stop, q.include_stop_str_in_output) == ({65: 100.0}, 2, (66,), ("zz",), True)
    plain = fe.parse({"messages": msg, "max_tokens": 8})
    assert (plain.logit_bias, plain.min_tokens, plain.stop_token_ids, plain.stop) == (None, 0, (), ())
    for bad in ({"logit_bias": {"x": 1}}, {"min_tokens": 9}, {"stop": ""}, {"stop_token_ids": [V]},
                {"min_tokens": 1, "guided_regex": "[ab]+"}):
        with pytest.raises(S.BadRequest):
            fe.parse(dict({"messages": msg, "max_tokens": 8}, **bad))


# ----------------------------------------------------------------------------- StepFeatures / tables
def test_step_features_with_adjust():
    of = lambda **kw: StepFeatures.of([SimpleNamespace(**kw)])
    assert StepFeatures(True, True, True) == StepFeatures(True, True, True, False)       # three positional arguments as before
    assert StepFeatures().adjust is False
    for kw in ({"logit_bias": {3: 1.0}}, {"min_tokens": 2}, {"stop_token_ids": (5,)}):
        assert needs_adjust(SimpleNamespace(**kw))
        assert of(**kw) == StepFeatures(True, False, False, True), kw                      # adjust implies sampling
    for kw in ({"logit_bias": None}, {"logit_bias": {}}, {"min_tokens": 0}, {"stop_token_ids": ()}, {}):
        assert not needs_adjust(SimpleNamespace(**kw)) and of(**kw) == StepFeatures()
    A_ = StepFeatures(True, False, False, True)
    assert StepFeatures(False, False, True) | A_ == StepFeatures(True, False, True, True)
    sampled_caps = StepFeatures(True, False, True, True)
    assert A_ & sampled_caps == A_
    assert A_ & StepFeatures(True, True, True) == StepFeatures(True, False, False, False)   # caps without adjust: pass dropped
    assert StepFeatures(False, False, False, True) & sampled_caps == A_                      # an adjusted step keeps its sampling pass
    assert A_ & StepFeatures() == StepFeatures()
    assert tuple(StepFeatures(True, True, False, True)) == (True, True, False, True)


def test_adjust_table_merges_bias_stop_and_eos():
    assert adjust_table(SimpleNamespace(), EOS, V) is None
    ids, vals, flags, meta = adjust_table(SimpleNamespace(logit_bias={7: 2.5, 9: -100.0}, stop_token_ids=(9, 11), min_tokens=0), EOS, V)
    assert len(set(ids.tolist())) == len(ids) == meta[0] == 3 and meta[1] == 0
    got = {int(i): (float(v), int(f)) for i, v, f in zip(ids, vals, flags)}
    assert got == {7: (2.5, 0), 9: (-100.0, 1), 11: (0.0, 1)}
    ids, vals, flags, meta = adjust_table(SimpleNamespace(logit_bias={EOS[0]: 100.0}, min_tokens=3), EOS, V)
    got = {int(i): (float(v), int(f)) for i, v, f in zip(ids, vals, flags)}
    assert got == {EOS[0]: (100.0, 1), EOS[1]: (0.0, 1)} and list(meta) == [2, 3, 0, 0]
    assert ids.dtype == np.int32 and vals.dtype == np.float32 and flags.dtype == np.int32 and meta.dtype == np.int32
    with pytest.raises(ValueError, match="vocabulary"):
        adjust_table(SimpleNamespace(stop_token_ids=(V,)), EOS, V)


# ----------------------------------------------------------------------------- stop strings
def matcher(stops, include=False):
    return StopStrings(stops, include, S.ByteTokenizer(CFG).token_bytes())


def test_stop_check_match_spanning_two_tokens():
    m = matcher(["lo w"])
    toks = list(b"hello world")
    assert m.check(toks[:4]) is None and m.check(toks[:6]) is None
    assert m.check(toks[:9]) == 7 and m.text == "hel"           # 'w' (index 6) completed it
    assert m.check(toks) == 7                                   # and it stays matched
    fresh = matcher(["lo w"])
    assert fresh.check(toks) == 7 and fresh.text == "hel"       # one call over everything = the incremental calls


def test_stop_check_earliest_match_wins_over_list_order():
    m = matcher(["world", "ell"])
    assert m.check(list(b"hello world")) == 4 and m.text == "h"
    m = matcher(["ab", "abc"])                                  # same start: the string listed first
    assert m.check(list(b"xabc")) == 3 and m.text == "x"


def test_stop_check_include_and_no_match_and_special_tokens():
    m = matcher(["ll"], include=True)
    assert m.check(list(b"hello")) == 4 and m.text == "hell"
    assert matcher(["xyz"]).check(list(b"hello world")) is None
    toks = [ord("a"), EOS[0], ord("b")]                         # a special token has no bytes: "ab" still matches across it
    m = matcher(["ab"])
    assert m.check(toks) == 3 and m.text == ""
    d = StopStrings(["lo"], False, None, S.ByteTokenizer(CFG).decode)      # tokenizers without byte strings: on decode()
    assert d.check(list(b"hel")) is None and d.check(list(b"hello")) == 5 and d.text == "hel"


# ----------------------------------------------------------------------------- scheduler
class StreamEngine:
    """Slot-API stand-in that emits a fixed token stream per request (page.stream, then 'z' forever), finishes a row on EOS or one
    of the page's stop_token_ids, and counts slot_tokens reads per slot."""
    cfg = CFG
    max_tokens = 4096
    max_patches = 1 << 20

    def __init__(self, B=2):
        self.B = B
        self.reads, self.features = [], []

    def begin_slots(self, max_new, sampling=False):
        self.page, self.hist, self.fin = [None] * self.B, [[] for _ in range(self.B)], [True] * self.B

    def set_step_features(self, sampling, guided, processing=False, adjust=False):
        self.features.append(StepFeatures(sampling, guided, processing, adjust))

    def _emit(self, j):
        if not self.fin[j]:
            k, st = len(self.hist[j]), self.page[j].stream
            tok = st[k] if k < len(st) else ord("z")
            self.hist[j].append(tok)
            self.fin[j] = tok in EOS or tok in self.page[j].stop_token_ids

    def admit(self, pages, slots):
        for p, j in zip(pages, slots):
            self.page[j], self.hist[j], self.fin[j] = p, [], False
            self._emit(j)
        return [len(p.input_ids) for p in pages]

    def decode_steps(self, n):
        for _ in range(n):
            for j in range(self.B):
                self._emit(j)

    def poll_slots(self):
        return np.asarray(self.fin), np.asarray([len(h) for h in self.hist])

    def slot_tokens(self, j, n):
        self.reads.append((j, n))
        return np.asarray(self.hist[j][:n], np.int64)

    def retire(self, j):
        self.fin[j] = True


def stream_page(text, **kw):
    kw.setdefault("stop_token_ids", ())
    return SimpleNamespace(input_ids=np.zeros(3, np.int64), grids=[], stream=list(text), **kw)


def test_scheduler_retires_a_stop_string_request_at_the_first_harvest_after_the_match():
    eng = StreamEngine()
    sch = SlotScheduler(eng, max_tokens_cap=32, chunk=2, eos_token_ids=EOS)
    m = matcher(["END"])
    stopper = SlotRequest(stream_page(b"abcdEND and more text"), 30, tag="s", stop_check=m)
    plain = SlotRequest(stream_page(b"0123456789ABCDEFGHIJKL"), 22, tag="p")
    sch.submit(stopper)
    sch.submit(plain)
    done, harvests = {}, 0
    while not sch.idle:
        for r in sch.step():
            done[r.tag] = (r, harvests, len(eng.hist[0]))
        harvests += 1
        if "s" in done and "p" not in done:
            assert all(j != 1 for j, _ in eng.reads), "a request without stop strings is not read before it finishes"
    r, at, generated = done["s"]
    # admission emits 1 token, every chunk 2 more: 'D' (the 7th token) exists after the third chunk = the third harvest
    assert at == 2 and generated == 7
    assert r.finish_reason == "stop" and r.error is None
    assert bytes(r.tokens.tolist()) == b"abcdEND" and m.text == "abcd"
    assert [n for j, n in eng.reads if j == 0] == [3, 5, 7]
    p = done["p"][0]
    assert p.finish_reason == "length" and len(p.tokens) == 22
    assert [n for j, n in eng.reads if j == 1] == [22]           # exactly one read, at the end


def test_scheduler_treats_stop_token_ids_like_eos_and_sets_the_adjust_feature():
    eng = StreamEngine()
    sch = SlotScheduler(eng, max_tokens_cap=32, chunk=2, eos_token_ids=EOS, sampling=True)
    a = SlotRequest(stream_page(b"abXcd", stop_token_ids=(ord("X"),)), 30, tag="a")
    b = SlotRequest(stream_page(b"abXc"), 6, tag="b")
    res = {r.tag: r for r in sch.run([a, b])}
    assert bytes(res["a"].tokens.tolist()) == b"abX" and res["a"].finish_reason == "stop"
    assert bytes(res["b"].tokens.tolist()) == b"abXczz" and res["b"].finish_reason == "length"     # not its stop id
    assert eng.features[0] == StepFeatures(True, False, False, True)
    assert eng.features[-1] == StepFeatures()                    # switched off once the adjusted request has left


# ----------------------------------------------------------------------------- server surface
class EchoEngine:
    """generate() emits every page's canned stream; records the pages it was given."""
    B = 4
    cfg = CFG

    def __init__(self, stream):
        self.stream, self.pages = list(stream), []

    def generate(self, pages, max_new_tokens, **kw):
        self.pages += list(pages)
        toks = [np.asarray(self.stream[:max_new_tokens], np.int64) for _ in pages]
        reasons = ["stop" if len(t) and (int(t[-1]) in EOS or int(t[-1]) in p.stop_token_ids) else "length" for t, p in zip(toks, pages)]
        return SimpleNamespace(tokens=toks, finish_reasons=reasons, prompt_tokens=[len(p.input_ids) for p in pages])


def test_static_server_cuts_at_the_stop_string_and_copies_the_fields():
    eng = EchoEngine(b"one two three four")
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None)
    msg = [{"role": "user", "content": "x"}]
    try:
        st, body = srv.chat_completions({"messages": msg, "max_tokens": 18, "stop": ["four", "o t"], "logit_bias": {"65": 5},
                                         "min_tokens": 2, "stop_token_ids": [300]})
        assert st == 200
        c = body["choices"][0]
        assert c["message"]["content"] == "one tw" and c["finish_reason"] == "stop"
        assert body["usage"]["completion_tokens"] == 9            # through the 't' of "three" that completed "o t"
        p = eng.pages[-1]
        assert (p.logit_bias, p.min_tokens, tuple(p.stop_token_ids)) == ({65: 5.0}, 2, (300,))
        st, body = srv.chat_completions({"messages": msg, "max_tokens": 18, "stop": "two", "include_stop_str_in_output": True})
        assert body["choices"][0]["message"]["content"] == "one two" and body["usage"]["completion_tokens"] == 7
        st, body = srv.chat_completions({"messages": msg, "max_tokens": 18, "stop": "never"})
        assert body["choices"][0]["message"]["content"] == "one two three four" and body["choices"][0]["finish_reason"] == "length"
        st, body = srv.chat_completions({"messages": msg, "max_tokens": 18, "min_tokens": 19})
        assert st == 400 and "min_tokens" in body["error"]["message"]
    finally:
        srv.close()
    # a stop id ends the message as EOS does: kept in the token list by the engine, dropped from the content
    eng = EchoEngine(list(b"ab") + [300] + list(b"cd"))
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None)
    try:
        st, body = srv.chat_completions({"messages": msg, "max_tokens": 3, "stop_token_ids": [300]})
        assert body["choices"][0]["message"]["content"] == "ab" and body["choices"][0]["finish_reason"] == "stop"
        assert body["usage"]["completion_tokens"] == 2
    finally:
        srv.close()
    # --greedy ignores all of them
    eng = EchoEngine(b"one two three four")
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, honor_temperature=False)
    try:
        st, body = srv.chat_completions({"messages": msg, "max_tokens": 18, "stop": "two", "logit_bias": {"65": 5}, "min_tokens": 2,
                                         "stop_token_ids": [300]})
        assert body["choices"][0]["message"]["content"] == "one two three four"
        p = eng.pages[-1]
        assert (p.logit_bias, p.min_tokens, tuple(p.stop_token_ids)) == (None, 0, ())
    finally:
        srv.close()


# ----------------------------------------------------------------------------- the GPU integration cases are decisive on the CPU
@pytest.mark.parametrize("kind", ["plain", "processed"])
@pytest.mark.parametrize("vocab", [A.V_SMALL, A.V_PROD])
def test_integration_case_seeds_excuse_nothing(kind, vocab):
    """tests/test_gpu_logit_adjust.py compares the device token of every row with the numpy one under the excuse rule of the
    sampling-kernel tests (top-2 gap above 1e-4, no truncation-boundary token).  With these seeds the numpy reference alone
    excuses no row, so the share of excused steps is zero; and the adjustments decide: no row keeps its unadjusted winner."""
    case = A.integration_case(kind, vocab)
    assert all(A.decisive(case)), case["ref"]
    assert A.V_SMALL % 64 != 0
    for b, (tok, _, _) in enumerate(case["ref"][:5]):
        banned = case["ids"][b, :3]
        assert tok not in banned or b == 4            # row 4 (n == min_tokens) may take a stop entry again
        assert np.isinf(case["adjusted"][b][banned[1]]) == (b != 4)
        if case["spec"][b][0] == 0 and case["spec"][b][4:] == (1, 0, 0):
            assert tok != int(np.argmax(case["logits"][b])) and tok == int(np.argmax(case["adjusted"][b]))
    np.testing.assert_array_equal(case["adjusted"][5], case["logits"][5])
