"""Sampling controls on the host (no GPU): the six vLLM fields reach PageRequest through the server with vLLM's validation,
--greedy ignores them, StepFeatures decides the passes a set of pages needs, and the slot scheduler switches the passes with
the requests in the slots, the overlapped admission in flight included."""
from types import SimpleNamespace

import numpy as np
import pytest

from karanta_ocr_amd import serving as S
from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.engine import PageRequest
from karanta_ocr_amd.sampling import NEUTRAL, StepFeatures, needs_processing, sampling_params
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler

CFG = CONFIGS["tiny"]
MSG = [{"role": "user", "content": "x"}]
FIELDS = dict(top_k=7, top_p=0.85, min_p=0.05, repetition_penalty=1.1, frequency_penalty=0.5, presence_penalty=-0.25)


class RecordingEngine:
    """Static-mode stand-in: answers b"OK<eos>" and keeps the pages it was given."""
    B = 4
    cfg = CFG

    def __init__(self):
        self.pages = []

    def generate(self, pages, max_new_tokens, **kw):
        self.pages += list(pages)
        full = np.asarray(list(b"OK") + [CFG.eos_token_ids[0]], np.int64)
        return SimpleNamespace(tokens=[full] * len(pages), finish_reasons=["stop"] * len(pages),
                               prompt_tokens=[len(p.input_ids) for p in pages])


@pytest.fixture
def server():
    srv = S.LocalServer(RecordingEngine(), S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None)
    yield srv
    srv.close()


def test_fields_reach_the_page(server):
    assert server.chat_completions({"messages": MSG, "temperature": 0.7, "seed": 3, **FIELDS})[0] == 200
    p = server.engine.pages[-1]
    for k, v in FIELDS.items():
        assert getattr(p, k) == pytest.approx(v), k
    assert needs_processing(p)
    np.testing.assert_allclose(sampling_params(p)[:6], [7, 0.85, 0.05, 1.1, 0.5, -0.25], rtol=1e-6)
    # penalties apply to greedy requests as well
    assert server.chat_completions({"messages": MSG, "repetition_penalty": 1.2})[0] == 200
    assert server.engine.pages[-1].repetition_penalty == pytest.approx(1.2) and server.engine.pages[-1].temperature == 0.0


@pytest.mark.parametrize("extra", [{}, {k: None for k in FIELDS}, dict(NEUTRAL), {"top_k": -1}])
def test_absent_or_neutral_fields_leave_the_page_as_today(server, extra):
    assert server.chat_completions({"messages": MSG, "temperature": 0.5, "seed": 9, **extra})[0] == 200
    p = server.engine.pages[-1]
    ref = PageRequest(p.input_ids, p.pixel_values, p.grids, temperature=p.temperature, seed=p.seed, images=p.images)
    assert p == ref
    assert not needs_processing(p)


@pytest.mark.parametrize("bad", [
    {"top_p": 0}, {"top_p": 1.5}, {"top_p": -0.1}, {"top_p": float("nan")}, {"top_k": -2}, {"top_k": 2.5}, {"top_k": "5"},
    {"min_p": -0.01}, {"min_p": 1.01}, {"repetition_penalty": 0}, {"repetition_penalty": -1.0},
    {"repetition_penalty": float("inf")}, {"frequency_penalty": 2.5}, {"frequency_penalty": -2.01}, {"presence_penalty": 3},
    {"presence_penalty": -2.5}, {"top_p": "0.9"}, {"min_p": [0.1]}, {"repetition_penalty": True}, {"frequency_penalty": {}},
])
def test_invalid_values_are_400(server, bad):
    n = len(server.engine.pages)
    code, body = server.chat_completions({"messages": MSG, **bad})
    assert code == 400, (bad, body)
    assert len(server.engine.pages) == n


def test_boundary_values_are_accepted(server):
    for ok in ({"top_p": 1.0}, {"top_p": 1e-6}, {"top_k": 0}, {"top_k": 1}, {"top_k": 3.0}, {"min_p": 0}, {"min_p": 1},
               {"frequency_penalty": -2}, {"presence_penalty": 2}, {"repetition_penalty": 0.5}):
        assert server.chat_completions({"messages": MSG, "temperature": 1.0, **ok})[0] == 200, ok


def test_honor_temperature_off_ignores_the_fields():
    eng = RecordingEngine()
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, honor_temperature=False)
    try:
        assert srv.chat_completions({"messages": MSG, "temperature": 0.9, **FIELDS})[0] == 200
    finally:
        srv.close()
    p = eng.pages[-1]
    assert not needs_processing(p) and p.temperature == 0.0


# ----------------------------------------------------------------------------- StepFeatures
def test_step_features_of_pages():
    of = lambda **kw: StepFeatures.of([SimpleNamespace(**kw)])
    assert StepFeatures.of([]) == of() == StepFeatures(False, False, False)
    for t in (None, 0, 0.0):
        assert of(temperature=t) == StepFeatures()
    assert of(temperature=0.5) == StepFeatures(True, False, False)
    assert of(guide="x") == of(guide="x", temperature=0.0) == StepFeatures(True, True, False)     # guided implies sampling
    assert of(guide=None, temperature=None) == StepFeatures()
    for k, v in FIELDS.items():
        assert of(**{k: v}) == StepFeatures(False, False, True), k
        assert of(**{k: NEUTRAL[k]}) == of(**{k: None}) == StepFeatures(), k
    assert of(top_k=-1) == StepFeatures()


def test_step_features_union_and_clamp():
    S_, G, P = StepFeatures(True, False, False), StepFeatures(True, True, False), StepFeatures(False, False, True)
    assert S_ | P == StepFeatures(True, False, True) and G | S_ == G and StepFeatures() | P == P
    pages = [SimpleNamespace(temperature=0.3), SimpleNamespace(guide="x"), SimpleNamespace(min_p=0.1)]
    assert StepFeatures.of(pages) == StepFeatures.of(pages[:1]) | StepFeatures.of(pages[1:2]) | StepFeatures.of(pages[2:])
    everything = StepFeatures(True, True, True)
    assert everything & StepFeatures() == StepFeatures()
    assert everything & StepFeatures(True, False, True) == StepFeatures(True, False, True)
    assert StepFeatures(False, True, False) & everything == G             # a guided step keeps the pass it is masked in
    assert StepFeatures(False, True, False) & StepFeatures(True, False, True) == StepFeatures()
    assert P & G == StepFeatures() and G & G == G


# ----------------------------------------------------------------------------- scheduler: the step features
class Page:
    def __init__(self, key, **kw):
        self.input_ids = np.asarray([key, 0])
        self.pixel_values, self.grids = None, []
        for k, v in kw.items():
            setattr(self, k, v)


class FeatureEngine:
    """Slot engine with the overlapped-admission API and set_step_features(s, g, processing); a page emits input_ids[0]
    tokens then EOS.  Records the StepFeatures every decode chunk and every admission's first token run with."""
    class cfg:
        eos_token_ids = (99,)

    latency = 2

    def __init__(self, n_slots):
        self.B = n_slots
        self.features = StepFeatures()
        self.log, self.eos_at = [], []

    def begin_slots(self, max_new, sampling=False, guided=False, logprobs=None):
        self.seq, self.gen, self.fin = [None] * self.B, [0] * self.B, [True] * self.B
        self.hist = [[] for _ in range(self.B)]

    def set_step_features(self, sampling, guided, processing=False):
        self.features = StepFeatures(sampling, guided, processing)
        self.log.append(("features", self.features))

    def admit(self, pages, slots):
        for p, j in zip(pages, slots):
            self.seq[j] = [5] * int(p.input_ids[0]) + [99]
            self.hist[j], self.gen[j], self.fin[j] = [], 0, False
            self._emit(j)
        return [len(p.input_ids) for p in pages]

    def admit_begin(self, pages, slots):
        need = StepFeatures.of(pages)
        self.log.append(("begin", need, list(slots)))
        self.features |= need       # like Engine.prefill: an admission switches on what it needs by itself
        return {"pages": pages, "slots": list(slots), "polls": 0}

    def admit_ready(self, h):
        h["polls"] += 1
        return h["polls"] > self.latency

    def admit_end(self, h):
        # the first token of the admission is sampled with the features the steps carry now
        self.log.append(("end", self.features, StepFeatures.of(h["pages"])))
        return self.admit(h["pages"], h["slots"])

    def _emit(self, j):
        if self.fin[j]:
            return
        tok = self.seq[j][min(self.gen[j], len(self.seq[j]) - 1)]
        self.hist[j].append(tok)
        self.gen[j] += 1
        self.fin[j] = tok == 99
        if self.fin[j]:
            self.eos_at.append((len(self.log), j))    # (log position, slot)

    def decode_steps(self, n):
        self.log.append(("steps", self.features))
        for _ in range(n):
            for j in range(self.B):
                self._emit(j)

    def poll_slots(self):
        return np.asarray(self.fin), np.asarray(self.gen)

    def slot_tokens(self, j, n):
        return np.asarray(self.hist[j][:n])

    def retire(self, j):
        self.fin[j] = True


def test_processing_follows_the_slots_and_the_admission_in_flight():
    eng = FeatureEngine(2)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=2, sampling=True, overlap=True)
    assert sch.overlap
    reqs = [SlotRequest(Page(30), 40, tag="plain-long"), SlotRequest(Page(4, top_p=0.9), 10, tag="proc-short"),
            SlotRequest(Page(6, repetition_penalty=1.2), 10, tag="proc-2"), SlotRequest(Page(5), 10, tag="plain-2")]
    res = sch.run(reqs)
    assert all(r.error is None for r in res)
    # every processed admission's first token ran with processing on, although the slots held no processed request
    ends = [e for e in eng.log if e[0] == "end"]
    assert any(e[2].processing for e in ends) and all(e[1].processing for e in ends if e[2].processing)
    # a processed admission begun while only plain requests decode switches processing on for the chunks in between
    i = next(k for k, e in enumerate(eng.log) if e[0] == "begin" and e[1].processing)
    j = next(k for k in range(i, len(eng.log)) if eng.log[k][0] == "end")
    assert all(e[1].processing for e in eng.log[i:j] if e[0] == "steps")
    # ... and off again once the last processed request has left (the long plain one keeps decoding)
    steps = [e[1].processing for e in eng.log if e[0] == "steps"]
    assert True in steps and steps[-1] is False
    assert eng.log[-1][0] == "steps" and not eng.features.processing


def test_processing_stays_off_for_plain_traffic():
    eng = FeatureEngine(2)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=2, sampling=True, overlap=True)
    sch.run([SlotRequest(Page(3, temperature=0.5), 8, tag=i) for i in range(3)])
    assert not any(e[1].processing for e in eng.log if e[0] == "steps")


def test_guided_admission_in_flight_keeps_its_passes():
    """guided C finishes while guided B is between admit_begin and admit_end and plain A decodes.  The
    chunks in between must keep the guided / sampling passes that B's first token needs, not switch them off with C."""
    eng = FeatureEngine(3)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=2, sampling=True, guided=True, overlap=True)
    a, c, b = (SlotRequest(Page(30), 40, tag="plain-A"), SlotRequest(Page(5, guide="x"), 10, tag="guided-C"),
               SlotRequest(Page(6, guide="y", temperature=0.7), 10, tag="guided-B"))
    sch.submit(a)
    sch.submit(c)
    done = []
    while len(sch.active) < 2:
        done += sch.step()
    sch.submit(b)
    while not sch.idle:
        done += sch.step()
    assert sorted(r.tag for r in done) == ["guided-B", "guided-C", "plain-A"] and all(r.error is None for r in done)
    i = next(k for k, e in enumerate(eng.log) if e[0] == "begin" and e[2] == [2])     # B's admission (A, C: slots 0, 1)
    j = next(k for k in range(i, len(eng.log)) if eng.log[k][0] == "end")
    assert any(i < k <= j and slot == 1 for k, slot in eng.eos_at), "the scenario needs C (slot 1) to finish while B is in flight"
    assert eng.log[j][2] == StepFeatures(True, True, False)
    assert eng.log[j][1].guided and eng.log[j][1].sampling, eng.log[i:j + 1]
    assert all(e[1].guided for e in eng.log[i:j] if e[0] == "steps")
