"""n > 1 and prompt reuse, host logic only: the slot scheduler against a fake engine that records `admit` / `admit_reuse`, request
validation of the chat front end, and the response shape through LocalServer (static and continuous)."""
from types import SimpleNamespace

import numpy as np
import pytest

from karanta_ocr_amd import image_processing as IP
from karanta_ocr_amd import serving as S
from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler

CFG = CONFIGS["tiny"]
EOS = int(CFG.eos_token_ids[0])


class Page:
    def __init__(self, ids, n=1, seed=0):
        self.input_ids, self.n, self.seed, self.grids = np.asarray(ids), n, seed, []


def sequence(ids, seed):
    """What the fake generates for (prompt, seed): ids[0] + 1 tokens with value 65 + seed % 26, then EOS — so the children of a page
    (seeds seed + c) differ from one another and a longer first id decodes for longer."""
    return [65 + seed % 26] * (int(ids[0]) + 1) + [EOS]


class FakeSlotEngine:
    """The Engine slot API with n and admit_reuse: every sequence follows `sequence(prompt, seed + child)`; what each slot holds
    (the prompt of its last admission) is remembered as the real engine's KV rows are."""
    cfg = CFG
    first_id = None      # set: every prompt generates as if it began with this id (the server tests' prompts are chat templates)

    def __init__(self, n_slots):
        self.B, self.log, self.pages_prefilled = n_slots, [], 0

    def begin_slots(self, max_new, sampling=False, **kw):
        B = self.B
        self.max_new, self.seq, self.gen, self.fin, self.hist = max_new, [None] * B, [0] * B, [True] * B, [[] for _ in range(B)]
        self.held = [None] * B

    def _start(self, j, page, c):
        assert self.fin[j], f"slot {j} is busy"
        ids = page.input_ids if self.first_id is None else [self.first_id]
        self.seq[j], self.hist[j], self.gen[j], self.fin[j] = sequence(ids, page.seed + c), [], 0, False
        self.held[j] = tuple(page.input_ids.tolist())
        self._emit(j)

    def admit(self, pages, slots, budgets=None):
        assert len(slots) == sum(p.n for p in pages) == len(set(slots))
        self.log.append(("admit", [p.n for p in pages], list(slots), [j for j in range(self.B) if not self.fin[j]]))
        self.pages_prefilled += len(pages)
        it = iter(slots)
        return [self._start(next(it), p, c) or len(p.input_ids) for p in pages for c in range(p.n)]

    def admit_reuse(self, pages, srcs, slots, budgets=None):
        assert len(srcs) == len(pages) and len(slots) == sum(p.n for p in pages)
        self.log.append(("reuse", list(srcs), list(slots)))
        it = iter(slots)
        for p, src in zip(pages, srcs):
            assert self.held[src] == tuple(p.input_ids.tolist()), "the source slot holds another prompt"
        return [self._start(next(it), p, c) or len(p.input_ids) for p in pages for c in range(p.n)]

    def _emit(self, j):
        if self.fin[j]:
            return
        tok = self.seq[j][self.gen[j]] if self.gen[j] < len(self.seq[j]) else 7
        self.hist[j].append(tok)
        self.gen[j] += 1
        self.fin[j] = tok == EOS

    def decode_steps(self, n):
        for _ in range(n):
            for j in range(self.B):
                self._emit(j)

    def poll_slots(self):
        return np.asarray(self.fin), np.asarray(self.gen)

    def slot_tokens(self, j, n):
        return np.asarray(self.hist[j][:n])

    def retire(self, j):
        self.fin[j] = True


def scheduler(n_slots, **kw):
    eng = FakeSlotEngine(n_slots)
    return eng, SlotScheduler(eng, max_tokens_cap=64, chunk=1, **kw)


def expect(page, c, limit=64):
    seq = sequence(page.input_ids, page.seed + c)[:limit]
    return seq, "stop" if seq[-1] == EOS else "length"


def test_a_request_takes_n_slots_and_answers_once_with_its_children_in_order():
    eng, sch = scheduler(4)
    page = Page([3, 1, 2], n=3, seed=5)
    res = sch.run([SlotRequest(page, 64, tag="a"), SlotRequest(Page([1]), 2, tag="b")])
    assert eng.log[0][:3] == ("admit", [3, 1], [0, 1, 2, 3]) and eng.pages_prefilled == 2
    a, b = res
    assert a.tag == "a" and a.error is None and len(a.choices) == 3 and b.choices is None
    for c, kid in enumerate(a.choices):
        toks, reason = expect(page, c)
        assert kid.tokens.tolist() == toks and kid.finish_reason == reason and kid.prompt_tokens == 3
    assert a.tokens.tolist() == a.choices[0].tokens.tolist() and a.finish_reason == a.choices[0].finish_reason
    assert b.tokens.tolist() == expect(b.request.page, 0, 2)[0] and b.finish_reason == "length"
    assert sch.sequences_admitted == 4 and sch.sequences_forked == 2 and sch.pages_admitted == 2


def test_the_queue_stays_fifo_and_a_childs_slot_is_free_as_soon_as_it_ends():
    """3 slots: A (n = 2, child 0 cut after two tokens by its stop matcher) runs, B (n = 2) needs two slots and waits although one
    is free, C (n = 1) does not overtake B; when A's short child ends, B starts beside A's long child."""
    eng, sch = scheduler(3)
    two_short = Page([0], n=2)                        # both children: 1 token + EOS
    a = SlotRequest(Page([9], n=2), 64, tag="a")      # 10 tokens + EOS per child
    a.stop_checks = [lambda t: 2 if len(t) >= 2 else None, None]      # child 0 ends after two tokens, child 1 runs on
    b, c = SlotRequest(two_short, 64, tag="b"), SlotRequest(Page([0]), 64, tag="c")
    for r in (a, b, c):
        sch.submit(r)
    out = []
    while not sch.idle:
        out += sch.step()
    admits = [e for e in eng.log if e[0] == "admit"]
    assert admits[0][1:3] == ([2], [0, 1]), "A alone: B does not fit the one slot left and C must not overtake it"
    assert admits[1] == ("admit", [2], [0, 2], [1]), "B: beside A's second child (slot 1), into the slot its first child left"
    assert admits[2] == ("admit", [1], [0], [1]), "C after B"
    assert [r.tag for r in out] == ["b", "c", "a"]
    ra = [r for r in out if r.tag == "a"][0]
    assert [len(k.tokens) for k in ra.choices] == [2, 11] and [k.finish_reason for k in ra.choices] == ["stop", "stop"]
    assert sum(1 for r in out if r.tag == "a") == 1, "one result per request"


def test_more_children_than_slots_is_a_client_error_for_that_request_alone():
    eng, sch = scheduler(2)
    res = sch.run([SlotRequest(Page([1], n=3), 8, tag="big"), SlotRequest(Page([1], n=2), 8, tag="ok")])
    assert res[0].status == 400 and "slots" in res[0].error and res[1].error is None and len(res[1].choices) == 2


def test_admit_min_counts_slots():
    eng, sch = scheduler(4, admit_min=3, admit_max_wait=50)
    sch.submit(SlotRequest(Page([20]), 64, tag="long"))
    sch.step()
    sch.submit(SlotRequest(Page([1], n=3), 64, tag="three"))       # one request, but three slots' worth of work: no waiting
    sch.step()
    assert [e[1] for e in eng.log if e[0] == "admit"] == [[1], [3]]


def test_engines_and_pages_without_n_behave_as_before():
    class Plain:
        def __init__(self, ids):
            self.input_ids, self.seed, self.grids = np.asarray(ids), 0, []
    eng, sch = scheduler(2)
    eng.admit = lambda pages, slots, budgets=None, _f=eng.admit: _f([Page(p.input_ids) for p in pages], slots)
    res = sch.run([SlotRequest(Plain([2]), 64), SlotRequest(Plain([0]), 64)])
    assert [r.choices for r in res] == [None, None] and [len(r.tokens) for r in res] == [4, 2]


def test_residency_reuse_and_eviction_order():
    eng, sch = scheduler(3, prefix_cache=True)
    k = lambda i: bytes([i]) * 16
    run1 = lambda page, key, limit=64: sch.run([SlotRequest(page, limit, prompt_key=key)])[0]
    p1, p2, p3, p4 = (Page([i, 7, 7]) for i in (1, 2, 3, 4))
    for p, key in ((p1, k(1)), (p2, k(2)), (p3, k(3))):
        run1(p, key)
    # slots without a resident prompt are taken first: the three prompts sit in slots 0, 1, 2
    assert [e[2] for e in eng.log] == [[0], [1], [2]] and sch._resident == {0: (k(1), 3), 1: (k(2), 3), 2: (k(3), 3)}
    # a hit runs in place: no admit, the source is the slot itself
    r = run1(Page([2, 7, 7], seed=4), k(2))
    assert eng.log[-1] == ("reuse", [1], [1]) and r.tokens.tolist() == sequence([2], 4) and sch.prefix_cache_hits == 1
    # a cold admission evicts the prompt that finished longest ago: slot 0 (slot 1 was used again since)
    run1(p4, k(4))
    assert eng.log[-1][:3] == ("admit", [1], [0]) and sch._resident[0] == (k(4), 3)
    # ... so the first prompt is a miss now, and takes the next oldest: slot 2
    run1(p1, k(1))
    assert eng.log[-1][:3] == ("admit", [1], [2]) and eng.pages_prefilled == 5
    # the same key with another prompt length is not the same prompt
    run1(Page([2, 7, 7, 7]), k(2))
    assert eng.log[-1][0] == "admit"
    # requests without a key, and schedulers without the option, never reuse
    run1(Page([4, 7, 7]), None)
    assert eng.log[-1][0] == "admit"
    eng2, sch2 = scheduler(2)
    for _ in range(2):
        sch2.run([SlotRequest(Page([1]), 8, prompt_key=k(1))])
    assert [e[0] for e in eng2.log] == ["admit", "admit"] and not sch2._resident


def test_reuse_forks_from_an_active_slot_and_serves_n_children():
    eng, sch = scheduler(4, prefix_cache=True)
    key = b"p" * 16
    first = SlotRequest(Page([30, 1]), 64, prompt_key=key, tag="first")
    sch.submit(first)
    sch.step()
    assert sch.active and eng.log[-1][:3] == ("admit", [1], [0])
    again = SlotRequest(Page([30, 1], n=2, seed=3), 64, prompt_key=key, tag="again")      # its prompt is in slot 0, which is busy
    sch.submit(again)
    out = []
    while not sch.idle:
        out += sch.step()
    assert eng.log[-1] == ("reuse", [0], [1, 2]) and eng.pages_prefilled == 1
    assert sch.prefix_cache_hits == 1 and sch.sequences_forked == 2 and sch.sequences_admitted == 3
    res = {r.tag: r for r in out}
    assert [kid.tokens.tolist() for kid in res["again"].choices] == [sequence([30], 3), sequence([30], 4)]
    assert res["first"].tokens.tolist() == sequence([30], 0)
    # all three slots hold the prompt now; an n = 2 request runs child 0 in place and forks one sibling
    sch.run([SlotRequest(Page([30, 1], n=2), 4, prompt_key=key)])
    kind, srcs, slots = eng.log[-1]
    assert kind == "reuse" and slots[0] == srcs[0] and len(slots) == 2 and eng.pages_prefilled == 1


def vision_message(seed=1, text="read this"):
    url = IP.encode_png_data_url(IP.synthetic_page(seed, 56, 84))
    return [{"role": "user", "content": [{"type": "text", "text": text}, {"type": "image_url", "image_url": {"url": url}}]}]


def test_request_validation():
    fe = S.ChatFrontend(CFG, S.ByteTokenizer(CFG))
    ok = {"messages": vision_message(), "max_tokens": 4, "temperature": 0.5}
    assert fe.parse(ok).n == 1 and fe.parse({**ok, "n": None}).n == 1 and fe.parse({**ok, "n": 3}).n == 3
    assert fe.parse({**ok, "n": 3, "best_of": 3}).n == 3 and fe.parse({**ok, "n": 1, "temperature": 0}).n == 1
    for bad in ({"n": True}, {"n": "2"}, {"n": 2.5}, {"n": 2.0}, {"n": 0}, {"n": -1}, {"n": 2, "temperature": 0}, {"n": 2, "temperature": None},
                {"n": 2, "best_of": 3}, {"best_of": 2}):
        with pytest.raises(S.BadRequest):
            fe.parse({**ok, **bad})
    # prompt keys: off by default; 16 bytes over prompt ids, grids and image bytes when on
    assert fe.parse(ok).prompt_key is None
    fe.prompt_keys = True
    a, b = fe.parse(ok).prompt_key, fe.parse({**ok, "temperature": 0.9, "seed": 5, "max_tokens": 9}).prompt_key
    assert isinstance(a, bytes) and len(a) == 16 and a == b, "sampling fields are not part of the prompt"
    assert fe.parse({**ok, "messages": vision_message(2)}).prompt_key != a, "another image"
    assert fe.parse({**ok, "messages": vision_message(1, "read that")}).prompt_key != a, "another text"
    dev = S.ChatFrontend(CFG, S.ByteTokenizer(CFG), device_images=True)
    dev.prompt_keys = True
    assert len(dev.parse(ok).prompt_key) == 16 and dev.parse(ok).prompt_key == dev.parse(ok).prompt_key


class StaticEngine:
    """generate() with n: per sequence `sequence(prompt, seed + c)`, as the real engine's rows."""
    B, cfg = 4, CFG

    def __init__(self):
        self.calls = []

    def generate(self, pages, max_new_tokens, **kw):
        self.calls.append([p.n for p in pages])
        assert sum(p.n for p in pages) <= self.B
        toks = [np.asarray(sequence([2], p.seed + c)[:max_new_tokens], np.int64) for p in pages for c in range(p.n)]
        return SimpleNamespace(tokens=toks, finish_reasons=["stop" if t[-1] == EOS else "length" for t in toks],
                               prompt_tokens=[len(p.input_ids) for p in pages for _ in range(p.n)])


class ContinuousEngine(FakeSlotEngine):
    first_id = 2


@pytest.mark.parametrize("continuous", [False, True], ids=["static", "continuous"])
def test_response_shape_through_the_server(continuous):
    eng = ContinuousEngine(4) if continuous else StaticEngine()
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, continuous=continuous, max_tokens_cap=16)
    req = {"messages": vision_message(), "max_tokens": 8, "temperature": 0.7, "seed": 10}
    st, body = srv.chat_completions({**req, "n": 3})
    assert st == 200 and [c["index"] for c in body["choices"]] == [0, 1, 2]
    assert [c["message"]["content"] for c in body["choices"]] == [chr(65 + 10 + c) * 3 for c in range(3)]
    assert all(c["finish_reason"] == "stop" for c in body["choices"])
    n_in = body["usage"]["prompt_tokens"]
    assert n_in == len(srv.frontend.parse(req).input_ids) and body["usage"]["completion_tokens"] == 9     # 3 x 3 (EOS not counted)
    assert body["usage"]["total_tokens"] == n_in + 9
    st, one = srv.chat_completions(req)
    assert st == 200 and len(one["choices"]) == 1 and one["choices"][0]["message"]["content"] == "KKK"
    assert one["usage"] == {"prompt_tokens": n_in, "completion_tokens": 3, "total_tokens": n_in + 3}
    # without a seed the children still take consecutive seeds from one base
    st, body = srv.chat_completions({k: v for k, v in {**req, "n": 3}.items() if k != "seed"})
    letters = [ord(c["message"]["content"][0]) - 65 for c in body["choices"]]
    assert st == 200 and [(x - letters[0]) % 26 for x in letters] == [0, 1, 2]
    for bad in ({"n": 5}, {"n": 0}, {"n": 2, "temperature": 0}, {"n": 2, "best_of": 1}, {"n": "3"}):
        st, err = srv.chat_completions({**req, **bad})
        assert st == 400 and "error" in err, bad
    srv.close()
    # --greedy serves n as 1
    eng = ContinuousEngine(4) if continuous else StaticEngine()
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, continuous=continuous, max_tokens_cap=16,
                        honor_temperature=False)
    st, body = srv.chat_completions({**req, "n": 3})
    assert st == 200 and len(body["choices"]) == 1
    srv.close()


def test_static_batches_are_packed_by_sequences():
    import threading
    eng = StaticEngine()
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, batch_wait_s=0.3)
    req = {"messages": vision_message(), "max_tokens": 4, "temperature": 0.7, "seed": 1, "n": 3}
    got = [None] * 3
    ts = [threading.Thread(target=lambda i=i: got.__setitem__(i, srv.chat_completions(req))) for i in range(3)]
    [t.start() for t in ts]; [t.join() for t in ts]
    srv.close()
    assert all(st == 200 and len(b["choices"]) == 3 for st, b in got)
    assert all(sum(c) <= 4 for c in eng.calls) and sum(sum(c) for c in eng.calls) == 9


def test_prefix_caching_flag_and_metrics():
    from karanta_ocr_amd import cli
    a = cli.parse_args(["serve", "/models/x", "--enable-prefix-caching"])
    assert a.enable_prefix_caching and "--enable-prefix-caching" not in a.ignored
    eng = ContinuousEngine(2)
    srv = S.LocalServer(eng, S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, continuous=True, max_tokens_cap=16,
                        prefix_cache=True)
    req = {"messages": vision_message(), "max_tokens": 8, "temperature": 0.7, "seed": 10}
    assert srv.prefix_cache and srv.frontend.prompt_keys
    assert srv.chat_completions(req)[0] == 200 and srv.chat_completions({**req, "seed": 11, "n": 2})[0] == 200
    stats = srv.metrics()[1]["scheduler"]
    assert stats["prefix_cache_hits"] == 1 and stats["sequences_admitted"] == 3 and stats["sequences_forked"] == 1
    assert [e[0] for e in eng.log] == ["admit", "reuse"]
    srv.close()
    static = S.LocalServer(StaticEngine(), S.ChatFrontend(CFG, S.ByteTokenizer(CFG)), log=lambda *_: None, prefix_cache=True)
    assert not static.prefix_cache, "prompt reuse applies in continuous mode only"
    static.close()
