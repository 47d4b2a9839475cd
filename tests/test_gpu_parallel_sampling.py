"""n > 1 and repeated pages on the engine: a page with n = k is exactly k copies of it with seeds seed + c — tokens, logits and
log-probabilities — although it is prefilled once and its siblings start from forked KV rows (kr_kv_fork); a request whose prompt
is still resident in a slot starts from that slot (Engine.admit_reuse).  Every comparison is an exact equality: the engine's
tokens do not depend on the batch a sequence runs in, so a child can be compared with its solo run.

Prompt lengths sit on both sides of a V^T block boundary (64 keys): P < 64, P = 64, 64 < P < 128."""
import dataclasses
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd.engine import Engine, PageRequest  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler  # noqa: E402

MODELS = ["tiny", "tiny-gqa"]
LENGTHS = [40, 64, 100]
PATTERN = r"[a-f]{3}-[0-9]{2}(?:;[a-z ]{2,5})?"


def make_engine(cfg, w, max_batch=4, **kw):
    e = Engine(cfg, max_batch=max_batch, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2, **kw)
    e.load_weights(w)
    return e


@pytest.fixture(scope="module")
def engines(tiny_models):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from karanta_ocr_amd.serving import ByteTokenizer
    out = {}
    for name in MODELS:
        cfg, w, _ = tiny_models[name]
        out[name] = make_engine(cfg, w)
        out[name].set_vocab(ByteTokenizer(cfg).token_bytes())
    yield out
    for e in out.values():
        e.close()


def page_of(cfg, P, variant=0, **kw):
    """A page whose prompt has exactly P tokens: text, one 56 x 84 image (6 image tokens), text.  `variant` picks the image and
    the text; the sampler's seed and everything else of the request goes through `kw`."""
    pv, grid = IP.image_to_patches(IP.synthetic_page(30 + variant, 56, 84))
    T = grid[1] * grid[2] // 4
    rng = np.random.default_rng(1000 + P + variant)
    pre = (P - T - 2) // 2
    ids = np.concatenate([rng.integers(0, 400, pre), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                          [cfg.vision_end_token_id], rng.integers(0, 400, P - T - 2 - pre)]).astype(np.int64)
    assert len(ids) == P
    return PageRequest(ids, pv, [grid], **kw)


def copies(page, n=None):
    n = page.n if n is None else n
    return [dataclasses.replace(page, n=1, seed=(page.seed + c) & 0xFFFFFFFF) for c in range(n)]


def hot(eng, page):
    """The temperature of test_sampled_generation_matches_oracle: hot enough that the noise decides."""
    lg = eng.generate([dataclasses.replace(page, n=1, temperature=0.0)], 1, ignore_eos=True, return_logits=True).logits
    return max(0.9, 0.3 * float(np.abs(lg[0, 0]).max()))


def assert_same(a, b, rows_a, rows_b, what=""):
    for i, j in zip(rows_a, rows_b):
        np.testing.assert_array_equal(a.tokens[i], b.tokens[j], err_msg=f"{what} tokens {i} / {j}")
        assert a.finish_reasons[i] == b.finish_reasons[j]
        la = a.logprobs[i] if a.logprobs is not None else None
        lb = b.logprobs[j] if b.logprobs is not None else None
        assert (la is None) == (lb is None)
        if la is not None:
            for key in ("token", "top", "top_ids"):
                np.testing.assert_array_equal(la[key], lb[key], err_msg=f"{what} logprobs {key} {i} / {j}")


@pytest.mark.parametrize("P", LENGTHS)
@pytest.mark.parametrize("name", MODELS)
def test_greedy_children_are_bit_equal(engines, tiny_models, name, P):
    cfg = tiny_models[name][0]
    eng = engines[name]
    one = eng.generate([page_of(cfg, P)], 12, ignore_eos=True, return_logits=True)
    three = eng.generate([page_of(cfg, P, n=3)], 12, ignore_eos=True, return_logits=True)
    assert three.logits.shape[0] == 3 and len(three.tokens) == 3 and three.prompt_tokens == [P] * 3
    for c in (1, 2):
        np.testing.assert_array_equal(three.logits[c].view(np.uint32), three.logits[0].view(np.uint32), err_msg=f"child {c}")
    np.testing.assert_array_equal(three.logits[0].view(np.uint32), one.logits[0].view(np.uint32))
    for c in range(3):
        np.testing.assert_array_equal(three.tokens[c], one.tokens[0])


@pytest.mark.parametrize("P", LENGTHS)
@pytest.mark.parametrize("name", MODELS)
def test_sampled_children_equal_explicit_copies(engines, tiny_models, name, P):
    cfg = tiny_models[name][0]
    eng = engines[name]
    page = page_of(cfg, P, seed=0xFFFFFFFE, logprobs=3, n=4)          # the seeds wrap: s, s + 1, 0, 1
    page.temperature = hot(eng, page)
    before = eng.pages_prefilled
    forked = eng.generate([page], 14, ignore_eos=True)
    assert eng.pages_prefilled - before == 1
    before = eng.pages_prefilled
    explicit = eng.generate(copies(page), 14, ignore_eos=True)
    assert eng.pages_prefilled - before == 4
    assert copies(page)[2].seed == 0
    assert_same(forked, explicit, range(4), range(4), "n = 4 against four copies")
    for c, child in enumerate(copies(page)):
        assert_same(forked, eng.generate([child], 14, ignore_eos=True), [c], [0], f"child {c} against its solo run")
    assert len({tuple(t.tolist()) for t in forked.tokens}) >= 2, "the children sample with different seeds"


def test_per_child_sampler_state(engines, tiny_models):
    """Penalty counts, adjustment tables and the DFA state are per slot: every child of a forked page has its own."""
    cfg = tiny_models["tiny"][0]
    eng = engines["tiny"]
    base = page_of(cfg, 64, variant=7)
    T = hot(eng, base)
    first = int(eng.generate([base], 1, ignore_eos=True).tokens[0][0])
    cases = {
        "penalties": dataclasses.replace(base, n=2, temperature=T, repetition_penalty=1.3, frequency_penalty=0.7),
        "bias and min_tokens": dataclasses.replace(base, n=2, temperature=T, logit_bias={first: -50.0, 17: 4.0}, min_tokens=5,
                                                   stop_token_ids=(first,)),
        "guide": dataclasses.replace(base, n=2, temperature=T, guide=PATTERN),
    }
    voc = None
    for what, page in cases.items():
        forked = eng.generate([page], 16)
        explicit = eng.generate(copies(page), 16)
        assert_same(forked, explicit, range(2), range(2), what)
        if what == "guide":
            from karanta_ocr_amd.serving import ByteTokenizer
            voc = ByteTokenizer(cfg).token_bytes()
            for toks, reason in zip(forked.tokens, forked.finish_reasons):
                assert reason == "stop"
                assert re.fullmatch(PATTERN.encode(), b"".join(voc[int(t)] for t in toks[:-1])), toks


def test_children_in_the_packed_family():
    """17..32 rows (tiny-w512, max_batch 20): two pages with n = 10 decode as 20 forked rows, equal to the 20 explicit copies."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.weights import random_weights
    cfg = CONFIGS["tiny-w512"]
    eng = make_engine(cfg, random_weights(cfg, 909), max_batch=20)
    assert eng.family32
    pages = [page_of(cfg, 64, variant=1, n=10), page_of(cfg, 100, variant=2, n=10)]
    for p in pages:
        p.temperature = hot(eng, p)
    before = eng.pages_prefilled
    forked = eng.generate(pages, 10, ignore_eos=True)
    assert eng.pages_prefilled - before == 2 and eng.sequences_forked == 18
    explicit = eng.generate(copies(pages[0]) + copies(pages[1]), 10, ignore_eos=True)
    assert_same(forked, explicit, range(20), range(20))
    assert len({tuple(t.tolist()) for t in forked.tokens}) >= 4
    eng.close()


def _scheduler_setup(tiny_models, name="tiny"):
    """Six pages of ragged prompts, sampled; an EOS set that some free-running children hit early, some late, some never (as in
    test_slot_scheduler_equals_solo_generation); an engine with that EOS set."""
    cfg, w, _ = tiny_models[name]
    base = make_engine(cfg, w)
    ns, limits = [1, 3, 1, 2, 4, 1], [9, 20, 5, 14, 11, 17]
    pages = []
    for i, (n, P) in enumerate(zip(ns, [40, 64, 100, 33, 65, 90])):
        p = page_of(cfg, P, variant=100 + 10 * i, n=n)
        p.temperature = hot(base, p)
        pages.append(p)
    free = [base.generate([ch], 20, ignore_eos=True).tokens[0] for ch in [copies(pages[1])[1], copies(pages[4])[0], copies(pages[4])[3]]]
    base.close()
    eos = (int(free[0][4]), int(free[1][8]), int(free[2][2]))
    eng = make_engine(dataclasses.replace(cfg, eos_token_ids=eos), w)
    return eng, pages, ns, limits


@pytest.mark.parametrize("overlap", [False, True])
def test_scheduler_serves_children_in_their_own_slots(tiny_models, overlap):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    eng, pages, ns, limits = _scheduler_setup(tiny_models)
    solo = [[eng.generate([ch], mt) for ch in copies(pg)] for pg, mt in zip(pages, limits)]
    sch = SlotScheduler(eng, max_tokens_cap=20, chunk=3, sampling=True, overlap=overlap)
    assert sch.overlap == overlap and sch.n_slots == 4
    admitted = []                      # (slots of the admission, slots that were busy when it was made)
    for meth in ("admit", "admit_begin"):
        def spy(pgs, slots, *a, _f=getattr(eng, meth), **k):
            admitted.append(([p.n for p in pgs], list(slots), sorted(sch.active)))
            return _f(pgs, slots, *a, **k)
        setattr(eng, meth, spy)
    before = eng.pages_prefilled
    reqs = [SlotRequest(pg, mt, tag=i) for i, (pg, mt) in enumerate(zip(pages, limits))]
    too_many = SlotRequest(dataclasses.replace(pages[0], n=5), 4, tag="n5")
    res = sch.run(reqs + [too_many])
    assert eng.pages_prefilled - before == 6 and sch.sequences_admitted == sum(ns) and sch.sequences_forked == sum(ns) - 6
    assert res[-1].status == 400 and res[-1].error and "5" in res[-1].error
    reasons = set()
    for i, (r, n) in enumerate(zip(res[:-1], ns)):
        assert r.error is None and r.tag == i and r.prompt_tokens == len(pages[i].input_ids)
        kids = r.choices if n > 1 else [r]
        assert (r.choices is None) == (n == 1) and len(kids) == n
        for c, (kid, s) in enumerate(zip(kids, solo[i])):
            np.testing.assert_array_equal(kid.tokens, s.tokens[0], err_msg=f"request {i} child {c}")
            assert kid.finish_reason == s.finish_reasons[0]
            reasons.add(kid.finish_reason)
        np.testing.assert_array_equal(r.tokens, kids[0].tokens)
    assert reasons == {"stop", "length"}, "the construction should exercise both ways out of a slot"
    four = [a for a in admitted if 4 in a[0]]
    assert len(four) == 1 and four[0][0] == [4] and sorted(four[0][1]) == [0, 1, 2, 3] and four[0][2] == [], four
    eng.close()


def test_prompt_reuse(tiny_models):
    """prefix_cache: a hit in place, a fork from an active slot, a miss after eviction — always the solo run's tokens."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, w, _ = tiny_models["tiny"]
    eng = make_engine(cfg, w)
    page = page_of(cfg, 100, variant=5)
    page.temperature = hot(eng, page)
    retry = dataclasses.replace(page, seed=77, temperature=1.5 * page.temperature)     # the same prompt, sampled differently
    others = [page_of(cfg, 40 + i, variant=20 + i, temperature=page.temperature) for i in range(4)]
    solo = {k: eng.generate([p], 12).tokens[0] for k, p in (("page", page), ("retry", retry))}
    long_solo = eng.generate([page], 20).tokens[0]
    sch = SlotScheduler(eng, max_tokens_cap=20, chunk=2, sampling=True, prefix_cache=True)
    assert sch.prefix_cache
    key = b"k" * 16
    # twice in a row: the second is a hit, in place
    r1 = sch.run([SlotRequest(page, 12, prompt_key=key)])[0]
    slot = next(iter(sch._resident))
    before = (eng.pages_prefilled, eng.sequences_forked)
    r2 = sch.run([SlotRequest(retry, 12, prompt_key=key)])[0]
    assert (eng.pages_prefilled, eng.sequences_forked) == before and sch.prefix_cache_hits == 1 and eng.sequences_reused == 1
    assert list(sch._resident) == [slot]
    np.testing.assert_array_equal(r1.tokens, solo["page"])
    np.testing.assert_array_equal(r2.tokens, solo["retry"])
    # while the first is still decoding: forked from the active slot
    a, b = SlotRequest(page, 20, prompt_key=key), SlotRequest(retry, 12, prompt_key=key)
    sch.submit(a)
    got = sch.step() + sch.step()
    assert not got and len(sch.active) == 1, "the first request must still be decoding"
    sch.submit(b)
    while not sch.idle:
        got += sch.step()
    assert eng.pages_prefilled == before[0] and eng.sequences_forked == before[1] + 1 and sch.prefix_cache_hits == 3
    by_req = {id(r.request): r for r in got}
    np.testing.assert_array_equal(by_req[id(a)].tokens, long_solo)
    np.testing.assert_array_equal(by_req[id(b)].tokens, solo["retry"])
    # after every slot was given to another prompt: a miss
    for r in sch.run([SlotRequest(p, 6, prompt_key=bytes([i]) * 16) for i, p in enumerate(others)]):
        assert r.error is None
    assert key not in [e[0] for e in sch._resident.values()]
    before = eng.pages_prefilled
    r3 = sch.run([SlotRequest(page, 12, prompt_key=key)])[0]
    assert eng.pages_prefilled == before + 1 and sch.prefix_cache_hits == 3
    np.testing.assert_array_equal(r3.tokens, solo["page"])
    # the engine refuses a source that holds another prompt
    from karanta_ocr_amd._lib import KarantaHipError
    with pytest.raises(KarantaHipError, match="holds a prompt"):
        eng.admit_reuse([others[0]], [[j for j, e in sch._resident.items() if e[0] == key][0]], [3])
    eng.close()


@pytest.mark.parametrize("continuous", [True, False], ids=["continuous", "static"])
def test_server_returns_n_choices(tiny_models, continuous):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from karanta_ocr_amd import serving as S
    cfg, w, _ = tiny_models["tiny"]
    eng = make_engine(cfg, w)
    srv = S.LocalServer(eng, S.ChatFrontend(cfg, S.ByteTokenizer(cfg)), log=lambda *_: None, continuous=continuous,
                        max_tokens_cap=16, chunk=2, max_logprobs=2)
    url = IP.encode_png_data_url(IP.synthetic_page(44, 56, 84))
    req = {"messages": [{"role": "user", "content": [{"type": "text", "text": "page"}, {"type": "image_url", "image_url": {"url": url}}]}],
           "max_tokens": 10, "temperature": 40.0, "seed": 11, "logprobs": True, "top_logprobs": 2}
    st, body = srv.chat_completions({**req, "n": 3})
    assert st == 200 and [c["index"] for c in body["choices"]] == [0, 1, 2]
    total = 0
    for c, choice in enumerate(body["choices"]):
        st1, one = srv.chat_completions({**req, "seed": 11 + c})
        assert st1 == 200 and len(one["choices"]) == 1
        assert choice["message"]["content"] == one["choices"][0]["message"]["content"]
        assert choice["finish_reason"] == one["choices"][0]["finish_reason"]
        assert choice["logprobs"] == one["choices"][0]["logprobs"] and choice["logprobs"]["content"]
        assert one["usage"]["prompt_tokens"] == body["usage"]["prompt_tokens"]
        total += one["usage"]["completion_tokens"]
    assert body["usage"]["completion_tokens"] == total
    assert body["usage"]["total_tokens"] == body["usage"]["prompt_tokens"] + total
    assert len({c["message"]["content"] for c in body["choices"]}) >= 2
    for bad in ({"n": True}, {"n": "2"}, {"n": 2.5}, {"n": 0}, {"n": 2, "temperature": 0.0}, {"n": 2, "best_of": 3}, {"n": 5}):
        st, err = srv.chat_completions({**req, **bad})
        assert st == 400 and "error" in err, bad
    srv.close()
    eng.close()
