"""Speculative decode steps on the engine and through the slot scheduler: with speculation on, every request returns exactly the
tokens it returns with speculation off — greedy and sampled, whatever is accepted.  The baseline is the same engine class built
without `speculative`.  Scripted drafts (Engine.set_draft_script) make the acceptance pattern a choice of the test; the counters are
compared with tests/spec_ref.simulate.  Every comparison is an exact integer equality."""
import dataclasses
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError  # noqa: E402
from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests import spec_ref as R  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402

LENGTHS = [40, 64, 100]
MODELS = [("tiny-w512", "bf16"), ("tiny-w512", "fp8"), ("tiny-w3584", "bf16")]
LAYOUTS = [(5, 3), (8, 3), (4, 1)]            # (max_batch, K): 20 and 32 rows, and 8 rows run as 17
PATTERN = r"[a-f]{3}-[0-9]{2}(?:;[a-z ]{2,5})?"

_WEIGHTS, _ENGINES = {}, {}


def weights(name):
    if name not in _WEIGHTS:
        _WEIGHTS[name] = random_weights(CONFIGS[name], 909)
    return _WEIGHTS[name]


def engine_pair(name, dtype, B, K, n_min=2, n_max=4):
    """(plain engine, speculative engine) of one configuration, kept for the module."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    key = (name, dtype, B, K, n_min, n_max)
    if key not in _ENGINES:
        while len(_ENGINES) >= 16:
            for e in _ENGINES.pop(next(iter(_ENGINES))):
                e.close()
        kw = dict(max_batch=B, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2, weight_dtype=dtype)
        pair = (Engine(CONFIGS[name], **kw), Engine(CONFIGS[name], speculative=SpecConfig(K, n_min, n_max), **kw))
        for e in pair:
            e.load_weights(weights(name))
        _ENGINES[key] = pair
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for pair in _ENGINES.values():
        for e in pair:
            e.close()
    _ENGINES.clear()


def pages_for(cfg, B, **kw):
    return [page_of(cfg, LENGTHS[b % 3], variant=b, **kw) for b in range(B)]


def plain_run(eng, pages, n_tokens, sampling=False):
    """Slot mode, plain steps: per slot the first n_tokens generated tokens (fewer where an EOS ended the sequence)."""
    eng.begin_slots(n_tokens + 8, sampling=sampling)
    eng.admit(pages, list(range(len(pages))))
    eng.decode_steps(n_tokens - 1)
    _, gen = eng.poll_slots()
    return [eng.slot_tokens(b, int(min(gen[b], n_tokens))) for b in range(len(pages))]


def eos_of(eng):
    return set(int(e) for e in eng.cfg.eos_token_ids)


# ----------------------------------------------------------------------------- the engine, scripted drafts
@pytest.mark.parametrize("B,K", LAYOUTS)
@pytest.mark.parametrize("name,dtype", MODELS)
def test_full_acceptance_gives_the_plain_tokens_in_fewer_steps(name, dtype, B, K):
    """Scripts equal to the plain run's continuation: every draft is accepted, every live slot advances K + 1 tokens per step, and
    the tokens are the plain run's.  (Fails on a tree without the feature: Engine takes no `speculative`.)"""
    plain, spec = engine_pair(name, dtype, B, K)
    cfg = plain.cfg
    pages = pages_for(cfg, B)
    S = 6
    N = 1 + S * (K + 1)
    truth = plain_run(plain, pages, N)
    spec.begin_slots(N + 8)
    assert spec.rows == max(17, B * (K + 1)) and spec.seq_room() == plain.seq_room() - K
    spec.admit(pages, list(range(B)))
    for b in range(B):
        spec.set_draft_script(b, truth[b])
    for s in range(1, S + 1):
        spec.decode_steps(1, speculative=True)
        _, gen = spec.poll_slots()
        for b in range(B):
            assert gen[b] == min(len(truth[b]), 1 + s * (K + 1)), f"slot {b} after {s} steps"
    for b in range(B):
        np.testing.assert_array_equal(spec.slot_tokens(b, len(truth[b])), truth[b], err_msg=f"slot {b}")
    prop, acc = spec.spec_counters()
    np.testing.assert_array_equal(acc, prop)
    sim = [R.simulate([int(t) for t in tr], [int(t) for t in tr], K, S, eos=eos_of(plain)) for tr in truth]
    np.testing.assert_array_equal(acc, [a for _, _, a in sim])
    assert all(a > 0 for a in acc)
    assert spec.spec_steps == S == math.ceil((N - 1) / (K + 1)) and spec.plain_steps == 0
    for b in range(B):
        spec.set_draft_script(b, None)


@pytest.mark.parametrize("B,K", LAYOUTS)
@pytest.mark.parametrize("name,dtype", MODELS)
def test_partial_acceptance_gives_the_plain_tokens_and_the_scripted_counts(name, dtype, B, K):
    """Scripts wrong at chosen positions — draft 1, 2 and 3 of a step, at several steps, in different slots: the tokens are still the
    plain run's and generated / proposed / accepted per slot are what the script implies."""
    plain, spec = engine_pair(name, dtype, B, K)
    cfg = plain.cfg
    pages = pages_for(cfg, B)
    S = 7
    N = 2 + S * (K + 1)
    truth = plain_run(plain, pages, N)
    eos = eos_of(plain)
    scripts, want, first_wrong = [], [], set()
    for b in range(B):
        sc = [int(t) for t in truth[b]]
        for i in (2 + b, 6 + 2 * b, 11 + b, 17, 18 + b):
            if i < len(sc):
                sc[i] = (sc[i] + 1 + b) % 400
        trace = []
        want.append(R.simulate(sc, [int(t) for t in truth[b]], K, S, eos=eos, trace=trace))
        first_wrong |= {e - 1 for nd, e in trace if e <= nd}        # index of the draft that stopped a run
        scripts.append(sc)
    assert first_wrong >= set(range(K)), f"the scripts must go wrong at every draft index, got {sorted(first_wrong)}"
    spec.begin_slots(N + 8)
    spec.admit(pages, list(range(B)))
    for b in range(B):
        spec.set_draft_script(b, scripts[b])
    spec.decode_steps(S, speculative=True)
    _, gen = spec.poll_slots()
    prop, acc = spec.spec_counters()
    for b in range(B):
        assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b}: generated / proposed / accepted"
        np.testing.assert_array_equal(spec.slot_tokens(b, int(gen[b])), truth[b][:int(gen[b])], err_msg=f"slot {b}")
    assert int(acc.sum()) < int(prop.sum())
    for b in range(B):
        spec.set_draft_script(b, None)


def repeated_pages(cfg, B, **kw):
    """Prompts whose text repeats a short span, so that an n-gram of the sequence's end has an earlier occurrence."""
    out = []
    for b in range(B):
        p = page_of(cfg, LENGTHS[b % 3], variant=b, **kw)
        ids = p.input_ids.copy()
        tail = np.flatnonzero(ids == cfg.vision_end_token_id)[0] + 1
        span = np.asarray([7 + b, 9, 11 + b, 13])
        ids[tail:] = np.resize(span, len(ids) - tail)
        ids[:4] = span
        out.append(dataclasses.replace(p, input_ids=ids))
    return out


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B,K", LAYOUTS)
@pytest.mark.parametrize("name,dtype", MODELS[:2])
def test_prompt_lookup_gives_the_plain_tokens(name, dtype, B, K, sampled):
    """The real lookup (1..3-grams) on prompts with repeated spans: drafts are proposed, and the tokens are the plain run's — greedy, and
    sampled at a temperature at which the noise decides (the noise of a draft row is the noise of its own token index)."""
    plain, spec = engine_pair(name, dtype, B, K, 1, 3)
    cfg = plain.cfg
    pages = repeated_pages(cfg, B)
    if sampled:
        T = hot(plain, pages[0])
        pages = [dataclasses.replace(p, temperature=T, seed=(0xFFFFFFFE + b) & 0xFFFFFFFF) for b, p in enumerate(pages)]
    N, S = 33, 14
    truth = plain_run(plain, pages, N, sampling=sampled)
    spec.begin_slots(2 + S * (K + 1), sampling=sampled)          # every step may emit K + 1 tokens
    spec.admit(pages, list(range(B)))
    spec.decode_steps(S, speculative=True)
    _, gen = spec.poll_slots()
    prop, acc = spec.spec_counters()
    assert int(prop.sum()) > 0, "the lookup proposed nothing: the test needs prompts it finds matches in"
    for b in range(B):
        n = int(min(gen[b], len(truth[b])))
        assert n >= min(len(truth[b]), 1 + S)
        np.testing.assert_array_equal(spec.slot_tokens(b, n), truth[b][:n], err_msg=f"slot {b} ({prop[b]} proposed, {acc[b]} accepted)")
    if sampled:
        greedy = plain_run(plain, [dataclasses.replace(p, temperature=0.0) for p in pages], N)
        assert any(len(g) != len(t) or (g != t).any() for g, t in zip(greedy, truth)), "the temperature must change the tokens"


def test_engine_refusals():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg = CONFIGS["tiny-w512"]
    kw = dict(s_max=256, max_patches=256, max_prompt_tokens=256)
    with pytest.raises(KarantaHipError, match="rows > 32"):
        Engine(cfg, max_batch=9, speculative=SpecConfig(3), **kw)
    with pytest.raises(KarantaHipError, match="ngram_min"):
        Engine(cfg, max_batch=2, speculative=SpecConfig(3, 3, 2), **kw)
    with pytest.raises(KarantaHipError, match="max_batch > 16"):
        Engine(CONFIGS["tiny"], max_batch=2, speculative=SpecConfig(3), **kw)          # hidden 256: no wide kernel
    plain, spec = engine_pair("tiny-w512", "bf16", 4, 1)
    plain.begin_slots(8)
    with pytest.raises(KarantaHipError, match="without speculative"):
        plain.decode_steps(1, speculative=True)
    spec.begin_slots(8, sampling=True, logprobs=2)
    with pytest.raises(KarantaHipError, match="log-probabilities"):
        spec.decode_steps(1, speculative=True)
    spec.begin_slots(8, sampling=True)
    spec.set_step_features(True, False, processing=True)
    with pytest.raises(KarantaHipError, match="sampling controls"):
        spec.decode_steps(1, speculative=True)
    assert not spec.can_speculate()
    spec.set_step_features(True, False)
    assert spec.can_speculate()


# ----------------------------------------------------------------------------- through the scheduler
def set_eos(eng, ids):
    """Two EOS ids of the test's choice on an engine (device list and host config alike)."""
    ids = tuple(int(i) for i in ids)
    assert len(ids) == eng.d_eos.numel()
    eng.cfg = dataclasses.replace(eng.cfg, eos_token_ids=ids)
    eng.d_eos.copy_(torch.tensor(ids, dtype=torch.int32))
    torch.cuda.synchronize()


ALWAYS = SpecPolicy(break_even=0.0)


def solo(plain, page, max_tokens):
    r = plain.generate([page], max_tokens)
    return r.tokens[0], r.finish_reasons[0]


@pytest.mark.parametrize("overlap,launch_ahead", [(False, False), (False, True), (True, False)])
def test_scheduler_speculative_equals_solo_runs(overlap, launch_ahead):
    """14 requests over 5 slots (every slot is reused: the newcomer finds the draft K/V of its predecessor behind its prompt), token
    limits that fall inside accepted runs, EOS ids that end sequences early, late and never, full and wrong scripts and the real
    lookup side by side."""
    B, K = 5, 3
    plain, spec = engine_pair("tiny-w512", "bf16", B, K)
    cfg0 = CONFIGS["tiny-w512"]
    pages = [page_of(cfg0, LENGTHS[i % 3], variant=20 + i) for i in range(14)]
    limits = [5 + (7 * i) % 23 for i in range(14)]
    for e in (plain, spec):
        set_eos(e, cfg0.eos_token_ids)
    free = [np.asarray(solo(plain, p, 30)[0]) for p in pages[:6]]
    early, late = int(free[0][3]), int(free[1][min(len(free[1]) - 1, 20)])
    try:
        for e in (plain, spec):
            set_eos(e, (early, late))
        want = [solo(plain, p, n) for p, n in zip(pages, limits)]
        assert any(r == "stop" and len(t) <= 5 for t, r in want) and any(r == "length" for t, r in want)
        sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, speculative=True, spec_policy=ALWAYS, overlap=overlap,
                            launch_ahead=launch_ahead)
        # slots 0 and 1 draft from the plain continuation of whatever request sits there first (right for one request, wrong for
        # the later ones: rejected drafts), slot 2 from garbage, slots 3 and 4 from the lookup
        spec.set_draft_script(0, want[0][0])
        spec.set_draft_script(1, want[1][0])
        spec.set_draft_script(2, [3] * 64)
        res = sch.run([SlotRequest(p, n, tag=i) for i, (p, n) in enumerate(zip(pages, limits))])
        for i, (r, (toks, reason)) in enumerate(zip(res, want)):
            assert r.error is None, r.error
            np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
            assert r.finish_reason == reason, f"request {i}"
        assert sch.spec_steps > 0 and sch.plain_steps == 0 and sch.spec_draft_tokens > sch.spec_accepted_tokens > 0
        prop, acc = spec.spec_counters()
        assert sch.spec_draft_tokens <= int(prop.sum()) and sch.spec_accepted_tokens <= int(acc.sum())   # (the last chunk may be unread)
    finally:
        for j in range(3):
            spec.set_draft_script(j, None)
        for e in (plain, spec):
            set_eos(e, cfg0.eos_token_ids)


def test_scheduler_mixes_plain_and_speculative_chunks():
    """A policy that alternates the two kinds of chunk, a request with a penalty and a guided request in the batch (their chunks are
    plain), sampled requests, and prompt reuse (admit_reuse writes the prompt ids of the forked slot): every result is its solo run."""
    from karanta_ocr_amd.serving import ByteTokenizer
    B, K = 5, 3
    plain, spec = engine_pair("tiny-w512", "bf16", B, K)
    cfg = plain.cfg
    for e in (plain, spec):
        e.set_vocab(ByteTokenizer(cfg).token_bytes())
    base = [page_of(cfg, LENGTHS[i % 3], variant=40 + i) for i in range(8)]
    T = hot(plain, base[0])
    pages = [dataclasses.replace(p, temperature=T if i % 2 else 0.0, seed=11 + i) for i, p in enumerate(base)]
    pages[2] = dataclasses.replace(pages[2], repetition_penalty=1.3, frequency_penalty=0.5)
    pages[5] = dataclasses.replace(pages[5], guide=PATTERN, temperature=T)
    # the prompts of the first two requests again, right behind the five that fill the slots: whichever slot frees first, slots 0
    # and 1 still hold those prompts (in place when it is their own slot, else forked from it)
    keys = [b"page %d" % i for i in range(8)]
    pages, keys = pages[:5] + [pages[0], pages[1]] + pages[5:], keys[:5] + [keys[0], keys[1]] + keys[5:]
    limits = [9 + (5 * i) % 11 for i in range(len(pages))]
    want = [solo(plain, p, n) for p, n in zip(pages, limits)]

    class Alternate(SpecPolicy):
        def __init__(self):
            super().__init__(0.0)
            self.n = 0

        def want(self):
            self.n += 1
            return self.n % 3 != 0

    sch = SlotScheduler(spec, max_tokens_cap=24, chunk=2, sampling=True, guided=True, speculative=True, spec_policy=Alternate(),
                        prefix_cache=True)
    res = sch.run([SlotRequest(p, n, tag=i, prompt_key=k) for i, (p, n, k) in enumerate(zip(pages, limits, keys))])
    for i, (r, (toks, reason)) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
        assert r.finish_reason == reason, f"request {i}"
    assert sch.spec_steps > 0 and sch.plain_steps > 0 and sch.prefix_cache_hits >= 1
    assert spec.spec_steps == sch.spec_steps and spec.plain_steps == sch.plain_steps
    # a request with a penalty alone: the policy always wants speculation, its chunks are plain all the same
    sch = SlotScheduler(spec, max_tokens_cap=24, chunk=2, sampling=True, guided=True, speculative=True, spec_policy=ALWAYS)
    r = sch.run([SlotRequest(pages[2], limits[2], tag=0)])[0]
    np.testing.assert_array_equal(r.tokens, want[2][0])
    assert sch.spec_steps == 0 and sch.plain_steps > 0
