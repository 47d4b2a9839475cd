"""Guided requests in speculative decode steps (SpecConfig(guided=True)) on the engine and through the slot scheduler: every request
returns exactly the tokens, the finish reason and the DFA state it has without speculation — guided and unguided, greedy and sampled
slots side by side, whatever is drafted.  The baseline is the same engine class built without `speculative`; scripted drafts
(Engine.set_draft_script) make the acceptance pattern, and the tokens the guide has to trim, a choice of the test, and the counters
are compared with tests/spec_guide_ref.simulate.  Every comparison is an exact integer equality.  (Fails on a tree without the
feature: SpecConfig takes no `guided`.)"""
import dataclasses
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError  # noqa: E402
from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler  # noqa: E402
from karanta_ocr_amd.serving import ByteTokenizer  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests import spec_guide_ref as G  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402
from tests.test_gpu_spec_engine import ALWAYS, LENGTHS, PATTERN, solo  # noqa: E402

NAME = "tiny-w512"
CFG = CONFIGS[NAME]
FIXED = [r"[a-f]{3}-[0-9]{2}", r"[a-f]{3}-[0-9]{3};", r"[a-f]{4}-[0-9]{3}"]     # after the last byte only the EOS is allowed
REPEAT = r"(?:[ab]{2}-){8,40}"
KW = dict(s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
# (weights, slots, K, shared rows)
LAYOUTS = [("bf16", 5, 3, False), ("bf16", 3, 3, True), ("bf16", 20, 3, True), ("fp8", 5, 3, False)]
FORBIDDEN = ord("#")          # a byte no pattern of this module allows anywhere
_E, _W, _P = {}, {}, {}


def token_table():
    """The byte tokenizer's table with ids 256.. made multi-byte tokens (spec_guide_ref.MULTI)."""
    tb = ByteTokenizer(CFG).token_bytes()
    for i, s in enumerate(G.MULTI):
        assert tb[256 + i] == b""
        tb[256 + i] = s
    return tb


TOKENS = token_table()
EOS_IDS = tuple(int(e) for e in CFG.eos_token_ids)


def engines(dtype, B, K, shared, guided=True, n_min=2, n_max=4):
    """(plain engine, speculative engine) of one configuration, with the module's token table, kept for the module."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if NAME not in _W:
        _W[NAME] = random_weights(CFG, 909)
    keys = (("plain", dtype, B), ("spec", dtype, B, K, shared, guided, n_min, n_max))
    for key in keys:
        if key not in _E:
            sc = {} if key[0] == "plain" else {"speculative": SpecConfig(K, n_min, n_max, share_rows=shared, guided=guided)}
            e = _E[key] = Engine(CFG, max_batch=B, weight_dtype=dtype, **KW, **sc)
            e.load_weights(_W[NAME])
            e.set_vocab(TOKENS)
    return _E[keys[0]], _E[keys[1]]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _E.values():
        e.close()
    _E.clear()


def pattern(text):
    if text not in _P:
        _P[text] = G.Pattern(text, TOKENS, EOS_IDS)
    return _P[text]


def mixed_pages(plain, B, T=None):
    """Guided and unguided, greedy and sampled requests in turn: unguided greedy, a pattern whose end forces the EOS (sampled), the
    optional-tail pattern (greedy), the long repetitive one (sampled), unguided sampled, a forced end again (greedy)."""
    T = hot(plain, page_of(CFG, LENGTHS[0])) if T is None else T
    kinds = [(None, 0.0), (FIXED[0], T), (PATTERN, 0.0), (REPEAT, T), (None, T), (FIXED[1], 0.0), (FIXED[2], T), (REPEAT, 0.0)]
    out = []
    for b in range(B):
        guide, temp = kinds[b % len(kinds)]
        out.append(page_of(CFG, LENGTHS[b % 3], variant=b, guide=guide, temperature=temp, seed=(0xFFFFFFF0 + 3 * b) & 0xFFFFFFFF))
    return out


def plain_run(eng, pages, n_tokens):
    """Slot mode, plain guided steps: per slot the first n_tokens generated tokens (fewer where an EOS ended the sequence)."""
    eng.begin_slots(n_tokens + 8, sampling=True, guided=True)
    eng.admit(pages, list(range(len(pages))))
    eng.decode_steps(n_tokens - 1)
    _, gen = eng.poll_slots()
    return [eng.slot_tokens(b, int(min(gen[b], n_tokens))) for b in range(len(pages))]


def check_states(eng, pages, tokens):
    """The DFA state of every guided slot is the pattern's walk over the bytes of its tokens (a finishing EOS excluded)."""
    eng.stream.synchronize()
    got = eng.sampler.d_gstate[:len(pages)].cpu().numpy()
    for b, (p, toks) in enumerate(zip(pages, tokens)):
        if p.guide is None:
            continue
        g = pattern(p.guide).guide
        st = g.start
        for t in toks:
            if int(t) not in EOS_IDS:
                st = g.walk(st, TOKENS[int(t)])
        assert st != 0 and int(got[b]) == st, f"slot {b}: DFA state {got[b]}, the walk over its tokens gives {st}"


def pats_of(pages):
    return [None if p.guide is None else pattern(p.guide) for p in pages]


def clear_scripts(eng, B):
    for b in range(B):
        eng.set_draft_script(b, None)


# ----------------------------------------------------------------------------- scripted drafts
@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS)
def test_full_acceptance_gives_the_plain_guided_tokens_in_fewer_steps(dtype, B, K, shared):
    """Scripts equal to the plain guided run's continuation: every draft is allowed and accepted; the tokens are the plain run's, a
    pattern that completes inside a step is followed by its forced EOS and by nothing else."""
    plain, spec = engines(dtype, B, K, shared)
    pages = mixed_pages(plain, B)
    S = 6
    N = 1 + S * (K + 1)
    truth = plain_run(plain, pages, N)
    check_states(plain, pages, truth)
    for b, p in enumerate(pages):        # the forced end: the pattern is complete, the EOS follows, the sequence is over
        if p.guide in FIXED:
            assert int(truth[b][-1]) in EOS_IDS and pattern(p.guide).guide.fullmatch(b"".join(TOKENS[int(t)] for t in truth[b][:-1]))
    ends = [len(truth[b]) - 1 for b, p in enumerate(pages) if p.guide in FIXED]
    assert any(i % (K + 1) != 0 for i in ends), f"no pattern completes inside a step: EOS at token indices {ends}"
    scripts = [[int(t) for t in tr] for tr in truth]
    trace = []
    want = G.simulate(scripts, truth, pats_of(pages), TOKENS, K, S, eos=EOS_IDS, rows=spec.rows if shared else None, trace=trace)
    assert all(w == c for w, c, _ in trace), "a right draft is never trimmed"
    spec.begin_slots(N + 8, sampling=True, guided=True)
    assert spec.spec_guided and spec.can_speculate()
    spec.admit(pages, list(range(B)))
    try:
        for b in range(B):
            spec.set_draft_script(b, scripts[b])
        for s in range(1, S + 1):
            spec.decode_steps(1, speculative=True)
            if B * (K + 1) <= spec.rows:             # every draft has a row: K + 1 tokens per live slot and step
                _, gen = spec.poll_slots()
                for b in range(B):
                    assert gen[b] == min(len(truth[b]), 1 + s * (K + 1)), f"slot {b} after {s} steps"
        _, gen = spec.poll_slots()
        prop, acc = spec.spec_counters()
        got = [spec.slot_tokens(b, int(gen[b])) for b in range(B)]
        for b in range(B):
            assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b}: generated / proposed / accepted"
            np.testing.assert_array_equal(got[b], truth[b][:int(gen[b])], err_msg=f"slot {b}")
        check_states(spec, pages, got)
        np.testing.assert_array_equal(acc, prop)
        assert any(acc[b] > 0 for b, p in enumerate(pages) if p.guide is not None)
        if B * (K + 1) <= spec.rows:
            assert all(acc[b] > 0 for b, p in enumerate(pages) if p.guide is not None)
        assert spec.spec_steps == S == math.ceil((N - 1) / (K + 1)) and spec.plain_steps == 0
    finally:
        clear_scripts(spec, B)


def wrong_scripts(pages, truth, K):
    """The plain continuation gone wrong at chosen generated-token indices — draft 1, 2 and 3 of a step, in turn a token the slot's
    guide forbids there and one it allows (where it allows another than the right one)."""
    scripts, n_forbidden, n_allowed = [], 0, 0
    for b, (p, tr) in enumerate(zip(pages, truth)):
        sc = [int(t) for t in tr]
        pat = None if p.guide is None else pattern(p.guide)
        for n, i in enumerate((1 + b % 3, 6 + b % 2, 11 + b % 3, 17, 18 + b % 4)):
            if i >= len(sc):
                continue
            other = None
            if pat is not None and (n + b) % 2 == 1:
                st = pat.start
                for t in sc[:i]:
                    st = pat.guide.walk(st, TOKENS[t])
                ok = [int(t) for t in np.flatnonzero(pat.mask[st]) if int(t) != int(tr[i])]
                other = ok[(b + i) % len(ok)] if ok else None
            if other is None:
                sc[i] = FORBIDDEN if int(tr[i]) != FORBIDDEN else FORBIDDEN + 1
                n_forbidden += pat is not None
            else:
                sc[i] = other
                n_allowed += 1
        scripts.append(sc)
    assert n_forbidden > 0 and n_allowed > 0
    return scripts


@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS)
def test_partial_acceptance_gives_the_plain_tokens_and_the_trimmed_counts(dtype, B, K, shared):
    plain, spec = engines(dtype, B, K, shared)
    pages = mixed_pages(plain, B)
    S = 7
    N = 2 + S * (K + 1)
    truth = plain_run(plain, pages, N)
    scripts = wrong_scripts(pages, truth, K)
    trace, loose = [], []
    want = G.simulate(scripts, truth, pats_of(pages), TOKENS, K, S, eos=EOS_IDS, rows=spec.rows if shared else None, trace=trace)
    untrimmed = G.simulate(scripts, truth, [None] * B, TOKENS, K, S, eos=EOS_IDS, rows=spec.rows if shared else None, trace=loose)
    assert sum(sum(w) - sum(c) for w, c, _ in trace) > 0, "the scripts must hold drafts the guides forbid"
    fits = B * (K + 1) <= spec.rows          # (where the budget binds, a row the trim frees is another slot's draft)
    assert want != untrimmed, "the counts must tell the trim from a rejection"
    if fits:
        assert [w[0] for w in want] == [u[0] for u in untrimmed], "trimmed or rejected, a forbidden draft emits nothing"
    spec.begin_slots(N + 8, sampling=True, guided=True)
    spec.admit(pages, list(range(B)))
    try:
        for b in range(B):
            spec.set_draft_script(b, scripts[b])
        spec.decode_steps(S, speculative=True)
        _, gen = spec.poll_slots()
        prop, acc = spec.spec_counters()
        got = [spec.slot_tokens(b, int(gen[b])) for b in range(B)]
        for b in range(B):
            np.testing.assert_array_equal(got[b], truth[b][:int(gen[b])], err_msg=f"slot {b}")
            assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b}: generated / proposed / accepted"
        check_states(spec, pages, got)
        if fits:
            assert int(prop.sum()) < sum(u[1] for u in untrimmed), "the trim must show in the proposed drafts"
        assert 0 < int(acc.sum()) < int(prop.sum())
    finally:
        clear_scripts(spec, B)


# ----------------------------------------------------------------------------- the real lookup
def repetitive_pages(plain, B, T):
    """Guided by the repetitive pattern, with prompts whose text already holds its tokens — and two unguided slots beside them."""
    a, b_, dash = ord("a"), ord("b"), ord("-")
    out = []
    for b in range(B):
        p = page_of(CFG, LENGTHS[b % 3], variant=b, guide=None if b % 5 == 4 else REPEAT, temperature=T if b % 2 else 0.0, seed=31 + b)
        ids = p.input_ids.copy()
        tail = np.flatnonzero(ids == CFG.vision_end_token_id)[0] + 1
        span = np.asarray([a, b_, dash, b_, a, dash, a, a, dash, b_, b_, dash][b % 4:] + [a, b_, dash])
        ids[tail:] = np.resize(span, len(ids) - tail)
        out.append(dataclasses.replace(p, input_ids=ids))
    return out


@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS[:3])
def test_prompt_lookup_on_guided_slots_gives_the_solo_tokens(dtype, B, K, shared):
    """No script: n-gram drafts from the prompt and the output so far, on a pattern whose output repeats.  Drafts are proposed and
    accepted, and every slot — guided or not, greedy or sampled — returns its solo plain run."""
    plain, spec = engines(dtype, B, K, shared, n_min=1, n_max=3)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    pages = repetitive_pages(plain, B, T)
    S, N = 12, 30
    want = [solo(plain, p, N) for p in pages]
    spec.begin_slots(2 + S * (K + 1), sampling=True, guided=True)
    spec.admit(pages, list(range(B)))
    spec.decode_steps(S, speculative=True)
    _, gen = spec.poll_slots()
    prop, acc = spec.spec_counters()
    guided = [b for b, p in enumerate(pages) if p.guide is not None]
    assert int(prop[guided].sum()) > 0 and int(acc[guided].sum()) > 0, f"proposed {prop.tolist()}, accepted {acc.tolist()}"
    got = []
    for b in range(B):
        n = int(min(gen[b], len(want[b][0])))
        assert n >= min(len(want[b][0]), 1 + S)
        got.append(spec.slot_tokens(b, n))
        np.testing.assert_array_equal(got[b], want[b][0][:n], err_msg=f"slot {b} ({prop[b]} proposed, {acc[b]} accepted)")
    check_states(spec, pages, [spec.slot_tokens(b, int(gen[b])) for b in range(B)])


# ----------------------------------------------------------------------------- through the scheduler
def traffic(plain):
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    kinds = [(FIXED[0], T), (None, 0.0), (PATTERN, 0.0), (REPEAT, T), (FIXED[2], 0.0), (None, T), (REPEAT, 0.0), (PATTERN, T),
             (FIXED[1], T), (None, 0.0), (REPEAT, T), (FIXED[0], 0.0), (PATTERN, T), (REPEAT, 0.0)]
    pages = [page_of(CFG, LENGTHS[i % 3], variant=20 + i, guide=g, temperature=t, seed=50 + i) for i, (g, t) in enumerate(kinds)]
    limits = [5 + (7 * i) % 23 for i in range(len(pages))]
    return pages, limits


@pytest.mark.parametrize("shared,B", [(False, 5), (True, 3)])
def test_scheduler_speculates_on_guided_requests_and_equals_solo_runs(shared, B):
    """14 requests over the slots, guided ones coming and going beside plain ones, right, wrong and forbidden scripts and the real
    lookup side by side: every chunk is speculative and every result is the request's solo run."""
    K = 3
    plain, spec = engines("bf16", B, K, shared)
    pages, limits = traffic(plain)
    want = [solo(plain, p, n) for p, n in zip(pages, limits)]
    assert any(r == "stop" for (_, r), p in zip(want, pages) if p.guide) and any(r == "length" for (_, r), p in zip(want, pages) if p.guide)
    sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, sampling=True, guided=True, speculative=True, spec_policy=ALWAYS)
    try:
        spec.set_draft_script(0, want[0][0])                 # right for the first request in the slot, wrong for its successors
        spec.set_draft_script(1, [FORBIDDEN] * 64)           # unguided: rejected; guided: trimmed
        res = sch.run([SlotRequest(p, n, tag=i) for i, (p, n) in enumerate(zip(pages, limits))])
    finally:
        clear_scripts(spec, 2)
    for i, (r, (toks, reason)) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
        assert r.finish_reason == reason, f"request {i}"
    assert sch.spec_steps > 0 and sch.plain_steps == 0 and sch.spec_draft_tokens >= sch.spec_accepted_tokens > 0
    assert spec.spec_steps == sch.spec_steps and spec.plain_steps == 0


def test_without_the_option_the_same_traffic_runs_plain_chunks():
    """SpecConfig(3): guided=False, the behaviour before the option existed — chunks are plain while a guided request is in a slot."""
    plain, spec = engines("bf16", 5, 3, False, guided=False)
    assert not spec.spec_guided
    pages, limits = traffic(plain)
    pages, limits = pages[:8], limits[:8]
    want = [solo(plain, p, n) for p, n in zip(pages, limits)]
    sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, sampling=True, guided=True, speculative=True, spec_policy=ALWAYS)
    res = sch.run([SlotRequest(p, n, tag=i) for i, (p, n) in enumerate(zip(pages, limits))])
    for i, (r, (toks, reason)) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
        assert r.finish_reason == reason, f"request {i}"
    assert sch.plain_steps > 0 and spec.plain_steps == sch.plain_steps
    # one guided request alone: never a speculative chunk
    sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, sampling=True, guided=True, speculative=True, spec_policy=ALWAYS)
    r = sch.run([SlotRequest(pages[3], limits[3], tag=0)])[0]
    np.testing.assert_array_equal(r.tokens, want[3][0])
    assert sch.spec_steps == 0 and sch.plain_steps > 0


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    _, spec = engines("bf16", 5, 3, False)
    spec.begin_slots(8, sampling=True, guided=True)
    spec.set_step_features(True, True)
    assert spec.can_speculate()
    spec.set_step_features(True, True, processing=True)
    with pytest.raises(KarantaHipError, match="sampling controls"):
        spec.decode_steps(1, speculative=True)
    spec.set_step_features(True, True, adjust=True)
    with pytest.raises(KarantaHipError, match="logit adjustments"):
        spec.decode_steps(1, speculative=True)
    assert not spec.can_speculate()
    spec.begin_slots(8, sampling=True, guided=True, logprobs=2)
    spec.set_step_features(True, True)
    with pytest.raises(KarantaHipError, match="log-probabilities"):
        spec.decode_steps(1, speculative=True)
    _, off = engines("bf16", 5, 3, False, guided=False)
    off.begin_slots(8, sampling=True, guided=True)
    off.set_step_features(True, True)
    with pytest.raises(KarantaHipError, match=r"SpecConfig\(guided=True\)"):
        off.decode_steps(1, speculative=True)
    assert not off.can_speculate()
    off.set_step_features(True, False)
    assert off.can_speculate()
