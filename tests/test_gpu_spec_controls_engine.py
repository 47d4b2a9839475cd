"""Requests with sampling controls and logit adjustments in speculative decode steps (SpecConfig(controls=True)) on the engine and
through the slot scheduler: every request returns exactly the tokens, the finish reason and the output counts it has without
speculation — top_k, top_p, min_p, the three penalties, logit_bias, min_tokens, stop_token_ids, all of them and none, greedy and
sampled slots side by side, whatever is drafted.  The baseline is the same engine class built without `speculative`; scripted drafts
(Engine.set_draft_script) make the acceptance pattern a choice of the test, and the counters are compared with
tests/spec_controls_ref.simulate.  Every comparison is an exact integer equality.  (Fails on a tree without the feature: SpecConfig
takes no `controls`.)"""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.sampling import needs_processing  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests import spec_controls_ref as X  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402
from tests.test_gpu_spec_engine import ALWAYS, LENGTHS, solo  # noqa: E402
from tests.test_gpu_spec_guided_engine import (CFG, EOS_IDS, FIXED, KW, LAYOUTS, NAME, REPEAT, TOKENS, clear_scripts,  # noqa: E402
                                               pattern)

V = CFG.text.vocab_size
KINDS = ["top_k", "top_p", "min_p", "repetition", "freq_pres", "logit_bias", "min_tokens", "stop", "all", "greedy", "sampled"]
CONTROL_KINDS = KINDS[:9]
MIN_TOKENS = 6
# where the kinds start per layout, so that the two static layouts cover all of them between them and the 20 slots all at once
OFFSET = {("bf16", 5, 3, False): 0, ("bf16", 3, 3, True): 4, ("bf16", 20, 3, True): 0, ("fp8", 5, 3, False): 6}
_E, _W = {}, {}


def engines(dtype, B, K, shared, controls=True, guided=False, n_min=2, n_max=4, **more):
    """(plain engine, speculative engine) of one configuration, kept for the module."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if NAME not in _W:
        _W[NAME] = random_weights(CFG, 909)
    extra = tuple(sorted(more.items()))
    keys = (("plain", dtype, B, extra), ("spec", dtype, B, K, shared, controls, guided, n_min, n_max, extra))
    for key in keys:
        if key not in _E:
            sc = {} if key[0] == "plain" else {"speculative": SpecConfig(K, n_min, n_max, share_rows=shared, guided=guided,
                                                                        controls=controls)}
            e = _E[key] = Engine(CFG, max_batch=B, weight_dtype=dtype, **KW, **more, **sc)
            e.load_weights(_W[NAME])
            e.set_vocab(TOKENS)
    return _E[keys[0]], _E[keys[1]]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _E.values():
        e.close()
    _E.clear()


def bare_pages(plain, B, off=0, T=None):
    """Per slot its kind and the page WITHOUT any control: temperature and seed alone (the penalty slots and the logit_bias slot are greedy, like
    the neutral greedy one: a greedy sequence of this model repeats itself, which is what the penalties act on)."""
    T = hot(plain, page_of(CFG, LENGTHS[0])) if T is None else T
    kinds = [KINDS[(b + off) % len(KINDS)] for b in range(B)]
    greedy = ("repetition", "freq_pres", "logit_bias", "greedy")
    return kinds, [page_of(CFG, LENGTHS[b % 3], variant=b, temperature=0.0 if k in greedy else T, seed=(0xFFFFFFF0 + 3 * b) & 0xFFFFFFFF)
                   for b, k in enumerate(kinds)]


def controlled(kinds, pages, bare_tokens):
    """The pages with their slot's control; what a control names comes from the slot's uncontrolled run, so that it bites."""
    eos = int(EOS_IDS[0])
    out = []
    for k, p, toks in zip(kinds, pages, bare_tokens):
        toks = [int(t) for t in toks]
        common = [int(t) for t in np.argsort(-np.bincount(toks, minlength=V))[:3]]
        late = next((t for i, t in enumerate(toks) if i >= 5 and t not in toks[:i] and t not in EOS_IDS), toks[-1])
        kw = {"top_k": dict(top_k=2), "top_p": dict(top_p=0.3), "min_p": dict(min_p=0.5), "repetition": dict(repetition_penalty=1.8),
              "freq_pres": dict(frequency_penalty=1.9, presence_penalty=1.0), "logit_bias": dict(logit_bias={t: -100.0 for t in common}),
              "min_tokens": dict(logit_bias={eos: 100.0}, min_tokens=MIN_TOKENS), "stop": dict(stop_token_ids=(late,)),
              "all": dict(top_k=8, top_p=0.9, min_p=0.02, repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.3,
                          logit_bias={common[0]: -100.0, common[1]: 1.5}, min_tokens=3, stop_token_ids=(late,)),
              "greedy": {}, "sampled": {}}[k]
        out.append(dataclasses.replace(p, **kw))
    return out


def stops_of(pages):
    """Per page the stop entries of its adjustment table: its stop_token_ids, and the EOS ids while it carries min_tokens."""
    return [set(int(t) for t in p.stop_token_ids) | (set(EOS_IDS) if p.min_tokens > 0 else set()) for p in pages]


def plain_run(eng, pages, n_tokens):
    """Slot mode, plain steps: per slot (the first n_tokens generated tokens — fewer where the sequence ended —, finished, the
    slot's output counts)."""
    B = len(pages)
    eng.begin_slots(n_tokens + 8, sampling=True)
    eng.admit(pages, list(range(B)))
    eng.decode_steps(n_tokens - 1)
    fin, gen = eng.poll_slots()
    counts = eng.sampler.d_counts[:B].cpu().numpy()
    return [eng.slot_tokens(b, int(min(gen[b], n_tokens))) for b in range(B)], [bool(f) for f in fin[:B]], counts


def check_counts(pages, tokens, counts, who):
    """The output counts of every slot that carries a sampling control are the histogram of its tokens."""
    for b, (p, toks) in enumerate(zip(pages, tokens)):
        if needs_processing(p):
            np.testing.assert_array_equal(counts[b], np.bincount(np.asarray(toks, np.int64), minlength=V), err_msg=f"{who}: slot {b}")


def truth_of(dtype, B, K, shared, N):
    """The plain engine's uncontrolled and controlled runs of one layout, and that every control kind bites."""
    plain, spec = engines(dtype, B, K, shared)
    kinds, bare = bare_pages(plain, B, OFFSET[(dtype, B, K, shared)])
    bare_tokens, _, _ = plain_run(plain, bare, N)
    pages = controlled(kinds, bare, bare_tokens)
    truth, fin, counts = plain_run(plain, pages, N)
    check_counts(pages, truth, counts, "plain run")
    for b, k in enumerate(kinds):             # decisive: no slot is skipped, every control changes its slot's tokens
        same = len(truth[b]) == len(bare_tokens[b]) and (np.asarray(truth[b]) == np.asarray(bare_tokens[b])).all()
        if k in CONTROL_KINDS:
            assert not same, f"slot {b} ({k}): the control does not change the plain engine's tokens"
        else:
            assert same, f"slot {b} ({k}): a neutral slot's tokens do not depend on its neighbours"
        if k == "min_tokens":      # the +100 EOS is held back for exactly min_tokens tokens
            assert len(truth[b]) == MIN_TOKENS + 1 and int(truth[b][-1]) in EOS_IDS and fin[b]
        if k == "stop":
            assert fin[b] and int(truth[b][-1]) in pages[b].stop_token_ids and len(truth[b]) < N
    return plain, spec, kinds, pages, truth, fin


def spec_run(spec, pages, scripts, steps, budget, features=None):
    B = len(pages)
    spec.begin_slots(budget, sampling=True, **(features or {}))
    spec.admit(pages, list(range(B)))
    assert spec.spec_controls and spec.can_speculate()
    try:
        for b in range(B):
            spec.set_draft_script(b, scripts[b])
        spec.decode_steps(steps, speculative=True)
        fin, gen = spec.poll_slots()
        prop, acc = spec.spec_counters()
        got = [spec.slot_tokens(b, int(gen[b])) for b in range(B)]
        counts = spec.sampler.d_counts[:B].cpu().numpy()
    finally:
        clear_scripts(spec, B)
    return got, [bool(f) for f in fin[:B]], gen, prop, acc, counts


def check_against(pages, truth, fin_truth, got, fin, gen, counts, N):
    for b in range(len(pages)):
        n = int(gen[b])
        np.testing.assert_array_equal(got[b], truth[b][:n], err_msg=f"slot {b}: tokens")
        ended = fin_truth[b] and n == len(truth[b])
        assert fin[b] == ended, f"slot {b}: finished after {n} of {len(truth[b])} tokens"
    check_counts(pages, got, counts, "speculative run")


# ----------------------------------------------------------------------------- scripted drafts
@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS)
def test_full_acceptance_gives_the_plain_controlled_tokens_in_fewer_steps(dtype, B, K, shared):
    S = 6
    N = 1 + S * (K + 1)
    plain, spec, kinds, pages, truth, fin_truth = truth_of(dtype, B, K, shared, N)
    scripts = [[int(t) for t in tr] for tr in truth]
    depths = [[] for _ in range(B)]
    want = X.simulate(scripts, truth, stops_of(pages), K, S, eos=EOS_IDS, rows=spec.rows if shared else None, depths=depths)
    got, fin, gen, prop, acc, counts = spec_run(spec, pages, scripts, S, N + 8)
    check_against(pages, truth, fin_truth, got, fin, gen, counts, N)
    for b in range(B):
        assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b} ({kinds[b]}): generated / proposed / accepted"
    if B * (K + 1) <= spec.rows:          # every draft has a row: the plain run's tokens, all of them, and its counts
        plain_counts = plain_run(plain, pages, N)[2]
        for b, p in enumerate(pages):
            assert int(gen[b]) == len(truth[b])
            if needs_processing(p):
                np.testing.assert_array_equal(counts[b], plain_counts[b], err_msg=f"slot {b}: the plain run's counts")
    if B * (K + 1) <= spec.rows:
        for b, k in enumerate(kinds):
            if k == "freq_pres":      # per-draft counts are exercised: rows at depth >= 2 were spent on this slot and accepted
                assert max(depths[b] or [0]) >= 2, f"slot {b}: accepted per step {depths[b]}"
        assert any(max(depths[b] or [0]) >= 2 for b, k in enumerate(kinds) if k in ("freq_pres", "repetition", "all"))
    assert int(acc.sum()) > 0 and spec.spec_steps == S and spec.plain_steps == 0


def wrong_scripts(truth, stops):
    """The plain continuation gone wrong at chosen generated-token indices — draft 1, 2 and 3 of a step in turn —, never with a
    stop entry (a stop entry is trimmed, not rejected: test_a_drafted_stop_id_is_trimmed)."""
    scripts = []
    for b, tr in enumerate(truth):
        sc = [int(t) for t in tr]
        for i in (1 + b % 3, 6 + b % 2, 11 + b % 3, 17, 18 + b % 4):
            if i < len(sc):
                sc[i] = next(t for t in range(sc[i] + 1, sc[i] + 9) if t % 256 not in stops[b] and t % 256 != sc[i]) % 256
        scripts.append(sc)
    return scripts


@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS)
def test_partial_acceptance_gives_the_plain_tokens_and_the_simulated_counts(dtype, B, K, shared):
    S = 7
    N = 2 + S * (K + 1)
    plain, spec, kinds, pages, truth, fin_truth = truth_of(dtype, B, K, shared, N)
    scripts = wrong_scripts(truth, stops_of(pages))
    want = X.simulate(scripts, truth, stops_of(pages), K, S, eos=EOS_IDS, rows=spec.rows if shared else None)
    got, fin, gen, prop, acc, counts = spec_run(spec, pages, scripts, S, N + 8)
    check_against(pages, truth, fin_truth, got, fin, gen, counts, N)
    for b in range(B):
        assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b} ({kinds[b]}): generated / proposed / accepted"
    assert 0 < int(acc.sum()) < int(prop.sum())


@pytest.mark.parametrize("dtype,B,K,shared", [LAYOUTS[2], LAYOUTS[3]])
def test_a_drafted_stop_id_is_trimmed(dtype, B, K, shared):
    """The scripts hold a stop entry of their slot where the model goes on: the draft is cut (it shows in `proposed`, and with
    shared rows another slot gets the row), the tokens are the plain run's, and the slot does not finish on a token it never chose."""
    S = 6
    N = 1 + S * (K + 1)
    plain, spec, kinds, pages, truth, fin_truth = truth_of(dtype, B, K, shared, N)
    stops = stops_of(pages)
    scripts = [[int(t) for t in tr] for tr in truth]
    n_stop = 0
    for b, sc in enumerate(scripts):
        for i in (2, 3 + b % 3, 9):
            if stops[b] and i < len(sc) - 1:
                sc[i] = sorted(stops[b])[0]
                n_stop += 1
    assert n_stop > 0
    trace = []
    want = X.simulate(scripts, truth, stops, K, S, eos=EOS_IDS, rows=spec.rows if shared else None, trace=trace)
    loose = X.simulate(scripts, truth, stops, K, S, eos=EOS_IDS, rows=spec.rows if shared else None, trim=False)
    assert sum(sum(w) - sum(c) for w, c, _ in trace) > 0 and want != loose, "the counts must tell the trim from a rejection"
    got, fin, gen, prop, acc, counts = spec_run(spec, pages, scripts, S, N + 8)
    check_against(pages, truth, fin_truth, got, fin, gen, counts, N)
    for b in range(B):
        assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b} ({kinds[b]}): generated / proposed / accepted"


# ----------------------------------------------------------------------------- the real lookup
@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS[:2])
def test_prompt_lookup_under_controls_gives_the_solo_tokens(dtype, B, K, shared):
    """No script: n-gram drafts from the prompt and the output so far.  The prompts end on a repetitive span of three tokens and a
    logit_bias keeps the output to those three, so the lookup finds drafts and some are right; penalties and truncation on top."""
    plain, spec = engines(dtype, B, K, shared, n_min=1, n_max=3)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    a, b_, dash = ord("a"), ord("b"), ord("-")
    bias = {a: 30.0, b_: 30.0, dash: 30.0}
    extra = [dict(), dict(frequency_penalty=0.2), dict(top_p=0.9, temperature=T), dict(repetition_penalty=1.05), dict(top_k=2, temperature=T)]
    pages = []
    for b in range(B):
        p = page_of(CFG, LENGTHS[b % 3], variant=b, seed=31 + b, logit_bias=bias, **extra[b % len(extra)])
        ids = p.input_ids.copy()
        tail = np.flatnonzero(ids == CFG.vision_end_token_id)[0] + 1
        ids[tail:] = np.resize(np.asarray([a, b_, dash, b_, a, dash, a, a, dash, b_, b_, dash][b % 4:] + [a, b_, dash]), len(ids) - tail)
        pages.append(dataclasses.replace(p, input_ids=ids))
    S, N = 12, 30
    want = [solo(plain, p, N) for p in pages]
    spec.begin_slots(2 + S * (K + 1), sampling=True)
    spec.admit(pages, list(range(B)))
    spec.decode_steps(S, speculative=True)
    _, gen = spec.poll_slots()
    prop, acc = spec.spec_counters()
    assert int(prop.sum()) > 0 and int(acc.sum()) > 0, f"proposed {prop.tolist()}, accepted {acc.tolist()}"
    for b in range(B):
        n = int(min(gen[b], len(want[b][0])))
        assert n >= min(len(want[b][0]), 1 + S)
        np.testing.assert_array_equal(spec.slot_tokens(b, n), want[b][0][:n], err_msg=f"slot {b} ({prop[b]} proposed, {acc[b]} accepted)")


# ----------------------------------------------------------------------------- guided and controlled
def check_states(eng, pages, tokens, fin):
    """The DFA state of every guided slot is the pattern's walk over the bytes of its tokens, the token that finished the slot — an
    EOS or a stop id — excluded (kr_guide_advance skips the rows the step has finished)."""
    eng.stream.synchronize()
    got = eng.sampler.d_gstate[:len(pages)].cpu().numpy()
    for b, (p, toks) in enumerate(zip(pages, tokens)):
        if p.guide is None:
            continue
        g = pattern(p.guide).guide
        st = g.start
        for t in (toks[:-1] if fin[b] else toks):
            st = g.walk(st, TOKENS[int(t)])
        assert st != 0 and int(got[b]) == st, f"slot {b}: DFA state {got[b]}, the walk over its tokens gives {st}"


def test_guided_and_controlled_requests_speculate_together():
    """SpecConfig(guided=True, controls=True): guided slots with truncation, penalties, a bias and a stop id beside unguided ones;
    both trims run, the draft rows are masked AND penalised, and tokens, DFA states and counts are the plain run's."""
    dtype, B, K, shared = LAYOUTS[0]
    plain, spec = engines(dtype, B, K, shared, guided=True)
    assert spec.spec_guided and spec.spec_controls
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    kinds = [(REPEAT, T, dict(top_p=0.5)), (REPEAT, 0.0, dict(frequency_penalty=1.5, presence_penalty=0.5)), (None, T, dict(top_k=3)),
             (FIXED[1], T, dict(repetition_penalty=1.4, logit_bias={ord("a"): -100.0})), (REPEAT, T, dict(stop_token_ids=(ord("b"),), min_p=0.1))]
    pages = [page_of(CFG, LENGTHS[b % 3], variant=b, guide=g, temperature=t, seed=77 + b, **kw) for b, (g, t, kw) in enumerate(kinds)]
    S = 5
    N = 1 + S * (K + 1)

    def run(eng, steps, speculative):
        eng.begin_slots(N + 8, sampling=True, guided=True)
        eng.admit(pages, list(range(B)))
        return eng

    run(plain, N - 1, False).decode_steps(N - 1)
    fin_t, gen_t = plain.poll_slots()
    truth = [plain.slot_tokens(b, int(min(gen_t[b], N))) for b in range(B)]
    check_states(plain, pages, truth, fin_t)
    assert any(fin_t[b] and int(truth[b][-1]) in pages[b].stop_token_ids for b in range(B)), "a guided slot ends on its stop id"
    counts_t = plain.sampler.d_counts[:B].cpu().numpy()
    run(spec, S, True)
    try:
        for b in range(B):
            sc = [int(t) for t in truth[b]]
            for i in (3 + b, 10):              # wrong here and there: "#" is forbidden by every guide, and rejected elsewhere
                if i < len(sc):
                    sc[i] = ord("#")
            spec.set_draft_script(b, sc)
        assert spec.can_speculate()
        spec.decode_steps(S, speculative=True)
        fin, gen = spec.poll_slots()
        prop, acc = spec.spec_counters()
        got = [spec.slot_tokens(b, int(gen[b])) for b in range(B)]
        for b in range(B):
            np.testing.assert_array_equal(got[b], truth[b][:int(gen[b])], err_msg=f"slot {b}")
            assert bool(fin[b]) == (bool(fin_t[b]) and int(gen[b]) == len(truth[b])), f"slot {b}: finished"
        check_states(spec, pages, got, fin)
        check_counts(pages, got, spec.sampler.d_counts[:B].cpu().numpy(), "speculative run")
        check_counts(pages, truth, counts_t, "plain run")
        assert 0 < int(acc.sum()) < int(prop.sum()) and spec.spec_steps == S
    finally:
        clear_scripts(spec, B)


def test_an_fp8_kv_cache_takes_controlled_speculative_steps():
    dtype, B, K, shared = LAYOUTS[0]
    plain, spec = engines(dtype, B, K, shared, kv_cache_dtype="fp8")
    S = 4
    N = 1 + S * (K + 1)
    kinds, bare = bare_pages(plain, B, 4)
    pages = controlled(kinds, bare, plain_run(plain, bare, N)[0])
    truth, fin_truth, _ = plain_run(plain, pages, N)
    scripts = wrong_scripts(truth, stops_of(pages))
    got, fin, gen, prop, acc, counts = spec_run(spec, pages, scripts, S, N + 8)
    check_against(pages, truth, fin_truth, got, fin, gen, counts, N)
    assert 0 < int(acc.sum()) < int(prop.sum())


# ----------------------------------------------------------------------------- through the scheduler
def traffic(plain):
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    eos = int(EOS_IDS[0])
    kws = [dict(top_p=0.4, temperature=T), dict(), dict(frequency_penalty=1.5), dict(top_k=3, temperature=T, repetition_penalty=1.3),
           dict(logit_bias={eos: 100.0}, min_tokens=4), dict(temperature=T), dict(min_p=0.3, temperature=T, presence_penalty=0.8),
           dict(logit_bias={ord("a"): 8.0, ord("b"): 8.0}, stop_token_ids=(ord("b"),), temperature=T), dict(),
           dict(top_k=5, top_p=0.8, temperature=T), dict(repetition_penalty=1.6), dict(logit_bias={eos: 100.0}, min_tokens=9, temperature=T),
           dict(frequency_penalty=-0.5, temperature=T), dict(stop_token_ids=tuple(range(0, 256, 16)), temperature=T)]
    pages = [page_of(CFG, LENGTHS[i % 3], variant=20 + i, seed=50 + i, **kw) for i, kw in enumerate(kws)]
    limits = [5 + (7 * i) % 23 for i in range(len(pages))]
    return pages, limits


@pytest.mark.parametrize("shared,B", [(False, 5), (True, 3)])
def test_scheduler_speculates_on_controlled_requests_and_equals_solo_runs(shared, B):
    """14 requests over the slots, controlled ones coming and going beside plain ones, right and wrong scripts and the real lookup
    side by side: every chunk is speculative and every result is the request's solo run."""
    K = 3
    plain, spec = engines("bf16", B, K, shared)
    pages, limits = traffic(plain)
    want = [solo(plain, p, n) for p, n in zip(pages, limits)]
    reasons = [r for _, r in want]
    assert "stop" in reasons and "length" in reasons
    sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, sampling=True, speculative=True, spec_policy=ALWAYS)
    try:
        spec.set_draft_script(0, want[0][0])                 # right for the first request in the slot, wrong for its successors
        spec.set_draft_script(1, [ord("b")] * 64)            # a stop entry of one request, a wrong draft for the others
        res = sch.run([SlotRequest(p, n, tag=i) for i, (p, n) in enumerate(zip(pages, limits))])
    finally:
        clear_scripts(spec, 2)
    for i, (r, (toks, reason)) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
        assert r.finish_reason == reason, f"request {i}"
    assert sch.spec_steps > 0 and sch.plain_steps == 0 and sch.spec_draft_tokens >= sch.spec_accepted_tokens > 0
    assert spec.spec_steps == sch.spec_steps and spec.plain_steps == 0


def test_without_the_option_the_same_traffic_runs_plain_chunks_and_the_refusals_are_todays():
    plain, off = engines("bf16", 5, 3, False, controls=False)
    assert not off.spec_controls
    pages, limits = traffic(plain)
    pages, limits = pages[:8], limits[:8]
    want = [solo(plain, p, n) for p, n in zip(pages, limits)]
    sch = SlotScheduler(off, max_tokens_cap=32, chunk=2, sampling=True, speculative=True, spec_policy=ALWAYS)
    res = sch.run([SlotRequest(p, n, tag=i) for i, (p, n) in enumerate(zip(pages, limits))])
    for i, (r, (toks, reason)) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
        assert r.finish_reason == reason, f"request {i}"
    assert sch.plain_steps > 0 and off.plain_steps == sch.plain_steps
    # one controlled request alone: never a speculative chunk
    sch = SlotScheduler(off, max_tokens_cap=32, chunk=2, sampling=True, speculative=True, spec_policy=ALWAYS)
    r = sch.run([SlotRequest(pages[0], limits[0], tag=0)])[0]
    np.testing.assert_array_equal(r.tokens, want[0][0])
    assert sch.spec_steps == 0 and sch.plain_steps > 0
    # the refusal strings, verbatim
    old = "the step carries guided decoding, sampling controls or logit adjustments"
    off.begin_slots(8, sampling=True)
    for kw in (dict(processing=True), dict(adjust=True)):
        off.set_step_features(True, False, **kw)
        assert off._spec_refusal() == old and not off.can_speculate()
        with pytest.raises(KarantaHipError, match=old):
            off.decode_steps(1, speculative=True)
    off.set_step_features(True, False)
    assert off.can_speculate()


def test_refusals_that_stay():
    _, spec = engines("bf16", 5, 3, False)
    spec.begin_slots(8, sampling=True)
    spec.set_step_features(True, False, processing=True, adjust=True)
    assert spec.can_speculate()
    # guided steps need SpecConfig(guided=True), with or without controls
    spec.set_vocab(TOKENS)
    spec.begin_slots(8, sampling=True, guided=True)
    spec.set_step_features(True, True, processing=True)
    with pytest.raises(KarantaHipError, match=r"SpecConfig\(guided=True\)"):
        spec.decode_steps(1, speculative=True)
    # log-probabilities force plain steps
    spec.begin_slots(8, sampling=True, logprobs=2)
    spec.set_step_features(True, False, processing=True)
    with pytest.raises(KarantaHipError, match="log-probabilities"):
        spec.decode_steps(1, speculative=True)
    assert not spec.can_speculate()
    spec.begin_slots(8)              # the greedy configuration: not in slot mode's sampled caps, nothing to refuse
    assert spec.can_speculate()


def test_an_uncontrolled_step_issues_the_launches_it_issued_before():
    """The option changes nothing for steps that carry neither pass: the same launch names, in the same order, as an engine built
    without it; a step with only `adjust` has no count launch, one with `processing` has all four."""
    from tests.launch_trace import launch_trace
    plain, on = engines("bf16", 5, 3, False)
    _, off = engines("bf16", 5, 3, False, controls=False)

    T = hot(plain, page_of(CFG, LENGTHS[0]))
    pages = [page_of(CFG, LENGTHS[b % 3], variant=b, temperature=T, seed=b) for b in range(5)]

    def names(eng, **features):
        eng.begin_slots(16, sampling=True)
        eng.admit(pages, list(range(5)))
        eng.set_step_features(True, False, **features)
        with launch_trace(eng) as calls, torch.cuda.stream(eng.stream):       # (eager, as the first step of decode_steps runs it)
            eng._spec_step_launches()
        eng.stream.synchronize()
        return [c[0] for c in calls]

    assert names(on) == names(off)
    base = names(on)
    adj = names(on, adjust=True)
    assert [n for n in adj if n not in base] == ["kr_spec_controls_trim", "kr_spec_controls_rows", "kr_logits_adjust_rows", "kr_stop_tokens"]
    proc = names(on, processing=True, adjust=True)
    new = [n for n in proc if n not in base]
    assert new == ["kr_spec_controls_trim", "kr_spec_controls_rows", "kr_logits_adjust_rows", "kr_sample_threshold_rows",
                   "kr_gumbel_argmax_processed_rows", "kr_stop_tokens", "kr_spec_controls_count"]
    assert "kr_logits_restore" not in proc and "kr_sample_count" not in proc
