"""Log-probabilities in speculative decode steps (SpecConfig(logprobs=True)) on the engine and through the slot scheduler: every
request returns exactly the tokens AND the log-probability records it has without speculation — `token`, `top` and `top_ids` as
exact arrays, the float bits included — greedy and sampled slots side by side, in the static and the shared-row layout, whatever is
drafted, beside guides and sampling controls.  The baseline is the same engine class built without `speculative`, in slot mode with
begin_slots(logprobs=5); scripted drafts (Engine.set_draft_script) make the acceptance pattern a choice of the test.  The equality
rests on the row invariance tests/test_gpu_decode32.py and tests/test_gpu_spec_engine.py pin: a draft row's logits are the bits a
one-row step at that context computes.  (Fails on a tree without the feature: SpecConfig takes no `logprobs`.)"""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402
from tests.test_gpu_spec_engine import ALWAYS, LENGTHS, repeated_pages, set_eos  # noqa: E402
from tests.test_gpu_spec_guided_engine import CFG, EOS_IDS, KW, NAME, REPEAT, TOKENS, clear_scripts  # noqa: E402

V = CFG.text.vocab_size
KLP = 5
# (weights, slots, K, shared rows): 20 rows and 8 rows run as 17, each in both layouts and with both weight formats
LAYOUTS = [("bf16", 5, 3, False), ("bf16", 5, 3, True), ("bf16", 4, 1, False), ("bf16", 4, 1, True),
           ("fp8", 5, 3, False), ("fp8", 5, 3, True), ("fp8", 4, 1, False), ("fp8", 4, 1, True)]
_E, _W = {}, {}


def engines(dtype, B, K, shared, logprobs=True, guided=False, controls=False, n_min=2, n_max=4):
    """(plain engine, speculative engine) of one configuration, kept for the module."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if NAME not in _W:
        _W[NAME] = random_weights(CFG, 909)
    keys = (("plain", dtype, B), ("spec", dtype, B, K, shared, logprobs, guided, controls, n_min, n_max))
    for key in keys:
        if key not in _E:
            sc = {} if key[0] == "plain" else {"speculative": SpecConfig(K, n_min, n_max, share_rows=shared, guided=guided,
                                                                        controls=controls, logprobs=logprobs)}
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


def mixed_pages(plain, B, **kw):
    """Greedy and sampled slots in turn, the sampled ones at a temperature at which the noise decides."""
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    return [page_of(CFG, LENGTHS[b % 3], variant=b, temperature=T if b % 2 else 0.0, seed=(0xFFFFFFF0 + 3 * b) & 0xFFFFFFFF, **kw)
            for b in range(B)]


def records(eng, B, gen, fin, n_max=None):
    """Per slot (tokens, log-probability records): the token that finished a slot has none."""
    out = []
    for b in range(B):
        n = int(gen[b]) if n_max is None else int(min(gen[b], n_max))
        ended = bool(fin[b]) and n == int(gen[b])
        out.append((eng.slot_tokens(b, n), eng.slot_logprobs(b, n - (1 if ended else 0), KLP)))
    return out


def plain_run(eng, pages, n_tokens, **features):
    B = len(pages)
    eng.begin_slots(n_tokens + 8, sampling=True, logprobs=KLP, **features)
    eng.admit(pages, list(range(B)))
    eng.decode_steps(n_tokens - 1)
    fin, gen = eng.poll_slots()
    return records(eng, B, gen, fin, n_tokens), [bool(f) for f in fin[:B]]


def spec_run(spec, pages, scripts, steps, budget, **features):
    B = len(pages)
    spec.begin_slots(budget, sampling=True, logprobs=KLP, **features)
    spec.admit(pages, list(range(B)))
    assert spec.spec_logprobs and spec.can_speculate()
    try:
        for b in range(B):
            if scripts is not None:
                spec.set_draft_script(b, scripts[b])
        spec.decode_steps(steps, speculative=True)
        fin, gen = spec.poll_slots()
        prop, acc = spec.spec_counters()
        got = records(spec, B, gen, fin)
    finally:
        clear_scripts(spec, B)
    return got, [bool(f) for f in fin[:B]], gen, prop, acc


def same_bits(a, b, msg):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b,
                                  err_msg=msg)


def check(truth, fin_truth, got, fin, gen):
    """Every slot: its tokens are a prefix of the plain run's, and the records of those tokens are the plain run's, bit for bit."""
    n_rec = 0
    for b, ((toks, lp), (t_toks, t_lp)) in enumerate(zip(got, truth)):
        n = int(gen[b])
        n = min(n, len(t_toks))
        np.testing.assert_array_equal(toks[:n], t_toks[:n], err_msg=f"slot {b}: tokens")
        ended = fin_truth[b] and n == len(t_toks)
        assert fin[b] == ended or int(gen[b]) > len(t_toks), f"slot {b}: finished after {n} of {len(t_toks)} tokens"
        m = min(len(lp["token"]), len(t_lp["token"]))
        assert m == min(n - (1 if ended else 0), len(t_lp["token"])), f"slot {b}: {m} records for {n} tokens"
        for key in ("token", "top", "top_ids"):
            same_bits(lp[key][:m], t_lp[key][:m], f"slot {b}: logprobs[{key!r}]")
        assert np.isfinite(lp["token"][:m]).all() and (lp["top"][:m, 0] >= lp["token"][:m]).all()
        n_rec += m
    return n_rec


def wrong(truth_tokens):
    """The plain continuation gone wrong at chosen generated-token indices: draft 1, 2 and 3 of a step in turn."""
    scripts = []
    for b, tr in enumerate(truth_tokens):
        sc = [int(t) for t in tr]
        for i in (1 + b % 3, 6 + b % 2, 11 + b % 3, 17, 18 + b % 4):
            if i < len(sc):
                sc[i] = (sc[i] + 1 + b) % 256
        scripts.append(sc)
    return scripts


# ----------------------------------------------------------------------------- scripted drafts
@pytest.mark.parametrize("mode", ["full", "partial"])
@pytest.mark.parametrize("dtype,B,K,shared", LAYOUTS)
def test_the_records_are_the_plain_steps(dtype, B, K, shared, mode):
    """Full acceptance (every live slot gains K + 1 records per step where it has the rows) and scripts wrong at draft 1, 2 and 3 of
    a step; half of the slots sample."""
    S = 6
    N = 1 + S * (K + 1)
    plain, spec = engines(dtype, B, K, shared)
    pages = mixed_pages(plain, B)
    assert any(p.temperature > 0 for p in pages) and any(p.temperature == 0 for p in pages)
    truth, fin_truth = plain_run(plain, pages, N)
    toks = [t for t, _ in truth]
    scripts = [[int(t) for t in tr] for tr in toks] if mode == "full" else wrong(toks)
    got, fin, gen, prop, acc = spec_run(spec, pages, scripts, S, N + 8)
    n_rec = check(truth, fin_truth, got, fin, gen)
    assert n_rec > B * S, "some step recorded more than one token of a slot"
    if mode == "full":
        assert int(acc.sum()) == int(prop.sum()) > 0
        if B * (K + 1) <= spec.rows:
            assert all(int(gen[b]) == len(toks[b]) for b in range(B))
    else:
        assert 0 < int(acc.sum()) < int(prop.sum())
    assert spec.spec_steps == S and spec.plain_steps == 0


@pytest.mark.parametrize("dtype,B,K,shared", [LAYOUTS[0], LAYOUTS[3], LAYOUTS[5]])
def test_prompt_lookup_records_the_plain_steps(dtype, B, K, shared):
    """No script: n-gram drafts from prompts with repeated spans."""
    plain, spec = engines(dtype, B, K, shared, n_min=1, n_max=3)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    pages = [dataclasses.replace(p, temperature=T if b % 2 else 0.0, seed=(0xFFFFFFFE + b) & 0xFFFFFFFF)
             for b, p in enumerate(repeated_pages(CFG, B))]
    N, S = 33, 14
    truth, fin_truth = plain_run(plain, pages, N)
    got, fin, gen, prop, acc = spec_run(spec, pages, None, S, 2 + S * (K + 1))
    assert int(prop.sum()) > 0, "the lookup proposed nothing: the test needs prompts it finds matches in"
    assert check(truth, fin_truth, got, fin, gen) >= B * min(S, N - 1)


# ----------------------------------------------------------------------------- beside guides and controls
def test_a_guided_step_records_the_plain_steps():
    """SpecConfig(guided=True, controls=True, logprobs=True), guided and unguided slots: kr_spec_guide_trim writes ctx_before, no mark
    launch; the records are of the RAW logits, not of the masked ones."""
    dtype, B, K, shared = LAYOUTS[0]
    plain, spec = engines(dtype, B, K, shared, guided=True, controls=True)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    pages = [page_of(CFG, LENGTHS[b % 3], variant=b, guide=REPEAT if b % 2 == 0 else None, temperature=T if b % 3 else 0.0, seed=77 + b)
             for b in range(B)]
    S = 5
    N = 1 + S * (K + 1)
    truth, fin_truth = plain_run(plain, pages, N, guided=True)
    scripts = wrong([t for t, _ in truth])
    got, fin, gen, prop, acc = spec_run(spec, pages, scripts, S, N + 8, guided=True)
    assert check(truth, fin_truth, got, fin, gen) > B * S and 0 < int(acc.sum()) < int(prop.sum())
    # raw: somewhere the guide forbids the most probable token, and the record still names it
    assert any(int(lp["top_ids"][i, 0]) != int(toks[i]) and pages[b].temperature == 0
               for b, (toks, lp) in enumerate(got) for i in range(len(lp["token"])) if pages[b].guide is not None)


def test_a_controlled_step_records_the_raw_logits():
    """logit_bias + min_tokens + a stop id + penalties: the adjusted logits are put back (kr_logits_restore_rows) before the
    records are taken, so they are the plain run's, which records behind kr_logits_restore; the stop id ends its slot without a
    record."""
    dtype, B, K, shared = LAYOUTS[0]
    plain, spec = engines(dtype, B, K, shared, guided=True, controls=True)
    S = 6
    N = 1 + S * (K + 1)
    bare = mixed_pages(plain, B)
    bare_truth, _ = plain_run(plain, bare, N)
    eos = int(EOS_IDS[0])
    pages = []
    for b, (p, (toks, _)) in enumerate(zip(bare, bare_truth)):
        toks = [int(t) for t in toks]
        common = [int(t) for t in np.argsort(-np.bincount(toks, minlength=V))[:2]]
        late = next((t for i, t in enumerate(toks) if i >= 5 and t not in toks[:i] and t not in EOS_IDS), toks[-1])
        kw = [dict(logit_bias={common[0]: -100.0, common[1]: 2.5}, min_tokens=3, stop_token_ids=(late,), repetition_penalty=1.3,
                   frequency_penalty=0.5), dict(logit_bias={eos: 100.0}, min_tokens=6), dict(stop_token_ids=(late,)),
              dict(presence_penalty=0.8, top_k=8), dict()][b % 5]
        pages.append(dataclasses.replace(p, **kw))
    truth, fin_truth = plain_run(plain, pages, N)
    assert any(f and len(t) < N for f, (t, _) in zip(fin_truth, truth)), "a slot ends on its stop id or on the biased EOS"
    assert any(len(t) != len(bt) or (np.asarray(t) != np.asarray(bt)).any() for (t, _), (bt, _) in zip(truth, bare_truth))
    scripts = wrong([t for t, _ in truth])
    got, fin, gen, prop, acc = spec_run(spec, pages, scripts, S, N + 8)
    assert check(truth, fin_truth, got, fin, gen) > B * 3 and int(acc.sum()) > 0
    # raw: the slot whose EOS carries +100 until min_tokens lets it through reports the EOS far from the top
    toks, lp = got[1]
    assert int(toks[-1]) in EOS_IDS and len(lp["token"]) == len(toks) - 1


def test_an_eos_inside_a_step_ends_the_records_one_short_of_the_tokens():
    """EOS ids of the test's choice that the sequences emit as the second or third token of an accepted run."""
    dtype, B, K, shared = LAYOUTS[0]
    plain, spec = engines(dtype, B, K, shared)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    pages = [page_of(CFG, LENGTHS[b % 3], variant=b, temperature=T, seed=900 + b) for b in range(B)]     # (sampled: no token twice early on)
    S = 4
    N = 1 + S * (K + 1)
    # the first token at index >= lo that is new to its sequence and, under full acceptance, not the first token of a step
    first_new = lambda toks, lo: next(int(t) for i, t in enumerate(toks)
                                      if i >= lo and (i - 1) % (K + 1) != 0 and int(t) not in [int(x) for x in toks[:i]])
    try:
        free, _ = plain_run(plain, pages, N)
        ids = (first_new(free[0][0], 2), first_new(free[1][0], 6))      # slot 0 ends inside its first step, slot 1 inside a later one
        for e in (plain, spec):
            set_eos(e, ids)
        truth, fin_truth = plain_run(plain, pages, N)
        assert fin_truth[0] and fin_truth[1] and 3 <= len(truth[0][0]) < N and 3 <= len(truth[1][0]) < N
        assert any((len(truth[b][0]) - 2) % (K + 1) != 0 for b in (0, 1)), "an EOS that is not the first token of its step"
        scripts = [[int(t) for t in tr] + [3] * 8 for tr, _ in free]
        got, fin, gen, prop, acc = spec_run(spec, pages, scripts, S, N + 8)
        check(truth, fin_truth, got, fin, gen)
        for b in (0, 1):
            toks, lp = got[b]
            assert fin[b] and int(toks[-1]) in ids and len(toks) == len(truth[b][0]) and len(lp["token"]) == len(toks) - 1
    finally:
        for e in (plain, spec):
            set_eos(e, CFG.eos_token_ids)


# ----------------------------------------------------------------------------- through the scheduler
@pytest.mark.parametrize("shared,B", [(False, 5), (True, 3)])
def test_scheduler_results_carry_the_solo_runs_records(shared, B):
    """12 requests over the slots, with different top_logprobs and without, right and wrong scripts and the real lookup side by side:
    every chunk is speculative, every result's tokens and SlotResult.logprobs are those of the request's solo plain run."""
    K = 3
    plain, spec = engines("bf16", B, K, shared)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    ks = [5, 0, None, 2, 5, 1, 3, None, 5, 4, 0, 5]
    pages = [page_of(CFG, LENGTHS[i % 3], variant=20 + i, seed=50 + i, temperature=T if i % 3 == 1 else 0.0, logprobs=k)
             for i, k in enumerate(ks)]
    limits = [5 + (7 * i) % 23 for i in range(len(pages))]
    want = [plain.generate([p], n) for p, n in zip(pages, limits)]
    sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, sampling=True, logprobs=KLP, speculative=True, spec_policy=ALWAYS)
    try:
        spec.set_draft_script(0, want[0].tokens[0])          # right for the first request in the slot, wrong for its successors
        spec.set_draft_script(1, [3] * 64)
        res = sch.run([SlotRequest(p, n, tag=i) for i, (p, n) in enumerate(zip(pages, limits))])
    finally:
        clear_scripts(spec, 2)
    for i, (r, w) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, w.tokens[0], err_msg=f"request {i}")
        assert r.finish_reason == w.finish_reasons[0], f"request {i}"
        wl = w.logprobs[0] if w.logprobs is not None else None
        assert (r.logprobs is None) == (wl is None) == (ks[i] is None), f"request {i}"
        if wl is not None:
            for key in ("token", "top", "top_ids"):
                same_bits(r.logprobs[key], wl[key], f"request {i}: logprobs[{key!r}]")
            assert r.logprobs["top"].shape == (len(r.tokens) - (r.finish_reason == "stop"), ks[i])
    assert sch.spec_steps > 0 and sch.plain_steps == 0 and sch.spec_accepted_tokens > 0
    assert spec.spec_steps == sch.spec_steps and spec.plain_steps == 0


# ----------------------------------------------------------------------------- the launches, and the refusal that stays
def test_the_launches_of_a_step_with_and_without_records():
    """An engine built without logprobs=True issues the launches of an engine that never heard of the option; one built with it
    issues them too while nothing is recorded, and the three new ones at their places when it is: the mark at the head where no trim
    runs, restore and records behind the verification and kr_stop_tokens, in front of the counts, the guide's advance and the
    repetition pass."""
    from tests.launch_trace import launch_trace
    plain, on = engines("bf16", 5, 3, False, guided=True, controls=True)
    _, off = engines("bf16", 5, 3, False, logprobs=False, guided=True, controls=True)
    _, shared = engines("bf16", 5, 3, True)
    T = hot(plain, page_of(CFG, LENGTHS[0]))
    pages = [page_of(CFG, LENGTHS[b % 3], variant=b, temperature=T, seed=b) for b in range(5)]

    def names(eng, logprobs=None, guided=False, **features):
        eng.begin_slots(16, sampling=True, guided=guided, logprobs=logprobs)
        eng.admit(pages, list(range(5)))
        eng.set_step_features(True, guided, **features)
        with launch_trace(eng) as calls, torch.cuda.stream(eng.stream):       # (eager, as the first step of decode_steps runs it)
            eng._spec_step_launches()
        eng.stream.synchronize()
        return [c[0] for c in calls]

    new = ("kr_spec_mark", "kr_logits_restore_rows", "kr_logprobs_topk_rows")
    for kw in (dict(), dict(adjust=True), dict(processing=True, adjust=True, repetition=True), dict(guided=True)):
        base = names(off, **kw)
        assert names(on, **kw) == base and not set(new) & set(base), kw
    # nothing but the Gumbel pass: mark first, the records last
    base, rec = names(on), names(on, logprobs=KLP)
    assert rec == ["kr_spec_mark"] + base + ["kr_logprobs_topk_rows"]
    assert base[-1] == "kr_spec_accept"
    rec = names(shared, logprobs=KLP)
    assert rec[0] == "kr_spec_mark" and rec[-2:] == ["kr_spec_accept_rows", "kr_logprobs_topk_rows"]
    assert names(shared) == rec[1:-1]
    # adjustments, controls and repetition: the trim marks; restore and records between kr_stop_tokens and the counts
    base, rec = names(on, processing=True, adjust=True, repetition=True), names(on, logprobs=KLP, processing=True, adjust=True, repetition=True)
    i = base.index("kr_stop_tokens") + 1
    assert base[i:] == ["kr_spec_controls_count", "kr_repeat_detect"]
    assert rec == base[:i] + ["kr_logits_restore_rows", "kr_logprobs_topk_rows"] + base[i:]
    # a guide alone: its trim marks, nothing is restored, the records come before the advance
    base, rec = names(on, guided=True), names(on, logprobs=KLP, guided=True)
    assert base[-2:] == ["kr_spec_accept", "kr_spec_guide_advance"]
    assert rec == base[:-1] + ["kr_logprobs_topk_rows", "kr_spec_guide_advance"]


def test_without_the_option_the_refusal_is_todays():
    _, off = engines("bf16", 5, 3, False, logprobs=False, guided=True, controls=True)
    assert not off.spec_logprobs
    off.begin_slots(8, sampling=True, logprobs=2)
    assert off._spec_refusal() == "log-probabilities are recorded" and not off.can_speculate()
    with pytest.raises(KarantaHipError, match="log-probabilities are recorded"):
        off.decode_steps(1, speculative=True)
    with pytest.raises(KarantaHipError, match="speculative decode step refused: log-probabilities are recorded"):
        off._spec_step_launches()
    off.begin_slots(8, sampling=True)
    assert off.can_speculate()
    # through the scheduler: plain chunks, and the records of the plain run
    plain, _ = engines("bf16", 5, 3, False)
    page = page_of(CFG, LENGTHS[0], variant=3, logprobs=2)
    w = plain.generate([page], 9)
    sch = SlotScheduler(off, max_tokens_cap=16, chunk=2, sampling=True, logprobs=2, speculative=True, spec_policy=ALWAYS)
    r = sch.run([SlotRequest(page, 9, tag=0)])[0]
    np.testing.assert_array_equal(r.tokens, w.tokens[0])
    same_bits(r.logprobs["top"], w.logprobs[0]["top"], "the plain chunks' records")
    assert sch.spec_steps == 0 and sch.plain_steps > 0
