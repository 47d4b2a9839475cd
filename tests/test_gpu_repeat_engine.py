"""Repetition detection end to end on the engine: a response under detection equals the response without it, cut where
tests/repeat_ref.py cuts it.  Guided patterns that allow exactly one token in every state (test_repeat_cpu.py proves that on the
CPU) force the output, so the loops are certain whatever the random weights say; for every row the reference's index is asserted
first — an index for the loops, none for the controls — so no comparison below can pass vacuously.  Covered: Engine.generate, the
slot scheduler with plain steps, speculative steps on guided requests in both row layouts (drafts accepted), a logit_bias-forced
loop on the adjust path, n = 2, a reused slot, log-probabilities.  (Fails on a tree without the feature: PageRequest takes no
`repetition`.)"""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.request import RepetitionParams  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy  # noqa: E402
from karanta_ocr_amd.serving import ByteTokenizer  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests import repeat_ref as R  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402

NAME = "tiny-w512"
CFG = CONFIGS[NAME]
EOS = tuple(int(e) for e in CFG.eos_token_ids)
KW = dict(s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
B, K = 5, 3
N = 48                    # tokens a row may generate: past every trigger below and past the control's end
P5 = RepetitionParams(8, 2, 5)
# (guide, what it forces, parameters, tokens kept)
ROWS = [(r"(?:abc){40}", b"abc" * 40, P5, 15),
        (r"hello (?:abc){40}", b"hello " + b"abc" * 40, P5, 21),
        (r"x{100}", b"x" * 100, RepetitionParams(4, 1, 6), 6),
        (r"(?:abcdefg){20}", b"abcdefg" * 20, P5, 35),
        (r"abcdefghijklmnopqrstuvwxyz0123456789", b"abcdefghijklmnopqrstuvwxyz0123456789", P5, None)]
_E = {}


def engine(kind):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if "w" not in _E:
        _E["w"] = random_weights(CFG, 909)
    if kind not in _E:
        sc = {} if kind == "plain" else {"speculative": SpecConfig(K, 2, 4, share_rows=kind == "shared", guided=True)}
        e = _E[kind] = Engine(CFG, max_batch=B, **KW, **sc)
        e.load_weights(_E["w"])
        e.set_vocab(ByteTokenizer(CFG).token_bytes())
    return _E[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k, e in _E.items():
        if k != "w":
            e.close()
    _E.clear()


def pages(detect=True, **kw):
    return [page_of(CFG, 40 + 8 * i, variant=i, guide=g, repetition=p if detect else None, **kw) for i, (g, _, p, _) in enumerate(ROWS)]


def expected():
    """Per row (tokens without the EOS a completed pattern ends on, finish_reason, stop_reason) from the reference, checked against
    the hand-worked counts first."""
    out = []
    for _, forced, p, kept in ROWS:
        y = list(forced)[:N]
        g = R.first_repeat(y, *p.row())
        assert (g is None) == (kept is None) and (g is None or g + 1 == kept), (forced[:12], g, kept)
        full = len(forced) < N                              # the pattern completes: the EOS follows, "stop"
        toks, reason, cause = R.cut(y + ([EOS[0]] if full else []), p.row(), stop_ids=EOS)
        out.append((toks[:-1] if reason == "stop" else toks, reason, cause))
    assert [e[2] for e in out] == ["repetition"] * 4 + [None] and out[4][1] == "stop"
    return out


def same(tokens, reason, cause, want, what):
    toks = [int(t) for t in tokens]
    if want[1] == "stop":
        assert toks[-1] in EOS, what
        toks = toks[:-1]
    assert (toks, reason, cause) == want, what


def test_generate_cuts_where_the_reference_does():
    eng, want = engine("plain"), expected()
    free = eng.generate(pages(detect=False), N)
    assert free.stop_reasons == [None] * len(ROWS)
    for b, (_, forced, p, _) in enumerate(ROWS):            # the guides do force the output: the undetected run is the pattern
        n = min(N, len(forced))
        assert [int(t) for t in free.tokens[b][:n]] == list(forced)[:n], b
        same(*R.cut(free.tokens[b], p.row(), stop_ids=EOS), want[b], f"the reference's cut of the undetected row {b}")
    got = eng.generate(pages(), N, sync_every=8)
    for b in range(len(ROWS)):
        same(got.tokens[b], got.finish_reasons[b], got.stop_reasons[b], want[b], f"row {b}")
    # the device finished the rows: the batch ends at the first look after its last row's end (the control's EOS, token 37)
    assert got.timings["decode_steps"] == 39 and free.timings["decode_steps"] == N - 1


def run_scheduler(eng, reqs, **kw):
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=2, sampling=True, guided=True, **kw)
    res = sch.run(reqs)
    assert all(r.error is None for r in res), [r.error for r in res]
    return sch, res


@pytest.mark.parametrize("launch_ahead", [False, True])
def test_slot_scheduler_plain_steps(launch_ahead):
    eng, want = engine("plain"), expected()
    sch, res = run_scheduler(eng, [SlotRequest(p, N) for p in pages()], launch_ahead=launch_ahead)
    for b, r in enumerate(res):
        same(r.tokens, r.finish_reason, r.stop_reason, want[b], f"row {b}")
    assert sch.repetition_stops == 4 and sch.repetition_tokens_cut == sum(N - k for *_, k in ROWS if k)
    assert sch.spec_steps == 0


@pytest.mark.parametrize("kind", ["static", "shared"])
def test_speculative_steps_cut_at_the_same_index(kind):
    eng, want = engine(kind), expected()
    assert eng.spec_guided and eng.share_rows == (kind == "shared")
    sch, res = run_scheduler(eng, [SlotRequest(p, N) for p in pages()], speculative=True, spec_policy=SpecPolicy(break_even=0.0))
    for b, r in enumerate(res):
        same(r.tokens, r.finish_reason, r.stop_reason, want[b], f"{kind} row {b}")
    assert sch.spec_steps > 0 and sch.plain_steps == 0, "a request with detection must not force plain steps"
    assert sch.spec_accepted_tokens > 0, "no draft was accepted: the cut was never inside a speculative step"
    assert sch.repetition_stops == 4


def test_logit_bias_forced_loop_on_the_adjust_path():
    eng = engine("plain")
    tok, p = 65, RepetitionParams(1, 1, 8)
    base = page_of(CFG, 64, variant=7, logit_bias={tok: 100.0})
    _, (free,) = run_scheduler(eng, [SlotRequest(base, 20)])
    assert free.tokens.tolist() == [tok] * 20 and R.first_repeat(free.tokens.tolist(), *p.row()) == 7
    sch, (got,) = run_scheduler(eng, [SlotRequest(dataclasses.replace(base, repetition=p), 20)])
    assert (got.tokens.tolist(), got.finish_reason, got.stop_reason) == ([tok] * 8, "length", "repetition")
    assert sch.repetition_tokens_cut == 12


def test_both_children_of_n_2_are_cut():
    eng, want = engine("plain"), expected()
    T = hot(eng, page_of(CFG, 40))
    page = page_of(CFG, 40, variant=3, guide=ROWS[0][0], repetition=P5, temperature=T, seed=11, n=2)
    _, (res,) = run_scheduler(eng, [SlotRequest(page, N)])
    assert len(res.choices) == 2
    for c, ch in enumerate(res.choices):
        same(ch.tokens, ch.finish_reason, ch.stop_reason, want[0], f"child {c}")
    got = eng.generate([page], N)
    for c in range(2):
        same(got.tokens[c], got.finish_reasons[c], got.stop_reasons[c], want[0], f"generate child {c}")


def test_a_reused_slot_starts_clean():
    """The first request stops at max_tokens one token short of its trigger; the next one in the same slot is cut by its own tokens."""
    eng, want = engine("plain"), expected()
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=2, sampling=True, guided=True)
    first, second = pages()[0], pages()[1]
    (r,) = sch.run([SlotRequest(first, 14)])
    assert (bytes(r.tokens.tolist()), r.finish_reason, r.stop_reason) == (b"abc" * 4 + b"ab", "length", None)
    (r,) = sch.run([SlotRequest(second, N)])
    same(r.tokens, r.finish_reason, r.stop_reason, want[1], "the slot's second request")
    (r,) = sch.run([SlotRequest(dataclasses.replace(first, repetition=None), 20)])       # ... and a third without the feature
    assert (bytes(r.tokens.tolist()), r.stop_reason) == ((b"abc" * 7)[:20], None)
    assert sch.repetition_stops == 1


def test_logprobs_cover_the_kept_tokens():
    eng, want = engine("plain"), expected()
    ps = [dataclasses.replace(p, logprobs=2) for p in pages()[:2]]
    got = eng.generate(ps, N)
    for b in range(2):
        assert len(got.tokens[b]) == ROWS[b][3]
        assert got.logprobs[b]["token"].shape == (ROWS[b][3],) and got.logprobs[b]["top_ids"].shape == (ROWS[b][3], 2)
    sch = SlotScheduler(eng, max_tokens_cap=64, chunk=2, sampling=True, guided=True, logprobs=2)
    for b, r in enumerate(sch.run([SlotRequest(p, N) for p in ps])):
        same(r.tokens, r.finish_reason, r.stop_reason, want[b], f"row {b}")
        assert r.logprobs["token"].shape == (ROWS[b][3],) and r.logprobs["top"].shape == (ROWS[b][3], 2)


def test_unguided_rows_are_the_undetected_rows_cut():
    """Whatever random weights generate: with detection on, a row is the reference's cut of the same row without it.  (This may
    find no loop at all; the guided rows above are the ones that must.)"""
    eng = engine("plain")
    p = RepetitionParams(16, 1, 3)
    base = [page_of(CFG, 40 + 12 * i, variant=10 + i) for i in range(B)]
    free = eng.generate(base, 40)
    got = eng.generate([dataclasses.replace(x, repetition=p) for x in base], 40)
    for b in range(B):
        toks, reason, cause = R.cut(free.tokens[b], p.row(), stop_ids=EOS)
        assert ([int(t) for t in got.tokens[b]], got.finish_reasons[b], got.stop_reasons[b]) == (toks, reason, cause), b
