"""Sampling controls through the engine (top_k / top_p / min_p / repetition, frequency and presence penalties) on the tiny
models: truncation to one token is greedy, a mixed batch leaves its neutral rows untouched and its processed rows equal the
numpy restatement of every decisive step, the graph path equals the eager one, a guided row stays inside its pattern, the
slot scheduler reproduces solo runs, and a batch above 16 rows takes the same path."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd._lib import KarantaHipError  # noqa: E402
from karanta_ocr_amd.engine import Engine, PageRequest  # noqa: E402
from oracle import qwen2vl_oracle as O  # noqa: E402
from tests import sampling_ref as R  # noqa: E402

STEPS = 12


@pytest.fixture(scope="module")
def engines(tiny_models):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for name in ("tiny", "tiny-2.5"):
        cfg, w, _ = tiny_models[name]
        e = Engine(cfg, max_batch=4, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
        e.load_weights(w)
        out[name] = e
    yield out
    for e in out.values():
        e.close()


def _page(cfg, i, **kw):
    rng = np.random.default_rng(500 + i)
    h, wd = [(56, 84), (84, 56), (56, 56), (112, 84)][i % 4]
    pv, grid = IP.image_to_patches(IP.synthetic_page(300 + i, h, wd))
    T = grid[1] * grid[2] // 4
    ids = np.concatenate([rng.integers(0, 400, 2 + i % 3), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                          [cfg.vision_end_token_id], rng.integers(0, 400, 3)]).astype(np.int64)
    return PageRequest(ids, pv, [grid], **kw)


def _restate(res, b, page, vocab, allowed_fn=None):
    """Engine tokens of row b against sample_step on the row's own raw logits and history; returns the decisive steps."""
    toks = res.tokens[b]
    n_ok = 0
    for i in range(len(toks)):
        allowed = None if allowed_fn is None else allowed_fn(toks[:i])
        tok, margin, excused = R.sample_step(res.logits[b, i], page.temperature, page.seed, i, page.input_ids, toks[:i], vocab,
                                             allowed, page.top_k, page.top_p, page.min_p, page.repetition_penalty,
                                             page.frequency_penalty, page.presence_penalty)
        if margin > 1e-3 and not excused:
            assert int(toks[i]) == tok, f"row {b} step {i}: engine {int(toks[i])} numpy {tok} (margin {margin:.4f})"
            n_ok += 1
    return n_ok


@pytest.mark.parametrize("name", ["tiny", "tiny-2.5"])
def test_truncation_to_one_token_is_greedy(engines, tiny_models, name):
    """top_k = 1, min_p = 1 and top_p = 1e-6 at T = 2 keep only the top token: the tokens are the greedy ones (today's code,
    which ignored the fields, samples at T = 2 instead)."""
    cfg = tiny_models[name][0]
    eng = engines[name]
    greedy = eng.generate([_page(cfg, i) for i in range(3)], STEPS, ignore_eos=True)
    pages = [_page(cfg, 0, temperature=2.0, seed=11, top_k=1), _page(cfg, 1, temperature=2.0, seed=12, min_p=1.0),
             _page(cfg, 2, temperature=2.0, seed=13, top_p=1e-6)]
    res = eng.generate(pages, STEPS, ignore_eos=True)
    for b in range(3):
        np.testing.assert_array_equal(res.tokens[b], greedy.tokens[b])


@pytest.mark.parametrize("name", ["tiny", "tiny-2.5"])
def test_mixed_batch_neutral_rows_untouched_processed_rows_restated(engines, tiny_models, name):
    cfg = tiny_models[name][0]
    V = cfg.text.vocab_size
    eng = engines[name]
    pages = [_page(cfg, 0), _page(cfg, 1, temperature=1.0, seed=5),
             _page(cfg, 2, temperature=1.2, seed=6, top_p=0.8, top_k=40, repetition_penalty=1.3, frequency_penalty=0.5,
                   presence_penalty=0.4),
             _page(cfg, 3, repetition_penalty=1.5, frequency_penalty=0.3)]
    eager = eng.generate(pages, STEPS, ignore_eos=True, return_logits=True)
    graph = eng.generate(pages, STEPS, ignore_eos=True)
    for b in range(4):
        np.testing.assert_array_equal(graph.tokens[b], eager.tokens[b])        # graph path = eager path
    for b in (0, 1):
        solo = eng.generate([pages[b]], STEPS, ignore_eos=True)
        np.testing.assert_array_equal(graph.tokens[b], solo.tokens[0])        # neutral rows bit for bit
    for b in (2, 3):
        n = _restate(eager, b, pages[b], V)
        assert n >= 3, f"row {b}: only {n} decisive steps"
    with pytest.raises(KarantaHipError, match="force_tokens"):
        eng.generate(pages, 3, force_tokens=np.zeros((4, 3), np.int64))


def test_guided_row_with_controls_stays_in_its_pattern(engines, tiny_models):
    from karanta_ocr_amd import guided as G
    from karanta_ocr_amd.serving import ByteTokenizer
    cfg = tiny_models["tiny"][0]
    eng = engines["tiny"]
    voc = ByteTokenizer(cfg).token_bytes()
    eng.set_vocab(voc)
    pattern = r"[a-f]{3}-[0-9]{2}(?:;[a-z ]{2,5})?"
    g = G.compile_regex(pattern)
    page = _page(cfg, 1, guide=g, temperature=1.0, seed=21, top_p=0.7, repetition_penalty=1.4)
    res = eng.generate([page, _page(cfg, 2)], 16, return_logits=True)
    toks = res.tokens[0]
    assert res.finish_reasons[0] == "stop"
    assert re.fullmatch(pattern, b"".join(voc[int(t)] for t in toks[:-1]).decode())

    def allowed(prev):
        st = g.start
        for t in prev:
            st = O.guide_walk(g.trans, st, voc[int(t)])
        return O.guide_token_mask(g.trans, g.accept, st, voc, cfg.eos_token_ids)

    assert _restate(res, 0, page, cfg.text.vocab_size, allowed) >= 3


def test_slot_scheduler_processed_requests_equal_solo(tiny_models):
    """Slot reuse: processed requests land in slots that held others (counts cleared, prompt bits rewritten) and give their solo
    generate() tokens; a neutral request next to them too."""
    from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
    cfg, w, _ = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=2, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
    eng.load_weights(w)
    pages = [_page(cfg, 0, temperature=1.0, seed=3, top_p=0.9, repetition_penalty=1.3, frequency_penalty=0.6),
             _page(cfg, 1),
             _page(cfg, 2, repetition_penalty=1.5, presence_penalty=0.8),
             _page(cfg, 3, temperature=0.8, seed=4, min_p=0.05, top_k=20, frequency_penalty=1.0)]
    limits = [9, 5, 12, 10]
    solo = [eng.generate([p], m) for p, m in zip(pages, limits)]
    sch = SlotScheduler(eng, max_tokens_cap=12, chunk=3, sampling=True)
    res = sch.run([SlotRequest(p, m, tag=i) for i, (p, m) in enumerate(zip(pages, limits))])
    for r, s in zip(res, solo):
        assert r.error is None
        np.testing.assert_array_equal(r.tokens, s.tokens[0])
    with pytest.raises(KarantaHipError, match="greedy configuration"):
        SlotScheduler(eng, max_tokens_cap=12, chunk=3)
        eng.admit([pages[2]], [0])
    eng.close()


def test_batch_above_16_rows(tiny_models):
    """tiny-w512 at 17 rows (wide mode, two 16-row column tiles): top_k = 1 rows at T = 2 are greedy, neutral rows untouched."""
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.weights import random_weights
    cfg = CONFIGS["tiny-w512"]
    eng = Engine(cfg, max_batch=17, s_max=512, max_patches=4096, max_prompt_tokens=4096, decode_splits=2)
    eng.load_weights(random_weights(cfg, 909))
    plain = [_page(cfg, i) for i in range(17)]
    greedy = eng.generate(plain, 8, ignore_eos=True)
    pages = [_page(cfg, i, temperature=2.0, seed=i, top_k=1) if i % 2 else _page(cfg, i) for i in range(17)]
    res = eng.generate(pages, 8, ignore_eos=True)
    for b in range(17):
        np.testing.assert_array_equal(res.tokens[b], greedy.tokens[b])
    eng.close()
