"""The engine with an fp8 (e4m3fn) KV cache — Engine(kv_cache_dtype="fp8"): prefill through the bf16 scratch + kr_kv_quantize,
the ROPE_KV8 append of the qkv launches, attention on fp8 operands, the byte-sized fork — on the seeded tiny models.

Exactness: the quantisation is elementwise and deterministic, so every property that holds bit for bit on the bf16 cache holds
on the fp8 cache — a page's tokens do not depend on the batch, the slot or the scheduler it runs in, forked children and
prefix-cache hits equal their own prefill, a speculative run emits the plain run's tokens.  Accuracy: against the fp32 oracle,
teacher-forced, next to the bf16-cache engine on the same pages.  The default (kv_cache_dtype="auto") is the engine as it was."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd._lib import KarantaHipError  # noqa: E402
from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, PageRequest, SpecConfig  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from oracle import qwen2vl_oracle as O  # noqa: E402
from oracle.tolerances import LOGIT_TOL_REL, LOGIT_TOL_REL_FP32, TOKEN_MARGIN_FACTOR  # noqa: E402
from tests.prodwidth import compare_teacher_forced, margins  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402
from tests.test_gpu_spec_engine import plain_run, repeated_pages  # noqa: E402

KW = dict(s_max=512, max_patches=4096, max_prompt_tokens=4096, decode_splits=2)

# Teacher-forced relative logit error (max |engine - oracle(fp32)| over a step's logits / max |oracle logit| at the last prompt
# position), worst of 16 steps, tiny-gqa, weight seeds 4000 / 4001 / 4002, measured on an MI355X (scales 1.0):
#   bf16 KV cache   0.43 %, 0.43 %, 0.55 %      (asserted under LOGIT_TOL_REL_FP32 = 3 %)
#   fp8 KV cache    1.16 %, 1.16 %, 1.64 %      (the prefill step is the bf16 run's: 0.27 %, 0.30 %, 0.39 %)
# 1.5 x the largest fp8 figure would be 2.45 %; the fp8 error already fits under LOGIT_TOL_REL = 2 % — the tolerance of the
# same-policy comparison, tighter than the one the bf16 cache is held to against this oracle — so that constant is the threshold.
# All 16 steps of every seed are decisive at either tolerance (oracle margins, computed without the engine).
ORACLE_SEEDS = (4000, 4001, 4002)
KV8_LOGIT_TOL_REL_FP32 = LOGIT_TOL_REL


def ragged_pages(cfg, n, seed=99):
    rng = np.random.default_rng(seed)
    pages = []
    for i in range(n):
        h, wd = [(112, 168), (56, 84), (140, 140), (56, 56), (84, 56)][i % 5]
        pv, grid = IP.image_to_patches(IP.synthetic_page(i, h, wd))
        T = grid[1] * grid[2] // 4
        ids = np.concatenate([rng.integers(0, 400, 2 + (7 * i) % 23), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                              [cfg.vision_end_token_id], rng.integers(0, 400, 3 + i % 4)]).astype(np.int64)
        pages.append(PageRequest(ids, pv, [grid]))
    return pages


def layer_scales(cfg):
    """Scales that differ per layer and between K and V, so that a wrong row of the table changes the tokens' logits."""
    i = np.arange(cfg.text.num_layers)
    return 0.25 * (1 + i / 4.0), 0.125 * (1 + i / 2.0)


def kv8_engine(cfg, w, max_batch=4, scales=True, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine(cfg, max_batch=max_batch, kv_cache_dtype="fp8", **{**KW, **kw})
    e.load_weights(w)
    assert e.kv8 and e.kcache.dtype == torch.uint8 and e.vtcache.dtype == torch.uint8
    if scales:
        e.set_kv_scales(*layer_scales(cfg))
    return e


# ----------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", ["tiny", "tiny-gqa"])
def test_three_ragged_pages_equal_their_solo_runs(tiny_models, name):
    cfg, w, _ = tiny_models[name]
    eng = kv8_engine(cfg, w)
    pages = ragged_pages(cfg, 3)
    together = eng.generate(pages, 12, ignore_eos=True, return_logits=True)
    for i, pg in enumerate(pages):
        alone = eng.generate([pg], 12, ignore_eos=True, return_logits=True)
        np.testing.assert_array_equal(alone.tokens[0], together.tokens[i])
        np.testing.assert_array_equal(alone.logits[0].view(np.uint32), together.logits[i].view(np.uint32))
    graph = eng.generate(pages, 12, ignore_eos=True, use_graph=True)             # the scale table is a static device buffer
    for i in range(3):
        np.testing.assert_array_equal(graph.tokens[i], together.tokens[i])
    # the cache really is quantised: the bf16-cache engine gives other logits from the first decode step on, the same prefill logits
    ref = Engine(cfg, max_batch=4, **KW)
    ref.load_weights(w)
    r16 = ref.generate(pages[:1], 4, ignore_eos=True, return_logits=True)
    np.testing.assert_array_equal(r16.logits[0, 0], together.logits[0, 0])
    assert np.abs(r16.logits[0, 1] - together.logits[0, 1]).max() > 1e-4
    assert eng.kv_cache_bytes() * 2 == ref.kv_cache_bytes()
    ref.close(), eng.close()


@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8"])
def test_twenty_ragged_pages_equal_their_solo_runs(weight_dtype):
    """20 rows: the packed 17..32-row family (kr_linear_decode32_kv8); the solo runs and a batch of three take the <= 16-row launches
    (kr_linear_decode_narrow_kv8).  weight_dtype fp8: both on e4m3 weights."""
    cfg = CONFIGS["tiny-w512"]
    eng = kv8_engine(cfg, random_weights(cfg, 909), max_batch=20, weight_dtype=weight_dtype)
    pages = ragged_pages(cfg, 20, seed=77)
    together = eng.generate(pages, 10, ignore_eos=True)
    three = eng.generate(pages[5:8], 10, ignore_eos=True)
    for i in (0, 1, 6, 13, 19):
        np.testing.assert_array_equal(eng.generate([pages[i]], 10, ignore_eos=True).tokens[0], together.tokens[i], err_msg=f"page {i}")
    for j in range(3):
        np.testing.assert_array_equal(three.tokens[j], together.tokens[5 + j])
    assert len({tuple(t.tolist()) for t in together.tokens}) > 10
    eng.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_slot_scheduler_equals_solo(tiny_models, overlap):
    cfg, w, _ = tiny_models["tiny-gqa"]
    pages, limits = ragged_pages(cfg, 7, seed=123), [9, 20, 5, 14, 1, 17, 11]
    eng = kv8_engine(cfg, w, max_batch=3)
    free = [eng.generate([pg], 20, ignore_eos=True).tokens[0] for pg in pages]
    eng.close()
    eng = kv8_engine(dataclasses.replace(cfg, eos_token_ids=(int(free[0][4]), int(free[3][9]), int(free[5][2]))), w, max_batch=3)
    solo = [eng.generate([pg], mt) for pg, mt in zip(pages, limits)]
    sch = SlotScheduler(eng, max_tokens_cap=20, chunk=3, overlap=overlap)
    res = sch.run([SlotRequest(pg, mt, tag=i) for i, (pg, mt) in enumerate(zip(pages, limits))])
    for r, s in zip(res, solo):
        assert r.error is None
        np.testing.assert_array_equal(r.tokens, s.tokens[0])
        assert r.finish_reason == s.finish_reasons[0]
    assert {r.finish_reason for r in res} == {"stop", "length"}
    eng.close()


@pytest.mark.parametrize("P", [40, 64, 100])
def test_children_and_prefix_cache_hits_equal_their_own_prefill(tiny_models, P):
    """n = 3 (kr_kv_fork8 of the prompt's codes) and a prefix-cache hit in place: the tokens and logits of the page's own prefill."""
    cfg, w, _ = tiny_models["tiny-gqa"]
    eng = kv8_engine(cfg, w)
    one = eng.generate([page_of(cfg, P)], 12, ignore_eos=True, return_logits=True)
    before = eng.pages_prefilled
    three = eng.generate([page_of(cfg, P, n=3)], 12, ignore_eos=True, return_logits=True)
    assert eng.pages_prefilled - before == 1 and three.logits.shape[0] == 3
    for c in range(3):
        np.testing.assert_array_equal(three.tokens[c], one.tokens[0])
        np.testing.assert_array_equal(three.logits[c].view(np.uint32), one.logits[0].view(np.uint32), err_msg=f"child {c}")
    page = page_of(cfg, P, variant=5)
    page.temperature = hot(eng, page)
    retry = dataclasses.replace(page, seed=77)
    solo = [eng.generate([p], 12).tokens[0] for p in (page, retry)]
    sch = SlotScheduler(eng, max_tokens_cap=20, chunk=2, sampling=True, prefix_cache=True)
    r1 = sch.run([SlotRequest(page, 12, prompt_key=b"k" * 16)])[0]
    before = eng.pages_prefilled
    r2 = sch.run([SlotRequest(retry, 12, prompt_key=b"k" * 16)])[0]
    assert eng.pages_prefilled == before and sch.prefix_cache_hits == 1
    np.testing.assert_array_equal(r1.tokens, solo[0])
    np.testing.assert_array_equal(r2.tokens, solo[1])
    eng.close()


@pytest.mark.parametrize("share_rows,B", [(False, 5), (True, 9)])
def test_speculative_run_emits_the_plain_runs_tokens(share_rows, B):
    """Prompt-lookup drafts on prompts with repeated spans, K = 3: 20 rows on 5 slots, and 9 slots sharing the rows of a step
    (kr_linear_decode32_kv8 with the row map, kr_attn_decode_rows_kv8)."""
    cfg = CONFIGS["tiny-w512"]
    w = random_weights(cfg, 909)
    plain = kv8_engine(cfg, w, max_batch=B)
    spec = kv8_engine(cfg, w, max_batch=B, speculative=SpecConfig(3, 1, 3, share_rows=share_rows))
    pages = repeated_pages(cfg, B)
    N, S = 33, 14
    truth = plain_run(plain, pages, N)
    spec.begin_slots(2 + S * 4)
    spec.admit(pages, list(range(B)))
    spec.decode_steps(S, speculative=True)
    _, gen = spec.poll_slots()
    prop, acc = spec.spec_counters()
    assert int(prop.sum()) > 0 and int(acc.sum()) > 0, "the test needs drafts that are proposed and accepted"
    for b in range(B):
        n = int(min(gen[b], len(truth[b])))
        assert n >= min(len(truth[b]), 1 + S)
        np.testing.assert_array_equal(spec.slot_tokens(b, n), truth[b][:n], err_msg=f"slot {b}")
    plain.close(), spec.close()


# ----------------------------------------------------------------------------- the default, refusals, the counter
def test_auto_is_the_engine_without_the_keyword(tiny_models):
    cfg, w, _ = tiny_models["tiny-gqa"]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pages = ragged_pages(cfg, 3)
    out = []
    for kw in ({}, {"kv_cache_dtype": "auto"}, {"kv_cache_dtype": "bfloat16"}):
        e = Engine(cfg, max_batch=4, **KW, **kw)
        e.load_weights(w)
        assert not e.kv8 and e.kcache.dtype == torch.bfloat16 and e.kv_clamped == 0
        with pytest.raises(KarantaHipError, match="bfloat16"):
            e.set_kv_scales(np.ones(cfg.text.num_layers), np.ones(cfg.text.num_layers))
        out.append(e.generate(pages, 10, ignore_eos=True, return_logits=True))
        e.close()
    for r in out[1:]:
        np.testing.assert_array_equal(r.logits.view(np.uint32), out[0].logits.view(np.uint32))
        for a, b in zip(r.tokens, out[0].tokens):
            np.testing.assert_array_equal(a, b)


def test_refusals_and_the_clamp_counter(tiny_models):
    cfg, w, _ = tiny_models["tiny-gqa"]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        Engine(cfg, max_batch=2, kv_cache_dtype="fp8_e5m2", **KW)
    odd = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, head_dim=64))
    with pytest.raises(KarantaHipError, match="head_dim of 128"):
        Engine(odd, max_batch=2, kv_cache_dtype="fp8_e4m3", **KW)
    eng = kv8_engine(cfg, w, scales=False)
    pages = ragged_pages(cfg, 2)
    eng.generate(pages, 4, ignore_eos=True)
    assert eng.kv_clamped == 0, "random-init K / V stay far inside +-448"
    nl = cfg.text.num_layers
    with pytest.raises(ValueError):
        eng.set_kv_scales(np.ones(nl + 1), np.ones(nl))
    eng.set_kv_scales(np.full(nl, 2.0 ** -12), np.ones((nl, cfg.text.num_kv_heads)))     # K far too fine: it clamps, and says so
    eng.generate(pages, 4, ignore_eos=True)
    assert eng.kv_clamped > 0
    eng.close()


# ----------------------------------------------------------------------------- against the fp32 oracle
def rel_errors(eng, cfg, w, page, n_new):
    """Teacher-forced on the fp32 oracle's tokens: (per-step max |logit error|, oracle tokens, oracle logits, the run)."""
    o_tok, o_log = O.generate_greedy(cfg, w, page.input_ids[None], page.pixel_values, page.grids, n_new, policy="fp32", ignore_eos=True,
                                     return_logits=True)
    run = eng.generate([page], n_new, ignore_eos=True, return_logits=True, force_tokens=o_tok[:, :n_new - 1])
    return np.abs(run.logits[0] - o_log[0]).max(-1), o_tok[0], o_log[0], run


@pytest.mark.parametrize("seed", ORACLE_SEEDS)
def test_fp8_cache_against_the_fp32_oracle(seed):
    """The bf16-cache and the fp8-cache engine (scales 1.0) on the same page, teacher-forced over 16 steps: the bf16 run within
    LOGIT_TOL_REL_FP32, the fp8 run within KV8_LOGIT_TOL_REL_FP32 (= LOGIT_TOL_REL; the measured figures stand at the constant), argmax equal wherever the oracle's
    margin exceeds TOKEN_MARGIN_FACTOR x the tolerance, and at least 12 of the 16 steps decisive at both tolerances."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg = CONFIGS["tiny-gqa"]
    w = random_weights(cfg, seed)
    page = ragged_pages(cfg, 1, seed=5)[0]
    n_new = 16
    figures = {}
    for kind in ("bf16", "fp8"):
        eng = Engine(cfg, max_batch=2, kv_cache_dtype="auto" if kind == "bf16" else "fp8", **KW)
        eng.load_weights(w)
        err, o_tok, o_log, run = rel_errors(eng, cfg, w, page, n_new)
        scale = float(np.abs(o_log[0]).max())
        figures[kind] = float(err.max()) / scale
        print(f"\nseed {seed} {kind} KV cache: relative logit error vs the fp32 oracle, worst of {n_new} steps = {figures[kind]:.5f} "
              f"(prefill step {err[0] / scale:.5f}, logit range {scale:.2f})")
        tol_rel = LOGIT_TOL_REL_FP32 if kind == "bf16" else KV8_LOGIT_TOL_REL_FP32
        tol = tol_rel * scale
        assert int((margins(o_log) > TOKEN_MARGIN_FACTOR * tol).sum()) >= 12
        # compare_teacher_forced allows 1.5 tol per step; the stated tolerance itself is asserted here
        assert err.max() < tol, f"{kind}: {figures[kind]:.5f} of the logit range (tolerance {tol_rel})"
        assert compare_teacher_forced(run.tokens[0], run.logits[0], o_tok, o_log, tol, f"seed {seed} {kind}") >= 12
        eng.close()
    assert figures["fp8"] > figures["bf16"], "the quantisation is in the path"
