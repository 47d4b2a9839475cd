"""End-to-end parity of the MI355X engine (ViT -> prefill -> greedy decode) against the oracle and
against the committed Hugging Face golden vectors, on the seeded tiny models.

Tolerance (stated): the engine computes bf16 storage / fp32 accumulate.  Against the
oracle run at the same dtype policy, last-position logits must agree within 2 % of the logit
range, and greedy tokens must be identical at every step whose oracle top-2 margin exceeds twice
that tolerance (below that margin an argmax flip is rounding noise, and the comparison stops at
the first such step because the sequences legitimately diverge).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd.engine import Engine, PageRequest  # noqa: E402
from karanta_ocr_amd.weights import bf16_round  # noqa: E402
from oracle import qwen2vl_oracle as O  # noqa: E402

MODELS = ["tiny", "tiny-gqa", "tiny-2.5"]


@pytest.fixture(scope="module")
def engines(tiny_models):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for name, (cfg, w, P) in tiny_models.items():
        e = Engine(cfg, max_batch=4, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
        e.load_weights(w)
        out[name] = e
    yield out
    for e in out.values():
        e.close()


def compare_tokens(got, ref_tokens, ref_logits, tol):
    """Token equality up to the first low-margin step."""
    n_checked = 0
    for i in range(min(len(got), len(ref_tokens))):
        top2 = np.sort(ref_logits[i])[-2:]
        if top2[1] - top2[0] <= 2 * tol:
            break
        assert got[i] == ref_tokens[i], f"step {i}: engine {got[i]} vs oracle {ref_tokens[i]} (margin {top2[1]-top2[0]:.3f})"
        n_checked += 1
    return n_checked


@pytest.mark.parametrize("name", MODELS)
def test_vit_matches_oracle_and_hf(engines, golden, tiny_models, name):
    cfg, w, P = tiny_models[name]
    eng = engines[name]
    pv, grid = golden[P + "vit_pixel_values"], [tuple(int(x) for x in g) for g in golden[P + "vit_grid"]]
    got = eng.vit_forward(pv, grid)
    eng.stream.synchronize()
    got = got.float().cpu().numpy()
    ref_bf = O.vit_forward(pv, grid, w, cfg.vision, policy="bf16")
    ref_hf = golden[P + "vit_merged"]
    scale = np.abs(ref_hf).max()
    assert np.abs(got - ref_bf).max() < 0.02 * scale, np.abs(got - ref_bf).max()
    assert np.abs(got - ref_hf).max() < 0.03 * scale, np.abs(got - ref_hf).max()


@pytest.mark.parametrize("name", MODELS)
def test_generate_matches_oracle_and_hf(engines, golden, tiny_models, name):
    cfg, w, P = tiny_models[name]
    eng = engines[name]
    ids = golden[P + "e2e_input_ids"][0]
    pv, grid = golden[P + "e2e_pixel_values"], [tuple(int(x) for x in golden[P + "e2e_grid"][0])]
    n_new = golden[P + "e2e_gen_ids"].shape[1]
    page = PageRequest(input_ids=ids, pixel_values=pv, grids=grid)
    res = eng.generate([page], n_new, ignore_eos=True, return_logits=True)
    # oracle at the engine's dtype policy
    o_tok, o_log = O.generate_greedy(cfg, w, ids[None], pv, grid, n_new, policy="bf16", ignore_eos=True, return_logits=True)
    tol = 0.02 * np.abs(o_log[0, 0]).max()
    assert np.abs(res.logits[0, 0] - o_log[0, 0]).max() < tol, "prefill logits vs bf16-policy oracle"
    assert np.abs(res.logits[0, 0] - golden[P + "e2e_prompt_logits"][-1]).max() < 1.5 * tol, "prefill logits vs HF fp32"
    n1 = compare_tokens(res.tokens[0], o_tok[0], o_log[0], tol)
    n2 = compare_tokens(res.tokens[0], golden[P + "e2e_gen_ids"][0], golden[P + "e2e_gen_scores"], tol)
    # decode-step logits stay within tolerance for as long as the sequences agree
    for i in range(1, n1):
        assert np.abs(res.logits[0, i] - o_log[0, i]).max() < 1.5 * tol, f"decode step {i}"
    # A free run can only be compared up to its first near-tie (these random-init toys can start with one), so the
    # MINIMUM COUNT is asserted on a teacher-forced run: the engine is fed the oracle's tokens, every one of the 16
    # steps compares (logits within 1.5 tol, argmax equal wherever the oracle's margin exceeds 2 tol) and at least 10
    # of them must be decisive (12 / 16 / 11 by the committed goldens' margins).  Same against HF's own fp32 run.
    from tests.prodwidth import compare_teacher_forced
    forced = eng.generate([page], n_new, ignore_eos=True, return_logits=True, force_tokens=o_tok[:, :n_new - 1])
    n_dec = compare_teacher_forced(forced.tokens[0], forced.logits[0], o_tok[0], o_log[0], tol, f"{name} forced")
    assert n_dec >= 10, f"only {n_dec} decisive steps of {n_new}"
    hf_ids, hf_scores = golden[P + "e2e_gen_ids"], golden[P + "e2e_gen_scores"]
    forced_hf = eng.generate([page], n_new, ignore_eos=True, return_logits=True, force_tokens=hf_ids[:, :n_new - 1])
    n_hf = compare_teacher_forced(forced_hf.tokens[0], forced_hf.logits[0], hf_ids[0], hf_scores, tol, f"{name} forced, HF fp32")   # 1.5 tol = the stated 3 % vs HF fp32
    assert n_hf >= 8, f"only {n_hf} decisive steps of {n_new} against the HF fp32 golden"
    # the graph-replayed decode loop produces the same tokens as the eager loop
    res_g = eng.generate([page], n_new, ignore_eos=True, use_graph=True)
    np.testing.assert_array_equal(res_g.tokens[0], res.tokens[0])
    assert res_g.finish_reasons == ["length"]


@pytest.mark.parametrize("name", MODELS)
def test_batched_pages_are_independent(engines, tiny_models, name):
    """Ragged batch (different image sizes and prompt lengths): every page's tokens equal the
    tokens it gets when run alone — pages share nothing but the launch."""
    cfg, w, P = tiny_models[name]
    eng = engines[name]
    rng = np.random.default_rng(99)
    pages = []
    for i, (h, wd, npre) in enumerate([(112, 168, 4), (56, 84, 9), (140, 140, 2)]):
        pv, grid = IP.image_to_patches(IP.synthetic_page(i, h, wd))
        T = grid[1] * grid[2] // 4
        ids = np.concatenate([rng.integers(0, 400, npre), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                              [cfg.vision_end_token_id], rng.integers(0, 400, 5)]).astype(np.int64)
        pages.append(PageRequest(ids, pv, [grid]))
    together = eng.generate(pages, 12, ignore_eos=True)
    for i, pg in enumerate(pages):
        alone = eng.generate([pg], 12, ignore_eos=True)
        np.testing.assert_array_equal(alone.tokens[0], together.tokens[i])
    assert together.prompt_tokens == [len(p.input_ids) for p in pages]


def test_eos_stops_and_pads(engines, tiny_models):
    """Make the first generated token an EOS by construction: finish_reason 'stop', one token."""
    cfg, w, P = tiny_models["tiny"]
    eng = engines["tiny"]
    pv, grid = IP.image_to_patches(IP.synthetic_page(5, 56, 56))
    ids = np.concatenate([[1, 2, cfg.vision_start_token_id], [cfg.image_token_id] * 4, [cfg.vision_end_token_id, 3]]).astype(np.int64)
    free = eng.generate([PageRequest(ids, pv, [grid])], 6, ignore_eos=True)
    first = int(free.tokens[0][0])
    import dataclasses
    eng2 = Engine(dataclasses.replace(cfg, eos_token_ids=(first, 496)), max_batch=2, s_max=256, max_patches=256,
                  max_prompt_tokens=256, decode_splits=2)
    eng2.load_weights(w)
    res = eng2.generate([PageRequest(ids, pv, [grid])], 6)
    assert res.finish_reasons == ["stop"] and res.tokens[0].tolist() == [first]
    eng2.close()


def test_image_token_mismatch_is_an_error(engines, tiny_models):
    cfg, w, P = tiny_models["tiny"]
    eng = engines["tiny"]
    pv, grid = IP.image_to_patches(IP.synthetic_page(5, 56, 56))
    ids = np.asarray([1, cfg.image_token_id, cfg.image_token_id, 2], np.int64)  # needs 4 placeholders
    with pytest.raises(ValueError, match="do not match"):
        eng.generate([PageRequest(ids, pv, [grid])], 2)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True, "cu-mask"])
@pytest.mark.parametrize("name", MODELS)
def test_slot_scheduler_equals_solo_generation(engines, tiny_models, name, overlap):
    """Continuous batching: 7 ragged requests through 3 slots (2 of the engine's 4 stay idle throughout) — every
    request's tokens equal the ones it gets alone from `generate`, whichever slot it lands in, whatever its slot
    held before and whatever its neighbours are doing; EOS (made frequent by construction) and length limits both
    free slots mid-flight."""
    import dataclasses
    from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
    cfg, w, P = tiny_models[name]
    base = engines[name]
    rng = np.random.default_rng(123)
    pages, limits = [], [9, 20, 5, 14, 1, 17, 11]
    for i, mt in enumerate(limits):
        h, wd = [(112, 168), (56, 84), (140, 140), (56, 56)][i % 4]
        pv, grid = IP.image_to_patches(IP.synthetic_page(20 + i, h, wd))
        T = grid[1] * grid[2] // 4
        ids = np.concatenate([rng.integers(0, 400, 2 + i), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                              [cfg.vision_end_token_id], rng.integers(0, 400, 3)]).astype(np.int64)
        pages.append(PageRequest(ids, pv, [grid]))
    free = [base.generate([pg], 20, ignore_eos=True).tokens[0] for pg in pages]
    # an EOS set that some of the free-running sequences hit early, some late, some never
    eos = (int(free[0][4]), int(free[3][9]), int(free[5][2]))
    cfg2 = dataclasses.replace(cfg, eos_token_ids=eos)
    # "cu-mask": the admission stream is restricted to 192 compute units (kr_stream_create_cu_mask): the serving path's form
    eng = Engine(cfg2, max_batch=3, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2,
                 admission_cus=192 if overlap == "cu-mask" else None)
    eng.load_weights(w)
    solo = [eng.generate([pg], mt) for pg, mt in zip(pages, limits)]
    # overlap: ViT + prefill of an admission on a second stream while the other slots keep decoding (target slots
    # parked on the last cache row meanwhile)
    sch = SlotScheduler(eng, max_tokens_cap=20, chunk=3, overlap=bool(overlap))
    assert sch.overlap == bool(overlap)
    res = sch.run([SlotRequest(pg, mt, tag=i) for i, (pg, mt) in enumerate(zip(pages, limits))])
    assert [r.tag for r in res] == list(range(len(pages)))
    reasons = set()
    for r, s, pg in zip(res, solo, pages):
        assert r.error is None and r.prompt_tokens == len(pg.input_ids)
        np.testing.assert_array_equal(r.tokens, s.tokens[0])
        assert r.finish_reason == s.finish_reasons[0]
        reasons.add(r.finish_reason)
    assert reasons == {"stop", "length"}, "the construction should exercise both ways out of a slot"
    assert sch.steps > 0 and sch.slot_steps_busy <= sch.steps * 3
    if overlap == "cu-mask":
        assert eng._adm_stream_handle is not None, "the admissions ran on the CU-masked stream"
    # static generate() still works on the same engine afterwards (leaves slot mode)
    again = eng.generate([pages[1]], limits[1])
    np.testing.assert_array_equal(again.tokens[0], solo[1].tokens[0])
    eng.close()


@pytest.mark.gpu
def test_server_continuous_mode_end_to_end(engines, tiny_models):
    """OpenAI-shaped requests through LocalServer(continuous=True) on the real engine: concurrent callers, ragged
    images and limits; every completion equals the one the static server gives for the same request."""
    import threading
    from karanta_ocr_amd import serving as S
    cfg, w, P = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=2, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
    eng.load_weights(w)
    front = S.ChatFrontend(cfg, S.ByteTokenizer(cfg))
    def request(i):
        h, wd = [(56, 84), (112, 112), (84, 56)][i % 3]
        url = IP.encode_png_data_url(IP.synthetic_page(40 + i, h, wd))
        return {"model": "karantaocr", "max_tokens": [6, 15, 3, 11, 9][i], "temperature": 0.0,
                "messages": [{"role": "user", "content": [{"type": "text", "text": f"page {i}"},
                                                          {"type": "image_url", "image_url": {"url": url}}]}]}
    static = S.LocalServer(eng, front, log=lambda *_: None)
    want = [static.chat_completions(request(i)) for i in range(5)]
    static.close()
    logs = []
    srv = S.LocalServer(eng, front, log=logs.append, continuous=True, max_tokens_cap=16, chunk=2)
    got = [None] * 5
    ts = [threading.Thread(target=lambda i=i: got.__setitem__(i, srv.chat_completions(request(i)))) for i in range(5)]
    [t.start() for t in ts]; [t.join() for t in ts]
    srv.close()
    for (ws, wb), (gs, gb) in zip(want, got):
        assert ws == gs == 200
        assert gb["choices"][0]["message"]["content"] == wb["choices"][0]["message"]["content"]
        assert gb["choices"][0]["finish_reason"] == wb["choices"][0]["finish_reason"]
        assert gb["usage"] == wb["usage"]
    assert any("Running:" in l for l in logs) and srv.pages_done == 5
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_sampled_generation_matches_oracle(engines, tiny_models, name):
    """temperature > 0: the engine's tokens equal the oracle's Gumbel-max draws (same counter-based noise) up to the
    first step whose top-2 noisy scores are closer than the logit tolerance; a batch mixes sampled pages, another
    seed and a greedy page; the same seed reproduces, another seed differs."""
    import dataclasses
    cfg, w, P = tiny_models[name]
    eng = engines[name]
    pv, grid = IP.image_to_patches(IP.synthetic_page(3, 84, 112))
    T = grid[1] * grid[2] // 4
    ids = np.concatenate([[5, 6, cfg.vision_start_token_id], [cfg.image_token_id] * T, [cfg.vision_end_token_id, 7, 8]]).astype(np.int64)
    _, lg0 = O.generate_greedy(cfg, w, ids[None], pv, [grid], 1, policy="bf16", ignore_eos=True, return_logits=True)
    # hot enough that the noise decides: the tied-embedding model's logits are an order of magnitude larger
    temp, steps = max(0.9, 0.3 * float(np.abs(lg0[0, 0]).max())), 14
    pages = [PageRequest(ids, pv, [grid], temperature=temp, seed=4242), PageRequest(ids, pv, [grid], temperature=temp, seed=4243),
             PageRequest(ids, pv, [grid])]
    res = eng.generate(pages, steps, ignore_eos=True)
    again = eng.generate(pages[:1], steps, ignore_eos=True)
    np.testing.assert_array_equal(res.tokens[0], again.tokens[0])                  # reproducible, batch-independent
    assert not np.array_equal(res.tokens[0], res.tokens[1])                        # another seed, another draw
    greedy = eng.generate([PageRequest(ids, pv, [grid])], steps, ignore_eos=True)
    np.testing.assert_array_equal(res.tokens[2], greedy.tokens[0])                 # T = 0 row of a sampling batch
    assert not np.array_equal(res.tokens[0], greedy.tokens[0])
    tol = 0.02 * float(np.abs(lg0[0, 0]).max()) / temp        # the logit tolerance of the greedy tests, scaled by 1 / T
    for k, seed in ((0, 4242), (1, 4243)):
        ref_tok, ref_sc = O.generate_greedy(cfg, w, ids[None], pv, [grid], steps, policy="bf16", ignore_eos=True,
                                            return_logits=True, temperature=temp, seed=seed)
        n = compare_tokens(res.tokens[k], ref_tok[0], ref_sc[0], tol)
        assert n >= 3, f"only {n} sampled tokens could be checked"


@pytest.mark.gpu
def test_gpu_image_front_end_end_to_end(engines, tiny_models):
    """Pages handed over as uint8 images (GPU resize / normalise / patchify) give the pixel_values and the tokens of
    the host PIL path, exactly; grids are checked against the prompt's."""
    cfg, w, P = tiny_models["tiny"]
    eng = engines["tiny"]
    imgs = [IP.synthetic_page(60, 100, 150), IP.synthetic_page(61, 56, 84), IP.synthetic_page(62, 131, 97)]
    pages_host, pages_dev = [], []
    for im in imgs:
        pv, grid = IP.image_to_patches(im, max_pixels=28 * 28 * 12)      # forces a down-scale on the larger pages
        T = grid[1] * grid[2] // 4
        ids = np.concatenate([[9, cfg.vision_start_token_id], [cfg.image_token_id] * T, [cfg.vision_end_token_id, 3]]).astype(np.int64)
        pages_host.append(PageRequest(ids, pv, [grid]))
        pages_dev.append(PageRequest(ids, None, [grid], images=[im]))
    pix, grids = eng.patches_from_images(imgs, max_pixels=28 * 28 * 12)
    assert grids == [p.grids[0] for p in pages_host]
    np.testing.assert_array_equal(pix.cpu().numpy(), np.concatenate([p.pixel_values for p in pages_host], 0))
    a = eng.generate(pages_host, 8, ignore_eos=True)
    b = eng.generate(pages_dev, 8, ignore_eos=True)          # sizes come from the pages' grids
    for x, y in zip(a.tokens, b.tokens):
        np.testing.assert_array_equal(x, y)
    from karanta_ocr_amd._lib import KarantaHipError
    with pytest.raises(KarantaHipError, match="images but"):
        eng.generate([PageRequest(pages_dev[0].input_ids, None, pages_dev[0].grids, images=[imgs[0], imgs[1]])], 2)


@pytest.mark.gpu
def test_fp8_weight_engine_matches_oracle_on_dequantised_weights():
    """weight_dtype="fp8" (BASELINE.json config 5): decode streams e4m3fn codes + per-row scales, prefill reads their
    dequantised bf16 copy.  Reference: the oracle on the state dict with every decoder Linear replaced by
    scale * e4m3(codes) — the same model, so the usual logit tolerance and token rule apply; the fp8 engine differs
    from the bf16 engine (the quantisation is really in the path), and half the decode bytes are gone."""
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.weights import fp8_dequantized_weights, random_weights
    cfg = CONFIGS["tiny-w512"]
    w = random_weights(cfg, 808)
    pv, grid = IP.image_to_patches(IP.synthetic_page(70, 84, 112))
    T = grid[1] * grid[2] // 4
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.integers(0, 400, 5), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                          [cfg.vision_end_token_id], rng.integers(0, 400, 4)]).astype(np.int64)
    page = PageRequest(ids, pv, [grid])
    n_new = 12
    eng8 = Engine(cfg, max_batch=2, s_max=512, max_patches=1024, max_prompt_tokens=1024, decode_splits=2, weight_dtype="fp8")
    eng8.load_weights(w)
    assert eng8.fp8 and eng8.wide_mode and eng8.narrow_mode
    res = eng8.generate([page], n_new, ignore_eos=True, return_logits=True)
    wq = fp8_dequantized_weights(w, cfg)
    o_tok, o_log = O.generate_greedy(cfg, wq, ids[None], pv, [grid], n_new, policy="bf16", ignore_eos=True, return_logits=True)
    tol = 0.02 * np.abs(o_log[0, 0]).max()
    assert np.abs(res.logits[0, 0] - o_log[0, 0]).max() < tol, "prefill logits vs the oracle on dequantised weights"
    n1 = compare_tokens(res.tokens[0], o_tok[0], o_log[0], tol)
    for i in range(1, n1):
        assert np.abs(res.logits[0, i] - o_log[0, i]).max() < 1.5 * tol, f"decode step {i}"
    # graph replay and a batch of two agree with the eager single run
    g = eng8.generate([page, page], n_new, ignore_eos=True)
    np.testing.assert_array_equal(g.tokens[0], res.tokens[0]); np.testing.assert_array_equal(g.tokens[1], res.tokens[0])
    # the quantisation is really there: the bf16 engine on the original weights gives other logits
    eng16 = Engine(cfg, max_batch=2, s_max=512, max_patches=1024, max_prompt_tokens=1024, decode_splits=2)
    eng16.load_weights(w)
    r16 = eng16.generate([page], 2, ignore_eos=True, return_logits=True)
    assert np.abs(r16.logits[0, 0] - res.logits[0, 0]).max() > 1e-3
    assert cfg.decoder_weight_bytes("fp8") < 0.75 * cfg.decoder_weight_bytes()
    eng8.close(); eng16.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny-w512", "tiny-w3584", "tiny-w512+resnorm", "tiny-w3584+fp8"])
def test_batches_above_16_rows_equal_solo_generation(name):
    """max_batch up to 32: 21 ragged pages decoded together give each page the tokens it gets alone; the slot scheduler
    runs 20 slots.  tiny-w512: two 16-row column tiles per weight fragment, all x rows in LDS (hidden_size <= 2048).
    tiny-w3584 (the 7B decoder width, BASELINE config 3's 32-rows-per-GPU variant): 32 x rows of 3584 do not fit the LDS,
    gate/up and lm_head stage K in two halves (dec_wide_kh_kernel), the qkv launch runs once per 16-row range, o_proj /
    down_proj on two column tiles; round 3: there the residual sum + RMSNorm run once (kr_decode_resnorm) and ONE direct qkv
    launch covers all rows.  "+resnorm": that two-launch form forced on at the width where the fused launch is the default
    (round 3's sequence: csrc/tools/experiment_engine.ExperimentEngine on the product library, no experiment mode).  The other
    three cases run the product engine, whose > 16-row steps are the packed family (kr_decode_resnorm32 + kr_linear_decode32)."""
    from karanta_ocr_amd._lib import KarantaHipError
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
    from karanta_ocr_amd.weights import random_weights
    weight_dtype = "bf16"
    if name.endswith("+fp8"):          # fp8 weights through the same >16-row launches (direct qkv on e4m3 codes)
        name, weight_dtype = name[:-len("+fp8")], "fp8"
    engine_cls, want_resnorm = Engine, name == "tiny-w3584"
    if name.endswith("+resnorm"):
        from karanta_ocr_amd.csrc.tools.experiment_engine import ExperimentEngine
        name, engine_cls, want_resnorm = name[:-len("+resnorm")], ExperimentEngine, True
    cfg = CONFIGS[name]
    w = random_weights(cfg, 909)
    eng = engine_cls(cfg, max_batch=21, s_max=512, max_patches=4096, max_prompt_tokens=4096, decode_splits=2, weight_dtype=weight_dtype)
    if engine_cls is not Engine:
        eng.resnorm_qkv = True
        assert not (eng.family32 or eng.fast_residual or eng.attn_fused_merge or eng.merge_in_o_proj or eng._prefetch_mode)
    eng.load_weights(w)
    if weight_dtype == "fp8":
        from karanta_ocr_amd.weights import fp8_dequantized_weights
        w = fp8_dequantized_weights(w, cfg)      # what the oracle comparison below runs on
    assert eng.row_split == (name == "tiny-w3584") and eng.defer_down == (name == "tiny-w3584") and eng.resnorm_qkv == want_resnorm
    rng = np.random.default_rng(77)
    pages = []
    for i in range(21):
        h, wd = [(56, 84), (84, 56), (56, 56), (112, 84)][i % 4]
        pv, grid = IP.image_to_patches(IP.synthetic_page(100 + i, h, wd))
        T = grid[1] * grid[2] // 4
        ids = np.concatenate([rng.integers(0, 400, 1 + i % 5), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                              [cfg.vision_end_token_id], rng.integers(0, 400, 2)]).astype(np.int64)
        pages.append(PageRequest(ids, pv, [grid]))
    together = eng.generate(pages, 10, ignore_eos=True)
    for i in (0, 7, 15, 16, 17, 20):
        alone = eng.generate([pages[i]], 10, ignore_eos=True)
        np.testing.assert_array_equal(alone.tokens[0], together.tokens[i])
    # a page of the SECOND 16-row range against the oracle, teacher-forced inside the full batch (rows 16 .. 20 go through
    # the second pass of every x-staging launch)
    from tests.prodwidth import compare_teacher_forced
    k = 17
    o_tok, o_log = O.generate_greedy(cfg, w, pages[k].input_ids[None], pages[k].pixel_values, pages[k].grids, 10, policy="bf16",
                                     ignore_eos=True, return_logits=True)
    ft = np.stack([np.asarray(t[:9], np.int64) for t in together.tokens])
    ft[k] = o_tok[0, :9]
    forced = eng.generate(pages, 10, ignore_eos=True, return_logits=True, force_tokens=ft)
    tol = 0.02 * float(np.abs(o_log[0, 0]).max())
    n_dec = compare_teacher_forced(forced.tokens[k], forced.logits[k], o_tok[0], o_log[0], tol, f"{name} row {k} of 21")
    assert n_dec >= 3, f"only {n_dec} decisive steps"
    sch = SlotScheduler(eng, max_tokens_cap=10, chunk=3)
    res = sch.run([SlotRequest(p, 4 + i % 7, tag=i) for i, p in enumerate(pages)])
    for i in (0, 3, 8, 16, 19, 20):        # EOS-aware solo runs (the tiny vocabulary hits an EOS id now and then)
        solo = eng.generate([pages[i]], 4 + i % 7)
        np.testing.assert_array_equal(res[i].tokens, solo.tokens[0])
        assert res[i].finish_reason == solo.finish_reasons[0]
    eng.close()
    with pytest.raises(KarantaHipError, match="max_batch > 16"):
        Engine(CONFIGS["tiny"], max_batch=17, s_max=256, max_patches=256, max_prompt_tokens=256)   # hidden 256: no wide kernel
    with pytest.raises(KarantaHipError, match="max_batch > 32"):
        Engine(cfg, max_batch=33, s_max=256, max_patches=256, max_prompt_tokens=256)


GUIDE_PATTERN = r"[a-f]{3}-[0-9]{2}(?:;[a-z ]{2,5})?"


def _guided_pages(cfg, temp):
    pv, grid = IP.image_to_patches(IP.synthetic_page(71, 84, 112))
    T = grid[1] * grid[2] // 4
    ids = np.concatenate([[5, 6, cfg.vision_start_token_id], [cfg.image_token_id] * T, [cfg.vision_end_token_id, 7, 8]]).astype(np.int64)
    pv2, grid2 = IP.image_to_patches(IP.synthetic_page(72, 56, 84))
    ids2 = np.concatenate([[9, cfg.vision_start_token_id], [cfg.image_token_id] * (grid2[1] * grid2[2] // 4),
                           [cfg.vision_end_token_id, 3]]).astype(np.int64)
    return (ids, pv, grid), (ids2, pv2, grid2), temp


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "tiny-gqa"])
def test_guided_generation_and_logprobs_match_oracle(engines, tiny_models, name):
    """guided_regex (karanta/pipeline.py:304-307) and logprobs / top_logprobs on the device: guided rows (greedy and
    sampled) produce text that matches the pattern and stop by themselves, and equal the oracle's masked argmax up to
    the first low-margin step; an unguided row of the same batch is untouched; log-probabilities equal the log-softmax
    of the engine's own logits (ids exact) and the oracle's within the logit tolerance."""
    import re
    from karanta_ocr_amd import guided as G
    from karanta_ocr_amd.serving import ByteTokenizer
    cfg, w, P = tiny_models[name]
    eng = engines[name]
    voc = ByteTokenizer(cfg).token_bytes()
    eng.set_vocab(voc)
    g = G.compile_regex(GUIDE_PATTERN)
    (ids, pv, grid), (ids2, pv2, grid2), _ = _guided_pages(cfg, 0)
    _, lg0 = O.generate_greedy(cfg, w, ids[None], pv, [grid], 1, policy="bf16", ignore_eos=True, return_logits=True)
    rng_ = float(np.abs(lg0[0, 0]).max())
    temp = max(0.9, 0.3 * rng_)
    pages = [PageRequest(ids, pv, [grid], guide=g, logprobs=3),
             PageRequest(ids, pv, [grid], guide=GUIDE_PATTERN, temperature=temp, seed=77),
             PageRequest(ids2, pv2, [grid2], logprobs=5),
             PageRequest(ids2, pv2, [grid2], guide=g)]
    steps = 16
    res = eng.generate(pages, steps)
    eos = set(cfg.eos_token_ids)
    for b in (0, 1, 3):
        toks = res.tokens[b]
        assert res.finish_reasons[b] == "stop" and int(toks[-1]) in eos, (b, toks)
        text = b"".join(voc[int(t)] for t in toks[:-1]).decode()
        assert re.fullmatch(GUIDE_PATTERN, text), (b, text)
    plain = eng.generate([PageRequest(ids2, pv2, [grid2])], steps)
    np.testing.assert_array_equal(res.tokens[2], plain.tokens[0])                   # unguided row of a guided batch
    assert res.logprobs[1] is None and res.logprobs[3] is None
    # oracle: masked argmax with the same DFA (as data), greedy and sampled
    tol = 0.02 * rng_
    for b, (i_, p_, g_), T_, seed in ((0, (ids, pv, grid), 0.0, 0), (1, (ids, pv, grid), temp, 77), (3, (ids2, pv2, grid2), 0.0, 0)):
        ref_tok, ref_sc = O.generate_greedy(cfg, w, i_[None], p_, [g_], steps, policy="bf16", return_logits=True, temperature=T_,
                                            seed=seed, guide=(g.trans, g.accept, g.start), token_bytes=voc)
        n = compare_tokens(res.tokens[b], ref_tok[0], ref_sc[0], tol / (T_ if T_ > 0 else 1.0))
        assert n >= 2, f"row {b}: only {n} guided tokens could be checked"
    # log-probabilities against the engine's own logits (eager run returning them) and against the oracle model
    eager = eng.generate(pages, steps, return_logits=True)
    for b, k in ((0, 3), (2, 5)):
        np.testing.assert_array_equal(eager.tokens[b], res.tokens[b])
        lp = res.logprobs[b]
        n = len(res.tokens[b]) - (1 if res.finish_reasons[b] == "stop" else 0)
        assert lp["token"].shape == (n,) and lp["top"].shape == (n, k) and lp["top_ids"].shape == (n, k)
        for i in range(n):
            ids_, vals = O.top_logprobs(eager.logits[b, i], k)
            np.testing.assert_array_equal(lp["top_ids"][i], ids_)
            np.testing.assert_allclose(lp["top"][i], vals, rtol=1e-5, atol=1e-4)
            np.testing.assert_allclose(lp["token"][i], O.log_softmax(eager.logits[b, i])[int(res.tokens[b][i])], rtol=1e-5, atol=1e-4)
            np.testing.assert_array_equal(eager.logprobs[b]["top_ids"][i], ids_)
    ref_tok, _, raw = O.generate_greedy(cfg, w, ids2[None], pv2, [grid2], steps, policy="bf16", return_raw_logits=True)
    m = 0
    while m < min(len(ref_tok[0]), len(res.tokens[2])) and ref_tok[0][m] == res.tokens[2][m]:
        m += 1
    m = min(m + 1, len(res.logprobs[2]["token"]))        # the logits of the first differing step still share their prefix
    assert m >= 3
    for i in range(m):
        want = O.log_softmax(raw[0, i])[int(res.tokens[2][i])]
        assert abs(res.logprobs[2]["token"][i] - want) <= 2 * tol, (i, res.logprobs[2]["token"][i], want)
    # errors: a guide without the vocabulary table, logprobs out of range
    from karanta_ocr_amd._lib import KarantaHipError
    with pytest.raises(KarantaHipError, match="0..20"):
        eng.generate([PageRequest(ids, pv, [grid], logprobs=21)], 2)
    eng.sampler.d_voc_off = None
    eng.sampler._guides.clear()
    with pytest.raises(KarantaHipError, match="set_vocab"):
        eng.generate([PageRequest(ids, pv, [grid], guide=r"zz+")], 2)
    eng.set_vocab(voc)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True])
def test_slot_scheduler_guided_and_logprobs_equal_solo(engines, tiny_models, overlap):
    """Continuous batching with guides and log-probabilities: patterns, DFA states and log-prob histories are per slot
    and reset on admission — every request equals its solo `generate`, whatever held its slot before.  overlap: the
    admissions run beside the decode chunks, and a guided one's first token keeps its guided pass."""
    from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
    from karanta_ocr_amd.serving import ByteTokenizer
    cfg, w, P = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=2, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
    eng.load_weights(w)
    voc = ByteTokenizer(cfg).token_bytes()
    eng.set_vocab(voc)
    (ids, pv, grid), (ids2, pv2, grid2), _ = _guided_pages(cfg, 0)
    pats = [GUIDE_PATTERN, None, r"(?:yes|no)\n", r"\{\"ok\": (?:true|false)\}", None, GUIDE_PATTERN]
    pages = []
    for i, pat in enumerate(pats):
        src = (ids, pv, grid) if i % 2 == 0 else (ids2, pv2, grid2)
        pages.append(PageRequest(src[0], src[1], [src[2]], guide=pat, logprobs=(4 if i in (0, 1, 3) else None),
                                 temperature=(0.8 if i == 5 else 0.0), seed=5))
    limits = [16, 7, 16, 16, 5, 16]
    solo = [eng.generate([pg], mt) for pg, mt in zip(pages, limits)]
    sch = SlotScheduler(eng, max_tokens_cap=16, chunk=3, sampling=True, guided=True, logprobs=4, overlap=overlap)
    res = sch.run([SlotRequest(pg, mt, tag=i) for i, (pg, mt) in enumerate(zip(pages, limits))])
    for i, (r, s) in enumerate(zip(res, solo)):
        assert r.error is None
        np.testing.assert_array_equal(r.tokens, s.tokens[0], err_msg=f"request {i}")
        assert r.finish_reason == s.finish_reasons[0]
        if pages[i].logprobs is None:
            assert r.logprobs is None
        else:
            for key in ("token", "top", "top_ids"):
                np.testing.assert_array_equal(r.logprobs[key], s.logprobs[0][key], err_msg=f"request {i} {key}")
    assert {r.finish_reason for r in res} == {"stop", "length"}
    assert b"".join(voc[int(t)] for t in res[2].tokens[:-1]) in (b"yes\n", b"no\n")
    eng.close()


@pytest.mark.gpu
def test_server_guided_json_and_logprobs(engines, tiny_models):
    """The OpenAI surface: response_format json_schema -> parseable JSON of the schema's shape, guided_regex -> a match,
    logprobs -> the `choices[0].logprobs.content` list; static and continuous servers agree."""
    import json
    import re
    from karanta_ocr_amd import serving as S
    cfg, w, P = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=2, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
    eng.load_weights(w)
    front = S.ChatFrontend(cfg, S.ByteTokenizer(cfg))
    url = IP.encode_png_data_url(IP.synthetic_page(44, 56, 84))
    msg = [{"role": "user", "content": [{"type": "text", "text": "page"}, {"type": "image_url", "image_url": {"url": url}}]}]
    schema = {"type": "object", "properties": {"lang": {"type": ["string", "null"], "maxLength": 3}, "rot": {"enum": [0, 90]},
                                               "tab": {"type": "boolean"}}, "required": ["lang", "rot", "tab"]}
    reqs = [{"messages": msg, "max_tokens": 80, "temperature": 0.0,
             "response_format": {"type": "json_schema", "json_schema": {"name": "p", "schema": schema, "strict": True}}},
            {"messages": msg, "max_tokens": 30, "temperature": 0.0, "guided_regex": r"lang: (?:[a-z]{2}|null)\nrot: (?:0|90)\n",
             "logprobs": True, "top_logprobs": 2},
            {"messages": msg, "max_tokens": 4, "logprobs": True}]
    out = {}
    for mode in ("static", "continuous"):
        srv = S.LocalServer(eng, front, log=lambda *_: None, continuous=(mode == "continuous"), max_tokens_cap=96, chunk=4,
                            max_logprobs=5)
        out[mode] = [srv.chat_completions(r) for r in reqs]
        if mode == "continuous":
            st, body = srv.chat_completions({**reqs[2], "top_logprobs": 9})
            assert st == 400 and "max-logprobs" in body["error"]["message"]
        st, body = srv.chat_completions({**reqs[1], "guided_regex": "(?=x)y"})
        assert st == 400 and "guided decoding" in body["error"]["message"]
        srv.close()
    for (s0, b0), (s1, b1) in zip(out["static"], out["continuous"]):
        assert s0 == s1 == 200
        assert b0["choices"][0]["message"]["content"] == b1["choices"][0]["message"]["content"]
        assert b0["choices"][0]["finish_reason"] == b1["choices"][0]["finish_reason"]
        assert b0["choices"][0].get("logprobs") == b1["choices"][0].get("logprobs")
    doc = json.loads(out["static"][0][1]["choices"][0]["message"]["content"])
    assert list(doc) == ["lang", "rot", "tab"] and doc["rot"] in (0, 90) and isinstance(doc["tab"], bool)
    assert out["static"][0][1]["choices"][0]["finish_reason"] == "stop"
    c1 = out["static"][1][1]["choices"][0]
    assert re.fullmatch(reqs[1]["guided_regex"], c1["message"]["content"]) and c1["finish_reason"] == "stop"
    items = c1["logprobs"]["content"]
    assert "".join(i["token"] for i in items) == c1["message"]["content"]
    assert all(len(i["top_logprobs"]) == 2 and i["logprob"] <= 0 and i["top_logprobs"][0]["logprob"] >= i["top_logprobs"][1]["logprob"]
               for i in items)
    c2 = out["static"][2][1]["choices"][0]
    assert len(c2["logprobs"]["content"]) == 4 and all(i["top_logprobs"] == [] for i in c2["logprobs"]["content"])
    eng.close()


@pytest.mark.gpu
def test_disjoint_decode_stream_follows_the_admission_in_flight(tiny_models):
    """while an overlapped admission is in flight on its CU-masked stream the decode graph replays on the complementary
    compute units; after admit_end — or after begin_slots() of a scheduler rebuilt with an admission still in flight — it is back
    on the engine's stream (the counter used to stay above zero for ever: ~47 % decode speed with nothing reporting it)."""
    cfg, w, _ = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=3, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2, admission_cus=128)
    eng.load_weights(w)
    def page(i, h, wd):
        pv, grid = IP.image_to_patches(IP.synthetic_page(60 + i, h, wd))
        T = grid[1] * grid[2] // 4
        ids = np.concatenate([[3 + i, cfg.vision_start_token_id], [cfg.image_token_id] * T, [cfg.vision_end_token_id, 9]]).astype(np.int64)
        return PageRequest(ids, pv, [grid])
    solo = eng.generate([page(0, 56, 84)], 8).tokens[0]      # EOS-aware, as a slot decodes
    k = min(len(solo), 6)
    eng.begin_slots(16)
    eng.admit([page(0, 56, 84)], [0])
    eng.decode_steps(2)                         # first step eager, then the captured graph
    assert eng.last_decode_disjoint is False
    h = eng.admit_begin([page(1, 84, 56)], [1])
    assert eng._adm_inflight == 1
    eng.decode_steps(2)
    assert eng.last_decode_disjoint is True and eng._dec_stream is not None
    eng.admit_end(h)
    eng.decode_steps(2)
    assert eng.last_decode_disjoint is False and eng._adm_inflight == 0
    eng.stream.synchronize()
    np.testing.assert_array_equal(eng.slot_tokens(0, k), solo[:k])      # slot 0 decoded through both paths: the same tokens
    h2 = eng.admit_begin([page(2, 56, 56)], [2])                        # ... and a scheduler rebuilt with this one still in flight
    assert eng._adm_inflight == 1
    eng.begin_slots(16)
    assert eng._adm_inflight == 0
    eng.admit([page(0, 56, 84)], [0])
    eng.decode_steps(3)
    assert eng.last_decode_disjoint is False
    eng.stream.synchronize()
    np.testing.assert_array_equal(eng.slot_tokens(0, min(k, 4)), solo[:min(k, 4)])
    eng.close()
