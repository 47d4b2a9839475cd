"""logit_bias / min_tokens / stop_token_ids on the device: kr_logits_adjust / kr_logits_restore / kr_stop_tokens against numpy bit
for bit, the adjusted logits through the existing sampler kernels against tests/sampling_ref.py (-inf passes the truncation), and
the engine, the slot scheduler and the in-process server on the tiny model."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd._lib import ADJ_CAP, lib, ptr  # noqa: E402
from karanta_ocr_amd.engine import Engine, PageRequest  # noqa: E402
from tests import adjust_cases as A  # noqa: E402

DEV = "cuda:0"
V = A.V_SMALL        # 1000: not a multiple of 64
LD = V + 37          # row stride above the vocabulary: the padding must stay as it is
PAD = np.float32(-7.5)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def d(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- kernels
def _kernel_rows(rng):
    """Seven rows: empty; one entry at id 0; one at id V - 1; KR_ADJ_CAP entries; stop entries at n = m - 1 (masked); the same at
    n = m (not masked); an id with bias AND stop flag while the mask is on.  Returns (per-row entries, min_tokens, n_b)."""
    full = [(int(i), float(v), int(f)) for i, v, f in zip(rng.permutation(V)[:ADJ_CAP], rng.uniform(-100, 100, ADJ_CAP),
                                                          rng.integers(0, 2, ADJ_CAP))]
    stops = [(17, 0.0, 1), (V - 2, 3.5, 1), (400, -2.25, 0), (63, 0.0, 1), (64, 1.0, 0)]
    rows = [([], 0), ([(0, 1.5, 0)], 0), ([(V - 1, -100.0, 0)], 0), (full, 2), (stops, 4), (stops, 4), ([(5, 100.0, 1), (6, 100.0, 0)], 9)]
    n_b = np.asarray([0, 3, 1, 5, 3, 4, 0], np.int32)     # row 3: n > m, nothing masked; row 4: n = m - 1; row 5: n = m
    return rows, n_b


def _expected(logits, ids, vals, flags, meta, n_b, rows):
    out = logits.copy()
    for b in rows:
        out[b, :V] = A.adjust_ref(logits[b, :V], ids[b], vals[b], flags[b], meta[b, 0], meta[b, 1], int(n_b[b]))
    return out


def test_adjust_and_restore_bit_for_bit(L):
    rng = np.random.default_rng(11)
    rows, n_b = _kernel_rows(rng)
    B = len(rows)
    ids, vals, flags, meta = A.tables(B, rows)
    ids[0, :8], vals[0, :8], flags[0, :8] = np.arange(8), 50.0, 1        # stale entries behind n_entries == 0: never read
    logits = np.full((B, LD), PAD, np.float32)
    logits[:, :V] = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    plen = np.full(B, 11, np.int32)
    ctx = (plen + n_b - 1).astype(np.int32)
    want = _expected(logits, ids, vals, flags, meta, n_b, range(B))
    assert np.isinf(want[4, [17, V - 2, 63]]).all() and not np.isinf(want[5]).any() and not np.isinf(want[3]).any()
    assert np.isinf(want[6, 5]) and want[6, 6] == logits[6, 6] + np.float32(100.0)      # the mask wins over the bias
    np.testing.assert_array_equal(bits(want[0]), bits(logits[0]))
    dl, di, dv, df, dm = d(logits), d(ids), d(vals), d(flags), d(meta)
    dc, dp = d(ctx), d(plen)
    saved = torch.full((B, ADJ_CAP), 123.0, device=DEV)
    assert L.kr_logits_adjust(ptr(dl), LD, V, ptr(di), ptr(dv), ptr(df), ptr(dm), ptr(dc), ptr(dp), ptr(saved), B, 0) == 0
    torch.cuda.synchronize()
    got = dl.cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))                   # entries adjusted, everything else (padding too) unchanged
    sv = saved.cpu().numpy()
    for b in range(B):
        n = int(meta[b, 0])
        np.testing.assert_array_equal(bits(sv[b, :n]), bits(logits[b, ids[b, :n]]))
        assert (sv[b, n:] == 123.0).all()
    assert L.kr_logits_restore(ptr(dl), LD, V, ptr(di), ptr(dm), ptr(saved), B, 0) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(dl.cpu().numpy()), bits(logits))    # what the lm_head wrote, bit for bit


def test_adjust_with_a_slot_offset_touches_only_its_rows(L):
    """The engine's first-token pass of a slot hands every array in at row slot0: rows 2..4 of 7 here."""
    rng = np.random.default_rng(12)
    rows, n_b = _kernel_rows(rng)
    B, j, n = len(rows), 2, 3
    ids, vals, flags, meta = A.tables(B, rows)
    logits = np.full((B, LD), PAD, np.float32)
    logits[:, :V] = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    plen = np.full(B, 5, np.int32)
    ctx = (plen + n_b - 1).astype(np.int32)
    want = _expected(logits, ids, vals, flags, meta, n_b, range(j, j + n))
    dl, di, dv, df, dm, dc, dp = d(logits), d(ids), d(vals), d(flags), d(meta), d(ctx), d(plen)
    saved = torch.zeros(B, ADJ_CAP, device=DEV)
    L.kr_logits_adjust(ptr(dl[j:]), LD, V, ptr(di[j:]), ptr(dv[j:]), ptr(df[j:]), ptr(dm[j:]), ptr(dc[j:]), ptr(dp[j:]), ptr(saved[j:]), n, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(dl.cpu().numpy()), bits(want))
    assert not saved[:j].any() and not saved[j + n:].any()
    L.kr_logits_restore(ptr(dl[j:]), LD, V, ptr(di[j:]), ptr(dm[j:]), ptr(saved[j:]), n, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(dl.cpu().numpy()), bits(logits))


def test_host_validation(L):
    from karanta_ocr_amd._lib import KarantaHipError
    with pytest.raises(KarantaHipError, match="null pointer"):
        L.kr_logits_adjust(16, LD, V, 0, 16, 16, 16, 16, 16, 16, 1, 0)
    with pytest.raises(KarantaHipError, match="bad sizes"):
        L.kr_logits_restore(16, V - 1, V, 16, 16, 16, 1, 0)
    with pytest.raises(KarantaHipError, match="bad sizes"):
        L.kr_stop_tokens(16, 16, 16, 16, 16, 0, 0, 0)


def test_stop_tokens(L):
    stops = [(17, 0.0, 1), (400, 2.0, 0), (V - 1, -1.0, 1)] + [(100 + i, 0.0, 0) for i in range(70)] + [(900, 0.0, 1)]
    rows = [(stops, 0)] * 6 + [([], 0), (stops, 50)]
    B = len(rows)
    ids, vals, flags, meta = A.tables(B, rows)
    ids[6, :4], flags[6, :4] = 17, 1                          # row 6: n_entries == 0, stale entries behind it
    #        stop    not in table  bias-only entry  finished   stop past lane 63  last id  empty  min_tokens on: still stops
    toks = [17,      18,           400,             17,        900,               V - 1,   17,    17]
    fin0 = [0,       0,            0,               1,         0,                 0,       0,     0]
    want = [1,       0,            0,               1,         1,                 1,       0,     1]
    di, df, dm, dt = d(ids), d(flags), d(meta), d(toks, np.int32)
    for flags_word, expect in ((0, want), (2, want), (1, fin0), (3, fin0)):       # bit 0 of ignore_eos: nothing finishes
        fin = d(fin0, np.int32)
        assert L.kr_stop_tokens(ptr(dt), ptr(di), ptr(df), ptr(dm), ptr(fin), flags_word, B, 0) == 0
        torch.cuda.synchronize()
        assert fin.cpu().numpy().tolist() == expect, flags_word
    fin = d(fin0, np.int32)                                   # slot offset: rows 4..5 only
    L.kr_stop_tokens(ptr(dt[4:]), ptr(di[4:]), ptr(df[4:]), ptr(dm[4:]), ptr(fin[4:]), 0, 2, 0)
    torch.cuda.synchronize()
    assert fin.cpu().numpy().tolist() == [0, 0, 0, 1, 1, 1, 0, 0]


@pytest.mark.parametrize("vocab", [A.V_SMALL, A.V_PROD])
@pytest.mark.parametrize("kind", ["plain", "processed"])
def test_adjusted_logits_through_the_sampler_kernels(L, kind, vocab):
    """kr_logits_adjust, then kr_gumbel_argmax_guided (plain) or kr_sample_threshold + kr_gumbel_argmax_processed: the token of
    every row is sample_step's on the numpy-adjusted logits, T = 0 and T > 0, top_k / top_p / min_p / penalties on, with the row's
    best tokens at -inf.  Excuse rule of test_gpu_sampling_kernels.py; tests/test_adjust_cpu.py shows these seeds excuse no row."""
    from tests.test_gpu_sampling_kernels import Rows, pick
    c = A.integration_case(kind, vocab)
    B, Vv = c["B"], c["V"]
    rows = Rows(c["logits"], c["temps"], c["seeds"], c["params"], c["counts"], c["pbits"], c["ctx"], c["plen"])
    di, dv, df, dm = d(c["ids"]), d(c["vals"]), d(c["flags"]), d(c["meta"])
    saved = torch.zeros(B, ADJ_CAP, device=DEV)
    L.kr_logits_adjust(ptr(rows.logits), Vv, Vv, ptr(di), ptr(dv), ptr(df), ptr(dm), ptr(rows.ctx), ptr(rows.plen), ptr(saved), B, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(rows.logits.cpu().numpy()), bits(c["adjusted"]))
    if kind == "plain":
        av = torch.zeros(B, 64, device=DEV)
        ai = torch.zeros(B, 64, dtype=torch.int32, device=DEV)
        L.kr_gumbel_argmax_guided(ptr(rows.logits), Vv, Vv, ptr(rows.temps), ptr(rows.seeds), ptr(rows.ctx), ptr(rows.plen), ptr(av),
                                  ptr(ai), 64, B, None, None, 0, 0, 0)
        torch.cuda.synchronize()
        av, ai = av.cpu().numpy(), ai.cpu().numpy()
    else:
        rows.threshold(L)
        av, ai = rows.argmax(L, 64)
    toks = pick(av, ai)
    checked = 0
    for b, (tok, margin, excused) in enumerate(c["ref"]):
        print(f"{kind} V={Vv} row {b} {c['spec'][b]}: device {toks[b]} numpy {tok} margin {margin:.4f} excused {excused}")
        if margin > A.MARGIN and not excused:
            assert toks[b] == tok, f"row {b}: device {toks[b]} numpy {tok}"
            checked += 1
    assert checked == B                                       # no row excused
    L.kr_logits_restore(ptr(rows.logits), Vv, Vv, ptr(di), ptr(dm), ptr(saved), B, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(rows.logits.cpu().numpy()), bits(c["logits"]))


# ----------------------------------------------------------------------------- engine
X = 123              # an ordinary token of the tiny vocabulary


@pytest.fixture(scope="module")
def tiny(tiny_models):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, w, _ = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=3, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
    eng.load_weights(w)
    yield cfg, eng
    eng.close()


def _page(cfg, i, **kw):
    rng = np.random.default_rng(700 + i)
    h, wd = [(56, 84), (84, 56), (56, 56), (112, 84)][i % 4]
    pv, grid = IP.image_to_patches(IP.synthetic_page(400 + i, h, wd))
    T = grid[1] * grid[2] // 4
    ids = np.concatenate([rng.integers(0, 400, 2 + i % 3), [cfg.vision_start_token_id], [cfg.image_token_id] * T,
                          [cfg.vision_end_token_id], rng.integers(0, 400, 3)]).astype(np.int64)
    return PageRequest(ids, pv, [grid], **kw)


def test_bias_forces_a_token_and_min_tokens_holds_back_eos(tiny):
    cfg, eng = tiny
    eos = int(cfg.eos_token_ids[0])
    res = eng.generate([_page(cfg, 0, logit_bias={X: 100.0})], 6)
    assert res.tokens[0].tolist() == [X] * 6 and res.finish_reasons[0] == "length"
    res = eng.generate([_page(cfg, 0, logit_bias={eos: 100.0}, min_tokens=3)], 8)
    t = res.tokens[0].tolist()
    assert len(t) == 4 and t[3] == eos and not set(t[:3]) & set(cfg.eos_token_ids) and res.finish_reasons[0] == "stop"
    res = eng.generate([_page(cfg, 0, logit_bias={eos: 100.0})], 8)            # without min_tokens: EOS at once
    assert res.tokens[0].tolist() == [eos]


def test_stop_token_ids_finish_the_row(tiny):
    cfg, eng = tiny
    res = eng.generate([_page(cfg, 1, logit_bias={X: 100.0}, stop_token_ids=(X,))], 8)
    assert res.tokens[0].tolist() == [X] and res.finish_reasons[0] == "stop"
    res = eng.generate([_page(cfg, 1, logit_bias={X: 100.0}, stop_token_ids=(X,), min_tokens=3)], 8)
    t = res.tokens[0].tolist()
    assert len(t) == 4 and X not in t[:3] and t[3] == X and res.finish_reasons[0] == "stop"
    res = eng.generate([_page(cfg, 1, logit_bias={X: 100.0}, stop_token_ids=(X,))], 4, ignore_eos=True)   # bit 0: runs on
    assert res.tokens[0].tolist() == [X] * 4 and res.finish_reasons[0] == "length"


def test_ban_moves_step_0_to_the_runner_up_and_logits_stay_raw(tiny):
    cfg, eng = tiny
    plain = eng.generate([_page(cfg, 2)], 8, ignore_eos=True, return_logits=True)
    t0 = int(plain.tokens[0][0])
    for graph in (False, True):
        res = eng.generate([_page(cfg, 2, logit_bias={t0: -100.0})], 8, ignore_eos=True, return_logits=not graph)
        biased = plain.logits[0, 0].astype(np.float32).copy()
        biased[t0] = biased[t0] + np.float32(-100.0)
        assert int(res.tokens[0][0]) == int(np.argmax(biased)) != t0
        assert t0 not in res.tokens[0].tolist()
        if not graph:      # returned logits are the lm_head's: step 0 has the same input as the unbiased run
            np.testing.assert_array_equal(bits(res.logits[0, 0]), bits(plain.logits[0, 0]))
            eager = res
    np.testing.assert_array_equal(res.tokens[0], eager.tokens[0])              # graph path = eager path


def test_plain_rows_next_to_an_adjusted_row_equal_their_solo_runs(tiny):
    cfg, eng = tiny
    pages = [_page(cfg, 0), _page(cfg, 1, logit_bias={X: 4.0, 7: -100.0}, min_tokens=5, stop_token_ids=(9,)), _page(cfg, 2)]
    res = eng.generate(pages, 10, ignore_eos=True)
    for b in (0, 2):
        solo = eng.generate([pages[b]], 10, ignore_eos=True)
        np.testing.assert_array_equal(res.tokens[b], solo.tokens[0])
    solo = eng.generate([pages[1]], 10, ignore_eos=True)
    np.testing.assert_array_equal(res.tokens[1], solo.tokens[0])


def test_logprobs_report_the_raw_logits(tiny):
    cfg, eng = tiny
    plain = eng.generate([_page(cfg, 3, logprobs=5)], 4, ignore_eos=True)
    res = eng.generate([_page(cfg, 3, logprobs=5, logit_bias={X: 100.0})], 4, ignore_eos=True)
    assert res.tokens[0].tolist() == [X] * 4
    np.testing.assert_array_equal(res.logprobs[0]["top_ids"][0], plain.logprobs[0]["top_ids"][0])
    np.testing.assert_array_equal(bits(res.logprobs[0]["top"][0]), bits(plain.logprobs[0]["top"][0]))
    assert res.logprobs[0]["token"][0] <= plain.logprobs[0]["top"][0][0] and res.logprobs[0]["token"][0] < -0.5   # log p(X) under the
    #                                                                              raw distribution, not the forced ~0
    # a row finished by a stop id records no log-prob for that step, as on EOS
    res = eng.generate([_page(cfg, 3, logprobs=5, logit_bias={X: 100.0}, stop_token_ids=(X,), min_tokens=2)], 6)
    assert len(res.tokens[0]) == 3 and len(res.logprobs[0]["token"]) == 2


@pytest.fixture(scope="module")
def tiny2(tiny_models):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, w, _ = tiny_models["tiny"]
    eng = Engine(cfg, max_batch=2, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
    eng.load_weights(w)
    yield cfg, eng
    eng.close()


def test_slot_scheduler_adjusted_request_comes_and_goes(tiny2):
    """A plain greedy request decodes in slot 0 while an adjusted one is admitted into slot 1, finishes and leaves; a later plain
    request reuses slot 1.  The adjusted request bans the later request's first token: a table left behind would change it."""
    from karanta_ocr_amd._lib import KarantaHipError
    from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler
    cfg, eng = tiny2
    p, q = _page(cfg, 0), _page(cfg, 2)
    solo_p, solo_q = eng.generate([p], 14), eng.generate([q], 6)
    q0 = int(solo_q.tokens[0][0])
    a = _page(cfg, 1, logit_bias={q0: -100.0, X: 100.0}, min_tokens=2, stop_token_ids=(X,))
    solo_a = eng.generate([a], 8)
    assert solo_a.tokens[0].tolist()[2:] == [X] and solo_a.finish_reasons[0] == "stop"
    sch = SlotScheduler(eng, max_tokens_cap=14, chunk=2, sampling=True)
    res = sch.run([SlotRequest(p, 14, tag="p"), SlotRequest(a, 8, tag="a"), SlotRequest(q, 6, tag="q")])
    for r, s in zip(res, (solo_p, solo_a, solo_q)):
        assert r.error is None
        np.testing.assert_array_equal(r.tokens, s.tokens[0])
        assert r.finish_reason == s.finish_reasons[0]
    with pytest.raises(KarantaHipError, match="greedy configuration"):
        SlotScheduler(eng, max_tokens_cap=14, chunk=2)
        eng.admit([a], [0])


def test_server_request_with_stop_string_and_bias(tiny2):
    from karanta_ocr_amd import serving as S
    cfg, eng = tiny2
    srv = S.LocalServer(eng, S.ChatFrontend(cfg, S.ByteTokenizer(cfg)), log=lambda *_: None, continuous=True, max_tokens_cap=16, chunk=2)
    try:
        req = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 12, "logit_bias": {str(ord("a")): 100}, "stop": ["aaa"],
               "include_stop_str_in_output": True}
        st, body = srv.chat_completions(req)
        assert st == 200, body
        assert body["choices"][0]["message"]["content"] == "aaa" and body["choices"][0]["finish_reason"] == "stop"
        assert body["usage"]["completion_tokens"] == 3
        assert body["usage"]["total_tokens"] == body["usage"]["prompt_tokens"] + 3
        st, body = srv.chat_completions(dict(req, stop=["aaaa"], include_stop_str_in_output=False, logit_bias={str(ord("a")): 100}))
        assert body["choices"][0]["message"]["content"] == "" and body["usage"]["completion_tokens"] == 4
    finally:
        srv.close()
