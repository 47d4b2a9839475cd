"""The sampler tail on the rows of tests/select_cases.py: kr_sample_threshold must return the expected KEY (count mode from a
sort, mass mode under the 2^-10 margin, the combined rows, penalties, guide masks; no token is excused), the filter of
kr_gumbel_argmax_processed must drop tokens one key below the threshold whatever their noise, the partials of every partition
count reduce through kr_sample_greedy to the expected token, and kr_logprobs_topk holds up to the largest candidate table its
argument check accepts.  tests/test_select_cases_cpu.py proves the cases themselves in the default suite."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError, lib, ptr  # noqa: E402
from oracle import qwen2vl_oracle as O  # noqa: E402
from tests import select_cases as S  # noqa: E402
from tests.sampling_rows import DEV, Rows, d, pick  # noqa: E402

CHUNK = 448           # rows per launch
CTX, PLEN = 7, 5      # generated-token index CTX + 1 - PLEN = S.N_STEP


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def bits_of(idx, words):
    out = np.zeros(words, np.uint32)
    idx = np.asarray(idx, np.int64)
    np.bitwise_or.at(out, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return out


def rows_of(case_rows, params, seeds=None):
    """Rows for a list of select_cases.Row of one vocabulary (counts, prompt bits and per-row guide masks uploaded)."""
    B, V = len(case_rows), case_rows[0].V
    W, mw = (V + 31) // 32, 2 * ((V + 63) // 64)
    dense = {}
    for r in case_rows:
        if id(r) not in dense:
            dense[id(r)] = (np.bincount(r.outs, minlength=V).astype(np.int32), bits_of(r.prompt, W),
                            None if r.allow is None else bits_of(np.flatnonzero(r.allow), mw))
    logits = np.stack([r.logits for r in case_rows])
    counts = np.stack([dense[id(r)][0] for r in case_rows])
    pbits = np.stack([dense[id(r)][1] for r in case_rows])
    masks = None
    if any(r.allow is not None for r in case_rows):
        table = d(np.stack([np.zeros(mw, np.uint32) if r.allow is None else dense[id(r)][2] for r in case_rows]).view(np.int32))
        gm = np.asarray([0 if r.allow is None else table.data_ptr() + b * mw * 4 for b, r in enumerate(case_rows)], np.int64)
        masks = (d(gm), table)
    return Rows(logits, np.ones(B, np.float32), np.zeros(B, np.uint32) if seeds is None else seeds, np.asarray(params, np.float32),
                counts, pbits, np.full(B, CTX, np.int32), np.full(B, PLEN, np.int32), masks=masks)


def check_thresholds(L, cases):
    """every case's threshold, in launches of CHUNK rows of one vocabulary, each launched twice"""
    bad = []
    for V in sorted({c.row.V for c in cases}):
        cs = [c for c in cases if c.row.V == V]
        for i in range(0, len(cs), CHUNK):
            part = cs[i:i + CHUNK]
            rows = rows_of([c.row for c in part], [c.params() for c in part])
            thr = rows.threshold(L)
            np.testing.assert_array_equal(thr, rows.threshold(L), err_msg="a repeated call must return the same bits")
            want = np.asarray([c.expect for c in part], np.uint64)
            work = None
            for j in np.flatnonzero(thr != want):
                if work is None:
                    work = rows.work.cpu().numpy()
                c = part[j]
                same = (work[j].view(np.uint32) == c.row.scores.view(np.uint32)).all()
                bad.append(S.describe(f"{c.family} {c.note} (V {V}, top_k {c.top_k}, top_p {c.top_p!r}, min_p {c.min_p!r}; work row "
                                      f"{'as expected' if same else 'DIFFERS from the penalised scores'})", c.expect, thr[j]))
    assert not bad, f"{len(bad)} of {len(cases)} thresholds differ:\n" + "\n".join(bad[:12])


def family_cases(prefix):
    return [c for c in S.threshold_cases() if c.family.startswith(prefix)]


@pytest.mark.parametrize("V", S.VS)
@pytest.mark.parametrize("fill", ["ninf", "m3e38"])
def test_top_k_returns_the_key_of_the_kth_score_at_every_landmark(L, V, fill):
    cases = [c for c in S.threshold_cases() if c.family == f"count/V{V}/{fill}"]
    assert len(cases) > 1200 and not any(c.row.pen for c in cases)
    check_thresholds(L, cases)


def test_top_k_behind_penalties_and_guide_masks(L):
    cases = [c for c in S.threshold_cases() if c.family in (f"count/V{S.VS[1]}/ninf/pen", "count/mask")]
    assert sum(c.row.pen for c in cases) > 1200 and sum(c.row.allow is not None for c in cases) == 6
    check_thresholds(L, cases)


def test_top_p_returns_the_key_of_the_cut_group(L):
    """every mass family: alone, over what top_k kept, behind penalties, behind a mask that halves the cut group"""
    S.check_coverage()
    cases = family_cases("mass/")
    cuts = {c.expect for c in cases}
    assert 0x80000000 in cuts and 0x7FFFFFFF in cuts and len(cases) > 1000
    check_thresholds(L, cases)


def test_min_p_cut_alone_and_under_top_k_and_top_p(L):
    cases = family_cases("min_p/")
    assert len(cases) >= 12 + 6
    check_thresholds(L, cases)


def test_landmarks_scattered_over_the_production_vocabulary(L):
    cases = S.prod_landmark_cases()
    assert len(cases) == 32 and cases[0].row.V == S.V_PROD
    check_thresholds(L, cases)


def greedy(L, av, ai, B, table, ctx=CTX, plen=PLEN):
    """kr_sample_greedy over device partials [B, n_part]: (tokens, next-step embedding rows)"""
    n_part, dm = av.shape[1], table.shape[1]
    tok = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    hist = torch.full((ctx + 2 - plen, B), -1, dtype=torch.int32, device=DEV)
    d_plen, d_ctx = d(np.full(B, plen, np.int32)), d(np.full(B, ctx, np.int32))
    fin, eos = torch.zeros(B, dtype=torch.int32, device=DEV), torch.tensor([-5], dtype=torch.int32, device=DEV)
    xn = torch.zeros(B, dm, dtype=torch.bfloat16, device=DEV)
    assert L.kr_sample_greedy(ptr(av), ptr(ai), n_part, ptr(table), dm, ptr(tok), ptr(hist), B, ptr(d_plen), ptr(d_ctx), ptr(fin),
                              ptr(eos), 1, 0, 0, ptr(xn), B, 0) == 0
    torch.cuda.synchronize()
    t = tok.cpu().numpy()
    np.testing.assert_array_equal(hist.cpu().numpy()[ctx + 1 - plen], t)
    np.testing.assert_array_equal(xn.float().cpu().numpy(), table.float().cpu().numpy()[t])
    return t


def embed_table(n_rows):
    g = torch.Generator().manual_seed(n_rows)
    return torch.randn(n_rows, 8, generator=g).to(torch.bfloat16).to(DEV)


def test_filter_drops_one_key_below_the_threshold_whatever_the_noise(L):
    cases = S.filter_cases()
    for V in S.VS:
        cs = [c for c in cases if c.row.V == V]
        assert {c.kind for c in cs} == set(S.FILTER_KINDS)
        rows = rows_of([c.row for c in cs], [[S.N_KEPT, 1, 0, 1, 0, 0, 0, 0]] * len(cs), np.asarray([c.seed for c in cs], np.uint32))
        thr = rows.threshold(L)
        for c, t in zip(cs, thr):
            assert t == c.thr, S.describe(f"filter/{c.kind} threshold", c.thr, t)
        table = embed_table(V)
        for n_part in (1, 7):
            av, ai = rows.argmax(L, n_part)
            toks = greedy(L, d(av), d(ai), len(cs), table)
            np.testing.assert_array_equal(toks, pick(av, ai))
            for c, t in zip(cs, toks):
                what = "a DROPPED token" if t in c.dropped else "another kept token" if t in c.kept else "a token outside the groups"
                assert t == c.expect, f"filter/{c.kind} (V {V}, n_part {n_part}, seed {c.seed}): token {t} ({what}), expected {c.expect}"


@pytest.mark.parametrize("V", S.VS)
def test_partitions_reduce_to_the_winner(L, V):
    table = embed_table(V)
    for n_part in S.N_PARTS:
        logits, temps, win = S.partition_rows(V, n_part)
        B = len(win)
        params = np.tile(np.asarray([0, 1, 0, 1, 0, 0, 0, 0], np.float32), (B, 1))
        rows = Rows(logits, temps, np.arange(B, dtype=np.uint32) + 11, params, np.zeros((B, V), np.int32),
                    np.zeros((B, (V + 31) // 32), np.uint32), np.full(B, CTX, np.int32), np.full(B, PLEN, np.int32))
        assert not rows.threshold(L).any()
        av, ai = rows.argmax(L, n_part)
        per, ne = S.part_span(V, n_part)
        for r in range(B):
            assert (ai[r, ne:] == S.IDX_NONE).all() and np.isneginf(av[r, ne:]).all(), f"V {V} n_part {n_part}: empty partitions"
            if temps[r] == 0:
                val, idx = S.partials_ref(logits[r], V, n_part)
                np.testing.assert_array_equal(av[r].view(np.uint32), val.view(np.uint32), err_msg=f"V {V} n_part {n_part} row {r}")
                np.testing.assert_array_equal(ai[r], idx, err_msg=f"V {V} n_part {n_part} row {r}")
            else:
                lo_, hi_ = np.arange(n_part) * per, np.minimum(V, (np.arange(n_part) + 1) * per)
                assert ((ai[r, :ne] >= lo_[:ne]) & (ai[r, :ne] < hi_[:ne])).all(), "a partial's token lies in its partition"
        toks = greedy(L, d(av), d(ai), B, table)
        np.testing.assert_array_equal(toks, win, err_msg=f"V {V} n_part {n_part} (per {per}, {ne} non-empty)")


@pytest.mark.parametrize("n_part", S.GREEDY_N_PARTS)
def test_greedy_reads_every_partial_and_prefers_the_lower_id(L, n_part):
    val, ids, want, spots = S.greedy_partials(n_part)
    toks = greedy(L, d(val), d(ids, np.int32), len(want), embed_table(int(ids.max()) + 1))
    for r, p in enumerate(spots):
        assert toks[r] == want[r], f"n_part {n_part}, maximum at partial {p} (id {ids[r, p]}): token {toks[r]}, expected {want[r]}"


# ----------------------------------------------------------------------------- kr_logprobs_topk
def logprobs(L, logits, toks, k, n_part):
    """(out_lp [B, 1 + k], out_idx [B, k]) of one call, every row at history index 0"""
    B, V = logits.shape
    kk = max(k, 1)
    ld, pv = d(logits), torch.zeros(B, n_part, kk, device=DEV)
    pi, ms = torch.zeros(B, n_part, kk, dtype=torch.int32, device=DEV), torch.zeros(B, n_part, 2, device=DEV)
    out, oi = torch.full((1, B, 1 + kk), 7.0, device=DEV), torch.full((1, B, kk), -3, dtype=torch.int32, device=DEV)
    z = torch.zeros(B, dtype=torch.int32, device=DEV)
    L.kr_logprobs_topk(ptr(ld), V, V, k, n_part, ptr(pv), ptr(pi), ptr(ms), ptr(d(toks, np.int32)), ptr(z), ptr(z), ptr(z), ptr(out),
                       ptr(oi), 1, B, kk, B, 0)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0], oi.cpu().numpy()[0]


def check_logprobs(logits, toks, k, lp, ix, tag):
    for b in range(logits.shape[0]):
        ids, vals = O.top_logprobs(logits[b], k)
        n = min(k, int(np.isfinite(logits[b]).sum()))
        np.testing.assert_array_equal(ix[b, :n], ids[:n], err_msg=f"{tag} row {b}")
        np.testing.assert_allclose(lp[b, 1:1 + n], vals[:n], rtol=1e-5, atol=5e-5, err_msg=f"{tag} row {b}")
        assert (ix[b, n:k] == S.IDX_NONE).all() and np.isneginf(lp[b, 1 + n:1 + k]).all(), f"{tag} row {b}: no token left"
        want = O.log_softmax(logits[b])[toks[b]]
        if np.isneginf(want):
            assert np.isneginf(lp[b, 0]), f"{tag} row {b}"
        else:
            np.testing.assert_allclose(lp[b, 0], want, rtol=1e-5, atol=5e-5, err_msg=f"{tag} row {b}")


# n_part * k * 8 bytes of candidates against the 159 KiB the argument check accepts (20352 candidates): 1024 * 19 and, the most
# that n_part <= 1024 and k <= 20 can reach, 1017 * 20; at V = 4096 a slice holds 4 or 5 logits, fewer than k
@pytest.mark.parametrize("n_part,k", [(1024, 19), (1017, 20)])
def test_logprobs_topk_at_the_largest_candidate_table(L, n_part, k):
    rng = np.random.default_rng(n_part)
    B, V = 3, 4096
    logits = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    logits[1] = np.round(logits[1])                                # many ties
    logits[2, 5:] = -np.inf                                         # fewer than k finite logits
    toks = np.asarray([17, 4095, 9], np.int32)
    assert n_part * k * 8 > 64 * 1024 and n_part * k * 8 <= 159 * 1024
    lp, ix = logprobs(L, logits, toks, k, n_part)
    check_logprobs(logits, toks, k, lp, ix, f"n_part {n_part} k {k}")


def test_logprobs_topk_rejects_the_first_table_beyond_the_bound(L):
    logits = np.zeros((1, 4096), np.float32)
    for n_part, k in ((1018, 20), (1024, 20)):
        assert n_part * k * 8 > 159 * 1024
        with pytest.raises(KarantaHipError, match="candidates exceed the LDS"):
            logprobs(L, logits, np.zeros(1, np.int32), k, n_part)
    lp, ix = logprobs(L, logits, np.zeros(1, np.int32), 20, 1017)   # and the call after a rejection runs
    np.testing.assert_array_equal(ix[0], np.arange(20))


def test_logprobs_topk_slice_borders_and_missing_tokens(L):
    V, n_part, k = 5003, 4, 5
    per = (V + n_part - 1) // n_part
    rng = np.random.default_rng(12)
    logits = (rng.standard_normal((6, V)) * 2).astype(np.float32)
    logits[0, [10, 3000, 4000, 4900]] = [20, 19, 18, 17]
    logits[0, [per - 1, per]] = 16.0                                # k-th and (k+1)-th tied across the border of slices 0 and 1
    logits[1, [3000, 4000, 4900]] = [20, 19, 18]
    logits[1, [per - 1, per, 2 * per]] = 16.0                       # the tie takes the last two places: lowest ids first
    logits[2, 2 * per + 7:2 * per + 12] = [30, 31, 31, 29, 28]      # all k winners in one slice
    logits[3, per:2 * per] = -np.inf                                # a slice made entirely of -inf
    logits[4] = -np.inf
    logits[4, [per - 1, per, V - 1]] = [1.0, 1.0, 2.0]              # fewer than k finite logits
    logits[5, 77] = -np.inf                                         # the sampled token at -inf
    toks = np.asarray([per, per - 1, 5, per + 1, V - 1, 77], np.int32)
    lp, ix = logprobs(L, logits, toks, k, n_part)
    check_logprobs(logits, toks, k, lp, ix, "borders")
    assert ix[0, 4] == per - 1 and list(ix[1, 3:5]) == [per - 1, per] and list(ix[4]) == [V - 1, per - 1, per, S.IDX_NONE, S.IDX_NONE]
    assert np.isneginf(lp[3, 0]) and np.isneginf(lp[5, 0]) and np.isfinite(lp[[0, 1, 2, 4], 0]).all()
