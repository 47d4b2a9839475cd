"""Sampling controls on the device (kr_sample_threshold, kr_gumbel_argmax_processed, kr_sample_count) against the numpy
restatement in tests/sampling_ref.py: kept sets at the production vocabulary, the sampled distribution of a small
vocabulary, determinism, neutral rows untouched, output counts."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import lib, ptr  # noqa: E402
from tests import sampling_ref as R  # noqa: E402
from tests.sampling_rows import DEV, V_PROD, Rows, d, pick, prod_batch as _prod_batch  # noqa: E402


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def test_kept_sets_match_numpy_at_the_production_vocabulary(L):
    rng = np.random.default_rng(5)
    logits, temps, params, prompts, outs, counts, pbits, spec = _prod_batch(rng)
    B, V = logits.shape
    # row 25 guided: a random half of the vocabulary allowed (mask table with one state)
    mw = 2 * ((V + 63) // 64)
    allow = rng.random(V) < 0.5
    allow[np.argsort(-logits[25])[:3]] = [True, False, True]
    mbits = np.zeros(mw, np.uint32)
    idx = np.flatnonzero(allow)
    np.bitwise_or.at(mbits, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    mt = d(mbits.view(np.int32))
    gm = np.zeros(B, np.int64); gm[25] = mt.data_ptr()
    masks = (d(gm),)
    seeds = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
    ctx = rng.integers(100, 200, B).astype(np.int32); plen = np.full(B, 90, np.int32)
    rows = Rows(logits, temps, seeds, params, counts, pbits, ctx, plen, masks=masks)
    thr = rows.threshold(L)
    thr2 = rows.threshold(L)
    np.testing.assert_array_equal(thr, thr2)
    av, ai = rows.argmax(L, 64)
    av2, ai2 = rows.argmax(L, 64)
    np.testing.assert_array_equal(av.view(np.uint32), av2.view(np.uint32))    # deterministic, bit for bit
    np.testing.assert_array_equal(ai, ai2)
    toks = pick(av, ai)
    for b, (T, k, p, m, rep, fq, pr) in enumerate(spec):
        allowed = allow if b == 25 else np.ones(V, bool)
        lp = R.penalise(logits[b], prompts[b], outs[b], V, rep, fq, pr)
        if T == 0:
            assert thr[b] == 0, f"row {b}: greedy rows are not truncated"
            assert toks[b] == int(np.argmax(np.where(allowed, lp, -np.inf))), f"row {b}"
            continue
        v = R.tempered(lp, T)
        keep, exc = R.kept_set(v, allowed, int(k), float(p), float(m))
        dev_keep = allowed & (R.fkey(v) >= thr[b])
        bad = (keep != dev_keep) & ~exc
        assert not bad.any(), f"row {b} {spec[b]}: {bad.sum()} tokens differ (numpy keeps {keep.sum()}, device {dev_keep.sum()})"
        if k == 1 or p <= 1e-6 or m == 1.0:
            assert dev_keep.sum() == (v[allowed] == v[allowed].max()).sum(), f"row {b}: a single (tied) top token"
        assert dev_keep[toks[b]], f"row {b}: sampled token {toks[b]} outside the kept set"
        tok, margin, excused = R.sample_step(logits[b], T, int(seeds[b]), int(ctx[b] + 1 - plen[b]), prompts[b], outs[b], V,
                                             allowed, int(k), float(p), float(m), rep, fq, pr)
        if margin > 1e-4 and not excused:
            assert toks[b] == tok, f"row {b}: device {toks[b]} numpy {tok}"


def test_neutral_rows_match_gumbel_argmax_guided_bit_for_bit(L):
    rng = np.random.default_rng(9)
    logits, temps, params, prompts, outs, counts, pbits, spec = _prod_batch(rng)
    B, V = logits.shape
    params[:] = 0
    params[:, 1], params[:, 3] = 1.0, 1.0            # every row neutral, counts and prompt bits set regardless
    seeds = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
    ctx = rng.integers(10, 20, B).astype(np.int32); plen = np.full(B, 5, np.int32)
    mw = 2 * ((V + 63) // 64)
    mbits = rng.integers(0, 2 ** 32, mw, dtype=np.uint64).astype(np.uint32)
    mt = d(mbits.view(np.int32))
    gm = np.zeros(B, np.int64); gm[3] = gm[22] = mt.data_ptr()
    rows = Rows(logits, temps, seeds, params, counts, pbits, ctx, plen, masks=(d(gm),))
    assert not rows.threshold(L).any()
    av, ai = rows.argmax(L, 64)
    av0 = torch.zeros(B, 64, device=DEV); ai0 = torch.zeros(B, 64, dtype=torch.int32, device=DEV)
    L.kr_gumbel_argmax_guided(ptr(rows.logits), V, V, ptr(rows.temps), ptr(rows.seeds), ptr(rows.ctx), ptr(rows.plen), ptr(av0),
                              ptr(ai0), 64, B, rows.gm(), ptr(rows.gstate), rows.mask_words, 0, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(av.view(np.uint32), av0.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ai, ai0.cpu().numpy())


def test_small_vocabulary_draws_follow_the_truncated_distribution(L):
    """16 tokens, 20,000 seeds (one row each): no dropped token is ever drawn, and the frequencies of the kept ones match the
    renormalised softmax over the kept set (chi-square below df + 7 sqrt(2 df), beyond 5 standard deviations)."""
    V, N = 16, 20000
    base = np.asarray([3.0, 2.5, 2.5, 2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -5.0, -6.0], np.float32)
    cases = [(1.0, 0, 0.8, 0.0), (0.7, 4, 1.0, 0.0), (1.0, 0, 1.0, 0.1), (1.5, 6, 0.9, 0.02)]
    for T, k, p, m in cases:
        logits = np.tile(base, (N, 1))
        params = np.zeros((N, 8), np.float32); params[:, :6] = [k, p, m, 1.0, 0.0, 0.0]
        seeds = (np.arange(N, dtype=np.uint64) * 2654435761 % (2 ** 32)).astype(np.uint32)
        rows = Rows(logits, np.full(N, T, np.float32), seeds.astype(np.uint32), params, np.zeros((N, V), np.int32),
                    np.zeros((N, 1), np.uint32), np.zeros(N, np.int32), np.zeros(N, np.int32))
        rows.threshold(L)
        av, ai = rows.argmax(L, 1)
        drawn = ai[:, 0]
        v = R.tempered(base, T)
        keep, exc = R.kept_set(v, np.ones(V, bool), k, p, m)
        assert not exc.any()
        assert keep[drawn].all(), f"{(T, k, p, m)}: a dropped token was drawn"
        pr = np.exp(v[keep].astype(np.float64) - v.max()); pr /= pr.sum()
        got = np.bincount(drawn, minlength=V)[keep]
        chi2 = float(((got - N * pr) ** 2 / (N * pr)).sum())
        df = max(1, int(keep.sum()) - 1)
        assert chi2 < df + 7 * np.sqrt(2 * df), f"{(T, k, p, m)}: chi2 {chi2:.1f} over df {df}"


def test_counts_follow_the_history_with_frozen_rows(L):
    """kr_sample_count after each step adds the step's token where the row is live (not finished, or ignore_eos)."""
    rng = np.random.default_rng(3)
    B, V, steps = 8, 1000, 40
    rows = Rows(np.zeros((B, V), np.float32), np.zeros(B, np.float32), np.zeros(B, np.uint32), np.tile([0, 1, 0, 1, 0, 0, 0, 0], (B, 1)),
                np.zeros((B, V), np.int32), np.zeros((B, (V + 31) // 32), np.uint32), np.zeros(B, np.int32), np.zeros(B, np.int32))
    hist = [[] for _ in range(B)]
    fin = np.zeros(B, np.int32)
    for s in range(steps):
        if s == 10:
            fin[[1, 4]] = 1
        if s == 25:
            fin[6] = 1
        rows.fin.copy_(torch.from_numpy(fin))
        ign = 1 if s == 30 else 0                # ignore_eos: finished rows still append a real token
        rows.threshold(L, ignore_eos=ign)
        toks = rng.integers(0, V, B).astype(np.int32)
        tk = d(toks)
        assert L.kr_sample_count(ptr(tk), ptr(rows.live), ptr(rows.counts), V, V, B, 0) == 0
        for b in range(B):
            if ign or not fin[b]:
                hist[b].append(int(toks[b]))
    torch.cuda.synchronize()
    got = rows.counts.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b], np.bincount(np.asarray(hist[b], np.int64), minlength=V))
