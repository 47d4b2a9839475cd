"""The three launches that let a speculative decode step record log-probabilities, through the C-ABI on a real MI355X
(include/karanta_hip.h): kr_logprobs_topk_rows against kr_logprobs_topk on a one-row batch holding the same logits row (bit for bit:
the two share their bodies, csrc/kr_logprobs.h), against the float64 oracle (the tolerance of
tests/test_gpu_kernels.py::test_logprobs_topk_matches_oracle) and against the numpy statement of which tokens record
(tests/spec_logprobs_ref.py); kr_logits_restore_rows behind kr_logits_adjust_rows; kr_spec_mark.  Every output lies between guard
words or in a buffer pre-filled with a sentinel, and the rows that record nothing hold NaN logits.
(Fails on a tree without the feature: the library exports none of the three.)"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import ADJ_CAP, KarantaHipError, Spec, SpecLogprobs, lib, ptr  # noqa: E402
from oracle import qwen2vl_oracle as O  # noqa: E402
from tests import adjust_cases as A  # noqa: E402
from tests import spec_logprobs_ref as LR  # noqa: E402
from tests.test_gpu_spec_guide_kernels import Guarded  # noqa: E402

DEV = "cuda:0"
KS, PAD = 20, 3                       # k_stride of the history; the pad token
LP_FILL, ID_FILL = 7.0, -3            # sentinels of the two histories


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# per layout: slots, K, rows, the dealt map (None: static), and per slot (prompt_len, ctx_before, emitted, finished after the step)
LAYOUTS = {
    # static, 3 slots x (2 + 1) rows of 17.  History of 6 records:
    #   slot 0  finished by its only token: no record;  slot 1  e = K + 1, its last token at h = 6 = hist_len: two records, no third;
    #   slot 2  a middle e
    "static": dict(slots=3, k=2, rows=17, draft_row=None,
                   state=[(9, 12, 1, 1), (5, 8, 3, 0), (20, 20, 2, 0)]),
    # shared, 5 slots, K = 3, 17 rows, the map written by hand: rows out of order, -1 where a draft has no row.
    #   slot 0  frozen (e = 0);  slot 1  e = 1, its first draft wrong;  slot 2  e = 2 of 3 drafts;  slot 3  e = K + 1;
    #   slot 4  finished by the third of its 3 tokens: two records
    "shared": dict(slots=5, k=3, rows=17,
                   draft_row=[[-1, -1, -1], [11, -1, -1], [16, 5, 9], [14, 7, 12], [6, 15, -1]],
                   state=[(4, 7, 0, 1), (6, 6, 1, 0), (3, 5, 2, 0), (10, 10, 4, 0), (8, 9, 3, 1)]),
}
HIST_LEN, HIST_ROWS, COL0 = 6, 9, 1   # records kept / rows of the token history / first history column of the slots


class Step:
    """The state a speculative step leaves behind its verification, and the buffers kr_logprobs_topk_rows reads and writes."""

    def __init__(self, layout, V, n_part, k_top, seed=0):
        lay = LAYOUTS[layout]
        self.S, self.K, self.R, self.V, self.n_part, self.k_top = lay["slots"], lay["k"], lay["rows"], V, n_part, k_top
        S, K, R = self.S, self.K, self.R
        rng = np.random.default_rng(seed + V + 31 * k_top + (7 if layout == "shared" else 0))
        self.draft_row = None if lay["draft_row"] is None else np.asarray(lay["draft_row"], np.int32)
        self.plen = np.asarray([s[0] for s in lay["state"]], np.int32)
        self.before = np.asarray([s[1] for s in lay["state"]], np.int32)
        self.ctx = self.before + np.asarray([s[2] for s in lay["state"]], np.int32)
        self.fin = np.asarray([s[3] for s in lay["state"]], np.int32)
        self.HB = S + 2                                 # the history is wider than the step: columns COL0 .. COL0 + S - 1
        self.hist = rng.integers(0, V, (HIST_ROWS, S)).astype(np.int32)
        self.recs = LR.records(self.before, self.ctx, self.plen, self.fin, K, R, HIST_LEN, self.draft_row, hist_rows=HIST_ROWS)
        # one recorded token lies outside the vocabulary: its value is -inf, its top-k is written (kr_logprobs_topk's rule)
        s, _, _, h = self.recs[-1]
        self.hist[h, s] = V + 5
        logits = np.full((R, V), np.nan, np.float32)    # the rows that record nothing: NaN
        for i, (_, _, row, _) in enumerate(self.recs):
            lg = (rng.standard_normal(V) * 4).astype(np.float32)
            if i % 3 == 0:
                lg[7] = lg[3] = lg.max() + 1.0          # an exact tie at the top
            if i % 3 == 1:
                lg = np.round(lg)                       # many ties further down
            logits[row] = lg
        self.logits = logits
        kk = max(k_top, 1)
        self.pv, self.pi = Guarded(np.full((R, n_part, kk), -9.0, np.float32)), Guarded(np.full((R, n_part, kk), -9, np.int32))
        self.ms = Guarded(np.full((R, n_part, 2), -9.0, np.float32))
        self.out = Guarded(np.full((HIST_LEN, self.HB, 1 + KS), LP_FILL, np.float32))
        self.oi = Guarded(np.full((HIST_LEN, self.HB, KS), ID_FILL, np.int32))
        full = lambda a, fill: t_(np.concatenate([a, np.full(R - S, fill, a.dtype)]))
        self.d_logits = t_(logits)
        self.d_hist, self.d_ctx, self.d_plen, self.d_fin = t_(self.hist), full(self.ctx, -5), full(self.plen, -5), full(self.fin, 1)
        self.d_before = t_(self.before)
        self.d_map = None if self.draft_row is None else t_(self.draft_row)
        self.d_i = t_(np.zeros(max(R, S * K, 64), np.int32))            # what the launches under test never read
        self.d_f = t_(np.zeros(64 * 8, np.float32))

    def spec(self, **change):
        i, f = ptr(self.d_i), ptr(self.d_f)
        a = Spec(self.S, self.K, self.R, 2, 4, 64, i, 64, ptr(self.d_hist), self.d_hist.stride(0), HIST_ROWS, None, None, i, ptr(self.d_ctx),
                 ptr(self.d_plen), ptr(self.d_fin), f, i, i, i, f, 64, PAD, self.V, f, 64, i, i)
        for k, v in change.items():
            setattr(a, k, v)
        return a

    def lp(self, **change):
        off = COL0 * (1 + KS) * 4, COL0 * KS * 4
        p = SpecLogprobs(self.k_top, self.n_part, self.pv.ptr, self.pi.ptr, self.ms.ptr, self.out.ptr + off[0], self.oi.ptr + off[1],
                         HIST_LEN, self.HB, KS, ptr(self.d_before))
        for k, v in change.items():
            setattr(p, k, v)
        return p

    def launch(self, L):
        a, p = self.spec(), self.lp()
        L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), ptr(self.d_map) if self.d_map is not None else None, ptr(self.d_logits), self.V, 0)
        torch.cuda.synchronize()
        return self.out.get(), self.oi.get()


def one_row(L, logits_row, tok, n_part, k):
    """kr_logprobs_topk on a one-row batch holding this row: (values [1 + KS], ids [KS]) of its record."""
    V = logits_row.shape[0]
    kk = max(k, 1)
    lg = t_(logits_row[None])
    pv, pi = torch.zeros(1, n_part, kk, device=DEV), torch.zeros(1, n_part, kk, dtype=torch.int32, device=DEV)
    ms = torch.zeros(1, n_part, 2, device=DEV)
    out, oi = torch.full((1, 1, 1 + KS), LP_FILL, device=DEV), torch.full((1, 1, KS), ID_FILL, dtype=torch.int32, device=DEV)
    d_tok, d_ctx, d_plen, d_fin = t_(np.asarray([tok], np.int32)), t_(np.asarray([4], np.int32)), t_(np.asarray([4], np.int32)), t_(np.zeros(1, np.int32))
    L.kr_logprobs_topk(ptr(lg), V, V, k, n_part, ptr(pv), ptr(pi), ptr(ms), ptr(d_tok), ptr(d_ctx), ptr(d_plen), ptr(d_fin), ptr(out), ptr(oi),
                       1, 1, KS, 1, 0)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0, 0], oi.cpu().numpy()[0, 0]


@pytest.mark.parametrize("layout", ["static", "shared"])
@pytest.mark.parametrize("V,n_part,k", [(300, 1, 20), (300, 1, 0), (5003, 2, 20), (151936, 64, 5)])
def test_records_are_the_one_row_launchs_and_nothing_else_is_written(L, V, n_part, k, layout):
    st = Step(layout, V, n_part, k)
    want_n = {"static": 0 + 2 + 2, "shared": 0 + 1 + 2 + 4 + 2}[layout]
    assert len(st.recs) == want_n and len({r for _, _, r, _ in st.recs}) == want_n          # the cases named at LAYOUTS
    out, oi = st.launch(L)
    touched = np.zeros((HIST_LEN, st.HB), bool)
    for s, j, row, h in st.recs:
        who = f"{layout}: slot {s}, token {j} on row {row} at h = {h}"
        tok = int(st.hist[h, s])
        ref_v, ref_i = one_row(L, st.logits[row], tok, n_part, k)
        np.testing.assert_array_equal(u32(out[h, COL0 + s]), u32(ref_v), err_msg=who + ": values, bit for bit")
        np.testing.assert_array_equal(oi[h, COL0 + s], ref_i, err_msg=who + ": ids")
        touched[h, COL0 + s] = True
        # ... and the oracle, in float64
        lp = O.log_softmax(st.logits[row])
        if 0 <= tok < V:
            np.testing.assert_allclose(out[h, COL0 + s, 0], lp[tok], rtol=1e-5, atol=5e-5, err_msg=who)
        else:
            assert out[h, COL0 + s, 0] == -np.inf, who + ": a token outside the vocabulary"
        ids, vals = O.top_logprobs(st.logits[row], k)
        np.testing.assert_array_equal(oi[h, COL0 + s, :k], ids, err_msg=who)
        np.testing.assert_allclose(out[h, COL0 + s, 1:1 + k], vals, rtol=1e-5, atol=5e-5, err_msg=who)
        assert (out[h, COL0 + s, 1 + k:] == LP_FILL).all() and (oi[h, COL0 + s, k:] == ID_FILL).all(), who + ": past k"
    assert (out[~touched] == LP_FILL).all() and (oi[~touched] == ID_FILL).all(), "an entry no plain step would have written"
    # no partial was computed for a row that records nothing
    ms = st.ms.get()
    rec_rows = sorted({r for _, _, r, _ in st.recs})
    idle = np.setdiff1d(np.arange(st.R), rec_rows)
    assert (ms[idle] == -9.0).all() and (st.pv.get()[idle] == -9.0).all() and (st.pi.get()[idle] == -9).all()
    assert not (ms[rec_rows] == -9.0).any()
    # the state is read, never written
    np.testing.assert_array_equal(st.d_ctx.cpu().numpy()[:st.S], st.ctx)
    np.testing.assert_array_equal(st.d_fin.cpu().numpy()[:st.S], st.fin)
    np.testing.assert_array_equal(st.d_before.cpu().numpy(), st.before)
    np.testing.assert_array_equal(st.d_hist.cpu().numpy(), st.hist)


def test_a_step_of_idle_slots_writes_nothing(L):
    """Every slot frozen or finished by its only token: both launches return at once, on NaN logits throughout."""
    st = Step("shared", 300, 1, 5)
    st.d_ctx[:st.S] = t_(st.before + np.asarray([0, 1, 0, 1, 0], np.int32))
    st.d_fin[:st.S] = 1
    st.d_logits.fill_(float("nan"))
    out, oi = st.launch(L)
    assert (out == LP_FILL).all() and (oi == ID_FILL).all() and (st.ms.get() == -9.0).all()


def test_argument_checks_launch_nothing(L):
    st = Step("static", 300, 1, 5)
    lg = ptr(st.d_logits)
    bad = [(st.spec(), st.lp(k_top=21), None, lg, 300, "k must be"), (st.spec(), st.lp(n_part=0), None, lg, 300, "slice"),
           (st.spec(vocab=4097), st.lp(), None, lg, 4097, "slice"), (st.spec(), st.lp(n_part=1024, k_top=20), None, lg, 300, "LDS"),
           (st.spec(), st.lp(ctx_before=None), None, lg, 300, "null"), (st.spec(), st.lp(out_lp=None), None, lg, 300, "null"),
           (st.spec(), st.lp(), None, None, 300, "null"), (st.spec(), st.lp(), None, lg, 299, "bad sizes"),
           (st.spec(rows=8), st.lp(), None, lg, 300, "rows"), (st.spec(slots=17), st.lp(), ptr(st.d_i), lg, 300, "slots"),
           (st.spec(), st.lp(hist_batch=2), None, lg, 300, "bad sizes")]
    for a, p, m, logits, ld, why in bad:
        with pytest.raises(KarantaHipError, match=why):
            L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), m, logits, ld, 0)
    with pytest.raises(KarantaHipError, match="null ctx_before"):
        L.kr_spec_mark(C.byref(st.spec()), None, 0)
    with pytest.raises(KarantaHipError, match="rows"):
        L.kr_logits_restore_rows(lg, 300, 300, ptr(st.d_i), ptr(st.d_i), ptr(st.d_f), 33, ptr(st.d_i), 3, 0)
    torch.cuda.synchronize()
    assert (st.out.get() == LP_FILL).all() and (st.oi.get() == ID_FILL).all() and (st.ms.get() == -9.0).all()


def test_spec_mark_writes_ctx_before_and_nothing_else(L):
    st = Step("shared", 300, 1, 5)
    mark = Guarded(np.full(st.S, -9, np.int32))
    ctx0, fin0, hist0 = st.d_ctx.cpu().numpy().copy(), st.d_fin.cpu().numpy().copy(), st.d_hist.cpu().numpy().copy()
    L.kr_spec_mark(C.byref(st.spec()), mark.ptr, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mark.get(), st.ctx)
    np.testing.assert_array_equal(st.d_ctx.cpu().numpy(), ctx0)
    np.testing.assert_array_equal(st.d_fin.cpu().numpy(), fin0)
    np.testing.assert_array_equal(st.d_hist.cpu().numpy(), hist0)
    assert (st.d_i.cpu().numpy() == 0).all() and (st.d_f.cpu().numpy() == 0).all()


@pytest.mark.parametrize("V", [300, 5003])
def test_restore_rows_gives_back_the_lm_heads_bits(L, V):
    """17 rows of 5 slots under a map that is not monotonic (two entries outside 0..slots-1: clamped as in kr_logits_adjust_rows);
    slot 1 has no table, slot 2 masks its stop entries (min_tokens), slot 4 has an id outside the vocabulary and a count above the
    table's width.  After adjust + restore every row holds its bits again, one NaN row included, and nothing else was written."""
    S, R = 5, 17
    rng = np.random.default_rng(V)
    logits = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    logits[13] = np.nan                                            # (a row of slot 2)
    entries = lambda n, stop: [(int(i), float(v), int(stop and e % 2)) for e, (i, v) in
                               enumerate(zip(rng.choice(V, n, replace=False), rng.uniform(-8, 8, n)))]
    ids, vals, flags, meta = A.tables(S, [(entries(40, False), 0), ([], 0), (entries(9, True), 50), (entries(min(ADJ_CAP, V // 2), True), 0),
                                          (entries(5, False), 0)])
    ids[4, 2] = V + 7
    ids[4, 5:] = V + 9                                             # (past the five entries: skipped, so every id still occurs once)
    meta[4, 0] = ADJ_CAP + 9                                       # counts as ADJ_CAP
    row_slot = np.asarray([0, 1, 2, 3, 4, 3, 0, 4, 2, 1, 4, 7, -2, 2, 0, 3, 1], np.int32)
    ctx, plen = rng.integers(20, 40, R).astype(np.int32), np.full(R, 10, np.int32)
    lg = Guarded(logits, fill=-5)
    saved = Guarded(np.full((R, ADJ_CAP), -9.0, np.float32))
    dv = [t_(x) for x in (ids, vals, flags, meta, ctx, plen, row_slot)]
    d_ids, d_vals, d_flags, d_meta, d_ctx, d_plen, d_slot = dv
    L.kr_logits_adjust_rows(lg.ptr, V, V, ptr(d_ids), ptr(d_vals), ptr(d_flags), ptr(d_meta), ptr(d_ctx), ptr(d_plen), saved.ptr, R,
                            ptr(d_slot), S, 0)
    torch.cuda.synchronize()
    mid = lg.get().copy()
    changed = [r for r in range(R) if not np.array_equal(u32(mid[r]), u32(logits[r]))]
    assert set(changed) >= {0, 2, 3, 4, 5, 6, 7, 8} and 1 not in changed and 16 not in changed       # the adjust launch did its work
    sv = saved.get().copy()
    L.kr_logits_restore_rows(lg.ptr, V, V, ptr(d_ids), ptr(d_meta), saved.ptr, R, ptr(d_slot), S, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(lg.get()), u32(logits), err_msg="every row holds the lm_head's bits again")
    np.testing.assert_array_equal(u32(saved.get()), u32(sv), err_msg="saved is read, never written")
    for t, src in zip(dv, (ids, vals, flags, meta, ctx, plen, row_slot)):
        np.testing.assert_array_equal(t.cpu().numpy(), src)
