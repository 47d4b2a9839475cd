"""The launches that let requests with sampling controls and logit adjustments take part in a speculative decode step, through the
C-ABI on a real MI355X (include/karanta_hip.h): the row-mapped logit passes kr_logits_adjust_rows, kr_sample_threshold_rows and
kr_gumbel_argmax_processed_rows against the launches they share a body with — per row a one-row batch of kr_logits_adjust,
kr_sample_threshold and kr_gumbel_argmax_processed that holds the slot's params, prompt bits and table and the counts
counts[slot] + bincount(d_1..d_depth) — and the three integer launches kr_spec_controls_trim / _rows / _count against the numpy
restatement in tests/spec_controls_ref.py.  Every comparison is an integer or bit equality and every output lies between guard words.
(Fails on a tree without the feature: the library exports none of the six.)"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import ADJ_CAP, SpecControls, lib, ptr  # noqa: E402
from tests import adjust_cases as A  # noqa: E402
from tests import spec_controls_ref as X  # noqa: E402
from tests import spec_deal_ref as D  # noqa: E402
from tests import spec_ref as R  # noqa: E402
from tests.sampling_rows import DEV, V_PROD, d, pick, prod_batch  # noqa: E402
from tests.test_gpu_spec_guide_kernels import Guarded  # noqa: E402
from tests.test_gpu_spec_kernels import SpecState, bits  # noqa: E402

PAD, EOS = 3, 7
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def set_bits(words, idx):
    idx = np.asarray(idx, np.int64)
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))


# ----------------------------------------------------------------------------- the row-mapped logit passes
class Batch:
    """S slots (params, counts, prompt bits, adjustment tables, drafts [S, K]) and R rows (slot, depth, logits, temperature, seed,
    ctx_len, prompt_len, finished, guide mask address, guide state)."""

    def __init__(self, V, K, params, counts, pbits, tables, drafts, row_slot, depth, logits, temps, seeds, ctx, plen, fin, gm=None,
                 gstate=None, keep=()):
        self.V, self.K, self.S, self.R = V, K, len(params), len(row_slot)
        self.params, self.counts, self.pbits = np.asarray(params, np.float32), np.asarray(counts, np.int32), np.asarray(pbits, np.uint32)
        self.ids, self.vals, self.flags, self.meta = tables
        self.drafts, self.row_slot, self.depth = np.asarray(drafts, np.int32), np.asarray(row_slot, np.int32), np.asarray(depth, np.int32)
        self.logits, self.temps, self.seeds = np.asarray(logits, np.float32), np.asarray(temps, np.float32), np.asarray(seeds, np.uint32)
        self.ctx, self.plen, self.fin = np.asarray(ctx, np.int32), np.asarray(plen, np.int32), np.asarray(fin, np.int32)
        self.gm = np.zeros(self.R, np.int64) if gm is None else np.asarray(gm, np.int64)
        self.gstate = np.zeros(self.R, np.int32) if gstate is None else np.asarray(gstate, np.int32)
        self.keep = keep            # device tensors the mask addresses point into
        self.mask_words = 2 * ((V + 63) // 64)
        self.W = self.pbits.shape[1]

    def row_counts(self, r, extras=True):
        s = int(self.row_slot[r])
        return X.effective_counts(self.counts[s], self.drafts[s], int(self.depth[r]) if extras else 0)

    def launch_rows(self, L, n_part, flags=2):
        """The three row-mapped launches over all rows; every output between guard words."""
        V, R, S, K = self.V, self.R, self.S, self.K
        lg = Guarded(self.logits, fill=-5)
        saved = Guarded(np.full((R, ADJ_CAP), -9.0, np.float32))
        work = Guarded(np.full((R, V), -9.0, np.float32))
        thr, live = Guarded(np.full(R, -9, np.int32)), Guarded(np.full(R, -9, np.int32))
        av, ai = Guarded(np.full((R, n_part), -9.0, np.float32)), Guarded(np.full((R, n_part), -9, np.int32))
        dv = {k: d(v) for k, v in dict(temps=self.temps, seeds=self.seeds.view(np.int32), params=self.params, counts=self.counts,
                                       pbits=self.pbits.view(np.int32), ids=self.ids, vals=self.vals, flags=self.flags, meta=self.meta,
                                       drafts=self.drafts, slot=self.row_slot, depth=self.depth, ctx=self.ctx, plen=self.plen,
                                       fin=self.fin, gm=self.gm, gstate=self.gstate).items()}
        gm = ptr(dv["gm"]) if self.gm.any() else None
        L.kr_logits_adjust_rows(lg.ptr, V, V, ptr(dv["ids"]), ptr(dv["vals"]), ptr(dv["flags"]), ptr(dv["meta"]), ptr(dv["ctx"]),
                                ptr(dv["plen"]), saved.ptr, R, ptr(dv["slot"]), S, 0)
        L.kr_sample_threshold_rows(lg.ptr, V, V, ptr(dv["temps"]), ptr(dv["params"]), ptr(dv["counts"]), V, ptr(dv["pbits"]), self.W, gm,
                                   ptr(dv["gstate"]), self.mask_words, ptr(dv["fin"]), flags, work.ptr, V, thr.ptr, live.ptr, R,
                                   ptr(dv["slot"]), ptr(dv["depth"]), ptr(dv["drafts"]), K, S, 0)
        L.kr_gumbel_argmax_processed_rows(lg.ptr, V, V, ptr(dv["temps"]), ptr(dv["seeds"]), ptr(dv["ctx"]), ptr(dv["plen"]), av.ptr,
                                          ai.ptr, n_part, R, gm, ptr(dv["gstate"]), self.mask_words, EOS, ptr(dv["params"]),
                                          ptr(dv["counts"]), V, ptr(dv["pbits"]), self.W, thr.ptr, ptr(dv["slot"]), ptr(dv["depth"]),
                                          ptr(dv["drafts"]), K, S, 0)
        torch.cuda.synchronize()
        # the inputs the launches only read
        for name, src in (("counts", self.counts), ("params", self.params), ("drafts", self.drafts), ("depth", self.depth)):
            np.testing.assert_array_equal(dv[name].cpu().numpy(), src, err_msg=f"{name} is read, never written")
        return dict(logits=lg.get(), saved=saved.get(), thr=thr.get(), live=live.get(), av=av.get(), ai=ai.get())

    def launch_one(self, L, r, n_part, flags=2, extras=True):
        """Row r through the existing launches as a one-row batch holding its slot's state and the counts behind its drafts."""
        V, s = self.V, int(self.row_slot[r])
        one = lambda a: d(np.ascontiguousarray(a[None]))
        lg, saved = one(self.logits[r]), torch.full((1, ADJ_CAP), -9.0, device=DEV)
        work, thr, live = torch.full((1, V), -9.0, device=DEV), one(np.int32(-9)), one(np.int32(-9))
        av, ai = torch.full((1, n_part), -9.0, device=DEV), torch.full((1, n_part), -9, dtype=torch.int32, device=DEV)
        t = [one(x) for x in (self.ids[s], self.vals[s], self.flags[s], self.meta[s], self.ctx[r], self.plen[r], self.temps[r],
                              self.seeds.view(np.int32)[r], self.params[s], self.row_counts(r, extras), self.pbits.view(np.int32)[s],
                              self.fin[r], self.gm[r], self.gstate[r])]
        ids, vals, fl, meta, ctx, plen, temp, seed, prm, cnt, pb, fin, gm_, gs = t
        gm = ptr(gm_) if self.gm[r] else None
        L.kr_logits_adjust(ptr(lg), V, V, ptr(ids), ptr(vals), ptr(fl), ptr(meta), ptr(ctx), ptr(plen), ptr(saved), 1, 0)
        L.kr_sample_threshold(ptr(lg), V, V, ptr(temp), ptr(prm), ptr(cnt), V, ptr(pb), self.W, gm, ptr(gs), self.mask_words, ptr(fin),
                              flags, ptr(work), V, ptr(thr), ptr(live), 1, 0)
        L.kr_gumbel_argmax_processed(ptr(lg), V, V, ptr(temp), ptr(seed), ptr(ctx), ptr(plen), ptr(av), ptr(ai), n_part, 1, gm, ptr(gs),
                                     self.mask_words, EOS, ptr(prm), ptr(cnt), V, ptr(pb), self.W, ptr(thr), 0)
        torch.cuda.synchronize()
        return dict(logits=lg.cpu().numpy()[0], saved=saved.cpu().numpy()[0], thr=thr.cpu().numpy()[0], live=live.cpu().numpy()[0],
                    av=av.cpu().numpy()[0], ai=ai.cpu().numpy()[0])


def compare(L, bt, n_part, label):
    """Every row of the row-mapped launches equals its one-row reference, bit for bit.  Returns (rows output, per-row tokens, per
    row (threshold, token) of the same row computed with the slot's counts alone)."""
    got = bt.launch_rows(L, n_part)
    toks = pick(got["av"], got["ai"])
    alone = []
    for r in range(bt.R):
        ref = bt.launch_one(L, r, n_part)
        who = f"{label}: row {r} (slot {bt.row_slot[r]}, depth {bt.depth[r]})"
        np.testing.assert_array_equal(u32(got["logits"][r]), u32(ref["logits"]), err_msg=who + ": adjusted logits")
        np.testing.assert_array_equal(u32(got["saved"][r]), u32(ref["saved"]), err_msg=who + ": saved logits")
        assert int(got["thr"][r]) == int(ref["thr"]), who + ": threshold"
        assert int(got["live"][r]) == int(ref["live"]), who + ": live"
        np.testing.assert_array_equal(u32(got["av"][r]), u32(ref["av"]), err_msg=who + ": partial values")
        np.testing.assert_array_equal(got["ai"][r], ref["ai"], err_msg=who + ": partial indices")
        if bt.depth[r] > 0:
            base = bt.launch_one(L, r, n_part, extras=False)
            alone.append((r, int(base["thr"]) != int(ref["thr"]), int(pick(base["av"][None], base["ai"][None])[0]) != int(toks[r])))
    return got, toks, alone


def small_batch():
    """V = 1003 (no multiple of 32 or of 4 * n_part = 32), 5 slots, K = 3, 17 rows under a map that is not monotonic."""
    V, K, S = 1003, 3, 5
    rng = np.random.default_rng(77)
    base = (rng.standard_normal((S, V)) * 3).astype(np.float32)
    top = [np.argsort(-base[s]) for s in range(S)]
    # (top_k, top_p, min_p, repetition, frequency, presence) and temperature per slot
    params = np.zeros((S, 8), np.float32)
    params[:, :6] = [(0, 0.8, 0, 1.3, 0.5, 0), (0, 1, 0, 1, 1.5, 0.5), (0, 1, 0, 1, 0, 0), (5, 1, 0, 1.2, 0, 1.0), (0, 1, 0.05, 1, 0, 0)]
    temp_s = [1.0, 0.0, 0.9, 1.0, 0.7]
    W = (V + 31) // 32
    counts, pbits = np.zeros((S, V), np.int32), np.zeros((S, W), np.uint32)
    for s in range(S):
        counts[s] = np.bincount(np.r_[rng.integers(0, V, 12), top[s][3:5]], minlength=V)
        set_bits(pbits[s], np.r_[rng.integers(0, V, 20), top[s][1:2]])
    # the drafts: the slot's best token twice (count + 2 at depth 2), then its second best, a prompt token
    drafts = np.asarray([[top[s][0], top[s][0], top[s][1]] for s in range(S)], np.int32)
    n_slot = np.asarray([2, 5, 1, 3, 4], np.int32)               # generated tokens so far
    plen_s = np.asarray([7, 9, 6, 8, 5], np.int32)
    assert base[1][top[1][0]] - base[1][top[1][1]] < 3.0       # two more copies of the best token cost it 2 x 1.5 + 0.5
    tables = A.tables(S, [([], 0), ([(int(top[1][40]), 1.0, 0)], 0), ([], 0), ([(int(top[3][2]), 4.0, 0), (int(top[3][6]), 0.0, 1)], 0),
                          # slot 4: min_tokens = n + 1: its own row masks the stop entries, the row behind one draft does not
                          ([(EOS, 0.0, 1), (int(top[4][0]), 2.0, 1), (int(top[4][3]), 1.0, 0)], int(n_slot[4]) + 1)])
    # row -> (slot, depth); -1: parked (slot 0, depth 0, s_max - 1, finished, greedy)
    rows = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 2), (0, 1), (0, 3), (3, 2), (1, 1), (2, 2), (4, 1), (-1, 0), (0, 2), (-1, 0),
            (4, 3), (-1, 0)]
    R_ = len(rows)
    s_max = 512
    slot = np.asarray([max(s, 0) for s, _ in rows], np.int32)
    depth = np.asarray([j for _, j in rows], np.int32)
    parked = np.asarray([s < 0 for s, _ in rows])
    logits = base[slot].copy()
    temps = np.where(parked, 0.0, np.asarray(temp_s, np.float32)[slot]).astype(np.float32)
    seeds = np.where(parked, 0, rng.integers(0, 2 ** 32, S, dtype=np.uint64)[slot]).astype(np.uint32)
    plen = np.where(parked, s_max - 1, plen_s[slot]).astype(np.int32)
    ctx = np.where(parked, s_max - 1, plen_s[slot] + n_slot[slot] - 1 + depth).astype(np.int32)
    fin = parked.astype(np.int32)
    # slot 3 is guided: a random half of the vocabulary in state 1 of a two-state table, its best tokens in and out
    mw = 2 * ((V + 63) // 64)
    allow = rng.random(V) < 0.5
    allow[top[3][:4]] = [False, True, True, True]
    table = np.zeros((2, mw), np.uint32)
    set_bits(table[1], np.flatnonzero(allow))
    mt = d(table.view(np.int32))
    gm = np.where(slot == 3, mt.data_ptr(), 0).astype(np.int64)
    gm[parked] = 0
    gstate = np.where(slot == 3, 1, 0).astype(np.int32)
    return Batch(V, K, params, counts, pbits, tables, drafts, slot, depth, logits, temps, seeds, ctx, plen, fin, gm, gstate, keep=(mt,))


def test_rows_equal_one_row_batches_of_the_existing_launches(L):
    """Depth 0 is the slot's own row; a draft repeated twice; a draft that is a prompt token; two and three rows of one slot at
    different depths; a map that is not monotonic; parked rows; a neutral slot; a guided and controlled row; min_tokens per row."""
    bt = small_batch()
    n_part = 8
    assert bt.V % 32 and bt.V % (4 * n_part)
    got, toks, alone = compare(L, bt, n_part, "V = 1003")
    _CACHE["small"] = (bt, got, toks)
    assert any(t for _, t, _ in alone), "no row's threshold depends on its drafts: a kernel that ignores them would pass"
    assert any(k for _, _, k in alone), "no row's token depends on its drafts: a kernel that ignores them would pass"
    # the greedy slot with a frequency penalty: two copies of its best token in front of the row push it off the top
    r = 5
    assert bt.row_slot[r] == 1 and bt.depth[r] == 2 and toks[r] != toks[1] and dict((a, k) for a, _, k in alone)[r]
    # the slot's own rows read no draft: the same launch with other drafts gives them the same bits
    other = Batch(bt.V, bt.K, bt.params, bt.counts, bt.pbits, (bt.ids, bt.vals, bt.flags, bt.meta), bt.drafts[:, ::-1] + 1, bt.row_slot,
                  bt.depth, bt.logits, bt.temps, bt.seeds, bt.ctx, bt.plen, bt.fin, bt.gm, bt.gstate, keep=bt.keep)
    got2 = other.launch_rows(L, n_part)
    own = np.flatnonzero(bt.depth == 0)
    np.testing.assert_array_equal(u32(got2["av"][own]), u32(got["av"][own]))
    np.testing.assert_array_equal(got2["ai"][own], got["ai"][own])
    np.testing.assert_array_equal(got2["thr"][own], got["thr"][own])
    # min_tokens is per row: slot 4's own row masks its stop entries, its row behind one draft gets their bias
    s4 = [int(t) for t in bt.ids[4][:3]]
    assert np.isneginf(got["logits"][4][s4[:2]]).all() and np.isfinite(got["logits"][11][s4]).all()
    assert np.isfinite(got["logits"][4][s4[2]])
    # live is per row
    np.testing.assert_array_equal(got["live"], 1 - bt.fin)


def test_a_neutral_slots_rows_get_the_guided_launchs_partials(L):
    """Rows of the slot with neutral params, at depth 0 and 2: the partials of kr_gumbel_argmax_guided, bit for bit."""
    bt, got, _ = _CACHE["small"] if "small" in _CACHE else (small_batch(), None, None)
    n_part = 8
    if got is None:
        got = bt.launch_rows(L, n_part)
    rows = [r for r in range(bt.R) if bt.row_slot[r] == 2 and bt.temps[r] > 0]
    assert [int(bt.depth[r]) for r in rows] == [0, 2]
    V = bt.V
    lg, temps, seeds, ctx, plen = (d(got["logits"][rows]), d(bt.temps[rows]), d(bt.seeds.view(np.int32)[rows]), d(bt.ctx[rows]),
                                   d(bt.plen[rows]))
    av = torch.zeros(len(rows), n_part, device=DEV)
    ai = torch.zeros(len(rows), n_part, dtype=torch.int32, device=DEV)
    L.kr_gumbel_argmax_guided(ptr(lg), V, V, ptr(temps), ptr(seeds), ptr(ctx), ptr(plen), ptr(av), ptr(ai), n_part, len(rows), None, None,
                              0, 0, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(got["av"][rows]), u32(av.cpu().numpy()))
    np.testing.assert_array_equal(got["ai"][rows], ai.cpu().numpy())
    assert (got["thr"][rows] == 0).all()


def test_the_production_rows_on_eight_slots_at_depths_0_to_3(L):
    """The 32 Gaussian rows at the production vocabulary: row r is (slot r % 8, depth r // 8); the slots carry the penalties and the
    truncation of eight of the batch's rows, every row its own logits, and a slot's drafts are the best tokens of its rows."""
    rng = np.random.default_rng(21)
    logits, temps, params, prompts, outs, counts, pbits, spec = prod_batch(rng)
    V, K, S = V_PROD, 3, 8
    src = [18, 19, 20, 24, 30, 16, 21, 8]          # penalties (two of them greedy or hot), truncation alone, a neutral row
    slot, depth = np.arange(32) % S, np.arange(32) // S
    drafts = np.asarray([[int(np.argmax(logits[j * S + s])) for j in range(1, K + 1)] for s in range(S)], np.int32)
    drafts[0, 0] = drafts[0, 1]                      # slot 0: a draft repeated twice in front of its depth-2 row's favourite
    plen_s = np.full(S, 90, np.int32)
    n_slot = rng.integers(5, 60, S).astype(np.int32)
    tables = A.tables(S, [([], 0)] * 5 + [([(int(np.argmax(logits[5])), -100.0, 0), (EOS, 0.0, 1)], int(n_slot[5]) + 2), ([], 0),
                          ([(int(np.argmax(logits[15])), 3.0, 1)], 0)])
    bt = Batch(V, K, params[src], counts[src], pbits[src], tables, drafts, slot, depth, logits, temps[src][slot],
               rng.integers(0, 2 ** 32, S, dtype=np.uint64)[slot], plen_s[slot] + n_slot[slot] - 1 + depth, plen_s[slot], np.zeros(32, np.int32))
    got, toks, alone = compare(L, bt, 64, "production vocabulary")
    assert any(t for _, t, _ in alone) and any(k for _, _, k in alone)
    assert (got["thr"][slot == 6] == 0).all(), "the neutral slot's rows are not truncated"


# ----------------------------------------------------------------------------- the three integer launches
# per kind of slot: (table entries, min_tokens, drafts, finished)
STOP, STOP2, BIAS = 50, 60, 70
TABLE = [(STOP, 0.0, 1), (STOP2, 2.0, 1), (BIAS, -5.0, 0)]
KINDS = [
    (TABLE, 0, [10, 11, 12], 0),            # 0 no stop id among the drafts
    (TABLE, 0, [STOP, 11, 12], 0),          # 1 a stop id at depth 1
    (TABLE, 0, [10, STOP2, 12], 0),         # 2 ... at depth 2
    (TABLE, 0, [10, 11, STOP], 0),          # 3 ... at depth 3
    ([], 0, [STOP, STOP2, EOS], 0),         # 4 an unadjusted slot: everything stays
    (TABLE, 0, [STOP, 11, 12], 1),          # 5 finished
    ([(EOS, 0.0, 1)], 9, [10, EOS, 12], 0),  # 6 min_tokens: the EOS is a stop entry
    (TABLE, 0, [BIAS, BIAS, BIAS], 0),      # 7 a biased token that is no stop entry
    (TABLE, 0, [10, STOP2, STOP], 0),       # 8 two stop ids: the first decides
]
PICK = {(5, 3, 20): [2, 4, 5, 6, 0], (4, 1, 17): [1, 0, 4, 7], (3, 3, 17): [3, 8, 0],
        (20, 3, 32): [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 0, 4, 7, 1, 0, 2, 0, 3, 0, 0]}
V_INT = 300


def setup(B, K, rows):
    kinds = [KINDS[i] for i in PICK[(B, K, rows)]]
    seqs = []
    for b, (_, _, drafts, fin) in enumerate(kinds):
        gen = [20 + b] * (1 + b % 3)
        seqs.append(([1, 2, 3 + b], gen, fin, gen + drafts[:K]))
    st = SpecState(seqs, K, rows, vocab=V_INT, pad=PAD, seed=B)
    ids, vals, flags, meta = A.tables(B, [(k[0], k[1]) for k in kinds])
    assert ids.shape[1] == ADJ_CAP
    bufs = {"before": Guarded(np.full(B, -9, np.int32)), "count": Guarded(np.full(B, -9, np.int32)),
            "draft": Guarded(np.full((B, K), -9, np.int32)), "depth": Guarded(np.full(rows, -9, np.int32)),
            "fin": Guarded(np.concatenate([st.fin, np.full(rows - B, -5, np.int32)])), "row": Guarded(np.full((B, K), -9, np.int32)),
            "counts": Guarded(np.zeros((B, V_INT), np.int32))}
    dev = [d(x) for x in (ids, flags, meta)]
    a = st.args()
    a.draft_tok, a.finished = bufs["draft"].ptr, bufs["fin"].ptr
    c = SpecControls(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), bufs["counts"].ptr, V_INT, bufs["depth"].ptr, bufs["before"].ptr)
    return st, (ids, flags, meta), dev, bufs, a, c


@pytest.mark.parametrize("B,K,rows", [(5, 3, 20), (4, 1, 17)])
def test_trim_and_rows_in_the_static_layout(L, B, K, rows):
    st, (ids, flags, meta), dev, bufs, a, c = setup(B, K, rows)
    a.n_draft = bufs["count"].ptr
    L.kr_spec_propose(C.byref(a), 0)
    ref = R.propose(st.prompts, st.hist, st.ctx, st.plen, st.fin, st.temp, st.seed, K, rows, st.n_min, st.n_max, st.s_max, PAD, V_INT,
                    scripts=st.scripts)
    np.testing.assert_array_equal(bufs["count"].get(), ref["n_draft"])
    np.testing.assert_array_equal(bufs["draft"].get(), ref["draft_tok"])
    # ---- trim
    L.kr_spec_controls_trim(C.byref(a), C.byref(c), bufs["count"].ptr, 0)
    n, tok_, before = X.trim(ids, flags, meta, st.fin, st.ctx, ref["n_draft"], ref["draft_tok"], PAD)
    np.testing.assert_array_equal(bufs["count"].get(), n, err_msg="n_draft")
    np.testing.assert_array_equal(bufs["draft"].get(), tok_, err_msg="draft_tok")
    np.testing.assert_array_equal(bufs["before"].get(), before, err_msg="ctx_before")
    np.testing.assert_array_equal(bufs["fin"].get(), ref["fin"], err_msg="the trim writes no finished")
    kept = [b for b in range(B) if meta[b, 0] == 0 or st.fin[b]]
    assert kept and all(n[b] == ref["n_draft"][b] and (tok_[b] == ref["draft_tok"][b]).all() for b in kept)
    assert (n < ref["n_draft"]).any()
    # ---- rows
    L.kr_spec_controls_rows(C.byref(a), C.byref(c), None, 0)
    depth, want_fin = X.depth_rows(ref["fin"], n, B, K, rows)
    np.testing.assert_array_equal(bufs["depth"].get(), depth, err_msg="depth")
    np.testing.assert_array_equal(bufs["fin"].get(), want_fin, err_msg="finished")
    assert (want_fin[B:B * (K + 1)] != ref["fin"][B:B * (K + 1)]).any(), "a trimmed draft's row is finished"
    assert int((depth > 0).sum()) == int(n[st.fin == 0].sum()) + int(n[st.fin != 0].sum())
    np.testing.assert_array_equal(bufs["count"].get(), n, err_msg="n_draft after the rows")
    np.testing.assert_array_equal(bufs["draft"].get(), tok_, err_msg="draft_tok after the rows")
    np.testing.assert_array_equal(bufs["counts"].get(), 0, err_msg="neither launch writes the counts")


@pytest.mark.parametrize("B,K,rows", [(3, 3, 17), (20, 3, 32)])
def test_trim_deal_and_rows_with_shared_rows(L, B, K, rows):
    st, (ids, flags, meta), dev, bufs, a, c = setup(B, K, rows)
    nd = Guarded(np.full(B, -9, np.int32))
    a.n_draft = nd.ptr
    L.kr_spec_lookup(C.byref(a), bufs["count"].ptr, 0)
    n_want, tok0 = D.lookup(st.prompts, st.hist, st.ctx, st.plen, st.fin, K, st.n_min, st.n_max, st.s_max, PAD, V_INT, st.scripts)
    np.testing.assert_array_equal(bufs["count"].get(), n_want)
    # ---- trim, between the lookup and the deal
    L.kr_spec_controls_trim(C.byref(a), C.byref(c), bufs["count"].ptr, 0)
    n, tok_, before = X.trim(ids, flags, meta, st.fin, st.ctx, n_want, tok0, PAD)
    np.testing.assert_array_equal(bufs["count"].get(), n, err_msg="n_want")
    np.testing.assert_array_equal(bufs["draft"].get(), tok_, err_msg="draft_tok")
    np.testing.assert_array_equal(bufs["before"].get(), before, err_msg="ctx_before")
    assert (n < n_want).any()
    # ---- the deal on the trimmed counts
    L.kr_spec_deal(C.byref(a), bufs["count"].ptr, bufs["row"].ptr, 0)
    deal = D.deal(n, tok_, st.ctx, st.plen, st.fin, st.temp, st.seed, K, rows, st.s_max, PAD)
    np.testing.assert_array_equal(bufs["row"].get(), deal["draft_row"], err_msg="draft_row")
    np.testing.assert_array_equal(nd.get(), deal["n_draft"], err_msg="n_draft")
    if (B, K, rows) == (20, 3, 32):
        # slot 1's depth-1 draft is a stop id: the row it would have taken goes to a slot that would have got none
        untrimmed = D.deal_rows(n_want, [not f for f in st.fin], K, rows)
        assert n_want[1] == K and n[1] == 0 and untrimmed[1, 0] >= B and deal["draft_row"][1, 0] == -1
        gained = [b for b in range(B) if (deal["draft_row"][b] >= 0).sum() > (untrimmed[b] >= 0).sum()]
        assert gained, "a trimmed draft must free a row for another slot"
        assert (deal["n_draft"] < n).any(), "the budget binds"
    # ---- rows
    L.kr_spec_controls_rows(C.byref(a), C.byref(c), bufs["row"].ptr, 0)
    depth, want_fin = X.depth_rows(deal["fin"], deal["n_draft"], B, K, rows, draft_row=deal["draft_row"])
    np.testing.assert_array_equal(bufs["depth"].get(), depth, err_msg="depth")
    np.testing.assert_array_equal(bufs["fin"].get(), deal["fin"], err_msg="with a dealt map `finished` is the deal's")
    np.testing.assert_array_equal(want_fin, deal["fin"])
    assert (depth > 0).any() and int((depth > 0).sum()) == int(deal["n_draft"].sum())
    np.testing.assert_array_equal(bufs["row"].get(), deal["draft_row"], err_msg="draft_row after the rows")


def test_rows_with_a_map_that_is_not_monotonic(L):
    """kr_spec_controls_rows on a map written by hand: a slot's deeper draft on a lower row, an entry beyond the dealt depth."""
    B, K, rows = 3, 3, 17
    st, _, dev, bufs, a, c = setup(B, K, rows)
    nd = d(np.asarray([2, 0, 1], np.int32))
    a.n_draft = ptr(nd)
    row = np.asarray([[9, 4, 12], [-1, -1, -1], [3, 16, -1]], np.int32)
    bufs["row"] = Guarded(row)
    L.kr_spec_controls_rows(C.byref(a), C.byref(c), bufs["row"].ptr, 0)
    depth, _ = X.depth_rows(np.zeros(rows, np.int32), [2, 0, 1], B, K, rows, draft_row=row)
    assert depth.tolist() == [0, 0, 0, 1, 2, 0, 0, 0, 0, 1] + [0] * 7
    np.testing.assert_array_equal(bufs["depth"].get(), depth)


def test_count_follows_the_emitted_tokens(L):
    """Emitted counts 0 (a frozen finished slot), 1, K + 1 with one token twice, a step that ends on a stop id and one on the EOS
    (both counted), on counts that are not zero."""
    K, rows = 3, 32
    plan = [([5], [], 1), ([5, 6], [8], 0), ([9], [6, 1, 6, 2], 0), ([9, 9], [4, STOP], 1), ([9], [EOS], 1), ([1, 2, 3], [7, 7], 0)]
    B = len(plan)
    seqs = [([1, 2, 3 + b], gen + em, fin, None) for b, (gen, em, fin) in enumerate(plan)]
    st = SpecState(seqs, K, rows, vocab=V_INT, pad=PAD)
    before = np.asarray([st.ctx[b] - len(plan[b][1]) for b in range(B)], np.int32)
    rng = np.random.default_rng(3)
    counts0 = rng.integers(0, 3, (B, V_INT)).astype(np.int32)
    ids, vals, flags, meta = A.tables(B, [(TABLE, 0)] * B)
    dev = [d(x) for x in (ids, flags, meta)]
    bufs = {"counts": Guarded(counts0), "before": Guarded(before), "depth": Guarded(np.full(rows, -9, np.int32))}
    a = st.args()
    c = SpecControls(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), bufs["counts"].ptr, V_INT, bufs["depth"].ptr, bufs["before"].ptr)
    L.kr_spec_controls_count(C.byref(a), C.byref(c), 0)
    want = X.count_update(counts0, before, st.ctx, st.plen, st.hist, K)
    delta = want - counts0
    assert [int(x.sum()) for x in delta] == [0, 1, 4, 2, 1, 2] and delta[2, 6] == 2 and delta[3, STOP] == 1 and delta[4, EOS] == 1
    np.testing.assert_array_equal(bufs["counts"].get(), want)
    np.testing.assert_array_equal(bufs["before"].get(), before)
    np.testing.assert_array_equal(bufs["depth"].get(), -9)
    np.testing.assert_array_equal(bits(st.d_hist), st.hist)
    np.testing.assert_array_equal(bits(st.d_ctx)[:B], st.ctx)
