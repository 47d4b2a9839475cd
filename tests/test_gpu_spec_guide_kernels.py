"""The three launches that let guided slots take part in a speculative decode step (include/karanta_hip.h: kr_spec_guide_trim,
kr_spec_guide_rows, kr_spec_guide_advance) through the C-ABI on a real MI355X, behind the real kr_spec_propose / kr_spec_lookup /
kr_spec_deal, against the numpy restatement in tests/spec_guide_ref.py.  All quantities are integers and every comparison is an
equality; every output array lies between guard words.  (Fails on a tree without the feature: the library exports none of the
three.)"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import SpecGuide, lib, ptr  # noqa: E402
from karanta_ocr_amd.guided import pack_vocab  # noqa: E402
from tests import spec_deal_ref as D  # noqa: E402
from tests import spec_guide_ref as G  # noqa: E402
from tests import spec_ref as R  # noqa: E402
from tests.test_gpu_spec_kernels import SpecState, bits, t_  # noqa: E402

PATTERN = r"[a-f]{3}-[0-9]{2}(?:;[a-z ]{2,5})?"
LONG = r"(?:[a-c]{2,3}-[0-9]{2};){1,4}"
TB = G.synthetic_vocab(300)
V, PAD, EOS, SPECIAL = len(TB), 3, G.EOS, G.SPECIAL
MASK_WORDS = 2 * ((V + 63) // 64)
GUARD = 8
_T = {}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def tables(L):
    """The two patterns on the device, once: DFA tables, the masks kr_guide_build_masks writes, the packed vocabulary."""
    if not _T:
        off, flat = pack_vocab(TB)
        _T["off"], _T["bytes"], _T["eos"] = t_(off), t_(flat), t_(np.asarray([EOS], np.int32))
        _T["pats"], _T["trans"], _T["masks"] = [G.Pattern(PATTERN, TB, (EOS,)), G.Pattern(LONG, TB, (EOS,))], [], []
        for p in _T["pats"]:
            S = p.guide.n_states
            tr = t_(np.ascontiguousarray(p.guide.trans).view(np.int16))
            ac = t_(np.ascontiguousarray(p.guide.accept).astype(np.uint8))
            mk = torch.zeros(S, MASK_WORDS, dtype=torch.int32, device="cuda:0")
            L.kr_guide_build_masks(ptr(tr), ptr(ac), S, ptr(_T["off"]), ptr(_T["bytes"]), V, ptr(_T["eos"]), 1, ptr(mk), MASK_WORDS, 0)
            _T["trans"].append(tr)
            _T["masks"].append(mk)
    return _T


def test_the_restatements_mask_is_the_devices(L):
    """The bit kr_gumbel_argmax_guided tests, and the trim with it: word t >> 5, bit t & 31 of the state's row."""
    T = tables(L)
    for p, mk in zip(T["pats"], T["masks"]):
        words = bits(mk).view(np.uint32)
        got = ((words[:, np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1).astype(bool)
        np.testing.assert_array_equal(got, p.mask)


class Guarded:
    """A device array between guard words; `get` checks them."""

    def __init__(self, arr, fill=-5):
        arr = np.asarray(arr)
        self.shape, self.fill = arr.shape, fill
        g = np.full(GUARD, fill, arr.dtype)
        self.t = t_(np.concatenate([g, arr.ravel(), g]))

    @property
    def ptr(self):
        return self.t[GUARD:].data_ptr()

    def get(self):
        b = bits(self.t)
        assert (b[:GUARD] == self.fill).all() and (b[-GUARD:] == self.fill).all(), "a guard word was written"
        return b[GUARD:-GUARD].reshape(self.shape)


def tok(b: bytes) -> int:
    return TB.index(b)


def cases(T):
    """(pattern index or 0, DFA state, drafts, finished) per kind of slot."""
    p1, p2 = T["pats"]
    s1 = lambda text: p1.guide.walk(p1.start, text)
    s2 = lambda text: p2.guide.walk(p2.start, text)
    a, b, c, dash, one = tok(b"a"), tok(b"b"), tok(b"c"), tok(b"-"), tok(b"1")
    return [
        (1, s1(b""), [a, b, c], 0),                               # 0 every draft allowed
        (1, s1(b""), [dash, b, c], 0),                            # 1 forbidden at depth 1
        (1, s1(b""), [a, one, c], 0),                             # 2 ... at depth 2
        (1, s1(b""), [a, b, dash], 0),                            # 3 ... at depth 3
        (1, s1(b""), [tok(b"ab-"), a, a], 0),                     # 4 a multi-byte draft that dies on its last byte
        (1, s1(b"abc-12"), [EOS, a, b], 0),                       # 5 EOS in an accepting state: kept, ends the run
        (1, s1(b"a"), [b, EOS, c], 0),                            # 6 EOS in a non-accepting state: trimmed
        (1, s1(b"abc-12"), [SPECIAL, a, b], 0),                   # 7 no bytes and no EOS: trimmed
        (0, 0, [dash, SPECIAL, EOS], 0),                          # 8 unguided: everything stays
        (2, s2(b"ab"), [a, b, c], 1),                             # 9 finished
        (2, s2(b""), [tok(b"ab"), tok(b"c-"), tok(b"12;")], 0),   # 10 multi-byte drafts, all allowed
        (2, s2(b"ab-12;"), [tok(b"ab-1"), tok(b"2;"), EOS], 0),   # 11 ... and an EOS at depth 3 of an accepting run
    ]


PICK = {(5, 3, 20): [2, 8, 9, 5, 10], (4, 1, 17): [1, 0, 8, 5], (3, 3, 17): [3, 4, 11], (4, 3, 17): [0, 0, 0, 8],
        (20, 3, 32): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0, 10, 8, 1, 9, 2, 11, 0]}


def setup(L, B, K, rows):
    T = tables(L)
    kinds = [cases(T)[i] for i in PICK[(B, K, rows)]]
    seqs = []
    for b, (_, _, drafts, fin) in enumerate(kinds):
        gen = [20 + b] * (1 + b % 3)
        seqs.append(([1, 2, 3 + b], gen, fin, gen + drafts))
    st = SpecState(seqs, K, rows, vocab=V, pad=PAD, seed=B)
    gid = np.asarray([k[0] for k in kinds] + [0] * (rows - B))
    gstate = np.asarray([k[1] for k in kinds] + [-5] * (rows - B), np.int32)
    addr = lambda tabs: np.asarray([0 if g == 0 else tabs[g - 1].data_ptr() for g in gid[:B]] + [-5] * (rows - B), np.int64)
    bufs = {"trans": Guarded(addr(T["trans"])), "masks": Guarded(addr(T["masks"])), "state": Guarded(gstate),
            "dstate": Guarded(np.full((B, K), -9, np.int32)), "before": Guarded(np.full(B, -9, np.int32)),
            "count": Guarded(np.full(B, -9, np.int32)), "draft": Guarded(np.full((B, K), -9, np.int32)),
            "fin": Guarded(np.concatenate([st.fin, np.full(rows - B, -5, np.int32)])),
            "row": Guarded(np.full((B, K), -9, np.int32))}
    a = st.args()
    a.draft_tok, a.finished = bufs["draft"].ptr, bufs["fin"].ptr
    g = SpecGuide(bufs["trans"].ptr, bufs["masks"].ptr, bufs["state"].ptr, MASK_WORDS, ptr(T["off"]), ptr(T["bytes"]),
                  bufs["dstate"].ptr, bufs["before"].ptr)
    return T, st, gid, gstate, bufs, a, g


def addresses(T, gid, name):
    return np.asarray([0 if g == 0 else T[name][int(g) - 1].data_ptr() for g in gid], np.int64)


def check_rows(T, bufs, B, want_gid, want_state, want_fin, gid, gstate):
    """The per-row arrays after kr_spec_guide_rows; entries 0..B-1 are the caller's and unchanged."""
    np.testing.assert_array_equal(bufs["trans"].get()[B:], addresses(T, want_gid[B:], "trans"), err_msg="guide_trans of the draft rows")
    np.testing.assert_array_equal(bufs["masks"].get()[B:], addresses(T, want_gid[B:], "masks"), err_msg="guide_masks of the draft rows")
    np.testing.assert_array_equal(bufs["state"].get()[B:], want_state[B:], err_msg="guide_state of the draft rows")
    np.testing.assert_array_equal(bufs["fin"].get(), want_fin, err_msg="finished")
    np.testing.assert_array_equal(bufs["trans"].get()[:B], addresses(T, gid[:B], "trans"), err_msg="guide_trans of the slots")
    np.testing.assert_array_equal(bufs["masks"].get()[:B], addresses(T, gid[:B], "masks"), err_msg="guide_masks of the slots")
    np.testing.assert_array_equal(bufs["state"].get()[:B], gstate[:B], err_msg="guide_state of the slots")


@pytest.mark.parametrize("B,K,rows", [(5, 3, 20), (4, 1, 17)])
def test_trim_and_rows_in_the_static_layout(L, B, K, rows):
    T, st, gid, gstate, bufs, a, g = setup(L, B, K, rows)
    a.n_draft = bufs["count"].ptr
    L.kr_spec_propose(C.byref(a), 0)
    ref = R.propose(st.prompts, st.hist, st.ctx, st.plen, st.fin, st.temp, st.seed, K, rows, st.n_min, st.n_max, st.s_max, PAD, V,
                    scripts=st.scripts)
    np.testing.assert_array_equal(bufs["count"].get(), ref["n_draft"])
    np.testing.assert_array_equal(bufs["draft"].get(), ref["draft_tok"])
    np.testing.assert_array_equal(bufs["fin"].get(), ref["fin"])
    # ---- trim
    L.kr_spec_guide_trim(C.byref(a), C.byref(g), bufs["count"].ptr, 0)
    n, tok_, dstate, before = G.trim(T["pats"], gid[:B], gstate[:B], st.fin, st.ctx, ref["n_draft"], ref["draft_tok"],
                                     np.full((B, K), -9), PAD, TB)
    np.testing.assert_array_equal(bufs["count"].get(), n, err_msg="n_draft")
    np.testing.assert_array_equal(bufs["draft"].get(), tok_, err_msg="draft_tok")
    np.testing.assert_array_equal(bufs["dstate"].get(), dstate, err_msg="draft_state")
    np.testing.assert_array_equal(bufs["before"].get(), before, err_msg="ctx_before")
    np.testing.assert_array_equal(bufs["state"].get(), gstate, err_msg="the trim writes no guide_state")
    np.testing.assert_array_equal(bufs["fin"].get(), ref["fin"], err_msg="the trim writes no finished")
    unguided = [b for b in range(B) if gid[b] == 0 or st.fin[b]]
    assert unguided and all(n[b] == ref["n_draft"][b] and (tok_[b] == ref["draft_tok"][b]).all() for b in unguided)
    assert (n < ref["n_draft"]).any() and (n == ref["n_draft"])[gid[:B] > 0].any()
    # ---- rows
    L.kr_spec_guide_rows(C.byref(a), C.byref(g), None, 0)
    want_gid, want_state, want_fin = G.rows(gid, gstate, ref["fin"], n, dstate, B, K, rows)
    check_rows(T, bufs, B, want_gid, want_state, want_fin, gid, gstate)
    assert (want_gid[B:] != 0).any() and (want_fin[B:B * (K + 1)] != ref["fin"][B:B * (K + 1)]).any()
    for b in unguided:
        assert all(want_gid[j * B + b] == 0 and want_state[j * B + b] == 0 for j in range(1, K + 1))
    np.testing.assert_array_equal(bufs["count"].get(), n, err_msg="n_draft after the rows")
    np.testing.assert_array_equal(bufs["draft"].get(), tok_, err_msg="draft_tok after the rows")


@pytest.mark.parametrize("B,K,rows", [(3, 3, 17), (20, 3, 32)])
def test_trim_deal_and_rows_with_shared_rows(L, B, K, rows):
    T, st, gid, gstate, bufs, a, g = setup(L, B, K, rows)
    nd = Guarded(np.full(B, -9, np.int32))
    a.n_draft = nd.ptr
    L.kr_spec_lookup(C.byref(a), bufs["count"].ptr, 0)
    n_want, tok0 = D.lookup(st.prompts, st.hist, st.ctx, st.plen, st.fin, K, st.n_min, st.n_max, st.s_max, PAD, V, st.scripts)
    np.testing.assert_array_equal(bufs["count"].get(), n_want)
    np.testing.assert_array_equal(bufs["draft"].get(), tok0)
    # ---- trim, between the lookup and the deal
    L.kr_spec_guide_trim(C.byref(a), C.byref(g), bufs["count"].ptr, 0)
    n, tok_, dstate, before = G.trim(T["pats"], gid[:B], gstate[:B], st.fin, st.ctx, n_want, tok0, np.full((B, K), -9), PAD, TB)
    np.testing.assert_array_equal(bufs["count"].get(), n, err_msg="n_want")
    np.testing.assert_array_equal(bufs["draft"].get(), tok_, err_msg="draft_tok")
    np.testing.assert_array_equal(bufs["dstate"].get(), dstate, err_msg="draft_state")
    np.testing.assert_array_equal(bufs["before"].get(), before, err_msg="ctx_before")
    assert (n < n_want).any()
    # ---- the deal on the trimmed counts
    L.kr_spec_deal(C.byref(a), bufs["count"].ptr, bufs["row"].ptr, 0)
    deal = D.deal(n, tok_, st.ctx, st.plen, st.fin, st.temp, st.seed, K, rows, st.s_max, PAD)
    np.testing.assert_array_equal(bufs["row"].get(), deal["draft_row"], err_msg="draft_row")
    np.testing.assert_array_equal(nd.get(), deal["n_draft"], err_msg="n_draft")
    np.testing.assert_array_equal(bufs["fin"].get(), deal["fin"], err_msg="finished after the deal")
    untrimmed = D.deal_rows(n_want, [not f for f in st.fin], K, rows)
    if (B, K, rows) == (20, 3, 32):
        # slot 1's depth-1 draft is forbidden: the row it would have taken goes to a slot that would have got none
        assert n_want[1] == K and n[1] == 0 and untrimmed[1, 0] >= B and deal["draft_row"][1, 0] == -1
        assert (untrimmed != deal["draft_row"]).any()
        gained = [b for b in range(B) if (deal["draft_row"][b] >= 0).sum() > (untrimmed[b] >= 0).sum()]
        assert gained, "a trimmed draft must free a row for another slot"
        assert (deal["n_draft"] < n).any(), "the budget binds"
    # ---- rows
    L.kr_spec_guide_rows(C.byref(a), C.byref(g), bufs["row"].ptr, 0)
    want_gid, want_state, want_fin = G.rows(gid, gstate, deal["fin"], deal["n_draft"], dstate, B, K, rows, draft_row=deal["draft_row"])
    check_rows(T, bufs, B, want_gid, want_state, want_fin, gid, gstate)
    assert (want_gid[B:] != 0).any() and (want_gid[B:] == 0).any()
    np.testing.assert_array_equal(want_fin, deal["fin"], err_msg="with a dealt map `finished` is the deal's")
    np.testing.assert_array_equal(bufs["row"].get(), deal["draft_row"], err_msg="draft_row after the rows")
    np.testing.assert_array_equal(nd.get(), deal["n_draft"], err_msg="n_draft after the rows")


def test_trim_leaves_a_finished_slots_count_and_drafts(L):
    """The trim called by hand on counts kr_spec_propose would not leave — a finished guided slot with a count and forbidden drafts: it
    keeps both — beside a count of 0, a full run and an unguided slot."""
    B, K, rows = 4, 3, 17
    T, st, gid, gstate, bufs, a, g = setup(L, B, K, rows)
    p1 = T["pats"][0]
    gid[:B], gstate[:B] = [1, 1, 1, 0], [p1.start] * 4
    bufs["trans"], bufs["masks"], bufs["state"] = (Guarded(np.concatenate([addresses(T, gid[:B], "trans"), [-5] * (rows - B)])),
                                                   Guarded(np.concatenate([addresses(T, gid[:B], "masks"), [-5] * (rows - B)])),
                                                   Guarded(gstate))
    g.guide_trans, g.guide_masks, g.guide_state = bufs["trans"].ptr, bufs["masks"].ptr, bufs["state"].ptr
    fin = np.asarray([1, 0, 0, 0], np.int32)
    bufs["fin"] = Guarded(np.concatenate([fin, np.full(rows - B, -5, np.int32)]))
    a.finished = bufs["fin"].ptr
    dash, x = tok(b"-"), tok(b"a")
    count = np.asarray([2, 0, 3, 3], np.int32)
    draft = np.asarray([[dash, dash, PAD], [PAD, PAD, PAD], [x, x, x], [dash, dash, dash]], np.int32)
    bufs["count"], bufs["draft"] = Guarded(count), Guarded(draft)
    a.draft_tok = bufs["draft"].ptr
    L.kr_spec_guide_trim(C.byref(a), C.byref(g), bufs["count"].ptr, 0)
    n, tok_, dstate, before = G.trim(T["pats"], gid[:B], gstate[:B], fin, st.ctx, count, draft, np.full((B, K), -9), PAD, TB)
    assert n.tolist() == [2, 0, 3, 3] and tok_[0].tolist() == [dash, dash, PAD]
    np.testing.assert_array_equal(bufs["count"].get(), n)
    np.testing.assert_array_equal(bufs["draft"].get(), tok_)
    np.testing.assert_array_equal(bufs["dstate"].get(), dstate)
    np.testing.assert_array_equal(bufs["before"].get(), before)


def test_advance_walks_the_emitted_tokens(L):
    """Emitted counts 0 (a frozen finished slot), 1, K + 1, a step that ends on an EOS (the EOS is not walked; nor is a last token
    with bytes on which the step stopped), and an unguided slot."""
    K, rows = 3, 32
    T = tables(L)
    p1, p2 = T["pats"]
    s1 = lambda text: p1.guide.walk(p1.start, text)
    s2 = lambda text: p2.guide.walk(p2.start, text)
    t = tok
    # (pattern, state before, generated before the step, emitted, finished afterwards)
    plan = [
        (1, s1(b"abc-12"), [t(b"a")], [], 1),                                            # frozen: nothing emitted
        (1, s1(b"ab"), [t(b"a"), t(b"b")], [t(b"c")], 0),                                # one token
        (1, s1(b""), [9], [t(b"abc-"), t(b"1"), t(b"2"), t(b";")], 0),                   # K + 1 tokens, a multi-byte one among them
        (1, s1(b"abc-1"), [9, 9], [t(b"2"), EOS], 1),                                    # ends on an EOS
        (0, 77, [9], [t(b"-"), t(b"-")], 0),                                             # unguided
        (2, s2(b""), [9], [t(b"ab-1"), t(b"2;"), t(b"cab"), t(b"-12")], 0),              # K + 1 multi-byte tokens
        (2, s2(b"ab-1"), [9, 9, 9], [t(b"2;"), t(b"a")], 1),                             # stopped on a token with bytes: not walked
        (2, s2(b"ab-12;"), [9], [EOS], 1),                                               # the step's only token is the EOS
    ]
    B = len(plan)
    seqs = [([1, 2, 3 + b], gen + em, fin, None) for b, (_, _, gen, em, fin) in enumerate(plan)]
    st = SpecState(seqs, K, rows, vocab=V, pad=PAD)
    gid = np.asarray([p[0] for p in plan])
    gstate = np.asarray([p[1] for p in plan] + [-5] * (rows - B), np.int32)
    before = np.asarray([st.ctx[b] - len(plan[b][3]) for b in range(B)], np.int32)
    full = lambda name: np.concatenate([addresses(T, gid, name), np.full(rows - B, -5, np.int64)])
    bufs = {"trans": Guarded(full("trans")), "masks": Guarded(full("masks")), "state": Guarded(gstate),
            "dstate": Guarded(np.full((B, K), -9, np.int32)), "before": Guarded(before)}
    a = st.args()
    g = SpecGuide(bufs["trans"].ptr, bufs["masks"].ptr, bufs["state"].ptr, MASK_WORDS, ptr(T["off"]), ptr(T["bytes"]),
                  bufs["dstate"].ptr, bufs["before"].ptr)
    L.kr_spec_guide_advance(C.byref(a), C.byref(g), 0)
    want = G.advance(T["pats"], gid, gstate[:B], before, st.ctx, st.plen, st.fin, st.hist, TB)
    assert want.tolist() == [s1(b"abc-12"), s1(b"abc"), s1(b"abc-12;"), s1(b"abc-12"), 77, s2(b"ab-12;cab-12"), s2(b"ab-12;"),
                             s2(b"ab-12;")]
    assert 0 not in want.tolist()[:4] + want.tolist()[5:]
    got = bufs["state"].get()
    np.testing.assert_array_equal(got[:B], want, err_msg="guide_state of the slots")
    np.testing.assert_array_equal(got[B:], gstate[B:], err_msg="guide_state of the draft rows")
    np.testing.assert_array_equal(bufs["trans"].get(), full("trans"))
    np.testing.assert_array_equal(bufs["masks"].get(), full("masks"))
    np.testing.assert_array_equal(bufs["before"].get(), before)
    np.testing.assert_array_equal(bufs["dstate"].get(), np.full((B, K), -9))
    np.testing.assert_array_equal(bits(st.d_hist), st.hist)
    np.testing.assert_array_equal(bits(st.d_ctx)[:B], st.ctx)
