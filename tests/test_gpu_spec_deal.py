"""Speculative decoding with shared draft rows (SpecConfig(share_rows=True): kr_spec_lookup, kr_spec_deal, kr_spec_accept_rows) on a real
MI355X: the three launches through the C-ABI against the numpy restatement in tests/spec_deal_ref.py, and the engine and the slot
scheduler at slot counts the static layout refuses — every request returns exactly the tokens it returns without speculation, and
the counters are the restatement's.  Every comparison is an integer or bit equality.  Widths: hidden 512, head_dim 128."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError, lib, ptr  # noqa: E402
from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.scheduler import SlotRequest, SlotScheduler, SpecPolicy  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests import spec_deal_ref as D  # noqa: E402
from tests import spec_ref as R  # noqa: E402
from tests.test_gpu_parallel_sampling import hot, page_of  # noqa: E402
from tests.test_gpu_spec_engine import plain_run, repeated_pages, set_eos, solo  # noqa: E402
from tests.test_gpu_spec_kernels import SpecState, bits, host, partials, t_  # noqa: E402

LENGTHS = [40, 64, 100]
GUARD = 8           # sentinel entries behind n_want / draft_row: a write past the end shows


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


# ----------------------------------------------------------------------------- kr_spec_lookup, kr_spec_deal
def mixed_slots(B, s_max):
    """(prompt, generated, finished, script) per slot: looked-up and scripted drafts, slots that find nothing, finished slots (one
    of them with a match it must not use), a script that runs out, and the last slot at ctx = s_max - 2 (room for one draft)."""
    kinds = [
        lambda b: ([10, 11, 12, 13, 14, 15, 11, 12], [], 0, None),                       # the lookup finds 13, 14, 15
        lambda b: ([1, 2, 3], [4], 0, [4, 60 + b, 61, 62, 63]),                          # scripted: 60 + b, 61, 62
        lambda b: ([1, 2, 3, 4, 5, 6, 7], [8, 9], 0, None),                              # no match
        lambda b: ([10, 11, 12, 13, 10, 11], [], 1, None),                               # finished
        lambda b: ([1, 2, 3], [4, 5, 6], 0, [4, 5, 6, 9]),                               # the script runs out: one draft
        lambda b: ([20, 21, 22], [30, 31, 32, 33, 34, 35, 31, 32], 0, None),             # a match in the history: 33, 34, 35
    ]
    seqs = [kinds[b % len(kinds)](b) for b in range(B)]
    seqs[-1] = (list(range(200, 200 + s_max - 3)) + [200, 201], [], 0, None)            # plen = s_max - 1, ctx = s_max - 2
    return seqs


@pytest.mark.parametrize("B,K,rows", [(5, 3, 17), (20, 2, 32), (31, 3, 32), (4, 3, 17)])
def test_lookup_and_deal_equal_the_restatement(L, B, K, rows):
    s_max = 64
    st = SpecState(mixed_slots(B, s_max), K, rows, s_max=s_max, seed=B)
    assert st.ctx[-1] == s_max - 2
    d_want = t_(np.full(B + GUARD, -5, np.int32))
    d_row = t_(np.full(B * K + GUARD, -5, np.int32))
    a = st.args()
    # ---- lookup: n_want and draft_tok, nothing else
    L.kr_spec_lookup(C.byref(a), ptr(d_want), 0)
    n_want, tok = D.lookup(st.prompts, st.hist, st.ctx, st.plen, st.fin, K, st.n_min, st.n_max, s_max, st.pad, st.vocab, st.scripts)
    np.testing.assert_array_equal(bits(d_want), np.concatenate([n_want, np.full(GUARD, -5)]), err_msg="n_want")
    np.testing.assert_array_equal(bits(st.d_draft), tok, err_msg="draft_tok")
    assert n_want[-1] == 1 and n_want.max() == K and (n_want == 0).any()
    for name, t in (("row_slot", st.d_slot), ("ctx", st.d_ctx), ("plen", st.d_plen), ("fin", st.d_fin)):
        assert (bits(t)[B:] == -5).all(), f"kr_spec_lookup wrote {name} of a draft row"
    assert (bits(st.d_nd) == -5).all() and (host(st.d_x) == -7.0).all()
    # ---- deal
    L.kr_spec_deal(C.byref(a), ptr(d_want), ptr(d_row), 0)
    want = D.deal(n_want, tok, st.ctx, st.plen, st.fin, st.temp, st.seed, K, rows, s_max, st.pad)
    np.testing.assert_array_equal(bits(d_row), np.concatenate([want["draft_row"].ravel(), np.full(GUARD, -5)]), err_msg="draft_row")
    np.testing.assert_array_equal(bits(st.d_nd), want["n_draft"], err_msg="n_draft")
    got = {"slot": st.d_slot, "ctx": st.d_ctx, "plen": st.d_plen, "fin": st.d_fin, "temp": st.d_temp, "seed": st.d_seed}
    for name, t in got.items():
        np.testing.assert_array_equal(bits(t).view(np.uint32) if name == "seed" else bits(t), want[name], err_msg=name)
    x, table = bits(st.d_x), bits(st.d_table)
    for r in range(rows):
        if r < B:
            assert (host(st.d_x[r]) == -7.0).all(), f"x of slot {r}'s own row is not the dealer's to write"
        else:
            np.testing.assert_array_equal(x[r], table[want["tok"][r]], err_msg=f"x row {r}")
    np.testing.assert_array_equal(bits(st.d_draft), tok, err_msg="draft_tok after the deal")
    # the rows nobody was dealt are parked, and the layouts are the cases they are meant to be
    owned = set(int(r) for r in want["draft_row"].ravel() if r >= 0)
    ctx_d, fin_d, slot_d = bits(st.d_ctx), bits(st.d_fin), bits(st.d_slot)
    for r in range(B, rows):
        if r not in owned:
            assert (slot_d[r], ctx_d[r], fin_d[r]) == (0, s_max - 1, 1), f"row {r} is not parked"
        else:
            assert fin_d[r] == 0 and ctx_d[r] <= s_max - 1
    live_want = int(np.where(st.fin == 0, n_want, 0).sum())
    if (B, K, rows) in ((5, 3, 17), (4, 3, 17)):
        assert len(owned) == live_want < rows - B                      # everything fits, rows are left over
    elif (B, K, rows) == (20, 2, 32):
        assert len(owned) == 12 < live_want and (want["n_draft"] < n_want).any()
    else:
        assert len(owned) == 1 and want["draft_row"][0, 0] == 31      # one spare row: the first slot that wants one


# ----------------------------------------------------------------------------- kr_spec_accept_rows
@pytest.mark.parametrize("n_part", [64, 1120])
@pytest.mark.parametrize("flags", [2, 0])
def test_accept_over_a_permuted_map_equals_accept_on_the_static_layout(L, n_part, flags):
    """test_gpu_spec_kernels' plan (0 .. K accepted, fewer drafts than K, EOS inside and at the head of a run, a finished slot): the
    same partials once in the static layout through kr_spec_accept, once scattered over rows 8 .. 31 through kr_spec_accept_rows."""
    K, EOS, pad, V = 3, (50, 51), 3, 300
    plan = [([10, 11, 12, 13], [99, 11, 12], 3, 0), ([10, 11, 12, 13], [10, 99, 12], 3, 0), ([10, 11, 12, 13], [10, 11, 99], 3, 0),
            ([10, 11, 12, 13], [10, 11, 12], 3, 0), ([10, 11, 12, 13], [10, 11, 12], 2, 0), ([20, 50, 22, 23], [20, 50, 22], 3, 0),
            ([51, 11, 12, 13], [51, 11, 12], 3, 0), ([10, 11, 12, 13], [10, 11, 12], 0, 1)]
    B = len(plan)
    rows = B * (K + 1)
    rng = np.random.default_rng(n_part + flags)
    seqs = [([1, 2, 3 + b], list(range(60, 60 + b % 3 + 1)), f, None) for b, (_, _, _, f) in enumerate(plan)]
    val, idx = partials([plan[r % B][0][r // B] for r in range(rows)], n_part, V, rng)
    n_draft = np.asarray([p[2] for p in plan], np.int32)
    draft = np.asarray([p[1] for p in plan], np.int32)
    # the map: the dealt drafts on distinct rows of 8 .. 31 in a random order; the rows left over hold partials that would win
    free = list(rng.permutation(np.arange(B, rows)))
    draft_row = np.full((B, K), -1, np.int32)
    val2, idx2 = np.full_like(val, 9.0), np.full_like(idx, 77)
    val2[:B], idx2[:B] = val[:B], idx[:B]
    for b in range(B):
        for j in range(1, int(n_draft[b]) + 1):
            r = int(free.pop())
            draft_row[b, j - 1] = r
            val2[r], idx2[r] = val[j * B + b], idx[j * B + b]
    assert sorted(draft_row[draft_row >= 0].tolist()) != draft_row[draft_row >= 0].tolist()
    out = []
    for shared in (False, True):
        st = SpecState(seqs, K, rows, vocab=V, pad=pad)
        st.d_nd.copy_(t_(n_draft))
        st.d_draft.copy_(t_(draft))
        tok_d, eos_d = t_(np.full(B, -5, np.int32)), t_(np.asarray(EOS, np.int32))
        a = st.args()
        if shared:
            row_d, val_d, idx_d = t_(draft_row), t_(val2), t_(idx2)
            L.kr_spec_accept_rows(C.byref(a), ptr(row_d), ptr(val_d), ptr(idx_d), n_part, ptr(tok_d), ptr(eos_d), len(EOS), flags, 0)
        else:
            val_d, idx_d = t_(val), t_(idx)
            L.kr_spec_accept(C.byref(a), ptr(val_d), ptr(idx_d), n_part, ptr(tok_d), ptr(eos_d), len(EOS), flags, 0)
        out.append({"tokens": bits(tok_d), "history": bits(st.d_hist), "ctx": bits(st.d_ctx), "fin": bits(st.d_fin),
                    "proposed": bits(st.d_prop), "accepted": bits(st.d_acc), "x": bits(st.d_x)})
    for name in out[0]:
        np.testing.assert_array_equal(out[1][name], out[0][name], err_msg=name)
    # ... and both are the restatement
    st = SpecState(seqs, K, rows, vocab=V, pad=pad)
    hist, ctx, fin = st.hist.copy(), st.ctx.copy(), st.fin.copy()
    want_tok, prop, acc = D.accept_rows(val2, idx2, n_draft, draft, draft_row, hist, ctx, st.plen, fin, EOS, pad, flags, K)
    np.testing.assert_array_equal(out[1]["tokens"], want_tok)
    np.testing.assert_array_equal(out[1]["history"], hist)
    np.testing.assert_array_equal(out[1]["ctx"][:B], ctx)
    np.testing.assert_array_equal(out[1]["proposed"], 100 + np.arange(B) + prop)
    np.testing.assert_array_equal(out[1]["accepted"], 200 + np.arange(B) + acc)
    assert acc.tolist() == [0, 1, 2, 3, 2, 2, 1, 0]


def test_shared_rows_entry_points_refuse_bad_layouts(L):
    st = SpecState([([1, 2, 3], [4], 0, None)] * 4, 3, 17)
    buf = t_(np.zeros(32, np.int32))
    for change, what in ((dict(rows=4), "rows"), (dict(rows=33), "rows"), (dict(k=0), "k="), (dict(k=32), "k="), (dict(slots=0), "slots"),
                         (dict(ngram_max=9), "ngram")):
        a = st.args()
        for key, v in change.items():
            setattr(a, key, v)
        with pytest.raises(KarantaHipError, match=what):
            L.kr_spec_lookup(C.byref(a), ptr(buf), 0)
        with pytest.raises(KarantaHipError, match=what):
            L.kr_spec_deal(C.byref(a), ptr(buf), ptr(buf), 0)
        with pytest.raises(KarantaHipError, match=what):
            L.kr_spec_accept_rows(C.byref(a), ptr(buf), ptr(buf), ptr(buf), 4, ptr(buf), ptr(buf), 1, 0, 0)
    a = st.args()
    with pytest.raises(KarantaHipError, match="null"):
        L.kr_spec_lookup(C.byref(a), 0, 0)
    with pytest.raises(KarantaHipError, match="null"):
        L.kr_spec_deal(C.byref(a), ptr(buf), 0, 0)


# ----------------------------------------------------------------------------- the engine
NAME, B20, K = "tiny-w512", 20, 3
KW = dict(s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)
_E = {}


def engines():
    """The plain and the shared-rows engine at 20 slots, kept for the module, with two EOS ids taken from the plain greedy run: the
    fourth token of one slot (eos_slot) — so that its first scripted run of K drafts ends in an accepted EOS — and a late token
    of another."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not _E:
        cfg = CONFIGS[NAME]
        w = random_weights(cfg, 909)
        _E["plain"] = Engine(cfg, max_batch=B20, **KW)
        _E["spec"] = Engine(cfg, max_batch=B20, speculative=SpecConfig(K, share_rows=True), **KW)
        for e in (_E["plain"], _E["spec"]):
            e.load_weights(w)
        _E["pages"] = [page_of(cfg, LENGTHS[b % 3], variant=b) for b in range(B20)]
        free = plain_run(_E["plain"], _E["pages"], 12)
        s0 = next(b for b in range(B20) if len(free[b]) > 3 and free[b][3] not in free[b][:3])
        late = next(int(free[b][9]) for b in range(B20 - 1, -1, -1) if b != s0 and len(free[b]) > 9 and free[b][9] not in free[s0][:4])
        _E["eos_slot"], _E["eos"] = s0, (int(free[s0][3]), late)
        for e in (_E["plain"], _E["spec"]):
            set_eos(e, _E["eos"])
    return _E["plain"], _E["spec"], _E["pages"]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k in ("plain", "spec", "plain4", "spec4", "static4"):
        if k in _E:
            _E[k].close()
    _E.clear()


def truth_of(sampled):
    """The plain engine's tokens for the module's 20 pages (greedy, or sampled at a temperature at which the noise decides), once."""
    plain, _, pages = engines()
    key = ("truth", sampled)
    if key not in _E:
        if sampled:
            T = hot(plain, pages[0])
            pages = [dataclasses.replace(p, temperature=T, seed=(0xFFFFFFF0 + b) & 0xFFFFFFFF) for b, p in enumerate(pages)]
        _E[key] = (pages, plain_run(plain, pages, 1 + 16 * (K + 1), sampling=sampled))
    return _E[key]


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("scripted", ["all", "three"])
def test_twenty_slots_give_the_plain_tokens_and_the_restatements_counts(scripted, sampled):
    """Scripts equal to the plain continuation on every slot — 60 wanted drafts for 12 spare rows: the budget binds in every step —
    and on three slots only (the others draft nothing: it never binds).  Tokens: the plain run's; generated / proposed /
    accepted per slot: spec_deal_ref.simulate's."""
    plain, spec, _ = engines()
    pages, truth = truth_of(sampled)
    S = 16
    eos = set(_E["eos"])
    s0 = _E["eos_slot"]
    which = list(range(B20)) if scripted == "all" else [s0, (s0 + 7) % B20, (s0 + 13) % B20]
    scripts = [[int(t) for t in truth[b]] if b in which else [] for b in range(B20)]
    trace = []
    want = D.simulate([p.input_ids for p in pages], scripts, truth, K, spec.rows, S, eos=eos, trace=trace)
    assert spec.rows == 32 and spec.share_rows
    if scripted == "all":
        assert all(sum(nd) == min(12, sum(w)) for w, nd in trace) and sum(trace[0][0]) > 12 == sum(trace[0][1])
        assert sum(1 for w, nd in trace if sum(w) > 12) >= S // 2, "the budget must bind in most steps"
    else:
        assert all(nd == w and sum(w) <= 9 for w, nd in trace)
        assert all(want[b][2] > 0 for b in which) and all(want[b][1] == 0 for b in range(B20) if b not in which)
        if not sampled:      # eos_slot's first step: its three drafts are right and the third is the EOS — the row behind it emits nothing
            assert len(truth[s0]) == 4 and want[s0] == (4, 3, 3)
    spec.begin_slots(2 + S * (K + 1), sampling=sampled)
    spec.admit(pages, list(range(B20)))
    try:
        for b in range(B20):
            spec.set_draft_script(b, scripts[b])
        spec.decode_steps(S, speculative=True)
        _, gen = spec.poll_slots()
        prop, acc = spec.spec_counters()
        for b in range(B20):
            assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b}: generated / proposed / accepted"
            np.testing.assert_array_equal(spec.slot_tokens(b, int(gen[b])), truth[b][:int(gen[b])], err_msg=f"slot {b}")
        assert int(acc.sum()) == int(prop.sum()) > 0
    finally:
        for b in range(B20):
            spec.set_draft_script(b, None)


@pytest.mark.parametrize("sampled", [False, True])
def test_plain_and_shared_speculative_chunks_alternate(sampled):
    """The real lookup on prompts with repeated spans at 20 slots, two speculative steps and one plain step in turn."""
    plain, spec, _ = engines()
    pages = repeated_pages(plain.cfg, B20)
    if sampled:
        T = hot(plain, pages[0])
        pages = [dataclasses.replace(p, temperature=T, seed=77 + b) for b, p in enumerate(pages)]
    rounds = 6
    N = 1 + rounds * (2 * (K + 1) + 1)
    truth = plain_run(plain, pages, N, sampling=sampled)
    spec.begin_slots(N + 8, sampling=sampled)
    spec.admit(pages, list(range(B20)))
    for _ in range(rounds):
        spec.decode_steps(2, speculative=True)
        spec.decode_steps(1)
    _, gen = spec.poll_slots()
    prop, acc = spec.spec_counters()
    assert int(prop.sum()) > 0, "the lookup proposed nothing: the test needs prompts it finds matches in"
    assert (prop <= 2 * rounds * K).all() and int(prop.sum()) <= 2 * rounds * 12
    for b in range(B20):
        n = int(min(gen[b], len(truth[b])))
        assert n >= min(len(truth[b]), 1 + 3 * rounds)
        np.testing.assert_array_equal(spec.slot_tokens(b, n), truth[b][:n], err_msg=f"slot {b} ({prop[b]} proposed, {acc[b]} accepted)")
    assert spec.spec_steps == 2 * rounds and spec.plain_steps == rounds


def test_where_everything_fits_sharing_changes_nothing():
    """max_batch = 4, K = 3 (16 of 17 rows): the static layout and shared rows give the same tokens and the same counters, with the
    real lookup and a wrong script side by side."""
    plain, _, _ = engines()
    cfg = plain.cfg
    w = random_weights(cfg, 909)
    for key, sc in (("static4", SpecConfig(K, 1, 3)), ("spec4", SpecConfig(K, 1, 3, share_rows=True))):
        _E[key] = Engine(cfg, max_batch=4, speculative=sc, **KW)
        _E[key].load_weights(w)
    pages = repeated_pages(cfg, 4)
    S = 12
    truth = plain_run(plain, pages, 1 + S * (K + 1))
    wrong = [int(t) for t in truth[3]]
    for i in (2, 5, 6, 11):
        if i < len(wrong):
            wrong[i] = (wrong[i] + 1) % 400
    res = []
    for key in ("static4", "spec4"):
        e = _E[key]
        set_eos(e, _E["eos"])
        assert e.rows == 17
        e.begin_slots(2 + S * (K + 1))
        e.admit(pages, list(range(4)))
        e.set_draft_script(3, wrong)
        e.decode_steps(S, speculative=True)
        _, gen = e.poll_slots()
        prop, acc = e.spec_counters()
        e.set_draft_script(3, None)
        res.append((gen, prop, acc, [e.slot_tokens(b, int(gen[b])) for b in range(4)]))
    (g0, p0, a0, t0), (g1, p1, a1, t1) = res
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(a1, a0)
    assert int(p0.sum()) > int(a0.sum()) > 0
    for b in range(4):
        np.testing.assert_array_equal(t1[b], t0[b], err_msg=f"slot {b}")
        np.testing.assert_array_equal(t1[b], truth[b][:len(t1[b])], err_msg=f"slot {b} against the plain run")


def test_nine_slots_with_three_drafts_construct_and_decode():
    """36 rows in the static layout: refused there, 32 shared rows here.  (Fails on a tree without the feature: SpecConfig takes no
    share_rows.)"""
    plain, _, pages = engines()
    cfg = plain.cfg
    with pytest.raises(KarantaHipError, match="rows > 32"):
        Engine(cfg, max_batch=9, speculative=SpecConfig(3), **KW)
    with pytest.raises(KarantaHipError, match="no row is spare"):
        Engine(cfg, max_batch=32, speculative=SpecConfig(3, share_rows=True), **KW)
    e = Engine(cfg, max_batch=9, speculative=SpecConfig(3, share_rows=True), **KW)
    try:
        e.load_weights(random_weights(cfg, 909))
        set_eos(e, _E["eos"])
        assert e.rows == 32 and e.K == 3
        S = 8
        truth = plain_run(plain, pages[:9], 1 + S * (K + 1))
        e.begin_slots(2 + S * (K + 1))
        e.admit(pages[:9], list(range(9)))
        for b in range(9):
            e.set_draft_script(b, truth[b])
        e.decode_steps(S, speculative=True)
        _, gen = e.poll_slots()
        prop, acc = e.spec_counters()
        want = D.simulate([p.input_ids for p in pages[:9]], [[int(t) for t in tr] for tr in truth], truth, K, 32, S, eos=set(_E["eos"]))
        for b in range(9):
            assert (int(gen[b]), int(prop[b]), int(acc[b])) == want[b], f"slot {b}"
            np.testing.assert_array_equal(e.slot_tokens(b, int(gen[b])), truth[b][:int(gen[b])], err_msg=f"slot {b}")
        assert any(g == min(len(t), 1 + S * (K + 1)) for g, t in zip(gen, truth))          # 23 spare rows: some slots run at full depth
    finally:
        e.close()


# ----------------------------------------------------------------------------- through the scheduler
def test_scheduler_at_twenty_slots_equals_solo_runs():
    """34 requests over 20 slots (slots are reused), token limits inside accepted runs, full and wrong scripts and the real lookup
    side by side, and one request with top_k, whose chunks are plain: every result is the request's solo run."""
    plain, spec, _ = engines()
    cfg = plain.cfg
    n = 34
    pages = [page_of(cfg, LENGTHS[i % 3], variant=60 + i) for i in range(n)]
    T = hot(plain, pages[0])
    pages[5] = dataclasses.replace(pages[5], temperature=T, top_k=5, seed=5)
    pages[9] = dataclasses.replace(pages[9], temperature=T, seed=9)
    limits = [6 + (7 * i) % 19 for i in range(n)]
    want = [solo(plain, p, m) for p, m in zip(pages, limits)]
    sch = SlotScheduler(spec, max_tokens_cap=32, chunk=2, sampling=True, speculative=True, spec_policy=SpecPolicy(break_even=0.0))
    try:
        for j in (0, 1, 2, 3):          # right for the first request in the slot, wrong for its successors
            spec.set_draft_script(j, want[j][0])
        spec.set_draft_script(4, [3] * 64)
        res = sch.run([SlotRequest(p, m, tag=i) for i, (p, m) in enumerate(zip(pages, limits))])
    finally:
        for j in range(5):
            spec.set_draft_script(j, None)
    for i, (r, (toks, reason)) in enumerate(zip(res, want)):
        assert r.error is None, r.error
        np.testing.assert_array_equal(r.tokens, toks, err_msg=f"request {i}")
        assert r.finish_reason == reason, f"request {i}"
    assert sch.spec_steps > 0 and sch.plain_steps > 0 and sch.spec_draft_tokens > sch.spec_accepted_tokens > 0
