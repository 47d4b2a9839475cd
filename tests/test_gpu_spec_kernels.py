"""The four launches a speculative decode step adds (include/karanta_hip.h: kr_attn_decode_rows, kr_linear_decode32_rows,
kr_spec_propose, kr_spec_accept), through the C-ABI on a real MI355X.  The two indexed variants are compared bit for bit with the
launches they index (kr_attn_decode_slots, kr_linear_decode32), the two new kernels with the numpy restatement in
tests/spec_ref.py.  Every comparison is an integer or bit equality.  Widths: hidden 512, head_dim 128."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import positions as POS  # noqa: E402
from karanta_ocr_amd import weights as WT  # noqa: E402
from karanta_ocr_amd._lib import DEC_PLAIN, DEC_ROPE_KV, Dec32, KarantaHipError, Spec, lib, ptr  # noqa: E402
from karanta_ocr_amd.weights import bf16_round, pack_w16x64  # noqa: E402
from tests import attn_patterns as AP  # noqa: E402
from tests import spec_ref as R  # noqa: E402

DEV = "cuda:0"
HD = 128


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def bits(t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def rnd(rng, *shape, scale=1.0):
    return bf16_round(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


# ----------------------------------------------------------------------------- kr_attn_decode_rows
@pytest.mark.parametrize("n_split", [2, 4])
@pytest.mark.parametrize("c", [29, 30, 61, 62, 63])
def test_attn_rows_gives_the_records_of_one_row_steps(L, c, n_split):
    """Rows (slot 0, j) at contexts c .. c + 3 — across the 32-key unit and the 64-key block — and the rows of a second slot with a
    context of its own, one of them finished, in ONE launch, against K + 1 launches of kr_attn_decode_slots at those contexts."""
    H, KVH, B, K, s_max = 4, 2, 2, 3, 128
    rows = B * (K + 1)
    rng = np.random.default_rng(100 * c + n_split)
    q = rnd(rng, rows, H, HD)
    kc, v = rnd(rng, B, KVH, s_max, HD), rnd(rng, B, KVH, s_max, HD)
    c1 = 40
    row_slot = np.asarray([r % B for r in range(rows)], np.int32)
    ctx = np.asarray([(c if r % B == 0 else c1) + r // B for r in range(rows)], np.int32)
    fin = np.zeros(rows, np.int32)
    fin[3 * B + 1] = 1                           # (slot 1, j = 3)
    q_d, k_d, vt_d = dev_bf16(q), dev_bf16(kc), dev_bf16(POS.vt_blocks(v))
    rec = (HD + 4) * n_split * H
    ws = torch.full((rows * rec,), 9.0, dtype=torch.float32, device=DEV)
    ctx_d, fin_d, slot_d = t_(ctx), t_(fin), t_(row_slot)        # (named: a temporary's memory is reused by the next upload)
    L.kr_attn_decode_rows(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(slot_d), ptr(ws), rows, H, KVH, HD, s_max,
                          n_split, HD ** -0.5, 0)
    got = bits(ws).reshape(rows, rec)
    for j in range(K + 1):
        sl = slice(j * B, (j + 1) * B)
        ref = torch.full((B * rec,), 9.0, dtype=torch.float32, device=DEV)
        L.kr_attn_decode_slots(ptr(q_d[sl]), ptr(k_d), ptr(vt_d), ptr(ctx_d[sl]), ptr(fin_d[sl]), ptr(ref), B, H, KVH, HD, s_max,
                               n_split, HD ** -0.5, 0)
        np.testing.assert_array_equal(got[sl].view(np.uint32), bits(ref).reshape(B, rec).view(np.uint32), err_msg=f"rows of j = {j}")
    assert (got[3 * B + 1] == 9.0).all(), "the finished row's records are not to be written"
    assert not (got[np.flatnonzero(fin == 0)] == 9.0).all(1).any()


@pytest.mark.parametrize("n_split", [2, 4])
@pytest.mark.parametrize("c", [29, 30, 61, 62, 63])
def test_attn_rows_mask_the_later_drafts_keys(L, c, n_split):
    """The `up` ramp of tests/attn_patterns.py over ONE slot's cache: row j sees keys 0 .. c + j and must return key c + j, while the
    keys the later draft rows stored behind it — real V rows, not stale filler — outrank it."""
    H, KVH, K, s_max = 4, 2, 3, 128
    rows, g = K + 1, H // KVH
    base = AP.decode_case([(c + j, 0) for j in range(rows)], H, KVH, "up", s_max=s_max)
    rng = np.random.default_rng(c)
    v = AP.ints_1_15(rng, 1, KVH, s_max, HD)
    case = AP.Case(HD, H, KVH, base.q, base.k[:1], v, s_max=s_max, ctx=base.ctx, finished=base.finished)
    cand = v[0].reshape(KVH * s_max, HD)
    a = np.arange(s_max)
    for j in range(rows):
        vis = (a <= c + j)[None]
        win = AP.check_gaps(a, vis, ~vis, HD, f"row {j}")
        assert win[0] == c + j
        for h in range(H):
            case.units.append(AP.Unit(np.asarray([j]), h, cand, (h // g) * s_max + win, (lambda i, j=j: f"row {j} (ctx_len {c + j})"),
                                      (lambda i: "key %d of kv head %d" % (i % s_max, i // s_max))))
    q_d, k_d, vt_d = dev_bf16(case.q), dev_bf16(case.k), dev_bf16(case.vt)
    ws = torch.zeros(rows * H * n_split * (HD + 4), dtype=torch.float32, device=DEV)
    o_d = torch.full((rows, H * HD), -7.0, dtype=torch.bfloat16, device=DEV)
    ctx_d, fin_d, slot_d = t_(case.ctx), t_(case.finished), t_(np.zeros(rows, np.int32))
    L.kr_attn_decode_rows(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(slot_d), ptr(ws), rows, H, KVH, HD, s_max, n_split,
                          HD ** -0.5, 0)
    L.kr_attn_decode_merge(ptr(ws), ptr(o_d), rows, H, HD, n_split, 0)
    AP.check_output(host(o_d), case, f"draft rows of one slot, c = {c}, n_split = {n_split}")


# ----------------------------------------------------------------------------- kr_linear_decode32_rows
def qkv_launch(L, hp, Wd, sd, bd, M, N, K, cs_d, T, pl_d, ctx_d, q_d, kc_d, vt_d, H, KVH, s_max, row_slot="plain"):
    a = Dec32(ptr(hp), ptr(Wd), ptr(sd), ptr(bd), 0, 0, 0, 0, 0, M, N, K, 8, 1, 0, 0, 0, 0, 0, 0, ptr(cs_d), T, ptr(pl_d), ptr(ctx_d),
              ptr(q_d), ptr(kc_d), ptr(vt_d), H, KVH, s_max)
    if isinstance(row_slot, str):
        L.kr_linear_decode32(DEC_ROPE_KV, C.byref(a), 0)
    else:
        L.kr_linear_decode32_rows(DEC_ROPE_KV, C.byref(a), ptr(row_slot), 0)


@pytest.mark.parametrize("fp8", [False, True])
def test_linear_decode32_rows(L, fp8):
    """NULL and identity maps give kr_linear_decode32's bits; with 3 slots x 3 rows the q rows are the identity run's, K / V land at
    (row_slot, row's ctx_len), every other cache element keeps its value, and the rotary row is the slot's."""
    H, KVH, K, s_max, T = 4, 2, 512, 128, 9
    S, J = 3, 3
    M, N = S * J, (H + 2 * KVH) * HD
    rng = np.random.default_rng(7 + fp8)
    x, W, bias = rnd(rng, M, K, scale=2.0), rnd(rng, N, K, scale=K ** -0.5), rnd(rng, N, scale=0.1)
    ang = rng.uniform(0, 6.28, size=(S, T, 64)).astype(np.float32)
    cs3 = np.concatenate([bf16_round(np.cos(ang)), bf16_round(np.sin(ang))], -1).astype(np.float32)
    slot_of = np.asarray([r % S for r in range(M)], np.int32)
    plen3 = np.asarray([20, 61, 90], np.int32)
    ctx3 = plen3 + np.asarray([2, 1, 4], np.int32)           # slot 1: rows at 62, 63, 64 — across the V^T block border
    ctx = (ctx3[slot_of] + np.arange(M) // S).astype(np.int32)
    plen = plen3[slot_of]
    sd = None
    if fp8:
        codes, scale = WT.quantize_fp8_rows(W)
        Wd, sd = torch.from_numpy(WT.pack_w16x64_fp8(codes)).to(DEV), torch.from_numpy(scale).to(DEV)
    else:
        Wd = dev_bf16(pack_w16x64(W))
    bd = dev_bf16(bias)
    hp = torch.zeros(32 * K, dtype=torch.bfloat16, device=DEV)
    x_d = dev_bf16(x)
    L.kr_pack_rows32(ptr(x_d), K, M, K, ptr(hp), 0)
    # the identity layout: every row a slot of its own, with its slot's rotary row, context and prompt length
    kc9, v9 = rnd(rng, M, KVH, s_max, HD), rnd(rng, M, KVH, s_max, HD)
    cs9_d, pl9_d, ctx_d = t_(cs3[slot_of]), t_(plen), t_(ctx)
    out = {}
    for form in ("plain", None, t_(np.arange(M, dtype=np.int32))):
        q_d = torch.zeros(M, H, HD, dtype=torch.bfloat16, device=DEV)
        kc_d, vt_d = dev_bf16(kc9), dev_bf16(POS.vt_blocks(v9))
        qkv_launch(L, hp, Wd, sd, bd, M, N, K, cs9_d, T, pl9_d, ctx_d, q_d, kc_d, vt_d, H, KVH, s_max, row_slot=form)
        key = "plain" if isinstance(form, str) else "null" if form is None else "identity"
        out[key] = (bits(q_d), bits(kc_d), bits(vt_d))
    for key in ("null", "identity"):
        for a, b, what in zip(out["plain"], out[key], ("q", "K cache", "V^T cache")):
            np.testing.assert_array_equal(a, b, err_msg=f"{key} map: {what}")
    assert (out["plain"][1] != bits(dev_bf16(kc9))).any()
    # 3 slots x 3 rows.  The cache and the rotary table keep M entries, so that a launch that took the ROW for the slot would write
    # slots 3 .. 8 and read their (different) table rows: it fails the comparisons below instead of leaving the buffers
    kc3, v3 = rnd(rng, M, KVH, s_max, HD), rnd(rng, M, KVH, s_max, HD)
    other = rng.uniform(0, 6.28, size=(M - S, T, 128)).astype(np.float32)
    q_d = torch.zeros(M, H, HD, dtype=torch.bfloat16, device=DEV)
    kc_d, vt_d = dev_bf16(kc3), dev_bf16(POS.vt_blocks(v3))
    cs_m, slot_d = t_(np.concatenate([cs3, bf16_round(np.cos(other))])), t_(slot_of)
    qkv_launch(L, hp, Wd, sd, bd, M, N, K, cs_m, T, pl9_d, ctx_d, q_d, kc_d, vt_d, H, KVH, s_max, row_slot=slot_d)
    np.testing.assert_array_equal(bits(q_d), out["plain"][0], err_msg="q rows")
    want_k = bits(dev_bf16(kc3)).copy()
    want_v = bits(dev_bf16(v3)).copy()
    ident_k = out["plain"][1]
    ident_v = POS.vt_rows(out["plain"][2])
    for r in range(M):
        want_k[slot_of[r], :, ctx[r]] = ident_k[r, :, ctx[r]]
        want_v[slot_of[r], :, ctx[r]] = ident_v[r, :, ctx[r]]
    np.testing.assert_array_equal(bits(kc_d), want_k, err_msg="K cache: rows at (row_slot, ctx_len), nothing else")
    np.testing.assert_array_equal(POS.vt_rows(bits(vt_d)), want_v, err_msg="V^T cache: columns at (row_slot, ctx_len), nothing else")
    with pytest.raises(KarantaHipError, match="ROPE_KV only"):
        L.kr_linear_decode32_rows(DEC_PLAIN, C.byref(Dec32()), 0, 0)


# ----------------------------------------------------------------------------- kr_spec_propose
class SpecState:
    """Device buffers of a kr_spec for `slots` sequences given as (prompt, generated tokens, finished, script | None)."""

    def __init__(self, seqs, k, rows, s_max=64, n_min=2, n_max=4, vocab=300, d=512, pad=3, hist_rows=40, seed=0):
        B = len(seqs)
        rng = np.random.default_rng(seed)
        self.B, self.k, self.rows, self.s_max, self.n_min, self.n_max, self.vocab, self.d, self.pad = B, k, rows, s_max, n_min, n_max, vocab, d, pad
        self.prompts = [np.asarray(p, np.int32) for p, _, _, _ in seqs]
        self.scripts = [None if sc is None else list(sc) for _, _, _, sc in seqs]
        self.hist = np.full((hist_rows, B), -1, np.int32)
        self.plen = np.asarray([len(p) for p in self.prompts], np.int32)
        self.ctx = np.zeros(B, np.int32)
        for b, (_, gen, _, _) in enumerate(seqs):
            self.hist[:len(gen), b] = gen
            self.ctx[b] = self.plen[b] + len(gen) - 1
        self.fin = np.asarray([f for _, _, f, _ in seqs], np.int32)
        self.temp = rng.uniform(0, 1, B).astype(np.float32)
        self.seed = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
        self.table = rnd(rng, vocab, d)
        pid = np.full((B, s_max), -9, np.int32)
        for b, p in enumerate(self.prompts):
            pid[b, :len(p)] = p
        full = lambda a, fill, dt: t_(np.concatenate([a, np.full(rows - B, fill, dt)]).astype(dt))
        self.d_pid, self.d_hist = t_(pid), t_(self.hist)
        self.d_slot = t_(np.concatenate([np.arange(B), np.full(rows - B, -5)]).astype(np.int32))
        self.d_ctx, self.d_plen, self.d_fin = full(self.ctx, -5, np.int32), full(self.plen, -5, np.int32), full(self.fin, -5, np.int32)
        self.d_temp, self.d_seed = full(self.temp, -5, np.float32), t_(np.concatenate([self.seed, np.full(rows - B, 77, np.uint32)]).view(np.int32))
        self.d_nd, self.d_draft = t_(np.full(B, -5, np.int32)), t_(np.full((B, k), -5, np.int32))
        self.d_table = dev_bf16(self.table)
        self.d_x = torch.full((rows, d), -7.0, dtype=torch.bfloat16, device=DEV)
        self.d_prop, self.d_acc = t_(np.arange(B, dtype=np.int32) + 100), t_(np.arange(B, dtype=np.int32) + 200)
        self.keep = [t_(np.asarray(sc, np.int32)) if sc is not None else None for sc in self.scripts]
        self.d_script = t_(np.asarray([0 if s is None else s.data_ptr() for s in self.keep], np.int64))
        self.d_slen = t_(np.asarray([0 if s is None else len(s) for s in self.scripts], np.int32))

    def args(self):
        return Spec(self.B, self.k, self.rows, self.n_min, self.n_max, self.s_max, ptr(self.d_pid), self.d_pid.stride(0), ptr(self.d_hist),
                    self.d_hist.stride(0), self.d_hist.shape[0], ptr(self.d_script), ptr(self.d_slen), ptr(self.d_slot), ptr(self.d_ctx),
                    ptr(self.d_plen), ptr(self.d_fin), ptr(self.d_temp), ptr(self.d_seed), ptr(self.d_nd), ptr(self.d_draft),
                    ptr(self.d_table), self.d, self.pad, self.vocab, ptr(self.d_x), self.d_x.stride(0), ptr(self.d_prop), ptr(self.d_acc))

    def reference(self):
        return R.propose(self.prompts, self.hist, self.ctx, self.plen, self.fin, self.temp, self.seed, self.k, self.rows, self.n_min,
                         self.n_max, self.s_max, self.pad, self.vocab, scripts=self.scripts)


def check_propose(L, st):
    a = st.args()
    L.kr_spec_propose(C.byref(a), 0)
    want = st.reference()
    got = {"n_draft": st.d_nd, "draft_tok": st.d_draft, "slot": st.d_slot, "ctx": st.d_ctx, "plen": st.d_plen, "fin": st.d_fin,
           "temp": st.d_temp, "seed": st.d_seed}
    for name, t in got.items():
        np.testing.assert_array_equal(bits(t).view(np.uint32) if name == "seed" else bits(t), want[name], err_msg=name)
    x = bits(st.d_x)
    table = bits(st.d_table)
    for r in range(st.rows):
        if r < st.B:
            assert (host(st.d_x[r]) == -7.0).all(), f"x of slot {r}'s own row is not the proposer's to write"
        else:
            np.testing.assert_array_equal(x[r], table[want["tok"][r]], err_msg=f"x row {r}")
    return want


def test_spec_propose_lookup_cases(L):
    """One slot per case of the matching rule; 7 slots x (3 + 1) rows in a 30-row step, so two rows lie past the layout."""
    K = 3
    seqs = [
        ([1, 2, 3, 4, 5, 6, 7], [8, 9], 0, None),                                   # 0 no match
        ([10, 11, 12, 13, 14, 15, 11, 12], [], 0, None),                            # 1 a match in the prompt only (L = plen)
        ([20, 21, 22], [30, 31, 32, 33, 34, 35, 31, 32], 0, None),                  # 2 a match in the strided history only
        ([40, 41, 50, 51, 52, 40], [41], 0, None),                                  # 3 the suffix [40, 41] lies across the border
        ([1, 2, 3, 40, 41, 42, 9, 2], [3], 0, None),                                # 4 fallback from n_max to n_min
        ([5, 6, 70, 71, 72, 9, 5, 6, 5], [6], 0, None),                             # 5 a truncated continuation loses to a full one
        ([5, 6, 70, 71, 72, 5, 6, 80], [5, 6], 0, None),                            # 6 equal counts: the larger i
    ]
    want = check_propose(L, SpecState(seqs, K, 30))
    assert want["n_draft"].tolist() == [0, 3, 3, 3, 3, 3, 3]
    assert want["draft_tok"].tolist()[1:] == [[13, 14, 15], [33, 34, 35], [50, 51, 52], [40, 41, 42], [70, 71, 72], [80, 5, 6]]
    assert want["fin"][28:].tolist() == [1, 1] and want["ctx"][28:].tolist() == [63, 63]


def test_spec_propose_edges_and_script(L):
    """L <= n_min, a finished slot (its match is not used), a parked slot (ctx = plen = s_max - 1: every row clamped), the scripted
    mode (it replaces the lookup, runs out, and a token outside the vocabulary ends the run), and a slot with room for one draft."""
    K, s_max = 3, 64
    park = list(range(100, 100 + s_max - 1))
    seqs = [
        ([7], [7], 0, None),                                                         # L = 2 = n_min
        ([10, 11, 12, 13, 10, 11], [], 1, None),                                     # finished
        (park, [], 1, None),                                                         # parked: plen = ctx = s_max - 1
        ([10, 11, 12, 13, 10, 11], [1, 2], 0, [1, 2, 60, 61, 62, 63]),               # scripted: drafts 60, 61, 62 (not the lookup's 12, 13)
        ([1, 2, 3], [4, 5, 6], 0, [4, 5, 6, 9]),                                     # the script runs out: one draft
        ([1, 2, 3], [4], 0, [4, 8, 999, 8]),                                         # 999 is outside the vocabulary of 300: one draft
        (list(range(200, 200 + s_max - 4)) + [200, 201], [], 0, None),               # ctx = s_max - 3: room for 2 of the 3 drafts
    ]
    st = SpecState(seqs, K, 28, s_max=s_max)
    st.ctx[2] = st.plen[2] = s_max - 1          # a parked slot's ctx_len is not plen - 1 + generated
    st.d_ctx[2], st.d_plen[2] = s_max - 1, s_max - 1
    want = check_propose(L, st)
    assert want["n_draft"].tolist() == [0, 0, 0, 3, 1, 1, 2]
    assert want["ctx"].reshape(K + 1, 7)[:, 2].tolist() == [s_max - 1] * 4
    assert want["draft_tok"][3].tolist() == [60, 61, 62]


# ----------------------------------------------------------------------------- kr_spec_accept
def partials(tokens, n_part, vocab, rng):
    """ARGMAX partials [rows, n_part] whose final argmax is tokens[r]: the winning value twice — with the token in one part and
    with a HIGHER index in an earlier or later part — over random lower values."""
    rows = len(tokens)
    val = rng.uniform(-5, 2, (rows, n_part)).astype(np.float32)
    idx = rng.integers(0, vocab, (rows, n_part)).astype(np.int32)
    for r, t in enumerate(tokens):
        p, q = rng.choice(n_part, 2, replace=False)
        val[r, p], idx[r, p] = 3.0, t
        val[r, q], idx[r, q] = 3.0, min(t + 1 + int(rng.integers(0, 5)), vocab - 1) if t < vocab - 1 else t
    return val, idx


@pytest.mark.parametrize("n_part", [64, 1120])
@pytest.mark.parametrize("flags", [2, 0])
def test_spec_accept_is_sample_greedy_token_by_token(L, n_part, flags):
    """0 .. K accepted, fewer drafts than K, EOS inside an accepted run (nothing after it), argmax ties across partials (every
    row), a finished slot (frozen with flags = 2; the pad token appended with 0), the history outside the emitted rows, counters."""
    K, EOS, pad, V = 3, (50, 51), 3, 300
    #        model's tokens t_0..t_3    drafts            n_draft  finished
    plan = [([10, 11, 12, 13], [99, 11, 12], 3, 0),       # 0 accepted
            ([10, 11, 12, 13], [10, 99, 12], 3, 0),       # 1
            ([10, 11, 12, 13], [10, 11, 99], 3, 0),       # 2
            ([10, 11, 12, 13], [10, 11, 12], 3, 0),       # 3
            ([10, 11, 12, 13], [10, 11, 12], 2, 0),       # n_draft < K: draft 3 is right but was not proposed
            ([20, 50, 22, 23], [20, 50, 22], 3, 0),       # EOS at t_1, inside the accepted run
            ([51, 11, 12, 13], [51, 11, 12], 3, 0),       # EOS at t_0
            ([10, 11, 12, 13], [10, 11, 12], 0, 1)]       # finished
    B = len(plan)
    rows = B * (K + 1)
    rng = np.random.default_rng(n_part + flags)
    seqs = [([1, 2, 3 + b], list(range(60, 60 + b % 3 + 1)), f, None) for b, (_, _, _, f) in enumerate(plan)]
    st = SpecState(seqs, K, rows, vocab=V, pad=pad)
    tokens = [plan[r % B][0][r // B] for r in range(rows)]
    val, idx = partials(tokens, n_part, V, rng)
    n_draft = np.asarray([p[2] for p in plan], np.int32)
    draft = np.asarray([p[1] for p in plan], np.int32)
    st.d_nd.copy_(t_(n_draft))
    st.d_draft.copy_(t_(draft))
    tok_d = t_(np.full(B, -5, np.int32))
    a = st.args()
    val_d, idx_d, eos_d = t_(val), t_(idx), t_(np.asarray(EOS, np.int32))
    L.kr_spec_accept(C.byref(a), ptr(val_d), ptr(idx_d), n_part, ptr(tok_d), ptr(eos_d), len(EOS), flags, 0)
    hist, ctx, fin = st.hist.copy(), st.ctx.copy(), st.fin.copy()
    want_tok, prop, acc = R.accept(val, idx, n_draft, draft, hist, ctx, st.plen, fin, EOS, pad, flags, K)
    np.testing.assert_array_equal(bits(tok_d), want_tok)
    np.testing.assert_array_equal(bits(st.d_hist), hist, err_msg="history (rows outside the emitted ones keep their value)")
    np.testing.assert_array_equal(bits(st.d_ctx)[:B], ctx)
    np.testing.assert_array_equal(bits(st.d_fin)[:B], fin)
    np.testing.assert_array_equal(bits(st.d_prop), 100 + np.arange(B) + prop)
    np.testing.assert_array_equal(bits(st.d_acc), 200 + np.arange(B) + acc)
    table = bits(st.d_table)
    x = bits(st.d_x)
    for b in range(B):
        np.testing.assert_array_equal(x[b], table[want_tok[b]], err_msg=f"x_next of slot {b}")
    assert (host(st.d_x[B:]) == -7.0).all()
    # the cases are the ones named above
    assert (ctx - st.ctx).tolist() == [1, 2, 3, 4, 3, 2, 1, 0 if flags & 2 else 1]
    assert acc.tolist() == [0, 1, 2, 3, 2, 2, 1, 0] and fin.tolist() == [0, 0, 0, 0, 0, 1, 1, 1]


def test_spec_entry_points_refuse_bad_layouts(L):
    st = SpecState([([1, 2, 3], [4], 0, None)] * 4, 3, 16)
    for change, what in ((dict(rows=15), "rows"), (dict(rows=33), "rows"), (dict(k=0), "k="), (dict(ngram_min=0), "ngram"),
                         (dict(ngram_max=9), "ngram"), (dict(ngram_min=5), "ngram")):
        a = st.args()
        for key, val in change.items():
            setattr(a, key, val)
        with pytest.raises(KarantaHipError, match=what):
            L.kr_spec_propose(C.byref(a), 0)
