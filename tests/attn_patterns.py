"""Attention inputs whose softmax has ONE winner per query, so that the expected output is a stored V row and a
one-key masking or indexing error returns a different row (not a test module; shared by test_attention_patterns_cpu.py,
which proves the patterns on the fp64 reference, and test_gpu_attention_exact.py, which runs the kernels on them).

Encoding.  The score of stored K row r is C_Q * a(r) for an integer a(r) < 8192 the test chooses: k[r] is zero except
the two channels (c_hi, c_lo) of its kv head, which hold a // 64 and a % 64; q is zero except the same two channels,
which hold 64 * C_Q and C_Q.  All of these are exact in bf16 and q.k = C_Q * a is an exact integer below 2^24, so the
MFMA sums are exact.  Adjacent values of a are C_Q * hd^-0.5 * log2(e) apart: 65 log2 units at hd 128, 82 at hd 80.
The hd 80 kernel rounds q * scale * log2(e) to bf16 first; 64 * C_Q and C_Q share a mantissa, so both round by the
same factor and the scores stay an exact multiple of a (the gap checks below are made with the rounded q as well).

a is a function of the row's index in K STORAGE (not of the position inside its segment):
  up    a = r - r0              the newest visible key wins; every row stored after it outranks it
  down  a = r_end - r           the first key wins; every row stored before it (ragged storage) outranks it
  tent  a = A - |r - p|         the key at p wins

Preconditions (check_gaps, fp64, asserted wherever a case is built): among the keys a query may see the winner leads
by >= GAP log2 units, and every row named as `forbidden` — the rows a faulty kernel could reach: cache rows past the
context, the next / previous segment's rows, causally masked rows — leads the winner by >= GAP.

Expected output: V[winner].  V is drawn from the integers 1..15, so another row differs by >= 1/15 relative in most
channels.  Tolerance rel 2^-7, abs 2^-20, from the arithmetic and not from a run: the losing keys add at most
n_keys * 2^-48 * 15 < 2^-30; the hd 128 varlen kernel sums its denominator from f32 P and its numerator from bf16 P
while its reference maximum carries the f32 rounding of max * scale * log2(e) (about 0.02 log2 units at these
magnitudes), so the winner's P can sit 2^-9 from its bf16 rounding; the output is rounded to bf16 once more (2^-9) and
1/l in f32: 2^-9 + 2^-9 + slack < 2^-7.  The decode kernel and the hd 80 path use the same bf16 P above and below the
line and come out tighter; one tolerance is used everywhere.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from karanta_ocr_amd import positions as POS
from karanta_ocr_amd.weights import bf16_round

C_Q = 512.0
GAP = 48.0
TOL_REL, TOL_ABS = 2.0 ** -7, 2.0 ** -20
LOG2E_F32 = np.float32(1.4426950408889634)
STALE_V = 99.0          # what a longer earlier page leaves in the V^T columns past a reused slot's context

# ----------------------------------------------------------------------------- the parametrisations (CPU proof = GPU run)
VIT_LENS = {"ragged": [1, 63, 64, 65, 130, 257, 300], "windows": [64, 64, 16, 48, 64, 32]}
VIT_PEAKS = [0, 31, 32, 63, 64, 127, 128, 255, 256, "last"]
VIT_LONG = [1408]
PREFILL_LENS, PREFILL_S_MAX = [36, 130, 257, 300], 320
PREFILL_HEADS = [(2, 1), (14, 2), (3, 3)]
PREFILL_LONG, PREFILL_LONG_S_MAX, PREFILL_LONG_HEADS = [1394, 77], 1408, (14, 2)
DECODE_HEADS = [(12, 2), (14, 2), (28, 4)]
DECODE_SPLITS = [8, 16, 32]
DECODE_S_MAX = 2176
DECODE_CTX = [0, 30, 31, 32, 63, 64, 2047, 2048, 2079, 2080, 2175]
DECODE_PEAKS = [0, 31, 32, 33, 63, 64, "ctx-1", "ctx"]
# two slots whose finished flag is set sit between the live ones: their workgroups must leave their records alone
DECODE_BATCH = [(0, 0), (30, 0), (77, 1), (31, 0), (32, 0), (63, 0), (64, 0), (2047, 0), (2048, 0), (2100, 1), (2079, 0),
                (2080, 0), (2175, 0)]
# the 17..32-row batch of kr_attn_decode_merge32: the same contexts and ten more on and beside unit borders
DECODE_BATCH32 = [(c, 0) for c in DECODE_CTX + [1, 33, 95, 96, 1023, 1024, 1393, 2015, 2016, 2111]]


def vit_patterns(lens: Sequence[int]) -> List[str]:
    """up, down and one tent per peak that fits at least one segment ('last' = every segment's last key)."""
    return ["up", "down"] + [f"tent-{p}" for p in VIT_PEAKS if p == "last" or any(p < n for n in lens)]


def decode_patterns() -> List[str]:
    return ["up", "down"] + [f"tent-{p}" for p in DECODE_PEAKS]


# ----------------------------------------------------------------------------- encoding
def channel_pairs(kv_heads: int, hd: int) -> List[Tuple[int, int]]:
    """(c_hi, c_lo) per kv head: two different 8-channel groups, no group shared between heads, different lanes of the
    group from head to head — head and channel addressing both take part, and another head's K rows score 0."""
    groups = hd // 8
    assert 2 * kv_heads <= groups, "not enough 8-channel groups for disjoint pairs"
    return [(8 * (2 * h) + (3 * h) % 8, 8 * (2 * h + 1) + (5 * h + 1) % 8) for h in range(kv_heads)]


def k_from_a(a: np.ndarray, hd: int) -> np.ndarray:
    """a int [..., KVH, R] -> K [..., KVH, R, hd]."""
    a = np.asarray(a)
    assert a.min() >= 0 and a.max() < 8192
    _assert_bf16_exact(a // 64, a % 64)
    k = np.zeros(a.shape + (hd,), np.float32)
    for h, (ch, cl) in enumerate(channel_pairs(a.shape[-2], hd)):
        k[..., h, :, ch] = a[..., h, :] // 64
        k[..., h, :, cl] = a[..., h, :] % 64
    return k


def q_vectors(heads: int, kv_heads: int, hd: int) -> np.ndarray:
    """[heads, hd]: the one query vector of each head (every query of a head is the same vector)."""
    q = np.zeros((heads, hd), np.float32)
    pairs = channel_pairs(kv_heads, hd)
    for h in range(heads):
        ch, cl = pairs[h // (heads // kv_heads)]
        q[h, ch], q[h, cl] = 64 * C_Q, C_Q
    _assert_bf16_exact(q)
    return q


def scale_log2e(hd: int) -> np.float32:
    """What the launchers pass to the kernels: float(hd^-0.5) * 1.4426950408889634f, in f32."""
    return np.float32(np.float32(hd ** -0.5) * LOG2E_F32)


def scores_log2(a: np.ndarray, hd: int, prescaled: bool = False) -> np.ndarray:
    """fp64 score of a row with ramp value a, in the kernels' log2 units.  prescaled: with q replaced by
    bf16_round(q * scale * log2e), what the hd 80 kernel multiplies K with."""
    a = np.asarray(a, np.int64)
    sl = scale_log2e(hd)
    if prescaled:
        qh, ql = (float(x) for x in bf16_round(np.asarray([64 * C_Q, C_Q], np.float32) * sl))
        return qh * (a // 64).astype(np.float64) + ql * (a % 64).astype(np.float64)
    return C_Q * a.astype(np.float64) * float(sl)


def check_gaps(a: np.ndarray, visible: np.ndarray, forbidden: Optional[np.ndarray], hd: int, what: str = "") -> np.ndarray:
    """a [R]; visible / forbidden bool [nq, R].  Returns the winner [nq] (numpy argmax of a over the visible rows) after
    asserting the two gap preconditions in fp64 (for hd 80 also with the kernel's bf16-rounded prescaled q)."""
    a = np.asarray(a, np.int64)
    nq = visible.shape[0]
    assert visible.any(1).all(), f"{what}: a query without a visible key"
    winner = np.where(visible, a[None], -1).argmax(1)
    for prescaled in ([False, True] if hd == 80 else [False]):
        s = scores_log2(a, hd, prescaled)
        sw = s[winner]
        others = np.where(visible, s[None], -np.inf)
        others[np.arange(nq), winner] = -np.inf
        lead = sw - others.max(1)
        assert (lead >= GAP).all(), f"{what}: a visible key comes within {lead.min():.1f} log2 units of the winner (prescaled={prescaled})"
        if forbidden is not None and forbidden.any():
            assert not (forbidden & visible).any()
            f = np.where(forbidden, s[None], np.inf).min(1)
            assert (f - sw >= GAP).all(), f"{what}: a forbidden row leads the winner by only {(f - sw).min():.1f} (prescaled={prescaled})"
    return winner


def ints_1_15(rng, *shape) -> np.ndarray:
    return rng.integers(1, 16, size=shape).astype(np.float32)


def _assert_bf16_exact(*arrays):
    for x in arrays:
        x = np.asarray(x, np.float32)
        np.testing.assert_array_equal(x, bf16_round(x))


_assert_bf16_exact(np.arange(16), STALE_V, C_Q, 64 * C_Q)     # every value a case stores


# ----------------------------------------------------------------------------- reference
def ref_attention(q, k, v, scale, causal, q_pos0=0):
    """q [H,nq,hd], k/v [KVH,nk,hd] -> [nq, H*hd]: the suite's fp64 softmax reference, restated."""
    H, nq, hd = q.shape
    KVH = k.shape[0]
    g = H // KVH
    out = np.zeros((nq, H, hd), np.float64)
    for h in range(H):
        s = (q[h].astype(np.float64) @ k[h // g].astype(np.float64).T) * scale
        if causal:
            mask = np.arange(k.shape[1])[None, :] <= (np.arange(nq)[:, None] + q_pos0)
            s = np.where(mask, s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
        out[:, h] = p @ v[h // g].astype(np.float64)
    return out.reshape(nq, H * hd).astype(np.float32)


# ----------------------------------------------------------------------------- expected rows and the diagnostic
@dataclass
class Unit:
    """The queries of one (segment or slot, q head): rows `rows` of the output, columns of head `head`; `cand` [R, hd]
    are the stored V rows they could have been given, `win` [nq] the ones they must be given."""
    rows: np.ndarray
    head: int
    cand: np.ndarray
    win: np.ndarray
    qname: Callable[[int], str]
    rname: Callable[[int], str]


@dataclass
class Case:
    hd: int
    heads: int
    kv_heads: int
    q: np.ndarray
    k: np.ndarray
    v: np.ndarray             # V rows in the shape POS.vt_blocks takes
    units: List[Unit] = field(default_factory=list)
    lens: Optional[List[int]] = None
    s_max: int = 0
    ctx: Optional[np.ndarray] = None
    finished: Optional[np.ndarray] = None

    @property
    def vt(self) -> np.ndarray:
        return POS.vt_blocks(self.v)

    def expected(self, n_rows: int) -> np.ndarray:
        out = np.zeros((n_rows, self.heads * self.hd), np.float32)
        for u in self.units:
            out[u.rows, u.head * self.hd:(u.head + 1) * self.hd] = u.cand[u.win]
        return out


def nearest_row(vec: np.ndarray, cand: np.ndarray) -> Tuple[int, float]:
    """The stored row whose V the output matches best (max abs error over the channels), and that error."""
    err = np.abs(cand.astype(np.float64) - vec.astype(np.float64)[None]).max(1)
    i = int(err.argmin())
    return i, float(err[i])


def check_output(got: np.ndarray, case: Case, what: str = "", max_lines: int = 6) -> None:
    """got [n_rows, heads*hd] against V[winner] within (TOL_REL, TOL_ABS); a failure names, per failing query, the
    stored row whose V came back."""
    lines, n_bad, n_all = [], 0, 0
    for u in case.units:
        g = got[u.rows, u.head * case.hd:(u.head + 1) * case.hd].astype(np.float64)
        want = u.cand[u.win].astype(np.float64)
        bad = (np.abs(g - want) > TOL_ABS + TOL_REL * np.abs(want)).any(1)
        n_all += bad.size
        n_bad += int(bad.sum())
        for i in np.flatnonzero(bad):
            if len(lines) >= max_lines:
                break
            j, e = nearest_row(g[i], u.cand)
            wj = u.cand[j].astype(np.float64)
            hit = bool((np.abs(g[i] - wj) <= TOL_ABS + TOL_REL * np.abs(wj)).all())
            if hit:
                src = f"returned {u.rname(j)}"
            elif not g[i].any():
                src = "returned zeros"
            elif not np.isfinite(g[i]).all():
                src = "returned non-finite values"
            else:
                src = f"returned no stored row (closest: {u.rname(j)}, max abs error {e:.4g}; first channels {g[i][:4]})"
            lines.append(f"{u.qname(int(i))} head {u.head} {src}, expected {u.rname(int(u.win[i]))}")
    assert n_bad == 0, f"{what}: {n_bad} of {n_all} (query, head) outputs are not V[winner]:\n  " + "\n  ".join(lines)


# ----------------------------------------------------------------------------- ViT: ragged storage, hd 80, not causal
def vit_case(lens: Sequence[int], pattern: str, hd: int = 80, heads: int = 4, seed: int = 0) -> Case:
    """K rows of the segments follow one another without padding ([heads, n, hd]); V^T starts a new 64-key block per
    segment, zero past the segment's last key (what kr_qkv_prep writes).  The ramp runs on across segment borders."""
    lens = [int(x) for x in lens]
    n, S = sum(lens), len(lens)
    r0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    nb = [(x + 63) // 64 for x in lens]
    vb0 = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
    seg_of = np.repeat(np.arange(S), lens)
    r = np.arange(n)
    if pattern == "up":
        a = r.copy()
    elif pattern == "down":
        a = n - 1 - r
    else:
        peak = pattern.split("-", 1)[1]
        A = 512
        a = np.zeros(n, np.int64)
        for s, ln in enumerate(lens):
            p = ln - 1 if peak == "last" or int(peak) >= ln else int(peak)
            a[r0[s]:r0[s] + ln] = A - np.abs(np.arange(ln) - p)
    rng = np.random.default_rng(seed + n)
    q = np.broadcast_to(q_vectors(heads, heads, hd)[:, None], (heads, n, hd)).copy()
    k = k_from_a(np.broadcast_to(a, (heads, n)), hd)
    v = np.zeros((heads, sum(nb) * 64, hd), np.float32)
    k2v = np.zeros(n, np.int64)
    for s, ln in enumerate(lens):
        v[:, vb0[s] * 64:vb0[s] * 64 + ln] = ints_1_15(rng, heads, ln, hd)
        k2v[r0[s]:r0[s] + ln] = vb0[s] * 64 + np.arange(ln)
    case = Case(hd, heads, heads, q, k, v, lens=lens)
    R = v.shape[1]
    v_seg = np.full(R, -1, np.int64)
    v_seg[k2v] = seg_of
    v_key = np.zeros(R, np.int64)
    v_key[k2v] = r - r0[seg_of]
    cand = v.reshape(heads * R, hd)

    def rname(i):
        h, j = divmod(i, R)
        where = f"key {v_key[j]} of segment {v_seg[j]}" if v_seg[j] >= 0 else f"V^T padding row {j}"
        return where + ("" if heads == 1 else f" (head {h})")

    for s, ln in enumerate(lens):
        vis = np.zeros((ln, n), bool)
        vis[:, r0[s]:r0[s] + ln] = True
        forb = None
        if pattern == "up":
            forb = np.zeros((ln, n), bool)
            forb[:, r0[s] + ln:] = True
        elif pattern == "down":
            forb = np.zeros((ln, n), bool)
            forb[:, :r0[s]] = True
        win = check_gaps(a, vis, forb, hd, f"vit {pattern} segment {s}")
        for h in range(heads):
            case.units.append(Unit(np.arange(r0[s], r0[s] + ln), h, cand, h * R + k2v[win],
                                   (lambda i, s=s: f"query {i} of segment {s}"), rname))
    return case


def vit_reference(case: Case) -> np.ndarray:
    out = np.zeros((sum(case.lens), case.heads * case.hd), np.float32)
    off = voff = 0
    for ln in case.lens:
        sl = slice(off, off + ln)
        out[sl] = ref_attention(case.q[:, sl], case.k[:, sl], case.v[:, voff:voff + ln], case.hd ** -0.5, False)
        off += ln
        voff += (ln + 63) // 64 * 64
    return out


# ----------------------------------------------------------------------------- prefill: cache layout, hd 128, causal, GQA
def prefill_case(lens: Sequence[int], heads: int, kv_heads: int, s_max: int, hd: int = 128, seed: int = 0) -> Case:
    """Sequence b lives in cache slot b ([B, KVH, s_max, hd]).  The ramp fills all s_max rows of every slot: up on even kv
    heads (every query's winner is its own diagonal key; the next key, masked only by causality, and the stale rows past
    the prompt outrank it), down on odd ones (key 0 wins) — a wrong GQA mapping returns the other kind of head's V.
    V^T is zero from the prompt's end to the end of its 64-key block (kr_qkv_prep) and stale beyond."""
    lens = [int(x) for x in lens]
    B, n, g = len(lens), sum(lens), heads // kv_heads
    r = np.arange(s_max)
    a = np.zeros((B, kv_heads, s_max), np.int64)
    a[:, 0::2] = r
    a[:, 1::2] = s_max - 1 - r
    rng = np.random.default_rng(seed + n + heads)
    q = np.broadcast_to(q_vectors(heads, kv_heads, hd)[:, None], (heads, n, hd)).copy()
    k = k_from_a(a, hd)
    v = ints_1_15(rng, B, kv_heads, s_max, hd)
    for b, ln in enumerate(lens):
        v[b, :, ln:(ln + 63) // 64 * 64] = 0
    case = Case(hd, heads, kv_heads, q, k, v, lens=lens, s_max=s_max)
    off = 0
    for b, ln in enumerate(lens):
        cand = v[b].reshape(kv_heads * s_max, hd)

        def rname(i, b=b, ln=ln):
            h, j = divmod(i, s_max)
            return f"key {j} of slot {b}, kv head {h}" + (" (past the prompt)" if j >= ln else "")

        vis = np.arange(s_max)[None, :] <= np.arange(ln)[:, None]
        for kvh in range(kv_heads):
            up = kvh % 2 == 0
            win = check_gaps(a[b, kvh], vis, ~vis if up else None, hd, f"prefill slot {b} kv head {kvh}")
            np.testing.assert_array_equal(win, np.arange(ln) if up else 0)
            for h in range(kvh * g, (kvh + 1) * g):
                case.units.append(Unit(np.arange(off, off + ln), h, cand, kvh * s_max + win,
                                       (lambda i, b=b: f"query {i} of segment {b}"), rname))
        off += ln
    return case


def prefill_reference(case: Case) -> np.ndarray:
    out = np.zeros((sum(case.lens), case.heads * case.hd), np.float32)
    off = 0
    for b, ln in enumerate(case.lens):
        sl = slice(off, off + ln)
        out[sl] = ref_attention(case.q[:, sl], case.k[b, :, :ln], case.v[b, :, :ln], case.hd ** -0.5, True)
        off += ln
    return out


# ----------------------------------------------------------------------------- decode: one query per slot, hd 128
def decode_case(batch: Sequence[Tuple[int, int]], heads: int, kv_heads: int, pattern: str, s_max: int = DECODE_S_MAX,
                hd: int = 128, seed: int = 0) -> Case:
    """batch: (ctx_len, finished) per slot; the query sees keys 0 .. ctx_len (the step's own key is row ctx_len).  The K ramp
    fills all s_max rows; the V^T columns past ctx_len hold the finite stale value a longer earlier page leaves."""
    ctx = np.asarray([c for c, _ in batch], np.int64)
    fin = np.asarray([f for _, f in batch], np.int32)
    B, g = len(batch), heads // kv_heads
    r = np.arange(s_max)
    if pattern == "up":
        a1 = np.broadcast_to(r, (B, s_max))
    elif pattern == "down":
        a1 = np.broadcast_to(s_max - 1 - r, (B, s_max))
    else:
        peak = pattern.split("-", 1)[1]
        p = ctx if peak == "ctx" else np.maximum(ctx - 1, 0) if peak == "ctx-1" else np.minimum(int(peak), ctx)
        a1 = 4096 - np.abs(r[None, :] - p[:, None])
    a = np.broadcast_to(a1[:, None], (B, kv_heads, s_max))
    rng = np.random.default_rng(seed + heads + B)
    q = np.broadcast_to(q_vectors(heads, kv_heads, hd)[None], (B, heads, hd)).copy()
    k = k_from_a(a, hd)
    v = ints_1_15(rng, B, kv_heads, s_max, hd)
    for b in range(B):
        v[b, :, ctx[b] + 1:] = STALE_V
    case = Case(hd, heads, kv_heads, q, k, v, s_max=s_max, ctx=ctx.astype(np.int32), finished=fin)
    for b in range(B):
        if fin[b]:
            continue
        vis = (r <= ctx[b])[None]
        win = check_gaps(a1[b], vis, ~vis if pattern == "up" else None, hd, f"decode {pattern} slot {b}")
        if pattern in ("up", "down"):
            assert win[0] == (ctx[b] if pattern == "up" else 0)
        cand = v[b].reshape(kv_heads * s_max, hd)

        def rname(i, b=b):
            h, j = divmod(i, s_max)
            return f"key {j} of kv head {h}" + (f" (a stale row: ctx_len is {ctx[b]})" if j > ctx[b] else "")

        for h in range(heads):
            case.units.append(Unit(np.asarray([b]), h, cand, (h // g) * s_max + win,
                                   (lambda i, b=b: f"slot {b} (ctx_len {ctx[b]})"), rname))
    return case


def decode_reference(case: Case, extra_keys: int = 0, whole_units_only: bool = False) -> np.ndarray:
    """extra_keys / whole_units_only restate two faults (one key too many; the last partial 32-key unit dropped): the
    CPU tests use them to show that the expected rows tell them from the right answer."""
    out = np.zeros((len(case.ctx), case.heads * case.hd), np.float32)
    for b, c in enumerate(case.ctx):
        nk = min(int(c) + 1 + extra_keys, case.s_max)
        if whole_units_only and nk >= 32:
            nk = nk // 32 * 32
        out[b] = ref_attention(case.q[b][:, None], case.k[b, :, :nk], case.v[b, :, :nk], case.hd ** -0.5, False)
    return out
