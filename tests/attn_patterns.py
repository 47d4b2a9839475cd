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

The fp8 KV cache (attn_decode2_kernel<KV8>) takes the same patterns in an encoding that is exact in e4m3 (the last section of
this file).  K holds the four base-16 digits of a(r) as e4m3 codes (0 .. 15 are exact) in four channels of its kv head, q holds
C_Q8 * (4096, 256, 16, 1) in the same channels (C_Q8 = 2048, powers of two, exact in bf16): q . value(K codes) = 2048 * a, an
exact integer below 2^24 for a < 8192.  The kernel's score is that integer times f32(f32(hd^-0.5 * log2 e) * k_scale[kvh]):
adjacent a are 261 * k_scale log2 units apart, so GAP holds for every k_scale >= 0.37 (check_gaps decides, per kv head, with
that folded f32 scale).  The four channels of a kv head lie in four different 16-channel groups, two in channels 0 .. 63 and
two in 64 .. 127 (both 16-byte loads of a K row; the bf16 cases leave 64 .. 127 empty); the two heads that meet in a group sit
in different 8-channel halves of it (both k-steps of a 16-byte piece), in both halves of either load also when there are only two kv
heads; no channel is shared, so another head's rows score 0; the lane inside the group differs from head to head
(kv8_channels asserts all of this for 1 .. 4 kv heads).  V codes are the integers 1 .. 15, a code stands for
value * v_scale[kvh]: the expected row is V_int * f32(v_scale).  Stale V^T columns hold code 0x7E (448).  Tolerance: the
same.  The winner's P is still exactly 1 (the f32 fold of k_scale moves every score of a head by the same factor, 2^-24
relative, far inside GAP), and the wave's O = V_int exactly is multiplied by v_scale once in f32 (2^-24) before the merge's one
bf16 rounding of the output: two 2^-24 terms inside the slack above.  (With power-of-two scales the output is V_int * v_scale
exactly; with the odd ones the bf16 rounding of that product is the whole error.)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from karanta_ocr_amd import positions as POS
from karanta_ocr_amd.weights import bf16_round, f32_to_fp8_e4m3, fp8_e4m3_to_f32
from tests import kv_fp8_ref as KV8R

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
# 43: the last unit ends inside its keys 8 .. 23 (12 keys), where a key-order permutation of the mask shows (the fp8 kernel's pi)
DECODE_CTX = [0, 30, 31, 32, 43, 63, 64, 2047, 2048, 2079, 2080, 2175]
DECODE_PEAKS = [0, 31, 32, 33, 63, 64, "ctx-1", "ctx"]
# two slots whose finished flag is set sit between the live ones: their workgroups must leave their records alone
DECODE_BATCH = [(0, 0), (30, 0), (77, 1), (31, 0), (32, 0), (43, 0), (63, 0), (64, 0), (2047, 0), (2048, 0), (2100, 1), (2079, 0),
                (2080, 0), (2175, 0)]
# the 17..32-row batch of kr_attn_decode_merge32: the border contexts and ten more on and beside unit borders (21 rows)
DECODE_BATCH32 = [(c, 0) for c in [0, 30, 31, 32, 63, 64, 2047, 2048, 2079, 2080, 2175, 1, 33, 95, 96, 1023, 1024, 1393, 2015, 2016, 2111]]


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


def check_gaps(a: np.ndarray, visible: np.ndarray, forbidden: Optional[np.ndarray], hd: int, what: str = "",
               kv8_k_scale: Optional[float] = None) -> np.ndarray:
    """a [R]; visible / forbidden bool [nq, R].  Returns the winner [nq] (numpy argmax of a over the visible rows) after
    asserting the two gap preconditions in fp64 (for hd 80 also with the kernel's bf16-rounded prescaled q).  kv8_k_scale: the
    scores are those of the e4m3 encoding under that K scale (scores_log2_kv8)."""
    a = np.asarray(a, np.int64)
    nq = visible.shape[0]
    assert visible.any(1).all(), f"{what}: a query without a visible key"
    winner = np.where(visible, a[None], -1).argmax(1)
    for prescaled in ([False, True] if hd == 80 else [False]):
        s = scores_log2(a, hd, prescaled) if kv8_k_scale is None else scores_log2_kv8(a, kv8_k_scale, hd)
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


# ----------------------------------------------------------------------------- the fp8 KV cache: an encoding exact in e4m3
C_Q8 = 2048.0
KV8_WEIGHTS = (4096, 256, 16, 1)                   # q holds C_Q8 times these; K holds the base-16 digits of a
KV8_CODE_OF_INT = f32_to_fp8_e4m3(np.arange(16, dtype=np.float32))
# [K | V][kv head] (the first kv_heads columns are used).  pow2: a wrong head's V scale is off by a factor >= 2 and K's entry of
# a head is not its V entry; odd: no power of two, K >= 0.37, cyclic neighbours' V scales >= 25 % apart
KV8_SCALE_SETS = {
    "unit": [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]],
    "pow2": [[1.0, 0.5, 4.0, 2.0], [0.5, 2.0, 0.25, 8.0]],
    "odd": [[0.37, 1.3, 0.73, 2.9], [1.9, 0.6, 1.45, 0.41]],
}
KV8_SCALE_NAMES = list(KV8_SCALE_SETS)
KV8_EXTRA_SPLITS = [1, 4]            # the split counts of the fp8 bound test that DECODE_SPLITS does not hold
KV8_ROWS_C, KV8_ROWS_SPLITS = [29, 30, 61, 62, 63], [2, 4]
KV8_FAULTS = ["mask-fg", "p-unpermuted", "v-scale-next-head", "v-tiles-swapped", "k-halves-swapped"]


def kv8_decode_params() -> List[Tuple[str, str]]:
    """(pattern, scale set) of the fp8 decode runs: every pattern at every scale set (a run takes ~0.1 s on the device)."""
    return [(p, s) for s in KV8_SCALE_NAMES for p in decode_patterns()]


def kv8_scales(name, kv_heads: int) -> np.ndarray:
    """[2][kv_heads] f32 of a named set (or of a table handed in)."""
    t = np.asarray(KV8_SCALE_SETS[name] if isinstance(name, str) else name, np.float32)[:, :kv_heads]
    assert t.shape == (2, kv_heads) and (t > 0).all()
    return np.ascontiguousarray(t)


def _check_scale_sets():
    for kvh in (1, 2, 4):
        assert (kv8_scales("unit", kvh) == 1).all()
        p, o = kv8_scales("pow2", kvh).astype(np.float64), kv8_scales("odd", kvh).astype(np.float64)
        assert (np.log2(p) % 1 == 0).all() and (np.log2(o) % 1 != 0).all() and (o[0] >= 0.37).all()
        assert (p[0] != p[1]).all() and (o[0] != o[1]).all()                      # K's entry read for V's shows
        for row, far in ((p[0], 2.0), (p[1], 2.0), (o[1], 1.25)) if kvh > 1 else ():
            r = row / np.roll(row, 1)
            assert (np.maximum(r, 1 / r) >= far).all(), "neighbouring heads' scales are too close"


def kv8_channels(kv_heads: int, hd: int = 128) -> List[Tuple[int, int, int, int]]:
    """The channels of the four digits (most significant first) per kv head; the placement the module docstring states, asserted."""
    assert hd == 128 and 1 <= kv_heads <= 4
    out = []
    for h in range(kv_heads):
        groups = (h % 4, (h + 2) % 4, 4 + (h + 1) % 4, 4 + (h + 3) % 4)
        out.append(tuple(16 * gr + 8 * ((h >> 1) ^ (i >> 1) ^ (h & 1)) + (2 * h + 3 * i) % 8 for i, gr in enumerate(groups)))
    flat = [c for t in out for c in t]
    assert len(set(flat)) == 4 * kv_heads and 0 <= min(flat) and max(flat) < hd                      # no channel shared
    for t in out:
        assert len({c // 16 for c in t}) == 4 and sorted(c // 64 for c in t) == [0, 0, 1, 1]           # 4 groups, two per load
    for i in range(4):
        assert len({t[i] % 16 for t in out}) == kv_heads                                                # the lane differs per head
    for half in (0, 1):                                                                                 # both k-steps of either load
        assert len({(c % 16) // 8 for c in flat if c // 64 == half}) == (2 if kv_heads > 1 else 1)
    by_group = {}
    for c in flat:
        by_group.setdefault(c // 16, []).append((c % 16) // 8)
    assert all(len(v) == len(set(v)) for v in by_group.values())                 # heads that meet in a group: different halves
    if kv_heads == 4:
        assert all(sorted(v) == [0, 1] for v in by_group.values()) and len(by_group) == 8
    return out


def kv8_k_codes(a: np.ndarray, hd: int = 128) -> np.ndarray:
    """a int [..., KVH, R] -> K codes uint8 [..., KVH, R, hd]: the base-16 digits of a in the head's four channels, 0 elsewhere."""
    a = np.asarray(a, np.int64)
    assert a.min() >= 0 and a.max() < 8192
    k = np.zeros(a.shape + (hd,), np.uint8)
    for h, chans in enumerate(kv8_channels(a.shape[-2], hd)):
        for c, w in zip(chans, KV8_WEIGHTS):
            k[..., h, :, c] = KV8_CODE_OF_INT[(a[..., h, :] // w) % 16]
    return k


def kv8_q_vectors(heads: int, kv_heads: int, hd: int = 128) -> np.ndarray:
    """[heads, hd]: C_Q8 * (4096, 256, 16, 1) in the four channels of the head's kv head."""
    q = np.zeros((heads, hd), np.float32)
    chans = kv8_channels(kv_heads, hd)
    for h in range(heads):
        for c, w in zip(chans[h // (heads // kv_heads)], KV8_WEIGHTS):
            q[h, c] = C_Q8 * w
    _assert_bf16_exact(q)
    return q


def scale_log2e_kv8(k_scale, hd: int = 128) -> np.float32:
    """The kernel's fold: f32(f32(hd^-0.5 * log2 e) * k_scale[kvh])."""
    return np.float32(scale_log2e(hd) * np.float32(k_scale))


def scores_log2_kv8(a: np.ndarray, k_scale, hd: int = 128) -> np.ndarray:
    """fp64 score, in the kernel's log2 units, of a K row that holds the digits of a, under that K scale."""
    return C_Q8 * np.asarray(a, np.int64).astype(np.float64) * float(scale_log2e_kv8(k_scale, hd))


def _check_kv8_encoding():
    np.testing.assert_array_equal(fp8_e4m3_to_f32(KV8_CODE_OF_INT), np.arange(16))                 # the digits are e4m3 values
    a = np.arange(8192)
    dig = np.stack([(a // w) % 16 for w in KV8_WEIGHTS], -1).astype(np.float32)
    s = np.zeros(8192, np.float32)
    for i, w in enumerate(KV8_WEIGHTS):                                          # f32 sums in any order: every partial sum is exact
        s = s + dig[:, i] * np.float32(C_Q8 * w)
    np.testing.assert_array_equal(s, np.float32(C_Q8) * a.astype(np.float32))
    assert C_Q8 * 8191 < 2 ** 24
    assert fp8_e4m3_to_f32(np.asarray([KV8R.STALE_CODE], np.uint8))[0] == 448.0
    _check_scale_sets()
    for kvh in (1, 2, 3, 4):
        kv8_channels(kvh)


@dataclass
class Case8:
    """A decode case on an fp8 cache.  q [rows, heads, hd] (bf16 values), k_codes / v_codes uint8 [slots, KVH, s_max, hd] (v_codes
    token-major: `vt` is what the kernel reads), scales [2][KVH] f32; row r reads slot row_slot[r] (None: slot r)."""
    hd: int
    heads: int
    kv_heads: int
    q: np.ndarray
    k_codes: np.ndarray
    v_codes: np.ndarray
    scales: np.ndarray
    s_max: int
    ctx: np.ndarray
    finished: np.ndarray
    row_slot: Optional[np.ndarray] = None
    units: List[Unit] = field(default_factory=list)

    @property
    def vt(self) -> np.ndarray:
        return KV8R.vt_blocks8(self.v_codes)

    def slot_of(self, r: int) -> int:
        return r if self.row_slot is None else int(self.row_slot[r])


def _kv8_case(a_slots: np.ndarray, ctx: np.ndarray, fin: np.ndarray, row_slot: Optional[np.ndarray], heads: int, kv_heads: int,
              scales, s_max: int, forbid_past_ctx: bool, seed: int, what: str) -> Case8:
    """a_slots int [slots, s_max]: the ramp of every slot's K rows (the same for all its kv heads).  V holds codes of 1 .. 15 up to
    the longest context on the slot and STALE_CODE beyond; the candidates of a row are all V rows of its slot, times v_scale."""
    hd, g = 128, heads // kv_heads
    S, rows = a_slots.shape[0], len(ctx)
    sc = kv8_scales(scales, kv_heads)
    slot = np.arange(rows) if row_slot is None else np.asarray(row_slot, np.int64)
    rng = np.random.default_rng(seed + heads + rows)
    q = np.broadcast_to(kv8_q_vectors(heads, kv_heads, hd)[None], (rows, heads, hd)).copy()
    k_codes = kv8_k_codes(np.broadcast_to(a_slots[:, None], (S, kv_heads, s_max)), hd)
    v_int = rng.integers(1, 16, size=(S, kv_heads, s_max, hd))
    v_codes = KV8_CODE_OF_INT[v_int]
    last = np.full(S, -1, np.int64)
    np.maximum.at(last, slot, ctx)
    for s in range(S):
        v_codes[s, :, last[s] + 1:] = KV8R.STALE_CODE
    case = Case8(hd, heads, kv_heads, q, k_codes, v_codes, sc, s_max, ctx.astype(np.int32), fin.astype(np.int32),
                 None if row_slot is None else slot.astype(np.int32))
    # V_int * f32(v_scale), kept in f32 (one rounding of 2^-24, the kernel's own)
    cands = [(fp8_e4m3_to_f32(v_codes[s]) * sc[1][:, None, None]).reshape(kv_heads * s_max, hd) for s in range(S)]
    r_ = np.arange(s_max)
    for r in range(rows):
        if fin[r]:
            continue
        s, vis = int(slot[r]), (r_ <= ctx[r])[None]
        for kvh in range(kv_heads):          # the gap is asserted per kv head: its K scale is in the score
            win = check_gaps(a_slots[s], vis, ~vis if forbid_past_ctx else None, hd, f"{what} row {r} kv head {kvh}", kv8_k_scale=sc[0, kvh])

            def rname(i, r=r, s=s):
                h, j = divmod(i, s_max)
                return f"key {j} of kv head {h}" + ("" if row_slot is None else f" of slot {s}") + \
                    (f" (a stale row: ctx_len is {ctx[r]})" if j > ctx[r] else "")

            for h in range(kvh * g, (kvh + 1) * g):
                case.units.append(Unit(np.asarray([r]), h, cands[s], kvh * s_max + win,
                                       (lambda i, r=r: ("slot" if row_slot is None else "row") + f" {r} (ctx_len {ctx[r]})"), rname))
    return case


def decode_case_kv8(batch: Sequence[Tuple[int, int]], heads: int, kv_heads: int, pattern: str, scales,
                    s_max: int = DECODE_S_MAX, seed: int = 0) -> Case8:
    """decode_case on an fp8 cache: the same (ctx_len, finished) batches and patterns.  scales: a name of KV8_SCALE_SETS or a
    [2][kv_heads] table.  The K ramp fills all s_max rows (with `up` every row past the context outranks the winner); the V^T
    columns past ctx_len hold STALE_CODE."""
    ctx = np.asarray([c for c, _ in batch], np.int64)
    fin = np.asarray([f for _, f in batch], np.int32)
    B, r = len(batch), np.arange(s_max)
    assert ctx.max() <= s_max - 1
    if pattern == "up":
        a1 = np.broadcast_to(r, (B, s_max))
    elif pattern == "down":
        a1 = np.broadcast_to(s_max - 1 - r, (B, s_max))
    else:
        peak = pattern.split("-", 1)[1]
        p = ctx if peak == "ctx" else np.maximum(ctx - 1, 0) if peak == "ctx-1" else np.minimum(int(peak), ctx)
        a1 = 4096 - np.abs(r[None, :] - p[:, None])
    case = _kv8_case(np.ascontiguousarray(a1), ctx, fin, None, heads, kv_heads, scales, s_max, pattern == "up", seed, f"kv8 decode {pattern}")
    if pattern in ("up", "down"):
        for u in case.units:
            assert u.win[0] % s_max == (ctx[u.rows[0]] if pattern == "up" else 0)
    return case


def rows_case_kv8(c: int, scales="odd", heads: int = 4, kv_heads: int = 2, drafts: int = 3, s_max: int = 128) -> Case8:
    """The speculative step on an fp8 cache: rows j = 0 .. drafts of slot 0 at contexts c + j and of slot 1 at c + 32 + j, behind the
    row map row -> slot (1, 0, 1, 0, ...); `up` ramps, so the keys the later draft rows stored — real V codes — outrank a row's own."""
    rows = 2 * (drafts + 1)
    row_slot = np.asarray([(r + 1) % 2 for r in range(rows)], np.int64)
    ctx = np.asarray([(c if row_slot[r] == 0 else c + 32) + r // 2 for r in range(rows)], np.int64)
    assert ctx.max() <= s_max - 1
    a = np.broadcast_to(np.arange(s_max), (2, s_max)).copy()
    case = _kv8_case(a, ctx, np.zeros(rows, np.int32), row_slot, heads, kv_heads, scales, s_max, True, 7 * c, f"kv8 rows c={c}")
    for u in case.units:
        assert u.win[0] % s_max == ctx[u.rows[0]]
    assert (case.v_codes[0, :, :c + drafts + 1] != KV8R.STALE_CODE).all() and (case.v_codes[0, :, c + drafts + 1:] == KV8R.STALE_CODE).all()
    return case


def kv8_swap_8_16(key: np.ndarray) -> np.ndarray:
    """Keys 8 .. 15 and 16 .. 23 of every 32-key unit exchanged: pi = (0, 2, 1, 3) on the unit's four 8-key groups."""
    key = np.asarray(key, np.int64)
    grp = (key >> 3) & 3
    return key + 8 * (np.asarray([0, 2, 1, 3])[grp] - grp)


def decode_reference_kv8(case: Case8, extra_keys: int = 0, whole_units_only: bool = False, fault: Optional[str] = None) -> np.ndarray:
    """The fp64 softmax over the DEQUANTISED operands (kv_fp8_ref.dequantize) of every live row.  extra_keys / whole_units_only as in
    decode_reference; fault restates one addressing error of the fp8 kernel (KV8_FAULTS):
      mask-fg            the mask computed with fg in place of pi(fg): the visible set with keys 8..15 and 16..23 of a unit exchanged
      p-unpermuted       P applied to V in unpermuted key order: key k's weight meets V of key swap(k)
      v-scale-next-head  the V scale of kv head (h + 1) % KVH
      v-tiles-swapped    channel tiles 2i and 2i + 1 of V exchanged
      k-halves-swapped   K channels 0..63 exchanged with 64..127, on the K side only"""
    assert fault is None or fault in KV8_FAULTS
    H, KVH, hd = case.heads, case.kv_heads, case.hd
    g = H // KVH
    out = np.zeros((len(case.ctx), H * hd), np.float32)
    for r, c in enumerate(case.ctx):
        if case.finished[r]:
            continue
        s = case.slot_of(r)
        nk = min(int(c) + 1 + extra_keys, case.s_max)
        if whole_units_only and nk >= 32:
            nk = nk // 32 * 32
        key = np.arange((nk + 31) // 32 * 32)                      # the whole units the kernel loads: inside the cache
        vis = (kv8_swap_8_16(key) if fault == "mask-fg" else key) < nk
        vkey = kv8_swap_8_16(key) if fault == "p-unpermuted" else key
        for kvh in range(KVH):
            kd = KV8R.dequantize(case.k_codes[s, kvh, key], case.scales[0, kvh])
            if fault == "k-halves-swapped":
                kd = np.roll(kd, 64, -1)
            vd = KV8R.dequantize(case.v_codes[s, kvh, vkey], case.scales[1, (kvh + 1) % KVH if fault == "v-scale-next-head" else kvh])
            for h in range(kvh * g, (kvh + 1) * g):
                sc = np.where(vis, kd @ case.q[r, h].astype(np.float64) * hd ** -0.5, -np.inf)
                p = np.exp(sc - sc.max())
                o = (p / p.sum()) @ vd
                if fault == "v-tiles-swapped":
                    o = o.reshape(hd // 32, 2, 16)[:, ::-1].reshape(hd)
                out[r, h * hd:(h + 1) * hd] = o
    return out


def max_ratio(got: np.ndarray, case) -> float:
    """max |got - V[winner]| / (TOL_ABS + TOL_REL |V[winner]|) over the case's units (<= 1: check_output passes)."""
    worst = 0.0
    for u in case.units:
        g = got[u.rows, u.head * case.hd:(u.head + 1) * case.hd].astype(np.float64)
        want = u.cand[u.win].astype(np.float64)
        worst = max(worst, float((np.abs(g - want) / (TOL_ABS + TOL_REL * np.abs(want))).max()))
    return worst


_check_kv8_encoding()
