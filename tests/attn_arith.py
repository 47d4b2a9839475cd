"""Attention inputs whose outputs are O(1) and whose softmax arithmetic matters: the denominator, the rescale factors, the
accumulation over tiles / units and the merges (not a test module; shared by test_attn_arith_cpu.py, which proves every
case on the reference alone, and test_gpu_attention_arith.py, which runs the three kernels on them).

Scores.  The channels of a head are split in two directions, U (even channels) and W (odd channels), each with a fixed
sign pattern.  A query is g * (signs on U) + h * (signs on W) for two bf16 gains (g, h); a K row carries a target T on U
and a target T' on W, spread over the channels so that the signed channel sum is T (T') to ~2^-18 relative although every
channel is a rounded bf16 value with noise of its own (`spread`).  The score of (query, key) is therefore
gamma(g) * T + gamma(h) * T' with gamma(x) = x * scale * log2(e) at hd 128 and gamma(x) = bf16(f32(x) * f32(scale_log2e)) at
hd 80 — the rounding the hd 80 kernel documents at PRESCALE; the gains are taken from candidates whose product is not within
2^-20 relative of a bf16 tie (`tie_margin`), so the rounded value does not depend on how the constant was rounded.  T is
the wanted level in log2 units divided by gamma(1): a query with g = 1 sees the profile as written, other gains see it
stretched, so the 32 queries of a wave walk different trajectories.  Only one query per wave has h != 0 and only one key per
profile has T' != 0: that query alone rises in the tile where its neighbours stay or fall.

Reference: plain softmax in float64 over the operands as stored (hd 80: with q~ = bf16(q * scale_log2e)), no rounding of P.

Bound.  With p the reference weights and o the reference output of (query, channel d):

    E = (2^-9 + 2^-12) * sum_j p_j |v_jd| + 2^-9 * |o|                                              (the first line)   
        + 2^-9 * sum_j p_j |v_jd|                                                                    (term A)
        + 2^-9 * |o|                                                                                 (term B)
        + 2^-8 * (sum_j p_j |v_jd| + |o|) * 2^-7   where l sums the rounded P (hd 80, decode)        (term C, second order)
        + 2^-8 * |o|                               where l sums the rounded P (hd 80, decode)        (term C)
        + 2^-125 * n_keys * max_j |v_jd|                                                             (term D)

  The first line is the derivation this module started from: round-to-nearest of every P entry to bf16, the output's own
  rounding, and 2^-12 for every fp32 effect (v_exp_f32, the score accumulation at |s| <~ 2^7, 1/l, the merge factors).
  It takes 2^-9 for the relative error of one bf16 rounding.  That is the error at the TOP of a binade: bf16 keeps 8
  significant bits, the spacing in [1, 2) is 2^-7, so round-to-nearest errs by up to 2^-8 relative just above a power of
  two (1 + 2^-8 rounds to 1).  test_attn_arith_cpu.py shows it on the reference alone: the kernels' own arithmetic
  restated in float64 with P rounded to bf16 (`model(..., round_p=True)`) exceeds the first line, and so do the kernels
  (measured on an MI355X against the first line alone: hd 128 prefill 1.28, decode 1.15; hd 80 0.90).
  Term A makes the P rounding 2^-8 (unit roundoff of bf16) and term B does the same for the output's rounding.
  Term C: the hd 80 kernel (ones row) and the decode kernel (psum of the rounded values) divide by l~ = sum p_j (1 + d_j),
  |d_j| <= 2^-8: got = sum p_j (1 + d_j) v_j / l~, so got - o = sum p_j d_j (v_j - o) / (l~ / l), bounded by
  2^-8 (sum p|v| + |o|) / (1 - 2^-8): the |o| part is new (the hd 128 varlen kernel sums the unrounded P and does not
  have it), and 1 / (1 - 2^-8) < 1 + 2^-7 gives the second-order part.
  Term D is the underflow of the formats, not a tolerance: the lazy profiles fall by 140 and rise by 160 on purpose, so a
  class-indicator channel whose class only occurs among the keys 2^-140 below the maximum has a reference output of 1e-45,
  which neither an f32 P (smallest normal 2^-126) nor a bf16 output can hold: the kernels return 0.  Every P entry is held
  relative to a reference that is at most the running maximum, so the key at the maximum has P >= 1 and l >= 1 in the units
  of the final reference, and every rescale factor is <= 1: a P entry or a product P * v that is flushed is wrong by at most
  2^-126 |v| in those units, n_keys of them by n_keys * 2^-126 max|v|; the factor 2 covers the flush of an accumulator on a
  rescale and of the output.  With |v| = O(1) that is 1e-35.  There is no other absolute floor and there are no excused elements.

Measured on an MI355X, max |got - o| / E: hd 80 varlen 0.31, hd 128 varlen (prefill) 0.75, decode + merge / merge32 0.40, the
same at both query-block sizes and at every split count.  The constant channels came back bit for bit from all three kernels
(hd 128 prefill included, where a neighbouring bf16 value would have been allowed for the queries with a weight above 1/64).

Families (each for the ViT hd 80 kernel, the causal hd 128 prefill kernel and the decode kernels):
  mass   keys in four classes half a log2 unit apart, tile / unit offsets of 0 .. -3 log2 units, gains within 1/16 of 1, and V
         scaled per tile (64 keys) or unit (32 keys) by the power of two inverse to its softmax mass: every tile carries a
         comparable part of sum p|v| (`contribution_ok`), so a dropped, doubled or mis-scaled tile moves the output.
  lazy   tile maxima that walk the lazy-rescale state machine of attn_varlen_kernel (`VIT_REL`, `PREFILL_REL`: levels relative to
         the running reference) resp. the in-wave and merge transitions of the decode kernel (`DECODE_LEVELS`).  V is again
         scaled inverse to the tile's mass (2^(highest level - the tile's level), at most 2^100): a rise of 8.5 leaves 2^-8.5 of
         what was accumulated before it, and without the scale a wrong alpha there would move the output by less than E.
  sum1-mass, sum1-lazy   the same scores with every V channel constant over the keys: the weights must sum to one.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from karanta_ocr_amd import positions as POS
from karanta_ocr_amd.weights import bf16_round

F32, F64 = np.float32, np.float64
LOG2E_F32 = F32(1.4426950408889634)

# ----------------------------------------------------------------------------- the parametrisations (CPU proof = GPU run)
FAMILIES = ["mass", "lazy", "sum1-mass", "sum1-lazy"]
VIT_LENS, VIT_HEADS = [577, 40, 200], 2
PREFILL_LENS, PREFILL_SLOTS, PREFILL_N_SLOTS, PREFILL_S_MAX = [449, 97], [1, 0], 3, 512
PREFILL_HEADS = [(4, 2), (7, 1)]
DECODE_HEADS = [(12, 2), (28, 4)]
DECODE_CTX, DECODE_S_MAX = [30, 31, 95, 700, 1055], 1088
DECODE_FINISHED_CTX = 333                 # one finished row between the live ones
DECODE_SPLITS = [1, 4, 8, 16, 32]
DECODE_BATCH32 = 21

# tile maxima relative to the running reference of a g = 1 query (first entry: absolute), per (segment, head % 2)
VIT_REL = {
    (0, 0): [60, 7.5, 0, 8.5, 6, 12, -30, 40, -140, 9],          # 577 keys: 10 tiles, the last one key wide and rising
    (1, 0): [-40],
    (2, 0): [-100, 160, 6, 12],                                   # 200 keys: the ragged tile takes the second rise of 6
    (0, 1): [-40, 160, -140, 9, 7.5, 0, 8.5, 6, 12, -30],
    (1, 1): [60],
    (2, 1): [60, -30, 40, 9],
}
PREFILL_REL = {
    (0, 0): [60, 7.5, 0, 8.5, 6, 12, 0, 9],                       # 449 keys: 8 tiles, the last one key wide and rising
    (1, 0): [-40, 160],                                           # 97 keys: 33 in the ragged tile
    (0, 1): [-40, 160, -140, 40, 0, 0, -30, 9],
    (1, 1): [60, -30],
}
# decode, level of 32-key unit u = DECODE_LEVELS[u // 8][u % 8]: with one split wave w walks units w, w + 8, ... (a column);
# units 8..15 are a whole split at 4 and more splits, 150 below the others
DECODE_LEVELS = [
    [0, -40, 7.5, -8.5, 3, -3, 1, -1],
    [-160, -158, -162, -159, -161, -160, -157, -163],
    [40, 20, 7.5, 31.5, -137, 37, 41, 39],
    [40, 41, 39, 40, 38, 42, 40, 41],
    [49],
]
VIT_PEAK_LAST = {(0, 1): [8]}     # tiles whose maximum sits on their LAST key and stands 3 above the rest: the key a short ones row loses
V_EXP_MAX = 100              # lazy: V of a tile is scaled by 2^min(100, highest level - the tile's level)
SPIKE_UNIT_TILE = 2          # the tile whose one key carries T' (the query with h = 1 rises by 9 there)

MASS_GAINS = [1.0, 1.03125, 0.96875, 1.0625, 0.9375]
LAZY_GAINS = [1.0, 1.0, 1.0, 0.75, 1.0, 0.5, 1.0, 1.0]
LOW_GAINS = [1.0, 2.0, 4.0]          # the one-tile segment at -40: the gain-4 queries see -160
V_MANT = np.asarray([1.0, 1.25, 1.5], F32)
SUM1_VALUES = [1.5, 0.75, -3.0, 1.0 + 2.0 ** -7] + [s * 2.0 ** e for e in range(-6, 7) for s in (1.0, -1.0)]
N_CLASS = 4
STALE_V, STALE_K = 24576.0, 8.0     # large finite values where a correct kernel must not read


def is_bf16(*arrays) -> bool:
    return all(np.array_equal(np.asarray(x, F32), bf16_round(np.asarray(x, F32))) for x in arrays)


def scale_log2e(hd: int) -> np.float32:
    """What attn_varlen_impl and attn_decode_impl pass to the kernels: `scale * 1.4426950408889634f` in f32, scale = float(hd^-0.5)."""
    return F32(F32(hd ** -0.5) * LOG2E_F32)


def q_tilde(q: np.ndarray, hd: int) -> np.ndarray:
    """bf16(f32(q) * f32(scale_log2e)): the operand the hd 80 kernel multiplies K with (PRESCALE)."""
    return bf16_round(np.asarray(q, F32) * scale_log2e(hd))


def tie_margin(q: np.ndarray, hd: int) -> float:
    """Smallest relative distance of q * scale_log2e (exact product of the two f32 values) from a bf16 rounding tie, over
    the non-zero elements of q."""
    x = np.abs(np.asarray(q, F64).ravel()) * F64(scale_log2e(hd))
    x = x[x > 0]
    e = np.floor(np.log2(x))
    ulp = 2.0 ** (e - 7)                       # bf16 spacing in the binade of x
    frac = np.mod(x / ulp, 1.0)                # a tie sits at frac = 0.5
    return float((np.abs(frac - 0.5) * ulp / x).min())


def gamma(g, hd: int) -> np.ndarray:
    """Score per unit of key target for a query of gain g, in log2 units."""
    g = np.asarray(g, F32)
    return q_tilde(g, hd).astype(F64) if hd == 80 else g.astype(F64) * F64(F32(hd ** -0.5)) * F64(LOG2E_F32)


def pick_gains(cands: Sequence[float], hd: int) -> List[float]:
    """The candidates whose prescaled product keeps 2^-20 from a bf16 tie (all of them are kept at hd 128, which does not round q)."""
    out = [g for g in cands if hd != 80 or tie_margin(np.asarray([g]), hd) > 2.0 ** -20]
    assert out and out[0] == 1.0, "the unit gain itself sits on a tie"
    return out


def signs(hd: int) -> np.ndarray:
    return np.where((np.arange(hd) * 7 + np.arange(hd) // 3) % 5 < 2, -1.0, 1.0).astype(F32)


def spread(T: np.ndarray, m: int, rng, noise: float) -> np.ndarray:
    """[n] targets -> [n, m] bf16 values whose row sums are T to ~2^-18 relative: channels 0 .. m-3 take the running mean of
    what is left plus noise, channel m-2 all that is left, channel m-1 that value's rounding error."""
    T = np.asarray(T, F64)
    out = np.zeros((T.size, m), F32)
    res = T.copy()
    for c in range(m):
        if c < m - 2:
            x = res / (m - c) + rng.uniform(-noise, noise, T.size) * (T != 0)
        else:
            x = res
        out[:, c] = bf16_round(x.astype(F32))
        res = res - out[:, c].astype(F64)
    return out


def levels_from_rel(rel: Sequence[float]) -> List[float]:
    """Absolute tile maxima from maxima relative to the lazy reference (which moves when a maximum exceeds it by more than 8)."""
    ref = float(rel[0])
    out = [ref]
    for r in rel[1:]:
        out.append(ref + r)
        if r > 8:
            ref += r
    return out


# ----------------------------------------------------------------------------- problems and cases
@dataclass
class Prob:
    """The queries of one (segment or slot, q head) over their keys: one softmax problem per query."""
    rows: np.ndarray                 # output rows
    head: int
    kvh: int
    q: np.ndarray                    # [nq, hd]
    k: np.ndarray                    # [nk, hd] the visible keys
    v: np.ndarray                    # [nk, hd]
    qpos: Optional[np.ndarray]       # causal: key j is visible iff j <= qpos[i]
    unit: int                        # 64 (varlen tile) or 32 (decode unit)
    exact: np.ndarray                # bool [nq]: g = 1, the queries meant to take the profile as written
    name: str = ""


@dataclass
class Case:
    kind: str                        # vit | prefill | decode
    family: str
    hd: int
    heads: int
    kv_heads: int
    q: np.ndarray
    k: np.ndarray
    v: np.ndarray                    # V rows in the shape POS.vt_blocks takes
    probs: List[Prob] = field(default_factory=list)
    lens: Optional[List[int]] = None
    slots: Optional[List[int]] = None
    s_max: int = 0
    ctx: Optional[np.ndarray] = None
    finished: Optional[np.ndarray] = None
    const: Optional[np.ndarray] = None      # sum1: [kv_heads, hd] the value of every channel
    n_rows: int = 0

    @property
    def vt(self) -> np.ndarray:
        return POS.vt_blocks(self.v)

    @property
    def sum1(self) -> bool:
        return self.family.startswith("sum1")

    @property
    def scores(self) -> str:
        return self.family.split("-")[-1]

    @property
    def l_rounded(self) -> bool:
        """hd 80 (ones row) and decode (psum of bf16 values) sum the rounded P; the hd 128 varlen kernel the f32 P."""
        return self.kind != "prefill"


def scores_log2(case: Case, pr: Prob) -> np.ndarray:
    """[nq, nk] float64 scores in log2 units over the stored operands, -inf where masked."""
    if case.hd == 80:
        s = q_tilde(pr.q, 80).astype(F64) @ pr.k.astype(F64).T
    else:
        s = (pr.q.astype(F64) @ pr.k.astype(F64).T) * F64(F32(case.hd ** -0.5)) * F64(LOG2E_F32)
    if pr.qpos is not None:
        s = np.where(np.arange(pr.k.shape[0])[None, :] <= pr.qpos[:, None], s, -np.inf)
    return s


def reference(case: Case, pr: Prob):
    """(o, sum p|v|, largest weight) in float64: plain softmax, no rounding of P."""
    s = scores_log2(case, pr)
    p = np.exp2(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    v = pr.v.astype(F64)
    return p @ v, p @ np.abs(v), p.max(1)


def bound(case: Case, pr: Prob, o: np.ndarray, spv: np.ndarray, first_line_only: bool = False) -> np.ndarray:
    """E per output element (module docstring)."""
    e = (2.0 ** -9 + 2.0 ** -12) * spv + 2.0 ** -9 * np.abs(o)
    if first_line_only:
        return e
    e = e + 2.0 ** -9 * spv + 2.0 ** -9 * np.abs(o)
    if case.l_rounded:
        e = e + 2.0 ** -8 * np.abs(o) + 2.0 ** -15 * (spv + np.abs(o))
    return e + 2.0 ** -125 * pr.k.shape[0] * np.abs(pr.v.astype(F64)).max(0)[None, :]


# ----------------------------------------------------------------------------- builders
def _key_levels(n: int, unit: int, unit_levels: Sequence[float], rng, peak_last: Sequence[int] = ()) -> Tuple[np.ndarray, np.ndarray]:
    """lazy: the level of every key.  One key of every tile / unit carries the tile maximum exactly (its position moves from tile
    to tile; the tiles in `peak_last` have it on their last key), the others lie 0.8 .. 1.0 below: a causal query that sees a tile
    without its peak key rises 7.5 .. 7.7 where the profile says 8.5, on the same side of the threshold as 7.5."""
    a = np.zeros(n, F64)
    peaks = []
    for t in range((n + unit - 1) // unit):
        lo, hi = t * unit, min(n, (t + 1) * unit)
        a[lo:hi] = unit_levels[t] - (3.0 if t in peak_last else 0.8) - rng.uniform(0.0, 0.2, hi - lo)
        p = hi - 1 if t in peak_last else lo + (7 + 11 * t) % (hi - lo)
        a[p] = unit_levels[t]
        peaks.append(p)
    return a, np.asarray(peaks)


def _mass_levels(n: int, unit: int, rng, decay: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """mass: (level, class, log2 of the V scale) per key.  Classes half a log2 unit apart, +-1/8 noise, an optional decay along the
    tile (causal: most of a tile's mass then sits on its first keys, so a query a few keys into its diagonal tile already sees
    it), and a tile offset chosen so that the tile's mass is 2^k (k = 0 .. -3) times the mean: V is scaled by 2^-k."""
    cls = rng.integers(0, N_CLASS, n)
    a = -0.5 * cls - decay * (np.arange(n) % unit) + rng.uniform(-0.125, 0.125, n)
    ve = np.zeros(n, np.int64)
    nt = (n + unit - 1) // unit
    for t in range(nt):
        lo, hi = t * unit, min(n, (t + 1) * unit)
        k = -int(rng.integers(0, 4))
        a[lo:hi] += k - np.log2(np.exp2(a[lo:hi]).sum())
        ve[lo:hi] = -k
    return a, cls, ve


def _values(cls: np.ndarray, vexp: np.ndarray, hd: int, rng) -> np.ndarray:
    """V rows: class indicators, then non-negative dyadic channels, then mixed-sign ones, the last two scaled by 2^vexp."""
    n = cls.size
    v = np.zeros((n, hd), F32)
    v[np.arange(n), cls] = 1.0
    half = hd // 2
    sc = np.exp2(vexp.astype(F64)).astype(F32)[:, None]
    v[:, N_CLASS:half] = V_MANT[rng.integers(0, V_MANT.size, (n, half - N_CLASS))] * sc
    v[:, half:] = V_MANT[rng.integers(0, V_MANT.size, (n, hd - half))] * rng.choice(np.asarray([-1.0, 1.0], F32), (n, hd - half)) * sc
    return v


def nonneg_channels(hd: int) -> slice:
    return slice(N_CLASS, hd // 2)


def _const_values(kv_heads: int, hd: int, rng) -> np.ndarray:
    c = np.asarray(SUM1_VALUES, F32)[rng.integers(0, len(SUM1_VALUES), (kv_heads, hd))]
    c[:, :4] = np.asarray([1.5, 0.75, -3.0, 1.0 + 2.0 ** -7], F32)
    return c


def _k_rows(level: np.ndarray, spike: np.ndarray, hd: int, rng) -> np.ndarray:
    """K rows from the level per key (log2 units at g = 1) and the spike per key (log2 units at h = 1)."""
    g1 = float(gamma(np.asarray([1.0]), hd)[0])
    s = signs(hd)
    k = np.zeros((level.size, hd), F32)
    k[:, 0::2] = spread(level / g1, (hd + 1) // 2, rng, 0.25) * s[0::2]
    k[:, 1::2] = spread(spike / g1, hd // 2, rng, 0.25) * s[1::2]
    return k


def _q_rows(g: np.ndarray, h: np.ndarray, hd: int) -> np.ndarray:
    s = signs(hd)
    q = np.zeros((g.size, hd), F32)
    q[:, 0::2] = g[:, None].astype(F32) * s[0::2]
    q[:, 1::2] = h[:, None].astype(F32) * s[1::2]
    return q


def _gains(n: int, cands: Sequence[float], hd: int, rng, spike: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(g, h) per query: g is drawn from the candidates; with `spike` one g = 1 query of every wave of 32 has
    h = 1."""
    cands = pick_gains(cands, hd)
    g = np.asarray(cands, F64)[rng.integers(0, len(cands), n)]
    h = np.zeros(n, F64)
    if spike:
        for w in range((n + 31) // 32):
            i = min(n - 1, w * 32 + (5 + 7 * w) % 32)
            g[i], h[i] = 1.0, 1.0
    return g, h


def _segment(scores: str, n: int, unit: int, rel: Optional[Sequence[float]], hd: int, rng, vrng, causal: bool, sum1: bool,
             const: Optional[np.ndarray], levels: Optional[Sequence[float]] = None, low: bool = False, peak_last: Sequence[int] = ()):
    """K rows, V rows and the per-query gains of one segment / slot of n keys (and, for varlen, n queries).  Scores come from `rng`,
    values from `vrng`: a sum1 case has the K and q of the case whose scores it names, bit for bit."""
    if scores == "mass":
        a, cls, vexp = _mass_levels(n, unit, rng, 0.15 if causal else 0.0)
        spike = np.zeros(n, F64)
        cands = MASS_GAINS
    else:
        lv = list(levels) if levels is not None else levels_from_rel(rel)
        nt = (n + unit - 1) // unit
        assert len(lv) >= nt, (len(lv), nt)
        a, peaks = _key_levels(n, unit, lv, rng, peak_last)
        # V inverse to the tile's softmax mass (as a g = 1 query sees it), so that what was accumulated before a rescale still
        # shows in the output after it; beyond 2^100 (tiles that underflow anyway) the scale stops
        cls = rng.integers(0, N_CLASS, n)
        top = max(lv[:nt])
        vexp = np.repeat(np.minimum(V_EXP_MAX, np.round(top - np.asarray(lv[:nt], F64))).astype(np.int64), unit)[:n]
        spike = np.zeros(n, F64)
        if rel is not None and nt > SPIKE_UNIT_TILE and rel[SPIKE_UNIT_TILE] == 0:
            # the reference a g = 1 query holds when it reaches that tile is the level of the last rescale before it
            ref = levels_from_rel(list(rel[:SPIKE_UNIT_TILE]) + [9.0])[-1] - 9.0
            j = SPIKE_UNIT_TILE * unit + 50
            assert j not in peaks
            spike[j] = ref + 9.0 - a[j]
        cands = LOW_GAINS if low else LAZY_GAINS
    k = _k_rows(a, spike, hd, rng)
    v = np.broadcast_to(const, (n, hd)).copy() if sum1 else _values(cls, vexp, hd, vrng)
    g, h = _gains(n, cands, hd, rng, bool(spike.any()))
    return k, v, g, h


def _rngs(seed: int, family: str):
    """(the generator of the scores — one per score family, shared by the sum1 case — , the generator of the values)."""
    return np.random.default_rng(seed + FAMILIES.index(family.split("-")[-1])), np.random.default_rng(seed + 500 + FAMILIES.index(family))


def vit_case(family: str, seed: int = 0) -> Case:
    """hd 80, not causal, H = KVH = 2: K rows of the segments follow one another ([H, n, 80]); V^T starts a new 64-key block per
    segment and is zero past the segment's last key (what kr_qkv_prep writes)."""
    hd, H, lens = 80, VIT_HEADS, VIT_LENS
    scores, sum1 = family.split("-")[-1], family.startswith("sum1")
    rng, vrng = _rngs(1000 + seed, family)
    n = sum(lens)
    nb = [(x + 63) // 64 for x in lens]
    r0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    vb0 = np.concatenate([[0], np.cumsum(nb)[:-1]])
    const = _const_values(H, hd, vrng) if sum1 else None
    q, k = np.zeros((H, n, hd), F32), np.zeros((H, n, hd), F32)
    v = np.zeros((H, sum(nb) * 64, hd), F32)
    case = Case("vit", family, hd, H, H, q, k, v, lens=list(lens), const=const, n_rows=n)
    for s, ln in enumerate(lens):
        for h in range(H):
            rel = VIT_REL[(s, h % 2)]
            ks, vs, g, hh = _segment(scores, ln, 64, rel, hd, rng, vrng, False, sum1, None if const is None else const[h],
                                     low=rel[0] == -40 and len(rel) == 1, peak_last=VIT_PEAK_LAST.get((s, h % 2), ()))
            sl = slice(r0[s], r0[s] + ln)
            k[h, sl], q[h, sl] = ks, _q_rows(g, hh, hd)
            v[h, vb0[s] * 64:vb0[s] * 64 + ln] = vs
            case.probs.append(Prob(np.arange(r0[s], r0[s] + ln), h, h, q[h, sl], ks, vs, None, 64, g == 1.0, f"segment {s} head {h}"))
    return case


def prefill_case(family: str, H: int, KVH: int, seed: int = 0) -> Case:
    """hd 128, causal, GQA, cache layout [slots, KVH, s_max, 128]: prompt b lives in slot PREFILL_SLOTS[b]; the unused slot and the
    rows past each prompt hold large finite stale values."""
    hd, lens, slots, s_max = 128, PREFILL_LENS, PREFILL_SLOTS, PREFILL_S_MAX
    scores, sum1 = family.split("-")[-1], family.startswith("sum1")
    rng, vrng = _rngs(2000 + seed + 10 * H, family)
    n, grp = sum(lens), H // KVH
    const = _const_values(KVH, hd, vrng) if sum1 else None
    q = np.zeros((H, n, hd), F32)
    k = bf16_round(rng.standard_normal((PREFILL_N_SLOTS, KVH, s_max, hd)).astype(F32) * F32(STALE_K))
    v = np.where(rng.random((PREFILL_N_SLOTS, KVH, s_max, hd)) < 0.5, -STALE_V, STALE_V).astype(F32)
    case = Case("prefill", family, hd, H, KVH, q, k, v, lens=list(lens), slots=list(slots), s_max=s_max, const=const, n_rows=n)
    off = 0
    for b, ln in enumerate(lens):
        for kvh in range(KVH):
            ks, vs, _, _ = _segment(scores, ln, 64, PREFILL_REL[(b, kvh % 2)], hd, rng, vrng, True, sum1, None if const is None else const[kvh])
            k[slots[b], kvh, :ln], v[slots[b], kvh, :ln] = ks, vs
            for h in range(kvh * grp, (kvh + 1) * grp):
                g, hh = _gains(ln, MASS_GAINS if scores == "mass" else LAZY_GAINS, hd, rng, scores == "lazy" and ln > 64 * SPIKE_UNIT_TILE)
                q[h, off:off + ln] = _q_rows(g, hh, hd)
                case.probs.append(Prob(np.arange(off, off + ln), h, kvh, q[h, off:off + ln], ks, vs, np.arange(ln), 64, g == 1.0,
                                       f"prompt {b} (slot {slots[b]}) head {h}"))
        off += ln
    return case


def decode_batch(n_rows: Optional[int] = None) -> List[Tuple[int, int]]:
    """(ctx_len, finished) per row: the five contexts with one finished row between them; n_rows > 6 repeats the contexts."""
    base = [(c, 0) for c in DECODE_CTX]
    base.insert(2, (DECODE_FINISHED_CTX, 1))
    if n_rows is None:
        return base
    return [base[i % len(base)] for i in range(n_rows)]


def decode_levels() -> List[float]:
    return [x for row in DECODE_LEVELS for x in row]


def decode_case(family: str, H: int, KVH: int, n_rows: Optional[int] = None, seed: int = 0) -> Case:
    """hd 128, one query per row; row b sees keys 0 .. ctx_len[b] of its cache [rows, KVH, s_max, 128]; the K rows and V^T columns
    past them are stale (finite, large)."""
    hd, s_max = 128, DECODE_S_MAX
    scores, sum1 = family.split("-")[-1], family.startswith("sum1")
    batch = decode_batch(n_rows)
    B, grp = len(batch), H // KVH
    rng, vrng = _rngs(3000 + seed + 10 * H + B, family)
    const = _const_values(KVH, hd, vrng) if sum1 else None
    q = np.zeros((B, H, hd), F32)
    k = bf16_round(rng.standard_normal((B, KVH, s_max, hd)).astype(F32) * F32(STALE_K))
    v = np.where(rng.random((B, KVH, s_max, hd)) < 0.5, -STALE_V, STALE_V).astype(F32)
    ctx = np.asarray([c for c, _ in batch], np.int32)
    fin = np.asarray([f for _, f in batch], np.int32)
    case = Case("decode", family, hd, H, KVH, q, k, v, s_max=s_max, ctx=ctx, finished=fin, const=const, n_rows=B)
    for b in range(B):
        nk = int(ctx[b]) + 1
        for kvh in range(KVH):
            ks, vs, _, _ = _segment(scores, nk, 32, None, hd, rng, vrng, False, sum1, None if const is None else const[kvh], levels=decode_levels())
            k[b, kvh, :nk], v[b, kvh, :nk] = ks, vs
            g, hh = _gains(grp, MASS_GAINS if scores == "mass" else LAZY_GAINS, hd, rng, False)
            g[0] = 1.0
            q[b, kvh * grp:(kvh + 1) * grp] = _q_rows(g, hh, hd)
            if fin[b]:
                continue
            for i, h in enumerate(range(kvh * grp, (kvh + 1) * grp)):
                case.probs.append(Prob(np.asarray([b]), h, kvh, q[b, h][None], ks, vs, None, 32, np.asarray([g[i] == 1.0]),
                                       f"row {b} (ctx_len {ctx[b]}) head {h}"))
    return case


# ----------------------------------------------------------------------------- the kernels' arithmetic, restated in float64
MUTANTS = ["l_not_rescaled", "o_not_rescaled", "threshold_vs_previous_max", "unit_dropped", "unit_doubled", "sc_on_o_only",
           "first_reference_clamped", "ones_row_63"]
FLUSH = 2.0 ** -149          # what f32 cannot hold comes out of v_exp_f32 as 0


def _p_of(s: np.ndarray, round_p: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(P as f32 would hold it, P as the PV product takes it)."""
    with np.errstate(over="ignore", under="ignore"):
        p = np.exp2(s)
    p = np.where(p < FLUSH, 0.0, p)
    return p, (bf16_round(p.astype(F32)).astype(F64) if round_p else p)


def model_varlen(case: Case, pr: Prob, mutant: Optional[str] = None, which: int = 0, round_p: bool = False):
    """attn_varlen_kernel's accumulation over 64-key tiles with its lazy reference, in float64: exact up to the named mutant and, with
    round_p, the bf16 rounding of P.  Returns (output [nq, hd], trace): trace[t] = (rise of every query's tile maximum over its
    reference before the tile, whether its wave rescaled)."""
    s_all = scores_log2(case, pr)
    nq, nk = s_all.shape
    hd80 = case.hd == 80
    v = pr.v.astype(F64)
    wave = np.arange(nq) // 32
    m = np.zeros(nq) if hd80 else np.full(nq, -1e30)
    l, o = np.zeros(nq), np.zeros((nq, case.hd))
    prev_mx = np.full(nq, -np.inf)
    trace = []
    for t in range((nk + 63) // 64):
        idx = np.arange(t * 64, min(nk, t * 64 + 64))
        s = s_all[:, idx]
        mx = s.max(1)
        rise = mx - m
        if hd80:
            over = rise > 8.0
            d = np.where(mx > -np.inf, rise, 0.0) if t == 0 else np.maximum(rise, 0.0)
            if mutant == "first_reference_clamped":
                d = np.maximum(rise, 0.0)
            m_new = m + d
        else:
            m_new = np.maximum(m, mx)
            d = m_new - m
            over = d > 8.0
        trig = np.zeros(nq, bool)
        for w in np.unique(wave):
            trig[wave == w] = over[wave == w].any() or (hd80 and t == 0)
        if mutant == "threshold_vs_previous_max":           # the reference follows every tile; o and l only a rise of 8 over the last tile
            with np.errstate(invalid="ignore"):
                over_prev = (mx - prev_mx > 8.0) | (t == 0)
            resc = np.zeros(nq, bool)
            for w in np.unique(wave):
                resc[wave == w] = over_prev[wave == w].any()
            move, trig = np.ones(nq, bool), resc
        else:
            move = trig
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            alpha = np.where(trig, np.exp2(-d), 1.0)
        if hd80 and t == 0:
            alpha = np.ones(nq)
        m = np.where(move, m_new, m)
        if mutant != "l_not_rescaled":
            l = l * alpha
        if mutant != "o_not_rescaled":
            o = o * alpha[:, None]
        trace.append((rise.copy(), trig.copy()))
        prev_mx = mx
        p, pb = _p_of(s - m[:, None], round_p)
        reps = 0 if (mutant == "unit_dropped" and t == which) else 2 if (mutant == "unit_doubled" and t == which) else 1
        pl = pb if hd80 else p                              # hd 80: the ones row sums what the PV product takes
        if mutant == "ones_row_63" and idx.size == 64:
            pl = pl[:, :63]
        l = l + reps * pl.sum(1)
        o = o + reps * (pb @ v[idx])
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(l[:, None] > 0, o / l[:, None], 0.0)
    return out, trace


def decode_waves(n_split: int) -> int:
    """The workgroup shape attn_decode_impl picks."""
    return 8 if n_split <= 8 else 4 if n_split <= 16 else 2


def model_decode(case: Case, pr: Prob, n_split: int, mutant: Optional[str] = None, which: int = 0, round_p: bool = False) -> np.ndarray:
    """attn_decode2_kernel + attn_merge_kernel in float64: eager rescale per 32-key unit, the merge of a workgroup's waves, the merge
    of the n_split records."""
    s_all = scores_log2(case, pr)[0]
    nk = s_all.size
    v = pr.v.astype(F64)
    waves = decode_waves(n_split)
    n_part, nu = waves * n_split, (nk + 31) // 32
    recs = []
    with np.errstate(over="ignore", under="ignore"):
        for split in range(n_split):
            parts = []
            for w in range(waves):
                m, l, o = -1e30, 0.0, np.zeros(case.hd)
                for u in range(split * waves + w, nu, n_part):
                    idx = np.arange(u * 32, min(nk, u * 32 + 32))
                    m_new = max(m, s_all[idx].max())
                    alpha = np.exp2(m - m_new)
                    m = m_new
                    _, pb = _p_of(s_all[idx] - m, round_p)
                    reps = 0 if (mutant == "unit_dropped" and u == which) else 2 if (mutant == "unit_doubled" and u == which) else 1
                    l = l * (1.0 if mutant == "l_not_rescaled" else alpha) + reps * pb.sum()
                    o = o * (1.0 if mutant == "o_not_rescaled" else alpha) + reps * (pb @ v[idx])
                parts.append((m, l, o))
            mm = max(p[0] for p in parts)
            sc = [np.exp2(p[0] - mm) for p in parts]
            recs.append((mm, sum(p[1] * c for p, c in zip(parts, sc)), sum(p[2] * c for p, c in zip(parts, sc))))
        mm = max(r[0] for r in recs)
        sc = [np.exp2(r[0] - mm) for r in recs]
        l = sum(r[1] * (1.0 if mutant == "sc_on_o_only" else c) for r, c in zip(recs, sc))
        o = sum(r[2] * c for r, c in zip(recs, sc))
    return (o / l if l > 0 else np.zeros(case.hd))[None]


def model(case: Case, pr: Prob, n_split: int = 1, **kw) -> np.ndarray:
    return model_decode(case, pr, n_split, **kw) if case.kind == "decode" else model_varlen(case, pr, **kw)[0]


# ----------------------------------------------------------------------------- checks shared by the CPU proof and the GPU run
def contribution_ok(case: Case, pr: Prob) -> np.ndarray:
    """bool [nq]: every tile / unit the query sees carries at least 1 / (2 n) of sum p|v| in every non-negative channel, n the
    number of tiles / units it sees."""
    s = scores_log2(case, pr)
    p = np.exp2(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    v = pr.v.astype(F64)[:, nonneg_channels(case.hd)]
    nk = s.shape[1]
    nt = (nk + pr.unit - 1) // pr.unit
    part = np.stack([p[:, t * pr.unit:(t + 1) * pr.unit] @ v[t * pr.unit:(t + 1) * pr.unit] for t in range(nt)], 1)    # [nq, nt, ch]
    seen = np.stack([np.isfinite(s[:, t * pr.unit:(t + 1) * pr.unit]).any(1) for t in range(nt)], 1)                 # [nq, nt]
    share = part / part.sum(1, keepdims=True)
    need = 1.0 / (2.0 * seen.sum(1))
    return ((share >= need[:, None, None]) | ~seen[:, :, None]).all((1, 2))


def got_block(got: np.ndarray, case: Case, pr: Prob) -> np.ndarray:
    return got[pr.rows, pr.head * case.hd:(pr.head + 1) * case.hd].astype(F64)


def max_ratio(got: np.ndarray, case: Case, first_line_only: bool = False) -> Tuple[float, str]:
    """max |got - o| / E over every output element of the case (an element with E = 0 must be met exactly), and where it is."""
    worst, where = 0.0, ""
    for pr in case.probs:
        o, spv, _ = reference(case, pr)
        e = bound(case, pr, o, spv, first_line_only)
        err = np.abs(got_block(got, case, pr) - o)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / e)
        r = np.where(np.isfinite(r), r, np.inf)
        if r.max() > worst:
            i, d = np.unravel_index(r.argmax(), r.shape)
            worst, where = float(r.max()), f"{pr.name} query {i} channel {d}: got {got_block(got, case, pr)[i, d]:.6g}, reference {o[i, d]:.6g}, E {e[i, d]:.3g}"
    return worst, where


def bf16_neighbours(c: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The bf16 values next to the (bf16) values c, below and above."""
    bits = np.ascontiguousarray(c, F32).view(np.uint32).astype(np.int64)
    step = np.int64(1 << 16)
    away = ((bits + step) & 0xFFFFFFFF).astype(np.uint32).view(F32)          # larger magnitude
    toward = ((bits - step) & 0xFFFFFFFF).astype(np.uint32).view(F32)        # smaller magnitude
    return np.minimum(away, toward), np.maximum(away, toward)


def check_sum1(got: np.ndarray, case: Case, what: str = "") -> Dict[str, int]:
    """Constant V channels: the output is the constant bit for bit where l sums the rounded P (hd 80, decode); at the hd 128
    varlen kernel the constant or a neighbouring bf16 value, and the constant itself for every query whose largest weight is
    <= 1/64.  Returns the counts for the report."""
    n_all = n_exact = n_flat = 0
    for pr in case.probs:
        g = got_block(got, case, pr).astype(F32)
        c = np.broadcast_to(case.const[pr.kvh], g.shape)
        same = g == c
        n_all += same.size
        n_exact += int(same.sum())
        if case.l_rounded:
            assert same.all(), f"{what} {pr.name}: {int((~same).sum())} of {same.size} outputs differ from the constant V channel, the first " \
                               f"at query {np.argwhere(~same)[0][0]} channel {np.argwhere(~same)[0][1]}: {g[~same][0]!r} for {c[~same][0]!r}"
        else:
            lo, hi = bf16_neighbours(c)
            near = same | (g == lo) | (g == hi)
            assert near.all(), f"{what} {pr.name}: {int((~near).sum())} outputs are neither the constant nor a neighbouring bf16 value, " \
                               f"the first: {g[~near][0]!r} for {c[~near][0]!r}"
            flat = reference(case, pr)[2] <= 1.0 / 64
            n_flat += int(flat.sum())
            assert same[flat].all(), f"{what} {pr.name}: a query whose largest weight is <= 1/64 missed the constant: " \
                                     f"{g[flat][~same[flat]][0]!r} for {c[flat][~same[flat]][0]!r}"
    return {"outputs": n_all, "exact": n_exact, "flat_queries": n_flat}


_CASES: Dict[tuple, Case] = {}


def cached(kind: str, *args) -> Case:
    """A case is built once for the tests that launch on it, and left unchanged."""
    key = (kind,) + args
    if key not in _CASES:
        _CASES[key] = {"vit": vit_case, "prefill": prefill_case, "decode": decode_case}[kind](*args)
    return _CASES[key]


# ----------------------------------------------------------------------------- the trajectory a lazy case realizes
def tile_maxima(case: Case, pr: Prob) -> np.ndarray:
    """[nq, n_tiles] the maximum of every query over every 64-key tile (-inf: nothing visible)."""
    s = scores_log2(case, pr)
    return np.stack([s[:, t:t + 64].max(1) for t in range(0, s.shape[1], 64)], 1)


def lazy_events(case: Case) -> Tuple[set, float]:
    """The transitions of attn_varlen_kernel's lazy reference that the g = 1 queries of a case take (names below), and the
    distance of their closest rise from the threshold of 8."""
    ev, closest = set(), np.inf
    for pr in case.probs:
        _, trace = model_varlen(case, pr)
        mx = tile_maxima(case, pr)
        nq, nk = mx.shape[0], pr.k.shape[0]
        wave = np.arange(nq) // 32
        ex0 = pr.exact & np.isfinite(mx[:, 0])
        if (mx[ex0, 0] <= -39).any():
            ev.add("first tile far below zero")
        if (mx[ex0, 0] >= 59).any():
            ev.add("first tile far above zero")
        for t in range(1, len(trace)):
            rise, trig = trace[t]
            prev_rise, prev_trig = trace[t - 1]
            seen = np.isfinite(mx[:, t])
            ex = pr.exact & seen
            if not ex.any():
                continue
            r = rise[ex]
            closest = min(closest, float(np.abs(r - 8.0).min()))
            ragged = nk - t * 64 < 64
            if ((r >= 7.25) & (r <= 7.75) & ~trig[ex]).any():
                ev.add("rise of 7.5, no rescale")
            if ((r >= 8.25) & (r <= 8.75) & trig[ex]).any():
                ev.add("rise of 8.5, rescale")
            if (ex & (rise >= 11.5) & (rise <= 12.5) & trig & (prev_rise >= 5.5) & (prev_rise <= 6.5) & ~prev_trig).any():
                ev.add("second rise of 6 rescales")
            if ((r >= 39) & (r <= 41)).any():
                ev.add("rise of 40")
            if (r >= 150).any():
                ev.add("rise of 160, alpha = 0")
            if ((r <= -29) & (r >= -31)).any():
                ev.add("fall of 30")
            if (r <= -130).any():
                ev.add("fall of 140, p = 0")
            if ragged and (r >= 8.25).any():
                ev.add(f"ragged tile of {nk % 64} keys rises")
            for w in np.unique(wave[ex]):
                lanes = (wave == w) & seen
                up = lanes & (rise >= 8.25)
                if up.sum() == 1 and (rise[lanes & ~up] <= 0.01).all() and lanes.sum() == 32:
                    ev.add("one query of a wave rises, 31 fall or stay")
                if pr.qpos is not None and up.any():
                    peak = int(np.argmax(scores_log2(case, pr)[np.flatnonzero(up)[-1], t * 64:t * 64 + 64])) + t * 64
                    hidden = (wave == w) & (pr.qpos < peak) & (pr.qpos >= t * 64)
                    if hidden.any() and (rise[hidden] <= 7.75).all():
                        ev.add("rising key masked for the earlier queries of its wave")
    return ev, closest


VIT_EVENTS = {"first tile far below zero", "first tile far above zero", "rise of 7.5, no rescale", "rise of 8.5, rescale",
              "second rise of 6 rescales", "rise of 40", "rise of 160, alpha = 0", "fall of 30", "fall of 140, p = 0",
              "one query of a wave rises, 31 fall or stay", "ragged tile of 1 keys rises", "ragged tile of 8 keys rises"}
# the causal kernel: with one kv head only the profiles of the even kv heads exist
PREFILL_EVENTS_1 = {"first tile far below zero", "first tile far above zero", "rise of 7.5, no rescale", "rise of 8.5, rescale",
                    "second rise of 6 rescales", "rise of 160, alpha = 0", "one query of a wave rises, 31 fall or stay",
                    "ragged tile of 1 keys rises", "ragged tile of 33 keys rises", "rising key masked for the earlier queries of its wave"}
PREFILL_EVENTS_2 = PREFILL_EVENTS_1 | {"rise of 40", "fall of 30", "fall of 140, p = 0"}
