"""Dyadic operands for the linears: inputs whose expected output is ONE bit pattern, whatever the order of the sum (not
a test module; shared by test_exact_cases_cpu.py, which proves the cases and their sensitivity on the float64 reference,
and test_gpu_exact_linears.py, which runs the kernels on them).

Every operand is an integer times a power of two, exactly representable in its storage type (bf16, e4m3 codes with
power-of-two scales, f32 slabs and tables), and the magnitudes are bounded so that every partial sum of an accumulation
is an integer multiple of one common unit 2^-s and stays below 2^24 units.  Every f32 accumulation is then exact in any
order and any split, with FMA or without: the accumulator has exactly one correct value and the output exactly one
correct bit pattern, round-to-nearest-even at the documented points (include/karanta_hip.h):

  linears    out = bf16(acc * scales + bias + residual)            one rounding (f32 outputs: none)
  ROPE_KV    t = bf16(acc * scale + bias); q, k = bf16(lo * cos - hi * sin | hi * cos + lo * sin); v = t
  RMSNorm    h = bf16(w * bf16(x * rsqrt(mean(x^2) + eps)))
  residual   x_new = bf16(x + slab 0 + slab 1)                     one rounding of the f32 sum

Linears: A and W from the non-zero integers -8..8 (no k element is invisible), bias from the integers in [-64, 64],
residual from the integers in [-256, 256]; sum |a||w| <= 64 K < 2^24 up to K = 262144.
RMSNorm rows: magnitudes {0.5, 1, 2, 4} with counts chosen so that mean(x^2) = 4 exactly (a entries at |4|, 4 s at |1|,
16 t at |0.5|, the rest at |2|, a = s + 5 t); bf16(x * rsqrt(4 + 1e-6)) is then x / 2 exactly, also with rsqrt moved by
+-8 ulp, and with norm weights from {0.5, 0.75, 1, 1.25, 1.5, 2} the product is representable: h = w * x / 2.
Residual sums: the target x_new is such a row; x = integers / 64 and the slabs = integers / 1024 are built around it so
that x + p0 + p1 is exact in f32 in every association, off the bf16 grid (ties included) and rounds to the target.
Rotary: cos and sin from {0, +-0.25, +-0.5, +-0.75, +-1} (never both zero): lo * cos - hi * sin is exact in f32.

check_case() asserts representability, the 2^24 bound and the coverage conditions of a case wherever it is built.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from karanta_ocr_amd import weights as WT
from karanta_ocr_amd.weights import bf16_round, from_bf16_bits, to_bf16_bits
from oracle import qwen2vl_oracle as O

F32, F64 = np.float32, np.float64
LIMIT = float(2 ** 24)
EPS = 1e-6

# poison: inputs NaN (anything read beyond an operand poisons the result), outputs a fixed non-NaN pattern
POISON_IN = {"bf16": 0x7FC0, "f32": 0x7FC00000, "u8": 0x7F, "i32": 0x7FC00000}
POISON_OUT = {"bf16": 0x5A5A, "f32": 0x5A5A5A5A, "u8": 0x5A, "i32": 0x5A5A5A5A}
NP_BITS = {"bf16": np.uint16, "f32": np.uint32, "u8": np.uint8, "i32": np.uint32}

# coverage conditions (shares of a case's outputs), asserted by check_case on the reference alone
MIN_ROUNDED_K64, MIN_ROUNDED, MIN_TIES = 0.10, 0.25, 0.05
MIN_DOUBLE_ROUNDING, MIN_PRE_ROTARY = 0.10, 0.50


# ----------------------------------------------------------------------------- roundings of exact values
def exact_f32(v: np.ndarray) -> np.ndarray:
    """float64 values that an exact f32 accumulation holds: they must be f32 values."""
    f = np.asarray(v, F64).astype(F32)
    assert (f.astype(F64) == v).all(), "value is not exact in f32: the case's bound is wrong"
    return f


def rne_bits(v) -> np.ndarray:
    return to_bf16_bits(exact_f32(v))


def trunc_bits(v) -> np.ndarray:
    return (np.ascontiguousarray(exact_f32(v)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def half_away_bits(v) -> np.ndarray:
    return ((np.ascontiguousarray(exact_f32(v)).view(np.uint32) + np.uint32(0x8000)) >> np.uint32(16)).astype(np.uint16)


def rne(v) -> np.ndarray:
    """bf16_round of exact values, as float64."""
    return from_bf16_bits(rne_bits(v)).astype(F64)


def needs_rounding(v) -> np.ndarray:
    return (np.ascontiguousarray(exact_f32(v)).view(np.uint32) & np.uint32(0xFFFF)) != 0


def is_tie(v) -> np.ndarray:
    return (np.ascontiguousarray(exact_f32(v)).view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000)


def is_bf16(x) -> bool:
    x = np.asarray(x, F32)
    return bool((bf16_round(x) == x).all())


def bits16(x) -> np.ndarray:
    """bf16 bit patterns of values that are bf16 values."""
    x = np.asarray(x, F32)
    assert is_bf16(x), "operand is not representable in bf16"
    return to_bf16_bits(x)


def is_multiple(x, unit: float) -> bool:
    q = np.asarray(x, F64) / unit
    return bool((q == np.rint(q)).all())


def nz_ints(rng, *shape, hi: int = 8) -> np.ndarray:
    """Non-zero integers in [-hi, hi]."""
    r = rng.integers(0, 2 * hi, size=shape, dtype=np.int16)            # 0 .. 2 hi - 1 -> -hi .. -1, 1 .. hi
    return (r - hi + (r >= hi)).astype(F32)


def ints(rng, bound: int, *shape) -> np.ndarray:
    return rng.integers(-bound, bound + 1, size=shape).astype(F32)


PREP_SEGMENTS_DEFAULT = (1, 63, 65)


# ----------------------------------------------------------------------------- linear cases
@dataclass
class LinearCase:
    """out[M, N] = bf16((a_scale * A) (w_scale * W)^T + bias + res).  A, W: non-zero integers in [-8, 8] (times one
    power of two in the activation cases; A = the normalised rows h in the norm-prologue cases); w_scale / a_scale:
    powers of two per row (the fp8 forms)."""
    name: str
    M: int
    N: int
    K: int
    A: np.ndarray
    W: np.ndarray
    bias: Optional[np.ndarray] = None
    res: Optional[np.ndarray] = None
    w_scale: Optional[np.ndarray] = None
    a_scale: Optional[np.ndarray] = None
    unit: float = 1.0                      # the common unit of every partial sum and epilogue operand
    rounds: bool = True                    # the output is rounded to bf16 (coverage conditions apply)
    _cache: Dict = field(default_factory=dict, repr=False)

    PROOF_ROWS, FAST_FROM = 256, 2.0e9

    def proof_rows(self) -> np.ndarray:
        """The rows the coverage conditions and the CPU proof look at: all of them, or the first and last 128 of a tall
        case (the entries are i.i.d.: the shares are those of the whole)."""
        if self.M <= self.PROOF_ROWS:
            return np.arange(self.M)
        return np.r_[0:self.PROOF_ROWS // 2, self.M - self.PROOF_ROWS // 2:self.M]

    def scales(self, rows) -> Tuple[np.ndarray, np.ndarray]:
        sa = np.ones(len(rows)) if self.a_scale is None else self.a_scale[rows].astype(F64)
        sw = np.ones(self.N) if self.w_scale is None else self.w_scale.astype(F64)
        return sa, sw

    def acc(self, rows=None) -> np.ndarray:
        """The exact accumulator (with the scales applied), float64, of `rows`."""
        rows = np.arange(self.M) if rows is None else np.asarray(rows)
        sa, sw = self.scales(rows)
        return (self.A[rows].astype(F64) @ self.W.astype(F64).T) * sa[:, None] * sw[None, :]

    def pre(self, acc, rows=None, bias=True, res=True) -> np.ndarray:
        """acc + bias + res: the exact value the epilogue rounds."""
        rows = np.arange(self.M) if rows is None else np.asarray(rows)
        v = acc
        if bias and self.bias is not None:
            v = v + self.bias.astype(F64)[None, :]
        if res and self.res is not None:
            v = v + self.res[rows].astype(F64)
        return v

    def full_pre(self) -> np.ndarray:
        """pre() of every row.  A product that would take float64 more than about a second runs as a float32 BLAS
        product: with the bound below every partial sum of it is exact in any order; one block of rows is compared."""
        if "pre" not in self._cache:
            if float(self.M) * self.N * self.K < self.FAST_FROM:
                acc = self.acc()
            else:
                assert self.K * float(np.abs(self.A).max()) * float(np.abs(self.W).max()) < LIMIT
                sa, sw = self.scales(np.arange(self.M))
                acc = (self.A @ self.W.T).astype(F64) * sa[:, None] * sw[None, :]
                rows = self.proof_rows()
                np.testing.assert_array_equal(acc[rows], self.acc(rows))
            self._cache["pre"] = self.pre(acc)
        return self._cache["pre"]

    def ref_bits(self) -> np.ndarray:
        if "bits" not in self._cache:
            self._cache["bits"] = rne_bits(self.full_pre())
        return self._cache["bits"]

    def ref_f32(self) -> np.ndarray:
        return exact_f32(self.full_pre())


def _bound_units(c: LinearCase) -> float:
    """max over the outputs of sum |a||w| + |bias| + |res|, in units (a tall case: its upper bound K max|a| max|w| max
    scales + max|bias| + max|res|)."""
    if float(c.M) * c.N * c.K < c.FAST_FROM:
        sa, sw = c.scales(np.arange(c.M))
        b = float(((np.abs(c.A).astype(F64) @ np.abs(c.W).astype(F64).T) * sa[:, None] * sw[None, :]).max())
    else:
        sa = 1.0 if c.a_scale is None else float(c.a_scale.max())
        sw = 1.0 if c.w_scale is None else float(c.w_scale.max())
        b = c.K * float(np.abs(c.A).max()) * float(np.abs(c.W).max()) * sa * sw
    b += 0.0 if c.bias is None else float(np.abs(c.bias).max())
    b += 0.0 if c.res is None else float(np.abs(c.res).max())
    return b / c.unit


def dyadic_unit(x) -> float:
    """The largest power of two that divides every entry."""
    u = 2.0 ** 8
    while not is_multiple(x, u):
        u /= 2
        assert u >= 2.0 ** -24
    return u


def _pow2(x) -> bool:
    m, _ = np.frexp(np.asarray(x, F64))
    return bool((m == 0.5).all())


def linear_conditions(c: LinearCase) -> Tuple[float, float]:
    """(share of outputs that need the rounding, share of exact ties) on the proof rows."""
    rows = c.proof_rows()
    v = c.pre(c.acc(rows), rows)
    return float(needs_rounding(v).mean()), float(is_tie(v).mean())


def check_case(c: LinearCase) -> None:
    # representability in the storage type
    assert is_bf16(c.A) and is_bf16(c.W), f"{c.name}: A / W not bf16"
    if c.w_scale is not None:     # fp8 weights: W holds the e4m3 values, the scales are powers of two
        assert (WT.fp8_e4m3_to_f32(WT.f32_to_fp8_e4m3(c.W)) == c.W).all() and _pow2(c.w_scale), f"{c.name}: W not e4m3 x 2^n"
    if c.a_scale is not None:
        assert (WT.fp8_e4m3_to_f32(WT.f32_to_fp8_e4m3(c.A)) == c.A).all() and _pow2(c.a_scale), f"{c.name}: A not e4m3 x 2^n"
    for name, t in (("bias", c.bias), ("res", c.res)):
        assert t is None or (is_bf16(t) and is_multiple(t, c.unit)), f"{c.name}: {name} not a bf16 multiple of the unit"
    # every k element is visible
    assert (c.A != 0).all() and (c.W != 0).all(), f"{c.name}: a zero entry hides its k element"
    # one unit for every partial sum, below 2^24 units
    ua = dyadic_unit(c.A) * (1.0 if c.a_scale is None else float(c.a_scale.min()))
    uw = dyadic_unit(c.W) * (1.0 if c.w_scale is None else float(c.w_scale.min()))
    assert is_multiple(ua * uw, c.unit), f"{c.name}: products are not multiples of the unit"
    assert _bound_units(c) < LIMIT, f"{c.name}: {_bound_units(c)} units >= 2^24"
    if c.rounds:
        rounded, ties = linear_conditions(c)
        need = MIN_ROUNDED_K64 if c.K < 320 else MIN_ROUNDED
        assert rounded >= need, f"{c.name}: only {rounded:.3f} of the outputs need the rounding (< {need})"
        assert ties >= MIN_TIES, f"{c.name}: only {ties:.3f} of the outputs are ties (< {MIN_TIES})"


@functools.lru_cache(maxsize=6)
def linear_case(M: int, N: int, K: int, kind: str = "bf16", bias: bool = True, res: bool = True, rounds: bool = True) -> LinearCase:
    """kind: "bf16" | "fp8" (weights e4m3 with power-of-two row scales 2^-2..2^2) | "fp8a" (both operands codes, a_scale
    2^-2..2^1).  The seed is the case: (M, N, K, kind).  Small cases are redrawn (a fixed number of times, in order)
    until they meet the coverage conditions: a handful of outputs may miss a share by chance."""
    for attempt in range(64):
        rng = np.random.default_rng([M, N, K, {"bf16": 0, "fp8": 1, "fp8a": 2}[kind], attempt])
        A = nz_ints(rng, M, K)
        for edge in (0, 63):       # |a| = 8 on both sides of every 64-boundary: a k element dropped there moves the sum by 8..64
            A[:, edge::64] = np.sign(A[:, edge::64]) * 8
        c = LinearCase(f"{kind}-{M}x{N}x{K}", M, N, K, A, nz_ints(rng, N, K),
                       ints(rng, 64, N) if bias else None, ints(rng, 256, M, N) if res else None, rounds=rounds)
        if kind in ("fp8", "fp8a"):
            c.w_scale = (2.0 ** rng.integers(-2, 3, size=N)).astype(F32)
            c.unit = 0.25
        if kind == "fp8a":
            c.a_scale = (2.0 ** rng.integers(-2, 2, size=M)).astype(F32)
            c.unit = 2.0 ** -4
        if not rounds:
            break
        rounded, ties = linear_conditions(c)
        if rounded >= (MIN_ROUNDED_K64 if K < 320 else MIN_ROUNDED) and ties >= MIN_TIES and \
                (M * N > 4096 or not missed_shares(c, ())):
            break
    check_case(c)
    return c


# ---- mutations of the reference (the CPU proof): the bit patterns a faulty kernel would give on the proof rows
def linear_mutants(c: LinearCase, positions):
    """Yields (mutation, reference bits, mutated bits) on the proof rows; drop / duplicate once per k in `positions`."""
    rows = c.proof_rows()
    acc = c.acc(rows)
    ref = rne_bits(c.pre(acc, rows))
    sa, sw = c.scales(rows)
    for k in positions:
        rank1 = np.outer(c.A[rows, k].astype(F64) * sa, c.W[:, k].astype(F64) * sw)
        yield "drop_k", ref, rne_bits(c.pre(acc - rank1, rows))
        yield "dup_k", ref, rne_bits(c.pre(acc + rank1, rows))
    yield "truncate", ref, trunc_bits(c.pre(acc, rows))
    yield "half_away", ref, half_away_bits(c.pre(acc, rows))
    if c.res is not None:
        yield "round_before_residual", ref, rne_bits(rne(c.pre(acc, rows, res=False)) + c.res[rows].astype(F64))
    if c.bias is not None:
        yield "bias_after_rounding", ref, rne_bits(rne(c.pre(acc, rows, bias=False)) + c.bias.astype(F64)[None, :])
        if c.N > 16:       # the bias of the neighbouring 16-row tile
            yield "shift_bias", ref, rne_bits(c.pre(acc, rows, bias=False) + np.roll(c.bias.astype(F64), 16)[None, :])


def min_share(what: str, K: int) -> float:
    """What a mutation must change: half of what the generator's numbers support (measured on the float64 reference for
    K = 64 / K >= 320: rounding before the residual 7 % / 16-23 %, truncation 9 % / 18-39 %, ties 13-22 % of which half
    round the other way, dropping one k 84-99 %)."""
    small = K < 320
    return {"drop_k": 0.50, "dup_k": 0.50, "truncate": 0.045 if small else 0.09, "half_away": 0.03,
            "round_before_residual": 0.035 if small else 0.08, "bias_after_rounding": 0.02 if small else 0.04,
            "shift_bias": 0.25}[what]


def linear_mutation_shares(c: LinearCase, cuts) -> Dict[str, float]:
    """mutation -> the smallest share of the proof rows' outputs it changes (over the k positions, for drop / duplicate)."""
    out: Dict[str, float] = {}
    for what, ref, mut in linear_mutants(c, drop_positions(c.K, cuts)):
        share = float((ref != mut).mean())
        out[what] = min(out.get(what, 1.0), share)
    return out


def missed_shares(c: LinearCase, cuts) -> Dict[str, float]:
    return {k: v for k, v in linear_mutation_shares(c, cuts).items() if v < min_share(k, c.K)}


def drop_positions(K: int, cuts) -> List[int]:
    """First, last, and both sides of every 64-boundary of the case's K partition."""
    ks = {0, K - 1}
    for cut in cuts:
        if 0 < cut < K:
            ks.update((cut - 1, cut))
    return sorted(ks)


def gemm_cuts(K: int, parts: int = 1) -> Tuple[int, ...]:
    """The GEMMs step K by 64 through a ring of 2 or 4 stages: the boundaries of the first ring turn and of the last two
    steps; a tail cut along K (`parts` ranges: an even share of the steps, the remainder to the first ranges) adds its
    range boundaries."""
    cuts = {64, 128, 192, 256, K - 128, K - 64}
    nk = K // 64
    q, r = nk // parts, nk % parts
    pos = 0
    for i in range(parts - 1):
        pos += q + (1 if i < r else 0)
        cuts.add(pos * 64)
    return tuple(sorted(c for c in cuts if 0 < c < K))


def k_partition(K: int, parts: int) -> Tuple[int, ...]:
    """The 64-boundaries where the K / 64 chunks are cut into `parts` ranges of ceil(chunks / parts) chunks: the wave
    ranges of the decode launches."""
    chunks = K // 64
    per = -(-chunks // parts)
    return tuple(min(i * per, chunks) * 64 for i in range(1, parts))


# ----------------------------------------------------------------------------- activation epilogues
ACT_ABS = 2.0 ** -20      # covers GELU's cancellation below -2: 0.5 |x| (erff error) < 2^-20 for |x| <= 8


def _erf(x):
    try:
        from scipy.special import erf
        return erf(x)
    except Exception:  # pragma: no cover
        return np.vectorize(math.erf, otypes=[F64])(x)


def act_ref(name: str, pre: np.ndarray, dtype=F64) -> np.ndarray:
    """The activation epilogues on exact pre-activations; dtype float32 restates the formula as the kernels evaluate it
    (the CPU module checks that this meets the bracket rule)."""
    x = pre.astype(dtype)
    one = dtype(1)
    if name == "quick_gelu":
        return x / (one + np.exp(-dtype(1.702) * x))
    if name == "gelu_erf":
        return dtype(0.5) * x * (one + _erf(x * dtype(math.sqrt(0.5))).astype(dtype))
    if name in ("silu_mul", "silu_mul8"):
        grp = 16 if name == "silu_mul" else 8
        m, n = x.shape
        g = x.reshape(m, n // (2 * grp), 2, grp)
        gate, up = g[:, :, 0].reshape(m, -1), g[:, :, 1].reshape(m, -1)
        return gate / (one + np.exp(-gate)) * up
    raise ValueError(name)


def bracket_ok(got_bits: np.ndarray, ref64: np.ndarray) -> np.ndarray:
    """Every output is one of the two bf16 values that bracket the float64 reference, or within ACT_ABS of it."""
    r32 = np.ascontiguousarray(ref64.astype(F32))
    mag = ((r32.view(np.uint32) >> np.uint32(16)) & np.uint32(0x7FFF)).astype(np.int64)
    a = np.abs(ref64)
    # the bracket is among the bf16 magnitudes next to the truncated f32 value (the f32 rounding moves far less than a step)
    vals = [from_bf16_bits(np.clip(mag + d, 0, 0x7F7F).astype(np.uint16)).astype(F64) for d in (-1, 0, 1)]
    down = np.max([np.where(v <= a, v, -np.inf) for v in vals], axis=0)
    up = np.min([np.where(v >= a, v, np.inf) for v in vals], axis=0)
    g = from_bf16_bits(got_bits).astype(F64)
    same_sign = (np.signbit(g) == np.signbit(ref64)) | (g == 0)
    return (same_sign & ((np.abs(g) == down) | (np.abs(g) == up))) | (np.abs(g - ref64) <= ACT_ABS)


@functools.lru_cache(maxsize=4)
def act_case(M: int, N: int, K: int, bias: bool = True) -> LinearCase:
    """Operands scaled by 2^-4 each: the exact pre-activations spread over about +-4 (std sqrt(650 K) / 256 = 3.5 at
    K = 1216); bias = integers / 16 in [-1, 1]."""
    rng = np.random.default_rng([M, N, K, 77])
    c = LinearCase(f"act-{M}x{N}x{K}", M, N, K, nz_ints(rng, M, K) / F32(16), nz_ints(rng, N, K) / F32(16),
                   ints(rng, 16, N) / F32(16) if bias else None, None, unit=2.0 ** -8, rounds=False)
    check_case(c)
    pre = c.full_pre()
    assert 2.5 < pre.std() < 5 and np.abs(pre).max() < 32, f"{c.name}: pre-activations spread {pre.std()}"
    return c


# ----------------------------------------------------------------------------- RMSNorm / LayerNorm rows
NORM_W = np.asarray([0.5, 0.75, 1.0, 1.25, 1.5, 2.0], F32)


def norm_rows(rng, rows: int, K: int, pairs: bool = False) -> np.ndarray:
    """Rows with mean(x^2) = 4 exactly.  pairs: every value has its negative in the row (mean 0: LayerNorm rows)."""
    n = K // 2 if pairs else K
    out = np.empty((rows, K), F32)
    for r in range(rows):
        t = int(rng.integers(1, max(2, n // 64)))
        s = int(rng.integers(1, max(2, n // 16)))
        a = s + 5 * t
        assert a + 4 * s + 16 * t <= n
        mag = np.full(n, 2.0, F32)
        mag[:a] = 4.0
        mag[a:a + 4 * s] = 1.0
        mag[a + 4 * s:a + 4 * s + 16 * t] = 0.5
        if pairs:
            row = np.concatenate([mag, -mag])
        else:
            row = mag * (rng.integers(0, 2, size=n) * 2 - 1)
        out[r] = rng.permutation(row)
    assert ((out.astype(F64) ** 2).mean(1) == 4.0).all()
    return out


def norm_weights(rng, K: int) -> np.ndarray:
    return NORM_W[rng.integers(0, len(NORM_W), size=K)]


def rms_ref(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Qwen2VLRMSNorm under the oracle's bf16 policy; on norm_rows it is w * x / 2 exactly (asserted)."""
    h = O.rms_norm(x, w, EPS, O._Policy("bf16"))
    assert (h.astype(F64) == w.astype(F64) * x.astype(F64) / 2).all() and is_bf16(h)
    return h


def rms_ref_perturbed(x: np.ndarray, w: np.ndarray, ulps: int) -> np.ndarray:
    """The kernels' arithmetic in float32 with rsqrt moved by `ulps`: bf16(w * bf16(x * rs))."""
    ss = (x.astype(F32) ** 2).sum(1, dtype=F32)
    rs = (F32(1) / np.sqrt(ss / F32(x.shape[1]) + F32(EPS), dtype=F32)).astype(F32)
    rs = (np.ascontiguousarray(rs).view(np.int32) + np.int32(ulps)).view(F32)
    return bf16_round(w * bf16_round(x * rs[:, None]))


def ln_case(rows: int, d: int):
    """LayerNorm rows (mean 0, variance 4), dyadic weights, biases = odd integers / 32 (|b| <= 2):
    y = (x / 2) * w + b is an odd multiple of 1/32 below 8: a bf16 value, and never the exact cancellation 0 (where an
    rsqrt off by one ulp would leave a residue instead of a rounding error)."""
    rng = np.random.default_rng([rows, d, 5])
    x, w = norm_rows(rng, rows, d, pairs=True), norm_weights(rng, d)
    b = (2 * ints(rng, 31, d) + 1) / F32(32)
    y = x.astype(F64) / 2 * w.astype(F64) + b.astype(F64)
    assert (x.astype(F64).mean(1) == 0).all() and is_bf16(y) and is_bf16(b)
    assert (bf16_round(O.layer_norm(x, w, b, EPS)) == y).all(), "the oracle's LayerNorm is not exact on these rows"
    return x, w, b, y.astype(F32)


def ln_ref_perturbed(x, w, b, ulps: int) -> np.ndarray:
    """kr_layernorm's arithmetic in float32 with rsqrt moved by `ulps`: bf16((x - mean) * rstd * w + b)."""
    x = x.astype(F32)
    mean = x.sum(1, dtype=F32) / F32(x.shape[1])
    t = x - mean[:, None]
    rstd = (F32(1) / np.sqrt((t * t).sum(1, dtype=F32) / F32(x.shape[1]) + F32(EPS), dtype=F32)).astype(F32)
    rstd = (np.ascontiguousarray(rstd).view(np.int32) + np.int32(ulps)).view(F32)
    return bf16_round(t * rstd[:, None] * w + b)


# ----------------------------------------------------------------------------- residual sums around a target row
def residual_sum(rng, target: np.ndarray, n_part: int):
    """x (integers / 64, bf16) and n_part f32 slabs (integers / 1024, |p| <= 2) with bf16(x + p0 [+ p1]) = target, the
    exact sum sitting off the bf16 grid by d / 1024, |d| up to HALF the spacing on that side (ties to the even target
    included).  The targets are powers of two: spacing 2^-7 |v| above and 2^-8 |v| below in magnitude."""
    rows, K = target.shape
    mag = np.abs(target).astype(F64)
    up, down = np.rint(mag * 2 ** -8 * 1024).astype(np.int64), np.rint(mag * 2 ** -9 * 1024).astype(np.int64)   # half spacings
    d = rng.integers(-down, up + 1) * np.sign(target).astype(np.int64)      # away from zero: up to `up`, towards: `down`
    if n_part == 0:
        return target.copy(), np.zeros((0, rows, K), F32), target.astype(F64)
    m = rng.integers(-64, 65, size=(rows, K))
    x = target.astype(F64) + m / 64.0
    odd = (np.abs(x) >= 4) & (m % 2 != 0)                                    # [4, 8): bf16 holds multiples of 1/32
    x = np.where(odd, x - 1 / 64.0, x)
    rest = target.astype(F64) + d / 1024.0 - x                               # what the slabs add: a multiple of 1/1024
    if n_part == 1:
        p = rest[None]
    else:
        p0 = rng.integers(-512, 513, size=(rows, K)) / 1024.0
        p = np.stack([p0, rest - p0])
    assert np.abs(p).max() <= 2 and is_multiple(p, 2.0 ** -10) and is_multiple(x, 2.0 ** -6) and np.abs(x).max() <= 8
    total = x + p.sum(0)
    assert (rne(total) == target).all()
    return x.astype(F32), p.astype(F32), total


def min_share_round_between_slabs() -> float:
    return MIN_DOUBLE_ROUNDING


def double_rounding_share(x: np.ndarray, p: np.ndarray) -> float:
    """Share of elements where bf16(bf16(x + p0) + p1) differs from the single rounding."""
    once = rne_bits(x.astype(F64) + p.astype(F64).sum(0))
    twice = rne_bits(rne(x.astype(F64) + p[0]) + p[1])
    return float((once != twice).mean())


@dataclass
class NormLinearCase:
    """x (+ slabs) -> x_new = target rows -> h = RMSNorm(x_new) -> a LinearCase on h (A = h)."""
    x: np.ndarray
    parts: np.ndarray
    x_new: np.ndarray
    norm_w: np.ndarray
    h: np.ndarray
    lin: LinearCase


def _norm_linear(rng, name, M, N, K, n_part, bias=True, res=True, w_scale=False, rounds=True) -> NormLinearCase:
    x_new, nw = norm_rows(rng, M, K), norm_weights(rng, K)
    x, parts, total = residual_sum(rng, x_new, n_part)
    if n_part:
        assert needs_rounding(total).mean() >= 0.75
    if n_part == 2:
        share = double_rounding_share(x, parts)
        assert share >= MIN_DOUBLE_ROUNDING, f"{name}: double rounding differs in only {share:.3f}"
    h = rms_ref(x_new, nw)
    b = None
    if bias:
        b = ints(rng, 64, N)
    lin = LinearCase(name, M, N, K, h, nz_ints(rng, N, K), b, ints(rng, 256, M, N) if res else None, unit=2.0 ** -4, rounds=rounds)
    if w_scale:
        lin.w_scale = (2.0 ** rng.integers(-2, 3, size=N)).astype(F32)
        lin.unit = 2.0 ** -6
    check_case(lin)
    return NormLinearCase(x, parts, x_new, nw, h, lin)


@functools.lru_cache(maxsize=8)
def norm_linear_case(M: int, N: int, K: int, n_part: int, fp8: bool = False, rounds: bool = True, res: bool = True,
                     bias: bool = True) -> NormLinearCase:
    for attempt in range(64):       # a few hundred outputs may miss a share by chance: redraw (a fixed sequence of seeds)
        rng = np.random.default_rng([M, N, K, n_part, int(fp8), 11, attempt])
        try:
            c = _norm_linear(rng, f"norm-{M}x{N}x{K}-p{n_part}{'-fp8' if fp8 else ''}", M, N, K, n_part, w_scale=fp8,
                             rounds=rounds, res=res, bias=bias)
        except AssertionError:
            if M * N > 4096:
                raise
            continue
        if not rounds or M * N > 4096 or not missed_shares(c.lin, ()):
            return c
    raise AssertionError(f"norm_linear_case({M}, {N}, {K}, {n_part}): no draw meets the conditions")


@functools.lru_cache(maxsize=4)
def silu8_norm_case(M: int, ff: int, K: int, fp8: bool = False) -> NormLinearCase:
    """Fused RMSNorm + gate/up projection (rows interleaved in groups of 8): W = non-zero integers * 2^-s with s chosen so
    that the exact pre-activations spread over about +-4; no bias, no residual; the output goes through SiLU * up."""
    rng = np.random.default_rng([M, ff, K, int(fp8), 19])
    x, nw = norm_rows(rng, M, K), norm_weights(rng, K)
    h = rms_ref(x, nw)
    s = int(round(math.log2(math.sqrt(K * 1.6 * 25.5) / 3.5)))
    W = nz_ints(rng, 2 * ff, K)
    lin = LinearCase(f"silu8-{M}x{ff}x{K}", M, 2 * ff, K, h, W if fp8 else W * F32(2.0 ** -s), unit=2.0 ** -(4 + s + (1 if fp8 else 0)),
                     rounds=False)
    if fp8:
        lin.w_scale = (2.0 ** (-s + rng.integers(-1, 2, size=2 * ff))).astype(F32)
    check_case(lin)
    pre = lin.full_pre()
    assert 1.5 < pre.std() < 8, pre.std()
    return NormLinearCase(x, np.zeros((0, M, K), F32), x, nw, h, lin)


# ----------------------------------------------------------------------------- rotary
CS_VALUES = np.asarray([-1, -0.75, -0.5, -0.25, 0, 0.25, 0.5, 0.75, 1], F32)


def cs_pairs(rng, *shape) -> Tuple[np.ndarray, np.ndarray]:
    """cos, sin from CS_VALUES, never both zero (a zero pair would mask its output element)."""
    c, s = CS_VALUES[rng.integers(0, 9, size=shape)], CS_VALUES[rng.integers(0, 9, size=shape)]
    both = (c == 0) & (s == 0)
    c = np.where(both, F32(0.75), c)
    return c.astype(F32), s.astype(F32)


def rotate(t: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    """t [..., hd] float64 exact, cos / sin [..., hd] (per channel): t * cos + rotate_half(t) * sin, exact in f32."""
    return t.astype(F64) * cos.astype(F64) + O.rotate_half(t.astype(F64)) * sin.astype(F64)


@dataclass
class RopeCase:
    """A ROPE_KV launch: B rows, N = (H + 2 KVH) * 128."""
    B: int
    H: int
    KVH: int
    K: int
    s_max: int
    T: int
    nl: NormLinearCase                # nl.lin: the projection (bias, no residual); nl.x / parts / norm_w: the fused prologue
    plen: np.ndarray
    step: np.ndarray
    cs: np.ndarray                    # [B, T, 128] f32: cos[0..64), sin[0..64)
    t: np.ndarray = None              # [B, N] float64: bf16(acc * scale + bias)
    q: np.ndarray = None              # bits [B, H, 128]
    k: np.ndarray = None              # bits [B, KVH, 128]
    v: np.ndarray = None              # bits [B, KVH, 128]

    @property
    def ctx(self):
        return (self.plen + self.step).astype(np.int32)


ROPE_POS = [(0, 0), (63, 0), (60, 3), (64, 0), (61, 3), (3, 2)]      # (prompt_len, step): cache positions 0, 63, 64 and the steps around them


@functools.lru_cache(maxsize=6)
def rope_case(B: int, H: int, KVH: int, K: int, n_part: int = 0, fp8: bool = False, s_max: int = 128, T: int = 4) -> RopeCase:
    rng = np.random.default_rng([B, H, KVH, K, n_part, int(fp8), 13])
    N = (H + 2 * KVH) * 128
    nl = _norm_linear(rng, f"rope-{B}x{H}x{KVH}x{K}-p{n_part}{'-fp8' if fp8 else ''}", B, N, K, n_part, res=False, w_scale=fp8,
                      rounds=False)
    pos = (ROPE_POS * (B // len(ROPE_POS) + 1))[:B]
    plen, step = np.asarray([p for p, _ in pos], np.int32), np.asarray([s for _, s in pos], np.int32)
    extra = B - len(ROPE_POS)
    if extra > 0:
        plen[len(ROPE_POS):] = rng.integers(0, s_max - T, size=extra)
        step[len(ROPE_POS):] = rng.integers(0, T, size=extra)
    cos, sin = cs_pairs(rng, B, T, 64)
    c = RopeCase(B, H, KVH, K, s_max, T, nl, plen, step, np.concatenate([cos, sin], -1).astype(F32))
    pre = nl.lin.full_pre()
    share = float(needs_rounding(pre).mean())
    assert share >= MIN_PRE_ROTARY, f"{nl.lin.name}: only {share:.3f} of t need the pre-rotary rounding"
    c.t = rne(pre)
    c.q, c.k, c.v = rope_outputs(c, c.t)
    return c


def rope_outputs(c: RopeCase, t: np.ndarray, rounder=rne_bits, slots=None):
    """q, k bits after the rotary at each row's step, v bits, from the projection output t [B, N].  slots: the cs_table
    row of each batch row (kr_linear_decode32_rows), default its own."""
    B, H, KVH = c.B, c.H, c.KVH
    t3 = t.reshape(B, H + 2 * KVH, 128)
    csb = c.cs[np.arange(B) if slots is None else np.asarray(slots), c.step]
    cos = np.concatenate([csb[:, :64], csb[:, :64]], -1)[:, None]
    sin = np.concatenate([csb[:, 64:], csb[:, 64:]], -1)[:, None]
    rot = rotate(t3[:, :H + KVH], cos, sin)
    assert (rot != 0).mean() > 0.99
    bits = rounder(rot)
    return bits[:, :H], bits[:, H:], rounder(t3[:, H + KVH:])


# ----------------------------------------------------------------------------- kr_qkv_prep
@dataclass
class PrepCase:
    lens: Tuple[int, ...]
    H: int
    KVH: int
    hd: int
    qkv: np.ndarray          # [n, (H + 2 KVH) hd]: non-zero integers / 16, |x| < 16 (8 significant bits)
    cos: np.ndarray          # [n, hd] per channel (both halves drawn independently)
    sin: np.ndarray
    q: np.ndarray = None     # bits [H, n, hd]
    k: np.ndarray = None     # bits [n, KVH, hd]
    v: np.ndarray = None     # bits [n, KVH, hd]


@functools.lru_cache(maxsize=4)
def prep_case(hd: int, H: int, KVH: int, lens: Tuple[int, ...] = tuple(PREP_SEGMENTS_DEFAULT)) -> PrepCase:
    rng = np.random.default_rng([hd, H, KVH, 17])
    n = sum(lens)
    qd, kd = H * hd, KVH * hd
    qkv = nz_ints(rng, n, qd + 2 * kd, hi=255) / F32(16)
    cos, sin = cs_pairs(rng, n, hd)
    c = PrepCase(tuple(lens), H, KVH, hd, qkv, cos, sin)
    assert is_bf16(qkv)
    q = rotate(qkv[:, :qd].reshape(n, H, hd), cos[:, None], sin[:, None])
    k = rotate(qkv[:, qd:qd + kd].reshape(n, KVH, hd), cos[:, None], sin[:, None])
    for t in (q, k):
        assert needs_rounding(t).mean() >= MIN_ROUNDED and is_tie(t).mean() >= MIN_TIES, (needs_rounding(t).mean(), is_tie(t).mean())
        assert (t != 0).mean() > 0.99
    c.q, c.k = rne_bits(q).transpose(1, 0, 2).copy(), rne_bits(k)
    c.v = bits16(qkv[:, qd + kd:]).reshape(n, KVH, hd)
    return c


# ----------------------------------------------------------------------------- guarded device buffers
class Guarded:
    """A device tensor [rows, cols] embedded in a larger poisoned allocation: a guard band before the pointer, padding
    columns (row stride ld > cols), guard rows after the last row and a guard band after the end.  Input poison is NaN,
    output poison a fixed non-NaN pattern; every check runs on raw bits.  role "in": nothing may change at all;
    role "out": everything but the logical [rows, cols] region must keep its poison."""
    BAND = 256

    def __init__(self, torch, device, kind: str, rows: int, cols: int, ld: Optional[int] = None, role: str = "in",
                 guard_rows: int = 16, offset: int = 0, init: Optional[np.ndarray] = None):
        self.torch, self.kind, self.rows, self.cols, self.role = torch, kind, rows, cols, role
        self.ld = cols if ld is None else ld
        assert self.ld >= cols
        self.front = self.BAND + offset
        np_t = NP_BITS[kind]
        self.poison = np_t((POISON_IN if role == "in" else POISON_OUT)[kind])
        n = self.front + (rows + guard_rows) * self.ld + self.BAND
        hostbuf = np.full(n, self.poison, np_t)
        body = hostbuf[self.front:self.front + rows * self.ld].reshape(rows, self.ld)
        self.mask = np.zeros(n, bool)
        self.mask[self.front:self.front + rows * self.ld].reshape(rows, self.ld)[:, :cols] = True
        if init is not None:                 # bit patterns (or f32 / int32 values of the same width)
            a = np.ascontiguousarray(init)
            assert a.dtype.itemsize == np_t().itemsize and a.size == rows * cols, (a.dtype, a.shape, kind, rows, cols)
            body[:, :cols] = a.view(np_t).reshape(rows, cols)
        self.before = hostbuf
        signed = {np.uint16: np.int16, np.uint32: np.int32, np.uint8: np.uint8}[np_t]
        self.dev = torch.from_numpy(hostbuf.view(signed).copy()).to(device)
        self.itemsize = hostbuf.itemsize

    @property
    def ptr(self) -> int:
        return self.dev.data_ptr() + self.front * self.itemsize

    def host(self) -> np.ndarray:
        if self.dev.is_cuda:
            self.torch.cuda.synchronize()
        return self.dev.cpu().numpy().view(self.before.dtype)

    def read(self) -> np.ndarray:
        """The logical region, as bits."""
        return self.host()[self.front:self.front + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols].copy()

    def assert_untouched(self, what: str = "") -> None:
        now = self.host()
        if self.role == "in":
            bad = now != self.before
        else:
            bad = (now != self.poison) & ~self.mask
        if bad.any():
            i = int(np.flatnonzero(bad)[0]) - self.front
            raise AssertionError(f"{what or self.kind}: {int(bad.sum())} guard / input elements changed, the first at row "
                                 f"{i // self.ld}, column {i % self.ld} of [{self.rows}, {self.cols}] (ld {self.ld})")


# ----------------------------------------------------------------------------- the parametrisations (CPU proof = GPU run)
# prefill / ViT GEMMs: id -> (M, N, K, environment, what the shape reaches)
GEMM_SHAPES = {
    "ring4-1x16x64": (1, 16, 64, {"KARANTA_GEMM_TILE": "128"}),
    "ring4-129x144x1216": (129, 144, 1216, {"KARANTA_GEMM_TILE": "128"}),
    "two-stage-2049x2064x320": (2049, 2064, 320, {"KARANTA_GEMM_TILE": "128"}),          # 17 x 17 = 289 workgroups > 256 CUs
    "tile256-257x272x1216": (257, 272, 1216, {"KARANTA_GEMM_TILE": "256"}),
    "tile512-513x1280x1216": (513, 1280, 1216, {"KARANTA_GEMM_TILE": "512"}),
    "tile512-group3-1793x768x320": (1793, 768, 320, {"KARANTA_GEMM_TILE": "512", "KARANTA_GEMM_GROUP_M": "3"}),
}
# the tail shapes: 43 x 6 = 258 tiles of 256 x 256, the last m tile has one row; K = 4160: 65 K steps over the split
GEMM_TAIL_SHAPES = {"tail-quarters": (10753, 1536, 320), "tail-k-cut": (10753, 1536, 4160)}
GEMM_TAIL_VARIANTS = {"tail": {}, "tail-off": {"KARANTA_GEMM_TAIL": "0"}, "tail-unsplit": {"KARANTA_GEMM_TAIL_KSPLIT": "1"}}
GEMM_FALLBACK = (300, 272, 320)            # ldc = N + 4, C offset by 4 elements, under KARANTA_GEMM_TILE=512
GEMM_FP8_SHAPES = [(257, 272, 1216), (2049, 768, 1280)]
ACT_SHAPE = (300, 528, 1216)


def act_shape(epi: str) -> Tuple[int, int, int]:
    """SILU_MUL interleaves gate / up in groups of 16 rows: N % 32 == 0, so 544 = 2 x 256 + 32 there (528 elsewhere)."""
    return (300, 544, 1216) if epi == "silu_mul" else ACT_SHAPE


@functools.lru_cache(maxsize=4)
def argmax_case(M: int, N: int, K: int) -> LinearCase:
    """lm_head logits (no bias, no residual, f32): the upper half of W repeats the lower one, so every logit, the
    maximum included, occurs twice, in different tiles: the lowest index must win."""
    c = linear_case(M, N, K, "bf16", False, False, False)
    W = c.W.copy()
    W[N // 2:] = W[:N - N // 2]
    d = LinearCase(f"argmax-{M}x{N}x{K}", M, N, K, c.A, W, rounds=False)
    check_case(d)
    logits = d.ref_f32()
    assert all((row == row.max()).sum() >= 2 for row in logits)
    return d

ACT_EPILOGUES = ["quick_gelu", "gelu_erf", "silu_mul", "silu_mul8", "silu_mul8_bias"]

NARROW_M = [1, 5, 16]
NARROW_SHAPES = [(1536, 1536, 8), (96, 8960, 16), (96, 8960, 8), (3072, 1216, 8)]      # (N, K, waves); the last: two tiles per workgroup
NARROW_NORM = [(M, K, n) for M in (3, 16) for K in (1536, 2048, 3584) for n in (0, 1, 2)]
ROPE_SHAPES = [(2, 1, 256), (12, 2, 1536), (28, 4, 3584)]                             # (H, KVH, K)
WIDE_SHAPES = [(16 * 37, 512, 3, 5), (16 * 37, 1536, 256, 4), (16 * 41, 3584, 5, 2)]  # (N, K, blocks, waves) of the wide tests
DEC32_M = [17, 21, 32]
DEC32_SHAPES = [(1536, 1536, 8, 1), (96, 8960, 16, 2), (96, 8960, 16, 1), (224, 3584, 8, 1), (80, 64 * 19, 16, 1)]   # (N, K, waves_ref, ksplit)
PREP_SEGMENTS = list(PREP_SEGMENTS_DEFAULT)
PREP_HEADS = [(80, 5, 5), (128, 6, 3)]       # (hd, q heads, kv heads): 10 / 9 head slots = two groups of kr_qkv_prep's 8
NORM_N = 16 * 24
NORM_D = [256, 1536, 2048, 3584]
LN_D = [320, 1280, 1536, 3584]


def linear_case_list() -> List[Tuple[str, tuple, Tuple[int, ...]]]:
    """(id, linear_case arguments, the 64-boundaries of the launch's K partition) of every accumulation case with a
    rounded output that the GPU module runs; the CPU module proves each."""
    out = [(k, (M, N, K), gemm_cuts(K)) for k, (M, N, K, _) in GEMM_SHAPES.items()]
    out += [(k, (M, N, K), gemm_cuts(K, 8)) for k, (M, N, K) in GEMM_TAIL_SHAPES.items()]      # 8 ranges: min(16, 65 / 8, 256 / 8)
    out += [("fallback", GEMM_FALLBACK, gemm_cuts(GEMM_FALLBACK[2]))]
    out += [(f"{kind}-{M}x{N}x{K}", (M, N, K, kind), gemm_cuts(K)) for kind in ("fp8", "fp8a") for (M, N, K) in GEMM_FP8_SHAPES]
    out += [(f"narrow-{M}x{N}x{K}-w{w}", (M, N, K), k_partition(K, w)) for M in NARROW_M for (N, K, w) in NARROW_SHAPES]
    out += [(f"narrow-fp8-{M}x{N}x{K}-w{w}", (M, N, K, "fp8"), k_partition(K, w)) for M in NARROW_M for (N, K, w) in NARROW_SHAPES[:2]]
    out += [(f"wide-{M}x{N}x{K}", (M, N, K), gemm_cuts(K)) for M in (1, 16) + tuple(DEC32_M) for (N, K, _, _) in WIDE_SHAPES]
    out += [(f"dec32-{M}x{N}x{K}-w{w}", (M, N, K), k_partition(K, w)) for M in DEC32_M for (N, K, w, ks) in DEC32_SHAPES]
    seen, uniq = set(), []
    for e in out:
        if e[0] not in seen:
            seen.add(e[0])
            uniq.append(e)
    return uniq
