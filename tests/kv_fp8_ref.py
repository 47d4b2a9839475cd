"""The fp8 (e4m3fn) KV cache restated in numpy (not a test module; shared by test_kv_fp8_cpu.py, which proves the rule and the
attention bound on the reference alone, and the GPU tests test_gpu_kv_fp8_kernels.py / test_gpu_kv_fp8_engine.py).

The rule (include/karanta_hip.h, kr_kv8; kv8_clamp / kv8_pack4 in csrc/kr_decode_common.h), wherever a value enters the cache:
the bf16-rounded value the bf16 cache would have held, divided by the scale in f32 (one correctly rounded division), clamped to
+-448 explicitly, rounded to the nearest e4m3 code, ties to the even mantissa (`weights.f32_to_fp8_e4m3`).  Code 0 is 0.0, -0 keeps
its sign, no NaN code is written.  A code stands for code * scale."""
from __future__ import annotations

from typing import Tuple

import numpy as np

from karanta_ocr_amd.weights import E4M3_MAX, bf16_round, f32_to_fp8_e4m3, fp8_e4m3_to_f32

F32, F64 = np.float32, np.float64
STALE_CODE = 0x7E                 # 448: what the tests write where a correct kernel must not look
SENTINEL = 0x55                   # the byte the tests prefill destinations with
# bf16 inputs at the edges of the format (under scale 1): the largest value and beyond it, the smallest subnormal 2^-9 and half
# of it (a tie with zero: even), signed zeros, ties between neighbouring codes — 17 (16 | 18), 19 (18 | 20), 1.5 and 2.5 x 2^-9
# (subnormal codes 1 | 2 | 3) — and 464, the tie between 448 and the 480 that e4m3fn does not have: it clamps before it rounds
EDGES = np.asarray([448.0, -448.0, 450.0, 9984.0, -9984.0, 2.0 ** -9, 2.0 ** -10, -(2.0 ** -10), 0.0, -0.0,
                    17.0, 19.0, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 464.0, 480.0], F32)


def codes_of_quotient(y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The second half of the rule: (codes, clamped) of the f32 quotients y = x / scale — the explicit clamp, then the conversion."""
    y = np.asarray(y, F32)
    c = np.clip(y, F32(-E4M3_MAX), F32(E4M3_MAX))
    codes = f32_to_fp8_e4m3(c)
    assert not ((codes & 0x7F) == 0x7F).any()
    return codes, c != y


def quantize(x: np.ndarray, scale) -> Tuple[np.ndarray, np.ndarray]:
    """(codes uint8, clamped bool) of the bf16 values x under `scale` (a float or an array broadcast against x)."""
    x = np.asarray(x, F32)
    assert np.array_equal(x, bf16_round(x), equal_nan=True), "the cache takes bf16 values"
    return codes_of_quotient((x / np.asarray(scale, F32)).astype(F32))          # IEEE f32 division, as the device's


def dequantize(codes: np.ndarray, scale) -> np.ndarray:
    """float64 code * scale: the operand the attention multiplies with (the product of two f32 values, exact in float64)."""
    return fp8_e4m3_to_f32(codes).astype(F64) * np.asarray(scale, F32).astype(F64)


def vt_blocks8(v_codes: np.ndarray) -> np.ndarray:
    """[..., s_max, 128] codes -> the V^T blocks [..., s_max / 64, 2, 128, 32] (kr_vt_off: two contiguous 32-key halves)."""
    *lead, s, hd = v_codes.shape
    assert s % 64 == 0
    b = v_codes.reshape(*lead, s // 64, 2, 32, hd)
    return np.ascontiguousarray(np.swapaxes(b, -1, -2))


def vt_bf16_halves(vt64: np.ndarray) -> np.ndarray:
    """POS.vt_blocks' logical [..., hd, 64] view of a V^T block -> the stored [..., 2, hd, 32] halves."""
    *lead, hd, k = vt64.shape
    assert k == 64
    return np.ascontiguousarray(np.swapaxes(vt64.reshape(*lead, hd, 2, 32), -2, -3))


def scale_table(k, v, layers: int, kv_heads: int) -> np.ndarray:
    """[L, 2, KVH] f32 from [L] or [L, KVH] arrays (Engine.set_kv_scales's contract)."""
    out = np.empty((layers, 2, kv_heads), F32)
    for j, a in enumerate((k, v)):
        a = np.asarray(a, F32)
        if a.shape == (layers,):
            a = np.repeat(a[:, None], kv_heads, 1)
        if a.shape != (layers, kv_heads) or not (np.isfinite(a).all() and (a > 0).all()):
            raise ValueError(f"kv scales must be positive, finite and [L] or [L, KVH] = [{layers}] / [{layers}, {kv_heads}], not {a.shape}")
        out[:, j] = a
    return out


# ----------------------------------------------------------------------------- the fp8 kernel's arithmetic in float64
def model_decode_kv8(q: np.ndarray, k_codes: np.ndarray, v_codes: np.ndarray, k_scale, v_scale, n_split: int, waves: int,
                     hd: int = 128) -> np.ndarray:
    """attn_decode2_kernel<KV8> + attn_merge_kernel for the queries q [nq, hd] of one head over ctx keys: scores from the CODES'
    values, scale_log2e * k_scale folded in f32, P rounded to bf16, l from the rounded P, O += P~ V(code values), the wave's O times
    v_scale, the waves and the records merged.  Everything else in float64."""
    ctx = k_codes.shape[0]
    kv, vv = fp8_e4m3_to_f32(k_codes).astype(F64), fp8_e4m3_to_f32(v_codes).astype(F64)
    sl2 = F64(F32(F32(F32(hd ** -0.5) * F32(1.4426950408889634)) * F32(k_scale)))
    s = (q.astype(F64) @ kv.T) * sl2
    nu = (ctx + 31) // 32
    n_part = n_split * waves
    recs = []
    for part in range(n_part):
        m, l, o = np.full(q.shape[0], -1e30), np.zeros(q.shape[0]), np.zeros((q.shape[0], hd))
        for u in range(part, nu, n_part):
            sl = slice(u * 32, min(u * 32 + 32, ctx))
            m_new = np.maximum(m, s[:, sl].max(1))
            alpha = np.exp2(m - m_new)
            p = bf16_round(np.exp2(s[:, sl] - m_new[:, None]).astype(F32)).astype(F64)
            l = l * alpha + p.sum(1)
            o = o * alpha[:, None] + p @ vv[sl]
            m = m_new
        recs.append((m, l, o * F64(F32(v_scale))))
    mm = np.max([r[0] for r in recs], 0)
    acc, ll = np.zeros((q.shape[0], hd)), np.zeros(q.shape[0])
    for m, l, o in recs:
        sc = np.exp2(m - mm)
        acc += o * sc[:, None]
        ll += l * sc
    return bf16_round((acc / ll[:, None]).astype(F32)).astype(F64)


# ----------------------------------------------------------------------------- decode attention cases (CPU proof = GPU run)
DECODE_HEADS = [(12, 2), (28, 4)]
DECODE_CTX = [1, 31, 32, 33, 64, 65, 1100]     # keys per live row: unit and block borders; 1100 at 4 splits x 8 waves: two units per wave
DECODE_FINISHED_AT, DECODE_FINISHED_CTX = 3, 40          # one finished row between the live ones
DECODE_S_MAX = 1152
DECODE_SPLITS = [1, 4, 16, 32]
# (k_scale, v_scale): a float for all kv heads, or a tuple of per-head values of which the first KVH are used (the last entry: every
# head reads an entry of its own, in the K row and in the V row of the [2][KVH] table)
DECODE_SCALES = [(1.0, 1.0), (0.5, 2.0), (0.37, 1.9), ((0.5, 1.3, 0.37, 2.0), (1.9, 0.6, 2.5, 1.0))]


def scale_rows(k_scale, v_scale, KVH: int) -> np.ndarray:
    """[2][KVH] f32, the table the kernels take, from a float or a per-kv-head sequence each (the first KVH values of a longer one)."""
    out = np.empty((2, KVH), F32)
    for j, s in enumerate((k_scale, v_scale)):
        s = np.asarray(s, F32)
        assert s.ndim == 0 or (s.ndim == 1 and s.size >= KVH), "a scale is a float or a vector with an entry per kv head"
        out[j] = s if s.ndim == 0 else s[:KVH]
    return out


def decode_rows():
    """[(keys, finished)] of the batch."""
    rows = [(c, 0) for c in DECODE_CTX]
    rows.insert(DECODE_FINISHED_AT, (DECODE_FINISHED_CTX, 1))
    return rows


def decode_case(H: int, KVH: int, k_scale, v_scale, seed: int = 0):
    """(attn_arith.Case over the DEQUANTISED operands, k_codes [B, KVH, s_max, 128], v_codes likewise): K and V drawn, quantised by
    the rule, and the code values times the scale are what the reference and the bound see.  Rows at or beyond a row's keys hold
    STALE_CODE (448).  k_scale / v_scale: a float, or per-kv-head values (scale_rows)."""
    from tests import attn_arith as AA
    sc = scale_rows(k_scale, v_scale, KVH)
    rng = np.random.default_rng(1000 * H + 10 * KVH + seed)
    rows = decode_rows()
    B, hd, G = len(rows), 128, H // KVH
    q = bf16_round(rng.standard_normal((B, H, hd)).astype(F32))
    k_codes = np.full((B, KVH, DECODE_S_MAX, hd), STALE_CODE, np.uint8)
    v_codes = np.full((B, KVH, DECODE_S_MAX, hd), STALE_CODE, np.uint8)
    case = AA.Case("decode", "kv8", hd, H, KVH, q.reshape(B, H * hd), None, None, s_max=DECODE_S_MAX,
                   ctx=np.asarray([c - 1 for c, _ in rows], np.int32), finished=np.asarray([f for _, f in rows], np.int32), n_rows=B)
    for b, (n, fin) in enumerate(rows):
        for h in range(KVH):
            kr = bf16_round((rng.standard_normal((n, hd)) * (1.0 + 0.5 * h)).astype(F32))
            vr = bf16_round((rng.standard_normal((n, hd)) * 1.5 + 0.25).astype(F32))
            k_codes[b, h, :n], _ = quantize(kr, sc[0, h])
            v_codes[b, h, :n], _ = quantize(vr, sc[1, h])
        if fin:
            continue
        for hq in range(H):
            h = hq // G
            case.probs.append(AA.Prob(np.asarray([b]), hq, h, q[b, hq][None], dequantize(k_codes[b, h, :n], sc[0, h]),
                                      dequantize(v_codes[b, h, :n], sc[1, h]), None, 32, np.asarray([True]), f"row {b} ({n} keys) head {hq}"))
    return case, k_codes, v_codes


NEEDLE_V = 3.5


def needle_case(H: int, KVH: int):
    """An independent check of the operand mapping, no reference arithmetic: q is channel-distinct, ONE key per row carries q's own
    pattern (its score stands ~80 log2 units above every other key's, whose K rows are the same pattern rotated over the channels),
    and V is constant over the channels of a key: NEEDLE_V on the needle, another value on every other key.  The output must be
    NEEDLE_V bit for bit; a K / Q channel permutation that does not match, or P against the wrong keys of V^T, moves it.  All
    values are exact e4m3 codes under scale 1."""
    rows = decode_rows()
    B, hd = len(rows), 128
    pat = (np.random.default_rng(5).permutation(hd) - 63.5) / 16.0            # 128 distinct values in (-4, 4), in no order
    pat_codes, _ = quantize(bf16_round(pat.astype(F32)), 1.0)
    patq = fp8_e4m3_to_f32(pat_codes)                                           # the pattern as e4m3 holds it (exact in bf16)
    q = np.broadcast_to(patq, (B, H, hd)).astype(F32)
    k_codes = np.full((B, KVH, DECODE_S_MAX, hd), STALE_CODE, np.uint8)
    v_codes = np.full((B, KVH, DECODE_S_MAX, hd), STALE_CODE, np.uint8)
    needles = []
    for b, (n, _) in enumerate(rows):
        j0 = (7 * b + 3) * 29 % n
        needles.append(j0)
        for j in range(n):
            k_codes[b, :, j] = pat_codes if j == j0 else np.roll(pat_codes, 1 + j % 127)
            val = NEEDLE_V if j == j0 else (j % 13) * 0.25 - 1.5
            v_codes[b, :, j] = quantize(np.full(hd, val, F32), 1.0)[0]
    s = patq.astype(F64) @ np.stack([np.roll(patq, r) for r in range(128)]).astype(F64).T * (hd ** -0.5) * 1.4426950408889634
    assert s[0] - s[1:].max() > 40, "the needle does not stand out"
    ctx = np.asarray([n - 1 for n, _ in rows], np.int32)
    fin = np.asarray([f for _, f in rows], np.int32)
    return q.reshape(B, H * hd), k_codes, v_codes, ctx, fin, needles
