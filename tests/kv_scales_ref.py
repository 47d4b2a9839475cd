"""--calculate-kv-scales restated in numpy (not a test module; shared by test_kv_scales_cpu.py, test_gpu_kv_scales_kernels.py and
test_gpu_kv_scales_engine.py).

The rule (include/karanta_hip.h, kr_kv_absmax), per K and V and per kv head: amax = the largest |x| over the FINITE bf16 elements
of K rows [0, len) and of V keys [0, len) of every (slot, len) of the plan — NaN and +-inf are skipped, rows and keys at or beyond
len and slots outside the plan are never looked at — and

    scale = 1.0 if amax == 0 (or nothing finite) else max(f32(amax) / f32(range), FLT_MIN)

with one correctly rounded f32 division, range = the K range or the V range.  A maximum does not depend on the order of its
operands, so the device's result equals this one bit for bit."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

F32 = np.float32
FLT_MIN = np.finfo(F32).tiny
K_RANGE, V_RANGE = 200.0, 100.0               # vLLM's K_SCALE_CONSTANT / V_SCALE_CONSTANT


def amax_finite(x: np.ndarray, axis=None) -> np.ndarray:
    """Largest |x| over the finite elements along `axis` (0 where there is none)."""
    x = np.asarray(x, F32)
    return np.max(np.where(np.isfinite(x), np.abs(x), F32(0)), axis=axis, initial=F32(0)).astype(F32)


def scale_of(amax, rng) -> np.ndarray:
    amax = np.asarray(amax, F32)
    with np.errstate(under="ignore"):
        q = (amax / F32(rng)).astype(F32)
    return np.where(amax == 0, F32(1), np.maximum(q, FLT_MIN)).astype(F32)


def scales_kv(k: np.ndarray, v: np.ndarray, plan: Sequence[Tuple[int, int]], k_range=K_RANGE, v_range=V_RANGE) -> np.ndarray:
    """[2, KVH] f32 from token-major k and v [slots, KVH, s_max, hd] (bf16 values as f32) and the plan [(slot, len), ...]."""
    kvh = k.shape[1]
    am = np.zeros((2, kvh), F32)
    for slot, n in plan:
        am[0] = np.maximum(am[0], amax_finite(k[slot, :, :n], axis=(1, 2)))
        am[1] = np.maximum(am[1], amax_finite(v[slot, :, :n], axis=(1, 2)))
    return np.stack([scale_of(am[0], k_range), scale_of(am[1], v_range)])


def vt_to_tokens(vt: np.ndarray) -> np.ndarray:
    """The stored V^T blocks [..., s_max / 64, 2, hd, 32] -> token-major [..., s_max, hd] (the inverse of kv_fp8_ref.vt_blocks8)."""
    *lead, nb, two, hd, k32 = vt.shape
    assert two == 2 and k32 == 32
    return np.ascontiguousarray(np.swapaxes(vt, -1, -2)).reshape(*lead, nb * 64, hd)


def scales_scratch(k: np.ndarray, vt: np.ndarray, plan, k_range=K_RANGE, v_range=V_RANGE) -> np.ndarray:
    """scales_kv of the scratch as the prefill leaves it: k [slots, KVH, s_max, hd], vt the V^T blocks."""
    return scales_kv(k, vt_to_tokens(vt), plan, k_range, v_range)
