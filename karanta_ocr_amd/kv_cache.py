"""The KV cache of the engine: its storage, its scales and every launch that depends on how it is stored.  `KVCache` is the
bfloat16 cache, `KVCacheFp8` the e4m3 one with an f32 scale per (layer, K or V, kv head) (--kv-cache-dtype fp8); `make` picks
by the engine's `kv8`.  The engine's launch sequence asks the component four things and never which cache it has:
  prefill   the (K, V^T) tensors layer i's attention writes (`prefill_target`), what runs behind that attention
            (`prefill_layer_done`) and behind the last layer (`prefill_done`)
  decode    the cache keywords of layer i's qkv launch (`qkv`: kc / vc addresses, or the kr_kv8 descriptor) and the launch of
            its attention partials (`attention`)
  fork      the copy of a prompt's rows to its sibling slots (`fork`)
  scales    set / read / calibrate-once / checkpoint (`set_scales`, `scales`, `load_scales`, ...): Engine.set_kv_scales and its kin
            delegate here
Launches go through `self.L.<name>` at the moment of the call, to the engine's current stream."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import KarantaHipError, fork_plan, kv8, kvq_plan, ptr
from .weights import kv_scale_table, kv_scales_from_checkpoint

KV_SCALES_FLAG_WINS = ("fp8 KV cache scales: the checkpoint ships k_scale / v_scale, but --calculate-kv-scales wins: the first "
                       "admission calculates them")


def make(eng):
    return (KVCacheFp8 if eng.kv8 else KVCache)(eng)


class KVCache:
    """[layers, max_batch, kv heads, s_max, head_dim] K rows and [.., s_max / 64, head_dim, 64] V^T blocks, bfloat16."""
    dtype = torch.bfloat16
    fork_entry, attn_slots_entry, attn_rows_entry = "kr_kv_fork", "kr_attn_decode_slots", "kr_attn_decode_rows"
    calibrated = scales_ready = False
    clamped = 0

    def __init__(self, eng):
        self.eng, self.L = eng, eng.L
        t, z = eng.cfg.text, self._zeros
        # zero-initialised: masked keys must be finite (fp8: code 0 is 0.0, the zero-initialised cache is still finite padding)
        self.kcache = z(t.num_layers, eng.B, t.num_kv_heads, eng.s_max, t.head_dim, dtype=self.dtype)
        self.vtcache = z(t.num_layers, eng.B, t.num_kv_heads, eng.s_max // 64, t.head_dim, 64, dtype=self.dtype)

    def _zeros(self, *shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype, device=self.eng.device)

    def nbytes(self) -> int:
        return self.kcache.numel() * self.kcache.element_size() + self.vtcache.numel() * self.vtcache.element_size()

    # ------------------------------------------------------------------ scales: the bfloat16 cache has none
    def set_scales(self, k, v, source: str = "set_kv_scales"):
        raise KarantaHipError("set_kv_scales: the KV cache is bfloat16 (kv_cache_dtype=\"fp8\" quantises it)")

    def scales(self) -> np.ndarray:
        raise KarantaHipError("kv_scales: the KV cache is bfloat16 (kv_cache_dtype=\"fp8\" quantises it)")

    def load_scales(self, weights, log=None):
        pass

    # ------------------------------------------------------------------ prefill
    def prefill_target(self, i: int):
        """(K, V^T) [max_batch, kv heads, ...] that layer i's prefill attention writes: the plan's rows count from slot 0."""
        return self.kcache[i], self.vtcache[i]

    def prefill_layer_done(self, i: int, adm):
        pass

    def prefill_done(self, adm):
        pass

    # ------------------------------------------------------------------ decode
    def layer(self, i: int) -> tuple:
        """Layer i as the decode entry points take it."""
        return ptr(self.kcache[i]), ptr(self.vtcache[i])

    def qkv(self, i: int) -> dict:
        """The cache keywords of layer i's qkv launch (Engine._dec_narrow / _dec32)."""
        return {"kc": ptr(self.kcache[i]), "vc": ptr(self.vtcache[i])}

    def attention(self, i: int, rows: int, row_slot=None):
        """Split-KV attention partials of layer i over `rows` rows of d_q into d_ws; row_slot (a speculative step): row r reads
        the cache of slot row_slot[r]."""
        e, t = self.eng, self.eng.cfg.text
        front = (ptr(e.d_q), *self.layer(i), ptr(e.d_ctx), ptr(e.d_fin))
        back = (ptr(e.d_ws), rows, t.num_heads, t.num_kv_heads, t.head_dim, e.s_max, e.n_split, t.head_dim ** -0.5, e.s)
        if row_slot is not None:
            getattr(self.L, self.attn_rows_entry)(*front, ptr(row_slot), *back)
        else:
            getattr(self.L, self.attn_slots_entry)(*front, *back)

    def fork(self, groups):
        """The prompt's KV rows of every (source slot, prompt length, [destination slots]), in one launch."""
        e, t, kc, vc = self.eng, self.eng.cfg.text, self.kcache, self.vtcache
        getattr(self.L, self.fork_entry)(ptr(kc), ptr(vc), kc.stride(0), kc.stride(1), kc.stride(2), vc.stride(0), vc.stride(1),
                                         vc.stride(2), t.num_layers, t.num_kv_heads, t.head_dim, e.B, e.s_max, fork_plan(groups), e.s)


class KVCacheFp8(KVCache):
    """The same layout in e4m3 codes; a code stands for code x scale.  The prefill and its attention stay on bf16: they write and
    read ONE layer of bf16 scratch (the strides of a layer of the bf16 cache, so the prefill plan is unchanged), which
    kr_kv_quantize converts into layer i after layer i's attention.  calculate_kv_scales: the FIRST prefill writes the scale
    table from the absolute maxima of its own K / V (kr_kv_absmax): scale = amax / range; `_calibrate` is armed until then
    (set_scales disarms it)."""
    dtype = torch.uint8
    fork_entry, attn_slots_entry, attn_rows_entry = "kr_kv_fork8", "kr_attn_decode_slots_kv8", "kr_attn_decode_rows_kv8"

    def __init__(self, eng):
        super().__init__(eng)
        t, z = eng.cfg.text, self._zeros
        self.p_kscratch = z(eng.B, t.num_kv_heads, eng.s_max, t.head_dim)
        self.p_vtscratch = z(eng.B, t.num_kv_heads, eng.s_max // 64, t.head_dim, 64)
        self.d_kv_scale = torch.ones(t.num_layers, 2, t.num_kv_heads, dtype=torch.float32, device=eng.device)   # static: graphs read it
        # the table's host mirror (scales()): written by set_scales, refreshed behind the calibrating admission
        self.h_kv_scale = torch.ones(t.num_layers, 2, t.num_kv_heads, dtype=torch.float32).pin_memory()
        self.d_kv_clamped = z(1, dtype=torch.int32)
        self.h_kv_clamped = torch.zeros(1, dtype=torch.int32).pin_memory()    # its host mirror, refreshed behind every admission
        self.scale_source = "default (1.0)"
        self._calibrate = eng.calculate_kv_scales
        self.calibrated = False            # True once the calibrating admission has been launched
        if self._calibrate:    # kr_kv_absmax's [2][KVH] words: zero on entry, zero again behind every call
            self.d_kv_work = z(2 * t.num_kv_heads, dtype=torch.int32)

    # ------------------------------------------------------------------ scales
    def set_scales(self, k, v, source: str = "set_kv_scales"):
        t = self.eng.cfg.text
        table = torch.from_numpy(kv_scale_table(k, v, t.num_layers, t.num_kv_heads))
        self.d_kv_scale.copy_(table.to(self.eng.device))
        self.h_kv_scale.copy_(table)
        self.scale_source = source
        self._calibrate = False        # calculate_kv_scales: a table set by hand before the first admission stands

    def scales(self) -> np.ndarray:
        return self.h_kv_scale.numpy().copy()

    @property
    def scales_ready(self) -> bool:
        return self.calibrated and self._scale_event.query()

    @property
    def clamped(self) -> int:
        return int(self.h_kv_clamped[0])

    def load_scales(self, weights, log=None):
        """A checkpoint with a kv_cache_scheme ships one k_scale / v_scale per layer: broadcast over the kv heads, unless the
        first admission is to calculate them."""
        sc = kv_scales_from_checkpoint(weights, self.eng.cfg)
        if sc is not None and self._calibrate:
            if log is not None:
                log(KV_SCALES_FLAG_WINS)
        elif sc is not None:
            self.set_scales(*sc, source="checkpoint (self_attn.k_scale / v_scale)")
        if log is not None:
            log(f"fp8 KV cache scales: {self.scale_source}")

    # ------------------------------------------------------------------ prefill
    def prefill_target(self, i: int):
        return self.p_kscratch, self.p_vtscratch

    def prefill_layer_done(self, i: int, adm):
        """The admission's rows of the scratch -> layer i of the cache, on the admission's stream; a calibrating admission writes
        layer i's row of the scale table right before kr_kv_quantize reads it."""
        e, t = self.eng, self.eng.cfg.text
        front = (ptr(self.p_kscratch), ptr(self.p_vtscratch))
        shape = (t.num_kv_heads, t.head_dim, e.B, e.s_max, kvq_plan(adm.kvq))
        if self._calibrate:
            self.L.kr_kv_absmax(*front, *shape, e.kv_scale_ranges[0], e.kv_scale_ranges[1], ptr(self.d_kv_scale[i]),
                                ptr(self.d_kv_work), e.s)
        self.L.kr_kv_quantize(*front, *self.layer(i), *shape, ptr(self.d_kv_clamped), e.s)

    def prefill_done(self, adm):
        """Behind the last layer: the mirrors; the admission that calibrated was the only one that does."""
        e = self.eng
        self.h_kv_clamped.copy_(self.d_kv_clamped, non_blocking=True)
        if self._calibrate:
            self.h_kv_scale.copy_(self.d_kv_scale, non_blocking=True)
            self.scale_source = (f"calculated from the first admission ({adm.M} prompt tokens; ranges "
                                 f"{e.kv_scale_ranges[0]:g} / {e.kv_scale_ranges[1]:g})")
            self._scale_event = torch.cuda.Event()
            self._scale_event.record(e.stream)
            self.calibrated, self._calibrate = True, False

    # ------------------------------------------------------------------ decode
    def layer(self, i: int) -> tuple:
        return (kv8(ptr(self.kcache[i]), ptr(self.vtcache[i]), ptr(self.d_kv_scale[i])),)

    def qkv(self, i: int) -> dict:
        """The kr_kv8 descriptor beside the two addresses: the packed launch's kr_dec32 carries those as well."""
        return {**super().qkv(i), "kv8": self.layer(i)[0]}
