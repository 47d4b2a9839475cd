"""The model's parameters on the device: one packed arena, laid out for the kernels."""
from __future__ import annotations

from typing import Dict, FrozenSet, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import KarantaHipError
from .config import ModelConfig
from .weights import pack_w16x64, to_bf16_bits

BF16 = torch.bfloat16


def _bits(w: np.ndarray) -> np.ndarray:
    return w if w.dtype == np.uint16 else to_bf16_bits(np.asarray(w, dtype=np.float32))


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def narrow_weight_bytes(cfg: ModelConfig, weight_dtype: str = "bf16") -> List[Dict[str, int]]:
    """Per decoder layer, the bytes a <= 16-row decode step streams for each narrow launch: {"qkv", "o", "down"} -> bytes.
    bf16: the packed matrix; fp8: its e4m3 codes + one f32 scale per output row (what kr_linear_decode_narrow_fp8 reads)."""
    t = cfg.text
    shapes = {"qkv": (t.qkv_dim, t.hidden_size), "o": (t.hidden_size, t.q_dim), "down": (t.hidden_size, t.intermediate_size)}
    per = (lambda n, k: n * k + 4 * n) if weight_dtype == "fp8" else (lambda n, k: 2 * n * k)
    return [{kind: per(*shape) for kind, shape in shapes.items()} for _ in range(t.num_layers)]


def plan_resident(layer_bytes: Sequence[Dict[str, int]], gains: Sequence[Tuple[str, float]], budget_bytes: int,
                  min_us: float = 0.0) -> FrozenSet[Tuple[int, str]]:
    """Which (layer, launch kind) weights a decode step loads with the default cache policy, so that they stay in the
    Infinity Cache from step to step (kr_narrow_opts.w_resident), under a byte budget.
    layer_bytes: per layer {kind: bytes} (narrow_weight_bytes); gains: (kind, measured us saved per MB resident), kinds with no
    gain left out or <= 0.  Greedy by gain per byte: kinds in falling gain (ties: by name), layers in rising order; a weight that
    no longer fits is passed over, smaller ones behind it may still fit.  Never more than budget_bytes in all.
    min_us: a launch whose expected saving (gain x its MB) is below this is not planned: the per-MB figures were measured on
    matrices of several MB read from HBM and say nothing about one that is a fraction of that."""
    order = sorted(((g, kind) for kind, g in gains if g > 0), key=lambda e: (-e[0], e[1]))
    left, chosen = int(budget_bytes), set()
    for g, kind in order:
        for layer, sizes in enumerate(layer_bytes):
            n = sizes.get(kind, 0)
            if 0 < n <= left and g * n / 1e6 >= min_us and (layer, kind) not in chosen:
                chosen.add((layer, kind))
                left -= n
    return frozenset(chosen)


class DeviceWeights:
    """All parameters in one contiguous HBM arena, laid out for the kernels:

    * ViT Linears keep their [out, in] row-major layout (K contiguous = MFMA fragment order);
    * decoder q/k/v are fused into one [q+2kv, d] matrix, gate/up into one [2*ff, d] matrix with
      rows interleaved in groups of 8 (KR_EPI_SILU_MUL8: one 16-row MFMA tile = 8 gate rows + their 8 up rows);
    * every decoder Linear and the lm_head are stored PACKED as [N/16][K/64][16][64] tiles
      (weights.pack_w16x64): decode streams them linearly from HBM, prefill reads the same copy
      through kr_gemm_bf16(w_packed=1).  A tied lm_head gets its own packed copy (the embedding
      table itself stays row-major for the gather);
    * the patch-embed kernel matrix is zero-padded from K=1176 to 1216 (GEMM BK=64).
    """

    def __init__(self, cfg: ModelConfig, device: torch.device, weight_dtype: str = "bf16"):
        if weight_dtype not in ("bf16", "fp8"):
            raise ValueError(f"weight_dtype {weight_dtype!r} (bf16 or fp8)")
        self.cfg = cfg
        self.device = device
        # fp8 (BASELINE.json config 5): the decoder Linears are ALSO kept as e4m3fn codes + one f32 scale per output
        # row for the decode kernels (half the bytes per step); the bf16 entries then hold the dequantised values
        # (what the prefill GEMMs read).  lm_head, embeddings, norms, biases and the ViT stay bf16.
        self.weight_dtype = weight_dtype
        self.layout: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.nbytes = 0
        self.arena: Optional[torch.Tensor] = None
        self._plan()

    def _add(self, name: str, shape: Tuple[int, ...], itemsize: int = 2):
        self.layout[name] = (self.nbytes, tuple(shape))
        self.nbytes = _align(self.nbytes + itemsize * int(np.prod(shape)))

    def _plan(self):
        v, t = self.cfg.vision, self.cfg.text
        self._add("vit.patch", (v.embed_dim, v.patch_dim_padded))
        v25 = v.variant == "qwen2_5"
        for i in range(v.depth):
            p = f"vit.{i}."
            self._add(p + "ln1.w", (v.embed_dim,))
            self._add(p + "qkv.w", (3 * v.embed_dim, v.embed_dim)); self._add(p + "qkv.b", (3 * v.embed_dim,))
            self._add(p + "proj.w", (v.embed_dim, v.embed_dim)); self._add(p + "proj.b", (v.embed_dim,))
            self._add(p + "ln2.w", (v.embed_dim,))
            if v25:
                # biased SwiGLU (TF25:85-97): gate / up fused with rows AND biases interleaved in groups of 8
                # (KR_EPI_SILU_MUL8), width zero-padded to a multiple of 64 (3420 -> 3456)
                fp = v.mlp_dim_padded
                self._add(p + "gate_up.w", (2 * fp, v.embed_dim)); self._add(p + "gate_up.b", (2 * fp,))
                self._add(p + "down.w", (v.embed_dim, fp)); self._add(p + "down.b", (v.embed_dim,))
            else:
                self._add(p + "ln1.b", (v.embed_dim,)); self._add(p + "ln2.b", (v.embed_dim,))
                self._add(p + "fc1.w", (v.mlp_dim, v.embed_dim)); self._add(p + "fc1.b", (v.mlp_dim,))
                self._add(p + "fc2.w", (v.embed_dim, v.mlp_dim)); self._add(p + "fc2.b", (v.embed_dim,))
        self._add("vit.merger.ln.w", (v.embed_dim,))
        if not v25:
            self._add("vit.merger.ln.b", (v.embed_dim,))
        self._add("vit.merger.fc1.w", (v.merge_dim, v.merge_dim)); self._add("vit.merger.fc1.b", (v.merge_dim,))
        self._add("vit.merger.fc2.w", (v.hidden_size, v.merge_dim)); self._add("vit.merger.fc2.b", (v.hidden_size,))
        self._add("llm.embed", (t.vocab_size, t.hidden_size))
        for i in range(t.num_layers):
            p = f"llm.{i}."
            self._add(p + "ln1.w", (t.hidden_size,))
            self._add(p + "qkv.w", (t.qkv_dim, t.hidden_size)); self._add(p + "qkv.b", (t.qkv_dim,))
            self._add(p + "o.w", (t.hidden_size, t.q_dim))
            self._add(p + "ln2.w", (t.hidden_size,))
            self._add(p + "gate_up.w", (2 * t.intermediate_size, t.hidden_size))
            self._add(p + "down.w", (t.hidden_size, t.intermediate_size))
            if self.weight_dtype == "fp8":
                for n, shape in (("qkv", (t.qkv_dim, t.hidden_size)), ("o", (t.hidden_size, t.q_dim)),
                                 ("gate_up", (2 * t.intermediate_size, t.hidden_size)), ("down", (t.hidden_size, t.intermediate_size))):
                    self._add(p + n + ".w8", shape, itemsize=1)
                    self._add(p + n + ".s", (shape[0],), itemsize=4)
        self._add("llm.norm.w", (t.hidden_size,))
        self._add("llm.lm_head", (t.vocab_size, t.hidden_size))

    def allocate(self):
        self.arena = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)

    def view(self, name: str) -> torch.Tensor:
        off, shape = self.layout[name]
        n = int(np.prod(shape))
        return self.arena[off:off + 2 * n].view(BF16).view(*shape)

    def view_u8(self, name: str) -> torch.Tensor:
        off, shape = self.layout[name]
        return self.arena[off:off + int(np.prod(shape))].view(*shape)

    def view_f32(self, name: str) -> torch.Tensor:
        off, shape = self.layout[name]
        return self.arena[off:off + 4 * int(np.prod(shape))].view(torch.float32).view(*shape)

    def has(self, name: str) -> bool:
        return name in self.layout

    def _put(self, name: str, bits: np.ndarray):
        off, shape = self.layout[name]
        assert tuple(bits.shape) == shape, (name, bits.shape, shape)
        src = torch.from_numpy(np.ascontiguousarray(bits).view(np.uint8).reshape(-1))
        self.arena[off:off + src.numel()].copy_(src, non_blocking=False)

    def load(self, w: Dict[str, np.ndarray]):
        """Fill the arena from a HF-named state dict (fp32 arrays or bf16 bit patterns)."""
        if self.arena is None:
            self.allocate()
        v, t = self.cfg.vision, self.cfg.text
        V, Lm = "model.visual.", "model.language_model."
        pe = _bits(w[V + "patch_embed.proj.weight"]).reshape(v.embed_dim, -1)
        pad = np.zeros((v.embed_dim, v.patch_dim_padded), np.uint16)
        pad[:, :pe.shape[1]] = pe
        self._put("vit.patch", pad)
        v25 = v.variant == "qwen2_5"
        for i in range(v.depth):
            s, d = f"{V}blocks.{i}.", f"vit.{i}."
            names = [("norm1.weight", "ln1.w"), ("attn.qkv.weight", "qkv.w"), ("attn.qkv.bias", "qkv.b"),
                     ("attn.proj.weight", "proj.w"), ("attn.proj.bias", "proj.b"), ("norm2.weight", "ln2.w")]
            if not v25:
                names += [("norm1.bias", "ln1.b"), ("norm2.bias", "ln2.b"), ("mlp.fc1.weight", "fc1.w"),
                          ("mlp.fc1.bias", "fc1.b"), ("mlp.fc2.weight", "fc2.w"), ("mlp.fc2.bias", "fc2.b")]
            for a, b in names:
                self._put(d + b, _bits(w[s + a]))
            if v25:
                ffv, fp, D = v.mlp_dim, v.mlp_dim_padded, v.embed_dim
                def padded(a, rows):            # zero rows up to the padded width
                    out = np.zeros((rows,) + a.shape[1:], np.uint16)
                    out[:a.shape[0]] = a
                    return out
                g = padded(_bits(w[s + "mlp.gate_proj.weight"]), fp).reshape(fp // 8, 8, D)
                u = padded(_bits(w[s + "mlp.up_proj.weight"]), fp).reshape(fp // 8, 8, D)
                self._put(d + "gate_up.w", np.stack([g, u], 1).reshape(2 * fp, D))
                gb = padded(_bits(w[s + "mlp.gate_proj.bias"]), fp).reshape(fp // 8, 8)
                ub = padded(_bits(w[s + "mlp.up_proj.bias"]), fp).reshape(fp // 8, 8)
                self._put(d + "gate_up.b", np.stack([gb, ub], 1).reshape(2 * fp))
                dw = np.zeros((D, fp), np.uint16)
                dw[:, :ffv] = _bits(w[s + "mlp.down_proj.weight"])
                self._put(d + "down.w", dw)
                self._put(d + "down.b", _bits(w[s + "mlp.down_proj.bias"]))
        merger = [("merger.ln_q.weight", "ln.w"), ("merger.mlp.0.weight", "fc1.w"), ("merger.mlp.0.bias", "fc1.b"),
                  ("merger.mlp.2.weight", "fc2.w"), ("merger.mlp.2.bias", "fc2.b")]
        if not v25:
            merger.append(("merger.ln_q.bias", "ln.b"))
        for a, b in merger:
            self._put("vit.merger." + b, _bits(w[V + a]))
        self._put("llm.embed", _bits(w[Lm + "embed_tokens.weight"]))
        ff = t.intermediate_size
        if ff % 8:
            raise KarantaHipError(f"intermediate_size {ff} must be a multiple of 8")
        fp8 = self.weight_dtype == "fp8"
        for i in range(t.num_layers):
            s, d = f"{Lm}layers.{i}.", f"llm.{i}."
            self._put(d + "ln1.w", _bits(w[s + "input_layernorm.weight"]))
            self._put(d + "ln2.w", _bits(w[s + "post_attention_layernorm.weight"]))
            self._put(d + "qkv.b", np.concatenate([_bits(w[s + f"self_attn.{n}_proj.bias"]) for n in "qkv"], 0))
            if fp8:
                # quantise every original matrix row-wise (scale = max|row| / 448), then fuse / interleave codes,
                # scales and the dequantised bf16 copy alike
                from .weights import as_f32, fp8_e4m3_to_f32, pack_w16x64_fp8, quantize_fp8_rows
                qs = {n: quantize_fp8_rows(as_f32(w[s + n + ".weight"])) for n in
                      ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
                       "mlp.up_proj", "mlp.down_proj")}
                il = lambda a, b: np.stack([a.reshape((ff // 8, 8) + a.shape[1:]), b.reshape((ff // 8, 8) + b.shape[1:])], 1) \
                    .reshape((2 * ff,) + a.shape[1:])
                fused = {"qkv": tuple(np.concatenate([qs[f"self_attn.{n}_proj"][k] for n in "qkv"], 0) for k in (0, 1)),
                         "o": qs["self_attn.o_proj"],
                         "gate_up": (il(qs["mlp.gate_proj"][0], qs["mlp.up_proj"][0]), il(qs["mlp.gate_proj"][1], qs["mlp.up_proj"][1])),
                         "down": qs["mlp.down_proj"]}
                for n, (q, sc) in fused.items():
                    off8, _ = self.layout[d + n + ".w8"]
                    src = torch.from_numpy(np.ascontiguousarray(pack_w16x64_fp8(q)).reshape(-1))
                    self.arena[off8:off8 + src.numel()].copy_(src, non_blocking=False)
                    offs, _ = self.layout[d + n + ".s"]
                    srcs = torch.from_numpy(np.ascontiguousarray(sc, np.float32).view(np.uint8).reshape(-1))
                    self.arena[offs:offs + srcs.numel()].copy_(srcs, non_blocking=False)
                    self._put(d + n + ".w", pack_w16x64(to_bf16_bits(fp8_e4m3_to_f32(q) * sc[:, None])))
                continue
            self._put(d + "qkv.w", pack_w16x64(np.concatenate([_bits(w[s + f"self_attn.{n}_proj.weight"]) for n in "qkv"], 0)))
            self._put(d + "o.w", pack_w16x64(_bits(w[s + "self_attn.o_proj.weight"])))
            g = _bits(w[s + "mlp.gate_proj.weight"]).reshape(ff // 8, 8, -1)   # 8-row interleave: KR_EPI_SILU_MUL8
            u = _bits(w[s + "mlp.up_proj.weight"]).reshape(ff // 8, 8, -1)
            self._put(d + "gate_up.w", pack_w16x64(np.stack([g, u], 1).reshape(2 * ff, -1)))
            self._put(d + "down.w", pack_w16x64(_bits(w[s + "mlp.down_proj.weight"])))
        self._put("llm.norm.w", _bits(w[Lm + "norm.weight"]))
        head = w[Lm + "embed_tokens.weight"] if (t.tie_word_embeddings or "lm_head.weight" not in w) else w["lm_head.weight"]
        self._put("llm.lm_head", pack_w16x64(_bits(head)))
        torch.cuda.synchronize(self.device)
