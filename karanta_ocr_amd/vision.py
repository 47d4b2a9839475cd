"""The vision tower of the engine: its buffers, the per-geometry tables it caches, the GPU image front end and the ViT forward.
The launches go through the engine's helpers (Engine._gemm, Engine._attention) on the engine's current stream."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import image_processing as IP
from . import positions as POS
from ._lib import EPI_GELU_ERF, EPI_QUICK_GELU, EPI_SILU_MUL8, KarantaHipError, ptr
from .request import PageRequest

BF16 = torch.bfloat16


@dataclass
class DevicePlan:
    """A positions.AttnPlan whose six work lists are resident in HBM (what kr_qkv_prep / kr_attn_varlen_q read)."""
    host: POS.AttnPlan
    blk_tok0: torch.Tensor
    blk_ntok: torch.Tensor
    blk_kr: torch.Tensor
    blk_vb: torch.Tensor
    qblk: torch.Tensor
    qlen: torch.Tensor
    n_blk: int


def device_plan(plan: POS.AttnPlan, dev: torch.device) -> DevicePlan:
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return DevicePlan(plan, t_(plan.blk_tok0), t_(plan.blk_ntok), t_(plan.blk_k_row0), t_(plan.blk_vt_blk), t_(plan.qblk),
                      t_(plan.qblk_len), len(plan.blk_tok0))


@dataclass
class VitTables:
    """What the vision tower needs per batch geometry (VisionTower._vit_tables): rotary tables (Qwen2.5-VL: in window order) and the
    whole-image attention plan; Qwen2.5-VL also the window-order gather / its inverse and the window attention plan."""
    cos: torch.Tensor
    sin: torch.Tensor
    full: DevicePlan
    perm: Optional[torch.Tensor] = None
    inv: Optional[torch.Tensor] = None
    win: Optional[DevicePlan] = None


class VisionTower:
    def __init__(self, eng):
        self.eng, self.cfg, self.device, self.L = eng, eng.cfg, eng.device, eng.L
        self._resample_cache: Dict[tuple, tuple] = {}   # (h, w, rh, rw) -> device tables of the GPU image front end
        v, t, dev, N = self.cfg.vision, self.cfg.text, self.device, eng.max_patches
        z = lambda *shape, dtype=BF16: torch.zeros(*shape, dtype=dtype, device=dev)
        nvb = N // 64 + 64  # V^T blocks: every image may add one partial block
        if v.variant == "qwen2_5":  # windowed blocks: every window starts a V^T block, edge windows are partial ones
            per_win = (v.window_merge_units * v.spatial_merge_size) ** 2
            nvb = max(nvb, 2 * (N // max(1, min(64, per_win))) + 64)
        # ViT
        self.v_pix = z(N, v.patch_dim, dtype=torch.float32)
        self.v_in = z(N, v.patch_dim_padded)
        self.v_x = z(N, v.embed_dim)
        self.v_h = z(N, v.embed_dim)
        self.v_qkv = z(N, 3 * v.embed_dim)
        self.v_q = z(v.num_heads, N, v.head_dim)
        self.v_k = z(v.num_heads, N, v.head_dim)
        self.v_vt = z(v.num_heads, nvb, v.head_dim, 64)
        self.v_o = z(N, v.embed_dim)
        self.v_f = z(N, v.mlp_dim_padded)
        self.v_perm = None  # Qwen2.5-VL: window-order gather indices live in the per-geometry cache
        self.v_m1 = z(N // 4 + 1, v.merge_dim)
        self._vit_cache = {}
        self._vit_rot_cache = {}   # (t, h, w) -> (cos, sin) of one image, resident in HBM (_vit_tables)
        self.img_embeds = z(N // 4 + 1, t.hidden_size)

    def _vit_tables(self, grids) -> VitTables:
        """Rotary tables and attention work lists depend only on the image grids: build once per
        distinct batch geometry and keep them resident in HBM."""
        key = tuple(tuple(int(x) for x in g) for g in grids)
        hit = self._vit_cache.get(key)
        if hit is None:
            v, dev = self.cfg.vision, self.device
            t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            # the rotary tables of an image depend on its own grid only: kept per grid, so that a batch of a new COMPOSITION (every
            # admission of a corpus with mixed page sizes) costs a concatenation on the device, not ~0.7 ms of numpy per page with the
            # GPU waiting (the work lists below are a few hundred integers)
            per_img = []
            for g in key:
                hit_i = self._vit_rot_cache.get(g)
                if hit_i is None:
                    c_i, s_i = POS.vision_rotary_tables((g,), v.head_dim, v.spatial_merge_size)
                    hit_i = (t_(c_i), t_(s_i))
                    if len(self._vit_rot_cache) > 64:
                        self._vit_rot_cache.clear()
                    self._vit_rot_cache[g] = hit_i
                per_img.append(hit_i)
            cos = per_img[0][0] if len(per_img) == 1 else torch.cat([c for c, _ in per_img])
            sin = per_img[0][1] if len(per_img) == 1 else torch.cat([s_ for _, s_ in per_img])
            hit = VitTables(cos, sin, device_plan(POS.vit_attn_plan(key), dev))
            if v.variant == "qwen2_5":
                # window order (TF25:430-446): patches move in groups of merge^2; rotary tables move with them;
                # two attention work lists: windows, and whole images for the fullatt_block_indexes blocks
                unit = v.spatial_merge_size ** 2
                order, win_lens = POS.vision_window_order(key, v.spatial_merge_size, v.window_size, v.patch_size)
                perm = (order[:, None] * unit + np.arange(unit)[None, :]).reshape(-1)      # patch-level gather
                perm_long = t_(perm.astype(np.int64))
                hit.cos, hit.sin = cos.index_select(0, perm_long), sin.index_select(0, perm_long)
                hit.perm, hit.inv = t_(perm.astype(np.int32)), t_(np.argsort(order).astype(np.int32))
                hit.win = device_plan(POS.segments_attn_plan(win_lens), dev)
            if len(self._vit_cache) > 16:
                self._vit_cache.clear()
            self._vit_cache[key] = hit
        return hit

    # ------------------------------------------------------------------ GPU image front end
    def patches_from_images(self, images: Sequence[np.ndarray], min_pixels: int = IP.MIN_PIXELS,
                            max_pixels: int = IP.MAX_PIXELS_CLASS_DEFAULT,
                            grids: Optional[Sequence[Sequence[int]]] = None):
        """HWC uint8 RGB pages -> (pixel_values fp32 [n, 1176] resident in HBM, grids): smart_resize on the host
        (integers), PIL-identical bicubic resize, normalisation and patch order on the GPU
        (kr_image_resize_bicubic_u8 / kr_image_normalize_patchify).  Same numbers as
        image_processing.image_to_patches, bit for bit, without the host resample and with 3 bytes per pixel
        crossing PCIe instead of 2 x 1176 floats per patch.  ``grids`` (one (1, gh, gw) per image): resize to exactly
        gh x gw patches — what the prompt's placeholders were counted for — instead of running smart_resize here."""
        v, L, s, dev = self.cfg.vision, self.L, self.eng.s, self.device
        unit = v.patch_size * v.spatial_merge_size
        metas, total = [], 0
        if grids is not None and len(grids) != len(images):
            raise KarantaHipError(f"{len(images)} images but {len(grids)} grids")
        for k, im in enumerate(images):
            if isinstance(im, torch.Tensor):       # a page already resident in HBM (uint8 HWC): no copy at all
                if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
                    raise KarantaHipError("device images must be contiguous HWC uint8 RGB tensors")
            else:
                im = np.asarray(im)
                if im.ndim == 2:
                    im = np.stack([im] * 3, axis=-1)
                if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                    raise KarantaHipError("images must be HWC uint8 RGB arrays")
                im = np.ascontiguousarray(im)
            h, w = int(im.shape[0]), int(im.shape[1])
            if grids is not None:
                g = [int(x) for x in grids[k]]
                if g[0] != 1 or g[1] % v.spatial_merge_size or g[2] % v.spatial_merge_size or min(g[1:]) < 1:
                    raise KarantaHipError(f"image grid {tuple(g)} is not (1, even, even)")
                rh, rw = g[1] * v.patch_size, g[2] * v.patch_size
            else:
                rh, rw = IP.smart_resize(h, w, unit, min_pixels, max_pixels)
            metas.append((im, h, w, rh, rw))
            total += (rh // v.patch_size) * (rw // v.patch_size)
        out = torch.empty(total, v.patch_dim, dtype=torch.float32, device=dev)
        mean = (C.c_float * 3)(*[float(x) for x in IP.CLIP_MEAN])
        std = (C.c_float * 3)(*[float(x) for x in IP.CLIP_STD])
        grids, off = [], 0
        with torch.cuda.stream(self.eng.stream):
            for im, h, w, rh, rw in metas:
                if isinstance(im, torch.Tensor):
                    src = im if im.device == dev else im.to(dev)
                else:
                    src = torch.from_numpy(im if im.flags.writeable else im.copy()).to(dev)   # PIL-backed arrays are read-only
                key = (h, w, rh, rw)
                tabs = self._resample_cache.get(key)
                if tabs is None:
                    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                    hb, hk = IP.resample_tables(w, rw) if rw != w else (None, None)
                    vb, vk = IP.resample_tables(h, rh) if rh != h else (None, None)
                    tabs = tuple(None if a is None else t_(a) for a in (hb, hk, vb, vk))
                    if len(self._resample_cache) > 64:
                        self._resample_cache.clear()
                    self._resample_cache[key] = tabs
                hb, hk, vb, vk = tabs
                dst = torch.empty(rh, rw, 3, dtype=torch.uint8, device=dev)
                tmp = torch.empty(h, rw, 3, dtype=torch.uint8, device=dev) if (rw != w and rh != h) else None
                L.kr_image_resize_bicubic_u8(ptr(src), h, w, ptr(dst), rh, rw, ptr(tmp), ptr(hb), ptr(hk),
                                             hk.shape[1] if hk is not None else 0, ptr(vb), ptr(vk),
                                             vk.shape[1] if vk is not None else 0, s)
                n = (rh // v.patch_size) * (rw // v.patch_size)
                L.kr_image_normalize_patchify(ptr(dst), rh, rw, mean, std, v.patch_size, v.spatial_merge_size,
                                              v.temporal_patch_size, ptr(out[off:]), s)
                grids.append((1, rh // v.patch_size, rw // v.patch_size))
                off += n
        return out, grids

    def _pixels_for(self, pages: Sequence[PageRequest], pixel_values_device):
        """The pixel source of a batch of pages: caller-resident patches, the GPU front end (pages with `images`),
        or the pages' host arrays."""
        if pixel_values_device is not None:
            return pixel_values_device
        with_images = [p for p in pages if p.images]
        if with_images:
            if any(p.pixel_values is not None and len(p.pixel_values) for p in pages):
                raise KarantaHipError("a batch mixes pages with `images` and pages with `pixel_values`")
            for p in pages:
                if len(p.images or []) != len(p.grids):
                    raise KarantaHipError(f"a page has {len(p.images or [])} images but {len(p.grids)} grids")
            pix, _ = self.patches_from_images([im for p in pages for im in (p.images or [])],
                                              grids=[g for p in pages for g in p.grids])
            return pix
        pvs = [p.pixel_values for p in pages if p.pixel_values is not None and len(p.pixel_values)]
        if not pvs:
            return None
        return np.concatenate(pvs, 0) if len(pvs) > 1 else pvs[0]

    def vit_forward(self, pixel_values, grids: Sequence[Sequence[int]]) -> torch.Tensor:
        """Qwen2VisionTransformerPretrainedModel.forward (TF:700-731) or its Qwen2.5-VL successor.  ``pixel_values`` is fp32
        ``[n, 1176]`` — a numpy array (copied to the device here) or a torch tensor already resident
        in HBM.  Returns a view of the merged image embeddings ``[T, d]`` (bf16, device)."""
        v, L, s, w = self.cfg.vision, self.L, self.eng.s, self.eng.w
        n = int(pixel_values.shape[0])
        if n == 0:
            return self.img_embeds[:0]
        if n > self.eng.max_patches:
            raise KarantaHipError(f"{n} patches > max_patches {self.eng.max_patches}")
        with torch.cuda.stream(self.eng.stream):
            tab = self._vit_tables(grids)
            assert tab.full.host.n_tokens == n, (tab.full.host.n_tokens, n)
            if isinstance(pixel_values, torch.Tensor):
                pix = pixel_values
                if pix.dtype != torch.float32 or not pix.is_cuda or not pix.is_contiguous():
                    raise KarantaHipError("device pixel_values must be a contiguous fp32 CUDA tensor")
            else:
                self.eng._h2d(self.v_pix, np.asarray(pixel_values, dtype=np.float32))
                pix = self.v_pix
            D, H, hd, d_out = v.embed_dim, v.num_heads, v.head_dim, self.cfg.text.hidden_size
            x, h = self.v_x, self.v_h
            L.kr_cast_pad_f32_bf16(ptr(pix), ptr(self.v_in), n, v.patch_dim, v.patch_dim_padded, s)
            self.eng._gemm(self.v_in, w.view("vit.patch"), x, n)
            if max(pl.host.n_vt_blocks for pl in (tab.full, tab.win) if pl is not None) > self.v_vt.shape[1]:
                raise KarantaHipError("too many image segments for the V^T buffer")
            # what the variant decides.  Qwen2-VL (TF:700-731): LayerNorm, fc1 / QuickGELU / fc2, attention over whole images.
            # Qwen2.5-VL (TF25:430-472): RMSNorm, biased SwiGLU, attention inside the windows except in the
            # fullatt_block_indexes blocks, tokens gathered into window order for the blocks and scattered back after the merger
            v25 = v.variant == "qwen2_5"
            if v25:
                L.kr_embed_scatter(ptr(tab.perm), ptr(x), 0, ptr(h), n, D, s)   # image order -> window order
                x, h = h, x
                norm = lambda name: L.kr_rmsnorm(ptr(x), D, ptr(w.view(name + ".w")), ptr(h), n, D, 1e-6, s)
                up, down, epi = "gate_up", "down", EPI_SILU_MUL8
            else:
                norm = lambda name: L.kr_layernorm(ptr(x), ptr(w.view(name + ".w")), ptr(w.view(name + ".b")), ptr(h), n, D, 1e-6, s)
                up, down, epi = "fc1", "fc2", EPI_QUICK_GELU
            for i in range(v.depth):
                p = f"vit.{i}."
                norm(p + "ln1")
                self.eng._gemm(h, w.view(p + "qkv.w"), self.v_qkv, n, bias=w.view(p + "qkv.b"))
                self.eng._attention(self.v_qkv, D, 2 * D, tab.cos, tab.sin, tab.win if v25 and i not in v.fullatt_block_indexes else tab.full,
                                self.v_q, self.v_k, self.v_k.stride(0), self.v_vt, self.v_vt.stride(0), self.v_o, H, H, hd, causal=False)
                self.eng._gemm(self.v_o, w.view(p + "proj.w"), x, n, bias=w.view(p + "proj.b"), res=x)
                norm(p + "ln2")
                self.eng._gemm(h, w.view(p + up + ".w"), self.v_f, n, bias=w.view(p + up + ".b"), epi=epi)
                self.eng._gemm(self.v_f, w.view(p + down + ".w"), x, n, bias=w.view(p + down + ".b"), res=x)
            # PatchMerger (TF:277-290): norm -> view [n/4, 4D] -> Linear+GELU -> Linear
            norm("vit.merger.ln")
            T = n // (v.spatial_merge_size ** 2)
            merged_in = h.view(-1)[: T * v.merge_dim].view(T, v.merge_dim)
            self.eng._gemm(merged_in, w.view("vit.merger.fc1.w"), self.v_m1, T, bias=w.view("vit.merger.fc1.b"), epi=EPI_GELU_ERF)
            # window order: the second GEMM goes to v_o, then back to image order (reverse_indices, TF25:466-468)
            out = self.v_o.view(-1)[: T * d_out].view(T, d_out) if v25 else self.img_embeds
            self.eng._gemm(self.v_m1, w.view("vit.merger.fc2.w"), out, T, bias=w.view("vit.merger.fc2.b"))
            if v25:
                L.kr_embed_scatter(ptr(tab.inv), ptr(out), 0, ptr(self.img_embeds), T, d_out, s)
        return self.img_embeds[:T]
