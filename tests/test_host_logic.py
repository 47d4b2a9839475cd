"""Host-side product logic (no GPU): image front end, position ids, attention work lists,
weight packing — checked against the HF golden fixtures and against the oracle."""
import numpy as np
import pytest
import torch

from karanta_ocr_amd import image_processing as IP
from karanta_ocr_amd import positions as POS
from karanta_ocr_amd.config import CONFIGS, QWEN2_VL_2B, QWEN2_VL_7B
from karanta_ocr_amd.weights import bf16_round, from_bf16_bits, random_weights, to_bf16_bits, weight_shapes
from oracle import qwen2vl_oracle as O

MODELS = ["tiny", "tiny-gqa"]


def test_smart_resize_matches_hf_table(golden):
    for h, w, mp, eh, ew in golden["smart_resize_table"]:
        assert IP.smart_resize(int(h), int(w), 28, 3136, int(mp)) == (int(eh), int(ew))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_image_to_patches_matches_hf(golden, tag):
    pv, grid = IP.image_to_patches(golden[f"pre_img_{tag}"])
    assert grid == tuple(golden[f"pre_grid_{tag}"][0])
    np.testing.assert_allclose(pv, golden[f"pre_pv_{tag}"], rtol=0, atol=2e-6)


def test_data_url_round_trip():
    img = IP.synthetic_page(3, 120, 90)
    url = IP.encode_png_data_url(img)
    assert url.startswith("data:image/png;base64,")
    back = np.asarray(IP.decode_data_url(url))
    np.testing.assert_array_equal(back, img)


def test_synthetic_page_is_seeded():
    a, b = IP.synthetic_page(0, 64, 64), IP.synthetic_page(0, 64, 64)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, IP.synthetic_page(1, 64, 64))
    assert a.dtype == np.uint8 and a.shape == (64, 64, 3)


def test_bench_grid_sizes():
    """1024² -> 70x70 patches (grid A) / 74x74 (grid B)."""
    pv, g = IP.image_to_patches(IP.synthetic_page(0, 1024, 1024))
    assert g == (1, 70, 70) and pv.shape == (4900, 1176)
    assert IP.smart_resize(1024, 1024, 28, 3136, IP.MAX_PIXELS_HUB) == (1036, 1036)


@pytest.mark.parametrize("name", MODELS)
def test_vision_tables(golden, tiny_models, name):
    cfg, _, P = tiny_models[name]
    grid = golden[P + "vit_grid"]
    np.testing.assert_array_equal(POS.vision_position_ids(grid, 2), golden[P + "vit_pos_ids"])
    cos, sin = POS.vision_rotary_tables(grid, cfg.vision.head_dim, 2)
    np.testing.assert_allclose(cos, golden[P + "vit_cos"], atol=1e-6)
    np.testing.assert_allclose(sin, golden[P + "vit_sin"], atol=1e-6)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("tag", ["1img", "2img"])
def test_rope_index(golden, tiny_models, name, tag):
    cfg, _, P = tiny_models[name]
    pos, delta = POS.rope_index_one(golden[P + f"rope_{tag}_ids"][0], golden[P + f"rope_{tag}_grid"], cfg.image_token_id, 2)
    np.testing.assert_array_equal(pos, golden[P + f"rope_{tag}_pos"][:, 0])
    assert delta == int(golden[P + f"rope_{tag}_delta"][0])


def test_rope_index_errors():
    with pytest.raises(ValueError, match="do not match"):
        POS.rope_index_one(np.asarray([1, 9, 9, 9, 2]), [(1, 4, 4)], 9, 2)
    with pytest.raises(ValueError):
        POS.rope_index_one(np.asarray([1, 2, 3]), [(1, 4, 4)], 9, 2)


def test_rope_index_text_only():
    pos, delta = POS.rope_index_one(np.arange(7), [], 9999, 2)
    np.testing.assert_array_equal(pos, np.tile(np.arange(7), (3, 1)))
    assert delta == 0


@pytest.mark.parametrize("name", MODELS)
def test_mrope_tables_match_oracle(golden, tiny_models, name):
    cfg, _, P = tiny_models[name]
    pos = golden[P + "mrope_pos"]  # [3,1,7]
    co, so = O.mrope_cos_sin(pos, cfg.text.head_dim, cfg.text.rope_theta, cfg.text.mrope_section)
    c, s = POS.mrope_tables(pos[:, 0], cfg.text.head_dim, cfg.text.rope_theta, cfg.text.mrope_section, round_bf16=False)
    np.testing.assert_array_equal(c, co[0])
    np.testing.assert_array_equal(s, so[0])
    cb, _ = POS.mrope_tables(pos[:, 0], cfg.text.head_dim, cfg.text.rope_theta, cfg.text.mrope_section)
    np.testing.assert_array_equal(cb, bf16_round(c))


def test_attn_plan_vit():
    plan = POS.vit_attn_plan([(1, 4, 6), (1, 14, 14), (1, 2, 2)])  # 24, 196, 4 tokens
    assert plan.n_tokens == 224 and plan.n_vt_blocks == 1 + 4 + 1
    np.testing.assert_array_equal(plan.blk_tok0, [0, 24, 88, 152, 216, 220])
    np.testing.assert_array_equal(plan.blk_ntok, [24, 64, 64, 64, 4, 4])
    np.testing.assert_array_equal(plan.blk_vt_blk, [0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(plan.blk_k_row0, [0, 24, 88, 152, 216, 220])
    # q blocks of <=128 rows: (24), (128, 68), (4) — listed heaviest first (key tiles 4, 4, 1, 1), ties in token order
    np.testing.assert_array_equal(plan.qblk[:, 0], [24, 152, 0, 220])
    np.testing.assert_array_equal(plan.qblk[:, 1], [128, 68, 24, 4])
    np.testing.assert_array_equal(plan.qblk[:, 2], [24, 24, 0, 220])
    np.testing.assert_array_equal(plan.qblk[:, 3], [1, 1, 0, 5])
    np.testing.assert_array_equal(plan.qblk_len, [[196, 0], [196, 128], [24, 0], [4, 0]])


def test_attn_plan_prefill():
    plan = POS.prefill_attn_plan([130, 5], [0, 1], kv_heads=2, s_max=256)
    np.testing.assert_array_equal(plan.blk_k_row0, [0, 64, 128, 512])
    np.testing.assert_array_equal(plan.blk_vt_blk, [0, 1, 2, 8])
    # causal: the block at query 128 sees 3 key tiles, the one at 0 sees 2, the short sequence 1 — heaviest first
    np.testing.assert_array_equal(plan.qblk[:, 2], [0, 0, 512])
    np.testing.assert_array_equal(plan.qblk_len, [[130, 128], [130, 0], [5, 0]])
    big = POS.prefill_attn_plan([1394] * 3, [0, 1, 2], kv_heads=2, s_max=1408)
    tiles = (np.minimum(big.qblk_len[:, 0], big.qblk_len[:, 1] + big.qblk[:, 1]) + 63) // 64
    assert (np.diff(tiles) <= 0).all() and tiles[0] == 22 and tiles[-1] == 2
    assert sorted(map(tuple, big.qblk[:, :2].tolist())) == sorted((s * 1394 + j, min(128, 1394 - j)) for s in range(3)
                                                                  for j in range(0, 1394, 128))


def test_bf16_helpers():
    x = np.asarray([1.0, 1.00390625, 1.005859375, -3.1415927, 1e-40, 65504.0, np.inf], np.float32)
    bits = to_bf16_bits(x)
    back = from_bf16_bits(bits)
    np.testing.assert_array_equal(back, bf16_round(x))
    t = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(back, t)  # same rounding as torch (RNE)


def test_random_weights_are_deterministic_and_bf16():
    cfg = CONFIGS["tiny"]
    a, b = random_weights(cfg, 7), random_weights(cfg, 7)
    assert set(a) == set(weight_shapes(cfg))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k], bf16_round(a[k]))
    bits = random_weights(cfg, 7, as_bits=True)
    k = "model.language_model.layers.0.mlp.down_proj.weight"
    np.testing.assert_array_equal(from_bf16_bits(bits[k]), a[k])


def test_decoder_weight_bytes_match_survey():
    assert QWEN2_VL_2B.decoder_weight_bytes() == 3_087_428_608
    assert QWEN2_VL_7B.decoder_weight_bytes() == 14_141_238_272
    assert QWEN2_VL_2B.text.kv_bytes_per_token == 28_672
    assert QWEN2_VL_7B.text.kv_bytes_per_token == 57_344


def test_weight_arena_packing_on_cpu():
    """Fused qkv, 16-row gate/up interleave and the K-padded patch embed, checked without a GPU."""
    from karanta_ocr_amd.engine import DeviceWeights

    cfg = CONFIGS["tiny-gqa"]
    w = random_weights(cfg, 11)
    dw = DeviceWeights(cfg, torch.device("cpu"))
    dw.arena = torch.zeros(dw.nbytes, dtype=torch.uint8)
    dw.load.__func__  # exists
    # load() ends with a cuda synchronize; replicate its body on CPU through _put-level checks
    import unittest.mock as mock
    with mock.patch("torch.cuda.synchronize"):
        dw.load(w)
    from karanta_ocr_amd.weights import pack_w16x64, unpack_w16x64

    t = cfg.text
    gu = unpack_w16x64(dw.view("llm.1.gate_up.w").float().numpy())
    g, u = w["model.language_model.layers.1.mlp.gate_proj.weight"], w["model.language_model.layers.1.mlp.up_proj.weight"]
    np.testing.assert_array_equal(gu[0:8], g[0:8])
    np.testing.assert_array_equal(gu[8:16], u[0:8])
    np.testing.assert_array_equal(gu[16:24], g[8:16])
    qkv = unpack_w16x64(dw.view("llm.0.qkv.w").float().numpy())
    np.testing.assert_array_equal(qkv[: t.q_dim], w["model.language_model.layers.0.self_attn.q_proj.weight"])
    np.testing.assert_array_equal(qkv[t.q_dim + t.kv_dim:], w["model.language_model.layers.0.self_attn.v_proj.weight"])
    pe = dw.view("vit.patch").float().numpy()
    assert pe.shape == (cfg.vision.embed_dim, 1216)
    np.testing.assert_array_equal(pe[:, :1176], w["model.visual.patch_embed.proj.weight"].reshape(cfg.vision.embed_dim, -1))
    assert not pe[:, 1176:].any()
    # tied lm_head: a packed copy of the embedding table (the table itself stays row-major for the gather)
    emb = w["model.language_model.embed_tokens.weight"]
    np.testing.assert_array_equal(dw.view("llm.embed").float().numpy(), emb)
    np.testing.assert_array_equal(unpack_w16x64(dw.view("llm.lm_head").float().numpy()), emb)


def test_pack_w16x64_layout():
    from karanta_ocr_amd.weights import pack_w16x64, unpack_w16x64

    w = np.arange(32 * 128, dtype=np.float32).reshape(32, 128)
    p = pack_w16x64(w).reshape(-1)
    # element (n, k) lives at ((((n/16)*(K/32) + k/32)*4 + (k%32)/8)*16 + n%16)*8 + k%8
    for n, k in ((0, 0), (19, 69), (31, 127), (5, 40)):
        off = ((((n // 16) * 4 + k // 32) * 4 + (k % 32) // 8) * 16 + n % 16) * 8 + k % 8
        assert p[off] == w[n, k]
    # lane l = 16g + r of a wave reads 8 consecutive elements at 8l of a block: row r, columns 8g..8g+7
    blk = p[:512].reshape(64, 8)
    np.testing.assert_array_equal(blk[16 * 2 + 3], w[3, 16:24])
    np.testing.assert_array_equal(unpack_w16x64(pack_w16x64(w)), w)
    with pytest.raises(ValueError):
        pack_w16x64(np.zeros((8, 64), np.float32))


def test_resample_tables_reproduce_pil_bicubic():
    """The GPU image front end's integer tables + the oracle's two-pass restatement == PIL's BICUBIC resize, bit for
    bit (down- and up-scaling, one axis unchanged, both unchanged)."""
    from PIL import Image
    from karanta_ocr_amd import image_processing as IP
    from oracle import qwen2vl_oracle as O
    rng = np.random.default_rng(0)
    for (h, w, rh, rw) in [(100, 160, 56, 84), (60, 90, 140, 112), (300, 200, 300, 140), (37, 53, 37, 53), (17, 400, 28, 420),
                           (512, 384, 476, 364)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img, "RGB").resize((rw, rh), resample=Image.BICUBIC))
        np.testing.assert_array_equal(O.resize_bicubic_u8(img, rh, rw, IP.resample_tables), ref)
    b, k = IP.resample_tables(1024, 980)
    assert b.shape == (980, 2) and k.shape[0] == 980 and (k.sum(1) - (1 << 22)).__abs__().max() <= k.shape[1]
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 1024).all()


def test_qwen2_5_config_from_hf_dict_and_weight_names():
    """A Qwen2.5-VL config.json (tower width = hidden_size, merger output = out_hidden_size) maps onto the variant
    fields; the parameter list has RMSNorm weights without biases and the biased gate / up / down MLP."""
    from karanta_ocr_amd.config import CONFIGS, from_hf_config_dict
    from karanta_ocr_amd.weights import weight_shapes
    d = {"model_type": "qwen2_5_vl", "tie_word_embeddings": True, "image_token_id": 151655,
         "text_config": {"hidden_size": 2048, "intermediate_size": 11008, "num_hidden_layers": 36, "num_attention_heads": 16,
                         "num_key_value_heads": 2, "vocab_size": 151936, "rms_norm_eps": 1e-6,
                         "rope_parameters": {"rope_theta": 1000000.0, "mrope_section": [16, 24, 24]}},
         "vision_config": {"depth": 32, "hidden_size": 1280, "out_hidden_size": 2048, "num_heads": 16, "intermediate_size": 3420,
                           "window_size": 112, "fullatt_block_indexes": [7, 15, 23, 31], "patch_size": 14,
                           "spatial_merge_size": 2, "temporal_patch_size": 2}}
    cfg = from_hf_config_dict(d, "q25")
    ref = CONFIGS["Qwen2.5-VL-3B"]
    assert cfg.vision == ref.vision and cfg.text == ref.text
    v = cfg.vision
    assert (v.variant, v.mlp_dim, v.mlp_dim_padded, v.window_merge_units, v.head_dim) == ("qwen2_5", 3420, 3456, 4, 80)
    names = weight_shapes(CONFIGS["tiny-2.5"])
    assert "model.visual.blocks.0.norm1.bias" not in names and "model.visual.merger.ln_q.bias" not in names
    assert names["model.visual.blocks.3.mlp.gate_proj.weight"] == (200, 320) and names["model.visual.blocks.3.mlp.down_proj.bias"] == (320,)
    assert "model.visual.blocks.0.mlp.fc1.weight" not in names
    old = weight_shapes(CONFIGS["tiny"])
    assert "model.visual.blocks.0.norm1.bias" in old and "model.visual.blocks.0.mlp.fc1.weight" in old


def test_fp8_e4m3_codec_and_packing():
    """OCP e4m3fn: table values, round-to-nearest-even encoding, saturation, per-row scales, the decode layout."""
    from karanta_ocr_amd import weights as W
    t = W.E4M3
    assert t[0x00] == 0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0x38] == 1.0 and t[0x7E] == 448.0
    assert t[0xB8] == -1.0 and np.isnan(t[0x7F]) and np.isnan(t[0xFF])
    codes = np.asarray([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)
    np.testing.assert_array_equal(W.f32_to_fp8_e4m3(W.fp8_e4m3_to_f32(codes)) & 0x7F | (codes & 0x80), codes | 0)   # -0 keeps its sign bit
    # ties to even: 1.0625 is halfway between 1.0 (0x38) and 1.125 (0x39) -> 0x38; 1.1875 between 0x39 and 0x3A -> 0x3A
    np.testing.assert_array_equal(W.f32_to_fp8_e4m3(np.asarray([1.0625, 1.1875, 1000.0, -1000.0, 1e-10], np.float32)),
                                  np.asarray([0x38, 0x3A, 0x7E, 0xFE, 0x00], np.uint8))
    rng = np.random.default_rng(0)
    w = rng.standard_normal((32, 128)).astype(np.float32) * rng.uniform(0.01, 5, (32, 1)).astype(np.float32)
    w[7] = 0
    q, s = W.quantize_fp8_rows(w)
    deq = W.fp8_e4m3_to_f32(q) * s[:, None]
    assert s[7] == 1 and not deq[7].any()
    assert np.abs(deq - w).max() <= np.abs(w).max(1, keepdims=True).max() * 2.0 ** -4    # 3 mantissa bits
    assert (np.abs(q.astype(np.int64) & 0x7F).max(1)[np.arange(32) != 7] == 0x7E).all()      # every row uses the full range
    np.testing.assert_array_equal(W.unpack_w16x64_fp8(W.pack_w16x64_fp8(q)), q)
    p = W.pack_w16x64_fp8(q).reshape(2, 2, 4, 16, 16)                    # [tile][chunk][g][r][16]
    np.testing.assert_array_equal(p[1, 1, 2, 5], q[16 + 5, 64 + 32:64 + 48])


def test_load_checkpoint_bf16_and_fp8_compressed_tensors(tmp_path):
    """weights.load_checkpoint on a directory shaped like a hub snapshot: bf16 tensors come back bit-exact; an fp8
    checkpoint in the compressed-tensors layout (e4m3 `weight` + per-channel or per-tensor `weight_scale`, the shape of
    the reference's allenai/olmOCR-7B-0725-FP8, karanta/constants.py:23) comes back dequantised, and re-quantising it the
    engine's way reproduces the checkpoint's codes."""
    import json
    torch = pytest.importorskip("torch")
    st = pytest.importorskip("safetensors.torch")
    from karanta_ocr_amd import weights as W
    from karanta_ocr_amd.config import TINY
    cfg = TINY
    w = W.random_weights(cfg, 3)
    hf_cfg = {"model_type": "qwen2_vl", "tie_word_embeddings": False, "eos_token_id": list(cfg.eos_token_ids),
              "image_token_id": cfg.image_token_id, "video_token_id": cfg.video_token_id,
              "vision_start_token_id": cfg.vision_start_token_id, "vision_end_token_id": cfg.vision_end_token_id,
              "text_config": {"hidden_size": cfg.text.hidden_size, "intermediate_size": cfg.text.intermediate_size,
                              "num_hidden_layers": cfg.text.num_layers, "num_attention_heads": cfg.text.num_heads,
                              "num_key_value_heads": cfg.text.num_kv_heads, "vocab_size": cfg.text.vocab_size,
                              "rms_norm_eps": cfg.text.rms_norm_eps,
                              "rope_parameters": {"rope_theta": cfg.text.rope_theta, "mrope_section": list(cfg.text.mrope_section)}},
              "vision_config": {"depth": cfg.vision.depth, "embed_dim": cfg.vision.embed_dim, "num_heads": cfg.vision.num_heads,
                                "hidden_size": cfg.vision.hidden_size, "mlp_ratio": cfg.vision.mlp_ratio}}
    quantised = {}
    tensors = {}
    for name, arr in w.items():
        t = torch.from_numpy(np.ascontiguousarray(arr))
        is_dec_linear = ".language_model.layers." in name and name.endswith("_proj.weight")
        if is_dec_linear:
            codes, sc = W.quantize_fp8_rows(arr)
            per_tensor = name.endswith("o_proj.weight")                    # one layer kind with a single scale
            if per_tensor:
                s1 = np.float32(np.abs(arr).max() / 448.0)
                codes = W.f32_to_fp8_e4m3(arr / s1)
                sc = np.full(1, s1, np.float32)
            tensors[name] = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn)
            tensors[name[:-len("weight")] + "weight_scale"] = torch.from_numpy(sc.reshape(-1, 1) if not per_tensor else sc)
            quantised[name] = (codes, sc, per_tensor)
        else:
            tensors[name] = t.to(torch.bfloat16)
    d = tmp_path / "tiny-fp8"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(hf_cfg))
    st.save_file(tensors, str(d / "model.safetensors"))
    cfg2, got = W.load_checkpoint(str(d))
    assert cfg2.text == cfg.text and cfg2.vision.depth == cfg.vision.depth and cfg2.eos_token_ids == cfg.eos_token_ids
    assert set(got) == set(w), "scale tensors are folded in, nothing else is added or lost"
    for name, arr in w.items():
        if name in quantised:
            codes, sc, per_tensor = quantised[name]
            want = W.fp8_e4m3_to_f32(codes) * (sc[0] if per_tensor else sc.reshape(-1, 1))
            np.testing.assert_array_equal(got[name], want.astype(np.float32))
            if not per_tensor:                                          # the engine's quantiser finds the same codes again
                c2, s2 = W.quantize_fp8_rows(got[name])
                np.testing.assert_array_equal(c2, codes)
                np.testing.assert_allclose(s2, sc.reshape(-1), rtol=1e-6)
        else:
            assert got[name].dtype == np.uint16                          # bf16 bit patterns
            np.testing.assert_array_equal(W.from_bf16_bits(got[name]), arr)


def test_attn_plan_picks_the_workgroup_shape():
    P = POS
    assert P.vit_attn_plan([(1, 70, 70)]).q_block == 256 and P.segments_attn_plan([64] * 40).q_block == 128
    assert P.vit_attn_plan([(1, 28, 28)]).q_block == 128              # 784 patches: a few K / V tiles only
    assert P.vit_attn_plan([(1, 158, 122)]).q_block == 256            # config 5's 19 276-patch page
    assert P.prefill_attn_plan([1394, 77], [0, 1], 2, 1408).q_block == 128
    assert P.prefill_attn_plan([8000], [0], 2, 8192).q_block == 128   # causal: always the 4-wave shape
    p128, p256 = P.make_attn_plan([300], [0], [0], False, q_block=128), P.make_attn_plan([300], [0], [0], False, q_block=256)
    assert p128.qblk[:, 1].tolist() == [128, 128, 44] and p256.qblk[:, 1].tolist() == [256, 44]
    with pytest.raises(ValueError):
        P.make_attn_plan([300], [0], [0], False, q_block=64)




def test_gpu_busy_tool_on_a_synthetic_trace(tmp_path):
    """csrc/tools/gpu_busy.py (the corpus run's busy fraction, profiles/r04_corpus_gpu_busy.txt): union of intervals, gaps by class and
    by the kernels on both sides."""
    import os, subprocess, sys
    csv = tmp_path / "trace.csv"
    csv.write_text("Kernel_Name,Start_Timestamp,End_Timestamp\n"
                   "void a<1>(int),0,1000\nvoid b(int),1500,2500\nvoid c(int),2400,3000\nvoid d(int),303000,304000\n")
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "karanta_ocr_amd", "csrc", "tools", "gpu_busy.py")
    out = subprocess.run([sys.executable, tool, str(csv)], capture_output=True, text=True, check=True).stdout
    assert "kernels 4" in out and "= 1.2 %" in out                      # 3500 ns busy of 304000
    assert "c  ->  d" in out and "n=    1  avg    300.0 us" in out       # the one long gap, attributed
    out = subprocess.run([sys.executable, tool, str(csv), "--last-s", "0.0000015"], capture_output=True, text=True, check=True).stdout
    assert "kernels 1" in out and "= 100.0 %" in out


def test_request_types_and_serving_import_without_torch():
    """PageRequest and its companions are plain data: importing them, or the serving layer that builds them, loads neither
    torch nor the HIP library (engine.py re-exports them for its callers)."""
    import os
    import subprocess
    import sys
    code = ("import sys; import karanta_ocr_amd.request as r, karanta_ocr_amd.serving, karanta_ocr_amd._lib as l; "
            "assert 'torch' not in sys.modules and l._LIB is None; "
            "assert [c.seed for c in r.children([r.PageRequest([1, 2], n=3, seed=0xFFFFFFFF)])] == [0xFFFFFFFF, 0, 1]")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], cwd=root, check=True, timeout=60)
