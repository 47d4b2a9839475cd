"""The fp8 (e4m3fn) KV cache without a GPU: the quantisation rule of tests/kv_fp8_ref.py at the edges of the format, the
--kv-cache-dtype flag from the command line to the Engine's keyword, the per-layer k_scale / v_scale tensors of a checkpoint
through the loader into the [L, 2, KVH] table, and — on the reference alone, as test_attn_arith_cpu.py does for bf16 — that
attn_arith's bound over the dequantised operands holds for the fp8 kernel's arithmetic restated in float64."""
import types

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd import weights as W
from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.tools import synthetic_checkpoint as SC
from tests import attn_arith as AA
from tests import kv_fp8_ref as R

F32 = np.float32


# ----------------------------------------------------------------------------- the rule
def test_every_code_round_trips():
    codes = np.arange(256, dtype=np.uint8)
    finite = (codes & 0x7F) != 0x7F
    vals = W.fp8_e4m3_to_f32(codes[finite])
    assert np.array_equal(vals, W.bf16_round(vals))                        # every e4m3 value is exact in bf16
    got, clamped = R.quantize(vals, 1.0)
    np.testing.assert_array_equal(got, codes[finite])                      # -0 (0x80) included
    assert not clamped.any()
    for s in (0.5, 2.0 ** -3, 4.0):                                          # power-of-two scales: still exact
        np.testing.assert_array_equal(R.quantize(vals * F32(s), s)[0], codes[finite])
    np.testing.assert_array_equal(R.dequantize(codes[finite], 0.37), vals.astype(np.float64) * np.float64(F32(0.37)))


def test_ties_go_to_even_and_the_clamp_is_explicit():
    q = lambda x: W.fp8_e4m3_to_f32(R.quantize(np.asarray(x, F32), 1.0)[0]).tolist()
    assert q([17.0, 19.0, 21.0, 23.0]) == [16.0, 20.0, 20.0, 24.0]          # ties between neighbours: the even mantissa
    assert q([-17.0, -19.0]) == [-16.0, -20.0]
    sub = 2.0 ** -9                                                          # the smallest subnormal, and ties among the subnormals
    assert q([sub, sub / 2, 1.5 * sub, 2.5 * sub, 3.5 * sub]) == [sub, 0.0, 2 * sub, 2 * sub, 4 * sub]
    c, fl = R.quantize(np.asarray([sub / 2, -sub / 2, 0.0, -0.0], F32), 1.0)
    assert c.tolist() == [0x00, 0x80, 0x00, 0x80] and not fl.any()           # code 0 is 0.0; -0 keeps its sign
    # beyond the largest value: clamped BEFORE the conversion (449 and 464 would otherwise round, 480 and beyond have no code)
    c, fl = R.codes_of_quotient(np.asarray([448.0, -448.0, 449.0, 464.0, 480.0, 1e4, -1e4, np.inf, -np.inf], F32))
    assert c.tolist() == [0x7E, 0xFE, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0x7E, 0xFE]
    assert fl.tolist() == [False, False, True, True, True, True, True, True, True]
    # through a scale: the bf16 value is divided in f32 first
    c, fl = R.quantize(W.bf16_round(np.asarray([165.0, 166.0, 1e4, -1e4], F32)), 0.37)        # 165 / 0.37 = 445.9, 166 / 0.37 = 448.6
    assert c.tolist() == [0x7E, 0x7E, 0x7E, 0xFE] and fl.tolist() == [False, True, True, True]
    edges, _ = R.quantize(R.EDGES, 1.0)
    assert not ((edges & 0x7F) == 0x7F).any()                                # no NaN code, whatever comes in
    with pytest.raises(AssertionError):
        R.quantize(np.asarray([1.0 + 2.0 ** -10], F32), 1.0)                 # the cache takes bf16 values


def test_fast_and_reference_converters_agree_on_the_clamped_range():
    rng = np.random.default_rng(0)
    x = np.clip((rng.standard_normal(20000) * 150).astype(F32), -448, 448)
    np.testing.assert_array_equal(W.f32_to_fp8_e4m3(x), W.f32_to_fp8_e4m3_fast(x))


# ----------------------------------------------------------------------------- the flag
def test_kv_cache_dtype_spellings():
    assert [W.kv_cache_dtype_name(v) for v in ("auto", "bfloat16", "fp8", "fp8_e4m3")] == ["bf16", "bf16", "fp8", "fp8"]
    with pytest.raises(ValueError):
        W.kv_cache_dtype_name("fp8_e5m2")
    assert cli.parse_args(["serve", "/m"]).kv_cache_dtype == "auto"
    for v in ("auto", "bfloat16", "fp8", "fp8_e4m3"):
        assert cli.parse_args(["serve", "/m", "--kv-cache-dtype", v]).kv_cache_dtype == v
    with pytest.raises(SystemExit):
        cli.parse_args(["serve", "/m", "--kv-cache-dtype", "int8"])


def test_make_server_hands_the_dtype_and_the_checkpoint_scales_to_the_engine(tmp_path, monkeypatch):
    """cli.make_server on a synthetic checkpoint with k_scale / v_scale tensors and a stand-in Engine: the keyword arrives, the
    scales are read from the checkpoint and set, and the log names the cache's dtype, its bytes and the scales' source."""
    from karanta_ocr_amd import dp, engine, serving
    cfg = CONFIGS["tiny"]
    d = str(tmp_path / "ckpt")
    nl = cfg.text.num_layers
    ks, vs = 0.5 + np.arange(nl) / 4.0, 2.0 + np.arange(nl)
    SC.write_checkpoint(d, cfg, 0, kv_scales=(ks, vs))
    seen = {}

    class FakeEngine:
        def __init__(self, cfg, **kw):
            seen.update(kw)
            self.kv_cache_dtype = W.kv_cache_dtype_name(kw["kv_cache_dtype"])
            self.kv8 = self.kv_cache_dtype == "fp8"
            self.s_max, self.w, self.s, self.kv_scale_source = kw["s_max"], None, 0, "default (1.0)"

        def kv_cache_bytes(self):
            return 3 << 20

        def set_kv_scales(self, k, v, source=""):
            seen["scales"], self.kv_scale_source = (np.asarray(k), np.asarray(v)), source

    monkeypatch.setattr(engine, "Engine", FakeEngine)
    monkeypatch.setattr(dp, "load_or_receive_weights", lambda *a, **k: {"bytes": 0})
    monkeypatch.setattr(serving, "LocalServer", lambda eng, front, **kw: types.SimpleNamespace(eng=eng))
    lines = []
    cli.make_server(cli.parse_args(["serve", d, "--kv-cache-dtype", "fp8_e4m3", "--host-images"]), log=lines.append)
    assert seen["kv_cache_dtype"] == "fp8_e4m3"
    np.testing.assert_array_equal(seen["scales"][0], ks.astype(F32))
    np.testing.assert_array_equal(seen["scales"][1], vs.astype(F32))
    assert any(ln.startswith("KV cache: fp8, 3 MiB") for ln in lines) and any("scales: checkpoint" in ln for ln in lines)
    seen.clear(), lines.clear()
    cli.make_server(cli.parse_args(["serve", d, "--host-images"]), log=lines.append)
    assert seen["kv_cache_dtype"] == "auto" and "scales" not in seen and any(ln.startswith("KV cache: bf16") for ln in lines)


# ----------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("name,layout", [("tiny", "v4"), ("tiny-gqa", "v5")])
def test_checkpoint_scales_become_the_device_table(tmp_path, name, layout):
    cfg = CONFIGS[name]
    t = cfg.text
    d = str(tmp_path / "ckpt")
    ks, vs = 0.25 * (1 + np.arange(t.num_layers)), 3.0 - 0.5 * np.arange(t.num_layers)
    SC.write_checkpoint(d, cfg, 3, layout, kv_scales=(ks, vs))
    assert not cli._checkpoint_is_fp8(d)                                     # bf16 weights stay bf16 weights
    _, tensors = W.load_checkpoint(d)
    sc = W.kv_scales_from_checkpoint(tensors, cfg)
    sc2 = W.load_kv_scales(d, cfg)
    for a, b in zip(sc, sc2):
        np.testing.assert_array_equal(a, b)
    table = W.kv_scale_table(*sc, t.num_layers, t.num_kv_heads)
    assert table.shape == (t.num_layers, 2, t.num_kv_heads) and table.dtype == F32
    np.testing.assert_array_equal(table[:, 0], np.repeat(ks.astype(F32)[:, None], t.num_kv_heads, 1))    # broadcast over the heads
    np.testing.assert_array_equal(table[:, 1], np.repeat(vs.astype(F32)[:, None], t.num_kv_heads, 1))
    np.testing.assert_array_equal(table, R.scale_table(ks, vs, t.num_layers, t.num_kv_heads))
    # a checkpoint without them: None, and the weights are the seeded ones either way
    d0 = str(tmp_path / "plain")
    SC.write_checkpoint(d0, cfg, 3, layout)
    assert W.load_kv_scales(d0, cfg) is None and W.kv_scales_from_checkpoint(W.load_checkpoint(d0)[1], cfg) is None
    per_head = np.arange(t.num_layers * t.num_kv_heads, dtype=F32).reshape(t.num_layers, t.num_kv_heads) + 1
    np.testing.assert_array_equal(W.kv_scale_table(per_head, ks, t.num_layers, t.num_kv_heads)[:, 0], per_head)
    for bad in (np.ones(t.num_layers + 1), np.zeros(t.num_layers), -np.ones(t.num_layers), np.full(t.num_layers, np.nan)):
        with pytest.raises(ValueError):
            W.kv_scale_table(bad, vs, t.num_layers, t.num_kv_heads)
    del tensors["model.language_model.layers.0.self_attn.k_scale"]
    with pytest.raises(ValueError, match="k_scale for"):
        W.kv_scales_from_checkpoint(tensors, cfg)


# ----------------------------------------------------------------------------- the bound, on the reference alone
@pytest.mark.parametrize("ks,vs", R.DECODE_SCALES)
@pytest.mark.parametrize("H,KVH", R.DECODE_HEADS)
def test_the_bound_over_dequantised_operands_holds_for_the_fp8_kernels_arithmetic(H, KVH, ks, vs):
    """attn_arith.reference / bound over code x scale against the float64 model of attn_decode2_kernel<KV8> + the merge (scores
    from the code values with scale_log2e * k_scale folded in f32, P rounded to bf16, l from the rounded P, the wave's O times
    v_scale): every output within E at every split count the GPU test runs, with room to spare for the f32 arithmetic the model
    leaves out — and a model that forgets a scale misses it."""
    case, k_codes, v_codes = R.decode_case(H, KVH, ks, vs)
    sc = R.scale_rows(ks, vs, KVH)                                            # a float stands for every kv head
    assert len(case.probs) == H * len(R.DECODE_CTX) and case.l_rounded
    assert (k_codes[0, 0, 1:] == R.STALE_CODE).all()                          # row 0 has one key: the rest is the stale tail
    worst = 0.0
    for pr in case.probs[::3]:
        o, spv, _ = AA.reference(case, pr)
        e = AA.bound(case, pr, o, spv)
        b, n = int(pr.rows[0]), pr.k.shape[0]
        for n_split in R.DECODE_SPLITS:
            got = R.model_decode_kv8(pr.q, k_codes[b, pr.kvh, :n], v_codes[b, pr.kvh, :n], sc[0, pr.kvh], sc[1, pr.kvh], n_split,
                                     AA.decode_waves(n_split))
            err = np.abs(got - o)
            assert (err[e == 0] == 0).all()                                   # a zero V code under one key: met exactly
            worst = max(worst, float((err[e > 0] / e[e > 0]).max()))
    print(f"\nfp8 model H={H} KVH={KVH} scales=({ks}, {vs}): max |model - o| / E = {worst:.3f}")
    assert worst <= 0.75
    pr = case.probs[-1]
    if sc[1, pr.kvh] != 1.0:      # the V scale forgotten: far outside the bound
        o, spv, _ = AA.reference(case, pr)
        n = pr.k.shape[0]
        got = R.model_decode_kv8(pr.q, k_codes[-1, pr.kvh, :n], v_codes[-1, pr.kvh, :n], sc[0, pr.kvh], 1.0, 4, 8)
        assert (np.abs(got - o) / AA.bound(case, pr, o, spv)).max() > 10


def worst_ratio_of_the_model(case, k_codes, v_codes, sc, n_split=4):
    """max |model - o| / E over one q head per (row, kv head) when the model reads the [2][KVH] table sc."""
    g = case.heads // case.kv_heads
    worst = 0.0
    for pr in case.probs:
        if pr.head % g:
            continue
        o, spv, _ = AA.reference(case, pr)
        e = AA.bound(case, pr, o, spv)
        b, n = int(pr.rows[0]), pr.k.shape[0]
        got = R.model_decode_kv8(pr.q, k_codes[b, pr.kvh, :n], v_codes[b, pr.kvh, :n], sc[0, pr.kvh], sc[1, pr.kvh], n_split,
                                 AA.decode_waves(n_split))
        worst = max(worst, float((np.abs(got - o)[e > 0] / e[e > 0]).max()))
    return worst


@pytest.mark.parametrize("H,KVH", R.DECODE_HEADS)
def test_per_head_scales_meet_the_bound_and_another_heads_scale_does_not(H, KVH):
    """The DECODE_SCALES entry whose K and V scales differ from kv head to kv head, on the model alone: with each head's own entries
    the bound holds; with the K row of the table rotated by one head (kv_scale[(kvh + 1) % KVH] read for kv_scale[kvh]), or the V
    row, it is missed by far — what the GPU bound test would see of a kernel that indexes the table by another head."""
    ks, vs = R.DECODE_SCALES[-1]
    sc = R.scale_rows(ks, vs, KVH)
    assert len(set(sc[0])) == KVH and len(set(sc[1])) == KVH and np.ndim(ks) == 1
    case, k_codes, v_codes = R.decode_case(H, KVH, ks, vs)
    assert worst_ratio_of_the_model(case, k_codes, v_codes, sc) <= 0.75
    rot_k = np.stack([np.roll(sc[0], -1), sc[1]])
    rot_v = np.stack([sc[0], np.roll(sc[1], -1)])
    rk, rv = worst_ratio_of_the_model(case, k_codes, v_codes, rot_k), worst_ratio_of_the_model(case, k_codes, v_codes, rot_v)
    print(f"\nfp8 model H={H} KVH={KVH}: K scales rotated {rk:.1f} E, V scales rotated {rv:.1f} E")
    assert rk > 10 and rv > 10


def test_the_needle_case_is_what_it_says():
    q, k_codes, v_codes, ctx, fin, needles = R.needle_case(12, 2)
    kv, vv = W.fp8_e4m3_to_f32(k_codes), W.fp8_e4m3_to_f32(v_codes)
    for b, j0 in enumerate(needles):
        n = int(ctx[b]) + 1
        s = q[b, :128].astype(np.float64) @ kv[b, 0, :n].astype(np.float64).T * 128 ** -0.5 * 1.4426950408889634
        assert s.argmax() == j0 and (n == 1 or s[j0] - np.delete(s, j0).max() > 40)
        assert (vv[b, :, j0] == R.NEEDLE_V).all() and (vv[b, :, :n] == vv[b, :, :n, :1]).all()
        assert (np.delete(vv[b, 0, :n, 0], j0) != R.NEEDLE_V).all()
    assert len(set(np.abs(q[0, :128]).tolist())) > 8 and fin.sum() == 1
