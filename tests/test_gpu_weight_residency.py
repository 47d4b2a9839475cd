"""kr_narrow_opts.w_resident changes the cache policy of a narrow launch's weight loads and nothing else: every output byte of a
resident launch equals the nontemporal launch's, at the smallest shapes that reach the instantiations the switch touches, and an
engine gives the same tokens and logits whatever its residency budget."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd import weights as WT  # noqa: E402
from karanta_ocr_amd._lib import DEC_PLAIN, DEC_ROPE_KV, lib, narrow_opts, ptr  # noqa: E402
from karanta_ocr_amd.weights import bf16_round, pack_w16x64  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(bf16_round(np.asarray(a, np.float32)))).to(DEV).to(torch.bfloat16)


def raw(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def weights(rng, N, K, fp8):
    """(packed weight tensor, row scales or None)."""
    Wf = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    if fp8:
        q, sc = WT.quantize_fp8_rows(Wf)
        return torch.from_numpy(WT.pack_w16x64_fp8(q)).to(DEV), torch.from_numpy(sc).to(DEV)
    return dev_bf16(pack_w16x64(bf16_round(Wf))), None


def narrow(L, mode, x, W, sc, M, N, K, opts, out=0, out_f32=0, ldc=0, bias=0, norm_w=0, res=0, ldr=0, waves=8, ksplit=1,
           part_in=0, n_part=0, x_out=0, cs=0, cs_stride=0, plen=0, ctx=0, q_out=0, kc=0, vc=0, heads=0, kv_heads=0, s_max=64):
    head = (mode, x, K, part_in, n_part, x_out, K)
    tail = (bias, norm_w, 1e-6, res, ldr, out, out_f32, ldc, M, N, K, waves, ksplit, cs, cs_stride, plen, ctx, q_out, kc, vc, heads,
            kv_heads, s_max, opts, 0)
    if sc is not None:
        L.kr_linear_decode_narrow_fp8(*head, ptr(W), ptr(sc), *tail)
    else:
        L.kr_linear_decode_narrow(*head, ptr(W), *tail)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,fp8", [(1, False), (8, False), (16, False), (8, True)])
def test_rope_kv_resident_bits(L, M, fp8):
    """Norm prologue + one part_in slab at K = 1536 (the smallest K the slab prologue takes), one q head, one kv head: q, the K
    cache, the V^T cache, x_out and the accumulator the launch zeroes."""
    rng = np.random.default_rng(50 + M + fp8)
    K, H, KVH, hd, s_max, T = 1536, 1, 1, 128, 64, 5
    N = (H + 2 * KVH) * hd
    W, sc = weights(rng, N, K, fp8)
    x, nw = dev_bf16(rng.standard_normal((M, K)) * 2), dev_bf16(1 + 0.1 * rng.standard_normal(K))
    bias = dev_bf16(rng.standard_normal(N) * 0.1)
    part = torch.from_numpy((rng.standard_normal((1, M, K)) * 0.5).astype(np.float32)).to(DEV)
    ang = rng.uniform(0, 6.28, size=(M, T, 64)).astype(np.float32)
    cs = torch.from_numpy(np.concatenate([bf16_round(np.cos(ang)), bf16_round(np.sin(ang))], -1).astype(np.float32)).to(DEV)
    plen = rng.integers(0, s_max - T, size=M).astype(np.int32)
    ctx = torch.from_numpy(plen + rng.integers(0, T, size=M).astype(np.int32)).to(DEV)
    plen = torch.from_numpy(plen).to(DEV)
    kc0, vt0 = dev_bf16(rng.standard_normal((M, KVH, s_max, hd))), dev_bf16(rng.standard_normal((M, KVH, s_max // 64, hd, 64)))
    got = []
    for resident in (False, True):
        q = torch.full((M, H, hd), 3.0, dtype=torch.bfloat16, device=DEV)
        kc, vt = kc0.clone(), vt0.clone()
        xo = torch.full((M, K), 5.0, dtype=torch.bfloat16, device=DEV)
        acc = torch.full((M * K + 4,), 7.0, dtype=torch.float32, device=DEV)
        narrow(L, DEC_ROPE_KV, ptr(x), W, sc, M, N, K, narrow_opts(ptr(acc), M * K * 4, w_resident=resident), bias=ptr(bias),
               norm_w=ptr(nw), part_in=ptr(part), n_part=1, x_out=ptr(xo), cs=ptr(cs), cs_stride=T, plen=ptr(plen), ctx=ptr(ctx),
               q_out=ptr(q), kc=ptr(kc), vc=ptr(vt), heads=H, kv_heads=KVH, s_max=s_max)
        got.append([raw(t) for t in (q, kc, vt, xo, acc)])
    a = got[0]
    assert (a[0] != raw(torch.full((M, H, hd), 3.0, dtype=torch.bfloat16))).any() and (a[3] != raw(torch.full((M, K), 5.0, dtype=torch.bfloat16))).any()
    assert not a[4][:M * K * 4].any() and (a[1] != raw(kc0)).any() and (a[2] != raw(vt0)).any()
    for what, u, v in zip(("q", "K cache", "V^T cache", "x_out", "zeroed accumulator"), *got):
        np.testing.assert_array_equal(u, v, err_msg=what)


@pytest.mark.parametrize("K,waves,fp8", [(128, 8, False), (128, 16, False), (128, 8, True),
                                         (1536, 16, False)])           # the o_proj K of the 2B width
def test_plain_residual_bias_resident_bits(L, K, waves, fp8):
    rng = np.random.default_rng(60 + K + waves + fp8)
    M, N = 8, 32
    W, sc = weights(rng, N, K, fp8)
    x, bias, res = dev_bf16(rng.standard_normal((M, K))), dev_bf16(rng.standard_normal(N) * 0.1), dev_bf16(rng.standard_normal((M, N)))
    got = []
    for resident in (False, True):
        out = torch.full((M, N), 9.0, dtype=torch.bfloat16, device=DEV)
        narrow(L, DEC_PLAIN, ptr(x), W, sc, M, N, K, narrow_opts(w_resident=resident), out=ptr(out), ldc=N, bias=ptr(bias),
               res=ptr(res), ldr=N, waves=waves)
        got.append(raw(out))
    assert (got[0] != raw(torch.full((M, N), 9.0, dtype=torch.bfloat16))).any()
    np.testing.assert_array_equal(got[0], got[1])


@pytest.mark.parametrize("K,waves,fp8", [(256, 8, False), (256, 8, True),
                                         (8960, 16, False), (8960, 8, False)])   # the down_proj K of the 2B width: rings of 5 / 8 chunks
def test_ksplit2_atomic_slab_resident_bits(L, K, waves, fp8):
    rng = np.random.default_rng(70 + K + waves + fp8)
    M, N = 8, 32
    W, sc = weights(rng, N, K, fp8)
    x = dev_bf16(rng.standard_normal((M, K)))
    got = []
    for resident in (False, True):
        slab = torch.zeros(M, N, dtype=torch.float32, device=DEV)
        narrow(L, DEC_PLAIN, ptr(x), W, sc, M, N, K, narrow_opts(atomic_out=True, w_resident=resident), out_f32=ptr(slab), ldc=N,
               waves=waves, ksplit=2)
        got.append(raw(slab))
    assert got[0].any()
    np.testing.assert_array_equal(got[0], got[1])


def test_engine_tokens_and_logits_do_not_depend_on_the_budget():
    """The 2B widths at 2 ViT blocks and 3 decoder layers, 3 small pages, 8 replayed decode steps: budget 0, one layer's qkv,
    and everything (qkv, o_proj and down_proj of all layers)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from karanta_ocr_amd.device_weights import narrow_weight_bytes
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights
    from tests.prodwidth import page_inputs, truncated_config
    cfg = truncated_config("Qwen2-VL-2B", 2, 3)
    pages = []
    for i, (h, w) in enumerate([(56, 84), (84, 56), (112, 84)]):
        ids, pv, grid = page_inputs(cfg, 400 + i, h, w, 1024 * 1024, 3 + i, 4, 500 + i)
        pages.append(PageRequest(ids, pv, [grid]))
    eng = Engine(cfg, max_batch=4, s_max=256, max_patches=sum(len(p.pixel_values) for p in pages),
                 max_prompt_tokens=sum(len(p.input_ids) for p in pages), decode_splits=2)
    eng.load_weights(random_weights(cfg, 77))
    sizes = narrow_weight_bytes(cfg)
    gains = [("qkv", 3.0), ("o", 2.0), ("down", 1.0)]
    one = -(-sizes[0]["qkv"] // 10 ** 6)
    runs = {}
    for mb, n in ((0, 0), (one, 1), (10 ** 4, 9)):
        eng.set_resident_budget(mb, gains)
        assert len(eng.resident) == n
        # prefill token + 8 decode steps: replayed from the graph (tokens), then eager with the logits kept (a logits run does not replay)
        runs[mb] = (eng.generate(pages, 9, ignore_eos=True), eng.generate(pages, 9, ignore_eos=True, return_logits=True))
    eng.close()
    base_graph, base_eager = runs[0]
    for mb, (graph, eager) in runs.items():
        for i in range(len(pages)):
            np.testing.assert_array_equal(graph.tokens[i], base_graph.tokens[i], err_msg=f"budget {mb} MB, page {i}: replayed tokens")
            np.testing.assert_array_equal(eager.tokens[i], base_graph.tokens[i], err_msg=f"budget {mb} MB, page {i}: eager tokens")
            np.testing.assert_array_equal(eager.logits[i][-1], base_eager.logits[i][-1], err_msg=f"budget {mb} MB, page {i}: final logits")
