"""Timing of the varlen attention kernel on page-sized segments: ViT (hd 80, full, 8 images of 70x70 patches) and decoder
prefill (hd 128, causal GQA 12/2, 8 prompts of 1394 tokens), 128- vs 256-query workgroups.
    python karanta_ocr_amd/csrc/tools/attn_microbench.py
    python karanta_ocr_amd/csrc/tools/attn_microbench.py --decode [--kv-dtype fp8] [--ctx 1906] [--rows 8,32] [--splits 16]
--decode: the decode attention launch (kr_attn_decode_slots, with --kv-dtype fp8 next to kr_attn_decode_slots_kv8 in interleaved
rounds) at the 2B (12/2 heads) and 7B (28/4) widths over 16 DIFFERENT caches in turn, so that no launch finds its K / V in the
Infinity Cache: us per launch (median, min, max over the rounds) and the K / V bytes over the median."""
import ctypes as C, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from karanta_ocr_amd import positions as POS  # noqa: E402
from karanta_ocr_amd._lib import lib, ptr  # noqa: E402

L = lib()
dev = "cuda:0"
st = torch.cuda.Stream()
S = st.cuda_stream


def run(lens, H, KVH, hd, causal, q_block, reps=10):
    n = sum(lens)
    k_row0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    nb = [(x + 63) // 64 for x in lens]
    vt0 = np.concatenate([[0], np.cumsum(nb)[:-1]])
    plan = POS.make_attn_plan(lens, k_row0, vt0, causal, q_block=q_block)
    torch.manual_seed(1234)     # the same operands for both block sizes: their outputs must then be bit-identical
    q = (torch.randn(H, n, hd, device=dev) * 0.5).bfloat16()
    k = (torch.randn(KVH, n, hd, device=dev) * 0.5).bfloat16()
    vt = (torch.randn(KVH, plan.n_vt_blocks, hd, 64, device=dev)).bfloat16()
    o = torch.zeros(n, H * hd, device=dev).bfloat16()
    qb, ql = torch.from_numpy(plan.qblk).to(dev), torch.from_numpy(plan.qblk_len).to(dev)
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))

    def launch():
        L.kr_attn_varlen_q(ptr(q), ptr(k), ptr(vt), ptr(o), ptr(qb), ptr(ql), plan.qblk.shape[0], n, H, KVH, hd, n * hd,
                           plan.n_vt_blocks * hd * 64, hd ** -0.5, 1 if causal else 0, q_block, S)
    launch(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        L.kr_event_record(e0, S)
        for _ in range(reps):
            launch()
        L.kr_event_record(e1, S)
        L.kr_event_synchronize(e1)
        ms = C.c_float(); L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
        best = min(best, ms.value / reps)
    flops = sum(4.0 * x * x * hd * H * (0.5 if causal else 1.0) for x in lens)
    return best, flops / best / 1e9, o


def run_prep(lens, H, KVH, hd, reps=10):
    """kr_qkv_prep (rotary + re-layout + V transpose) on the same segments: useful bytes = qkv rows read + q/k/V^T written."""
    n = sum(lens)
    k_row0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    nb = [(x + 63) // 64 for x in lens]
    vt0 = np.concatenate([[0], np.cumsum(nb)[:-1]])
    plan = POS.make_attn_plan(lens, k_row0, vt0, False)
    ld = (H + 2 * KVH) * hd
    qkv = torch.randn(n, ld, device=dev).bfloat16()
    cos = torch.rand(n, hd, device=dev); sin = torch.rand(n, hd, device=dev)
    q = torch.empty(H, n, hd, device=dev).bfloat16(); k = torch.empty(KVH, n, hd, device=dev).bfloat16()
    vt = torch.empty(KVH, plan.n_vt_blocks, hd, 64, device=dev).bfloat16()
    t_ = lambda a: torch.from_numpy(a).to(dev)
    b0, bn, bk, bv = t_(plan.blk_tok0), t_(plan.blk_ntok), t_(plan.blk_k_row0), t_(plan.blk_vt_blk)
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))

    def launch():
        L.kr_qkv_prep(ptr(qkv), ld, 0, H * hd, (H + KVH) * hd, ptr(cos), ptr(sin), ptr(b0), ptr(bn), ptr(bk), ptr(bv),
                      plan.blk_tok0.shape[0], ptr(q), n * hd, ptr(k), n * hd, ptr(vt), plan.n_vt_blocks * hd * 64, H, KVH, hd, S)
    launch(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        L.kr_event_record(e0, S)
        for _ in range(reps):
            launch()
        L.kr_event_record(e1, S)
        L.kr_event_synchronize(e1)
        ms = C.c_float(); L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
        best = min(best, ms.value / reps)
    return best, 2.0 * n * ld * 2 / best / 1e6


def run_decode(B, H, KVH, ctx, n_split, kinds, rounds=7, n_caches=16):
    """{kind: us per launch of every round} of the decode attention over `n_caches` caches in turn, the kinds alternating."""
    from karanta_ocr_amd._lib import kv8
    hd, s_max = 128, (ctx + 64) // 64 * 64
    q = (torch.randn(B, H, hd, device=dev) * 0.5).bfloat16()
    ctx_d = torch.full((B,), ctx - 1, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = torch.zeros(B * H * n_split * (hd + 4), dtype=torch.float32, device=dev)
    sc = torch.ones(2, KVH, dtype=torch.float32, device=dev)
    caches = {}
    for kind in kinds:
        if kind == "fp8":
            caches[kind] = [(torch.randint(0, 0x78, (B, KVH, s_max, hd), dtype=torch.uint8, device=dev),
                             torch.randint(0, 0x78, (B, KVH, s_max, hd), dtype=torch.uint8, device=dev)) for _ in range(n_caches)]
        else:
            caches[kind] = [((torch.randn(B, KVH, s_max, hd, device=dev) * 0.5).bfloat16(),
                             torch.randn(B, KVH, s_max, hd, device=dev).bfloat16()) for _ in range(n_caches)]

    def launch(kind, i):
        k, vt = caches[kind][i]
        if kind == "fp8":
            L.kr_attn_decode_slots_kv8(ptr(q), kv8(ptr(k), ptr(vt), ptr(sc)), ptr(ctx_d), ptr(fin), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, S)
        else:
            L.kr_attn_decode_slots(ptr(q), ptr(k), ptr(vt), ptr(ctx_d), ptr(fin), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, S)
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
    out = {k: [] for k in kinds}
    passes = 8
    for r in range(rounds + 1):
        for kind in kinds:
            L.kr_event_record(e0, S)
            for _ in range(passes):
                for i in range(n_caches):
                    launch(kind, i)
            L.kr_event_record(e1, S)
            L.kr_event_synchronize(e1)
            ms = C.c_float(); L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
            if r:                                  # round 0 warms up
                out[kind].append(ms.value * 1e3 / (passes * n_caches))
    return out


def main_decode(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--kv-dtype", default="bf16", choices=("bf16", "fp8"), help="fp8: kr_attn_decode_slots_kv8 next to the bf16 launch")
    ap.add_argument("--ctx", type=int, default=1906)
    ap.add_argument("--rows", default="8,32")
    ap.add_argument("--splits", type=int, default=16)
    a = ap.parse_args(argv)
    kinds = ["bf16", "fp8"] if a.kv_dtype == "fp8" else ["bf16"]
    for name, (H, KVH) in {"2B (12/2 heads)": (12, 2), "7B (28/4 heads)": (28, 4)}.items():
        for B in [int(x) for x in a.rows.split(",")]:
            res = run_decode(B, H, KVH, a.ctx, a.splits, kinds)
            for kind in kinds:
                t = np.asarray(res[kind])
                mb = B * a.ctx * KVH * 128 * 2 * (1 if kind == "fp8" else 2) / 1e6
                print(f"decode attention {name} {B:2d} rows ctx {a.ctx} {a.splits} splits  {kind:4s} KV: median {np.median(t):7.2f} us  "
                      f"min {t.min():7.2f}  max {t.max():7.2f}  {mb:6.1f} MB of K/V  {mb / np.median(t):5.2f} TB/s", flush=True)


if __name__ == "__main__":
    if "--decode" in sys.argv:
        main_decode(sys.argv[1:])
        sys.exit(0)
    for name, (lens, H, KVH, hd) in {"qkv_prep vit 8 x 4900, 16 heads x 80": ([4900] * 8, 16, 16, 80),
                                     "qkv_prep prefill 8 x 1394, 12/2 heads x 128": ([1394] * 8, 12, 2, 128)}.items():
        ms, gbs = run_prep(lens, H, KVH, hd)
        print(f"{name:45s}            : {ms:8.3f} ms  {gbs:7.0f} GB/s (activations in + out)", flush=True)
    for name, (lens, H, KVH, hd, causal) in {"vit 8 x 4900, 16 heads x 80": ([4900] * 8, 16, 16, 80, False),
                                              "prefill 8 x 1394, 12/2 heads x 128 causal": ([1394] * 8, 12, 2, 128, True),
                                              "vit 1 x 19276": ([19276], 16, 16, 80, False)}.items():
        outs = {}
        for qb in (128, 256):
            ms, tf, o = run(lens, H, KVH, hd, causal, qb)
            outs[qb] = o
            print(f"{name:45s} q_block {qb}: {ms:8.3f} ms  {tf:7.1f} TFLOP/s", flush=True)
        print("    max |diff| between the block sizes:", max(float((outs[128].float() - o.float()).abs().max()) for o in outs.values()), flush=True)
