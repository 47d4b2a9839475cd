"""kr_kv_fork against a loop of Tensor.copy_ over the same spans, and the admission of one page with n = 4 against four copies.

Fork: the 2B cache geometry (28 layers, 2 KV heads, head_dim 128, s_max 16384), prompt of 1400 tokens, 1 / 3 / 7 destinations.
Every launch of a chain takes another source slot (8 slots x 40 MB of prompt rows: more than the 256 MB Infinity Cache), `reps`
launches per timed window between device events, best of `rounds`.  The baseline copies, per destination, kcache[:, d, :, :P] and
vtcache[:, d, :, :ceil(P / 64)] with Tensor.copy_: what the engine would do without the kernel.
Admission: Qwen2-VL-2B, random weights, one 1024x1024 page; generate(max_new_tokens=1) is ViT + prefill (+ fork) + first tokens.
Run on the GPU box: python karanta_ocr_amd/csrc/tools/fork_microbench.py [fork|admission]"""
import ctypes as C, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from karanta_ocr_amd._lib import fork_plan, lib  # noqa: E402

L = lib()
dev = "cuda:0"
st = torch.cuda.Stream()
S = st.cuda_stream
LAYERS, SLOTS, HEADS, S_MAX, HD, P = 28, 8, 2, 16384, 128, 1400


def time_window(run, reps=16, rounds=5):
    """Best time per call (us) of `reps` back-to-back calls on the stream, between device events."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
    for i in range(SLOTS):      # warm-up: every source slot once
        run(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        L.kr_event_record(e0, S)
        for i in range(reps):
            run(i)
        L.kr_event_record(e1, S)
        L.kr_event_synchronize(e1)
        ms = C.c_float()
        L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
        times.append(ms.value * 1e3 / reps)
    L.kr_event_destroy(e0); L.kr_event_destroy(e1)
    return min(times), float(np.median(times))


def fork_bench():
    k = torch.randint(-30000, 30000, (LAYERS, SLOTS, HEADS, S_MAX, HD), dtype=torch.int16, device=dev)
    v = torch.randint(-30000, 30000, (LAYERS, SLOTS, HEADS, S_MAX // 64, HD, 64), dtype=torch.int16, device=dev)
    nb = (P + 63) // 64
    span = LAYERS * HEADS * (P + nb * 64) * HD * 2           # bytes of one slot's prompt: K rows + whole V^T blocks
    print(f"geometry: {LAYERS} layers x {SLOTS} slots x {HEADS} KV heads x s_max {S_MAX} x hd {HD}; prompt {P} tokens = "
          f"{span / 1e6:.1f} MB per slot", flush=True)
    for nd in (1, 3, 7):
        # one plan per source slot, built outside the timed window
        plans = [fork_plan([(src, P, [(src + 1 + d) % SLOTS for d in range(nd)])]) for src in range(SLOTS)]

        def kernel(i):
            L.kr_kv_fork(k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                         LAYERS, HEADS, HD, SLOTS, S_MAX, plans[i % SLOTS], S)

        def copies(i):
            src = i % SLOTS
            with torch.cuda.stream(st):
                for d in range(nd):
                    dst = (src + 1 + d) % SLOTS
                    k[:, dst, :, :P].copy_(k[:, src, :, :P])
                    v[:, dst, :, :nb].copy_(v[:, src, :, :nb])
        moved = span * (1 + nd)                              # the source read once, every destination written
        moved_copy = span * 2 * nd                           # the loop reads the source once per destination
        (kb, km), (cb, cm) = time_window(kernel), time_window(copies)
        print(f"{nd} destination(s): kr_kv_fork {kb:8.1f} us best / {km:8.1f} median  {moved / kb / 1e6:5.2f} TB/s   |   "
              f"copy_ loop ({2 * nd} calls) {cb:8.1f} us best / {cm:8.1f} median  {moved_copy / cb / 1e6:5.2f} TB/s   |   "
              f"ratio {cb / kb:.2f}x", flush=True)


def admission_bench():
    import dataclasses
    from bench import build_prompt
    from karanta_ocr_amd import image_processing as IP
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights
    cfg = CONFIGS["Qwen2-VL-2B"]
    im = IP.synthetic_page(2000, 1024, 1024)
    rh, rw = IP.smart_resize(im.shape[0], im.shape[1], 28, IP.MIN_PIXELS, IP.MAX_PIXELS_CLASS_DEFAULT)
    g = (1, rh // 14, rw // 14)
    page = PageRequest(build_prompt(cfg, g[1] * g[2] // 4, np.random.default_rng(1)), None, [g],
                       images=[torch.from_numpy(np.ascontiguousarray(im)).to(dev)], temperature=1.0, seed=3)
    n_tok = len(page.input_ids)
    eng = Engine(cfg, device=dev, max_batch=4, s_max=(n_tok + 64 + 63) // 64 * 64, max_patches=4 * 5476, max_prompt_tokens=4 * n_tok)
    eng.load_weights(random_weights(cfg, 0, as_bits=True))
    forked = [dataclasses.replace(page, n=4)]
    explicit = [dataclasses.replace(page, seed=3 + c) for c in range(4)]
    single = [page]
    out = {}
    for _ in range(3):                        # alternating, the first round is the warm-up
        for name, pages in (("n = 4 (one prefill + fork)", forked), ("four copies (parent path)", explicit), ("one page", single)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eng.generate(pages, 1, ignore_eos=True)
            torch.cuda.synchronize()
            out.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
            out.setdefault(name + " tokens", r.tokens)
    same = all(np.array_equal(a, b) for a, b in zip(out["n = 4 (one prefill + fork) tokens"], out["four copies (parent path) tokens"]))
    print(f"admission of one 1024x1024 page ({n_tok} prompt tokens), Qwen2-VL-2B bf16, ViT + prefill + first tokens, ms per call "
          f"(warm-up, then two timed): first tokens equal: {same}", flush=True)
    for name in ("n = 4 (one prefill + fork)", "four copies (parent path)", "one page"):
        print(f"  {name:28s} {' '.join(f'{x:8.2f}' for x in out[name])}", flush=True)
    eng.close()


if __name__ == "__main__":
    torch.zeros(1, device=dev)
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "fork"):
        fork_bench()
    if which in ("all", "admission"):
        admission_bench()
