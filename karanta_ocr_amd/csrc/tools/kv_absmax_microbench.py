"""kr_kv_absmax next to kr_kv_quantize on the scratch of one admission: what --calculate-kv-scales adds to every layer of the
FIRST admission.

The 2B cache geometry (2 KV heads, head_dim 128), 8 slots, prompts of 1400 tokens (s_max 2048): 11.5 MB of bf16 K rows and V^T
blocks per layer.  The engine reuses ONE scratch for every layer, so the same scratch is read by every call here too (the data
may come from the Infinity Cache, as there).  `reps` calls per timed window between device events; windows of kr_kv_absmax (two
launches per call), of kr_kv_quantize and of the pair alternate, `rounds` of each; median with min-max, us per call.
Run on the GPU box: python karanta_ocr_amd/csrc/tools/kv_absmax_microbench.py [tokens per prompt] [slots]"""
import ctypes as C, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from karanta_ocr_amd._lib import kv8, kvq_plan, lib  # noqa: E402

L = lib()
dev = "cuda:0"
st = torch.cuda.Stream()
S = st.cuda_stream
KVH, HD = 2, 128


def window(run, reps):
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
    L.kr_event_record(e0, S)
    for _ in range(reps):
        run()
    L.kr_event_record(e1, S)
    L.kr_event_synchronize(e1)
    ms = C.c_float()
    L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
    L.kr_event_destroy(e0); L.kr_event_destroy(e1)
    return ms.value * 1e3 / reps


def main(P=1400, slots=8, reps=200, rounds=7):
    s_max = (P + 64 + 63) // 64 * 64
    g = torch.Generator(device=dev).manual_seed(0)
    k = torch.randn(slots, KVH, s_max, HD, device=dev, generator=g).to(torch.bfloat16)
    vt = (torch.randn(slots, KVH, s_max // 64, 2, HD, 32, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    k8, vt8 = torch.zeros(k.shape, dtype=torch.uint8, device=dev), torch.zeros(vt.shape, dtype=torch.uint8, device=dev)
    scale = torch.ones(2, KVH, dtype=torch.float32, device=dev)
    work = torch.zeros(2 * KVH, dtype=torch.int32, device=dev)
    nc = torch.zeros(1, dtype=torch.int32, device=dev)
    plan = [(j, P) for j in range(slots)]
    nb = (P + 63) // 64
    read = slots * KVH * (P + nb * 64) * HD * 2
    kv = lambda: kv8(k8.data_ptr(), vt8.data_ptr(), scale.data_ptr())
    absmax = lambda: L.kr_kv_absmax(k.data_ptr(), vt.data_ptr(), KVH, HD, slots, s_max, kvq_plan(plan), 200.0, 100.0, scale.data_ptr(), work.data_ptr(), S)
    quant = lambda: L.kr_kv_quantize(k.data_ptr(), vt.data_ptr(), kv(), KVH, HD, slots, s_max, kvq_plan(plan), nc.data_ptr(), S)

    def pair():
        absmax()
        quant()
    runs = {"kr_kv_absmax": absmax, "kr_kv_quantize": quant, "absmax + quantize": pair}
    for run in runs.values():           # warm-up
        window(run, 20)
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, run in runs.items():
            times[name].append(window(run, reps))
    torch.cuda.synchronize()
    want_k = float(k.float().abs().amax()) / 200.0
    print(f"geometry: {slots} slots x {KVH} KV heads x s_max {s_max} x hd {HD}; {slots} prompts of {P} tokens = {read / 1e6:.1f} MB of scratch "
          f"per call; {slots * KVH * 2 * nb} pieces; {reps} calls per window, {rounds} alternating rounds", flush=True)
    print(f"check: K scale {scale[0].max().item():.6g} (max |K| / 200 = {want_k:.6g}), work zero: {not bool(work.any())}, clamped {int(nc[0])}", flush=True)
    for name, ts in times.items():
        print(f"{name:20s} {np.median(ts):7.2f} us per call (min {min(ts):.2f}, max {max(ts):.2f})   {read / np.median(ts) / 1e6:5.2f} TB/s read", flush=True)


if __name__ == "__main__":
    torch.zeros(1, device=dev)
    main(*(int(a) for a in sys.argv[1:3]))
