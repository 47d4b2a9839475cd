"""Decode-step cost of the sampling controls (kr_sample_threshold + kr_gumbel_argmax_processed + kr_sample_count) at the
Qwen2-VL-2B widths: 32 text-only rows at T = 0.7, plain (kr_gumbel_argmax) against top_p = 0.9 + repetition_penalty = 1.05 on
every row.  Random-init weights; prints one JSON line.  For the per-kernel split run it under
``rocprofv3 --kernel-trace --stats -- python -m karanta_ocr_amd.tools.sampling_cost --only processed``."""
from __future__ import annotations

import argparse
import json

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--only", choices=["plain", "processed"], default=None)
    a = ap.parse_args()
    import torch
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights

    cfg = CONFIGS["Qwen2-VL-2B"]
    rng = np.random.default_rng(1)
    P = 96
    eng = Engine(cfg, max_batch=a.rows, s_max=(P + a.steps + 63) // 64 * 64, max_patches=64, max_prompt_tokens=a.rows * P)
    eng.load_weights(random_weights(cfg, 0, as_bits=True))
    out = {"model": cfg.name, "rows": a.rows, "steps": a.steps}
    kinds = [a.only] if a.only else ["plain", "processed", "plain", "processed"]
    for kind in kinds:
        extra = dict(top_p=0.9, repetition_penalty=1.05) if kind == "processed" else {}
        pages = [PageRequest(rng.integers(0, 150000, P).astype(np.int64), None, [], temperature=0.7, seed=i, **extra)
                 for i in range(a.rows)]
        eng.generate(pages, 8, ignore_eos=True)            # warm-up: first eager step, graph capture
        torch.cuda.synchronize()
        r = eng.generate(pages, a.steps, ignore_eos=True)
        out[f"{kind}_step_us"] = round(1e6 * r.timings["decode_s"] / r.timings["decode_steps"], 2)
    if not a.only:
        out["added_us_per_step"] = round(out["processed_step_us"] - out["plain_step_us"], 2)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
