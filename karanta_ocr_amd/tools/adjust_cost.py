"""Decode-step cost of the logit adjustments (kr_logits_adjust + kr_stop_tokens + kr_logits_restore) at the Qwen2-VL-2B widths:
8 text-only rows at T = 0.7, sampling only (kr_gumbel_argmax) against the same rows with a logit_bias, min_tokens and
stop_token_ids on ONE row — the step then carries the three launches for the whole batch.  Random-init weights; the two kinds
alternate in one process; prints one JSON line."""
from __future__ import annotations

import argparse
import json

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
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
    out = {"model": cfg.name, "rows": a.rows, "steps": a.steps, "sampling_step_us": [], "adjusted_step_us": []}
    ids = [rng.integers(0, 150000, P).astype(np.int64) for _ in range(a.rows)]
    for kind in ["sampling", "adjusted"] * a.repeats:
        pages = [PageRequest(ids[i], None, [], temperature=0.7, seed=i) for i in range(a.rows)]
        if kind == "adjusted":
            pages[0].logit_bias = {int(t): -5.0 for t in range(1000, 1300)}
            pages[0].min_tokens, pages[0].stop_token_ids = 16, tuple(range(2000, 2016))
        eng.generate(pages, 8)                             # warm-up: first eager step, graph capture
        torch.cuda.synchronize()
        r = eng.generate(pages, a.steps)                   # (not ignore_eos: that drops the kr_stop_tokens launch)
        out[f"{kind}_step_us"].append(round(1e6 * r.timings["decode_s"] / r.timings["decode_steps"], 2))
    out["added_us_per_step"] = round(float(np.median(out["adjusted_step_us"]) - np.median(out["sampling_step_us"])), 2)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
