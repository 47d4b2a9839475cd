"""Decode-step cost of repetition detection (kr_repeat_detect) at the Qwen2-VL-2B widths: whole replayed greedy decode steps of 8
and of 32 text-only rows, without the pass against the same rows with it on EVERY row, all 1024 periods watched and a min_count no
output reaches — the pass runs and never triggers, so both kinds generate the same tokens.  Random-init weights; the two kinds
alternate in one process, per row count; prints one JSON line."""
from __future__ import annotations

import argparse
import json

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.request import RepetitionParams
    from karanta_ocr_amd.weights import random_weights

    cfg = CONFIGS["Qwen2-VL-2B"]
    rng = np.random.default_rng(1)
    P = 96
    w = random_weights(cfg, 0, as_bits=True)
    never = RepetitionParams(max_pattern_size=1024, min_pattern_size=1, min_count=1 << 20)
    out = {"model": cfg.name, "steps": a.steps, "repeats": a.repeats, "params": list(never.row()), "rows": {}}
    for rows in a.rows:
        eng = Engine(cfg, max_batch=rows, s_max=(P + a.steps + 63) // 64 * 64, max_patches=64, max_prompt_tokens=rows * P)
        eng.load_weights(w)
        ids = [rng.integers(0, 150000, P).astype(np.int64) for _ in range(rows)]
        res = {"off_step_us": [], "on_step_us": [], "same_tokens": True, "repetition_stops": 0}
        tokens = {}
        for kind in ["off", "on"] * a.repeats:
            pages = [PageRequest(ids[i], None, [], repetition=never if kind == "on" else None) for i in range(rows)]
            eng.generate(pages, 8)                             # warm-up: first eager step, graph capture
            torch.cuda.synchronize()
            r = eng.generate(pages, a.steps, sync_every=a.steps)   # (not ignore_eos: that drops the launch)
            res[f"{kind}_step_us"].append(round(1e6 * r.timings["decode_s"] / r.timings["decode_steps"], 2))
            tokens[kind] = [t.tolist() for t in r.tokens]
            res["repetition_stops"] += sum(x is not None for x in r.stop_reasons)
        res["same_tokens"] = tokens["off"] == tokens["on"]
        res["live_rows_at_the_end"] = sum(len(t) == a.steps for t in tokens["on"])
        res["added_us_per_step"] = round(float(np.median(res["on_step_us"]) - np.median(res["off_step_us"])), 2)
        out["rows"][str(rows)] = res
        eng.close()
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
