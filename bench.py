#!/usr/bin/env python3
"""Headline benchmark: pages/sec (+ p50 page latency) of the karanta OCR hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W          (N > 1)

Workload (BASELINE.json configs[1]): Qwen2-VL-2B bf16, batch = 8 synthetic 1024x1024 scans per GPU,
greedy, fixed T_out decode (ignore-EOS throughput mode), seeded random-init weights
of the real architecture (no checkpoints exist offline).  A "step" is one pass of the hot path over
one batch: GPU image front end (bicubic resize, normalise, patchify) -> ViT -> scatter -> prefill -> T_out greedy
decode steps.  The timed region starts with the pages resident in HBM as uint8 RGB images (what a decoded PNG is).

Multi-GPU: pure data parallel (one process per GPU, disjoint pages, no steady-state collective);
the only collective is the one-time RCCL broadcast of the packed weight arena from rank 0
(kr_bcast_weights), timed separately.  `scaling` is therefore "weak".  `python bench.py --gpus N` starts its own
N ranks (fresh child processes, before anything touches the GPU) when it was not started by torch.distributed.run;
a rank that fails — the RCCL broadcast included: it raises on every rank, and there is no fallback unless
--allow-rccl-fallback is given — makes the whole run exit non-zero.

Prints ONE JSON line (rank 0) with the contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step) and the
phases of the timed steps.  A plain run does only that: set up, warm up, time --steps steps, print.  --full adds
  decode_roofline, roofline — the decode step against the HBM roofline, and the decode gate/up GEMV (half of the decoder's
                 HBM bytes) timed live with HIP events on its launch stream (one eager step per --profile-every inside the
                 timed steps, then a chain of its own), against the 8 TB/s HBM peak;
  cpu_baseline — the oracle (numpy restatement, kind "port") timed on the host cores on a bounded
                 sample of the same workload, and `parity`: the engine against that oracle run;
  secondary*   — Qwen2-VL-7B, Qwen2-VL-2B at 32 rows and the corpus through the API, each in a fresh child process.
--dump-outputs DIR writes what the last timed step returned (GenerateResult: tokens, prompt_tokens, log-probabilities
with --logprobs) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# multi-process GPU work on this pool needs dmabuf IPC (RCCL's hipIpcGetMemHandle fails on the legacy mode): keep the setting in every
# rank's environment, before anything initialises the GPU runtime, without overriding what the launcher exported
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)

# Token ids of the Qwen2 chat template around a vision message (text first, image second, as
# create_vision_message builds it: /root/reference/karanta/data/utils.py:283-297).
IM_START, IM_END, NL = 151644, 151645, 198
N_TEXT_TOKENS = 150  # olmo_ocr_system_prompt_no_anchor (configs/prompts/open_ai_data_generation.yaml:12-20), ~125 words


def build_prompt(cfg, n_image_tokens: int, rng) -> np.ndarray:
    sys_part = [IM_START] + list(rng.integers(1000, 100000, 6)) + [IM_END, NL]           # system\nYou are a helpful assistant.
    user = [IM_START] + list(rng.integers(1000, 100000, 2 + N_TEXT_TOKENS))
    img = [cfg.vision_start_token_id] + [cfg.image_token_id] * n_image_tokens + [cfg.vision_end_token_id]
    tail = [IM_END, NL, IM_START] + list(rng.integers(1000, 100000, 2))                   # assistant\n
    ids = np.asarray(sys_part + user + img + tail, dtype=np.int64)
    return np.minimum(ids, cfg.text.vocab_size - 1)


def cpu_baseline(cfg, pv_page: np.ndarray, grid, ids: np.ndarray, t_out: int, weights=None) -> dict:
    """Oracle (numpy) on the host cores, one 1024x1024 page of the bench workload.

    With the full model's weights at hand (rank 0 has just generated them for the GPU) and enough host cores, the
    sample is the WHOLE model: every ViT block, every decoder layer of the prefill and N_DEC decode tokens are
    measured, nothing about the depth is extrapolated — only the decode length (per-token median x T_out).
    Otherwise (small hosts): the architecture truncated to 2 ViT blocks + 2 decoder layers (full widths, full
    vocabulary), per-block / per-layer times by differencing against a 1-block / 1-layer run, extrapolated linearly
    to the full depth; `sample` says which of the two ran."""
    from karanta_ocr_amd.weights import random_weights
    from oracle import qwen2vl_oracle as O  # checker / baseline only

    t_start = time.perf_counter()
    N_DEC = 16   # 58 ms per token on 16 cores: the parity block compares prefill + 16 decode steps for one more second
    try:  # BLAS threads = this job's CPU share (16 cores per GPU on the bench boxes), not every core of the host
        import threadpoolctl
        cores = min(16, os.cpu_count() or 1)
        limiter = threadpoolctl.threadpool_limits(limits=cores)
    except Exception:
        limiter, cores = None, os.cpu_count() or 1
    full = weights is not None and cores >= 12 and os.environ.get("KARANTA_CPU_BASELINE", "full") == "full"
    oracle_run: dict = {}     # the full-depth run's greedy tokens [N_DEC + 1] and logits [N_DEC + 1, V]: bench parity block

    def llm(w, mcfg, layers, img):
        tc = dataclasses.replace(mcfg.text, num_layers=layers)
        emb = O.embed_and_scatter(ids[None], img, w, mcfg)
        pos, delta = O.get_rope_index(ids[None], [grid], mcfg.image_token_id, 2)
        cache = O.KVCache.empty(layers)
        t0 = time.perf_counter()
        logits = O.decoder_forward(emb, pos, w, tc, cache)
        t_pre = time.perf_counter() - t0
        per_tok = []
        toks, logs = [], [logits[0].copy()]
        for s in range(N_DEC):
            t0 = time.perf_counter()
            nxt = logits.argmax(-1)
            toks.append(int(nxt[0]))
            e = O.embed_and_scatter(nxt[:, None], None, w, mcfg)
            ppos = np.tile((len(ids) + s + delta)[None, :, None], (3, 1, 1))
            logits = O.decoder_forward(e, ppos, w, tc, cache)
            logs.append(logits[0].copy())
            per_tok.append(time.perf_counter() - t0)
        toks.append(int(logits.argmax(-1)[0]))
        oracle_run.update(tokens=np.asarray(toks, np.int64), logits=np.stack(logs))
        return t_pre, float(np.median(per_tok))   # median: the host is shared, single tokens get preempted

    if full:
        t0 = time.perf_counter()
        img = O.vit_forward(pv_page, [grid], weights, cfg.vision)
        t_vit = time.perf_counter() - t0
        # the decoder's parameters as resident fp32 arrays — what a CPU implementation holds; left as bf16 bit patterns
        # (how rank 0 keeps them for the upload) every call would re-expand them, 1.3 s per token for nothing
        wl, note = weights, ""
        try:
            import psutil
            need = 4 * sum(int(np.prod(v.shape)) for k, v in weights.items() if not k.startswith("model.visual."))
            if psutil.virtual_memory().available > need + (8 << 30):
                wl = {k: O._w(weights, k) for k in weights if not k.startswith("model.visual.")}
            else:
                note = " (decoder weights re-expanded from bf16 on every call: host memory too small to hold them in fp32)"
        except Exception:
            note = " (decoder weights re-expanded from bf16 on every call)"
        t_pre, t_dec = llm(wl, cfg, cfg.text.num_layers, img)
        del wl
        how = (f"FULL depth measured ({cfg.vision.depth} ViT blocks, {cfg.text.num_layers} decoder layers): vit {t_vit:.1f}s + prefill "
               f"{t_pre:.1f}s + decode {t_dec*1e3:.0f} ms/token (median of {N_DEC} tokens at ctx ~{len(ids)}); only T_out={t_out} is "
               f"extrapolated (per-token x T_out){note}")
    else:
        small = dataclasses.replace(cfg, vision=dataclasses.replace(cfg.vision, depth=2),
                                    text=dataclasses.replace(cfg.text, num_layers=2))
        w = random_weights(small, 7)

        def vit(depth):
            t0 = time.perf_counter()
            out = O.vit_forward(pv_page, [grid], w, dataclasses.replace(small.vision, depth=depth))
            return time.perf_counter() - t0, out

        v2, img = vit(2)
        v1, _ = vit(1)
        p2, d2 = llm(w, small, 2, img)
        p1, d1 = llm(w, small, 1, img)
        vit_blk, pre_l, dec_l = max(v2 - v1, 0.0), max(p2 - p1, 0.0), max(d2 - d1, 0.0)
        t_vit = (v1 - vit_blk) + cfg.vision.depth * vit_blk
        t_pre = (p1 - pre_l) + cfg.text.num_layers * pre_l
        t_dec = (d1 - dec_l) + cfg.text.num_layers * dec_l
        how = (f"{cfg.name} widths TRUNCATED to 2 ViT blocks + 2 decoder layers, {N_DEC} decode tokens (median); extrapolated "
               f"linearly to {cfg.vision.depth} blocks / {cfg.text.num_layers} layers / T_out={t_out}: vit {t_vit:.1f}s + prefill "
               f"{t_pre:.1f}s + decode {t_dec*1e3:.0f} ms/token")
    if limiter is not None:
        limiter.restore_original_limits()
    t_page = t_vit + t_pre + t_out * t_dec
    return {
        "value": 1.0 / t_page, "unit": "pages/s", "cores": int(cores), "kind": "port", "cpu_model": cpu_model_name(),
        "host_cores": os.cpu_count(),
        "sample": (f"oracle/qwen2vl_oracle.py (numpy fp32, BLAS threads={cores}), 1 page 1024x1024 ({grid[1]}x{grid[2]} patches, "
                   f"P={len(ids)}); {how}; sample wall {time.perf_counter()-t_start:.0f}s"),
    }, (oracle_run if full else None)


def cpu_model_name() -> str:
    """`model name` of /proc/cpuinfo ("state core count and CPU model")."""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine() or "unknown"


# engine (bf16 storage, fp32 accumulate) vs the fp32 CPU path: oracle/tolerances.py (DESIGN.md section 2 carries the same table)
from oracle.tolerances import LOGIT_TOL_REL_FP32 as PARITY_TOL_REL, TOKEN_MARGIN_FACTOR  # noqa: E402  (checker only)


def parity_block(eng, page, oracle_run) -> dict:
    """BASELINE.md section 4's parity statement for THIS run: the full-depth oracle (fp32 policy = what the CPU / HF path
    computes) has just produced page 0's prefill logits and N greedy tokens with the same weights; the engine re-runs that
    page TEACHER-FORCED with the oracle's tokens, so every step compares (call sequence of
    /root/reference/karanta/training/test_trained_model.py:76-99)."""
    o_tok, o_log = oracle_run["tokens"], oracle_run["logits"]
    steps = len(o_tok)
    res = eng.generate([page], steps, ignore_eos=True, return_logits=True, force_tokens=o_tok[None, :steps - 1])
    got_log, got_tok = res.logits[0], np.asarray(res.tokens[0])
    rng_ = float(np.abs(o_log[0]).max())
    errs = [float(np.abs(got_log[i] - o_log[i]).max()) for i in range(steps)]
    part = np.partition(o_log, -2, axis=-1)
    margins = part[:, -1] - part[:, -2]
    tol = PARITY_TOL_REL * rng_
    decisive = [i for i in range(steps) if margins[i] > TOKEN_MARGIN_FACTOR * tol]
    equal = [int(got_tok[i]) == int(o_tok[i]) for i in range(steps)]
    return {
        "oracle": "oracle/qwen2vl_oracle.py, fp32 policy, FULL depth, page 0 of this run's batch, same weights",
        "engine_run": f"teacher-forced with the oracle's tokens, {steps} steps (prefill + {steps - 1} decode steps)",
        "max_abs_dlogit": round(max(errs), 5), "logit_range": round(rng_, 4), "rel": round(max(errs) / rng_, 5),
        "tol_rel": PARITY_TOL_REL, "argmax_equal": f"{sum(equal)}/{steps}",
        "decisive_steps": len(decisive), "decisive_argmax_equal": f"{sum(equal[i] for i in decisive)}/{len(decisive)}",
        "min_margin": round(float(margins.min()), 4),
        "pass": bool(max(errs) < tol and all(equal[i] for i in decisive)),
    }


def distribute_weights(eng, rank: int, world: int, bcast, gather, make_weights, strict: bool, log=lambda *a: None):
    """N > 1: rank 0's weight arena to every rank.  Returns (seconds in the broadcast | None, rccl_ranks | None, rccl_error | None).

    "Did RCCL move the weights between N ranks?" is answered by rccl_ranks (ncclCommCount) and rccl_weight_bcast_GBps in the JSON
    line.  A broadcast that fails raises on EVERY rank (dp.BroadcastError, agreed over the host backend); the measurement itself has
    no collective in it, so with `strict` off (--allow-rccl-fallback) the bench says so in the JSON (rccl_error, rccl_ranks null),
    lets every other rank generate the same seeded weights and still measures N GPUs.  `strict` — THE DEFAULT since round 4
    (a driver that reads only `value` and the exit code must not record an N-GPU result whose RCCL / xGMI weight path never
    worked) — re-raises: every rank exits non-zero, as the serving launcher (launch.py) always does.  Either way the ranks compare
    a digest of their arenas before anything is timed."""
    import torch
    from karanta_ocr_amd.dp import BroadcastError

    def digest():
        a = eng.w.arena
        return int(a[:: max(1, a.numel() // (1 << 22))].to(torch.int64).sum().item())

    info, bcast_s, rccl_error = {}, None, None
    try:
        bcast_s = bcast(eng.w.arena, rank, world, stream=eng.s, info=info)
    except BroadcastError as e:
        if strict:
            raise
        rccl_error = repr(e)
        print(f"[bench] rank {rank}: RCCL WEIGHT BROADCAST FAILED ({rccl_error}); every rank generates the seeded weights itself "
              f"and the run goes on WITHOUT an RCCL data path", file=sys.stderr, flush=True)
        if rank != 0:
            eng.load_weights(make_weights())
    digs = gather(digest())
    if len(set(digs)) != 1:
        raise SystemExit(f"rank {rank}: weight arena digests differ across the ranks: {digs}")
    if rccl_error is None:
        log(f"weight broadcast (kr_bcast_weights, {info.get('rccl_ranks')} RCCL ranks): {eng.w.nbytes/1e9:.2f} GB in "
            f"{bcast_s*1e3:.0f} ms; digests equal")
    return bcast_s, (info.get("rccl_ranks") if rccl_error is None else None), rccl_error


def secondary_7b(args, local_rank: int, log, with_parity: bool = True) -> dict:
    """BASELINE.json config 3's model on the SAME driver record: Qwen2-VL-7B bf16 at its per-GPU
    shapes — 4 pages per GPU (batch 32 over 8 GPUs) and 32 pages per GPU — T_out = 1024, 1024x1024 scans, 2 timed
    steps after 1 warm-up, one engine with 32 decode slots (the decode kernels are chosen by the rows of the call)."""
    import torch
    from karanta_ocr_amd import image_processing as IP
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights

    cfg = CONFIGS["Qwen2-VL-7B"]
    T_out, Bmax = args.t_out, 32
    t0 = time.perf_counter()
    rng = np.random.default_rng(4321)
    pages, im0 = [], None
    for i in range(Bmax):
        im = IP.synthetic_page(1000 + i, 1024, 1024)
        im0 = im if i == 0 else im0
        rh, rw = IP.smart_resize(im.shape[0], im.shape[1], 28, IP.MIN_PIXELS, args.max_pixels)
        g = (1, rh // 14, rw // 14)
        dev_im = torch.from_numpy(np.ascontiguousarray(im)).to(f"cuda:{local_rank}")
        pages.append(PageRequest(build_prompt(cfg, g[1] * g[2] // 4, rng), None, [g], images=[dev_im]))
    P = len(pages[0].input_ids)
    s_max = (P + T_out + 63) // 64 * 64
    eng = Engine(cfg, device=f"cuda:{local_rank}", max_batch=Bmax, s_max=s_max, max_patches=Bmax * 4900,
                 max_prompt_tokens=Bmax * P, decode_splits=args.decode_splits)
    host_w = random_weights(cfg, 0, as_bits=True)
    eng.load_weights(host_w)
    if not with_parity:
        host_w = None
    log(f"secondary: random-init {cfg.name} weights generated + uploaded in {time.perf_counter()-t0:.1f}s ({eng.w.nbytes/1e9:.2f} GB arena)")
    out = {"model": cfg.name, "dtype": "bf16", "t_out": T_out, "prompt_tokens": P, "steps": 2, "warmup": 1,
           "workload": f"{cfg.name} bf16 greedy, synthetic 1024x1024 pages, T_out={T_out} (ignore_eos), random-init weights, "
                       f"one engine with {Bmax} decode slots; BASELINE.json config 3's per-GPU shapes"}
    kvb = cfg.text.kv_bytes_per_token
    try:
        for B in (4, 32):
            sub = pages[:B]
            eng.generate(sub, T_out, ignore_eos=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ph = {"vit_s": 0.0, "prefill_s": 0.0, "decode_s": 0.0}
            for _ in range(2):
                r = eng.generate(sub, T_out, ignore_eos=True)
                for k in ph:
                    ph[k] += r.timings[k] / 2
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            bytes_step = cfg.decoder_weight_bytes("bf16") + B * (P + T_out / 2) * kvb
            step_s = ph["decode_s"] / max(T_out - 1, 1)
            out[f"b{B}_per_gpu"] = {
                "pages_per_s": round(2 * B / el, 3), "ms_per_step": round(1e3 * el / 2, 1),
                "phases_s": {k: round(v, 4) for k, v in ph.items()}, "decode_step_ms": round(1e3 * step_s, 4),
                "bytes_per_step": int(bytes_step), "t_step_roof_ms": round(1e3 * bytes_step / (HBM_PEAK_GBS * 1e9), 4),
                "frac_of_hbm_peak": round(bytes_step / (HBM_PEAK_GBS * 1e9) / step_s, 4),
            }
            log(f"secondary: {cfg.name} B={B}: {out[f'b{B}_per_gpu']}")
        if with_parity:
            out["parity_full_depth"] = parity_full_depth(eng, cfg, host_w, pages[0], im0, args, log)
    finally:
        eng.close()
    return out


def parity_full_depth(eng, cfg, host_w, page, page_img, args, log) -> dict:
    """The 7B model at FULL depth against the oracle, once per driver record (VERDICT r3 weak #1b: the 7B parity tests
    truncate to 2 + 2 layers): page 0 through cpu_baseline() — the fp32-policy oracle (what the CPU / HF path computes) on the
    same weights, every ViT block and decoder layer, prefill + 16 greedy tokens — and the engine re-run teacher-forced with
    those tokens (parity_block).  Skipped, with the reason on the record, when the host cannot hold the oracle's fp32 decoder
    weights next to the bf16 originals (re-expanding 15 GB of bf16 on every call would take minutes per token)."""
    from karanta_ocr_amd import image_processing as IP

    need = 4 * sum(int(np.prod(v.shape)) for k, v in host_w.items() if not k.startswith("model.visual.")) + (12 << 30)
    try:
        import psutil
        avail = psutil.virtual_memory().available
    except Exception:
        avail = None
    if avail is not None and avail < need:
        return {"skipped": f"host memory: {avail / 2**30:.0f} GiB available, the full-depth oracle of {cfg.name} needs ~{need / 2**30:.0f} GiB"}
    if (os.cpu_count() or 1) < 12:
        return {"skipped": f"{os.cpu_count()} host cores: the full-depth oracle of {cfg.name} is not run on fewer than 12"}
    t0 = time.perf_counter()
    pv, grid = IP.image_to_patches(page_img, max_pixels=args.max_pixels)
    base, oracle_run = cpu_baseline(cfg, pv, grid, page.input_ids, args.t_out, weights=host_w)
    if oracle_run is None:
        return {"skipped": "cpu_baseline() did not run at full depth on this host", "cpu_baseline": base}
    res = parity_block(eng, page, oracle_run)
    res["oracle"] = (f"oracle/qwen2vl_oracle.py, fp32 policy, FULL depth ({cfg.vision.depth} ViT blocks, {cfg.text.num_layers} layers) of "
                     f"{cfg.name}, same weights")
    res["oracle_seconds"] = round(time.perf_counter() - t0, 1)
    res["cpu_baseline"] = base
    log(f"secondary: {cfg.name} full-depth parity: { {k: v for k, v in res.items() if k != 'cpu_baseline'} }")
    return res


def secondary_2b_b32(args, local_rank: int, log) -> dict:
    """The headline model at the batch the continuous server decodes with: 32 pages per GPU (VERDICT r3 next #1 asks for this figure
    on the driver's record), T_out as the headline, 2 timed steps after 1 warm-up."""
    import torch
    from karanta_ocr_amd import image_processing as IP
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights

    cfg = CONFIGS["Qwen2-VL-2B"]
    T_out, B = args.t_out, 32
    rng = np.random.default_rng(4322)
    pages = []
    for i in range(B):
        im = IP.synthetic_page(2000 + i, 1024, 1024)
        rh, rw = IP.smart_resize(im.shape[0], im.shape[1], 28, IP.MIN_PIXELS, args.max_pixels)
        g = (1, rh // 14, rw // 14)
        pages.append(PageRequest(build_prompt(cfg, g[1] * g[2] // 4, rng), None, [g],
                                 images=[torch.from_numpy(np.ascontiguousarray(im)).to(f"cuda:{local_rank}")]))
    P = len(pages[0].input_ids)
    eng = Engine(cfg, device=f"cuda:{local_rank}", max_batch=B, s_max=(P + T_out + 63) // 64 * 64, max_patches=B * 4900,
                 max_prompt_tokens=B * P, decode_splits=args.decode_splits)
    eng.load_weights(random_weights(cfg, 0, as_bits=True))
    out = {"model": cfg.name, "dtype": "bf16", "t_out": T_out, "prompt_tokens": P, "steps": 2, "warmup": 1,
           "workload": f"{cfg.name} bf16 greedy, {B} synthetic 1024x1024 pages per GPU, T_out={T_out} (ignore_eos), random-init weights"}
    try:
        eng.generate(pages, T_out, ignore_eos=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ph = {"vit_s": 0.0, "prefill_s": 0.0, "decode_s": 0.0}
        for _ in range(2):
            r = eng.generate(pages, T_out, ignore_eos=True)
            for k in ph:
                ph[k] += r.timings[k] / 2
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        bytes_step = cfg.decoder_weight_bytes("bf16") + B * (P + T_out / 2) * cfg.text.kv_bytes_per_token
        step_s = ph["decode_s"] / max(T_out - 1, 1)
        out["b32_per_gpu"] = {"pages_per_s": round(2 * B / el, 3), "ms_per_step": round(1e3 * el / 2, 1),
                              "phases_s": {k: round(v, 4) for k, v in ph.items()}, "decode_step_ms": round(1e3 * step_s, 4),
                              "bytes_per_step": int(bytes_step), "t_step_roof_ms": round(1e3 * bytes_step / (HBM_PEAK_GBS * 1e9), 4),
                              "frac_of_hbm_peak": round(bytes_step / (HBM_PEAK_GBS * 1e9) / step_s, 4)}
        log(f"secondary: 2B B=32: {out['b32_per_gpu']}")
    finally:
        eng.close()
    return out


def secondary_child(kind: str, args) -> dict:
    """What `bench.py --secondary-child KIND` runs: one secondary measurement in a process of its own (a GPU fault, hang
    or OOM kill in a secondary run must not cost the headline, and the headline engine's arena must be gone before a 16.6 GB one
    is built)."""
    log = lambda *a: print("[bench]", *a, file=sys.stderr, flush=True)
    if kind == "7b":
        return secondary_7b(args, 0, log)
    if kind == "2b_b32":
        return secondary_2b_b32(args, 0, log)
    if kind == "corpus":
        import subprocess
        r = subprocess.run([sys.executable, "-m", "karanta_ocr_amd.bench_corpus", "--pages", "768"], capture_output=True, text=True,
                           cwd=ROOT, timeout=900)
        sys.stderr.write(r.stderr[-2000:])
        for line in reversed(r.stdout.splitlines()):
            if line.lstrip().startswith("{"):
                return json.loads(line)
        return {"error": f"bench_corpus exited {r.returncode} without a JSON line"}
    raise SystemExit(f"unknown --secondary-child {kind}")


def run_secondary(kind: str, args, log, timeout_s: float = 1500.0) -> dict:
    """Parent side: a FRESH child process (started after the headline engine is closed; never an exec of this one)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--secondary-child", kind, "--t-out", str(args.t_out), "--max-pixels",
           str(args.max_pixels), "--decode-splits", str(args.decode_splits)]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=sys.stderr, text=True, timeout=timeout_s, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return {"error": f"secondary '{kind}' did not finish within {timeout_s:.0f}s"}
    for line in reversed(r.stdout.splitlines()):
        if line.lstrip().startswith("{"):
            try:
                out = json.loads(line)
                out["wall_s"] = round(time.perf_counter() - t0, 1)
                return out
            except ValueError:
                break
    return {"error": f"secondary '{kind}' exited with code {r.returncode} and no JSON line"}


def kernel_source_sha16() -> str:
    import hashlib
    h = hashlib.sha256()
    for name in ("kr_decode.hip", "kr_decode32.hip", "kr_common.h"):
        with open(os.path.join(ROOT, "karanta_ocr_amd", "csrc", name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic():
    """(HBM bytes per launch of the roofline kernel, where it comes from) from the newest committed PMC pass — quoted only
    while the pass was taken on THIS kernel source (the file carries the hash of kr_decode.hip + kr_decode32.hip + kr_common.h, taken by the profiling run itself; a figure
    measured on other kernel code is dropped, not silently kept: VERDICT r2 weak #9).  (None, reason) otherwise."""
    why = "no committed PMC pass"
    for name in ("r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                doc = json.load(f)
        except Exception:
            continue
        if doc.get("kernel_source_sha16") != kernel_source_sha16():
            why = f"profiles/{name} was measured on another kr_decode.hip (hash {doc.get('kernel_source_sha16')}): not quoted"
            continue
        for kname, v in doc["kernels"].items():
            if "dec_wide_kernel<4" in kname:   # <EPI=SILU8, K/64>: the gate/up launch
                return v["hbm_read_bytes_per_launch"], "profiles/" + name
    return None, why


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict, limit: int = DUMP_LIMIT_BYTES) -> list:
    """`--dump-outputs`: {name: array with the pages on axis 0} -> out_dir/<name>.npy, token ids as float64 (exact), everything
    else as float32.  When the arrays hold more than `limit` bytes together, the same seeded sample of pages is kept from each
    of them and the sampled page indices go to pages.npy.  Returns the names written."""
    conv = {k: np.asarray(v).astype(np.float64 if np.issubdtype(np.asarray(v).dtype, np.integer) else np.float32)
            for k, v in arrays.items()}
    n = min(len(a) for a in conv.values())
    per_page = sum(a.nbytes for a in conv.values()) / max(n, 1) + 8       # + the page's entry in pages.npy
    budget = limit - 4096 * (len(conv) + 1)                               # .npy headers
    if per_page * n > budget:
        keep = int(budget // per_page)
        if keep < 1:
            raise SystemExit(f"--dump-outputs: one page's outputs alone exceed {limit} bytes")
        idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        conv = {k: a[idx] for k, a in conv.items()}
        conv["pages"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in conv.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return sorted(conv)


def result_arrays(r) -> dict:
    """The arrays a caller of Engine.generate receives (finish_reasons are strings; with ignore_eos every page runs to
    T_out, so the per-page rows stack)."""
    out = {"tokens": np.stack([np.asarray(t) for t in r.tokens]), "prompt_tokens": np.asarray(r.prompt_tokens)}
    if r.logprobs is not None and all(lp is not None for lp in r.logprobs):
        for k in ("token", "top", "top_ids"):
            out["logprob_" + k] = np.stack([lp[k] for lp in r.logprobs])
    return out


class stdout_to_stderr:
    """File-descriptor level: native libraries (gloo's "[Gloo] Rank 0 is connected ..." banner) print to fd 1, and
    rank 0's stdout must carry exactly ONE line, the JSON."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)


def spawn_ranks(n: int, argv, script: str = None, env=None, grace_s: float = 15.0) -> int:
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes of this script (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR / MASTER_PORT set, HIP_VISIBLE_DEVICES untouched), relay rank 0's stdout (the JSON line),
    let the other ranks' stdout go to stderr, and return non-zero if ANY rank does.  When one rank dies the others are
    terminated by PID after `grace_s` (they would otherwise wait in a collective forever).  Nothing here imports torch
    or touches the GPU: the children are ordinary processes, not an exec of an initialised one."""
    import socket
    import subprocess

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    base = dict(os.environ if env is None else env)
    base.update(WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    script = script or os.path.abspath(__file__)
    procs = []
    for r in range(n):
        e = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, script, *argv], env=e,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr))
    import threading
    out0: list = []
    reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    first_bad = None
    while any(p.poll() is None for p in procs):
        bad = [p for p in procs if p.poll() not in (None, 0)]
        if bad and first_bad is None:
            first_bad = time.time()
        if first_bad is not None and time.time() - first_bad > grace_s:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()
            break
        time.sleep(0.2)
    reader.join(timeout=10)
    if out0 and out0[0]:
        for line in out0[0].decode("utf-8", "replace").splitlines():
            # only the JSON line is the result; anything else a library wrote to rank 0's stdout is log output
            (sys.stdout if line.lstrip().startswith("{") else sys.stderr).write(line + "\n")
        sys.stdout.flush()
    codes = [p.returncode for p in procs]
    if any(c != 0 for c in codes):
        print(f"[bench] rank exit codes {codes}: the run is INVALID", file=sys.stderr, flush=True)
        return next(c for c in codes if c != 0) or 1
    return 0


def dry_run(args, rank: int, world: int) -> None:
    """The N-rank control plane without an engine (CPU only; gloo): what every rank does around the timed region."""
    import torch
    import torch.distributed as dist

    def barrier():
        if world > 1:
            dist.all_reduce(torch.zeros(1))

    if os.environ.get("KARANTA_BENCH_DRY_FAIL_RANK") == str(rank):      # tests: a rank that dies before the barrier
        raise SystemExit(7)
    from karanta_ocr_amd.dp import shard_pages
    mine = list(shard_pages(world * args.batch, world, rank))
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.01 * (1 + rank))          # rank-dependent "work": the MAX over ranks must win
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        counts = [None] * world
        dist.all_gather_object(counts, len(mine))
    else:
        counts = [len(mine)]
    if rank == 0:
        print(json.dumps({"metric": "pages_per_sec", "dry_run": True, "value": None, "unit": "pages/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / max(args.steps, 1), 2),
                          "pages_per_rank": counts, "scaling": "weak"}), flush=True)
    if world > 1:
        dist.all_reduce(torch.zeros(1))
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="Qwen2-VL-2B")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--t-out", type=int, default=1024)
    ap.add_argument("--page", type=int, default=1024, help="synthetic page side in pixels")
    ap.add_argument("--page-width", type=int, default=None, help="page width when not square (config 5: --page 2200 --page-width 1700)")
    ap.add_argument("--max-pixels", type=int, default=1003520, help="grid A (transformers class default)")
    ap.add_argument("--profile-every", type=int, default=None,
                    help="one eager decode step with HIP events around the gate/up launch every N steps (default: 1000 with --full, "
                         "else 0: none)")
    ap.add_argument("--full", action="store_true",
                    help="measure beyond the headline: decode roofline, live kernel timing, CPU baseline + parity and, at N = 1, the "
                         "secondary runs (a plain run sets up, warms up, times --steps steps and prints the result line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32 / float64, <= 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity block")
    ap.add_argument("--allow-rccl-fallback", action="store_true",
                    help="N > 1: when the RCCL weight broadcast fails, report rccl_error / rccl_ranks null, let every rank generate the "
                         "seeded weights and still measure (default: the run exits non-zero — a failed broadcast is a failed N-GPU run)")
    ap.add_argument("--strict-rccl", action="store_true", help="(the default since round 4; accepted for older command lines)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the runs that follow the headline at N = 1 (Qwen2-VL-7B at BASELINE config 3's per-GPU shapes + its full-depth "
                         "parity, Qwen2-VL-2B at 32 rows, the corpus through the API): each is a fresh child process")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--guided", action="store_true",
                    help="every page carries a (permissive) guide: times the masked sampling pass + DFA advance in the decode graph")
    ap.add_argument("--logprobs", type=int, default=None, help="record top-k log-probabilities every step (0..20)")
    ap.add_argument("--decode-splits", type=int, default=16,
                    help="split-KV parts of the decode attention (16: 256 workgroups of 4 waves, every CU loads; r2: -4 %% per step vs 8)")
    ap.add_argument("--weights", default="bf16", choices=("bf16", "fp8"),
                    help="fp8: decoder Linears as e4m3fn codes + per-row scales (BASELINE.json config 5); activations stay bf16")
    ap.add_argument("--fp8-act", type=int, default=None, choices=(0, 1),
                    help="with --weights fp8: W8A8 prefill (per-token e4m3 activations through the fp8 matrix instruction) on / off; "
                         "default: the engine's default")
    ap.add_argument("--secondary-child", default=None, choices=("7b", "2b_b32", "corpus"),
                    help="(internal) run ONE secondary measurement and print its JSON: the parent starts these as fresh child processes")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU rehearsal of the N-rank control plane (self-launch, rendezvous, barriers, max-over-ranks timing, "
                         "rank 0's JSON line, exit codes) with no engine: the line carries \"dry_run\": true and no measurement")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.profile_every is None:
        args.profile_every = 1000 if args.full else 0

    if args.secondary_child:
        print(json.dumps(secondary_child(args.secondary_child, args)), flush=True)
        return
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # not under torch.distributed.run: start the N ranks ourselves, BEFORE torch is imported or the GPU is touched
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: one rank per GPU")
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # control plane (barriers, the RCCL unique id, max-over-ranks timing) over gloo on CPU tensors; the
        # data plane — the one-time weight broadcast — is RCCL through the C-ABI (kr_bcast_weights)
        with stdout_to_stderr():
            dist.init_process_group("gloo", rank=rank, world_size=world)
            dist.all_reduce(torch.zeros(1))      # the first collective connects the pairs (and prints gloo's banner)
    if args.dry_run:
        return dry_run(args, rank, world)
    n_dev = torch.cuda.device_count()
    if world > 1 and n_dev < world and os.environ.get("KARANTA_BENCH_SHARE_GPUS") != "1":
        # RCCL cannot put two ranks on one device (ncclCommInitRank fails): refuse instead of producing a number that
        # is not an N-GPU number.  KARANTA_BENCH_SHARE_GPUS=1 is a control-flow rehearsal and is labelled as such.
        raise SystemExit(f"--gpus {world} needs {world} visible GPUs, found {n_dev}")
    local_rank %= max(1, n_dev)
    if world > 1:
        torch.cuda.set_device(local_rank)

    from karanta_ocr_amd import image_processing as IP
    from karanta_ocr_amd._lib import lib, ptr
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights

    cfg = CONFIGS[args.model]
    B, T_out = args.batch, args.t_out
    dev = f"cuda:{local_rank}"
    log = (lambda *a: print("[bench]", *a, file=sys.stderr, flush=True)) if rank == 0 else (lambda *a: None)

    # ---------------- inputs: synthetic scans -> patches (host) -> HBM
    t0 = time.perf_counter()
    pvs, grids, page_imgs = [], [], []
    for i in range(B):
        im = IP.synthetic_page(rank * B + i, args.page, args.page_width or args.page)
        page_imgs.append(im)
        if i == 0 and rank == 0 and args.full:   # host-side patches of page 0: the CPU baseline's input (same pixels as the GPU's)
            pv, g = IP.image_to_patches(im, max_pixels=args.max_pixels)
            pvs.append(pv)
        else:
            rh, rw = IP.smart_resize(im.shape[0], im.shape[1], 28, IP.MIN_PIXELS, args.max_pixels)
            g = (1, rh // 14, rw // 14)
        grids.append(g)
    n_img_tok = [g[1] * g[2] // 4 for g in grids]
    rng = np.random.default_rng(1234 + rank)
    # the pages enter the timed region as uint8 RGB images resident in HBM (3 MB per 1024x1024 page): resize,
    # normalisation and patch order run on the GPU inside every step (PageRequest.images, kr_image_*)
    imgs_dev = [torch.from_numpy(np.ascontiguousarray(im)).to(f"cuda:{local_rank}") for im in page_imgs]
    pages = [PageRequest(build_prompt(cfg, n_img_tok[i], rng), None, [grids[i]], images=[imgs_dev[i]]) for i in range(B)]
    P = [len(p.input_ids) for p in pages]
    log(f"preprocessed {B} pages in {time.perf_counter()-t0:.1f}s: grid {grids[0]}, image tokens {n_img_tok[0]}, prompt P={P[0]}")

    s_max = (max(P) + T_out + 63) // 64 * 64
    eng = Engine(cfg, device=dev, max_batch=B, s_max=s_max, max_patches=sum(g[1] * g[2] for g in grids),
                 max_prompt_tokens=sum(P), decode_splits=args.decode_splits, weight_dtype=args.weights,
                 fp8_activations=None if args.fp8_act is None else bool(args.fp8_act))
    if args.guided:
        # no tokenizer ships with random-init weights: the byte tokens 0..255 carry their byte, the rest are specials;
        # the pattern allows any text, so the mask / advance kernels do their full per-step work
        eng.set_vocab([bytes([i]) for i in range(256)])
        for pg in pages:
            pg.guide = r"[\s\S]*"
    if args.logprobs is not None:
        for pg in pages:
            pg.logprobs = args.logprobs

    # ---------------- weights: rank 0 materialises them, the others receive the arena over RCCL
    t0 = time.perf_counter()
    bcast_s, rccl_ranks, host_weights, rccl_error = None, None, None, None
    if rank == 0:
        host_weights = random_weights(cfg, 0, as_bits=True)
        eng.load_weights(host_weights)
        log(f"random-init {cfg.name} weights generated + uploaded in {time.perf_counter()-t0:.1f}s "
            f"({eng.w.nbytes/1e9:.2f} GB arena)")
    else:
        eng.w.allocate()
    if world > 1:
        from karanta_ocr_amd.dp import broadcast_weights

        def gather(x):
            xs = [None] * world
            dist.all_gather_object(xs, x)
            return xs

        bcast_s, rccl_ranks, rccl_error = distribute_weights(
            eng, rank, world, broadcast_weights, gather, lambda: random_weights(cfg, 0, as_bits=True), not args.allow_rccl_fallback, log)

    def one_step(profile_every=0):
        return eng.generate(pages, T_out, ignore_eos=True, use_graph=not args.no_graph, profile_every=profile_every)

    for _ in range(args.warmup):
        one_step()
    import ctypes as C
    if args.full:
        eng.kernel_profile(reset=True)
        # dispatch gap of a dependent launch in a replayed graph on this stream (what a rocprofv3 kernel
        # span contains on top of the kernel's execution: spans are contiguous in a graph replay)
        floor_us = C.c_float()
        lib().kr_probe_launch_floor(eng.s, 200, 256, 0, C.byref(floor_us))
        floor_us = float(floor_us.value)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.all_reduce(torch.zeros(1))  # CPU tensor -> gloo: the control plane never touches RCCL

    barrier()
    t_begin = time.perf_counter()
    step_times, phase = [], {"vit_s": 0.0, "prefill_s": 0.0, "decode_s": 0.0}
    for _ in range(args.steps):
        ts = time.perf_counter()
        r = one_step(args.profile_every)
        step_times.append(time.perf_counter() - ts)
        for k in phase:
            phase[k] += r.timings[k] / args.steps
    barrier()
    elapsed = time.perf_counter() - t_begin
    per_rank_pps = [B * args.steps / max(sum(step_times), 1e-9)]   # each rank's own rate over its own steps (no barrier wait)
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        rates = [None] * world
        dist.all_gather_object(rates, per_rank_pps[0])
        per_rank_pps = rates
    if args.dump_outputs:
        arrays = result_arrays(r)            # the last timed step's result; the pages of all ranks, in rank order
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, arrays)
            arrays = {k: np.concatenate([p[k] for p in parts]) for k in arrays}
        if rank == 0:
            log(f"outputs of the last timed step -> {args.dump_outputs}: {dump_outputs(args.dump_outputs, arrays)}")
    if args.full:
        prof = eng.kernel_profile()
        chain = eng.gate_up_chain_profile(B)   # live, HIP events on the launch stream, right after the timed steps
        # what a read-only stream reaches on THIS device (achieved-vs-measured-stream next to the vendor peak): the
        # weight arena (GBs: far beyond the 256 MB Infinity Cache) read once with 16-byte nontemporal loads, best of 3
        stream_gbs = C.c_float()
        lib().kr_probe_stream_read(eng.w.arena.data_ptr(), min(int(eng.w.nbytes), 4 << 30) // 16 * 16, 2048, 3, eng.s, C.byref(stream_gbs))
        stream_gbs = float(stream_gbs.value)

    if rank == 0:
        pages_total = world * B * args.steps
        value = pages_total / elapsed
        # decode roofline: bytes/step = W_dec + sum_seq ctx*kv_B at mean ctx = P + T_out/2
        kvb = cfg.text.kv_bytes_per_token
        bytes_step = cfg.decoder_weight_bytes(args.weights) + sum(p + T_out / 2 for p in P) * kvb
        t_step_roof = bytes_step / (HBM_PEAK_GBS * 1e9)
        decode_step_s = phase["decode_s"] / max(T_out - 1, 1)
        out = {
            "metric": "pages_per_sec", "value": round(value, 4), "unit": "pages/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 2),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            # the arithmetic type of the path: bf16 MFMA with fp32 accumulation either way; with --weights fp8 the decoder
            # Linears are STORED as e4m3 codes (+ f32 row scales) and converted to bf16 in registers
            "dtype": "bf16" if args.weights == "bf16" else "fp8-weights/bf16", "data": "synthetic",
            "config": {
                "workload": f"{cfg.name} {'bf16' if args.weights == 'bf16' else ('fp8-weight, W8A8 prefill / bf16-activation decode' if eng.fp8_act else 'fp8-weight / bf16-activation')} greedy, batch={B} synthetic {args.page_width or args.page}x{args.page} pages per GPU, "
                            f"max_pixels={args.max_pixels} (grid {grids[0][1]}x{grids[0][2]}, {n_img_tok[0]} image tokens), "
                            f"prompt P={P[0]} tokens, T_out={T_out} (ignore_eos), random-init weights",
                "global_batch": world * B, "parallelism": f"dp{world}", "decode": "hipGraph replay" if not args.no_graph else "eager",
                **({"prefill": ("W8A8 (per-token e4m3 activations, " + ("v_mfma_f32_16x16x32_fp8_fp8)" if os.environ.get("KARANTA_FP8_MX") == "0"
                                                                                  else "block-scaled v_mfma_scale_f32_32x32x64_f8f6f4)")) if eng.fp8_act
                    else "fp8 weights converted to bf16 in registers, bf16 MFMA"} if args.weights == "fp8" else {}),
                **({"guided": "every page, pattern [\\s\\S]*"} if args.guided else {}),
                **({"logprobs": args.logprobs} if args.logprobs is not None else {}),
            },
            "p50_latency_s": round(float(np.median(step_times)), 4),
            "phases_s": {k: round(v, 4) for k, v in phase.items()},
            "decode_step_ms": round(1e3 * decode_step_s, 4),
        }
        if args.full:
            # kernel launches of one decode step: 6 per layer (7 above 16 rows with the separate residual-sum + RMSNorm launch) + lm_head + sampling
            per_layer = 6 + (1 if (B > 16 and (eng.resnorm_qkv or (eng.family32 and eng.resnorm32_qkv))) else 0)
            launches_per_step = per_layer * cfg.text.num_layers + 2
            traffic, traffic_src = pmc_traffic()   # the committed PMC pass is of the default workload: not quoted for other shapes
            if traffic is not None and abs(traffic / chain["bytes_per_launch"] - 1.0) > 0.25:
                traffic = None
            out["decode_roofline"] = {"bytes_per_step": int(bytes_step), "t_step_roof_ms": round(1e3 * t_step_roof, 4),
                                      "frac_of_hbm_peak": round(t_step_roof / decode_step_s, 4) if decode_step_s > 0 else None,
                                      "pages_per_s_roof_per_gpu": round(B / (T_out * t_step_roof), 3),
                                      # how much of the step is seams, and what the fraction is against what a stream reaches here
                                      # (VERDICT r3 next #5): launches per step x the measured dependent-launch gap; the read-only
                                      # streaming rate of this device measured by kr_probe_stream_read just after the timed steps
                                      "launches_per_step": launches_per_step, "dispatch_gap_us": round(floor_us, 3),
                                      "launch_floor_ms": round(launches_per_step * floor_us * 1e-3, 4),
                                      "hbm_stream_measured_GBps": round(stream_gbs, 1),
                                      "frac_of_measured_stream": (round(bytes_step / (stream_gbs * 1e9) / decode_step_s, 4)
                                                                  if decode_step_s > 0 and stream_gbs > 0 else None)}
            out["roofline"] = {
                "kernel": "dec_wide_kernel<4, K/64> = <SILU8> (decode gate/up projection + fused RMSNorm + SiLU*mul, one wave per weight tile)",
                "bound": "hbm",
                "achieved": round(chain["bytes_per_launch"] / (chain["avg_us"] * 1e-6) / 1e9, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(chain["bytes_per_launch"] / (chain["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                "traffic": traffic,
                "traffic_source": (f"{traffic_src} (separate rocprofv3 --pmc FETCH_SIZE pass on this kernel source, x2 gfx950 correction)"
                                   if traffic is not None else traffic_src),
                "bytes_per_launch": chain["bytes_per_launch"], "avg_us": round(chain["avg_us"], 3),
                "launches_timed": chain["launches"],
                "avg_us_definition": "HIP events on the launch stream around a chain of back-to-back launches of this kernel, one per "
                                     "decoder layer's weights (no cache reuse), total / launches; compare the rocprofv3 kernel-trace "
                                     "average of the same kernel in profiles/r04_kernel_trace_summary.txt",
                # the same launch bracketed by events inside the timed decode steps (eager steps every --profile-every):
                "in_step": {"event_bracket_us": round(prof["bracket_us"], 3), "empty_bracket_us": round(prof["null_bracket_us"], 3),
                            "dispatch_gap_us": round(floor_us, 3), "launches_timed": prof["launches"]},
            }
        out["timed_region"] = ("uint8 RGB pages resident in HBM -> GPU image front end -> ViT -> prefill -> "
                               f"{T_out} decode steps (host-side PNG decode and the 3 MB/page H2D copy are outside)")
        if rccl_error is not None:
            out["rccl_error"] = rccl_error
            out["rccl_ranks"] = None
            out["weights"] = "generated on every rank from the same seed (the RCCL broadcast failed: rccl_error)"
        if bcast_s is not None:
            out["rccl_weight_bcast_s"] = round(bcast_s, 4)
            out["rccl_weight_bcast_path"] = ("kr_bcast_weights: ncclBroadcast of the packed arena in <= 1 GiB pieces on the engine's stream "
                                             "(RCCL picks ring / tree; SURVEY section 5's scatter + all-gather form is not built)")
            ver = C.c_int()
            lib().kr_rccl_version(C.byref(ver))
            out["rccl_version"] = int(ver.value)
            out["rccl_weight_bcast_GBps"] = round(eng.w.nbytes / 1e9 / max(bcast_s, 1e-9), 1)
            out["rccl_ranks"] = rccl_ranks
            out["per_rank_pages_per_s"] = [round(float(x), 3) for x in per_rank_pps]
            if os.environ.get("KARANTA_BENCH_SHARE_GPUS") == "1" and n_dev < world:
                out["config"]["WARNING"] = f"control-flow rehearsal: {world} ranks on {n_dev} GPU(s) — not an N-GPU measurement"
        if args.full and world == 1 and not args.no_cpu_baseline:
            log("timing the CPU baseline (oracle, bounded sample) ...")
            out["cpu_baseline"], oracle_run = cpu_baseline(cfg, pvs[0], grids[0], pages[0].input_ids, T_out, weights=host_weights)
            if oracle_run is not None:
                out["parity"] = parity_block(eng, pages[0], oracle_run)
                log(f"parity vs the full-depth oracle: {out['parity']}")
            else:
                out["parity"] = None   # the host was too small for the full-depth oracle (cpu_baseline.sample says so)
    eng.close()
    if rank == 0:
        del host_weights
        default_workload = (args.model == "Qwen2-VL-2B" and args.batch == 8 and args.weights == "bf16" and args.page == 1024
                            and args.page_width is None)
        if args.full and world == 1 and default_workload and not args.no_secondary:
            # each in a FRESH child process, after this process has released its engine: a fault, hang or OOM kill there
            # cannot take the (complete) headline record down
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            out["secondary"] = run_secondary("7b", args, log)                      # BASELINE config 3's model and per-GPU shapes
            out["secondary_2b_b32"] = run_secondary("2b_b32", args, log)           # the headline model at the server's batch
            out["secondary_corpus"] = run_secondary("corpus", args, log)           # config 4's shape on one GPU, through the API
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.all_reduce(torch.zeros(1))
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
