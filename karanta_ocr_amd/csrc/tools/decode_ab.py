"""A/B timing of the decode step (one process, interleaved rounds: cdna_hip_programming.md §5.4 rule 24).

    python karanta_ocr_amd/csrc/tools/decode_ab.py [--model Qwen2-VL-2B] [--batch 8] [--ctx 1906[,2304,...]] [--steps 64] \
        [--rounds 5] variant [variant ...]

A variant is a comma-separated list of Engine attribute overrides, e.g. `base`, `attn_fused_merge=1`,
`attn_fused_merge=1,n_split=4`; `resident=<MB>[:kind@gain+kind@gain]` sets the Infinity-Cache residency budget of the narrow
launches' weights (Engine.set_resident_budget; kinds qkv, o, down; without kinds: the engine's measured gains), e.g.
`resident=177:qkv` = qkv alone, `resident=240:qkv@0.07+o@0.02` = the planner on those gains; `kv_cache_dtype=fp8` builds that variant's
engine with the fp8 KV cache (`--kv-dtype fp8`: every variant that does not say otherwise), e.g. `base kv_cache_dtype=fp8` = bf16
against fp8 cache in interleaved rounds; `KARANTA_<NAME>=<v>` sets that environment variable while the variant's engine is built
AND while its launches are captured (the switches the library reads per launch, e.g. `base KARANTA_NARROW_XBOUND=1` against a
-DKR_NARROW_XBOUND library of build_variant.py: the narrow launches with their x operand from one cache line, timing only);
`narrow_xp=0`: o_proj / down_proj of a <= 16-row step on row-major x.  The weight arena is filled with random bf16 values ON THE
DEVICE (timing does not depend on the values), the decode state is set up directly (every sequence at context `ctx`), and each variant's decode step
is captured in a hipGraph and replayed `steps` times between two HIP events; rounds alternate between the variants.
Prints per variant: median and min ms/step, and the HBM-roofline fraction of the step."""
import argparse
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from karanta_ocr_amd._lib import lib  # noqa: E402
from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import SEQUENCE_SWITCHES, Engine  # noqa: E402
from karanta_ocr_amd.csrc.tools.experiment_engine import ExperimentEngine  # noqa: E402

EXPERIMENT_KEYS = {"fast_residual", "attn_fused_merge", "merge_in_o_proj", "_prefetch_mode", "_extra_nulls", "experiment",
                   "narrow_mode", "narrow_o", "defer_down", "atomic_slab", "resnorm_qkv"}   # only ExperimentEngine branches on these
EXPERIMENT_ENV = {"KARANTA_PREFETCH", "KARANTA_FAST_RESIDUAL", "KARANTA_ATTN_FUSED", "KARANTA_MERGE_IN_OPROJ", "KARANTA_EXTRA_NULLS",
                  "KARANTA_RESNORM_QKV", *SEQUENCE_SWITCHES}      # the superseded launch sequences: the product engine refuses them


@contextlib.contextmanager
def spec_env(spec):
    """The KARANTA_* assignments of a variant spec, in the environment for the duration of the block."""
    env = dict(kv.split("=") for kv in spec.split(",") if kv.startswith("KARANTA_"))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fill_random(arena: torch.Tensor):
    """Small random bf16 values in every 2-byte slot (fp8 codes / f32 scales of an fp8 arena come out as garbage of
    harmless magnitude: timing only)."""
    n = arena.numel() // 2
    view = arena[: 2 * n].view(torch.bfloat16)
    step = 1 << 26
    for i in range(0, n, step):
        m = min(step, n - i)
        view[i:i + m] = (torch.randn(m, device=arena.device) * 0.02).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Qwen2-VL-2B")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ctx", default="1906", help="cached tokens per sequence (bench mean: P + T_out / 2); a comma-separated list "
                                                  "times every variant at each context in turn (plain steps and --chain)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--weights", default="bf16")
    ap.add_argument("--kv-dtype", default="bf16", choices=("bf16", "fp8"), help="KV cache of the variants without a kv_cache_dtype= of their own")
    ap.add_argument("--chain", default=None,
                    help="instead of whole steps: time ONE kind of launch as a chain over the layers' weights (graph of reps x "
                         "layers launches; the per-launch figure includes the dependent-launch gap): comma-separated list of "
                         "qkv,qkv0,attn,merge,o,oheads,gateup,gateup32,down,merge+o; the 17..32-row packed family: resnorm32,qkv32,"
                         "merge32,o32,gateupxp,down32,down32t1,down32t2,down32a,down32gs,down32gs2,down32gs4; round 3's > 16-row forms: resnorm,qkvd")
    ap.add_argument("--cus", default=None,
                    help="comma-separated CU counts: replay each variant's graph on a stream masked to the first N compute units "
                         "(kr_stream_create_cu_mask) — what a decode step keeps when part of the chip is given to something else")
    ap.add_argument("--concurrent", action="store_true",
                    help="launch the variants' graphs CONCURRENTLY, each engine on its own stream (e.g. `--batch 16 --concurrent base base` "
                         "= two independent 16-row decode batches side by side), and report the wall time per step of the group")
    ap.add_argument("variants", nargs="+")
    a = ap.parse_args()
    a.ctx_list = [int(x) for x in a.ctx.split(",")]
    a.ctx = max(a.ctx_list)                 # sizes the cache; the graphs read the context from the device
    cfg = CONFIGS[a.model]
    L = lib()
    B = a.batch
    s_max = (a.ctx + a.steps * (a.rounds + 2) + 128) // 64 * 64
    engines = []
    base = None
    for spec in a.variants:
        over = {}
        env = {}
        for kv in (spec.split(",") if spec != "base" else []):
            k, v = kv.split("=")
            if k.startswith("KARANTA_"):
                env[k] = v
            else:
                over[k] = v
        if "wide_mode" in over:
            raise SystemExit("wide_mode sizes the argmax partials at construction: use KARANTA_WIDE=0")
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        cls = ExperimentEngine if (EXPERIMENT_KEYS & set(over) or EXPERIMENT_ENV & set(env)) else Engine
        over.pop("experiment", None)
        eng = cls(cfg, max_batch=B, s_max=s_max, max_patches=64, max_prompt_tokens=64,
                  decode_splits=int(over.pop("n_split", 16)), weight_dtype=a.weights,
                  **({"kv_cache_dtype": "fp8"} if over.pop("kv_cache_dtype", a.kv_dtype).startswith("fp8") else {}))
        if eng.kv8:     # codes below the NaN encodings, every value finite (timing does not depend on them)
            eng.kv.kcache.copy_(torch.randint(0, 0x78, eng.kv.kcache.shape, dtype=torch.uint8, device=eng.device))
            eng.kv.vtcache.copy_(torch.randint(0, 0x78, eng.kv.vtcache.shape, dtype=torch.uint8, device=eng.device))
        over.pop("steps_per_graph", None)     # handled where the graph is captured
        if "resident" in over:                # resident=<MB>[:kind@gain+kind@gain]: Infinity-Cache budget (and the planner's gains)
            mb, _, kinds = over.pop("resident").partition(":")
            gains = [(k.split("@")[0], float(k.split("@")[1]) if "@" in k else 1.0) for k in kinds.split("+")] if kinds else None
            eng.set_resident_budget(int(mb), gains)
            print(f"{spec}: {len(eng.resident)} resident launches "
                  f"({', '.join(f'{k} x {sum(1 for _, kk in eng.resident if kk == k)}' for k in sorted({k for _, k in eng.resident}))})", flush=True)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if base is None:
            eng.w.allocate()
            fill_random(eng.w.arena)
            base = eng
        else:
            eng.w = base.w          # same arena: one copy of the weights for every variant
        for k, v in over.items():
            cur = getattr(eng, k)
            setattr(eng, k, type(cur)(int(v)) if isinstance(cur, (bool, int)) else type(cur)(v))
        eng._enter_mode(a.steps * (a.rounds + 2) + 8, ignore_eos=True, freeze_finished=False, want_logits=False, caps=eng._caps,
                        step=eng._step, logprobs=None)
        engines.append((spec, eng))

    def reset(eng, ctx=None):
        ctx = a.ctx if ctx is None else ctx
        with torch.cuda.stream(eng.stream):
            eng.d_ctx.fill_(ctx)            # the state a decode step finds: ctx tokens cached, decode position ctx - plen = 0
            eng.d_plen.fill_(ctx)
            eng.d_fin.zero_()
            eng.d_x.copy_((torch.randn(eng.d_x.shape, device=eng.device) * 0.5).to(torch.bfloat16))
        eng.stream.synchronize()

    if a.chain:
        return chains(a, engines, reset)
    graphs, per_graph = {}, {}
    for spec, eng in engines:
        reset(eng)
        k = 1
        for kv in spec.split(","):
            if kv.startswith("steps_per_graph="):
                k = int(kv.split("=")[1])
        per_graph[spec] = k
        with spec_env(spec), torch.cuda.stream(eng.stream):
            eng._decode_step_launches(B)          # eager once (function attributes), then captured
            eng.stream.synchronize()
            if k == 1:
                graphs[spec] = eng._graph_for(B)
            else:                                 # k consecutive steps in ONE graph (the state lives on the device)
                L.kr_graph_begin_capture(eng.s)
                for _ in range(k):
                    eng._decode_step_launches(B)
                g = C.c_void_p()
                L.kr_graph_end_capture(eng.s, C.byref(g))
                graphs[spec] = g.value
    if a.concurrent:
        import time
        kvb = cfg.text.kv_bytes_per_token
        ts = []
        for r in range(a.rounds + 1):
            for _, eng in engines:
                reset(eng)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                for spec, eng in engines:
                    L.kr_graph_launch(graphs[spec], eng.s)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) / a.steps * 1e3)
        n = len(engines)
        roof_ms = (n * cfg.decoder_weight_bytes(a.weights) + n * B * (a.ctx + a.steps / 2) * kvb) / 8e12 * 1e3
        print(f"{n} x {B} rows side by side: median {np.median(ts):.4f} ms per step of the group, min {min(ts):.4f}  "
              f"({n * B} rows per step; {roof_ms / np.median(ts) * 100:.1f} % of 8 TB/s on the bytes the group streams)", flush=True)
        return
    if a.cus:
        e0, e1 = C.c_void_p(), C.c_void_p()
        L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
        for n in [int(x) for x in a.cus.split(",")]:
            ms_ = C.c_void_p()
            L.kr_stream_create_cu_mask(C.byref(ms_), n)
            for spec, eng in engines:
                ts = []
                for r in range(a.rounds + 1):
                    reset(eng)
                    L.kr_event_record(e0, ms_)
                    for _ in range(a.steps // per_graph[spec]):
                        L.kr_graph_launch(graphs[spec], ms_)
                    L.kr_event_record(e1, ms_)
                    L.kr_event_synchronize(e1)
                    ms = C.c_float()
                    L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
                    if r:
                        ts.append(ms.value / a.steps)
                print(f"{spec:30s} on {n:3d} CUs: median {np.median(ts):.4f} ms/step  min {min(ts):.4f}", flush=True)
            L.kr_stream_destroy(ms_)
        return
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
    for ctx in a.ctx_list:
        times = {spec: [] for spec, _ in engines}
        for r in range(a.rounds + 1):
            for spec, eng in engines:
                reset(eng, ctx)
                L.kr_event_record(e0, eng.s)
                for _ in range(a.steps // per_graph[spec]):
                    L.kr_graph_launch(graphs[spec], eng.s)
                L.kr_event_record(e1, eng.s)
                L.kr_event_synchronize(e1)
                ms = C.c_float()
                L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
                if r:                                  # round 0 warms up
                    times[spec].append(ms.value / a.steps)
        for spec, eng in engines:
            kvb = cfg.text.kv_bytes_per_token // (2 if eng.kv8 else 1)       # the bytes THIS variant's step streams
            roof_ms = (cfg.decoder_weight_bytes(a.weights) + B * (ctx + a.steps / 2) * kvb) / 8e12 * 1e3
            t = np.asarray(times[spec])
            print(f"{spec:50s} ctx {ctx:5d} median {np.median(t):.4f} ms/step  min {t.min():.4f}  max {t.max():.4f}  "
                  f"({roof_ms / np.median(t) * 100:.1f} % of the 8 TB/s step roofline)", flush=True)


def chains(a, engines, reset):
    """Per-launch time of single kinds of decode launches (see --chain)."""
    from karanta_ocr_amd._lib import DEC_OUT_XP, DEC_OUT_XP16, DEC_PLAIN, DEC_ROPE_KV, DEC_SILU8, ptr
    L = lib()
    B = a.batch
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
    for spec, eng in engines:
        t, w = eng.cfg.text, eng.w
        H, KVH, hd = t.num_heads, t.num_kv_heads, t.head_dim

        def one(kind, i, eng=eng, t=t, w=w, H=H, KVH=KVH, hd=hd):      # bound now: called after the loop has moved on
            p = f"llm.{i}."
            xp16 = B <= 16 and eng.narrow_xp     # merge, o, gateup, down: the packed x operands of the product step (`narrow_xp=0`: row-major)
            xpkw = {"x_packed": True} if xp16 else {}
            kc, vc = ptr(eng.kv.kcache[i]), ptr(eng.kv.vtcache[i])
            cache = eng.kv.qkv(i)           # the product's qkv launches: the cache as the engine's own step hands it over
            if kind == "qkv":
                eng._dec_narrow(DEC_ROPE_KV, eng.d_x, w.view(p + "qkv.w"), B, bias=w.view(p + "qkv.b"), norm_w=w.view(p + "ln1.w"),
                                part_in=eng.d_part, x_out=eng.d_x2, **cache, **eng._w8kw(p + "qkv.w"))
            elif kind == "qkv0":                   # no pending slabs: the prologue reads x only
                eng._dec_narrow(DEC_ROPE_KV, eng.d_x, w.view(p + "qkv.w"), B, bias=w.view(p + "qkv.b"), norm_w=w.view(p + "ln1.w"),
                                **cache, **eng._w8kw(p + "qkv.w"))
            elif kind.startswith("down") and len(kind) > 4 and not kind.startswith("down32"):      # down<ksplit>[w<waves>]: e.g. down3, down4w8
                import re
                m = re.fullmatch(r"down(\d)(?:w(\d+))?", kind)
                ks, wv = int(m.group(1)), int(m.group(2) or 16)
                if not hasattr(eng, "_slabs_x"):
                    eng._slabs_x = torch.zeros(8, eng.B, t.hidden_size, dtype=torch.float32, device=eng.device)
                eng._dec_narrow(DEC_PLAIN, eng.d_act, w.view(p + "down.w"), B, out_f32=eng._slabs_x, waves=wv, ksplit=ks,
                                **eng._w8kw(p + "down.w"))
            elif kind in ("resnorm", "resnorm32"):
                args = (ptr(eng.d_x), eng.d_x.stride(0), ptr(eng.d_part[:1]), 1, B, ptr(eng.d_x2), eng.d_x2.stride(0), ptr(w.view(p + "ln1.w")),
                        t.rms_norm_eps, ptr(eng.d_h))
                if kind == "resnorm32":
                    L.kr_decode_resnorm32(*args, B, t.hidden_size, 0, eng.s)
                else:
                    L.kr_decode_resnorm(*args, eng.d_h.stride(0), B, t.hidden_size, eng.s)
            elif kind == "qkvd":
                eng._dec_narrow(DEC_ROPE_KV, eng.d_h, w.view(p + "qkv.w"), B, bias=w.view(p + "qkv.b"), kc=kc, vc=vc, **eng._w8kw(p + "qkv.w"))
            elif kind == "qkv32":
                eng._dec32(DEC_ROPE_KV, eng.d_h, w.view(p + "qkv.w"), B, 8, bias=w.view(p + "qkv.b"), **cache, **eng._w8kw(p + "qkv.w"))
            elif kind == "merge32":
                L.kr_attn_decode_merge32(ptr(eng.d_ws), ptr(eng.d_o), B, H, hd, eng.n_split, eng.s)
            elif kind in ("o32", "o32t1", "o32t2"):
                eng._dec32(DEC_PLAIN, eng.d_o, w.view(p + "o.w"), B, eng.o_waves, out=eng.d_x, res=eng.d_x,
                           tiles_per_wg={"o32": 0, "o32t1": 1, "o32t2": 2}[kind], **eng._w8kw(p + "o.w"))
            elif kind == "gateupxp":
                eng._dec_wide(DEC_SILU8 | DEC_OUT_XP, eng.d_x, w.view(p + "gate_up.w"), B, out=eng.d_act, norm_w=w.view(p + "ln2.w"),
                              **eng._w8kw(p + "gate_up.w"))
            elif kind in ("down32", "down32t1", "down32t2"):
                eng._dec32(DEC_PLAIN, eng.d_act, w.view(p + "down.w"), B, eng.down_waves_small, ksplit=2, out_f32=eng.d_part,
                           tiles_per_wg={"down32": 0, "down32t1": 1, "down32t2": 2}[kind], **eng._w8kw(p + "down.w"))
            elif kind in ("down32a", "down32gs", "down32gs2", "down32gs4"):   # atomic slab(s): the product form / group split
                gs = kind != "down32a"
                acc = eng.d_part.view(-1)[: 2 * B * t.hidden_size].view(2, B, t.hidden_size)
                eng._dec32(DEC_PLAIN, eng.d_act, w.view(p + "down.w"), B, eng.down_waves_small, ksplit=2, out_f32=acc if gs else acc[0],
                           atomic_out=True, group_split=gs, tiles_per_wg={"down32a": 0, "down32gs": 0, "down32gs2": 2, "down32gs4": 4}[kind],
                           **({} if gs else eng._w8kw(p + "down.w")))
            elif kind == "attn" and eng.kv8:
                eng.kv.attention(i, B)
            elif kind == "attn":
                L.kr_attn_decode_fused(ptr(eng.d_q), kc, vc, ptr(eng.d_ctx), 0, ptr(eng.d_ws), 0, B, H, KVH, hd, eng.s_max, eng.n_split,
                                       hd ** -0.5, eng.s)
            elif kind == "merge" and xp16:
                L.kr_attn_decode_merge16(ptr(eng.d_ws), ptr(eng.d_o_xp), B, H, hd, eng.n_split, eng.s)
            elif kind == "merge":
                L.kr_attn_decode_merge(ptr(eng.d_ws), ptr(eng.d_o), B, H, hd, eng.n_split, eng.s)
            elif kind == "o":
                eng._dec_narrow(DEC_PLAIN, eng.d_o_xp if xp16 else eng.d_o, w.view(p + "o.w"), B, out=eng.d_x, res=eng.d_x, waves=8, **xpkw,
                                **eng._w8kw(p + "o.w"))
            elif "+" in kind:                      # a group of launches per layer, e.g. attn+merge+o
                for k in kind.split("+"):
                    eng._one(k, i)
            elif kind == "oheads":
                w8o, sco = eng._w8(p + "o.w")
                L.kr_oproj_heads(ptr(eng.d_ws), eng.n_split, ptr(w8o if w8o is not None else w.view(p + "o.w")), ptr(sco),
                                 ptr(eng.d_xacc), eng.d_xacc.stride(0), B, t.hidden_size, H, eng.s)
            elif kind == "gateup":
                eng._dec_wide(DEC_SILU8 | (DEC_OUT_XP16 if xp16 else 0), eng.d_x, w.view(p + "gate_up.w"), B,
                              out=eng.d_act_xp if xp16 else eng.d_act, norm_w=w.view(p + "ln2.w"), **eng._w8kw(p + "gate_up.w"))
            elif kind == "gateup32":
                eng._dec_wide(DEC_SILU8, None, w.view(p + "gate_up.w"), B, out=eng.d_act, norm_w=w.view(p + "ln2.w"), x_f32=eng.d_xacc,
                              x_out=eng.d_x, **eng._w8kw(p + "gate_up.w"))
            elif kind == "down":
                eng._dec_narrow(DEC_PLAIN, eng.d_act_xp if xp16 else eng.d_act, w.view(p + "down.w"), B, out_f32=eng.d_part,
                                waves=eng.down_waves_small if B <= 16 else 8, ksplit=2, **xpkw, **eng._w8kw(p + "down.w"))
            else:
                raise SystemExit(f"unknown chain kind {kind}")

        eng._one = one
    # every (variant, kind) captured first, then timed in interleaved rounds: round r runs every variant once, so a drift of the
    # machine hits them alike; per launch group: median, min and max over the rounds
    reps = 4
    graphs = {}
    for spec, eng in engines:
        reset(eng)
        nl = eng.cfg.text.num_layers
        for kind in a.chain.split(","):
            with spec_env(spec), torch.cuda.stream(eng.stream):
                for i in range(nl):
                    eng._one(kind, i)                      # eager once (function attributes)
                eng.stream.synchronize()
                g = C.c_void_p()
                L.kr_graph_begin_capture(eng.s)
                try:
                    for _ in range(reps):
                        for i in range(nl):
                            eng._one(kind, i)
                finally:
                    L.kr_graph_end_capture(eng.s, C.byref(g))
                graphs[(spec, kind)] = g
    for ctx in a.ctx_list:         # a chain launch does not move the context: one reset per context
        for spec, eng in engines:
            reset(eng, ctx)
        times = {k: [] for k in graphs}
        for r in range(a.rounds + 1):
            for kind in a.chain.split(","):
                for spec, eng in engines:
                    L.kr_event_record(e0, eng.s)
                    L.kr_graph_launch(graphs[(spec, kind)], eng.s)
                    L.kr_event_record(e1, eng.s)
                    L.kr_event_synchronize(e1)
                    ms = C.c_float()
                    L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
                    if r:                                      # round 0 warms up
                        times[(spec, kind)].append(ms.value * 1e3 / (reps * eng.cfg.text.num_layers))
        for (spec, kind), g in graphs.items():
            t = np.asarray(times[(spec, kind)])
            eng = dict(engines)[spec]
            extra = ""
            if "attn" in kind.split("+"):      # the K / V bytes of the launch over its median time
                kvb = eng.cfg.text.kv_bytes_per_token // eng.cfg.text.num_layers // (2 if eng.kv8 else 1)
                extra = f"  {B * (ctx + 1) * kvb / 1e6:6.1f} MB of K/V: {B * (ctx + 1) * kvb / np.median(t) / 1e6:.2f} TB/s"
            print(f"{spec:30s} ctx {ctx:5d} chain {kind:16s} median {np.median(t):8.2f} us per launch group  min {t.min():8.2f}  max {t.max():8.2f}{extra}",
                  flush=True)
    for g in graphs.values():
        L.kr_graph_destroy(g)

if __name__ == "__main__":
    main()
