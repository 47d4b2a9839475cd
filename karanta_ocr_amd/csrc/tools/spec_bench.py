"""What a speculative decode step costs and what it buys, measured once on the GPU; writes profiles/r05_spec_decode.json (DESIGN.md
section 5j cites it, scheduler.SPEC_BREAK_EVEN is set from it).

    python karanta_ocr_amd/csrc/tools/spec_bench.py [--parent-tree DIR] [--out profiles/r05_spec_decode.json]

Random weights (timing only), context about 1900, graphs replayed as the engine replays them.

  * plain step: the 8-row and the 32-row plain step of the 2B decoder on this tree — and, with --parent-tree (a checkout of the parent
    commit with its library built), on the parent, in alternating child processes; the two must agree within the spread of this
    tree against itself in the same call;
  * ratio: t_spec / t_plain at the 2B decoder with 8 slots x K = 3 and at the 7B decoder with 4 slots x K = 3;
  * tokens/s at scripted acceptance of 0 .. 3 drafts per step (the scripts are the plain run's own continuation, made wrong where a
    run is to stop), against the plain steps' tokens/s;
  * the attention launches' share of the speculative step (every row of a slot reads the slot's K/V again).

    python karanta_ocr_amd/csrc/tools/spec_bench.py --shared [--parent-tree DIR] [--out profiles/r06_spec_shared_rows.json]

  * --shared: the leg for SpecConfig(share_rows=True) above 16 slots, where the plain step is already the 32-row family: 24 slots x
    K = 3 (8 spare rows per step) at the 2B decoder against the plain 24-row step of the PARENT commit (--parent-tree; without it
    this tree's own plain step stands in and the file says so), in alternating child processes; t_spec / t_plain and
    break_even_accepted_per_slot_step, at full acceptance and with every first draft wrong.

    python karanta_ocr_amd/csrc/tools/spec_bench.py --guided [--parent-tree DIR] [--out profiles/r07_spec_guided.json]

  * --guided: the leg for SpecConfig(guided=True): 8 slots x K = 3 at the 2B decoder, every slot under a guide that forbids half of the
    vocabulary, scripted full-acceptance drafts; the guided speculative step (three launches more: kr_spec_guide_trim / _rows /
    _advance) over the guided plain step of the PARENT commit (--parent-tree; without it this tree's own guided plain step stands in
    and the file says so), in alternating child processes, and the same engine's unguided pair beside it.

    python karanta_ocr_amd/csrc/tools/spec_bench.py --controls [--parent-tree DIR] [--out profiles/r08_spec_controls.json]

  * --controls: the leg for SpecConfig(controls=True): the 2B decoder with 8 slots x K = 3 and with 24 slots on shared rows, every slot
    with top_p and a repetition penalty, scripted full-acceptance drafts.  Per layout, in alternating child processes on this tree and
    (--parent-tree) on the parent commit: the controlled plain step, the uncontrolled plain step and the uncontrolled speculative
    step — the legs the parent can run; then, on this tree, the controlled speculative step (kr_spec_controls_trim / _rows / _count
    and the three row-mapped logit passes) with t_spec / t_plain for controlled steps and its break-even.

    python karanta_ocr_amd/csrc/tools/spec_bench.py --logprobs [--out profiles/r10_spec_logprobs.json]

  * --logprobs: the leg for SpecConfig(logprobs=True): the 2B decoder with 8 slots x K = 3 and with 24 slots on shared rows, every slot
    sampling at one temperature, k = 5 records, scripted full-acceptance drafts.  Per layout one engine runs four graphs in turn, twice
    over: the plain and the speculative step without records, then both with them (kr_logprobs_topk; kr_spec_mark and
    kr_logprobs_topk_rows).  Reported: the speculative step with records over the same step without them, and over the plain step
    with records, whose excess over 1 is the break-even acceptance of a server that records.

Every measurement is a child process under a time limit of its own; a child that fails ends the run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
CTX, STEPS, ROUNDS = 1900, 48, 5


GUIDE = r"[a-z]+"


def _token_bytes(i: int) -> bytes:
    """A synthetic token table for the guided leg: even ids spell lower-case letters (GUIDE allows them in every state), odd ids
    digits (it never does) — the mask is half set."""
    base = 97 if i % 2 == 0 else 48
    return bytes(base + (i // 10 ** p) % 10 for p in range(3))


def _engine(model, B, spec_k=0, share=False, guided=False, controls=False, logprobs=False):
    import torch
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.engine import Engine
    kw = {}
    if spec_k:
        from karanta_ocr_amd.engine import SpecConfig
        kw["speculative"] = (SpecConfig(spec_k, share_rows=share, logprobs=True) if logprobs
                             else SpecConfig(spec_k, share_rows=share, controls=True) if controls
                             else SpecConfig(spec_k, share_rows=share, guided=True) if guided
                             else SpecConfig(spec_k, share_rows=True) if share else SpecConfig(spec_k))
    n_new = STEPS * (ROUNDS + 3) * (spec_k + 1) + 16
    eng = Engine(CONFIGS[model], max_batch=B, s_max=(CTX + n_new + 128) // 64 * 64, max_patches=64, max_prompt_tokens=64, **kw)
    eng.w.allocate()
    n = eng.w.arena.numel() // 2
    view = eng.w.arena[: 2 * n].view(torch.bfloat16)
    for i in range(0, n, 1 << 26):
        m = min(1 << 26, n - i)
        view[i:i + m] = (torch.randn(m, device=eng.device) * 0.02).to(torch.bfloat16)
    # the state of a server's decode steps without the chance of an EOS: frozen-slot semantics, EOS ignored
    eng._enter_mode(n_new, ignore_eos=True, freeze_finished=True, want_logits=False, caps=eng._caps, step=eng._step, logprobs=None)
    eng._x0 = (torch.randn(B, eng.cfg.text.hidden_size, device=eng.device) * 0.5).to(torch.bfloat16)
    eng._guide = None
    return eng


def _guide_slots(eng, on=True):
    """Every slot under GUIDE (compiled once), or none: the steps carry the masked Gumbel pass and the DFA advance, or neither."""
    from karanta_ocr_amd.sampling import StepFeatures
    B, sm = eng.B, eng.sampler
    if on and eng._guide is None:
        V = eng.cfg.text.vocab_size
        table = [_token_bytes(i) for i in range(V)]
        for e in eng.cfg.eos_token_ids:
            table[int(e)] = b""
        eng.set_vocab(table)
        eng._guide = eng.compile_guide(GUIDE)
    eng.stream.synchronize()
    eng._caps = eng._step = StepFeatures(True, True, False, False) if on else StepFeatures()
    sm.d_gtrans[:B].fill_(eng._guide.trans.data_ptr() if on else 0)
    sm.d_gmasks[:B].fill_(eng._guide.masks.data_ptr() if on else 0)
    _reset(eng)


TOP_P, REPETITION, TEMPERATURE = 0.9, 1.2, 0.8        # --controls: every slot's request


def _control_slots(eng, on=True):
    """Every slot with TOP_P and REPETITION at TEMPERATURE over a prompt bit set that holds every seventh token, or (off) the same
    temperature without controls: the steps carry the Gumbel pass and, on, the threshold pass, the penalised argmax and the counts."""
    import numpy as np
    import torch
    from karanta_ocr_amd.sampling import StepFeatures
    B, sm, V = eng.B, eng.sampler, eng.cfg.text.vocab_size
    eng.stream.synchronize()
    eng._caps = eng._step = StepFeatures(True, False, bool(on), False)
    row = np.asarray([0, TOP_P, 0, REPETITION, 0, 0, 0, 0] if on else [0, 1, 0, 1, 0, 0, 0, 0], np.float32)
    sm.d_sp[:B].copy_(torch.from_numpy(np.tile(row, (B, 1))).to(eng.device))
    bits = np.zeros(sm.bits_words, np.uint32)
    ids = np.arange(0, V, 7)
    np.bitwise_or.at(bits, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    sm.d_pbits[:B].copy_(torch.from_numpy(np.tile(bits.view(np.int32), (B, 1))).to(eng.device))
    eng.d_temp[:B].fill_(TEMPERATURE)
    eng.d_seed[:B].copy_(torch.arange(1, B + 1, dtype=torch.int32, device=eng.device))
    eng._controls = bool(on)
    _reset(eng)


def _reset(eng):
    import torch
    with torch.cuda.stream(eng.stream):
        eng.d_ctx.fill_(CTX)
        eng.d_plen.fill_(CTX)
        eng.d_fin.zero_()
        eng.d_x[:eng.B].copy_(eng._x0)
        if getattr(eng, "_controls", False):       # the output counts start from an empty output, as the recorded continuation did
            eng.sampler.d_counts.zero_()
        if getattr(eng, "_guide", None) is not None:
            eng.sampler.d_gstate[:eng.B].fill_(eng._guide.start)
    eng.stream.synchronize()


def _time(eng, graph, steps=STEPS, rounds=ROUNDS, before=None):
    """Per-step milliseconds of `steps` replays, one figure per round (round 0 warms up)."""
    L = eng.L
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
    out = []
    for r in range(rounds + 1):
        _reset(eng)
        if before is not None:
            before()
        L.kr_event_record(e0, eng.s)
        for _ in range(steps):
            L.kr_graph_launch(graph, eng.s)
        L.kr_event_record(e1, eng.s)
        L.kr_event_synchronize(e1)
        ms = C.c_float()
        L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
        if r:
            out.append(ms.value / steps)
    return out


def _plain_graph(eng):
    import torch
    _reset(eng)
    with torch.cuda.stream(eng.stream):
        eng._decode_step_launches(eng.B)
        eng.stream.synchronize()
        return eng._graph_for(eng.B)


def child_plain(model, sizes=(8, 32)):
    """The plain step at 8 and at 32 rows (--shared: at 24): uses nothing the parent commit lacks."""
    import numpy as np
    out = {}
    for B in sizes:
        eng = _engine(model, B)
        ts = _time(eng, _plain_graph(eng))
        out[str(B)] = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "rounds_ms": [round(t, 5) for t in ts]}
        eng.close()
        del eng
    return out


def child_spec(model, B, K, share=False):
    """share: SpecConfig(share_rows=True) — the drafts compete for the rows - B spare rows, so a slot's progress per step is not the
    script's choice alone: only the two ends are run, every first draft wrong (0) and every draft right (K)."""
    import numpy as np
    import torch
    eng = _engine(model, B, K, share)
    L, t = eng.L, eng.cfg.text
    g_plain = _plain_graph(eng)
    t_plain = _time(eng, g_plain)
    # the model's own continuation from the reset state: what a right draft is
    n_truth = STEPS * (K + 1) + K + 4
    _reset(eng)
    for _ in range(n_truth):
        L.kr_graph_launch(g_plain, eng.s)
    eng.stream.synchronize()
    truth = eng.d_hist[:n_truth + 1].cpu().numpy().copy()          # [index, slot]; index 0 is not written from this state
    _reset(eng)
    with torch.cuda.stream(eng.stream):
        eng._spec_step_launches()
        eng.stream.synchronize()
        g_spec = eng._graph_for(eng.B, True)
    out = {"model": model, "slots": B, "K": K, "rows": eng.rows, "share_rows": bool(share), "ctx": CTX,
           "plain_ms": float(np.median(t_plain)), "plain_tokens_per_s": B / float(np.median(t_plain)) * 1e3, "accept": {}}
    for a in ((0, K) if share else range(K + 1)):
        scripts = truth.copy()
        if a < K:      # step s starts at generated index 1 + s * (a + 1): its draft a + 1 is made wrong
            for s in range(STEPS + 2):
                i = 1 + s * (a + 1) + a
                if i < len(scripts):
                    scripts[i] = (scripts[i] + 1) % t.vocab_size
        for b in range(B):
            eng.set_draft_script(b, scripts[:, b])
        count0 = [None]

        def before():
            count0[0] = eng.d_spec_count.cpu().numpy().astype(np.int64).copy()
        ts = _time(eng, g_spec, before=before)
        eng.stream.synchronize()
        d = eng.d_spec_count.cpu().numpy().astype(np.int64) - count0[0]
        gen = (eng.d_ctx.cpu().numpy() + 1 - eng.d_plen.cpu().numpy()).astype(np.int64)
        got = eng.d_hist[:int(gen.min()), :B].cpu().numpy()
        same = bool((got[1:] == truth[1:len(got)]).all())
        med = float(np.median(ts))
        out["accept"][str(a)] = {"spec_ms": med, "min_ms": float(min(ts)), "accepted_per_slot_step": float(d[1].sum()) / (B * STEPS),
                                 "proposed_per_slot_step": float(d[0].sum()) / (B * STEPS),
                                 "tokens_per_s": float((gen - 1).sum()) / (med * STEPS) * 1e3, "tokens_equal_plain": same}
    for b in range(B):
        eng.set_draft_script(b, None)
    spec_ms = float(np.median([v["spec_ms"] for v in out["accept"].values()]))
    out["ratio"] = spec_ms / out["plain_ms"]
    out["break_even_accepted_per_slot_step"] = out["ratio"] - 1
    # the attention launches alone: rows x (K + 1) reads of a slot's K/V against one

    def attn_graph(rows_variant):
        L.kr_graph_begin_capture(eng.s)
        for i in range(t.num_layers):
            if rows_variant:
                eng.kv.attention(i, eng.rows, eng.d_row_slot)
            else:
                eng.kv.attention(i, B)
        g = C.c_void_p()
        L.kr_graph_end_capture(eng.s, C.byref(g))
        return g.value
    # the row state a fully accepted step leaves (all K + 1 rows of every slot live)
    for b in range(B):
        eng.set_draft_script(b, truth[:, b])
    _reset(eng)
    L.kr_graph_launch(g_spec, eng.s)
    eng.stream.synchronize()
    for b in range(B):
        eng.set_draft_script(b, None)

    def keep_rows():
        pass
    for name, rv in (("attn_rows_ms", True), ("attn_slots_ms", False)):
        g = attn_graph(rv)
        e0, e1 = C.c_void_p(), C.c_void_p()
        L.kr_event_create(C.byref(e0)); L.kr_event_create(C.byref(e1))
        ts = []
        for r in range(ROUNDS + 1):
            L.kr_event_record(e0, eng.s)
            for _ in range(STEPS):
                L.kr_graph_launch(g, eng.s)
            L.kr_event_record(e1, eng.s)
            L.kr_event_synchronize(e1)
            ms = C.c_float()
            L.kr_event_elapsed_ms(e0, e1, C.byref(ms))
            if r:
                ts.append(ms.value / STEPS)
        out[name] = float(np.median(ts))
    out["attn_share_of_spec_step"] = out["attn_rows_ms"] / out["accept"][str(K)]["spec_ms"]
    out["attn_share_of_plain_step"] = out["attn_slots_ms"] / out["plain_ms"]
    eng.close()
    return out


def _all_allowed(eng, toks) -> bool:
    """Every generated token is one GUIDE allows: an even id, or an EOS id (allowed once the pattern matches; the steps ignore it)."""
    import numpy as np
    return bool(((toks % 2 == 0) | np.isin(toks, list(eng.cfg.eos_token_ids))).all())


def child_guided_plain(model, B):
    """The guided plain step (every slot under GUIDE): uses nothing the parent commit lacks."""
    import numpy as np
    eng = _engine(model, B)
    _guide_slots(eng)
    ts = _time(eng, _plain_graph(eng))
    eng.stream.synchronize()
    gen = eng.d_hist[1:STEPS, :B].cpu().numpy()
    out = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "rounds_ms": [round(t, 5) for t in ts],
           "tokens_all_allowed": _all_allowed(eng, gen)}
    eng.close()
    return out


def _full_acceptance_pair(eng, K):
    """The plain step and the speculative step at scripted full acceptance, with the passes the engine's steps carry now."""
    import numpy as np
    import torch
    L, B = eng.L, eng.B
    g_plain = _plain_graph(eng)
    t_plain = _time(eng, g_plain)
    n_truth = STEPS * (K + 1) + K + 4
    _reset(eng)
    for _ in range(n_truth):
        L.kr_graph_launch(g_plain, eng.s)
    eng.stream.synchronize()
    truth = eng.d_hist[:n_truth + 1].cpu().numpy().copy()
    _reset(eng)
    with torch.cuda.stream(eng.stream):
        eng._spec_step_launches()
        eng.stream.synchronize()
        g_spec = eng._graph_for(B, True)
    for b in range(B):
        eng.set_draft_script(b, truth[:, b])
    count0 = [None]

    def before():
        count0[0] = eng.d_spec_count.cpu().numpy().astype(np.int64).copy()
    ts = _time(eng, g_spec, before=before)
    eng.stream.synchronize()
    d = eng.d_spec_count.cpu().numpy().astype(np.int64) - count0[0]
    gen = (eng.d_ctx.cpu().numpy() + 1 - eng.d_plen.cpu().numpy()).astype(np.int64)
    got = eng.d_hist[:int(gen.min()), :B].cpu().numpy()
    for b in range(B):
        eng.set_draft_script(b, None)
    return {"plain_ms": float(np.median(t_plain)), "spec_ms": float(np.median(ts)), "spec_min_ms": float(min(ts)),
            "ratio": float(np.median(ts)) / float(np.median(t_plain)),
            "accepted_per_slot_step": float(d[1].sum()) / (B * STEPS), "proposed_per_slot_step": float(d[0].sum()) / (B * STEPS),
            "tokens_equal_plain": bool((got[1:] == truth[1:len(got)]).all()), "tokens": truth[1:STEPS]}


def child_guided(model, B, K):
    """SpecConfig(guided=True): the same engine's unguided pair (plain step, speculative step), then the guided pair."""
    eng = _engine(model, B, K, guided=True)
    out = {"model": model, "slots": B, "K": K, "rows": eng.rows, "ctx": CTX, "guide": GUIDE}
    for name, on in (("unguided", False), ("guided", True)):
        _guide_slots(eng, on)
        r = _full_acceptance_pair(eng, K)
        toks = r.pop("tokens")
        if on:
            r["tokens_all_allowed"] = _all_allowed(eng, toks)
        out[name] = r
    eng.close()
    return out


def child_controls_plain(model, B):
    """The uncontrolled and the controlled plain step on an engine without `speculative`: uses nothing the parent commit lacks."""
    import numpy as np
    eng = _engine(model, B)
    out = {}
    for name, on in (("uncontrolled", False), ("controlled", True)):
        _control_slots(eng, on)
        ts = _time(eng, _plain_graph(eng))
        out[name] = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "rounds_ms": [round(t, 5) for t in ts]}
    eng.close()
    return out


def child_pair(model, B, K, share):
    """The uncontrolled plain and speculative steps (temperature alone) at scripted full acceptance on SpecConfig(K[, share_rows]):
    uses nothing the parent commit lacks."""
    eng = _engine(model, B, K, share)
    _control_slots(eng, False)
    r = _full_acceptance_pair(eng, K)
    r.pop("tokens")
    eng.close()
    return r


def child_controls(model, B, K, share):
    """SpecConfig(controls=True): the same engine's uncontrolled pair (plain step, speculative step), then the controlled pair."""
    eng = _engine(model, B, K, share, controls=True)
    out = {"model": model, "slots": B, "K": K, "rows": eng.rows, "share_rows": bool(share), "ctx": CTX, "top_p": TOP_P,
           "repetition_penalty": REPETITION, "temperature": TEMPERATURE}
    for name, on in (("uncontrolled", False), ("controlled", True)):
        _control_slots(eng, on)
        r = _full_acceptance_pair(eng, K)
        r.pop("tokens")
        out[name] = r
    eng.close()
    return out


LOGPROBS_K = 5          # --logprobs: the reference's bulk requests ask for top_logprobs 5


def child_logprobs(model, B, K, share):
    """SpecConfig(logprobs=True): one engine's plain and speculative step at scripted full acceptance, without records and with them,
    the four graphs in turn and the turn twice, so that each figure has a neighbour taken minutes apart on the same process."""
    import numpy as np
    eng = _engine(model, B, K, share, logprobs=True)
    _control_slots(eng, False)
    # the log-probability history is allocated once (no graph exists yet); from here on the switch alone picks the graphs
    eng._enter_mode(eng._req_max_new, ignore_eos=True, freeze_finished=True, want_logits=False, caps=eng._caps, step=eng._step,
                    logprobs=LOGPROBS_K)
    out = {"model": model, "slots": B, "K": K, "rows": eng.rows, "share_rows": bool(share), "ctx": CTX, "top_logprobs": LOGPROBS_K,
           "temperature": TEMPERATURE, "turns": []}
    for _ in range(2):
        turn = {}
        for name, k in (("without_records", None), ("with_records", LOGPROBS_K)):
            eng._logprobs = k
            r = _full_acceptance_pair(eng, K)
            r.pop("tokens")
            turn[name] = r
        out["turns"].append(turn)
    med = lambda name, key: float(np.median([t[name][key] for t in out["turns"]]))
    for name in ("without_records", "with_records"):
        out[name] = {"plain_ms": med(name, "plain_ms"), "spec_ms": med(name, "spec_ms"),
                     "plain_turns_ms": [t[name]["plain_ms"] for t in out["turns"]], "spec_turns_ms": [t[name]["spec_ms"] for t in out["turns"]],
                     "accepted_per_slot_step": med(name, "accepted_per_slot_step"),
                     "tokens_equal_plain": all(t[name]["tokens_equal_plain"] for t in out["turns"])}
    out["spec_with_records_over_spec_without"] = out["with_records"]["spec_ms"] / out["without_records"]["spec_ms"]
    out["plain_with_records_over_plain_without"] = out["with_records"]["plain_ms"] / out["without_records"]["plain_ms"]
    out["t_spec_over_t_plain_with_records"] = out["with_records"]["spec_ms"] / out["with_records"]["plain_ms"]
    out["t_spec_over_t_plain_without_records"] = out["without_records"]["spec_ms"] / out["without_records"]["plain_ms"]
    out["break_even_accepted_per_slot_step_with_records"] = out["t_spec_over_t_plain_with_records"] - 1
    eng.close()
    return out


def run_child(args, tree, limit, sizes=None):
    """This file as a child process with `tree`'s package on the path (the child imports karanta_ocr_amd from its working directory).
    sizes: the plain child's batch sizes, for a tree whose engine this file's --sizes is to drive."""
    env = dict(os.environ, PYTHONPATH=tree)
    if sizes is not None:
        args = [*args, "--sizes", ",".join(str(x) for x in sizes)]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], cwd=tree, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {args} in {tree} ended with {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main_shared(a):
    """24 slots x K = 3 with shared rows against the parent commit's plain 24-row step, alternating child processes."""
    import numpy as np
    B, K = 24, 3
    report = {"context": CTX, "steps_per_round": STEPS, "rounds": ROUNDS, "weights": "random bf16 (timing only)", "slots": B, "K": K}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    runs = {"this": [], "parent": []}
    for _ in range(a.repeats):
        runs["this"].append(run_child(["--child", "plain", "--sizes", str(B)], ROOT, 240)[str(B)]["median_ms"])
        if a.parent_tree:
            runs["parent"].append(run_child(["--child", "plain"], os.path.abspath(a.parent_tree), 240, sizes=(B,))[str(B)]["median_ms"])
    base = runs["parent"] or runs["this"]
    report["plain_step"] = {"this_tree_ms": runs["this"], "parent_ms": runs["parent"], "aa_spread_ms": max(runs["this"]) - min(runs["this"]),
                            "t_plain_from": "parent commit" if runs["parent"] else "THIS tree (no --parent-tree given)",
                            "t_plain_ms": float(np.median(base))}
    save()
    spec = run_child(["--child", "spec", "--model", "Qwen2-VL-2B", "--slots", str(B), "--k", str(K), "--share"], ROOT, 420)
    report["spec"] = spec
    t_spec = float(np.median([v["spec_ms"] for v in spec["accept"].values()]))
    report["t_spec_ms"] = t_spec
    report["t_spec_over_t_plain"] = t_spec / report["plain_step"]["t_plain_ms"]
    report["break_even_accepted_per_slot_step"] = report["t_spec_over_t_plain"] - 1
    save()
    print(json.dumps(report, indent=1))
    return 0


def main_guided(a):
    """8 slots x K = 3, every slot guided, against the parent commit's guided plain step, alternating child processes."""
    import numpy as np
    B, K = 8, 3
    report = {"context": CTX, "steps_per_round": STEPS, "rounds": ROUNDS, "weights": "random bf16 (timing only)", "slots": B, "K": K,
              "guide": GUIDE}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    child = ["--child", "guided-plain", "--slots", str(B)]
    runs = {"this": [], "parent": []}
    for _ in range(a.repeats):
        runs["this"].append(run_child(child, ROOT, 240))
        if a.parent_tree:
            runs["parent"].append(run_child(child, os.path.abspath(a.parent_tree), 240))
    mine, theirs = [r["median_ms"] for r in runs["this"]], [r["median_ms"] for r in runs["parent"]]
    report["guided_plain_step"] = {"this_tree_ms": mine, "parent_ms": theirs, "aa_spread_ms": max(mine) - min(mine),
                                   "t_plain_from": "parent commit" if theirs else "THIS tree (no --parent-tree given)",
                                   "t_plain_ms": float(np.median(theirs or mine)),
                                   "tokens_all_allowed": all(r["tokens_all_allowed"] for r in runs["this"] + runs["parent"])}
    save()
    spec = run_child(["--child", "guided", "--model", "Qwen2-VL-2B", "--slots", str(B), "--k", str(K)], ROOT, 420)
    report["spec"] = spec
    report["t_spec_guided_ms"] = spec["guided"]["spec_ms"]
    report["t_spec_over_t_plain_guided"] = spec["guided"]["spec_ms"] / report["guided_plain_step"]["t_plain_ms"]
    report["break_even_accepted_per_slot_step"] = report["t_spec_over_t_plain_guided"] - 1
    report["t_spec_over_t_plain_unguided_same_engine"] = spec["unguided"]["ratio"]
    report["guided_spec_step_minus_unguided_spec_step_ms"] = spec["guided"]["spec_ms"] - spec["unguided"]["spec_ms"]
    report["guided_plain_step_minus_unguided_plain_step_ms"] = spec["guided"]["plain_ms"] - spec["unguided"]["plain_ms"]
    save()
    print(json.dumps(report, indent=1))
    return 0


def main_controls(a):
    """8 slots x K = 3 and 24 slots on shared rows, every slot with top_p and a repetition penalty; the legs the parent can run on both
    trees in alternating child processes, the controlled speculative step on this tree.  --layouts picks a subset (one call may be
    short of time for both); the report file is read back and extended."""
    import numpy as np
    K = 3
    report = {"context": CTX, "steps_per_round": STEPS, "rounds": ROUNDS, "weights": "random bf16 (timing only)", "K": K, "top_p": TOP_P,
              "repetition_penalty": REPETITION, "temperature": TEMPERATURE, "layouts": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            report = json.load(f)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    for name in a.layouts.split(","):
        B, share = {"8x3": (8, False), "24shared": (24, True)}[name]
        lay = report["layouts"][name] = {"slots": B, "share_rows": share}
        runs = {t: {"plain": [], "pair": []} for t, _ in trees}
        for _ in range(a.repeats):
            for t, tree in trees:
                runs[t]["plain"].append(run_child(["--child", "controls-plain", "--slots", str(B)], tree, 300))
                runs[t]["pair"].append(run_child(["--child", "pair", "--slots", str(B), "--k", str(K)] + (["--share"] if share else []),
                                                 tree, 300))
        legs = {"controlled_plain": lambda r: r["plain"], "uncontrolled_plain": lambda r: r["plain"], "uncontrolled_spec": lambda r: r["pair"]}
        pick = {"controlled_plain": lambda x: x["controlled"]["median_ms"], "uncontrolled_plain": lambda x: x["uncontrolled"]["median_ms"],
                "uncontrolled_spec": lambda x: x["spec_ms"]}
        for leg in legs:
            mine = [pick[leg](x) for x in legs[leg](runs["this"])]
            theirs = [pick[leg](x) for x in legs[leg](runs["parent"])] if a.parent_tree else []
            lay[leg] = {"this_tree_ms": mine, "parent_ms": theirs, "aa_spread_ms": max(mine) - min(mine)}
            if theirs:
                lay[leg]["parent_spread_ms"] = max(theirs) - min(theirs)
                lay[leg]["difference_of_medians_ms"] = float(np.median(mine) - np.median(theirs))
                lay[leg]["within_parent_spread"] = bool(abs(lay[leg]["difference_of_medians_ms"]) <= lay[leg]["parent_spread_ms"])
                lay[leg]["within_this_trees_spread"] = bool(abs(lay[leg]["difference_of_medians_ms"]) <= lay[leg]["aa_spread_ms"])
        lay["tokens_equal_plain_uncontrolled"] = all(x["tokens_equal_plain"] for t, _ in trees for x in runs[t]["pair"])
        save()
        spec = run_child(["--child", "controls", "--slots", str(B), "--k", str(K)] + (["--share"] if share else []), ROOT, 420)
        lay["spec"] = spec
        base = lay["controlled_plain"]["parent_ms"] or lay["controlled_plain"]["this_tree_ms"]
        lay["t_plain_controlled_from"] = "parent commit" if lay["controlled_plain"]["parent_ms"] else "THIS tree (no --parent-tree given)"
        lay["t_plain_controlled_ms"] = float(np.median(base))
        lay["t_spec_controlled_ms"] = spec["controlled"]["spec_ms"]
        lay["t_spec_over_t_plain_controlled"] = spec["controlled"]["spec_ms"] / lay["t_plain_controlled_ms"]
        lay["break_even_accepted_per_slot_step"] = lay["t_spec_over_t_plain_controlled"] - 1
        lay["t_spec_over_t_plain_uncontrolled_same_engine"] = spec["uncontrolled"]["ratio"]
        lay["controlled_spec_step_minus_uncontrolled_spec_step_ms"] = spec["controlled"]["spec_ms"] - spec["uncontrolled"]["spec_ms"]
        lay["controlled_plain_step_minus_uncontrolled_plain_step_ms"] = spec["controlled"]["plain_ms"] - spec["uncontrolled"]["plain_ms"]
        save()
    print(json.dumps(report, indent=1))
    return 0


def main_logprobs(a):
    """8 slots x K = 3 and 24 slots on shared rows, k = 5 records: one child per layout (--layouts picks a subset; the report file is
    read back and extended)."""
    report = {"context": CTX, "steps_per_round": STEPS, "rounds": ROUNDS, "weights": "random bf16 (timing only)", "K": 3,
              "top_logprobs": LOGPROBS_K, "layouts": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            report = json.load(f)
    for name in a.layouts.split(","):
        B, share = {"8x3": (8, False), "24shared": (24, True)}[name]
        report["layouts"][name] = run_child(["--child", "logprobs", "--slots", str(B), "--k", "3"] + (["--share"] if share else []), ROOT, 420)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    print(json.dumps(report, indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--model", default="Qwen2-VL-2B")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-7b", action="store_true")
    ap.add_argument("--shared", action="store_true", help="the shared-rows leg alone: 24 slots x K = 3 (profiles/r06_spec_shared_rows.json)")
    ap.add_argument("--guided", action="store_true", help="the guided leg alone: 8 slots x K = 3, every slot under a guide "
                                                          "(profiles/r07_spec_guided.json)")
    ap.add_argument("--controls", action="store_true", help="the controls leg alone: 8 slots x K = 3 and 24 slots shared, every slot with "
                                                            "top_p and a repetition penalty (profiles/r08_spec_controls.json)")
    ap.add_argument("--logprobs", action="store_true", help="the log-probability leg alone: 8 slots x K = 3 and 24 slots shared, k = 5 "
                                                            "records (profiles/r10_spec_logprobs.json)")
    ap.add_argument("--layouts", default="8x3,24shared", help="(--controls, --logprobs) which of the two layouts to run")
    ap.add_argument("--share", action="store_true", help="(child) SpecConfig(share_rows=True)")
    ap.add_argument("--sizes", default="8,32", help="(child plain) the batch sizes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.getcwd())
        res = (child_plain(a.model, [int(x) for x in a.sizes.split(",")]) if a.child == "plain"
               else child_guided_plain(a.model, a.slots) if a.child == "guided-plain"
               else child_guided(a.model, a.slots, a.k) if a.child == "guided"
               else child_controls_plain(a.model, a.slots) if a.child == "controls-plain"
               else child_pair(a.model, a.slots, a.k, a.share) if a.child == "pair"
               else child_controls(a.model, a.slots, a.k, a.share) if a.child == "controls"
               else child_logprobs(a.model, a.slots, a.k, a.share) if a.child == "logprobs"
               else child_spec(a.model, a.slots, a.k, a.share))
        print(json.dumps(res), flush=True)
        return 0
    import numpy as np
    a.out = a.out or os.path.join(ROOT, "profiles", "r10_spec_logprobs.json" if a.logprobs else "r08_spec_controls.json" if a.controls else "r07_spec_guided.json" if a.guided else
                                  "r06_spec_shared_rows.json" if a.shared else "r05_spec_decode.json")
    if a.logprobs:
        return main_logprobs(a)
    if a.controls:
        return main_controls(a)
    if a.guided:
        return main_guided(a)
    if a.shared:
        return main_shared(a)
    report = {"context": CTX, "steps_per_round": STEPS, "rounds": ROUNDS, "weights": "random bf16 (timing only)"}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    # ---- 1. the plain step on this tree and on the parent, alternating
    runs = {"this": [], "parent": []}
    for i in range(a.repeats):
        runs["this"].append(run_child(["--child", "plain"], ROOT, 240))
        if a.parent_tree:
            runs["parent"].append(run_child(["--child", "plain"], os.path.abspath(a.parent_tree), 240))
    plain = {}
    for B in ("8", "32"):
        mine = [r[B]["median_ms"] for r in runs["this"]]
        theirs = [r[B]["median_ms"] for r in runs["parent"]]
        plain[B] = {"this_tree_ms": mine, "parent_ms": theirs, "aa_spread_ms": max(mine) - min(mine)}
        if theirs:
            plain[B]["difference_of_medians_ms"] = float(np.median(mine) - np.median(theirs))
            plain[B]["within_aa_spread"] = bool(abs(plain[B]["difference_of_medians_ms"]) <= plain[B]["aa_spread_ms"])
    report["plain_step_2B"] = plain
    save()
    # ---- 2.-4. the speculative step
    report["spec_2B"] = run_child(["--child", "spec", "--model", "Qwen2-VL-2B", "--slots", "8", "--k", "3"], ROOT, 420)
    save()
    if not a.skip_7b:
        report["spec_7B"] = run_child(["--child", "spec", "--model", "Qwen2-VL-7B", "--slots", "4", "--k", "3"], ROOT, 420)
        save()
    print(json.dumps(report, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
