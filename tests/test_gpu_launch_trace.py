"""The engine issues the launches it issued when tests/golden/launch_trace.json was recorded: the same entry points in the same
order with the same arguments (tests/launch_trace.py), over whole-batch generation with and without sampling controls and a
guide, slot mode with every kind of admission, the packed 17..32-row family on bf16 and fp8 weights, and speculative steps;
over the same scenarios with the fp8 KV cache (a calibrating admission, pinned scales, the fork, both row maps); and over
speculative steps in both row layouts with guided requests, sampling controls, logit adjustments, log-probabilities and the
repetition pass.
A change that only moves host code leaves every trace as it is; one that adds, drops, reorders or re-parameterises a launch
fails here with the first call that differs.

The fixture is recorded by `python -m tests.test_gpu_launch_trace` on a tree whose launches are the wanted ones (it was made
on the commit before engine.py was split into modules; the fp8-cache keys were added on the commit before the KV cache moved
into kv_cache.py, and the h_ / i_ keys on the commit before the speculative step moved into speculative.py, each time with
every older key unchanged)."""
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.sampling import RepetitionParams, StepFeatures  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402
from tests.launch_trace import canonical, digest, launch_trace, names  # noqa: E402
from tests.test_gpu_engine import GUIDE_PATTERN  # noqa: E402
from tests.test_gpu_parallel_sampling import page_of  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json")
LENGTHS = [40, 64, 100]
_WEIGHTS = {}


def _engine(name, **kw):
    if name not in _WEIGHTS:
        _WEIGHTS[name] = random_weights(CONFIGS[name], 909)
    eng = Engine(CONFIGS[name], s_max=512, max_patches=2048, max_prompt_tokens=4096, decode_splits=2, **kw)
    eng.load_weights(_WEIGHTS[name])
    return eng


def _traced(eng, out, key, fn):
    with launch_trace(eng) as calls:
        fn()
        eng.stream.synchronize()
    out[key] = calls


def _slot_scenario(eng, pages):
    """Slot mode with every kind of admission: a fork, a reused prompt, an overlapped admission."""
    cfg = eng.cfg
    eng.begin_slots(8, sampling=True)
    # two pages, three sequences: the page with n = 2 takes slots 0 and 3
    eng.admit([pages[0], page_of(cfg, 64, variant=1, temperature=0.7, top_k=5, seed=9, n=2)], [2, 0, 3])
    eng.decode_steps(2)
    eng.admit_reuse([page_of(cfg, 40, variant=0, logit_bias={3: 1.0})], [2], [1])
    handle = eng.admit_begin([pages[2]], [3])
    eng.admit_end(handle)
    eng.decode_steps(1)


def group_tiny():
    """a: whole batches on the tiny model, eager; b: the same engine in slot mode."""
    from karanta_ocr_amd.serving import ByteTokenizer
    eng, out = _engine("tiny", max_batch=4), {}
    cfg = eng.cfg
    pages = [page_of(cfg, P, variant=b) for b, P in enumerate(LENGTHS)]
    _traced(eng, out, "a_greedy", lambda: eng.generate(pages, 4, use_graph=False))
    eng.set_vocab(ByteTokenizer(cfg).token_bytes())
    mixed = [pages[0],
             page_of(cfg, 64, variant=1, temperature=0.7, top_k=5, repetition_penalty=1.1, logit_bias={3: 1.0}, logprobs=2, seed=5),
             page_of(cfg, 100, variant=2, guide=GUIDE_PATTERN)]
    _traced(eng, out, "a_controls", lambda: eng.generate(mixed, 4, use_graph=False))
    _traced(eng, out, "b_slots", lambda: _slot_scenario(eng, pages))
    eng.close()
    return out


def _group_rows32(dtype, key="c_", **kw):
    """c: 18 pages at once, the packed 17..32-row decode family."""
    eng, out = _engine("tiny-w512", max_batch=21, weight_dtype=dtype, **kw), {}
    pages = [page_of(eng.cfg, LENGTHS[b % 3], variant=b) for b in range(18)]
    _traced(eng, out, key + dtype, lambda: eng.generate(pages, 3))
    eng.close()
    return out


def group_rows32_bf16():
    return _group_rows32("bf16")


def group_rows32_fp8():
    return _group_rows32("fp8")


def group_spec(key="d_spec", **kw):
    """d: four slots with K = 3 are 16 rows, which run as 17."""
    eng, out = _engine("tiny-w512", max_batch=4, speculative=SpecConfig(3, 2, 4), **kw), {}
    pages = [page_of(eng.cfg, LENGTHS[b % 3], variant=b) for b in range(4)]

    def steps():
        eng.begin_slots(16)
        eng.admit(pages, [0, 1, 2, 3])
        eng.set_draft_script(1, [7, 8, 9, 10, 11, 12, 13, 14])
        eng.decode_steps(2, speculative=True)
        eng.decode_steps(1)
    _traced(eng, out, key, steps)
    eng.close()
    return out


def group_kv8_tiny():
    """e: the fp8 KV cache on the tiny model.  The first admission calculates the scales (kr_kv_absmax before kr_kv_quantize in
    every layer), then the slot scenario of b, whose fork is kr_kv_fork8; a second engine with a table set by hand calculates
    nothing."""
    eng, out = _engine("tiny", max_batch=4, kv_cache_dtype="fp8", calculate_kv_scales=True), {}
    t = eng.cfg.text
    pages = [page_of(eng.cfg, P, variant=b) for b, P in enumerate(LENGTHS)]
    _traced(eng, out, "e_kv8_calibrate", lambda: eng.generate(pages, 4, use_graph=False))
    _traced(eng, out, "e_kv8_slots", lambda: _slot_scenario(eng, pages))
    eng.close()
    eng = _engine("tiny", max_batch=4, kv_cache_dtype="fp8", calculate_kv_scales=True)
    heads = np.arange(t.num_layers * t.num_kv_heads, dtype=np.float32).reshape(t.num_layers, t.num_kv_heads)
    eng.set_kv_scales(0.5 + heads / 8, 0.25 + heads / 16)
    _traced(eng, out, "e_kv8_pinned", lambda: eng.generate(pages, 4, use_graph=False))
    assert "kr_kv_absmax" not in names(out["e_kv8_pinned"]) and "kr_kv_absmax" in names(out["e_kv8_calibrate"])
    eng.close()
    return out


def group_kv8_rows32_bf16():
    """f: the packed family appending to and reading the fp8 cache, without a row map."""
    return _group_rows32("bf16", key="f_kv8_rows32_", kv_cache_dtype="fp8")


def group_kv8_rows32_fp8():
    return _group_rows32("fp8", key="f_kv8_rows32_", kv_cache_dtype="fp8")


def group_kv8_spec():
    """g: the speculative steps of d on the fp8 cache: the row map in the qkv launch and in the attention."""
    return group_spec(key="g_kv8_spec", kv_cache_dtype="fp8")


SPEC_FULL = ("kr_spec_guide_trim", "kr_spec_guide_rows", "kr_spec_guide_advance", "kr_spec_controls_trim", "kr_spec_controls_rows",
             "kr_spec_controls_count", "kr_logits_adjust_rows", "kr_sample_threshold_rows", "kr_gumbel_argmax_processed_rows",
             "kr_logits_restore_rows", "kr_logprobs_topk_rows")
ALL_PASSES = StepFeatures(True, True, True, True, True)


def _full_pages(cfg):
    """One page per feature of a speculative step: greedy, controls + adjustments, a guide, stop entries + repetition."""
    return [page_of(cfg, 40, variant=0),
            page_of(cfg, 64, variant=1, temperature=0.7, top_k=5, repetition_penalty=1.1, logit_bias={3: 1.0}, seed=5),
            page_of(cfg, 100, variant=2, guide=GUIDE_PATTERN),
            page_of(cfg, 40, variant=3, min_tokens=2, stop_token_ids=(7, 9), repetition=RepetitionParams(8, 2, 5))]


def _spec_engine(max_batch, **options):
    from karanta_ocr_amd.serving import ByteTokenizer
    eng = _engine("tiny-w512", max_batch=max_batch, speculative=SpecConfig(3, 2, 4, **options))
    eng.set_vocab(ByteTokenizer(eng.cfg).token_bytes())
    return eng


def _spec_steps(eng, pages, **mode):
    """The calls of group_spec: one admission, a scripted slot, two speculative steps (eager, then the captured graph) and a
    plain one.  Returns the step features the admission left."""
    eng.begin_slots(16, **mode)
    eng.admit(pages, list(range(len(pages))))
    eng.set_draft_script(1, [7, 8, 9, 10, 11, 12, 13, 14])
    step = eng._step
    eng.decode_steps(2, speculative=True)
    eng.decode_steps(1)
    return step


def _assert_full(calls, step):
    """Every pass on: the eleven launches only such a step issues, and the repetition pass last in each speculative step."""
    got = names(calls)
    assert step == ALL_PASSES, step
    assert not set(SPEC_FULL) - set(got), sorted(set(SPEC_FULL) - set(got))
    ends = [got[i + 1] for i, n in enumerate(got) if n == "kr_spec_guide_advance"]
    assert len(ends) == 2 and set(ends) == {"kr_repeat_detect"}, ends     # the eager step and the captured one


def group_spec_full():
    """h: the static layout with every option on.  h_spec_full: all five passes; h_spec_mark: a recording step without a trim."""
    eng, out, seen = _spec_engine(4, guided=True, controls=True, logprobs=True), {}, {}
    _traced(eng, out, "h_spec_full",
            lambda: seen.update(step=_spec_steps(eng, _full_pages(eng.cfg), sampling=True, guided=True, logprobs=2)))
    _assert_full(out["h_spec_full"], seen["step"])
    assert "kr_spec_propose" in names(out["h_spec_full"]) and "kr_spec_mark" not in names(out["h_spec_full"])
    warm = [page_of(eng.cfg, LENGTHS[b % 3], variant=b, temperature=0.7, seed=b) for b in range(4)]
    _traced(eng, out, "h_spec_mark", lambda: _spec_steps(eng, warm, sampling=True, logprobs=2))
    spec = [n for n in names(out["h_spec_mark"]) if n.startswith("kr_spec_")]
    assert spec[:2] == ["kr_spec_mark", "kr_spec_propose"] and not any("trim" in n for n in spec), spec
    assert "kr_logprobs_topk_rows" in names(out["h_spec_mark"]) and "kr_logits_restore_rows" not in names(out["h_spec_mark"])
    eng.close()
    return out


def group_spec_shared():
    """i: the dealt layout (nine slots, 32 rows).  i_spec_shared: greedy pages; i_spec_shared_full: every option on — the trims
    write d_nwant and the row-mapped launches take d_draft_row."""
    eng, out, seen = _spec_engine(9, share_rows=True), {}, {}
    greedy = [page_of(eng.cfg, LENGTHS[b % 3], variant=b) for b in range(9)]
    _traced(eng, out, "i_spec_shared", lambda: _spec_steps(eng, greedy))
    got = names(out["i_spec_shared"])
    assert {"kr_spec_lookup", "kr_spec_deal", "kr_spec_accept_rows"} <= set(got) and "kr_spec_propose" not in got
    eng.close()
    eng = _spec_engine(9, share_rows=True, guided=True, controls=True, logprobs=True)
    pages = _full_pages(eng.cfg) + greedy[4:]
    _traced(eng, out, "i_spec_shared_full",
            lambda: seen.update(step=_spec_steps(eng, pages, sampling=True, guided=True, logprobs=2)))
    _assert_full(out["i_spec_shared_full"], seen["step"])
    got = names(out["i_spec_shared_full"])
    assert {"kr_spec_lookup", "kr_spec_deal", "kr_spec_accept_rows"} <= set(got) and "kr_spec_propose" not in got
    eng.close()
    return out


GROUPS = {"tiny": group_tiny, "rows32_bf16": group_rows32_bf16, "rows32_fp8": group_rows32_fp8, "spec": group_spec,
          "kv8_tiny": group_kv8_tiny, "kv8_rows32_bf16": group_kv8_rows32_bf16, "kv8_rows32_fp8": group_kv8_rows32_fp8,
          "kv8_spec": group_kv8_spec, "spec_full": group_spec_full, "spec_shared": group_spec_shared}


def _arg_digests(calls):
    return [hashlib.sha256(canonical(c).encode()).hexdigest()[:12] for c in calls]


def summary(calls):
    return {"names": names(calls), "sha256": digest(calls), "arg_digests": _arg_digests(calls)}


@pytest.mark.parametrize("group", list(GROUPS))
def test_launches_equal_the_recorded_trace(group, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(FIXTURE) as f:
        want = json.load(f)
    got = GROUPS[group]()
    assert got, group
    for key, calls in got.items():
        ref, mine = want[key], summary(calls)
        if mine["sha256"] == ref["sha256"]:
            continue
        path = tmp_path / f"{key}.json"
        path.write_text(json.dumps(calls, indent=0))
        for i, (a, b) in enumerate(zip(mine["names"], ref["names"])):
            assert a == b, f"{key}: call {i} is {a}, recorded {b} (full trace: {path})"
        assert len(mine["names"]) == len(ref["names"]), (f"{key}: {len(mine['names'])} calls, recorded {len(ref['names'])}; the "
                                                         f"first {min(len(mine['names']), len(ref['names']))} have the same names "
                                                         f"(full trace: {path})")
        for i, (a, b) in enumerate(zip(mine["arg_digests"], ref["arg_digests"])):
            assert a == b, f"{key}: call {i} ({mine['names'][i]}) has other arguments than recorded: {calls[i][1]} (full trace: {path})"
        raise AssertionError(f"{key}: trace digest differs (full trace: {path})")


if __name__ == "__main__":
    import sys
    recorded = {}
    for make in GROUPS.values():
        for key, calls in make().items():
            recorded[key] = summary(calls)
            print(f"{key}: {len(calls)} calls, sha256 {recorded[key]['sha256']}")
    dst = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(dst, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
