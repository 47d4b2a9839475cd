"""device_weights.plan_resident: which (layer, kind) weights a decode step keeps in the Infinity Cache under a byte budget."""
import itertools

import pytest

from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.device_weights import narrow_weight_bytes, plan_resident

GAINS = [("o", 0.2), ("qkv", 0.3), ("down", 0.05)]


def used(sizes, plan):
    return sum(sizes[layer][kind] for layer, kind in plan)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("name", ["Qwen2-VL-2B", "Qwen2-VL-7B", "tiny"])
def test_never_exceeds_the_budget(name, dtype):
    sizes = narrow_weight_bytes(CONFIGS[name], dtype)
    total = sum(sum(s.values()) for s in sizes)
    for budget in (0, 1, sizes[0]["o"] - 1, sizes[0]["o"], 64 * 10 ** 6, 240 * 10 ** 6, total - 1, total, 2 * total):
        plan = plan_resident(sizes, GAINS, budget)
        assert used(sizes, plan) <= budget
        assert all(0 <= layer < len(sizes) and kind in sizes[layer] for layer, kind in plan)
    assert len(plan_resident(sizes, GAINS, total)) == 3 * len(sizes)


def test_nothing_at_budget_zero_and_nothing_without_a_gain():
    sizes = narrow_weight_bytes(CONFIGS["Qwen2-VL-2B"])
    assert plan_resident(sizes, GAINS, 0) == frozenset()
    assert plan_resident(sizes, [], 10 ** 12) == frozenset()
    assert plan_resident(sizes, [("qkv", 0.0), ("o", -1.0)], 10 ** 12) == frozenset()
    assert {k for _, k in plan_resident(sizes, [("qkv", 0.3), ("down", 0.0)], 10 ** 12)} == {"qkv"}


def test_deterministic_whatever_the_order_of_the_gains():
    sizes = narrow_weight_bytes(CONFIGS["Qwen2-VL-2B"])
    plans = {plan_resident(sizes, list(p), 240 * 10 ** 6) for p in itertools.permutations(GAINS)}
    plans.add(plan_resident(sizes, GAINS, 240 * 10 ** 6))
    assert len(plans) == 1
    tie = [("o", 0.3), ("qkv", 0.3)]
    assert plan_resident(sizes, tie, 5 * 10 ** 6) == plan_resident(sizes, tie[::-1], 5 * 10 ** 6) == frozenset({(0, "o")})


def test_orders_by_gain_per_byte():
    """2B at 240 MB: qkv (highest gain per MB) in all 28 layers = 176 MB, then o_proj in as many of the first layers as fit (13),
    down_proj (27.5 MB a layer) not at all; with the gains swapped o_proj comes first."""
    sizes = narrow_weight_bytes(CONFIGS["Qwen2-VL-2B"])
    assert sizes[0] == {"qkv": 2048 * 1536 * 2, "o": 1536 * 1536 * 2, "down": 1536 * 8960 * 2}
    plan = plan_resident(sizes, GAINS, 240 * 10 ** 6)
    assert {layer for layer, k in plan if k == "qkv"} == set(range(28))
    assert {layer for layer, k in plan if k == "o"} == set(range(13))
    assert not [1 for _, k in plan if k == "down"]
    swapped = plan_resident(sizes, [("o", 0.3), ("qkv", 0.2)], 150 * 10 ** 6)
    assert {layer for layer, k in swapped if k == "o"} == set(range(28))
    assert {layer for layer, k in swapped if k == "qkv"} == set(range((150 * 10 ** 6 - 28 * sizes[0]["o"]) // sizes[0]["qkv"]))
    # a weight that does not fit is passed over, a smaller one of a lesser kind behind it still goes in
    small = plan_resident(sizes, GAINS, sizes[0]["o"])
    assert small == frozenset({(0, "o")})


def test_a_launch_below_the_minimum_expected_saving_is_not_planned():
    """gain x MB of one launch against min_us: 2B qkv (6.29 MB x 0.07 = 0.44 us) goes in at 0.1 us, the tiny models' sub-MB
    matrices (0.26 / 0.79 MB: 0.02 / 0.06 us) do not; without a minimum they would."""
    gains, budget = [("qkv", 0.07)], 192 * 10 ** 6
    assert len(plan_resident(narrow_weight_bytes(CONFIGS["Qwen2-VL-2B"]), gains, budget, 0.1)) == 28
    for name in ("tiny", "tiny-w512"):
        sizes = narrow_weight_bytes(CONFIGS[name])
        assert plan_resident(sizes, gains, budget, 0.1) == frozenset()
        assert len(plan_resident(sizes, gains, budget)) == len(sizes)
    sizes = narrow_weight_bytes(CONFIGS["Qwen2-VL-2B"])
    assert {k for _, k in plan_resident(sizes, GAINS, 10 ** 12, 1.0)} == {"qkv", "down"}   # 0.3 x 6.29 = 1.9, 0.2 x 4.7 = 0.94, 0.05 x 27.5 = 1.4


def test_fp8_weights_count_their_own_bytes():
    cfg = CONFIGS["Qwen2-VL-2B"]
    bf, f8 = narrow_weight_bytes(cfg), narrow_weight_bytes(cfg, "fp8")
    assert f8[0] == {"qkv": 2048 * 1536 + 4 * 2048, "o": 1536 * 1536 + 4 * 1536, "down": 1536 * 8960 + 4 * 1536}
    budget = 100 * 10 ** 6
    n_bf, n_f8 = len(plan_resident(bf, [("qkv", 1.0)], budget)), len(plan_resident(f8, [("qkv", 1.0)], budget))
    assert n_bf == budget // bf[0]["qkv"] == 15 and n_f8 == 28      # all 28 fp8 qkv matrices are 88 MB
    assert used(f8, plan_resident(f8, GAINS, budget)) <= budget
