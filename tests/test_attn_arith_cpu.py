"""The attention arithmetic cases of tests/attn_arith.py, proven without a GPU: for every parametrisation that
test_gpu_attention_arith.py runs, the operands are bf16 values, the hd 80 prescaled q keeps its distance from rounding ties, the
lazy profiles realize every transition they are written for with a margin of 1/4 around the threshold, every tile of a mass case
carries its part of the output, and the outputs are large against the bound.  The kernels' accumulation restated in float64
(attn_arith.model) equals the plain softmax reference to 1e-12; with P rounded to bf16 it stays inside the bound E and exceeds the
bound's first line, which is why E has the terms A to D.  Each mutant of that model misses E by more than a factor 4 on the
families meant to catch it, and breaks the constant-channel equality where it treats o and l differently."""
import numpy as np
import pytest

from tests import attn_arith as AA

CONFIGS = [("vit",)] + [("prefill", H, KVH) for H, KVH in AA.PREFILL_HEADS] + [("decode", H, KVH) for H, KVH in AA.DECODE_HEADS]
IDS = ["-".join(str(x) for x in c) for c in CONFIGS]


def build(config, family):
    return AA.cached(config[0], family, *config[1:])


def splits_of(case):
    return AA.DECODE_SPLITS if case.kind == "decode" else [1]


def worst_ratio(case, out_of, first_line_only=False, probs=None):
    """max |out - o| / E over the problems, out_of(problem) the output to judge."""
    worst = 0.0
    for pr in (case.probs if probs is None else probs):
        o, spv, _ = AA.reference(case, pr)
        e = AA.bound(case, pr, o, spv, first_line_only)
        err = np.abs(out_of(pr) - o)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / e)
        worst = max(worst, float(np.nan_to_num(r, nan=np.inf).max()))
    return worst


@pytest.mark.parametrize("family", AA.FAMILIES)
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_operands_are_bf16_and_the_model_is_the_reference(config, family):
    case = build(config, family)
    assert AA.is_bf16(case.q, case.k, case.v)
    assert np.isfinite(case.k).all() and np.isfinite(case.v).all()
    if case.hd == 80:
        assert AA.tie_margin(case.q, 80) > 2.0 ** -20
    for pr in case.probs:
        o, spv, _ = AA.reference(case, pr)
        for ns in splits_of(case):
            m = AA.model(case, pr, ns)
            assert np.abs(m - o).max() <= 1e-12 * max(1.0, np.abs(o).max()), (pr.name, ns)


def test_prescaled_q_is_one_value_however_the_constant_is_rounded():
    """hd 80: the neighbouring f32 values of scale * log2(e) round every q element to the same bf16 value."""
    case = build(("vit",), "lazy")
    sl = AA.scale_log2e(80)
    want = AA.q_tilde(case.q, 80)
    for other in (np.nextafter(sl, np.float32(0)), np.nextafter(sl, np.float32(1)), np.float32(80 ** -0.5 * 1.4426950408889634)):
        np.testing.assert_array_equal(AA.bf16_round(case.q * other), want)


@pytest.mark.parametrize("config,want", [(("vit",), AA.VIT_EVENTS), (("prefill", 4, 2), AA.PREFILL_EVENTS_2),
                                         (("prefill", 7, 1), AA.PREFILL_EVENTS_1)], ids=["vit", "prefill-4-2", "prefill-7-1"])
def test_lazy_profiles_walk_every_transition_with_margin(config, want):
    ev, closest = AA.lazy_events(build(config, "lazy"))
    assert want <= ev, f"not realized: {sorted(want - ev)}"
    assert closest >= 0.25, f"a g = 1 query rises to within {closest:.3f} of the threshold"


def test_decode_levels_hold_the_in_wave_and_merge_transitions():
    lv = np.asarray(AA.decode_levels())
    assert lv.size == 33 and [c + 1 for c in AA.DECODE_CTX] == [31, 32, 96, 701, 1056]
    col = lv[0::8]                                        # wave 0 of the one-split launch: units 0, 8, 16, 24, 32
    d = np.diff(col)
    assert d[0] <= -150 and d[1] >= 150 and d[3] >= 8.25, d
    assert np.diff(lv[4::8])[1] >= 20                     # -161 -> -137: a rise whose alpha is 2^-24
    for ns in AA.DECODE_SPLITS[1:]:
        waves = AA.decode_waves(ns)
        split_of = (np.arange(33) % (ns * waves)) // waves
        m = [lv[split_of == s].max() for s in range(ns) if (split_of == s).any()]
        assert max(m) - min(m) > 150, (ns, m)             # two records whose sc is exp2(-150) = 0 in f32
        assert len(m) == ns or ns * waves > 33            # at ctx 1055 the 64-part launches leave splits without a unit, and
    assert (AA.DECODE_CTX[0] + 32) // 32 == 1             # at ctx 30 every launch with more than one split does


@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_every_tile_of_a_mass_case_carries_its_part(config):
    case = build(config, "mass")
    ok = np.concatenate([AA.contribution_ok(case, pr) for pr in case.probs])
    assert ok.mean() >= 0.9, ok.mean()


@pytest.mark.parametrize("family", ["mass", "lazy"])
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_outputs_are_large_against_the_bound(config, family):
    case = build(config, family)
    big = []
    for pr in case.probs:
        o, spv, _ = AA.reference(case, pr)
        e = AA.bound(case, pr, o, spv)
        ch = AA.nonneg_channels(case.hd)
        big.append((np.abs(o[:, ch]) >= 64 * e[:, ch]).ravel())
    assert np.concatenate(big).mean() >= 0.9


@pytest.mark.parametrize("family", ["mass", "lazy"])
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_correctly_rounded_arithmetic_stays_inside_E(config, family):
    """The model with P rounded to bf16 and the output rounded to bf16: inside E everywhere."""
    case = build(config, family)
    for ns in splits_of(case):
        r = worst_ratio(case, lambda pr: AA.bf16_round(AA.model(case, pr, ns, round_p=True).astype(np.float32)).astype(np.float64))
        assert r <= 1.0, (ns, r)


def test_the_first_line_of_E_alone_is_exceeded_by_correct_rounding():
    """Why E has terms A and B: a bf16 rounding errs by up to 2^-8 relative, not 2^-9, and the hd 128 varlen kernel — f32 P below the
    line, bf16 P above — shows it on most cases; an output below the smallest bf16 value shows term D."""
    for config, family in [(("prefill", 4, 2), "mass"), (("prefill", 7, 1), "mass"), (("prefill", 4, 2), "lazy")]:
        case = build(config, family)
        r = worst_ratio(case, lambda pr: AA.bf16_round(AA.model(case, pr, round_p=True).astype(np.float32)).astype(np.float64), first_line_only=True)
        assert r > 1.0, (config, family, r)


# ----------------------------------------------------------------------------- teeth
def mutant_ratio(case, mutant, ns=1, which=0, probs=None):
    return worst_ratio(case, lambda pr: AA.model(case, pr, ns, mutant=mutant, which=which), probs=probs)


@pytest.mark.parametrize("mutant", ["l_not_rescaled", "o_not_rescaled", "threshold_vs_previous_max"])
@pytest.mark.parametrize("config", CONFIGS[:3], ids=IDS[:3])
def test_lazy_cases_catch_a_wrong_rescale(config, mutant):
    assert mutant_ratio(build(config, "lazy"), mutant) > 4.0


@pytest.mark.parametrize("mutant", ["l_not_rescaled", "o_not_rescaled"])
@pytest.mark.parametrize("family", ["mass", "lazy"])
@pytest.mark.parametrize("config", CONFIGS[3:], ids=IDS[3:])
def test_decode_cases_catch_a_wrong_alpha(config, family, mutant):
    """One split: a wave walks up to five units, alpha is applied between them."""
    assert mutant_ratio(build(config, family), mutant, ns=1) > 4.0


@pytest.mark.parametrize("mutant", ["unit_dropped", "unit_doubled"])
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_mass_cases_catch_every_dropped_or_doubled_tile(config, mutant):
    """Varlen: every tile of the longest problem (ViT segment 0, 10 tiles; the 449-token prompt, 8 tiles) moves some output by more
    than 4 E.  Decode: with 22 and 33 units a unit holds 3-5 % of an output and E, with term C, is 1.2 % of it, so 4 E is out of reach
    for the lightest units: every unit of every row moves some output by more than 2 E — the kernel's own error is at most E, so the
    comparison fails whatever the rounding does — and in every row some unit by more than 4 E."""
    case = build(config, "mass")
    if case.kind != "decode":
        nk = max(pr.k.shape[0] for pr in case.probs)
        probs = [pr for pr in case.probs if pr.k.shape[0] == nk][:2]
        for t in range((nk + 63) // 64):
            assert mutant_ratio(case, mutant, which=t, probs=probs) > 4.0, t
        return
    for b in np.flatnonzero(case.finished == 0):
        probs = [pr for pr in case.probs if pr.rows[0] == b][:2]
        for ns in (1, 16):
            nu = (probs[0].k.shape[0] + 31) // 32
            if nu == 1 and mutant == "unit_doubled":
                continue                                  # o and l both double: nothing to see in a row of one unit
            r = [mutant_ratio(case, mutant, ns=ns, which=u, probs=probs) for u in range(nu)]
            assert min(r) > 2.0 and max(r) > 4.0, (b, ns, r)


@pytest.mark.parametrize("family", ["mass", "lazy"])
@pytest.mark.parametrize("config", CONFIGS[3:], ids=IDS[3:])
def test_decode_cases_catch_merge_weights_on_o_only(config, family):
    case = build(config, family)
    for ns in AA.DECODE_SPLITS[1:]:
        assert mutant_ratio(case, "sc_on_o_only", ns=ns) > 4.0, ns


@pytest.mark.parametrize("mutant", ["first_reference_clamped", "ones_row_63"])
def test_hd80_lazy_case_catches(mutant):
    assert mutant_ratio(build(("vit",), "lazy"), mutant) > 4.0


# ----------------------------------------------------------------------------- weights sum to one
def rounded_outputs(case, out_of):
    got = np.zeros((case.n_rows, case.heads * case.hd), np.float32)
    for pr in case.probs:
        got[pr.rows, pr.head * case.hd:(pr.head + 1) * case.hd] = AA.bf16_round(out_of(pr).astype(np.float32))
    return got


@pytest.mark.parametrize("family", ["sum1-mass", "sum1-lazy"])
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_constant_channels_come_back_from_the_reference(config, family):
    case = build(config, family)
    twin = build(config, case.scores)
    assert np.array_equal(case.q, twin.q) and np.array_equal(case.k, twin.k), "a sum1 case reuses the scores of its family"
    for pr in case.probs:
        assert (pr.v == case.const[pr.kvh]).all()
    got = rounded_outputs(case, lambda pr: AA.reference(case, pr)[0])
    stats = AA.check_sum1(got, case, "reference")
    assert stats["exact"] == stats["outputs"]
    if case.kind == "prefill" and family == "sum1-lazy":
        assert stats["flat_queries"] > 0, "no query whose largest weight is <= 1/64"
    # where l sums the rounded P, rounding P changes nothing: numerator and denominator share it
    if case.l_rounded:
        for ns in splits_of(case):
            AA.check_sum1(rounded_outputs(case, lambda pr: AA.model(case, pr, ns, round_p=True)), case, f"rounded P, {ns} splits")
    else:
        AA.check_sum1(rounded_outputs(case, lambda pr: AA.model(case, pr, round_p=True)), case, "rounded P above the line only")


SUM1_MUTANTS = [(("vit",), "l_not_rescaled", 1), (("vit",), "o_not_rescaled", 1), (("vit",), "first_reference_clamped", 1),
                (("vit",), "ones_row_63", 1), (("prefill", 4, 2), "l_not_rescaled", 1), (("prefill", 7, 1), "o_not_rescaled", 1),
                (("decode", 12, 2), "l_not_rescaled", 1), (("decode", 28, 4), "o_not_rescaled", 1), (("decode", 12, 2), "sc_on_o_only", 16),
                (("decode", 28, 4), "sc_on_o_only", 4)]


@pytest.mark.parametrize("config,mutant,ns", SUM1_MUTANTS, ids=[f"{'-'.join(map(str, c))}-{m}-{n}" for c, m, n in SUM1_MUTANTS])
def test_a_mutant_that_treats_o_and_l_differently_breaks_the_equality(config, mutant, ns):
    case = build(config, "sum1-lazy")
    got = rounded_outputs(case, lambda pr: AA.model(case, pr, ns, mutant=mutant))
    with pytest.raises(AssertionError):
        AA.check_sum1(got, case, mutant)
