"""Which decode steps may be speculative (sampling.spec_refusal, what Engine._spec_refusal and can_speculate answer with): the
whole table, without a GPU.  The expectation is written out here from the rule as its docstring states it — a pass that carries
state from token to token or records per step speculates only where the engine's SpecConfig has that state per draft — and not
taken from the function: the options cover passes (guided -> the guide, controls -> sampling controls and logit adjustments,
logprobs -> the record), a step whose passes are all covered speculates, and the message names what is not."""
import itertools

import pytest

from karanta_ocr_amd.request import SpecConfig
from karanta_ocr_amd.sampling import StepFeatures, spec_refusal

NO_CONFIG = "the engine was built without speculative=SpecConfig(...)"
NOT_SLOTS = "speculative steps run in slot mode (begin_slots)"
CONTROLS = "the step carries sampling controls or logit adjustments"
ANY_PASS = "the step carries guided decoding, sampling controls or logit adjustments"
HINT = " (guided requests speculate on an engine built with SpecConfig(guided=True))"
RECORDED = "log-probabilities are recorded"

ON_OFF = (False, True)
CONFIGS = [None] + [SpecConfig(3, 2, 4, guided=g, controls=c, logprobs=l) for g, c, l in itertools.product(ON_OFF, repeat=3)]


def expected(cfg, guided, processing, adjust, slot_mode, recording):
    if cfg is None:
        return NO_CONFIG
    if not slot_mode:
        return NOT_SLOTS
    uncovered = set()
    if guided and not cfg.guided:
        uncovered.add("guide")
    if (processing or adjust) and not cfg.controls:
        uncovered.add("controls")
    if uncovered:
        if cfg.guided:      # the guide is covered: what is left can only be the controls
            return CONTROLS
        return ANY_PASS + (HINT if "guide" in uncovered else "")
    if recording and not cfg.logprobs:
        return RECORDED
    return None


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "none" if c is None else f"g{c.guided:d}c{c.controls:d}l{c.logprobs:d}")
def test_the_whole_table(cfg):
    seen = set()
    for guided, processing, adjust, slot_mode, recording in itertools.product(ON_OFF, repeat=5):
        want = expected(cfg, guided, processing, adjust, slot_mode, recording)
        # the passes that carry no state per draft (the Gumbel pass, the repetition pass) decide nothing
        for sampling, repetition in itertools.product(ON_OFF, repeat=2):
            step = StepFeatures(sampling or guided or adjust, guided, processing, adjust, repetition)
            assert spec_refusal(cfg, step, slot_mode, recording) == want, (cfg, step, slot_mode, recording)
        seen.add(want)
    if cfg is None:
        assert seen == {NO_CONFIG}
    else:
        assert None in seen and NOT_SLOTS in seen
        assert (RECORDED in seen) == (not cfg.logprobs)
        assert (CONTROLS in seen) == (cfg.guided and not cfg.controls)
        assert (ANY_PASS + HINT in seen) == (not cfg.guided)
        assert (ANY_PASS in seen) == (not cfg.guided and not cfg.controls)


def test_the_cases_the_engine_tests_assert():
    """The refusals tests/test_gpu_spec_controls_engine.py, test_gpu_spec_logprobs_engine.py and test_gpu_spec_guided_engine.py
    provoke on a real engine, with the strings they match."""
    slot = dict(slot_mode=True, recording=False)
    bare, guided = SpecConfig(3, 1, 3), SpecConfig(3, 1, 3, guided=True)
    controls = SpecConfig(3, 1, 3, controls=True)
    # controls engine built without the option: the old string, verbatim, for either pass; a sampled step speculates
    for kw in (dict(processing=True), dict(adjust=True)):
        assert spec_refusal(bare, StepFeatures(True, False, **kw), **slot) == ANY_PASS
    assert spec_refusal(bare, StepFeatures(True, False), **slot) is None
    # refusals that stay on an engine with controls: a guide needs SpecConfig(guided=True), a record SpecConfig(logprobs=True)
    assert spec_refusal(controls, StepFeatures(True, False, True, True), **slot) is None
    assert "SpecConfig(guided=True)" in spec_refusal(controls, StepFeatures(True, True, True), **slot)
    assert "log-probabilities" in spec_refusal(controls, StepFeatures(True, False, True), slot_mode=True, recording=True)
    assert spec_refusal(controls, StepFeatures(), **slot) is None
    # the log-probabilities engine built without the option
    assert spec_refusal(SpecConfig(3, 1, 3, guided=True, controls=True), StepFeatures(True), slot_mode=True, recording=True) == RECORDED
    assert spec_refusal(SpecConfig(3, 1, 3, guided=True, controls=True), StepFeatures(True), **slot) is None
    # the guided engine: controls and adjustments refused by name, a record refused, and without the option the hint
    assert spec_refusal(guided, StepFeatures(True, True), **slot) is None
    assert "sampling controls" in spec_refusal(guided, StepFeatures(True, True, processing=True), **slot)
    assert "logit adjustments" in spec_refusal(guided, StepFeatures(True, True, adjust=True), **slot)
    assert "log-probabilities" in spec_refusal(guided, StepFeatures(True, True), slot_mode=True, recording=True)
    assert spec_refusal(bare, StepFeatures(True, True), **slot).endswith(HINT)
    assert spec_refusal(bare, StepFeatures(True, False), **slot) is None
    # generate() is not slot mode, and an engine without a SpecConfig has nothing to speculate with
    assert spec_refusal(bare, StepFeatures(), slot_mode=False, recording=False) == NOT_SLOTS
    assert "without speculative" in spec_refusal(None, StepFeatures(), **slot)
