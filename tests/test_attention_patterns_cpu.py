"""The one-winner attention patterns of tests/attn_patterns.py, proven without a GPU: for every parametrisation that
test_gpu_attention_exact.py runs, the gap preconditions hold (asserted while the case is built) and the suite's fp64
softmax reference returns V[winner] within the stated tolerance — so a kernel that fails there is wrong, not the
pattern.  The last tests restate single-key faults in the reference and show that the expected rows catch them."""
import numpy as np
import pytest

from tests import attn_patterns as AP


@pytest.mark.parametrize("pattern", AP.vit_patterns(AP.VIT_LENS["ragged"]))
def test_vit_ragged_patterns_on_the_reference(pattern):
    case = AP.vit_case(AP.VIT_LENS["ragged"], pattern)
    AP.check_output(AP.vit_reference(case), case, f"reference, vit ragged {pattern}")


@pytest.mark.parametrize("pattern", AP.vit_patterns(AP.VIT_LENS["windows"]))
def test_vit_window_patterns_on_the_reference(pattern):
    case = AP.vit_case(AP.VIT_LENS["windows"], pattern)
    AP.check_output(AP.vit_reference(case), case, f"reference, vit windows {pattern}")


def test_the_tent_peaks_that_fit_are_the_ones_listed():
    assert AP.vit_patterns(AP.VIT_LENS["ragged"]) == ["up", "down"] + [f"tent-{p}" for p in AP.VIT_PEAKS]
    assert AP.vit_patterns(AP.VIT_LENS["windows"]) == ["up", "down", "tent-0", "tent-31", "tent-32", "tent-63", "tent-last"]
    case = AP.vit_case(AP.VIT_LENS["ragged"], "tent-64")
    # segments shorter than the peak take their last key; the others the key at 64
    wins = {tuple(np.unique(u.win % case.v.shape[1])) for u in case.units if u.head == 0}
    assert len(wins) == len(AP.VIT_LENS["ragged"]) and all(len(w) == 1 for w in wins)


@pytest.mark.parametrize("pattern", ["up", "down"])
def test_vit_long_segment_on_the_reference(pattern):
    case = AP.vit_case(AP.VIT_LONG, pattern)
    AP.check_output(AP.vit_reference(case), case, f"reference, vit long {pattern}")


@pytest.mark.parametrize("H,KVH", AP.PREFILL_HEADS)
def test_prefill_patterns_on_the_reference(H, KVH):
    case = AP.prefill_case(AP.PREFILL_LENS, H, KVH, AP.PREFILL_S_MAX)
    assert sum(case.lens) == 723
    AP.check_output(AP.prefill_reference(case), case, f"reference, prefill H={H} KVH={KVH}")


def test_prefill_long_prompt_on_the_reference():
    H, KVH = AP.PREFILL_LONG_HEADS
    case = AP.prefill_case(AP.PREFILL_LONG, H, KVH, AP.PREFILL_LONG_S_MAX)
    AP.check_output(AP.prefill_reference(case), case, "reference, prefill long")


@pytest.mark.parametrize("H,KVH", AP.DECODE_HEADS)
@pytest.mark.parametrize("pattern", AP.decode_patterns())
def test_decode_patterns_on_the_reference(H, KVH, pattern):
    case = AP.decode_case(AP.DECODE_BATCH, H, KVH, pattern)
    live = [c for c, f in AP.DECODE_BATCH if not f]
    assert live == AP.DECODE_CTX and sum(f for _, f in AP.DECODE_BATCH) == 2
    assert (case.v[0, :, 1:] == AP.STALE_V).all() and (case.v[-1] != AP.STALE_V).all()    # ctx_len 0 and the last cache row
    AP.check_output(AP.decode_reference(case), case, f"reference, decode {pattern} H={H}")


@pytest.mark.parametrize("pattern", AP.decode_patterns())
def test_decode_batch_of_21_on_the_reference(pattern):
    case = AP.decode_case(AP.DECODE_BATCH32, 12, 2, pattern)
    assert len(case.ctx) == 21
    AP.check_output(AP.decode_reference(case), case, f"reference, decode B=21 {pattern}")


# ----------------------------------------------------------------------------- the expected rows tell a one-key fault apart
def test_one_key_too_many_is_named():
    case = AP.decode_case(AP.DECODE_BATCH, 12, 2, "up")
    with pytest.raises(AssertionError, match=r"slot 0 \(ctx_len 0\) head 0 returned key 1 of kv head 0 \(a stale row: ctx_len is 0\), expected key 0 of"):
        AP.check_output(AP.decode_reference(case, extra_keys=1), case, "key <= ctx")


def test_a_dropped_partial_unit_is_named():
    case = AP.decode_case(AP.DECODE_BATCH, 12, 2, "up")
    with pytest.raises(AssertionError, match=r"slot 4 \(ctx_len 32\) head 0 returned key 31 of kv head 0, expected key 32"):
        AP.check_output(AP.decode_reference(case, whole_units_only=True), case, "nu = ctx >> 5")
    case = AP.decode_case(AP.DECODE_BATCH, 12, 2, "tent-ctx")
    with pytest.raises(AssertionError, match=r"60 of 144 .*\n.*returned key 31 of kv head 0, expected key 32"):
        AP.check_output(AP.decode_reference(case, whole_units_only=True), case, "nu = ctx >> 5")


def test_a_causal_mask_one_key_late_is_named():
    case = AP.prefill_case(AP.PREFILL_LENS, 2, 1, AP.PREFILL_S_MAX)
    out = AP.prefill_reference(case)
    off = 0
    for b, ln in enumerate(case.lens):          # key <= qpos + 1, inside the prompt
        out[off:off + ln] = AP.ref_attention(case.q[:, off:off + ln], case.k[b, :, :ln], case.v[b, :, :ln], case.hd ** -0.5, True, q_pos0=1)
        off += ln
    with pytest.raises(AssertionError, match=r"query 0 of segment 0 head 0 returned key 1 of slot 0, kv head 0, expected key 0 of slot 0"):
        AP.check_output(out, case, "key <= qpos + 1")


def test_a_segment_that_reads_its_neighbours_first_row_is_named():
    case = AP.vit_case(AP.VIT_LENS["windows"], "up")
    out = AP.vit_reference(case)
    # segment 0 (64 keys) with the first K row of segment 1 as a 65th key, and that key's V
    k = case.k[:, :65]
    v = np.concatenate([case.v[:, :64], case.v[:, 64:65]], 1)
    out[:64] = AP.ref_attention(case.q[:, :64], k, v, case.hd ** -0.5, False)
    with pytest.raises(AssertionError, match=r"query 0 of segment 0 head 0 returned key 0 of segment 1"):
        AP.check_output(out, case, "k row past the segment")


def test_another_heads_keys_do_not_score():
    """The channel pairs of two kv heads share no channel: a wrong head's K gives a flat softmax, never the winner."""
    for kvh, hd in ((4, 80), (4, 128)):
        pairs = AP.channel_pairs(kvh, hd)
        chans = [c for p in pairs for c in p]
        assert len(set(chans)) == 2 * kvh and max(chans) < hd
        assert len({c // 8 for c in chans}) == 2 * kvh
    q = AP.q_vectors(4, 4, 80)
    k = AP.k_from_a(np.full((4, 1), 777), 80)
    s = q @ k[:, 0].T
    np.testing.assert_array_equal(s, np.diag([AP.C_Q * 777] * 4))
