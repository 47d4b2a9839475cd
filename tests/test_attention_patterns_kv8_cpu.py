"""The one-winner patterns in their e4m3-exact encoding (tests/attn_patterns.py, last section), proven without a GPU: for every
(heads, pattern, scale set) that test_gpu_attention_exact_kv8.py runs, the gap preconditions hold under each kv head's K scale
(asserted while the case is built) and the fp64 softmax over the dequantised operands returns V[winner] * v_scale within the
stated tolerance; for `up` and `down` the float64 model of the fp8 kernel (kv_fp8_ref.model_decode_kv8) does too.  The last tests
restate, in the reference, the addressing errors the fp8 instantiation could make on its own, and show that the expected rows
catch each of them and name the row."""
import numpy as np
import pytest

from karanta_ocr_amd.weights import fp8_e4m3_to_f32
from tests import attn_patterns as AP
from tests import kv_fp8_ref as R


@pytest.mark.parametrize("H,KVH", AP.DECODE_HEADS)
@pytest.mark.parametrize("pattern,scales", AP.kv8_decode_params())
def test_kv8_decode_patterns_on_the_reference(H, KVH, pattern, scales):
    case = AP.decode_case_kv8(AP.DECODE_BATCH, H, KVH, pattern, scales)
    assert [int(c) for c, f in zip(case.ctx, case.finished) if not f] == AP.DECODE_CTX and case.finished.sum() == 2
    assert case.k_codes.shape == case.v_codes.shape == (len(AP.DECODE_BATCH), KVH, AP.DECODE_S_MAX, 128)
    assert (case.v_codes[0, :, 1:] == R.STALE_CODE).all() and (case.v_codes[-1] != R.STALE_CODE).all()    # ctx_len 0; the last cache row
    assert len(case.units) == H * len(AP.DECODE_CTX)
    AP.check_output(AP.decode_reference_kv8(case), case, f"reference, kv8 decode {pattern} {scales} H={H}")
    if pattern in ("up", "down"):       # the kernel's own arithmetic, restated: 8 splits of 8 waves
        got = np.zeros((len(case.ctx), H * 128), np.float32)
        for b, c in enumerate(case.ctx):
            if case.finished[b]:
                continue
            for kvh in range(KVH):
                hs = slice(kvh * (H // KVH), (kvh + 1) * (H // KVH))
                o = R.model_decode_kv8(case.q[b, hs], case.k_codes[b, kvh, :c + 1], case.v_codes[b, kvh, :c + 1], case.scales[0, kvh],
                                       case.scales[1, kvh], 8, 8)
                got[b, hs.start * 128:hs.stop * 128] = o.reshape(-1)
        AP.check_output(got, case, f"model of the fp8 kernel, {pattern} {scales} H={H}")


@pytest.mark.parametrize("pattern,scales", AP.kv8_decode_params())
def test_kv8_decode_batch_of_21_on_the_reference(pattern, scales):
    case = AP.decode_case_kv8(AP.DECODE_BATCH32, 12, 2, pattern, scales)
    assert len(case.ctx) == 21
    AP.check_output(AP.decode_reference_kv8(case), case, f"reference, kv8 decode B=21 {pattern} {scales}")


@pytest.mark.parametrize("c", AP.KV8_ROWS_C)
def test_kv8_draft_rows_on_the_reference(c):
    case = AP.rows_case_kv8(c)
    assert case.row_slot.tolist() == [1, 0] * 4 and case.ctx.tolist() == [c + 32 + j // 2 if j % 2 == 0 else c + j // 2 for j in range(8)]
    assert len(set(case.scales[0])) == 2 and len(set(case.scales[1])) == 2
    AP.check_output(AP.decode_reference_kv8(case), case, f"reference, kv8 draft rows c={c}")


def test_the_kv8_encoding_is_what_the_docstring_says():
    """Exact products, the channel placement (asserted by kv8_channels itself for 1 .. 4 kv heads), another head's rows score 0,
    and the gap: 261 * k_scale log2 units per step of a, >= GAP at 0.37 and no longer at half of that."""
    chans = AP.kv8_channels(4)
    assert sorted(c // 16 for t in chans for c in t) == sorted(list(range(8)) * 2)
    assert all(max(t[:2]) < 64 <= min(t[2:]) for t in chans)
    q = AP.kv8_q_vectors(4, 4)
    k = fp8_e4m3_to_f32(AP.kv8_k_codes(np.full((4, 1), 7777)))
    np.testing.assert_array_equal(q @ k[:, 0].T, np.diag([AP.C_Q8 * 7777] * 4))
    step = float(AP.scores_log2_kv8(np.asarray([1]), 1.0)[0])
    assert 260 < step < 262
    vis = np.ones((1, 8), bool)
    AP.check_gaps(np.arange(8), vis, None, 128, "k_scale 0.37", kv8_k_scale=0.37)
    with pytest.raises(AssertionError, match="comes within"):
        AP.check_gaps(np.arange(8), vis, None, 128, "k_scale 0.18", kv8_k_scale=0.18)
    assert AP.kv8_swap_8_16(np.arange(64)).tolist() == [*range(8), *range(16, 24), *range(8, 16), *range(24, 40), *range(48, 56),
                                                        *range(40, 48), *range(56, 64)]
    assert len(AP.kv8_decode_params()) == 30 and AP.KV8_FAULTS == ["mask-fg", "p-unpermuted", "v-scale-next-head", "v-tiles-swapped",
                                                                    "k-halves-swapped"]


# ----------------------------------------------------------------------------- the expected rows tell the fp8 kernel's faults apart
@pytest.fixture(scope="module")
def up_odd():
    return AP.decode_case_kv8(AP.DECODE_BATCH, 12, 2, "up", "odd")


def test_kv8_one_key_too_many_is_named(up_odd):
    with pytest.raises(AssertionError, match=r"slot 0 \(ctx_len 0\) head 0 returned key 1 of kv head 0 \(a stale row: ctx_len is 0\), expected key 0 of"):
        AP.check_output(AP.decode_reference_kv8(up_odd, extra_keys=1), up_odd, "key <= ctx")


def test_kv8_a_dropped_partial_unit_is_named(up_odd):
    with pytest.raises(AssertionError, match=r"slot 4 \(ctx_len 32\) head 0 returned key 31 of kv head 0, expected key 32"):
        AP.check_output(AP.decode_reference_kv8(up_odd, whole_units_only=True), up_odd, "nu = ctx >> 5")
    case = AP.decode_case_kv8(AP.DECODE_BATCH, 12, 2, "tent-ctx", "pow2")
    with pytest.raises(AssertionError, match=r"60 of 144 .*\n.*returned key 31 of kv head 0, expected key 32"):
        AP.check_output(AP.decode_reference_kv8(case, whole_units_only=True), case, "nu = ctx >> 5")


def test_kv8_a_mask_in_unpermuted_key_order_is_named(up_odd):
    """key = key0 + 8 fg + 4 kt + r where the lane group holds keys 8 pi(fg) ..: at 44 keys (ctx_len 43, 12 keys in the last unit) keys
    40 .. 43 are masked and the stale keys 48 .. 51 are not (every stale V row holds the same code: the first one is named).  No
    other context of the batch ends inside keys 8 .. 23 of a unit, and at those this fault changes nothing: the one failing slot
    is the reason ctx_len 43 is in DECODE_CTX."""
    assert [c for c in AP.DECODE_CTX if 8 < (c + 1) % 32 < 24] == [43]
    with pytest.raises(AssertionError, match=r"12 of 144 .*\n.*slot 5 \(ctx_len 43\) head 0 returned key 44 of kv head 0 \(a stale row: ctx_len is 43\), expected key 43"):
        AP.check_output(AP.decode_reference_kv8(up_odd, fault="mask-fg"), up_odd, "mask with fg")
    case = AP.decode_case_kv8([(40, 0)], 12, 2, "tent-ctx", "unit")      # 41 keys: the winner itself is masked, and no row outranks it
    with pytest.raises(AssertionError, match=r"slot 0 \(ctx_len 40\) head 0 returned key 39 of kv head 0, expected key 40"):
        AP.check_output(AP.decode_reference_kv8(case, fault="mask-fg"), case, "mask with fg")


def test_kv8_p_against_v_in_unpermuted_key_order_is_named(up_odd):
    """The winner's weight meets the V of the key 8 further on (or back) wherever the winner sits in keys 8 .. 23 of its unit: in the
    batch that is ctx_len 43 alone (keys 43 and 42 meet the stale columns 51 and 50; the first stale row is named)."""
    with pytest.raises(AssertionError, match=r"12 of 144 .*\n.*slot 5 \(ctx_len 43\) head 0 returned key 44 of kv head 0 \(a stale row: ctx_len is 43\), expected key 43"):
        AP.check_output(AP.decode_reference_kv8(up_odd, fault="p-unpermuted"), up_odd, "P in S order")
    case = AP.decode_case_kv8(AP.DECODE_BATCH, 12, 2, "tent-ctx-1", "pow2")
    with pytest.raises(AssertionError, match=r"12 of 144 .*\n.*slot 5 \(ctx_len 43\) head 0 returned key 44 of kv head 0 \(a stale row: ctx_len is 43\), expected key 42"):
        AP.check_output(AP.decode_reference_kv8(case, fault="p-unpermuted"), case, "P in S order")
    case = AP.decode_case_kv8([(50, 0)], 12, 2, "tent-ctx-1", "odd")           # key 49 is key 17 of its unit: it meets V of key 41
    with pytest.raises(AssertionError, match=r"slot 0 \(ctx_len 50\) head 0 returned key 41 of kv head 0, expected key 49"):
        AP.check_output(AP.decode_reference_kv8(case, fault="p-unpermuted"), case, "P in S order")


@pytest.mark.parametrize("scales", ["pow2", "odd"])
def test_kv8_another_heads_v_scale_is_named(scales):
    case = AP.decode_case_kv8(AP.DECODE_BATCH, 12, 2, "down", scales)
    with pytest.raises(AssertionError, match=r"144 of 144 .*\n  slot 0 \(ctx_len 0\) head 0 returned no stored row \(closest: key"):
        AP.check_output(AP.decode_reference_kv8(case, fault="v-scale-next-head"), case, "kv_scale[kv_heads + kvh + 1]")
    unit = AP.decode_case_kv8([(5, 0)], 12, 2, "down", "unit")                  # equal scales cannot see it: why the sets differ per head
    AP.check_output(AP.decode_reference_kv8(unit, fault="v-scale-next-head"), unit, "unit scales")


def test_kv8_exchanged_v_channel_tiles_are_named(up_odd):
    with pytest.raises(AssertionError, match=r"144 of 144 .*\n  slot 0 \(ctx_len 0\) head 0 returned no stored row \(closest: key"):
        AP.check_output(AP.decode_reference_kv8(up_odd, fault="v-tiles-swapped"), up_odd, "tiles 2i <-> 2i + 1")


def test_kv8_exchanged_k_channel_halves_are_named(up_odd):
    """K channels 64j + c read as 64 (1 - j) + c against an unchanged q: every score is 0, the softmax is flat over the visible keys,
    and only the one-key context still returns its row."""
    with pytest.raises(AssertionError, match=r"132 of 144 .*\n  slot 1 \(ctx_len 30\) head 0 returned no stored row"):
        AP.check_output(AP.decode_reference_kv8(up_odd, fault="k-halves-swapped"), up_odd, "K halves")
