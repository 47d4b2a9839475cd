"""The decode attention on an fp8 (e4m3) KV cache — attn_decode2_kernel<KV8>, which has its own K load, K row order, mask index,
V^T load and scales — on inputs whose softmax has one winner per query, in the e4m3-exact encoding of tests/attn_patterns.py:
the expected output is a stored V row times its kv head's V scale, so one key too many or too few, a dropped unit, a mask or a P
in the wrong key order, exchanged channel tiles or another head's scale returns a DIFFERENT row and fails by >= 1/15 relative.
Cache rows past the context outrank every visible key (`up`), the V^T columns past it hold code 0x7E (448), and the K and V
scales differ from kv head to kv head.  test_attention_patterns_kv8_cpu.py proves every case here on the fp64 reference first and
shows that the expected rows name each of those faults.  q, the K codes, the V^T codes (kv_fp8_ref.vt_blocks8) and the [2][KVH]
scale table are uploaded directly.  Through the C-ABI, on a real MI355X.

Nothing was cut from the cross product heads x patterns x scale sets x splits x contexts: a parametrised case takes about 0.1 s on
the device (attn_patterns.kv8_decode_params lists patterns x scale sets)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError, kv8, lib, ptr  # noqa: E402
from karanta_ocr_amd.weights import bf16_round, unpack_rows32  # noqa: E402
from tests import attn_patterns as AP  # noqa: E402

DEV = "cuda:0"
HD = 128
REC = HD + 4


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def host(t: torch.Tensor) -> np.ndarray:
    torch.cuda.synchronize()
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def t_(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def upload(case):
    """(q, K codes, V^T codes, scales, ctx, finished, row_slot or None) on the device, in the shapes the engine's cache has."""
    S, KVH, s_max = case.k_codes.shape[0], case.kv_heads, case.s_max
    assert case.k_codes.shape == (S, KVH, s_max, HD) and case.vt.shape == (S, KVH, s_max // 64, 2, HD, 32)
    assert case.k_codes.dtype == case.vt.dtype == np.uint8 and case.scales.shape == (2, KVH) and case.scales.dtype == np.float32
    assert int(case.ctx.max()) <= s_max - 1 and (case.row_slot is None or int(case.row_slot.max()) < S)      # every read is inside
    return (dev_bf16(case.q), t_(case.k_codes), t_(case.vt), t_(case.scales), t_(case.ctx), t_(case.finished),
            None if case.row_slot is None else t_(case.row_slot))


def slots_records(L, dev, B, H, KVH, s_max, n_split):
    q_d, k_d, vt_d, sc_d, ctx_d, fin_d, _ = dev
    ws = torch.full((B * H * n_split * REC,), 9.0, dtype=torch.float32, device=DEV)
    L.kr_attn_decode_slots_kv8(ptr(q_d), kv8(ptr(k_d), ptr(vt_d), ptr(sc_d)), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, HD, s_max,
                               n_split, HD ** -0.5, 0)
    return ws


def check_records(ws, case, n_split):
    rec = host(ws).reshape(len(case.ctx), -1)
    for b, fin in enumerate(case.finished):
        if fin:
            assert (rec[b] == 9.0).all(), f"slot {b} is finished: its records are not to be written (n_split={n_split})"
        else:
            assert np.isfinite(rec[b]).all() and not (rec[b].reshape(-1, REC)[:, :HD + 2] == 9.0).all(1).any(), \
                f"slot {b}: a record was left unwritten (n_split={n_split})"


# ----------------------------------------------------------------------------- kr_attn_decode_slots_kv8 + kr_attn_decode_merge
@pytest.mark.parametrize("H,KVH", AP.DECODE_HEADS)
@pytest.mark.parametrize("pattern,scales", AP.kv8_decode_params())
def test_kv8_decode_attention_returns_the_winning_key(L, H, KVH, pattern, scales):
    """At 8, 16 and 32 splits (8-, 4- and 2-wave workgroups, 64 parts each) and at the 1 and 4 splits of the fp8 bound test (8 and 32
    parts: a wave walks up to nine units and the prefetch of unit u + n_part runs): contexts on both sides of a 32-key unit border,
    of a V^T block border and of the first context at which a wave gets a second unit, 44 keys (the last unit ends inside its keys
    8 .. 23, where the fp8 kernel's key order pi shows), and the last cache row.  Slots whose finished flag is set keep their
    records; live slots leave none unwritten."""
    case = AP.decode_case_kv8(AP.DECODE_BATCH, H, KVH, pattern, scales)
    B, s_max = len(case.ctx), case.s_max
    dev = upload(case)
    worst = 0.0
    for n_split in AP.DECODE_SPLITS + AP.KV8_EXTRA_SPLITS:
        ws = slots_records(L, dev, B, H, KVH, s_max, n_split)
        o_d = torch.full((B, H * HD), -7.0, dtype=torch.bfloat16, device=DEV)
        L.kr_attn_decode_merge(ptr(ws), ptr(o_d), B, H, HD, n_split, 0)
        check_records(ws, case, n_split)
        got = host(o_d)
        worst = max(worst, AP.max_ratio(got, case))
        AP.check_output(got, case, f"kv8 decode {pattern} {scales} H={H} KVH={KVH} n_split={n_split}")
    print(f"\nkv8 slots + merge {pattern} {scales} H={H} KVH={KVH}: max |got - want| / tol = {worst:.4f}")


@pytest.mark.parametrize("pattern,scales", AP.kv8_decode_params())
def test_kv8_decode_merge32_batch_of_21(L, pattern, scales):
    """A 17..32-row batch on an fp8 cache: the merge writes the packed XP layout; rows past the batch stay as they were."""
    H, KVH, n_split = 12, 2, 16
    case = AP.decode_case_kv8(AP.DECODE_BATCH32, H, KVH, pattern, scales)
    B = len(case.ctx)
    assert B == 21
    ws = slots_records(L, upload(case), B, H, KVH, case.s_max, n_split)
    pk = torch.full((32 * H * HD,), -7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_merge32(ptr(ws), ptr(pk), B, H, HD, n_split, 0)
    got = unpack_rows32(host(pk), H * HD)
    print(f"\nkv8 slots + merge32 {pattern} {scales}: max |got - want| / tol = {AP.max_ratio(got[:B], case):.4f}")
    AP.check_output(got[:B], case, f"kv8 decode merge32 {pattern} {scales}")
    assert (got[B:] == -7.0).all()


# ----------------------------------------------------------------------------- kr_attn_decode_rows_kv8 (the speculative step)
@pytest.mark.parametrize("n_split", AP.KV8_ROWS_SPLITS)
@pytest.mark.parametrize("c", AP.KV8_ROWS_C)
def test_kv8_attn_rows_mask_the_later_drafts_keys(L, c, n_split):
    """attn_patterns.rows_case_kv8: rows j = 0 .. 3 of slot 0 at contexts c + j and of slot 1 at c + 32 + j behind the row map
    (1, 0, 1, 0, ...), `up` ramps, K and V scales of each kv head its own: row j must return key c + j of ITS slot times its head's
    V scale, while the keys the later draft rows stored behind it — real V codes, not stale filler — outrank it."""
    case = AP.rows_case_kv8(c)
    rows, H, KVH = len(case.ctx), case.heads, case.kv_heads
    q_d, k_d, vt_d, sc_d, ctx_d, fin_d, slot_d = upload(case)
    ws = torch.zeros(rows * H * n_split * REC, dtype=torch.float32, device=DEV)
    o_d = torch.full((rows, H * HD), -7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_rows_kv8(ptr(q_d), kv8(ptr(k_d), ptr(vt_d), ptr(sc_d)), ptr(ctx_d), ptr(fin_d), ptr(slot_d), ptr(ws), rows, H, KVH, HD,
                              case.s_max, n_split, HD ** -0.5, 0)
    L.kr_attn_decode_merge(ptr(ws), ptr(o_d), rows, H, HD, n_split, 0)
    got = host(o_d)
    print(f"\nkv8 rows + merge c={c} n_split={n_split}: max |got - want| / tol = {AP.max_ratio(got, case):.4f}")
    AP.check_output(got, case, f"kv8 draft rows, c = {c}, n_split = {n_split}")


@pytest.mark.parametrize("n_split", AP.KV8_ROWS_SPLITS)
@pytest.mark.parametrize("c", AP.KV8_ROWS_C)
def test_kv8_attn_rows_gives_the_records_of_one_row_steps(L, c, n_split):
    """Rows (slot 0, j) at contexts c .. c + 3 — across the 32-key unit and the 64-key block — and the rows of a second slot with a
    context of its own, one of them finished, in ONE launch of kr_attn_decode_rows_kv8, against K + 1 launches of
    kr_attn_decode_slots_kv8 at those contexts: the same records, bit for bit.  Random codes (no NaN code), per-head scales."""
    H, KVH, B, K, s_max = 4, 2, 2, 3, 128
    rows = B * (K + 1)
    rng = np.random.default_rng(100 * c + n_split)
    q = bf16_round(rng.standard_normal((rows, H, HD)).astype(np.float32))
    codes = lambda *shape: (rng.integers(0, 0x7F, size=shape) | (rng.integers(0, 2, size=shape) << 7)).astype(np.uint8)
    kc, vt = codes(B, KVH, s_max, HD), codes(B, KVH, s_max // 64, 2, HD, 32)
    assert not ((kc & 0x7F) == 0x7F).any() and not ((vt & 0x7F) == 0x7F).any()
    c1 = 40
    row_slot = np.asarray([r % B for r in range(rows)], np.int32)
    ctx = np.asarray([(c if r % B == 0 else c1) + r // B for r in range(rows)], np.int32)
    fin = np.zeros(rows, np.int32)
    fin[3 * B + 1] = 1                           # (slot 1, j = 3)
    assert int(ctx.max()) <= s_max - 1
    q_d, k_d, vt_d, sc_d = dev_bf16(q), t_(kc), t_(vt), t_(AP.kv8_scales("odd", KVH))
    rec = REC * n_split * H
    ws = torch.full((rows * rec,), 9.0, dtype=torch.float32, device=DEV)
    ctx_d, fin_d, slot_d = t_(ctx), t_(fin), t_(row_slot)        # (named: a temporary's memory is reused by the next upload)
    kv = kv8(ptr(k_d), ptr(vt_d), ptr(sc_d))
    L.kr_attn_decode_rows_kv8(ptr(q_d), kv, ptr(ctx_d), ptr(fin_d), ptr(slot_d), ptr(ws), rows, H, KVH, HD, s_max, n_split, HD ** -0.5, 0)
    got = host(ws).reshape(rows, rec)
    for j in range(K + 1):
        sl = slice(j * B, (j + 1) * B)
        ref = torch.full((B * rec,), 9.0, dtype=torch.float32, device=DEV)
        L.kr_attn_decode_slots_kv8(ptr(q_d[sl]), kv, ptr(ctx_d[sl]), ptr(fin_d[sl]), ptr(ref), B, H, KVH, HD, s_max, n_split, HD ** -0.5, 0)
        np.testing.assert_array_equal(got[sl].view(np.uint32), host(ref).reshape(B, rec).view(np.uint32), err_msg=f"rows of j = {j}")
    assert (got[3 * B + 1] == 9.0).all(), "the finished row's records are not to be written"
    assert not (got[np.flatnonzero(fin == 0)] == 9.0).all(1).any()
    assert np.isfinite(got).all()


# ----------------------------------------------------------------------------- argument checks
def test_kv8_entry_points_refuse_a_misaligned_cache_and_other_head_dims(L):
    """Both fp8 entry points read 16 bytes per lane: a K or V^T pointer that is not 16-byte aligned, and hd != 128, are refused
    before anything is launched."""
    case = AP.rows_case_kv8(29)
    rows, H, KVH, s_max = len(case.ctx), case.heads, case.kv_heads, case.s_max
    q_d, k_d, vt_d, sc_d, ctx_d, fin_d, slot_d = upload(case)
    ws = torch.full((rows * H * 2 * REC,), 9.0, dtype=torch.float32, device=DEV)
    good = kv8(ptr(k_d), ptr(vt_d), ptr(sc_d))
    calls = []
    for kv, hd in ((kv8(ptr(k_d) + 1, ptr(vt_d), ptr(sc_d)), HD), (kv8(ptr(k_d), ptr(vt_d) + 8, ptr(sc_d)), HD), (good, 64), (good, 80)):
        calls.append(lambda kv=kv, hd=hd: L.kr_attn_decode_slots_kv8(ptr(q_d), kv, ptr(ctx_d), ptr(fin_d), ptr(ws), 2, H, KVH, hd, s_max, 2,
                                                                     hd ** -0.5, 0))
        calls.append(lambda kv=kv, hd=hd: L.kr_attn_decode_rows_kv8(ptr(q_d), kv, ptr(ctx_d), ptr(fin_d), ptr(slot_d), ptr(ws), rows, H, KVH,
                                                                    hd, s_max, 2, hd ** -0.5, 0))
    for call in calls:
        with pytest.raises(KarantaHipError):
            call()
    assert (host(ws) == 9.0).all()
