"""The attention kernels on inputs whose softmax has one winner per query (tests/attn_patterns.py): the expected output
is a stored V row, so one key too many or too few, a wrong row offset, a dropped partial unit or a wrong GQA mapping
returns a DIFFERENT row and fails by >= 1/15 relative, where N(0,1) inputs would move the output by 1/ctx of the
tolerance.  The rows a correct kernel must not reach — cache rows past the context (slot reuse after a longer page),
the neighbouring segment's rows in ragged storage, causally masked keys — outrank every visible key, and the V^T
columns past a decode context hold finite stale values.  test_attention_patterns_cpu.py proves every case here on the
fp64 reference first.  q, K and V^T are uploaded directly (no kr_qkv_prep); buffers have the product's shapes.
Through the C-ABI, on a real MI355X."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import positions as POS  # noqa: E402
from karanta_ocr_amd._lib import lib, ptr  # noqa: E402
from karanta_ocr_amd.weights import unpack_rows32  # noqa: E402
from tests import attn_patterns as AP  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def host(t: torch.Tensor) -> np.ndarray:
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def t_(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_CASES = {}


def cached(key, make):
    """A ViT / prefill case (small) is built, and its gap preconditions asserted, once for the query-block sizes that launch on it."""
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ----------------------------------------------------------------------------- kr_attn_varlen / kr_attn_varlen_q
def run_varlen(L, case, plan, causal, k_hs, vt_hs, what):
    n, H, KVH, hd = sum(case.lens), case.heads, case.kv_heads, case.hd
    q_d, k_d, vt_d = dev_bf16(case.q), dev_bf16(case.k), dev_bf16(case.vt)
    o = torch.full((n, H * hd), -7.0, dtype=torch.bfloat16, device=DEV)
    qb, ql = t_(plan.qblk), t_(plan.qblk_len)
    if plan.q_block == 128:      # the entry point without a block size = 128-query work lists
        L.kr_attn_varlen(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(o), ptr(qb), ptr(ql), plan.qblk.shape[0], n, H, KVH, hd, k_hs, vt_hs,
                         hd ** -0.5, 1 if causal else 0, 0)
    else:
        L.kr_attn_varlen_q(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(o), ptr(qb), ptr(ql), plan.qblk.shape[0], n, H, KVH, hd, k_hs, vt_hs,
                           hd ** -0.5, 1 if causal else 0, plan.q_block, 0)
    AP.check_output(host(o), case, what)


def run_vit(L, lens, pattern, q_block):
    case = cached(("vit", tuple(lens), pattern), lambda: AP.vit_case(lens, pattern))
    k_row0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    vt_blk0 = np.concatenate([[0], np.cumsum([(x + 63) // 64 for x in lens])[:-1]])
    plan = POS.make_attn_plan(lens, k_row0, vt_blk0, False, q_block=q_block)
    n = sum(lens)
    assert case.k.shape == (4, n, 80) and case.vt.shape == (4, plan.n_vt_blocks, 80, 64)
    run_varlen(L, case, plan, False, n * 80, plan.n_vt_blocks * 80 * 64, f"vit {lens} {pattern} q_block={q_block}")


@pytest.mark.parametrize("q_block", [128, 256])
@pytest.mark.parametrize("pattern", AP.vit_patterns(AP.VIT_LENS["ragged"]))
def test_vit_hd80_ragged_segments_return_the_winning_key(L, pattern, q_block):
    """Segments of 1 .. 300 keys stored back to back: with `up` the first K row of the next segment outranks a segment's
    last key, with `down` the previous segment's last row outranks its first; the tents put the winner on and beside
    every 32- and 64-key border."""
    run_vit(L, AP.VIT_LENS["ragged"], pattern, q_block)


@pytest.mark.parametrize("q_block", [128, 256])
@pytest.mark.parametrize("pattern", AP.vit_patterns(AP.VIT_LENS["windows"]))
def test_vit_hd80_window_segments_return_the_winning_key(L, pattern, q_block):
    """The segment lengths of Qwen2.5-VL's windows (64 and the ragged ones at the right / bottom edge)."""
    run_vit(L, AP.VIT_LENS["windows"], pattern, q_block)


@pytest.mark.parametrize("q_block", [128, 256])
@pytest.mark.parametrize("pattern", ["up", "down"])
def test_vit_hd80_long_segment(L, pattern, q_block):
    """22 KV tiles: `up` moves the lazy reference maximum in every tile, `down` never after the first."""
    run_vit(L, AP.VIT_LONG, pattern, q_block)


def run_prefill(L, lens, H, KVH, s_max, q_block):
    case = cached(("prefill", tuple(lens), H, KVH, s_max), lambda: AP.prefill_case(lens, H, KVH, s_max))
    B = len(lens)
    plan = POS.prefill_attn_plan(lens, list(range(B)), KVH, s_max)
    if q_block != plan.q_block:
        plan = POS.make_attn_plan(lens, [i * KVH * s_max for i in range(B)], [i * KVH * (s_max // 64) for i in range(B)], True,
                                  q_block=q_block)
    assert case.k.shape == (B, KVH, s_max, 128) and case.vt.shape == (B, KVH, s_max // 64, 128, 64)
    run_varlen(L, case, plan, True, s_max * 128, (s_max // 64) * 128 * 64, f"prefill {lens} H={H} KVH={KVH} q_block={q_block}")


@pytest.mark.parametrize("q_block", [128, 256])
@pytest.mark.parametrize("H,KVH", AP.PREFILL_HEADS)
def test_prefill_hd128_every_query_checks_its_own_mask_edge(L, H, KVH, q_block):
    """Even kv heads: each of the 723 queries must return its own diagonal key although the next key (masked only by
    causality) and the stale cache rows past the prompt outrank it — across tile (64), wave (32) and query-block borders.
    Odd kv heads: key 0 wins for every query."""
    run_prefill(L, AP.PREFILL_LENS, H, KVH, AP.PREFILL_S_MAX, q_block)


@pytest.mark.parametrize("q_block", [128, 256])
def test_prefill_hd128_long_prompt(L, q_block):
    H, KVH = AP.PREFILL_LONG_HEADS
    run_prefill(L, AP.PREFILL_LONG, H, KVH, AP.PREFILL_LONG_S_MAX, q_block)


# ----------------------------------------------------------------------------- decode: split-KV partials and their merges
def upload_decode(case):
    B, KVH, s_max = len(case.ctx), case.kv_heads, case.s_max
    assert case.k.shape == (B, KVH, s_max, 128) and case.vt.shape == (B, KVH, s_max // 64, 128, 64)
    return dev_bf16(case.q), dev_bf16(case.k), dev_bf16(case.vt), t_(case.ctx), t_(case.finished)


@pytest.mark.parametrize("H,KVH", AP.DECODE_HEADS)
@pytest.mark.parametrize("pattern", AP.decode_patterns())
def test_decode_attention_returns_the_winning_key(L, H, KVH, pattern):
    """kr_attn_decode_slots + kr_attn_decode_merge at 8, 16 and 32 splits (8-, 4- and 2-wave workgroups, 64 parts each), contexts
    on both sides of a 32-key unit border, of a V^T block border and of the first context at which a wave gets a second unit,
    and the last cache row.  `up`: the key at ctx_len wins and every stale row past it outranks it; `down`: key 0 wins, so
    the merge meets records whose m differ by 10^5 log2 units and parts without a unit.  Slots whose finished flag is set
    keep their records.  Then kr_attn_decode_fused with n_split = 1, which writes the output itself: 8 parts, so a wave walks
    up to nine units and the prefetch of unit u + n_part runs."""
    case = AP.decode_case(AP.DECODE_BATCH, H, KVH, pattern)
    B, hd, s_max = len(case.ctx), 128, case.s_max
    q_d, k_d, vt_d, ctx_d, fin_d = upload_decode(case)
    for n_split in AP.DECODE_SPLITS:
        ws = torch.full((B * H * n_split * (hd + 4),), 9.0, dtype=torch.float32, device=DEV)
        o_d = torch.full((B, H * hd), -7.0, dtype=torch.bfloat16, device=DEV)
        L.kr_attn_decode_slots(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, 0)
        L.kr_attn_decode_merge(ptr(ws), ptr(o_d), B, H, hd, n_split, 0)
        rec = ws.cpu().numpy().reshape(B, -1)
        for b in range(B):
            if case.finished[b]:
                assert (rec[b] == 9.0).all(), f"slot {b} is finished: its records are not to be written (n_split={n_split})"
            else:
                assert np.isfinite(rec[b]).all() and not (rec[b].reshape(-1, hd + 4)[:, :hd + 2] == 9.0).all(1).any(), \
                    f"slot {b}: a record was left unwritten (n_split={n_split})"
        AP.check_output(host(o_d), case, f"decode {pattern} H={H} KVH={KVH} n_split={n_split}")
    ws = torch.full((B * H * (hd + 4),), 9.0, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(B * KVH, dtype=torch.int32, device=DEV)
    o_d = torch.full((B, H * hd), -7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_fused(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(o_d), ptr(ws), ptr(cnt), B, H, KVH, hd, s_max, 1, hd ** -0.5, 0)
    AP.check_output(host(o_d), case, f"fused decode, one split, {pattern} H={H} KVH={KVH}")
    assert not cnt.cpu().numpy().any()


@pytest.mark.parametrize("pattern", AP.decode_patterns())
def test_decode_merge32_batch_of_21(L, pattern):
    """A 17..32-row batch: the merge writes the packed XP layout; rows past the batch stay as they were."""
    H, KVH, hd, n_split = 12, 2, 128, 16
    case = AP.decode_case(AP.DECODE_BATCH32, H, KVH, pattern)
    B, s_max = len(case.ctx), case.s_max
    assert B == 21
    q_d, k_d, vt_d, ctx_d, fin_d = upload_decode(case)
    ws = torch.full((B * H * n_split * (hd + 4),), 9.0, dtype=torch.float32, device=DEV)
    pk = torch.full((32 * H * hd,), -7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_slots(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, 0)
    L.kr_attn_decode_merge32(ptr(ws), ptr(pk), B, H, hd, n_split, 0)
    got = unpack_rows32(host(pk), H * hd)
    AP.check_output(got[:B], case, f"decode merge32 {pattern}")
    assert (got[B:] == -7.0).all()


@pytest.mark.parametrize("pattern", ["up", "down"])
def test_decode_gqa_entry_point(L, pattern):
    """kr_attn_decode_gqa (the first decode attention, still exported): 4 waves per split, partials of hd + 2 floats."""
    H, KVH, hd, n_split = 12, 2, 128, 4
    batch = [(c, 0) for c in AP.DECODE_CTX]
    case = AP.decode_case(batch, H, KVH, pattern)
    B, s_max = len(case.ctx), case.s_max
    q_d, k_d, vt_d, ctx_d, _ = upload_decode(case)
    ws = torch.full((B * H * n_split * 4 * (hd + 2),), 9.0, dtype=torch.float32, device=DEV)
    o_d = torch.full((B, H * hd), -7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_gqa(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(o_d), ptr(ws), B, H, KVH, hd, 0, s_max, n_split, hd ** -0.5, 0)
    AP.check_output(host(o_d), case, f"decode gqa {pattern}")
