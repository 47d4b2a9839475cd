"""The softmax arithmetic of the three attention kernels — attn_varlen_kernel at hd 80 (ViT) and hd 128 (causal prefill),
attn_decode2_kernel with attn_merge_kernel — on the cases of tests/attn_arith.py: outputs of order one, every tile or unit a
comparable part of them, tile maxima that walk the lazy-rescale state machine, and V channels that are constant over the keys.
The float64 softmax reference over the stored operands is met within the per-element bound E derived in attn_arith's docstring
(no absolute tolerance to hide in), and constant channels come back bit for bit where numerator and denominator share the
rounded P.  test_attn_arith_cpu.py proves every case on the reference first, including that the mistakes these cases are for
(a rescale of o but not l, a threshold against the wrong maximum, a dropped tile, a merge that weights l wrongly, ...) miss E.
Every test prints its measured max |got - o| / E.  q, K and V^T are uploaded directly (no kr_qkv_prep) into buffers of the
product's shapes.  Through the C-ABI, on a real MI355X."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import positions as POS  # noqa: E402
from karanta_ocr_amd._lib import lib, ptr  # noqa: E402
from karanta_ocr_amd.weights import unpack_rows32  # noqa: E402
from tests import attn_arith as AA  # noqa: E402
from tests.exact_cases import POISON_OUT, Guarded  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def t_(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def out_buffer(rows: int, cols: int) -> Guarded:
    """The output inside a poisoned allocation with guard bands and guard rows: nothing but [rows, cols] may be written."""
    return Guarded(torch, DEV, "bf16", rows, cols, role="out")


def values(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def judge(got: np.ndarray, case: AA.Case, what: str) -> None:
    assert np.isfinite(got).all(), f"{what}: non-finite outputs"
    if case.sum1:
        stats = AA.check_sum1(got, case, what)
        print(f"\n{what}: {stats['exact']} of {stats['outputs']} outputs are the constant bit for bit" +
              (f"; {stats['flat_queries']} (query, head) pairs with every weight <= 1/64" if not case.l_rounded else ""))
        return
    r, where = AA.max_ratio(got, case)
    print(f"\n{what}: max |got - o| / E = {r:.3f} (against the first line of E alone: {AA.max_ratio(got, case, first_line_only=True)[0]:.3f})")
    assert r <= 1.0, f"{what}: |got - o| = {r:.3f} E at {where}"


# ----------------------------------------------------------------------------- kr_attn_varlen / kr_attn_varlen_q
def run_varlen(L, case, plan, causal, k_hs, vt_hs, what):
    n, H, KVH, hd = sum(case.lens), case.heads, case.kv_heads, case.hd
    q_d, k_d, vt_d = dev_bf16(case.q), dev_bf16(case.k), dev_bf16(case.vt)
    o = out_buffer(n, H * hd)
    qb, ql = t_(plan.qblk), t_(plan.qblk_len)
    if plan.q_block == 128:      # the entry point without a block size = 128-query work lists
        L.kr_attn_varlen(ptr(q_d), ptr(k_d), ptr(vt_d), o.ptr, ptr(qb), ptr(ql), plan.qblk.shape[0], n, H, KVH, hd, k_hs, vt_hs,
                         hd ** -0.5, 1 if causal else 0, 0)
    else:
        L.kr_attn_varlen_q(ptr(q_d), ptr(k_d), ptr(vt_d), o.ptr, ptr(qb), ptr(ql), plan.qblk.shape[0], n, H, KVH, hd, k_hs, vt_hs,
                           hd ** -0.5, 1 if causal else 0, plan.q_block, 0)
    got = values(o.read())
    o.assert_untouched(what)
    judge(got, case, what)


@pytest.mark.parametrize("q_block", [128, 256])
@pytest.mark.parametrize("family", AA.FAMILIES)
def test_vit_hd80_softmax_arithmetic(L, family, q_block):
    """Segments of 577, 40 and 200 keys (10, 1 and 4 tiles, ragged ends; the 256-query launch has empty waves in its last blocks):
    prescaled q, accumulators that start at -m_ref, the first tile's reference at -40 and +60, the denominator from the ones row."""
    case = AA.cached("vit", family)
    lens = case.lens
    k_row0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    vt_blk0 = np.concatenate([[0], np.cumsum([(x + 63) // 64 for x in lens])[:-1]])
    plan = POS.make_attn_plan(lens, k_row0, vt_blk0, False, q_block=q_block)
    n = sum(lens)
    assert case.k.shape == (2, n, 80) and case.vt.shape == (2, plan.n_vt_blocks, 80, 64)
    run_varlen(L, case, plan, False, n * 80, plan.n_vt_blocks * 80 * 64, f"vit {family} q_block={q_block}")


@pytest.mark.parametrize("q_block", [128, 256])
@pytest.mark.parametrize("H,KVH", AA.PREFILL_HEADS)
@pytest.mark.parametrize("family", AA.FAMILIES)
def test_prefill_hd128_softmax_arithmetic(L, family, H, KVH, q_block):
    """Prompts of 449 and 97 tokens in slots 1 and 0 of a three-slot cache: l from the f32 P, the numerator from the bf16 P, the
    lazy reference under the causal mask.  The unused slot and the rows past each prompt hold large finite stale values."""
    case = AA.cached("prefill", family, H, KVH)
    s_max, n_slots = case.s_max, AA.PREFILL_N_SLOTS
    plan = POS.prefill_attn_plan(case.lens, case.slots, KVH, s_max)
    if q_block != plan.q_block:
        plan = POS.make_attn_plan(case.lens, [s * KVH * s_max for s in case.slots], [s * KVH * (s_max // 64) for s in case.slots], True,
                                  q_block=q_block)
    assert case.k.shape == (n_slots, KVH, s_max, 128) and case.vt.shape == (n_slots, KVH, s_max // 64, 128, 64)
    run_varlen(L, case, plan, True, s_max * 128, (s_max // 64) * 128 * 64, f"prefill {family} H={H} KVH={KVH} q_block={q_block}")


# ----------------------------------------------------------------------------- decode: split-KV partials and their merges
@pytest.mark.parametrize("H,KVH", AA.DECODE_HEADS)
@pytest.mark.parametrize("family", AA.FAMILIES)
@pytest.mark.parametrize("entry", ["slots", "rows"])
def test_decode_softmax_arithmetic(L, entry, family, H, KVH):
    """kr_attn_decode_slots / kr_attn_decode_rows (the caches permuted behind row_slot) + kr_attn_decode_merge at 1, 4, 8, 16 and 32
    splits: all five merge instantiations, 8-, 4- and 2-wave workgroups; l from the rounded P, eager alpha per unit, the merge of
    the waves through LDS, the merge of the records (two of them 150 log2 units apart, splits without a unit).  The finished row's
    records — what the attention launch writes — must keep their poison; the merge launch has no finished flag and nothing reads what
    it makes of them."""
    case = AA.cached("decode", family, H, KVH)
    B, hd, s_max = len(case.ctx), 128, case.s_max
    assert case.k.shape == (B, KVH, s_max, 128) and case.vt.shape == (B, KVH, s_max // 64, 128, 64)
    q_d, ctx_d, fin_d = dev_bf16(case.q), t_(case.ctx), t_(case.finished)
    if entry == "rows":
        row_slot = np.roll(np.arange(B, dtype=np.int32), 2)[::-1].copy()          # 3 2 1 0 5 4: no row keeps its own slot
        assert sorted(row_slot) == list(range(B)) and (row_slot != np.arange(B)).all()
        kc, vc = np.zeros_like(case.k), np.zeros_like(case.vt)
        kc[row_slot], vc[row_slot] = case.k, case.vt
        k_d, vt_d, rs_d = dev_bf16(kc), dev_bf16(vc), t_(row_slot)
    else:
        k_d, vt_d = dev_bf16(case.k), dev_bf16(case.vt)
    for n_split in AA.DECODE_SPLITS:
        ws = torch.full((B * H * n_split * (hd + 4),), 9.0, dtype=torch.float32, device=DEV)
        o_d = out_buffer(B, H * hd)
        if entry == "rows":
            L.kr_attn_decode_rows(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(rs_d), ptr(ws), B, H, KVH, hd, s_max, n_split,
                                  hd ** -0.5, 0)
        else:
            L.kr_attn_decode_slots(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, 0)
        rec = ws.cpu().numpy().reshape(B, -1)
        for b in np.flatnonzero(case.finished):
            assert (rec[b] == 9.0).all(), f"row {b} is finished: its records are not to be written (n_split={n_split})"
        for b in np.flatnonzero(case.finished == 0):
            assert np.isfinite(rec[b]).all() and not (rec[b].reshape(-1, hd + 4)[:, :hd + 2] == 9.0).all(1).any(), \
                f"row {b}: a record was left unwritten (n_split={n_split})"
        L.kr_attn_decode_merge(ptr(ws), o_d.ptr, B, H, hd, n_split, 0)
        what = f"decode {entry} {family} H={H} KVH={KVH} n_split={n_split}"
        got = values(o_d.read())
        o_d.assert_untouched(what)
        judge(got, case, what)


@pytest.mark.parametrize("family", AA.FAMILIES)
@pytest.mark.parametrize("H,KVH", AA.DECODE_HEADS)
def test_decode_merge32_softmax_arithmetic(L, H, KVH, family):
    """A batch of 21 rows (the five contexts and the finished row, repeated): kr_attn_decode_slots + kr_attn_decode_merge32, which
    writes the packed XP layout; the rows past the batch stay as they were."""
    case = AA.cached("decode", family, H, KVH, AA.DECODE_BATCH32)
    B, hd, s_max = len(case.ctx), 128, case.s_max
    assert B == 21
    q_d, k_d, vt_d, ctx_d, fin_d = dev_bf16(case.q), dev_bf16(case.k), dev_bf16(case.vt), t_(case.ctx), t_(case.finished)
    for n_split in AA.DECODE_SPLITS:
        ws = torch.full((B * H * n_split * (hd + 4),), 9.0, dtype=torch.float32, device=DEV)
        pk = out_buffer(1, 32 * H * hd)
        L.kr_attn_decode_slots(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, 0)
        rec = ws.cpu().numpy().reshape(B, -1)
        for b in np.flatnonzero(case.finished):
            assert (rec[b] == 9.0).all(), f"row {b} is finished: its records are not to be written (n_split={n_split})"
        L.kr_attn_decode_merge32(ptr(ws), pk.ptr, B, H, hd, n_split, 0)
        what = f"decode merge32 {family} H={H} KVH={KVH} n_split={n_split}"
        bits = unpack_rows32(pk.read().reshape(-1), H * hd)
        pk.assert_untouched(what)
        assert (bits[B:] == POISON_OUT["bf16"]).all(), f"{what}: rows past the batch were written"
        judge(values(bits[:B]), case, what)
