"""The kernels of the fp8 (e4m3fn) KV cache against the numpy rule of tests/kv_fp8_ref.py, through the C-ABI on a real MI355X:
kr_kv_quantize (byte-exact, nothing else written, the clamp count), the ROPE_KV8 append of the <= 16-row and the 17..32-row qkv
launches (the codes of exactly the bf16 values the bf16 launch stores, q bit for bit, every other byte untouched), the decode
attention on fp8 operands with the existing merges (within attn_arith's bound on the dequantised operands, and an independent
needle check of the operand mapping), and the byte-sized fork.  The bound and the needle do not see a one-key masking, unit or
key-order error of the fp8 attention (a flat softmax over 1100 keys moves by 1/1100): test_gpu_attention_exact_kv8.py holds the
to-the-key checks — one winner per query in an e4m3-exact encoding, at every unit border, behind the row map, with per-head scales."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import DEC_ROPE_KV, Dec32, KarantaHipError, fork_plan, kv8, kvq_plan, lib, ptr  # noqa: E402
from karanta_ocr_amd.weights import bf16_round, pack_rows32, pack_w16x64, unpack_rows32  # noqa: E402
from tests import attn_arith as AA  # noqa: E402
from tests import kv_fp8_ref as R  # noqa: E402

DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def rnd(rng, *shape, scale=1.0):
    return bf16_round(rng.standard_normal(shape).astype(F32) * F32(scale))


# ----------------------------------------------------------------------------- kr_kv_quantize
@pytest.mark.parametrize("scale", [1.0, 0.37, 2.0 ** -3])
def test_kv_quantize_is_the_numpy_rule_byte_for_byte(L, scale):
    """Five prompts of 1, 63, 64, 65 and 130 tokens in the odd slots of a ten-slot layer (no two adjacent), two kv heads with scales
    of their own; the inputs carry the edge values of the format and values beyond 448 x scale.  K rows at or beyond a prompt's
    length, the even slots and the scratch keep their bytes; n_clamped is the numpy count."""
    rng = np.random.default_rng(7)
    KVH, hd, slots, s_max = 2, 128, 10, 192
    plan = [(9, 1), (1, 63), (3, 64), (5, 65), (7, 130)]
    sc = np.asarray([[scale, scale * 2], [scale * 0.5, scale]], F32)          # [K | V][kv head]
    k = rnd(rng, slots, KVH, s_max, hd, scale=150.0 * scale)
    vt = rnd(rng, slots, KVH, s_max // 64, 2, hd, 32, scale=150.0 * scale)
    edges = bf16_round(R.EDGES * F32(scale))
    k[:, :, 0, :edges.size] = edges
    vt[:, :, 0, 0, :edges.size, 0] = edges
    k_d, vt_d, sc_d = dev_bf16(k), dev_bf16(vt), t_(sc)
    k8 = torch.full(k.shape, R.SENTINEL, dtype=torch.uint8, device=DEV)
    vt8 = torch.full(vt.shape, R.SENTINEL, dtype=torch.uint8, device=DEV)
    nc = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.kr_kv_quantize(ptr(k_d), ptr(vt_d), kv8(ptr(k8), ptr(vt8), ptr(sc_d)), KVH, hd, slots, s_max, kvq_plan(plan), ptr(nc), 0)
    want_k = np.full(k.shape, R.SENTINEL, np.uint8)
    want_vt = np.full(vt.shape, R.SENTINEL, np.uint8)
    n_clamped = 0
    for slot, n in plan:
        nb = (n + 63) // 64
        ck, fk = R.quantize(k[slot, :, :n], sc[0][:, None, None])
        cv, fv = R.quantize(vt[slot, :, :nb], sc[1][:, None, None, None, None])
        want_k[slot, :, :n], want_vt[slot, :, :nb] = ck, cv
        n_clamped += int(fk.sum()) + int(fv.sum())
    assert n_clamped > 50
    np.testing.assert_array_equal(host(k8), want_k)
    np.testing.assert_array_equal(host(vt8), want_vt)
    assert int(host(nc)[0]) == n_clamped
    np.testing.assert_array_equal(host(k_d), k)                                 # the scratch is read only
    # without a counter: the same bytes
    k8b, vt8b = torch.full_like(k8, R.SENTINEL), torch.full_like(vt8, R.SENTINEL)
    L.kr_kv_quantize(ptr(k_d), ptr(vt_d), kv8(ptr(k8b), ptr(vt8b), ptr(sc_d)), KVH, hd, slots, s_max, kvq_plan(plan), 0, 0)
    assert torch.equal(k8b, k8) and torch.equal(vt8b, vt8)
    for bad in ([(10, 5)], [(1, 5), (1, 6)], [(0, 0)], [(0, s_max + 1)], []):
        with pytest.raises(KarantaHipError):
            L.kr_kv_quantize(ptr(k_d), ptr(vt_d), kv8(ptr(k8), ptr(vt8), ptr(sc_d)), KVH, hd, slots, s_max, kvq_plan(bad), 0, 0)
    with pytest.raises(KarantaHipError, match="head_dim 128"):
        L.kr_kv_quantize(ptr(k_d), ptr(vt_d), kv8(ptr(k8), ptr(vt8), ptr(sc_d)), KVH, 64, slots, s_max, kvq_plan(plan), 0, 0)


# ----------------------------------------------------------------------------- the ROPE_KV8 append
POSITIONS = [64, 31, 32, 63, 65, 0, 198, 130, 33, 95, 96, 127, 128, 1, 191, 192]


def append_inputs(H, KVH, K, M, slots, seed):
    rng = np.random.default_rng(seed)
    hd, s_max, T = 128, 256, 7
    N = (H + 2 * KVH) * hd
    d = dict(hd=hd, s_max=s_max, T=T, N=N)
    d["x"], d["W"] = rnd(rng, M, K, scale=2.0), rnd(rng, N, K, scale=K ** -0.5)
    d["bias"], d["nw"] = rnd(rng, N, scale=0.1), bf16_round(1 + 0.1 * rnd(rng, K))
    d["p"] = (rng.standard_normal((2, M, K)) * 0.5).astype(F32)
    ang = rng.uniform(0, 6.28, size=(slots, T, 64)).astype(F32)
    d["cs"] = np.concatenate([bf16_round(np.cos(ang)), bf16_round(np.sin(ang))], -1).astype(F32)
    d["kc"], d["vt"] = rnd(rng, slots, KVH, s_max, hd), rnd(rng, slots, KVH, s_max // 64, 2, hd, 32)
    d["k8"] = rng.integers(0, 0x7E, size=d["kc"].shape).astype(np.uint8)
    d["vt8"] = rng.integers(0, 0x7E, size=d["vt"].shape).astype(np.uint8)
    d["sc"] = np.stack([0.01 * (1 + np.arange(KVH)), 0.02 * (2 + np.arange(KVH))]).astype(F32)      # small scales: some values clamp
    return d


def check_append(d, KVH, ctxs, row_slot, bf16_out, kv8_out, what):
    """bf16_out / kv8_out = (q, K cache, V^T cache) after the bf16 and after the fp8-cache launch."""
    np.testing.assert_array_equal(kv8_out[0], bf16_out[0], err_msg=f"{what}: q")
    k_mask, v_mask = np.zeros(d["kc"].shape, bool), np.zeros(d["vt"].shape, bool)
    for r, c in enumerate(ctxs):
        k_mask[row_slot[r], :, c] = True
        v_mask[row_slot[r], :, c >> 6, (c & 63) >> 5, :, c & 31] = True
    assert (bf16_out[1][~k_mask] == d["kc"][~k_mask]).all() and (bf16_out[2][~v_mask] == d["vt"][~v_mask]).all()
    want_k, want_v = d["k8"].copy(), d["vt8"].copy()
    ck, _ = R.quantize(bf16_out[1], d["sc"][0][None, :, None, None])
    cv, _ = R.quantize(bf16_out[2], d["sc"][1][None, :, None, None, None, None])
    want_k[k_mask], want_v[v_mask] = ck[k_mask], cv[v_mask]
    assert (want_k[k_mask] != d["k8"][k_mask]).mean() > 0.9                        # the append is visible
    np.testing.assert_array_equal(kv8_out[1], want_k, err_msg=f"{what}: K codes")
    np.testing.assert_array_equal(kv8_out[2], want_v, err_msg=f"{what}: V^T codes")


@pytest.mark.parametrize("H,KVH,K,parts", [(12, 2, 1536, True), (28, 4, 3584, False)])
@pytest.mark.parametrize("M", [1, 16])
def test_narrow_append_writes_the_codes_of_the_bf16_launch(L, H, KVH, K, parts, M):
    """kr_linear_decode_narrow(ROPE_KV) and kr_linear_decode_narrow_kv8 on the same inputs (the fused norm prologue, with and
    without deferred partial sums): equal q bits, and at the appended positions — on both sides of 32- and 64-key borders — the
    fp8 cache holds the rule's codes of the bf16 cache's values; no other byte of it changed."""
    d = append_inputs(H, KVH, K, M, M, 300 + H + M)
    hd, s_max, T, N = d["hd"], d["s_max"], d["T"], d["N"]
    step = (np.arange(M) % T).astype(np.int32)
    ctxs = np.asarray(POSITIONS[:M], np.int32)
    plen = np.maximum(ctxs - step, 0).astype(np.int32)
    ctxs = plen + step
    xd, Wd, bd, nd, pd = dev_bf16(d["x"]), dev_bf16(pack_w16x64(d["W"])), dev_bf16(d["bias"]), dev_bf16(d["nw"]), t_(d["p"])
    cs_d, ctx_d, pl_d, sc_d = t_(d["cs"]), t_(ctxs), t_(plen), t_(d["sc"])
    out = {}
    for form in ("bf16", "kv8"):
        q_d = torch.zeros(M, H, hd, dtype=torch.bfloat16, device=DEV)
        xo = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        if form == "bf16":
            kc_d, vt_d = dev_bf16(d["kc"]), dev_bf16(d["vt"])
            L.kr_linear_decode_narrow(DEC_ROPE_KV, ptr(xd), K, ptr(pd) if parts else 0, 2 if parts else 0, ptr(xo) if parts else 0, K, ptr(Wd),
                                      ptr(bd), ptr(nd), 1e-6, 0, 0, 0, 0, 0, M, N, K, 8, 1, ptr(cs_d), T, ptr(pl_d), ptr(ctx_d), ptr(q_d),
                                      ptr(kc_d), ptr(vt_d), H, KVH, s_max, None, 0)
        else:
            kc_d, vt_d = t_(d["k8"]), t_(d["vt8"])
            L.kr_linear_decode_narrow_kv8(ptr(xd), K, ptr(pd) if parts else 0, 2 if parts else 0, ptr(xo) if parts else 0, K, ptr(Wd), 0,
                                          ptr(bd), ptr(nd), 1e-6, M, N, K, 8, ptr(cs_d), T, ptr(pl_d), ptr(ctx_d), ptr(q_d),
                                          kv8(ptr(kc_d), ptr(vt_d), ptr(sc_d)), H, KVH, s_max, None, 0)
        out[form] = (host(q_d), host(kc_d), host(vt_d), host(xo))
    np.testing.assert_array_equal(out["kv8"][3], out["bf16"][3], err_msg="x_out")
    check_append(d, KVH, ctxs, np.arange(M), out["bf16"], out["kv8"], f"narrow M={M}")


@pytest.mark.parametrize("H,KVH,K,M,rows", [(12, 2, 1536, 32, False), (28, 4, 3584, 17, False), (12, 2, 1536, 20, True)])
def test_decode32_append_writes_the_codes_of_the_bf16_launch(L, H, KVH, K, M, rows):
    """kr_linear_decode32 / kr_linear_decode32_rows (ROPE_KV) and kr_linear_decode32_kv8 on the same packed rows.  rows: 20 rows
    over 10 slots, rows r and r + 10 on one slot at consecutive positions (a speculative step)."""
    slots = 10 if rows else M
    d = append_inputs(H, KVH, K, M, slots, 400 + H + M)
    hd, s_max, T, N = d["hd"], d["s_max"], d["T"], d["N"]
    row_slot = (np.arange(M) % slots).astype(np.int32)
    depth = (np.arange(M) // slots).astype(np.int32)
    base = np.asarray([POSITIONS[s % len(POSITIONS)] + (17 if s >= len(POSITIONS) else 0) for s in range(slots)], np.int32)
    step0 = (np.arange(slots) % (T - 1)).astype(np.int32)
    plen_s = np.maximum(base - step0, 0)
    ctxs = (plen_s + step0)[row_slot] + depth
    plen = plen_s[row_slot].astype(np.int32)
    assert len({(int(s), int(c)) for s, c in zip(row_slot, ctxs)}) == M and (ctxs - plen < T).all()
    hp = dev_bf16(pack_rows32(d["x"]))
    Wd, bd = dev_bf16(pack_w16x64(d["W"])), dev_bf16(d["bias"])
    cs_d, ctx_d, pl_d, sc_d, rs_d = t_(d["cs"]), t_(ctxs.astype(np.int32)), t_(plen), t_(d["sc"]), t_(row_slot)
    out = {}
    for form in ("bf16", "kv8"):
        q_d = torch.zeros(M, H, hd, dtype=torch.bfloat16, device=DEV)
        kc_d, vt_d = (dev_bf16(d["kc"]), dev_bf16(d["vt"])) if form == "bf16" else (t_(d["k8"]), t_(d["vt8"]))
        a = Dec32(ptr(hp), ptr(Wd), None, ptr(bd), None, 0, None, None, 0, M, N, K, 8, 1, 0, 0, 0, 0, None, 0, ptr(cs_d), T, ptr(pl_d),
                  ptr(ctx_d), ptr(q_d), ptr(kc_d) if form == "bf16" else None, ptr(vt_d) if form == "bf16" else None, H, KVH, s_max)
        if form == "kv8":
            L.kr_linear_decode32_kv8(C.byref(a), kv8(ptr(kc_d), ptr(vt_d), ptr(sc_d)), ptr(rs_d) if rows else 0, 0)
        elif rows:
            L.kr_linear_decode32_rows(DEC_ROPE_KV, C.byref(a), ptr(rs_d), 0)
        else:
            L.kr_linear_decode32(DEC_ROPE_KV, C.byref(a), 0)
        out[form] = (host(q_d), host(kc_d), host(vt_d))
    check_append(d, KVH, ctxs, row_slot, out["bf16"], out["kv8"], f"decode32 M={M} rows={rows}")


# ----------------------------------------------------------------------------- decode attention on fp8 operands
def run_attention(L, entry, q, k_codes, v_codes, ctx, fin, sc, H, KVH, n_split, merge32=False):
    B, hd, s_max = len(ctx), 128, k_codes.shape[2]
    q_d, ctx_d, fin_d, sc_d = dev_bf16(q), t_(ctx), t_(fin), t_(sc)
    vt = R.vt_blocks8(v_codes)
    if entry == "rows":
        row_slot = np.roll(np.arange(B, dtype=np.int32), 3)[::-1].copy()
        kc, vc = np.zeros_like(k_codes), np.zeros_like(vt)
        kc[row_slot], vc[row_slot] = k_codes, vt
        k_d, vt_d, rs_d = t_(kc), t_(vc), t_(row_slot)
    else:
        k_d, vt_d = t_(k_codes), t_(vt)
    ws = torch.full((B * H * n_split * (hd + 4),), 9.0, dtype=torch.float32, device=DEV)
    kv = kv8(ptr(k_d), ptr(vt_d), ptr(sc_d))
    if entry == "rows":
        L.kr_attn_decode_rows_kv8(ptr(q_d), kv, ptr(ctx_d), ptr(fin_d), ptr(rs_d), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, 0)
    else:
        L.kr_attn_decode_slots_kv8(ptr(q_d), kv, ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, hd, s_max, n_split, hd ** -0.5, 0)
    rec = host(ws).reshape(B, -1)
    for b in np.flatnonzero(fin):
        assert (rec[b] == 9.0).all(), f"row {b} is finished: its records are not to be written (n_split={n_split})"
    if merge32:
        pk = torch.full((32 * H * hd,), 7.0, dtype=torch.bfloat16, device=DEV)
        L.kr_attn_decode_merge32(ptr(ws), ptr(pk), B, H, hd, n_split, 0)
        return unpack_rows32(host(pk), H * hd)[:B]
    o_d = torch.full((B, H * hd), 7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_merge(ptr(ws), ptr(o_d), B, H, hd, n_split, 0)
    return host(o_d)


@pytest.fixture(scope="module")
def decode_cases():
    cache = {}

    def get(H, KVH, ks, vs):
        if (H, KVH, ks, vs) not in cache:
            cache[(H, KVH, ks, vs)] = R.decode_case(H, KVH, ks, vs)
        return cache[(H, KVH, ks, vs)]
    return get


@pytest.mark.parametrize("ks,vs", R.DECODE_SCALES)
@pytest.mark.parametrize("H,KVH", R.DECODE_HEADS)
@pytest.mark.parametrize("entry", ["slots", "rows", "merge32"])
def test_decode_attention_on_fp8_operands_meets_the_bound(L, decode_cases, entry, H, KVH, ks, vs):
    """kr_attn_decode_slots_kv8 / _rows_kv8 + kr_attn_decode_merge / _merge32 at 1, 4, 16 and 32 splits over rows of 1, 31, 32, 33,
    64, 65 and 1100 keys and one finished row: |got - o| <= E with attn_arith's reference and bound over the DEQUANTISED operands
    (the conversion is exact; the two folded scales are f32 roundings inside the bound's 2^-12).  The tail beyond a row's keys holds
    code 0x7E (448): masked, it must not move the output.  The last entry of DECODE_SCALES gives every kv head K and V scales of
    its own: kv_scale[kvh] and kv_scale[kv_heads + kvh] read for another head miss the bound (test_kv_fp8_cpu.py shows it on the model)."""
    case, k_codes, v_codes = decode_cases(H, KVH, ks, vs)
    sc = R.scale_rows(ks, vs, KVH)
    for n_split in R.DECODE_SPLITS:
        got = run_attention(L, "slots" if entry == "merge32" else entry, case.q, k_codes, v_codes, case.ctx, case.finished, sc, H, KVH,
                            n_split, merge32=entry == "merge32")
        live = case.finished == 0
        assert np.isfinite(got[live]).all()
        r, where = AA.max_ratio(got, case)
        print(f"\nfp8 decode {entry} H={H} KVH={KVH} scales=({ks}, {vs}) n_split={n_split}: max |got - o| / E = {r:.3f}")
        assert r <= 1.0, f"n_split={n_split}: |got - o| = {r:.3f} E at {where}"


@pytest.mark.parametrize("H,KVH", R.DECODE_HEADS)
def test_decode_attention_fp8_finds_the_needle(L, H, KVH):
    """The operand mapping without any reference arithmetic (kv_fp8_ref.needle_case): channel-distinct q and K, one key per row with
    q's pattern, V constant over the channels and distinct over the keys: every live output is the needle's value, bit for bit."""
    q, k_codes, v_codes, ctx, fin, _ = R.needle_case(H, KVH)
    sc = np.ones((2, KVH), F32)
    for n_split in R.DECODE_SPLITS:
        for entry in ("slots", "rows"):
            got = run_attention(L, entry, q, k_codes, v_codes, ctx, fin, sc, H, KVH, n_split)
            live = fin == 0
            assert (got[live] == R.NEEDLE_V).all(), f"{entry} n_split={n_split}: {np.unique(got[live])[:8]}"


# ----------------------------------------------------------------------------- kr_kv_fork8
def test_kv_fork8_copies_bytes(L):
    """A launch of two groups (65 tokens to three children, 64 tokens to one) and a launch that forks a single token, over 3 layers
    and 2 kv heads of one-byte elements: the spans are copied byte for byte; destination rows at or beyond the span and every other
    slot keep theirs."""
    rng = np.random.default_rng(3)
    Ln, slots, KVH, s_max, hd = 3, 8, 2, 192, 128
    k = rng.integers(0, 256, size=(Ln, slots, KVH, s_max, hd)).astype(np.uint8)
    vt = rng.integers(0, 256, size=(Ln, slots, KVH, s_max // 64, 2, hd, 32)).astype(np.uint8)
    for groups in ([(0, 65, [2, 5, 7]), (3, 64, [1])], [(4, 1, [6])]):
        k_d, vt_d = t_(k), t_(vt)
        L.kr_kv_fork8(ptr(k_d), ptr(vt_d), k_d.stride(0), k_d.stride(1), k_d.stride(2), vt_d.stride(0), vt_d.stride(1), vt_d.stride(2),
                      Ln, KVH, hd, slots, s_max, fork_plan(groups), 0)
        want_k, want_vt = k.copy(), vt.copy()
        for src, n, dst in groups:
            for j in dst:
                want_k[:, j, :, :n] = k[:, src, :, :n]
                want_vt[:, j, :, :(n + 63) // 64] = vt[:, src, :, :(n + 63) // 64]
        np.testing.assert_array_equal(host(k_d), want_k)
        np.testing.assert_array_equal(host(vt_d), want_vt)
    with pytest.raises(KarantaHipError):
        L.kr_kv_fork8(ptr(k_d), ptr(vt_d), k_d.stride(0), k_d.stride(1), k_d.stride(2), vt_d.stride(0), vt_d.stride(1), vt_d.stride(2),
                      Ln, KVH, 72, slots, s_max, fork_plan([(0, 5, [1])]), 0)
