"""kr_kv_absmax (--calculate-kv-scales) against the numpy rule of tests/kv_scales_ref.py, through the C-ABI on a real MI355X.  A
maximum does not depend on order, so every comparison is bit for bit: the extremum at the borders of the pieces, poison (9984, NaN,
inf) everywhere the kernel must not look, non-finite values where it does look, the reuse of `work`, more pieces than the grid
holds, the composition with kr_kv_quantize on one stream, and the host-side refusals."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError, kv8, kvq_plan, lib, ptr  # noqa: E402
from karanta_ocr_amd.weights import bf16_round, fp8_e4m3_to_f32  # noqa: E402
from tests import kv_fp8_ref as R  # noqa: E402
from tests import kv_scales_ref as S  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
KVH, HD, SLOTS, S_MAX = 2, 128, 4, 192
PLAN = [(2, 1), (0, 64), (3, 65), (1, 130)]           # the issue's lengths, the slots in no order
PLAN_WITHOUT_SLOT_0 = [(3, 65), (1, 130), (2, 1)]     # slot 0 is poison from end to end
PLAN_HALVES = [(1, 40), (3, 100), (0, 130), (2, 1)]   # len - 1 in the SECOND 32-key half of a partial V^T block (keys 39 and 99)
POISON = np.asarray([9984.0, np.nan, np.inf, -9984.0, -np.inf], F32)
PEAK = 77.0


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def scratch(plan, seed, slots=SLOTS, s_max=S_MAX, size=3.0):
    """Token-major k, v [slots, KVH, s_max, 128]: bf16 values of a few units in rows [0, len) of the plan's slots, POISON in every
    other element — the rows at or beyond len (so also the V^T tail of a slot's last block) and the slots outside the plan."""
    rng = np.random.default_rng(seed)
    shape = (slots, KVH, s_max, HD)
    k = np.resize(POISON, shape).copy()
    v = np.resize(np.roll(POISON, 2), shape).copy()
    for slot, n in plan:
        k[slot, :, :n] = bf16_round((rng.standard_normal((KVH, n, HD)) * size).astype(F32))
        v[slot, :, :n] = bf16_round((rng.standard_normal((KVH, n, HD)) * size * 0.01).astype(F32))
    return k, v


def absmax(L, k, v, plan, k_range=S.K_RANGE, v_range=S.V_RANGE, work=None, slots=SLOTS, s_max=S_MAX):
    """(scale_out [2, KVH] as written by the device, work after the call, the device tensors of the scratch)."""
    k_d, vt_d = dev_bf16(k), dev_bf16(R.vt_blocks8(v))
    out = torch.full((2, KVH), 7.0, dtype=torch.float32, device=DEV)
    work = torch.zeros(2 * KVH, dtype=torch.int32, device=DEV) if work is None else work
    L.kr_kv_absmax(ptr(k_d), ptr(vt_d), KVH, HD, slots, s_max, kvq_plan(plan), k_range, v_range, ptr(out), ptr(work), 0)
    return host(out), work, (k_d, vt_d)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(np.asarray(got, F32).view(np.uint32), np.asarray(want, F32).view(np.uint32), err_msg=what)


# ----------------------------------------------------------------------------- where the extremum sits
def positions(plan):
    """(name, [(which, head, plan row, token, channel, value)]): per case one planted extremum per (K | V, head), four in all."""
    last = [(f"last valid row of plan row {r} (len {n})",
             [(0, 0, r, n - 1, 127, PEAK), (0, 1, r, n - 1, 0, -PEAK), (1, 0, r, n - 1, 127, -PEAK), (1, 1, r, n - 1, 64, PEAK)])
            for r, (_, n) in enumerate(plan)]
    first = ("first element", [(0, 0, 0, 0, 0, PEAK), (0, 1, 0, 0, 0, PEAK), (1, 0, 0, 0, 0, PEAK), (1, 1, 0, 0, 0, -PEAK)])
    r130 = max(range(len(plan)), key=lambda r: plan[r][1])
    inner = ("a 32-key border inside a block", [(0, 0, r130, 31, 5, -PEAK), (0, 1, r130, 32, 6, PEAK), (1, 0, r130, 95, 7, PEAK), (1, 1, r130, 96, 8, -PEAK)])
    return [first, inner] + last


@pytest.mark.parametrize("plan", [PLAN, PLAN_WITHOUT_SLOT_0, PLAN_HALVES], ids=["four-slots", "slot-0-left-out", "second-halves"])
def test_the_extremum_is_found_wherever_it_sits_and_poison_never_counts(L, plan):
    """PLAN: lengths 1, 64, 65, 130 — a partial piece of one row (65), of two (130), a full one (64), a single token; the V key
    len - 1 is the first key of a block's first half (65), its second (130), the last of a full block (64).  PLAN_HALVES adds
    len - 1 in the second half of a partial block.  The extremum is planted, with either sign, in the first element, on both sides
    of a 32-key border, and in the last valid K row / V key of every plan row; right behind it — K row len, V key len, the rest of
    the last V^T block, the slots outside the plan — lies 9984, NaN and inf.  scale_out equals the rule's bits, which here are
    77 / range for all four (K | V, head)."""
    k0, v0 = scratch(plan, 21 + len(plan))
    for name, plants in positions(plan):
        k, v = k0.copy(), v0.copy()
        for which, h, r, tok, d, val in plants:
            (k, v)[which][plan[r][0], h, tok, d] = val
        got, work, _ = absmax(L, k, v, plan)
        want = S.scales_kv(k, v, plan)
        same_bits(want, [[F32(PEAK) / F32(200.0)] * KVH, [F32(PEAK) / F32(100.0)] * KVH], name + ": the planted value is the extremum")
        same_bits(got, want, name)
        assert not host(work).any(), name + ": work is zero again"
    # without a plant: every head has an extremum of its own, somewhere inside
    got, _, _ = absmax(L, k0, v0, plan)
    want = S.scales_scratch(k0, R.vt_blocks8(v0), plan)
    assert len(set(want.reshape(-1).tolist())) == 2 * KVH
    same_bits(got, want, "no plant")


def test_non_finite_values_inside_the_valid_region_are_skipped(L):
    k, v = scratch(PLAN, 5)
    rng = np.random.default_rng(6)
    for x in (k, v):
        for slot, n in PLAN:
            m = rng.random((KVH, n, HD)) < 0.05
            x[slot, :, :n][m] = np.resize(np.asarray([np.nan, np.inf, -np.inf], F32), int(m.sum()))
    k[3, 0, 64], v[1, 1, 129] = np.inf, np.nan                                 # a whole last row / last key of nothing finite
    got, work, _ = absmax(L, k, v, PLAN)
    want = S.scales_kv(k, v, PLAN)
    assert np.isfinite(want).all() and (want < 1).all()
    same_bits(got, want)
    # a head with nothing finite, and a head of zeros: 1.0
    k[:, 0], v[:, 1] = np.nan, 0.0
    v[1, 1, 3, 3] = -0.0
    got, _, _ = absmax(L, k, v, PLAN)
    same_bits(got, S.scales_kv(k, v, PLAN))
    assert got[0, 0] == 1.0 and got[1, 1] == 1.0 and got[0, 1] != 1.0
    # the FLT_MIN floor, and a range of one's own
    k2, v2 = scratch(PLAN, 8)
    k2[[s for s, _ in PLAN], 1] = 0.0
    k2[1, 1, 100, 77] = -(2.0 ** -126)
    got, _, _ = absmax(L, k2, v2, PLAN, k_range=448.0, v_range=12.5)
    same_bits(got, S.scales_kv(k2, v2, PLAN, 448.0, 12.5))
    assert got[0, 1] == S.FLT_MIN


def test_work_is_zero_afterwards_and_carries_nothing_into_the_next_call(L):
    k, v = scratch(PLAN, 31)
    got, work, _ = absmax(L, k, v, PLAN)
    same_bits(got, S.scales_kv(k, v, PLAN))
    assert work.dtype == torch.int32 and not host(work).any()
    ks, vs = k * F32(0.125), v * F32(0.125)                                    # exact in bf16; every maximum is 8 times smaller
    got2, work, _ = absmax(L, ks, vs, PLAN, work=work)
    want2 = S.scales_kv(ks, vs, PLAN)
    same_bits(got2, want2, "a second call through the same work")
    assert (got2 < got).all() and not host(work).any()


def test_more_pieces_than_the_grid_holds(L):
    """32 slots of 1088 tokens: 32 x 2 heads x (K | V) x 17 = 2176 pieces, more than any grid cap in this file (512; the quantiser's
    2048).  The extrema sit in the last piece of the last plan row and in a piece in the middle."""
    slots, s_max = 32, 1088
    g = torch.Generator().manual_seed(3)
    shape = (slots, KVH, s_max, HD)
    k = torch.randn(shape, generator=g).to(torch.bfloat16).float().numpy()
    v = (torch.randn(shape, generator=g) * 0.01).to(torch.bfloat16).float().numpy()
    plan = [(int(s), s_max) for s in np.random.default_rng(4).permutation(slots)]
    last = plan[-1][0]
    k[last, 1, s_max - 1, 127], v[last, 0, s_max - 1, 127] = -PEAK, PEAK
    k[plan[15][0], 0, 500, 3], v[plan[16][0], 1, 600, 9] = PEAK, -PEAK
    got, work, _ = absmax(L, k, v, plan, slots=slots, s_max=s_max)
    want = S.scales_kv(k, v, plan)
    same_bits(want, [[F32(PEAK) / F32(200.0)] * KVH, [F32(PEAK) / F32(100.0)] * KVH])
    same_bits(got, want)
    assert not host(work).any()


# ----------------------------------------------------------------------------- with the quantiser behind it
def test_absmax_then_quantize_on_one_stream(L):
    """kr_kv_absmax writes a row of the table, kr_kv_quantize right behind it on the same stream reads that row as dst->scale: the
    codes are quantize(x, reference scale), nothing clamps, and no byte outside the plan's rows is written."""
    k, v = scratch(PLAN_WITHOUT_SLOT_0, 41, size=30.0)
    plan = PLAN_WITHOUT_SLOT_0
    vt = R.vt_blocks8(v)
    k_d, vt_d = dev_bf16(k), dev_bf16(vt)
    table = torch.full((3, 2, KVH), 7.0, dtype=torch.float32, device=DEV)      # the row in the middle is this layer's
    work = torch.zeros(2 * KVH, dtype=torch.int32, device=DEV)
    k8 = torch.full(k.shape, R.SENTINEL, dtype=torch.uint8, device=DEV)
    vt8 = torch.full(vt.shape, R.SENTINEL, dtype=torch.uint8, device=DEV)
    nc = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.kr_kv_absmax(ptr(k_d), ptr(vt_d), KVH, HD, SLOTS, S_MAX, kvq_plan(plan), S.K_RANGE, S.V_RANGE, ptr(table[1]), ptr(work), 0)
    L.kr_kv_quantize(ptr(k_d), ptr(vt_d), kv8(ptr(k8), ptr(vt8), ptr(table[1])), KVH, HD, SLOTS, S_MAX, kvq_plan(plan), ptr(nc), 0)
    sc = S.scales_kv(k, v, plan)
    tab = host(table)
    same_bits(tab[1], sc)
    assert (tab[0] == 7.0).all() and (tab[2] == 7.0).all()
    want_k = np.full(k.shape, R.SENTINEL, np.uint8)
    want_vt = np.full(vt.shape, R.SENTINEL, np.uint8)
    for slot, n in plan:
        nb = (n + 63) // 64
        ck, fk = R.quantize(k[slot, :, :n], sc[0][:, None, None])
        assert not fk.any()
        want_k[slot, :, :n] = ck
        # whole V^T blocks are converted; the keys at or beyond len are stale either way (the comparison covers the keys below len)
        cv, fv = R.quantize(v[slot, :, :n], sc[1][:, None, None])
        assert not fv.any()
        got_v = S.vt_to_tokens(host(vt8)[slot])[:, :n]
        np.testing.assert_array_equal(got_v, cv)
        want_vt[slot, :, :nb] = host(vt8)[slot, :, :nb]
    np.testing.assert_array_equal(host(k8), want_k)                            # K rows at or beyond len, slot 0: sentinels
    np.testing.assert_array_equal(host(vt8), want_vt)                          # V^T blocks beyond the last, slot 0: sentinels
    top = np.max([np.abs(fp8_e4m3_to_f32(host(k8)[slot, :, :n])).max(axis=(1, 2)) for slot, n in plan], axis=0)
    assert ((top == 192) | (top == 208)).all(), top                            # every head's extremum sits next to 200
    # n_clamped counts the stale keys of the last V^T blocks too (9984 and inf lie there); on finite stale data, as in the engine,
    # it stays 0: the same two launches over a scratch whose tail is ordinary data
    kf, vf = np.where(np.isfinite(k), k, F32(1.0)), np.where(np.isfinite(v), v, F32(0.01))
    kf, vf = np.clip(kf, -40, 40), np.clip(vf, -0.375, 0.375)                  # both bounds are bf16 values
    k_d, vt_d = dev_bf16(kf), dev_bf16(R.vt_blocks8(vf))
    nc.zero_()
    L.kr_kv_absmax(ptr(k_d), ptr(vt_d), KVH, HD, SLOTS, S_MAX, kvq_plan(plan), S.K_RANGE, S.V_RANGE, ptr(table[1]), ptr(work), 0)
    L.kr_kv_quantize(ptr(k_d), ptr(vt_d), kv8(ptr(k8), ptr(vt8), ptr(table[1])), KVH, HD, SLOTS, S_MAX, kvq_plan(plan), ptr(nc), 0)
    same_bits(host(table)[1], S.scales_kv(kf, vf, plan))
    assert int(host(nc)[0]) == 0 and not host(work).any()


# ----------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(L):
    k, v = scratch(PLAN, 51)
    k_d, vt_d = dev_bf16(k), dev_bf16(R.vt_blocks8(v))
    out = torch.full((2, KVH), 7.0, dtype=torch.float32, device=DEV)
    work = torch.full((2 * KVH,), 0x1234, dtype=torch.int32, device=DEV)
    ok = dict(k=ptr(k_d), vt=ptr(vt_d), kvh=KVH, hd=HD, slots=SLOTS, s_max=S_MAX, plan=PLAN, kr=200.0, vr=100.0, out=ptr(out), work=ptr(work))
    bad = [("null pointer", dict(k=0)), ("null pointer", dict(vt=0)), ("null pointer", dict(out=0)), ("null pointer", dict(work=0)),
           ("null pointer", dict(plan=None)),
           ("head_dim 128", dict(hd=64)), ("bad geometry", dict(kvh=0)), ("bad geometry", dict(kvh=65)), ("bad geometry", dict(s_max=200)),
           ("bad geometry", dict(slots=33)),
           ("outside", dict(plan=[(4, 5)])), ("listed twice", dict(plan=[(1, 5), (1, 6)])), ("len 0", dict(plan=[(0, 0)])),
           ("len 193", dict(plan=[(0, S_MAX + 1)])), ("plan rows", dict(plan=[])), ("plan rows", dict(plan=[(0, 1)] * 33)),
           ("aligned", dict(k=ptr(k_d) + 2)), ("aligned", dict(vt=ptr(vt_d) + 8))]
    for r in (0.0, -1.0, float("nan"), float("inf")):
        bad += [("finite and positive", dict(kr=r)), ("finite and positive", dict(vr=r))]
    for match, change in bad:
        a = {**ok, **change}
        with pytest.raises(KarantaHipError, match=match):
            L.kr_kv_absmax(a["k"], a["vt"], a["kvh"], a["hd"], a["slots"], a["s_max"], None if a["plan"] is None else kvq_plan(a["plan"]),
                           a["kr"], a["vr"], a["out"], a["work"], 0)
        rc = L.kr_kv_absmax.raw(a["k"], a["vt"], a["kvh"], a["hd"], a["slots"], a["s_max"], None if a["plan"] is None else kvq_plan(a["plan"]),
                                a["kr"], a["vr"], a["out"], a["work"], 0)
        assert rc < 0, change
    assert (host(out) == 7.0).all() and (host(work) == 0x1234).all()
