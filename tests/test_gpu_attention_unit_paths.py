"""The decode attention's bodies by units per wave (attn_decode2_kernel branches once on a part's unit count: none, one, two,
three or more), on the one-winner inputs of tests/attn_patterns.py: the expected output is a stored V row, built on the CPU, so a
body that drops, repeats or mis-orders a unit, reads a key at or past the context, or lets a stale V^T column in returns a
DIFFERENT row and fails by >= 1/15 relative.

Geometry: one split of 8 waves = 8 parts (kr_attn_decode_slots with n_split = 1 writes the one record per head that
kr_attn_decode_merge then normalises), and two splits of 8 waves = 16 parts.  With K keys a slot has ceil(K / 32) units, part p
takes units p, p + 8, ...: the key counts 1 .. 1000 below give 8-part waves with 0, 1, 2, 3 and 4 units, whole and ragged last
units in the first, second and later position (asserted in test_the_contexts_reach_every_body).  The tents put the winner into
the first, second, third and fourth unit of part 0 and next to the unit borders; `up` lets every row past the context outrank
the winner (V^T there holds the stale value), `down` makes key 0 win.  Two slots are finished: their records stay as they were.
bf16 cache and fp8 cache (kr_attn_decode_slots_kv8).  Through the C-ABI, on a real MI355X."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import kv8, lib, ptr  # noqa: E402
from tests import attn_patterns as AP  # noqa: E402

DEV = "cuda:0"
HD, REC = 128, 132
S_MAX = 1024
KEYS = [1, 31, 32, 33, 255, 256, 257, 288, 511, 512, 513, 600, 769, 1000]       # keys a slot's query sees (ctx_len + 1)
# (ctx_len, finished): the two finished slots sit among the live ones, one of them with a context that would take the 3-unit body
BATCH = [(k - 1, 0) for k in KEYS[:5]] + [(700, 1)] + [(k - 1, 0) for k in KEYS[5:]] + [(40, 1)]
# winners in unit 0, 1, 7, 8 (part 0's second), 9, 15, 16 (part 0's third), 24 (its fourth) and on the last visible keys
PATTERNS = ["up", "down"] + [f"tent-{p}" for p in (0, 31, 32, 255, 256, 287, 288, 511, 512, 543, 768, 799, "ctx-1", "ctx")]
HEADS = [(12, 2), (28, 4)]
SPLITS = [1, 2]                     # x 8 waves: 8 and 16 parts


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def t_(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t: torch.Tensor) -> np.ndarray:
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def units_per_part(keys: int, parts: int):
    nu = (keys + 31) // 32
    return [len(range(p, nu, parts)) for p in range(parts)]


def test_the_contexts_reach_every_body():
    """The claim of the module docstring about KEYS, from the kernel's deal of units to parts (no device work)."""
    counts, ragged_at = set(), set()
    for k in KEYS:
        per = units_per_part(k, 8)
        counts.update(per)
        if k % 32:                      # the last unit is ragged: which unit of its part is it?
            nu = (k + 31) // 32
            ragged_at.add(min((nu - 1) // 8, 2))
    assert counts == {0, 1, 2, 3, 4}
    assert ragged_at == {0, 1, 2}       # first, second and a later unit of a wave
    assert {max(units_per_part(k, 16)) for k in KEYS} >= {1, 2}
    assert sum(f for _, f in BATCH) == 2 and max(c for c, _ in BATCH) < S_MAX


def check_records(ws, case, n_split, what):
    rec = host(ws).reshape(len(case.ctx), -1)
    for b, fin in enumerate(case.finished):
        if fin:
            assert (rec[b] == 9.0).all(), f"{what}: slot {b} is finished, its records are not to be written (n_split={n_split})"
        else:
            assert np.isfinite(rec[b]).all() and not (rec[b].reshape(-1, REC)[:, :HD + 2] == 9.0).all(1).any(), \
                f"{what}: slot {b}: a record was left unwritten (n_split={n_split})"


@pytest.mark.parametrize("H,KVH", HEADS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_bf16_bodies_return_the_winning_key(L, H, KVH, pattern):
    case = AP.decode_case(BATCH, H, KVH, pattern, s_max=S_MAX)
    B = len(case.ctx)
    assert case.k.shape == (B, KVH, S_MAX, HD) and case.vt.shape == (B, KVH, S_MAX // 64, HD, 64)
    q_d, k_d, vt_d, ctx_d, fin_d = dev_bf16(case.q), dev_bf16(case.k), dev_bf16(case.vt), t_(case.ctx), t_(case.finished)
    for n_split in SPLITS:
        what = f"bf16 {pattern} H={H} KVH={KVH} n_split={n_split}"
        ws = torch.full((B * H * n_split * REC,), 9.0, dtype=torch.float32, device=DEV)
        o_d = torch.full((B, H * HD), -7.0, dtype=torch.bfloat16, device=DEV)
        L.kr_attn_decode_slots(ptr(q_d), ptr(k_d), ptr(vt_d), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, HD, S_MAX, n_split, HD ** -0.5, 0)
        L.kr_attn_decode_merge(ptr(ws), ptr(o_d), B, H, HD, n_split, 0)
        check_records(ws, case, n_split, what)
        AP.check_output(host(o_d), case, what)


@pytest.mark.parametrize("H,KVH", HEADS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_fp8_bodies_return_the_winning_key(L, H, KVH, pattern):
    case = AP.decode_case_kv8(BATCH, H, KVH, pattern, "odd", s_max=S_MAX)
    B = len(case.ctx)
    assert case.k_codes.shape == (B, KVH, S_MAX, HD) and case.vt.shape == (B, KVH, S_MAX // 64, 2, HD, 32)
    q_d, k_d, vt_d, sc_d = dev_bf16(case.q), t_(case.k_codes), t_(case.vt), t_(case.scales)
    ctx_d, fin_d = t_(case.ctx), t_(case.finished)
    for n_split in SPLITS:
        what = f"fp8 {pattern} H={H} KVH={KVH} n_split={n_split}"
        ws = torch.full((B * H * n_split * REC,), 9.0, dtype=torch.float32, device=DEV)
        o_d = torch.full((B, H * HD), -7.0, dtype=torch.bfloat16, device=DEV)
        L.kr_attn_decode_slots_kv8(ptr(q_d), kv8(ptr(k_d), ptr(vt_d), ptr(sc_d)), ptr(ctx_d), ptr(fin_d), ptr(ws), B, H, KVH, HD, S_MAX,
                                   n_split, HD ** -0.5, 0)
        L.kr_attn_decode_merge(ptr(ws), ptr(o_d), B, H, HD, n_split, 0)
        check_records(ws, case, n_split, what)
        AP.check_output(host(o_d), case, what)
