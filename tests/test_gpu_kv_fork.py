"""kr_kv_fork against numpy, through ctypes, on int16 views: the prompt's K rows and whole V^T blocks of a source slot land in
every destination slot of its group, and NOTHING else changes — the destination beyond the span, the other slots, the source.
All claims are exact equalities of bit patterns."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import fork_plan, lib  # noqa: E402

KR_ERR_ARG = -1
LAYERS, SLOTS, HEADS, S_MAX, HD = 2, 5, 2, 256, 128


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


@pytest.fixture(scope="module")
def caches():
    """Random 16-bit patterns, made once: (kcache, vtcache) on the host; every test uploads its own copy."""
    rng = np.random.default_rng(2024)
    k = rng.integers(-32768, 32768, (LAYERS, SLOTS, HEADS, S_MAX, HD), dtype=np.int16)
    v = rng.integers(-32768, 32768, (LAYERS, SLOTS, HEADS, S_MAX // 64, HD, 64), dtype=np.int16)
    return k, v


def fork(L, k, v, groups, slots=SLOTS, s_max=S_MAX, raw=False):
    fn = L.kr_kv_fork.raw if raw else L.kr_kv_fork
    rc = fn(k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
            k.shape[0], k.shape[2], k.shape[4], slots, s_max, fork_plan(groups), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def expected(k, v, groups):
    ek, ev = k.copy(), v.copy()
    for src, n, dsts in groups:
        for d in dsts:
            ek[:, d, :, :n] = k[:, src, :, :n]
            ev[:, d, :, :(n + 63) // 64] = v[:, src, :, :(n + 63) // 64]
    return ek, ev


# every n_tokens of {1, 63, 64, 65, 200, 256}: one row, both sides of a V^T block boundary, a span that ends inside the
# fourth block, the whole slot; a group with three destinations; a plan with two groups of different lengths
PLANS = {
    "1": [(2, 1, [0])],
    "63": [(0, 63, [4])],
    "64": [(1, 64, [0, 2])],
    "65-three-destinations": [(0, 65, [2, 3, 4])],
    "200+63-two-groups": [(0, 200, [1, 2]), (4, 63, [3])],
    "256": [(3, 256, [1])],
    "64+1-two-groups": [(4, 64, [0]), (2, 1, [3, 1])],
}


@pytest.mark.parametrize("case", list(PLANS))
def test_fork_copies_the_span_and_nothing_else(L, caches, case):
    k0, v0 = caches
    groups = PLANS[case]
    k, v = torch.from_numpy(k0).cuda(), torch.from_numpy(v0).cuda()
    fork(L, k, v, groups)
    ek, ev = expected(k0, v0, groups)
    gk, gv = k.cpu().numpy(), v.cpu().numpy()
    for src, n, dsts in groups:     # the claim, spelled out for the first failure message; the whole-array equality below covers it
        for d in dsts:
            np.testing.assert_array_equal(gk[:, d, :, :n], k0[:, src, :, :n], err_msg=f"K rows of slot {d}")
            np.testing.assert_array_equal(gk[:, d, :, n:], k0[:, d, :, n:], err_msg=f"K rows of slot {d} beyond the span")
    np.testing.assert_array_equal(gk, ek)
    np.testing.assert_array_equal(gv, ev)


def test_fork_offsets_are_64_bit(L):
    """A layer stride above 2^31 elements: layer 1 of either cache starts beyond 4 GB.  Only the touched slices are initialised
    and compared."""
    slots, heads, s_max, n = 3, 1, 128, 100
    stride_l = 2 ** 31 + 4096
    span = s_max * HD
    total = stride_l + slots * heads * span
    rng = np.random.default_rng(7)
    k0 = rng.integers(-32768, 32768, (2, slots, heads, s_max, HD), dtype=np.int16)
    v0 = rng.integers(-32768, 32768, (2, slots, heads, s_max // 64, HD, 64), dtype=np.int16)
    kbuf = torch.empty(total, dtype=torch.int16, device="cuda")
    vbuf = torch.empty(total, dtype=torch.int16, device="cuda")
    k = kbuf.as_strided((2, slots, heads, s_max, HD), (stride_l, heads * span, span, HD, 1))
    v = vbuf.as_strided((2, slots, heads, s_max // 64, HD, 64), (stride_l, heads * span, span, HD * 64, 64, 1))
    k.copy_(torch.from_numpy(k0).cuda())
    v.copy_(torch.from_numpy(v0).cuda())
    groups = [(2, n, [0, 1])]
    fork(L, k, v, groups, slots=slots, s_max=s_max)
    ek, ev = expected(k0, v0, groups)
    gk = k.contiguous().cpu().numpy()
    np.testing.assert_array_equal(gk, ek)
    np.testing.assert_array_equal(v.contiguous().cpu().numpy(), ev)
    np.testing.assert_array_equal(gk[1, 0, :, :n], k0[1, 2, :, :n], err_msg="layer 1 starts beyond 2^31 elements")


BAD_PLANS = {
    "source-slot-too-large": [(SLOTS, 10, [0])],
    "source-slot-negative": [(-1, 10, [0])],
    "destination-slot-too-large": [(0, 10, [SLOTS])],
    "destination-slot-negative": [(0, 10, [1, -1])],
    "n_tokens-zero": [(0, 0, [1])],
    "n_tokens-above-s_max": [(0, S_MAX + 1, [1])],
    "destination-twice-in-a-group": [(0, 10, [1, 1])],
    "destination-twice-across-groups": [(0, 10, [1]), (2, 20, [3, 1])],
    "destination-is-its-source": [(0, 10, [1, 0])],
    "destination-is-another-source": [(0, 10, [1]), (2, 20, [0])],
    "empty-plan": [],
    "group-without-destinations": [(0, 10, [1]), (2, 20, [])],
    "too-many-groups": [(0, 10, [1])] * 33,
}


@pytest.mark.parametrize("case", list(BAD_PLANS))
def test_rejected_plans_return_err_arg_and_launch_nothing(L, caches, case):
    k0, v0 = caches
    k, v = torch.from_numpy(k0).cuda(), torch.from_numpy(v0).cuda()
    assert fork(L, k, v, BAD_PLANS[case], raw=True) == KR_ERR_ARG
    np.testing.assert_array_equal(k.cpu().numpy(), k0)
    np.testing.assert_array_equal(v.cpu().numpy(), v0)
