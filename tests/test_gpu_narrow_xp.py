"""kr_narrow_opts.x_packed: a <= 16-row narrow launch that reads its x operand from the XP16 buffer (one column tile of the packed
activation layout, at 8 row slots for M <= 8 and 16 above) gives, bit for bit, what the launch on the row-major tensor gives; the
two producers of such a buffer (kr_attn_decode_merge16, kr_linear_decode_wide with KR_DEC_OUT_XP16) store, element for element,
what their row-major forms store; and an engine at the 2B widths gives the same tokens and logits on either path.

The shapes are the smallest that keep what can go wrong: the shipped K values (24, 140 and 56 chunks, dealt over 8 / 16 waves and
1 / 2 K ranges in ragged shares), two or three weight tiles, row counts on both sides of the step from 8 to 16 row slots and at the tile's edge.  x is a
per-(row, k) ramp plus noise, so a swapped k-step, lane group or row changes the sums; the rows of the packed buffer behind M hold
NaN bits, which must reach nothing the launch stores."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import weights as WT  # noqa: E402
from karanta_ocr_amd._lib import DEC_OUT_XP16, DEC_PLAIN, DEC_SILU8, KarantaHipError, lib, narrow_opts, ptr  # noqa: E402
from karanta_ocr_amd.weights import bf16_round, pack_w16x64  # noqa: E402

DEV = "cuda:0"
NAN_BITS = 0x7FC1       # a bf16 NaN that is not the canonical one


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(bf16_round(np.asarray(a, np.float32)))).to(DEV).to(torch.bfloat16)


def raw(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def host_u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def slots(M):
    """Row slots of the XP16 buffer of an M-row launch (kr_xp16_rows of csrc/kr_common.h)."""
    return 8 if M <= 8 else 16


def xp16_index(rows, K, R):
    """[rows, K] int64: the bf16 slot of element (row b, column k) in an XP16 buffer of R row slots — include/karanta_hip.h,
    kr_narrow_opts.x_packed (kr_xp16_byte_offset of csrc/kr_common.h, over two)."""
    b, k = np.arange(rows)[:, None], np.arange(K)[None, :]
    byte = (k >> 6) * (R * 128) + ((k >> 5) & 1) * (R * 64) + ((((k >> 3) & 3) * R + b) * 16) + (k & 7) * 2
    return byte >> 1


def pack_xp16(x_rows: torch.Tensor, fill_bits: int) -> torch.Tensor:
    """The XP16 buffer (K * 32 bytes) of a row-major bf16 [M, K] tensor; everything but the M rows holds `fill_bits`."""
    M, K = x_rows.shape
    buf = np.full(16 * K, fill_bits, dtype=np.uint16)
    buf[xp16_index(M, K, slots(M)).ravel()] = x_rows.contiguous().view(torch.int16).cpu().numpy().astype(np.uint16).ravel()
    return torch.from_numpy(buf.view(np.int16)).to(DEV).view(torch.bfloat16)


def unpack_xp16(buf: torch.Tensor, rows: int, K: int, R: int) -> np.ndarray:
    """uint16 [rows, K]: the first `rows` row slots of an XP16 buffer of R row slots."""
    return buf.view(torch.int16).cpu().numpy().view(np.uint16)[xp16_index(rows, K, R)]


def weights(rng, N, K, fp8):
    Wf = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    if fp8:
        q, sc = WT.quantize_fp8_rows(Wf)
        return torch.from_numpy(WT.pack_w16x64_fp8(q)).to(DEV), torch.from_numpy(sc).to(DEV)
    return dev_bf16(pack_w16x64(bf16_round(Wf))), None


def ramp_x(rng, M, K):
    """Row b, column k: a ramp in both (distinct neighbours in a row, distinct rows) plus noise."""
    b, k = np.arange(M)[:, None], np.arange(K)[None, :]
    return dev_bf16((k % 97) / 97.0 - 0.5 + 0.125 * (b + 1) + 0.25 * rng.standard_normal((M, K)))


def narrow(L, x, W, sc, M, N, K, opts, out=0, out_f32=0, bias=0, res=0, waves=8, ksplit=1):
    head = (DEC_PLAIN, x, K, 0, 0, 0, 0)
    tail = (bias, 0, 1e-6, res, N if res else 0, out, out_f32, N, M, N, K, waves, ksplit, 0, 0, 0, 0, 0, 0, 0, 0, 0, 64, opts, 0)
    if sc is not None:
        L.kr_linear_decode_narrow_fp8(*head, ptr(W), ptr(sc), *tail)
    else:
        L.kr_linear_decode_narrow(*head, ptr(W), *tail)
    torch.cuda.synchronize()


SHAPES = [(32, 1536), (32, 8960), (48, 3584)]       # (N, K): o_proj of the 2B width, down_proj of the 2B width, o_proj of the 7B width
ROWS = [1, 7, 8, 9, 16]


@pytest.fixture(scope="module")
def operands(L):
    """Per (N, K, fp8): the weights, and per M the row-major x and its packed copy with NaN rows behind M — made once."""
    made = {}

    def get(N, K, fp8, M):
        key = (N, K, fp8)
        if key not in made:
            rng = np.random.default_rng(900 + N + K + fp8)
            made[key] = (weights(rng, N, K, fp8), dev_bf16(rng.standard_normal(N) * 0.1), dev_bf16(rng.standard_normal((16, N))), {})
        (W, sc), bias, res, xs = made[key]
        if M not in xs:
            x = ramp_x(np.random.default_rng(K + M), M, K)
            xs[M] = (x, pack_xp16(x, NAN_BITS))
        return W, sc, bias, res, xs[M]
    return get


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_plain_bias_residual_packed_x_bits(L, operands, N, K, M, fp8):
    """The o_proj form: PLAIN with bias and residual, 8-wave workgroups, the whole K in one workgroup."""
    W, sc, bias, res, (x, xp) = operands(N, K, fp8, M)
    got = []
    for packed in (False, True):
        out = torch.full((M, N), 9.0, dtype=torch.bfloat16, device=DEV)
        narrow(L, ptr(xp if packed else x), W, sc, M, N, K, narrow_opts(x_packed=packed), out=ptr(out), bias=ptr(bias), res=ptr(res))
        got.append(raw(out))
    assert (got[0] != raw(torch.full((M, N), 9.0, dtype=torch.bfloat16))).any()
    np.testing.assert_array_equal(got[0], got[1])


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_two_slab_partial_packed_x_bits(L, operands, N, K, M, fp8):
    """PARTIAL, two slabs: 16-wave workgroups, two K ranges, each range's sum in its own f32 slab."""
    W, sc, _, _, (x, xp) = operands(N, K, fp8, M)
    got = []
    for packed in (False, True):
        slabs = torch.full((2, M, N), 9.0, dtype=torch.float32, device=DEV)
        narrow(L, ptr(xp if packed else x), W, sc, M, N, K, narrow_opts(x_packed=packed), out_f32=ptr(slabs), waves=16, ksplit=2)
        got.append(raw(slabs))
    assert (got[0] != raw(torch.full((2, M, N), 9.0, dtype=torch.float32))).any()
    np.testing.assert_array_equal(got[0], got[1])


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_one_slab_atomic_packed_x_bits(L, operands, N, K, M, fp8):
    """The down_proj form: the two K ranges add into ONE slab that an earlier launch's zeroing job cleared (here: the row-major
    launch of the first pass zeroes the slab of the second, as a layer's qkv launch does for its down_proj)."""
    W, sc, _, _, (x, xp) = operands(N, K, fp8, M)
    acc = [torch.full((M, N), 9.0, dtype=torch.float32, device=DEV) for _ in range(2)]
    scratch = torch.zeros(2, M, N, dtype=torch.float32, device=DEV)
    narrow(L, ptr(x), W, sc, M, N, K, narrow_opts(ptr(acc[0]), M * N * 4), out_f32=ptr(scratch), waves=16, ksplit=2)   # zeroes acc[0]
    narrow(L, ptr(x), W, sc, M, N, K, narrow_opts(ptr(acc[1]), M * N * 4, atomic_out=True), out_f32=ptr(acc[0]), waves=16, ksplit=2)
    narrow(L, ptr(xp), W, sc, M, N, K, narrow_opts(atomic_out=True, x_packed=True), out_f32=ptr(acc[1]), waves=16, ksplit=2)
    assert raw(acc[0]).any()
    np.testing.assert_array_equal(raw(acc[0]), raw(acc[1]))


@pytest.mark.parametrize("fp8", [False, True])
def test_two_tiles_per_workgroup_packed_x_bits(L, monkeypatch, fp8):
    """down_proj of the 7B width (K = 18944: 296 chunks, 8-wave workgroups, 5-deep ring) runs TWO weight tiles per workgroup on one
    ring of x fragments where the launch has >= 192 tiles; KARANTA_NARROW_NT2=1 asks for that form at two tiles."""
    monkeypatch.setenv("KARANTA_NARROW_NT2", "1")
    M, N, K = 8, 32, 18944
    rng = np.random.default_rng(950 + fp8)
    W, sc = weights(rng, N, K, fp8)
    x = ramp_x(rng, M, K)
    xp = pack_xp16(x, NAN_BITS)
    acc = [torch.zeros(M, N, dtype=torch.float32, device=DEV) for _ in range(2)]
    for packed in (False, True):
        narrow(L, ptr(xp if packed else x), W, sc, M, N, K, narrow_opts(atomic_out=True, x_packed=packed), out_f32=ptr(acc[packed]),
               waves=8, ksplit=2)
    assert raw(acc[0]).any()
    np.testing.assert_array_equal(raw(acc[0]), raw(acc[1]))


def test_packed_x_rejects_what_it_is_not_built_for(L):
    z = torch.zeros(32 * 128, dtype=torch.bfloat16, device=DEV)
    W = torch.zeros(16 * 128, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(32, 16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(KarantaHipError, match="x_packed"):       # two column tiles: kr_linear_decode32 is that form
        narrow(L, ptr(z), W, None, 17, 16, 128, narrow_opts(x_packed=True), out=ptr(o))
    with pytest.raises(KarantaHipError, match="x_packed"):       # a norm prologue stages row-major rows
        L.kr_linear_decode_narrow(DEC_PLAIN, ptr(z), 128, 0, 0, 0, 0, ptr(W), 0, ptr(z), 1e-6, 0, 0, ptr(o), 0, 16, 8, 16, 128, 8, 1,
                                  0, 0, 0, 0, 0, 0, 0, 0, 0, 64, narrow_opts(x_packed=True), 0)


# ---- producers
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("M", [1, 8, 16])
def test_gate_up_xp16_is_the_row_major_output_packed(L, M, fp8):
    """SILU8 at K = 1536, 128 outputs (the packed layout takes whole 64-wide chunks: two of them, so that the chunk stride
    counts); slots of rows >= M keep what they held."""
    rng = np.random.default_rng(300 + M + fp8)
    N, K, nc = 4 * 64, 1536, 2 * 64          # 128 SiLU outputs = two 64-wide chunks of the packed buffer
    Wf = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    x, nw = dev_bf16(rng.standard_normal((M, K)) * 2), dev_bf16(1 + 0.1 * rng.standard_normal(K))
    rows = torch.zeros(M, nc, dtype=torch.bfloat16, device=DEV)
    pk = torch.full((16 * nc,), 7.0, dtype=torch.bfloat16, device=DEV)
    if fp8:
        q, scale = WT.quantize_fp8_rows(Wf)
        Wd, sd = torch.from_numpy(WT.pack_w16x64_fp8(q)).to(DEV), torch.from_numpy(scale).to(DEV)
        for mode, o in ((DEC_SILU8, rows), (DEC_SILU8 | DEC_OUT_XP16, pk)):
            L.kr_linear_decode_wide_fp8(mode, ptr(x), K, ptr(Wd), ptr(sd), 0, ptr(nw), 1e-6, 0, 0, ptr(o), 0, nc, M, N, K, 4, 4, 0, 0, 0)
    else:
        Wd = dev_bf16(pack_w16x64(bf16_round(Wf)))
        for mode, o in ((DEC_SILU8, rows), (DEC_SILU8 | DEC_OUT_XP16, pk)):
            L.kr_linear_decode_wide(mode, ptr(x), K, ptr(Wd), 0, ptr(nw), 1e-6, 0, 0, ptr(o), 0, nc, M, N, K, 4, 4, 0, 0, 0)
    torch.cuda.synchronize()
    want = rows.view(torch.int16).cpu().numpy().view(np.uint16)
    assert want.any()
    R = slots(M)
    np.testing.assert_array_equal(unpack_xp16(pk, M, nc, R), want)
    seven = torch.full((1,), 7.0, dtype=torch.bfloat16).view(torch.int16).item() & 0xFFFF
    assert (unpack_xp16(pk, R, nc, R)[M:] == seven).all() and (host_u16(pk)[R * nc:] == seven).all()
    with pytest.raises(KarantaHipError):                 # the one-tile layout is the <= 16-row form
        L.kr_linear_decode_wide(DEC_SILU8 | DEC_OUT_XP16, ptr(x), K, ptr(Wd), 0, ptr(nw), 1e-6, 0, 0, ptr(pk), 0, nc, 17, N, K, 4, 4, 0, 0, 0)


@pytest.mark.parametrize("n_split", [2, 16])
@pytest.mark.parametrize("M", [1, 8, 16])
def test_merge16_is_the_row_major_merge_packed(L, M, n_split):
    """12 heads of 128 channels (2 kv heads do not enter a merge): partial records [M][heads][n_split][128 + 4] f32."""
    rng = np.random.default_rng(400 + M + n_split)
    H, hd = 12, 128
    ws = rng.standard_normal((M, H, n_split, hd + 4)).astype(np.float32)
    ws[..., hd] = rng.uniform(-4, 4, size=(M, H, n_split))            # running maxima (log2 domain)
    ws[..., hd + 1] = rng.uniform(0.5, 8, size=(M, H, n_split))       # weight sums
    wsd = torch.from_numpy(ws).to(DEV)
    rows = torch.zeros(M, H * hd, dtype=torch.bfloat16, device=DEV)
    pk = torch.full((16 * H * hd,), 7.0, dtype=torch.bfloat16, device=DEV)
    L.kr_attn_decode_merge(ptr(wsd), ptr(rows), M, H, hd, n_split, 0)
    L.kr_attn_decode_merge16(ptr(wsd), ptr(pk), M, H, hd, n_split, 0)
    torch.cuda.synchronize()
    want = rows.view(torch.int16).cpu().numpy().view(np.uint16)
    assert want.any()
    R = slots(M)
    np.testing.assert_array_equal(unpack_xp16(pk, M, H * hd, R), want)
    seven = torch.full((1,), 7.0, dtype=torch.bfloat16).view(torch.int16).item() & 0xFFFF
    assert (unpack_xp16(pk, R, H * hd, R)[M:] == seven).all() and (host_u16(pk)[R * H * hd:] == seven).all()
    with pytest.raises(KarantaHipError):
        L.kr_attn_decode_merge16(ptr(wsd), ptr(pk), 17, H, hd, n_split, 0)


# ---- engine
def test_engine_tokens_and_logits_do_not_depend_on_the_x_layout():
    """The 2B widths at 1 ViT block and 3 decoder layers, 8 small pages, 6 tokens: the product engine (packed x operands of
    o_proj and down_proj) against ExperimentEngine(narrow_xp=False), whose step at <= 16 rows is the same launches on
    row-major operands; replayed tokens, eager tokens and the last step's logits, bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from karanta_ocr_amd.config import CONFIGS
    from karanta_ocr_amd.csrc.tools.experiment_engine import ExperimentEngine
    from karanta_ocr_amd.engine import Engine, PageRequest
    from karanta_ocr_amd.weights import random_weights
    from tests.launch_trace import launch_trace, names
    from tests.prodwidth import page_inputs
    base = CONFIGS["Qwen2-VL-2B"]
    cfg = dataclasses.replace(base, name="Qwen2-VL-2B-v1-l3", vision=dataclasses.replace(base.vision, depth=1),
                              text=dataclasses.replace(base.text, num_layers=3))
    pages = []
    for i in range(8):
        ids, pv, grid = page_inputs(cfg, 600 + i, 56 + 28 * (i % 3), 84 - 28 * (i % 2), 1024 * 1024, 3 + i % 4, 4, 700 + i)
        pages.append(PageRequest(ids, pv, [grid]))
    W = random_weights(cfg, 78)
    runs = {}
    for packed in (True, False):
        kw = dict(max_batch=8, s_max=256, max_patches=sum(len(p.pixel_values) for p in pages),
                  max_prompt_tokens=sum(len(p.input_ids) for p in pages), decode_splits=2)
        eng = Engine(cfg, **kw) if packed else ExperimentEngine(cfg, narrow_xp=False, **kw)
        assert eng.narrow_xp == packed
        eng.load_weights(W)
        graph = eng.generate(pages, 6, ignore_eos=True)
        with launch_trace(eng) as calls:
            eager = eng.generate(pages, 6, ignore_eos=True, return_logits=True)
        eng.close()
        called = names(calls)
        assert ("kr_attn_decode_merge16" in called) == packed and ("kr_attn_decode_merge" in called) == (not packed)
        narrow_launches = [c for c in calls if c[0] == "kr_linear_decode_narrow"]
        assert any(isinstance(c[1][-2], dict) and c[1][-2].get("x_packed") == 1 for c in narrow_launches) == packed
        runs[packed] = (graph, eager)
    for i in range(len(pages)):
        np.testing.assert_array_equal(runs[True][0].tokens[i], runs[False][0].tokens[i], err_msg=f"page {i}: replayed tokens")
        np.testing.assert_array_equal(runs[True][1].tokens[i], runs[False][1].tokens[i], err_msg=f"page {i}: eager tokens")
        np.testing.assert_array_equal(runs[True][1].tokens[i], runs[True][0].tokens[i], err_msg=f"page {i}: eager against replayed")
        a, b = runs[True][1].logits[i][-1], runs[False][1].logits[i][-1]
        np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                                      np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=f"page {i}: final logits")
