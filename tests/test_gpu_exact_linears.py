"""The linears on the dyadic cases of tests/exact_cases.py (proven on the float64 reference by test_exact_cases_cpu.py),
through the C-ABI on a real MI355X: every partial sum of these cases is exact in f32 in any order, so the outputs are
compared with the reference BIT FOR BIT at full K — a dropped or duplicated k element, a double or missing rounding, a
truncation, a residual added after the rounding all change the expected bits.  Every operand sits in a Guarded buffer:
row strides larger than the logical width (ldx = K + 8 / K + 24, ldc = N + 8, ldr = N + 16), NaN beyond every input,
a fixed pattern around every output that must still be there after the launch.  The activation epilogues are held to
the two bf16 values that bracket the float64 reference (or 2^-20 absolute): their accumulator is exact, the activation
is evaluated in f32."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import positions as POS  # noqa: E402
from karanta_ocr_amd import weights as WT  # noqa: E402
from karanta_ocr_amd._lib import (DEC_ARGMAX, DEC_OUT_XP, DEC_PLAIN, DEC_ROPE_KV, DEC_SILU8, EPI_GELU_ERF, EPI_NONE,  # noqa: E402
                                  EPI_QUICK_GELU, EPI_SILU_MUL, EPI_SILU_MUL8, Dec32, lib)
from tests import exact_cases as E  # noqa: E402

DEV = "cuda:0"
U16, U32 = np.uint16, np.uint32


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


# ----------------------------------------------------------------------------- guarded operands
def g2(kind, a, pad, role="in", offset=0, rows=None, cols=None):
    """A 2-D operand (bit patterns / f32 values) with `pad` padding columns."""
    if a is not None:
        rows, cols = a.shape
    return E.Guarded(torch, DEV, kind, rows, cols, cols + pad, role, 16, offset, a)


def g1(kind, a=None, n=None, role="in"):
    """A flat operand: guard bands before and after."""
    if a is not None:
        a = np.ascontiguousarray(a).reshape(-1)
        n = a.size
    return E.Guarded(torch, DEV, kind, 1, n, n, role, 0, 0, a)


def bf(a, pad, **kw):
    return g2("bf16", E.bits16(a), pad, **kw)


def bf1(a):
    return None if a is None else g1("bf16", E.bits16(a))


def p(g):
    return 0 if g is None else g.ptr


def untouched(**gs):
    for name, g in gs.items():
        if g is not None:
            g.assert_untouched(name)


def eq_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    bad = got != ref.reshape(got.shape)
    if bad.any():
        i = np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), got.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ from the exact reference, the first at {i}: "
                             f"got {int(got[i]):#x}, expected {int(ref.reshape(got.shape)[i]):#x}")


def pad_for(i):
    return 8 if i % 2 == 0 else 24


def f32_bits(v):
    return np.ascontiguousarray(E.exact_f32(v)).view(U32)


# ----------------------------------------------------------------------------- prefill / ViT GEMMs
_SCRATCH = None


def scratch():
    global _SCRATCH
    if _SCRATCH is None:
        _SCRATCH = g1("f32", n=512 * 65536 // 4, role="out")
    return _SCRATCH


def run_gemm(L, c, packed, lda_pad, use_scratch=True, inplace=False, ldc_pad=8, c_offset=0, epi=EPI_NONE, nc=None, res=True):
    M, N, K = c.M, c.N, c.K
    nc = N if nc is None else nc
    A = bf(c.A, lda_pad)
    W = bf1(WT.pack_w16x64(c.W) if packed else c.W)
    bias = bf1(c.bias)
    R = None
    if inplace:
        Cg = g2("bf16", E.bits16(c.res), ldc_pad, role="out")
        R = Cg
    else:
        Cg = g2("bf16", None, ldc_pad, role="out", offset=c_offset, rows=M, cols=nc)
        if res and c.res is not None:
            R = bf(c.res, 16)
    S = scratch() if use_scratch else None
    L.kr_gemm_bf16_ws(A.ptr, A.ld, W.ptr, p(bias), p(R), R.ld if R else 0, Cg.ptr, Cg.ld, M, N, K, epi, 1 if packed else 0,
                      p(S), S.cols * 4 if S else 0, 0)
    got = Cg.read()
    untouched(A=A, W=W, bias=bias, C=Cg, scratch_bands=S, **({} if inplace else {"residual": R}))
    return got


@pytest.mark.parametrize("packed", [False, True], ids=["row-major", "packed"])
@pytest.mark.parametrize("cid", list(E.GEMM_SHAPES))
def test_gemm_exact_at_full_k(L, monkeypatch, cid, packed):
    M, N, K, env = E.GEMM_SHAPES[cid]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = E.linear_case(M, N, K)
    eq_bits(run_gemm(L, c, packed, 24 if packed else 8, use_scratch=not packed), c.ref_bits(), cid)


@pytest.mark.parametrize("cid", ["ring4-129x144x1216", "tile512-513x1280x1216"])
def test_gemm_in_place_residual_exact(L, monkeypatch, cid):
    M, N, K, env = E.GEMM_SHAPES[cid]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = E.linear_case(M, N, K)
    eq_bits(run_gemm(L, c, False, 8, inplace=True), c.ref_bits(), cid + " in place")


TAIL_RUNS = [("tail-quarters", "tail", True, False), ("tail-quarters", "tail-off", True, True), ("tail-quarters", "tail-unsplit", True, False),
             ("tail-k-cut", "tail", True, True), ("tail-k-cut", "tail", False, False), ("tail-k-cut", "tail-off", True, False),
             ("tail-k-cut", "tail-unsplit", True, True)]


@pytest.mark.parametrize("shape,variant,with_scratch,packed", TAIL_RUNS,
                         ids=[f"{s}-{v}-{'scratch' if w else 'null'}-{'packed' if pk else 'rows'}" for s, v, w, pk in TAIL_RUNS])
def test_gemm_tail_round_variants_equal_the_one_reference(L, monkeypatch, shape, variant, with_scratch, packed):
    """The pipelined-256 launch with a tail round (as quarters; cut along K at K = 4160: 65 K steps over 8 ranges), the
    one-launch form and the unsplit tail, with the scratch and without: all the same bits, the reference's."""
    M, N, K = E.GEMM_TAIL_SHAPES[shape]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-M // 256) * (N // 256)
    assert tiles > cus and 0 < tiles % cus <= cus // 2 and M % 256 == 1, "shape no longer exercises the tail on this device"
    monkeypatch.setenv("KARANTA_GEMM_TILE", "512")
    for k, v in E.GEMM_TAIL_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    c = E.linear_case(M, N, K)
    eq_bits(run_gemm(L, c, packed, 24 if packed else 8, use_scratch=with_scratch), c.ref_bits(), f"{shape} {variant}")


def test_gemm_fallback_dispatch_for_an_unaligned_c(L, monkeypatch):
    """ldc % 8 != 0 and C only 8-byte aligned: launch_gemm2 falls back to the 128 tile under KARANTA_GEMM_TILE=512."""
    monkeypatch.setenv("KARANTA_GEMM_TILE", "512")
    c = E.linear_case(*E.GEMM_FALLBACK)
    for packed in (False, True):
        eq_bits(run_gemm(L, c, packed, 8, ldc_pad=4, c_offset=4), c.ref_bits(), "fallback")


def fp8_weights(c):
    q = WT.f32_to_fp8_e4m3_fast(c.W)
    assert (WT.fp8_e4m3_to_f32(q) == c.W).all()
    return g1("u8", WT.pack_w16x64_fp8(q)), g1("f32", c.w_scale)


@pytest.mark.parametrize("M,N,K", E.GEMM_FP8_SHAPES)
def test_gemm_fp8_exact_at_full_k(L, M, N, K):
    c = E.linear_case(M, N, K, "fp8")
    A, (W, ws), bias, R = bf(c.A, 8), fp8_weights(c), bf1(c.bias), bf(c.res, 16)
    Cg = g2("bf16", None, 8, role="out", rows=M, cols=N)
    L.kr_gemm_fp8(A.ptr, A.ld, W.ptr, ws.ptr, bias.ptr, R.ptr, R.ld, Cg.ptr, Cg.ld, M, N, K, EPI_NONE, 0)
    eq_bits(Cg.read(), c.ref_bits(), "gemm fp8")
    untouched(A=A, W=W, scale=ws, bias=bias, residual=R, C=Cg)


@pytest.mark.parametrize("mx", [(1, 0), (1, 1), (0, 0)], ids=["mx", "mx-two-k-tiles", "fp8-16x16x32"])
@pytest.mark.parametrize("M,N,K", E.GEMM_FP8_SHAPES)
def test_gemm_fp8a_exact_at_full_k(L, monkeypatch, M, N, K, mx):
    monkeypatch.setenv("KARANTA_FP8_MX", str(mx[0]))
    monkeypatch.setenv("KARANTA_FP8_MX2", str(mx[1]))
    c = E.linear_case(M, N, K, "fp8a")
    qa = WT.f32_to_fp8_e4m3(c.A)
    assert (WT.fp8_e4m3_to_f32(qa) == c.A).all()
    A, sa = g2("u8", qa, 16 if mx[1] else 48), g1("f32", c.a_scale)
    (W, ws), bias, R = fp8_weights(c), bf1(c.bias), bf(c.res, 16)
    Cg = g2("bf16", None, 8, role="out", rows=M, cols=N)
    L.kr_gemm_fp8a(A.ptr, A.ld, sa.ptr, W.ptr, ws.ptr, bias.ptr, R.ptr, R.ld, Cg.ptr, Cg.ld, M, N, K, EPI_NONE, 0)
    eq_bits(Cg.read(), c.ref_bits(), "gemm fp8a")
    untouched(A=A, a_scale=sa, W=W, scale=ws, bias=bias, residual=R, C=Cg)


EPI_OF = {"quick_gelu": EPI_QUICK_GELU, "gelu_erf": EPI_GELU_ERF, "silu_mul": EPI_SILU_MUL, "silu_mul8": EPI_SILU_MUL8,
          "silu_mul8_bias": EPI_SILU_MUL8}


@pytest.mark.parametrize("tile", ["128", "512"])
@pytest.mark.parametrize("epi", E.ACT_EPILOGUES)
def test_gemm_activation_epilogues_bracket_the_exact_reference(L, monkeypatch, epi, tile):
    monkeypatch.setenv("KARANTA_GEMM_TILE", tile)
    M, N, K = E.act_shape(epi)
    c = E.act_case(M, N, K, bias=epi in ("quick_gelu", "gelu_erf", "silu_mul8_bias"))
    name = epi.replace("_bias", "")
    ref = E.act_ref(name, c.full_pre())
    nc = N // 2 if name.startswith("silu") else N
    for packed in (False, True):
        got = run_gemm(L, c, packed, 8 if packed else 24, epi=EPI_OF[epi], nc=nc)
        ok = E.bracket_ok(got, ref)
        assert ok.all(), f"{epi} tile {tile}: {(~ok).sum()} of {ok.size} outputs outside the bracket, the first at " \
                         f"{np.unravel_index(int(np.flatnonzero(~ok.reshape(-1))[0]), ok.shape)}"


# ----------------------------------------------------------------------------- decode, <= 16 rows
def narrow(L, mode, x, W, M, N, K, *, w_scale=None, part=None, n_part=0, x_out=None, bias=None, norm_w=None, res=None, out=None,
           out_f32=None, ldc=0, waves=8, ksplit=1, rope=None, opts=None):
    cs, T, plen, ctx, q, kc, vc, H, KVH, s_max = rope if rope else (None, 0, None, None, None, None, None, 0, 0, 64)
    head = (mode, x.ptr, x.ld, p(part), n_part, p(x_out), x_out.ld if x_out else 0, W.ptr)
    tail = (p(bias), p(norm_w), E.EPS, p(res), res.ld if res else 0, p(out), p(out_f32), ldc, M, N, K, waves, ksplit, p(cs), T, p(plen),
            p(ctx), p(q), p(kc), p(vc), H, KVH, s_max, opts, 0)
    if w_scale is not None:
        L.kr_linear_decode_narrow_fp8(*head, w_scale.ptr, *tail)
    else:
        L.kr_linear_decode_narrow(*head, *tail)


def weights_of(c, fp8):
    if fp8:
        return fp8_weights(c)
    return bf1(WT.pack_w16x64(c.W)), None


@pytest.mark.parametrize("f32", [False, True], ids=["bf16-out", "f32-out"])
@pytest.mark.parametrize("M", E.NARROW_M)
@pytest.mark.parametrize("N,K,waves,fp8", [s + (False,) for s in E.NARROW_SHAPES] + [s + (True,) for s in E.NARROW_SHAPES[:2]])
def test_narrow_plain_exact_at_full_k(L, M, N, K, waves, fp8, f32):
    c = E.linear_case(M, N, K, "fp8" if fp8 else "bf16")
    x, (W, ws), bias, R = bf(c.A, pad_for(M)), weights_of(c, fp8), bf1(c.bias), bf(c.res, 16)
    out = g2("f32" if f32 else "bf16", None, 8, role="out", rows=M, cols=N)
    narrow(L, DEC_PLAIN, x, W, M, N, K, w_scale=ws, bias=bias, res=R, out=None if f32 else out, out_f32=out if f32 else None,
           ldc=out.ld, waves=waves)
    eq_bits(out.read(), f32_bits(c.full_pre()) if f32 else c.ref_bits(), c.name)
    untouched(x=x, W=W, scale=ws, bias=bias, residual=R, out=out)


@pytest.mark.parametrize("M,N,K,waves", [(5, 1536, 1536, 8), (16, 96, 8960, 16)])
def test_narrow_plain_in_place_residual_exact(L, M, N, K, waves):
    c = E.linear_case(M, N, K)
    x, (W, _), bias = bf(c.A, 24), weights_of(c, False), bf1(c.bias)
    out = g2("bf16", E.bits16(c.res), 8, role="out")
    narrow(L, DEC_PLAIN, x, W, M, N, K, bias=bias, res=out, out=out, ldc=out.ld, waves=waves)
    eq_bits(out.read(), c.ref_bits(), c.name + " in place")
    untouched(x=x, W=W, bias=bias, out=out)


def norm_operands(nl):
    n_part = nl.parts.shape[0]
    x = bf(nl.x, 8)
    part = g1("f32", nl.parts) if n_part else None
    x_out = g2("bf16", None, 24, role="out", rows=nl.x.shape[0], cols=nl.x.shape[1]) if n_part else None
    return x, part, n_part, x_out, bf1(nl.norm_w)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("M,K,n_part", E.NARROW_NORM)
def test_narrow_norm_prologue_exact(L, M, K, n_part, fp8):
    """x_new = bf16(x + slabs) (one rounding, two slabs included), RMSNorm(x_new) W^T + bias + residual: both exact."""
    nl = E.norm_linear_case(M, E.NORM_N, K, n_part, fp8)
    c, N = nl.lin, E.NORM_N
    x, part, n_part, x_out, nw = norm_operands(nl)
    (W, ws), bias, R = weights_of(c, fp8), bf1(c.bias), bf(c.res, 16)
    out = g2("bf16", None, 8, role="out", rows=M, cols=N)
    narrow(L, DEC_PLAIN, x, W, M, N, K, w_scale=ws, part=part, n_part=n_part, x_out=x_out, bias=bias, norm_w=nw, res=R, out=out,
           ldc=out.ld)
    if n_part:
        eq_bits(x_out.read(), E.bits16(nl.x_new), "x_new")
    eq_bits(out.read(), c.ref_bits(), c.name)
    untouched(x=x, slabs=part, x_out=x_out, norm_w=nw, W=W, scale=ws, bias=bias, residual=R, out=out)


@pytest.mark.parametrize("M,K,n_part", [(M, K, n) for M in (3, 16, 21, 32) for K in (1536, 2048, 3584) for n in (0, 1, 2)])
def test_decode_resnorm_exact(L, M, K, n_part):
    nl = E.norm_linear_case(M, 16, K, n_part, False, False)
    x, part, n_part, x_out, nw = norm_operands(nl)
    h = g2("bf16", None, 8, role="out", rows=M, cols=K)
    L.kr_decode_resnorm(x.ptr, x.ld, p(part), n_part, M, p(x_out), x_out.ld if x_out else 0, nw.ptr, E.EPS, h.ptr, h.ld, M, K, 0)
    if n_part:
        eq_bits(x_out.read(), E.bits16(nl.x_new), "x_new")
    eq_bits(h.read(), E.bits16(nl.h), "h")
    untouched(x=x, slabs=part, x_out=x_out, norm_w=nw, h=h)


class RopeBuffers:
    """q_out and the two caches of a ROPE_KV launch: the caches hold finite values the launch must keep everywhere but in
    the appended row / column."""

    def __init__(self, c):
        rng = np.random.default_rng(c.B + c.H)
        self.c = c
        self.kc0 = E.bits16(rng.integers(-100, 101, size=(c.B, c.KVH, c.s_max, 128)).astype(np.float32))
        self.vt0 = E.bits16(rng.integers(-100, 101, size=(c.B, c.KVH, c.s_max // 64, 128, 64)).astype(np.float32))
        self.q = g1("bf16", n=c.B * c.H * 128, role="out")
        self.kc, self.vt = g1("bf16", self.kc0, role="out"), g1("bf16", self.vt0, role="out")
        self.cs, self.plen, self.ctx = g1("f32", c.cs), g1("i32", c.plen.astype(np.int32)), g1("i32", c.ctx)

    def args(self):
        c = self.c
        return (self.cs, c.T, self.plen, self.ctx, self.q, self.kc, self.vt, c.H, c.KVH, c.s_max)

    def check(self, rows=None, slots=None, q=None, k=None, v=None):
        """rows: the batch rows that were computed (default all); slots: the cache slot of each row (default its own)."""
        c = self.c
        rows = np.arange(c.B) if rows is None else np.asarray(rows)
        slots = rows if slots is None else np.asarray(slots)
        q, k, v = (c.q if q is None else q), (c.k if k is None else k), (c.v if v is None else v)
        got_q = self.q.read().reshape(c.B, c.H, 128)
        eq_bits(got_q[rows], q[rows], "q")
        assert (got_q[np.setdiff1d(np.arange(c.B), rows)] == self.q.poison).all(), "q rows beyond the batch were written"
        want_k, want_v = self.kc0.copy(), POS.vt_rows(self.vt0).copy()
        for r, s in zip(rows, slots):
            want_k[s, :, c.ctx[r]] = k[r]
            want_v[s, :, c.ctx[r]] = v[r]
        eq_bits(self.kc.read().reshape(want_k.shape), want_k, "K cache")
        eq_bits(POS.vt_rows(self.vt.read().reshape(self.vt0.shape)), want_v, "V^T cache")
        untouched(q=self.q, kcache=self.kc, vtcache=self.vt, cs=self.cs, prompt_len=self.plen, ctx_len=self.ctx)


# the slab prologue exists at K = 1536, 2048 and 3584 only
ROPE_RUNS = [(H, KVH, K, form, B) for (H, KVH, K) in E.ROPE_SHAPES
             for form, B in [("fused-p0", 16), ("fused-p2", 16), ("fused-p1", 6), ("direct", 32), ("direct", 7)]
             if K >= 1536 or form in ("fused-p0", "direct")]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,KVH,K,form,B", ROPE_RUNS)
def test_narrow_rope_kv_exact(L, H, KVH, K, form, B, fp8):
    """t = bf16(acc * scale + bias), q / k = bf16(rotary of t), v = t, the rest of both caches as before: the fused norm
    prologue (with 0, 1, 2 slabs) and the direct form on normalised rows (norm_w = NULL, up to 32 rows)."""
    n_part = int(form[-1]) if form.startswith("fused") else 0
    c = E.rope_case(B, H, KVH, K, n_part, fp8)
    lin, N = c.nl.lin, (H + 2 * KVH) * 128
    (W, ws), bias, buf = weights_of(lin, fp8), bf1(lin.bias), RopeBuffers(c)
    if form == "direct":
        x = bf(c.nl.h, pad_for(B))
        narrow(L, DEC_ROPE_KV, x, W, B, N, K, w_scale=ws, bias=bias, rope=buf.args())
        untouched(x=x)
    else:
        x, part, n_part, x_out, nw = norm_operands(c.nl)
        narrow(L, DEC_ROPE_KV, x, W, B, N, K, w_scale=ws, part=part, n_part=n_part, x_out=x_out, bias=bias, norm_w=nw, rope=buf.args())
        if n_part:
            eq_bits(x_out.read(), E.bits16(c.nl.x_new), "x_new")
        untouched(x=x, slabs=part, x_out=x_out, norm_w=nw)
    buf.check()
    untouched(W=W, scale=ws, bias=bias)


# ---- wide
def wide(L, mode, x, W, M, N, K, blocks, waves, *, w_scale=None, bias=None, norm_w=None, res=None, out=None, out_f32=None, ldc=0,
         av=None, ai=None):
    head = (mode, x.ptr, x.ld, W.ptr)
    tail = (p(bias), p(norm_w), E.EPS, p(res), res.ld if res else 0, p(out), p(out_f32), ldc, M, N, K, blocks, waves, p(av), p(ai), 0)
    if w_scale is not None:
        L.kr_linear_decode_wide_fp8(*head, w_scale.ptr, *tail)
    else:
        L.kr_linear_decode_wide(*head, *tail)


# 17..32 rows at K = 3584 run SILU8 / ARGMAX only (the K-halves kernel)
WIDE_PLAIN_RUNS = [(M,) + s for s in E.WIDE_SHAPES for M in [1, 16] + E.DEC32_M if not (M > 16 and s[1] == 3584)]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("M,N,K,blocks,waves", WIDE_PLAIN_RUNS)
def test_wide_plain_exact_at_full_k(L, M, N, K, blocks, waves, fp8):
    c = E.linear_case(M, N, K, "fp8" if fp8 else "bf16")
    x, (W, ws), bias, R = bf(c.A, pad_for(M)), weights_of(c, fp8), bf1(c.bias), bf(c.res, 16)
    out = g2("bf16", None, 8, role="out", rows=M, cols=N)
    wide(L, DEC_PLAIN, x, W, M, N, K, blocks, waves, w_scale=ws, bias=bias, res=R, out=out, ldc=out.ld)
    eq_bits(out.read(), c.ref_bits(), c.name)
    untouched(x=x, W=W, scale=ws, bias=bias, residual=R, out=out)


def wide_launch_of(M, K, blocks, waves):
    """17..32 rows at K = 3584: the K-halves kernel, 8 waves."""
    return (blocks, 8) if (M > 16 and K == 3584) else (blocks, waves)


@pytest.mark.parametrize("M", [1, 16] + E.DEC32_M)
@pytest.mark.parametrize("N,K,blocks,waves", E.WIDE_SHAPES)
def test_wide_argmax_exact_logits_and_lowest_index_on_ties(L, M, N, K, blocks, waves):
    blocks, waves = wide_launch_of(M, K, blocks, waves)
    c = E.argmax_case(M, N, K)
    x, (W, _) = bf(c.A, pad_for(M)), weights_of(c, False)
    n_part = blocks * waves
    lg = g2("f32", None, 8, role="out", rows=M, cols=N)
    av, ai = g1("f32", n=M * n_part, role="out"), g1("i32", n=M * n_part, role="out")
    wide(L, DEC_ARGMAX, x, W, M, N, K, blocks, waves, out_f32=lg, ldc=lg.ld, av=av, ai=ai)
    logits = c.ref_f32()
    eq_bits(lg.read(), logits.view(U32), c.name)
    a_, i_ = av.read().view(np.float32).reshape(M, n_part), ai.read().view(np.int32).reshape(M, n_part)
    ties = 0
    for b in range(M):
        best = int(np.lexsort((i_[b], -a_[b]))[0])                  # the host's reduction: highest value, lowest index
        assert i_[b, best] == int(logits[b].argmax()) and a_[b, best] == logits[b].max(), f"row {b}"
        ties += int((logits[b] == logits[b].max()).sum() > 1)
    assert ties == M, "the case no longer ties at the maximum"
    untouched(x=x, W=W, logits=lg, amax_val=av, amax_idx=ai)


# the packed output is the 17..32-row form
SILU8_RUNS = [(M, xp) for M in [3, 16] + E.DEC32_M for xp in (False, True) if M > 16 or not xp]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("M,xp", SILU8_RUNS, ids=[f"{M}-{'packed-out' if xp else 'rows'}" for M, xp in SILU8_RUNS])
@pytest.mark.parametrize("K,blocks,waves", [(512, 3, 5), (1536, 256, 4), (3584, 5, 8)])
def test_wide_silu8_norm_brackets_the_exact_reference(L, M, K, blocks, waves, xp, fp8):
    ff = 320
    nl = E.silu8_norm_case(M, ff, K, fp8)
    c = nl.lin
    ref = E.act_ref("silu_mul8", c.full_pre())
    x, nw, (W, ws) = bf(nl.x, pad_for(M)), bf1(nl.norm_w), weights_of(c, fp8)
    if xp:
        out = g1("bf16", n=32 * ff, role="out")
        wide(L, DEC_SILU8 | DEC_OUT_XP, x, W, M, 2 * ff, K, blocks, waves, w_scale=ws, norm_w=nw, out=out, ldc=ff)
        full = WT.unpack_rows32(out.read().reshape(-1), ff)
        got = full[:M]
        assert (full[M:] == out.poison).all(), "rows beyond the batch were written"
    else:
        out = g2("bf16", None, 8, role="out", rows=M, cols=ff)
        wide(L, DEC_SILU8, x, W, M, 2 * ff, K, blocks, waves, w_scale=ws, norm_w=nw, out=out, ldc=out.ld)
        got = out.read()
    ok = E.bracket_ok(got, ref)
    assert ok.all(), f"{(~ok).sum()} of {ok.size} outputs outside the bracket"
    untouched(x=x, norm_w=nw, W=W, scale=ws, out=out)


# ----------------------------------------------------------------------------- decode, 17..32 rows
def dec32(L, mode, xp, W, M, N, K, waves_ref, *, ksplit=1, out=None, out_f32=None, ldc=0, bias=None, res=None, w_scale=None,
          atomic=False, tiles=0, gs=False, rope=None, row_slot=None):
    cs, T, plen, ctx, q, kc, vc, H, KVH, s_max = rope if rope else (None, 0, None, None, None, None, None, 0, 0, 64)
    a = Dec32(xp.ptr, W.ptr, p(w_scale), p(bias), p(res), res.ld if res else 0, p(out), p(out_f32), ldc, M, N, K, waves_ref, ksplit,
              1 if atomic else 0, tiles, 1 if gs else 0, 0, 0, 0, p(cs), T, p(plen), p(ctx), p(q), p(kc), p(vc), H, KVH, s_max)
    if row_slot is not None:
        L.kr_linear_decode32_rows(mode, C.byref(a), row_slot.ptr, 0)
    else:
        L.kr_linear_decode32(mode, C.byref(a), 0)


def packed_rows(x, nan_tail=False):
    """kr_pack_rows32's layout from the host; nan_tail: rows >= M hold NaN instead of zeros."""
    M, K = x.shape
    bits = np.zeros((32, K), U16)
    bits[:M] = E.bits16(x)
    if nan_tail:
        bits[M:] = 0x7FC0
    return g1("bf16", WT.pack_rows32(bits))


@pytest.mark.parametrize("M", E.DEC32_M)
@pytest.mark.parametrize("K", [64, 1536, 3584])
def test_pack_rows32_exact_and_zero_beyond_the_batch(L, M, K):
    rng = np.random.default_rng(M + K)
    xv = E.nz_ints(rng, M, K, hi=127)
    x = bf(xv, 24)
    xp = g1("bf16", n=32 * K, role="out")
    L.kr_pack_rows32(x.ptr, x.ld, M, K, xp.ptr, 0)
    full = WT.unpack_rows32(xp.read().reshape(-1), K)
    eq_bits(full[:M], E.bits16(xv), "packed rows")
    assert not full[M:].any(), "rows >= M of the packed buffer must be zero"
    untouched(x=x, xp=xp)


@pytest.mark.parametrize("tiles,nan_tail", [(0, False), (1, False), (2, False), (0, True)],
                         ids=["tiles0", "tiles1", "tiles2", "tiles0-nan-tail"])
@pytest.mark.parametrize("M", E.DEC32_M)
@pytest.mark.parametrize("N,K,waves,ksplit", E.DEC32_SHAPES)
def test_decode32_plain_exact_at_full_k(L, M, N, K, waves, ksplit, tiles, nan_tail):
    """PLAIN bf16 + bias + residual against the absolute reference; ksplit = 2: two slabs, one atomically accumulated slab
    and the group split into zeroed slabs, whose sums are the exact accumulator.  nan-tail: rows >= M of the packed input
    hold NaN — a row's numbers do not depend on its batch."""
    c = E.linear_case(M, N, K)
    xp, (W, _), bias, R = packed_rows(c.A, nan_tail), weights_of(c, False), bf1(c.bias), bf(c.res, 16)
    if ksplit == 1:
        out = g2("bf16", None, 8, role="out", rows=M, cols=N)
        dec32(L, DEC_PLAIN, xp, W, M, N, K, waves, out=out, ldc=out.ld, bias=bias, res=R, tiles=tiles)
        eq_bits(out.read(), c.ref_bits(), c.name)
        untouched(out=out)
    else:
        acc = f32_bits(c.acc())
        slabs = g1("f32", n=ksplit * M * N, role="out")
        dec32(L, DEC_PLAIN, xp, W, M, N, K, waves, ksplit=ksplit, out_f32=slabs, ldc=N, tiles=tiles)
        got = slabs.read().view(np.float32).reshape(ksplit, M, N)
        cut = -(-(K // 64) // ksplit) * 64
        for ks in range(ksplit):       # slab ks holds exactly its K range
            part = c.A[:, ks * cut:(ks + 1) * cut].astype(np.float64) @ c.W[:, ks * cut:(ks + 1) * cut].astype(np.float64).T
            eq_bits(got[ks].view(U32), f32_bits(part), f"slab {ks}")
        one = g2("f32", np.zeros((M, N), np.float32), 8, role="out")
        dec32(L, DEC_PLAIN, xp, W, M, N, K, waves, ksplit=ksplit, out_f32=one, ldc=one.ld, atomic=True, tiles=tiles)
        eq_bits(one.read(), acc, "atomic slab")
        untouched(slabs=slabs, atomic=one)
        if tiles == 0 and (N // 16) % (4 if waves == 8 else 2) == 0:
            pair = g1("f32", np.zeros(2 * M * N, np.float32), role="out")
            dec32(L, DEC_PLAIN, xp, W, M, N, K, waves, ksplit=2, out_f32=pair, ldc=N, atomic=True, gs=True)
            eq_bits(pair.read().view(np.float32).reshape(2, M, N).astype(np.float64).sum(0).astype(np.float32).view(U32), acc, "group split")
            untouched(pair=pair)
    untouched(xp=xp, W=W, bias=bias, residual=R)


@pytest.mark.parametrize("M,K,n_part,first", [(M, K, n, f) for M in E.DEC32_M for K in (1536, 3584)
                                              for n, f in ((0, 0), (1, 0), (2, 0), (2, 1))])       # first: sum_slabs_first (two slabs)
def test_decode_resnorm32_exact(L, M, K, n_part, first):
    nl = E.norm_linear_case(M, 16, K, n_part, False, False)
    x, part, n_part, x_out, nw = norm_operands(nl)
    hp = g1("bf16", n=32 * K, role="out")
    L.kr_decode_resnorm32(x.ptr, x.ld, p(part), n_part, M, p(x_out), x_out.ld if x_out else 0, nw.ptr, E.EPS, hp.ptr, M, K, first, 0)
    if n_part:
        eq_bits(x_out.read(), E.bits16(nl.x_new), "x_new")
    full = WT.unpack_rows32(hp.read().reshape(-1), K)
    eq_bits(full[:M], E.bits16(nl.h), "h")
    assert (full[M:] == hp.poison).all(), "rows beyond the batch were written"
    untouched(x=x, slabs=part, x_out=x_out, norm_w=nw, h_xp=hp)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("form", ["batch", "rows", "batch-nan-tail"])
@pytest.mark.parametrize("H,KVH,K,B", [(2, 1, 256, 17), (12, 2, 1536, 32), (28, 4, 3584, 21)])
def test_decode32_rope_kv_exact(L, H, KVH, K, B, form, fp8):
    """ROPE_KV through kr_linear_decode32 and, with a permuted row_slot (the cache slot and the cs_table row of a row) and
    per-row ctx_len, through kr_linear_decode32_rows."""
    c = E.rope_case(B, H, KVH, K, 0, fp8)
    lin, N = c.nl.lin, (H + 2 * KVH) * 128
    (W, ws), bias, buf = weights_of(lin, fp8), bf1(lin.bias), RopeBuffers(c)
    xp = packed_rows(c.nl.h, form.endswith("nan-tail"))
    if form == "rows":
        slots = np.random.default_rng(B).permutation(B).astype(np.int32)
        rs = g1("i32", slots)
        dec32(L, DEC_ROPE_KV, xp, W, B, N, K, 8, bias=bias, w_scale=ws, rope=buf.args(), row_slot=rs)
        q, k, v = E.rope_outputs(c, c.t, slots=slots)
        buf.check(slots=slots, q=q, k=k, v=v)
        untouched(row_slot=rs)
    else:
        dec32(L, DEC_ROPE_KV, xp, W, B, N, K, 8, bias=bias, w_scale=ws, rope=buf.args())
        buf.check()
    untouched(xp=xp, W=W, scale=ws, bias=bias)


# ----------------------------------------------------------------------------- prefill pieces
@pytest.mark.parametrize("as_cache", [False, True], ids=["flat", "cache"])
@pytest.mark.parametrize("hd,H,KVH", E.PREP_HEADS)
def test_qkv_prep_exact(L, hd, H, KVH, as_cache):
    c = E.prep_case(hd, H, KVH)
    lens, n = list(c.lens), sum(c.lens)
    qd, kd = H * hd, KVH * hd
    if as_cache:
        s_max, B = 128, len(lens)
        plan = POS.prefill_attn_plan(lens, list(range(B)), KVH, s_max)
        k_shape, vt_shape = (B * KVH, s_max, hd), (B * KVH, s_max // 64, hd, 64)
        k_hs, vt_hs = s_max * hd, (s_max // 64) * hd * 64
    else:
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        plan = POS.make_attn_plan(lens, starts, np.concatenate([[0], np.cumsum([(x + 63) // 64 for x in lens])[:-1]]), False)
        k_shape, vt_shape = (KVH, n, hd), (KVH, plan.n_vt_blocks, hd, 64)
        k_hs, vt_hs = n * hd, plan.n_vt_blocks * hd * 64
    qkv = bf(c.qkv, 8)
    cos, sin = g1("f32", c.cos), g1("f32", c.sin)
    lists = [g1("i32", plan.blk_tok0.astype(np.int32)), g1("i32", plan.blk_ntok.astype(np.int32)),
             g1("i32", plan.blk_k_row0.astype(np.int64).view(np.int32)), g1("i32", plan.blk_vt_blk.astype(np.int64).view(np.int32))]
    q_out = g1("bf16", n=H * n * hd, role="out")
    k_out, vt_out = g1("bf16", n=int(np.prod(k_shape)), role="out"), g1("bf16", n=int(np.prod(vt_shape)), role="out")
    L.kr_qkv_prep(qkv.ptr, qkv.ld, 0, qd, qd + kd, cos.ptr, sin.ptr, lists[0].ptr, lists[1].ptr, lists[2].ptr, lists[3].ptr,
                  len(plan.blk_tok0), q_out.ptr, n * hd, k_out.ptr, k_hs, vt_out.ptr, vt_hs, H, KVH, hd, 0)
    eq_bits(q_out.read().reshape(H, n, hd), c.q, "q")
    poison = k_out.poison
    want_k = np.full(k_shape, poison, U16)
    want_v = np.full((vt_shape[0], vt_shape[1] * 64, hd), poison, U16)          # as rows
    tok = 0
    for s, ln in enumerate(lens):
        pad = (ln + 63) // 64 * 64
        for h in range(KVH):
            if as_cache:
                want_k[s * KVH + h, :ln] = c.k[tok:tok + ln, h]
                want_v[s * KVH + h, :pad] = 0
                want_v[s * KVH + h, :ln] = c.v[tok:tok + ln, h]
            else:
                want_k[h, tok:tok + ln] = c.k[tok:tok + ln, h]
                b0 = int(plan.blk_vt_blk[[i for i in range(len(plan.blk_tok0)) if plan.blk_tok0[i] == tok][0]]) * 64
                want_v[h, b0:b0 + pad] = 0
                want_v[h, b0:b0 + ln] = c.v[tok:tok + ln, h]
        tok += ln
    eq_bits(k_out.read().reshape(k_shape), want_k, "K rows (and everything else untouched)")
    eq_bits(POS.vt_rows(vt_out.read().reshape(vt_shape)), want_v, "V^T blocks (padding zero, everything else untouched)")
    untouched(qkv=qkv, cos=cos, sin=sin, q=q_out, k=k_out, vt=vt_out, **{f"list{i}": g for i, g in enumerate(lists)})


@pytest.mark.parametrize("d", E.NORM_D)
@pytest.mark.parametrize("rows", [1, 9])
def test_rmsnorm_exact(L, d, rows):
    rng = np.random.default_rng(d + rows)
    xv, wv = E.norm_rows(rng, rows, d), E.norm_weights(rng, d)
    x, w = bf(xv, pad_for(rows)), bf1(wv)
    y = g1("bf16", n=rows * d, role="out")
    L.kr_rmsnorm(x.ptr, x.ld, w.ptr, y.ptr, rows, d, E.EPS, 0)
    eq_bits(y.read().reshape(rows, d), E.bits16(E.rms_ref(xv, wv)), "rmsnorm")
    untouched(x=x, w=w, y=y)


@pytest.mark.parametrize("d", E.LN_D)
@pytest.mark.parametrize("rows", [1, 5, 130])
def test_layernorm_exact(L, d, rows):
    xv, wv, bv, yv = E.ln_case(rows, d)
    x, w, b = g1("bf16", E.bits16(xv)), bf1(wv), bf1(bv)
    y = g1("bf16", n=rows * d, role="out")
    L.kr_layernorm(x.ptr, w.ptr, b.ptr, y.ptr, rows, d, E.EPS, 0)
    eq_bits(y.read().reshape(rows, d), E.bits16(yv), "layernorm")
    untouched(x=x, w=w, b=b, y=y)
