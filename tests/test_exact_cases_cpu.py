"""The dyadic cases of tests/exact_cases.py, proven without a GPU: every parametrised case passes check_case (exactly
representable operands, every partial sum below 2^24 units, enough outputs that need the rounding, enough ties) and its
float64 reference changes, in at least the stated share of outputs, under each mutation a faulty kernel could be: one k
element dropped or duplicated (first, last, both sides of every 64-boundary of the launch's K partition), truncation,
round-half-away, a rounding before the residual, the bias added after the rounding, no pre-rotary rounding, a rounding
between the two slab adds, gate and up swapped, the bias of the neighbouring 16-row tile."""
import numpy as np
import pytest

from tests import exact_cases as E

F64 = np.float64
LINEAR = E.linear_case_list()


@pytest.mark.parametrize("cid,args,cuts", LINEAR, ids=[c[0] for c in LINEAR])
def test_linear_case_is_exact_and_sensitive(cid, args, cuts):
    c = E.linear_case(*args)           # check_case runs where the case is built
    shares = E.linear_mutation_shares(c, cuts)
    print(cid, {k: round(v, 3) for k, v in shares.items()})
    assert set(shares) >= {"drop_k", "dup_k", "truncate", "half_away", "round_before_residual", "bias_after_rounding"}
    assert not E.missed_shares(c, cuts), f"{cid}: {E.missed_shares(c, cuts)} below {[E.min_share(k, c.K) for k in shares]}"


@pytest.mark.parametrize("M,N,K", [(10753, 1536, 320)])
def test_float32_blas_reference_equals_float64(M, N, K):
    """The tall cases take their reference from a float32 BLAS product: with every partial sum below 2^24 it is the
    float64 one (full_pre compares the proof rows; here every row of the smaller tall case)."""
    c = E.linear_case(M, N, K)
    fast = c.full_pre()
    rows = np.arange(0, M, 7)
    np.testing.assert_array_equal(fast[rows], c.pre(c.acc(rows), rows))


@pytest.mark.parametrize("K", E.NORM_D)
def test_rmsnorm_rows_are_exact_under_a_perturbed_rsqrt(K):
    rng = np.random.default_rng(K)
    x, w = E.norm_rows(rng, 9, K), E.norm_weights(rng, K)
    h = E.rms_ref(x, w)               # asserts O.rms_norm(policy bf16) == w * x / 2
    for ulps in (-8, -1, 0, 1, 8):
        np.testing.assert_array_equal(E.rms_ref_perturbed(x, w, ulps), h)
    assert len(np.unique(np.abs(x))) == 4 and len(np.unique(w)) == 6


@pytest.mark.parametrize("d", E.LN_D)
def test_layernorm_rows_are_exact_under_a_perturbed_rsqrt(d):
    x, w, b, y = E.ln_case(5, d)
    for ulps in (-8, -1, 0, 1, 8):
        np.testing.assert_array_equal(E.ln_ref_perturbed(x, w, b, ulps), y)


@pytest.mark.parametrize("M,K,n_part", E.NARROW_NORM)
@pytest.mark.parametrize("fp8", [False, True])
def test_norm_prologue_case_is_exact_and_sensitive(M, K, n_part, fp8):
    nl = E.norm_linear_case(M, E.NORM_N, K, n_part, fp8)
    if n_part:
        total = nl.x.astype(F64) + nl.parts.astype(F64).sum(0)
        assert (E.rne(total) == nl.x_new).all() and E.needs_rounding(total).mean() >= 0.75
        for order in ([0, 1], [1, 0])[:n_part]:            # exact in f32 in every association
            s = nl.x.astype(np.float32)
            for i in order[:n_part]:
                s = s + nl.parts[i]
            assert (s.astype(F64) == total).all()
        assert E.is_tie(total).mean() >= E.MIN_TIES
    if n_part == 2:
        assert E.double_rounding_share(nl.x, nl.parts) >= E.min_share_round_between_slabs()
    assert not E.missed_shares(nl.lin, E.k_partition(K, 8))


@pytest.mark.parametrize("H,KVH,K", E.ROPE_SHAPES)
@pytest.mark.parametrize("fp8", [False, True])
def test_rope_case_is_exact_and_sensitive(H, KVH, K, fp8):
    c = E.rope_case(16, H, KVH, K, 2, fp8)                   # asserts >= 50 % of t need the pre-rotary rounding
    lin = c.nl.lin
    pre = lin.full_pre()
    q2, k2, _ = E.rope_outputs(c, pre)                       # no pre-rotary rounding
    assert (q2 != c.q).mean() >= 0.10 and (k2 != c.k).mean() >= 0.10
    qt, kt, _ = E.rope_outputs(c, c.t, E.trunc_bits)
    assert (qt != c.q).mean() >= 0.09
    # one k element dropped from the projection: t, and with it q / k / v
    for k in E.drop_positions(K, E.k_partition(K, 8)):
        rank1 = np.outer(lin.A[:, k].astype(F64), lin.W[:, k].astype(F64) * (1 if lin.w_scale is None else lin.w_scale))
        t2 = E.rne(pre - rank1)
        assert (t2 != c.t).mean() >= 0.5
    assert {0, 63, 64} <= set(c.ctx.tolist()) and 0 in c.step.tolist() and 0 in c.plen.tolist()
    # sin and cos exchanged, the halves exchanged
    assert ((c.cs[..., :64] != c.cs[..., 64:]).mean()) > 0.5


@pytest.mark.parametrize("epi", E.ACT_EPILOGUES)
def test_activation_formula_in_float32_meets_the_bracket_rule(epi):
    M, N, K = E.act_shape(epi)
    c = E.act_case(M, N, K, bias=epi in ("quick_gelu", "gelu_erf", "silu_mul8_bias"))
    pre = c.full_pre()
    name = epi.replace("_bias", "")
    ref = E.act_ref(name, pre)
    f32 = E.act_ref(name, pre, np.float32)
    ok = E.bracket_ok(E.to_bf16_bits(f32.astype(np.float32)), ref)
    assert ok.all(), f"{(~ok).sum()} of {ok.size} float32 evaluations leave the bracket"
    assert not E.bracket_ok(E.to_bf16_bits((f32 * np.float32(1.02)).astype(np.float32)), ref).all()     # the rule can fail
    if name.startswith("silu_mul"):      # gate and up exchanged
        grp = 16 if name == "silu_mul" else 8
        sw = pre.reshape(M, N // (2 * grp), 2, grp)[:, :, ::-1].reshape(M, N)
        assert (E.to_bf16_bits(E.act_ref(name, sw).astype(np.float32)) != E.to_bf16_bits(ref.astype(np.float32))).mean() >= 0.5


@pytest.mark.parametrize("hd,H,KVH", E.PREP_HEADS)
def test_prep_case_needs_its_rounding(hd, H, KVH):
    c = E.prep_case(hd, H, KVH)
    assert c.q.shape == (H, sum(c.lens), hd) and c.k.shape == (sum(c.lens), KVH, hd)
    assert (c.cos[:, :hd // 2] != c.cos[:, hd // 2:]).mean() > 0.5      # the halves have their own tables: an exchange shows


def test_argmax_logits_tie():
    for (N, K, _, _) in E.WIDE_SHAPES:
        c = E.argmax_case(16, N, K)          # asserts that every row's maximum occurs at least twice
        assert (c.ref_f32().argmax(1) < N // 2).all()


def test_guarded_catches_a_write_outside_the_tensor():
    torch = pytest.importorskip("torch")
    g = E.Guarded(torch, "cpu", "bf16", 5, 16, ld=24, role="out")
    body = g.dev[g.front:g.front + 5 * 24].view(5, 24)
    body[:, :16] = 1
    g.assert_untouched()
    assert (g.read() == 1).all()
    for where in (g.front - 1, g.front + 16, g.front + 5 * 24, g.dev.numel() - 1):     # band, padding column, guard row, end band
        h = E.Guarded(torch, "cpu", "bf16", 5, 16, ld=24, role="out")
        h.dev[where] = 0
        with pytest.raises(AssertionError):
            h.assert_untouched()
    i = E.Guarded(torch, "cpu", "f32", 3, 8, ld=16, role="in", init=np.arange(24, dtype=np.float32))
    i.assert_untouched()
    assert np.isnan(i.host().view(np.float32)[:E.Guarded.BAND]).all()
    i.dev[i.front] = 7
    with pytest.raises(AssertionError):
        i.assert_untouched()
