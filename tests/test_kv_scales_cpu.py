"""--calculate-kv-scales without a GPU: the numpy rule of tests/kv_scales_ref.py on its own (with its scales the quantiser of
tests/kv_fp8_ref.py clamps nothing and the extremum lands on the range), its edge cases, and the flag and the two environment
variables from the command line to the Engine's keywords on the stand-in engine of test_kv_fp8_cpu.py."""
import types

import numpy as np
import pytest

from karanta_ocr_amd import cli
from karanta_ocr_amd import weights as W
from karanta_ocr_amd.config import CONFIGS
from karanta_ocr_amd.tools import synthetic_checkpoint as SC
from tests import kv_fp8_ref as R
from tests import kv_scales_ref as S

F32 = np.float32


def scratch(rng, slots=4, kvh=2, s_max=192, hd=128, spread=(3.0, 0.02)):
    """Token-major bf16 K and V whose heads differ in size (head h of K is 1 + h times as large)."""
    k = W.bf16_round((rng.standard_normal((slots, kvh, s_max, hd)) * spread[0]).astype(F32) * (1 + np.arange(kvh, dtype=F32))[None, :, None, None])
    v = W.bf16_round((rng.standard_normal((slots, kvh, s_max, hd)) * spread[1]).astype(F32))
    return k, v


# ----------------------------------------------------------------------------- the rule
def test_with_its_scales_nothing_clamps_and_the_extremum_lands_on_the_range():
    """scale = fl(a / r) with a relative error of at most 2^-24, so a / scale lies within r * 2^-24 of r before its own rounding —
    less than one ulp of r for r = 200 and r = 100 (both 1.5625 x a power of two: r * 2^-24 = 0.78 ulp) — and the nearest f32 to it
    is r or a neighbour of r: the largest |quotient| is within ONE f32 ulp of the range.  Every other |x| <= a has a quotient no
    larger (division by a positive number is monotonic), far below 448."""
    rng = np.random.default_rng(11)
    k, v = scratch(rng)
    plan = [(2, 130), (0, 1), (3, 64), (1, 65)]
    sc = S.scales_kv(k, v, plan)
    assert sc.shape == (2, 2) and sc.dtype == F32
    for which, (x, r) in enumerate(((k, S.K_RANGE), (v, S.V_RANGE))):
        for h in range(2):
            rows = np.concatenate([x[s, h, :n].reshape(-1) for s, n in plan])
            assert sc[which, h] == F32(np.abs(rows).max()) / F32(r)                     # restated once more, by hand
            codes, clamped = R.quantize(rows, sc[which, h])
            assert not clamped.any()
            top = np.abs((rows / sc[which, h]).astype(F32)).max()
            assert abs(float(top) - r) <= float(np.spacing(F32(r))), (which, h, top)
            assert W.fp8_e4m3_to_f32(codes).max() <= 208                                 # the code next to 200 is 192 or 208
    assert sc[0, 1] > 1.5 * sc[0, 0]                                                     # the heads have scales of their own
    # rows at or beyond len and slots outside the plan do not count
    k2, v2 = k.copy(), v.copy()
    k2[1, :, 65:], v2[1, :, 65:], k2[0, :, 1:], v2[3, :, 64:] = 9984.0, np.nan, np.inf, -9984.0
    np.testing.assert_array_equal(S.scales_kv(k2, v2, plan).view(np.uint32), sc.view(np.uint32))
    k2[3] = 9984.0
    np.testing.assert_array_equal(S.scales_kv(k2, v2, plan[:2] + plan[3:]).view(np.uint32), S.scales_kv(k, v, plan[:2] + plan[3:]).view(np.uint32))
    # the V^T block layout round-trips
    np.testing.assert_array_equal(S.vt_to_tokens(R.vt_blocks8(v)), v)
    np.testing.assert_array_equal(S.scales_scratch(k, R.vt_blocks8(v), plan), sc)


def test_edge_cases():
    one = lambda vals, r=200.0: float(S.scale_of(S.amax_finite(np.asarray(vals, F32)), r))
    assert one([0.0, -0.0, 0.0]) == 1.0                                                  # an all-zero head
    assert one([np.nan, np.inf, -np.inf]) == 1.0                                         # nothing finite
    assert one([np.nan, 3.0, np.inf, -np.inf, 1.0]) == float(F32(3.0) / F32(200.0))      # NaN / inf are skipped
    assert one([1.0, -50.0, 2.0]) == 0.25                                                # a negative extremum
    tiny = 2.0 ** -126                                                                   # exact in bf16; / 200 is far below FLT_MIN
    assert one([tiny, 0.0]) == float(S.FLT_MIN) == float(np.finfo(F32).tiny)
    assert one([2.0 ** -133]) == float(S.FLT_MIN)                                        # the smallest bf16 subnormal
    assert one([F32(2.0 ** -126) * F32(256.0)], 100.0) == float(F32(2.0 ** -118) / F32(100.0)) > float(S.FLT_MIN)
    big = float(W.bf16_round(np.asarray([3.3e38], F32))[0])
    assert one([big, -1.0]) == float(F32(big) / F32(200.0))
    assert S.scale_of(np.asarray([0.0, 400.0], F32), 100.0).tolist() == [1.0, 4.0]


# ----------------------------------------------------------------------------- the flag and the environment
def test_ranges_from_the_environment():
    assert W.KV_SCALE_RANGES == (200.0, 100.0) == (S.K_RANGE, S.V_RANGE)
    assert W.kv_scale_ranges_from_env({}) == (200.0, 100.0)
    assert W.kv_scale_ranges_from_env({"K_SCALE_CONSTANT": "448", "V_SCALE_CONSTANT": "12.5"}) == (448.0, 12.5)
    assert W.kv_scale_ranges_from_env({"V_SCALE_CONSTANT": "50"}) == (200.0, 50.0)
    for bad in ("0", "-3", "nan", "inf", "two hundred"):
        with pytest.raises(ValueError, match="K_SCALE_CONSTANT"):
            W.kv_scale_ranges_from_env({"K_SCALE_CONSTANT": bad})


def test_the_flag_parses():
    assert cli.parse_args(["serve", "/m"]).calculate_kv_scales is False
    a = cli.parse_args(["serve", "/m", "--kv-cache-dtype", "fp8", "--calculate-kv-scales"])
    assert a.calculate_kv_scales is True and "--calculate-kv-scales" not in a.ignored


def serve(monkeypatch, tmp_path, argv, kv_scales=None):
    """cli.make_server with a stand-in Engine: (the keywords it got, the scales set on it, the log lines)."""
    from karanta_ocr_amd import dp, engine, serving
    cfg = CONFIGS["tiny"]
    d = str(tmp_path / ("ckpt" + str(len(argv)) + ("s" if kv_scales else "")))
    SC.write_checkpoint(d, cfg, 0, kv_scales=kv_scales)
    seen = {}

    class FakeEngine:
        def __init__(self, cfg, **kw):
            seen.update(kw)
            self.kv_cache_dtype = W.kv_cache_dtype_name(kw["kv_cache_dtype"])
            self.kv8 = self.kv_cache_dtype == "fp8"
            self.s_max, self.w, self.s, self.kv_scale_source = kw["s_max"], None, 0, "default (1.0)"

        def kv_cache_bytes(self):
            return 3 << 20

        def set_kv_scales(self, k, v, source=""):
            seen["scales"], self.kv_scale_source = (np.asarray(k), np.asarray(v)), source

    monkeypatch.setattr(engine, "Engine", FakeEngine)
    monkeypatch.setattr(dp, "load_or_receive_weights", lambda *a, **k: {"bytes": 0})
    monkeypatch.setattr(serving, "LocalServer", lambda eng, front, **kw: types.SimpleNamespace(eng=eng))
    lines = []
    cli.make_server(cli.parse_args(["serve", d, "--host-images", *argv]), log=lines.append)
    return seen, lines


def test_make_server_hands_the_flag_and_the_ranges_to_the_engine(tmp_path, monkeypatch):
    monkeypatch.delenv("K_SCALE_CONSTANT", raising=False)
    monkeypatch.delenv("V_SCALE_CONSTANT", raising=False)
    seen, lines = serve(monkeypatch, tmp_path, ["--kv-cache-dtype", "fp8", "--calculate-kv-scales"])
    assert seen["calculate_kv_scales"] is True and seen["kv_scale_ranges"] == (200.0, 100.0) and "scales" not in seen
    assert any("to be calculated from the first admission (ranges 200 / 100)" in ln for ln in lines)
    monkeypatch.setenv("K_SCALE_CONSTANT", "300")
    monkeypatch.setenv("V_SCALE_CONSTANT", "25.5")
    seen, lines = serve(monkeypatch, tmp_path, ["--calculate-kv-scales", "--kv-cache-dtype", "fp8_e4m3"])
    assert seen["calculate_kv_scales"] is True and seen["kv_scale_ranges"] == (300.0, 25.5)
    assert any("ranges 300 / 25.5" in ln for ln in lines)
    # without the flag: the keywords do not appear, whatever the environment says
    seen, lines = serve(monkeypatch, tmp_path, ["--kv-cache-dtype", "fp8"])
    assert "calculate_kv_scales" not in seen and "kv_scale_ranges" not in seen
    assert any("scales: default (1.0)" in ln for ln in lines)


def test_the_flag_wins_over_checkpoint_scales_and_says_so(tmp_path, monkeypatch):
    nl = CONFIGS["tiny"].text.num_layers
    ck = (0.5 + np.arange(nl) / 4.0, 2.0 + np.arange(nl))
    seen, lines = serve(monkeypatch, tmp_path, ["--kv-cache-dtype", "fp8", "--calculate-kv-scales"], kv_scales=ck)
    assert seen["calculate_kv_scales"] is True and "scales" not in seen
    assert any("--calculate-kv-scales wins" in ln for ln in lines)
    seen, lines = serve(monkeypatch, tmp_path, ["--kv-cache-dtype", "fp8"], kv_scales=ck)
    assert "scales" in seen and not any("wins" in ln for ln in lines)


@pytest.mark.parametrize("dtype", [[], ["--kv-cache-dtype", "auto"], ["--kv-cache-dtype", "bfloat16"]])
def test_a_bf16_cache_logs_and_ignores_the_flag(tmp_path, monkeypatch, dtype):
    seen, lines = serve(monkeypatch, tmp_path, [*dtype, "--calculate-kv-scales"])
    assert "calculate_kv_scales" not in seen and "kv_scale_ranges" not in seen and "scales" not in seen
    assert sum("--calculate-kv-scales: ignored, the KV cache is bfloat16" in ln for ln in lines) == 1
    assert any(ln.startswith("KV cache: bf16") for ln in lines)


# ----------------------------------------------------------------------------- the server's line and /metrics
def test_the_server_logs_the_calibration_once_and_reports_the_cache():
    from karanta_ocr_amd.serving import LocalServer
    table = np.stack([np.stack([np.asarray([0.5, 0.25], F32), np.asarray([0.01, 0.04], F32)])] * 3)
    eng = types.SimpleNamespace(kv_cache_dtype="fp8", kv8=True, kv_scales_ready=False, kv_clamped=0, kv_scales=lambda: table,
                                kv_scale_source="calculated from the first admission (812 prompt tokens; ranges 200 / 100)")
    lines = []
    srv = types.SimpleNamespace(engine=eng, log=lines.append)
    srv._log_kv_scales = lambda: LocalServer._log_kv_scales(srv)
    LocalServer._log_kv_clamped(srv)
    assert lines == []                                                     # nothing before the calibrating admission has run
    eng.kv_scales_ready = True
    for _ in range(3):
        LocalServer._log_kv_clamped(srv)
    assert len(lines) == 1 and "calculated from the first admission (812 prompt tokens; ranges 200 / 100)" in lines[0]
    assert "K scales 0.25 .. 0.5" in lines[0] and "V scales 0.01 .. 0.04" in lines[0]
    eng.kv_clamped = 7
    LocalServer._log_kv_clamped(srv)
    assert len(lines) == 2 and "clamped 7 K/V elements" in lines[1]        # the per-admission clamp line stays
    assert LocalServer.kv_cache_stats(srv) == {"dtype": "fp8", "scale_source": eng.kv_scale_source, "clamped": 7}
    bf = types.SimpleNamespace(engine=types.SimpleNamespace(kv_cache_dtype="bf16", kv8=False))
    assert LocalServer.kv_cache_stats(bf) == {"dtype": "bf16"}
