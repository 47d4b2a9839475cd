"""The OpenAI surface of a speculative server that records log-probabilities (beside
tests/test_gpu_engine.py::test_server_guided_json_and_logprobs): LocalServer(speculative=True, max_logprobs=5) on an engine built
with SpecConfig(guided=True, logprobs=True) answers the reference's bulk request shape — `logprobs: true, top_logprobs: 5` and a
`response_format` — with the `choices[0].logprobs` JSON of the server without speculation, and /metrics shows accepted drafts.
(Fails on a tree without the feature: SpecConfig takes no `logprobs`.)"""
import json

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd import image_processing as IP  # noqa: E402
from karanta_ocr_amd import serving as S  # noqa: E402
from karanta_ocr_amd.config import CONFIGS  # noqa: E402
from karanta_ocr_amd.engine import Engine, SpecConfig  # noqa: E402
from karanta_ocr_amd.weights import random_weights  # noqa: E402

CFG = CONFIGS["tiny-w512"]
KW = dict(max_batch=2, s_max=512, max_patches=2048, max_prompt_tokens=2048, decode_splits=2)


def test_speculative_server_answers_logprobs_as_the_plain_server():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    w = random_weights(CFG, 909)
    front = S.ChatFrontend(CFG, S.ByteTokenizer(CFG))
    url = IP.encode_png_data_url(IP.synthetic_page(44, 56, 84))
    msg = [{"role": "user", "content": [{"type": "text", "text": "page"}, {"type": "image_url", "image_url": {"url": url}}]}]
    schema = {"type": "object", "properties": {"lang": {"type": ["string", "null"], "maxLength": 3}, "rot": {"enum": [0, 90]},
                                               "tab": {"type": "boolean"}}, "required": ["lang", "rot", "tab"]}
    reqs = [{"messages": msg, "max_tokens": 80, "temperature": 0.1, "seed": 5, "logprobs": True, "top_logprobs": 5,
             "response_format": {"type": "json_schema", "json_schema": {"name": "p", "schema": schema, "strict": True}}},
            {"messages": msg, "max_tokens": 12, "temperature": 0.0, "logprobs": True, "top_logprobs": 2},
            {"messages": msg, "max_tokens": 6, "temperature": 0.0}]
    plain = Engine(CFG, **KW)
    plain.load_weights(w)
    srv = S.LocalServer(plain, front, log=lambda *_: None, continuous=True, max_tokens_cap=96, chunk=2, max_logprobs=5)
    want = [srv.chat_completions(r) for r in reqs]
    srv.close()
    plain.close()
    assert all(st == 200 for st, _ in want)
    doc = json.loads(want[0][1]["choices"][0]["message"]["content"])
    assert list(doc) == ["lang", "rot", "tab"] and want[0][1]["choices"][0]["finish_reason"] == "stop"
    items = want[0][1]["choices"][0]["logprobs"]["content"]
    assert "".join(i["token"] for i in items) == want[0][1]["choices"][0]["message"]["content"]
    assert all(len(i["top_logprobs"]) == 5 for i in items)

    # an engine without the flag: the server refuses the combination, as before
    off = Engine(CFG, speculative=SpecConfig(3, guided=True), **KW)
    with pytest.raises(ValueError, match="max_logprobs"):
        S.LocalServer(off, front, log=lambda *_: None, continuous=True, max_tokens_cap=96, chunk=2, max_logprobs=5, speculative=True)
    off.close()

    spec = Engine(CFG, speculative=SpecConfig(3, guided=True, logprobs=True), **KW)
    spec.load_weights(w)
    srv = S.LocalServer(spec, front, log=lambda *_: None, continuous=True, max_tokens_cap=96, chunk=2, max_logprobs=5, speculative=True)
    try:
        # the drafts of both slots: the JSON document the plain server produced, so that drafts are accepted
        text = want[0][1]["choices"][0]["message"]["content"].encode()
        for j in range(2):
            spec.set_draft_script(j, list(text))
        got = [srv.chat_completions(r) for r in reqs]
        st, m = srv.metrics()
    finally:
        srv.close()
        spec.close()
    for i, ((s0, b0), (s1, b1)) in enumerate(zip(want, got)):
        assert s0 == s1 == 200, (i, b1)
        c0, c1 = b0["choices"][0], b1["choices"][0]
        assert c0["message"]["content"] == c1["message"]["content"] and c0["finish_reason"] == c1["finish_reason"], f"request {i}"
        assert c0.get("logprobs") == c1.get("logprobs"), f"request {i}: choices[0].logprobs"
        assert json.dumps(c0.get("logprobs"), sort_keys=True) == json.dumps(c1.get("logprobs"), sort_keys=True)
    assert got[2][1]["choices"][0].get("logprobs") is None
    sch = m["scheduler"]
    assert st == 200 and sch["spec_decode_steps"] > 0
    assert sch["spec_decode_num_draft_tokens"] >= sch["spec_decode_num_accepted_tokens"] > 0
