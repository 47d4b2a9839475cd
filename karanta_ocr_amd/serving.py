"""OpenAI-chat-completions surface of the MI355X engine — the boundary the reference talks to.

The reference never calls a model in-process: ``process_page`` POSTs ``build_page_query``'s dict to
``{server}/chat/completions`` (/root/reference/karanta/pipeline.py:115-171, :317-344) and the bulk
workers go through ``VLLMClient.generate`` (/root/reference/bulk_processing/workers/vllm_client.py:
155-227).  This module turns exactly that request dict into engine work and the engine's tokens
back into exactly the response JSON those callers parse:

    choices[0].message.content, choices[0].finish_reason in {"stop","length"},
    usage.{prompt_tokens, completion_tokens, total_tokens}, model

Status codes follow what ``process_page`` distinguishes (pipeline.py:321-332): 200, 400 (bad
request: caller skips the attempt), 500 (internal error: caller retries).

``temperature`` is honoured (0 or absent: greedy — the reference's ``build_page_query`` default, pipeline.py:170;
``process_page`` sends 0.1 on its first attempt, :281,:301): Gumbel-max sampling from softmax(logits / T)
(kr_gumbel_argmax), reproducible through the OpenAI ``seed`` field, a random seed per request otherwise.
``top_k`` / ``top_p`` / ``min_p`` / ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` are applied with
vLLM's semantics and validation (sampling.py; kr_sample_threshold / kr_gumbel_argmax_processed); ``honor_temperature=False``
(``--greedy``) ignores them with the temperature.  ``logit_bias`` / ``min_tokens`` / ``stop_token_ids`` are applied on the device
(sampling.parse_adjust_fields; kr_logits_adjust / kr_stop_tokens) and ``stop`` strings (``include_stop_str_in_output``) by the
scheduler between decode chunks (sampling.StopStrings); ``--greedy`` ignores all of these too.
``n`` (an integer >= 1; ``n > 1`` needs ``temperature > 0``, as in vLLM; ``best_of`` must equal it): the response carries
``choices[0..n-1]``, choice c being exactly what the same request with ``n = 1`` and ``seed + c`` returns (without a ``seed``
the server draws one base seed) — but the images go through the ViT once and the prompt through the prefill once, and the
children start from copies of its KV rows (kr_kv_fork).  ``usage.prompt_tokens`` counts the prompt once, ``completion_tokens``
is the sum over the choices.  ``n`` above the server's decode slots is a 400; ``--greedy`` serves ``n`` as 1.
``--enable-prefix-caching`` (``LocalServer(prefix_cache=True)``, continuous mode): a request whose whole prompt (token ids,
grids, image bytes) equals one still resident in a decode slot starts from that slot's rows, without ViT or prefill — the
reference's retry loop (the same page again at a higher temperature, pipeline.py ``process_page``) becomes decode-only.
``guided_regex`` / ``response_format`` / ``logprobs``: guided.py, engine.
``repetition_detection`` (vLLM's field: ``{"max_pattern_size", "min_pattern_size", "min_count", "min_span"}``; ``false`` / ``null``:
off for this request; absent: the server's ``--repetition-detection`` default, which is off unless given): the sequence ends with
``finish_reason: "length"`` and ``stop_reason: "repetition"`` at the token its output starts to repeat at (kr_repeat_detect, inside
the decode step).  It changes no token choice, so ``--greedy`` honours it.  Every choice carries ``stop_reason`` (``null`` otherwise).

Prompt text: the checkpoint's own ``chat_template`` when the model directory ships one (``chat_template.json`` /
``chat_template.jinja`` / ``tokenizer_config.json`` — what vLLM applies, pipeline.py:707-734), rendered with jinja2; the
hand-coded Qwen2-VL template otherwise.
"""
from __future__ import annotations

import hashlib
import json
import queue
import threading
import time
import uuid
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import image_processing as IP
from .config import ModelConfig
from .request import PageRequest
from .sampling import NEUTRAL, StopStrings, parse_adjust_fields, parse_repetition_field, parse_request_fields

DEFAULT_SYSTEM = "You are a helpful assistant."


def load_chat_template(model_dir: str) -> Optional[str]:
    """The checkpoint's chat template, as `transformers` / vLLM look it up: ``chat_template.jinja``, ``chat_template.json``
    (``{"chat_template": ...}``: the processor's file on Qwen2-VL checkpoints), then ``tokenizer_config.json``'s
    ``chat_template`` (a string, or a list of ``{"name", "template"}`` whose "default" entry is taken).  None when the
    directory has none: the caller falls back to the hand-coded Qwen2-VL template."""
    import os
    try:
        with open(os.path.join(model_dir, "chat_template.jinja"), encoding="utf-8") as f:
            return f.read()
    except OSError:
        pass
    for name in ("chat_template.json", "tokenizer_config.json"):
        try:
            with open(os.path.join(model_dir, name), encoding="utf-8") as f:
                t = json.load(f).get("chat_template")
        except (OSError, ValueError, AttributeError):
            continue
        if isinstance(t, list):
            named = {e.get("name"): e.get("template") for e in t if isinstance(e, dict)}
            t = named.get("default") or next(iter(named.values()), None)
        if isinstance(t, str) and t.strip():
            return t
    return None


# ----------------------------------------------------------------------------- tokenizers
class ByteTokenizer:
    """Tokenizer of last resort (tests, random-init models): UTF-8 bytes as ids 0..255.
    Special tokens keep the model's own ids.  Real checkpoints use :class:`HFTokenizer`."""

    def __init__(self, cfg: ModelConfig, im_start: Optional[int] = None, im_end: Optional[int] = None):
        self.cfg = cfg
        self.im_start = im_start if im_start is not None else min(cfg.text.vocab_size - 1, 151644)
        self.im_end = im_end if im_end is not None else cfg.eos_token_ids[0]
        self.newline = 10

    def encode(self, text: str) -> List[int]:
        return list(text.encode("utf-8"))

    def decode(self, ids: Sequence[int]) -> str:
        special = set(self.cfg.eos_token_ids) | {self.im_start, self.cfg.pad_token_id}
        return bytes(int(i) for i in ids if 0 <= int(i) < 256 and int(i) not in special).decode("utf-8", "replace")

    def token_bytes(self) -> List[bytes]:
        """Byte string of every token id (guided decoding matches patterns against these); b"" = never allowed."""
        special = set(self.cfg.eos_token_ids) | {self.im_start, self.cfg.pad_token_id}
        V = self.cfg.text.vocab_size
        return [bytes([i]) if i < 256 and i not in special else b"" for i in range(V)]


class HFTokenizer:
    """``tokenizer.json`` of a real Qwen2-VL checkpoint through the `tokenizers` library."""

    def __init__(self, path: str, cfg: ModelConfig):
        from tokenizers import Tokenizer

        self.tk = Tokenizer.from_file(path)
        self.cfg = cfg
        self.im_start = self.tk.token_to_id("<|im_start|>")
        self.im_end = self.tk.token_to_id("<|im_end|>")
        self.newline = self.tk.encode("\n", add_special_tokens=False).ids[0]

    def encode(self, text: str) -> List[int]:
        return self.tk.encode(text, add_special_tokens=False).ids

    def decode(self, ids: Sequence[int]) -> str:
        return self.tk.decode([int(i) for i in ids], skip_special_tokens=True)

    def token_bytes(self) -> List[bytes]:
        from .guided import vocab_bytes_from_hf
        return vocab_bytes_from_hf(self.tk, self.cfg.text.vocab_size)


# ----------------------------------------------------------------------------- request parsing
class BadRequest(ValueError):
    """Maps to HTTP 400 (the reference skips the attempt, pipeline.py:321-324)."""


@dataclass
class ParsedRequest:
    input_ids: np.ndarray
    pixel_values: Optional[np.ndarray]
    grids: List[Tuple[int, int, int]]
    max_tokens: int
    model: str
    temperature: float = 0.0
    seed: Optional[int] = None      # None: the server draws one per request
    images: Optional[List[np.ndarray]] = None   # device_images front end: decoded HWC uint8 pages instead of pixel_values
    guide: Any = None               # guided.Guide compiled from guided_regex / response_format (None: unconstrained)
    logprobs: Optional[int] = None  # None: not asked; k: log-prob of every token + top_logprobs = k alternatives
    # vLLM's sampling controls (sampling.parse_request_fields: validated, neutral when absent)
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    repetition_penalty: float = 1.0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    # vLLM's logit adjustments and stop conditions (sampling.parse_adjust_fields: validated, off when absent)
    logit_bias: Optional[Dict[int, float]] = None
    min_tokens: int = 0
    stop_token_ids: Tuple[int, ...] = ()
    stop: Tuple[str, ...] = ()
    include_stop_str_in_output: bool = False
    n: int = 1                      # choices to return (parallel sampling)
    prompt_key: Optional[bytes] = None   # ChatFrontend(prompt_keys): 16-byte digest of prompt ids, grids and image bytes
    # repetition_detection: the request's own RepetitionParams, or None with repetition_set = True where it switched detection off;
    # repetition_set = False: the field was absent and the server's default applies
    repetition: Any = None
    repetition_set: bool = False


ADJUST_FIELDS = ("logit_bias", "min_tokens", "stop_token_ids")


class ChatFrontend:
    """messages -> Qwen2-VL chat-template token ids + image patches.

    Template (Qwen2-VL): ``<|im_start|>system\\n{sys}<|im_end|>\\n<|im_start|>user\\n{content}<|im_end|>\\n
    <|im_start|>assistant\\n``; an ``image_url`` part becomes ``<|vision_start|><|image_pad|>*T<|vision_end|>``
    in place, parts in message order (the reference puts the text first, the image second:
    /root/reference/karanta/data/utils.py:283-297)."""

    def __init__(self, cfg: ModelConfig, tokenizer, min_pixels: int = IP.MIN_PIXELS,
                 max_pixels: int = IP.MAX_PIXELS_CLASS_DEFAULT, max_model_len: int = 16384, device_images: bool = False,
                 chat_template: Optional[str] = None, upload_device: Optional[str] = None):
        self.cfg, self.tok = cfg, tokenizer
        # device_images + upload_device: the decoded page goes to HBM HERE, in the request's own thread and on a stream of its
        # own, instead of at admission on the scheduler thread (a blocking 3 MB copy per page with the GPU waiting behind it)
        self._upload_device, self._upload_stream = None, None
        if upload_device is not None and device_images:
            import torch
            if torch.cuda.is_available():
                self._upload_device = torch.device(upload_device)
                self._upload_stream = torch.cuda.Stream(device=self._upload_device)
        # the checkpoint's own jinja template (load_chat_template); None: the hand-coded Qwen2-VL turns below
        self._template = None
        if chat_template:
            import jinja2
            from jinja2.sandbox import ImmutableSandboxedEnvironment

            def raise_exception(msg):
                raise jinja2.exceptions.TemplateError(msg)

            def tojson(x, ensure_ascii=False, indent=None, separators=None, sort_keys=False):
                import json as _json
                return _json.dumps(x, ensure_ascii=ensure_ascii, indent=indent, separators=separators, sort_keys=sort_keys)

            def strftime_now(fmt):
                import datetime
                return datetime.datetime.now().strftime(fmt)

            # the environment transformers renders chat templates in (utils/chat_template_utils.py): sandboxed, trim / lstrip blocks,
            # loop controls ({% break %} / {% continue %}), tojson without HTML escaping, raise_exception, strftime_now
            env = ImmutableSandboxedEnvironment(trim_blocks=True, lstrip_blocks=True, extensions=["jinja2.ext.loopcontrols"])
            env.filters["tojson"] = tojson
            env.globals["raise_exception"] = raise_exception
            env.globals["strftime_now"] = strftime_now
            try:
                self._template = env.from_string(chat_template)
            except jinja2.exceptions.TemplateSyntaxError as e:
                # a template this environment cannot compile must not keep the server from starting: say so and serve with
                # the hand-coded Qwen2-VL turns
                import sys
                print(f"[karanta] chat template of the checkpoint does not compile ({e}); falling back to the hand-coded "
                      f"Qwen2-VL template", file=sys.stderr, flush=True)
                self._template = None
        self.min_pixels, self.max_pixels = min_pixels, max_pixels
        # True: only decode the image here; the engine resizes / normalises / patchifies it on the GPU
        # (Engine.patches_from_images, bit-identical to the host path) and 3 bytes per pixel cross PCIe
        self.device_images = bool(device_images)
        self.max_model_len = max_model_len  # reference --max_model_len default (pipeline.py:1225-1230)
        self._guide_cache: Dict[str, Any] = {}   # regex -> guided.Guide (the pipeline sends one pattern for every page)
        self.prompt_keys = False     # LocalServer(prefix_cache=True) switches it on: parse() computes ParsedRequest.prompt_key

    def _upload(self, u8: np.ndarray):
        """HWC uint8 page -> a tensor resident in HBM (Engine.patches_from_images takes it as it is).  The copy blocks this thread
        and the upload stream only; the request holds the tensor until it has been answered."""
        import torch
        with torch.cuda.stream(self._upload_stream):
            u8 = np.ascontiguousarray(u8)
            if not u8.flags.writeable:        # PIL-backed arrays are read-only views
                u8 = u8.copy()
            return torch.from_numpy(u8).to(self._upload_device)

    def _guide_for(self, req: Dict[str, Any]):
        """guided_regex (pipeline.py:304-307) / response_format (vllm_client.py:196) -> byte DFA, or None."""
        from .guided import GuideError, compile_regex, regex_for_request
        try:
            rx = regex_for_request(req.get("guided_regex"), req.get("response_format"))
            if rx is None:
                return None
            g = self._guide_cache.get(rx)
            if g is None:
                g = compile_regex(rx)
                if len(self._guide_cache) >= 64:
                    self._guide_cache.pop(next(iter(self._guide_cache)))
                self._guide_cache[rx] = g
            return g
        except GuideError as e:
            raise BadRequest(f"guided decoding: {e}") from e

    def _turn(self, role: str, body: List[int]) -> List[int]:
        t = self.tok
        return [t.im_start] + t.encode(role) + [t.newline] + body + [t.im_end, t.newline]

    def _special_ids(self) -> Dict[str, int]:
        return {"<|im_start|>": self.tok.im_start, "<|im_end|>": self.tok.im_end,
                "<|vision_start|>": self.cfg.vision_start_token_id, "<|vision_end|>": self.cfg.vision_end_token_id,
                "<|image_pad|>": self.cfg.image_token_id}

    def _ids_from_template(self, messages: List[dict], n_tok: List[int]) -> List[int]:
        """Render the checkpoint's template (`add_generation_prompt=True`, as vLLM does for a chat completion) and
        tokenise it: the special-token strings map to their ids here (so the byte tokenizer of the tests and the HF
        tokenizer agree), the text between them goes through the tokenizer, and the k-th ``<|image_pad|>`` becomes the
        k-th image's T placeholders — what the HF processor does to the rendered text
        (/root/reference/karanta/training/test_trained_model.py:77-87)."""
        import re

        import jinja2
        msgs = []
        for m in messages:
            c = m.get("content")
            if isinstance(c, list):   # OpenAI parts -> the shape HF templates test for ('image' in content / type == 'image')
                c = [({"type": "image", "image": ""} if p.get("type") in ("image_url", "image") else p) for p in c]
            msgs.append({**m, "content": c})
        try:
            text = self._template.render(messages=msgs, add_generation_prompt=True, add_vision_id=False, bos_token="",
                                         eos_token="<|im_end|>", pad_token="<|endoftext|>", unk_token="")
        except jinja2.exceptions.TemplateError as e:
            raise BadRequest(f"chat template: {e}") from e
        except Exception as e:  # noqa: BLE001  — a template bug on this request's shape is the client's 400, not a 500
            raise BadRequest(f"chat template: {type(e).__name__}: {e}") from e
        sp = self._special_ids()
        ids: List[int] = []
        k = 0
        for piece in re.split("(" + "|".join(re.escape(x) for x in sp) + ")", text):
            if not piece:
                continue
            if piece == "<|image_pad|>":
                if k >= len(n_tok):
                    raise BadRequest("chat template: more image placeholders than images")
                ids += [sp[piece]] * n_tok[k]
                k += 1
            elif piece in sp:
                ids.append(sp[piece])
            else:
                ids += self.tok.encode(piece)
        if k != len(n_tok):
            raise BadRequest(f"chat template rendered {k} image placeholders for {len(n_tok)} images")
        return ids

    def parse(self, req: Dict[str, Any]) -> ParsedRequest:
        if not isinstance(req, dict) or not isinstance(req.get("messages"), list) or not req["messages"]:
            raise BadRequest("`messages` must be a non-empty list")
        mt = req.get("max_tokens", req.get("max_completion_tokens"))
        max_tokens = 100 if mt is None else int(mt)
        if max_tokens < 1:
            raise BadRequest("max_tokens must be >= 1")
        n = req.get("n")
        n = 1 if n is None else n
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise BadRequest("n must be an integer >= 1")
        if req.get("best_of") is not None and (isinstance(req["best_of"], bool) or req["best_of"] != n):
            raise BadRequest("best_of must equal n (only the n returned candidates are generated)")
        key = hashlib.blake2b(digest_size=16) if self.prompt_keys else None
        ids: List[int] = []
        pvs, grids, images, n_toks = [], [], [], []
        hand = self._template is None        # the hand-coded Qwen2-VL turns; with the checkpoint's own template only the images are
        #                                      collected here and the template decides roles, order and text (no double tokenisation)
        if hand and req["messages"][0].get("role") != "system":
            ids += self._turn("system", self.tok.encode(DEFAULT_SYSTEM))
        for msg in req["messages"]:
            role, content = msg.get("role"), msg.get("content")
            if hand and role not in ("system", "user", "assistant"):
                raise BadRequest(f"unsupported role {role!r}")
            body: List[int] = []
            parts = [{"type": "text", "text": content}] if isinstance(content, str) else content
            if not isinstance(parts, list):
                raise BadRequest("message content must be a string or a list of parts")
            for part in parts:
                kind = part.get("type")
                if kind == "text":
                    if hand:
                        body += self.tok.encode(part.get("text", ""))
                elif kind in ("image_url", "image"):
                    url = part["image_url"]["url"] if kind == "image_url" else part["image"]
                    try:
                        img = IP.decode_data_url(url)
                    except Exception as e:  # undecodable image -> 400, like vLLM
                        raise BadRequest(f"cannot decode image: {e}") from e
                    u8 = np.asarray(img.convert("RGB"), dtype=np.uint8) if self.device_images or key is not None else None
                    if key is not None:          # the decoded host bytes (about 3 MB per page), before any upload
                        key.update(repr(u8.shape).encode() + u8.tobytes())
                    if self.device_images:
                        unit = self.cfg.vision.patch_size * self.cfg.vision.spatial_merge_size
                        try:
                            rh, rw = IP.smart_resize(u8.shape[0], u8.shape[1], unit, self.min_pixels, self.max_pixels)
                        except ValueError as e:
                            raise BadRequest(str(e)) from e
                        grid = (1, rh // self.cfg.vision.patch_size, rw // self.cfg.vision.patch_size)
                        images.append(self._upload(u8) if self._upload_device is not None else u8)
                    else:
                        pv, grid = IP.image_to_patches(img, self.min_pixels, self.max_pixels)
                        pvs.append(pv)
                    grids.append(grid)
                    n_tok = grid[0] * grid[1] * grid[2] // (self.cfg.vision.spatial_merge_size ** 2)
                    n_toks.append(n_tok)
                    body += [self.cfg.vision_start_token_id] + [self.cfg.image_token_id] * n_tok + [self.cfg.vision_end_token_id]
                else:
                    raise BadRequest(f"unsupported content part {kind!r}")
            if hand:
                ids += self._turn(role, body)
        if hand:
            ids += [self.tok.im_start] + self.tok.encode("assistant") + [self.tok.newline]
        else:
            ids = self._ids_from_template(req["messages"], n_toks)
        if len(ids) + max_tokens > self.max_model_len:
            raise BadRequest(f"prompt ({len(ids)} tokens) + max_tokens ({max_tokens}) exceeds max_model_len {self.max_model_len}")
        try:
            temperature = float(req.get("temperature") or 0.0)
            seed = None if req.get("seed") is None else int(req["seed"]) & 0xFFFFFFFF
        except (TypeError, ValueError) as e:
            raise BadRequest(f"temperature / seed: {e}") from e
        if not (0.0 <= temperature <= 100.0):   # NaN fails both comparisons
            raise BadRequest("temperature must be in [0, 100]")
        if n > 1 and temperature == 0.0:
            raise BadRequest("n must be 1 when using greedy sampling (temperature 0)")
        logprobs = None
        if req.get("logprobs"):
            try:
                logprobs = int(req.get("top_logprobs") or 0)
            except (TypeError, ValueError) as e:
                raise BadRequest(f"top_logprobs: {e}") from e
            if not 0 <= logprobs <= 20:
                raise BadRequest("top_logprobs must be in 0..20")
        try:
            controls = parse_request_fields(req)
            guide = self._guide_for(req)
            controls.update(parse_adjust_fields(req, self.cfg.text.vocab_size, max_tokens, guided=guide is not None,
                                                eos_token_ids=self.cfg.eos_token_ids))
            if "repetition_detection" in req:
                controls.update(repetition=parse_repetition_field(req["repetition_detection"]), repetition_set=True)
        except BadRequest:
            raise
        except ValueError as e:
            raise BadRequest(str(e)) from e
        ids_arr = np.asarray(ids, np.int64)
        if key is not None:
            key.update(ids_arr.tobytes() + repr([tuple(int(x) for x in g) for g in grids]).encode())
        return ParsedRequest(ids_arr, np.concatenate(pvs, 0) if pvs else None, grids, max_tokens,
                             str(req.get("model", "karantaocr")), temperature, seed, images or None,
                             guide, logprobs, n=n, prompt_key=key.digest() if key is not None else None, **controls)


# ----------------------------------------------------------------------------- in-process server
class LocalServer:
    """Scheduler in front of one engine (one GPU).  Thread-safe: callers block in :meth:`chat_completions`
    while a worker thread runs the engine.

    ``continuous=False``: static batching — whatever is waiting (up to the engine's max batch) goes into one
    ``generate`` call and leaves together.  ``continuous=True``: the slot scheduler (scheduler.SlotScheduler) —
    a request leaves as soon as it hits EOS or its ``max_tokens`` and the next waiting request is prefilled into
    its slot while the others keep decoding; ``max_tokens_cap`` bounds any request's ``max_tokens`` and
    ``chunk`` is the number of decode steps between two looks at the device's finished flags (with launch_ahead the next chunk is
    queued before the look: scheduler.SlotScheduler)."""

    def __init__(self, engine, frontend: ChatFrontend, served_model_name: str = "karantaocr",
                 batch_wait_s: float = 0.005, log=print, continuous: bool = False, max_tokens_cap: int = 4096,
                 chunk: int = 2, honor_temperature: bool = True, max_logprobs: Optional[int] = None, admit_min: int = 1,
                 admit_max_wait: int = 16, overlap_admissions: bool = False, launch_ahead: bool = True,
                 prefix_cache: bool = False, speculative: bool = False, repetition=None):
        self.engine, self.frontend, self.name = engine, frontend, served_model_name
        # the default of the requests without a repetition_detection field (RepetitionParams, its dict form, or None: off)
        self.repetition = parse_repetition_field(repetition)
        # prompt-lookup speculative decoding (vLLM's --speculative-config, method ngram): continuous mode, an engine built with
        # speculative=SpecConfig(...), and log-probabilities only on an engine that records them in speculative steps
        # (SpecConfig(logprobs=True); SlotScheduler(speculative=True))
        self.speculative = bool(speculative)
        if self.speculative and (not continuous or not getattr(engine, "K", 0)
                                 or (max_logprobs is not None and not getattr(engine, "spec_logprobs", False))):
            raise ValueError("speculative=True needs continuous=True, max_logprobs=None and an engine built with "
                             "speculative=SpecConfig(...) (max_logprobs: one built with SpecConfig(logprobs=True))")
        self.honor_temperature = bool(honor_temperature)   # False: every request is served greedy
        # guided decoding needs the tokenizer's byte strings on the device; engines without set_vocab (test fakes)
        # answer guided requests with 400
        self.guided = hasattr(engine, "set_vocab") and hasattr(frontend.tok, "token_bytes")
        if self.guided:
            engine.set_vocab(frontend.tok.token_bytes())
        # continuous mode: the decode graph records log-probabilities only when this is set (top_logprobs bound,
        # vLLM's --max-logprobs); static mode decides per batch
        self.max_logprobs = None if max_logprobs is None else int(max_logprobs)
        self.batch_wait_s, self.log = batch_wait_s, log
        self.continuous, self.max_tokens_cap, self.chunk = bool(continuous), int(max_tokens_cap), int(chunk)
        self.admit_min, self.admit_max_wait = int(admit_min), int(admit_max_wait)   # SlotScheduler's admission batching
        # continuous mode: ViT + prefill of an admission on a second (CU-masked: Engine(admission_cus=...)) stream while the
        # other slots keep decoding (SlotScheduler(overlap=True))
        self.overlap_admissions = bool(overlap_admissions)
        self.launch_ahead = bool(launch_ahead)
        # prompt reuse (vLLM's --enable-prefix-caching): continuous mode only, engines with admit_reuse; the front end then keys
        # every request by its whole prompt
        self.prefix_cache = bool(prefix_cache) and self.continuous and hasattr(engine, "admit_reuse")
        if self.prefix_cache:
            frontend.prompt_keys = True
        self._tok_bytes = None       # the tokenizer's byte strings, fetched once for the stop-string matchers
        self._q: "queue.Queue" = queue.Queue()
        self._running = 0
        self._stop = False
        self.pages_done = 0
        self._t_start = time.time()
        self.latencies: List[float] = []
        self._thread = threading.Thread(target=self._loop_continuous if self.continuous else self._loop, daemon=True)
        self._thread.start()
        # the reference watches the server's output for one of these lines (pipeline.py:790-800)
        self.log("Starting vLLM API server (karanta MI355X engine)")

    # -- public surface -------------------------------------------------------
    def health(self) -> Tuple[int, dict]:
        return 200, {"status": "ok", "engine": "karanta-mi355x", "running": self._running, "waiting": self._q.qsize()}

    def metrics(self) -> Tuple[int, dict]:
        """Pages served and request latency percentiles (the reference computes neither)."""
        lat = sorted(self.latencies[-10000:])
        pct = lambda q: float(lat[min(len(lat) - 1, int(q * len(lat)))]) if lat else None
        up = max(1e-9, time.time() - self._t_start)
        return 200, {"pages_done": self.pages_done, "uptime_s": round(up, 3), "pages_per_s": round(self.pages_done / up, 4),
                     "running": self._running, "waiting": self._q.qsize(),
                     "latency_s": {"p50": pct(0.50), "p95": pct(0.95), "p99": pct(0.99), "n": len(lat)},
                     "scheduler": self.scheduler_stats(), "kv_cache": self.kv_cache_stats()}

    def scheduler_stats(self) -> Optional[dict]:
        """Continuous mode: where the scheduler thread's wall time went and how full the decode slots were."""
        sch = getattr(self, "_sch", None)
        if sch is None:
            return None
        return {"decode_steps": sch.steps, "slot_occupancy": round(sch.slot_steps_busy / max(1, sch.steps * sch.n_slots), 4),
                "admissions": sch.admissions, "pages_admitted": sch.pages_admitted,
                "sequences_admitted": sch.sequences_admitted, "sequences_forked": sch.sequences_forked,
                "prefix_cache_hits": sch.prefix_cache_hits,
                # speculative decoding (vLLM's counter names): drafts proposed / accepted, decode steps of either kind
                "spec_decode_num_draft_tokens": sch.spec_draft_tokens, "spec_decode_num_accepted_tokens": sch.spec_accepted_tokens,
                "spec_decode_steps": sch.spec_steps, "plain_decode_steps": sch.plain_steps,
                # repetition detection: sequences it ended, and the tokens up to their max_tokens that were not generated
                "repetition_stops": sch.repetition_stops, "repetition_tokens_cut": sch.repetition_tokens_cut,
                "host_phase_s": {k: round(v, 3) for k, v in sch.phase_s.items()}}

    def models(self) -> Tuple[int, dict]:
        return 200, {"object": "list", "data": [{"id": self.name, "object": "model", "owned_by": "karanta"}]}

    def chat_completions(self, req: Dict[str, Any]) -> Tuple[int, dict]:
        t0 = time.time()
        try:
            parsed = self.frontend.parse(req)
        except BadRequest as e:
            return 400, {"error": {"message": str(e), "type": "BadRequestError", "code": 400}}
        except Exception as e:  # malformed beyond recognition
            return 400, {"error": {"message": f"malformed request: {e}", "type": "BadRequestError", "code": 400}}
        if parsed.guide is not None and not self.guided:
            return 400, {"error": {"message": "guided decoding is not available on this server", "type": "BadRequestError", "code": 400}}
        if parsed.logprobs is not None and self.continuous and (self.max_logprobs is None or parsed.logprobs > self.max_logprobs):
            return 400, {"error": {"message": f"logprobs: this server records at most {self.max_logprobs} top_logprobs "
                                              "(start it with --max-logprobs)", "type": "BadRequestError", "code": 400}}
        if not self.honor_temperature:
            parsed.n = 1                  # --greedy: one greedy candidate, like the other generation controls
        if parsed.n > int(self.engine.B):
            return 400, {"error": {"message": f"n = {parsed.n} exceeds this server's {int(self.engine.B)} decode slots",
                                   "type": "BadRequestError", "code": 400}}
        room = self.engine.seq_room() if hasattr(self.engine, "seq_room") else None
        over = self.chunk * (2 if self.launch_ahead and not self.overlap_admissions else 1)   # steps past its limit (scheduler.over)
        if self.speculative:
            over *= int(self.engine.K) + 1        # a speculative step emits up to K + 1 tokens
        need = len(parsed.input_ids) + min(int(parsed.max_tokens), self.max_tokens_cap) + (over if self.continuous else 0)
        if room is not None and need > room:
            # the request's OWN prompt + max_tokens against one sequence's cache rows: a client error for this request
            # only (the reference skips the attempt on 400, pipeline.py:321-332) — never an engine exception that
            # would fail the requests admitted with it
            return 400, {"error": {"message": f"prompt ({len(parsed.input_ids)} tokens) + max_tokens ({parsed.max_tokens}) "
                                              f"exceeds this server's sequence capacity ({room})",
                                   "type": "BadRequestError", "code": 400}}
        slot: Dict[str, Any] = {"req": parsed, "done": threading.Event()}
        self._q.put(slot)
        slot["done"].wait()
        if "error" in slot:
            code = int(slot.get("status", 500))
            kind = "BadRequestError" if code == 400 else "InternalServerError"
            return code, {"error": {"message": slot["error"], "type": kind, "code": code}}
        self.latencies.append(time.time() - t0)
        if len(self.latencies) > 20000:          # bounded: /metrics reads the last 10000
            del self.latencies[:10000]
        choices, n_out = [], 0
        for c, ch in enumerate(slot["choices"]):           # one per child, in child order
            toks = ch["tokens"]
            text = ch["text"] if ch.get("text") is not None else self.frontend.tok.decode(toks)   # "text": cut at a stop string
            choice: Dict[str, Any] = {"index": c, "message": {"role": "assistant", "content": text}, "finish_reason": ch["reason"],
                                      "stop_reason": ch.get("stop_reason")}
            if parsed.logprobs is not None:
                choice["logprobs"] = self._logprobs_json(toks, ch.get("logprobs"), parsed.logprobs)
            choices.append(choice)
            n_out += int(len(toks))
        n_in = int(len(parsed.input_ids))                  # the prompt counts once
        return 200, {
            "id": "chatcmpl-" + uuid.uuid4().hex, "object": "chat.completion", "created": int(time.time()),
            "model": req.get("model", self.name),
            "choices": choices,
            "usage": {"prompt_tokens": n_in, "completion_tokens": n_out, "total_tokens": n_in + n_out},
        }

    def _logprobs_json(self, toks, lp, k: int) -> Optional[dict]:
        """OpenAI chat `logprobs` object: per generated token its text, log-prob, bytes and the top-k alternatives."""
        if lp is None:
            return None
        tok = self.frontend.tok
        piece = lambda i: tok.decode([int(i)])
        item = lambda i, v: {"token": piece(i), "logprob": float(v), "bytes": list(piece(i).encode("utf-8"))}
        n = min(len(toks), len(lp["token"]))
        return {"content": [dict(item(toks[i], lp["token"][i]),
                                 top_logprobs=[item(lp["top_ids"][i][j], lp["top"][i][j]) for j in range(min(k, lp["top"].shape[1]))])
                            for i in range(n)]}

    def close(self):
        self._stop = True
        self._q.put(None)
        self._thread.join(timeout=5)

    # -- scheduler --------------------------------------------------------------
    def _loop(self):
        carry = None             # a request that did not fit the previous batch's rows
        while not self._stop:
            first = carry if carry is not None else self._q.get()
            carry = None
            if first is None:
                break
            batch = [first]
            rows = first["req"].n            # a batch is packed by sequences: sum(n) <= engine.B
            deadline = time.time() + self.batch_wait_s
            while rows < self.engine.B:
                try:
                    nxt = self._q.get(timeout=max(0.0, deadline - time.time()))
                except queue.Empty:
                    break
                if nxt is None:
                    self._stop = True
                    break
                if rows + nxt["req"].n > self.engine.B:
                    carry = nxt
                    break
                batch.append(nxt)
                rows += nxt["req"].n
            self._running = len(batch)
            # same shape as vLLM's periodic stats line that the reference scrapes (pipeline.py:782-800)
            self.log(f"Running: {self._running} reqs, Waiting: {self._q.qsize()} reqs")
            for group in self._static_groups(batch):
                try:
                    pages = [self._page(s["req"]) for s in group]
                    res = self.engine.generate(pages, max(s["req"].max_tokens for s in group))
                    self._log_kv_clamped()
                    i = 0                    # the result's rows: a request's children consecutive
                    for s in group:
                        for c in range(s["req"].n):
                            lps = res.logprobs[i] if getattr(res, "logprobs", None) is not None else None
                            why = res.stop_reasons[i] if getattr(res, "stop_reasons", None) is not None else None
                            self._finish(s, res.tokens[i], res.finish_reasons[i], c, lps, why)
                            i += 1
                except Exception as e:  # engine failure -> 500 for every request of the group
                    for s in group:
                        s["error"] = f"{type(e).__name__}: {e}"
            self.pages_done += len(batch)
            self._running = 0
            for s in batch:
                s["done"].set()
        if carry is not None:     # stopped with a request held over for the next batch: nobody is left waiting forever
            carry["error"] = "server shutting down"
            carry["done"].set()


    def _log_kv_clamped(self):
        """fp8 KV cache: one line per admission that had to clamp values on their way into the cache (an operator running on
        scales of 1.0, or on scales that do not fit the model, must see it)."""
        self._log_kv_scales()
        n = int(getattr(self.engine, "kv_clamped", 0) or 0)
        if n > getattr(self, "_kv_clamped_seen", 0):
            self.log(f"fp8 KV cache: the last admission clamped {n - getattr(self, '_kv_clamped_seen', 0)} K/V elements to +-448 x scale "
                     f"({n} since start; scales: {getattr(self.engine, 'kv_scale_source', '?')})")
            self._kv_clamped_seen = n

    def _log_kv_scales(self):
        """--calculate-kv-scales: ONE line once the calibrating admission has run — where the scales come from and their spread.  From
        then on the clamp line above is the signal that a later page outgrew the first admission's headroom."""
        if getattr(self, "_kv_scales_logged", False) or not getattr(self.engine, "kv_scales_ready", False):
            return
        self._kv_scales_logged = True
        sc = self.engine.kv_scales()
        self.log(f"fp8 KV cache scales: {self.engine.kv_scale_source}; K scales {sc[:, 0].min():.6g} .. {sc[:, 0].max():.6g}, "
                 f"V scales {sc[:, 1].min():.6g} .. {sc[:, 1].max():.6g}")

    def kv_cache_stats(self) -> Optional[dict]:
        """/metrics: the KV cache's dtype and, for an fp8 cache, where its scales come from and what the admissions clamped."""
        eng = self.engine
        dtype = getattr(eng, "kv_cache_dtype", None)
        if dtype is None:
            return None
        if not getattr(eng, "kv8", False):
            return {"dtype": dtype}
        return {"dtype": dtype, "scale_source": getattr(eng, "kv_scale_source", None), "clamped": int(getattr(eng, "kv_clamped", 0) or 0)}

    def _static_groups(self, batch):
        """A static batch decodes every sequence for the LONGEST max_tokens of the batch, so a long prompt with a small
        limit can overflow its cache rows next to a short prompt with a large one although both fit alone (each was
        checked at the door).  Split such a batch into groups that fit together; normally one group."""
        room = self.engine.seq_room() if hasattr(self.engine, "seq_room") else None
        if room is None:
            return [batch]
        groups: List[list] = []
        for s in sorted(batch, key=lambda s: -int(s["req"].max_tokens)):
            for g in groups:
                mt = max(int(x["req"].max_tokens) for x in g + [s])
                if all(len(x["req"].input_ids) + mt <= room for x in g + [s]):
                    g.append(s)
                    break
            else:
                groups.append([s])
        return groups

    def _stop_strings(self, r: ParsedRequest) -> Optional[StopStrings]:
        """The matcher of a request's `stop` strings, on the tokenizer's byte strings where it has them (None: no stop strings,
        or --greedy, which ignores them with the other generation controls)."""
        stops = getattr(r, "stop", None)
        if not stops or not self.honor_temperature:
            return None
        tok = self.frontend.tok
        if self._tok_bytes is None and hasattr(tok, "token_bytes"):
            self._tok_bytes = tok.token_bytes()
        return StopStrings(stops, getattr(r, "include_stop_str_in_output", False), self._tok_bytes,
                           None if self._tok_bytes is not None else tok.decode)

    def _page(self, r: ParsedRequest):
        import random
        page = PageRequest(r.input_ids, r.pixel_values, r.grids, images=getattr(r, "images", None))
        if getattr(r, "guide", None) is not None:
            page.guide = r.guide
        if getattr(r, "logprobs", None) is not None:
            page.logprobs = r.logprobs
        if self.honor_temperature and r.temperature > 0:
            page.temperature = r.temperature
            page.seed = r.seed if r.seed is not None else random.getrandbits(32)   # the base seed: child c samples with seed + c
            page.n = int(getattr(r, "n", 1))
        if self.honor_temperature:        # --greedy: the plain greedy path, sampling controls ignored as well
            for name in NEUTRAL:
                setattr(page, name, getattr(r, name, NEUTRAL[name]))
            for name in ADJUST_FIELDS:
                if getattr(r, name, None):
                    setattr(page, name, getattr(r, name))
        # repetition detection chooses no token: --greedy serves it too.  The request's field wins over the server's default
        page.repetition = getattr(r, "repetition", None) if getattr(r, "repetition_set", False) else self.repetition
        return page

    def _finish(self, s: Dict[str, Any], toks, reason: str, c: int = 0, logprobs=None, stop_reason: Optional[str] = None):
        """Child c of a request is through: its tokens as the response reports them -> s["choices"][c]."""
        mt = s["req"].max_tokens
        if len(toks) > mt:       # (a static batch decodes for its longest member: this one's own limit came first)
            toks, reason, stop_reason = toks[:mt], "length", None
        eos = set(int(e) for e in self.engine.cfg.eos_token_ids)
        if self.honor_temperature:
            eos |= set(int(t) for t in getattr(s["req"], "stop_token_ids", None) or ())
        if reason == "stop" and len(toks) and int(toks[-1]) in eos:
            toks = toks[:-1]  # the EOS token (or the stop id that ended the sequence) is not part of the message content
        # stop strings: the earliest match cuts the text; usage counts through the token that completed it.  (Continuous mode:
        # the scheduler has already stopped the sequence there with this matcher; static mode: generation ran on.)
        m = s["stops"][c] if s.get("stops") is not None else self._stop_strings(s["req"])   # matchers keep state: one per child
        text = None
        if m is not None:
            keep = m.check(toks)
            if keep is not None:
                toks, reason, text, stop_reason = toks[:keep], "stop", m.text, None
        n = max(1, int(getattr(s["req"], "n", 1)))
        s.setdefault("choices", [None] * n)[c] = {"tokens": toks, "reason": reason, "text": text, "logprobs": logprobs,
                                                      "stop_reason": stop_reason}

    def _spec_kw(self) -> dict:
        return {"speculative": True} if self.speculative else {}      # (only named when on: test fakes of the scheduler's engine)

    def _rep_kw(self) -> dict:
        return {"repetition": self.repetition} if self.repetition is not None else {}      # (only named when set, as above)

    def _loop_continuous(self):
        from .scheduler import SlotRequest, SlotScheduler

        try:
            sch = SlotScheduler(self.engine, self.max_tokens_cap, self.chunk, sampling=self.honor_temperature,
                                guided=self.guided, logprobs=self.max_logprobs, admit_min=self.admit_min,
                                admit_max_wait=self.admit_max_wait, overlap=self.overlap_admissions,
                                launch_ahead=self.launch_ahead, prefix_cache=self.prefix_cache, **self._spec_kw(), **self._rep_kw())
        except Exception as e:  # cannot enter slot mode: every request gets a 500
            sch, boot_error = None, f"{type(e).__name__}: {e}"
        self._sch = sch
        last = (-1, -1)
        while not self._stop:
            # block only when there is nothing to decode; otherwise take what has arrived and keep stepping
            try:
                first = self._q.get(block=sch is None or sch.idle, timeout=None)
            except queue.Empty:
                first = False
            got = [] if first is False else [first]
            while True:
                try:
                    got.append(self._q.get_nowait())
                except queue.Empty:
                    break
            for s in got:
                if s is None:
                    self._stop = True
                elif sch is None:
                    s["error"] = boot_error
                    s["done"].set()
                else:
                    r = s["req"]
                    s["stops"] = [self._stop_strings(r) for _ in range(r.n)]
                    sch.submit(SlotRequest(self._page(r), max(1, int(r.max_tokens)), tag=s, stop_check=s["stops"][0],
                                           stop_checks=s["stops"] if r.n > 1 else None,
                                           prompt_key=r.prompt_key if self.prefix_cache else None,
                                           repetition_off=getattr(r, "repetition_set", False) and r.repetition is None))
            if self._stop or sch is None:
                continue
            try:
                results = sch.step()
            except Exception as e:  # engine failure mid-flight: everything in a slot or waiting fails, slot mode restarts
                msg = f"{type(e).__name__}: {e}"
                lost = {id(r): r for r in list(sch.active.values()) + list(sch.waiting)}   # a request with n children is in n slots
                for r in lost.values():
                    r.tag["error"] = msg
                    r.tag["done"].set()
                self.pages_done += len(lost)
                try:
                    sch = SlotScheduler(self.engine, self.max_tokens_cap, self.chunk, sampling=self.honor_temperature,
                                        guided=self.guided, logprobs=self.max_logprobs, admit_min=self.admit_min,
                                        admit_max_wait=self.admit_max_wait, overlap=self.overlap_admissions,
                                        launch_ahead=self.launch_ahead, prefix_cache=self.prefix_cache, **self._spec_kw(), **self._rep_kw())
                except Exception as e2:
                    sch, boot_error = None, f"{type(e2).__name__}: {e2}"
                self._sch = sch
                continue
            self._running = sch.running
            self._log_kv_clamped()
            now = (sch.running, len(sch.waiting) + self._q.qsize())
            if now != last:  # vLLM's stats line, printed when it changes (pipeline.py:782-800 scrapes it)
                self.log(f"Running: {now[0]} reqs, Waiting: {now[1]} reqs")
                last = now
            for res in results:
                s = res.tag
                if res.error:
                    s["error"] = res.error
                    s["status"] = getattr(res, "status", 500)
                else:
                    for c, ch in enumerate(res.choices if getattr(res, "choices", None) else [res]):
                        self._finish(s, ch.tokens, ch.finish_reason, c, ch.logprobs, getattr(ch, "stop_reason", None))
                self.pages_done += 1
                s["done"].set()
        # shutting down: nobody is left waiting forever
        if sch is not None:
            for r in list(sch.active.values()) + list(sch.waiting):
                r.tag["error"] = "server shutting down"
                r.tag["done"].set()


# registry used by the in-process VLLMClient (clients.py): port -> LocalServer
_LOCAL_SERVERS: Dict[Tuple[str, int], LocalServer] = {}


def register_local_server(port: int, server: LocalServer, host: str = "localhost") -> None:
    _LOCAL_SERVERS[(host, int(port))] = server


def unregister_local_server(port: int, host: str = "localhost") -> None:
    _LOCAL_SERVERS.pop((host, int(port)), None)


def local_server(host: str, port: int) -> Optional[LocalServer]:
    return _LOCAL_SERVERS.get((host, int(port))) or (_LOCAL_SERVERS.get(("localhost", int(port))) if host in ("127.0.0.1", "localhost") else None)


# ----------------------------------------------------------------------------- HTTP shim
def serve_http(server: LocalServer, port: int, host: str = "127.0.0.1"):
    """OpenAI-compatible HTTP front (``POST /v1/chat/completions``, ``GET /v1/models``, ``GET /health``)
    so the unmodified reference (``karanta.pipeline --server http://host:port/v1``, the Celery workers'
    ``VLLMClient``) can point at this engine.  Returns the running ``ThreadingHTTPServer``."""
    from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

    class Handler(BaseHTTPRequestHandler):
        protocol_version = "HTTP/1.1"

        def log_message(self, *a):  # --disable-log-requests
            pass

        def _send(self, status: int, body: dict):
            data = json.dumps(body).encode()
            self.send_response(status)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(data)))
            self.send_header("Connection", "close")
            self.end_headers()
            self.wfile.write(data)
            self.close_connection = True

        def do_GET(self):
            path = self.path.split("?")[0].rstrip("/")
            if path == "/health":
                self._send(*server.health())
            elif path in ("/v1/models", "/models"):
                self._send(*server.models())
            elif path == "/metrics":
                self._send(*server.metrics())
            else:
                self._send(404, {"error": {"message": "not found", "code": 404}})

        def do_POST(self):
            path = self.path.split("?")[0].rstrip("/")
            if path not in ("/v1/chat/completions", "/chat/completions"):
                return self._send(404, {"error": {"message": "not found", "code": 404}})
            try:
                n = int(self.headers.get("Content-Length", "0"))
                req = json.loads(self.rfile.read(n))
            except Exception as e:
                return self._send(400, {"error": {"message": f"invalid JSON: {e}", "type": "BadRequestError", "code": 400}})
            self._send(*server.chat_completions(req))

    httpd = ThreadingHTTPServer((host, port), Handler)
    httpd.daemon_threads = True
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    server.log("The server is fired up and ready to roll!")
    return httpd
