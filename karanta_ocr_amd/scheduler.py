"""Continuous batching over the engine's fixed decode slots.

The reference leaves scheduling to vLLM (one server per GPU, `scripts/start_multiple_vllm_servers.sh:283`; the
pipeline only watches its `Running: n reqs, Waiting: m reqs` lines, `karanta/pipeline.py:769-800`).  Here the decode
hipGraph always steps all `max_batch` slots; a sequence that hits EOS (device flag) or its `max_tokens` (host) frees
its slot, and the next waiting request is prefilled into that slot while the other sequences keep their state —
instead of the whole batch waiting for its longest member (`Engine.generate`, static batching).  A request's own
`stop_token_ids` end it on the device as EOS does; its stop strings (`SlotRequest.stop_check`) are looked for at each harvest.
A page with `repetition` (RepetitionParams; `SlotScheduler(repetition=...)` is the default of the pages that carry none) is ended on
the device at the token its output starts to repeat at (kr_repeat_detect): "length" with `stop_reason` "repetition".

A request whose page asks for `n` sequences takes n slots at once (one ViT + prefill, the siblings' KV rows forked from child 0's
slot: `Engine.admit`); its children end one by one, each freeing its slot, and its one result carries them as `choices`.  With
`prefix_cache=True` a request whose `prompt_key` names a prompt still resident in a slot starts from that slot's rows
(`Engine.admit_reuse`): no ViT, no prefill.

Only the host logic lives here; it drives `Engine.begin_slots / admit / decode_steps / poll_slots / slot_tokens /
retire`, and any object with those six methods (the CPU tests use a fake) can stand in for the engine.
"""
from __future__ import annotations

import collections
import os
import time
from dataclasses import dataclass
from typing import Any, Callable, Deque, Dict, Iterable, List, Optional, Sequence

import numpy as np

from .sampling import StepFeatures


@dataclass
class SlotRequest:
    page: Any                 # engine.PageRequest
    max_tokens: int
    tag: Any = None           # returned untouched with the result
    # stop strings: called at every harvest with the tokens generated so far; returns how many to keep (through the token that
    # completed a match) or None.  Requests without one cause no token reads before they finish.
    stop_check: Optional[Callable[[np.ndarray], Optional[int]]] = None
    # n > 1: matchers keep state between calls, so such a request carries one per child (child c: stop_checks[c])
    stop_checks: Optional[Sequence[Callable[[np.ndarray], Optional[int]]]] = None
    # SlotScheduler(prefix_cache=True): identifies the whole prompt (token ids, grids, image bytes); requests with equal keys
    # share the prompt's KV rows while a slot still holds them
    prompt_key: Optional[bytes] = None
    # the request itself switched repetition detection off: the scheduler's default (SlotScheduler(repetition=...)) does not apply
    repetition_off: bool = False


@dataclass
class SlotResult:
    tag: Any
    tokens: np.ndarray        # generated ids, EOS included when finish_reason == "stop"
    finish_reason: str        # "stop" | "length"
    prompt_tokens: int
    error: Optional[str] = None
    request: Optional[SlotRequest] = None   # the request this answers
    status: int = 500                       # HTTP-style class of `error`: 400 = the request itself cannot be served
    logprobs: Optional[Dict[str, np.ndarray]] = None   # when the page asked for them (Engine.slot_logprobs)
    # page.n > 1: one SlotResult per child, in child order (the fields above are child 0's); None for n == 1
    choices: Optional[List["SlotResult"]] = None
    stop_reason: Optional[str] = None       # "repetition" where the page's RepetitionParams ended the sequence ("length"), else None


# Break-even of a speculative chunk: accepted drafts per slot and step below which plain steps emit more tokens per second,
# t_spec / t_plain - 1 for the step times of the two kinds.  UNMEASURED: this is README's 32-row over 8-row step time of the 2B
# decoder (1.68 / 1.15 ms), which predates the speculative step and lacks its proposer launch and its repeated K/V reads;
# csrc/tools/spec_bench.py measures the ratio and writes profiles/r05_spec_decode.json, from which this constant is to be set.
# The same constant serves SpecConfig(share_rows=True) above 16 slots, where it is too high: there the plain step is already the
# 32-row family, so the ratio is only the two extra launches (lookup, deal) and the drafts' repeated K/V reads — measured once,
# 24 slots x K = 3 at the 2B decoder: t_spec / t_plain = 1.098, break-even 0.098 (spec_bench.py --shared,
# profiles/r06_spec_shared_rows.json).  One constant is kept until both modes are measured: too high a constant only falls back to
# plain chunks sooner than it must.
SPEC_BREAK_EVEN = 1.68 / 1.15 - 1


class SpecPolicy:
    """When speculative chunks pay, as a pure host rule: over the last `window` speculative chunks that had live slots, the accepted
    drafts per slot and step must reach `break_even`; below it the scheduler runs plain chunks and probes again after `probe_after`
    of them.  `want()` names the next chunk's kind, `record()` takes what a speculative chunk's counters showed."""

    def __init__(self, break_even: float = SPEC_BREAK_EVEN, window: int = 16, probe_after: int = 64):
        if window < 1 or probe_after < 1:
            raise ValueError("window and probe_after must be >= 1")
        self.break_even, self.window, self.probe_after = float(break_even), int(window), int(probe_after)
        self._recent: Deque[tuple] = collections.deque(maxlen=self.window)    # (accepted drafts, slot-steps) per speculative chunk
        self._plain_left = 0

    def want(self) -> bool:
        """True: the next chunk is speculative.  A plain chunk asked for here counts towards the next probe."""
        if self._plain_left > 0:
            self._plain_left -= 1
            return False
        return True

    def record(self, accepted: int, slot_steps: int) -> None:
        if slot_steps <= 0:
            return
        self._recent.append((int(accepted), int(slot_steps)))
        if len(self._recent) == self.window and self.rate() < self.break_even:
            self._plain_left = self.probe_after
            self._recent.clear()             # the probe starts a fresh window

    def rate(self) -> float:
        """Accepted drafts per slot and step over the window (0 before the first record)."""
        steps = sum(n for _, n in self._recent)
        return sum(a for a, _ in self._recent) / steps if steps else 0.0


def _n(r: SlotRequest) -> int:
    """Sequences (slots) a request takes; pages without the attribute (older engines, test fakes) take one."""
    return int(getattr(r.page, "n", 1) or 1)


class SlotScheduler:
    """`submit()` requests, call `step()` until `idle`; every step admits what fits, runs `chunk` decode steps and
    returns the requests that finished."""

    def __init__(self, engine, max_tokens_cap: int, chunk: int = 8, eos_token_ids: Optional[Sequence[int]] = None,
                 max_prompt_tokens: Optional[int] = None, max_patches: Optional[int] = None, sampling: bool = False,
                 overlap: bool = False, guided: bool = False, logprobs: Optional[int] = None, admit_min: int = 1,
                 admit_max_wait: int = 4, launch_ahead: bool = True, prefix_cache: bool = False, speculative: bool = False,
                 spec_policy: Optional[SpecPolicy] = None, repetition=None):
        if max_tokens_cap < 1 or chunk < 1:
            raise ValueError("max_tokens_cap and chunk must be >= 1")
        self.engine = engine
        self.n_slots = int(engine.B)
        self.cap, self.chunk = int(max_tokens_cap), int(chunk)
        self.eos = set(int(e) for e in (eos_token_ids if eos_token_ids is not None else engine.cfg.eos_token_ids))
        self.max_prompt_tokens = max_prompt_tokens if max_prompt_tokens is not None else getattr(engine, "max_tokens", None)
        self.max_patches = max_patches if max_patches is not None else getattr(engine, "max_patches", None)
        self.waiting: Deque[SlotRequest] = collections.deque()
        self.active: Dict[int, SlotRequest] = {}     # slot -> request (a request with n children is in n slots)
        self.prompt_len: Dict[int, int] = {}
        self._child: Dict[int, int] = {}             # slot -> which child of its request runs there
        self._open: Dict[int, list] = {}             # id(request) -> its children's results so far (None: still running)
        # prompt reuse: per slot (key, prompt length) of the prompt whose rows [0, P) it holds — set when an admission has
        # completed, kept after the request's end, dropped when the slot is given to another prompt — and when the slot's
        # last sequence ended (cold admissions evict the resident prompt that finished longest ago)
        self.prefix_cache = bool(prefix_cache) and hasattr(engine, "admit_reuse")
        self._resident: Dict[int, tuple] = {}
        self._freed_at: Dict[int, int] = {}
        self._tick = 0
        # overlap: ViT + prefill of an admission run on a second stream while the other slots keep decoding
        # (Engine.admit_begin / admit_ready / admit_end); one admission in flight at a time
        self.overlap = bool(overlap) and all(hasattr(engine, m) for m in ("admit_begin", "admit_ready", "admit_end"))
        self._inflight = None                        # (handle, requests, slots)
        # launch-ahead (engines with snapshot_slots / read_snapshot): the NEXT decode chunk is queued before the host waits for the
        # previous chunk's slot flags, so harvesting, the server loop and the next admission's host work run while the GPU decodes.
        # A finished slot is seen one chunk later (a slot may run up to 2 * chunk - 1 steps past its limit), so it goes with SHORT
        # chunks: measured on the corpus run (profiles/r04_corpus_launch_ahead.txt) chunk 8 loses 1 % to the r3 loop (slot occupancy
        # 0.86 -> 0.84), chunks of 2 gain 2 % (29.6-29.9 against 29.15 pages/s) — the server's defaults.
        self.launch_ahead = (bool(launch_ahead) and not self.overlap
                             and all(hasattr(engine, m) for m in ("snapshot_slots", "read_snapshot")))
        # speculative: the chunks are speculative steps (Engine(speculative=SpecConfig(...)): up to K + 1 tokens per slot and step, the
        # same tokens) while the scheduler records no log-probabilities, unless the engine speculates on recording steps
        # (engine.spec_logprobs: SpecConfig(logprobs=True)), and no request in a slot needs sampling controls or logit adjustments, unless it
        # speculates on such steps (engine.spec_controls: SpecConfig(controls=True)), or guided decoding, unless it speculates on guided
        # steps (engine.spec_guided: SpecConfig(guided=True)) — and the policy finds them worth their price; every other chunk is plain
        self.speculative = bool(speculative)
        self.spec_k = int(getattr(engine, "K", 0) or 0) if self.speculative else 0
        if self.speculative and self.spec_k < 1:
            raise ValueError("speculative=True needs an engine built with speculative=SpecConfig(...)")
        self.spec_policy = (spec_policy or SpecPolicy()) if self.speculative else None
        self.spec_steps = self.plain_steps = 0       # decode steps of either kind
        self.spec_draft_tokens = self.spec_accepted_tokens = 0
        self._spec_seen = (0, 0)                     # the engine's counters (summed over the slots) at the last look
        # (snapshot number, slot-steps) of the speculative chunks whose counters the host has not seen yet
        self._spec_pending: Deque[tuple] = collections.deque()
        # a step may emit K + 1 tokens: the steps a slot runs past its limit before the host looks count K + 1 tokens each
        self.over = (2 if self.launch_ahead else 1) * int(chunk) * (self.spec_k + 1)
        self._snap = None                            # (sequence number, handle) of the chunk whose flags are read next
        self._snap_seq = 0                           # snapshots taken so far
        self._adm_seq: Dict[int, int] = {}           # slot -> snapshots taken when its request was admitted
        # Admission batching: while sequences are decoding, wait until `admit_min` slots are free (and as many requests
        # wait) before interrupting the decode graph with an admission — one ViT + prefill over several pages runs its
        # GEMMs at several times the rows of a single page — but never longer than `admit_max_wait` scheduler steps.
        self.admit_min, self.admit_max_wait = max(1, int(admit_min)), max(0, int(admit_max_wait))
        self._held = 0                               # scheduler steps the oldest admissible request has been held back
        # repetition detection: the default of the requests that neither carry their own parameters nor switch it off, and what it did
        self.repetition = repetition
        self.repetition_stops = 0                    # sequences ended by it
        self.repetition_tokens_cut = 0               # sum of max_tokens - completion_tokens over those
        self._rep_active = 0                         # sequences in the slots that carry it
        self._rep_on = False
        self.steps = 0                               # decode steps run
        # host wall time by phase (seconds): admission launches, decode-chunk launches, the wait for the GPU in _harvest
        self.phase_s = {"admit": 0.0, "decode_launch": 0.0, "harvest": 0.0}
        self.admissions = 0                          # admission rounds that carried pages
        self.pages_admitted = 0
        self.sequences_admitted = 0                  # sequences started (children counted one by one)
        self.sequences_forked = 0                    # ... of which from another slot's KV rows, without their own prefill
        self.prefix_cache_hits = 0                   # requests started by admit_reuse
        self.slot_steps_busy = 0                     # sum over steps of occupied slots (utilisation numerator)
        # a slot may run up to chunk - 1 steps past its limit before the host looks: size the history for that
        # sampling: pages may carry temperature > 0 (the decode graph then includes the Gumbel-max pass)
        # guided: pages may carry a pattern (masked sampling pass + DFA advance in the graph); logprobs = k: every step
        # records log-probabilities (top-k alternatives) for the pages that ask
        self.logprobs = logprobs
        kw = {}
        if sampling:
            kw["sampling"] = True
        if guided:
            kw["guided"] = True
        if logprobs is not None:
            kw["logprobs"] = int(logprobs)
        engine.begin_slots(self.cap + self.over, **kw)
        # engines that can switch the sampling / guided passes of the decode graph off while no request in a slot needs them
        self._features = ((sampling or guided) and hasattr(engine, "set_step_features")
                          and os.environ.get("KARANTA_STEP_FEATURES", "1") == "1")
        self._features_now = None
        # a greedy configuration has no optional pass but the repetition pass: it is switched with the requests that carry it
        self._rep_switch = not (sampling or guided) and hasattr(engine, "set_step_features")

    # ------------------------------------------------------------------ public
    def submit(self, req: SlotRequest) -> None:
        if req.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if self.repetition is not None and not req.repetition_off and getattr(req.page, "repetition", None) is None:
            req.page.repetition = self.repetition
        self.waiting.append(req)

    @property
    def idle(self) -> bool:
        return not self.waiting and not self.active and self._inflight is None

    @property
    def running(self) -> int:
        return len(self.active)

    def step(self) -> List[SlotResult]:
        if self.launch_ahead:
            return self._step_ahead()
        if not self.overlap:
            t0 = time.perf_counter()
            done: List[SlotResult] = self._admit()
            t1 = time.perf_counter()
            self.phase_s["admit"] += t1 - t0
            if self.active:
                self._decode_chunk()
                t2 = time.perf_counter()
                done += self._harvest()
                self.phase_s["decode_launch"] += t2 - t1
                self.phase_s["harvest"] += time.perf_counter() - t2
            return done
        # overlapped: finish an admission that is through, queue the decode chunk, THEN spend host time launching the
        # next admission (the GPU has both to run), then look at the finished flags
        done = self._finish_admission(block=not self.active)
        if self.active:
            self._decode_chunk()
        if self._inflight is None:
            done += self._admit(begin_only=True)
        if self.active:
            done += self._harvest()
        return done

    def _step_ahead(self) -> List[SlotResult]:
        done: List[SlotResult] = []
        t0 = time.perf_counter()
        if self.active:
            if self._snap is None:                   # nothing queued yet: this chunk's flags are the first to be read
                self._decode_chunk()
                self._snap = self._take_snapshot()
            self._decode_chunk()                     # the GPU's work while the host does everything below
            nxt = self._take_snapshot()
            t1 = time.perf_counter()
            fin, gen = self.engine.read_snapshot(self._snap[1])
            done += self._harvest((fin, gen), self._snap[0])
            self._snap = nxt if self.active else None
            t2 = time.perf_counter()
            self.phase_s["decode_launch"] += t1 - t0
            self.phase_s["harvest"] += t2 - t1
            t0 = t2
        done += self._admit()                        # queued behind the chunk that is executing
        self.phase_s["admit"] += time.perf_counter() - t0
        return done

    def _take_snapshot(self):
        seq = self._snap_seq
        self._snap_seq += 1
        return seq, self.engine.snapshot_slots()

    def _decode_chunk(self):
        if self._features:
            # the passes the steps carry follow the requests in the slots and the admission in flight, whose first token is
            # sampled on the decode stream (admit_end)
            pending = self._inflight[1] if self._inflight is not None else []
            need = StepFeatures.of(r.page for r in [*self.active.values(), *pending])
            if need != self._features_now:
                # (engines older than the adjustment pass take three arguments: it is only named when a request needs it)
                self.engine.set_step_features(need.sampling, need.guided, need.processing, **({"adjust": True} if need.adjust else {}),
                                              **({"repetition": True} if need.repetition else {}))
                self._features_now = need
        elif self._rep_switch and (self._rep_active > 0) != self._rep_on:
            self._rep_on = self._rep_active > 0
            self.engine.set_step_features(False, False, False, repetition=self._rep_on)
        if self._spec_chunk():
            self.engine.decode_steps(self.chunk, speculative=True)
            self.spec_steps += self.chunk
            self._spec_pending.append((self._snap_seq, self.chunk * len(self.active)))
        else:
            self.engine.decode_steps(self.chunk)
            self.plain_steps += self.chunk
        self.steps += self.chunk
        self.slot_steps_busy += self.chunk * len(self.active)

    def _spec_chunk(self) -> bool:
        """Whether the next chunk is speculative: the scheduler's mode, the requests in the slots (and in the admission in flight),
        the engine's own conditions, then the policy."""
        if not self.speculative:
            return False
        if self.logprobs is not None and not getattr(self.engine, "spec_logprobs", False):     # SpecConfig(logprobs=True)
            return False
        pending = self._inflight[1] if self._inflight is not None else []
        need = StepFeatures.of(r.page for r in [*self.active.values(), *pending])
        if (need.processing or need.adjust) and not getattr(self.engine, "spec_controls", False):   # SpecConfig(controls=True)
            return False
        if need.guided and not getattr(self.engine, "spec_guided", False):     # Engine(speculative=SpecConfig(guided=True))
            return False
        if hasattr(self.engine, "can_speculate") and not self.engine.can_speculate():
            return False
        return self.spec_policy.want()

    def _spec_account(self, counts, seq: Optional[int]) -> None:
        """counts: the engine's (proposed[B], accepted[B]) as of the flags being harvested — snapshot number `seq`, or (None) the
        device's state now.  What they gained since the last look belongs to the speculative chunks queued up to that point."""
        if counts is None:
            return
        prop, acc = int(np.sum(counts[0])), int(np.sum(counts[1]))
        d_prop, d_acc = prop - self._spec_seen[0], acc - self._spec_seen[1]
        self._spec_seen = (prop, acc)
        self.spec_draft_tokens += d_prop
        self.spec_accepted_tokens += d_acc
        slot_steps = 0
        while self._spec_pending and (seq is None or self._spec_pending[0][0] <= seq):
            slot_steps += self._spec_pending.popleft()[1]
        self.spec_policy.record(d_acc, slot_steps)

    def _finish_admission(self, block: bool) -> List[SlotResult]:
        if self._inflight is None:
            return []
        handle, batch, slots = self._inflight
        if not block and not self.engine.admit_ready(handle):
            return []
        self._inflight = None
        try:
            lens = self.engine.admit_end(handle)
        except Exception as e:
            return [self._failure(r, f"{type(e).__name__}: {e}") for r in batch]
        self._activate(batch, slots, lens)
        return []

    def _activate(self, batch, slots, lens, cold: bool = True):
        """The admitted requests' children are in their slots (slots / lens: one entry per sequence, children consecutive)."""
        k = 0
        for r in batch:
            n = _n(r)
            self._open[id(r)] = [None] * n
            for c in range(n):
                j = slots[k]
                self.active[j], self._child[j], self.prompt_len[j] = r, c, int(lens[k])
                self._adm_seq[j] = self._snap_seq    # snapshots taken from now on see this request in the slot
                self._rep_active += getattr(r.page, "repetition", None) is not None
                if self.prefix_cache and r.prompt_key is not None:
                    self._resident[j] = (r.prompt_key, int(lens[k]))
                k += 1
            self.sequences_admitted += n
            if cold:
                self.sequences_forked += n - 1

    def run(self, requests: Iterable[SlotRequest]) -> List[SlotResult]:
        """All requests to completion; results in submission order."""
        reqs = list(requests)
        order = {id(r): i for i, r in enumerate(reqs)}
        for r in reqs:
            self.submit(r)
        out: List[Optional[SlotResult]] = [None] * len(reqs)
        left = len(reqs)
        while left:
            for res in self.step():
                i = order.get(id(res.request))
                if i is not None and out[i] is None:
                    out[i] = res
                    left -= 1
        return out  # type: ignore[return-value]

    # ------------------------------------------------------------------ internals
    def _admit(self, begin_only: bool = False) -> List[SlotResult]:
        # cold admissions take free slots without a resident prompt first, then the one whose prompt finished longest ago
        free = sorted((j for j in range(self.n_slots) if j not in self.active),
                      key=lambda j: (j in self._resident, self._freed_at.get(j, 0) if j in self._resident else 0, j))
        if self.active and self.waiting and free and self.admit_min > 1:
            ready = min(len(free), sum(_n(r) for r in self.waiting))     # in slots
            if ready < min(self.admit_min, self.n_slots) and self._held < self.admit_max_wait:
                self._held += 1
                return []
        self._held = 0
        batch: List[SlotRequest] = []
        tok_budget = self.max_prompt_tokens
        patch_budget = self.max_patches
        failed: List[SlotResult] = []
        room = self.engine.seq_room() if hasattr(self.engine, "seq_room") else None
        slots: List[int] = []                        # of the batch's sequences, children consecutive
        while self.waiting and free:
            r = self.waiting[0]
            n_seq = _n(r)
            if n_seq > self.n_slots:
                self.waiting.popleft()
                failed.append(self._failure(r, f"n = {n_seq} exceeds the server's {self.n_slots} slots", status=400))
                continue
            n_tok = int(len(r.page.input_ids))
            if room is not None and n_tok + self._budget(r) > room:
                # its own prompt + max_tokens (+ the chunk overshoot) exceed a sequence's cache rows: this request fails
                # alone, as a client error; whatever is admitted with it is unaffected
                self.waiting.popleft()
                failed.append(self._failure(r, f"prompt ({n_tok} tokens) + max_tokens ({min(int(r.max_tokens), self.cap)}) + "
                                               f"{self.over} scheduler steps exceed the sequence capacity {room}", status=400))
                continue
            hit = self._resident_slot(r, free)
            if hit is not None:
                # resident prompt: no ViT, no prefill.  In place when that slot is free, else forked from it
                src, in_place = hit
                if n_seq > len(free):
                    break
                self.waiting.popleft()
                if in_place:
                    free.remove(src)
                mine = ([src] if in_place else []) + [free.pop(0) for _ in range(n_seq - (1 if in_place else 0))]
                failed += self._admit_reuse(r, src, mine)
                continue
            n_patch = sum(int(np.prod(g)) for g in getattr(r.page, "grids", None) or [])   # from the grids: pages may
            #                                                    carry uint8 images (GPU front end) instead of patches
            over_tok = tok_budget is not None and n_tok > tok_budget
            over_patch = patch_budget is not None and n_patch > patch_budget
            if over_tok or over_patch:
                if not batch and (self.max_prompt_tokens is not None and n_tok > self.max_prompt_tokens
                                  or self.max_patches is not None and n_patch > self.max_patches):
                    # can never fit: fail it instead of blocking the queue
                    self.waiting.popleft()
                    failed.append(self._failure(r, f"request does not fit the engine ({n_tok} prompt tokens, {n_patch} patches)",
                                                status=400))
                    continue
                break  # fits an emptier admission round
            if n_seq > len(free):
                break  # FIFO: the head waits for its slots and nothing overtakes it
            self.waiting.popleft()
            batch.append(r)
            for _ in range(n_seq):
                j = free.pop(0)
                self._resident.pop(j, None)          # the slot is given to another prompt
                slots.append(j)
            if tok_budget is not None:
                tok_budget -= n_tok
            if patch_budget is not None:
                patch_budget -= n_patch
        if batch and begin_only:
            try:
                self._inflight = (self.engine.admit_begin([r.page for r in batch], slots, **self._budget_kw(batch)), batch, slots)
            except Exception as e:
                return failed + [self._failure(r, f"{type(e).__name__}: {e}") for r in batch]
        elif batch:
            try:
                lens = self.engine.admit([r.page for r in batch], slots, **self._budget_kw(batch))
            except Exception as e:  # the admission as a whole failed: none of these requests entered a slot
                return failed + [self._failure(r, f"{type(e).__name__}: {e}") for r in batch]
            self._activate(batch, slots, lens)
            self.admissions += 1
            self.pages_admitted += len(batch)
        return failed

    def _resident_slot(self, r: SlotRequest, free) -> Optional[tuple]:
        """(slot that holds the request's prompt, whether the request can run there in place) or None."""
        if not self.prefix_cache or r.prompt_key is None:
            return None
        want = (r.prompt_key, int(len(r.page.input_ids)))
        held = [j for j, e in self._resident.items() if e == want]
        idle = [j for j in held if j in free]
        return (idle[0], True) if idle else (held[0], False) if held else None

    def _admit_reuse(self, r: SlotRequest, src: int, slots: List[int]) -> List[SlotResult]:
        for j in slots:
            if j != src:
                self._resident.pop(j, None)
        try:
            lens = self.engine.admit_reuse([r.page], [src], slots, **self._budget_kw([r]))
        except Exception as e:
            return [self._failure(r, f"{type(e).__name__}: {e}")]
        self._activate([r], slots, lens, cold=False)
        self.prefix_cache_hits += 1
        self.sequences_forked += sum(1 for j in slots if j != src)
        return []

    def _budget(self, r: SlotRequest) -> int:
        """Cache rows a request may write after its prompt: its token limit plus the steps a slot can run past it
        before the host looks at the flags again."""
        return min(int(r.max_tokens), self.cap) + self.over

    def _budget_kw(self, batch) -> dict:
        # engines that check capacity per request take the budgets (test fakes without seq_room do not)
        return {"budgets": [self._budget(r) for r in batch for _ in range(_n(r))]} if hasattr(self.engine, "seq_room") else {}

    def _failure(self, r: SlotRequest, msg: str, status: int = 500) -> SlotResult:
        return SlotResult(r.tag, np.zeros(0, np.int64), "length", 0, error=msg, request=r, status=status)

    def _harvest(self, flags=None, seq: Optional[int] = None) -> List[SlotResult]:
        """Requests that finished.  flags / seq: a snapshot's (finished, generated) and its sequence number — slots admitted after it
        was taken still show their previous occupant there and are skipped."""
        fin, gen = flags if flags is not None else self.engine.poll_slots()
        if self.speculative:
            self._spec_account(self.engine.spec_counts() if hasattr(self.engine, "spec_counts") else None, seq)
        rep_at = self.engine.slot_rep_at() if self._rep_active and hasattr(self.engine, "slot_rep_at") else None
        out: List[SlotResult] = []
        for j in sorted(self.active):
            if seq is not None and self._adm_seq.get(j, 0) > seq:
                continue
            r, c = self.active[j], self._child.get(j, 0)
            check = r.stop_checks[c] if r.stop_checks is not None else r.stop_check
            limit = min(int(r.max_tokens), self.cap)
            n = int(min(gen[j], limit))
            over = bool(fin[j] or gen[j] >= limit)
            if not over and (check is None or n < 1):
                continue
            toks = np.asarray(self.engine.slot_tokens(j, n), np.int64)
            reason, on_token, cause = "length", False, None
            if over:
                stops = self.eos | set(int(t) for t in getattr(r.page, "stop_token_ids", None) or ())
                hit = np.flatnonzero(np.isin(toks, list(stops))) if stops else np.zeros(0, np.int64)
                if hit.size:
                    toks, reason, on_token = toks[: int(hit[0]) + 1], "stop", True
                # the token the sequence repeats at is kept; an EOS or stop id at or before it wins, and so does max_tokens
                g = int(rep_at[j]) if rep_at is not None and getattr(r.page, "repetition", None) is not None else -1
                if 0 <= g < len(toks) - (1 if on_token else 0):
                    toks, reason, on_token, cause = toks[: g + 1], "length", False, "repetition"
            if check is not None:
                keep = check(toks)
                if keep is not None and keep <= len(toks):
                    on_token = on_token and keep == len(toks)
                    toks, reason, cause = toks[:int(keep)], "stop", None
                elif not over:
                    continue
            if not fin[j]:
                self.engine.retire(j)
            lps = None
            k = getattr(r.page, "logprobs", None)
            if k is not None and self.logprobs is not None:
                n_lp = len(toks) - (1 if on_token else 0)     # the step that finishes on EOS / a stop id records nothing
                lps = self.engine.slot_logprobs(j, n_lp, int(k))
            res = SlotResult(r.tag, toks, reason, self.prompt_len.pop(j), request=r, logprobs=lps, stop_reason=cause)
            if cause == "repetition":
                self.repetition_stops += 1
                self.repetition_tokens_cut += limit - len(toks)
            self._rep_active -= getattr(r.page, "repetition", None) is not None
            del self.active[j]                       # the child's slot is free for the next admission
            self._child.pop(j, None)
            self._tick += 1
            self._freed_at[j] = self._tick
            kids = self._open.get(id(r), [None])
            kids[c] = res
            if all(k is not None for k in kids):     # the request's last child: its one result
                self._open.pop(id(r), None)
                if len(kids) > 1:
                    res = SlotResult(r.tag, kids[0].tokens, kids[0].finish_reason, kids[0].prompt_tokens, request=r,
                                     logprobs=kids[0].logprobs, choices=list(kids), stop_reason=kids[0].stop_reason)
                out.append(res)
        return out
