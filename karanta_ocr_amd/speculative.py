"""The speculative decode step of the engine (Engine(speculative=SpecConfig(...))): its device buffers (the row map, the prompt
ids the lookup searches, the drafts and where they were dealt, the counters, the scripted drafts of the test hook, the scratch
of the guided / controlled / recording steps), the argument records of its launches, and the step itself.  The per-row state a
plain step uses too (d_ctx, d_plen, d_fin, d_temp, d_seed, d_x) stays with the engine and the per-slot tables of the sampler
with the sampler; which steps may speculate is sampling.spec_refusal.  Launches go to the engine's current stream."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import KarantaHipError, Spec, SpecControls, SpecGuide, SpecLogprobs, ptr


class Speculator:
    def __init__(self, eng):
        self.eng, self.L = eng, eng.L
        sp, B, K, R = eng.spec, eng.B, eng.K, eng.rows
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=eng.device)
        # the slot of every row (a slot's own row: itself), the prompt ids per slot (written at every admission), the drafts
        # and the counters of proposed / accepted drafts, and the scripted continuations of the test hook (set_draft_script)
        self.d_row_slot = torch.arange(R, dtype=torch.int32, device=eng.device) % B
        self.d_prompt_ids = z(B, eng.s_max)
        self.d_ndraft = z(B)
        self.d_draft = z(B, K)
        if sp.share_rows:   # what every slot's lookup found, and the row each draft was dealt (-1: none)
            self.d_nwant = z(B)
            self.d_draft_row = torch.full((B, K), -1, dtype=torch.int32, device=eng.device)
        self.d_spec_count = z(2, B)
        self.d_script = z(B, dtype=torch.int64)
        self.d_script_len = z(B)
        self._scripts: Dict[int, torch.Tensor] = {}
        if sp.guided:     # the guide launches' scratch: the state behind every draft
            self.d_draft_state = z(B, K)
        if sp.guided or sp.controls or sp.logprobs:    # ctx_len at the start of the step (both trims and kr_spec_mark write it)
            self.d_ctx_before = z(B)
        if sp.controls:   # how many drafts lie in front of every row
            self.d_depth = z(R)

    # ------------------------------------------------------------------ argument records (read during the call: rebuilt per launch)
    def kr_spec(self) -> Spec:
        """kr_spec of this engine's speculative step (the history may have grown since the last one)."""
        e, t, sp = self.eng, self.eng.cfg.text, self.eng.spec
        return Spec(e.B, e.K, e.rows, int(sp.ngram_min), int(sp.ngram_max), e.s_max, ptr(self.d_prompt_ids),
                    self.d_prompt_ids.stride(0), ptr(e.d_hist), e.d_hist.stride(0), e.d_hist.shape[0], ptr(self.d_script),
                    ptr(self.d_script_len), ptr(self.d_row_slot), ptr(e.d_ctx), ptr(e.d_plen), ptr(e.d_fin), ptr(e.d_temp),
                    ptr(e.d_seed), ptr(self.d_ndraft), ptr(self.d_draft), ptr(e.w.view("llm.embed")), t.hidden_size,
                    e.cfg.pad_token_id, t.vocab_size, ptr(e.d_x), e.d_x.stride(0), ptr(self.d_spec_count[0]),
                    ptr(self.d_spec_count[1]))

    def kr_spec_guide(self) -> SpecGuide:
        """kr_spec_guide of a guided speculative step."""
        sm = self.eng.sampler
        return SpecGuide(ptr(sm.d_gtrans), ptr(sm.d_gmasks), ptr(sm.d_gstate), sm.mask_words, ptr(sm.d_voc_off), ptr(sm.d_voc_bytes),
                         ptr(self.d_draft_state), ptr(self.d_ctx_before))

    def kr_spec_controls(self) -> SpecControls:
        """kr_spec_controls of a controlled speculative step."""
        sm = self.eng.sampler
        return SpecControls(ptr(sm.d_adj_ids), ptr(sm.d_adj_flag), ptr(sm.d_adj_meta), ptr(sm.d_counts), self.eng.cfg.text.vocab_size,
                            ptr(self.d_depth), ptr(self.d_ctx_before))

    def kr_spec_logprobs(self) -> SpecLogprobs:
        """kr_spec_logprobs of a recording speculative step."""
        e, sm = self.eng, self.eng.sampler
        return SpecLogprobs(int(e._logprobs), sm.lp_part, ptr(sm.d_lp_pv), ptr(sm.d_lp_pi), ptr(sm.d_lp_ms), ptr(sm.d_lp), ptr(sm.d_lpi),
                            sm.d_lp.shape[0], e.B, 20, ptr(self.d_ctx_before))

    # ------------------------------------------------------------------ the step
    def step_launches(self):
        """One speculative step: drafts (kr_spec_propose) -> the layers over all rows -> lm_head -> the Gumbel pass when a request
        samples -> verification and bookkeeping (kr_spec_accept, in kr_sample_greedy's place).  It leaves d_ctx, d_tok, d_x[slot],
        the history and d_fin in the form a plain step leaves them, so the two kinds alternate freely.
        share_rows: the drafts are looked up (kr_spec_lookup), the rows behind the slots dealt to them (kr_spec_deal) and the
        verification reads each draft at the row it was dealt (kr_spec_accept_rows); everything between is the same launches —
        they take the row-to-slot map as it comes.
        A step that carries guided requests (SpecConfig(guided=True)) has three launches more: the drafts a slot's guide forbids are
        dropped before any row is spent on them (kr_spec_guide_trim: behind kr_spec_propose, or between kr_spec_lookup and
        kr_spec_deal), every draft row gets the guide and the DFA state behind its drafts (kr_spec_guide_rows) for the masked Gumbel
        pass, and the slots' states follow the tokens the verification emitted (kr_spec_guide_advance).  An unguided step issues
        none of them.  A step that carries sampling controls or logit adjustments (SpecConfig(controls=True)) has the same shape:
        kr_spec_controls_trim behind the guide's trim (a draft that is a stop entry of its slot ends the slot's drafts),
        kr_spec_controls_rows behind the guide's rows (every row's depth, for the row-mapped sampler passes Sampler.pre_token picks),
        kr_stop_tokens behind the verification where the step carries adjustments, and kr_spec_controls_count where it carries
        controls (the slots' output counts follow the emitted tokens).  A step without either issues none of them.
        A step that records log-probabilities (SpecConfig(logprobs=True)) starts on kr_spec_mark where no trim ran (the trims write
        ctx_before themselves) and, behind the verification and kr_stop_tokens, puts the adjusted logits back
        (kr_logits_restore_rows, where the step carries adjustments) and records every emitted token from the row that chose it
        (kr_logprobs_topk_rows) — Sampler.post_token's order.  A step that records nothing issues none of them.
        A step that carries repetition detection ends on kr_repeat_detect, as a plain step does."""
        e, L, sm = self.eng, self.L, self.eng.sampler
        s, R, step, V, shared = e.s, e.rows, e._step, e.cfg.text.vocab_size, e.spec.share_rows
        why = e._spec_refusal()
        if why is not None:
            raise KarantaHipError("speculative decode step refused: " + why)
        a = self.kr_spec()
        g = self.kr_spec_guide() if step.guided else None
        c = self.kr_spec_controls() if (step.processing or step.adjust) else None
        record = e._logprobs is not None
        # the two layouts differ in the lookup, in the count array the trims cut and in the map from drafts to rows
        count, draft_row = (ptr(self.d_nwant), ptr(self.d_draft_row)) if shared else (ptr(self.d_ndraft), None)
        if record and g is None and c is None:
            L.kr_spec_mark(C.byref(a), ptr(self.d_ctx_before), s)
        if shared:
            L.kr_spec_lookup(C.byref(a), count, s)
        else:
            L.kr_spec_propose(C.byref(a), s)
        if g is not None:
            L.kr_spec_guide_trim(C.byref(a), C.byref(g), count, s)
        if c is not None:
            L.kr_spec_controls_trim(C.byref(a), C.byref(c), count, s)
        if shared:
            L.kr_spec_deal(C.byref(a), count, draft_row, s)
        if g is not None:
            L.kr_spec_guide_rows(C.byref(a), C.byref(g), draft_row, s)
        if c is not None:
            L.kr_spec_controls_rows(C.byref(a), C.byref(c), draft_row, s)
        x = e._layer_launches(R, self.d_row_slot)
        logits, n_part = e._lm_head(R, x)
        flags = e._flags()
        # (an uncontrolled step: the Gumbel pass alone; a controlled one: the row-mapped adjustment and control passes)
        rows = (ptr(self.d_row_slot), ptr(self.d_depth), ptr(self.d_draft), e.K, e.B) if c is not None else None
        n_part = sm.pre_token(logits, n_part, R, 0, flags, rows)
        verdict = (ptr(e.d_amax_v), ptr(e.d_amax_i), n_part, ptr(e.d_tok), ptr(e.d_eos), e.d_eos.numel(), flags, s)
        if shared:
            L.kr_spec_accept_rows(C.byref(a), draft_row, *verdict)
        else:
            L.kr_spec_accept(C.byref(a), *verdict)
        if step.adjust:       # a stop entry can only be the step's last token (kr_spec_controls_trim): the plain step's launch
            L.kr_stop_tokens(ptr(e.d_tok), ptr(sm.d_adj_ids), ptr(sm.d_adj_flag), ptr(sm.d_adj_meta), ptr(e.d_fin), flags, e.B, s)
        if record:            # the logits of the step's rows put back where it adjusted them, then the record of every emitted token
            ld = e.d_logits.stride(0)
            if step.adjust:
                L.kr_logits_restore_rows(ptr(logits), ld, V, ptr(sm.d_adj_ids), ptr(sm.d_adj_meta), ptr(sm.d_adj_saved), R,
                                         ptr(self.d_row_slot), e.B, s)
            p = self.kr_spec_logprobs()
            L.kr_logprobs_topk_rows(C.byref(a), C.byref(p), draft_row, ptr(logits), ld, s)
        if step.processing:
            L.kr_spec_controls_count(C.byref(a), C.byref(c), s)
        if g is not None:
            L.kr_spec_guide_advance(C.byref(a), C.byref(g), s)
        if step.repetition:   # over the 1 .. K + 1 tokens every slot gained: the cut plain steps make
            sm.repeat_pass(e.B, 0, flags)

    # ------------------------------------------------------------------ admissions, slot mode, the host's view
    def write_prompts(self, a):
        """The speculative share of an admission's activation (Engine._activate): the lookup searches prompt + history."""
        for p, j in zip(a.rows, a.slots):
            self.eng._h2d(self.d_prompt_ids[j], np.asarray(p.input_ids, np.int64).reshape(-1).astype(np.int32))

    def reset_counters(self):
        """Slot mode begins: nothing proposed, nothing accepted."""
        self.d_spec_count.zero_()

    def set_draft_script(self, slot: int, tokens: Optional[Sequence[int]]):
        """Test hook: the drafts of `slot` come from a scripted continuation — draft j of a step is tokens[generated + j - 1] —
        instead of the n-gram lookup, until None is set (an admission does not clear it)."""
        e = self.eng
        if not 0 <= int(slot) < e.B:
            raise KarantaHipError(f"set_draft_script: slot {slot} outside 0..{e.B - 1}")
        j = int(slot)
        with torch.cuda.stream(e.stream):
            if tokens is None:
                self.d_script[j:j + 1].zero_()
                self.d_script_len[j:j + 1].zero_()
                e.stream.synchronize()       # a queued step may still read the tensor this drops
                self._scripts.pop(j, None)
                return
            arr = np.ascontiguousarray(np.asarray(tokens, np.int64).reshape(-1).astype(np.int32))
            buf = torch.zeros(max(1, arr.size), dtype=torch.int32, device=e.device)
            e._h2d(buf, arr)
            e._h2d(self.d_script[j:j + 1], np.asarray([buf.data_ptr()], np.int64))
            e._h2d(self.d_script_len[j:j + 1], np.asarray([arr.size], np.int32))
            e.stream.synchronize()
            self._scripts[j] = buf

    def counts(self) -> Tuple[np.ndarray, np.ndarray]:
        """(proposed[B], accepted[B]) as of the state the host last read: the snapshot given to read_snapshot(), else (after
        poll_slots()) the device's counters now."""
        return self.eng._snap_counts if self.eng._snap_counts is not None else self.counters()

    def counters(self) -> Tuple[np.ndarray, np.ndarray]:
        """(proposed[B], accepted[B]): draft tokens proposed / accepted per slot since begin_slots (synchronises)."""
        self.eng.stream.synchronize()
        c = self.d_spec_count.cpu().numpy().astype(np.int64)
        return c[0], c[1]
