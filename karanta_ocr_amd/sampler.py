"""The sampler of the engine: everything between the lm_head's logits and the step's tokens except the token choice itself —
its per-slot device state (sampling controls, logit adjustments, guides, log-probabilities), the host logic that turns an
admission's requests into that state, and the launches of a step's tail before and after the token is chosen.  Temperature
and seed are per ROW (a speculative step's draft rows have their own) and stay with the engine's decode state; so do the
switches of the current mode (Engine._caps, _step, _logprobs), which the graph key is made of.  Launches go to the engine's
current stream, read at the moment of each launch."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np
import torch

from ._lib import ADJ_CAP, REP_MAX_PERIOD, KarantaHipError, Repeat, ptr
from .request import PageRequest
from .sampling import StepFeatures, adjust_table, needs_processing, sampling_params, temperature


class DeviceGuide:
    """A compiled pattern resident in HBM: DFA transitions [S, 256] uint16 and one allowed-token bit row per state
    (kr_guide_build_masks).  Built by :meth:`Engine.compile_guide`."""

    def __init__(self, guide, trans: torch.Tensor, masks: torch.Tensor):
        self.guide, self.trans, self.masks = guide, trans, masks
        self.start = int(guide.start)


class Sampler:
    def __init__(self, eng):
        self.eng, self.cfg, self.device, self.L = eng, eng.cfg, eng.device, eng.L
        t, dev, B = self.cfg.text, self.device, eng.B
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)
        # guided decoding: per slot the device addresses of its pattern's tables (0 = unconstrained) + its DFA state.  An engine that
        # speculates on guided steps (SpecConfig(guided=True)) keeps them per ROW, the slots' entries in front: the step writes
        # those of its draft rows behind them, and admissions, reset_slots and plain steps stay per slot
        spec = eng.spec
        per_row = lambda on: max(B, eng.rows) if on else B      # (the option of an engine without a SpecConfig: off)
        G = per_row(spec is not None and spec.guided)
        self.d_gtrans = z(G, dtype=torch.int64)
        self.d_gmasks = z(G, dtype=torch.int64)
        self.d_gstate = z(G, dtype=torch.int32)
        # an engine that speculates on controlled steps (SpecConfig(controls=True)) runs the sampler's passes over ROWS: the scratch of
        # the threshold pass, the threshold keys, the live flags and the saved logits are per row there
        W = per_row(spec is not None and spec.controls)
        self.mask_words = 2 * ((t.vocab_size + 63) // 64)
        # sampling controls: per-slot params (sampling_params), output-token counts, prompt-token bit set, the threshold pass's
        # scratch scores, threshold keys and live flags (kr_sample_threshold / kr_gumbel_argmax_processed / kr_sample_count)
        self.d_sp = torch.tensor(np.tile(sampling_params(PageRequest(np.zeros(0, np.int64))), (B, 1)), device=dev)
        self.d_counts = z(B, t.vocab_size, dtype=torch.int32)
        self.bits_words = (t.vocab_size + 31) // 32
        self.d_pbits = z(B, self.bits_words, dtype=torch.int32)
        self.d_work = z(W, t.vocab_size, dtype=torch.float32)
        self.d_thr = z(W, dtype=torch.int32)
        self.d_live = z(W, dtype=torch.int32)
        # logit adjustments: per-slot tables (sampling.adjust_table; a row with n_entries == 0 is left alone) and the values
        # kr_logits_adjust saves for kr_logits_restore
        self.d_adj_ids = z(B, ADJ_CAP, dtype=torch.int32)
        self.d_adj_val = z(B, ADJ_CAP, dtype=torch.float32)
        self.d_adj_flag = z(B, ADJ_CAP, dtype=torch.int32)
        self.d_adj_meta = z(B, 4, dtype=torch.int32)
        self.d_adj_saved = z(W, ADJ_CAP, dtype=torch.float32)
        self.d_voc_off = self.d_voc_bytes = None   # set_vocab()
        # runaway repetition (kr_repeat_detect): per slot its cfg row {a, b, c, m} (b == 0: off), the run counters of the periods, how
        # many generated tokens the pass has looked at, and the index the sequence repeats at (-1: none).  _rep_slots: the slots whose
        # cfg row is not zero, so that an admission without the feature writes nothing here
        self.d_rep_cfg = z(B, 4, dtype=torch.int32)
        self.d_rep_run = z(B, REP_MAX_PERIOD, dtype=torch.int32)
        self.d_rep_seen = z(B, dtype=torch.int32)
        self.d_rep_at = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self._rep_slots: set = set()
        self._guides: Dict[str, DeviceGuide] = {}
        self._slot_guides: Dict[int, DeviceGuide] = {}   # keeps the tables of the running requests alive
        # log-probabilities: [hist][B][1 + 20] / [hist][B][20], allocated with the token history when asked for
        self.lp_part = max(64 if t.vocab_size > 4096 else 1, -(-t.vocab_size // 4096))   # slices of <= 4096 logits
        self.d_lp = self.d_lpi = None
        # an engine that speculates on recording steps (SpecConfig(logprobs=True)) records from any ROW of the step: partials per row
        P = per_row(spec is not None and spec.logprobs)
        self.d_lp_pv = z(P, self.lp_part, 20, dtype=torch.float32)
        self.d_lp_pi = z(P, self.lp_part, 20, dtype=torch.int32)
        self.d_lp_ms = z(P, self.lp_part, 2, dtype=torch.float32)

    def ensure_logprob_history(self, rows: int) -> bool:
        """The log-prob history sized for `rows` steps when log-probabilities are recorded; True where it was (re)allocated."""
        if self.eng._logprobs is None or (self.d_lp is not None and self.d_lp.shape[0] >= rows):
            return False
        self.d_lp = torch.zeros(rows, self.eng.B, 21, dtype=torch.float32, device=self.device)
        self.d_lpi = torch.zeros(rows, self.eng.B, 20, dtype=torch.int32, device=self.device)
        return True

    def reset_slots(self):
        """Slot mode begins: no slot carries a guide or an adjustment table."""
        self.d_gtrans.zero_()
        self.d_gmasks.zero_()
        self.d_adj_meta.zero_()
        self._slot_guides = {}
        if self._rep_slots:
            self.d_rep_cfg.zero_()
            self.d_rep_at.fill_(-1)
            self._rep_slots = set()

    # ------------------------------------------------------------------ guided decoding
    def set_vocab(self, token_bytes: Sequence[bytes]):
        """Byte string of every token id (b"" for special tokens) — what a pattern is matched against.  Needed once
        before any guided request (serving.ChatFrontend hands over its tokenizer's table)."""
        from .guided import pack_vocab
        V = self.cfg.text.vocab_size
        tb = list(token_bytes)[:V] + [b""] * max(0, V - len(token_bytes))
        off, flat = pack_vocab(tb)
        self.d_voc_off = torch.from_numpy(off).to(self.device)
        self.d_voc_bytes = torch.from_numpy(flat).to(self.device)
        self._guides.clear()

    def compile_guide(self, guide) -> DeviceGuide:
        """guided.Guide (or a regex string) -> device tables; cached by pattern."""
        from .guided import Guide, compile_regex
        if isinstance(guide, DeviceGuide):
            return guide
        if isinstance(guide, str):
            hit = self._guides.get(guide)
            if hit is not None:
                return hit
            guide = compile_regex(guide)
        if not isinstance(guide, Guide):
            raise KarantaHipError(f"not a guide: {type(guide).__name__}")
        if guide.pattern and guide.pattern in self._guides:
            return self._guides[guide.pattern]
        if self.d_voc_off is None:
            raise KarantaHipError("guided decoding needs the vocabulary's byte strings: call Engine.set_vocab() first")
        S, eng = guide.n_states, self.eng
        trans = torch.from_numpy(np.ascontiguousarray(guide.trans).view(np.int16)).to(self.device)
        accept = torch.from_numpy(np.ascontiguousarray(guide.accept).astype(np.uint8)).to(self.device)
        masks = torch.empty(S, self.mask_words, dtype=torch.int32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        with torch.cuda.stream(eng.stream):
            self.L.kr_guide_build_masks(ptr(trans), ptr(accept), S, ptr(self.d_voc_off), ptr(self.d_voc_bytes),
                                        self.cfg.text.vocab_size, ptr(eng.d_eos), eng.d_eos.numel(), ptr(masks),
                                        self.mask_words, eng.s)
        eng.stream.synchronize()
        dg = DeviceGuide(guide, trans, masks)
        if guide.pattern:
            if len(self._guides) >= 64:           # bounded cache: drop the oldest pattern
                self._guides.pop(next(iter(self._guides)))
            self._guides[guide.pattern] = dg
        return dg

    def _guide_rows(self, pages):
        """Per page: (trans address, masks address, start state, DeviceGuide | None)."""
        rows = []
        for p in pages:
            g = getattr(p, "guide", None)
            if g is None:
                rows.append((0, 0, 0, None))
                continue
            dg = self.compile_guide(g)
            rows.append((dg.trans.data_ptr(), dg.masks.data_ptr(), dg.start, dg))
        return rows

    # ------------------------------------------------------------------ admission: what the requests need, as host rows
    def check_features(self, need: StepFeatures):
        """Raises where an admission's pages need a pass the current mode does not allow."""
        caps = self.eng._caps
        if need.guided and not caps.guided:
            raise KarantaHipError("a page carries a guide but the engine is not in its guided configuration "
                                  "(generate() decides from its pages; begin_slots(guided=True) for slot mode)")
        if need.adjust and not caps.adjust:
            raise KarantaHipError("a page asks for logit_bias / min_tokens / stop_token_ids but the engine is in its greedy "
                                  "configuration (generate() decides from its pages; begin_slots(sampling=True) for slot mode)")
        if need.sampling and not caps.sampling:
            raise KarantaHipError("a page asks for temperature > 0 but the engine is in its greedy configuration "
                                  "(generate() decides from its pages; begin_slots(sampling=True) for slot mode)")
        if need.processing and not caps.processing:
            raise KarantaHipError("a page asks for top_k / top_p / min_p / penalties but the engine is in its greedy "
                                  "configuration (generate() decides from its pages; begin_slots(sampling=True) for slot mode)")

    def _control_rows(self, pages):
        """Per page (params row, prompt bit set or None, penalised) when the engine may run the processing launches, else None."""
        if not self.eng._caps.processing:
            return None
        V, rows = self.cfg.text.vocab_size, []
        for p in pages:
            sp, nd = sampling_params(p), needs_processing(p)
            bits = None
            if nd and sp[3] != 1.0:       # repetition penalty: the prompt's tokens (image placeholders included)
                ids = np.asarray(p.input_ids, np.int64).reshape(-1)
                ids = ids[(ids >= 0) & (ids < V)]
                bits = np.zeros(self.bits_words, np.uint32)
                np.bitwise_or.at(bits, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
            rows.append((sp, bits, nd))
        return rows

    def _adjust_rows(self, pages):
        """Per page its logit-adjustment table (sampling.adjust_table) or None, when the engine may run the adjustment launches,
        else None."""
        if not self.eng._caps.adjust:
            return None
        try:
            return [adjust_table(p, self.cfg.eos_token_ids, self.cfg.text.vocab_size) for p in pages]
        except ValueError as e:
            raise KarantaHipError(str(e)) from e

    def _sampler_rows(self, adm, rows):
        """What the sampler keeps per sequence, from the admission's sequences (`children` of its pages)."""
        adm.temps = np.asarray([temperature(p) for p in rows], np.float32)
        adm.seeds = np.asarray([int(getattr(p, "seed", 0) or 0) & 0xFFFFFFFF for p in rows], np.uint32).view(np.int32)
        adm.guides = self._guide_rows(rows)
        adm.procs = self._control_rows(rows)
        adm.adjs = self._adjust_rows(rows)
        adm.reps = [getattr(p, "repetition", None) for p in rows]

    def write(self, a):
        """The sampler's share of an admission's activation (Engine._activate): guide tables and start states, sampling controls,
        logit-adjustment tables and repetition state of the admission's slots."""
        h2d, B = self.eng._h2d, self.eng.B
        gt, gm, gs, dgs = zip(*a.guides)
        for dst, rows in ((self.d_gtrans, np.asarray(gt, np.int64)), (self.d_gmasks, np.asarray(gm, np.int64)),
                          (self.d_gstate, np.asarray(gs, np.int32))):
            for j, part in a.copies(rows, B):
                h2d(dst[j:], part)
        if a.whole_batch:     # the batch's guides replace every slot's; its tables start from empty rows
            self._slot_guides = {}
            if a.adjs is not None:
                self.d_adj_meta.zero_()
        for dg, j in zip(dgs, a.slots):
            self._slot_guides.pop(j, None)
            if dg is not None:
                self._slot_guides[j] = dg
        # sampling controls: params, prompt bits, output counts cleared
        for (sp, bits, nd), j in zip(a.procs or (), a.slots):
            h2d(self.d_sp[j], sp)
            if bits is not None:
                h2d(self.d_pbits[j], bits.view(np.int32))
            if nd:
                self.d_counts[j].zero_()
        # logit adjustments: the row's table; n_entries = 0 where the page has none, so a slot never keeps its predecessor's
        for tab, j in zip(a.adjs or (), a.slots):
            if tab is None:
                if not a.whole_batch:
                    self.d_adj_meta[j].zero_()
                continue
            for dst, rows in zip((self.d_adj_ids, self.d_adj_val, self.d_adj_flag, self.d_adj_meta), tab):
                h2d(dst[j], rows)

        # repetition: the slot's cfg row, and its place and verdict cleared (the run counters clear themselves at token 0); a slot
        # that neither carries the feature nor carried it is left alone
        if a.whole_batch and self._rep_slots and not any(r is not None for r in a.reps):
            self.d_rep_cfg.zero_()
            self.d_rep_at.fill_(-1)
            self._rep_slots = set()
        for r, j in zip(a.reps, a.slots):
            if r is None and j not in self._rep_slots:
                continue
            h2d(self.d_rep_cfg[j], np.asarray(r.row() if r is not None else (0, 0, 0, 0), np.int32))
            self.d_rep_seen[j:j + 1].zero_()
            self.d_rep_at[j:j + 1].fill_(-1)
            (self._rep_slots.add if r is not None else self._rep_slots.discard)(j)

    def repeat_pass(self, B: int, j: int, flags: int):
        """kr_repeat_detect over slots j .. j + B - 1, behind whatever appended the step's tokens (a plain step's tail, or a
        speculative step's verification): it finds its own place in every slot's history."""
        e = self.eng
        a = Repeat(B, ptr(e.d_hist[:, j:]), e.d_hist.stride(0), e.d_hist.shape[0], ptr(e.d_ctx[j:]), ptr(e.d_plen[j:]), ptr(e.d_fin[j:]),
                   ptr(self.d_rep_cfg[j:]), ptr(self.d_rep_run[j:]), ptr(self.d_rep_seen[j:]), ptr(self.d_rep_at[j:]), flags)
        self.L.kr_repeat_detect(C.byref(a), e.s)

    # ------------------------------------------------------------------ the step's tail around the token choice
    def _adj(self, j):
        return ptr(self.d_adj_ids[j:]), ptr(self.d_adj_val[j:]), ptr(self.d_adj_flag[j:]), ptr(self.d_adj_meta[j:])

    def pre_token(self, logits, n_part: int, B: int, j: int, flags: int, rows=None) -> int:
        """The passes between the lm_head and the token choice over rows j .. j + B - 1; returns the number of argmax partials
        per row the choice reads (`n_part` as the lm_head launch wrote them, at most 64 after a Gumbel pass).
        rows: the row map of a speculative step that carries adjustments or controls (j = 0, B = the engine's rows), as the
        row-mapped launches end on it — (row -> slot, row -> depth, the drafts, K, slots): a row takes its slot's table, params,
        prompt bits and counts, and the counts take in the drafts in front of it."""
        e, L, t, s = self.eng, self.L, self.cfg.text, self.eng.s
        step = e._step
        gm, gs = (ptr(self.d_gmasks[j:]), ptr(self.d_gstate[j:])) if step.guided else (None, None)
        if rows is not None:
            row_slot, _depth, _draft, _K, slots = rows
            V, ld = t.vocab_size, e.d_logits.stride(0)
            if step.adjust:     # (put back behind the token only where the step records log-probabilities)
                L.kr_logits_adjust_rows(ptr(logits), ld, V, *self._adj(0), ptr(e.d_ctx), ptr(e.d_plen), ptr(self.d_adj_saved), B,
                                        row_slot, slots, s)
            if step.processing:
                n_part = min(64, n_part)
                L.kr_sample_threshold_rows(ptr(logits), ld, V, ptr(e.d_temp), ptr(self.d_sp), ptr(self.d_counts), V, ptr(self.d_pbits),
                                           self.bits_words, gm, gs, self.mask_words, ptr(e.d_fin), flags, ptr(self.d_work), V,
                                           ptr(self.d_thr), ptr(self.d_live), B, *rows, s)
                L.kr_gumbel_argmax_processed_rows(ptr(logits), ld, V, ptr(e.d_temp), ptr(e.d_seed), ptr(e.d_ctx), ptr(e.d_plen),
                                                  ptr(e.d_amax_v), ptr(e.d_amax_i), n_part, B, gm, gs, self.mask_words,
                                                  int(self.cfg.eos_token_ids[0]), ptr(self.d_sp), ptr(self.d_counts), V,
                                                  ptr(self.d_pbits), self.bits_words, ptr(self.d_thr), *rows, s)
                return n_part
        elif step.adjust:
            # logit_bias / min_tokens somewhere in the batch: applied in place before the sampler (vLLM's order), undone after it
            L.kr_logits_adjust(ptr(logits), e.d_logits.stride(0), t.vocab_size, *self._adj(j), ptr(e.d_ctx[j:]), ptr(e.d_plen[j:]),
                               ptr(self.d_adj_saved[j:]), B, s)
        if step.processing:
            # sampling controls somewhere in the batch: per-row truncation threshold, then the Gumbel-max argmax over the
            # penalised scores above it (rows with neutral controls get exactly the partials of the branch below)
            n_part = min(64, n_part)
            V, ld = t.vocab_size, e.d_logits.stride(0)
            L.kr_sample_threshold(ptr(logits), ld, V, ptr(e.d_temp[j:]), ptr(self.d_sp[j:]), ptr(self.d_counts[j:]), V,
                                  ptr(self.d_pbits[j:]), self.bits_words, gm, gs, self.mask_words, ptr(e.d_fin[j:]), flags,
                                  ptr(self.d_work[j:]), V, ptr(self.d_thr[j:]), ptr(self.d_live[j:]), B, s)
            L.kr_gumbel_argmax_processed(ptr(logits), ld, V, ptr(e.d_temp[j:]), ptr(e.d_seed[j:]), ptr(e.d_ctx[j:]),
                                         ptr(e.d_plen[j:]), ptr(e.d_amax_v), ptr(e.d_amax_i), n_part, B, gm, gs,
                                         self.mask_words, int(self.cfg.eos_token_ids[0]), ptr(self.d_sp[j:]),
                                         ptr(self.d_counts[j:]), V, ptr(self.d_pbits[j:]), self.bits_words, ptr(self.d_thr[j:]), s)
        elif step.sampling:
            # temperature > 0 somewhere in the batch: the partial argmax is redone on logits / T + Gumbel noise
            # (rows with T = 0 get their plain argmax back); guided slots: only the tokens their DFA state allows take part
            # (unguided steps: null masks, as kr_gumbel_argmax passes them).  A speculative step's draft rows lie behind the
            # slots: the counter of a draft row's noise is its own token index, ctx_len and prompt_len are per row
            n_part = min(64, n_part)
            mw, fb = (self.mask_words, int(self.cfg.eos_token_ids[0])) if step.guided else (0, 0)
            L.kr_gumbel_argmax_guided(ptr(logits), e.d_logits.stride(0), t.vocab_size, ptr(e.d_temp[j:]), ptr(e.d_seed[j:]),
                                      ptr(e.d_ctx[j:]), ptr(e.d_plen[j:]), ptr(e.d_amax_v), ptr(e.d_amax_i), n_part, B,
                                      gm, gs, mw, fb, s)
        return n_part

    def post_token(self, logits, B: int, j: int, flags: int):
        """The passes behind the token choice of a plain step: stop tokens, output counts, guide advance, the logits put back,
        log-probabilities, repetition."""
        e, L, t, s = self.eng, self.L, self.cfg.text, self.eng.s
        step = e._step
        adj = self._adj(j) if step.adjust else None
        if step.adjust:
            L.kr_stop_tokens(ptr(e.d_tok[j:]), adj[0], adj[2], adj[3], ptr(e.d_fin[j:]), flags, B, s)
        if step.processing:
            L.kr_sample_count(ptr(e.d_tok[j:]), ptr(self.d_live[j:]), ptr(self.d_counts[j:]), t.vocab_size, t.vocab_size, B, s)
        if step.guided:
            L.kr_guide_advance(ptr(e.d_tok[j:]), ptr(e.d_fin[j:]), ptr(self.d_gtrans[j:]), ptr(self.d_gstate[j:]),
                               ptr(self.d_voc_off), ptr(self.d_voc_bytes), t.vocab_size, B, s)
        if step.adjust:     # log-probabilities and returned logits report what the lm_head wrote
            L.kr_logits_restore(ptr(logits), e.d_logits.stride(0), t.vocab_size, adj[0], adj[3], ptr(self.d_adj_saved[j:]), B, s)
        if e._logprobs is not None:
            L.kr_logprobs_topk(ptr(logits), e.d_logits.stride(0), t.vocab_size, int(e._logprobs), self.lp_part,
                               ptr(self.d_lp_pv), ptr(self.d_lp_pi), ptr(self.d_lp_ms), ptr(e.d_tok[j:]), ptr(e.d_ctx[j:]),
                               ptr(e.d_plen[j:]), ptr(e.d_fin[j:]), ptr(self.d_lp[:, j:]), ptr(self.d_lpi[:, j:]),
                               self.d_lp.shape[0], e.B, 20, B, s)
        if step.repetition:     # last: the token a sequence repeats at is kept, so its step still records its log-probabilities
            self.repeat_pass(B, j, flags)
