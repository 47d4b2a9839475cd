// The two ends of a speculative decode step (include/karanta_hip.h, kr_spec): prompt-lookup drafts in, verified tokens out.
//   spec_propose_kernel  per slot: the longest n-gram (ngram_max .. ngram_min) that ends the sequence is looked up earlier in
//                        prompt + history; the tokens after the match are the drafts.  Fills the draft rows of the step: their
//                        slot, position, sampler state and input embedding.
//   spec_accept_kernel   per slot: final argmax of its k + 1 rows, then kr_sample_greedy's bookkeeping token by token while the
//                        drafts agree with what the rows before them produced.
// Between them the rows run through the packed decode family with kr_linear_decode32_rows / kr_attn_decode_rows.
// Shared rows (kr_spec_lookup -> kr_spec_deal -> ... -> kr_spec_accept_rows): the rows behind the slots' own are a budget dealt per
// step to the slots whose lookup found something, instead of k rows owned by every slot.
//   spec_lookup_kernel   per slot: the same search; writes how many drafts the slot wants and their tokens, no row state.
//   spec_deal_kernel     ONE workgroup: rows slots .. rows - 1 breadth first (depth 1 of every slot in slot order, then depth 2, ...)
//                        and the row state of each; a row nobody got is parked like a padding row.
//   spec_accept_kernel   with a map: draft j of a slot is verified on row draft_row[slot * k + j - 1].
// Guided slots (kr_spec_guide_trim -> kr_spec_guide_rows -> ... -> kr_spec_guide_advance, around either layout): the drafts a slot's
// guide forbids are dropped, every draft row gets the DFA state behind its drafts, the slot's state follows the emitted tokens.
// Controlled slots (kr_spec_controls_trim -> kr_spec_controls_rows -> ... -> kr_stop_tokens -> kr_spec_controls_count, around either
// layout and beside the guide's three): a draft that is a stop entry of its slot ends the slot's drafts, every row learns how many
// drafts lie in front of it (the sampler's row-mapped passes add them to the slot's output counts), the counts follow the emitted tokens.
// Recorded slots (kr_spec_mark -> ... -> kr_logprobs_topk_rows, around either layout and beside the guide's and the controls' launches):
// every token the step emitted gets the log-probability record a plain step would have written for it, from the logits row that chose it.
#include "kr_decode_common.h"
#include "kr_logprobs.h"
#include "kr_spec_deal.h"

namespace {

constexpr int SPEC_MAX_ROWS = 32, SPEC_MAX_NGRAM = 8;

// The drafts of `slot` (256 threads, all of them call it): thread 0 returns their number and leaves the tokens in s_draft; the other
// threads return 0.  s_key: 4 words of scratch.
__device__ __forceinline__ int spec_drafts(const kr_spec& a, int slot, unsigned* s_key, int* s_draft) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.k;
    const int ctx = a.ctx_len[slot], plen = a.prompt_len[slot], fin = a.finished[slot];
    const int L = ctx + 1;
    const int32_t* prm = a.prompt_ids + (int64_t)slot * a.prompt_stride;
    auto tok = [&](int i) { return i < plen ? prm[i] : a.history[(int64_t)(i - plen) * a.hist_stride + slot]; };
    const uint64_t script = a.script != nullptr ? a.script[slot] : 0ull;
    unsigned best = 0u;
    if (!fin && script == 0ull && L > a.ngram_min) {
        // candidate p = where a continuation would start (1 <= p <= L - 1); m(p) = how many tokens before p equal the sequence's
        // last ones (up to ngram_max): p matches n-gram length n at i = p - n iff m(p) >= n.  The rule — the largest n that has
        // a match, then the largest (drafts available, i) — is the maximum of (m, min(K, L - p), p): one reduction.
        int tl[SPEC_MAX_NGRAM];
#pragma unroll
        for (int q = 0; q < SPEC_MAX_NGRAM; ++q) tl[q] = q < a.ngram_max && q < L ? tok(L - 1 - q) : -1;
        for (int p = 1 + tid; p <= L - 1; p += 256) {
            int m = 0;
#pragma unroll
            for (int q = 0; q < SPEC_MAX_NGRAM; ++q)
                if (m == q && q < a.ngram_max && q < p && tok(p - 1 - q) == tl[q]) m = q + 1;
            if (m >= a.ngram_min) {
                const unsigned key = ((unsigned)m << 26) | ((unsigned)min(K, L - p) << 20) | (unsigned)p;
                best = key > best ? key : best;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned ob = (unsigned)__shfl_xor((int)best, o, 64);
        best = ob > best ? ob : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    int nd = 0;
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = s_key[w] > best ? s_key[w] : best;
        if (!fin) {
            if (script != 0ull) {
                const int32_t* sc = reinterpret_cast<const int32_t*>(script);
                const int gen = ctx + 1 - plen;
                nd = max(0, min(K, a.script_len[slot] - gen));
                for (int j = 0; j < nd; ++j) s_draft[j] = sc[gen + j];
            } else if (best != 0u) {
                const int p = (int)(best & 0xFFFFFu);
                nd = (int)((best >> 20) & 63u);
                for (int j = 0; j < nd; ++j) s_draft[j] = tok(p + j);
            }
            nd = min(nd, max(0, a.s_max - 1 - ctx));           // every active row keeps a cache position of its own
            for (int j = 0; j < nd; ++j)
                if (s_draft[j] < 0 || s_draft[j] >= a.vocab) nd = j;   // (a scripted token outside the vocabulary ends the run)
        }
    }
    return nd;
}

__global__ void __launch_bounds__(256) spec_propose_kernel(const kr_spec a) {
    __shared__ unsigned s_key[4];
    __shared__ int s_nd, s_draft[SPEC_MAX_ROWS];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int B = a.slots, K = a.k;
    const int ctx = a.ctx_len[slot], plen = a.prompt_len[slot], fin = a.finished[slot];
    const int nd0 = spec_drafts(a, slot, s_key, s_draft);
    if (tid == 0) {
        s_nd = nd0;
        a.n_draft[slot] = nd0;
        for (int j = 0; j < K; ++j) a.draft_tok[slot * K + j] = j < nd0 ? s_draft[j] : a.pad_id;
    }
    __syncthreads();
    const int nd = s_nd;
    // the draft rows of this slot; workgroup 0 also parks the rows past slots * (k + 1) (inactive rows of slot 0 at s_max - 1)
    const int n_pad = slot == 0 ? a.rows - B * (K + 1) : 0;
    const float temp = a.temperature[slot];
    const unsigned seed = a.seed[slot];
    if (tid < K + n_pad) {
        const bool pad = tid >= K;
        const int j = tid + 1, r = pad ? B * (K + 1) + (tid - K) : j * B + slot;
        a.row_slot[r] = pad ? 0 : slot;
        a.ctx_len[r] = pad ? a.s_max - 1 : min(ctx + j, a.s_max - 1);
        a.prompt_len[r] = pad ? a.s_max - 1 : plen;
        a.temperature[r] = pad ? 0.f : temp;
        a.seed[r] = pad ? 0u : seed;
        a.finished[r] = (pad || fin || j > nd) ? 1 : 0;
    }
    const int d8 = a.d >> 3;
    for (int e = tid; e < (K + n_pad) * d8; e += 256) {
        const int q = e / d8, c = e - q * d8;
        const bool pad = q >= K;
        const int r = pad ? B * (K + 1) + (q - K) : (q + 1) * B + slot;
        const int t = (!pad && !fin && q < nd) ? s_draft[q] : a.pad_id;
        st8(a.x + (int64_t)r * a.ldx + c * 8, ld8(a.embed_table + (int64_t)t * a.d + c * 8));
    }
}

// The search alone: how many drafts the slot wants (n_want, kr_spec_propose's n_draft) and their tokens.
__global__ void __launch_bounds__(256) spec_lookup_kernel(const kr_spec a, int32_t* __restrict__ n_want) {
    __shared__ unsigned s_key[4];
    __shared__ int s_draft[SPEC_MAX_ROWS];
    const int slot = blockIdx.x, K = a.k;
    const int nd = spec_drafts(a, slot, s_key, s_draft);
    if (threadIdx.x == 0) {
        n_want[slot] = nd;
        for (int j = 0; j < K; ++j) a.draft_tok[slot * K + j] = j < nd ? s_draft[j] : a.pad_id;
    }
}

// One workgroup: rows B .. rows - 1 go breadth first to the drafts (slot, j) with j <= n_want[slot] — depth 1 of every slot in slot
// order, then depth 2, ... — so the row of (slot, j) is B + sum_{j' < j} #{s : want[s] >= j'} + #{s' < slot : want[s'] >= j} where that
// is below `rows`.  Every global write of row state is indexed by a row r in B .. rows - 1 taken from the loop, never by a computed
// row: s_owner[r] says whose it is, or that nobody got it (parked: slot 0 at s_max - 1, finished, the pad token).
__global__ void __launch_bounds__(256) spec_deal_kernel(const kr_spec a, const int32_t* __restrict__ n_want,
                                                        int32_t* __restrict__ draft_row) {
    __shared__ int s_want[SPEC_MAX_ROWS], s_cnt[SPEC_MAX_ROWS + 1], s_owner[SPEC_MAX_ROWS];
    const int tid = threadIdx.x, B = a.slots, K = a.k, R = a.rows;
    if (tid < SPEC_MAX_ROWS) {
        s_owner[tid] = -1;
        s_want[tid] = tid < B ? spec_deal_want(n_want[tid], a.finished[tid], K, a.ctx_len[tid], a.s_max) : 0;
    }
    __syncthreads();
    if (tid >= 1 && tid <= K) s_cnt[tid] = spec_deal_count(s_want, B, tid);      // (s_cnt[0] is not used)
    __syncthreads();
    for (int e = tid; e < B * K; e += 256) {
        const int slot = e / K, j = e - slot * K + 1;
        const int r = spec_deal_row(s_want, s_cnt, B, R, slot, j);
        draft_row[e] = r;
        if (r >= 0) s_owner[r] = e;       // (rows are distinct: one writer per entry)
    }
    __syncthreads();
    if (tid < B) {       // the dealt depths of a slot are a prefix: rows grow with the depth
        int nd = 0;
        for (int j = 1; j <= s_want[tid]; ++j)
            if (spec_deal_row(s_want, s_cnt, B, R, tid, j) >= 0) nd = j;
        a.n_draft[tid] = nd;
    }
    const int n_rows = R - B;
    if (tid < n_rows) {
        const int r = B + tid, e = s_owner[r];
        const bool pad = e < 0;
        const int slot = pad ? 0 : e / K, j = pad ? 0 : e - slot * K + 1;
        a.row_slot[r] = slot;
        a.ctx_len[r] = pad ? a.s_max - 1 : min(a.ctx_len[slot] + j, a.s_max - 1);
        a.prompt_len[r] = pad ? a.s_max - 1 : a.prompt_len[slot];
        a.temperature[r] = pad ? 0.f : a.temperature[slot];
        a.seed[r] = pad ? 0u : a.seed[slot];
        a.finished[r] = pad ? 1 : 0;
    }
    const int d8 = a.d >> 3;
    for (int i = tid; i < n_rows * d8; i += 256) {
        const int q = i / d8, c = i - q * d8;
        const int r = B + q, e = s_owner[r];
        int t = e < 0 ? a.pad_id : a.draft_tok[e];
        if (t < 0 || t >= a.vocab) t = a.pad_id;      // (kr_spec_lookup leaves none such below n_want)
        st8(a.x + (int64_t)r * a.ldx + c * 8, ld8(a.embed_table + (int64_t)t * a.d + c * 8));
    }
}

// draft_row == nullptr: the static layout (draft j of a slot on row j * slots + slot); else the map kr_spec_deal wrote.
__global__ void __launch_bounds__(256) spec_accept_kernel(const kr_spec a, const float* __restrict__ amax_val,
                                                          const int32_t* __restrict__ amax_idx, int n_part,
                                                          int32_t* __restrict__ tokens_out, const int32_t* __restrict__ eos, int n_eos,
                                                          int flags, const int32_t* __restrict__ draft_row) {
    __shared__ int s_t[SPEC_MAX_ROWS], s_last;
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.slots, K = a.k;
    // t_j: one wave per row, kr_sample_greedy's order (`better`: the larger value, ties to the lowest index)
    for (int j = wave; j <= K; j += 4) {
        const int row = j == 0 ? slot : draft_row == nullptr ? j * B + slot : draft_row[slot * K + j - 1];
        if (row < 0 || row >= a.rows) {       // draft j was not dealt a row: t_j is never looked at (j > n_draft)
            if (lane == 0) s_t[j] = -1;
            continue;
        }
        const int64_t r = (int64_t)row * n_part;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i0 = lane; i0 < n_part; i0 += 64 * 8) {
            float v[8];
            int ix[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 64, n_part - 1);
                v[u] = amax_val[r + i];
                ix[u] = amax_idx[r + i];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u * 64 < n_part) better(bv, bi, v[u], ix[u]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            better(bv, bi, ov, oi);
        }
        if (lane == 0) s_t[j] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        const bool ignore_eos = (flags & 1) != 0, freeze = (flags & 2) != 0;
        const int was_finished = a.finished[slot], ctx = a.ctx_len[slot], plen = a.prompt_len[slot];
        int last = a.pad_id;
        if (was_finished && !ignore_eos) {
            // kr_sample_greedy's finished row: the pad token; frozen, the slot idles at its position with its history as it is
            if (!freeze) {
                a.history[(int64_t)(ctx + 1 - plen) * a.hist_stride + slot] = last;
                a.ctx_len[slot] = ctx + 1;
            }
        } else {
            int nd = a.n_draft[slot];
            for (int j = 1; j <= min(nd, K); ++j)
                if (s_t[j] < 0) nd = j - 1;      // (a map that disagrees with n_draft: no token without a row)
            int e = 0, acc = 0;   // tokens emitted; drafts that turned out to be the token emitted at their position
            for (int j = 0; j <= K; ++j) {
                if (j > 0 && !(j <= nd && a.draft_tok[slot * K + j - 1] == s_t[j - 1])) break;
                const int h = ctx + 1 + j - plen;
                if (j > 0 && h >= a.hist_rows) break;     // (the caller's budgets keep h inside the history: kr_sample_greedy's contract)
                last = s_t[j];
                if (h >= 0 && h < a.hist_rows) a.history[(int64_t)h * a.hist_stride + slot] = last;
                ++e;
                acc = j;              // t_j is out: drafts 1..j were right
                if (!ignore_eos) {
                    int hit = 0;
                    for (int i = 0; i < n_eos; ++i) hit |= (last == eos[i]);
                    if (hit) {
                        a.finished[slot] = 1;
                        if (j < nd && a.draft_tok[slot * K + j] == last) acc = j + 1;   // the EOS itself was drafted: no token follows it
                        break;
                    }
                }
            }
            a.ctx_len[slot] = ctx + e;
            a.proposed[slot] += nd;
            a.accepted[slot] += acc;
        }
        tokens_out[slot] = last;
        s_last = last;
    }
    __syncthreads();
    const int last = s_last;
    for (int c = tid; c < (a.d >> 3); c += 256) st8(a.x + (int64_t)slot * a.ldx + c * 8, ld8(a.embed_table + (int64_t)last * a.d + c * 8));
}

int spec_check(const kr_spec* a, const char* who, bool shared_rows = false) {
    KR_CHECK_ARG(a, "%s: null args", who);
    if (shared_rows)
        KR_CHECK_ARG(a->slots >= 1 && a->k >= 1 && a->k < SPEC_MAX_ROWS && a->slots < a->rows && a->rows <= SPEC_MAX_ROWS,
                     "%s: slots=%d k=%d rows=%d (1 <= slots < rows <= 32, 1 <= k < 32)", who, a->slots, a->k, a->rows);
    else
        KR_CHECK_ARG(a->slots >= 1 && a->k >= 1 && a->k < SPEC_MAX_ROWS && a->slots * (a->k + 1) <= a->rows && a->rows <= SPEC_MAX_ROWS,
                     "%s: slots=%d k=%d rows=%d (slots * (k + 1) <= rows <= 32)", who, a->slots, a->k, a->rows);
    KR_CHECK_ARG(a->ngram_min >= 1 && a->ngram_min <= a->ngram_max && a->ngram_max <= SPEC_MAX_NGRAM, "%s: ngram_min=%d ngram_max=%d (1 <= min <= max <= 8)",
                 who, a->ngram_min, a->ngram_max);
    KR_CHECK_ARG(a->s_max >= 2 && a->s_max <= (1 << 20), "%s: s_max=%d", who, a->s_max);
    KR_CHECK_ARG(a->prompt_ids && a->history && a->row_slot && a->ctx_len && a->prompt_len && a->finished && a->temperature && a->seed &&
                 a->n_draft && a->draft_tok && a->embed_table && a->x && a->proposed && a->accepted, "%s: null pointer", who);
    KR_CHECK_ARG(a->hist_stride >= a->slots && a->hist_rows >= 1 && a->prompt_stride >= 1 && a->d > 0 && (a->d & 7) == 0 && a->ldx >= a->d &&
                 (a->ldx & 7) == 0 && a->vocab > 0 && a->pad_id >= 0 && a->pad_id < a->vocab, "%s: bad sizes", who);
    KR_CHECK_ARG(a->script == nullptr || a->script_len != nullptr, "%s: script without script_len", who);
    return KR_OK;
}

// ---------------------------------------------------------------- guided slots in a speculative step (kr_spec_guide)
// A guide's DFA state per draft: the state at depth j is the slot's state walked over drafts 1..j.  Integer work only.
//   spec_guide_trim_kernel     per slot, before any row is spent: the drafts are kept while the guide allows them (the bit
//                              kr_gumbel_argmax_guided tests); the state behind every kept draft goes to draft_state.
//   spec_guide_rows_kernel     ONE workgroup: the guide entries of every row behind the slots' own.
//   spec_guide_advance_kernel  per slot, after the verification: the slot's state walked over the tokens the step emitted.
constexpr int GUIDE_STAGE = 32;     // bytes of a token held in LDS; a longer token's tail is read from the table

// The tokens of one slot's walk, staged by the lanes: their byte ranges and first bytes (len -1: a token outside the vocabulary).
struct GuideStage {
    int tok[SPEC_MAX_ROWS], off[SPEC_MAX_ROWS], len[SPEC_MAX_ROWS];
    uint8_t bytes[SPEC_MAX_ROWS][GUIDE_STAGE];
};

__device__ __forceinline__ void guide_stage(GuideStage& s, int q, int t, int vocab, const int32_t* __restrict__ vocab_off,
                                            const uint8_t* __restrict__ vocab_bytes) {
    s.tok[q] = t;
    if (t < 0 || t >= vocab) {
        s.off[q] = 0;
        s.len[q] = -1;
        return;
    }
    const int o0 = vocab_off[t], n = max(0, vocab_off[t + 1] - o0);
    s.off[q] = o0;
    s.len[q] = n;
    for (int i = 0; i < min(n, GUIDE_STAGE); ++i) s.bytes[q][i] = vocab_bytes[o0 + i];
}

// walk(st, bytes(token q)): kr_guide_advance's loop
__device__ __forceinline__ unsigned guide_walk(const GuideStage& s, int q, unsigned st, const uint16_t* __restrict__ trans,
                                               const uint8_t* __restrict__ vocab_bytes) {
    for (int i = 0; i < s.len[q] && st != 0; ++i) {
        const unsigned byte = i < GUIDE_STAGE ? s.bytes[q][i] : vocab_bytes[s.off[q] + i];
        st = trans[st * 256u + byte];
    }
    return st;
}

__global__ void __launch_bounds__(64) spec_guide_trim_kernel(const kr_spec a, const kr_spec_guide g, int32_t* __restrict__ n_count) {
    __shared__ GuideStage s;
    const int slot = blockIdx.x, tid = threadIdx.x, K = a.k;
    if (tid == 0) g.ctx_before[slot] = a.ctx_len[slot];
    const uint64_t tp = g.guide_trans[slot];
    if (tp == 0 || a.finished[slot]) return;          // (uniform per workgroup) the slot keeps its count and its drafts
    const int n = max(0, min(K, n_count[slot]));
    if (tid < n) guide_stage(s, tid, a.draft_tok[slot * K + tid], a.vocab, g.vocab_off, g.vocab_bytes);
    __syncthreads();
    if (tid != 0) return;
    const uint16_t* trans = reinterpret_cast<const uint16_t*>(tp);
    const uint32_t* masks = reinterpret_cast<const uint32_t*>(g.guide_masks[slot]);
    unsigned st = (unsigned)g.guide_state[slot];
    int keep = n;
    for (int j = 0; j < n; ++j) {
        const int t = s.tok[j];
        const bool ok = s.len[j] >= 0 && masks != nullptr && ((masks[(int64_t)st * g.mask_words + (t >> 5)] >> (t & 31)) & 1u) != 0;
        if (!ok) {          // the guide forbids draft j + 1 in the state behind draft j
            keep = j;
            break;
        }
        st = guide_walk(s, j, st, trans, g.vocab_bytes);
        g.draft_state[slot * K + j] = (int)st;
        if (s.len[j] == 0) {      // allowed without bytes: an EOS in an accepting state, and nothing follows an EOS
            keep = j + 1;
            break;
        }
    }
    n_count[slot] = keep;
    for (int j = keep; j < K; ++j) a.draft_tok[slot * K + j] = a.pad_id;
}

// draft_row == nullptr: the static layout (draft j of a slot on row j * slots + slot); else the map kr_spec_deal wrote.  As in
// spec_deal_kernel every global write is indexed by a row taken from the loop: s_owner[r] says whose row r is, or nobody's.
__global__ void __launch_bounds__(64) spec_guide_rows_kernel(const kr_spec a, const kr_spec_guide g, const int32_t* __restrict__ draft_row) {
    __shared__ int s_owner[SPEC_MAX_ROWS];
    const int tid = threadIdx.x, B = a.slots, K = a.k, R = a.rows;
    if (tid < SPEC_MAX_ROWS) {
        int e = -1;
        if (draft_row == nullptr && tid >= B && tid < B * (K + 1)) e = (tid % B) * K + tid / B - 1;
        s_owner[tid] = e;
    }
    __syncthreads();
    if (draft_row != nullptr)
        for (int e = tid; e < B * K; e += 64) {
            const int r = draft_row[e];
            if (r >= B && r < R) s_owner[r] = e;       // (rows are distinct: one writer per entry)
        }
    __syncthreads();
    const int r = B + tid;
    if (r >= R) return;
    const int e = s_owner[r];
    const int slot = e < 0 ? 0 : e / K, j = e < 0 ? 0 : e - slot * K + 1;
    const bool live = e >= 0 && j <= a.n_draft[slot];
    const uint64_t tp = live ? g.guide_trans[slot] : 0ull;
    g.guide_trans[r] = tp;
    g.guide_masks[r] = tp != 0 ? g.guide_masks[slot] : 0ull;
    g.guide_state[r] = tp != 0 ? g.draft_state[slot * K + j - 1] : 0;
    if (draft_row == nullptr && e >= 0 && !live) a.finished[r] = 1;     // kr_spec_propose ran before the trim
}

__global__ void __launch_bounds__(64) spec_guide_advance_kernel(const kr_spec a, const kr_spec_guide g) {
    __shared__ GuideStage s;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const uint64_t tp = g.guide_trans[slot];
    if (tp == 0) return;                              // (uniform per workgroup)
    const int before = g.ctx_before[slot], plen = a.prompt_len[slot];
    const int e = max(0, min(a.k + 1, a.ctx_len[slot] - before));
    // a step that finished the slot: its last token is not walked (kr_guide_advance skips the rows kr_sample_greedy has just finished)
    const int n = e > 0 && a.finished[slot] ? e - 1 : e;
    if (tid < n) {
        const int h = before + 1 - plen + tid;
        guide_stage(s, tid, h >= 0 && h < a.hist_rows ? a.history[(int64_t)h * a.hist_stride + slot] : -1, a.vocab, g.vocab_off,
                    g.vocab_bytes);
    }
    __syncthreads();
    if (tid != 0 || n == 0) return;
    const uint16_t* trans = reinterpret_cast<const uint16_t*>(tp);
    unsigned st = (unsigned)g.guide_state[slot];
    for (int i = 0; i < n; ++i) st = guide_walk(s, i, st, trans, g.vocab_bytes);      // (len -1: the state stays, as in kr_guide_advance)
    g.guide_state[slot] = (int)st;
}

int spec_guide_check(const kr_spec* a, const kr_spec_guide* g, const char* who, bool shared_rows) {
    if (const int rc = spec_check(a, who, shared_rows)) return rc;
    KR_CHECK_ARG(g, "%s: null guide args", who);
    KR_CHECK_ARG(g->guide_trans && g->guide_masks && g->guide_state && g->vocab_off && g->vocab_bytes && g->draft_state && g->ctx_before,
                 "%s: null pointer in kr_spec_guide", who);
    KR_CHECK_ARG(g->mask_words > 0 && g->mask_words % 2 == 0 && (int64_t)g->mask_words * 32 >= a->vocab,
                 "%s: mask_words=%d must be even and cover the vocabulary", who, g->mask_words);
    return KR_OK;
}

// ---------------------------------------------------------------- controlled slots in a speculative step (kr_spec_controls)
// The sampler's per-slot state per draft: output counts and stop entries.  Integer work only.
//   spec_controls_trim_kernel   per slot, before any row is spent: the drafts end in front of the first one that is a stop entry of
//                               the slot's adjustment table, so a stop token can only be the LAST token a step emits and
//                               kr_stop_tokens behind the verification finishes the slot as it does in a plain step.
//   spec_controls_rows_kernel   ONE workgroup: depth[r] = how many drafts lie in front of row r (0: a slot's own row, a row nobody has).
//   spec_controls_count_kernel  per slot, after the verification: counts[slot][t] += 1 over the tokens the step emitted.
__global__ void __launch_bounds__(64) spec_controls_trim_kernel(const kr_spec a, const kr_spec_controls c, int32_t* __restrict__ n_count) {
    const int slot = blockIdx.x, tid = threadIdx.x, K = a.k;
    if (tid == 0) c.ctx_before[slot] = a.ctx_len[slot];
    const int ne = min(max(c.adj_meta[slot * 4], 0), KR_ADJ_CAP);
    if (ne == 0 || a.finished[slot]) return;          // (uniform per workgroup) the slot keeps its count and its drafts
    const int n = max(0, min(K, n_count[slot]));
    const int64_t t0 = (int64_t)slot * KR_ADJ_CAP;
    int first = n;                                    // 0-based index of the first draft that is a stop entry
    for (int e = tid; e < ne; e += 64) {
        if ((c.adj_flag[t0 + e] & 1) == 0) continue;
        const int id = c.adj_ids[t0 + e];
        for (int j = 0; j < first; ++j)
            if (a.draft_tok[slot * K + j] == id) first = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (tid != 0 || first >= n) return;
    n_count[slot] = first;
    for (int j = first; j < K; ++j) a.draft_tok[slot * K + j] = a.pad_id;
}

// draft_row == nullptr: the static layout (draft j of a slot on row j * slots + slot); else the map kr_spec_deal wrote.  As in
// spec_guide_rows_kernel every global write is indexed by a row taken from the thread index, never by a computed row.
__global__ void __launch_bounds__(64) spec_controls_rows_kernel(const kr_spec a, const kr_spec_controls c,
                                                                const int32_t* __restrict__ draft_row) {
    __shared__ int s_owner[SPEC_MAX_ROWS];
    const int tid = threadIdx.x, B = a.slots, K = a.k, R = a.rows;
    if (tid < SPEC_MAX_ROWS) {
        int e = -1;
        if (draft_row == nullptr && tid >= B && tid < B * (K + 1)) e = (tid % B) * K + tid / B - 1;
        s_owner[tid] = e;
    }
    __syncthreads();
    if (draft_row != nullptr)
        for (int e = tid; e < B * K; e += 64) {
            const int r = draft_row[e];
            if (r >= B && r < R) s_owner[r] = e;       // (rows are distinct: one writer per entry)
        }
    __syncthreads();
    const int r = tid;
    if (r >= R) return;
    const int e = r < B ? -1 : s_owner[r];
    const int slot = e < 0 ? 0 : e / K, j = e < 0 ? 0 : e - slot * K + 1;
    const bool live = e >= 0 && j <= a.n_draft[slot];
    c.depth[r] = live ? j : 0;
    if (draft_row == nullptr && e >= 0 && !live) a.finished[r] = 1;     // kr_spec_propose ran before the trim
}

__global__ void __launch_bounds__(64) spec_controls_count_kernel(const kr_spec a, const kr_spec_controls c) {
    const int slot = blockIdx.x;
    if (threadIdx.x != 0) return;           // at most k + 1 tokens, and two of them may be one id: one thread adds them in turn
    const int before = c.ctx_before[slot], plen = a.prompt_len[slot];
    const int e = max(0, min(a.k + 1, a.ctx_len[slot] - before));      // (a frozen finished slot: 0)
    for (int i = 0; i < e; ++i) {
        const int h = before + 1 - plen + i;
        if (h < 0 || h >= a.hist_rows) continue;
        const int t = a.history[(int64_t)h * a.hist_stride + slot];
        if (t >= 0 && t < a.vocab) c.counts[(int64_t)slot * c.ld_counts + t] += 1;
    }
}

int spec_controls_check(const kr_spec* a, const kr_spec_controls* c, const char* who, bool shared_rows) {
    if (const int rc = spec_check(a, who, shared_rows)) return rc;
    KR_CHECK_ARG(c, "%s: null controls args", who);
    KR_CHECK_ARG(c->adj_ids && c->adj_flag && c->adj_meta && c->counts && c->depth && c->ctx_before, "%s: null pointer in kr_spec_controls",
                 who);
    KR_CHECK_ARG(c->ld_counts >= a->vocab, "%s: ld_counts=%lld below the vocabulary", who, (long long)c->ld_counts);
    return KR_OK;
}

// ---------------------------------------------------------------- log-probabilities of a speculative step (kr_spec_logprobs)
// One record per token the step emitted and a plain step would have recorded: token j of a slot was chosen on the row of draft j
// (j = 0: the slot's own row), and a draft row's logits are the bits a one-row step at that context computes, so the record is
// kr_logprobs_topk's on a one-row batch holding that row (kr_logprobs.h: the same two bodies).
//   spec_mark_kernel            ctx_before = ctx_len where neither trim ran
//   spec_logprob_partial_kernel grid (n_part, slots * (k + 1)): the slices of the rows that record; every other workgroup returns at once
//   spec_logprob_merge_kernel   grid slots * (k + 1): the record of (slot, j) at its token's history index
__global__ void __launch_bounds__(64) spec_mark_kernel(const int32_t* __restrict__ ctx_len, int32_t* __restrict__ ctx_before, int slots) {
    const int slot = threadIdx.x;
    if (slot < slots) ctx_before[slot] = ctx_len[slot];
}

// Whether token j of `slot` records, on which row and at which history index (uniform per workgroup).  e tokens were emitted; the
// one that finished the slot (EOS, stop entry) records nothing, as in a plain step; a slot that idled (finished, frozen) has e = 0.
__device__ __forceinline__ bool spec_logprob_record(const kr_spec& a, const kr_spec_logprobs& p, const int32_t* __restrict__ draft_row,
                                                    int slot, int j, int& row, int& h) {
    const int before = p.ctx_before[slot];
    const int e = max(0, min(a.k + 1, a.ctx_len[slot] - before));
    const int n_rec = e - (a.finished[slot] != 0 ? 1 : 0);
    if (j >= n_rec) return false;
    row = j == 0 ? slot : draft_row == nullptr ? j * a.slots + slot : draft_row[slot * a.k + j - 1];
    if (row < 0 || row >= a.rows) return false;
    h = before + 1 + j - a.prompt_len[slot];
    return h >= 0 && h < p.hist_len && h < a.hist_rows;      // (the token is read from history[h]: kr_spec_accept wrote none past it)
}

__global__ void __launch_bounds__(256) spec_logprob_partial_kernel(const kr_spec a, const kr_spec_logprobs p,
                                                                   const int32_t* __restrict__ draft_row,
                                                                   const float* __restrict__ logits, int64_t ld) {
    const int part = blockIdx.x, slot = blockIdx.y / (a.k + 1), j = blockIdx.y - slot * (a.k + 1);
    int row, h;
    if (!spec_logprob_record(a, p, draft_row, slot, j, row, h)) return;
    const int64_t bp = (int64_t)row * p.n_part + part;
    logprob_partial_body(logits + (int64_t)row * ld, a.vocab, p.k_top, part, p.n_part, p.part_val + bp * p.k_top,
                         p.part_idx + bp * p.k_top, p.part_ms + bp * 2);
}

__global__ void __launch_bounds__(256) spec_logprob_merge_kernel(const kr_spec a, const kr_spec_logprobs p,
                                                                 const int32_t* __restrict__ draft_row,
                                                                 const float* __restrict__ logits, int64_t ld) {
    extern __shared__ float cand[];                          // n_part * k_top values, then as many indices
    const int slot = blockIdx.x / (a.k + 1), j = blockIdx.x - slot * (a.k + 1);
    int row, h;
    if (!spec_logprob_record(a, p, draft_row, slot, j, row, h)) return;
    const int k = p.k_top, nc = p.n_part * k;
    const int tok = a.history[(int64_t)h * a.hist_stride + slot];
    const int64_t o = (int64_t)h * p.hist_batch + slot;
    logprob_merge_body(p.part_val + (int64_t)row * nc, p.part_idx + (int64_t)row * nc, p.part_ms + (int64_t)row * p.n_part * 2, p.n_part,
                       k, logits + (int64_t)row * ld, a.vocab, tok, p.out_lp + o * (1 + p.k_stride), p.out_idx + o * p.k_stride, cand);
}

}  // namespace

extern "C" int kr_spec_mark(const kr_spec* a, int32_t* ctx_before, kr_stream s) {
    if (const int rc = spec_check(a, "kr_spec_mark", true)) return rc;
    KR_CHECK_ARG(ctx_before, "kr_spec_mark: null ctx_before");
    spec_mark_kernel<<<1, 64, 0, kr_hs(s)>>>(a->ctx_len, ctx_before, a->slots);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_logprobs_topk_rows(const kr_spec* a, const kr_spec_logprobs* p, const int32_t* draft_row, const float* logits,
                                     int64_t ld_logits, kr_stream s) {
    if (const int rc = spec_check(a, "kr_logprobs_topk_rows", draft_row != nullptr)) return rc;
    KR_CHECK_ARG(p, "kr_logprobs_topk_rows: null log-probability args");
    KR_CHECK_ARG(logits && p->part_val && p->part_idx && p->part_ms && p->out_lp && p->out_idx && p->ctx_before,
                 "kr_logprobs_topk_rows: null pointer");
    KR_CHECK_ARG(ld_logits >= a->vocab && a->slots <= p->hist_batch && p->hist_len > 0, "kr_logprobs_topk_rows: bad sizes");
    if (const int rc = logprob_check_sizes("kr_logprobs_topk_rows", a->vocab, p->k_top, p->k_stride, p->n_part)) return rc;
    const size_t lds = (size_t)p->n_part * (p->k_top > 0 ? p->k_top : 1) * 8;
    static KrPerDeviceOnce attr;
    if (attr.need()) {
        KR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spec_logprob_merge_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)LP_MERGE_LDS));
    }
    const int n_tok = a->slots * (a->k + 1);
    spec_logprob_partial_kernel<<<dim3(p->n_part, n_tok), 256, 0, kr_hs(s)>>>(*a, *p, draft_row, logits, ld_logits);
    KR_CHECK_LAUNCH();
    spec_logprob_merge_kernel<<<n_tok, 256, lds, kr_hs(s)>>>(*a, *p, draft_row, logits, ld_logits);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_controls_trim(const kr_spec* a, const kr_spec_controls* c, int32_t* n_count, kr_stream s) {
    if (const int rc = spec_controls_check(a, c, "kr_spec_controls_trim", true)) return rc;
    KR_CHECK_ARG(n_count, "kr_spec_controls_trim: null n_count");
    spec_controls_trim_kernel<<<a->slots, 64, 0, kr_hs(s)>>>(*a, *c, n_count);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_controls_rows(const kr_spec* a, const kr_spec_controls* c, const int32_t* draft_row, kr_stream s) {
    if (const int rc = spec_controls_check(a, c, "kr_spec_controls_rows", draft_row != nullptr)) return rc;
    spec_controls_rows_kernel<<<1, 64, 0, kr_hs(s)>>>(*a, *c, draft_row);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_controls_count(const kr_spec* a, const kr_spec_controls* c, kr_stream s) {
    if (const int rc = spec_controls_check(a, c, "kr_spec_controls_count", true)) return rc;
    spec_controls_count_kernel<<<a->slots, 64, 0, kr_hs(s)>>>(*a, *c);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_guide_trim(const kr_spec* a, const kr_spec_guide* g, int32_t* n_count, kr_stream s) {
    if (const int rc = spec_guide_check(a, g, "kr_spec_guide_trim", true)) return rc;
    KR_CHECK_ARG(n_count, "kr_spec_guide_trim: null n_count");
    spec_guide_trim_kernel<<<a->slots, 64, 0, kr_hs(s)>>>(*a, *g, n_count);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_guide_rows(const kr_spec* a, const kr_spec_guide* g, const int32_t* draft_row, kr_stream s) {
    if (const int rc = spec_guide_check(a, g, "kr_spec_guide_rows", draft_row != nullptr)) return rc;
    spec_guide_rows_kernel<<<1, 64, 0, kr_hs(s)>>>(*a, *g, draft_row);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_guide_advance(const kr_spec* a, const kr_spec_guide* g, kr_stream s) {
    if (const int rc = spec_guide_check(a, g, "kr_spec_guide_advance", true)) return rc;
    spec_guide_advance_kernel<<<a->slots, 64, 0, kr_hs(s)>>>(*a, *g);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_propose(const kr_spec* a, kr_stream s) {
    if (const int rc = spec_check(a, "kr_spec_propose")) return rc;
    spec_propose_kernel<<<a->slots, 256, 0, kr_hs(s)>>>(*a);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_accept(const kr_spec* a, const float* amax_val, const int32_t* amax_idx, int n_part, int32_t* tokens_out,
                              const int32_t* eos, int n_eos, int ignore_eos, kr_stream s) {
    if (const int rc = spec_check(a, "kr_spec_accept")) return rc;
    KR_CHECK_ARG(amax_val && amax_idx && tokens_out && n_part > 0 && (n_eos == 0 || eos), "kr_spec_accept: bad args");
    spec_accept_kernel<<<a->slots, 256, 0, kr_hs(s)>>>(*a, amax_val, amax_idx, n_part, tokens_out, eos, n_eos, ignore_eos, nullptr);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_lookup(const kr_spec* a, int32_t* n_want, kr_stream s) {
    if (const int rc = spec_check(a, "kr_spec_lookup", true)) return rc;
    KR_CHECK_ARG(n_want, "kr_spec_lookup: null n_want");
    spec_lookup_kernel<<<a->slots, 256, 0, kr_hs(s)>>>(*a, n_want);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_deal(const kr_spec* a, const int32_t* n_want, int32_t* draft_row, kr_stream s) {
    if (const int rc = spec_check(a, "kr_spec_deal", true)) return rc;
    KR_CHECK_ARG(n_want && draft_row, "kr_spec_deal: null n_want / draft_row");
    spec_deal_kernel<<<1, 256, 0, kr_hs(s)>>>(*a, n_want, draft_row);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_spec_accept_rows(const kr_spec* a, const int32_t* draft_row, const float* amax_val, const int32_t* amax_idx, int n_part,
                                   int32_t* tokens_out, const int32_t* eos, int n_eos, int ignore_eos, kr_stream s) {
    if (const int rc = spec_check(a, "kr_spec_accept_rows", true)) return rc;
    KR_CHECK_ARG(draft_row && amax_val && amax_idx && tokens_out && n_part > 0 && (n_eos == 0 || eos), "kr_spec_accept_rows: bad args");
    spec_accept_kernel<<<a->slots, 256, 0, kr_hs(s)>>>(*a, amax_val, amax_idx, n_part, tokens_out, eos, n_eos, ignore_eos, draft_row);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
