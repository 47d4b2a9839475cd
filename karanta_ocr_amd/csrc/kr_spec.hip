// The two ends of a speculative decode step (include/karanta_hip.h, kr_spec): prompt-lookup drafts in, verified tokens out.
//   spec_propose_kernel  per slot: the longest n-gram (ngram_max .. ngram_min) that ends the sequence is looked up earlier in
//                        prompt + history; the tokens after the match are the drafts.  Fills the draft rows of the step: their
//                        slot, position, sampler state and input embedding.
//   spec_accept_kernel   per slot: final argmax of its k + 1 rows, then kr_sample_greedy's bookkeeping token by token while the
//                        drafts agree with what the rows before them produced.
// Between them the rows run through the packed decode family with kr_linear_decode32_rows / kr_attn_decode_rows.
#include "kr_decode_common.h"

namespace {

constexpr int SPEC_MAX_ROWS = 32, SPEC_MAX_NGRAM = 8;

__global__ void __launch_bounds__(256) spec_propose_kernel(const kr_spec a) {
    __shared__ unsigned s_key[4];
    __shared__ int s_nd, s_draft[SPEC_MAX_ROWS];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.slots, K = a.k;
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
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = s_key[w] > best ? s_key[w] : best;
        int nd = 0;
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
        s_nd = nd;
        a.n_draft[slot] = nd;
        for (int j = 0; j < K; ++j) a.draft_tok[slot * K + j] = j < nd ? s_draft[j] : a.pad_id;
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

__global__ void __launch_bounds__(256) spec_accept_kernel(const kr_spec a, const float* __restrict__ amax_val,
                                                          const int32_t* __restrict__ amax_idx, int n_part,
                                                          int32_t* __restrict__ tokens_out, const int32_t* __restrict__ eos, int n_eos,
                                                          int flags) {
    __shared__ int s_t[SPEC_MAX_ROWS], s_last;
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.slots, K = a.k;
    // t_j: one wave per row, kr_sample_greedy's order (`better`: the larger value, ties to the lowest index)
    for (int j = wave; j <= K; j += 4) {
        const int64_t r = (int64_t)(j * B + slot) * n_part;
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
            const int nd = a.n_draft[slot];
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

int spec_check(const kr_spec* a, const char* who) {
    KR_CHECK_ARG(a, "%s: null args", who);
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

}  // namespace

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
    spec_accept_kernel<<<a->slots, 256, 0, kr_hs(s)>>>(*a, amax_val, amax_idx, n_part, tokens_out, eos, n_eos, ignore_eos);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
