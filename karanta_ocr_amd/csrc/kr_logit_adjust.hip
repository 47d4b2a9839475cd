// Per-request logit adjustments of a decode step (vLLM's logit_bias, min_tokens and stop_token_ids), applied on the device
// around the sampler of kr_sample.hip; DESIGN.md §5c.
//   logits_adjust_kernel   saves logits[b][id] of every table entry, then l += bias (fp32) and, while the row has generated
//                          fewer than min_tokens tokens, l = -inf on its stop entries (the mask wins over a bias)
//   logits_restore_kernel  writes the saved values back: the buffer is again what the lm_head wrote, bit for bit, for
//                          kr_logprobs_topk and return_logits
//   stop_tokens_kernel     after kr_sample_greedy: a live row whose token is one of its stop entries finishes as on EOS
//   logits_adjust_rows_kernel  the adjust body over the rows of a speculative step (ROWS): a row is adjusted with the table of its
//                          slot at the row's own token index; saved is per row
//   logits_restore_rows_kernel  its inverse, for a speculative step that records log-probabilities (kr_logprobs_topk_rows reads the
//                          lm_head's bits); a step that records nothing has no restore launch: nothing reads the
//                          logits behind the token choice and the next lm_head launch overwrites them
// Tables, per row, KR_ADJ_CAP entries wide, every id at most once in a row (the host merges bias keys, stop ids and EOS ids):
// adj_ids / adj_val / adj_flag (bit 0 = stop entry) and adj_meta[b] = {n_entries, min_tokens, 0, 0}.  One wave per row, the
// entries strided over its lanes; unique ids: plain loads and stores, no atomics.  n_entries is clamped to the table width
// and an id outside the vocabulary is skipped, so a corrupt table cannot reach past a row.
#include "kr_decode_common.h"

namespace {

constexpr int ADJ_META = 4;

__device__ __forceinline__ int adj_entries(const int32_t* meta) { return min(max(meta[0], 0), KR_ADJ_CAP); }

// ROWS: logits, ctx_len, prompt_len and saved are per row, the table is that of the row's slot
template <bool ROWS>
__device__ __forceinline__ void logits_adjust_body(float* __restrict__ logits, int64_t ld, int vocab,
                                                   const int32_t* __restrict__ adj_ids, const float* __restrict__ adj_val,
                                                   const int32_t* __restrict__ adj_flag, const int32_t* __restrict__ adj_meta,
                                                   const int32_t* __restrict__ ctx_len, const int32_t* __restrict__ prompt_len,
                                                   float* __restrict__ saved, const int32_t* __restrict__ row_slot, int slots) {
    const int b = blockIdx.x;
    const int sl = ROWS ? min(max(row_slot[b], 0), slots - 1) : b;
    const int32_t* meta = adj_meta + (int64_t)sl * ADJ_META;
    const int n = adj_entries(meta);
    if (n == 0) return;
    // index of the token being generated in its sequence: what the Gumbel kernels count with
    const bool mask = (ctx_len[b] + 1 - prompt_len[b]) < meta[1];
    float* row = logits + (int64_t)b * ld;
    const int64_t t0 = (int64_t)sl * KR_ADJ_CAP, s0 = (int64_t)b * KR_ADJ_CAP;
    for (int e = threadIdx.x; e < n; e += 64) {
        const int id = adj_ids[t0 + e];
        if (id < 0 || id >= vocab) continue;
        const float l = row[id];
        saved[s0 + e] = l;
        row[id] = (mask && (adj_flag[t0 + e] & 1)) ? -INFINITY : l + adj_val[t0 + e];
    }
}

__global__ void __launch_bounds__(64) logits_adjust_kernel(float* __restrict__ logits, int64_t ld, int vocab,
                                                           const int32_t* __restrict__ adj_ids, const float* __restrict__ adj_val,
                                                           const int32_t* __restrict__ adj_flag, const int32_t* __restrict__ adj_meta,
                                                           const int32_t* __restrict__ ctx_len, const int32_t* __restrict__ prompt_len,
                                                           float* __restrict__ saved) {
    logits_adjust_body<false>(logits, ld, vocab, adj_ids, adj_val, adj_flag, adj_meta, ctx_len, prompt_len, saved, nullptr, 0);
}

__global__ void __launch_bounds__(64) logits_adjust_rows_kernel(float* __restrict__ logits, int64_t ld, int vocab,
                                                                const int32_t* __restrict__ adj_ids, const float* __restrict__ adj_val,
                                                                const int32_t* __restrict__ adj_flag,
                                                                const int32_t* __restrict__ adj_meta,
                                                                const int32_t* __restrict__ ctx_len,
                                                                const int32_t* __restrict__ prompt_len, float* __restrict__ saved,
                                                                const int32_t* __restrict__ row_slot, int slots) {
    logits_adjust_body<true>(logits, ld, vocab, adj_ids, adj_val, adj_flag, adj_meta, ctx_len, prompt_len, saved, row_slot, slots);
}

__global__ void __launch_bounds__(64) logits_restore_kernel(float* __restrict__ logits, int64_t ld, int vocab,
                                                            const int32_t* __restrict__ adj_ids,
                                                            const int32_t* __restrict__ adj_meta, const float* __restrict__ saved) {
    const int b = blockIdx.x;
    const int n = adj_entries(adj_meta + (int64_t)b * ADJ_META);
    float* row = logits + (int64_t)b * ld;
    const int64_t t0 = (int64_t)b * KR_ADJ_CAP;
    for (int e = threadIdx.x; e < n; e += 64) {
        const int id = adj_ids[t0 + e];
        if (id < 0 || id >= vocab) continue;
        row[id] = saved[t0 + e];
    }
}

// row b is restored with the table of its slot (clamped as in logits_adjust_body<true>); saved is per row
__global__ void __launch_bounds__(64) logits_restore_rows_kernel(float* __restrict__ logits, int64_t ld, int vocab,
                                                                 const int32_t* __restrict__ adj_ids,
                                                                 const int32_t* __restrict__ adj_meta, const float* __restrict__ saved,
                                                                 const int32_t* __restrict__ row_slot, int slots) {
    const int b = blockIdx.x;
    const int sl = min(max(row_slot[b], 0), slots - 1);
    const int n = adj_entries(adj_meta + (int64_t)sl * ADJ_META);
    float* row = logits + (int64_t)b * ld;
    const int64_t t0 = (int64_t)sl * KR_ADJ_CAP, s0 = (int64_t)b * KR_ADJ_CAP;
    for (int e = threadIdx.x; e < n; e += 64) {
        const int id = adj_ids[t0 + e];
        if (id < 0 || id >= vocab) continue;
        row[id] = saved[s0 + e];
    }
}

__global__ void __launch_bounds__(64) stop_tokens_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ adj_ids,
                                                         const int32_t* __restrict__ adj_flag, const int32_t* __restrict__ adj_meta,
                                                         int32_t* __restrict__ finished) {
    const int b = blockIdx.x;
    const int n = adj_entries(adj_meta + (int64_t)b * ADJ_META);
    if (n == 0 || finished[b] != 0) return;       // a finished row holds the pad token, not a sampled one
    const int tok = tokens[b];
    const int64_t t0 = (int64_t)b * KR_ADJ_CAP;
    bool hit = false;
    for (int e = threadIdx.x; e < n; e += 64) hit |= (adj_flag[t0 + e] & 1) && adj_ids[t0 + e] == tok;
    if (__ballot(hit) != 0ull && threadIdx.x == 0) finished[b] = 1;
}

}  // namespace

extern "C" int kr_logits_adjust(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const float* adj_val,
                                const int32_t* adj_flag, const int32_t* adj_meta, const int32_t* ctx_len,
                                const int32_t* prompt_len, float* saved, int batch, kr_stream s) {
    KR_CHECK_ARG(logits && adj_ids && adj_val && adj_flag && adj_meta && ctx_len && prompt_len && saved,
                 "kr_logits_adjust: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && batch > 0, "kr_logits_adjust: bad sizes");
    logits_adjust_kernel<<<batch, 64, 0, kr_hs(s)>>>(logits, ld_logits, vocab, adj_ids, adj_val, adj_flag, adj_meta, ctx_len,
                                                     prompt_len, saved);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_logits_adjust_rows(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const float* adj_val,
                                     const int32_t* adj_flag, const int32_t* adj_meta, const int32_t* ctx_len,
                                     const int32_t* prompt_len, float* saved, int batch, const int32_t* row_slot, int slots,
                                     kr_stream s) {
    KR_CHECK_ARG(logits && adj_ids && adj_val && adj_flag && adj_meta && ctx_len && prompt_len && saved && row_slot,
                 "kr_logits_adjust_rows: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && batch > 0, "kr_logits_adjust_rows: bad sizes");
    KR_CHECK_ARG(slots >= 1 && slots <= batch && batch <= 32, "kr_logits_adjust_rows: slots=%d rows=%d (1 <= slots <= rows <= 32)",
                 slots, batch);
    logits_adjust_rows_kernel<<<batch, 64, 0, kr_hs(s)>>>(logits, ld_logits, vocab, adj_ids, adj_val, adj_flag, adj_meta, ctx_len,
                                                          prompt_len, saved, row_slot, slots);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_logits_restore(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const int32_t* adj_meta,
                                 const float* saved, int batch, kr_stream s) {
    KR_CHECK_ARG(logits && adj_ids && adj_meta && saved, "kr_logits_restore: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && batch > 0, "kr_logits_restore: bad sizes");
    logits_restore_kernel<<<batch, 64, 0, kr_hs(s)>>>(logits, ld_logits, vocab, adj_ids, adj_meta, saved);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_logits_restore_rows(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const int32_t* adj_meta,
                                      const float* saved, int batch, const int32_t* row_slot, int slots, kr_stream s) {
    KR_CHECK_ARG(logits && adj_ids && adj_meta && saved && row_slot, "kr_logits_restore_rows: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && batch > 0, "kr_logits_restore_rows: bad sizes");
    KR_CHECK_ARG(slots >= 1 && slots <= batch && batch <= 32, "kr_logits_restore_rows: slots=%d rows=%d (1 <= slots <= rows <= 32)",
                 slots, batch);
    logits_restore_rows_kernel<<<batch, 64, 0, kr_hs(s)>>>(logits, ld_logits, vocab, adj_ids, adj_meta, saved, row_slot, slots);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_stop_tokens(const int32_t* tokens, const int32_t* adj_ids, const int32_t* adj_flag, const int32_t* adj_meta,
                              int32_t* finished, int ignore_eos, int batch, kr_stream s) {
    KR_CHECK_ARG(tokens && adj_ids && adj_flag && adj_meta && finished, "kr_stop_tokens: null pointer");
    KR_CHECK_ARG(batch > 0, "kr_stop_tokens: bad sizes");
    if (ignore_eos & 1) return KR_OK;             // fixed-length runs: no row finishes, on a stop entry as little as on EOS
    stop_tokens_kernel<<<batch, 64, 0, kr_hs(s)>>>(tokens, adj_ids, adj_flag, adj_meta, finished);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
