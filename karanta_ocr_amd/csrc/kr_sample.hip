// The on-device sampler of a decode step: from the lm_head's fp32 logits / ARGMAX partials (kr_linear_decode_wide) to the
// next step's input rows.
//   gumbel_argmax_kernel  temperature sampling as an argmax (Gumbel-max) over the logits, guide mask applied
//   sample_threshold_kernel / gumbel_argmax_proc_kernel / sample_count_kernel  vLLM's sampling controls (top_k, top_p,
//                         min_p, repetition / frequency / presence penalties) around the same argmax; DESIGN.md §5c
//   <..., ROWS>           the same two bodies over the rows of a speculative step (ROWS): params, counts and prompt bits are those
//                         of the row's slot, and the counts take in the drafts in front of the row; DESIGN.md §5o
//   sample_greedy_kernel  final argmax over the partials, token history, EOS bookkeeping, next-token embedding gather,
//                         context advance.  (The rotary table of every decode position is built once per request on the host.)
#include "kr_decode_common.h"

namespace {

// =====================================================================================
// temperature sampling as an argmax (Gumbel-max): token = argmax_i( logit_i / T + G_i )
// =====================================================================================
// G_i = -ln(-ln(u_i)), u_i = ((h_i >> 9) + 0.5) * 2^-23, h_i = mix(mix(seed ^ n * 0x9E3779B1) + i) with
// mix = the "lowbias32" integer finaliser and n = the index of the token being generated in its sequence
// (ctx_len + 1 - prompt_len).  A counter-based generator: no state, any (sequence, step, token) draw can be
// recomputed — the oracle does exactly that.  T == 0 rows get no noise: plain argmax, ties to the lowest index.
// The reference's requests carry temperature 0.1 (first attempt, karanta/pipeline.py:281,301) or 0.7
// (VLLMClient.generate default, bulk_processing/workers/vllm_client.py:155); vLLM's own sampler draws from the
// same softmax(logits / T) distribution with a different generator.
__device__ __forceinline__ unsigned kr_mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// guided slot: allowed-token bits of row b's DFA state (kr_guide_build_masks); nullptr = unconstrained
__device__ __forceinline__ const uint32_t* kr_guide_row(const uint64_t* guide_masks, const int32_t* guide_state, int mask_words,
                                                        int b) {
    if (guide_masks == nullptr || guide_masks[b] == 0) return nullptr;
    return reinterpret_cast<const uint32_t*>(guide_masks[b]) + (int64_t)guide_state[b] * mask_words;
}

// G_i of token i for the row whose counter base is `base` (kr_mix32 of its seed and step)
__device__ __forceinline__ float kr_gumbel_noise(unsigned base, int i) {
    const unsigned h = kr_mix32(base + (unsigned)i);
    // 23-bit integer + 0.5 is exact in f32 (24 significant bits): u in [2^-24, 1 - 2^-24], never 0 or 1
    // (a 24-bit integer + 0.5 rounds to 2^24 at the top code: u = 1, noise = +inf)
    const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;  // 2^-23
    return -logf(-logf(u));
}

// =====================================================================================
// sampling controls: penalties, min_p / top_k / top_p truncation (vLLM's sampling parameters)
// =====================================================================================
// Per row, on the fp32 lm_head logits l, after the guide mask: repetition penalty r on every token of the prompt set or
// with an output count c > 0 (l > 0 ? l / r : l * r), then l -= f * c + p * (c > 0); v = l * (1 / T); truncation keeps
// v >= a per-row threshold (min_p: v_max + ln(min_p); top_k: the k-th largest v; top_p: the v at which the mass of the
// descending v reaches p, over what min_p / top_k kept; the largest of the three), and the Gumbel-max argmax runs over
// the kept tokens with the noise of gumbel_argmax_kernel unchanged: a draw from the renormalised truncated softmax.
// params[b][KR_SP_STRIDE] = {top_k (<= 0: off), top_p (>= 1: off), min_p (<= 0: off), repetition, frequency, presence}.
constexpr int KR_SP_STRIDE = 8;

__device__ __forceinline__ uint32_t kr_fkey(float v) {   // order-preserving: a < b <=> key(a) < key(b) (-0 < +0)
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool kr_sp_penalised(const float* prm) {
    return prm[3] != 1.0f || prm[4] != 0.0f || prm[5] != 0.0f;
}

// fp32, this operation order, no fused multiply-add: the numpy restatement matches bit for bit
__device__ __forceinline__ float kr_penalise(float l, uint32_t in_prompt, int c, float rep, float freq, float pres) {
#pragma clang fp contract(off)
    if (in_prompt != 0u || c > 0) l = l > 0.f ? l / rep : l * rep;
    const float cf = (float)c;
    const float sub = freq * cf + pres * (c > 0 ? 1.0f : 0.0f);
    return l - sub;
}

// A row of a speculative step (ROWS): the sampler state of a row is its slot's, and its output so far is the slot's plus the drafts
// d_1..d_depth in front of it (draft_tok [slots][k]).  nx = how many of them the penalties have to look at: 0 for a slot's own
// row, a parked row and a row without penalties, so those run the loop-free expression.  Everything here is uniform per workgroup.
struct SpecRow {
    int slot, nx;
    const int32_t* dt;
};

template <bool ROWS>
__device__ __forceinline__ int kr_row_slot(int b, const int32_t* row_slot, int slots) {
    return ROWS ? min(max(row_slot[b], 0), slots - 1) : b;      // (a corrupt map cannot reach past the slots' arrays)
}

template <bool ROWS>
__device__ __forceinline__ SpecRow kr_spec_row(int b, bool pen, const int32_t* row_slot, const int32_t* depth,
                                               const int32_t* draft_tok, int k, int slots) {
    SpecRow r{b, 0, nullptr};
    if constexpr (ROWS) {
        r.slot = kr_row_slot<ROWS>(b, row_slot, slots);
        r.nx = pen ? min(max(depth[b], 0), k) : 0;
        r.dt = draft_tok + (int64_t)r.slot * k;
    }
    return r;
}

// the count of token i in the row's output so far: the slot's, plus the drafts in front of the row that are token i
__device__ __forceinline__ int kr_row_count(const int32_t* cnt, int i, const SpecRow& r) {
    int c = cnt[i];
    for (int e = 0; e < r.nx; ++e) c += (r.dt[e] == i) ? 1 : 0;
    return c;
}

__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned lo = (unsigned)__shfl_up((int)(unsigned)x, o, 64);
        const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(x >> 32), o, 64);
        if (lane >= o) x += ((unsigned long long)hi << 32) | lo;
    }
    return x;
}

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long x, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)x, src, 64), hi = (unsigned)__shfl((int)(unsigned)(x >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}

constexpr int SEL_T = 1024;

// Radix select over the keys of one row's scores w (excluded tokens hold -inf): the largest key t >= lo whose weight
// sum over keys >= t reaches the target, in three histogram passes (11 / 11 / 10 key bits).  Weights: 1 (count mode,
// target = k), or exp(v - vmax) in 32.32 fixed point (mass mode, target = ceil(frac * mass of the keys >= lo)).  Integer
// LDS atomics: the histograms, and so the result, do not depend on the order the threads add in.  Returns lo when the
// keys >= lo weigh less than the target (k above the surviving count).
__device__ uint32_t radix_select(const float* __restrict__ w, int vocab, uint32_t lo, bool mass, float vmax, double want,
                                 unsigned long long* hist, unsigned long long* s_misc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t prefix = 0, hi_mask = 0;
    unsigned long long target = 0;
    for (int lvl = 0; lvl < 3; ++lvl) {
        const int shift = lvl == 0 ? 21 : lvl == 1 ? 10 : 0;
        const int nb = lvl == 2 ? 1024 : 2048;
        for (int j = tid; j < 2048; j += SEL_T) hist[j] = 0ull;
        __syncthreads();
        for (int i0 = tid; i0 < vocab; i0 += 4 * SEL_T) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * SEL_T;
                v[u] = i < vocab ? w[i] : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t k = kr_fkey(v[u]);
                if (k >= lo && (k & hi_mask) == prefix) {
                    const unsigned long long wt = mass ? (unsigned long long)(__expf(v[u] - vmax) * 4294967296.0f) : 1ull;
                    // a zero weight never moves the crossing bin: the LDS atomic (the pass's cost) is skipped
                    if (wt != 0ull) atomicAdd(&hist[(k >> shift) & (nb - 1)], wt);
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            // lane l owns nb / 64 bins, highest keys first; the first lane whose inclusive sum reaches the target holds the bin
            const int per = nb / 64;
            const int top = nb - 1 - lane * per;
            unsigned long long sl = 0;
            for (int q = 0; q < per; ++q) sl += hist[top - q];
            const unsigned long long incl = wave_incl_scan_u64(sl, lane);
            if (lvl == 0) {
                const unsigned long long total = shfl_u64(incl, 63);
                if (mass) {
                    const double t = ceil(want * (double)total);
                    target = t < 1.0 ? 1ull : (t > (double)total ? total : (unsigned long long)t);
                } else {
                    target = (unsigned long long)want;
                }
            }
            const unsigned long long bal = __ballot(incl >= target);
            if (bal == 0ull) {
                if (lane == 0) s_misc[0] = 1ull;
            } else {
                const int L = __ffsll((long long)bal) - 1;
                const unsigned long long before = shfl_u64(incl - sl, L);
                const int topL = nb - 1 - L * per;
                const unsigned long long hq = lane < per ? hist[topL - lane] : 0ull;
                const unsigned long long inc2 = wave_incl_scan_u64(hq, lane) + before;
                const unsigned long long bal2 = __ballot(lane < per && inc2 >= target);
                const int Q = __ffsll((long long)bal2) - 1;
                const unsigned long long before2 = shfl_u64(inc2 - hq, Q);
                if (lane == 0) {
                    s_misc[0] = 0ull;
                    s_misc[1] = (unsigned long long)(topL - Q);
                    s_misc[2] = target - before2;
                }
            }
        }
        __syncthreads();
        if (s_misc[0] != 0ull) return lo;
        prefix |= (uint32_t)s_misc[1] << shift;
        hi_mask |= (uint32_t)(nb - 1) << shift;
        target = s_misc[2];
        __syncthreads();
    }
    return prefix;
}

// One workgroup per row: the row's scores (penalised, tempered, guide-masked; -inf where excluded) go to work once,
// v_max, then the min_p / top_k / top_p threshold key -> thr[b] (0: keep every allowed token).  Rows with T == 0 or
// neutral truncation stop after writing 0.  live[b]: whether kr_sample_greedy appends a real token to this row in this
// step (not a finished row's pad token) — what kr_sample_count counts.
// ROWS (kr_sample_threshold_rows): b is a row of a speculative step; logits, temperature, guide, finished, work, thr and live are per
// row, params / counts / prompt_bits per slot (kr_spec_row).  One kernel template, as dec32_kernel<..., ROWS>: the plain launch
// passes null for the row map and compiles to the code it had without it.
template <bool ROWS>
__global__ void __launch_bounds__(SEL_T) sample_threshold_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                                 const float* __restrict__ temperature,
                                                                 const float* __restrict__ params,
                                                                 const int32_t* __restrict__ counts, int64_t ld_counts,
                                                                 const uint32_t* __restrict__ prompt_bits, int bits_words,
                                                                 const uint64_t* __restrict__ guide_masks,
                                                                 const int32_t* __restrict__ guide_state, int mask_words,
                                                                 const int32_t* __restrict__ finished, int ignore_eos,
                                                                 float* __restrict__ work, int64_t ld_work,
                                                                 uint32_t* __restrict__ thr, int32_t* __restrict__ live,
                                                                 const int32_t* __restrict__ row_slot,
                                                                 const int32_t* __restrict__ depth,
                                                                 const int32_t* __restrict__ draft_tok, int k, int slots) {
    __shared__ unsigned long long hist[2048];
    __shared__ unsigned long long s_misc[4];
    __shared__ float s_m[SEL_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = kr_row_slot<ROWS>(b, row_slot, slots);
    const float* prm = params + (int64_t)sl * KR_SP_STRIDE;
    if (tid == 0) live[b] = ((ignore_eos & 1) != 0 || finished[b] == 0) ? 1 : 0;
    const float T = temperature[b];
    const int top_k = (int)prm[0];
    const float top_p = prm[1], min_p = prm[2];
    const bool use_k = top_k > 0 && top_k < vocab, use_p = top_p < 1.0f, use_m = min_p > 0.0f;
    if (!(T > 0.f) || !(use_k || use_p || use_m)) {
        if (tid == 0) thr[b] = 0u;
        return;
    }
    const float inv_t = 1.0f / T;
    const bool pen = kr_sp_penalised(prm);
    const float rep = prm[3], freq = prm[4], pres = prm[5];
    const SpecRow sr = kr_spec_row<ROWS>(b, pen, row_slot, depth, draft_tok, k, slots);
    const float* row = logits + (int64_t)b * ld;
    const int32_t* cnt = counts + (int64_t)sl * ld_counts;
    const uint32_t* pb = prompt_bits + (int64_t)sl * bits_words;
    float* wr = work + (int64_t)b * ld_work;
    const uint32_t* allow = kr_guide_row(guide_masks, guide_state, mask_words, b);
    float m = -INFINITY;
    for (int i = tid; i < vocab; i += SEL_T) {
        float v = -INFINITY;
        if (allow == nullptr || ((allow[i >> 5] >> (i & 31)) & 1u)) {
            float lp = row[i];
            if (pen) lp = kr_penalise(lp, (pb[i >> 5] >> (i & 31)) & 1u, kr_row_count(cnt, i, sr), rep, freq, pres);
            v = lp * inv_t;
        }
        wr[i] = v;
        m = fmaxf(m, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_m[wave] = m;
    __syncthreads();   // also orders this workgroup's work-row writes before its reads below
    m = s_m[0];
#pragma unroll
    for (int q = 1; q < SEL_T / 64; ++q) m = fmaxf(m, s_m[q]);
    uint32_t lo = kr_fkey(-INFINITY) + 1u;        // every allowed (finite) score
    if (use_m) {
        const uint32_t km = kr_fkey(m + logf(min_p));
        lo = km > lo ? km : lo;
    }
    if (use_k) {
        const uint32_t kk = radix_select(wr, vocab, lo, false, m, (double)top_k, hist, s_misc);
        lo = kk > lo ? kk : lo;
    }
    if (use_p) {
        const uint32_t kp = radix_select(wr, vocab, lo, true, m, (double)top_p, hist, s_misc);
        lo = kp > lo ? kp : lo;
    }
    if (tid == 0) thr[b] = lo;
}

// =====================================================================================
// the Gumbel-max partial argmax: [batch][n_part] partials for kr_sample_greedy's reduction
// =====================================================================================
// One body for both launches.  PROC (gumbel_argmax_proc_kernel) adds the penalties and the truncation threshold of
// sample_threshold_kernel; a row with neutral parameters (no penalty, threshold 0) runs the value expression of the plain
// launch and gets its partials bit for bit.
template <bool PROC, bool ROWS = false>
__device__ __forceinline__ void gumbel_argmax_body(const float* logits, int64_t ld, int vocab, const float* temperature,
                                                   const unsigned* seed, const int32_t* ctx_len, const int32_t* prompt_len,
                                                   float* amax_val, int32_t* amax_idx, const uint64_t* guide_masks,
                                                   const int32_t* guide_state, int mask_words, int fallback_token,
                                                   const float* params, const int32_t* counts, int64_t ld_counts,
                                                   const uint32_t* prompt_bits, int bits_words, const uint32_t* thr,
                                                   const int32_t* row_slot = nullptr, const int32_t* depth = nullptr,
                                                   const int32_t* draft_tok = nullptr, int k = 0, int slots = 0) {
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int p = blockIdx.x, n_part = gridDim.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (((vocab + n_part - 1) / n_part) + 3) & ~3;
    const int i0 = p * per, i1 = min(vocab, i0 + per);
    const float T = temperature[b];
    const float inv_t = T > 0.f ? 1.0f / T : 1.0f;
    const unsigned base = kr_mix32(seed[b] ^ ((unsigned)(ctx_len[b] + 1 - prompt_len[b]) * 0x9E3779B1u));
    const float* row = logits + (int64_t)b * ld;
    bool pen = false;
    float rep = 1.0f, freq = 0.0f, pres = 0.0f;
    const int32_t* cnt = nullptr;
    const uint32_t* pb = nullptr;
    uint32_t th = 0u;
    SpecRow sr{b, 0, nullptr};
    if constexpr (PROC) {
        const int sl = kr_row_slot<ROWS>(b, row_slot, slots);     // (ROWS: params, counts and prompt bits are the slot's, thr is the row's)
        const float* prm = params + (int64_t)sl * KR_SP_STRIDE;
        pen = kr_sp_penalised(prm);
        rep = prm[3], freq = prm[4], pres = prm[5];
        cnt = counts + (int64_t)sl * ld_counts;
        pb = prompt_bits + (int64_t)sl * bits_words;
        th = T > 0.f ? thr[b] : 0u;    // greedy rows: truncation cannot move the argmax
        sr = kr_spec_row<ROWS>(b, pen, row_slot, depth, draft_tok, k, slots);
    }
    const uint32_t* allow = kr_guide_row(guide_masks, guide_state, mask_words, b);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = i0 + tid; i < i1; i += 256) {
        if (allow != nullptr && !((allow[i >> 5] >> (i & 31)) & 1u)) continue;
        float lp = row[i];
        if (PROC && pen) lp = kr_penalise(lp, (pb[i >> 5] >> (i & 31)) & 1u, kr_row_count(cnt, i, sr), rep, freq, pres);
        float v = lp * inv_t;
        if (PROC && th != 0u && kr_fkey(v) < th) continue;
        if (T > 0.f) v += kr_gumbel_noise(base, i);
        better(bv, bi, v, i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        better(bv, bi, ov, oi);
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) better(bv, bi, s_v[w], s_i[w]);
        // a row whose mask allows nothing (cannot happen for a live DFA state) must still yield a valid token id
        if (p == 0 && bi == 0x7fffffff) bi = fallback_token;
        amax_val[(int64_t)b * n_part + p] = bv;
        amax_idx[(int64_t)b * n_part + p] = bi;
    }
}

__global__ void __launch_bounds__(256) gumbel_argmax_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                            const float* __restrict__ temperature,
                                                            const unsigned* __restrict__ seed,
                                                            const int32_t* __restrict__ ctx_len,
                                                            const int32_t* __restrict__ prompt_len,
                                                            float* __restrict__ amax_val, int32_t* __restrict__ amax_idx,
                                                            const uint64_t* __restrict__ guide_masks,
                                                            const int32_t* __restrict__ guide_state, int mask_words,
                                                            int fallback_token) {
    gumbel_argmax_body<false>(logits, ld, vocab, temperature, seed, ctx_len, prompt_len, amax_val, amax_idx, guide_masks,
                              guide_state, mask_words, fallback_token, nullptr, nullptr, 0, nullptr, 0, nullptr);
}

__global__ void __launch_bounds__(256) gumbel_argmax_proc_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                                 const float* __restrict__ temperature,
                                                                 const unsigned* __restrict__ seed,
                                                                 const int32_t* __restrict__ ctx_len,
                                                                 const int32_t* __restrict__ prompt_len,
                                                                 float* __restrict__ amax_val, int32_t* __restrict__ amax_idx,
                                                                 const uint64_t* __restrict__ guide_masks,
                                                                 const int32_t* __restrict__ guide_state, int mask_words,
                                                                 int fallback_token, const float* __restrict__ params,
                                                                 const int32_t* __restrict__ counts, int64_t ld_counts,
                                                                 const uint32_t* __restrict__ prompt_bits, int bits_words,
                                                                 const uint32_t* __restrict__ thr) {
    gumbel_argmax_body<true>(logits, ld, vocab, temperature, seed, ctx_len, prompt_len, amax_val, amax_idx, guide_masks,
                             guide_state, mask_words, fallback_token, params, counts, ld_counts, prompt_bits, bits_words, thr);
}

__global__ void __launch_bounds__(256) gumbel_argmax_proc_rows_kernel(
    const float* __restrict__ logits, int64_t ld, int vocab, const float* __restrict__ temperature, const unsigned* __restrict__ seed,
    const int32_t* __restrict__ ctx_len, const int32_t* __restrict__ prompt_len, float* __restrict__ amax_val,
    int32_t* __restrict__ amax_idx, const uint64_t* __restrict__ guide_masks, const int32_t* __restrict__ guide_state, int mask_words,
    int fallback_token, const float* __restrict__ params, const int32_t* __restrict__ counts, int64_t ld_counts,
    const uint32_t* __restrict__ prompt_bits, int bits_words, const uint32_t* __restrict__ thr, const int32_t* __restrict__ row_slot,
    const int32_t* __restrict__ depth, const int32_t* __restrict__ draft_tok, int k, int slots) {
    gumbel_argmax_body<true, true>(logits, ld, vocab, temperature, seed, ctx_len, prompt_len, amax_val, amax_idx, guide_masks,
                                   guide_state, mask_words, fallback_token, params, counts, ld_counts, prompt_bits, bits_words, thr,
                                   row_slot, depth, draft_tok, k, slots);
}

// after kr_sample_greedy: counts[b][tokens[b]] += 1 where live[b] (sample_threshold_kernel)
__global__ void __launch_bounds__(64) sample_count_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ live,
                                                          int32_t* __restrict__ counts, int64_t ld_counts, int vocab, int batch) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch || live[b] == 0) return;
    const int t = tokens[b];
    if (t >= 0 && t < vocab) counts[(int64_t)b * ld_counts + t] += 1;
}

// =====================================================================================
// greedy sampling from the lm_head partials + per-step bookkeeping
// =====================================================================================
__global__ void __launch_bounds__(256) sample_greedy_kernel(const float* __restrict__ amax_val,
                                                            const int32_t* __restrict__ amax_idx, int n_part,
                                                            const kr_bf16* __restrict__ table, int d,
                                                            int32_t* __restrict__ tokens_out, int32_t* __restrict__ history,
                                                            int hist_stride, const int32_t* __restrict__ prompt_len,
                                                            int32_t* __restrict__ ctx_len, int32_t* __restrict__ finished,
                                                            const int32_t* __restrict__ eos, int n_eos, int pad_id,
                                                            int ignore_eos, kr_bf16* __restrict__ x_next) {
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    // eight partials per thread requested at once (clamped indices, no branch around the loads): the lm_head leaves up to 2048
    // partials per row, and one load pair per loop iteration was eight dependent L2 round trips in a 6 us launch
    for (int i0 = tid; i0 < n_part; i0 += 256 * 8) {
        float v[8];
        int ix[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + u * 256, n_part - 1);
            v[u] = amax_val[(int64_t)b * n_part + i];
            ix[u] = amax_idx[(int64_t)b * n_part + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * 256 < n_part) better(bv, bi, v[u], ix[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        better(bv, bi, ov, oi);
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    bv = s_v[0];
    bi = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) better(bv, bi, s_v[w], s_i[w]);
    int tok = bi;
    const int was_finished = finished[b];
    const bool freeze = (ignore_eos & 2) != 0;  // bit 1: a finished sequence stops advancing (slot scheduler)
    ignore_eos &= 1;
    if (was_finished && !ignore_eos) tok = pad_id;
    const int new_ctx = ctx_len[b] + 1;  // tokens cached once the sampled token has been fed back
    __syncthreads();
    if (freeze && was_finished && !ignore_eos) {
        // the slot idles at its last position (its KV row is rewritten in place, its history stays as it is)
        // until the host admits a new request into it
        if (tid == 0) tokens_out[b] = tok;
        for (int c = tid; c < (d >> 3); c += 256) st8(x_next + (int64_t)b * d + c * 8, ld8(table + (int64_t)tok * d + c * 8));
        return;
    }
    if (tid == 0) {
        tokens_out[b] = tok;
        history[(int64_t)(new_ctx - prompt_len[b]) * hist_stride + b] = tok;  // generated-token index of this sequence
        ctx_len[b] = new_ctx;
        if (!ignore_eos && !was_finished) {
            int hit = 0;
            for (int i = 0; i < n_eos; ++i) hit |= (tok == eos[i]);
            if (hit) finished[b] = 1;
        }
    }
    for (int c = tid; c < (d >> 3); c += 256) st8(x_next + (int64_t)b * d + c * 8, ld8(table + (int64_t)tok * d + c * 8));
}

}  // namespace

extern "C" int kr_gumbel_argmax_guided(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                                       const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len,
                                       float* amax_val, int32_t* amax_idx, int n_part, int batch,
                                       const uint64_t* guide_masks, const int32_t* guide_state, int mask_words,
                                       int fallback_token, kr_stream s) {
    KR_CHECK_ARG(logits && temperature && seed && ctx_len && prompt_len && amax_val && amax_idx, "kr_gumbel_argmax: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && n_part > 0 && n_part <= 65535 && batch > 0, "kr_gumbel_argmax: bad sizes");
    KR_CHECK_ARG(guide_masks == nullptr || (guide_state != nullptr && (int64_t)mask_words * 32 >= vocab),
                 "kr_gumbel_argmax_guided: guide_state missing or mask_words * 32 < vocab");
    KR_CHECK_ARG(fallback_token >= 0 && fallback_token < vocab, "kr_gumbel_argmax_guided: fallback_token out of vocabulary");
    gumbel_argmax_kernel<<<dim3(n_part, batch), 256, 0, kr_hs(s)>>>(logits, ld_logits, vocab, temperature, seed, ctx_len, prompt_len,
                                                                    amax_val, amax_idx, guide_masks, guide_state, mask_words,
                                                                    fallback_token);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_gumbel_argmax(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                                const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len, float* amax_val,
                                int32_t* amax_idx, int n_part, int batch, kr_stream s) {
    return kr_gumbel_argmax_guided(logits, ld_logits, vocab, temperature, seed, ctx_len, prompt_len, amax_val, amax_idx, n_part,
                                   batch, nullptr, nullptr, 0, 0, s);
}

extern "C" int kr_sample_greedy(const float* amax_val, const int32_t* amax_idx, int n_part, const kr_bf16* embed_table,
                                int d, int32_t* tokens_out, int32_t* history, int hist_stride, const int32_t* prompt_len,
                                int32_t* ctx_len, int32_t* finished, const int32_t* eos, int n_eos, int pad_id,
                                int ignore_eos, kr_bf16* x_next, int batch, kr_stream s) {
    KR_CHECK_ARG(amax_val && amax_idx && embed_table && tokens_out && history && prompt_len && ctx_len && finished && x_next,
                 "kr_sample_greedy: null pointer");
    KR_CHECK_ARG(n_part > 0 && batch > 0 && (d & 7) == 0 && hist_stride >= batch && (n_eos == 0 || eos),
                 "kr_sample_greedy: bad sizes");
    sample_greedy_kernel<<<batch, 256, 0, kr_hs(s)>>>(amax_val, amax_idx, n_part, embed_table, d, tokens_out, history,
                                                      hist_stride, prompt_len, ctx_len, finished, eos, n_eos, pad_id,
                                                      ignore_eos, x_next);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_sample_threshold(const float* logits, int64_t ld_logits, int vocab, const float* temperature, const float* params,
                                   const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                                   const uint64_t* guide_masks, const int32_t* guide_state, int mask_words, const int32_t* finished,
                                   int ignore_eos, float* work, int64_t ld_work, uint32_t* threshold, int32_t* live, int batch,
                                   kr_stream s) {
    KR_CHECK_ARG(logits && temperature && params && counts && prompt_bits && finished && work && threshold && live,
                 "kr_sample_threshold: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && ld_counts >= vocab && ld_work >= vocab && (int64_t)bits_words * 32 >= vocab &&
                 batch > 0, "kr_sample_threshold: bad sizes");
    KR_CHECK_ARG(guide_masks == nullptr || (guide_state != nullptr && (int64_t)mask_words * 32 >= vocab),
                 "kr_sample_threshold: guide_state missing or mask_words * 32 < vocab");
    sample_threshold_kernel<false><<<batch, SEL_T, 0, kr_hs(s)>>>(logits, ld_logits, vocab, temperature, params, counts, ld_counts,
                                                                  prompt_bits, bits_words, guide_masks, guide_state, mask_words,
                                                                  finished, ignore_eos, work, ld_work, threshold, live, nullptr,
                                                                  nullptr, nullptr, 0, 0);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_gumbel_argmax_processed(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                                          const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len, float* amax_val,
                                          int32_t* amax_idx, int n_part, int batch, const uint64_t* guide_masks,
                                          const int32_t* guide_state, int mask_words, int fallback_token, const float* params,
                                          const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                                          const uint32_t* threshold, kr_stream s) {
    KR_CHECK_ARG(logits && temperature && seed && ctx_len && prompt_len && amax_val && amax_idx && params && counts && prompt_bits &&
                 threshold, "kr_gumbel_argmax_processed: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && ld_counts >= vocab && (int64_t)bits_words * 32 >= vocab && n_part > 0 &&
                 n_part <= 65535 && batch > 0, "kr_gumbel_argmax_processed: bad sizes");
    KR_CHECK_ARG(guide_masks == nullptr || (guide_state != nullptr && (int64_t)mask_words * 32 >= vocab),
                 "kr_gumbel_argmax_processed: guide_state missing or mask_words * 32 < vocab");
    KR_CHECK_ARG(fallback_token >= 0 && fallback_token < vocab, "kr_gumbel_argmax_processed: fallback_token out of vocabulary");
    gumbel_argmax_proc_kernel<<<dim3(n_part, batch), 256, 0, kr_hs(s)>>>(logits, ld_logits, vocab, temperature, seed, ctx_len,
                                                                         prompt_len, amax_val, amax_idx, guide_masks, guide_state,
                                                                         mask_words, fallback_token, params, counts, ld_counts,
                                                                         prompt_bits, bits_words, threshold);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

// Host-side checks of the row map of the two _rows entry points: the map itself lives on the device (kr_spec_controls_rows wrote the
// depths, kr_spec_propose / kr_spec_deal the slots), so only its shape is checked here; the kernels clamp the depth to [0, k].
#define KR_CHECK_ROW_MAP(who)                                                                                                 \
    do {                                                                                                                      \
        KR_CHECK_ARG(row_slot && depth && draft_tok, who ": null row_slot / depth / draft_tok");                              \
        KR_CHECK_ARG(slots >= 1 && slots <= batch && batch <= 32 && k >= 1 && k < 32, who ": slots=%d rows=%d k=%d "          \
                     "(1 <= slots <= rows <= 32, 1 <= k < 32)", slots, batch, k);                                             \
    } while (0)

extern "C" int kr_sample_threshold_rows(const float* logits, int64_t ld_logits, int vocab, const float* temperature, const float* params,
                                        const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                                        const uint64_t* guide_masks, const int32_t* guide_state, int mask_words,
                                        const int32_t* finished, int ignore_eos, float* work, int64_t ld_work, uint32_t* threshold,
                                        int32_t* live, int batch, const int32_t* row_slot, const int32_t* depth,
                                        const int32_t* draft_tok, int k, int slots, kr_stream s) {
    KR_CHECK_ARG(logits && temperature && params && counts && prompt_bits && finished && work && threshold && live,
                 "kr_sample_threshold_rows: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && ld_counts >= vocab && ld_work >= vocab && (int64_t)bits_words * 32 >= vocab &&
                 batch > 0, "kr_sample_threshold_rows: bad sizes");
    KR_CHECK_ARG(guide_masks == nullptr || (guide_state != nullptr && (int64_t)mask_words * 32 >= vocab),
                 "kr_sample_threshold_rows: guide_state missing or mask_words * 32 < vocab");
    KR_CHECK_ROW_MAP("kr_sample_threshold_rows");
    sample_threshold_kernel<true><<<batch, SEL_T, 0, kr_hs(s)>>>(logits, ld_logits, vocab, temperature, params, counts, ld_counts,
                                                                 prompt_bits, bits_words, guide_masks, guide_state, mask_words,
                                                                 finished, ignore_eos, work, ld_work, threshold, live, row_slot, depth,
                                                                 draft_tok, k, slots);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_gumbel_argmax_processed_rows(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                                               const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len,
                                               float* amax_val, int32_t* amax_idx, int n_part, int batch, const uint64_t* guide_masks,
                                               const int32_t* guide_state, int mask_words, int fallback_token, const float* params,
                                               const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                                               const uint32_t* threshold, const int32_t* row_slot, const int32_t* depth,
                                               const int32_t* draft_tok, int k, int slots, kr_stream s) {
    KR_CHECK_ARG(logits && temperature && seed && ctx_len && prompt_len && amax_val && amax_idx && params && counts && prompt_bits &&
                 threshold, "kr_gumbel_argmax_processed_rows: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_logits >= vocab && ld_counts >= vocab && (int64_t)bits_words * 32 >= vocab && n_part > 0 &&
                 n_part <= 65535 && batch > 0, "kr_gumbel_argmax_processed_rows: bad sizes");
    KR_CHECK_ARG(guide_masks == nullptr || (guide_state != nullptr && (int64_t)mask_words * 32 >= vocab),
                 "kr_gumbel_argmax_processed_rows: guide_state missing or mask_words * 32 < vocab");
    KR_CHECK_ARG(fallback_token >= 0 && fallback_token < vocab, "kr_gumbel_argmax_processed_rows: fallback_token out of vocabulary");
    KR_CHECK_ROW_MAP("kr_gumbel_argmax_processed_rows");
    gumbel_argmax_proc_rows_kernel<<<dim3(n_part, batch), 256, 0, kr_hs(s)>>>(
        logits, ld_logits, vocab, temperature, seed, ctx_len, prompt_len, amax_val, amax_idx, guide_masks, guide_state, mask_words,
        fallback_token, params, counts, ld_counts, prompt_bits, bits_words, threshold, row_slot, depth, draft_tok, k, slots);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_sample_count(const int32_t* tokens, const int32_t* live, int32_t* counts, int64_t ld_counts, int vocab, int batch,
                               kr_stream s) {
    KR_CHECK_ARG(tokens && live && counts, "kr_sample_count: null pointer");
    KR_CHECK_ARG(vocab > 0 && ld_counts >= vocab && batch > 0, "kr_sample_count: bad sizes");
    sample_count_kernel<<<(batch + 63) / 64, 64, 0, kr_hs(s)>>>(tokens, live, counts, ld_counts, vocab, batch);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
