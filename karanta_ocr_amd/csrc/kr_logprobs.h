// The arithmetic of the log-probability launches, shared by kr_logprobs_topk (kr_guide.hip: one record per row of a plain step)
// and kr_logprobs_topk_rows (kr_spec.hip: one record per token a speculative step emitted).  ONE statement of the slice
// partition, the max / sum-exp fold order and the tie rule, so that a record does not depend on which launch wrote it:
//   logprob_partial_body   one vocabulary slice of one logits row (LDS resident): max, sum exp, top-k by k rounds of block argmax
//   logprob_merge_body     one logits row: log-sum-exp over the slices, log-prob of the token, merged top-k
// Both are called by every thread of a 256-thread workgroup, with arguments that are uniform over the workgroup.
#pragma once
#include "kr_common.h"

constexpr int LP_MAX_K = 20;       // OpenAI's top_logprobs bound
constexpr int LP_SLICE = 4096;     // floats of one vocabulary slice held in LDS
constexpr size_t LP_MERGE_LDS = 160 * 1024 - 1024;   // largest candidate table of the merge (bytes of dynamic LDS)

__device__ __forceinline__ void better_lp(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

__device__ __forceinline__ void block_argmax(float& bv, int& bi, float* s_v, int* s_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        better_lp(bv, bi, ov, oi);
    }
    __syncthreads();                 // s_v / s_i of the previous round have been read by everyone
    if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
    __syncthreads();
    bv = s_v[0]; bi = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) better_lp(bv, bi, s_v[w], s_i[w]);
}

// Slice p of n_part of the logits row `row_logits` [vocab].  pv / pi: the k partial values and ids of (row, p); pms: its
// (max, sum exp(v - max)).
__device__ __forceinline__ void logprob_partial_body(const float* __restrict__ row_logits, int vocab, int k, int p, int n_part,
                                                     float* __restrict__ pv, int32_t* __restrict__ pi, float* __restrict__ pms) {
    __shared__ float sl[LP_SLICE];
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int tid = threadIdx.x;
    const int per = (vocab + n_part - 1) / n_part;          // <= LP_SLICE (checked by the launcher)
    const int i0 = p * per, n = max(0, min(vocab, i0 + per) - i0);
    const float* row = row_logits + i0;
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 256) { const float v = row[i]; sl[i] = v; mx = fmaxf(mx, v); }
    int dummy = 0;
    block_argmax(mx, dummy, s_v, s_i);                       // (value only; the index is unused)
    float se = 0.f;
    for (int i = tid; i < n; i += 256) se += expf(sl[i] - mx);
    se = wave_sum(se);
    __shared__ float s_se[4];
    if ((tid & 63) == 0) s_se[tid >> 6] = se;
    __syncthreads();
    if (tid == 0) {
        pms[0] = mx;
        pms[1] = n > 0 ? s_se[0] + s_se[1] + s_se[2] + s_se[3] : 0.f;
    }
    for (int r = 0; r < k; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 256) {
            const float v = sl[i];
            if (v != -INFINITY) better_lp(bv, bi, v, i);     // retired elements never come back
        }
        block_argmax(bv, bi, s_v, s_i);
        if (tid == 0) {
            pv[r] = bv;
            pi[r] = bi == 0x7fffffff ? 0x7fffffff : i0 + bi;
        }
        if (bi != 0x7fffffff && tid == (bi & 255)) sl[bi] = -INFINITY;   // the owner of that element retires it
    }
}

// The record of one logits row from its partials: pv / pi [n_part][k], pms [n_part][2].  lp[0] = log p(tok) (-inf for a token
// outside the vocabulary), lp[1 + r] / ix[r] = the r-th most probable token (ties: lowest id).  cand: n_part * k values, then as
// many indices, of dynamic LDS.
__device__ __forceinline__ void logprob_merge_body(const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                   const float* __restrict__ pms, int n_part, int k,
                                                   const float* __restrict__ row_logits, int vocab, int tok,
                                                   float* __restrict__ lp, int32_t* __restrict__ ix, float* cand) {
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int tid = threadIdx.x, nc = n_part * k;
    int* cidx = reinterpret_cast<int*>(cand + nc);
    for (int i = tid; i < nc; i += 256) { cand[i] = pv[i]; cidx[i] = pi[i]; }
    float mx = -INFINITY;
    for (int i = tid; i < n_part; i += 256) mx = fmaxf(mx, pms[i * 2]);
    int dummy = 0;
    block_argmax(mx, dummy, s_v, s_i);
    float se = 0.f;
    for (int i = tid; i < n_part; i += 256) {
        const float m = pms[i * 2], sv = pms[i * 2 + 1];
        if (sv > 0.f) se += sv * expf(m - mx);
    }
    se = wave_sum(se);
    __shared__ float s_se[4];
    if ((tid & 63) == 0) s_se[tid >> 6] = se;
    __syncthreads();
    const float lse = mx + logf(s_se[0] + s_se[1] + s_se[2] + s_se[3]);
    if (tid == 0) lp[0] = (tok >= 0 && tok < vocab) ? row_logits[tok] - lse : -INFINITY;
    for (int r = 0; r < k; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff, bslot = -1;
        for (int i = tid; i < nc; i += 256) {
            const float v = cand[i];
            const int id = cidx[i];
            if (v != -INFINITY && (v > bv || (v == bv && id < bi))) { bv = v; bi = id; bslot = i; }
        }
        // block argmax on (value, token id); the winning candidate slot is found again by its unique token id
        block_argmax(bv, bi, s_v, s_i);
        if (tid == 0) { lp[1 + r] = bv - lse; ix[r] = bi; }
        if (bslot >= 0 && cidx[bslot] == bi && cand[bslot] == bv) cand[bslot] = -INFINITY;
        __syncthreads();
    }
}

// What kr_logprobs_topk and kr_logprobs_topk_rows refuse alike: k, the slice bound and the merge's candidate table.  0: fine.
// Host only; `who` names the entry point in the message.
inline int logprob_check_sizes(const char* who, int vocab, int k, int k_stride, int n_part) {
    KR_CHECK_ARG(k >= 0 && k <= LP_MAX_K && k <= k_stride, "%s: k must be in 0..%d and <= k_stride", who, LP_MAX_K);
    KR_CHECK_ARG(n_part > 0 && n_part <= 1024 && (vocab + n_part - 1) / n_part <= LP_SLICE,
                 "%s: a vocabulary slice (vocab / n_part) must fit %d floats", who, LP_SLICE);
    // the merge's candidate table (n_part * k values and ids) next to its 48 static bytes: checked before anything is launched
    KR_CHECK_ARG((size_t)n_part * (k > 0 ? k : 1) * 8 <= LP_MERGE_LDS, "%s: n_part * k candidates exceed the LDS", who);
    return KR_OK;
}
