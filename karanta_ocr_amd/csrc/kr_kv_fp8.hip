// fp8 (e4m3fn) KV cache, the prefill side: kr_kv_quantize converts what an admission's prefill wrote into the one-layer bf16
// scratch into a layer of the fp8 cache (include/karanta_hip.h, kr_kv8).  The decode side is the ROPE_KV8
// epilogue of the qkv launches (kr_decode.hip, kr_decode32.hip), the fp8 operands of attn_decode2_kernel (kr_attn_decode.hip) and
// the byte-sized fork (kr_kv_fork.hip); the rule they share is kv8_clamp / kv8_pack4 in kr_decode_common.h.
//   kv_quantize_kernel   a PIECE is 64 tokens of one (plan row, kv head) in one cache, as in kv_fork_kernel: 64 K rows (the last
//                        piece of a prompt holds fewer: rows at or beyond len belong to whoever decodes there) or one whole V^T
//                        block — 8192 elements, 1024 vectors of 8: a 16-byte load and an 8-byte store each, four per lane, all
//                        loads of a piece in flight before its first store.  Element index = byte index in the destination, so
//                        source and destination offsets are the same number.  The grid is capped and strides over the pieces.
// kr_kv_absmax (--calculate-kv-scales) reads the same scratch right before kr_kv_quantize and writes the layer's row of the scale
// table: scale = max(amax / range, FLT_MIN) per (K or V, kv head), amax over the finite elements of the plan's rows.
//   kv_absmax_kernel     the quantiser's pieces and capped, strided grid; a piece's (up to) four 16-byte loads per lane are all in
//                        flight before the first compare.  |x| of a bf16 is its low 15 bits, which order as an unsigned integer;
//                        NaN / inf (>= 0x7F80) count as 0.  Of a V^T block's vectors only the keys below len are used: a vector is
//                        8 consecutive keys of one channel in one 32-key half, so it is whole, cut at len, or skipped (not loaded).
//                        Wave reduction by shuffles, LDS atomic max per (K | V, head), then at most one vector atomic max per
//                        workgroup and (K | V, head) into `work`.
//   kv_absmax_finish_kernel   a SECOND tiny launch behind it, not a last-workgroup ticket: the kernel boundary orders every
//                        workgroup's atomics before the read and needs no release / acquire protocol between workgroups of one
//                        launch (an in-launch hand-off costs an agent-scope fence per workgroup and is about as long as the
//                        boundary it saves; this runs once per layer of ONE admission).  2 * kv_heads lanes: read work[t], write
//                        scale_out[t] (one IEEE f32 division), store 0 back into work[t].
#include <float.h>

#include "kr_decode_common.h"

namespace {

constexpr int KVQ_THREADS = 256;
constexpr int KVQ_MAX_BLOCKS = 2048;
constexpr int KVQ_PIECE_VECS = 128 * 64 / 8;      // vectors of 8 elements in a piece (hd 128)

struct KvqArgs {
    const kr_bf16* k_src; const kr_bf16* vt_src;
    Kv8 dst;
    int32_t* n_clamped;
    int64_t head_stride, slot_stride;             // elements: s_max * 128, kv_heads * that
    int32_t kv_heads, n, total;
    int32_t piece0[KR_KVQ_MAX_ROWS + 1];          // first piece of plan row r (prefix sums)
    int32_t slot[KR_KVQ_MAX_ROWS];
    int32_t len[KR_KVQ_MAX_ROWS];
};

__global__ void __launch_bounds__(KVQ_THREADS) kv_quantize_kernel(const KvqArgs a) {
    __shared__ int clamped_s;
    if (threadIdx.x == 0) clamped_s = 0;
    __syncthreads();
    int clamped = 0;
    for (int w = blockIdx.x; w < a.total; w += gridDim.x) {
        int r = 0;
        while (r + 1 < a.n && w >= a.piece0[r + 1]) ++r;
        const int len = a.len[r];
        const int nblk = (len + 63) >> 6;
        int p = w - a.piece0[r];
        const int blk = p % nblk;
        p /= nblk;
        const int is_v = p & 1;
        const int h = p >> 1;                     // < kv_heads: piece0 counts kv_heads * 2 * nblk pieces per row
        const int vecs = is_v ? KVQ_PIECE_VECS : min(64, len - blk * 64) * 16;
        const int64_t off = (int64_t)a.slot[r] * a.slot_stride + (int64_t)h * a.head_stride + (int64_t)blk * (128 * 64);
        const kr_bf16* src = (is_v ? a.vt_src : a.k_src) + off;
        uint8_t* dst = (is_v ? a.dst.vt : a.dst.k) + off;
        const float sc = a.dst.scale[is_v * a.kv_heads + h];
        bf16x8 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = (int)threadIdx.x + i * KVQ_THREADS;
            if (v < vecs) x[i] = ld8(src + v * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = (int)threadIdx.x + i * KVQ_THREADS;
            if (v < vecs) {
                u32x2 o;
                o[0] = kv8_pack4(bf2f(x[i][0]), bf2f(x[i][1]), bf2f(x[i][2]), bf2f(x[i][3]), sc, clamped);
                o[1] = kv8_pack4(bf2f(x[i][4]), bf2f(x[i][5]), bf2f(x[i][6]), bf2f(x[i][7]), sc, clamped);
                *reinterpret_cast<u32x2*>(dst + v * 8) = o;
            }
        }
    }
    if (a.n_clamped == nullptr) return;           // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) clamped += __shfl_xor(clamped, o, 64);
    if ((threadIdx.x & 63) == 0 && clamped) atomicAdd(&clamped_s, clamped);     // LDS
    __syncthreads();
    if (threadIdx.x == 0 && clamped_s) atomicAdd(a.n_clamped, clamped_s);
}

constexpr int KVA_MAX_BLOCKS = 512;               // two workgroups per CU; 1024 and 2048 measured slower (10.4 -> 12.5 us)
constexpr int KVA_MAX_HEADS = 64;

struct KvaArgs {
    const kr_bf16* k_src; const kr_bf16* vt_src;
    uint32_t* work;
    int64_t head_stride, slot_stride;
    int32_t kv_heads, n, total;
    int32_t piece0[KR_KVQ_MAX_ROWS + 1];
    int32_t slot[KR_KVQ_MAX_ROWS];
    int32_t len[KR_KVQ_MAX_ROWS];
};

// max |x| over the first `keep` (1..8) bf16 of a vector, as bf16 bits; a NaN or an inf counts as 0
__device__ __forceinline__ unsigned kva_vec_amax(u32x4 x, int keep) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned b = (x[i >> 1] >> ((i & 1) * 16)) & 0x7FFFu;
        m = max(m, (i < keep && b < 0x7F80u) ? b : 0u);
    }
    return m;
}

__global__ void __launch_bounds__(KVQ_THREADS) kv_absmax_kernel(const KvaArgs a) {
    __shared__ unsigned amax_s[2 * KVA_MAX_HEADS];
    if ((int)threadIdx.x < 2 * a.kv_heads) amax_s[threadIdx.x] = 0;
    __syncthreads();
    for (int w = blockIdx.x; w < a.total; w += gridDim.x) {
        int r = 0;
        while (r + 1 < a.n && w >= a.piece0[r + 1]) ++r;
        const int len = a.len[r];
        const int nblk = (len + 63) >> 6;
        int p = w - a.piece0[r];
        const int blk = p % nblk;
        p /= nblk;
        const int is_v = p & 1;
        const int h = p >> 1;
        const int rows = min(64, len - blk * 64);          // K rows, or keys of the V^T block, below len: 1..64
        const int64_t off = (int64_t)a.slot[r] * a.slot_stride + (int64_t)h * a.head_stride + (int64_t)blk * (128 * 64);
        const kr_bf16* src = (is_v ? a.vt_src : a.k_src) + off;
        u32x4 x[4];
        int keep[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = (int)threadIdx.x + i * KVQ_THREADS;
            // K: vector v is 8 channels of row v / 16.  V^T [2][128][32]: keys (v >> 9) * 32 + (v & 3) * 8 .. + 7 of one channel
            keep[i] = is_v ? min(8, rows - ((v >> 9) * 32 + (v & 3) * 8)) : (v < rows * 16 ? 8 : 0);
            if (keep[i] > 0) x[i] = *reinterpret_cast<const u32x4*>(src + v * 8);
        }
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (keep[i] > 0) m = max(m, kva_vec_amax(x[i], keep[i]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&amax_s[is_v * a.kv_heads + h], m);     // LDS
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * a.kv_heads && amax_s[threadIdx.x])
        __hip_atomic_fetch_max(a.work + threadIdx.x, amax_s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(2 * KVA_MAX_HEADS) kv_absmax_finish_kernel(uint32_t* work, float* scale_out, int kv_heads,
                                                                             float k_range, float v_range) {
    const int t = (int)threadIdx.x;
    if (t >= 2 * kv_heads) return;
    const unsigned b = work[t];
    work[t] = 0;
    const float q = __uint_as_float(b << 16) / (t < kv_heads ? k_range : v_range);
    scale_out[t] = b == 0 ? 1.0f : fmaxf(q, FLT_MIN);
}

// The host side the two entry points share: what they refuse of the geometry, the scratch and the plan, and the plan as the kernels
// walk it (a.piece0 / slot / len / n / total, the strides, the sources).  `who` is the entry point's name in the messages.
template <class Args>
int kvq_fill(Args& a, const char* who, const kr_bf16* k_src, const kr_bf16* vt_src, int kv_heads, int hd, int slots, int s_max,
             const kr_kvq_plan* plan) {
    KR_CHECK_ARG(hd == 128, "%s: hd=%d (the fp8 KV cache is for head_dim 128)", who, hd);
    KR_CHECK_ARG(kv_heads > 0 && slots > 0 && slots <= KR_KVQ_MAX_ROWS && s_max > 0 && s_max % 64 == 0,
                 "%s: bad geometry (1 <= slots <= %d, s_max %% 64)", who, KR_KVQ_MAX_ROWS);
    KR_CHECK_ARG((((uintptr_t)k_src | (uintptr_t)vt_src) & 15) == 0, "%s: the scratch must be 16-byte aligned", who);
    KR_CHECK_ARG(plan->n >= 1 && plan->n <= KR_KVQ_MAX_ROWS, "%s: %d plan rows (1..%d)", who, plan->n, KR_KVQ_MAX_ROWS);
    uint32_t seen = 0;
    int64_t total = 0;
    for (int r = 0; r < plan->n; ++r) {
        const int sl = plan->slot[r], len = plan->len[r];
        KR_CHECK_ARG(sl >= 0 && sl < slots, "%s: row %d: slot %d outside [0, %d)", who, r, sl, slots);
        KR_CHECK_ARG(!((seen >> sl) & 1u), "%s: slot %d listed twice", who, sl);
        KR_CHECK_ARG(len >= 1 && len <= s_max, "%s: row %d: len %d outside [1, %d]", who, r, len, s_max);
        seen |= 1u << sl;
        a.slot[r] = sl;
        a.len[r] = len;
        a.piece0[r] = (int32_t)total;
        total += (int64_t)kv_heads * 2 * ((len + 63) / 64);
        KR_CHECK_ARG(total <= INT32_MAX, "%s: too many pieces", who);
    }
    a.piece0[plan->n] = (int32_t)total;
    a.k_src = k_src; a.vt_src = vt_src;
    a.head_stride = (int64_t)s_max * 128;
    a.slot_stride = a.head_stride * kv_heads;
    a.kv_heads = kv_heads; a.n = plan->n; a.total = (int32_t)total;
    return KR_OK;
}

}  // namespace

extern "C" int kr_kv_absmax(const kr_bf16* k_src, const kr_bf16* vt_src, int kv_heads, int hd, int slots, int s_max,
                            const kr_kvq_plan* plan, float k_range, float v_range, float* scale_out, uint32_t* work, kr_stream s) {
    KR_CHECK_ARG(k_src && vt_src && plan && scale_out && work, "kr_kv_absmax: null pointer");
    KR_CHECK_ARG(kv_heads <= KVA_MAX_HEADS, "kr_kv_absmax: bad geometry (%d kv heads, at most %d)", kv_heads, KVA_MAX_HEADS);
    KR_CHECK_ARG(k_range > 0.0f && k_range <= FLT_MAX && v_range > 0.0f && v_range <= FLT_MAX,
                 "kr_kv_absmax: the ranges must be finite and positive (k_range %g, v_range %g)", (double)k_range, (double)v_range);
    KR_CHECK_ARG((((uintptr_t)scale_out | (uintptr_t)work) & 3) == 0, "kr_kv_absmax: scale_out and work must be 4-byte aligned");
    KvaArgs a = {};
    if (int rc = kvq_fill(a, "kr_kv_absmax", k_src, vt_src, kv_heads, hd, slots, s_max, plan)) return rc;
    a.work = work;
    const int grid = a.total < KVA_MAX_BLOCKS ? a.total : KVA_MAX_BLOCKS;
    kv_absmax_kernel<<<grid, KVQ_THREADS, 0, kr_hs(s)>>>(a);
    KR_CHECK_LAUNCH();
    kv_absmax_finish_kernel<<<1, 2 * KVA_MAX_HEADS, 0, kr_hs(s)>>>(work, scale_out, kv_heads, k_range, v_range);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_kv_quantize(const kr_bf16* k_src, const kr_bf16* vt_src, const kr_kv8* dst, int kv_heads, int hd, int slots,
                              int s_max, const kr_kvq_plan* plan, int32_t* n_clamped, kr_stream s) {
    KR_CHECK_ARG(k_src && vt_src && dst && dst->k && dst->vt && dst->scale && plan, "kr_kv_quantize: null pointer");
    KR_CHECK_ARG((((uintptr_t)dst->k | (uintptr_t)dst->vt) & 7) == 0, "kr_kv_quantize: the cache must be 8-byte aligned");
    KvqArgs a = {};
    if (int rc = kvq_fill(a, "kr_kv_quantize", k_src, vt_src, kv_heads, hd, slots, s_max, plan)) return rc;
    a.dst = Kv8{dst->k, dst->vt, dst->scale};
    a.n_clamped = n_clamped;
    const int grid = a.total < KVQ_MAX_BLOCKS ? a.total : KVQ_MAX_BLOCKS;
    kv_quantize_kernel<<<grid, KVQ_THREADS, 0, kr_hs(s)>>>(a);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
