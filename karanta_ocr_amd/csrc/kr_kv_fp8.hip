// fp8 (e4m3fn) KV cache, the prefill side: kr_kv_quantize converts what an admission's prefill wrote into the one-layer bf16
// scratch into a layer of the fp8 cache (include/karanta_hip.h, kr_kv8).  The decode side is the ROPE_KV8
// epilogue of the qkv launches (kr_decode.hip, kr_decode32.hip), the fp8 operands of attn_decode2_kernel (kr_attn_decode.hip) and
// the byte-sized fork (kr_kv_fork.hip); the rule they share is kv8_clamp / kv8_pack4 in kr_decode_common.h.
//   kv_quantize_kernel   a PIECE is 64 tokens of one (plan row, kv head) in one cache, as in kv_fork_kernel: 64 K rows (the last
//                        piece of a prompt holds fewer: rows at or beyond len belong to whoever decodes there) or one whole V^T
//                        block — 8192 elements, 1024 vectors of 8: a 16-byte load and an 8-byte store each, four per lane, all
//                        loads of a piece in flight before its first store.  Element index = byte index in the destination, so
//                        source and destination offsets are the same number.  The grid is capped and strides over the pieces.
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

}  // namespace

extern "C" int kr_kv_quantize(const kr_bf16* k_src, const kr_bf16* vt_src, const kr_kv8* dst, int kv_heads, int hd, int slots,
                              int s_max, const kr_kvq_plan* plan, int32_t* n_clamped, kr_stream s) {
    KR_CHECK_ARG(k_src && vt_src && dst && dst->k && dst->vt && dst->scale && plan, "kr_kv_quantize: null pointer");
    KR_CHECK_ARG(hd == 128, "kr_kv_quantize: hd=%d (the fp8 KV cache is for head_dim 128)", hd);
    KR_CHECK_ARG(kv_heads > 0 && slots > 0 && slots <= KR_KVQ_MAX_ROWS && s_max > 0 && s_max % 64 == 0,
                 "kr_kv_quantize: bad geometry (1 <= slots <= %d, s_max %% 64)", KR_KVQ_MAX_ROWS);
    KR_CHECK_ARG((((uintptr_t)k_src | (uintptr_t)vt_src) & 15) == 0 && (((uintptr_t)dst->k | (uintptr_t)dst->vt) & 7) == 0,
                 "kr_kv_quantize: the scratch must be 16-byte, the cache 8-byte aligned");
    KR_CHECK_ARG(plan->n >= 1 && plan->n <= KR_KVQ_MAX_ROWS, "kr_kv_quantize: %d plan rows (1..%d)", plan->n, KR_KVQ_MAX_ROWS);
    KvqArgs a = {};
    uint32_t seen = 0;
    int64_t total = 0;
    for (int r = 0; r < plan->n; ++r) {
        const int sl = plan->slot[r], len = plan->len[r];
        KR_CHECK_ARG(sl >= 0 && sl < slots, "kr_kv_quantize: row %d: slot %d outside [0, %d)", r, sl, slots);
        KR_CHECK_ARG(!((seen >> sl) & 1u), "kr_kv_quantize: slot %d listed twice", sl);
        KR_CHECK_ARG(len >= 1 && len <= s_max, "kr_kv_quantize: row %d: len %d outside [1, %d]", r, len, s_max);
        seen |= 1u << sl;
        a.slot[r] = sl;
        a.len[r] = len;
        a.piece0[r] = (int32_t)total;
        total += (int64_t)kv_heads * 2 * ((len + 63) / 64);
        KR_CHECK_ARG(total <= INT32_MAX, "kr_kv_quantize: too many pieces");
    }
    a.piece0[plan->n] = (int32_t)total;
    a.k_src = k_src; a.vt_src = vt_src;
    a.dst = Kv8{dst->k, dst->vt, dst->scale};
    a.n_clamped = n_clamped;
    a.head_stride = (int64_t)s_max * 128;
    a.slot_stride = a.head_stride * kv_heads;
    a.kv_heads = kv_heads; a.n = plan->n; a.total = (int32_t)total;
    const int grid = (int)(total < KVQ_MAX_BLOCKS ? total : KVQ_MAX_BLOCKS);
    kv_quantize_kernel<<<grid, KVQ_THREADS, 0, kr_hs(s)>>>(a);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
