// Fork of a prefilled KV-cache slot: the prompt rows of a source slot copied to other slots, so that several sequences start
// from one ViT pass and one prefill (n > 1 of a request, a repeated page); DESIGN.md §5i.
//   kv_fork_kernel   one launch; a PIECE is 64 tokens of one (layer, KV head) in one cache: 64 K rows (64 x hd bf16, the last
//                    piece of a span may hold fewer rows) or one whole V^T block ([2][hd][32] bf16) — hd x 128 bytes either
//                    way, 16 KB at hd 128.  A workgroup takes whole pieces: 16 B per lane, up to four loads per lane in flight
//                    before the first store, and what it loaded is stored to EVERY destination of the group, so the source is
//                    read once however many children there are.  The grid is capped and strides over the pieces.
//                    kr_kv_fork8 (the fp8 cache): the same kernel over one-byte elements, a piece is hd x 64 bytes.
// The plan (kr_fork_plan, host memory) is validated and flattened on the host into the kernel's arguments: no device table,
// no copy, no allocation.  All offsets are 64-bit: a layer of the 2B cache at 32 slots x 16384 rows is 268 M elements.
#include "kr_common.h"

namespace {

constexpr int FORK_THREADS = 256;
constexpr int FORK_INFLIGHT = 4;          // 16-byte loads per lane before the first store: 16 KB per workgroup pass
constexpr int FORK_MAX_BLOCKS = 2048;

struct ForkArgs {
    uint4* kc;
    uint4* vc;
    int64_t k_sl, k_ss, k_sh;             // strides in 16-byte units
    int64_t v_sl, v_ss, v_sh;
    int32_t kv_heads, piece_vecs, row_vecs, n_groups;
    int32_t total;                        // pieces of all groups
    // all 32-bit: a workgroup reads them with scalar loads from the kernel arguments
    int32_t piece0[KR_FORK_MAX_GROUPS + 1];   // first piece of group g (prefix sums)
    int32_t n_tokens[KR_FORK_MAX_GROUPS];
    int32_t dst0[KR_FORK_MAX_GROUPS + 1];     // group g's destinations: dst[dst0[g] .. dst0[g + 1])
    int32_t src[KR_FORK_MAX_GROUPS];
    int32_t dst[KR_FORK_MAX_SLOTS];
};

constexpr int FORK_PASS = FORK_THREADS * FORK_INFLIGHT;   // 16-byte vectors a workgroup moves per pass

__global__ void __launch_bounds__(FORK_THREADS) kv_fork_kernel(const ForkArgs a) {
    for (int w = blockIdx.x; w < a.total; w += gridDim.x) {
        int g = 0;
        while (g + 1 < a.n_groups && w >= a.piece0[g + 1]) ++g;
        const int n_tok = a.n_tokens[g];
        const int nblk = (n_tok + 63) >> 6;
        int r = w - a.piece0[g];
        const int blk = r % nblk;
        r /= nblk;
        const int is_v = r & 1;
        r >>= 1;
        const int h = r % a.kv_heads;
        const int l = r / a.kv_heads;
        // a K piece ends with the span (rows >= n_tokens belong to the destination); a V^T block is copied whole
        const int vecs = is_v ? a.piece_vecs : min(64, n_tok - blk * 64) * a.row_vecs;
        uint4* base = is_v ? a.vc : a.kc;
        const int64_t s_slot = is_v ? a.v_ss : a.k_ss;
        const int64_t off = (is_v ? (int64_t)l * a.v_sl + (int64_t)h * a.v_sh : (int64_t)l * a.k_sl + (int64_t)h * a.k_sh)
                            + (int64_t)blk * a.piece_vecs;
        const uint4* src = base + (int64_t)a.src[g] * s_slot + off;
        const int d0 = a.dst0[g], d1 = a.dst0[g + 1];
        for (int v0 = 0; v0 < vecs; v0 += FORK_PASS) {
            const int v = v0 + (int)threadIdx.x;
            const uint4* sp = src + v;
            if (v0 + FORK_PASS <= vecs) {
                // a whole pass (every pass of a full piece at hd 128): four unguarded loads, then the stores of every destination
                const uint4 x0 = sp[0], x1 = sp[FORK_THREADS], x2 = sp[2 * FORK_THREADS], x3 = sp[3 * FORK_THREADS];
#pragma unroll 1
                for (int d = d0; d < d1; ++d) {
                    uint4* q = base + (int64_t)a.dst[d] * s_slot + off + v;
                    q[0] = x0;
                    q[FORK_THREADS] = x1;
                    q[2 * FORK_THREADS] = x2;
                    q[3 * FORK_THREADS] = x3;
                }
            } else {
                // the tail of a span's last K piece (or a piece that is no multiple of the pass): the same, lane by lane guarded
                const bool p0 = v < vecs, p1 = v + FORK_THREADS < vecs, p2 = v + 2 * FORK_THREADS < vecs,
                           p3 = v + 3 * FORK_THREADS < vecs;
                uint4 x0 = {}, x1 = {}, x2 = {}, x3 = {};
                if (p0) x0 = sp[0];
                if (p1) x1 = sp[FORK_THREADS];
                if (p2) x2 = sp[2 * FORK_THREADS];
                if (p3) x3 = sp[3 * FORK_THREADS];
#pragma unroll 1
                for (int d = d0; d < d1; ++d) {
                    uint4* q = base + (int64_t)a.dst[d] * s_slot + off + v;
                    if (p0) q[0] = x0;
                    if (p1) q[FORK_THREADS] = x1;
                    if (p2) q[2 * FORK_THREADS] = x2;
                    if (p3) q[3 * FORK_THREADS] = x3;
                }
            }
        }
    }
}

}  // namespace

// EPV = elements per 16-byte vector: 8 (kr_kv_fork, bf16) or 16 (kr_kv_fork8, the fp8 cache's bytes).  The kernel moves vectors and
// does not know the difference.
static int fork_impl(void* kcache, void* vtcache, int64_t k_layer_stride, int64_t k_slot_stride, int64_t k_head_stride,
                     int64_t vt_layer_stride, int64_t vt_slot_stride, int64_t vt_head_stride, int layers, int kv_heads,
                     int hd, int slots, int s_max, const kr_fork_plan* plan, const int EPV, kr_stream s) {
    KR_CHECK_ARG(kcache && vtcache && plan, "kr_kv_fork: null pointer");
    KR_CHECK_ARG(layers > 0 && kv_heads > 0 && hd > 0 && hd % EPV == 0 && slots > 0 && slots <= KR_FORK_MAX_SLOTS && s_max > 0
                 && s_max % 64 == 0, "kr_kv_fork: bad geometry (hd %% %d, 1 <= slots <= %d, s_max %% 64)", EPV, KR_FORK_MAX_SLOTS);
    KR_CHECK_ARG(((uintptr_t)kcache | (uintptr_t)vtcache) % 16 == 0, "kr_kv_fork: caches must be 16-byte aligned");
    const int64_t span = (int64_t)s_max * hd;     // elements of one (layer, slot, head) in either cache
    const int64_t strides[6] = {k_layer_stride, k_slot_stride, k_head_stride, vt_layer_stride, vt_slot_stride, vt_head_stride};
    for (int i = 0; i < 6; ++i) KR_CHECK_ARG(strides[i] > 0 && strides[i] % EPV == 0, "kr_kv_fork: strides must be multiples of %d elements", EPV);
    KR_CHECK_ARG(k_head_stride >= span && vt_head_stride >= span, "kr_kv_fork: head stride below s_max x hd");
    KR_CHECK_ARG(k_slot_stride >= (int64_t)kv_heads * k_head_stride && vt_slot_stride >= (int64_t)kv_heads * vt_head_stride,
                 "kr_kv_fork: slot stride below kv_heads x head stride");
    KR_CHECK_ARG(k_layer_stride >= (int64_t)slots * k_slot_stride && vt_layer_stride >= (int64_t)slots * vt_slot_stride,
                 "kr_kv_fork: layer stride below slots x slot stride");
    KR_CHECK_ARG(plan->n_groups >= 1 && plan->n_groups <= KR_FORK_MAX_GROUPS, "kr_kv_fork: %d groups (1..%d)", plan->n_groups,
                 KR_FORK_MAX_GROUPS);
    ForkArgs a = {};
    uint32_t is_src = 0, is_dst = 0;
    for (int g = 0; g < plan->n_groups; ++g) {
        const int sj = plan->groups[g].src;
        KR_CHECK_ARG(sj >= 0 && sj < slots, "kr_kv_fork: group %d: source slot %d outside [0, %d)", g, sj, slots);
        is_src |= 1u << sj;
    }
    int64_t total = 0;
    int nd = 0;
    for (int g = 0; g < plan->n_groups; ++g) {
        const kr_fork_group& gr = plan->groups[g];
        KR_CHECK_ARG(gr.n_tokens >= 1 && gr.n_tokens <= s_max, "kr_kv_fork: group %d: n_tokens %d outside [1, %d]", g, gr.n_tokens, s_max);
        KR_CHECK_ARG(gr.n_dst >= 1 && gr.n_dst <= KR_FORK_MAX_SLOTS, "kr_kv_fork: group %d: %d destinations", g, gr.n_dst);
        a.src[g] = gr.src;
        a.n_tokens[g] = gr.n_tokens;
        a.piece0[g] = (int32_t)total;
        a.dst0[g] = nd;
        for (int i = 0; i < gr.n_dst; ++i) {
            const int dj = gr.dst[i];
            KR_CHECK_ARG(dj >= 0 && dj < slots, "kr_kv_fork: group %d: destination slot %d outside [0, %d)", g, dj, slots);
            KR_CHECK_ARG(!((is_src >> dj) & 1u), "kr_kv_fork: slot %d is a destination and a source", dj);
            KR_CHECK_ARG(!((is_dst >> dj) & 1u), "kr_kv_fork: destination slot %d listed twice", dj);
            is_dst |= 1u << dj;
            a.dst[nd++] = dj;      // distinct slots below KR_FORK_MAX_SLOTS: nd stays within dst[]
        }
        total += (int64_t)layers * kv_heads * 2 * ((gr.n_tokens + 63) / 64);
        KR_CHECK_ARG(total <= INT32_MAX, "kr_kv_fork: too many pieces");
    }
    a.piece0[plan->n_groups] = (int32_t)total;
    a.dst0[plan->n_groups] = nd;
    a.kc = reinterpret_cast<uint4*>(kcache);
    a.vc = reinterpret_cast<uint4*>(vtcache);
    a.k_sl = k_layer_stride / EPV, a.k_ss = k_slot_stride / EPV, a.k_sh = k_head_stride / EPV;
    a.v_sl = vt_layer_stride / EPV, a.v_ss = vt_slot_stride / EPV, a.v_sh = vt_head_stride / EPV;
    a.kv_heads = kv_heads;
    a.piece_vecs = hd * 64 / EPV;         // 64 tokens x hd elements / 16 B
    a.row_vecs = hd / EPV;
    a.n_groups = plan->n_groups;
    a.total = (int32_t)total;
    const int grid = (int)(total < FORK_MAX_BLOCKS ? total : FORK_MAX_BLOCKS);
    kv_fork_kernel<<<grid, FORK_THREADS, 0, kr_hs(s)>>>(a);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_kv_fork(kr_bf16* kcache, kr_bf16* vtcache, int64_t k_layer_stride, int64_t k_slot_stride, int64_t k_head_stride,
                          int64_t vt_layer_stride, int64_t vt_slot_stride, int64_t vt_head_stride, int layers, int kv_heads,
                          int hd, int slots, int s_max, const kr_fork_plan* plan, kr_stream s) {
    return fork_impl(kcache, vtcache, k_layer_stride, k_slot_stride, k_head_stride, vt_layer_stride, vt_slot_stride, vt_head_stride,
                     layers, kv_heads, hd, slots, s_max, plan, 8, s);
}

extern "C" int kr_kv_fork8(uint8_t* kcache, uint8_t* vtcache, int64_t k_layer_stride, int64_t k_slot_stride, int64_t k_head_stride,
                           int64_t vt_layer_stride, int64_t vt_slot_stride, int64_t vt_head_stride, int layers, int kv_heads,
                           int hd, int slots, int s_max, const kr_fork_plan* plan, kr_stream s) {
    return fork_impl(kcache, vtcache, k_layer_stride, k_slot_stride, k_head_stride, vt_layer_stride, vt_slot_stride, vt_head_stride,
                     layers, kv_heads, hd, slots, s_max, plan, 16, s);
}
