// Attention path of the ViT and of the decoder prefill: rotary + layout prep, flash-style varlen attention (ViT full /
// decoder causal) on v_mfma bf16 with fp32 softmax.  Decode attention (q_len = 1) is in kr_attn_decode.hip.
//
// Data layout in HBM (chosen for the matrix cores, not inherited from any framework):
//   Q   : [heads, n, hd]                     rotated, bf16
//   K   : [kv_heads, rows, hd]               rotated, bf16 (decoder: the KV cache itself)
//   V^T : [kv_heads, blocks, 2, hd, 32]      V transposed inside 64-token blocks, each block as two contiguous 32-key halves
//                                            (kr_common.h, kr_vt_off; rounds 1-3: [hd, 64]), so that the
//                                            P*V MFMA operand (8 consecutive keys for one d)
//                                            is one contiguous 16-byte read per lane.
#include "kr_common.h"

namespace {

// =====================================================================================
// rotary helpers
// =====================================================================================

// x*cos + rotate_half(x)*sin on one head vector, 8 elements [c0, c0+8) per call.
// `other` holds x[(c + hd/2) mod hd]; sign = -1 for the first half, +1 for the second.
__device__ __forceinline__ bf16x8 rope8(bf16x8 x, bf16x8 other, const float* cs, const float* sn, float sign) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(x[j]) * cs[j] + sign * bf2f(other[j]) * sn[j]);
    return o;
}

// In-place rotary on [n, heads, hd] (row stride given): standalone operator.
__global__ void __launch_bounds__(256) rope_inplace_kernel(kr_bf16* __restrict__ x, const float* __restrict__ cos,
                                                           const float* __restrict__ sin, int64_t n, int heads, int hd,
                                                           int64_t row_stride) {
    const int half_chunks = hd >> 4;  // chunks of 8 in half a head
    const int64_t total = n * heads * half_chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % half_chunks);
        const int64_t t = i / half_chunks;
        const int h = (int)(t % heads);
        const int64_t tok = t / heads;
        kr_bf16* p = x + tok * row_stride + (int64_t)h * hd;
        const int d0 = c * 8, d1 = d0 + (hd >> 1);
        const bf16x8 a = ld8(p + d0), b = ld8(p + d1);
        float c0[8], s0[8], c1[8], s1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c0[j] = cos[tok * hd + d0 + j];
            s0[j] = sin[tok * hd + d0 + j];
            c1[j] = cos[tok * hd + d1 + j];
            s1[j] = sin[tok * hd + d1 + j];
        }
        st8(p + d0, rope8(a, b, c0, s0, -1.f));
        st8(p + d1, rope8(b, a, c1, s1, 1.f));
    }
}

// =====================================================================================
// prep: rotary + re-layout (+ V transpose through LDS) for 64-token blocks
// =====================================================================================
// grid = (n_blocks, ceil((q_heads + kv_heads) / PREP_G)).  Block i covers tokens blk_tok0[i] .. +blk_ntok[i] (<= 64)
// of the flattened activation `qkv` (row stride ld_qkv); they belong to one segment/sequence and
// start at a multiple of 64 inside it, so the block owns one whole V^T block.  Head slot y of the PREP_G the block takes:
//   y <  q_heads : rotate q head y            -> q_out[y][tok][hd]
//   y >= q_heads : rotate k head, copy V^T    -> k rows (k_row0[i] + j), V^T block vt_blk[i]
// Column offsets of q / k / v inside a qkv row are given in elements.
// A thread keeps the cos / sin of its (token, 8-channel chunk) in registers across the block's head slots: with one
// head per block (r1) the fp32 tables were 4x the bytes of the activations they rotate and the ViT launch ran at
// 2.5 TB/s of useful traffic (240 us per layer for 8 pages).
constexpr int PREP_G = 8;
template <int HD>
__global__ void __launch_bounds__(256) qkv_prep_kernel(const kr_bf16* __restrict__ qkv, int64_t ld_qkv, int q_off,
                                                       int k_off, int v_off, const float* __restrict__ cos,
                                                       const float* __restrict__ sin,
                                                       const int32_t* __restrict__ blk_tok0,
                                                       const int32_t* __restrict__ blk_ntok,
                                                       const int64_t* __restrict__ blk_k_row0,
                                                       const int64_t* __restrict__ blk_vt_blk, kr_bf16* __restrict__ q_out,
                                                       int64_t q_head_stride, kr_bf16* __restrict__ k_out,
                                                       int64_t k_head_stride, kr_bf16* __restrict__ vt_out,
                                                       int64_t vt_head_stride, int q_heads, int n_slots) {
    constexpr int HC = HD / 16;  // 8-element chunks in half a head
    constexpr int VT_RS = 33;    // dwords per V^T row in LDS: 32 token pairs + 1
    __shared__ unsigned vt_s[HD * VT_RS];
    const int i = blockIdx.x;
    const int y0 = blockIdx.y * PREP_G, y1 = min(y0 + PREP_G, n_slots);
    const int tok0 = blk_tok0[i], ntok = blk_ntok[i];
    const int64_t k_row0 = blk_k_row0[i];
    // ---- rotary on 64 tokens x HD, all head slots of the block
    for (int e = threadIdx.x; e < 64 * HC; e += 256) {
        const int j = e / HC, c = e - j * HC;
        if (j >= ntok) continue;
        const int64_t tok = tok0 + j;
        const int d0 = c * 8, d1 = d0 + HD / 2;
        float c0[8], s0[8], c1[8], s1[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            c0[jj] = cos[tok * HD + d0 + jj];
            s0[jj] = sin[tok * HD + d0 + jj];
            c1[jj] = cos[tok * HD + d1 + jj];
            s1[jj] = sin[tok * HD + d1 + jj];
        }
        const kr_bf16* row = qkv + tok * ld_qkv;
#pragma unroll 2
        for (int y = y0; y < y1; ++y) {
            const bool is_q = y < q_heads;
            const int head = is_q ? y : y - q_heads;
            const kr_bf16* p = row + (is_q ? q_off : k_off) + head * HD;
            kr_bf16* dst = is_q ? q_out + (int64_t)head * q_head_stride + tok * HD
                                : k_out + (int64_t)head * k_head_stride + (k_row0 + j) * HD;
            const bf16x8 a = ld8(p + d0), b = ld8(p + d1);
            st8(dst + d0, rope8(a, b, c0, s0, -1.f));
            st8(dst + d1, rope8(b, a, c1, s1, 1.f));
        }
    }
    // ---- V of the block's k-head slots: [64 tok][HD] -> LDS transposed -> V^T block [HD][64], zero padded past ntok.
    // A thread takes one 8-channel chunk of a PAIR of tokens and writes 8 whole dwords (two tokens of one channel): rows
    // of 33 dwords put the 10 / 16 chunks of a pair on distinct banks (r1 / early r2: 2-byte writes, 8-way conflicts).
    for (int y = max(y0, q_heads); y < y1; ++y) {
        const int head = y - q_heads;
        for (int e = threadIdx.x; e < 32 * (HD / 8); e += 256) {
            const int jp = e / (HD / 8), c = e - jp * (HD / 8);
            u32x4 va = (u32x4){0u, 0u, 0u, 0u}, vb = va;
            const kr_bf16* src = qkv + (int64_t)(tok0 + 2 * jp) * ld_qkv + v_off + head * HD + c * 8;
            if (2 * jp < ntok) va = *reinterpret_cast<const u32x4*>(src);
            if (2 * jp + 1 < ntok) vb = *reinterpret_cast<const u32x4*>(src + ld_qkv);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const unsigned lo = (va[jj >> 1] >> ((jj & 1) * 16)) & 0xffffu, hi = (vb[jj >> 1] >> ((jj & 1) * 16)) & 0xffffu;
                vt_s[(c * 8 + jj) * VT_RS + jp] = lo | (hi << 16);
            }
        }
        __syncthreads();
        kr_bf16* vt = vt_out + (int64_t)head * vt_head_stride + blk_vt_blk[i] * (int64_t)(HD * 64);
        for (int e = threadIdx.x; e < HD * 8; e += 256) {   // e = the 16-byte piece in MEMORY order: consecutive threads, whole lines
            const int half = e >= HD * 4 ? 1 : 0, rem = e - half * (HD * 4);
            const int d = rem >> 2, c = half * 4 + (rem & 3);
            const unsigned* r = vt_s + d * VT_RS + c * 4;
            *reinterpret_cast<u32x4*>(vt + e * 8) = (u32x4){r[0], r[1], r[2], r[3]};      // = vt + kr_vt_off(d, c * 8, HD)
        }
        __syncthreads();
    }
}

// =====================================================================================
// flash-style varlen attention, v_mfma_f32_32x32x16_bf16
// =====================================================================================
// Block = 4 waves = 128 queries of one head; each wave owns 32 queries.  Per 64-key tile:
//   S^T[key][q]  = K (A operand, LDS) x Q^T (B operand, registers)        2 x HD/16 MFMA
//   online softmax in registers: the query is on the lane, its 32 keys in 2x16 accumulator
//   registers; one cross-lane max with lane^32
//   O^T[d][q]   += V^T (A operand, LDS) x P^T (B operand = the S^T accumulators, converted in
//   place to bf16: no LDS round trip, the MFMA k-order permutation is absorbed by reading V^T
//   keys in the same order)                                               HD/32 x 4 MFMA
template <int HD>
struct AttnCfg {
    static constexpr int KS = HD / 16;               // QK^T k-steps
    static constexpr int DT = (HD + 31) / 32;        // 32-row tiles of O^T
    static constexpr int KCH = HD / 8;               // 16-byte chunks per K row
    static constexpr int KROW = (HD == 128) ? 256 : (KCH + 1) * 16;  // LDS K row bytes (hd=80: 176, conflict-free)
    static constexpr int VROW = 136;                 // LDS V^T row bytes (64 keys + 8 B pad: conflict-free b64 reads)
    static constexpr bool PRESCALE = HD == 80;       // Q carries scale * log2(e), QK^T starts at -m_ref (see the kernel)
    static constexpr int VPRE = HD == 80 ? 3 : 0;    // V^T fragment tiles requested ahead of the softmax
};

// Chunk `vi` of a V^T block in MEMORY order — the block is [2 halves][HD][32 keys] (kr_common.h, kr_vt_off), a chunk is 8 keys of
// one channel — goes to row d = channel, 16-byte piece 4 * half + (vi & 3) of the [HD][64 keys] LDS image.  The staging loads
// stay linear over the block (whole lines), only the LDS destination knows about the halves.
template <int HD>
__device__ __forceinline__ int vt_lds_piece(int vi, int vrow) {
    const int half = vi >= HD * 4 ? 1 : 0, rem = vi - half * (HD * 4);
    return (rem >> 2) * vrow + (half * 4 + (rem & 3)) * 16;
}

template <int HD>
__device__ __forceinline__ int k_lds_off(int key, int c) {
    if (HD == 128) return key * 256 + ((c ^ (key & 15)) << 4);
    return key * AttnCfg<HD>::KROW + (c << 4);
}

// NW = waves per workgroup: 4 (128 queries) or 8 (256 queries sharing one K / V^T tile image: half the tile staging per
// query).  Either way the registers (~200-254) allow two waves per SIMD — amdgpu_waves_per_eu(2) makes the compiler keep
// that — and the loop is bound by vector-ALU ISSUE slots (per 64-key tile and wave: 32 v_exp + 32 v_fma + 16 v_max3 +
// 16 v_cvt_pk + addresses, about as many cycles as the tile's 22 (hd 80) / 32 (hd 128) MFMAs hold the matrix pipe), so
// what the r2 work removed were instructions and waits, not bytes: see the comments at the staging lambdas, at ONES
// and at the permlane swap (per-segment cycle stamps: profiles/r02_attn_stamps.txt).
// Two other loop structures were built, measured and removed; 4bd05ea is the last tree that contains them.  Software
// pipelining inside each wave (scores two 32-key sub-tiles ahead of their PV) gained nothing: 1.071 against 1.068 ms
// (profiles/r03_attn_pipe_ablation.txt).  A 256-query workgroup as 4 waves x 64 queries, one wave per SIMD, was 6 %
// slower (profiles/r04_attn_q64.txt).
template <int HD, bool CAUSAL, int NW>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) attn_varlen_kernel(const kr_bf16* __restrict__ q, const kr_bf16* __restrict__ k,
                                                          const kr_bf16* __restrict__ vt, kr_bf16* __restrict__ out,
                                                          const int32_t* __restrict__ qblk,
                                                          const int32_t* __restrict__ qblk_len, int64_t nq_total,
                                                          int q_heads, int group, int64_t k_head_stride,
                                                          int64_t vt_head_stride, float scale_log2e) {
    using C = AttnCfg<HD>;
    constexpr int NTHR = NW * 64;
    // staging: the tile's 16-byte chunks, K rows then V^T rows, as ONE list dealt to the threads in whole passes
    constexpr int K_CH = 64 * C::KCH, V_CH = HD * 8, T_CH = K_CH + V_CH, PASSES = (T_CH + NTHR - 1) / NTHR;
    constexpr int VPRE = C::VPRE;  // V^T tiles prefetched across the softmax
    // two tile images [K | V^T]: tile t+1 is written while tile t is read, one barrier per tile
    constexpr int K_BYTES = 64 * C::KROW, V_BYTES = C::DT * 32 * C::VROW, IMG = K_BYTES + V_BYTES;
    __shared__ __attribute__((aligned(16))) char img_s[2 * IMG];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, lh = lane >> 5;
    // head is the fastest index of the 1-D grid: the workgroups of one query block start together (the plan lists the
    // blocks heaviest first, so a causal launch is scheduled longest-job-first over ALL heads), and with workgroups
    // dealt round-robin to the 8 XCDs each L2 holds the K / V^T of heads h = xcd (mod 8) only
    const int bi = blockIdx.x / q_heads, head = blockIdx.x - bi * q_heads, kvh = head / group;
    const int64_t q_row0 = qblk[4 * bi + 0];
    const int n_q = qblk[4 * bi + 1];
    const int64_t k_row0 = (int64_t)qblk[4 * bi + 2];
    const int64_t vt_blk0 = (int64_t)qblk[4 * bi + 3];
    const int kv_len_seg = qblk_len[2 * bi + 0];
    const int q_pos0 = qblk_len[2 * bi + 1];
    int kv_len = kv_len_seg;
    if (CAUSAL) kv_len = min(kv_len, q_pos0 + n_q);
    const int n_tiles = (kv_len + 63) >> 6;

    // The padded V^T rows (hd=80: rows 80..95, never staged) are written once: row HD to ONES, the rest to zero.  The PV
    // MFMAs compute those rows anyway, so O^T row HD comes out as sum_k P[k][q] — the softmax denominator, summed over
    // the same bf16 P the numerator uses, rescaled with O, for no instruction at all: the 32 adds per tile it replaces
    // were an eighth of the loop's vector-ALU issue slots, which — not the matrix pipe — bound this kernel.
    constexpr bool ONES = C::DT * 32 > HD;
    if (ONES) {
        for (int e = tid; e < (C::DT * 32 - HD) * C::VROW / 8; e += NTHR) {
            const unsigned v = e < 16 ? 0x3F803F80u : 0u;  // 64 keys x bf16 1.0 = the first 16 8-byte units
            reinterpret_cast<u32x2*>(img_s + K_BYTES + HD * C::VROW)[e] = (u32x2){v, v};
            reinterpret_cast<u32x2*>(img_s + IMG + K_BYTES + HD * C::VROW)[e] = (u32x2){v, v};
        }
    }

    // ---- Q fragments (B operand): lane = query, 8 d per k-step half
    int ql = wave * 32 + lq;
    const bool q_valid = ql < n_q;
    if (!q_valid) ql = n_q - 1;
    const kr_bf16* qp = q + ((int64_t)head * nq_total + q_row0 + ql) * HD + lh * 8;
    bf16x8 qf[C::KS];
#pragma unroll
    for (int s = 0; s < C::KS; ++s) qf[s] = ld8(qp + s * 16);
    // PRESCALE (hd 80, where the registers allow a second accumulator-sized tuple): Q is multiplied by scale * log2(e) ONCE
    // and rounded back to bf16, and the QK^T accumulators START at -m_ref (the lazy reference maximum, a per-query constant
    // held in `cinit`), so that S^T comes out of the matrix pipe as the exp2 argument itself: the 32 v_fma per tile that
    // applied scale and reference were a fifth of the loop's vector-ALU issue slots.  The extra rounding of Q (relative
    // 2^-9 per element) is of the size of the bf16 rounding the HF reference applies to the scores themselves.
    constexpr bool PRESCALE = C::PRESCALE;
    if (PRESCALE) {
#pragma unroll
        for (int s = 0; s < C::KS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[s][j] = f2bf(bf2f(qf[s][j]) * scale_log2e);
    }
    f32x16 cinit;   // PRESCALE: -m_run in every register of the lane (lane = query)
#pragma unroll
    for (int r = 0; r < 16; ++r) cinit[r] = 0.f;
    const int qpos = q_pos0 + wave * 32 + lq;

    const kr_bf16* kbase = k + (int64_t)kvh * k_head_stride + k_row0 * HD;
    const kr_bf16* vbase = vt + (int64_t)kvh * vt_head_stride + vt_blk0 * (int64_t)(HD * 64);

    f32x16 o[C::DT];
#pragma unroll
    for (int t = 0; t < C::DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = PRESCALE ? 0.f : -1e30f, l_run = 0.f;

    // Every thread takes exactly one chunk in every pass, in the loop ALWAYS (a tile index past the end re-loads the last
    // tile, a list index past the end the last chunk: the same bytes to the same place), and a chunk goes to LDS as two
    // 8-byte halves whether it is a K chunk (16-byte aligned) or a V^T chunk (rows of 136 B: 8-byte aligned).  No
    // lane-predicated or tile-count-dependent branch is left around a load or its wait.  With them (r1 / early r2) the
    // compiler had to assume a load into the same registers might still be in flight on the path that skipped the
    // stores, put s_waitcnt vmcnt(0) in front of the LAST load of every tile — i.e. waited for the five loads issued
    // just before it — and cycle stamps around the loop's segments showed 1500-2400 of the ~4300 cycles per tile in
    // "load issue" (profiles/r02_attn_stamps.txt).
    bf16x8 treg[PASSES];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            int idx = p * NTHR + tid;
            idx = idx < T_CH ? idx : T_CH - 1;
            const int key = idx / C::KCH, c = idx - key * C::KCH;
            int kg = t * 64 + key;
            kg = kg < kv_len_seg ? kg : kv_len_seg - 1;
            const kr_bf16* kp = kbase + (int64_t)kg * HD + c * 8;
            const kr_bf16* vp = vbase + (int64_t)t * (HD * 64) + (idx - K_CH) * 8;   // the block in MEMORY order (see vt_lds_piece)
            treg[p] = ld8(idx < K_CH ? kp : vp);
        }
    };
    auto store_tile = [&](char* img) {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            int idx = p * NTHR + tid;
            idx = idx < T_CH ? idx : T_CH - 1;
            const int key = idx / C::KCH, c = idx - key * C::KCH;
            const int off = idx < K_CH ? k_lds_off<HD>(key, c) : K_BYTES + vt_lds_piece<HD>(idx - K_CH, C::VROW);
            const u32x4 w = __builtin_bit_cast(u32x4, treg[p]);
            u32x2* dstp = reinterpret_cast<u32x2*>(img + off);
            dstp[0] = (u32x2){w[0], w[1]};
            dstp[1] = (u32x2){w[2], w[3]};
        }
    };

    if (n_tiles > 0) {
    load_tile(0);
    store_tile(img_s);
    // every load so far (Q fragments, tile 0) has landed; saying so keeps "Q may be in flight" out of the loop header
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    load_tile(n_tiles > 1 ? 1 : 0);
    __syncthreads();
    // P (bf16) and the V^T fragments of a tile
    bf16x8 vf[C::DT][4], pf[2][2];
    auto load_v = [&](const char* v_s, int dt) {
        const char* vrow = v_s + (dt * 32 + lq) * C::VROW;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int kb = f * 16 + 4 * lh;  // keys kb..kb+3 and kb+8..kb+11
            const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow + kb * 2);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + (kb + 8) * 2);
            vf[dt][f] = __builtin_bit_cast(bf16x8, (u32x4){lo[0], lo[1], hi[0], hi[1]});
        }
    };
    // ---- O^T += V^T P^T
    auto do_pv = [&](const char* v_s) {
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) {
            if (dt + VPRE < C::DT) load_v(v_s, dt + VPRE);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int ss = 0; ss < 2; ++ss)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt][sub * 2 + ss], pf[sub][ss], o[dt], 0, 0, 0);
        }
    };
    // Not here: running the second half of an 8-wave workgroup's PV one barrier late, from registers, so that a SIMD's two
    // waves are out of phase, measured 1.196-1.200 ms against 1.135-1.152 per ViT block (ViT attention r2 table;
    // 4bd05ea is the last tree with the code).
    for (int t = 0; t < n_tiles; ++t) {
        const char* k_s = img_s + (t & 1) * IMG;
        const char* v_s = k_s + K_BYTES;

        // ---- S^T = K Q^T.  All K fragments of the tile are requested before the first MFMA.
        // (r2: requesting one 32-key half at a time does not lower the register peak, and forcing 3 waves per SIMD
        // with __launch_bounds__ spills into the loop: 1.65 ms per ViT block against 1.42 on the same box.)
        // causal: a wave whose 32 queries all sit before this tile's first key has nothing to add (every score would be
        // masked: p = 0 exactly), it only takes part in the staging — waves 0 and 1 of a block skip its last tile
        // a wave without a valid query (the ragged last query block of a segment: 4900 = 19 x 256 + 36 leaves six of eight waves
        // empty) only takes part in the staging: the matrix pipe and the LDS ports go to the waves that have rows
        // (8-wave workgroups only: the same test in the 4-wave instantiation measured 5 % slower on full blocks)
        if ((!CAUSAL || t * 64 <= q_pos0 + wave * 32 + 31) && (NW == 4 || wave * 32 < n_q)) {
        bf16x8 kf[2][C::KS];
        if (HD == 128) {
            // k_lds_off(32 sub + lq, 2 ks + lh) = 8192 sub + [256 lq + ((lh ^ (lq & 15)) << 4)] ^ (ks << 5): ONE lane
            // constant, and the xor is taken after the image offset is added (bits 5-7 of IMG are 0), so that the
            // compiler cannot hoist eight per-k-step addresses out of the loop and hold them in registers it lacks
            static_assert(HD != 128 || (IMG & 0xe0) == 0, "image offset must leave the swizzle bits alone");
            const int base = (t & 1) * IMG + lq * 256 + ((lh ^ (lq & 15)) << 4);
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks) {
                const char* kp = img_s + (base ^ (ks << 5));
                kf[0][ks] = *reinterpret_cast<const bf16x8*>(kp);
                kf[1][ks] = *reinterpret_cast<const bf16x8*>(kp + 32 * 256);
            }
        } else {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int ks = 0; ks < C::KS; ++ks)
                    kf[sub][ks] = *reinterpret_cast<const bf16x8*>(k_s + k_lds_off<HD>(sub * 32 + lq, 2 * ks + lh));
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 s[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            if (PRESCALE) {
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[sub][0], qf[0], cinit, 0, 0, 0);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[sub][0], qf[0], s[sub], 0, 0, 0);
            }
#pragma unroll
            for (int ks = 1; ks < C::KS; ++ks)
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[sub][ks], qf[ks], s[sub], 0, 0, 0);
        }
        // V^T fragments of the first VPRE 32-row tiles of O^T are requested here, behind the QK^T MFMAs: their LDS
        // round trips run under the softmax instead of in front of each PV MFMA (the register file has the room since
        // the accumulators stopped being copied: 186 -> ~230 of the 256 two waves per SIMD allow)
#pragma unroll
        for (int dt = 0; dt < VPRE; ++dt) load_v(v_s, dt);
        // ---- mask, online softmax (lane = query; rows = keys).  The softmax is the VALU-bound part of this
        // kernel (PMC: vector ALU ~70 % busy, MFMA 22 %), so: masks only on tiles that need one (wave-uniform
        // test), the scale folded into one fma per score, P converted to bf16 pairwise, and a LAZY running max:
        // O and l are rescaled only when some query's max grew by more than 2^8 since its last rescale — the
        // numerator and the denominator keep using the same (stale) reference, so the quotient is unchanged and
        // bf16(P) keeps its relative precision at values up to 256.
        bool need_mask = t * 64 + 64 > kv_len_seg;
        if (CAUSAL) need_mask |= t * 64 + 63 > q_pos0 + wave * 32;
        if (need_mask) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const bool ok = key < kv_len_seg && (!CAUSAL || key <= qpos);
                    s[sub][r] = ok ? s[sub][r] : -INFINITY;
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sub][r]);
        {   // the other half-wave's maximum: one v_permlane32_swap (vector ALU) instead of an LDS round trip
            const unsigned mb = __builtin_bit_cast(unsigned, mx);
            const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
            mx = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
        }
        if (!PRESCALE) mx *= scale_log2e;  // scale > 0: max commutes with it
        if (PRESCALE) {
            // the scores ARE s - m_run already: mx is this tile's maximum relative to the reference.  The first tile moves
            // the reference onto its own maximum (o and l are still zero: nothing to scale), later tiles move it only
            // when a query's maximum grew by more than 2^8 — both rare enough to pay 48 extra subtractions there.
            const bool first = t == 0;
            if (first || __any(mx > 8.0f)) {
                const float d = first ? (mx > -INFINITY ? mx : 0.f) : fmaxf(mx, 0.f);
                m_run += d;
#pragma unroll
                for (int r = 0; r < 16; ++r) cinit[r] = -m_run;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[sub][r] -= d;
                if (!first) {
                    const float alpha = __builtin_amdgcn_exp2f(-d);
                    l_run *= alpha;
#pragma unroll
                    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                }
            }
        } else {
            const float m_new = fmaxf(m_run, mx);
            if (__any(m_new - m_run > 8.0f)) {  // first tile (m_run = -1e30), then rarely
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
            }
        }
        float psum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int h8 = 0; h8 < 2; ++h8) {
                f32x8 pv;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    pv[j] = PRESCALE ? __builtin_amdgcn_exp2f(s[sub][h8 * 8 + j])
                                     : __builtin_amdgcn_exp2f(__builtin_fmaf(s[sub][h8 * 8 + j], scale_log2e, -m_run));
                    if (!ONES) psum += pv[j];
                }
                pf[sub][h8] = __builtin_convertvector(pv, bf16x8);
            }
        l_run += psum;
        do_pv(v_s);
        }
        // tile t+1 (in registers since the previous barrier) -> the other image; it was last read during tile
        // t-1, which every wave left at the previous barrier
        store_tile(img_s + ((t + 1) & 1) * IMG);
        __syncthreads();
        load_tile(t + 2 < n_tiles ? t + 2 : n_tiles - 1);
    }
    }  // n_tiles > 0

    // ---- normalise and store: lane = query, 4 consecutive d per register quad
    float l_tot;
    if (ONES) {  // O^T row HD: tile HD/32, row HD%32 = 16 -> register 8 of the lanes lh = 0
        static_assert(!ONES || HD % 32 == 16, "ones row register");
        l_tot = __shfl(o[HD / 32][8], lq, 64);
    } else {
        l_tot = l_run + __shfl_xor(l_run, 32, 64);
    }
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    if (!q_valid) return;
    kr_bf16* op = out + (q_row0 + ql) * ((int64_t)q_heads * HD) + (int64_t)head * HD;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = dt * 32 + 8 * i + 4 * lh;
            if (d < HD) {
                bf16x4 ov;
#pragma unroll
                for (int j = 0; j < 4; ++j) ov[j] = f2bf(o[dt][4 * i + j] * inv);
                *reinterpret_cast<bf16x4*>(op + d) = ov;
            }
        }
}

}  // namespace

// =====================================================================================
// C-ABI
// =====================================================================================
static int launch_rope_inplace(kr_bf16* x, const float* cos, const float* sin, int64_t n, int heads, int hd,
                               int64_t row_stride, kr_stream s, const char* who) {
    KR_CHECK_ARG(x && cos && sin && n >= 0 && heads > 0 && hd > 0 && hd % 16 == 0 && (row_stride & 7) == 0 &&
                     row_stride >= (int64_t)heads * hd,
                 "%s: bad args", who);
    if (n == 0) return KR_OK;
    const int64_t total = n * heads * (hd >> 4);
    int grid = (int)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    rope_inplace_kernel<<<grid, 256, 0, kr_hs(s)>>>(x, cos, sin, n, heads, hd, row_stride);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_rope2d_vision(kr_bf16* x, const float* cos, const float* sin, int64_t n, int heads, int hd,
                                int64_t row_stride, kr_stream s) {
    return launch_rope_inplace(x, cos, sin, n, heads, hd, row_stride, s, "kr_rope2d_vision");
}

extern "C" int kr_mrope(kr_bf16* x, const float* cos, const float* sin, int64_t n, int heads, int hd,
                        int64_t row_stride, kr_stream s) {
    return launch_rope_inplace(x, cos, sin, n, heads, hd, row_stride, s, "kr_mrope");
}

extern "C" int kr_qkv_prep(const kr_bf16* qkv, int64_t ld_qkv, int q_off, int k_off, int v_off, const float* cos,
                           const float* sin, const int32_t* blk_tok0, const int32_t* blk_ntok,
                           const int64_t* blk_k_row0, const int64_t* blk_vt_blk, int n_blk, kr_bf16* q_out,
                           int64_t q_head_stride, kr_bf16* k_out, int64_t k_head_stride, kr_bf16* vt_out,
                           int64_t vt_head_stride, int q_heads, int kv_heads, int hd, kr_stream s) {
    KR_CHECK_ARG(qkv && cos && sin && blk_tok0 && blk_ntok && blk_k_row0 && blk_vt_blk && q_out && k_out && vt_out,
                 "kr_qkv_prep: null pointer");
    KR_CHECK_ARG(hd == 80 || hd == 128, "kr_qkv_prep: hd=%d (only 80, 128)", hd);
    KR_CHECK_ARG((ld_qkv & 7) == 0 && (q_off & 7) == 0 && (k_off & 7) == 0 && (v_off & 7) == 0, "kr_qkv_prep: alignment");
    if (n_blk == 0) return KR_OK;
    const int n_slots = q_heads + kv_heads;
    dim3 grid(n_blk, (n_slots + PREP_G - 1) / PREP_G);
    if (hd == 80)
        qkv_prep_kernel<80><<<grid, 256, 0, kr_hs(s)>>>(qkv, ld_qkv, q_off, k_off, v_off, cos, sin, blk_tok0, blk_ntok,
                                                        blk_k_row0, blk_vt_blk, q_out, q_head_stride, k_out,
                                                        k_head_stride, vt_out, vt_head_stride, q_heads, n_slots);
    else
        qkv_prep_kernel<128><<<grid, 256, 0, kr_hs(s)>>>(qkv, ld_qkv, q_off, k_off, v_off, cos, sin, blk_tok0, blk_ntok,
                                                         blk_k_row0, blk_vt_blk, q_out, q_head_stride, k_out,
                                                         k_head_stride, vt_out, vt_head_stride, q_heads, n_slots);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

static int attn_varlen_impl(const kr_bf16* q, const kr_bf16* k, const kr_bf16* vt, kr_bf16* out, const int32_t* qblk,
                            const int32_t* qblk_len, int n_qblk, int64_t nq_total, int q_heads, int kv_heads, int hd,
                            int64_t k_head_stride, int64_t vt_head_stride, float scale, int causal, int q_block, kr_stream s) {
    KR_CHECK_ARG(q && k && vt && out && qblk && qblk_len, "kr_attn_varlen: null pointer");
    KR_CHECK_ARG(hd == 80 || hd == 128, "kr_attn_varlen: hd=%d (only 80, 128)", hd);
    KR_CHECK_ARG(q_heads > 0 && kv_heads > 0 && q_heads % kv_heads == 0, "kr_attn_varlen: heads");
    KR_CHECK_ARG(q_block == 128 || q_block == 256, "kr_attn_varlen: q_block=%d (128 or 256)", q_block);
    if (n_qblk == 0) return KR_OK;
    KR_CHECK_ARG((int64_t)n_qblk * q_heads < (1ll << 31), "kr_attn_varlen: %d query blocks x %d heads", n_qblk, q_heads);
    dim3 grid((unsigned)(n_qblk * q_heads));
    const float sl = scale * 1.4426950408889634f;
    const int group = q_heads / kv_heads;
#define KR_LAUNCH_ATTN(HD_, C_, NW_)                                                                                       \
    attn_varlen_kernel<HD_, C_, NW_><<<grid, NW_ * 64, 0, kr_hs(s)>>>(q, k, vt, out, qblk, qblk_len, nq_total, q_heads, group, \
                                                                      k_head_stride, vt_head_stride, sl)
#define KR_LAUNCH_ATTN_Q(HD_, C_)                                                                                          \
    do {                                                                                                                   \
        if (q_block == 256) KR_LAUNCH_ATTN(HD_, C_, 8);                                                                    \
        else KR_LAUNCH_ATTN(HD_, C_, 4);                                                                                   \
    } while (0)
    if (hd == 80) {
        if (causal) KR_LAUNCH_ATTN_Q(80, true); else KR_LAUNCH_ATTN_Q(80, false);
    } else {
        if (causal) KR_LAUNCH_ATTN_Q(128, true); else KR_LAUNCH_ATTN_Q(128, false);
    }
#undef KR_LAUNCH_ATTN_Q
#undef KR_LAUNCH_ATTN
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_attn_varlen(const kr_bf16* q, const kr_bf16* k, const kr_bf16* vt, kr_bf16* out, const int32_t* qblk,
                              const int32_t* qblk_len, int n_qblk, int64_t nq_total, int q_heads, int kv_heads, int hd,
                              int64_t k_head_stride, int64_t vt_head_stride, float scale, int causal, kr_stream s) {
    return attn_varlen_impl(q, k, vt, out, qblk, qblk_len, n_qblk, nq_total, q_heads, kv_heads, hd, k_head_stride, vt_head_stride,
                            scale, causal, 128, s);
}

extern "C" int kr_attn_varlen_q(const kr_bf16* q, const kr_bf16* k, const kr_bf16* vt, kr_bf16* out, const int32_t* qblk,
                                const int32_t* qblk_len, int n_qblk, int64_t nq_total, int q_heads, int kv_heads, int hd,
                                int64_t k_head_stride, int64_t vt_head_stride, float scale, int causal, int q_block, kr_stream s) {
    return attn_varlen_impl(q, k, vt, out, qblk, qblk_len, n_qblk, nq_total, q_heads, kv_heads, hd, k_head_stride, vt_head_stride,
                            scale, causal, q_block, s);
}
