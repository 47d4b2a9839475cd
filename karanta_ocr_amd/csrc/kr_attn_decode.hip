// Decode attention (one query token per live sequence); the ViT and prefill attention are in kr_attention.hip.
//   attn_decode2_kernel  split-KV MFMA attention: one (o[128], m, l) record per (sequence, head, split).  The engine passes
//                        out == NULL and merges with a launch of its own; the in-launch merge by the last-arriving
//                        workgroup of each (sequence, kv head) is an experiment build (-DKR_EXPERIMENTS).
//   attn_merge_kernel    the merge launch: row-major rows (kr_attn_decode_merge) or the packed XP layout of 17..32-row
//                        batches (kr_attn_decode_merge32).
// The closing section holds the first-generation decode operators, which the engine does not launch.
#include "kr_decode_common.h"

namespace {

// grid = (n_split, kv_heads, batch); WAVES waves; wave `part` = split*WAVES + wave walks 32-key units
// part, part + WAVES*n_split, ...   Layouts as in kr_attention.hip (K rows, V^T 64-key blocks).
#ifndef KR_ATTN_DEC_LD        // -DKR_ATTN_DEC_LD=ld8: default-policy K / V^T loads (A/B builds, csrc/tools/build_variant.py)
#define KR_ATTN_DEC_LD ld8_nt
#endif
// ROWS (kr_attn_decode_rows, the speculative step): blockIdx.z is a ROW — q, ctx_len, finished and the records are the row's, the
// cache is the one of slot row_slot[row]; the new pointer sits at the tail of the arguments, past the preloaded ones.
// KV8 (kr_attn_decode_slots_kv8 / _rows_kv8): the cache holds e4m3 codes, one byte per element, same layout; kv_scale = [2][kv_heads]
// sits at the tail of the arguments too.  A unit is 4 KiB of K rows + 4 KiB of V^T, every load 16 bytes per lane:
//   K    load j of key tile kt: lane (fr, fg) reads channels 64j + 16fg .. +15 of its key row — the four lane groups cover 64
//        contiguous bytes of each of 16 rows, the two loads of a tile a whole 128-byte row.  The 16 bytes are TWO k-steps: k-step
//        2j + h pairs K[key][64j + 16fg + 8h + e] with Q[g][the same channel], e = 0..7 — the Q fragments are loaded in that
//        permutation (a dot product does not care).
//   V^T  load i: lane (fr, fg) reads keys 16 (fg & 1) .. +15 of channel 32i + 16 (fg >> 1) + fr: one instruction = 1 KiB of
//        contiguous memory.  Its low 8 bytes belong to channel tile 2i in lane groups 0, 1 and to tile 2i + 1 in groups 2, 3; one
//        v_permlane32_swap per register (low halves of the upper 32 lanes <-> high halves of the lower 32) leaves tile 2i in the
//        low and tile 2i + 1 in the high registers of every lane, lane group fg holding keys 8 pi(fg) .. +7 with pi = (0, 2, 1, 3).
//        K row fr of tile kt is therefore key 8 pi(fr >> 2) + 4kt + (fr & 3): P comes out of the S accumulators in V's key order.
//   The codes are converted to bf16 in registers (exact) right before their matrix instruction; K's scale is folded into
//   scale_log2e, V's multiplies the wave's O once.
template <bool KV8> struct KvElem { using T = kr_bf16; };
template <> struct KvElem<true> { using T = uint8_t; };

template <int WAVES, bool ROWS = false, bool KV8 = false>
__global__ void __launch_bounds__(WAVES * 64) attn_decode2_kernel(const kr_bf16* __restrict__ q, const typename KvElem<KV8>::T* __restrict__ kcache,
                                                                  const typename KvElem<KV8>::T* __restrict__ vtcache,
                                                                  const int32_t* __restrict__ ctx_len,
                                                                  const int32_t* __restrict__ finished, int heads, int kv_heads,
                                                                  int group, int n_split, int s_max, float scale_log2e,
                                                                  kr_bf16* __restrict__ out, float* __restrict__ ws,
                                                                  int* __restrict__ counters, int ws_bytes,
                                                                  const int32_t* __restrict__ row_slot,
                                                                  const float* __restrict__ kv_scale) {
    // argument order: everything the first loads need sits in the 16 preloaded dwords (kernarg preload), so the
    // scalar load of ctx_len[b] leaves at once instead of behind a load of the argument tail
    constexpr int HD = 128, DT = HD / 16, REC = HD + 4;
    __shared__ __attribute__((aligned(16))) float o_s[WAVES][16][HD];
    __shared__ float m_s[WAVES][16], l_s[WAVES][16];
    __shared__ int last_s;
    // the wave index in a scalar register: the branch on this part's unit count below is a scalar branch
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    // group (= heads / kv_heads) and n_split (= gridDim.x) are arguments: a runtime division and a read of the dispatch
    // packet would both sit in front of the first loads
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int n_part = n_split * WAVES, part = split * WAVES + wave;
    const int ctx = ctx_len[b] + 1;
    // a sequence that has finished (EOS flag set by the sampling launch, or retired by the host): nothing downstream reads its rows
    // any more — its workgroups leave without touching its cache (a server's idle slots: ~18 % of the rows in the corpus run)
    if (finished != nullptr && finished[b] != 0) return;

    const int g = fr < group ? fr : 0;
    // MFMA k-step i pairs K[key][32i + 8fg + j] with Q[g][32i + 8fg + j]: per load instruction the
    // four lane groups cover 64 contiguous bytes of each of 16 key rows
    const kr_bf16* qp = q + ((int64_t)b * heads + kvh * group + g) * HD + fg * (KV8 ? 16 : 8);
    bf16x8 qf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qf[i] = ld8(qp + (KV8 ? (i >> 1) * 64 + (i & 1) * 8 : i * 32));
    const int64_t kv_base = (int64_t)(ROWS ? row_slot[b] : b) * kv_heads + kvh;
    const typename KvElem<KV8>::T* kc = kcache + kv_base * s_max * HD;
    const typename KvElem<KV8>::T* vc = vtcache + kv_base * (int64_t)(s_max >> 6) * (HD * 64);
    // KV8: lane group fg of a key tile / of P stands for keys 8 pi(fg) .. +7
    const int pfg = KV8 ? ((fg & 1) << 1) | (fg >> 1) : fg;
    float sl2 = scale_log2e;
    if constexpr (KV8) sl2 *= kv_scale[kvh];

    f32x4 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) o[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;
    // unit = 32 keys (half a V^T block); wave `part` takes units part, part + n_part, ...: 64 parts leave one unit — one
    // memory round trip — per wave up to 2048 keys; a page runs from 1.4k to 2.5k keys (46 .. 78 units), so past 2048 keys
    // parts 0 .. nu - 65 carry two units, both requested before the first is folded
    const int nu = (ctx + 31) >> 5;
    // KV8: a unit is half the registers — K [kt][j] and V^T [i] of 16 bytes each
    constexpr int KI = KV8 ? 2 : 4, VI = KV8 ? 4 : DT;
    bf16x8 kf[2][KI], vf[VI], kf2[2][KI], vf2[VI];
    auto load_k = [&](int u, bf16x8 (&kk)[2][KI]) {
        const int key0 = u * 32;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            if constexpr (KV8) {
                const char* kp = reinterpret_cast<const char*>(kc) +
                                 (int64_t)(key0 + 8 * ((((fr >> 2) & 1) << 1) | (fr >> 3)) + 4 * kt + (fr & 3)) * HD + fg * 16;
#pragma unroll
                for (int j = 0; j < 2; ++j) kk[kt][j] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kp + j * 64));
            } else {
                const kr_bf16* kp = kc + (int64_t)(key0 + 8 * (fr >> 2) + 4 * kt + (fr & 3)) * HD + fg * 8;
#pragma unroll
                for (int i = 0; i < 4; ++i) kk[kt][i] = KR_ATTN_DEC_LD(kp + i * 32);
            }
        }
    };
    auto load_v = [&](int u, bf16x8 (&vv)[VI]) {
        if constexpr (KV8) {
            const char* vp = reinterpret_cast<const char*>(vc) + (int64_t)(u >> 1) * (HD * 64) + (u & 1) * (HD * 32) +
                             ((fg >> 1) * 16 + fr) * 32 + (fg & 1) * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) vv[i] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vp + i * (32 * 32)));
        } else {
            // the unit's half of its V^T block is contiguous ([2][HD][32]: kr_common.h): 16 channel rows x 64 B per instruction = 1 KiB of
            // whole lines (rounds 1-3: [HD][64], half of every line — 4.0 against 6.5 TB/s for this shape, profiles/r04_halfline_read.txt)
            const kr_bf16* vp = vc + (int64_t)(u >> 1) * (HD * 64) + (u & 1) * (HD * 32) + fg * 8;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) vv[dt] = KR_ATTN_DEC_LD(vp + (dt * 16 + fr) * 32);
        }
    };
    auto load_unit = [&](int u, bf16x8 (&kk)[2][KI], bf16x8 (&vv)[VI]) {
        load_k(u, kk);
        load_v(u, vv);
    };
    // fold one unit into the running (m, l, o): QK^T needs the unit's K registers only, PV its V^T registers — in straight-line
    // code each waits (counted vmcnt) for exactly the loads it reads, younger loads stay in flight
    auto fold_unit = [&](int u, const bf16x8 (&kk)[2][KI], const bf16x8 (&vv)[VI]) {
        const int key0 = u * 32;
        f32x4 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bf16x8 ka;
                if constexpr (KV8) {
                    const u32x4 w = __builtin_bit_cast(u32x4, kk[kt][i >> 1]);
                    ka = kv8_to_bf16x8(w[2 * (i & 1)], w[2 * (i & 1) + 1]);
                } else {
                    ka = kk[kt][i];
                }
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[i], s[kt], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = key0 + 8 * pfg + 4 * kt + r;
                const float v = key < ctx ? s[kt][r] * sl2 : -INFINITY;
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        bf16x8 pf;
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const __bf16 pb = f2bf(__builtin_amdgcn_exp2f(s[kt][r] - m_new));
                psum += bf2f(pb);
                pf[kt * 4 + r] = pb;
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
            if constexpr (!KV8) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vv[dt], pf, o[dt], 0, 0, 0);
        }
        if constexpr (KV8) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // load i after the swap of the halves: channel tile 2i in the low registers, 2i + 1 in the high ones
                const u32x4 w = __builtin_bit_cast(u32x4, vv[i]);
                const auto s0 = __builtin_amdgcn_permlane32_swap(w[0], w[2], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(w[1], w[3], false, false);
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    o[2 * i + h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kv8_to_bf16x8(s0[h], s1[h]), pf, o[2 * i + h], 0, 0, 0);
            }
        }
    };
    // One wave-uniform branch on this part's unit count; the bodies for one and two units are branch-free from their first load on.
    // (A load group under `if (un < nu)` in front of the fold makes the fold's waits count the group that MAY be in flight: with
    // two units the first QK^T then waited for the second unit's 16 loads as well — DESIGN §5, lesson 1.)  Every body folds
    // the units part, part + n_part, ... in that order with the same instructions: the records are the same bits.
    const int u0 = part, u1 = part + n_part;
    if (u1 + n_part < nu) {             // three or more units: unit u + n_part is requested before unit u is folded
        int u = u0;
        load_unit(u, kf, vf);
        while (u < nu) {
            const int un = u + n_part;
            if (un < nu) load_unit(un, kf2, vf2);
            fold_unit(u, kf, vf);
            if (un < nu) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int i = 0; i < KI; ++i) kf[kt][i] = kf2[kt][i];
#pragma unroll
                for (int dt = 0; dt < VI; ++dt) vf[dt] = vf2[dt];
            }
            u = un;
        }
    } else if (u1 < nu) {               // two units (2049 .. 4096 keys at 64 parts): all 32 loads in flight at once, both K first —
        load_k(u0, kf);                 // 0.2 us per launch against K, V^T, K, V^T at 2176 .. 2485 keys (profiles/r07_attn_ctx_sweep.txt)
        load_k(u1, kf2);
        load_v(u0, vf);
        load_v(u1, vf2);
        __builtin_amdgcn_sched_barrier(0);      // every load leaves before the first wait: the scheduler would sink V^T below QK^T
        fold_unit(u0, kf, vf);
        __builtin_amdgcn_sched_barrier(0);      // the folds one after the other, each product behind the wait for its own operand
        fold_unit(u1, kf2, vf2);
    } else if (u0 < nu) {               // one unit
        load_unit(u0, kf, vf);
        __builtin_amdgcn_sched_barrier(0);
        fold_unit(u0, kf, vf);
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    // ---- merge the waves through LDS
    if constexpr (KV8) {
        const float vs = kv_scale[kv_heads + kvh];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= vs;
    }
    if (fr < group) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(&o_s[wave][fr][dt * 16 + fg * 4]) = o[dt];
        if (fg == 0) {
            m_s[wave][fr] = m_run;
            l_s[wave][fr] = l_run;
        }
    }
    __syncthreads();
    // element t < group * 32 = 4 consecutive channels d4 .. d4+3 of head gg: one 16-byte piece of the record
    // [o[128], m, l, 0, 0] (REC floats) of this (sequence, head, split); a thread owns elements tid, tid + NTHR, ...
    constexpr int NTHR = WAVES * 64, IT = (16 * 32 + NTHR - 1) / NTHR;
    const int bh0 = b * heads + kvh * group;
    const int nq = group * (HD / 4);
    f32x4 acc4[IT];
    float mm[IT], ll[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int t = tid + it * NTHR, gg = t >> 5, d4 = (t & 31) << 2;
        acc4[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mm[it] = -1e30f;
        ll[it] = 0.f;
        if (t < nq) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) mm[it] = fmaxf(mm[it], m_s[w][gg]);
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const float sc = __builtin_amdgcn_exp2f(m_s[w][gg] - mm[it]);
                const f32x4 ow = *reinterpret_cast<const f32x4*>(&o_s[w][gg][d4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc4[it][j] += ow[j] * sc;
                ll[it] += l_s[w][gg] * sc;
            }
        }
    }
    auto store_out = [&](int t, const f32x4& a, float l) {
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        bf16x4 ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = f2bf(a[j] * inv);
        *reinterpret_cast<bf16x4*>(out + (int64_t)(bh0 + (t >> 5)) * HD + ((t & 31) << 2)) = ov;
    };
    auto rec_of = [&](int t) { return ((int64_t)(bh0 + (t >> 5)) * n_split) * REC; };   // first record of element t's head (floats)
    if (n_split == 1 && out) {
#pragma unroll
        for (int it = 0; it < IT; ++it)
            if (tid + it * NTHR < nq) store_out(tid + it * NTHR, acc4[it], ll[it]);
        return;
    }
    if (!KR_EXP || !out) {  // a later launch (kr_attn_decode_merge) merges the partials: plain stores
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int t = tid + it * NTHR, d4 = (t & 31) << 2;
            if (t < nq) {
                float* w = ws + rec_of(t) + (int64_t)split * REC;
                *reinterpret_cast<f32x4*>(w + d4) = acc4[it];
                if (d4 == 0) *reinterpret_cast<f32x4*>(w + HD) = (f32x4){mm[it], ll[it], 0.f, 0.f};
            }
        }
        return;
    }
    // ---- in-launch merge by the last-arriving split of this (sequence, kv head).  Hand-off in the form the guide
    // measures (MI355X_MICROARCH.md, visibility, "Valid forms" row 1): every payload byte leaves as a 16-byte sc1
    // (write-through) store, every storing wave drains its stores (vmcnt(0)) before the workgroup barrier, ONE lane
    // then adds to the group's counter; the workgroup whose add returns n_split - 1 is the last one and reads all
    // records with 16-byte sc1 loads (never a plain load of these bytes), all requested at once.  Nobody waits:
    // the other workgroups just leave.  Correct for any placement of the splits on XCDs / CUs.
    // (Measured r2: 1.2200 ms per step against 1.2033 with the separate merge launch — the hand-off costs what the
    // launch costs; kept for the ABI and as the tested example of the protocol.  CAUTION before reusing it: the same form
    // with 64 KB payloads per workgroup — a split-K GEMM fix-up, profiles/r02_decode_experiments.txt — let the last arriver
    // read a few 16-byte pieces too early in 1 of ~10^6; nothing on the default path depends on an in-launch hand-off.)
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(ws, 0, ws_bytes, 0x00020000);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int t = tid + it * NTHR, d4 = (t & 31) << 2;
        if (t < nq) {
            const int off = (int)((rec_of(t) + (int64_t)split * REC + d4) * 4);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc4[it]), rsrc, off, 0, 16);
            if (d4 == 0)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4){mm[it], ll[it], 0.f, 0.f}), rsrc,
                                                       (int)((rec_of(t) + (int64_t)split * REC + HD) * 4), 0, 16);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's record stores have been acknowledged
    __syncthreads();
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(counters + b * kv_heads + kvh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = (old == n_split - 1);
        if (old == n_split - 1) __hip_atomic_store(counters + b * kv_heads + kvh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_s) return;
    constexpr int MAXS = 16;
    for (int it = 0; it < IT; ++it) {
        const int t = tid + it * NTHR, d4 = (t & 31) << 2;
        if (t >= nq) continue;
        u32x4 ro[MAXS], rm[MAXS];
#pragma unroll
        for (int p = 0; p < MAXS; ++p) {
            if (p < n_split) {
                ro[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((rec_of(t) + (int64_t)p * REC + d4) * 4), 0, 16);
                rm[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((rec_of(t) + (int64_t)p * REC + HD) * 4), 0, 16);
            }
        }
        float mt = -1e30f;
#pragma unroll
        for (int p = 0; p < MAXS; ++p)
            if (p < n_split) mt = fmaxf(mt, __builtin_bit_cast(f32x4, rm[p])[0]);
        f32x4 at = {0.f, 0.f, 0.f, 0.f};
        float lt = 0.f;
#pragma unroll
        for (int p = 0; p < MAXS; ++p) {
            if (p < n_split) {
                const f32x4 mlp = __builtin_bit_cast(f32x4, rm[p]), op = __builtin_bit_cast(f32x4, ro[p]);
                const float sc = __builtin_amdgcn_exp2f(mlp[0] - mt);
#pragma unroll
                for (int j = 0; j < 4; ++j) at[j] += op[j] * sc;
                lt += mlp[1] * sc;
            }
        }
        store_out(t, at, lt);
    }
}

// Merge of the split-KV partials as a launch of its own: one 128-thread workgroup per (sequence, head).
// (Cheaper end-to-end than replicating the merge in every o_proj workgroup's prologue: measured.)
// NS > 0: all n_split records are requested at once (one memory round trip instead of two dependent loops).
template <int NS>
__global__ void __launch_bounds__(128) attn_merge_kernel(const float* __restrict__ ws, kr_bf16* __restrict__ out, int n_split, int heads_xp,
                                                         int xp16) {
    // heads_xp > 0: out is the XP layout of a 17..32-row batch (row = sequence, column = head * 128 + d), heads_xp = heads;
    // with xp16 > 0 the XP16 layout of a <= 16-row batch at xp16 row slots (kr_common.h: the x_packed operand of the narrow
    // o_proj launch)
    constexpr int HD = 128, REC = HD + 4;
    const int bh = blockIdx.x, d = threadIdx.x;
    float acc = 0.f, ll = 0.f;
    if constexpr (NS > 0) {
        const float* w = ws + (int64_t)bh * NS * REC;
        float m[NS], l[NS], o[NS];
#pragma unroll
        for (int p = 0; p < NS; ++p) {
            m[p] = w[p * REC + HD];
            l[p] = w[p * REC + HD + 1];
            o[p] = w[p * REC + d];
        }
        float mm = -1e30f;
#pragma unroll
        for (int p = 0; p < NS; ++p) mm = fmaxf(mm, m[p]);
#pragma unroll
        for (int p = 0; p < NS; ++p) {
            const float sc = __builtin_amdgcn_exp2f(m[p] - mm);
            acc += o[p] * sc;
            ll += l[p] * sc;
        }
    } else {
        const float* w = ws + (int64_t)bh * n_split * REC;
        float mm = -1e30f;
        for (int p = 0; p < n_split; ++p) mm = fmaxf(mm, w[p * REC + HD]);
        for (int p = 0; p < n_split; ++p) {
            const float sc = __builtin_amdgcn_exp2f(w[p * REC + HD] - mm);
            acc += w[p * REC + d] * sc;
            ll += w[p * REC + HD + 1] * sc;
        }
    }
    const kr_bf16 r = __builtin_bit_cast(kr_bf16, f2bf(ll > 0.f ? acc / ll : 0.f));
    if (heads_xp > 0) {
        const int b = bh / heads_xp, hh = bh - b * heads_xp;
        *reinterpret_cast<kr_bf16*>(reinterpret_cast<char*>(out) + (xp16 ? kr_xp16_byte_offset(b, hh * HD + d, xp16) : kr_xp_byte_offset(b, hh * HD + d))) = r;
    } else {
        out[(int64_t)bh * HD + d] = r;
    }
}

}  // namespace

template <bool ROWS = false, bool KV8 = false>
static int attn_decode_impl(const kr_bf16* q, const typename KvElem<KV8>::T* kcache, const typename KvElem<KV8>::T* vtcache,
                            const int32_t* ctx_len, const int32_t* finished, kr_bf16* out, float* workspace, int32_t* counters,
                            int batch, int heads, int kv_heads, int hd, int s_max, int n_split, float scale, kr_stream s,
                            const int32_t* row_slot = nullptr, const float* kv_scale = nullptr) {
    KR_CHECK_ARG(q && kcache && vtcache && ctx_len && (out || workspace), "kr_attn_decode_fused: null pointer");
    KR_CHECK_ARG(hd == 128, "kr_attn_decode_fused: hd=%d (only 128)", hd);
    KR_CHECK_ARG(heads % kv_heads == 0 && heads / kv_heads <= 16, "kr_attn_decode_fused: GQA group must be <= 16");
    KR_CHECK_ARG(batch > 0 && n_split > 0 && s_max % 64 == 0, "kr_attn_decode_fused: bad sizes");
    KR_CHECK_ARG(KR_EXP || !out || n_split == 1,
                 "kr_attn_decode_fused: the in-launch merge (out != NULL with n_split > 1) is an experiment build (-DKR_EXPERIMENTS); "
                 "pass out = NULL and run kr_attn_decode_merge");
    KR_CHECK_ARG(!out || n_split <= 16, "kr_attn_decode_fused: the in-launch merge takes at most 16 splits");
    KR_CHECK_ARG(!out || n_split == 1 || (workspace && counters), "kr_attn_decode_fused: split needs workspace + counters");
    KR_CHECK_ARG(workspace || n_split == 1, "kr_attn_decode_fused: the split partials need a workspace");
    // Workgroup shape: n_split x WAVES parts of 32-key units: 64 parts give a wave ONE unit (one memory round trip) up to
    // 2048 keys; the page contexts (1.4k .. 2.5k keys = 46 .. 78 units) run past that, the first nu - 64 parts then hold two.  r2 chain timings (B = 8, ctx 1906, launch + dependent-launch gap):
    // 8 splits x 8 waves (128 workgroups) 7.8 us; 16 splits x 4 waves (256 workgroups, every CU loads) 5.8 us;
    // 6 x 8 (two units per wave) 12.7 us.  Hence: up to 8 splits 8 waves, up to 16 splits 4 waves, beyond 2 waves
    // (KARANTA_ATTN_WAVES = 2 / 4 / 8 overrides for A/B runs).
    static const int waves_env = [] { const char* e = getenv("KARANTA_ATTN_WAVES"); return e ? atoi(e) : 0; }();
    const int waves = waves_env ? waves_env : (n_split <= 8 ? 8 : n_split <= 16 ? 4 : 2);
    KR_CHECK_ARG(waves == 2 || waves == 4 || waves == 8, "kr_attn_decode_fused: KARANTA_ATTN_WAVES=%d (2, 4 or 8)", waves);
    const int64_t ws_bytes = (int64_t)batch * heads * n_split * (hd + 4) * 4;
    KR_CHECK_ARG(ws_bytes < ((int64_t)1 << 31), "kr_attn_decode_fused: workspace of %lld bytes", (long long)ws_bytes);
    const dim3 grid(n_split, kv_heads, batch);
    const float sl2 = scale * 1.4426950408889634f;
    const int group = heads / kv_heads;
    if (waves == 8)
        attn_decode2_kernel<8, ROWS, KV8><<<grid, 512, 0, kr_hs(s)>>>(q, kcache, vtcache, ctx_len, finished, heads, kv_heads, group, n_split, s_max,
                                                                      sl2, out, workspace, counters, (int)ws_bytes, row_slot, kv_scale);
    else if (waves == 4)
        attn_decode2_kernel<4, ROWS, KV8><<<grid, 256, 0, kr_hs(s)>>>(q, kcache, vtcache, ctx_len, finished, heads, kv_heads, group, n_split, s_max,
                                                                      sl2, out, workspace, counters, (int)ws_bytes, row_slot, kv_scale);
    else
        attn_decode2_kernel<2, ROWS, KV8><<<grid, 128, 0, kr_hs(s)>>>(q, kcache, vtcache, ctx_len, finished, heads, kv_heads, group, n_split, s_max,
                                                                      sl2, out, workspace, counters, (int)ws_bytes, row_slot, kv_scale);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_attn_decode_fused(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache, const int32_t* ctx_len,
                                    kr_bf16* out, float* workspace, int32_t* counters, int batch, int heads, int kv_heads,
                                    int hd, int s_max, int n_split, float scale, kr_stream s) {
    return attn_decode_impl(q, kcache, vtcache, ctx_len, nullptr, out, workspace, counters, batch, heads, kv_heads, hd, s_max, n_split, scale, s);
}

extern "C" int kr_attn_decode_slots(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache, const int32_t* ctx_len,
                                    const int32_t* finished, float* workspace, int batch, int heads, int kv_heads, int hd, int s_max,
                                    int n_split, float scale, kr_stream s) {
    KR_CHECK_ARG(finished && workspace, "kr_attn_decode_slots: null pointer");
    return attn_decode_impl(q, kcache, vtcache, ctx_len, finished, nullptr, workspace, nullptr, batch, heads, kv_heads, hd, s_max, n_split, scale, s);
}

extern "C" int kr_attn_decode_rows(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache, const int32_t* ctx_len,
                                   const int32_t* finished, const int32_t* row_slot, float* workspace, int rows, int heads, int kv_heads,
                                   int hd, int s_max, int n_split, float scale, kr_stream s) {
    KR_CHECK_ARG(finished && workspace && row_slot, "kr_attn_decode_rows: null pointer");
    return attn_decode_impl<true>(q, kcache, vtcache, ctx_len, finished, nullptr, workspace, nullptr, rows, heads, kv_heads, hd, s_max, n_split,
                                  scale, s, row_slot);
}

extern "C" int kr_attn_decode_slots_kv8(const kr_bf16* q, const kr_kv8* kv, const int32_t* ctx_len, const int32_t* finished,
                                        float* workspace, int batch, int heads, int kv_heads, int hd, int s_max, int n_split,
                                        float scale, kr_stream s) {
    KR_CHECK_ARG(finished && workspace && kv && kv->k && kv->vt && kv->scale, "kr_attn_decode_slots_kv8: null pointer");
    KR_CHECK_ARG((((uintptr_t)kv->k | (uintptr_t)kv->vt) & 15) == 0, "kr_attn_decode_slots_kv8: the cache must be 16-byte aligned");
    return attn_decode_impl<false, true>(q, kv->k, kv->vt, ctx_len, finished, nullptr, workspace, nullptr, batch, heads, kv_heads, hd,
                                         s_max, n_split, scale, s, nullptr, kv->scale);
}

extern "C" int kr_attn_decode_rows_kv8(const kr_bf16* q, const kr_kv8* kv, const int32_t* ctx_len, const int32_t* finished,
                                       const int32_t* row_slot, float* workspace, int rows, int heads, int kv_heads, int hd,
                                       int s_max, int n_split, float scale, kr_stream s) {
    KR_CHECK_ARG(finished && workspace && row_slot && kv && kv->k && kv->vt && kv->scale, "kr_attn_decode_rows_kv8: null pointer");
    KR_CHECK_ARG((((uintptr_t)kv->k | (uintptr_t)kv->vt) & 15) == 0, "kr_attn_decode_rows_kv8: the cache must be 16-byte aligned");
    return attn_decode_impl<true, true>(q, kv->k, kv->vt, ctx_len, finished, nullptr, workspace, nullptr, rows, heads, kv_heads, hd,
                                        s_max, n_split, scale, s, row_slot, kv->scale);
}

static int merge_impl(const float* workspace, kr_bf16* out, int batch, int heads, int hd, int n_split, int xp, kr_stream s) {
    KR_CHECK_ARG(workspace && out && batch > 0 && heads > 0 && n_split > 0, "kr_attn_decode_merge: bad args");
    KR_CHECK_ARG(hd == 128, "kr_attn_decode_merge: hd=%d (only 128)", hd);
    // xp: 0 row-major rows, 1 the XP layout (<= 32 rows), 2 the XP16 layout (<= 16 rows)
    KR_CHECK_ARG(!xp || (batch <= (xp == 2 ? 16 : 32) && ((uintptr_t)out & 15) == 0), "kr_attn_decode_merge%d: batch=%d (<= %d)",
                 xp == 2 ? 16 : 32, batch, xp == 2 ? 16 : 32);
    const int hx = xp ? heads : 0, xp16 = xp == 2 ? kr_xp16_rows(batch) : 0;
    switch (n_split) {
        case 4: attn_merge_kernel<4><<<batch * heads, 128, 0, kr_hs(s)>>>(workspace, out, n_split, hx, xp16); break;
        case 8: attn_merge_kernel<8><<<batch * heads, 128, 0, kr_hs(s)>>>(workspace, out, n_split, hx, xp16); break;
        case 16: attn_merge_kernel<16><<<batch * heads, 128, 0, kr_hs(s)>>>(workspace, out, n_split, hx, xp16); break;
        case 32: attn_merge_kernel<32><<<batch * heads, 128, 0, kr_hs(s)>>>(workspace, out, n_split, hx, xp16); break;
        default: attn_merge_kernel<0><<<batch * heads, 128, 0, kr_hs(s)>>>(workspace, out, n_split, hx, xp16);
    }
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_attn_decode_merge(const float* workspace, kr_bf16* out, int batch, int heads, int hd, int n_split,
                                    kr_stream s) {
    return merge_impl(workspace, out, batch, heads, hd, n_split, 0, s);
}

extern "C" int kr_attn_decode_merge32(const float* workspace, kr_bf16* out_xp, int batch, int heads, int hd, int n_split,
                                      kr_stream s) {
    return merge_impl(workspace, out_xp, batch, heads, hd, n_split, 1, s);
}

extern "C" int kr_attn_decode_merge16(const float* workspace, kr_bf16* out_xp16, int batch, int heads, int hd, int n_split,
                                      kr_stream s) {
    return merge_impl(workspace, out_xp16, batch, heads, hd, n_split, 2, s);
}

// =====================================================================================
// First-generation decode operators: kr_decode_qkv_prep, kr_attn_decode_gqa, kr_kv_append
// =====================================================================================
// The engine does not launch any of these: its decode step rotates and appends in the qkv linear's epilogue (kr_decode.hip)
// and attends with attn_decode2_kernel above.  They stay exported and tested as standalone operators.
namespace {

// =====================================================================================
// decode: rotary + KV append for one new token per sequence
// =====================================================================================
__global__ void __launch_bounds__(256) decode_qkv_prep_kernel(const kr_bf16* __restrict__ qkv,
                                                              const float* __restrict__ inv_freq,
                                                              const int32_t* __restrict__ ctx_len,
                                                              const int32_t* __restrict__ rope_delta,
                                                              kr_bf16* __restrict__ q_out, kr_bf16* __restrict__ kcache,
                                                              kr_bf16* __restrict__ vtcache, int heads, int kv_heads,
                                                              int hd, int layer, int batch, int s_max) {
    const int b = blockIdx.x;
    const int pos = ctx_len[b];
    const float rp = (float)(pos + rope_delta[b]);
    const int half = hd >> 1;
    const int qkv_dim = (heads + 2 * kv_heads) * hd;
    const kr_bf16* row = qkv + (int64_t)b * qkv_dim;
    const int64_t kv_base = ((int64_t)layer * batch + b) * kv_heads;
    // rotary on q heads and k heads: one thread per (head, i < hd/2)
    for (int e = threadIdx.x; e < (heads + kv_heads) * half; e += blockDim.x) {
        const int h = e / half, i = e - h * half;
        const float ang = rp * inv_freq[i];
        // HF casts cos/sin to the activation dtype (TF:modeling_qwen2_vl.py:169)
        const float c = bfround(cosf(ang)), s = bfround(sinf(ang));
        const float x0 = bfbits2f(row[h * hd + i]), x1 = bfbits2f(row[h * hd + i + half]);
        const __bf16 y0 = f2bf(x0 * c - x1 * s), y1 = f2bf(x1 * c + x0 * s);
        kr_bf16* dst;
        if (h < heads) {
            dst = q_out + ((int64_t)b * heads + h) * hd;
        } else {
            dst = kcache + ((kv_base + (h - heads)) * s_max + pos) * hd;
        }
        dst[i] = __builtin_bit_cast(kr_bf16, y0);
        dst[i + half] = __builtin_bit_cast(kr_bf16, y1);
    }
    // V -> transposed cache column
    const kr_bf16* vrow = row + (heads + kv_heads) * hd;
    for (int e = threadIdx.x; e < kv_heads * hd; e += blockDim.x) {
        const int h = e / hd, d = e - h * hd;
        vtcache[((kv_base + h) * (s_max >> 6) + (pos >> 6)) * (hd * 64) + kr_vt_off(d, pos & 63, hd)] = vrow[e];
    }
}

// =====================================================================================
// decode attention, v_mfma_f32_16x16x32_bf16, K and V^T straight from HBM to registers
// =====================================================================================
// grid = (n_split, kv_heads, batch), 4 waves per block; wave `part` = split*4 + wave walks the
// 64-key blocks part, part + n_part, ...  Heads of the GQA group sit on the 16 MFMA columns.
//   S[key][g]   : A = K rows (keys permuted so that lane group fg ends up with keys 8fg..8fg+7)
//                 B = Q^T
//   O^T[d][g]  += A = V^T (16 B = 8 consecutive keys per lane), B = P^T (the S accumulators)
// Partials (m, l, O) go to the fp32 workspace; attn_decode_combine_kernel merges them.
template <int HD>
__global__ void __launch_bounds__(256) attn_decode_kernel(const kr_bf16* __restrict__ q, const kr_bf16* __restrict__ kcache,
                                                          const kr_bf16* __restrict__ vtcache,
                                                          const int32_t* __restrict__ ctx_len, float* __restrict__ ws,
                                                          int heads, int kv_heads, int layer, int batch, int s_max,
                                                          float scale_log2e) {
    constexpr int DT = HD / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int group = heads / kv_heads;
    const int n_part = gridDim.x * 4;
    const int part = blockIdx.x * 4 + wave;
    const int ctx = ctx_len[b] + 1;
    const int nb = (ctx + 63) >> 6;

    const int g = fr < group ? fr : 0;
    const kr_bf16* qp = q + ((int64_t)b * heads + kvh * group + g) * HD + fg * 32;
    bf16x8 qf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qf[i] = ld8(qp + i * 8);

    const int64_t kv_base = ((int64_t)layer * batch + b) * kv_heads + kvh;
    const kr_bf16* kc = kcache + kv_base * s_max * HD;
    const kr_bf16* vc = vtcache + kv_base * (int64_t)(s_max >> 6) * (HD * 64);

    f32x4 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) o[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    for (int blk = part; blk < nb; blk += n_part) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int key0 = blk * 64 + hf * 32;
            if (key0 >= ctx) break;  // wave-uniform
            // K fragments: tile kt, row r holds key 8(r>>2) + 4kt + (r&3)
            bf16x8 kf[2][4];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const kr_bf16* kp = kc + (int64_t)(key0 + 8 * (fr >> 2) + 4 * kt + (fr & 3)) * HD + fg * 32;
#pragma unroll
                for (int i = 0; i < 4; ++i) kf[kt][i] = ld8_nt(kp + i * 8);
            }
            // V^T fragments: row d = dt*16 + fr, keys key0 + 8fg .. +7
            bf16x8 vf[DT];
            const kr_bf16* vp = vc + (int64_t)blk * (HD * 64) + hf * (HD * 32) + fg * 8;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) vf[dt] = ld8_nt(vp + (dt * 16 + fr) * 32);

            f32x4 s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][i], qf[i], s[kt], 0, 0, 0);
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + 8 * fg + 4 * kt + r;
                    const float v = key < ctx ? s[kt][r] * scale_log2e : -INFINITY;
                    s[kt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            bf16x8 pf;
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const __bf16 pb = f2bf(__builtin_amdgcn_exp2f(s[kt][r] - m_new));
                    psum += bf2f(pb);
                    pf[kt * 4 + r] = pb;
                }
            l_run = l_run * alpha + psum;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[dt], pf, o[dt], 0, 0, 0);
            }
        }
    }
    // l: sum the four key groups of each head column
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (fr < group) {
        float* w = ws + (((int64_t)b * heads + kvh * group + fr) * n_part + part) * (HD + 2);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(w + dt * 16 + fg * 4) = o[dt];
        if (fg == 0) {
            w[HD] = m_run;
            w[HD + 1] = l_run;
        }
    }
}

// grid = batch*heads blocks of HD threads
__global__ void attn_decode_combine_kernel(const float* __restrict__ ws, kr_bf16* __restrict__ out, int n_part, int hd) {
    const int bh = blockIdx.x, d = threadIdx.x;
    const float* w = ws + (int64_t)bh * n_part * (hd + 2);
    float mx = -1e30f;
    for (int p = 0; p < n_part; ++p) mx = fmaxf(mx, w[p * (hd + 2) + hd]);
    float acc = 0.f, l = 0.f;
    for (int p = 0; p < n_part; ++p) {
        const float sc = __builtin_amdgcn_exp2f(w[p * (hd + 2) + hd] - mx);
        l += w[p * (hd + 2) + hd + 1] * sc;
        acc += w[p * (hd + 2) + d] * sc;
    }
    out[(int64_t)bh * hd + d] = __builtin_bit_cast(kr_bf16, f2bf(l > 0.f ? acc / l : 0.f));
}

// scattered K / V^T append (standalone operator; the engine uses the blocked prep kernels)
__global__ void __launch_bounds__(256) kv_append_kernel(const kr_bf16* __restrict__ k, const kr_bf16* __restrict__ v,
                                                        int64_t row_stride, const int32_t* __restrict__ tok_seq,
                                                        const int32_t* __restrict__ tok_pos, kr_bf16* __restrict__ kcache,
                                                        kr_bf16* __restrict__ vtcache, int64_t n, int kv_heads, int hd,
                                                        int layer, int batch, int s_max) {
    const int64_t total = n * kv_heads * hd;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % hd);
        const int64_t t = i / hd;
        const int h = (int)(t % kv_heads);
        const int64_t tok = t / kv_heads;
        const int sq = tok_seq[tok], pos = tok_pos[tok];
        const int64_t base = ((int64_t)layer * batch + sq) * kv_heads + h;
        kcache[(base * s_max + pos) * hd + d] = k[tok * row_stride + h * hd + d];
        vtcache[(base * (s_max >> 6) + (pos >> 6)) * (hd * 64) + kr_vt_off(d, pos & 63, hd)] = v[tok * row_stride + h * hd + d];
    }
}

}  // namespace

extern "C" int kr_kv_append(const kr_bf16* k, const kr_bf16* v, int64_t row_stride, const int32_t* tok_seq,
                            const int32_t* tok_pos, kr_bf16* kcache, kr_bf16* vtcache, int64_t n, int kv_heads, int hd,
                            int layer, int batch, int s_max, kr_stream s) {
    KR_CHECK_ARG(k && v && tok_seq && tok_pos && kcache && vtcache && s_max % 64 == 0, "kr_kv_append: bad args");
    if (n == 0) return KR_OK;
    const int64_t total = n * kv_heads * hd;
    int grid = (int)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    kv_append_kernel<<<grid, 256, 0, kr_hs(s)>>>(k, v, row_stride, tok_seq, tok_pos, kcache, vtcache, n, kv_heads, hd,
                                                 layer, batch, s_max);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_decode_qkv_prep(const kr_bf16* qkv, const float* inv_freq, const int32_t* ctx_len,
                                  const int32_t* rope_delta, kr_bf16* q_out, kr_bf16* kcache, kr_bf16* vtcache, int batch,
                                  int heads, int kv_heads, int hd, int layer, int s_max, kr_stream s) {
    KR_CHECK_ARG(qkv && inv_freq && ctx_len && rope_delta && q_out && kcache && vtcache, "kr_decode_qkv_prep: null");
    KR_CHECK_ARG(batch > 0 && s_max % 64 == 0 && hd % 2 == 0, "kr_decode_qkv_prep: bad sizes");
    decode_qkv_prep_kernel<<<batch, 256, 0, kr_hs(s)>>>(qkv, inv_freq, ctx_len, rope_delta, q_out, kcache, vtcache, heads,
                                                        kv_heads, hd, layer, batch, s_max);
    KR_CHECK_LAUNCH();
    return KR_OK;
}

extern "C" int kr_attn_decode_gqa(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache, const int32_t* ctx_len,
                                  kr_bf16* out, float* workspace, int batch, int heads, int kv_heads, int hd, int layer,
                                  int s_max, int n_split, float scale, kr_stream s) {
    KR_CHECK_ARG(q && kcache && vtcache && ctx_len && out && workspace, "kr_attn_decode_gqa: null pointer");
    KR_CHECK_ARG(hd == 128, "kr_attn_decode_gqa: hd=%d (only 128)", hd);
    KR_CHECK_ARG(heads % kv_heads == 0 && heads / kv_heads <= 16, "kr_attn_decode_gqa: GQA group must be <= 16");
    KR_CHECK_ARG(batch > 0 && n_split > 0 && s_max % 64 == 0, "kr_attn_decode_gqa: bad sizes");
    dim3 grid(n_split, kv_heads, batch);
    attn_decode_kernel<128><<<grid, 256, 0, kr_hs(s)>>>(q, kcache, vtcache, ctx_len, workspace, heads, kv_heads, layer,
                                                        batch, s_max, scale * 1.4426950408889634f);
    KR_CHECK_LAUNCH();
    attn_decode_combine_kernel<<<batch * heads, hd, 0, kr_hs(s)>>>(workspace, out, n_split * 4, hd);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
