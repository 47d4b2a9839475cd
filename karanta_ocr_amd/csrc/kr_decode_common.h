// What more than one decode source uses (kr_decode.hip, kr_decode32.hip, kr_attn_decode.hip, kr_sample.hip): the
// experiment switch, the epilogue modes, the weight chunk of the decode linears, two small device helpers.
#pragma once
#include "kr_common.h"

namespace {

// -DKR_EXPERIMENTS (csrc/tools/build_variant.py): the measured-and-not-adopted decode experiments of rounds 1-2 — Infinity-Cache
// prefetch workgroups riding on the qkv launch, the fast-residual mode (per-head o_proj with float atomics: dec_oproj_heads_kernel,
// f32 x rows in the wide / narrow kernels; kr_decode.hip), the in-launch split-KV merge of the attention kernel
// (kr_attn_decode.hip).  The shipped library holds the product path and the general dec_linear_kernel fallback only; the
// experiment entry points are declared in include/karanta_hip_experiments.h.
#ifdef KR_EXPERIMENTS
constexpr bool KR_EXP = true;
#else
constexpr bool KR_EXP = false;
#endif

constexpr int DEPI_PLAIN = 0, DEPI_SILU = 1, DEPI_ROPE_KV = 2, DEPI_ARGMAX = 3, DEPI_SILU8 = 4;
constexpr int DEPI_PARTIAL = 16;  // internal: PLAIN with deferred split-K slabs

// One 64-wide K chunk of a 16-row weight tile in registers, and where its operands sit.
//  bf16 : 2 KiB per chunk, two 16-byte loads per lane; lane (r, g) holds k = 32h + 8g .. +7 of k-step h
//  fp8  : 1 KiB per chunk, ONE 16-byte load per lane; lane (r, g) holds k = 16g .. 16g+15, k-step h takes 16g + 8h .. +7
//         (x is read in the same order, a dot product does not care), converted to bf16 in registers
//         (v_cvt_scalef32_pk_bf16_fp8: every e4m3 value is exact in bf16; the per-row scale is applied in the epilogue)
// x_byte: the operand inside the chunk's 128 B of a row-major x row (<= 16-row kernels); xp_off: inside a column tile's
// 2 KiB of a packed chunk (XP layout of 17..32-row batches, kr_decode32.hip).
// load<RES>: the cache policy of the weight loads.  false (every launch but the ones the engine picks): nontemporal, the line is
// not kept behind the wave that read it; true: default policy, the line stays in the Infinity Cache for the next decode step
// (the narrow kernel's w_resident launches: DESIGN section 5-r5).  The bytes loaded are the same.
template <bool W8> struct WChunk;
template <> struct WChunk<false> {
    static constexpr int BYTES = 2048;
    bf16x8 v[2];
    template <bool RES = false> __device__ __forceinline__ void load(const char* p, int64_t c) {
        const kr_bf16* q = reinterpret_cast<const kr_bf16*>(p + c * BYTES);
        v[0] = RES ? ld8(q) : ld8_nt(q);
        v[1] = RES ? ld8(q + 512) : ld8_nt(q + 512);
    }
    __device__ __forceinline__ bf16x8 frag(int h) const { return v[h]; }
    static __device__ __forceinline__ int x_byte(int h, int fg) { return h * 64 + fg * 16; }
    // lane (fr, fg) of k-step h holds k = 32h + 8fg .. +7: block h, lane's own 16 bytes
    static __device__ __forceinline__ int xp_off(int h, int fr, int fg) { return h * 1024 + (fg * 16 + fr) * 16; }
    // the same inside a chunk of R row slots (XP16 layout, kr_common.h): row fr < R
    static __device__ __forceinline__ int xp16_off(int h, int fr, int fg, int R) { return h * (R * 64) + (fg * R + fr) * 16; }
};
template <> struct WChunk<true> {
    static constexpr int BYTES = 1024;
    u32x4 q;
    template <bool RES = false> __device__ __forceinline__ void load(const char* p, int64_t c) {
        const u32x4* w = reinterpret_cast<const u32x4*>(p + c * BYTES);
        q = RES ? *w : __builtin_nontemporal_load(w);
    }
    __device__ __forceinline__ bf16x8 frag(int h) const {
        // each conversion yields two bf16 packed in one register; they are moved as 32-bit words (element-wise
        // extraction of the builtin's 2 x bf16 result is mis-lowered by this compiler: both halves read the low one)
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int w = (int)q[2 * h + i];
            o[2 * i + 0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
            o[2 * i + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
        }
        return __builtin_bit_cast(bf16x8, o);
    }
    static __device__ __forceinline__ int x_byte(int h, int fg) { return fg * 32 + h * 16; }
    // fp8 chunk: lane (fr, fg) of k-step h holds k = 16fg + 8h .. +7 = block (fg >> 1), lane group 2 (fg & 1) + h
    static __device__ __forceinline__ int xp_off(int h, int fr, int fg) { return (fg >> 1) * 1024 + ((((fg & 1) << 1) | h) * 16 + fr) * 16; }
    static __device__ __forceinline__ int xp16_off(int h, int fr, int fg, int R) {
        return (fg >> 1) * (R * 64) + ((((fg & 1) << 1) | h) * R + fr) * 16;
    }
};

__device__ __forceinline__ void apply_w_scale(const float* w_scale, int n, f32x4& acc) {
    if (w_scale) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(w_scale + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] *= sc[j];
    }
}

// ---------------------------------------------------------------- fp8 (e4m3fn) KV cache (include/karanta_hip.h, kr_kv8)
// DEPI_ROPE_KV8: ROPE_KV whose K / V go to an fp8 cache.  A value of the EPI template parameter only (the fp8-cache entry points
// pick it); the public mode stays KR_DEC_ROPE_KV.
constexpr int DEPI_ROPE_KV8 = 5;
constexpr bool depi_rope(int epi) { return epi == DEPI_ROPE_KV || epi == DEPI_ROPE_KV8; }

// The cache pointers of an fp8-cache launch as they travel in kernel arguments (kr_kv8 by value).
struct Kv8 {
    uint8_t* k; uint8_t* vt; const float* scale;
};

// THE quantisation rule: a bf16-rounded value x, divided by the scale in f32 (a correctly rounded division: tests/kv_fp8_ref.py
// restates it in numpy), clamped to +-448 explicitly, converted with v_cvt_pk_fp8_f32 (RNE).  `clamped` counts the values the
// clamp changed.  v_med3_f32 returns the minimum of the two bounds for a NaN input: -448, a finite code.
__device__ __forceinline__ float kv8_clamp(float x, float sc, int& clamped) {
    const float y = x / sc;
    const float c = __builtin_amdgcn_fmed3f(y, -448.f, 448.f);
    clamped += (c != y) ? 1 : 0;
    return c;
}
// four values -> four codes in one register, byte j = value j
__device__ __forceinline__ unsigned kv8_pack4(float x0, float x1, float x2, float x3, float sc, int& clamped) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(x0, sc, clamped), kv8_clamp(x1, sc, clamped), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(x2, sc, clamped), kv8_clamp(x3, sc, clamped), w, true);
    return (unsigned)w;
}
__device__ __forceinline__ uint8_t kv8_code(float x, float sc, int& clamped) {
    return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(x, sc, clamped), 0.f, 0, false) & 0xff);
}
// eight codes (two registers, ascending bytes) -> eight bf16, exactly (moved as 32-bit words: see WChunk<true>::frag)
__device__ __forceinline__ bf16x8 kv8_to_bf16x8(unsigned w0, unsigned w1) {
    u32x4 o;
    o[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w0, 1.0f, false));
    o[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w0, 1.0f, true));
    o[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w1, 1.0f, false));
    o[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w1, 1.0f, true));
    return __builtin_bit_cast(bf16x8, o);
}

// The ROPE_KV8 append of one lane: channels i0 .. i0+3 and 64+i0 .. 64+i0+3 of row `pos` of a (slot, kv head) whose K rows start
// at `krow0` and whose V^T blocks at `vt0`.  K: two packed 4-byte stores; V^T: byte stores at stride 32 (kr_vt_off).
__device__ __forceinline__ void kv8_append_k(uint8_t* krow0, int pos, int i0, const bf16x4& o0, const bf16x4& o1, float sc) {
    int n = 0;
    uint8_t* dst = krow0 + (int64_t)pos * 128;
    *reinterpret_cast<unsigned*>(dst + i0) = kv8_pack4(bf2f(o0[0]), bf2f(o0[1]), bf2f(o0[2]), bf2f(o0[3]), sc, n);
    *reinterpret_cast<unsigned*>(dst + 64 + i0) = kv8_pack4(bf2f(o1[0]), bf2f(o1[1]), bf2f(o1[2]), bf2f(o1[3]), sc, n);
}
__device__ __forceinline__ void kv8_append_v(uint8_t* vt0, int pos, int i0, const float (&lo)[4], const float (&hi)[4], float sc) {
    int n = 0;
    uint8_t* vt = vt0 + (int64_t)(pos >> 6) * (128 * 64) + kr_vt_off(0, pos & 63, 128);
    // lo / hi are bf16-rounded already (the projection output is a bf16 tensor)
    const unsigned a = kv8_pack4(lo[0], lo[1], lo[2], lo[3], sc, n), b = kv8_pack4(hi[0], hi[1], hi[2], hi[3], sc, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        vt[(i0 + j) * 32] = (uint8_t)(a >> (8 * j));
        vt[(64 + i0 + j) * 32] = (uint8_t)(b >> (8 * j));
    }
}

__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

}  // namespace
