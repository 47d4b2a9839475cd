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
};

__device__ __forceinline__ void apply_w_scale(const float* w_scale, int n, f32x4& acc) {
    if (w_scale) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(w_scale + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] *= sc[j];
    }
}

__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

}  // namespace
