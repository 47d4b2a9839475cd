/*
 * karanta_hip.h — C-ABI of libkaranta_hip.so, the MI355X (gfx950) kernel library behind the
 * karanta-ocr VLM inference hot path.
 *
 * What it replaces.  The reference has NO in-process kernel interface: the Qwen2-VL
 * image-encoder + text-decoder forward runs in an external `vllm serve` process
 * (reference karanta/pipeline.py:707-742 spawn, :317-319 HTTP POST;
 * bulk_processing/workers/vllm_client.py:209 POST) or inside Hugging Face `model.generate`
 * (karanta/training/test_trained_model.py:76-99).  The entry points below are therefore the
 * operator set those third-party forwards execute, one C function per
 * operator, each citing the Hugging Face symbol whose arithmetic it reproduces
 * ("TF:" = transformers/models/qwen2_vl/modeling_qwen2_vl.py, line numbers as in SURVEY.md §8 a-ii).
 * INTEGRATION.md shows the ctypes binding a reference maintainer adds.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.  Device pointers are raw HIP device addresses
 *    (e.g. torch.Tensor.data_ptr()); the caller owns every buffer.
 *  - Every launch takes `kr_stream` (a hipStream_t cast to void*; NULL = default stream) and is
 *    asynchronous on it.  No function synchronises unless its name says so.
 *  - Return value: 0 = ok, <0 = error; kr_last_error() gives a thread-local message.
 *    No exceptions cross the ABI.  No global mutable state besides the error string.
 *  - "bf16" buffers are raw uint16 bit patterns (round-to-nearest-even); fp32 accumulate inside
 *    every kernel.  Row-major unless stated.
 *  - Shapes that a kernel cannot serve are rejected on the host with an error (never launched).
 */
#ifndef KARANTA_HIP_H
#define KARANTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* kr_stream; /* hipStream_t */
typedef uint16_t kr_bf16;

/* kr_version() of the library this header describes: major * 100 + minor.  The major changes with every incompatible
 * change of a signature or struct below (r4: kr_narrow_opts argument of round 3, packed 17..32-row family; r9:
 * kr_narrow_opts.x_packed, which the library reads from every caller's struct); a caller built against major X must refuse a
 * library whose kr_version() / 100 != X. */
#define KR_ABI_VERSION 500

#define KR_OK 0
#define KR_ERR_ARG (-1)    /* unsupported shape / null pointer */
#define KR_ERR_HIP (-2)    /* HIP runtime error */
#define KR_ERR_RCCL (-3)   /* RCCL error */
#define KR_ERR_STATE (-4)  /* wrong call order (graph capture etc.) */

/* GEMM / GEMV epilogues (applied to the fp32 accumulator, then one rounding to the output type) */
#define KR_EPI_NONE 0
#define KR_EPI_QUICK_GELU 1 /* x*sigmoid(1.702x): ViT fc1, TF:293-301 */
#define KR_EPI_GELU_ERF 2   /* exact GELU: PatchMerger, TF:277-290 */
#define KR_EPI_SILU_MUL 3   /* silu(gate)*up with gate/up rows interleaved in 16-row groups: Qwen2MLP, TF:453-466 */
#define KR_EPI_SILU_MUL8 4  /* same, interleaved in 8-row groups (g0..g7,u0..u7,g8..): one 16-row MFMA tile = 8 features;
                             * kr_gemm_bf16 takes an optional bias here, interleaved like the rows (the biased SwiGLU
                             * MLP of the Qwen2.5-VL vision blocks, TF25:85-97) */

/* ------------------------------------------------------------------ library / device */
int kr_version(void);
const char* kr_last_error(void);
/* fills name (<=63 chars), CU count, total memory bytes of `device`. */
int kr_device_info(int device, char* name64, int* compute_units, size_t* total_mem);
int kr_set_device(int device);
int kr_stream_synchronize(kr_stream s);
/* A stream restricted to `cus_enabled` of the device's compute units (hipExtStreamCreateWithCUMask; the first cus_enabled
 * bits of the mask: on an 8-XCD part cus_enabled / 8 CUs of every XCD).  The continuous-batching server runs its admissions
 * (ViT + prefill: MFMA-bound, long-running workgroups) on such a stream beside the decode graph (HBM-bound, short
 * launches) on the main one — the reference gets the same overlap from vLLM's chunked prefill.  kr_stream_destroy frees it. */
int kr_stream_create_cu_mask(kr_stream* out, int cus_enabled);
/* The same with the mask bits [first_cu, first_cu + n_cus): a second stream on the COMPLEMENT of a kr_stream_create_cu_mask stream shares no
 * compute unit with it (the decode graph beside an admission: neither launch waits for a workgroup slot of the other). */
int kr_stream_create_cu_range(kr_stream* out, int first_cu, int n_cus);
int kr_stream_destroy(kr_stream s);

/* ------------------------------------------------------------------ profiling events
 * HIP events on the caller's stream, used by bench.py to time kernels on the stream they are
 * launched on (torch.cuda.Event only sees torch's current stream). */
int kr_event_create(void** ev);
int kr_event_destroy(void* ev);
int kr_event_record(void* ev, kr_stream s);
/* hipStreamWaitEvent: inside a stream capture this forks / joins the graph (a second stream pulled in by an event of
 * the capturing stream becomes a parallel branch; an event of that stream waited on by the capturing one is the join). */
int kr_stream_wait_event(kr_stream s, void* ev);
int kr_event_synchronize(void* ev);
int kr_event_elapsed_ms(void* start, void* stop, float* ms);

/* ------------------------------------------------------------------ HIP graphs (decode step replay) */
int kr_graph_begin_capture(kr_stream s);
int kr_graph_end_capture(kr_stream s, void** graph_exec);
int kr_graph_launch(void* graph_exec, kr_stream s);
int kr_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------ elementwise / norms */

/* pixel_values fp32 [rows, k] -> bf16 [rows, k_pad], zero padded (k_pad % 8 == 0).
 * Front of PatchEmbed (TF:251-274): `hidden_states.to(dtype=target_dtype)`. */
int kr_cast_pad_f32_bf16(const float* src, kr_bf16* dst, int64_t rows, int k, int k_pad, kr_stream s);

/* nn.LayerNorm with bias, fp32 statistics (ViT blocks TF:425-449, merger ln_q TF:277-290).
 * x,y bf16 [rows, d]; w,b bf16 [d]; d % 8 == 0, d <= 8192. */
int kr_layernorm(const kr_bf16* x, const kr_bf16* w, const kr_bf16* b, kr_bf16* y,
                 int64_t rows, int d, float eps, kr_stream s);

/* Qwen2VLRMSNorm (TF:96-110): y = w * bf16(x * rsqrt(mean(x^2)+eps)).
 * x has row stride ldx (elements); y is dense [rows, d]. */
int kr_rmsnorm(const kr_bf16* x, int64_t ldx, const kr_bf16* w, kr_bf16* y,
               int64_t rows, int d, float eps, kr_stream s);

/* ------------------------------------------------------------------ dense linears */

/* C[M,N] = epi(A[M,K] * W[N,K]^T + bias[N]) (+ residual[M,N]); nn.Linear with the weight in its
 * native [out,in] layout.  bf16 in, fp32 MFMA accumulate, bf16 out.  K % 64 == 0.
 * bias / residual may be NULL.  With KR_EPI_SILU_MUL, W holds gate/up rows interleaved in groups
 * of 16 (g0..g15,u0..u15,g16..), N counts both, C is [M, N/2] and N % 32 == 0.
 * lda / ldc / ldr are row strides in elements.  w_packed != 0: W is stored in the decode layout
 * [N/16][K/32][4][16][8] (see kr_linear_decode) instead of row-major — one copy of the decoder
 * weights serves prefill and decode.  Used for every ViT Linear, the merger, and every decoder
 * Linear at prefill. */
int kr_gemm_bf16(const kr_bf16* A, int64_t lda, const kr_bf16* W, const kr_bf16* bias,
                 const kr_bf16* residual, int64_t ldr, kr_bf16* C, int64_t ldc,
                 int64_t M, int N, int K, int epilogue, int w_packed, kr_stream s);

/* kr_gemm_bf16 with a CALLER-OWNED split-K scratch (>= KR_GEMM_SCRATCH_BYTES, 16-byte aligned; NULL = kr_gemm_bf16).
 * A launch whose last round of 256x256 tiles is at most half full runs that round as 128x128 quarters; with K >= 4096
 * and a scratch each quarter is also cut along K (partials into the scratch, then a reduce-in-split-order + epilogue
 * launch; prefill down_proj 353 -> 259 us).  The library allocates nothing and keeps nothing between calls: the same
 * call with the same scratch argument gives the same bits whatever ran before it, inside a stream capture or not.  The
 * scratch must not be used by another stream's GEMM at the same time. */
#define KR_GEMM_SCRATCH_BYTES ((size_t)512 * 65536)
int kr_gemm_bf16_ws(const kr_bf16* A, int64_t lda, const kr_bf16* W, const kr_bf16* bias,
                    const kr_bf16* residual, int64_t ldr, kr_bf16* C, int64_t ldc,
                    int64_t M, int N, int K, int epilogue, int w_packed, float* scratch, size_t scratch_bytes, kr_stream s);

/* kr_gemm_bf16 with weight-only fp8 (BASELINE.json config 5: "fp8 weights, bf16 activations"; SURVEY.md §8(b2)
 * kr_gemm_fp8): W as OCP e4m3fn codes in the decode layout [N/16][K/64][4][16][16] (weights.pack_w16x64_fp8) with one
 * f32 scale per output row, C = epi(A (scale * W)^T + bias) (+ residual).  The codes are converted to bf16 on the way
 * from LDS to the MFMA, accumulation is fp32, the scale multiplies the accumulator.  Epilogues KR_EPI_NONE and
 * KR_EPI_SILU_MUL8 (the decoder's prefill linears).  K % 64 == 0, N % 16 == 0, ldc % 8 == 0, C 16-byte aligned. */
int kr_gemm_fp8(const kr_bf16* A, int64_t lda, const uint8_t* w_packed_fp8, const float* w_scale, const kr_bf16* bias,
                const kr_bf16* residual, int64_t ldr, kr_bf16* C, int64_t ldc, int64_t M, int N, int K, int epilogue,
                kr_stream s);

/* W8A8 prefill on the fp8 matrix instruction (BASELINE.json config 5: "Qwen2-VL-7B fp8 weights (CDNA4 fp8 MFMA)"; the
 * reference's default OLMO_7B_0725_FP8, /root/reference/karanta/constants.py:23, is served by vLLM with dynamic per-token
 * activation scales):
 *   kr_quantize_rows_fp8 : x bf16 [rows, K] (row stride ldx elements) -> q e4m3fn codes [rows, K] (row stride ldq BYTES,
 *       a multiple of 16) + scale f32 [rows]: scale = max|row| / 448 (1 for an all-zero row), code = e4m3(x / scale), round
 *       to nearest even (bit-identical to weights.quantize_fp8_rows on the host);
 *   kr_gemm_fp8a : C = epi((a_scale * A8) (w_scale * W8)^T + bias) (+ residual) with both operands as codes through
 *       v_mfma_f32_16x16x32_fp8_fp8 (products of two e4m3 values are exact in f32; f32 accumulation), the two scales applied
 *       to the accumulators.  A8 row-major [M, lda bytes]; weights, epilogues and constraints as kr_gemm_fp8. */
int kr_quantize_rows_fp8(const kr_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, float* scale, int64_t rows, int K, kr_stream s);
int kr_gemm_fp8a(const uint8_t* A8, int64_t lda, const float* a_scale, const uint8_t* w_packed_fp8, const float* w_scale,
                 const kr_bf16* bias, const kr_bf16* residual, int64_t ldr, kr_bf16* C, int64_t ldc, int64_t M, int N, int K,
                 int epilogue, kr_stream s);

/* Decode-time Linear for M <= 16 rows (one row per live sequence): the weight matrix is streamed
 * exactly once from HBM (this is the HBM-roofline kernel of the decode loop).
 * Same semantics and epilogues as kr_gemm_bf16.  If out_f32 != NULL the result is written there
 * as fp32 [M, ldc] instead of bf16 (lm_head logits, TF:1320-1323).
 * If norm_w != NULL, x is first RMS-normalised (Qwen2VLRMSNorm, eps=norm_eps) on the fly. */
int kr_gemv_bf16(const kr_bf16* x, int64_t ldx, const kr_bf16* W, const kr_bf16* bias,
                 const kr_bf16* residual, int64_t ldr, kr_bf16* out, float* out_f32, int64_t ldc,
                 int M, int N, int K, int epilogue,
                 const kr_bf16* norm_w, float norm_eps, kr_stream s);

/* ------------------------------------------------------------------ ViT attention path */

/* Rotary + re-layout in 64-token blocks, shared by the ViT (apply_rotary_pos_emb_vision,
 * TF:225-236, rotate_half TF:173-177) and the decoder prefill (apply_multimodal_rotary_pos_emb,
 * TF:180-222, with section-interleaved cos/sin precomputed on the host).
 * `qkv` is the fused projection output, row stride ld_qkv, with q / k / v starting at column
 * q_off / k_off / v_off (elements), heads contiguous.  cos,sin fp32 [n, hd] by token row.
 * Block i covers tokens blk_tok0[i] .. +blk_ntok[i] (<= 64) of one segment, starting at a
 * multiple of 64 inside that segment:
 *   q_out  [q_heads][token row][hd]                    (head stride q_head_stride elements)
 *   k_out  [kv_heads][rows][hd]: token j -> row blk_k_row0[i] + j   (head stride k_head_stride)
 *   vt_out [kv_heads][blocks][2][hd][32]: V transposed in 64-token blocks, each block as two contiguous 32-token halves
 *          (element (channel d, token j of the block) at ((j / 32) * hd + d) * 32 + j % 32; round 4: a decode-attention wave reads
 *          a 32-key unit as whole cache lines — rounds 1-3 stored [hd][64]), block blk_vt_blk[i], zero padded
 * For the decoder, k_out / vt_out are the KV cache of one layer. hd in {80, 128}. */
int kr_qkv_prep(const kr_bf16* qkv, int64_t ld_qkv, int q_off, int k_off, int v_off,
                const float* cos, const float* sin,
                const int32_t* blk_tok0, const int32_t* blk_ntok,
                const int64_t* blk_k_row0, const int64_t* blk_vt_blk, int n_blk,
                kr_bf16* q_out, int64_t q_head_stride, kr_bf16* k_out, int64_t k_head_stride,
                kr_bf16* vt_out, int64_t vt_head_stride, int q_heads, int kv_heads, int hd,
                kr_stream s);

/* Plain in-place rotary on a [n, heads, hd] tensor (kept for API parity with SURVEY §8 b2
 * `kr_rope2d_vision`; the engine uses the fused kr_vit_qkv_prep). */
int kr_rope2d_vision(kr_bf16* x, const float* cos, const float* sin, int64_t n, int heads, int hd,
                     int64_t row_stride, kr_stream s);

/* Flash-style attention over variable-length segments, fp32 online softmax, bf16 P (as
 * eager_attention_forward TF:317-339 computes it: softmax in fp32, cast, P*V).
 *   q : [q_heads, nq_total, hd]   k : [kv_heads, *, hd] rows   vt : [kv_heads, *, 2, hd, 32] blocks (kr_qkv_prep's layout)
 *   out : [nq_total, q_heads*hd]
 * Work list: qblk[4*i+0..3] = {q_row0 (global row of first query), n_q_rows (<=128),
 *   k_row0 (global k row of the segment's key 0), vt_block0}; qblk_len[2*i+0..1] =
 *   {kv_len visible to the LAST query of the block when causal / segment length otherwise,
 *    position of the block's first query inside its segment}.
 * kv head = q head / (q_heads / kv_heads).  k_head_stride / vt_head_stride in elements.
 * hd in {80, 128}.  causal=0: ViT full attention per image (VisionAttention TF:342-422, segments
 * from cu_seqlens TF:399-418); causal=1: decoder prefill (Qwen2VLAttention TF:469-556). */
int kr_attn_varlen(const kr_bf16* q, const kr_bf16* k, const kr_bf16* vt, kr_bf16* out,
                   const int32_t* qblk, const int32_t* qblk_len, int n_qblk,
                   int64_t nq_total, int q_heads, int kv_heads, int hd,
                   int64_t k_head_stride, int64_t vt_head_stride, float scale, int causal,
                   kr_stream s);
/* The same with the work list's query-block size stated: 128 (4-wave workgroups, what kr_attn_varlen assumes) or 256
 * (8-wave workgroups: twice the queries per staged K / V^T tile; the list must have been built for that block size). */
int kr_attn_varlen_q(const kr_bf16* q, const kr_bf16* k, const kr_bf16* vt, kr_bf16* out,
                     const int32_t* qblk, const int32_t* qblk_len, int n_qblk,
                     int64_t nq_total, int q_heads, int kv_heads, int hd,
                     int64_t k_head_stride, int64_t vt_head_stride, float scale, int causal,
                     int q_block, kr_stream s);

/* ------------------------------------------------------------------ decoder: embedding, M-RoPE, KV cache */

/* inputs_embeds (TF:1159-1168): row i of out = table[src[i]] if src[i] >= 0, else
 * image_embeds[-src[i]-1] (masked_scatter order precomputed on the host). bf16, d % 8 == 0. */
int kr_embed_scatter(const int32_t* src, const kr_bf16* table, const kr_bf16* image_embeds,
                     kr_bf16* out, int64_t rows, int d, kr_stream s);

/* KV cache of one model:
 *   kcache  : [layers, batch, kv_heads, s_max, hd]
 *   vtcache : [layers, batch, kv_heads, s_max/64, 2, hd, 32]   (V transposed in 64-token blocks of two contiguous 32-token
 *             halves: kr_qkv_prep's layout; every writer and reader of the cache in this library uses it)
 * zero-initialised by the caller (masked keys are multiplied by P = 0, so they must be finite). */

/* SURVEY §8 b2 names kept as thin standalone operators (tests call them directly). */
int kr_mrope(kr_bf16* x, const float* cos, const float* sin, int64_t n, int heads, int hd,
             int64_t row_stride, kr_stream s);
int kr_kv_append(const kr_bf16* k, const kr_bf16* v, int64_t row_stride,
                 const int32_t* tok_seq, const int32_t* tok_pos,
                 kr_bf16* kcache, kr_bf16* vtcache,
                 int64_t n, int kv_heads, int hd, int layer, int batch, int s_max, kr_stream s);

/* Decode step front: for each live sequence b (one new token): M-RoPE at position
 * ctx_len[b] + rope_delta[b] (all three axes equal for text tokens, TF:1124-1136), computed from
 * inv_freq fp32 [hd/2]; writes q_out [batch, heads, hd] and appends K / V^T at cache position
 * ctx_len[b].  ctx_len is NOT modified (kr_argmax_embed advances it once per step). */
int kr_decode_qkv_prep(const kr_bf16* qkv, const float* inv_freq, const int32_t* ctx_len,
                       const int32_t* rope_delta, kr_bf16* q_out, kr_bf16* kcache, kr_bf16* vtcache,
                       int batch, int heads, int kv_heads, int hd, int layer, int s_max, kr_stream s);

/* Decode attention, q_len = 1, GQA, context = ctx_len[b] + 1 tokens (the new token included),
 * split over `n_split` key ranges; partials go to `workspace` (fp32,
 * batch*heads*n_split*(hd+2) floats) and are merged by the same call's second kernel.
 * out : [batch, heads*hd] bf16.  (Qwen2VLAttention with cache, TF:469-556.) */
int kr_attn_decode_gqa(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache,
                       const int32_t* ctx_len, kr_bf16* out, float* workspace,
                       int batch, int heads, int kv_heads, int hd, int layer, int s_max,
                       int n_split, float scale, kr_stream s);

/* Greedy sampling (`generate(do_sample=False)`, reference test_trained_model.py:91): argmax of
 * fp32 logits [batch, vocab] (lowest index wins ties), token written to tokens_out[b] and to
 * history[step_ptr[0]*hist_stride + b]; the token's embedding row is gathered into x_next [batch, d];
 * ctx_len[b] += 1; step_ptr[0] += 1 (by a trailing 1-thread kernel).  Sequences with finished[b] != 0 emit pad_id; a
 * sequence becomes finished when it emits one of eos[0..n_eos).  */
int kr_argmax_embed(const float* logits, int64_t ld_logits, int vocab,
                    const kr_bf16* embed_table, int d,
                    int32_t* tokens_out, int32_t* history, int32_t* step_ptr, int32_t* ctx_len,
                    int32_t* finished, const int32_t* eos, int n_eos, int pad_id, int ignore_eos,
                    kr_bf16* x_next, int batch, int hist_stride, kr_stream s);

/* Plain argmax (SURVEY §8 b2 `kr_argmax`). */
int kr_argmax(const float* logits, int64_t ld_logits, int vocab, int32_t* out, int batch, kr_stream s);

/* ------------------------------------------------------------------ fused decode step (5 launches per layer + 2)
 * Decode linears over PACKED weights: W[N][K] stored as [N/16][K/32][4][16][8] bf16 (element
 * (n, k) at ((((n/16)*(K/32) + k/32)*4 + (k%32)/8)*16 + n%16)*8 + k%8): one (16 x 32) block is an
 * MFMA fragment set in lane order, so the matrix is read from HBM as one linear stream, 1 KiB of
 * contiguous memory per wave-level load.  y[M<=16, N] = epi(x W^T).  K is split over the `waves` (4, 8 or 16) waves of a
 * workgroup.  max_blocks > 0 (and ksplit == 1): at most that many PERSISTENT workgroups walk the
 * 16-row tile groups (the prologue runs once per workgroup, the next group's weights are put in
 * flight before the current group's reduction); 0 = one workgroup per tile group.
 * ksplit > 1 additionally splits K over workgroups with a deterministic in-launch
 * reduction (ws: f32 [N/16][ksplit][256] slabs, counters: int32 [N/16], zero-initialised, left
 * zero).  Prologues: Qwen2VLRMSNorm on x (norm_w, K <= 4096), or x = merge of the decode
 * attention partials (attn_partials [M][K/128][attn_split][hd+4] f32 as kr_attn_decode_fused
 * leaves them with out == NULL; x itself may then be NULL).
 * mode 0 PLAIN   : +bias, +residual, bf16 `out` or fp32 `out_f32` [M, ldc]      (o_proj, down_proj)
 *      1 SILU    : silu(gate)*up, rows interleaved in 16-row groups, out [M, N/2] (gate/up)
 *      2 ROPE_KV : fused q/k/v projection (+bias) -> M-RoPE -> q_out [M, heads, 128]; k -> kcache
 *                  row ctx_len[b]; v -> vtcache column ctx_len[b] (cache pointers = this layer's
 *                  base, layout as kr_decode_qkv_prep).  cos/sin come from cs_table
 *                  [M][cs_stride][128] fp32 (cos[0..64), sin[0..64)), entry ctx_len[b] -
 *                  prompt_len[b] = index of the decode position.  head_dim 128 only.
 *                  (TF:469-556, :180-222)
 *      3 ARGMAX  : lm_head: per-workgroup (max, lowest index) partials amax_val/amax_idx
 *                  [M][ceil(N/32)]; fp32 logits also written when out_f32 != NULL   (TF:1320-1323) */
#define KR_DEC_PLAIN 0
#define KR_DEC_SILU 1
#define KR_DEC_ROPE_KV 2
#define KR_DEC_ARGMAX 3
#define KR_DEC_SILU8 4      /* SILU with 8-row interleave: one tile per workgroup -> 2x the workgroups of KR_DEC_SILU */
#define KR_DEC_OUT_XP 0x100 /* kr_linear_decode_wide*, OR-ed into KR_DEC_SILU8 at 17..32 rows: `out` is written in the packed
                             * activation layout of kr_pack_rows32 (ldc ignored) — the input format of kr_linear_decode32 */
#define KR_DEC_OUT_XP16 0x200 /* the same at <= 16 rows: `out` is written in the XP16 layout (below, kr_narrow_opts.x_packed; ldc
                               * ignored; N/2 * 32 bytes) — the x operand of the down_proj launch kr_linear_decode_narrow */
int kr_linear_decode(int mode, const kr_bf16* x, int64_t ldx, const kr_bf16* w_packed, const kr_bf16* bias,
                     const kr_bf16* norm_w, float norm_eps, const kr_bf16* residual, int64_t ldr,
                     kr_bf16* out, float* out_f32, int64_t ldc, int M, int N, int K, int waves, int max_blocks, int ksplit,
                     float* ws, int32_t* counters, const float* attn_partials, int attn_split,
                     const float* cs_table, int cs_stride, const int32_t* prompt_len, const int32_t* ctx_len,
                     kr_bf16* q_out, kr_bf16* kcache, kr_bf16* vtcache, int heads, int kv_heads, int s_max,
                     float* amax_val, int32_t* amax_idx, kr_stream s);

/* Wide decode linears (gate/up, lm_head): one WAVE per 16-row weight tile over the full K — no cross-wave
 * reduction and no barrier after the prologue; an 8-deep register ring streams on across tile boundaries
 * (K % 512 == 0, K <= 4096).  `blocks` workgroups of `waves` (<= 8) waves; wave (b, w) walks tiles
 * b + blocks*(w + waves*i).  Modes PLAIN / SILU8 / ARGMAX as kr_linear_decode; ARGMAX partials are per
 * wave: amax_val / amax_idx [M][blocks*waves], slot b + blocks*w (value -inf, index INT_MAX for a wave
 * without tiles). */
int kr_linear_decode_wide(int mode, const kr_bf16* x, int64_t ldx, const kr_bf16* w_packed, const kr_bf16* bias,
                          const kr_bf16* norm_w, float norm_eps, const kr_bf16* residual, int64_t ldr,
                          kr_bf16* out, float* out_f32, int64_t ldc, int M, int N, int K, int blocks, int waves,
                          float* amax_val, int32_t* amax_idx, kr_stream s);

/* Options of one narrow launch (NULL = all zero).  They replace round 2's thread-local one-shot setters
 * (kr_decode_slab_next / kr_decode_part_rows_next): nothing about a launch is decided by an earlier call.
 *   atomic_out != 0 : a ksplit == 2 launch ADDS its two K ranges into ONE f32 slab out_f32 [M][ldc] with float atomics
 *                     instead of writing two slabs (the ONE-slab form of the deferred split-K between a layer's down_proj
 *                     and the next layer's qkv prologue).  The slab must hold zeros; two addends onto zero give the same
 *                     bits in either arrival order, so the path stays reproducible.  The consumer passes it as part_in
 *                     with n_part_in = 1 and reads half the slab bytes in every workgroup's prologue.
 *   zero_ptr, zero_bytes : the launch also zeroes that f32 range (16-byte aligned, a multiple of 16 bytes): the engine
 *                     lets layer L's qkv launch zero the slab layer L's down_proj will add into.
 *   part_rows       : the part_in slabs have `part_rows` rows each ([n_part_in][part_rows][K]) instead of M — the launch
 *                     covers a row range of a larger batch whose down_proj wrote the slabs (decode batches above 16 rows
 *                     at the 7B width run the norm-prologue launches once per 16-row range).  0: = M.
 *   w_resident != 0 : the launch loads its weights with the default cache policy instead of nontemporal loads, so their
 *                     lines stay in the 256 MiB Infinity Cache for the next call on the same weights (the other launches'
 *                     nontemporal streams do not displace them: profiles/r05_ic_residency.txt).  The caller keeps the sum of
 *                     the weights it marks below the cache size.  Same bytes loaded, same output bits.
 *   x_packed != 0   : x is not a row-major tensor but an XP16 buffer: the packed activation layout below restricted to one
 *                     column tile of R row slots, R = 8 for M <= 8 and 16 above:
 *                     [K/64 chunks][2 k-steps of 32][4 groups of 8 k][R rows][8] bf16, element (row b, column k) at byte
 *                     (k/64)*R*128 + (k/32 % 2)*R*64 + (R*(k/8 % 4) + b)*16 + (k%8)*2.  The buffer is K * 32 bytes whatever M
 *                     is.  KR_DEC_PLAIN without norm_w (o_proj, down_proj), M <= 16; ldx is not used.  A wave then fetches the
 *                     operand of an MFMA as R * 64 bytes of whole cache lines instead of 16 rows x 64 B (at 8 live rows:
 *                     eight half lines).  The same values enter the same MFMAs: the output bits are those of the row-major
 *                     launch.  Row slots >= M are read and never used (they reach accumulator columns the epilogue drops),
 *                     so they may hold anything.  Producers, with the same M: kr_attn_decode_merge16,
 *                     kr_linear_decode_wide(KR_DEC_SILU8 | KR_DEC_OUT_XP16). */
typedef struct kr_narrow_opts {
    float* zero_ptr;
    uint64_t zero_bytes;
    int32_t atomic_out;
    int32_t part_rows;
    int32_t w_resident;
    int32_t x_packed;
} kr_narrow_opts;

/* Narrow decode linears (qkv, o_proj, down_proj): one workgroup per 16-row tile (ROPE_KV: per rotary tile
 * pair), K split over its `waves` (8 or 16; the norm prologue always runs 8) waves; x / norm weight / epilogue
 * operands are requested before the weights.  Modes PLAIN and ROPE_KV as kr_linear_decode.  ROPE_KV with norm_w ==
 * NULL: x is already normalised (kr_decode_resnorm) and its fragments are read straight from L2 (M up to 32, 8 waves).
 *   ksplit > 1 (PLAIN only): K is also split over `ksplit` workgroups and the reduction is DEFERRED: out_f32
 *     receives f32 slabs [ksplit][M][ldc] (no bias / residual / norm) — or, with opts->atomic_out, one slab the
 *     K ranges add into; the consumer adds them.
 *   part_in (with norm_w): n_part_in (1 or 2) slabs [n][M][K] f32 are added to x in the prologue,
 *     x_new = bf16(x + sum of slabs) is RMS-normalised and, by workgroup 0, stored to x_out (ldxo), which
 *     must not alias x (other workgroups still read x).  K must be 1536, 2048 or 3584 for this. */
int kr_linear_decode_narrow(int mode, const kr_bf16* x, int64_t ldx, const float* part_in, int n_part_in,
                            kr_bf16* x_out, int64_t ldxo, const kr_bf16* w_packed, const kr_bf16* bias,
                            const kr_bf16* norm_w, float norm_eps, const kr_bf16* residual, int64_t ldr,
                            kr_bf16* out, float* out_f32, int64_t ldc, int M, int N, int K, int waves, int ksplit,
                            const float* cs_table, int cs_stride, const int32_t* prompt_len, const int32_t* ctx_len,
                            kr_bf16* q_out, kr_bf16* kcache, kr_bf16* vtcache, int heads, int kv_heads, int s_max,
                            const kr_narrow_opts* opts, kr_stream s);

/* Residual sum + RMSNorm ONCE for a decode batch (the form of batches above 16 rows):
 *   x_new = bf16(x + part_in[0] + part_in[1] + ...)  (n_part_in slabs [n][part_rows][K] f32, in that order; part_rows 0 = M),
 *   stored to x_out (ldxo; must not alias x; untouched when n_part_in == 0), and
 *   h = norm_w * bf16(x_new * rsqrt(mean(x_new^2) + eps))  (Qwen2VLRMSNorm, TF:96-110) stored to h [M, ldh].
 * One wave per row with the narrow NORM kernel's summation structure: the rows are bit-identical to the ones
 * kr_linear_decode_narrow's fused prologue computes, so kr_linear_decode_narrow(ROPE_KV, x = h, norm_w = NULL) — x fragments
 * straight from L2, no per-workgroup staging of 32 rows and their slabs — gives the fused launch's q / K / V bits. */
int kr_decode_resnorm(const kr_bf16* x, int64_t ldx, const float* part_in, int n_part_in, int part_rows, kr_bf16* x_out,
                      int64_t ldxo, const kr_bf16* norm_w, float norm_eps, kr_bf16* h, int64_t ldh, int M, int K, kr_stream s);

/* The same two kernels on fp8 (OCP e4m3fn) weights — BASELINE.json config 5: decoder Linears in fp8 with one f32 scale
 * per output row, activations bf16.  w_packed_fp8 = weights.pack_w16x64_fp8 (one 16-row x 64-column block = 1 KiB in
 * lane order: half the bytes per launch), converted to bf16 in registers (exact) and fed to the bf16 MFMA; w_scale
 * [N] (in the row order of the packed matrix, i.e. interleaved like the rows for SILU8) multiplies the f32
 * accumulators before bias / activation / rotary / slab store.  Everything else as the bf16 entry points. */
int kr_linear_decode_wide_fp8(int mode, const kr_bf16* x, int64_t ldx, const uint8_t* w_packed_fp8, const float* w_scale,
                              const kr_bf16* bias, const kr_bf16* norm_w, float norm_eps, const kr_bf16* residual,
                              int64_t ldr, kr_bf16* out, float* out_f32, int64_t ldc, int M, int N, int K, int blocks,
                              int waves, float* amax_val, int32_t* amax_idx, kr_stream s);
int kr_linear_decode_narrow_fp8(int mode, const kr_bf16* x, int64_t ldx, const float* part_in, int n_part_in,
                                kr_bf16* x_out, int64_t ldxo, const uint8_t* w_packed_fp8, const float* w_scale,
                                const kr_bf16* bias, const kr_bf16* norm_w, float norm_eps, const kr_bf16* residual,
                                int64_t ldr, kr_bf16* out, float* out_f32, int64_t ldc, int M, int N, int K, int waves,
                                int ksplit, const float* cs_table, int cs_stride, const int32_t* prompt_len,
                                const int32_t* ctx_len, kr_bf16* q_out, kr_bf16* kcache, kr_bf16* vtcache, int heads,
                                int kv_heads, int s_max, const kr_narrow_opts* opts, kr_stream s);
/* ---- decode batches of 17..32 rows (two 16-row MFMA column tiles): the continuous server's steady state and BASELINE
 * config 3's 32-rows-per-GPU variant (the callers: bulk_processing/workers/inference_worker.py:331-339, one in-flight
 * request per worker x workers per port).
 *
 * PACKED ACTIVATIONS ("XP").  The input of a decode linear at more than 16 rows is stored
 *     [K/64 chunks][2 column tiles][2 k-steps of 32][64 lanes = 16 * (k/8 % 4) + row % 16][8] bf16      (4 KiB per chunk)
 * i.e. element (row b, column k) at byte (k/64)*4096 + (b/16)*2048 + (k/32 % 2)*1024 + (16*(k/8 % 4) + b%16)*16 + (k%8)*2:
 * the operand of one v_mfma_f32_16x16x32_bf16 is 1 KiB of contiguous memory in lane order, so a wave fetches it as eight
 * whole cache lines (row-major x costs sixteen half lines per fragment, and at two column tiles a wave moves twice as many
 * x bytes from L2 as weight bytes from HBM).  Producers: kr_pack_rows32 (from row-major rows; rows >= M are zero),
 * kr_decode_resnorm32, kr_attn_decode_merge32, kr_linear_decode_wide(KR_DEC_SILU8 | KR_DEC_OUT_XP).  A buffer holds 32 rows
 * whatever M is: K * 64 bytes. */
int kr_pack_rows32(const kr_bf16* x, int64_t ldx, int M, int K, kr_bf16* xp, kr_stream s);

/* kr_linear_decode_narrow's contract (modes KR_DEC_PLAIN and KR_DEC_ROPE_KV, bf16 or fp8 weights, deferred split-K into
 * f32 slabs or one atomically accumulated slab, the zeroing job) for M <= 32 on packed activations, WITH THE NARROW LAUNCH'S
 * SUMMATION ORDER: `waves_ref` and `ksplit` name the K partition the <= 16-row launch of the same layer uses (its `waves`
 * and `ksplit` arguments) — the same chunk ranges accumulated from zero in ascending k, folded in the same order — so row b
 * of the result has the bits kr_linear_decode_narrow gives for that row alone: a page's tokens do not depend on its batch.
 * 8-wave workgroups; a 16-wave partition runs as two ranges per wave.  tiles_per_wg: 0 = automatic (two weight tiles share
 * one ring of x fragments where that leaves >= 192 workgroups), 1, 2 (4 with group_split).  No norm prologue: x is kr_decode_resnorm32's output. */
typedef struct kr_dec32 {
    const kr_bf16* xp;            /* packed activations, K * 64 bytes */
    const void* w_packed;         /* weights.pack_w16x32 (bf16) or pack_w16x64_fp8 (with w_scale) */
    const float* w_scale;         /* fp8 weights: one f32 per output row; NULL for bf16 */
    const kr_bf16* bias;          /* [N] or NULL (ROPE_KV: required) */
    const kr_bf16* residual;      /* PLAIN: [M, ldr] or NULL */
    int64_t ldr;
    kr_bf16* out;                 /* PLAIN: bf16 [M, ldc] ... */
    float* out_f32;               /* ... or f32 [M, ldc]; ksplit > 1: slabs [ksplit][M][ldc], or one slab with atomic_out */
    int64_t ldc;
    int32_t M, N, K;
    int32_t waves_ref, ksplit;    /* the <= 16-row launch's K partition */
    int32_t atomic_out;           /* ksplit == 2: both K ranges ADD into out_f32 (zeroed by an earlier launch) */
    int32_t tiles_per_wg;
    int32_t group_split;          /* atomic_out, ksplit 2, bf16 weights: each K range's atoms in TWO workgroups (first / second half
                                   * of the partition), each adding its half's fold into slab [ks] of out_f32 = [2][M][ldc]: the slab
                                   * holds (half 0) + (half 1) = the narrow launch's fold of that range, and the consumer adds
                                   * x + (slab 0 + slab 1) (kr_decode_resnorm32, sum_slabs_first) = x + the narrow launch's one slab.
                                   * Twice the weight tiles per workgroup at the same number of workgroups: half the x bytes */
    int32_t reserved0;
    float* zero_ptr;              /* this launch also zeroes [zero_ptr, zero_ptr + zero_bytes) (16-byte multiples) */
    uint64_t zero_bytes;
    /* KR_DEC_ROPE_KV (as kr_linear_decode): */
    const float* cs_table; int32_t cs_stride; const int32_t* prompt_len; const int32_t* ctx_len;
    kr_bf16* q_out; kr_bf16* kcache; kr_bf16* vtcache; int32_t heads, kv_heads, s_max;
} kr_dec32;
int kr_linear_decode32(int mode, const kr_dec32* args, kr_stream s);

/* kr_decode_resnorm with h written in the packed layout (h_xp: K * 64 bytes); x_out stays row-major.  sum_slabs_first
 * (n_part_in == 2): x + (slab 0 + slab 1) instead of (x + slab 0) + slab 1 — the slabs of a group_split down_proj. */
int kr_decode_resnorm32(const kr_bf16* x, int64_t ldx, const float* part_in, int n_part_in, int part_rows, kr_bf16* x_out,
                        int64_t ldxo, const kr_bf16* norm_w, float norm_eps, kr_bf16* h_xp, int M, int K, int sum_slabs_first,
                        kr_stream s);

/* n fp8 e4m3fn codes -> bf16 through the hardware conversion the kernels use (test hook: pins the number format). */
int kr_fp8_to_bf16(const uint8_t* src, kr_bf16* dst, int64_t n, kr_stream s);

/* Decode attention (q_len 1, GQA, MFMA, split over n_split key ranges), kcache / vtcache = the
 * layer's base pointers.  workspace: fp32 [batch*heads][n_split][hd+4] partials (o[hd], m, l, 2 pad: 16-byte aligned records).
 * out == NULL (the product path): only the partials are produced; kr_attn_decode_merge (or kr_linear_decode's
 * attn_partials prologue) merges them.  out != NULL with n_split == 1: the single range is written as bf16
 * [batch, heads*hd].  out != NULL with n_split > 1 — the in-launch merge by the last-arriving workgroup (counters:
 * int32 [batch*kv_heads], zero-initialised, left zero), measured slower than the merge launch — exists in experiment
 * builds only (-DKR_EXPERIMENTS, include/karanta_hip_experiments.h) and is refused otherwise. */
int kr_attn_decode_fused(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache,
                         const int32_t* ctx_len, kr_bf16* out, float* workspace, int32_t* counters,
                         int batch, int heads, int kv_heads, int hd, int s_max, int n_split,
                         float scale, kr_stream s);
/* The serving form: kr_attn_decode_fused(out = NULL) for a batch of decode SLOTS — the workgroups of a slot whose `finished` flag
 * is set (EOS seen by kr_sample_greedy, or retired by the host: an idle slot of the continuous server,
 * bulk_processing/workers/inference_worker.py:331-339 keeps the slots filled one request at a time) return at once and leave its
 * partials as they were; nothing downstream consumes a finished row.  Live rows: the same partials, bit for bit. */
int kr_attn_decode_slots(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache, const int32_t* ctx_len,
                         const int32_t* finished, float* workspace, int batch, int heads, int kv_heads, int hd, int s_max,
                         int n_split, float scale, kr_stream s);

/* Merge of the partials kr_attn_decode_fused leaves with out == NULL into bf16 out [batch, heads*hd]
 * (one small launch; the alternative to merging inside the consumer's prologue). */
int kr_attn_decode_merge(const float* workspace, kr_bf16* out, int batch, int heads, int hd, int n_split,
                         kr_stream s);

/* kr_attn_decode_merge with the merged heads written in the packed activation layout (row = sequence, column =
 * head * 128 + d; batch <= 32; out_xp: heads * 128 * 64 bytes) — the o_proj launch of a 17..32-row batch reads it. */
int kr_attn_decode_merge32(const float* workspace, kr_bf16* out_xp, int batch, int heads, int hd, int n_split,
                           kr_stream s);

/* The same for batch <= 16 in the XP16 layout at M = batch (kr_narrow_opts.x_packed; out_xp16: heads * 128 * 32 bytes; row
 * slots >= batch are not written) — the o_proj launch of a <= 16-row batch reads it.  One kernel body with the two above. */
int kr_attn_decode_merge16(const float* workspace, kr_bf16* out_xp16, int batch, int heads, int hd, int n_split,
                           kr_stream s);

/* GPU image front end.  kr_image_resize_bicubic_u8: HWC uint8 RGB [h][w][3] -> [rh][rw][3], bit-identical to
 * PIL's Image.resize(..., BICUBIC) (the HF PIL processor's resize, image_processing_pil_qwen2_vl.py:126-150):
 * horizontal pass then vertical pass of Pillow's 8-bit resample with the host-built integer tables
 * (image_processing.resample_tables: bounds [out][2] = (first input index, taps), coeffs [out][ksize], 22
 * fractional bits); an axis whose size does not change is skipped (tables may be NULL), tmp [h][rw][3] is needed
 * when both change.  kr_image_normalize_patchify: x/255 -> (x - mean) / std in fp32 (mean3 / std3 are HOST
 * arrays of 3 floats) written as pixel_values [gh*gw][3*temporal*patch*patch] in the processor's patch order
 * (:152-187, :226-229). */
int kr_image_resize_bicubic_u8(const uint8_t* src, int h, int w, uint8_t* dst, int rh, int rw, uint8_t* tmp,
                               const int32_t* h_bounds, const int32_t* h_coeffs, int h_ksize,
                               const int32_t* v_bounds, const int32_t* v_coeffs, int v_ksize, kr_stream s);
int kr_image_normalize_patchify(const uint8_t* img, int rh, int rw, const float* mean3, const float* std3,
                                int patch, int merge, int temporal, float* out, kr_stream s);

/* Temperature sampling as an argmax (Gumbel-max): per row b, partial argmax over n_part vocabulary slices of
 * logits[b][i] / T_b + G(seed_b, n_b, i), n_b = ctx_len[b] + 1 - prompt_len[b] (index of the token being
 * generated), G = -ln(-ln(u)) from a counter-based hash (definition in kr_sample.hip, restated in the oracle);
 * T_b == 0: plain argmax.  Writes amax_val / amax_idx [batch][n_part] for kr_sample_greedy, replacing the
 * greedy partials of the lm_head.  Replaces vLLM's sampler for requests with temperature > 0
 * (/root/reference/karanta/pipeline.py:281,301; bulk_processing/workers/vllm_client.py:155). */
int kr_gumbel_argmax(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                     const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len, float* amax_val,
                     int32_t* amax_idx, int n_part, int batch, kr_stream s);

/* ------------------------------------------------------------------ guided decoding + log-probabilities
 * Replaces vLLM's guided-decoding logits processor and its logprobs output for the requests the reference sends:
 * `guided_regex` (/root/reference/karanta/pipeline.py:304-307), `response_format` json_schema
 * (/root/reference/karanta/data/utils.py:322-440, bulk_processing/workers/vllm_client.py:196), `logprobs` /
 * `top_logprobs` (/root/reference/karanta/data/create_batch_data_prompts.py:117-118).  The host compiles the pattern
 * to a byte DFA (state 0 = dead; karanta_ocr_amd/guided.py); per token everything stays on the device.
 *
 * kr_guide_build_masks: masks[s][w] bit j = token 32*w+j allowed in DFA state s <=> the token has bytes and walking
 * them from s through trans[state][byte] (uint16, [n_states][256]) never reaches state 0; a token listed in eos is
 * allowed exactly where accept[s] != 0.  vocab_off [vocab+1] / vocab_bytes: the byte string of every token id.
 * mask_words: words per row, even, mask_words * 32 >= vocab. */
int kr_guide_build_masks(const uint16_t* trans, const uint8_t* accept, int n_states, const int32_t* vocab_off,
                         const uint8_t* vocab_bytes, int vocab, const int32_t* eos, int n_eos, uint32_t* masks,
                         int mask_words, kr_stream s);

/* kr_gumbel_argmax with a token mask per row: guide_masks[b] = device address (as an integer) of the mask table of
 * row b's pattern (0: row unconstrained), guide_state[b] its current DFA state; tokens whose bit is clear do not
 * take part.  guide_masks == NULL: identical to kr_gumbel_argmax.  fallback_token: what a row with no allowed token
 * yields (cannot happen in a live state; keeps the token id valid). */
int kr_gumbel_argmax_guided(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                            const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len, float* amax_val,
                            int32_t* amax_idx, int n_part, int batch, const uint64_t* guide_masks,
                            const int32_t* guide_state, int mask_words, int fallback_token, kr_stream s);

/* ------------------------------------------------------------------ sampling controls (vLLM's top_k / top_p / min_p and
 * repetition / frequency / presence penalties).  Per row b, params[b * 8 + j]: j = 0 top_k (<= 0: off), 1 top_p (>= 1: off),
 * 2 min_p (<= 0: off), 3 repetition_penalty (1: off), 4 frequency_penalty, 5 presence_penalty (0: off), 6-7 unused.
 * counts [batch][ld_counts]: how often each token occurs in the row's output so far (kr_sample_count);
 * prompt_bits [batch][bits_words]: bit i set <=> token i occurs in the row's prompt.  The score of an allowed token
 * (guide mask as in kr_gumbel_argmax_guided) is v = l' * (1 / T) with l' = the logit after the penalties, in fp32:
 * l' = (in prompt or c > 0) ? (l > 0 ? l / r : l * r) : l, then l' -= f * c + p * (c > 0).  Logits are read, never written.
 *
 * kr_sample_threshold: per row with T > 0 and any truncation on, threshold[b] = the order-preserving key
 * (sign-flipped float bits) of the smallest kept score: the largest of v_max + ln(min_p), the top_k-th largest v (ties kept)
 * and the top_p cut (the v of the first token, by descending v, at which the cumulative probability of what min_p / top_k
 * kept reaches top_p; ties kept).  0: keep every allowed token (T == 0 or neutral truncation).  Deterministic (integer
 * histograms).  work [batch][ld_work] fp32 is scratch.  live[b] = whether this step appends a real token to row b
 * (ignore_eos bit 0 set or finished[b] == 0): what kr_sample_count counts after kr_sample_greedy. */
int kr_sample_threshold(const float* logits, int64_t ld_logits, int vocab, const float* temperature, const float* params,
                        const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                        const uint64_t* guide_masks, const int32_t* guide_state, int mask_words, const int32_t* finished,
                        int ignore_eos, float* work, int64_t ld_work, uint32_t* threshold, int32_t* live, int batch,
                        kr_stream s);

/* kr_gumbel_argmax_guided over the penalised scores, restricted to the tokens whose score key is >= threshold[b] (rows
 * with T > 0; a T == 0 row is the plain argmax of l').  Same [batch][n_part] partials for kr_sample_greedy; a row with
 * neutral params gets the partials of kr_gumbel_argmax_guided bit for bit. */
int kr_gumbel_argmax_processed(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                               const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len, float* amax_val,
                               int32_t* amax_idx, int n_part, int batch, const uint64_t* guide_masks,
                               const int32_t* guide_state, int mask_words, int fallback_token, const float* params,
                               const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                               const uint32_t* threshold, kr_stream s);

/* After kr_sample_greedy: counts[b][tokens[b]] += 1 for the rows with live[b] != 0 (kr_sample_threshold of this step). */
int kr_sample_count(const int32_t* tokens, const int32_t* live, int32_t* counts, int64_t ld_counts, int vocab, int batch,
                    kr_stream s);

/* The two launches above over the rows of a speculative step (kr_spec).  Row r belongs to slot row_slot[r] (clamped to
 * 0..slots-1) and depth[r] drafts of that slot lie in front of it (kr_spec_controls_rows; clamped to 0..k): params, counts and
 * prompt_bits are read at the SLOT, [slots] rows of them, and the count of token i is counts[slot][i] + #{e < depth[r] :
 * draft_tok[slot * k + e] == i} — the output so far of a row whose drafts were all accepted.  Everything else is per row, `batch` =
 * rows entries: logits, temperature, seed, ctx_len, prompt_len, guide_masks / guide_state, finished, work, threshold, live and the
 * partials.  The contract of a row is equality: threshold, partials (value bits and index) are those of kr_sample_threshold /
 * kr_gumbel_argmax_processed on a one-row batch that holds the slot's params and prompt bits and the counts above; a row at depth 0
 * or of a slot without penalties never looks at draft_tok.  1 <= slots <= batch <= 32, 1 <= k < 32. */
int kr_sample_threshold_rows(const float* logits, int64_t ld_logits, int vocab, const float* temperature, const float* params,
                             const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                             const uint64_t* guide_masks, const int32_t* guide_state, int mask_words, const int32_t* finished,
                             int ignore_eos, float* work, int64_t ld_work, uint32_t* threshold, int32_t* live, int batch,
                             const int32_t* row_slot, const int32_t* depth, const int32_t* draft_tok, int k, int slots, kr_stream s);
int kr_gumbel_argmax_processed_rows(const float* logits, int64_t ld_logits, int vocab, const float* temperature,
                                    const uint32_t* seed, const int32_t* ctx_len, const int32_t* prompt_len, float* amax_val,
                                    int32_t* amax_idx, int n_part, int batch, const uint64_t* guide_masks,
                                    const int32_t* guide_state, int mask_words, int fallback_token, const float* params,
                                    const int32_t* counts, int64_t ld_counts, const uint32_t* prompt_bits, int bits_words,
                                    const uint32_t* threshold, const int32_t* row_slot, const int32_t* depth,
                                    const int32_t* draft_tok, int k, int slots, kr_stream s);

/* ------------------------------------------------------------------ per-request logit adjustments (vLLM's logit_bias,
 * min_tokens and stop_token_ids).  Per row b a table of adj_meta[b * 4 + 0] = n_entries <= KR_ADJ_CAP entries, every token id
 * at most once in a row (the host merges bias keys, stop ids and the model's EOS ids); entry e of row b, at
 * [b * KR_ADJ_CAP + e]: adj_ids (token id), adj_val (the bias, fp32, 0 where none; -inf allowed), adj_flag (bit 0 = stop
 * entry: one of the row's stop_token_ids or an EOS id).  adj_meta[b * 4 + 1] = min_tokens, [2..3] unused.  n_entries above
 * KR_ADJ_CAP counts as KR_ADJ_CAP and an id outside [0, vocab) is skipped.  vLLM's order: these run on the lm_head's fp32
 * logits BEFORE the penalties, temperature and truncation of the sampler; log-probabilities and returned logits stay raw.
 *
 * kr_logits_adjust: saved[b][e] = logits[b][id]; then, with n = ctx_len[b] + 1 - prompt_len[b] (the index of the token being
 * generated, as in kr_gumbel_argmax): logits[b][id] = -inf on a stop entry while n < min_tokens (the mask wins over a bias,
 * nothing is masked at n == min_tokens), else logits[b][id] + adj_val in fp32.  Rows with n_entries == 0 are not touched.
 * saved [batch][KR_ADJ_CAP] fp32 belongs to the step: kr_logits_restore reads it. */
#define KR_ADJ_CAP 320   /* OpenAI's 300 logit_bias entries + 16 stop ids + the EOS ids */
int kr_logits_adjust(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const float* adj_val,
                     const int32_t* adj_flag, const int32_t* adj_meta, const int32_t* ctx_len, const int32_t* prompt_len,
                     float* saved, int batch, kr_stream s);

/* kr_logits_adjust over the rows of a speculative step: row r is adjusted with the table of slot row_slot[r] (clamped to
 * 0..slots-1; the tables hold [slots] rows) at the row's own n = ctx_len[r] + 1 - prompt_len[r]; logits, ctx_len, prompt_len and
 * saved are per row (`batch` = rows entries).  The adjusted row equals kr_logits_adjust's on a one-row batch with that table.  A
 * speculative step that records nothing has no restore launch: nothing reads the logits behind the token choice there and the
 * next lm_head launch overwrites them; one that records log-probabilities puts them back with kr_logits_restore_rows. */
int kr_logits_adjust_rows(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const float* adj_val,
                          const int32_t* adj_flag, const int32_t* adj_meta, const int32_t* ctx_len, const int32_t* prompt_len,
                          float* saved, int batch, const int32_t* row_slot, int slots, kr_stream s);

/* After the sampler: logits[b][id] = saved[b][e] for every entry — the buffer equals what the lm_head wrote, bit for bit
 * (kr_logprobs_topk and returned logits report the unadjusted values). */
int kr_logits_restore(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const int32_t* adj_meta,
                      const float* saved, int batch, kr_stream s);

/* kr_logits_restore over the rows of a speculative step, the inverse of kr_logits_adjust_rows: logits[r][id] = saved[r][e] for
 * every entry of the table of slot row_slot[r] (clamped to 0..slots-1; n_entries and ids clamped / skipped as there), so the buffer
 * equals what the lm_head wrote, bit for bit, on every row — kr_logprobs_topk_rows reports the unadjusted values, as
 * kr_logprobs_topk does in a plain step.  1 <= slots <= batch <= 32. */
int kr_logits_restore_rows(float* logits, int64_t ld_logits, int vocab, const int32_t* adj_ids, const int32_t* adj_meta,
                           const float* saved, int batch, const int32_t* row_slot, int slots, kr_stream s);

/* After kr_sample_greedy: finished[b] = 1 where the row was still live (finished[b] == 0: it appended a sampled token, not a
 * pad) and tokens[b] is one of its stop entries — from here on the row is what an EOS row is (frozen in slot mode, no
 * log-prob for the finishing step).  ignore_eos bit 0 (kr_sample_greedy's): nothing finishes. */
int kr_stop_tokens(const int32_t* tokens, const int32_t* adj_ids, const int32_t* adj_flag, const int32_t* adj_meta,
                   int32_t* finished, int ignore_eos, int batch, kr_stream s);

/* After the sampler: guide_state[b] <- walk(guide_state[b], bytes(tokens[b])) through the table at device address
 * guide_trans[b] (0: row unconstrained); rows with finished[b] != 0 keep their state. */
int kr_guide_advance(const int32_t* tokens, const int32_t* finished, const uint64_t* guide_trans, int32_t* guide_state,
                     const int32_t* vocab_off, const uint8_t* vocab_bytes, int vocab, int batch, kr_stream s);

/* Log-probabilities of one decode step from the fp32 logits [batch][ld_logits] (log-softmax over the vocabulary,
 * unscaled and unmasked): out_lp[h][b][0] = log p(tokens[b]), out_lp[h][b][1 + j] / out_idx[h][b][j] = the j-th most
 * probable token (ties: lowest id), j < k <= 20, rows strided by hist_batch * (1 + k_stride) / hist_batch * k_stride;
 * h = ctx_len[b] - prompt_len[b] as left by kr_sample_greedy (the token-history index); rows with finished[b] != 0
 * record nothing.  part_val / part_idx [batch][n_part][k] and part_ms [batch][n_part][2] are scratch;
 * ceil(vocab / n_part) <= 4096, n_part <= 1024 and n_part * max(k, 1) * 8 <= 159 KiB (the merge's candidate table in LDS). */
int kr_logprobs_topk(const float* logits, int64_t ld_logits, int vocab, int k, int n_part, float* part_val,
                     int32_t* part_idx, float* part_ms, const int32_t* tokens, const int32_t* ctx_len,
                     const int32_t* prompt_len, const int32_t* finished, float* out_lp, int32_t* out_idx, int hist_len,
                     int hist_batch, int k_stride, int batch, kr_stream s);

/* Fork of prefilled KV-cache slots (n > 1 of a request, a repeated page): for every group of the plan, every layer and KV head,
 * rows [0, n_tokens) of kcache and V^T blocks [0, ceil(n_tokens / 64)) of vtcache are copied from slot `src` to each slot of
 * `dst`.  The partial last V^T block is copied whole: a decode step appends column by column into it, and its columns at or
 * beyond n_tokens are masked by ctx_len.  Nothing else is written: destination rows / blocks beyond the span, the other slots
 * and the sources keep their bytes.  One launch; a source piece (64 tokens of one head: hd x 128 bytes) is loaded once and
 * stored to every destination of its group.
 * The caches arrive as explicit ELEMENT strides of (layer, slot, head); a head holds [s_max][hd] (kcache) or
 * [s_max / 64][2][hd][32] (vtcache) contiguously; all offsets are 64-bit.  hd % 8 == 0, s_max % 64 == 0, 1 <= slots <= 32,
 * strides multiples of 8 and at least the extent below them.
 * `plan` is HOST memory, read during the call only and carried in the kernel arguments (no device table, copy or allocation).
 * KR_ERR_ARG, and nothing launches: a slot outside [0, slots), n_tokens outside [1, s_max], a destination listed twice (in any
 * group), a destination equal to any group's source, a group without destinations, n_groups outside [1, 32]. */
#define KR_FORK_MAX_GROUPS 32
#define KR_FORK_MAX_SLOTS 32
typedef struct kr_fork_group {
    int32_t src;                       /* source slot */
    int32_t n_tokens;                  /* prompt length: rows [0, n_tokens) */
    int32_t n_dst;                     /* 1 .. KR_FORK_MAX_SLOTS */
    int32_t dst[KR_FORK_MAX_SLOTS];    /* destination slots */
} kr_fork_group;
typedef struct kr_fork_plan {
    int32_t n_groups;                  /* 1 .. KR_FORK_MAX_GROUPS */
    kr_fork_group groups[KR_FORK_MAX_GROUPS];
} kr_fork_plan;
int kr_kv_fork(kr_bf16* kcache, kr_bf16* vtcache, int64_t k_layer_stride, int64_t k_slot_stride, int64_t k_head_stride,
               int64_t vt_layer_stride, int64_t vt_slot_stride, int64_t vt_head_stride, int layers, int kv_heads, int hd,
               int slots, int s_max, const kr_fork_plan* plan, kr_stream s);

/* ------------------------------------------------------------------ fp8 (e4m3fn) KV cache
 * The same logical layout as the bf16 cache with one byte per element: K [slots, kv_heads, s_max, 128] and V^T
 * [slots, kv_heads, s_max / 64, 2, 128, 32] per layer (element index = byte index), and one f32 scale per (K or V, kv head):
 * `scale` = [2][kv_heads] of this layer, a code stands for code * scale.  ONE quantisation rule, wherever a value enters the cache:
 * the bf16 value the bf16 cache would have held, divided by the scale in f32, clamped to +-448 (v_med3_f32, not the conversion's
 * saturation), converted with v_cvt_pk_fp8_f32 (round to nearest even).  Code 0 is 0.0 and no NaN code is ever written.  Only
 * head_dim 128.  The entry points below are the fp8-cache forms of existing ones: same launches, same records, plus a kr_kv8. */
typedef struct kr_kv8 {
    uint8_t* k;                        /* this layer's K codes */
    uint8_t* vt;                       /* this layer's V^T codes */
    const float* scale;                /* device, [2][kv_heads]: K scales, then V scales */
} kr_kv8;

/* Prefill side: the rows an admission wrote into a ONE-LAYER bf16 scratch (k_src [slots, kv_heads, s_max, 128], vt_src the V^T
 * blocks, contiguous, the strides of a layer of the bf16 cache) are converted into `dst`, a layer of the fp8 cache.  Per (slot, len)
 * of the plan and per kv head: K rows [0, len) and whole V^T blocks [0, ceil(len / 64)).  K rows at or beyond len, the other slots
 * and the scratch keep their bytes.  Elementwise, 16-byte loads and 8-byte stores, one launch, the grid capped and strided; the
 * plan is HOST memory carried in the kernel arguments (as kr_kv_fork).  n_clamped (device, optional): += the number of converted
 * elements whose |value / scale| exceeded 448 — at most one atomic add per workgroup, and only by a workgroup that clamped.
 * KR_ERR_ARG: hd != 128, a slot outside [0, slots) or listed twice, len outside [1, s_max], n outside [1, 32]. */
#define KR_KVQ_MAX_ROWS 32
typedef struct kr_kvq_plan {
    int32_t n;                         /* 1 .. KR_KVQ_MAX_ROWS */
    int32_t slot[KR_KVQ_MAX_ROWS];
    int32_t len[KR_KVQ_MAX_ROWS];      /* prompt length: rows [0, len) */
} kr_kvq_plan;
int kr_kv_quantize(const kr_bf16* k_src, const kr_bf16* vt_src, const kr_kv8* dst, int kv_heads, int hd, int slots, int s_max,
                   const kr_kvq_plan* plan, int32_t* n_clamped, kr_stream s);

/* --calculate-kv-scales: one layer's row of the scale table from the absolute maxima of what kr_kv_quantize is about to convert.
 * Same scratch, geometry and plan.  Per K and V and per kv head, amax = the largest |x| over the FINITE bf16 elements of K rows
 * [0, len) and of V keys [0, len) of every listed slot (in the last V^T block the keys at or beyond len are stale and excluded;
 * NaN and +-inf are skipped; slots not in the plan are never read), and
 *     scale_out[(K: 0 | V: 1) * kv_heads + h] = amax == 0 ? 1.0f : max(amax / range, FLT_MIN)
 * with one IEEE f32 division, range = k_range for K, v_range for V.  A maximum does not depend on order: the result is exact.
 * `work`: device, 2 * kv_heads words owned by the caller (the library allocates nothing), ZERO on entry and zero again when the
 * call's work completes, so the next layer's call reuses it.  Two launches on `s`: the reduction (pieces and capped, strided grid
 * as kr_kv_quantize; at most one atomic max per workgroup and (K | V, head) into `work`) and a one-workgroup launch behind it that
 * writes scale_out and clears `work`; both are complete before the next launch on `s` starts.
 * KR_ERR_ARG, nothing launched: a null pointer, hd != 128, kv_heads > 64, what kr_kv_quantize refuses of the geometry and the plan,
 * a range that is not finite and positive, a scratch that is not 16-byte aligned. */
int kr_kv_absmax(const kr_bf16* k_src, const kr_bf16* vt_src, int kv_heads, int hd, int slots, int s_max, const kr_kvq_plan* plan,
                 float k_range, float v_range, float* scale_out, uint32_t* work, kr_stream s);

/* kr_kv_fork for a cache of one-byte elements (a piece is hd x 64 bytes): strides in elements = bytes, multiples of 16; hd % 16. */
int kr_kv_fork8(uint8_t* kcache, uint8_t* vtcache, int64_t k_layer_stride, int64_t k_slot_stride, int64_t k_head_stride,
                int64_t vt_layer_stride, int64_t vt_slot_stride, int64_t vt_head_stride, int layers, int kv_heads, int hd,
                int slots, int s_max, const kr_fork_plan* plan, kr_stream s);

/* kr_attn_decode_slots / kr_attn_decode_rows on an fp8 cache: the same unit partition, split and wave geometry, early return and
 * records, so kr_attn_decode_merge / _merge32 run unchanged.  The codes are converted to bf16 in registers (exact) and multiplied
 * with the bf16 matrix instruction as there; scale[kvh] of K is folded into the score scale, the wave's O is multiplied by
 * scale[kv_heads + kvh] once. */
int kr_attn_decode_slots_kv8(const kr_bf16* q, const kr_kv8* kv, const int32_t* ctx_len, const int32_t* finished, float* workspace,
                             int batch, int heads, int kv_heads, int hd, int s_max, int n_split, float scale, kr_stream s);
int kr_attn_decode_rows_kv8(const kr_bf16* q, const kr_kv8* kv, const int32_t* ctx_len, const int32_t* finished,
                            const int32_t* row_slot, float* workspace, int rows, int heads, int kv_heads, int hd, int s_max,
                            int n_split, float scale, kr_stream s);

/* The KV append of a decode step into an fp8 cache: kr_linear_decode_narrow / _narrow_fp8 (w_scale NULL: bf16 weights) and
 * kr_linear_decode32 / _rows (row_slot NULL: the slots' own rows) in mode KR_DEC_ROPE_KV with the epilogue ROPE_KV8 — q is written
 * as there, K goes out as two packed 4-byte stores of codes, V^T as byte stores; kcache / vtcache of the record are ignored. */
int kr_linear_decode_narrow_kv8(const kr_bf16* x, int64_t ldx, const float* part_in, int n_part_in, kr_bf16* x_out, int64_t ldxo,
                                const void* w_packed, const float* w_scale, const kr_bf16* bias, const kr_bf16* norm_w,
                                float norm_eps, int M, int N, int K, int waves, const float* cs_table, int cs_stride,
                                const int32_t* prompt_len, const int32_t* ctx_len, kr_bf16* q_out, const kr_kv8* kv, int heads,
                                int kv_heads, int s_max, const kr_narrow_opts* opts, kr_stream s);
int kr_linear_decode32_kv8(const kr_dec32* args, const kr_kv8* kv, const int32_t* row_slot, kr_stream s);

/* Greedy sampling from the ARGMAX partials + per-step bookkeeping: token -> tokens_out[b] and
 * history[(ctx_len[b] + 1 - prompt_len[b]) * hist_stride + b] (= this sequence's generated-token
 * index), EOS / pad handling as kr_argmax_embed, ctx_len[b] += 1, embedding gather into x_next.
 * ignore_eos is a bit set: bit 0 = ignore EOS (fixed-length benchmarking), bit 1 = a finished sequence is
 * frozen (no history write, ctx_len not advanced; the pad token is still fed back) — the slot scheduler's mode:
 * a finished slot idles in place until the host prefills a new request into it. */
int kr_sample_greedy(const float* amax_val, const int32_t* amax_idx, int n_part,
                     const kr_bf16* embed_table, int d, int32_t* tokens_out, int32_t* history,
                     int hist_stride, const int32_t* prompt_len, int32_t* ctx_len, int32_t* finished,
                     const int32_t* eos, int n_eos, int pad_id, int ignore_eos, kr_bf16* x_next,
                     int batch, kr_stream s);

/* ------------------------------------------------------------------ speculative decode step (prompt-lookup drafts)
 * `slots` sequences x (k + 1) rows in ONE step of the packed 17..32-row family: row r = j * slots + slot (j = 0..k) processes the
 * token at position ctx_len[slot] + j of its slot; rows 0..slots-1 are the slots' own rows, so the per-slot state arrays are the
 * FRONT of the per-row arrays below.  kr_spec_propose fills the draft rows, the layers run over `rows` rows with
 * kr_linear_decode32_rows / kr_attn_decode_rows, kr_spec_accept replaces kr_sample_greedy.  Every row's numbers are the ones a
 * one-row step at that context computes, and the sampler's noise is a function of (seed, token index) alone, so a draft is
 * verified by equality at any temperature: the step emits exactly the tokens `emitted` plain steps would. */
typedef struct kr_spec {
    int32_t slots, k, rows;            /* rows >= slots * (k + 1), <= 32 */
    int32_t ngram_min, ngram_max;      /* 1 <= ngram_min <= ngram_max <= 8 */
    int32_t s_max;
    const int32_t* prompt_ids;         /* [slots][prompt_stride]: the prompt's token ids of every slot */
    int64_t prompt_stride;
    int32_t* history;                  /* [.][hist_stride]: kr_sample_greedy's token history */
    int32_t hist_stride;
    int32_t hist_rows;                 /* rows of `history`: kr_spec_accept never writes at or past it */
    const uint64_t* script;            /* NULL, or [slots] device addresses (0: none) of a scripted continuation (test hook): */
    const int32_t* script_len;         /*   draft j = script[generated + j - 1] replaces the lookup; [slots] lengths */
    int32_t* row_slot;                 /* [rows] per-row state; entries 0..slots-1 belong to the caller (row_slot[r] = r) */
    int32_t* ctx_len;
    int32_t* prompt_len;
    int32_t* finished;
    float* temperature;
    uint32_t* seed;
    int32_t* n_draft;                  /* [slots] */
    int32_t* draft_tok;                /* [slots][k] */
    const kr_bf16* embed_table;        /* [vocab][d] */
    int32_t d, pad_id, vocab;
    kr_bf16* x;                        /* [rows][ldx] input rows of the step */
    int64_t ldx;
    int32_t* proposed;                 /* [slots] counters kr_spec_accept adds to: drafts proposed / accepted */
    int32_t* accepted;
} kr_spec;

/* One workgroup per slot.  The slot's sequence s[0..L), L = ctx_len + 1: prompt_ids below prompt_len, then the history.  For n from
 * ngram_max down to ngram_min (n <= L - 1) the matches are the i with i + n <= L - 1 and s[i..i+n) == s[L-n..L); the first n that
 * has one decides, and among its matches the one maximising (min(k, L - i - n), i); the drafts are the tokens after it.  Writes
 * n_draft / draft_tok, and for every row r >= slots: row_slot, ctx_len = min(ctx_len[slot] + j, s_max - 1), prompt_len,
 * temperature and seed of the slot, finished = 1 where the slot is finished or j > n_draft, and x[r] = the draft's embedding (the
 * pad token's for an inactive row).  Rows at and past slots * (k + 1) are inactive rows of slot 0 parked at s_max - 1. */
int kr_spec_propose(const kr_spec* a, kr_stream s);

/* One workgroup per slot, in place of kr_sample_greedy: reduces the ARGMAX partials [rows][n_part] of the slot's k + 1 rows to
 * t_0..t_k (kr_sample_greedy's order and tie rule) and applies that launch's semantics token by token: t_j is emitted while j = 0, or
 * j <= n_draft and draft[j - 1] == t_{j-1}; nothing follows an emitted EOS.  Emitted token j -> history[ctx + 1 + j - prompt_len],
 * ctx_len += emitted, tokens_out / x[slot] take the last one, finished is set on EOS; a finished slot under the freeze bit behaves as
 * in kr_sample_greedy.  proposed += n_draft; accepted += the drafts that equal the token emitted at their position (emitted - 1, or
 * `emitted` when the last emitted token is an EOS that was drafted: nothing follows it). */
int kr_spec_accept(const kr_spec* a, const float* amax_val, const int32_t* amax_idx, int n_part, int32_t* tokens_out,
                   const int32_t* eos, int n_eos, int ignore_eos, kr_stream s);

/* Shared rows: the same step with the rows behind the slots' own as a BUDGET of rows - slots draft rows per step, dealt to the slots
 * whose lookup found something, instead of k rows owned by every slot: 1 <= slots < rows <= 32 whatever k is.  The three launches
 * below take kr_spec_propose's and kr_spec_accept's places; kr_spec is read the same way.
 *
 * kr_spec_lookup, one workgroup per slot: kr_spec_propose's search (same rule, same script override, same clamps: s_max - 1 -
 * ctx_len, tokens outside the vocabulary).  Writes n_want[slot] — what kr_spec_propose calls n_draft — and draft_tok; no row state. */
int kr_spec_lookup(const kr_spec* a, int32_t* n_want, kr_stream s);

/* One workgroup.  Rows slots .. rows - 1 are dealt breadth first: for depth j = 1..k, for the slots in ascending order, a slot that is
 * not finished and has n_want >= j takes the next free row until none is left; i.e. (slot, j) gets row
 * slots + sum_{j' < j} #{s : n_want[s] >= j'} + #{s' < slot : n_want[s'] >= j} where that is < rows.  A slot's dealt depths are a
 * prefix 1..n_draft[slot].  Writes n_draft, draft_row[slot * k + j - 1] (the row, or -1: [slots][k]) and, for every dealt row, what
 * kr_spec_propose writes for an active draft row: row_slot, ctx_len = min(ctx_len[slot] + j, s_max - 1), prompt_len, temperature,
 * seed, finished = 0 and x[row] = the draft's embedding.  Every row in slots .. rows - 1 that was not dealt belongs to no slot: it is
 * parked like a row past kr_spec_propose's layout (slot 0, position s_max - 1, finished = 1, the pad token's embedding). */
int kr_spec_deal(const kr_spec* a, const int32_t* n_want, int32_t* draft_row, kr_stream s);

/* kr_spec_accept with the ARGMAX partials of a slot's draft j read at row draft_row[slot * k + j - 1] (t_0 at row `slot`); everything
 * else as there.  proposed += n_draft: the drafts that were dealt a row. */
int kr_spec_accept_rows(const kr_spec* a, const int32_t* draft_row, const float* amax_val, const int32_t* amax_idx, int n_part,
                        int32_t* tokens_out, const int32_t* eos, int n_eos, int ignore_eos, kr_stream s);

/* Guided slots in a speculative step.  A draft row needs the DFA state its token is chosen under; the state at draft depth j is the
 * slot's state walked over drafts 1..j.  Three launches of integer work (one workgroup or less per slot) around the step; the
 * launches between them are unchanged, and kr_gumbel_argmax_guided reads the per-row entries written here.  The per-row arrays hold
 * `rows` entries; entries 0..slots-1 are the caller's (the slots' own guides and states) and only kr_spec_guide_advance writes them. */
typedef struct kr_spec_guide {
    uint64_t* guide_trans;             /* [rows] device address of the row's DFA table [S][256] uint16 (0: unconstrained) */
    uint64_t* guide_masks;             /* [rows] address of the pattern's mask table (kr_guide_build_masks) */
    int32_t* guide_state;              /* [rows] DFA state the row's token is chosen under */
    int32_t mask_words;                /* even, mask_words * 32 >= kr_spec.vocab */
    const int32_t* vocab_off;          /* as kr_guide_advance: [vocab + 1] */
    const uint8_t* vocab_bytes;
    int32_t* draft_state;              /* [slots][k] scratch: the state after drafts 1..j */
    int32_t* ctx_before;               /* [slots] scratch: ctx_len at the start of the step */
} kr_spec_guide;

/* Before any row is spent on a draft.  n_count: kr_spec_propose's n_draft (static layout: after kr_spec_propose) or kr_spec_lookup's
 * n_want (shared rows: between kr_spec_lookup and kr_spec_deal, so a forbidden draft is not dealt a row another slot could use).
 * Per slot: ctx_before = ctx_len, always.  A finished slot, or one with guide_trans == 0, keeps its count and its drafts.  Otherwise,
 * from st = guide_state[slot], for j = 1..n_count: draft j is kept iff its bit is set in mask row st (the bit
 * kr_gumbel_argmax_guided tests); the first draft that is not cuts the count to j - 1; a kept draft moves st = walk(st, bytes(draft))
 * and draft_state[slot][j - 1] = st; a kept draft without bytes (an EOS id in an accepting state) cuts the count to j: nothing follows
 * an EOS.  draft_tok at and beyond the new count becomes pad_id. */
int kr_spec_guide_trim(const kr_spec* a, const kr_spec_guide* g, int32_t* n_count, kr_stream s);

/* After the trim (static layout, draft_row == NULL: draft j of a slot on row j * slots + slot) or after kr_spec_deal (draft_row: its
 * map, -1 entries belong to nobody).  Every row r >= slots: the row of draft (slot, j) with j <= n_draft[slot] of a guided slot gets
 * the slot's guide_trans and guide_masks and guide_state = draft_state[slot][j - 1]; every other row (inactive, parked, padding, of an
 * unguided slot) gets zeros in all three.  Static layout only: a row (slot, j) with j > n_draft[slot] also gets finished = 1, because
 * kr_spec_propose ran before the trim. */
int kr_spec_guide_rows(const kr_spec* a, const kr_spec_guide* g, const int32_t* draft_row, kr_stream s);

/* After kr_spec_accept / kr_spec_accept_rows.  Per slot with guide_trans != 0: guide_state is walked over the e = ctx_len - ctx_before
 * tokens the step emitted (read from `history`), except the last one where the step set finished (kr_guide_advance skips the rows
 * kr_sample_greedy has just finished): the state e plain guided steps leave. */
int kr_spec_guide_advance(const kr_spec* a, const kr_spec_guide* g, kr_stream s);

/* Controlled slots in a speculative step: sampling controls (kr_sample_threshold_rows / kr_gumbel_argmax_processed_rows) and logit
 * adjustments (kr_logits_adjust_rows) on draft rows.  Row (slot, j) chooses t_j, which counts only if drafts 1..j were accepted: its
 * output so far is the slot's plus d_1..d_j.  Params, prompt bits and the adjustment table are the slot's; min_tokens needs nothing,
 * n = ctx_len + 1 - prompt_len is per row already; the output counts take in the drafts in front of the row (depth); the stop entries
 * are kept out of the drafts, because kr_spec_accept knows the EOS ids only.  Three launches of integer work around the step, in
 * either layout, beside kr_spec_guide_*'s (both trims may run: each only lowers the count). */
typedef struct kr_spec_controls {
    const int32_t* adj_ids;            /* [slots][KR_ADJ_CAP] the slots' adjustment tables (kr_logits_adjust) */
    const int32_t* adj_flag;
    const int32_t* adj_meta;           /* [slots][4] */
    int32_t* counts;                   /* [slots][ld_counts] output-token counts (kr_sample_count's) */
    int64_t ld_counts;                 /* >= kr_spec.vocab */
    int32_t* depth;                    /* [rows] drafts in front of the row: what the _rows launches take */
    int32_t* ctx_before;               /* [slots] scratch: ctx_len at the start of the step (kr_spec_guide.ctx_before may be the same array) */
} kr_spec_controls;

/* Before any row is spent on a draft; n_count as for kr_spec_guide_trim (n_draft behind kr_spec_propose, n_want between kr_spec_lookup
 * and kr_spec_deal).  Per slot: ctx_before = ctx_len, always.  A finished slot, or one whose table is empty, keeps its count and its
 * drafts.  Otherwise the count is cut to j - 1 at the first draft j that is a stop entry (adj_flag bit 0) of the slot's table, whatever
 * min_tokens says, and draft_tok at and beyond the new count becomes pad_id.  Then a stop token can only be the last token the step
 * emits, and kr_stop_tokens over tokens_out behind kr_spec_accept / kr_spec_accept_rows finishes the slot as in a plain step. */
int kr_spec_controls_trim(const kr_spec* a, const kr_spec_controls* c, int32_t* n_count, kr_stream s);

/* After the trims (static layout, draft_row == NULL) or after kr_spec_deal (draft_row: its map).  depth[r] for every row r < rows: j
 * for the row of draft (slot, j) with j <= n_draft[slot], 0 for every other row (a slot's own, inactive, parked, padding).  Static
 * layout only: a row (slot, j) with j > n_draft[slot] also gets finished = 1, as from kr_spec_guide_rows. */
int kr_spec_controls_rows(const kr_spec* a, const kr_spec_controls* c, const int32_t* draft_row, kr_stream s);

/* After kr_spec_accept / kr_spec_accept_rows (and kr_stop_tokens).  Per slot: counts[slot][t] += 1 for each of the e = ctx_len -
 * ctx_before tokens the step emitted (0 <= e <= k + 1, read from `history`), a finishing EOS or stop token included — a plain step
 * counts it too (kr_sample_threshold's live is taken before the token).  A finished slot frozen in place has e = 0 (speculative
 * steps run under the freeze bit). */
int kr_spec_controls_count(const kr_spec* a, const kr_spec_controls* c, kr_stream s);

/* Log-probabilities of a speculative step: one record per token the step emitted and a plain step would have recorded, written
 * where the plain steps would have written it.  Token j of a slot (j = 0: on the slot's own row) was chosen on the row of its draft
 * j, and that row's logits are the bits a one-row step at that context computes, so the contract of a record is equality: it is, bit
 * for bit, what kr_logprobs_topk writes with the same n_part and k on a one-row batch holding that logits row (same slice
 * partition, same max / sum-exp fold order, same tie rule). */
typedef struct kr_spec_logprobs {
    int32_t k_top;                     /* 0..20: kr_logprobs_topk's k */
    int32_t n_part;                    /* vocabulary slices: ceil(vocab / n_part) <= 4096, n_part <= 1024 */
    float* part_val;                   /* [rows][n_part][max(k_top, 1)] scratch, as kr_logprobs_topk's */
    int32_t* part_idx;
    float* part_ms;                    /* [rows][n_part][2] */
    float* out_lp;                     /* [hist_len][hist_batch][1 + k_stride], as kr_logprobs_topk's */
    int32_t* out_idx;                  /* [hist_len][hist_batch][k_stride] */
    int32_t hist_len, hist_batch, k_stride;
    const int32_t* ctx_before;         /* [slots]: ctx_len at the start of the step (a trim's, or kr_spec_mark's) */
} kr_spec_logprobs;

/* At the head of a speculative step that records log-probabilities and carries neither kr_spec_guide_trim nor
 * kr_spec_controls_trim (both write the array always): ctx_before[slot] = ctx_len[slot] for every slot, nothing else. */
int kr_spec_mark(const kr_spec* a, int32_t* ctx_before, kr_stream s);

/* After kr_spec_accept (draft_row == NULL: draft j of a slot on row j * slots + slot) / kr_spec_accept_rows (draft_row: kr_spec_deal's
 * map) and kr_stop_tokens, before kr_repeat_detect.  logits [rows][ld_logits]: what the lm_head wrote (after kr_logits_restore_rows
 * where the step adjusted them).  Per slot e = ctx_len - ctx_before tokens were emitted (0 <= e <= k + 1; a finished slot frozen in
 * place: 0) and n_rec = e - (finished != 0) of them record: the token that finished the slot (EOS, stop entry) records nothing, as
 * in a plain step.  For j = 0 .. n_rec - 1: the row is `slot` (j = 0), else the draft's; h = ctx_before + 1 + j - prompt_len; the
 * token is history[h][slot]; out_lp[h][slot][0] = log p(token) (-inf for a token outside the vocabulary), out_lp[h][slot][1 + i] /
 * out_idx[h][slot][i] = the i-th most probable token of that row (ties: lowest id), i < k_top.  Nothing is written for h outside
 * [0, hist_len) or at or past kr_spec.hist_rows, nor for a row outside [0, rows).  The logits and partials of a row that records
 * nothing are never read (parked rows may hold anything) and no partial is computed for it: two launches, grids (n_part,
 * slots * (k + 1)) and slots * (k + 1), whose other workgroups return at once.
 * KR_ERR_ARG, nothing launched: what kr_spec_accept / kr_spec_accept_rows refuse of kr_spec, a null pointer, ld_logits < vocab,
 * slots > hist_batch, hist_len < 1, and kr_logprobs_topk's bounds on k_top, k_stride, n_part. */
int kr_logprobs_topk_rows(const kr_spec* a, const kr_spec_logprobs* p, const int32_t* draft_row, const float* logits,
                          int64_t ld_logits, kr_stream s);

/* ------------------------------------------------------------------ runaway repetition (vLLM's repetition_detection)
 * The rule is a function of a sequence's generated tokens y[0..g] alone (the prompt never counts).  Per slot the cfg row holds
 * min_pattern_size a, max_pattern_size b, min_count c, min_span m with 1 <= a <= b <= KR_REP_MAX_PERIOD, c >= 2, m >= 0; b == 0
 * switches the slot off (so does a row outside those bounds).  For a period p, run_p(g) is the number of consecutive indices i,
 * counted back from g, with i >= p and y[i] == y[i - p].  The sequence REPEATS AT g when some p in [a, b] has
 * run_p(g) >= max((c - 1) p, m - p): the last c p tokens are c copies of one block, and the repeated stretch is at least m tokens long.
 * The sequence ends at the smallest such g; that token is kept.
 *
 * kr_repeat_detect, one workgroup per slot, behind kr_sample_greedy / kr_stop_tokens or kr_spec_accept / kr_spec_accept_rows /
 * kr_spec_guide_advance.  A slot holds gen = ctx_len - prompt_len + 1 generated tokens after those (capped at hist_rows), token i at
 * history[i * hist_stride + slot].  A live slot: tokens seen .. gen - 1 are walked in order, run[p] = (g >= p && y[g] == y[g - p]) ?
 * run[p] + 1 : 0 for the periods a..b; at the first g that repeats, rep_at = g, finished = 1, seen = g + 1 and the walk ends there
 * (run is the state at g); without one, seen = gen.  So one launch per token and one launch per several tokens leave the same
 * rep_at, seen and run.  run needs no clearing: at g = 0 every period is reset by g < p, and an admission only sets seen = 0,
 * rep_at = -1 and the cfg row.
 * Untouched: a slot that is off, a slot with rep_at >= 0 (it is written once), a finished slot without the freeze bit (its new
 * tokens are pads) and a finished slot without new tokens (frozen).  A finished slot WITH new tokens under the freeze bit was
 * finished by this very step — a speculative step that emitted several tokens, the last of them the EOS: the tokens before the
 * last are walked and only rep_at is written, so the cut is where one-token steps would have made it.
 * flags: kr_sample_greedy's word; bit 0 (nothing finishes): nothing is recorded and nothing is launched.
 * KR_ERR_ARG, and nothing launches: a null pointer, slots outside 1..32, hist_stride < slots, hist_rows < 1, unknown flag bits. */
#define KR_REP_MAX_PERIOD 1024
typedef struct kr_repeat {
    int32_t slots;
    const int32_t* history;            /* [hist_rows][hist_stride]: kr_sample_greedy's token history */
    int32_t hist_stride;
    int32_t hist_rows;
    const int32_t* ctx_len;            /* [slots] */
    const int32_t* prompt_len;         /* [slots] */
    int32_t* finished;                 /* [slots] */
    const int32_t* cfg;                /* [slots][4]: a, b, c, m */
    int32_t* run;                      /* [slots][KR_REP_MAX_PERIOD]: run[p - 1] of period p */
    int32_t* seen;                     /* [slots]: generated tokens looked at so far */
    int32_t* rep_at;                   /* [slots]: the index the sequence repeats at, -1: none */
    int32_t flags;
} kr_repeat;
int kr_repeat_detect(const kr_repeat* a, kr_stream s);

/* kr_linear_decode32, KR_DEC_ROPE_KV only, for the rows of a speculative step: the cache base and the cs_table row of row r come
 * from row_slot[r]; the cache position and the rotary index from the row's own ctx_len / prompt_len entries.  q_out stays per row.
 * row_slot == NULL: kr_linear_decode32's bits. */
int kr_linear_decode32_rows(int mode, const kr_dec32* args, const int32_t* row_slot, kr_stream s);

/* kr_attn_decode_slots with q, ctx_len, finished and the workspace records per ROW and the cache base from row_slot[row]: the same
 * unit partition, accumulation order and records, so row (slot, j) gets the partials of a one-row step at that context. */
int kr_attn_decode_rows(const kr_bf16* q, const kr_bf16* kcache, const kr_bf16* vtcache, const int32_t* ctx_len,
                        const int32_t* finished, const int32_t* row_slot, float* workspace, int rows, int heads, int kv_heads,
                        int hd, int s_max, int n_split, float scale, kr_stream s);

/* ------------------------------------------------------------------ multi-GPU: one-time weight broadcast (RCCL)
 * One process per GPU.  Rank 0 calls kr_comm_unique_id and shares the 128 bytes through any host
 * channel (the Python host uses torch.distributed's store); every rank then calls kr_comm_init.
 * kr_bcast_weights is ncclBroadcast of the packed weight arena from `root`; it is
 * the only collective on the path — steady state has none. */
#define KR_UNIQUE_ID_BYTES 128
int kr_comm_unique_id(uint8_t* id128);
int kr_comm_init(void** comm, int n_ranks, int rank, const uint8_t* id128);
/* Number of ranks RCCL itself reports for the communicator (ncclCommCount): bench.py prints it, so "did RCCL see N
 * ranks?" is answered by the library, not by the launcher's environment. */
int kr_comm_count(void* comm, int* n_ranks);
int kr_comm_destroy(void* comm);
/* ncclGetVersion of the RCCL this library is bound to (major * 10000 + minor * 100 + patch): reported beside the broadcast rate. */
int kr_rccl_version(int* version);
int kr_bcast_weights(void* comm, void* buf, size_t bytes, int root, kr_stream s);

/* ------------------------------------------------------------------ device self-tests (used by tests/ -m gpu) */
/* Runs an MFMA lane-layout check (A=I, asymmetric B) on the device; returns 0 if exact. */
int kr_selftest_mfma(kr_stream s);
/* Diagnostic: microseconds per kernel of a dependent chain of `n` tiny kernels (`blocks` x 256
 * threads; dirty != 0: each block also writes 4 KiB) replayed from a hipGraph on stream `s`. */
int kr_probe_launch_floor(kr_stream s, int n, int blocks, int dirty, float* us_per_kernel);
/* Diagnostic: the read-only streaming rate (GB/s, best of `reps` launches timed with HIP events on `s`) of `blocks` x 256
 * threads reading [ptr, ptr + bytes) once with 16-byte nontemporal loads, 8 in flight per lane — the measured counterpart of
 * the vendor HBM peak when the range is far larger than the 256 MB Infinity Cache. */
int kr_probe_stream_read(const void* ptr, size_t bytes, int blocks, int reps, kr_stream s, float* gbytes_per_s);
/* Launches an empty kernel (1 wave): calibrates the cost of a HIP-event bracket around one launch. */
int kr_launch_null(kr_stream s);

#ifdef __cplusplus
}
#endif
#endif /* KARANTA_HIP_H */
