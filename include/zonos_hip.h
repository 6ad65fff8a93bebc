/* zonos_hip.h -- C ABI of libzonos_hip.so, the MI355X (gfx950) engine for the Zonos
 * decode hot path: generate() autoregressive DAC-token decode and the DAC decoder.
 *
 * Conventions
 *   - Plain C types only: device pointers are passed as `void*`/typed pointers obtained
 *     from the caller's allocator (torch.Tensor.data_ptr() in zonos_amd), sizes as int.
 *   - Every call is asynchronous on the `stream` argument (a hipStream_t passed as void*;
 *     NULL = default stream) and returns 0 on success, <0 on error; the message is
 *     available from zk_last_error() (thread-local). No C++ exception crosses the ABI.
 *   - bf16 tensors are raw uint16 bit patterns (torch.bfloat16 storage).
 *   - The reference interface each entry point replaces is cited as file:line relative
 *     to the coezbek/Zonos checkout (modeling_dac.py = transformers' DAC).
 */
#ifndef ZONOS_HIP_H
#define ZONOS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ library */
int zk_version(void);                 /* ABI version (monotonic) */
const char* zk_last_error(void);      /* thread-local message of the last failing call */
int zk_device_sync(void);             /* hipDeviceSynchronize + error check */
long zk_abi_size(int which);          /* sizeof / offsetof of the ABI structs (binding self-check) */

/* ------------------------------------------------------------------ sampling
 * Mirrors sample_from_logits (zonos/sampling.py:232-328) incl.
 * modify_logit_for_repetition_penalty (131-169), apply_unified (54-75),
 * apply_top_p (96-111), apply_top_k (77-93), apply_min_p (114-128) and the
 * exponential-race multinomial (11-33). The Exp(1) noise is the engine's
 * Philox4x32-10 stream keyed by (seed, step, draw, row_base+b, codebook, token);
 * see oracle/philox.py for the exact definition. */
typedef struct zk_sampling_params {
    float temperature;        /* 0 => argmax (sampling.py:325-326) */
    float top_p;              /* 0 disables */
    float min_p;              /* 0 disables */
    float linear, conf, quad; /* unified sampler; linear<=0 disables */
    int32_t top_k;            /* 0 disables */
    int32_t rp_window;        /* repetition_penalty_window; see "window contract" below */
    float cfg_scale;          /* classifier-free guidance scale (model.py:112-114) */
    int32_t force_full_length;/* benchmark mode: cb0 EOS logit forced to -inf every step */
} zk_sampling_params;

/* Standalone sampler over fp32 logits [B][K][V] (already CFG-combined).
 * generated: int64 [B][K][gen_stride] token history (the reference passes
 *            delayed_codes[..., :offset]), 0 <= gen_len <= gen_stride; tokens >= V count as V-1
 *            (sampling.py:143), tokens must be >= 0; NULL => no repetition penalty (prefill call).
 * rp:        float [B] per-row repetition penalty (model.py:342,356).
 * out:       int64 [B][K] sampled tokens.
 *
 * Window contract (all three sampler entries). The reference penalises generated[..., -rp_window:]
 * (sampling.py:142), so the penalised columns are the last W of the first gen_len, with
 *     W = gen_len                  when rp_window == 0 (Python's -0: selects everything),
 *     W = min(rp_window, gen_len)  otherwise;
 * rp_window == 0 does not switch the penalty off (rp == 1 or generated == NULL does). The kernel holds
 * at most 512 columns. zk_sample_logits and zk_sample_logits_torch know gen_len on the host: a call
 * with W <= 512 matches the reference, a call with W > 512 returns an error and launches nothing.
 * zk_sample_heads reads the history length from the device word scal[0], which outgrows 512 during a
 * generation: it takes 1 <= rp_window <= 512 only and returns an error otherwise. */
int zk_sample_logits(const float* logits, int B, int K, int V,
                     const int64_t* generated, int gen_stride, int gen_len, const float* rp,
                     const zk_sampling_params* sp, uint64_t seed, int step, int draw, int row_base,
                     int64_t* out, void* stream);

/* zk_sample_logits with torch's GPU noise instead of the keyed stream: the [B][K][V] race noise is
 * what `torch.empty_like(logits).exponential_(1)` returns when torch's CUDA generator holds
 * (seed, offset) (sampling.py:26-28); stride from zk_torch_noise_policy(B*K*V, ...). The caller
 * advances the generator by the policy's incr, as torch's own call would. History, window contract
 * and refusals as zk_sample_logits. */
int zk_sample_logits_torch(const float* logits, int B, int K, int V,
                           const int64_t* generated, int gen_stride, int gen_len, const float* rp,
                           const zk_sampling_params* sp, uint64_t seed, uint64_t offset, int stride,
                           int64_t* out, void* stream);
/* out[e] = element e of torch's GPU `Tensor.exponential_(1)` over n elements whose call took the
 * generator's Philox (seed, offset) (torch 2.10 ATen/native/hip/DistributionTemplates.h:52-91 with
 * hiprand Philox4x32-10 and TransformationHelper.h:129-146; oracle/torch_philox.py). */
int zk_torch_exponential(float* out, long n, uint64_t seed, uint64_t offset, int stride, void* stream);
/* Host-only: torch's calc_execution_policy for an n-element distribution call on a device with
 * mp_count CUs of max_threads_per_mp threads: the kernel's grid-stride (256 x grid) and the Philox
 * offset the call consumes (DistributionTemplates.h:52-63). */
int zk_torch_noise_policy(long n, int mp_count, int max_threads_per_mp, int* stride, long* incr);

/* Delay pattern (zonos/codebook_pattern.py:5-12). codes int64 [B][K][T] ->
 * delayed int64 [B][K][T+K]; revert: delayed [B][K][L] -> codes [B][K][L-K]. */
int zk_delay_apply(const int64_t* codes, int B, int K, int T, int64_t mask_token,
                   int64_t* delayed, void* stream);
int zk_delay_revert(const int64_t* delayed, int B, int K, int L, int64_t* codes, void* stream);

/* ------------------------------------------------------------------ backbone building blocks
 * (zonos/backbone/_torch.py). All activations bf16 row-major. */

/* embed_codes (model.py:97-98) + the CFG row duplication (model.py:141) + the first
 * LayerNorm of layer 0 (_torch.py:100). ids: int64 codes read at ids[b*ids_bstride +
 * k*ids_kstride + col] with col = t + (col_dev ? *col_dev + col_add : 0), t in [0,S).
 * Output row r*out_S + out_t0 + t for r in [0, rows_dup*B) uses utterance r % B.
 * x_out = embedding sum; if ln_w != NULL also xn_out = LayerNorm(x_out).
 * skip (nullable, device int32): when *skip != 0 the kernel does nothing (generation done). */
int zk_embed_codes(const int64_t* ids, int B, int S, int K, long ids_bstride, long ids_kstride,
                   const int32_t* col_dev, int col_add, const void* emb, int V, int D, int rows_dup,
                   void* x_out, int out_S, int out_t0, const void* ln_w, const void* ln_b, float eps,
                   void* xn_out, const int32_t* skip, void* stream);

/* Prefill placement and epilogue of a request batch whose conditionings differ in length (zk_prefill_rows;
 * the reference pads every text to the longest, conditioning.py, and attends to the pad tokens). row_off: device
 * int32 [rows], <= 0.
 * zk_embed_codes_rows: zk_embed_codes without col_dev, LayerNorm and skip, each row at its own position -- output
 * row r*out_S + out_t0 + row_off[r] + t (the start clamped into [0, out_S - S] on the device), the same sum.
 * zk_gather_last_rows: out bf16 [R][D] = x[r*S + S - 1 + row_off[r]] (offset clamped into [-(S-1), 0]): the last
 * valid position of every row, compact, for the heads GEMM of the prefill (model.py:300-304). */
int zk_embed_codes_rows(const int64_t* ids, int B, int S, int K, long ids_bstride, long ids_kstride,
                        const void* emb, int V, int D, int rows_dup, void* x_out, int out_S, int out_t0,
                        const int32_t* row_off, void* stream);
int zk_gather_last_rows(const void* x, int R, int S, int D, const int32_t* row_off, void* out, void* stream);

/* y = LayerNorm(x) (nn.LayerNorm with bias, _torch.py:88,90,62), rows x D. */
int zk_layernorm(const void* x, const void* w, const void* b, float eps, int rows, int D,
                 void* y, void* stream);

/* x_out = bf16(x_in + bf16(sum_s part[s])) ; xn = LayerNorm(x_out) (_torch.py:100-101).
 * ln_on_sum is a flags word. Bit 0: xn = LayerNorm(x_in + bf16(sum)) of the fp32 sum before rounding
 * (mamba_ssm layer_norm_fn with prenorm, the hybrid backbone's fused add + norm). With bit 0 set, the
 * hybrid config variants (mamba_ssm Block, _mamba_ssm.py:18-31,49-57): bit 1 RMS norm
 * (is_rms_norm: y = x * rsqrt(mean(x^2) + eps) * w (+ b); b may be NULL), bit 2 x_in is fp32, bit 3
 * x_out is fp32 (residual_in_fp32), and nsplit = 0 adds no projection (part unused: the first
 * block's norm of the embedding, layer_norm_fn with residual = None).
 * part: fp32 [nsplit][rows][D] split-K slabs of the preceding projection. */
int zk_resid_ln(const float* part, int nsplit, const void* x_in, const void* w, const void* b,
                float eps, int rows, int D, void* x_out, void* xn_out, int ln_on_sum,
                const int32_t* skip, void* stream);

/* C = A[M][K] . W[N][K]^T (nn.Linear, bias-free). bf16 in, fp32 accumulation (MFMA).
 * mode 0: fp32 split-K slabs Cpart[split][M][N] (nsplit = K-split count);
 * mode 1: SwiGLU epilogue for FeedForward fc1 (_torch.py:147,151-152): W rows must be
 *         in the engine's interleaved order (zk_permute_fc1) and Cout is bf16 [M][N/2].
 * lda = row stride of A in elements (lets the heads GEMM read only the last token).
 * W is in the engine's fragment-packed layout (zk_pack_weights; rows padded to 64). */
int zk_gemm_bf16(const void* A, long lda, const void* W, int M, int N, int K, int nsplit, int mode,
                 float* Cpart, void* Cout, const int32_t* skip, void* stream);
/* Host-only (no GPU): the number of 16-column tiles of W's packed image that the L2 warm-up of
 * this decode GEMM (warm.h: issued by the kernel before it) reads; 0 when the GEMM is not warmed.
 * Never more than ceil(N / 16), the tiles of the packed image that hold a column < N. */
int zk_gemm_warm_tiles(int M, int N, int K, int nsplit, int mode, int chunks);
/* The launch plan of zk_gemm_bf16(M, N, K, nsplit, mode), by the entry's own shape checks (with lda = K) and
 * the plan it launches from. Host only: no GPU is touched. Fills plan[ZK_GEMM_PLAN_N]; fields that do not
 * belong to the family are 0:
 *   0 family (0 k_gemv_rk, 1 k_gemm_ws, 2 k_gemm_pf, 3 k_gemm)
 *   1 ks (k_gemv_rk: k-steps of 32 per wave)        2 pf (k_gemv_rk: k-steps, k_gemm_ws: chunks in flight)
 *   3 nchunks (k_gemm_ws, k_gemm: 64-deep chunks of a K slice)
 *   4 mt (k_gemm_ws: 16-row tiles)                  5 ncw (k_gemm_ws: compute waves = 16-column tiles)
 *   6 u (k_gemm: ring slots)                        7 ntw (k_gemm: 16-column tiles per wave)
 *   8, 9, 10 grid x, y, z   11 threads per workgroup   12 dynamic LDS bytes
 *   13 k_gemm_pf: columns of its 256-row tile
 * Returns 0, or -1 with zk_last_error set where the entry would refuse the shape. */
#define ZK_GEMM_PLAN_N 14
int zk_gemm_plan(int M, int N, int K, int nsplit, int mode, int32_t* plan);
/* Small-batch (M <= 16) GEMV without split-K, for the B <= 8 decode layer (five launches per
 * transformer block instead of seven; replaces the k_resid_ln launches of _torch.py:100-101):
 *   ln_w/ln_b non-NULL: A holds the residual rows x (bf16, K = D = 2048) and every workgroup
 *     applies nn.LayerNorm(eps) to them in its prologue (TransformerBlock.norm / norm2 /
 *     backbone norm_f, _torch.py:78,100-101) before the product;
 *   mode 0: Cf fp32 [M][N] = LN?(A) . W^T            (in_proj, heads: one "slab", nsplit 1)
 *   mode 1: Cb bf16 [M][N/2] = SwiGLU(LN?(A) . W^T)  (fc1, interleaved rows as zk_gemm_bf16)
 *   mode 2: Cb bf16 [M][N] += bf16(A . W^T), i.e. x = bf16(x + bf16(proj))   (out_proj, fc2)
 * W fragment-packed (zk_pack_weights). K in {2048, 4096, 8192}; results depend on (N, K) only. */
int zk_gemv_fused(const void* A, long lda, const void* W, int M, int N, int K, int mode,
                  const void* ln_w, const void* ln_b, float eps, float* Cf, void* Cb,
                  const int32_t* skip, void* stream);
/* The launch plan of zk_gemv_fused(M, N, K, mode, ln: with the LayerNorm prologue or not), by the entry's own
 * shape checks (with lda = K). Host only: no GPU is touched. Fills plan[ZK_GEMV_PLAN_N]:
 *   0 lay (0 half a 16-column tile per workgroup, 1 one tile, 2 two tiles)
 *   1 ksw (K / 32)   2 xr (rows of the LDS activation image: 2 or 16)   3 workgroups   4 threads per workgroup
 *   5 ntw (tiles per workgroup)   6 half (0 / 1)   7 nw (waves splitting K)   8 ks (k-steps per wave)
 *   9 pf (weight loads in flight per wave)
 * Returns 0, or -1 with zk_last_error set where the entry would refuse the shape. */
#define ZK_GEMV_PLAN_N 10
int zk_gemv_plan(int M, int N, int K, int mode, int ln, int32_t* plan);
/* Attention out_proj of a small decode batch (M = 2B <= 2 rows) straight from the split
 * partials of zk_attn_decode_qkv_part: x[M][N] = bf16(x + bf16(merge(work) . W^T))
 * (_torch.py:66 + the residual add of :100), the merge being k_attn_combine's arithmetic
 * (bit-identical to zk_attn_decode_qkv + zk_gemv_fused mode 2 with the same nsplit).
 * K = 2048 (16 heads x 128), nsplit in {2, 4, 8, 16}. Also the consumer of zk_attn_decode_q_part. */
int zk_gemv_attn_out(const float* work, int nsplit, int Hkv, const void* W, int M, int N, int K,
                     void* x, const int32_t* skip, void* stream);
/* in_proj of the B = 1 decode layer (M = 2 rows) with the RoPE / KV-write epilogue
 * (_torch.py:61-65 + apply_rotary_emb :18-30 + _update_kv_cache :33-49): LayerNorm(x) (ln_w, ln_b,
 * the norm prologue of zk_gemv_fused) . Wqkv^T, each column rounded to bf16, q and k rotated by the
 * interleaved RoPE pairs at position p = min(*pos_dev, Smax - 1) (freqs as zk_qkv_rope), q stored to
 * q_out bf16 [M][H*hd], k and v written into the layer's cache at key p (layout of zk_qkv_rope).
 * Bit-identical to zk_gemv_fused mode 0 + the fused prologue of zk_attn_decode_qkv. d_model = H*hd =
 * 2048, hd = 128. */
int zk_gemv_qkv_rope(const void* x, const void* W, int M, int H, int Hkv, int hd, const void* ln_w,
                     const void* ln_b, float eps, void* q_out, void* k_cache, void* vt_cache, int Smax,
                     const int32_t* pos_dev, const float* freqs, const int32_t* skip, void* stream);
/* fc1 weight [2F][D] (rows: F "y" then F "gate") -> interleaved groups of 8 y + 8 gate rows. */
int zk_permute_fc1(const void* w_fc1, int F, int D, void* w_out, void* stream);
/* nn.Linear weight [N][K] bf16 -> fragment-packed [ceil64(N)/16][K/32][64][8] (rows >= N zero):
 * each 16x32 MFMA B fragment is one contiguous 1 KB block in lane order, a 16-row tile's
 * K-slices consecutive, so every wave streams its weights as one sequential run.
 * out holds ceil64(N)*K elements. K % 64 == 0. */
int zk_pack_weights(const void* w, int N, int K, void* out, void* stream);

/* Opt-in FP8 (e4m3fn) weights of the small-batch GEMVs (generate(weight_dtype="fp8"); format and packed
 * image: zonos_amd/wlayout.py). zk_pack_weights_e4m3 is the load-time quantiser, the FP8 counterpart of
 * zk_pack_weights: nn.Linear weight [N][K] bf16 (fc1: in zk_permute_fc1 order) -> OCP e4m3fn bytes with one
 * power-of-two scale per output row (biased exponent byte, 2^(b-127); the scale rule of
 * zk_kv_quantize_e4m3 on the row's amax), out = the packed image [ceil64(N)/16][K/64][64][2][8] bytes
 * (ceil64(N)*K bytes; rows >= N zero), scales = uint8 [ceil64(N)] (rows >= N: 127). K % 64 == 0.
 * The three GEMV entries are their bf16 counterparts with the byte image and its scales in place of W:
 * same argument checks, same layout / K split / summation order per shape, so each returns the bits of
 * the bf16 entry on zk_pack_weights(dequantised weights). */
int zk_pack_weights_e4m3(const void* w, int N, int K, void* out, void* scales, void* stream);
int zk_gemv_fused_w8(const void* A, long lda, const void* W8, const void* w_scale, int M, int N, int K, int mode,
                     const void* ln_w, const void* ln_b, float eps, float* Cf, void* Cb,
                     const int32_t* skip, void* stream);
int zk_gemv_qkv_rope_w8(const void* x, const void* W8, const void* w_scale, int M, int H, int Hkv, int hd,
                        const void* ln_w, const void* ln_b, float eps, void* q_out, void* k_cache,
                        void* vt_cache, int Smax, const int32_t* pos_dev, const float* freqs,
                        const int32_t* skip, void* stream);
int zk_gemv_attn_out_w8(const float* work, int nsplit, int Hkv, const void* W8, const void* w_scale, int M,
                        int N, int K, void* x, const int32_t* skip, void* stream);

/* Sum split-K slabs of in_proj, round to bf16, apply interleaved RoPE to q and k
 * (apply_rotary_emb _torch.py:18-30; positions pos0 + t (+ *pos_dev if non-NULL);
 * freqs = precompute_freqs_cis table [16384][hd/2][2], _torch.py:9-15), store q
 * [rows][H*hd] and write k, v into the layer cache (_update_kv_cache _torch.py:33-49).
 * Cache layout (engine-owned; hd = 128): per (row, kv head) Smax keys in 32-key slices of
 * 8 KB stored in MFMA-fragment order (backbone.hip k_off / v_off; zonos_amd.kvlayout):
 *   K: [R][Hkv][Smax/32][h 2][ks 4][lane 64][8],  V: [R][Hkv][Smax/32][dt 8][lane 64][8].
 * v_rows (nullable): also write V as [R][Hkv][S][hd] (prefill scratch).
 * rope_neox = 0: interleaved pairs (2j, 2j+1) (the transformer); 1: GPT-NeoX pairs (j, j+hd/2)
 * (mamba_ssm MHA via flash_attn RotaryEmbedding, interleaved=False; hybrid backbone). freqs is
 * then the bf16-rounded cos/sin cache (oracle/hybrid_ref.py rotary_table).
 * rows = R*S tokens ordered r*S + t. */
int zk_qkv_rope(const float* part, int nsplit, int R, int S, int H, int Hkv, int hd,
                const float* freqs, int pos0, const int32_t* pos_dev,
                void* q_out, void* k_cache, void* vt_cache, int Smax, void* v_rows,
                int rope_neox, const int32_t* skip, void* stream);

/* Scaled-dot-product attention over the cache (F.scaled_dot_product_attention,
 * _torch.py:136; GQA, scale 1/sqrt(hd)).
 * decode: one query per row, keys [0, ctx) with ctx = ctx0 + *ctx_dev; flash-decoding
 *         over 128-key blocks split across `nsplit` workgroups per (row, kv head)
 *         (nsplit <= Smax/128; work: fp32 [R][Hkv][nsplit][8 + 4*hd] when nsplit > 1).
 * prefill: S queries per row at positions 0..S-1, causal (is_causal=S>1), K and V from the cache.
 * Output bf16 [rows][H*hd].
 * Every zk_attn_decode* entry, bf16 or FP8 cache, fails before any launch, with zk_last_error starting
 * with its own name, on hd != 128, a GQA group above 4, Smax <= 0 or not a multiple of 128 (_q_part: of
 * 32), nsplit out of range, a missing work buffer, a NULL cache, scale or output pointer, a NULL q, or
 * (fused forms) NULL part / freqs or gemm_nsplit outside [1, 8]. */
int zk_attn_decode(const void* q, const void* k_cache, const void* vt_cache, int R, int H, int Hkv,
                   int hd, int Smax, int ctx0, const int32_t* ctx_dev, float* work, int nsplit,
                   void* out, const int32_t* skip, void* stream);
int zk_attn_prefill(const void* q, const void* k_cache, const void* vt_cache, int R, int S, int H,
                    int Hkv, int hd, int Smax, void* out, void* stream);
/* Decode with the in_proj epilogue fused in (= zk_qkv_rope at pos = ctx-1, S = 1, followed by
 * zk_attn_decode): reduces the in_proj slabs (gemm_nsplit x [R][(H+2Hkv)*hd] fp32), applies
 * RoPE, writes the new K / V^T cache entries and attends over keys [0, ctx). q is not stored. */
int zk_attn_decode_qkv(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                       void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                       const int32_t* ctx_dev, float* work, int nsplit, void* out, int rope_neox,
                       const int32_t* skip, void* stream);

/* zk_attn_decode_qkv with the split-KV partials merged inside the launch (no k_attn_combine):
 * counters = uint32 [R][Hkv], zeroed once before the first launch (each launch adds nsplit per
 * (row, kv head); the workgroup drawing the last ticket merges). nsplit == 1 or counters == NULL
 * launches what zk_attn_decode_qkv launches. Same results as the two-launch form, bit for bit. */
int zk_attn_decode_qkv_sc(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                          void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                          const int32_t* ctx_dev, float* work, int nsplit, uint32_t* counters, void* out,
                          int rope_neox, const int32_t* skip, void* stream);

/* zk_attn_decode_qkv_sc with a context per row (interleaved RoPE only): workgroup (split, kv head, r) uses
 * ctx_r = ctx0 + *ctx_dev + row_off[r], clamped into [1, Smax] on the device (row_off: device int32 [R]).
 * RoPE row ctx_r - 1, the new key's slot, the key range of every split and the mask all follow ctx_r, so row r
 * gets, bit for bit, what zk_attn_decode_qkv_sc gives it at that context; row_off all zero is that entry.
 * The rows of a batch whose prompts differ in length (_torch.py:33-49 keeps one position for the batch). */
int zk_attn_decode_qkv_sc_rows(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                               void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                               const int32_t* ctx_dev, const int32_t* row_off, float* work, int nsplit,
                               uint32_t* counters, void* out, const int32_t* skip, void* stream);

/* zk_attn_decode_qkv for nsplit >= 2 key ranges WITHOUT the merge: leaves the split partials
 * (m, l, unnormalised O per query head) in work [R][Hkv][nsplit][8 + 4*128] fp32 for the
 * consumer, zk_gemv_attn_out, which merges them in its prologue (replaces the
 * F.scaled_dot_product_attention output of _torch.py:64-65 feeding out_proj, :66). */
int zk_attn_decode_qkv_part(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                            void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                            const int32_t* ctx_dev, float* work, int nsplit, int rope_neox,
                            const int32_t* skip, void* stream);

/* Decode attention of the B = 1 step when q and the new key / value come from zk_gemv_qkv_rope:
 * F.scaled_dot_product_attention of one query per row over keys [0, ctx), ctx = min(ctx0 + *ctx_dev,
 * Smax) (_torch.py:64-65), with the keys split in 32-key slices over nsplit workgroups per (row, kv
 * head) (workgroup s, wave w: slices 4s + w + 4 nsplit j). Leaves the partials (m, l, unnormalised O)
 * in work [R][Hkv][nsplit][8 + 4*128] fp32 for zk_gemv_attn_out. nsplit <= 64. */
int zk_attn_decode_q_part(const void* q, const void* k_cache, const void* vt_cache, int R, int H, int Hkv,
                          int hd, int Smax, int ctx0, const int32_t* ctx_dev, float* work, int nsplit,
                          const int32_t* skip, void* stream);

/* ------------------------------------------------------------------ FP8 (e4m3fn) KV cache
 * The same attention (F.scaled_dot_product_attention, _torch.py:136, over the cache kept by
 * _update_kv_cache, _torch.py:33-49) with K and V stored as OCP e4m3fn bytes plus one power-of-two scale
 * per (row, kv head, key) for K and one for V (byte b = 2^(b-127), uint8 [R][Hkv][Smax]). Layout and the
 * exact scale rule: zonos_amd.kvlayout (K8: [R][Hkv][Smax/32][h 2][kp 2][lane 64][q 2][8], V8:
 * [R][Hkv][Smax/32][dp 4][lane 64][q 2][8]). hd = 128, Smax % 128 == 0, interleaved RoPE only.
 * Every entry returns the bits the bf16 entry of the same role returns on the dequantised cache.
 *
 * zk_kv_quantize_e4m3: keys [0, S) of a bf16 fragment-order cache pair of Smax_src keys per (row, kv
 * head) (what zk_qkv_rope wrote during prefill, _torch.py:33-49) -> the FP8 cache of Smax keys and its
 * scales; destination keys >= S are left untouched. */
int zk_kv_quantize_e4m3(const void* k_src, const void* vt_src, int R, int Hkv, int hd, int S, int Smax_src,
                        void* k8, void* v8, void* k_scale, void* v_scale, int Smax, void* stream);
/* zk_attn_decode over the FP8 cache (replaces the same lines, _torch.py:64-65 / :136). */
int zk_attn_decode_f8(const void* q, const void* k8, const void* v8, const void* k_scale, const void* v_scale,
                      int R, int H, int Hkv, int hd, int Smax, int ctx0, const int32_t* ctx_dev, float* work,
                      int nsplit, void* out, const int32_t* skip, void* stream);
/* zk_attn_decode_qkv_sc over the FP8 cache (_torch.py:61-65 + apply_rotary_emb :18-30 + _update_kv_cache
 * :33-49): reduces the in_proj slabs, applies the interleaved RoPE, quantises the new key and value (one
 * amax over the 128 dims each), attends over keys [0, ctx) with the new key's dequantised values and
 * stores its bytes and scale bytes. counters non-NULL and nsplit > 1: in-launch combine as _sc;
 * otherwise the combine launch. = zk_qkv_rope at ctx - 1 into a bf16 scratch + the quantisation of
 * that key + zk_attn_decode_f8, bit for bit. */
int zk_attn_decode_qkv_f8(const float* part, int gemm_nsplit, const float* freqs, void* k8, void* v8,
                          void* k_scale, void* v_scale, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                          const int32_t* ctx_dev, float* work, int nsplit, uint32_t* counters, void* out,
                          const int32_t* skip, void* stream);
/* zk_attn_decode_qkv_f8 with a context per row, as zk_attn_decode_qkv_sc_rows (_torch.py:33-49, :61-65). */
int zk_attn_decode_qkv_f8_rows(const float* part, int gemm_nsplit, const float* freqs, void* k8, void* v8,
                               void* k_scale, void* v_scale, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                               const int32_t* ctx_dev, const int32_t* row_off, float* work, int nsplit,
                               uint32_t* counters, void* out, const int32_t* skip, void* stream);

/* ------------------------------------------------------------------ graphs and timing
 * The decode step is captured once into a hipGraph and replayed (the reference runs the
 * transformer step eagerly: model.py:138-142, 220-222). */
int zk_graph_begin(void* stream);
int zk_graph_end(void* stream, void** graph_exec);
int zk_graph_launch(void* graph_exec, int repeat, void* stream);
int zk_graph_destroy(void* graph_exec);
int zk_event_create(void** ev);
int zk_event_record(void* ev, void* stream);
int zk_event_elapsed_ms(void* start, void* end, float* ms);
int zk_event_destroy(void* ev);

/* ------------------------------------------------------------------ generation state machine
 * One step of the generate() loop body after the backbone (model.py:353-424). */
typedef struct zk_gen_state {
    int32_t* scal;        /* device int32[16]: 0 offset, 1 pos, 2 step, 3 done, 4 any_new_eos,
                             5 max_steps, 6 error flags */
    int32_t* eos_mode;    /* [B] */
    int32_t* steps_after; /* [B] */
    int32_t* remaining;   /* [B] */
    int32_t* stopping;    /* [B] */
    int32_t* act;         /* [B] eos_active for the current step */
    float* rp;            /* [B] repetition penalty in effect */
    int32_t* tok0;        /* [B*K] draw-0 tokens */
    int32_t* tok1;        /* [B*K] draw-1 (EOS resample) tokens */
    int64_t* delayed;     /* [B][K][Ld] delayed codes (model.py:295) */
    int32_t B, K, Ld, V;
    uint64_t seed;
    int32_t row_base;     /* global index of utterance 0 (batch sharding) */
    /* Noise mode. 0: the engine's keyed stream (seed, step, draw, row_base + b, codebook, token).
     * 1: torch's own GPU stream -- the values `torch.empty_like(probs).exponential_(1)` gives the
     * reference's sampler (sampling.py:26-28) when torch's CUDA generator holds (seed, noise_offset):
     * sampler call c (0 = the prefill sample, model.py:304; then one per decode step, model.py:365,
     * and one per EOS resample, model.py:388) reads the stream at Philox offset noise_offset +
     * c * noise_incr over the [B][K][V] tensor with grid-stride noise_stride (zk_torch_noise_policy). */
    int32_t noise_mode;
    uint64_t noise_offset;
    int32_t noise_stride;
    int32_t noise_incr;
} zk_gen_state;

/* Engine sampler: logits from the heads GEMM split-K slabs part [nsplit][2B][K*V] (rows
 * [0,B) cond, [B,2B) uncond), bf16-rounded per head (model.py:111), CFG-combined
 * (model.py:112-115), biased (model.py:322-324,353,360-362) and sampled. prefill=1 is the
 * first sample (model.py:304: no bias, no penalty). draw 1 = EOS resample (model.py:386-393):
 * a no-op unless some row has a new EOS. dbg_logits (nullable) receives the fp32 CFG logits
 * before bias [B][K][V]. The history is st->delayed[..., :scal[0]]; sp->rp_window must be in
 * [1, 512] (the window contract at zk_sample_logits), anything else is an error return. */
int zk_sample_heads(const float* part, int nsplit, const zk_gen_state* st, const zk_sampling_params* sp,
                    int prefill, int draw, float* dbg_logits, void* stream);
/* EOS protocol + frame write + counters (model.py:376-424); prefill=1 only writes the
 * first frame (model.py:310-319). */
int zk_eos_step(const zk_gen_state* st, int prefill, int prefix_len, void* stream);

/* ------------------------------------------------------------------ request batches
 * A batch of independent requests: utterance b samples with its own parameters and its own noise key and
 * runs the EOS protocol on its own, so its codes are what Zonos.generate (model.py:224-457) returns for
 * it at batch size 1, whatever else shares the batch. The reference has one sampling_params / cfg_scale
 * for the whole batch (model.py:224-247) and redraws EVERY row when any row emits its first EOS
 * (model.py:380-393), which couples the rows; zk_sample_heads / zk_eos_step keep that protocol. */
typedef struct zk_row_params {
    zk_sampling_params sp;   /* this utterance's, cfg_scale and force_full_length included */
    uint64_t seed;           /* keyed-noise seed */
    int32_t  key;            /* row index the noise is keyed by (in place of row_base + b) */
    int32_t  reserved;       /* 0 */
} zk_row_params;

/* zk_sample_heads with per-utterance parameters (replaces sample_from_logits' batch-wide arguments,
 * model.py:365,388, and the batch-wide cfg_scale of model.py:112-114): rows = device zk_row_params
 * [st->B]; workgroup (b, k) reads rows[b] with its other up-front loads. The noise is the keyed stream
 * of (rows[b].seed, step, draw, rows[b].key, codebook, token); st->seed / st->row_base are not read and
 * st->noise_mode must be 0 (torch's stream is one call per batch). draw 1 (model.py:386-393) runs for
 * row b only when row b itself has a new EOS (tok0[b*K] == EOS and !eos_mode[b]); every other row's
 * workgroups return. Per row this is zk_sample_heads at B = 1 with that row's parameters, bit for bit.
 * Window contract: 1 <= rows[b].sp.rp_window <= 512 for every b is the CALLER's to keep -- the
 * parameters are in device memory, which this entry cannot read; the kernel clamps the window to 512
 * columns, so a violation stays in bounds but does not match the reference. Errors before any launch:
 * a NULL argument (rows included), st->noise_mode != 0, V out of range. */
int zk_sample_heads_rows(const float* part, int nsplit, const zk_gen_state* st, const zk_row_params* rows,
                         int prefill, int draw, float* dbg_logits, void* stream);   /* rows: device [st->B] */
/* zk_eos_step for a request batch (model.py:376-424 per row): row b takes the draw-1 tokens iff row b
 * itself had the new EOS (model.py:380-393 at batch size 1), else the draw-0 tokens; hold-off,
 * remaining = min(remaining, 9), the MASK / EOS staircase, the counters and the done word are
 * zk_eos_step's. Per-row budgets are the host's: remaining[b] starts at n_b + 8 and Ld fits the largest
 * n_b; a row whose budget is spent is still stepped until the done word (its cells past the budget hold
 * MASK from the host's delay pattern, so it writes nothing there; the kernel does not freeze it). */
int zk_eos_step_rows(const zk_gen_state* st, int prefill, int prefix_len, void* stream);

/* ------------------------------------------------------------------ one decode step
 * The whole autoregressive step of Zonos.generate (model.py:322-424: _decode_one_token's
 * embed -> 26 blocks -> norm_f -> 9 heads -> CFG, then the sampler, the EOS protocol and the
 * delayed-frame write) enqueued on `stream` with no host synchronisation, exactly the launch
 * sequence of zonos_amd.engine.HipDecoder._decode_step (the Python engine calls this entry):
 * small = 1 (B <= 8): five launches per block (zk_gemv_fused LayerNorm prologues / residual
 * epilogues; attn_merge > 0: zk_gemv_qkv_rope + zk_attn_decode_q_part + zk_gemv_attn_out, or with
 * rope_neox zk_gemv_fused + zk_attn_decode_qkv_part + zk_gemv_attn_out); small = 0: seven
 * (split-K zk_gemm_bf16 + zk_attn_decode_qkv_sc + zk_resid_ln). Every position/offset is read
 * from st.scal on the device, so one call is captured once into a hipGraph and replayed.
 * Replaces the per-token Python loop body of model.py:322-424 for a C/C++ host.
 * kv_fp8 = 1 (opt-in FP8 KV cache; a zeroed field is the bf16 cache): the seven-launch sequence at any
 * batch size with zk_attn_decode_qkv_f8 as the attention; together with small = 1, or with a layer whose
 * scale pointers (zk_prefill: or the scratch pair) are missing, both entries fail before any launch.
 * w_fp8 = 1 (opt-in FP8 weights; a zeroed field is the bf16 weights): zk_decode_step runs the five-launch
 * sequence with the _w8 GEMV entries on each layer's byte images (the heads stay bf16); it fails before any
 * launch unless small = 1, kv_fp8 = 0 and every layer has its four images and scales. zk_prefill ignores
 * the field and uses the bf16 weights. */
typedef struct zk_step_layer {
    const void* ln1_w;    /* norm.weight / bias (bf16 [D]) */
    const void* ln1_b;
    const void* wqkv;     /* mixer.in_proj, packed (zk_pack_weights) */
    const void* wo;       /* mixer.out_proj, packed */
    const void* ln2_w;    /* norm2 */
    const void* ln2_b;
    const void* fc1;      /* mlp.fc1 in zk_permute_fc1 order, packed */
    const void* fc2;      /* mlp.fc2, packed */
    void* k_cache;        /* this layer's K / V^T cache (fragment order, Smax keys per (row, kv head));
                             kv_fp8: the e4m3fn byte caches K8 / V8 of zk_attn_decode_f8 */
    void* vt_cache;
    void* k_scale;        /* kv_fp8 only: the scale bytes uint8 [2B][n_kv][smax] of K and of V */
    void* v_scale;
    /* w_fp8 only: the packed e4m3fn images (zk_pack_weights_e4m3) of wqkv / wo / fc1 / fc2 and their
     * scale bytes uint8 [ceil64(N)] */
    const void* wqkv8;
    const void* wo8;
    const void* fc18;
    const void* fc28;
    const void* wqkv_scale;
    const void* wo_scale;
    const void* fc1_scale;
    const void* fc2_scale;
} zk_step_layer;

typedef struct zk_step_desc {
    int32_t B, n_layer, d_model, n_heads, n_kv, head_dim, d_ff, smax;
    int32_t split_qkv, split_o, split_fc2, split_heads;   /* split-K counts (small = 0) */
    int32_t attn_splits, attn_merge, rope_neox, small;
    float eps;
    int32_t kv_fp8;                /* 0: bf16 KV cache; 1: FP8 (e4m3fn) cache, small must be 0 (below) */
    const zk_step_layer* layers;   /* [n_layer] */
    const void* emb;               /* codebook embeddings bf16 [9][1026][D] */
    const void* heads;             /* 9 heads stacked, packed */
    const void* lnf_w;             /* norm_f */
    const void* lnf_b;
    const float* freqs;            /* RoPE table (engine.rope_table) */
    void* x;                       /* residual rows bf16 [2B][D] */
    void* xn;                      /* LayerNorm'd rows bf16 [2B][D] */
    void* y;                       /* attention output bf16 [2B][H*hd] */
    void* h;                       /* SwiGLU output bf16 [2B][d_ff] */
    float* part;                   /* split-K slabs / logits */
    float* attn_work;              /* split-KV partials */
    uint32_t* attn_cnt;            /* in-launch combine tickets [2B][Hkv] */
    float* dbg;                    /* nullable: fp32 CFG logits of draw 0 */
    zk_gen_state st;
    zk_sampling_params sp;
    /* kv_fp8 only, read by zk_prefill: one bf16 fragment-order K / V^T scratch pair of pre_smax keys per
     * (row, kv head) (pre_smax % 32 == 0, >= S), reused by every layer: zk_qkv_rope and zk_attn_prefill
     * run on it unchanged, then zk_kv_quantize_e4m3 fills the layer's FP8 cache. */
    void* pre_k;
    void* pre_vt;
    int32_t pre_smax;
    int32_t w_fp8;                 /* 0: bf16 weights; 1: FP8 (e4m3fn) layer weights, small must be 1 (above) */
    /* NULL (a zeroed field): the batch-wide sampler and EOS protocol above. Non-NULL, device
     * zk_row_params [B]: a request batch -- zk_decode_step and zk_prefill enqueue zk_sample_heads_rows /
     * zk_eos_step_rows in place of zk_sample_heads / zk_eos_step (sp, st.seed and st.row_base are then
     * not read); with st.noise_mode == 1 both fail before any launch. */
    const zk_row_params* rows;
} zk_step_desc;

int zk_decode_step(const zk_step_desc* d, void* stream);

/* The prefill of Zonos.generate (model.py:297-319, _prefill 181-202) on the same descriptor:
 * x rows [2B][S][D] = [prefix conditioning (cond, bf16 [2B][Lc][D]) | codebook embeddings of the
 * P audio-prefix frames + the first delayed frame], layer 0's LayerNorm, the 26 blocks over all
 * 2B*S positions (split-K 1, causal prefill attention filling the KV cache), the heads on the
 * last position, the first sample (model.py:304: no bias, no penalty) and the first frame write.
 * S = Lc + P + 1; q: bf16 [2B*S][H*hd] scratch; x / xn / y / h / part sized for 2B*S rows.
 * The loop state (st.scal, eos_mode, ...) is initialised by the host afterwards (model.py:316-342).
 * Fails (-1, before any launch) unless smax >= Lc + st.Ld, the context of the last decode step. */
int zk_prefill(const zk_step_desc* d, const void* cond, int Lc, int P, void* q, void* stream);

/* The two entries above for a batch whose conditionings differ in length (a request batch, rows != NULL, is
 * the use; the reference pads every text to the longest and attends to the pad tokens, conditioning.py). Every
 * row is left-aligned at position 0: row r holds cond_r (Lc_r tokens), then the P + 1 embedded frames.
 * row_off: device int32 [2B], row_off[r] = Lc_r - Lc <= 0 with Lc the longest (the cond and the uncond row of an
 * utterance alike), fixed for the generation, so a captured step replays with it. NULL: the entries above.
 * Row r's position at a step is st.scal[1] + row_off[r], its context one more; st.scal[1] counts from
 * S = Lc + P + 1 as before and the descriptor's buffers and smax are sized by Lc.
 * zk_prefill_rows: cond is bf16 [2B][Lc][D], zero-padded at the end. The frames of row r are embedded at
 * positions Lc + row_off[r] ... (zk_embed_codes_rows), the P + 1 positions behind Lc are zeroed first, so every
 * position behind a row's own S_r = Lc_r + P + 1 holds zeros and its keys are finite (the causal prefill
 * computes a row's valid positions exactly as it computes them alone); the heads read each row's last valid
 * position (zk_gather_last_rows into y). zk_decode_step_rows: zk_attn_decode_qkv_sc_rows /
 * zk_attn_decode_qkv_f8_rows as the attention. Both fail before any launch with attn_merge > 0, with rope_neox,
 * or in a build without those kernels. (The offsets are an argument, not a descriptor field: zk_step_desc
 * keeps its size and `rows` stays its last field.) */
int zk_decode_step_rows(const zk_step_desc* d, const int32_t* row_off, void* stream);
int zk_prefill_rows(const zk_step_desc* d, const void* cond, int Lc, int P, void* q, const int32_t* row_off,
                    void* stream);

/* ------------------------------------------------------------------ hybrid decode step
 * The same two entries for the Zonos-v0.1-hybrid backbone (zonos/backbone/_mamba_ssm.py:9-57 ->
 * mamba_ssm create_block: Mamba2 mixers, MHA + GatedMLP at attn_layer_idx, fused add + LayerNorm
 * of the fp32 sum), the launch sequence of zonos_amd.hybrid.HybridDecoder:
 *   Mamba2 layer : in_proj GEMM -> zk_mamba_step (conv + SSM state update, y * silu(z)) ->
 *                  zk_gated_rmsnorm -> out_proj GEMM -> zk_resid_ln(ln_on_sum = 1, next norm)
 *   attention    : Wqkv GEMM -> zk_attn_decode_qkv (GPT-NeoX RoPE) -> out_proj -> zk_resid_ln(norm2)
 *                  -> fc1 (SwiGLU) -> fc2 -> zk_resid_ln(next norm)
 * (a Mamba2 block with d_mlp > 0 continues like the attention block from zk_resid_ln(norm2); with
 * norm_flags != 0 the first block's norm is its own zk_resid_ln(nsplit = 0) after the embedding)
 * then norm_f, the 9 heads, the sampler and the EOS protocol exactly as zk_decode_step. Conv and
 * SSM states are double-buffered by step parity ({a, b}, zk_mamba_step). Replaces the
 * `_decode_one_token` / `_prefill` bodies of model.py:118-202 for the mamba_ssm backbone (the one
 * the reference CUDA-graph-captures, model.py:220-222). */
typedef struct zk_hybrid_layer {
    int32_t type;           /* 0 attention block, 1 Mamba2 block */
    int32_t d_mlp;          /* Mamba2 block: GatedMLP width (d_intermediate; 0 = no norm2 / MLP, the
                               Zonos-v0.1-hybrid case); attention block: 0 = d_ff of the descriptor */
    const void* ln1_w;      /* norm.weight / bias (bf16 [D]; ln1_b NULL under rms_norm) */
    const void* ln1_b;
    /* attention block (norm2 / mlp also of a Mamba2 block with d_mlp > 0) */
    const void* wqkv;       /* mixer.in_proj, packed */
    const void* wo;         /* mixer.out_proj, packed */
    const void* ln2_w;      /* norm2 (ln2_b NULL under rms_norm: bias-free RMSNorm) */
    const void* ln2_b;
    const void* fc1;        /* mlp.fc1 (zk_permute_fc1 order), packed */
    const void* fc2;        /* mlp.fc2, packed */
    void* k_cache;          /* fragment-order K / V^T caches */
    void* vt_cache;
    /* Mamba2 block */
    const void* w_in;       /* mixer.in_proj, packed [2 d_inner + 2 d_state + nheads][D] */
    const float* conv_w;    /* conv1d weight fp32 [conv_dim][4] */
    const float* conv_b;    /* conv1d bias fp32 [conv_dim] */
    const float* A;         /* -exp(A_log) fp32 [nheads] */
    const float* dt_bias;   /* fp32 [nheads] */
    const float* Dskip;     /* D fp32 [nheads] */
    const float* norm_w;    /* RMSNormGated weight fp32 [d_inner] */
    const void* w_out;      /* mixer.out_proj, packed [D][d_inner] */
    void* conv_state[2];    /* bf16 [R][conv_dim][4], parity buffers */
    void* ssm_state[2];     /* bf16 [R][nheads][headdim][d_state], parity buffers */
} zk_hybrid_layer;

typedef struct zk_hybrid_desc {
    int32_t B, n_layer, d_model, n_heads, n_kv, head_dim, d_ff, smax;
    int32_t d_inner, nheads_ssm, headdim_ssm, d_state;
    int32_t split_qkv, split_o, split_fc2, split_heads, split_inp, split_out, attn_splits;
    int32_t norm_flags;            /* BackboneConfig variants: bit 1 rms_norm (block norms are bias-free
                                      RMSNorms, norm_f an RMS norm with its bias), bit 2 residual_in_fp32
                                      (residual stream in xf, fp32); 0 = Zonos-v0.1-hybrid */
    float eps;                     /* LayerNorm eps (norm_epsilon) */
    float gate_eps;                /* RMSNormGated eps (1e-5 in mamba_ssm Mamba2) */
    const zk_hybrid_layer* layers; /* [n_layer] */
    const void* emb;               /* codebook embeddings bf16 [9][1026][D] */
    const void* heads;             /* 9 heads stacked, packed */
    const void* lnf_w;             /* norm_f */
    const void* lnf_b;
    const float* freqs;            /* bf16-rounded cos/sin cache [pos][hd/2][2] (rope_neox) */
    void* x;                       /* residual rows bf16 [rows][D] */
    void* xn;                      /* LayerNorm'd rows bf16 */
    void* y;                       /* attention output bf16 [rows][H*hd] */
    void* h;                       /* SwiGLU output bf16 [rows][d_ff] */
    float* part;                   /* split-K slabs / logits */
    float* attn_work;              /* split-KV partials */
    float* yz;                     /* Mamba y * silu(z) fp32 [rows][d_inner] */
    void* ym;                      /* RMSNormGated output bf16 [rows][d_inner] */
    void* xc;                      /* prefill conv scratch bf16 [rows][conv_dim] */
    float* dbg;                    /* nullable: fp32 CFG logits of draw 0 */
    zk_gen_state st;
    zk_sampling_params sp;
    void* xf;                      /* residual rows fp32 [rows][D] (norm_flags bit 2; else unused) */
    const zk_row_params* rows;     /* NULL, or a request batch: as zk_step_desc.rows, for the two entries below */
} zk_hybrid_desc;

int zk_hybrid_decode_step(const zk_hybrid_desc* d, void* stream);
int zk_hybrid_prefill(const zk_hybrid_desc* d, const void* cond, int Lc, int P, void* q, void* stream);

/* ------------------------------------------------------------------ DAC decoder
 * (zonos/autoencoder.py:44-47 -> modeling_dac.py:610-640). fp32 activations, layout
 * [B][C][T] (channels-first, like torch). Per-row valid lengths (in frames) make a
 * padded batch decode identical to per-utterance decode (autoencoder.py:219-226). */

/* E_k[c][ch] = out_proj_k(codebook_k[c]) + bias_k  (modeling_dac.py:364-370), k < ncb. */
int zk_dac_rvq_tables(const float* codebooks, const float* out_w, const float* out_b, int ncb,
                      int ncode, int cdim, int hidden, float* tables, void* stream);
/* z[b][ch][t] = sum_k E_k[codes[b][k][t]][ch] (sequential fp32, k ascending). */
int zk_dac_rvq_decode(const int64_t* codes, int B, int ncb, int T, long code_bstride,
                      const float* tables, int ncode, int hidden, float* z, int Tz,
                      const int32_t* lens, void* stream);
/* Generic conv over time with fused Snake input activation and epilogue:
 *   out[b][co][t_out(q)] = bias[co] + sum_{ci,k} W[co][ci][k] * act(in[b][ci][q + k*dil - pad])
 *                          (+ resid[b][co][t_out]) (tanh if do_tanh)
 * t_out(q) = q*out_stride + out_off. act = Snake(alpha) if alpha != NULL (modeling_dac.py:95-100).
 * in positions outside [0, len_in_b) read as 0; len_in_b = lens[b]*in_scale (lens NULL => Tin).
 * Outputs outside [0, len_out_b) are written as 0. */
int zk_dac_conv(const float* in, int B, int Cin, int Tin, const float* alpha,
                const float* w, const float* bias, int Cout, int ks, int dil, int pad,
                int Qn, int out_stride, int out_off, float* out, int Tout, const float* resid,
                int do_tanh, const int32_t* lens, int in_scale, int out_scale, void* stream);
/* ConvTranspose1d weight [Cin][Cout][2s] -> s polyphase 2-tap conv weights
 * [s][Cout][Cin][2] so that zk_dac_conv(ks=2, pad=1, out_stride=s, out_off=r-ceil(s/2)). */
int zk_dac_prep_convt(const float* w, int Cin, int Cout, int s, float* w_out, void* stream);

/* fp16-MFMA variant of zk_dac_conv (same semantics). npass = 3: split precision
 * (hi/lo fp16 operands, hi*hi + lo*hi + hi*lo, ~fp32 accuracy); npass = 1: plain fp16
 * operands (the reference's own GPU numerics: autocast fp16, autoencoder.py:46).
 * Weights prepacked by zk_dac_prep_w16: mode 0 conv [Cout][Cin][ks] -> [ks][Cout][Cin];
 * mode 1 ConvTranspose1d [Cin][Cout][2s] -> [s][2][Cout][Cin] (phase r at offset 2*r*Cout*Cin,
 * run with ks=2, dil=1, pad=1, out_stride=s, out_off=r-ceil(s/2)). Cin % 32 == 0. w_lo may be
 * NULL (plain fp16 packing). */
int zk_dac_prep_w16(const float* w, int Cout, int Cin, int ks, int s, int mode, uint16_t* w_hi,
                    uint16_t* w_lo, void* stream);
int zk_dac_conv16(const float* in, int B, int Cin, int Tin, const float* alpha, const uint16_t* w_hi,
                  const uint16_t* w_lo, const float* bias, int Cout, int ks, int dil, int pad,
                  int Qn, int out_stride, int out_off, float* out, int Tout, const float* resid,
                  int do_tanh, const int32_t* lens, int in_scale, int out_scale, int npass, void* stream);
/* Final Snake -> Conv1d(C -> 1, k7, pad 3) -> tanh (modeling_dac.py:437-439); out [B][T]. */
int zk_dac_tail(const float* in, int B, int C, int T, const float* alpha, const float* w,
                const float* bias, float* out, const int32_t* lens, int scale, void* stream);

/* ---- channels-last fp16 pipeline (default "fp16" precision; dac_cl.hip). Activations are
 * s = fp16(Snake(x)) [B][T][C] with C padded to a multiple of 32 (zero channels), the
 * residual stream x fp32 [B][T][C]. Each conv applies the NEXT Snake in its epilogue. */
/* z[b][t][ch] = fp16(sum_k E_k[codes[b][k][t]][ch]) (k ascending), channels [hidden, cpad) = 0. */
int zk_dac_rvq_decode_cl(const int64_t* codes, int B, int ncb, int T, long code_bstride,
                         const float* tables, int ncode, int hidden, int cpad, uint16_t* z,
                         const int32_t* lens, void* stream);
/* For q < Qn, phase r < nphase, t = q*out_stride + out_off0 + r in [0, Tout):
 *   v = bias[co] + sum_{ci,k} W_r[k][co][ci] * in[b][q + k*dil - pad][ci]  (+ resid[b][t][co])
 *   x_out[b][t][co] = v (if x_out);  s_out[b][t][co] = fp16(Snake_{alpha_next}(v))
 *   (s_f32 = 1: s_out is fp32 and the Snake uses the exact sinf -- the input of zk_dac_tail_cl)
 * W_r = w + r*w_phase_stride (zk_dac_prep_w16 hi layout). Inputs outside [0, lens[b]*in_scale)
 * read 0; outputs at t >= lens[b]*out_scale are written 0. Cin, Cout % 32 == 0; ks <= 7,
 * (ks-1)*dil <= 64. Conv1d: nphase=1, out_stride=1, out_off0=0. ConvTranspose1d(stride s):
 * ks=2, dil=1, pad=1, Qn=Tin+1, nphase=s, out_stride=s, out_off0=-ceil(s/2).
 * How a shape is launched (workgroup shape, tile, LDS, tiles): zk_dac_conv_plan below. */
int zk_dac_conv_cl(const uint16_t* in, int B, int Cin, int Tin, const uint16_t* w, long w_phase_stride,
                   const float* bias, int Cout, int ks, int dil, int pad, int Qn, int nphase,
                   int out_stride, int out_off0, int Tout, const float* resid, float* x_out,
                   const float* alpha_next, void* s_out, int s_f32, const int32_t* lens, int in_scale,
                   int out_scale, void* stream);
/* One whole DAC residual unit (modeling_dac.py:222-233, ResidualUnit.forward) in one launch:
 *   y  = b7 + conv7_dil(s_in)                      (s_in = fp16 Snake_a1(x), [B][T][C])
 *   s2 = fp16(Snake_a2(y));  v = x + b1 + W1 s2     (1x1 conv; the fp16 s2 never leaves the chip)
 *   x[b][t][c] = v;  s_out[b][t][c] = fp16(Snake_{alpha_next}(v))  (s_f32 = 1: fp32, exact sinf)
 * Replaces the pair zk_dac_conv_cl(k7 -> s2) + zk_dac_conv_cl(1x1, resid = x); the same masking
 * (inputs at t >= lens[b]*scale read 0, outputs there written 0). w7 fp16 [7][C][C], w1 fp16
 * [C][C] (zk_dac_prep_w16 layouts). s_out must not alias s_in. Built for C = 96, 192; the 1x1 sums
 * run on 16x16x16 MFMAs (a different fp32 summation grouping than the 32-deep unfused conv:
 * results equal to rounding, not bit for bit). zk_dac_resunit_supported(C): 0 = not fused at this
 * C, 1 = fused except the decode's last unit (the fp32-Snake one), 2 = every unit; zk_dac_decode
 * and the Python-issued sequence both follow it. */
int zk_dac_resunit_supported(int C);
int zk_dac_resunit_cl(const uint16_t* s_in, int B, int C, int T, const uint16_t* w7, const float* b7, int dil,
                      const float* a2, const uint16_t* w1, const float* b1, float* x, const float* alpha_next,
                      void* s_out, int s_f32, const int32_t* lens, int scale, void* stream);
/* The launch plan of zk_dac_conv_cl (fused = 0; resid, s_f32: whether it gets a residual / writes the fp32
 * Snake) or of zk_dac_resunit_cl (fused = 1: C = Cout, T = Qn; Cin, ks, nphase, resid are not read), by the
 * entries' own shape checks and rule. Host only: no GPU is touched. Fills plan[ZK_DAC_PLAN_N]:
 *   0 workgroup shape (0 pair: two per CU, 1 fat: one per CU, 2 fused C = 96, 3 fused C = 192)
 *   1 FM (16-row MFMA blocks of output channels per wave)   2 positions per tile
 *   3 dx (steps the input windows are loaded ahead)         4 nx (window ring slots)
 *   5 dynamic LDS bytes per workgroup                       6 position tiles per row
 *   7 tiles in all = B * [6] * channel tiles * nphase       8 workgroups per CU the shape is built for
 * Returns 0, or -1 with zk_last_error set where the entry would refuse the shape. */
#define ZK_DAC_PLAN_N 9
int zk_dac_conv_plan(int fused, int B, int Cin, int Cout, int ks, int dil, int Qn, int nphase, int resid,
                     int s_f32, int32_t* plan);
/* out[b][t] = tanh(bias + sum_{c,k} w[c*7+k] * s[b][t+k-3][c]), 0 at t >= lens[b]*scale
 * (s = fp32 output of the final Snake, zk_dac_conv_cl with s_f32 = 1; modeling_dac.py:437-439). */
int zk_dac_tail_cl(const float* s, int B, int C, int T, const float* w, const float* bias,
                   float* out, const int32_t* lens, int scale, void* stream);

/* The whole channels-last DAC decode (DACAutoencoder.decode, autoencoder.py:44-47 ->
 * DacModel.decode, modeling_dac.py:610-640) as one call: RVQ lookup -> conv1 -> per block
 * ConvTranspose1d + 3 residual units (k7 dilated + 1x1 with the residual add) -> Snake -> conv2
 * -> tanh, the launch sequence of zonos_amd.autoencoder.HipDacDecoder._decode_cl. Weights in the
 * zk_dac_conv_cl layouts (channels padded to 32; zk_dac_prep_w16). codes int64 [B][ncb][T];
 * lens int32 [B] frames (nullable = all T); out fp32 [B][1][T * prod(strides)]; workspace of
 * zk_dac_decode_workspace(d, B, T) bytes (device memory). */
#define ZK_DAC_MAXB 6
#define ZK_DAC_MAXR 3
typedef struct zk_dac_resunit {
    int32_t dil;
    const float* a1;       /* Snake alpha before the k7 conv */
    const uint16_t* w1;    /* k7 conv, fp16 [7][C][C] */
    const float* b1;
    const float* a2;       /* Snake alpha before the 1x1 conv */
    const uint16_t* w2;    /* 1x1 conv, fp16 [1][C][C] */
    const float* b2;
} zk_dac_resunit;
typedef struct zk_dac_block {
    int32_t stride, cin, cout, nres;
    const float* alpha;    /* Snake alpha before the ConvTranspose1d */
    const uint16_t* wt;    /* ConvTranspose1d, fp16 [stride][2][cout][cin] */
    const float* bt;
    zk_dac_resunit res[ZK_DAC_MAXR];
} zk_dac_block;
typedef struct zk_dac_desc {
    int32_t nblocks, ncb, codebook_size, hidden, cin0, c0;
    const float* tables;   /* RVQ codebooks projected to the latent (zk_dac_rvq_decode_cl) */
    const uint16_t* conv1_w;
    const float* conv1_b;
    const float* final_alpha;
    const float* conv2_w;  /* [C][7] fp32 */
    const float* conv2_b;
    zk_dac_block blocks[ZK_DAC_MAXB];
} zk_dac_desc;
size_t zk_dac_decode_workspace(const zk_dac_desc* d, int B, int T);
int zk_dac_decode(const zk_dac_desc* d, const int64_t* codes, int B, int T, const int32_t* lens, void* workspace,
                  size_t workspace_bytes, float* out, void* stream);

/* ---- Streaming: audio chunks of a generation that is still running (stream.hip). The reference decodes after
 * generate() has returned (model.py:437-457, then autoencoder.py:44-47); these entries do the same work on a
 * window of final frames. codes[b][k][t] = delayed[b][k][t + k + 1], so frame t is whole once column t + K is
 * written: at a poll that read off = scal[0] - 1 the host passes upto = off - K BY VALUE (the device word moves
 * on while the kernels run) and frames < upto are final. Windows are [f0, f1) in absolute code frames. */
/* Window assembly: revert_delay_pattern (codebook_pattern.py), the `>= 1024 -> 0` fill and the per-row slice of
 * model.py:437-451 on a window. delayed int64 [B][K][Ld]; P = audio-prefix frames; P <= f0 < f1; 0 <= upto <= Ld - K.
 * end int32 [B]: the row's end frame if a first EOS (1024) of codebook 0 lies at a frame in [1, upto) -- model.py:439-440,
 * argmax then `eos_pos == 0 -> length`, so an EOS at frame 0 counts as none and hides later ones -- else -1 (the row is
 * live; its end is taken as upto). codes_w int64
 * [B][K][f1 - f0]: un-delayed codes, ids >= 1024 and frames at or past the row's end as 0. lens_w int32 [B] =
 * clamp(end_b - f0, 0, f1 - f0). Reads only columns < upto + K. */
int zk_stream_window(const int64_t* delayed, int B, int K, int Ld, int P, int f0, int f1, int upto, int64_t* codes_w,
                     int32_t* lens_w, int32_t* end, void* stream);
/* The chunk [c0, c1) out of the window's waveform wav_w fp32 [B][1][(f1 - f0) hop] (f0 <= c0 < c1 <= f1): samples
 * [(c0 - f0) hop, (min(end_b, c1) - f0) hop) of each row into chunk fp32 [B][(c1 - c0) hop], zero behind them; their
 * count into n int32 [B] (0 for a row that ended before c0). end as zk_stream_window wrote it (-1: the row reaches c1). */
int zk_stream_crop(const float* wav_w, int B, int hop, int f0, int c0, int c1, int f1, const int32_t* end, float* chunk,
                   int32_t* n, void* stream);
/* zk_stream_window -> the zk_dac_decode sequence on (codes_w, lens_w) -> zk_stream_crop, for the default fp16 pipeline.
 * Refused before any launch, with zk_last_error starting "zk_stream_chunk:": a NULL pointer, f0 < P, a window not ordered
 * f0 <= c0 < c1 <= f1, f1 > upto (only the device knows which rows have ended, so the host clamps f1 = min(c1 + H, upto)
 * for every window; the kernel clamps through the row's end as well), upto > Ld - K, a workspace smaller than
 * zk_stream_workspace(d, f1 - f0). workspace: device memory (window codes, lens, window waveform, the DAC workspace). */
typedef struct zk_stream_desc {
    const zk_dac_desc* dac;
    const int64_t* delayed;    /* [B][K][Ld], the running generation's delayed codes (zk_gen_state.delayed) */
    int32_t B, K, Ld, P;
} zk_stream_desc;
size_t zk_stream_workspace(const zk_stream_desc* d, int Wmax);    /* bytes for windows of <= Wmax frames; 0 if invalid */
int zk_stream_chunk(const zk_stream_desc* d, int f0, int c0, int c1, int f1, int upto, void* workspace,
                    size_t workspace_bytes, float* chunk_out, int32_t* n_out, int32_t* end_out, void* stream);

/* ---- DAC encoder (prefix audio -> codes; DACAutoencoder.encode, autoencoder.py:27-28 ->
 * DacModel.encode). Convolutions run on zk_dac_conv_cl (channels-last fp16 operands); a strided
 * Conv1d(k = 2s, stride s, pad ceil(s/2)) runs as a stride-1 3-tap conv over the input folded to
 * [T/s][s*C] (weights repacked on the host). zk_dac_conv_cl accepts s_out = NULL (x_out only). */
/* conv1 (1 -> C, k7, pad 3) of wav fp32 [B][T]: x_out fp32 [B][T][Cp], s_out = fp16(Snake(x)). */
int zk_dac_enc_conv1(const float* wav, int B, int T, const float* w, const float* bias,
                     const float* alpha_next, int C, int Cp, float* x_out, uint16_t* s_out, void* stream);
/* Residual VQ encode of z fp32 [B][T][hidden] -> codes int64 [B][ncb][T]: per codebook
 * e = normalize(in_w z + in_b); code = argmax_n -(|e|^2 - 2 e.cn_n) + |cn_n|^2 (first on ties,
 * cn = normalised codebook); z -= out_w cb[code] + out_b (modeling_dac DacVectorQuantize). */
int zk_dac_rvq_encode(const float* z, int B, int T, int hidden, int ncb, int ncode, int cdim,
                      const float* in_w, const float* in_b, const float* cb_norm, const float* cb_norm_sq,
                      const float* cb, const float* out_w, const float* out_b, int64_t* codes, void* stream);

/* Resampler of DACAutoencoder.preprocess (autoencoder.py:21-25 -> torchaudio.functional.resample,
 * sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): x fp32 [B][T] -> out fp32 [B][Tout],
 * out[n] = sum_k kern[n % up][k] * x[(n / up) * down + k - width] (zero outside [0, T)), where
 * up/down = new/orig rate over their gcd and kern [up][K = 2 width + down] the windowed-sinc table. */
int zk_resample(const float* x, int B, long T, const float* kern, int up, int down, int width, int K,
                float* out, long Tout, void* stream);

/* ---- PrefixConditioner.forward (zonos/conditioning.py:373-389; Zonos.prepare_conditioning,
 * model.py:210-218): conditioner rows -> concat over the sequence -> prefix projection ->
 * LayerNorm, one launch, out bf16 [B][L][D]. A plan lists the segments in the conditioners'
 * order; a segment's input batch `bin` is 1 (broadcast, the reference's expand) or B. */
#define ZK_COND_MAXSEG 16
#define ZK_COND_MAXIN 64
enum { ZK_SEG_VECTOR = 0,   /* learned uncond vector: table bf16 [D], len 1 */
       ZK_SEG_EMBED = 1,    /* embedding: input int64 ids [bin][in_bstride], row = table[id - id_min] */
       ZK_SEG_FOURIER = 2,  /* Fourier: input fp32 [bin][len][in_dim], table = W bf16 [cin/2][in_dim] */
       ZK_SEG_PASS = 3 };   /* passthrough: input bf16 [bin][len][cin] */
typedef struct {
    int type, len, cin, in_dim, bin, proj;   /* proj: 0 none, 1 linear, 2 mlp (conditioning.py:27-34) */
    long in_bstride, id_min;
    float vmin, vden;                        /* Fourier: (x - vmin) / vden */
    const void* table;
    const void* input;
    const void* pw0; const void* pb0; const void* pw1; const void* pb1;   /* bf16 projection [D][cin], [D][D] */
} ZkCondSeg;
typedef struct {
    int nseg, D, L, proj;
    float eps;
    const void* pw0; const void* pb0; const void* pw1; const void* pb1;   /* prefix projection */
    const void* norm_w; const void* norm_b;                                /* LayerNorm (NULL: none) */
    ZkCondSeg seg[ZK_COND_MAXSEG];
} ZkCondPlan;
int zk_prefix_cond(const ZkCondPlan* plan, int B, void* out, void* stream);

/* ------------------------------------------------------------------ hybrid backbone: Mamba2 mixer
 * (zonos/backbone/_mamba_ssm.py -> mamba_ssm Mamba2; restated in oracle/hybrid_ref.py).
 * in_proj output columns [z (d_inner) | xBC (conv_dim = d_inner + 2 d_state) | dt (nheads)].
 * Conv state bf16 [R][conv_dim][4] (last 4 inputs), double-buffered by step parity: the step at
 * position *pos_dev reads buffer (pos & 1) of {a, b} and writes the other. SSM state bf16
 * [R][nheads][headdim][d_state]: updated in place when ssm_state_b is NULL, otherwise
 * double-buffered like the conv state ({ssm_state, ssm_state_b}: read (pos & 1), write the other;
 * the in-place read-modify-write of the same lines streams ~5 % slower). A = -exp(A_log), dt_bias, D fp32 [nheads]; conv_w fp32
 * [conv_dim][4], conv_b fp32 [conv_dim]. yz (fp32 [rows][d_inner]) = bf16(C.h + D x) * silu(z),
 * normalised by zk_gated_rmsnorm (RMSNormGated, norm_before_gate=False) into the out_proj input.
 * (headdim, d_state) in {(64,128), (64,64), (32,64)}. */
int zk_mamba_step(const float* part, int gemm_nsplit, int R, int d_inner, int nheads, int headdim,
                  int d_state, const float* conv_w, const float* conv_b, void* conv_state_a,
                  void* conv_state_b, const int32_t* pos_dev, void* ssm_state, void* ssm_state_b,
                  const float* A, const float* dt_bias, const float* D, float* yz, const int32_t* skip,
                  void* stream);
/* zk_mamba_step computed by the per-(head, row) kernel instead of the grouped one: same arguments,
 * same results (bit for bit, or within 1 bf16 ulp of y where the C.h row sum is reduced in another
 * order). The verification twin of zk_mamba_step; not on the decode path. */
int zk_mamba_step_per_head(const float* part, int gemm_nsplit, int R, int d_inner, int nheads, int headdim,
                           int d_state, const float* conv_w, const float* conv_b, void* conv_state_a,
                           void* conv_state_b, const int32_t* pos_dev, void* ssm_state, void* ssm_state_b,
                           const float* A, const float* dt_bias, const float* D, float* yz, const int32_t* skip,
                           void* stream);
/* prefill over S positions per row: zx = in_proj output fp32 [R*S][cols] (split 1); xc_scratch
 * bf16 [R*S][conv_dim]; conv_state receives the last 4 inputs (the buffer the first decode step
 * reads); ssm_state receives the final state (bf16; with double-buffered decode states, the
 * buffer the first decode step reads). */
int zk_mamba_prefill(const float* zx, int R, int S, int d_inner, int nheads, int headdim, int d_state,
                     const float* conv_w, const float* conv_b, void* xc_scratch, void* conv_state,
                     void* ssm_state, const float* A, const float* dt_bias, const float* D, float* yz,
                     void* stream);
int zk_gated_rmsnorm(const float* g, int rows, int d_inner, const float* w, float eps, void* out,
                     const int32_t* skip, void* stream);

/* ------------------------------------------------------------------ codes_to_wavs post-processing
 * Loudness of each decoded utterance as normalize_loudness measures it (autoencoder.py:172-186
 * -> pyloudnorm 0.1.1 Meter(rate, block).integrated_loudness, BS.1770-4 K-weighting + gating;
 * block 0.4 s if the utterance is longer than 2 s else 0.1 s). wav fp32 [B][T] (row b valid for
 * lens[b] samples, NULL = T). gains[b] = 10^((target - L_b)/20), loudness[b] = L_b; utterances
 * shorter than one block get gain 1 and loudness NaN (the reference's except path).
 * scratch: fp64, B*T + B*zk_loudness_max_blocks(T, rate) elements. */
int zk_loudness_max_blocks(long T, int rate);
int zk_loudness_gains(const float* wav, int B, long T, const int32_t* lens, int rate, double target_lufs,
                      double* scratch, double* gains, double* loudness, void* stream);

/* ------------------------------------------------------------------ speaker embedding (voice cloning)
 * zonos/speaker_cloning.py: SpeakerEmbeddingLDA (:387-411) = logFbankCal (:12-34) -> ResNet293 of
 * SimAMBasicBlock (:63-95, :152-195) -> ASP (:37-60) -> bottleneck Linear (:213, :222) -> LDA Linear
 * (:404, :411). Activations are channels-last [B][F][T][C] (F mel rows, T frames): x fp32 (residual
 * stream) and s fp16 (the next conv's input). Channel counts are multiples of 32. */
/* logFbankCal on 16 kHz mono wav fp32 [B][n], n > 256: MelSpectrogram(n_fft 512, win 400, hop 160,
 * center + reflect padding, power 2, HTK mel scale, no filter norm), log(x + 1e-6), minus the mean
 * over time -> out fp32 [B][n_mels][T], T = 1 + n / 160. window fp32 [512] (Hann of 400 zero-padded
 * centrally), twiddle fp64 [512][2] (cos, sin of 2 pi j / 512), melfb fp32 [257][n_mels]: host tables. */
int zk_spk_logfbank(const float* wav, int B, int n, const float* window, const double* twiddle,
                    const float* melfb, int n_mels, float* out, void* stream);
/* ResNet.conv1 + bn1 + relu (:169-171, :186): feat fp32 [B][F][T] -> x fp32, s fp16 [B][F][T][C];
 * w fp32 [C][9] (kh major), scale / shift the eval-mode BatchNorm. */
int zk_spk_stem(const float* feat, int B, int F, int T, const float* w, const float* scale, const float* shift,
                int C, float* x, uint16_t* s, void* stream);
/* Conv2d (ks 3 pad 1, or ks 1 pad 0; stride 1 or 2 on both axes; no bias) + eval-mode BatchNorm as fp32
 * scale / shift [Cout] + optional ReLU. in fp16 [B][Fi][Ti][Cin]; w fp16 packed
 * [ceil(Cout / 64)][Cin / 32][kh * ks + kw][64][32] (rows past Cout zero); outputs [B][Fo][To][Cout],
 * Fo = (Fi - 1) / stride + 1: out_s fp16 and / or out_x fp32 (either may be NULL). stats (NULL: none)
 * fp32 [B][zk_spk_conv_tiles(Fo, To)][3][Cout]: count, mean and sum of squared deviations of out_x
 * per tile, the input of zk_spk_simam. */
int zk_spk_conv2d_cl(const uint16_t* in, int B, int Cin, int Fi, int Ti, const uint16_t* w, int Cout, int ks,
                     int stride, const float* scale, const float* shift, int relu, uint16_t* out_s, float* out_x,
                     float* stats, void* stream);
int zk_spk_conv_tiles(int Fo, int To);      /* tiles per clip of a conv with that output size */
/* SimAMBasicBlock.SimAM + shortcut + relu (:85-95): y fp32 [B][F][T][C] = bn2(conv2), stats its tile
 * partials (combined in tile order, no atomics); x_out = relu(y sigmoid((y - mu)^2 / (4 (v + 1e-4)) + 0.5)
 * + shortcut), v = sum (y - mu)^2 / (F T - 1) per (clip, channel); s_out = fp16(x_out). x_out may be
 * shortcut. moments: fp32 [B][2][C] scratch. */
int zk_spk_simam(const float* y, int B, int C, int F, int T, const float* stats, const float* shortcut,
                 float* moments, float* x_out, uint16_t* s_out, void* stream);
/* ASP.forward (:52-60) on x fp32 [B][F][T][C]: w1 fp32 [att_dim][F * C] and w2 fp32 [F * C][att_dim],
 * b2 [F * C] with the feature axis permuted from the reference's c F + f to f C + c; bn_scale / bn_shift
 * the BatchNorm1d(att_dim). hidden: fp32 [B][T][att_dim] scratch. pooled fp32 [B][2 C F] in the
 * reference's order (mu then sg, feature c F + f). att_dim = 128. */
int zk_spk_asp(const float* x, int B, int C, int F, int T, const float* w1, const float* b1, const float* bn_scale,
               const float* bn_shift, const float* w2, const float* b2, int att_dim, float* hidden, float* pooled,
               void* stream);
/* bottleneck Linear K -> E (:222) then the LDA Linear E -> L (:411), fp32: emb [B][E], lda [B][L]. */
int zk_spk_head(const float* pooled, int B, int K, const float* wb, const float* bb, int E, const float* wl,
                const float* bl, int L, float* emb, float* lda, void* stream);
/* The whole phase wav -> (embedding, LDA) on a descriptor. blocks is a host array; every other pointer
 * is device memory. Validated on the host before any launch (zk_last_error()). */
typedef struct zk_spk_block {
    int32_t cin, cout, stride, pad_;
    const uint16_t* w1; const float* scale1; const float* shift1;      /* conv1 3x3 stride s + bn1 */
    const uint16_t* w2; const float* scale2; const float* shift2;      /* conv2 3x3 + bn2 */
    const uint16_t* wd; const float* scaled; const float* shiftd;      /* downsample 1x1 stride s + BN, or NULL */
} zk_spk_block;
typedef struct zk_spk_desc {
    int32_t n_mels, c0, nblocks, pool_dim, att_dim, emb_dim, lda_dim, pad_;   /* pool_dim = C F after the last block */
    const float* window; const double* twiddle; const float* melfb;
    const float* stem_w; const float* stem_scale; const float* stem_shift;
    const zk_spk_block* blocks;
    const float* asp_w1; const float* asp_b1; const float* asp_bn_scale; const float* asp_bn_shift;
    const float* asp_w2; const float* asp_b2;
    const float* bott_w; const float* bott_b; const float* lda_w; const float* lda_b;
} zk_spk_desc;
size_t zk_speaker_workspace_bytes(const zk_spk_desc* d, int B, int n);    /* 0 + zk_last_error() if invalid */
int zk_speaker_embed(const zk_spk_desc* d, const float* wav16k, int B, int n, void* workspace,
                     size_t workspace_bytes, float* emb256, float* lda128, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZONOS_HIP_H */
