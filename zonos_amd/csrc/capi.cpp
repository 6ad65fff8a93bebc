// C ABI glue for libzonos_hip.so: error reporting, device sync and hipGraph capture of the
// decode step (the reference runs the transformer step eagerly, model.py:138-142,220-222).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/zonos_hip.h"
#include "warm.h"

// The FP8 KV-cache entries live with their kernels (backbone.hip). Weak here, so that this file alone still
// links in a host-only build that provides just the entries it drives; fp8_ok() refuses kv_fp8 without them.
#pragma weak zk_attn_decode_qkv_f8
#pragma weak zk_kv_quantize_e4m3
// The FP8-weight GEMV entries (gemm.hip), weak in the same way; w8_ok() refuses w_fp8 without them.
#pragma weak zk_gemv_fused_w8
#pragma weak zk_gemv_qkv_rope_w8
#pragma weak zk_gemv_attn_out_w8
// The request-batch sampler entries (sampler.hip), weak in the same way; rows_ok() refuses rows without them.
#pragma weak zk_sample_heads_rows
#pragma weak zk_eos_step_rows
// The per-row-context entries (attn_rows.hip), weak in the same way; row_off_ok() refuses row_off without them.
#pragma weak zk_attn_decode_qkv_sc_rows
#pragma weak zk_attn_decode_qkv_f8_rows
#pragma weak zk_embed_codes_rows
#pragma weak zk_gather_last_rows

static thread_local char g_err[1024] = "";

extern "C" void zk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* zk_last_error(void) { return g_err; }

extern "C" int zk_version(void) { return 3; }

// sizeof / offsetof of the by-value ABI structs, so a binding (ctypes here) can verify its
// layout without a GPU: which = 0 zk_sampling_params, 1 zk_gen_state, 4 ZkCondSeg, 5 ZkCondPlan,
// 6 zk_step_layer, 7 zk_step_desc, 8 zk_dac_desc; 12-25 sizes / field offsets (see the cases);
// 26-30 zk_spk_block / zk_spk_desc; 31-32 the FP8-weight fields of zk_step_desc / zk_step_layer;
// 33-34 zk_stream_desc; 35-39 zk_row_params and the rows field of zk_step_desc / zk_hybrid_desc.
extern "C" long zk_abi_size(int which) {
    switch (which) {
        case 0: return (long)sizeof(zk_sampling_params);
        case 1: return (long)sizeof(zk_gen_state);
        case 4: return (long)sizeof(ZkCondSeg);
        case 5: return (long)sizeof(ZkCondPlan);
        case 12: return (long)offsetof(zk_gen_state, seed);
        case 6: return (long)sizeof(zk_step_layer);
        case 7: return (long)sizeof(zk_step_desc);
        case 13: return (long)offsetof(zk_step_desc, eps);
        case 14: return (long)offsetof(zk_step_desc, st);
        case 15: return (long)offsetof(zk_step_desc, sp);
        case 8: return (long)sizeof(zk_dac_desc);
        case 16: return (long)offsetof(zk_dac_desc, blocks);
        case 17: return (long)sizeof(zk_dac_block);
        case 18: return (long)sizeof(zk_hybrid_layer);
        case 19: return (long)sizeof(zk_hybrid_desc);
        case 20: return (long)offsetof(zk_hybrid_desc, st);
        case 21: return (long)offsetof(zk_hybrid_desc, eps);
        case 22: return (long)offsetof(zk_gen_state, noise_offset);
        case 23: return (long)offsetof(zk_step_desc, kv_fp8);
        case 24: return (long)offsetof(zk_step_desc, pre_k);
        case 25: return (long)offsetof(zk_step_layer, k_scale);
        case 26: return (long)sizeof(zk_spk_block);
        case 27: return (long)sizeof(zk_spk_desc);
        case 28: return (long)offsetof(zk_spk_block, wd);
        case 29: return (long)offsetof(zk_spk_desc, blocks);
        case 30: return (long)offsetof(zk_spk_desc, lda_b);
        case 31: return (long)offsetof(zk_step_desc, w_fp8);
        case 32: return (long)offsetof(zk_step_layer, wqkv8);
        case 33: return (long)sizeof(zk_stream_desc);
        case 34: return (long)offsetof(zk_stream_desc, B);
        case 35: return (long)sizeof(zk_row_params);
        case 36: return (long)offsetof(zk_row_params, seed);
        case 37: return (long)offsetof(zk_row_params, key);
        case 38: return (long)offsetof(zk_step_desc, rows);
        case 39: return (long)offsetof(zk_hybrid_desc, rows);
        default: return -1;
    }
}

extern "C" int zk_device_sync(void) {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        zk_set_error("hipDeviceSynchronize: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

#define HIPCHK(expr, what)                                                 \
    do {                                                                   \
        hipError_t _e = (expr);                                            \
        if (_e != hipSuccess) {                                            \
            zk_set_error("%s: %s", what, hipGetErrorString(_e));           \
            return -1;                                                     \
        }                                                                  \
    } while (0)

extern "C" int zk_graph_begin(void* stream) {
    HIPCHK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal), "zk_graph_begin");
    return 0;
}

extern "C" int zk_graph_end(void* stream, void** graph_exec) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamEndCapture((hipStream_t)stream, &g), "zk_graph_end(capture)");
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPCHK(e, "zk_graph_end(instantiate)");
    *graph_exec = (void*)ex;
    return 0;
}

extern "C" int zk_graph_launch(void* graph_exec, int repeat, void* stream) {
    for (int i = 0; i < repeat; ++i)
        HIPCHK(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream), "zk_graph_launch");
    return 0;
}

extern "C" int zk_graph_destroy(void* graph_exec) {
    if (graph_exec) HIPCHK(hipGraphExecDestroy((hipGraphExec_t)graph_exec), "zk_graph_destroy");
    return 0;
}

// ---------------------------------------------------------------- event timing (bench roofline)
extern "C" int zk_event_create(void** ev) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e), "zk_event_create");
    *ev = (void*)e;
    return 0;
}
extern "C" int zk_event_record(void* ev, void* stream) {
    HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream), "zk_event_record");
    return 0;
}
extern "C" int zk_event_elapsed_ms(void* a, void* b, float* ms) {
    HIPCHK(hipEventSynchronize((hipEvent_t)b), "zk_event_elapsed(sync)");
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b), "zk_event_elapsed");
    return 0;
}
extern "C" int zk_event_destroy(void* ev) {
    if (ev) HIPCHK(hipEventDestroy((hipEvent_t)ev), "zk_event_destroy");
    return 0;
}

// ------------------------------------------------------------------ one decode step
// The launch sequences of zonos_amd.engine.HipDecoder and zonos_amd.hybrid.HybridDecoder (see
// zonos_hip.h). Each entry below checks its own arguments; the first failing one aborts the step
// with its message.
#define ZK_STEP(call)                  \
    do {                               \
        if ((call) != 0) return -1;    \
    } while (0)

// L2 warm-up descriptor of the decode GEMM zk_gemm_bf16(M, N, K, nsplit) (2 chunks per wave:
// profiles/r3_l2_warm_micro.txt)
static ZkWarm warm_desc(const void* W, int M, int N, int K, int nsplit, int mode = 0) {
    return zk_gemm_warm_desc(W, M, N, K, nsplit, mode, 2);
}

namespace {
const ZkWarm kNoWarm{nullptr, 0, 0, 0, 0};   // zk_resid_ln / zk_gemm_bf16 are their _warm forms with this

// ---- what the transformer and the hybrid entries share: Desc is zk_step_desc or zk_hybrid_desc,
// `who` the entry's name in its error messages

// Prefill prologue: the argument checks, the prefix conditioning and the codebook embeddings into
// x rows [2B][S = Lc + P + 1][D]. desc_ok: the entry's own descriptor check (false for d == nullptr).
// row_off (zk_prefill_rows, else NULL): cond is zero-padded to Lc, the frames of row r start at
// Lc + row_off[r] and the P + 1 positions behind Lc are zeroed first (a short row's padding must be finite).
template <class Desc>
int prefill_prologue(const char* who, bool desc_ok, const Desc* d, const void* cond, int Lc, int P, const void* q,
                     void* stream, const int32_t* row_off = nullptr) {
    if (!desc_ok || cond == nullptr || q == nullptr || Lc < 0 || P < 0) {
        zk_set_error("%s: bad arguments", who);
        return -1;
    }
    // The last decode step attends over Lc + Ld keys (S = Lc + P + 1 after the prefill, plus
    // Ld - (P + 1) steps, model.py:335-345). The decode attention clamps its context to smax so a
    // no-op launch after the last step stays in bounds; a real step must never need that clamp.
    if (Lc + d->st.Ld > d->smax) {
        zk_set_error("%s: KV cache of %d keys is shorter than Lc + Ld = %d", who, d->smax, Lc + d->st.Ld);
        return -1;
    }
    const int K = d->st.K, S = Lc + P + 1;
    const size_t row = (size_t)d->d_model * 2;
    // prefix conditioning into the first Lc positions of every row (model.py:184-186)
    if (Lc > 0) {
        hipError_t e = hipMemcpy2DAsync(d->x, S * row, cond, Lc * row, Lc * row, 2 * d->B, hipMemcpyDeviceToDevice,
                                        (hipStream_t)stream);
        if (e != hipSuccess) {
            zk_set_error("%s: conditioning copy: %s", who, hipGetErrorString(e));
            return -1;
        }
    }
    if (row_off != nullptr) {
        hipError_t e = hipMemset2DAsync(static_cast<char*>(d->x) + Lc * row, S * row, 0, (P + 1) * row, 2 * d->B,
                                        (hipStream_t)stream);
        if (e != hipSuccess) {
            zk_set_error("%s: clearing the padded positions: %s", who, hipGetErrorString(e));
            return -1;
        }
        return zk_embed_codes_rows(d->st.delayed, d->B, P + 1, K, (long)d->st.Ld * K, d->st.Ld, d->emb, d->st.V,
                                   d->d_model, 2, d->x, S, Lc, row_off, stream);
    }
    return zk_embed_codes(d->st.delayed, d->B, P + 1, K, (long)d->st.Ld * K, d->st.Ld, nullptr, 0, d->emb, d->st.V,
                          d->d_model, 2, d->x, S, Lc, nullptr, nullptr, d->eps, nullptr, nullptr, stream);
}

// Prefill epilogue: the heads on the last position of every row (rows r*S + S-1 via lda = S*D), the
// first sample and the first frame write. row_off: each row's last VALID position, gathered into y (free by now)
template <class Desc>
int prefill_epilogue(const Desc* d, int S, int P, void* stream, const int32_t* row_off = nullptr) {
    const int R = 2 * d->B, D = d->d_model;
    if (row_off != nullptr) {
        ZK_STEP(zk_gather_last_rows(d->xn, R, S, D, row_off, d->y, stream));
        ZK_STEP(zk_gemm_bf16(d->y, D, d->heads, R, d->st.K * d->st.V, D, d->split_heads, 0, d->part, nullptr, nullptr,
                             stream));
    } else {
        ZK_STEP(zk_gemm_bf16(static_cast<const char*>(d->xn) + (size_t)(S - 1) * D * 2, (long)S * D, d->heads, R,
                             d->st.K * d->st.V, D, d->split_heads, 0, d->part, nullptr, nullptr, stream));
    }
    if (d->rows != nullptr) {   // a request batch: per-utterance parameters
        ZK_STEP(zk_sample_heads_rows(d->part, d->split_heads, &d->st, d->rows, 1, 0, d->dbg, stream));
        return zk_eos_step_rows(&d->st, 1, P + 1, stream);
    }
    ZK_STEP(zk_sample_heads(d->part, d->split_heads, &d->st, &d->sp, 1, 0, d->dbg, stream));
    return zk_eos_step(&d->st, 1, P + 1, stream);
}

// A request batch (rows != NULL) samples from the keyed noise only; checked before the first launch
template <class Desc>
int rows_ok(const char* who, const Desc* d) {
    if (d->rows != nullptr && (&zk_sample_heads_rows == nullptr || &zk_eos_step_rows == nullptr)) {
        zk_set_error("%s: this build has no request-batch sampler kernels", who);
        return -1;
    }
    if (d->rows != nullptr && d->st.noise_mode != 0) {
        zk_set_error("%s: rows (a request batch) takes the keyed noise only, st.noise_mode = %d (torch's stream is "
                     "one call per batch)", who, d->st.noise_mode);
        return -1;
    }
    return 0;
}

// Decode tail: both sampler draws over the nsp logit slabs in part, then the EOS protocol
template <class Desc>
int decode_tail(const Desc* d, int nsp, void* stream) {
    if (d->rows != nullptr) {   // a request batch: per-utterance parameters, rows independent
        ZK_STEP(zk_sample_heads_rows(d->part, nsp, &d->st, d->rows, 0, 0, d->dbg, stream));
        ZK_STEP(zk_sample_heads_rows(d->part, nsp, &d->st, d->rows, 0, 1, nullptr, stream));
        return zk_eos_step_rows(&d->st, 0, 0, stream);
    }
    ZK_STEP(zk_sample_heads(d->part, nsp, &d->st, &d->sp, 0, 0, d->dbg, stream));
    ZK_STEP(zk_sample_heads(d->part, nsp, &d->st, &d->sp, 0, 1, nullptr, stream));
    return zk_eos_step(&d->st, 0, 0, stream);
}

// The seven-launch split-K block sequence of HipBackbone._layers over M = R*S rows, xn -> xn.
// Prefill (S positions per row): splits of 1, no skip / position words, zk_qkv_rope +
// zk_attn_prefill as the attention, no L2 warm-up.
// row_off (zk_decode_step_rows, else NULL): the decode attention with a context per row.
int transformer_layers(const zk_step_desc* d, int R, int S, bool prefill, void* q, void* stream,
                       const int32_t* row_off = nullptr) {
    const int M = R * S;
    const int D = d->d_model, H = d->n_heads, Hk = d->n_kv, hd = d->head_dim, Fd = d->d_ff;
    const int Nqkv = (H + 2 * Hk) * hd;
    const int32_t* skip = prefill ? nullptr : d->st.scal + 3;
    const int32_t* pos = prefill ? nullptr : d->st.scal + 1;
    const int sq = prefill ? 1 : d->split_qkv, so = prefill ? 1 : d->split_o, sf = prefill ? 1 : d->split_fc2;
    // each k_resid_ln and the fc1 GEMM warm the next GEMM's first weight chunks into L2 (warm.h)
    auto warm = [&](const void* W, int N, int K, int nsplit, int mode = 0) {
        return prefill ? kNoWarm : warm_desc(W, M, N, K, nsplit, mode);
    };
    for (int i = 0; i < d->n_layer; ++i) {
        const zk_step_layer& L = d->layers[i];
        ZK_STEP(zk_gemm_bf16(d->xn, D, L.wqkv, M, Nqkv, D, sq, 0, d->part, nullptr, skip, stream));
        if (prefill && d->kv_fp8) {
            // exact prefill on the bf16 scratch pair (one layer live at a time), then this layer's FP8 cache
            ZK_STEP(zk_qkv_rope(d->part, 1, R, S, H, Hk, hd, d->freqs, 0, nullptr, q, d->pre_k, d->pre_vt, d->pre_smax,
                                nullptr, 0, nullptr, stream));
            ZK_STEP(zk_attn_prefill(q, d->pre_k, d->pre_vt, R, S, H, Hk, hd, d->pre_smax, d->y, stream));
            ZK_STEP(zk_kv_quantize_e4m3(d->pre_k, d->pre_vt, R, Hk, hd, S, d->pre_smax, L.k_cache, L.vt_cache, L.k_scale,
                                        L.v_scale, d->smax, stream));
        } else if (prefill) {
            ZK_STEP(zk_qkv_rope(d->part, 1, R, S, H, Hk, hd, d->freqs, 0, nullptr, q, L.k_cache, L.vt_cache, d->smax,
                                nullptr, d->rope_neox, nullptr, stream));
            ZK_STEP(zk_attn_prefill(q, L.k_cache, L.vt_cache, R, S, H, Hk, hd, d->smax, d->y, stream));
        } else if (d->kv_fp8 && row_off != nullptr) {
            ZK_STEP(zk_attn_decode_qkv_f8_rows(d->part, sq, d->freqs, L.k_cache, L.vt_cache, L.k_scale, L.v_scale, R, H,
                                               Hk, hd, d->smax, 1, pos, row_off, d->attn_work, d->attn_splits,
                                               d->attn_cnt, d->y, skip, stream));
        } else if (d->kv_fp8) {
            ZK_STEP(zk_attn_decode_qkv_f8(d->part, sq, d->freqs, L.k_cache, L.vt_cache, L.k_scale, L.v_scale, R, H, Hk,
                                          hd, d->smax, 1, pos, d->attn_work, d->attn_splits, d->attn_cnt, d->y, skip,
                                          stream));
        } else if (row_off != nullptr) {
            ZK_STEP(zk_attn_decode_qkv_sc_rows(d->part, sq, d->freqs, L.k_cache, L.vt_cache, R, H, Hk, hd, d->smax, 1,
                                               pos, row_off, d->attn_work, d->attn_splits, d->attn_cnt, d->y, skip,
                                               stream));
        } else {
            ZK_STEP(zk_attn_decode_qkv_sc(d->part, sq, d->freqs, L.k_cache, L.vt_cache, R, H, Hk, hd, d->smax, 1, pos,
                                          d->attn_work, d->attn_splits, d->attn_cnt, d->y, d->rope_neox, skip,
                                          stream));
        }
        ZK_STEP(zk_gemm_bf16(d->y, H * hd, L.wo, M, D, H * hd, so, 0, d->part, nullptr, skip, stream));
        ZK_STEP(zk_resid_ln_warm(d->part, so, d->x, L.ln2_w, L.ln2_b, d->eps, M, D, d->x, d->xn, 0, skip,
                                 warm(L.fc1, 2 * Fd, D, 1, 1), stream));
        ZK_STEP(zk_gemm_bf16_warm(d->xn, D, L.fc1, M, 2 * Fd, D, 1, 1, nullptr, d->h, skip, warm(L.fc2, D, Fd, sf),
                                  stream));
        ZK_STEP(zk_gemm_bf16(d->h, Fd, L.fc2, M, D, Fd, sf, 0, d->part, nullptr, skip, stream));
        const bool last = i + 1 == d->n_layer;
        const ZkWarm next = last ? warm(d->heads, d->st.K * d->st.V, D, d->split_heads)
                                 : warm(d->layers[i + 1].wqkv, Nqkv, D, sq);
        ZK_STEP(zk_resid_ln_warm(d->part, sf, d->x, last ? d->lnf_w : d->layers[i + 1].ln1_w,
                                 last ? d->lnf_b : d->layers[i + 1].ln1_b, d->eps, M, D, d->x, d->xn, 0, skip, next,
                                 stream));
    }
    return 0;
}

bool step_ok(const zk_step_desc* d) { return d != nullptr && d->layers != nullptr && d->n_layer > 0 && d->B > 0; }

// kv_fp8 descriptors are checked whole before the first launch (prefill: also the bf16 scratch pair)
int fp8_ok(const char* who, const zk_step_desc* d, bool prefill, int S) {
    if (!d->kv_fp8) return 0;
    if (&zk_attn_decode_qkv_f8 == nullptr || &zk_kv_quantize_e4m3 == nullptr) {
        zk_set_error("%s: this build has no FP8 KV-cache kernels", who);
        return -1;
    }
    if (d->small) {
        zk_set_error("%s: kv_fp8 = 1 runs the seven-launch sequence only (small must be 0)", who);
        return -1;
    }
    if (d->rope_neox || d->head_dim != 128 || d->smax % 128 != 0) {
        zk_set_error("%s: kv_fp8 needs interleaved RoPE, head_dim 128 and smax %% 128 == 0", who);
        return -1;
    }
    for (int i = 0; i < d->n_layer; ++i) {
        const zk_step_layer& L = d->layers[i];
        if (L.k_cache == nullptr || L.vt_cache == nullptr || L.k_scale == nullptr || L.v_scale == nullptr) {
            zk_set_error("%s: kv_fp8 layer %d lacks its cache or scale pointers", who, i);
            return -1;
        }
    }
    if (prefill && (d->pre_k == nullptr || d->pre_vt == nullptr || d->pre_smax < S || d->pre_smax % 32 != 0)) {
        zk_set_error("%s: kv_fp8 needs the bf16 prefill scratch pair (pre_k, pre_vt, pre_smax=%d >= S=%d, %% 32 == 0)",
                     who, d->pre_smax, S);
        return -1;
    }
    return 0;
}

// row_off (a context per row) runs the rows forms of the fused attention only; checked before the first launch
int row_off_ok(const char* who, const zk_step_desc* d, const int32_t* row_off) {
    if (row_off == nullptr) return 0;
    if (&zk_attn_decode_qkv_sc_rows == nullptr || &zk_attn_decode_qkv_f8_rows == nullptr ||
        &zk_embed_codes_rows == nullptr || &zk_gather_last_rows == nullptr) {
        zk_set_error("%s: this build has no per-row-context kernels (row_off)", who);
        return -1;
    }
    if (d->attn_merge > 0 || d->rope_neox) {
        zk_set_error("%s: row_off runs the fused attention with interleaved RoPE only (attn_merge = %d must be 0, "
                     "rope_neox = %d must be 0)", who, d->attn_merge, d->rope_neox);
        return -1;
    }
    return 0;
}

// w_fp8 descriptors are checked whole before the first launch
int w8_ok(const char* who, const zk_step_desc* d) {
    if (!d->w_fp8) return 0;
    if (&zk_gemv_fused_w8 == nullptr || &zk_gemv_qkv_rope_w8 == nullptr || &zk_gemv_attn_out_w8 == nullptr) {
        zk_set_error("%s: this build has no FP8-weight GEMV kernels", who);
        return -1;
    }
    if (!d->small || d->kv_fp8) {
        zk_set_error("%s: w_fp8 = 1 runs the five-launch sequence on the bf16 KV cache only (small must be 1, "
                     "kv_fp8 0)", who);
        return -1;
    }
    for (int i = 0; i < d->n_layer; ++i) {
        const zk_step_layer& L = d->layers[i];
        if (L.wqkv8 == nullptr || L.wo8 == nullptr || L.fc18 == nullptr || L.fc28 == nullptr ||
            L.wqkv_scale == nullptr || L.wo_scale == nullptr || L.fc1_scale == nullptr || L.fc2_scale == nullptr) {
            zk_set_error("%s: w_fp8 layer %d lacks a weight image or its scale pointer", who, i);
            return -1;
        }
    }
    return 0;
}

// The small-batch layer GEMVs of one step, on the bf16 weights or (w_fp8) on the byte images: the same three
// entries with the image and its scales in place of W
struct StepGemv {
    bool w8;
    void* stream;
    int fused(const void* A, long lda, const void* W, const void* W8, const void* sc, int M, int N, int K, int mode,
              const void* ln_w, const void* ln_b, float eps, float* Cf, void* Cb, const int32_t* skip) const {
        return w8 ? zk_gemv_fused_w8(A, lda, W8, sc, M, N, K, mode, ln_w, ln_b, eps, Cf, Cb, skip, stream)
                  : zk_gemv_fused(A, lda, W, M, N, K, mode, ln_w, ln_b, eps, Cf, Cb, skip, stream);
    }
    int qkv_rope(const zk_step_desc* d, const zk_step_layer& L, int R, const int32_t* pos, const int32_t* skip) const {
        const int H = d->n_heads, Hk = d->n_kv, hd = d->head_dim;
        return w8 ? zk_gemv_qkv_rope_w8(d->x, L.wqkv8, L.wqkv_scale, R, H, Hk, hd, L.ln1_w, L.ln1_b, d->eps, d->y,
                                        L.k_cache, L.vt_cache, d->smax, pos, d->freqs, skip, stream)
                  : zk_gemv_qkv_rope(d->x, L.wqkv, R, H, Hk, hd, L.ln1_w, L.ln1_b, d->eps, d->y, L.k_cache, L.vt_cache,
                                     d->smax, pos, d->freqs, skip, stream);
    }
    int attn_out(const zk_step_desc* d, const zk_step_layer& L, int R, const int32_t* skip) const {
        const int D = d->d_model, Kd = d->n_heads * d->head_dim;
        return w8 ? zk_gemv_attn_out_w8(d->attn_work, d->attn_merge, d->n_kv, L.wo8, L.wo_scale, R, D, Kd, d->x, skip,
                                        stream)
                  : zk_gemv_attn_out(d->attn_work, d->attn_merge, d->n_kv, L.wo, R, D, Kd, d->x, skip, stream);
    }
};
}  // namespace

namespace {
// zk_decode_step (row_off NULL) / zk_decode_step_rows; `who` names the entry in the error messages
int decode_step(const char* who, const zk_step_desc* d, const int32_t* row_off, void* stream) {
    if (!step_ok(d)) {
        zk_set_error("%s: bad descriptor", who);
        return -1;
    }
    ZK_STEP(rows_ok(who, d));
    ZK_STEP(fp8_ok(who, d, false, 0));
    ZK_STEP(w8_ok(who, d));
    ZK_STEP(row_off_ok(who, d, row_off));
    const int K = d->st.K, V = d->st.V, B = d->B, R = 2 * B;
    const int D = d->d_model, H = d->n_heads, Hk = d->n_kv, hd = d->head_dim, Fd = d->d_ff;
    const int Nqkv = (H + 2 * Hk) * hd;
    int32_t* scal = d->st.scal;
    const int32_t* skip = scal + 3;
    const int32_t* pos = scal + 1;
    const zk_step_layer& L0 = d->layers[0];
    // embed_codes (model.py:97-98) + CFG row duplication; layer 0's LayerNorm here unless the
    // small path runs it in the in_proj prologue
    ZK_STEP(zk_embed_codes(d->st.delayed, B, 1, K, (long)d->st.Ld * K, d->st.Ld, scal, -1, d->emb, V, D, 2, d->x, 1,
                           0, d->small ? nullptr : L0.ln1_w, d->small ? nullptr : L0.ln1_b, d->eps,
                           d->small ? nullptr : d->xn, skip, stream));
    if (!d->small) {
        ZK_STEP(transformer_layers(d, R, 1, false, nullptr, stream, row_off));
        ZK_STEP(zk_gemm_bf16(d->xn, D, d->heads, R, K * V, D, d->split_heads, 0, d->part, nullptr, skip, stream));
        return decode_tail(d, d->split_heads, stream);
    }
    // B <= 8: five launches per block, the attention (through out_proj) in one of three forms
    const StepGemv gv{d->w_fp8 != 0, stream};
    for (int i = 0; i < d->n_layer; ++i) {
        const zk_step_layer& L = d->layers[i];
        if (d->attn_merge > 0 && !d->rope_neox) {
            // B = 1: RoPE + KV write in the in_proj epilogue, a prologue-free attention over 32-key
            // slices, its partials merged by the out_proj GEMV
            ZK_STEP(gv.qkv_rope(d, L, R, pos, skip));
            ZK_STEP(zk_attn_decode_q_part(d->y, L.k_cache, L.vt_cache, R, H, Hk, hd, d->smax, 1, pos, d->attn_work,
                                          d->attn_merge, skip, stream));
            ZK_STEP(gv.attn_out(d, L, R, skip));
        } else {
            ZK_STEP(gv.fused(d->x, D, L.wqkv, L.wqkv8, L.wqkv_scale, R, Nqkv, D, 0, L.ln1_w, L.ln1_b, d->eps, d->part,
                             nullptr, skip));
            if (d->attn_merge > 0) {
                ZK_STEP(zk_attn_decode_qkv_part(d->part, 1, d->freqs, L.k_cache, L.vt_cache, R, H, Hk, hd, d->smax, 1,
                                                pos, d->attn_work, d->attn_merge, d->rope_neox, skip, stream));
                ZK_STEP(gv.attn_out(d, L, R, skip));
            } else {
                if (row_off != nullptr)
                    ZK_STEP(zk_attn_decode_qkv_sc_rows(d->part, 1, d->freqs, L.k_cache, L.vt_cache, R, H, Hk, hd,
                                                       d->smax, 1, pos, row_off, d->attn_work, d->attn_splits,
                                                       d->attn_cnt, d->y, skip, stream));
                else
                    ZK_STEP(zk_attn_decode_qkv_sc(d->part, 1, d->freqs, L.k_cache, L.vt_cache, R, H, Hk, hd, d->smax, 1,
                                                  pos, d->attn_work, d->attn_splits, d->attn_cnt, d->y, d->rope_neox,
                                                  skip, stream));
                ZK_STEP(gv.fused(d->y, H * hd, L.wo, L.wo8, L.wo_scale, R, D, H * hd, 2, nullptr, nullptr, d->eps,
                                 nullptr, d->x, skip));
            }
        }
        ZK_STEP(gv.fused(d->x, D, L.fc1, L.fc18, L.fc1_scale, R, 2 * Fd, D, 1, L.ln2_w, L.ln2_b, d->eps, nullptr, d->h,
                         skip));
        ZK_STEP(gv.fused(d->h, Fd, L.fc2, L.fc28, L.fc2_scale, R, D, Fd, 2, nullptr, nullptr, d->eps, nullptr, d->x,
                         skip));
    }
    // 9 heads (model.py:104-111) with norm_f as the GEMV prologue, one slab
    ZK_STEP(zk_gemv_fused(d->x, D, d->heads, R, K * V, D, 0, d->lnf_w, d->lnf_b, d->eps, d->part, nullptr, skip,
                          stream));
    return decode_tail(d, 1, stream);
}

// zk_prefill (row_off NULL) / zk_prefill_rows
int prefill(const char* who, const zk_step_desc* d, const void* cond, int Lc, int P, void* q, const int32_t* row_off,
            void* stream) {
    if (step_ok(d)) ZK_STEP(rows_ok(who, d));
    if (step_ok(d)) ZK_STEP(fp8_ok(who, d, true, Lc + P + 1));
    if (step_ok(d)) ZK_STEP(row_off_ok(who, d, row_off));
    ZK_STEP(prefill_prologue(who, step_ok(d), d, cond, Lc, P, q, stream, row_off));
    const int R = 2 * d->B, S = Lc + P + 1;
    ZK_STEP(zk_layernorm(d->x, d->layers[0].ln1_w, d->layers[0].ln1_b, d->eps, R * S, d->d_model, d->xn, stream));
    ZK_STEP(transformer_layers(d, R, S, true, q, stream));
    return prefill_epilogue(d, S, P, stream, row_off);
}
}  // namespace

extern "C" int zk_decode_step(const zk_step_desc* d, void* stream) {
    return decode_step("zk_decode_step", d, nullptr, stream);
}

extern "C" int zk_decode_step_rows(const zk_step_desc* d, const int32_t* row_off, void* stream) {
    return decode_step("zk_decode_step_rows", d, row_off, stream);
}

extern "C" int zk_prefill(const zk_step_desc* d, const void* cond, int Lc, int P, void* q, void* stream) {
    return prefill("zk_prefill", d, cond, Lc, P, q, nullptr, stream);
}

extern "C" int zk_prefill_rows(const zk_step_desc* d, const void* cond, int Lc, int P, void* q, const int32_t* row_off,
                               void* stream) {
    return prefill("zk_prefill_rows", d, cond, Lc, P, q, row_off, stream);
}

// ------------------------------------------------------------------ hybrid step (zonos_amd.hybrid)
namespace {
bool hybrid_ok(const zk_hybrid_desc* d) {
    return d != nullptr && d->layers != nullptr && d->n_layer > 0 && d->B > 0 && d->d_inner > 0 &&
           d->nheads_ssm * d->headdim_ssm == d->d_inner && (d->norm_flags & ~6) == 0;
}

// the block sequence of HybridDecoder._layers over M = R*S rows; prefill: S positions per row
// norm_flags (zk_hybrid_desc): bit 1 rms_norm, bit 2 residual_in_fp32 -> zk_resid_ln flag words
int hybrid_resid_flags(const zk_hybrid_desc* d) {
    return 1 | (d->norm_flags & 2) | ((d->norm_flags & 4) ? (4 | 8) : 0);
}
void* hybrid_resid(const zk_hybrid_desc* d) { return (d->norm_flags & 4) ? d->xf : d->x; }

// split-K of a GEMM with reduction length K: the requested split, lowered until it divides K into
// 64-deep chunks (the Mamba-block MLP may be narrower than the attention MLP split_fc2 was chosen for)
int fit_split(int K, int s) {
    while (s > 1 && K % (s * 64) != 0) --s;
    return s;
}

// the first block's norm of the embedding when the config variants are on (layer_norm_fn with
// residual = None: residual = hidden, in fp32 under residual_in_fp32); x holds the embedding rows
int hybrid_prenorm(const zk_hybrid_desc* d, int M, const int32_t* skip, void* stream) {
    const int rf = 1 | (d->norm_flags & 2) | ((d->norm_flags & 4) ? 8 : 0);
    return zk_resid_ln(nullptr, 0, d->x, d->layers[0].ln1_w, d->layers[0].ln1_b, d->eps, M, d->d_model,
                       hybrid_resid(d), d->xn, rf, skip, stream);
}

int hybrid_layers(const zk_hybrid_desc* d, int R, int S, bool prefill, void* q, void* stream) {
    const int M = R * S;
    const int D = d->d_model, H = d->n_heads, Hk = d->n_kv, hd = d->head_dim;
    const int Nqkv = (H + 2 * Hk) * hd, di = d->d_inner, nh = d->nheads_ssm;
    const int nin = 2 * di + 2 * d->d_state + nh;
    const int32_t* scal = d->st.scal;
    const int32_t* skip = prefill ? nullptr : scal + 3;
    const int32_t* pos = prefill ? nullptr : scal + 1;
    const int sq = prefill ? 1 : d->split_qkv, so = prefill ? 1 : d->split_o, sf = prefill ? 1 : d->split_fc2;
    const int si = prefill ? 1 : d->split_inp, su = prefill ? 1 : d->split_out;
    const int K = d->st.K, V = d->st.V;
    const int rf = hybrid_resid_flags(d);
    void* xr = hybrid_resid(d);
    if ((d->norm_flags & 4) && d->xf == nullptr) {
        zk_set_error("zk_hybrid: residual_in_fp32 needs the fp32 residual buffer xf");
        return -1;
    }
    // L2 warm-up (warm.h) of the GEMM that follows layer i's last k_resid_ln: the next layer's first
    // GEMM, or the heads
    auto next_warm = [&](int i) {
        if (prefill) return kNoWarm;
        if (i + 1 == d->n_layer) return warm_desc(d->heads, M, K * V, D, d->split_heads);
        const zk_hybrid_layer& N1 = d->layers[i + 1];
        return N1.type == 0 ? warm_desc(N1.wqkv, M, Nqkv, D, sq) : warm_desc(N1.w_in, M, nin, D, si);
    };
    for (int i = 0; i < d->n_layer; ++i) {
        const zk_hybrid_layer& L = d->layers[i];
        const bool last = i + 1 == d->n_layer;
        const void* nw = last ? d->lnf_w : d->layers[i + 1].ln1_w;
        const void* nb = last ? d->lnf_b : d->layers[i + 1].ln1_b;
        int smix;                               // split-K of the mixer's output projection
        if (L.type == 0) {
            ZK_STEP(zk_gemm_bf16(d->xn, D, L.wqkv, M, Nqkv, D, sq, 0, d->part, nullptr, skip, stream));
            if (prefill) {
                ZK_STEP(zk_qkv_rope(d->part, 1, R, S, H, Hk, hd, d->freqs, 0, nullptr, q, L.k_cache, L.vt_cache,
                                    d->smax, nullptr, 1, nullptr, stream));
                ZK_STEP(zk_attn_prefill(q, L.k_cache, L.vt_cache, R, S, H, Hk, hd, d->smax, d->y, stream));
            } else {
                ZK_STEP(zk_attn_decode_qkv(d->part, sq, d->freqs, L.k_cache, L.vt_cache, R, H, Hk, hd, d->smax, 1,
                                           pos, d->attn_work, d->attn_splits, d->y, 1, skip, stream));
            }
            ZK_STEP(zk_gemm_bf16(d->y, H * hd, L.wo, M, D, H * hd, so, 0, d->part, nullptr, skip, stream));
            smix = so;
        } else if (L.type == 1) {
            ZK_STEP(zk_gemm_bf16(d->xn, D, L.w_in, M, nin, D, si, 0, d->part, nullptr, skip, stream));
            if (prefill) {
                // the first decode step (position S) reads the parity-(S & 1) buffers
                ZK_STEP(zk_mamba_prefill(d->part, R, S, di, nh, d->headdim_ssm, d->d_state, L.conv_w, L.conv_b, d->xc,
                                         L.conv_state[S & 1], L.ssm_state[S & 1], L.A, L.dt_bias, L.Dskip, d->yz,
                                         stream));
            } else {
                ZK_STEP(zk_mamba_step(d->part, si, R, di, nh, d->headdim_ssm, d->d_state, L.conv_w, L.conv_b,
                                      L.conv_state[0], L.conv_state[1], pos, L.ssm_state[0], L.ssm_state[1], L.A,
                                      L.dt_bias, L.Dskip, d->yz, skip, stream));
            }
            ZK_STEP(zk_gated_rmsnorm(d->yz, M, di, L.norm_w, d->gate_eps, d->ym, skip, stream));
            ZK_STEP(zk_gemm_bf16(d->ym, di, L.w_out, M, D, di, su, 0, d->part, nullptr, skip, stream));
            smix = su;
        } else {
            zk_set_error("zk_hybrid: layer %d has unknown type %d", i, L.type);
            return -1;
        }
        // Block.mlp (_mamba_ssm.py:18-22: GatedMLP of d_intermediate on Mamba2 blocks when it is
        // nonzero, of attn_mlp_d_intermediate on attention blocks): norm2 -> fc1 (SwiGLU) -> fc2
        const int Fl = L.type == 0 ? (L.d_mlp > 0 ? L.d_mlp : d->d_ff) : L.d_mlp;
        if (Fl > 0) {
            const int sfl = prefill ? 1 : fit_split(Fl, sf);
            ZK_STEP(zk_resid_ln_warm(d->part, smix, xr, L.ln2_w, L.ln2_b, d->eps, M, D, xr, d->xn, rf, skip,
                                     prefill ? kNoWarm : warm_desc(L.fc1, M, 2 * Fl, D, 1, 1), stream));
            ZK_STEP(zk_gemm_bf16_warm(d->xn, D, L.fc1, M, 2 * Fl, D, 1, 1, nullptr, d->h, skip,
                                      prefill ? kNoWarm : warm_desc(L.fc2, M, D, Fl, sfl), stream));
            ZK_STEP(zk_gemm_bf16(d->h, Fl, L.fc2, M, D, Fl, sfl, 0, d->part, nullptr, skip, stream));
            smix = sfl;
        }
        ZK_STEP(zk_resid_ln_warm(d->part, smix, xr, nw, nb, d->eps, M, D, xr, d->xn, rf, skip, next_warm(i), stream));
    }
    return 0;
}
}  // namespace

extern "C" int zk_hybrid_decode_step(const zk_hybrid_desc* d, void* stream) {
    if (!hybrid_ok(d)) {
        zk_set_error("zk_hybrid_decode_step: bad descriptor");
        return -1;
    }
    ZK_STEP(rows_ok("zk_hybrid_decode_step", d));
    const int K = d->st.K, V = d->st.V, B = d->B, R = 2 * B, D = d->d_model;
    int32_t* scal = d->st.scal;
    const int32_t* skip = scal + 3;
    const bool var = (d->norm_flags & 6) != 0;       // config variants: the first norm is its own launch
    ZK_STEP(zk_embed_codes(d->st.delayed, B, 1, K, (long)d->st.Ld * K, d->st.Ld, scal, -1, d->emb, V, D, 2, d->x, 1, 0,
                           var ? nullptr : d->layers[0].ln1_w, var ? nullptr : d->layers[0].ln1_b, d->eps,
                           var ? nullptr : d->xn, skip, stream));
    if (var) ZK_STEP(hybrid_prenorm(d, R, skip, stream));
    ZK_STEP(hybrid_layers(d, R, 1, false, nullptr, stream));
    ZK_STEP(zk_gemm_bf16(d->xn, D, d->heads, R, K * V, D, d->split_heads, 0, d->part, nullptr, skip, stream));
    return decode_tail(d, d->split_heads, stream);
}

extern "C" int zk_hybrid_prefill(const zk_hybrid_desc* d, const void* cond, int Lc, int P, void* q, void* stream) {
    if (hybrid_ok(d)) ZK_STEP(rows_ok("zk_hybrid_prefill", d));
    ZK_STEP(prefill_prologue("zk_hybrid_prefill", hybrid_ok(d), d, cond, Lc, P, q, stream));
    const int R = 2 * d->B, S = Lc + P + 1, D = d->d_model;
    if (d->norm_flags & 6) ZK_STEP(hybrid_prenorm(d, R * S, nullptr, stream));
    else ZK_STEP(zk_layernorm(d->x, d->layers[0].ln1_w, d->layers[0].ln1_b, d->eps, R * S, D, d->xn, stream));
    ZK_STEP(hybrid_layers(d, R, S, true, q, stream));
    return prefill_epilogue(d, S, P, stream);
}


// ------------------------------------------------------------------ DAC decode (whole)
namespace {
struct DacPlan {
    size_t z, a, b, x, tmp, last, total;
};
size_t zk_align(size_t v) { return (v + 255) & ~(size_t)255; }
bool dac_plan(const zk_dac_desc* d, int B, int T, DacPlan& p) {
    if (d == nullptr || d->nblocks < 0 || d->nblocks > ZK_DAC_MAXB || B <= 0 || T <= 0) return false;
    size_t L = (size_t)T, act = (size_t)B * T * d->c0, big = 0, lastc = d->c0;
    for (int i = 0; i < d->nblocks; ++i) {
        const zk_dac_block& k = d->blocks[i];
        if (k.nres < 1 || k.nres > ZK_DAC_MAXR) return false;
        L *= (size_t)k.stride;
        const size_t n = (size_t)B * L * k.cout;
        act = std::max(act, n);
        big = std::max(big, n);
        lastc = k.cout;
    }
    p.z = 0;
    p.a = zk_align(p.z + (size_t)B * T * d->cin0 * 2);
    p.b = zk_align(p.a + act * 2);
    p.x = zk_align(p.b + act * 2);
    p.tmp = zk_align(p.x + big * 4);
    p.last = zk_align(p.tmp + act * 2);
    p.total = zk_align(p.last + (size_t)B * L * lastc * 4);
    return true;
}

// The decoder's three uses of zk_dac_conv_cl (zonos_hip.h). s: fp16 Snake'd activations [B][L][Cin]; every conv
// applies the next Snake (alpha) in its epilogue; lens counts frames, `scale` samples per frame at this stage.
// k7 conv, dilated, 'same' padding (the first conv; conv1 of a residual unit): s_out = fp16 Snake(conv + b)
int dac_conv_k7(const uint16_t* s, int B, int Cin, int L, const uint16_t* w, const float* b, int Cout, int dil,
                const float* alpha, uint16_t* s_out, const int32_t* lens, int scale, void* stream) {
    return zk_dac_conv_cl(s, B, Cin, L, w, 0, b, Cout, 7, dil, 3 * dil, L, 1, 1, 0, L, nullptr, nullptr, alpha, s_out, 0,
                          lens, scale, scale, stream);
}
// 1x1 conv + residual (conv2 of a residual unit): x += conv + b, s_out = Snake(x) (s_f32: fp32, for the tail)
int dac_conv_1x1_res(const uint16_t* s, int B, int C, int L, const uint16_t* w, const float* b, float* x,
                     const float* alpha, void* s_out, int s_f32, const int32_t* lens, int scale, void* stream) {
    return zk_dac_conv_cl(s, B, C, L, w, 0, b, C, 1, 1, 0, L, 1, 1, 0, L, x, x, alpha, s_out, s_f32, lens, scale, scale,
                          stream);
}
// ConvTranspose1d(k = 2 st, stride st) as st polyphase 2-tap convs, L -> L st: x = conv + b, s_out = fp16 Snake(x)
int dac_convt(const uint16_t* s, int B, int Cin, int L, const uint16_t* w, const float* b, int Cout, int st, float* x,
              const float* alpha, uint16_t* s_out, const int32_t* lens, int scale, void* stream) {
    return zk_dac_conv_cl(s, B, Cin, L, w, 2L * Cout * Cin, b, Cout, 2, 1, 1, L + 1, st, st, -((st + 1) / 2), L * st,
                          nullptr, x, alpha, s_out, 0, lens, scale, scale * st, stream);
}
}  // namespace

extern "C" size_t zk_dac_decode_workspace(const zk_dac_desc* d, int B, int T) {
    DacPlan p;
    return dac_plan(d, B, T, p) ? p.total : 0;
}

extern "C" int zk_dac_decode(const zk_dac_desc* d, const int64_t* codes, int B, int T, const int32_t* lens,
                             void* workspace, size_t workspace_bytes, float* out, void* stream) {
    DacPlan p;
    if (!dac_plan(d, B, T, p) || codes == nullptr || out == nullptr || workspace == nullptr) {
        zk_set_error("zk_dac_decode: bad arguments");
        return -1;
    }
    if (workspace_bytes < p.total) {
        zk_set_error("zk_dac_decode: workspace %zu bytes < %zu needed", workspace_bytes, p.total);
        return -1;
    }
    char* ws = static_cast<char*>(workspace);
    uint16_t* z = reinterpret_cast<uint16_t*>(ws + p.z);
    // three fp16 activation buffers; each conv writes one its input is not in (a fused residual unit
    // reads its input's neighbours as the k7 halo, so it never writes in place)
    uint16_t* bufs[3] = {reinterpret_cast<uint16_t*>(ws + p.a), reinterpret_cast<uint16_t*>(ws + p.b),
                         reinterpret_cast<uint16_t*>(ws + p.tmp)};
    auto other = [&](const void* u, const void* v) -> uint16_t* {
        for (uint16_t* c : bufs)
            if (c != u && c != v) return c;
        return nullptr;
    };
    float* x = reinterpret_cast<float*>(ws + p.x);
    float* last_act = reinterpret_cast<float*>(ws + p.last);
    ZK_STEP(zk_dac_rvq_decode_cl(codes, B, d->ncb, T, (long)d->ncb * T, d->tables, d->codebook_size, d->hidden,
                                 d->cin0, z, lens, stream));
    const float* a_next = d->nblocks ? d->blocks[0].alpha : d->final_alpha;
    ZK_STEP(dac_conv_k7(z, B, d->cin0, T, d->conv1_w, d->conv1_b, d->c0, 1, a_next, bufs[0], lens, 1, stream));
    int L = T, scale = 1, cch = d->c0;
    const void* act = bufs[0];
    bool act_f32 = false;
    for (int bi = 0; bi < d->nblocks; ++bi) {
        const zk_dac_block& k = d->blocks[bi];
        const int st = k.stride, Lo = L * st;
        uint16_t* s_new = other(act, nullptr);
        ZK_STEP(dac_convt(static_cast<const uint16_t*>(act), B, k.cin, L, k.wt, k.bt, k.cout, st, x, k.res[0].a1, s_new,
                          lens, scale, stream));
        act = s_new;
        scale *= st;
        L = Lo;
        for (int j = 0; j < k.nres; ++j) {
            const zk_dac_resunit& ru = k.res[j];
            const float* an = j + 1 < k.nres ? k.res[j + 1].a1 : (bi + 1 < d->nblocks ? d->blocks[bi + 1].alpha
                                                                                           : d->final_alpha);
            const bool last = j + 1 == k.nres && bi + 1 == d->nblocks;
            uint16_t* tmp = other(act, nullptr);
            const int fm = zk_dac_resunit_supported(k.cout);
            if (fm == 2 || (fm == 1 && !last)) {
                // the whole unit in one launch (k7 -> Snake -> 1x1 -> + x -> next Snake)
                void* s_out = last ? static_cast<void*>(last_act) : static_cast<void*>(tmp);
                ZK_STEP(zk_dac_resunit_cl(static_cast<const uint16_t*>(act), B, k.cout, L, ru.w1, ru.b1, ru.dil,
                                          ru.a2, ru.w2, ru.b2, x, an, s_out, last ? 1 : 0, lens, scale, stream));
                act = s_out;
            } else {
                ZK_STEP(dac_conv_k7(static_cast<const uint16_t*>(act), B, k.cout, L, ru.w1, ru.b1, k.cout, ru.dil, ru.a2,
                                    tmp, lens, scale, stream));
                void* s_out = last ? static_cast<void*>(last_act) : const_cast<void*>(act);
                ZK_STEP(dac_conv_1x1_res(tmp, B, k.cout, L, ru.w2, ru.b2, x, an, s_out, last ? 1 : 0, lens, scale, stream));
                act = s_out;
            }
            if (last) act_f32 = true;
        }
        cch = k.cout;
    }
    if (!act_f32) {
        zk_set_error("zk_dac_decode: the tail needs at least one block (fp32 Snake input)");
        return -1;
    }
    ZK_STEP(zk_dac_tail_cl(static_cast<const float*>(act), B, cch, L, d->conv2_w, d->conv2_b, out, lens, scale,
                           stream));
    return 0;
}
#undef ZK_STEP
