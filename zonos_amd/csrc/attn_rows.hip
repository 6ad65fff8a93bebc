// Ragged request batches (conditionings of different lengths, every row left-aligned at its own KV position):
// the decode attention with a context per row, bf16 and FP8 cache, the prefill placement of the prefix frames and
// the gather of every row's last valid position. A translation unit of its own: backbone.hip's kernels and its
// code object stay what they were. The kernels are the shared bodies of attn_common.h (attn_decode_wg, ROWS) and
// attn_f8_body.inc under names of their own.
#include "common.h"
#include "attn_common.h"
#define ZK_ATTN_F8_HELPERS_ONLY
#include "attn_f8.h"
#include "../../include/zonos_hip.h"
#include "attn_launch.h"

namespace {

constexpr int RW_NT = 256;
constexpr int EMB_MAXK = 9;   // codebooks summed (Zonos: 9), as k_embed_ln

// Prefill placement of a request batch with conditionings of different lengths (zk_embed_codes_rows): k_embed_ln's
// embedding sum (the same loads, the same left-to-right bf16 adds) without a LayerNorm, written to a position
// per row -- output row r*out_S + out_t0 + row_off[r] + t, the start clamped into [0, out_S - S] (row_off is
// device data). Workgroup = (r, t), thread -> 8 channels.
__global__ __launch_bounds__(RW_NT) void k_embed_rows(const int64_t* ids, int B, int S, int K, long bstr, long kstr,
                                                      const bf16_t* emb, int V, int D, bf16_t* x_out, int out_S,
                                                      int out_t0, const int32_t* row_off) {
    const int r = blockIdx.x / S, t = blockIdx.x % S, b = r % B;
    const int t0 = max(0, min(out_t0 + uni(ld_word(row_off + r)), out_S - S));
    const size_t row = (size_t)r * out_S + t0 + t;
    int64_t idv[EMB_MAXK];
#pragma unroll
    for (int k = 0; k < EMB_MAXK; ++k) {
        const int64_t id = ids[b * bstr + min(k, K - 1) * kstr + t];
        idv[k] = id < 0 ? 0 : (id >= V ? V - 1 : id);
    }
    for (int c = threadIdx.x * 8; c < D; c += RW_NT * 8) {
        float acc[8];
        uint4 ev[EMB_MAXK];
#pragma unroll
        for (int k = 0; k < EMB_MAXK; ++k)
            ev[k] = *reinterpret_cast<const uint4*>(emb + ((size_t)min(k, K - 1) * V + idv[k]) * D + c);
#pragma unroll
        for (int k = 0; k < EMB_MAXK; ++k) {
            float e[8];
            unpack8(ev[k], e);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (k < K) acc[q] = (k == 0) ? e[q] : round_bf(acc[q] + e[q]);
        }
        *reinterpret_cast<uint4*>(x_out + row * D + c) = pack8(acc);
    }
}

// Prefill epilogue of the same batches (zk_gather_last_rows): row r's last valid position,
// x[r*S + S - 1 + row_off[r]] (the offset clamped into [-(S - 1), 0]), into the compact out [R][D].
__global__ __launch_bounds__(RW_NT) void k_gather_last_rows(const bf16_t* x, int S, int D, const int32_t* row_off,
                                                            bf16_t* out) {
    const int r = blockIdx.x;
    const int t = S - 1 + max(-(S - 1), min(uni(ld_word(row_off + r)), 0));
    const bf16_t* src = x + ((size_t)r * S + t) * D;
    for (int c = threadIdx.x * 8; c < D; c += RW_NT * 8)
        *reinterpret_cast<uint4*>(out + (size_t)r * D + c) = *reinterpret_cast<const uint4*>(src + c);
}

// The fused kernel with a context per row (a request batch with conditionings of different lengths): workgroup
// (split, g, r) uses ctx0 + *ctx_dev + row_off[r], clamped into [1, Smax]. A kernel of its own name around the
// same text; row_off + r is wave-uniform and its load goes out with the skip and the context word.
template <bool KVNT, bool COMB>
__global__ __launch_bounds__(256, 2) void k_attn_decode_f8_rows(const bf16_t* q, uint8_t* k8, uint8_t* v8,
                                                                uint8_t* ksc, uint8_t* vsc, int R, int H, int Hkv,
                                                                int Smax, int ctx0, const int32_t* ctx_dev,
                                                                float* work, float scale, bf16_t* out,
                                                                const int32_t* skip, const float* part, int gsplit,
                                                                const float* freqs, uint32_t* cnt,
                                                                const int32_t* row_off) {
    constexpr int HD = 128;
    constexpr bool FUSED = true, ROWS = true;
    __shared__ AttnSmem sm;
    __shared__ Attn8Smem s8;
    const int sk = ld_word(skip);
    const int cwr = ld_word(ctx_dev);
    const int ro = ld_word(row_off + blockIdx.z);
#include "attn_f8_body.inc"
}

}  // namespace

extern "C" int zk_embed_codes_rows(const int64_t* ids, int B, int S, int K, long ids_bstride, long ids_kstride,
                                   const void* emb, int V, int D, int rows_dup, void* x_out, int out_S, int out_t0,
                                   const int32_t* row_off, void* stream) {
    ZK_REQUIRE(D % 8 == 0 && D > 0, "zk_embed_codes_rows: D=%d must be a multiple of 8", D);
    ZK_REQUIRE(B > 0 && S > 0 && K > 0 && rows_dup > 0, "zk_embed_codes_rows: empty shape");
    ZK_REQUIRE(K <= EMB_MAXK, "zk_embed_codes_rows: K=%d codebooks > %d", K, EMB_MAXK);
    ZK_REQUIRE(out_S >= S, "zk_embed_codes_rows: out_S=%d < S=%d", out_S, S);
    ZK_REQUIRE(ids != nullptr && emb != nullptr && x_out != nullptr && row_off != nullptr,
               "zk_embed_codes_rows: NULL buffer");
    hipLaunchKernelGGL(k_embed_rows, dim3(rows_dup * B * S), dim3(RW_NT), 0, (hipStream_t)stream, ids, B, S, K,
                       ids_bstride, ids_kstride, (const bf16_t*)emb, V, D, (bf16_t*)x_out, out_S, out_t0, row_off);
    ZK_CHECK_LAUNCH("zk_embed_codes_rows");
    return 0;
}

extern "C" int zk_gather_last_rows(const void* x, int R, int S, int D, const int32_t* row_off, void* out,
                                   void* stream) {
    ZK_REQUIRE(D % 8 == 0 && D > 0 && R > 0 && S > 0, "zk_gather_last_rows: bad shape (R=%d, S=%d, D=%d)", R, S, D);
    ZK_REQUIRE(x != nullptr && row_off != nullptr && out != nullptr, "zk_gather_last_rows: NULL buffer");
    hipLaunchKernelGGL(k_gather_last_rows, dim3(R), dim3(RW_NT), 0, (hipStream_t)stream, (const bf16_t*)x, S, D,
                       row_off, (bf16_t*)out);
    ZK_CHECK_LAUNCH("zk_gather_last_rows");
    return 0;
}

// zk_attn_decode_qkv_sc with a context per row (interleaved RoPE only): the same instantiation choice
template <bool COMB>
static auto rows_attn_kernel(bool kvnt, int gemm_nsplit) {
    if (gemm_nsplit == 4) return kvnt ? k_attn_decode_rows<true, COMB, 4> : k_attn_decode_rows<false, COMB, 4>;
    return kvnt ? k_attn_decode_rows<true, COMB, 0> : k_attn_decode_rows<false, COMB, 0>;
}

extern "C" int zk_attn_decode_qkv_sc_rows(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                                          void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                                          const int32_t* ctx_dev, const int32_t* row_off, float* work, int nsplit,
                                          uint32_t* counters, void* out, const int32_t* skip, void* stream) {
    AttnDecode a{"zk_attn_decode_qkv_sc_rows", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    a.counters = counters;
    a.row_off = row_off;
    a.fused = true;
    a.part = part;
    a.gemm_nsplit = gemm_nsplit;
    a.freqs = freqs;
    const bool nt = kv_nt(R, Hkv, Smax, hd, 2);
    auto kern = a.comb() ? rows_attn_kernel<true>(nt, gemm_nsplit) : rows_attn_kernel<false>(nt, gemm_nsplit);
    return attn_decode_launch<true>(a, kern, (bf16_t*)k_cache, (bf16_t*)vt_cache);
}

extern "C" int zk_attn_decode_qkv_f8_rows(const float* part, int gemm_nsplit, const float* freqs, void* k8, void* v8,
                                          void* k_scale, void* v_scale, int R, int H, int Hkv, int hd, int Smax,
                                          int ctx0, const int32_t* ctx_dev, const int32_t* row_off, float* work,
                                          int nsplit, uint32_t* counters, void* out, const int32_t* skip,
                                          void* stream) {
    AttnDecode a{"zk_attn_decode_qkv_f8_rows", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    a.fused = true;
    a.part = part;
    a.gemm_nsplit = gemm_nsplit;
    a.freqs = freqs;
    a.counters = counters;
    a.row_off = row_off;
    const bool nt = kv_nt(R, Hkv, Smax, hd, 1);
    auto kern = a.comb() ? (nt ? k_attn_decode_f8_rows<true, true> : k_attn_decode_f8_rows<false, true>)
                         : (nt ? k_attn_decode_f8_rows<true, false> : k_attn_decode_f8_rows<false, false>);
    return attn_decode_launch<true>(a, kern, (uint8_t*)k8, (uint8_t*)v8, (uint8_t*)k_scale, (uint8_t*)v_scale);
}
