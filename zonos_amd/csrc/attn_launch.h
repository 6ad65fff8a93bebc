// Host side of the decode-attention entries (backbone.hip, attn_f8.h, attn_rows.hip): the launch descriptor, the
// family's argument checks and the launch. Included after attn_common.h.
#pragma once
#include <math.h>

// k_attn_combine over `work` (backbone.hip). Internal to the library: hidden, not part of the C ABI.
__attribute__((visibility("hidden"))) int zk_attn_combine_launch(const float* work, int R, int H, int Hkv, int nsplit, void* out, const int32_t* skip,
                           void* stream);

// non-temporal KV loads (ld_kv): one launch streams >= KV_NT_BYTES of cache, K and V together
static bool kv_nt(int R, int Hkv, int Smax, int hd, int elem_bytes) {
    return (double)R * Hkv * Smax * hd * elem_bytes * 2 >= KV_NT_BYTES;
}

// One launch of the k_attn_decode / k_attn_decode_f8 family, grid (nsplit, Hkv, R) x 256 threads: the arguments
// every entry has (brace-initialised in this order), then the ones that tell the forms apart.
struct AttnDecode {
    const char* name;      // the extern "C" entry the caller called: every message starts with it
    int R, H, Hkv, hd, Smax, ctx0;
    const int32_t* ctx_dev;
    float* work;
    int nsplit;
    void* out;
    const int32_t* skip;
    void* stream;
    const void* q = nullptr;            // the query rows, or (fused) the in_proj slabs and the RoPE table:
    bool fused = false;
    const float* part = nullptr;
    int gemm_nsplit = 0;
    const float* freqs = nullptr;
    bool part_only = false;             // the splits' partials stay in `work` for a later kernel (no out)
    uint32_t* counters = nullptr;       // fused, nsplit > 1: the splits combine in the launch
    const int32_t* row_off = nullptr;   // the _rows entries: device int32 [R], row r's context is the word's + row_off[r]
    bool comb() const { return fused && !part_only && nsplit > 1 && counters != nullptr; }
};

// Every check of the family, then the launch of `kern` (the entry's instantiation) and, where the splits were
// neither combined in the launch nor asked for as partials, k_attn_combine. `cache` are the kernel's cache
// arguments: K and V^T, then the two scale arrays of the FP8 cache.
// ROWS: `kern` is a _rows kernel, which takes a.row_off behind the family's arguments.
template <bool ROWS = false, class Kern, class... Cache>
static int attn_decode_launch(const AttnDecode& a, Kern kern, Cache... cache) {
    const int min_split = a.part_only ? 2 : 1;
    ZK_REQUIRE(a.hd == 128, "%s: head_dim %d unsupported (128 only)", a.name, a.hd);
    ZK_REQUIRE(a.Hkv > 0 && a.H % a.Hkv == 0 && a.H / a.Hkv <= AT_G, "%s: GQA group %d > %d", a.name,
               a.Hkv > 0 ? a.H / a.Hkv : 0, AT_G);
    ZK_REQUIRE(a.Smax > 0 && a.Smax % AT_KB == 0, "%s: Smax=%d must be a multiple of %d", a.name, a.Smax, AT_KB);
    ZK_REQUIRE(a.nsplit >= min_split && a.nsplit <= a.Smax / AT_KB, "%s: nsplit=%d out of [%d, %d]", a.name, a.nsplit,
               min_split, a.Smax / AT_KB);
    ZK_REQUIRE(a.nsplit == 1 || a.work != nullptr,
               a.part_only ? "%s: null work buffer" : "%s: nsplit > 1 needs the work buffer", a.name);
    ZK_REQUIRE(((cache != nullptr) && ...) && (a.part_only || a.out != nullptr),
               sizeof...(Cache) > 2 ? "%s: null cache, scale or output buffer" : "%s: null cache or output buffer",
               a.name);
    if (a.fused)
        ZK_REQUIRE(a.part != nullptr && a.freqs != nullptr && a.gemm_nsplit >= 1 && a.gemm_nsplit <= AT_MAXGS,
                   "%s: bad arguments (gemm_nsplit=%d, max %d)", a.name, a.gemm_nsplit, AT_MAXGS);
    else
        ZK_REQUIRE(a.q != nullptr, "%s: null q", a.name);
    const float scale = 1.0f / sqrtf((float)a.hd);
    if constexpr (ROWS) {
        ZK_REQUIRE(a.row_off != nullptr && a.fused && !a.part_only, "%s: null row_off", a.name);
        hipLaunchKernelGGL(kern, dim3(a.nsplit, a.Hkv, a.R), dim3(256), 0, (hipStream_t)a.stream, (const bf16_t*)a.q,
                           cache..., a.R, a.H, a.Hkv, a.Smax, a.ctx0, a.ctx_dev, a.work, scale, (bf16_t*)a.out, a.skip,
                           a.part, a.gemm_nsplit, a.freqs, a.comb() ? a.counters : nullptr, a.row_off);
    } else {
        hipLaunchKernelGGL(kern, dim3(a.nsplit, a.Hkv, a.R), dim3(256), 0, (hipStream_t)a.stream, (const bf16_t*)a.q,
                           cache..., a.R, a.H, a.Hkv, a.Smax, a.ctx0, a.ctx_dev, a.work, scale, (bf16_t*)a.out, a.skip,
                           a.part, a.gemm_nsplit, a.freqs, a.comb() ? a.counters : nullptr);
    }
    ZK_CHECK_LAUNCH(a.name);
    if (a.nsplit > 1 && !a.comb() && !a.part_only) {
        if (zk_attn_combine_launch(a.work, a.R, a.H, a.Hkv, a.nsplit, a.out, a.skip, a.stream) != 0) return -1;
    }
    return 0;
}

