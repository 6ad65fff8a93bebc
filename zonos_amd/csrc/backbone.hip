// Transformer backbone step kernels for gfx950 (zonos/backbone/_torch.py restated).
//
//   k_embed_ln   : sum of 9 codebook embeddings (bf16 left-to-right adds, model.py:97-98),
//                  duplicated for the CFG rows (model.py:141) + layer-0 LayerNorm.
//   k_resid_ln   : split-K slab reduction of the preceding projection + residual add
//                  (bf16, _torch.py:100-101) + the next LayerNorm, one pass over the row.
//   k_qkv_rope   : in_proj slab reduction -> bf16 -> interleaved RoPE (_torch.py:18-30)
//                  -> q buffer + KV cache store (_torch.py:33-49).
//   k_attn_decode: split-KV GQA decode attention on MFMA 16x16x32 bf16 (K on the A side,
//                  the 4 query heads of a KV head on the B side), k_attn_combine merges splits.
//   k_attn_prefill: causal prefill attention on MFMA (16 queries per wave, two passes).
//
// KV cache layout: see "KV cache layout" below (32-key slices in MFMA-fragment order).
#include "common.h"
#include "attn_common.h"
#include "../../include/zonos_hip.h"
#include "warm.h"
#include <algorithm>
#include <stdlib.h>

namespace {



// ------------------------------------------------------------------ LayerNorm helper
// Row of D elements, 8 per thread (D = 8 * NT * n8). Two-pass mean/var in fp32,
// y = (x - mean) * rstd * w + b rounded to bf16 (nn.LayerNorm, eps from config).
// wv / bv: this thread's 8-element chunks of w and b, loaded by the caller before its own
// loads complete (so they share the row's memory round trip); red: 2 * NT / 64 floats (one
// partial-sum slot per wave for the mean and one for the variance: one barrier per reduction).
// rms (block-uniform): RMS norm as mamba_ssm's layer_norm_fn(is_rms_norm=True) computes it -- no mean
// (mean = 0, so x - mean = x and nb = -0.0: y = x * rstd * w + b exactly), var = sum(x^2) / D.
template <int NT, int n8>
ZK_DEV void ln_row_pre(const float* x, const uint4* wv, const uint4* bv, float eps, int D, bf16_t* y, float* red,
                       bool rms = false) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float t = 0.f;
    if (!rms) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < n8; ++j)
            if ((threadIdx.x + NT * j) * 8 < D)
                for (int e = 0; e < 8; ++e) s += x[j * 8 + e];
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) red[w] = s;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) t += red[i];
    }
    const float mean = t / (float)D;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < n8; ++j)
        if ((threadIdx.x + NT * j) * 8 < D)
            for (int e = 0; e < 8; ++e) { const float d = x[j * 8 + e] - mean; v += d * d; }
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[NT / 64 + w] = v;
    __syncthreads();
    t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[NT / 64 + i];
    const float var = t / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
    const float nb = -rstd * mean;
#pragma unroll
    for (int j = 0; j < n8; ++j) {
        const int c = (threadIdx.x + NT * j) * 8;
        if (c >= D) continue;
        float wf[8], bf[8], o[8];
        unpack8(wv[j], wf);
        unpack8(bv[j], bf);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            o[e] = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(x[j * 8 + e], rstd), nb), wf[e]), bf[e]);
        *reinterpret_cast<uint4*>(y + c) = pack8(o);
    }
}
// the caller's w / b chunks (clamped index: unconditional loads stay in registers). b == nullptr (a
// bias-free RMSNorm): -0.0, the additive identity, so y = x_hat * w bit for bit.
template <int NT, int n8>
ZK_DEV void ln_load_wb(const bf16_t* w, const bf16_t* b, int D, uint4* wv, uint4* bv) {
#pragma unroll
    for (int j = 0; j < n8; ++j) {
        const int c = min((int)(threadIdx.x + NT * j) * 8, D - 8);
        wv[j] = *reinterpret_cast<const uint4*>(w + c);
        bv[j] = b ? *reinterpret_cast<const uint4*>(b + c) : make_uint4(0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u);
    }
}
template <int NT, int n8>
ZK_DEV void ln_row(const float* x, const bf16_t* w, const bf16_t* b, float eps, int D, bf16_t* y, float* red) {
    uint4 wv[n8], bv[n8];
    ln_load_wb<NT, n8>(w, b, D, wv, bv);
    ln_row_pre<NT, n8>(x, wv, bv, eps, D, y, red);
}

constexpr int LN_NT = 256;
constexpr int RL_MAXS = 8;    // split-K slabs k_resid_ln reduces with all loads in flight
constexpr int MAX_N8 = 4;     // D <= 8192
constexpr int EMB_MAXK = 9;   // codebooks summed by k_embed_ln (Zonos: 9)

template <int N8>
__global__ __launch_bounds__(LN_NT) void k_embed_ln(const int64_t* ids, int B, int S, int K, long bstr, long kstr,
                                                    const int32_t* col_dev, int col_add, const bf16_t* emb, int V,
                                                    int D, bf16_t* x_out, int out_S, int out_t0, const bf16_t* lw,
                                                    const bf16_t* lb, float eps, bf16_t* xn_out, const int32_t* skip) {
    __shared__ float red[2 * LN_NT / 64];
    if (skip && *skip) return;
    const int r = blockIdx.x / S, t = blockIdx.x % S, b = r % B;
    const int row = r * out_S + out_t0 + t;   // output row
    const int col = t + (col_dev ? *col_dev + col_add : 0);
    constexpr int n8 = N8;
    float x[N8 * 8];
    // all code ids, then all embedding rows, issued before the first add (two memory round
    // trips per step instead of 2K dependent ones); K <= EMB_MAXK (host-checked)
    // (loads unconditional with a clamped codebook index, so the arrays stay in registers)
    int64_t idv[EMB_MAXK];
#pragma unroll
    for (int k = 0; k < EMB_MAXK; ++k) {
        const int64_t id = ids[b * bstr + min(k, K - 1) * kstr + col];
        idv[k] = id < 0 ? 0 : (id >= V ? V - 1 : id);
    }
#pragma unroll
    for (int j = 0; j < n8; ++j) {
        const int c = (threadIdx.x + LN_NT * j) * 8;
        if (c >= D) continue;
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
#pragma unroll
        for (int q = 0; q < 8; ++q) x[j * 8 + q] = acc[q];
        *reinterpret_cast<uint4*>(x_out + (size_t)row * D + c) = pack8(acc);
    }
    if (lw != nullptr) ln_row<LN_NT, N8>(x, lw, lb, eps, D, xn_out + (size_t)row * D, red);
}

template <int N8>
__global__ __launch_bounds__(LN_NT) void k_layernorm(const bf16_t* x, const bf16_t* w, const bf16_t* b, float eps,
                                                     int D, bf16_t* y) {
    __shared__ float red[2 * LN_NT / 64];
    const int row = blockIdx.x;
    constexpr int n8 = N8;
    float xv[N8 * 8];
#pragma unroll
    for (int j = 0; j < n8; ++j) {
        const int c = (threadIdx.x + LN_NT * j) * 8;
        if (c >= D) continue;
        unpack8(*reinterpret_cast<const uint4*>(x + (size_t)row * D + c), xv + 8 * j);
    }
    ln_row<LN_NT, N8>(xv, w, b, eps, D, y + (size_t)row * D, red);
}

template <int N8>
__global__ __launch_bounds__(LN_NT) void k_resid_ln(const float* part, int nsplit, const bf16_t* x_in,
                                                    const bf16_t* w, const bf16_t* b, float eps, int rows, int D,
                                                    bf16_t* x_out, bf16_t* xn_out, int ln_on_sum,
                                                    const int32_t* skip) {
    __shared__ float red[2 * LN_NT / 64];
    if (skip && *skip) return;
    const int row = blockIdx.x;
    constexpr int n8 = N8;
    const size_t slab = (size_t)rows * D;
    // LayerNorm weights and the residual row issued with the slab loads: one memory round trip
    uint4 wv[N8], bv[N8], xiv[N8];
    ln_load_wb<LN_NT, N8>(w, b, D, wv, bv);
#pragma unroll
    for (int j = 0; j < n8; ++j)
        xiv[j] = *reinterpret_cast<const uint4*>(x_in + (size_t)row * D + min((int)(threadIdx.x + LN_NT * j) * 8, D - 8));
    float xv[N8 * 8];
#pragma unroll
    for (int j = 0; j < n8; ++j) {
        const int c = (threadIdx.x + LN_NT * j) * 8;
        if (c >= D) continue;
        const float* p = part + (size_t)row * D + c;
        float acc[8];
        if (nsplit <= RL_MAXS) {
            // every slab load issued before the first add (clamped index, sum masked), so the
            // row costs one memory round trip instead of nsplit; same left-to-right fp32 sum
            float4 a0[RL_MAXS], a1[RL_MAXS];
#pragma unroll
            for (int s = 0; s < RL_MAXS; ++s) {
                const float* ps = p + (size_t)min(s, nsplit - 1) * slab;
                a0[s] = *reinterpret_cast<const float4*>(ps);
                a1[s] = *reinterpret_cast<const float4*>(ps + 4);
            }
            acc[0] = a0[0].x; acc[1] = a0[0].y; acc[2] = a0[0].z; acc[3] = a0[0].w;
            acc[4] = a1[0].x; acc[5] = a1[0].y; acc[6] = a1[0].z; acc[7] = a1[0].w;
#pragma unroll
            for (int s = 1; s < RL_MAXS; ++s)
                if (s < nsplit) {
                    acc[0] += a0[s].x; acc[1] += a0[s].y; acc[2] += a0[s].z; acc[3] += a0[s].w;
                    acc[4] += a1[s].x; acc[5] += a1[s].y; acc[6] += a1[s].z; acc[7] += a1[s].w;
                }
        } else {
            const float4 a0 = *reinterpret_cast<const float4*>(p);
            const float4 a1 = *reinterpret_cast<const float4*>(p + 4);
            acc[0] = a0.x; acc[1] = a0.y; acc[2] = a0.z; acc[3] = a0.w;
            acc[4] = a1.x; acc[5] = a1.y; acc[6] = a1.z; acc[7] = a1.w;
            for (int s = 1; s < nsplit; ++s) {
                const float4 b0 = *reinterpret_cast<const float4*>(p + s * slab);
                const float4 b1 = *reinterpret_cast<const float4*>(p + s * slab + 4);
                acc[0] += b0.x; acc[1] += b0.y; acc[2] += b0.z; acc[3] += b0.w;
                acc[4] += b1.x; acc[5] += b1.y; acc[6] += b1.z; acc[7] += b1.w;
            }
        }
        float xi[8];
        unpack8(xiv[j], xi);
        // transformer (_torch.py:100-101): x = bf16(x + bf16(proj)), LN of the rounded x;
        // ln_on_sum (mamba_ssm layer_norm_fn prenorm): LN of the fp32 sum, residual stored bf16
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[j * 8 + e] = xi[e] + round_bf(acc[e]);
        *reinterpret_cast<uint4*>(x_out + (size_t)row * D + c) = pack8(xv + 8 * j);
        if (!ln_on_sum) {
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[j * 8 + e] = round_bf(xv[j * 8 + e]);
        }
    }
    ln_row_pre<LN_NT, N8>(xv, wv, bv, eps, D, xn_out + (size_t)row * D, red);
}

// The hybrid backbone's config variants (mamba_ssm Block / layer_norm_fn with prenorm,
// _mamba_ssm.py:18-31,49-57): flags bit 0 ln_on_sum (always set by the hybrid), bit 1 RMS norm
// (is_rms_norm; b may be NULL for the bias-free block RMSNorm), bit 2 x_in fp32, bit 3 x_out fp32
// (residual_in_fp32: the residual stream stays fp32 and hidden + residual is added in fp32);
// nsplit 0 adds no projection (the first block's norm of the embedding: residual = hidden).
// x_out = x_in + bf16(sum_s part[s]) in fp32 (rounded to bf16 unless bit 3); xn = norm of that fp32 sum.
constexpr int RL_RMS = 2, RL_XIN32 = 4, RL_XOUT32 = 8;
template <int N8>
__global__ __launch_bounds__(LN_NT) void k_resid_ln_var(const float* part, int nsplit, const void* x_in,
                                                        const bf16_t* w, const bf16_t* b, float eps, int rows, int D,
                                                        void* x_out, bf16_t* xn_out, int flags, const int32_t* skip) {
    __shared__ float red[2 * LN_NT / 64];
    if (skip && *skip) return;
    const int row = blockIdx.x;
    const size_t slab = (size_t)rows * D;
    uint4 wv[N8], bv[N8];
    ln_load_wb<LN_NT, N8>(w, b, D, wv, bv);
    float xv[N8 * 8];
#pragma unroll
    for (int j = 0; j < N8; ++j) {
        const int c = (threadIdx.x + LN_NT * j) * 8;
        if (c >= D) continue;
        float xi[8];
        if (flags & RL_XIN32) {
            const float4* q = reinterpret_cast<const float4*>(static_cast<const float*>(x_in) + (size_t)row * D + c);
            const float4 a = q[0], bb = q[1];
            xi[0] = a.x; xi[1] = a.y; xi[2] = a.z; xi[3] = a.w; xi[4] = bb.x; xi[5] = bb.y; xi[6] = bb.z; xi[7] = bb.w;
        } else {
            unpack8(*reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(x_in) + (size_t)row * D + c), xi);
        }
        if (nsplit > 0) {
            const float* p = part + (size_t)row * D + c;
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = p[e];
            for (int sp = 1; sp < nsplit; ++sp)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += p[sp * slab + e];
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[j * 8 + e] = xi[e] + round_bf(acc[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[j * 8 + e] = xi[e];
        }
        if (flags & RL_XOUT32) {
            float4* q = reinterpret_cast<float4*>(static_cast<float*>(x_out) + (size_t)row * D + c);
            q[0] = make_float4(xv[j * 8], xv[j * 8 + 1], xv[j * 8 + 2], xv[j * 8 + 3]);
            q[1] = make_float4(xv[j * 8 + 4], xv[j * 8 + 5], xv[j * 8 + 6], xv[j * 8 + 7]);
        } else {
            *reinterpret_cast<uint4*>(static_cast<bf16_t*>(x_out) + (size_t)row * D + c) = pack8(xv + 8 * j);
            if (!(flags & 1)) {
#pragma unroll
                for (int e = 0; e < 8; ++e) xv[j * 8 + e] = round_bf(xv[j * 8 + e]);
            }
        }
    }
    ln_row_pre<LN_NT, N8>(xv, wv, bv, eps, D, xn_out + (size_t)row * D, red, (flags & RL_RMS) != 0);
}

// k_resid_ln for D = 2048 with whole-line slab reads: 512 threads, thread t owns float4 piece t of
// the row, so every fp32 slab load instruction of a wave reads 1 KB contiguous; all slab loads of
// a row are issued before the first add (one memory round trip); LayerNorm sums over 8 waves.
// NS > 0: exactly NS slabs (only real slabs loaded); NS = 0: nsplit <= RL_MAXS with clamped loads
// WARM: a ninth wave warms the next GEMM's first weight chunks into L2 (warm.h) and keeps the
// block's barrier count (two per row) without waiting for its loads.
// Argument order: the first 14 dwords arrive preloaded in SGPRs (DESIGN §6 "Kernel-argument preload") and
// hold everything the row loads and the step-word test need; the outputs and the warm-up descriptor follow.
template <int NS, bool WARM = false>
__global__ __launch_bounds__(WARM ? 576 : 512) void k_resid_ln_d2k512(const float* part, const bf16_t* x_in,
                                                         const bf16_t* w, const bf16_t* b, const int32_t* skip,
                                                         int nsplit, int rows, float eps, int ln_on_sum,
                                                         bf16_t* x_out, bf16_t* xn_out, const bf16_t* wW, int wK,
                                                         int wgx, int wgz, int wch) {
    constexpr int D = 2048;
    __shared__ float red[16];
    if (WARM && threadIdx.x >= 512)         // (two tests of one condition: folded into one block, hipcc
        if (skip && *skip) return;          // emits different code for the WARM instantiations)
    if (WARM && threadIdx.x >= 512) {
        __shared__ __attribute__((aligned(16))) char sink[1024];
        warm_units(wW, wK, wgx, wgz, wch, blockIdx.x, gridDim.x, 0, 1, threadIdx.x & 63, sink);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
    const int row = blockIdx.x, t = threadIdx.x;
    const size_t slab = (size_t)rows * D;
    const int c0 = 4 * t;
    const uint2 w0 = *reinterpret_cast<const uint2*>(w + c0);
    const uint2 b0 = *reinterpret_cast<const uint2*>(b + c0);
    const uint2 x0 = *reinterpret_cast<const uint2*>(x_in + (size_t)row * D + c0);
    const float* p = part + (size_t)row * D;
    constexpr int NL = NS ? NS : RL_MAXS;
    float4 a0[NL];
#pragma unroll
    for (int sp = 0; sp < NL; ++sp)
        a0[sp] = *reinterpret_cast<const float4*>(p + (size_t)(NS ? sp : min(sp, nsplit - 1)) * slab + c0);
    // the step word after the row's loads (all in bounds): its round trip overlaps theirs
    if (ld_word_here(skip)) {
        keep_live(w0);
        keep_live(b0);
        keep_live(x0);
#pragma unroll
        for (int sp = 0; sp < NL; ++sp) keep_live(a0[sp]);
        return;
    }
    float acc[4] = {a0[0].x, a0[0].y, a0[0].z, a0[0].w};
#pragma unroll
    for (int sp = 1; sp < NL; ++sp)
        if (NS || sp < nsplit) { acc[0] += a0[sp].x; acc[1] += a0[sp].y; acc[2] += a0[sp].z; acc[3] += a0[sp].w; }
    auto un4 = [](uint2 v, float* f) {
        f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
        f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    };
    float xi[4], wf[4], bf[4], xv[4];
    un4(x0, xi);
    un4(w0, wf);
    un4(b0, bf);
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] = xi[e] + round_bf(acc[e]);
    *reinterpret_cast<uint2*>(x_out + (size_t)row * D + c0) = make_uint2(pack2(xv[0], xv[1]), pack2(xv[2], xv[3]));
    if (!ln_on_sum) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[e] = round_bf(xv[e]);
    }
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    float sum = xv[0] + xv[1] + xv[2] + xv[3];
    sum = wave_sum(sum);
    if ((t & 63) == 0) red[wv] = sum;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += red[i];
    const float mean = tot / (float)D;
    float var = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float dd = xv[e] - mean; var += dd * dd; }
    var = wave_sum(var);
    if ((t & 63) == 0) red[8 + wv] = var;
    __syncthreads();
    float vt = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) vt += red[8 + i];
    const float rstd = 1.0f / sqrtf(vt / (float)D + eps);
    const float nb = -rstd * mean;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(xv[e], rstd), nb), wf[e]), bf[e]);
    *reinterpret_cast<uint2*>(xn_out + (size_t)row * D + c0) = make_uint2(pack2(o[0], o[1]), pack2(o[2], o[3]));
}
template <bool NEOX>
__global__ __launch_bounds__(256) void k_qkv_rope(const float* part, int nsplit, int R, int S, int H, int Hkv,
                                                  int hd, const float* freqs, int pos0, const int32_t* pos_dev,
                                                  bf16_t* q_out, bf16_t* kc, bf16_t* vt, int Smax, bf16_t* v_rows,
                                                  const int32_t* skip) {
    if (skip && *skip) return;
    const int row = blockIdx.x;   // r*S + t
    const int r = row / S, t = row % S;
    const int pos = pos0 + t + (pos_dev ? *pos_dev : 0);
    const int N = (H + 2 * Hkv) * hd;
    const size_t slab = (size_t)R * S * N;
    const float* p = part + (size_t)row * N;
    const float* fc = freqs + (size_t)pos * hd;     // [hd/2][2]
    for (int pi = threadIdx.x; pi < N / 2; pi += blockDim.x) {
        const int head = pi / (hd / 2), j = pi % (hd / 2);     // head over q | k | v heads
        int d0, d1;
        rope_dims<NEOX>(j, hd, d0, d1);
        const int c0 = head * hd + d0, c1 = head * hd + d1;
        float a = p[c0], bb = p[c1];
        for (int s = 1; s < nsplit; ++s) { a += p[s * slab + c0]; bb += p[s * slab + c1]; }
        a = round_bf(a); bb = round_bf(bb);
        if (head < H + Hkv) {
            const float c = fc[2 * j], sn = fc[2 * j + 1];
            const float o0 = __fsub_rn(__fmul_rn(a, c), __fmul_rn(bb, sn));
            const float o1 = __fadd_rn(__fmul_rn(bb, c), __fmul_rn(a, sn));
            const bf16_t b0 = f2bf(o0), b1 = f2bf(o1);
            if (head < H) {
                bf16_t* qr = q_out + (size_t)row * H * hd + head * hd;
                qr[d0] = b0;
                qr[d1] = b1;
            } else {
                bf16_t* kb = kc + ((size_t)r * Hkv + (head - H)) * Smax * hd;
                kb[k_off(pos, d0 >> 3) + (d0 & 7)] = b0;
                kb[k_off(pos, d1 >> 3) + (d1 & 7)] = b1;
            }
        } else {
            const int g = head - H - Hkv;
            bf16_t* base = vt + ((size_t)r * Hkv + g) * Smax * hd;
            const bf16_t va = f2bf(a), vb = f2bf(bb);
            base[v_off(pos, d0)] = va;
            base[v_off(pos, d1)] = vb;
            if (v_rows) {
                bf16_t* vr = v_rows + (((size_t)r * Hkv + g) * S + t) * hd;
                vr[d0] = va;
                vr[d1] = vb;
            }
        }
    }
}


__global__ __launch_bounds__(64) void k_attn_combine(const float* work, int H, int Hkv, int nsplit, bf16_t* out,
                                                     const int32_t* skip) {
    constexpr int HD = 128;
    if (skip && *skip) return;
    const int h = blockIdx.x, r = blockIdx.y;
    const int G = H / Hkv, g = h / G, j = h % G;
    const float* base = work + ((size_t)r * Hkv + g) * nsplit * AT_STR;
    const int d = threadIdx.x * 2;
    *reinterpret_cast<uint32_t*>(out + (size_t)r * H * HD + (size_t)h * HD + d) = attn_combine_pair(base, nsplit, j, d);
}

// ------------------------------------------------------------------ prefill attention (causal)
// MFMA form of the decode kernel's slice step with 16 QUERIES as the B operand: workgroup =
// (64-query tile, head, row), each wave owns 16 queries and walks the 32-key slices of the
// packed cache up to its last query (causal). Two passes like the reference's CPU flash kernel
// on a single KV block: the exact row max first (S^T = K.Q^T), then p = exp(s - max) summed in
// fp32 and rounded to bf16 for O^T = V^T.P^T. Each wave's queries are independent (no merge).
__global__ __launch_bounds__(256) void k_attn_prefill(const bf16_t* q, const bf16_t* kc, const bf16_t* vt, int R,
                                                      int S, int H, int Hkv, int Smax, float scale, bf16_t* out) {
    constexpr int HD = 128;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ln = lane & 15, lg = lane >> 4;
    const int h = blockIdx.y, r = blockIdx.z;
    const int q0 = blockIdx.x * 64 + w * 16;               // this wave's first query
    if (q0 >= S) return;
    const int G = H / Hkv, g = h / G;
    const int qt = min(q0 + ln, S - 1);                     // query of this lane's B column
    bf16x8 qf[4];
    {
        const bf16_t* qr = q + ((size_t)(r * S + qt) * H + h) * HD;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = as_frag(*reinterpret_cast<const uint4*>(qr + ks * 32 + lg * 8));
    }
    const bf16_t* kb = kc + ((size_t)r * Hkv + g) * Smax * HD;
    const bf16_t* vb = vt + ((size_t)r * Hkv + g) * Smax * HD;
    const int last = min(q0 + 15, S - 1);                   // keys 0..last can be visible
    const int nsl = last / 32 + 1;
    // lane's 8 score values: keys 8lg .. 8lg+7 of the slice (tile h: 8lg + 4h + i), query qt
    auto scores = [&](int sl, f32x4* sacc) {
        const int lanei = lg * 16 + ln;
        const bf16_t* k0 = kb + (size_t)sl * 4096 + lanei * 8;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            sacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    as_frag(*reinterpret_cast<const uint4*>(k0 + (t * 4 + ks) * 512)), qf[ks], sacc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = sl * 32 + 8 * lg + 4 * t + i;
                sacc[t][i] = key <= qt ? sacc[t][i] * scale : -INFINITY;
            }
    };
    float m = -INFINITY;
    for (int sl = 0; sl < nsl; ++sl) {
        f32x4 sacc[2];
        scores(sl, sacc);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) m = fmaxf(m, sacc[t][i]);
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int sl = 0; sl < nsl; ++sl) {
        f32x4 sacc[2];
        scores(sl, sacc);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pv = __expf(sacc[t][i] - m);       // masked keys: exp(-inf) = 0
                sacc[t][i] = pv;
                l += pv;
            }
        const uint4 pa = make_uint4(pack2(sacc[0][0], sacc[0][1]), pack2(sacc[0][2], sacc[0][3]),
                                    pack2(sacc[1][0], sacc[1][1]), pack2(sacc[1][2], sacc[1][3]));
        const bf16_t* v0 = vb + (size_t)sl * 4096 + (lg * 16 + ln) * 8;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(*reinterpret_cast<const uint4*>(v0 + dt * 512)),
                                                            as_frag(pa), o[dt], 0, 0, 0);
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    // o[dt][i] = O^T[dim = 16dt + 4lg + i][query q0 + ln]
    if (q0 + ln < S) {
        const float inv = 1.0f / l;
        bf16_t* orow = out + ((size_t)(r * S + q0 + ln) * H + h) * HD;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            const int d = dt * 16 + lg * 4;
            *reinterpret_cast<uint2*>(orow + d) =
                make_uint2(pack2(o[dt][0] * inv, o[dt][1] * inv), pack2(o[dt][2] * inv, o[dt][3] * inv));
        }
    }
}

}  // namespace

#define ZK_LN_DISPATCH(D, kern, ...)                                              \
    do {                                                                           \
        const int _n8 = ((D) / 8 + LN_NT - 1) / LN_NT;                             \
        if (_n8 == 1) hipLaunchKernelGGL(kern<1>, __VA_ARGS__);                    \
        else if (_n8 == 2) hipLaunchKernelGGL(kern<2>, __VA_ARGS__);               \
        else if (_n8 == 3) hipLaunchKernelGGL(kern<3>, __VA_ARGS__);               \
        else hipLaunchKernelGGL(kern<4>, __VA_ARGS__);                             \
    } while (0)

extern "C" int zk_embed_codes(const int64_t* ids, int B, int S, int K, long ids_bstride, long ids_kstride,
                              const int32_t* col_dev, int col_add, const void* emb, int V, int D, int rows_dup,
                              void* x_out, int out_S, int out_t0, const void* ln_w, const void* ln_b, float eps,
                              void* xn_out, const int32_t* skip, void* stream) {
    ZK_REQUIRE(D % 8 == 0 && D <= 8 * LN_NT * MAX_N8, "zk_embed_codes: D=%d must be a multiple of 8 (<= %d)", D,
               8 * LN_NT * MAX_N8);
    ZK_REQUIRE(B > 0 && S > 0 && K > 0 && rows_dup > 0, "zk_embed_codes: empty shape");
    ZK_REQUIRE(K <= EMB_MAXK, "zk_embed_codes: K=%d codebooks > %d", K, EMB_MAXK);
    const int rows = rows_dup * B * S;
    ZK_REQUIRE(out_S >= out_t0 + S, "zk_embed_codes: out_S=%d < out_t0+S", out_S);
    ZK_LN_DISPATCH(D, k_embed_ln, dim3(rows), dim3(LN_NT), 0, (hipStream_t)stream, ids, B, S, K, ids_bstride,
                   ids_kstride, col_dev, col_add, (const bf16_t*)emb, V, D, (bf16_t*)x_out, out_S, out_t0,
                   (const bf16_t*)ln_w, (const bf16_t*)ln_b, eps, (bf16_t*)xn_out, skip);
    ZK_CHECK_LAUNCH("zk_embed_codes");
    return 0;
}

extern "C" int zk_layernorm(const void* x, const void* w, const void* b, float eps, int rows, int D, void* y,
                            void* stream) {
    ZK_REQUIRE(D % 8 == 0 && D <= 8 * LN_NT * MAX_N8, "zk_layernorm: unsupported D=%d", D);
    if (rows == 0) return 0;
    ZK_LN_DISPATCH(D, k_layernorm, dim3(rows), dim3(LN_NT), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)w, (const bf16_t*)b, eps, D, (bf16_t*)y);
    ZK_CHECK_LAUNCH("zk_layernorm");
    return 0;
}

extern "C" int zk_resid_ln(const float* part, int nsplit, const void* x_in, const void* w, const void* b, float eps,
                           int rows, int D, void* x_out, void* xn_out, int ln_on_sum, const int32_t* skip,
                           void* stream) {
    return zk_resid_ln_warm(part, nsplit, x_in, w, b, eps, rows, D, x_out, xn_out, ln_on_sum, skip,
                            ZkWarm{nullptr, 0, 0, 0, 0}, stream);
}

int zk_resid_ln_warm(const float* part, int nsplit, const void* x_in, const void* w, const void* b, float eps,
                     int rows, int D, void* x_out, void* xn_out, int ln_on_sum, const int32_t* skip, ZkWarm warm,
                     void* stream) {
    ZK_REQUIRE(D % 8 == 0 && D <= 8 * LN_NT * MAX_N8, "zk_resid_ln: unsupported D=%d", D);
    ZK_REQUIRE(ln_on_sum >= 0 && ln_on_sum < 16, "zk_resid_ln: flags=%d", ln_on_sum);
    ZK_REQUIRE(nsplit >= 1 || (nsplit == 0 && (ln_on_sum & 1)), "zk_resid_ln: nsplit must be >= 1 (0 with ln_on_sum)");
    ZK_REQUIRE(nsplit == 0 || part != nullptr, "zk_resid_ln: part is NULL");
    ZK_REQUIRE(b != nullptr || (ln_on_sum & RL_RMS), "zk_resid_ln: a LayerNorm needs its bias");
    ZK_REQUIRE(x_in != nullptr && x_out != nullptr && w != nullptr && xn_out != nullptr, "zk_resid_ln: NULL buffer");
    if (rows == 0) return 0;
    if (nsplit == 0 || (ln_on_sum & ~1)) {
        // the hybrid variants (RMS norm, fp32 residual, no projection): rare configurations, one
        // generic kernel; the default ln_on_sum paths below are untouched
        ZK_LN_DISPATCH(D, k_resid_ln_var, dim3(rows), dim3(LN_NT), 0, (hipStream_t)stream, part, nsplit, x_in,
                       (const bf16_t*)w, (const bf16_t*)b, eps, rows, D, x_out, (bf16_t*)xn_out, ln_on_sum, skip);
        ZK_CHECK_LAUNCH("zk_resid_ln");
        return 0;
    }
    // D = 2048: 512-thread rows (8 slabs 4.27 vs 4.41 us with 256 threads x 2 pieces, c3 decode
    // step 3.635 vs 3.646 ms, profiles/r2_s4_resid_ln_512_ab.txt)
    if (D == 2048 && nsplit <= RL_MAXS) {
        // the warm-up wave needs rows % 8 == 0 to keep each GEMM workgroup's chunks on its own XCD
        const bool wm = warm.W != nullptr && rows % 8 == 0;
        auto kern = wm ? (nsplit == 4 ? k_resid_ln_d2k512<4, true> : nsplit == 8 ? k_resid_ln_d2k512<8, true>
                                                                                : k_resid_ln_d2k512<0, true>)
                       : (nsplit == 4 ? k_resid_ln_d2k512<4> : nsplit == 8 ? k_resid_ln_d2k512<8> : k_resid_ln_d2k512<0>);
        hipLaunchKernelGGL(kern, dim3(rows), dim3(wm ? 576 : 512), 0, (hipStream_t)stream, part,
                           (const bf16_t*)x_in, (const bf16_t*)w, (const bf16_t*)b, skip, nsplit, rows, eps, ln_on_sum,
                           (bf16_t*)x_out, (bf16_t*)xn_out, (const bf16_t*)warm.W, warm.K, warm.gx, warm.gz,
                           warm.chunks);
        ZK_CHECK_LAUNCH("zk_resid_ln");
        return 0;
    }
    ZK_LN_DISPATCH(D, k_resid_ln, dim3(rows), dim3(LN_NT), 0, (hipStream_t)stream, part, nsplit,
                       (const bf16_t*)x_in, (const bf16_t*)w, (const bf16_t*)b, eps, rows, D, (bf16_t*)x_out,
                       (bf16_t*)xn_out, ln_on_sum, skip);
    ZK_CHECK_LAUNCH("zk_resid_ln");
    return 0;
}

extern "C" int zk_qkv_rope(const float* part, int nsplit, int R, int S, int H, int Hkv, int hd, const float* freqs,
                           int pos0, const int32_t* pos_dev, void* q_out, void* k_cache, void* vt_cache, int Smax,
                           void* v_rows, int rope_neox, const int32_t* skip, void* stream) {
    ZK_REQUIRE(hd % 2 == 0 && nsplit >= 1, "zk_qkv_rope: bad args");
    if (R * S == 0) return 0;
    if (rope_neox)
        hipLaunchKernelGGL(k_qkv_rope<true>, dim3(R * S), dim3(256), 0, (hipStream_t)stream, part, nsplit, R, S, H,
                           Hkv, hd, freqs, pos0, pos_dev, (bf16_t*)q_out, (bf16_t*)k_cache, (bf16_t*)vt_cache, Smax,
                           (bf16_t*)v_rows, skip);
    else
        hipLaunchKernelGGL(k_qkv_rope<false>, dim3(R * S), dim3(256), 0, (hipStream_t)stream, part, nsplit, R, S, H,
                           Hkv, hd, freqs, pos0, pos_dev, (bf16_t*)q_out, (bf16_t*)k_cache, (bf16_t*)vt_cache, Smax,
                           (bf16_t*)v_rows, skip);
    ZK_CHECK_LAUNCH("zk_qkv_rope");
    return 0;
}

#include "attn_launch.h"

// the combine launch of attn_decode_launch (attn_launch.h), also for the rows entries of attn_rows.hip
int zk_attn_combine_launch(const float* work, int R, int H, int Hkv, int nsplit, void* out, const int32_t* skip,
                           void* stream) {
    hipLaunchKernelGGL(k_attn_combine, dim3(H, R), dim3(64), 0, (hipStream_t)stream, work, H, Hkv, nsplit,
                       (bf16_t*)out, skip);
    ZK_CHECK_LAUNCH("zk_attn_combine");
    return 0;
}

extern "C" int zk_attn_decode(const void* q, const void* k_cache, const void* vt_cache, int R, int H, int Hkv,
                              int hd, int Smax, int ctx0, const int32_t* ctx_dev, float* work, int nsplit,
                              void* out, const int32_t* skip, void* stream) {
    AttnDecode a{"zk_attn_decode", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    a.q = q;
    auto kern = kv_nt(R, Hkv, Smax, hd, 2) ? k_attn_decode<false, false, true> : k_attn_decode<false, false, false>;
    return attn_decode_launch(a, kern, (bf16_t*)k_cache, (bf16_t*)vt_cache);
}

// the fused decode attention instantiation: RoPE form, non-temporal KV loads, in-launch combine, and the
// slab pre-load form when the in_proj GEMM ran with exactly 4 splits (every c3-c5 decode step)
template <bool COMB>
static auto fused_attn_kernel(bool neox, bool kvnt, int gemm_nsplit) {
    const bool pre = gemm_nsplit == 4;
    if (pre)
        return neox ? (kvnt ? k_attn_decode<true, true, true, COMB, 4> : k_attn_decode<true, true, false, COMB, 4>)
                    : (kvnt ? k_attn_decode<true, false, true, COMB, 4> : k_attn_decode<true, false, false, COMB, 4>);
    return neox ? (kvnt ? k_attn_decode<true, true, true, COMB, 0> : k_attn_decode<true, true, false, COMB, 0>)
                : (kvnt ? k_attn_decode<true, false, true, COMB, 0> : k_attn_decode<true, false, false, COMB, 0>);
}

// the fused bf16 launch of `a` (zk_attn_decode_qkv, _qkv_part, _qkv_sc)
static int attn_decode_qkv(AttnDecode a, const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                           void* vt_cache, int rope_neox) {
    a.fused = true;
    a.part = part;
    a.gemm_nsplit = gemm_nsplit;
    a.freqs = freqs;
    const bool nt = kv_nt(a.R, a.Hkv, a.Smax, a.hd, 2);
    auto kern = a.comb() ? fused_attn_kernel<true>(rope_neox, nt, gemm_nsplit)
                         : fused_attn_kernel<false>(rope_neox, nt, gemm_nsplit);
    return attn_decode_launch(a, kern, (bf16_t*)k_cache, (bf16_t*)vt_cache);
}

extern "C" int zk_attn_decode_qkv(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                                  void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                                  const int32_t* ctx_dev, float* work, int nsplit, void* out, int rope_neox,
                                  const int32_t* skip, void* stream) {
    const AttnDecode a{"zk_attn_decode_qkv", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    return attn_decode_qkv(a, part, gemm_nsplit, freqs, k_cache, vt_cache, rope_neox);
}

extern "C" int zk_attn_decode_qkv_part(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                                       void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                                       const int32_t* ctx_dev, float* work, int nsplit, int rope_neox,
                                       const int32_t* skip, void* stream) {
    AttnDecode a{"zk_attn_decode_qkv_part", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, nullptr, skip, stream};
    a.part_only = true;
    return attn_decode_qkv(a, part, gemm_nsplit, freqs, k_cache, vt_cache, rope_neox);
}

extern "C" int zk_attn_decode_q_part(const void* q, const void* k_cache, const void* vt_cache, int R, int H,
                                     int Hkv, int hd, int Smax, int ctx0, const int32_t* ctx_dev, float* work,
                                     int nsplit, const int32_t* skip, void* stream) {
    ZK_REQUIRE(hd == 128, "zk_attn_decode_q_part: head_dim %d unsupported (128 only)", hd);
    ZK_REQUIRE(Hkv > 0 && H % Hkv == 0 && H / Hkv <= AT_G, "zk_attn_decode_q_part: GQA group %d > %d",
               Hkv > 0 ? H / Hkv : 0, AT_G);
    ZK_REQUIRE(Smax % 32 == 0 && Smax > 0, "zk_attn_decode_q_part: Smax=%d must be a multiple of 32", Smax);
    ZK_REQUIRE(nsplit >= 1 && nsplit <= 64, "zk_attn_decode_q_part: nsplit=%d out of [1, 64]", nsplit);
    ZK_REQUIRE(q != nullptr && work != nullptr && k_cache != nullptr && vt_cache != nullptr,
               "zk_attn_decode_q_part: null buffer");
    const float scale = 1.0f / sqrtf((float)hd);
    auto kern = kv_nt(R, Hkv, Smax, hd, 2) ? k_attn_decode_qs<true> : k_attn_decode_qs<false>;
    hipLaunchKernelGGL(kern, dim3(nsplit, Hkv, R), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q,
                       (const bf16_t*)k_cache, (const bf16_t*)vt_cache, H, Hkv, Smax, ctx0, ctx_dev, work, scale, skip);
    ZK_CHECK_LAUNCH("zk_attn_decode_q_part");
    return 0;
}

extern "C" int zk_attn_decode_qkv_sc(const float* part, int gemm_nsplit, const float* freqs, void* k_cache,
                                     void* vt_cache, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                                     const int32_t* ctx_dev, float* work, int nsplit, uint32_t* counters, void* out,
                                     int rope_neox, const int32_t* skip, void* stream) {
    AttnDecode a{"zk_attn_decode_qkv_sc", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    a.counters = counters;
    return attn_decode_qkv(a, part, gemm_nsplit, freqs, k_cache, vt_cache, rope_neox);
}

#ifdef ZK_ATT_PROF
extern "C" int zk_att_prof_set(uint64_t* p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_att_prof), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int zk_attn_prefill(const void* q, const void* k_cache, const void* vt_cache, int R, int S, int H,
                               int Hkv, int hd, int Smax, void* out, void* stream) {
    ZK_REQUIRE(hd == 128, "zk_attn_prefill: head_dim %d unsupported (128 only)", hd);
    ZK_REQUIRE(H % Hkv == 0, "zk_attn_prefill: H %% Hkv != 0");
    if (R * S == 0) return 0;
    const float scale = 1.0f / sqrtf((float)hd);
    ZK_REQUIRE(S <= Smax && Smax % 32 == 0, "zk_attn_prefill: S=%d Smax=%d", S, Smax);
    hipLaunchKernelGGL(k_attn_prefill, dim3((S + 63) / 64, H, R), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k_cache, (const bf16_t*)vt_cache, R, S, H, Hkv, Smax, scale,
                       (bf16_t*)out);
    ZK_CHECK_LAUNCH("zk_attn_prefill");
    return 0;
}

// FP8 KV cache: decode attention and the post-prefill quantiser (zk_*_f8, zk_kv_quantize_e4m3)
#include "attn_f8.h"
