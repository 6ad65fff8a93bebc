// Decode attention over the FP8 (OCP e4m3fn) KV cache and the quantiser that fills it after prefill
// (included by backbone.hip). Same block / wave structure as attn_decode_wg (attn_common.h): 128-key
// blocks, 32 keys per wave, the same split rule, the same mfma_f32_16x16x32_bf16 steps (attn_step) and the
// same tail (attn_finish), so the result is bit for bit that of the bf16 kernel on the dequantised cache.
//
// Cache layout per (row, kv head), 32-key slices of 4 KB (zonos_amd.kvlayout), each lane's load 16 B:
//   K8: [slice][h 2][kp 2][lane 64][q 2][8]  lane = 16*lg + ln holds key 8*(ln>>2) + 4h + (ln&3),
//       dims 32*(2kp + q) + 8lg .. +8
//   V8: [slice][dp 4][lane 64][q 2][8]       lane holds channel 16*(2dp + q) + ln, keys 8lg .. 8lg+7
//   scales: uint8 [Smax] per (row, kv head) for K and for V, byte b = scale 2^(b - 127)
// The bytes are converted to bf16 UNSCALED (exact); the power-of-two scales of the lane's 8 keys multiply
// the scores (K) and the bf16-rounded p (V) inside attn_step<true>, which is exact as well.
//
// In bounds: every data load reads 16 B at slice * 4096 + j * 1024 + lane * 16 (j < 4, lane < 64), every
// scale load 8 B at slice * 32 + 8 * lg (lg < 4), with slice clamped to [0, Smax / 32 - 1] by slice_of();
// so all of them lie inside the (row, kv head) block of Smax * 128 data bytes / Smax scale bytes, for any
// context word, split and wave, including the loads issued before the skip / context test.
#pragma once
#include "attn_common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// ------------------------------------------------------------------ layout and scale rule
ZK_DEV size_t k8_off(int key, int c8) {      // dims 8*c8 .. 8*c8+7 of key (8 contiguous bytes)
    const int o = key & 31, grp = o >> 3, h = (o >> 2) & 1, i = o & 3;
    const int ln = 4 * grp + i, ks = c8 >> 2, lg = c8 & 3;
    return (size_t)(key >> 5) * 4096 + ((h * 2 + (ks >> 1)) * 64 + lg * 16 + ln) * 16 + (ks & 1) * 8;
}
ZK_DEV size_t v8_off(int key, int ch) {      // channel ch of key
    const int o = key & 31, lg = o >> 3, e = o & 7, dt = ch >> 4;
    return (size_t)(key >> 5) * 4096 + ((dt >> 1) * 64 + lg * 16 + (ch & 15)) * 16 + (dt & 1) * 8 + e;
}
// (the scale rule: kv_scale_exp / kv_pow2 of common.h)
// two / four e4m3fn bytes of x * inv, round to nearest even
ZK_DEV uint32_t quant2(float a, float b, float inv) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false) & 0xffffu;
}
ZK_DEV uint32_t quant4(const float* f, float inv) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, w, true);
    return (uint32_t)w;
}

// ------------------------------------------------------------------ fragments
struct KV8Frag {
    uint4 k[2][2];   // [tile h][d-step pair]
    uint4 v[4];      // [d-tile pair]
    uint2 ks, vs;    // scale bytes of keys 8lg .. 8lg+7
};

template <bool NT>
ZK_DEV void load_kv8(KV8Frag& f, const uint8_t* kb, const uint8_t* vb, const uint8_t* ksb, const uint8_t* vsb,
                     int slice, int lane, int lg) {
    const uint8_t* k0 = kb + (size_t)slice * 4096 + lane * 16;
    const uint8_t* v0 = vb + (size_t)slice * 4096 + lane * 16;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) f.k[h][kp] = ld_kv<NT>(reinterpret_cast<const bf16_t*>(k0 + (h * 2 + kp) * 1024));
#pragma unroll
    for (int dp = 0; dp < 4; ++dp) f.v[dp] = ld_kv<NT>(reinterpret_cast<const bf16_t*>(v0 + dp * 1024));
    f.ks = *reinterpret_cast<const uint2*>(ksb + slice * 32 + 8 * lg);
    f.vs = *reinterpret_cast<const uint2*>(vsb + slice * 32 + 8 * lg);
}
ZK_DEV void keep_live(const KV8Frag& f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { keep_live(f.k[i >> 1][i & 1]); keep_live(f.v[i]); }
    keep_live(f.ks);
    keep_live(f.vs);
}

// four e4m3fn bytes -> four bf16 (exact)
ZK_DEV uint2 cvt4(uint32_t w) {
    const bf16x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
    const bf16x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true);
    return make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
}
ZK_DEV void cvt16(uint4 raw, uint4& a, uint4& b) {
    const uint2 x = cvt4(raw.x), y = cvt4(raw.y), z = cvt4(raw.z), w = cvt4(raw.w);
    a = make_uint4(x.x, x.y, y.x, y.y);
    b = make_uint4(z.x, z.y, w.x, w.y);
}
ZK_DEV void scales8(uint2 b, float* s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = __uint_as_float(((b.x >> (8 * j)) & 0xffu) << 23);
        s[4 + j] = __uint_as_float(((b.y >> (8 * j)) & 0xffu) << 23);
    }
}
// one 32-key step: dequantise in registers, then the bf16 step with the scales on the scores and on p
ZK_DEV void attn_step8(AttnState& st, const KV8Frag& f, const bf16x8* qf, int key_base, int ctx, float scale, int lg) {
    KVFrag d;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) cvt16(f.k[h][kp], d.k[h][2 * kp], d.k[h][2 * kp + 1]);
#pragma unroll
    for (int dp = 0; dp < 4; ++dp) cvt16(f.v[dp], d.v[2 * dp], d.v[2 * dp + 1]);
    float sk[8], sv[8];
    scales8(f.ks, sk);
    scales8(f.vs, sv);
    attn_step<true>(st, d, qf, key_base, ctx, scale, lg, sk, sv);
}

// the new key's bytes and scales (fused form), kept in LDS until the end of the kernel
struct __attribute__((aligned(16))) Attn8Smem {
    uint32_t k8[32];     // 128 e4m3fn bytes in dim order
    uint32_t v8[32];
    uint32_t sc[2];      // scale byte of the new key (0) and value (1)
};
ZK_DEV uint2 put_byte(uint2 v, int e, uint32_t b) {      // byte e (0..7) of the 8 <- b
    uint64_t x = (uint64_t)v.x | ((uint64_t)v.y << 32);
    x = (x & ~(0xffull << (8 * e))) | ((uint64_t)b << (8 * e));
    return make_uint2((uint32_t)x, (uint32_t)(x >> 32));
}
// Replace the newest key's bytes and scales in a loaded 32-key slice by the ones kept in LDS (their
// cache lines are written at the end of the kernel), like patch_kv. Wave-uniform early out.
ZK_DEV void patch_kv8(KV8Frag& f, const Attn8Smem& s8, int key_base, int pos, int ln, int lg) {
    if (pos < key_base || pos >= key_base + 32) return;
    const uint8_t* kn = reinterpret_cast<const uint8_t*>(s8.k8);
    const uint8_t* vn = reinterpret_cast<const uint8_t*>(s8.v8);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int key = key_base + 8 * (ln >> 2) + 4 * h + (ln & 3);
        if (key == pos) {
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const uint2 a = *reinterpret_cast<const uint2*>(kn + 64 * kp + 8 * lg);
                const uint2 b = *reinterpret_cast<const uint2*>(kn + 64 * kp + 32 + 8 * lg);
                f.k[h][kp] = make_uint4(a.x, a.y, b.x, b.y);
            }
        }
    }
    const int e = pos - key_base - 8 * lg;      // element of this lane's 8-key group
    if (e >= 0 && e < 8) {
#pragma unroll
        for (int dp = 0; dp < 4; ++dp) {
            const uint2 a = put_byte(make_uint2(f.v[dp].x, f.v[dp].y), e, vn[32 * dp + ln]);
            const uint2 b = put_byte(make_uint2(f.v[dp].z, f.v[dp].w), e, vn[32 * dp + 16 + ln]);
            f.v[dp] = make_uint4(a.x, a.y, b.x, b.y);
        }
        f.ks = put_byte(f.ks, e, s8.sc[0]);
        f.vs = put_byte(f.vs, e, s8.sc[1]);
    }
}

// qkv_prologue restates attn_decode_wg's slab-reduce / RoPE loop line for line; the bf16 kernel keeps its own
// inline copy (with the pre-issued slab form) so that its generated code stays what it was.
// The in_proj epilogue of one workgroup, pairs first, first + 256, ... of [0, (G + 2) * 64): q of heads
// g*G.. (RoPE) into sm.s_q, then the new key (RoPE) into sm.s_kn and the new value into sm.s_vn. prow: the
// row's first slab, fc: the position's (cos, sin) row.
template <bool NEOX>
ZK_DEV void qkv_prologue(AttnSmem& sm, int first, const float* prow, size_t slab, int gsplit, const float* fc,
                         int g, int G, int H, int Hkv) {
    constexpr int HD = 128;
    uint16_t* q16 = reinterpret_cast<uint16_t*>(&sm.s_q[0][0]);
    uint16_t* k16 = reinterpret_cast<uint16_t*>(sm.s_kn);
    auto& s_vn = sm.s_vn;
    for (int pi = first; pi < (G + 2) * (HD / 2); pi += 256) {
        const int hp = pi / (HD / 2), j = pi % (HD / 2);      // hp < G: q head g*G+hp; G: k; G+1: v
        int d0, d1;
        rope_dims<NEOX>(j, HD, d0, d1);
        const int cb = hp < G ? (g * G + hp) * HD : (hp == G ? H * HD + g * HD : (H + Hkv) * HD + g * HD);
        // all slab loads issued together (clamped slab index, select after) -- same
        // left-to-right fp32 sum as k_qkv_rope
        // the slab count is dispatched to an exact-size instantiation (B <= 8: 1 slab, c3: 4),
        // so only real slabs are loaded (one 8-byte load per slab for the interleaved pair)
        float a, bb;
        switch (gsplit) {
            case 1: slab_pair<1, NEOX>(prow + cb, slab, d0, d1, a, bb); break;
            case 2: slab_pair<2, NEOX>(prow + cb, slab, d0, d1, a, bb); break;
            case 4: slab_pair<4, NEOX>(prow + cb, slab, d0, d1, a, bb); break;
            default: slab_pair_n(prow + cb, slab, gsplit, d0, d1, a, bb); break;
        }
        const float2 cs = *reinterpret_cast<const float2*>(fc + 2 * j);
        a = round_bf(a);
        bb = round_bf(bb);
        if (hp <= G) {
            const float o0 = __fsub_rn(__fmul_rn(a, cs.x), __fmul_rn(bb, cs.y));
            const float o1 = __fadd_rn(__fmul_rn(bb, cs.x), __fmul_rn(a, cs.y));
            uint16_t* dst = hp < G ? q16 + hp * HD : k16;
            dst[d0] = f2bf(o0);
            dst[d1] = f2bf(o1);
        } else {
            s_vn[d0] = f2bf(a);
            s_vn[d1] = f2bf(bb);
        }
    }
}

// grid (nsplit, Hkv, R), 256 threads. FUSED: part / gsplit / freqs are the in_proj slabs and the RoPE table
// (interleaved pairs) and the workgroup of the last split stores the new key's bytes and scales at the end;
// otherwise q holds the query rows. COMB (FUSED, nsplit > 1): in-launch combine on cnt.
template <bool FUSED, bool KVNT, bool COMB>
__global__ __launch_bounds__(256, 2) void k_attn_decode_f8(const bf16_t* q, uint8_t* k8, uint8_t* v8, uint8_t* ksc,
                                                           uint8_t* vsc, int R, int H, int Hkv, int Smax, int ctx0,
                                                           const int32_t* ctx_dev, float* work, float scale,
                                                           bf16_t* out, const int32_t* skip, const float* part,
                                                           int gsplit, const float* freqs, uint32_t* cnt) {
    constexpr int HD = 128;
    __shared__ AttnSmem sm;
    __shared__ Attn8Smem s8;
    const int sk = ld_word(skip);
    const int cwr = ld_word(ctx_dev);
    constexpr bool ROWS = false;
    constexpr int ro = 0;
#include "attn_f8_body.inc"
}

#ifndef ZK_ATTN_F8_HELPERS_ONLY      // (attn_rows.hip takes the helpers and the body above only)
// Keys [0, S) of a bf16 fragment-ordered K / V^T cache pair of Ssrc keys per (row, kv head) (a layer's
// prefill scratch) -> the FP8 cache of Smax keys plus scales. grid (ceil(S / 32), Hkv, R), 256 threads:
// thread t takes 16 dims of key t >> 3 of the slice; the 8 threads of a key reduce its amax.
__global__ __launch_bounds__(256) void k_kv_quantize_e4m3(const bf16_t* ksrc, const bf16_t* vsrc, int Hkv, int S,
                                                          int Ssrc, uint8_t* k8, uint8_t* v8, uint8_t* ksc,
                                                          uint8_t* vsc, int Smax) {
    const int key = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;      // key < Ssrc (Ssrc % 32 == 0)
    const size_t blk = (size_t)blockIdx.z * Hkv + blockIdx.y;
    const bf16_t* ks = ksrc + blk * Ssrc * 128;
    const bf16_t* vs = vsrc + blk * Ssrc * 128;
    float fk[16], fv[16];
    unpack8(*reinterpret_cast<const uint4*>(ks + k_off(key, 2 * j)), fk);
    unpack8(*reinterpret_cast<const uint4*>(ks + k_off(key, 2 * j + 1)), fk + 8);
#pragma unroll
    for (int i = 0; i < 16; ++i) fv[i] = bf2f(vs[v_off(key, 16 * j + i)]);
    float ak = 0.f, av = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { ak = fmaxf(ak, fabsf(fk[i])); av = fmaxf(av, fabsf(fv[i])); }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { ak = fmaxf(ak, __shfl_xor(ak, o, 64)); av = fmaxf(av, __shfl_xor(av, o, 64)); }
    if (key >= S) return;      // destination keys >= S stay untouched
    const int ek = kv_scale_exp(ak), ev = kv_scale_exp(av);
    const float ik = kv_pow2(-ek), iv = kv_pow2(-ev);
    uint8_t* kd = k8 + blk * Smax * 128;
    uint8_t* vd = v8 + blk * Smax * 128;
    *reinterpret_cast<uint2*>(kd + k8_off(key, 2 * j)) = make_uint2(quant4(fk, ik), quant4(fk + 4, ik));
    *reinterpret_cast<uint2*>(kd + k8_off(key, 2 * j + 1)) = make_uint2(quant4(fk + 8, ik), quant4(fk + 12, ik));
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
        const uint32_t wv = quant4(fv + i, iv);
#pragma unroll
        for (int b = 0; b < 4; ++b) vd[v8_off(key, 16 * j + i + b)] = (uint8_t)(wv >> (8 * b));
    }
    if (j == 0) {
        ksc[blk * Smax + key] = (uint8_t)(ek + 127);
        vsc[blk * Smax + key] = (uint8_t)(ev + 127);
    }
}

#endif  // ZK_ATTN_F8_HELPERS_ONLY
}  // namespace

#ifndef ZK_ATTN_F8_HELPERS_ONLY
// ------------------------------------------------------------------ entries
extern "C" int zk_kv_quantize_e4m3(const void* k_src, const void* vt_src, int R, int Hkv, int hd, int S, int Smax_src,
                                   void* k8, void* v8, void* k_scale, void* v_scale, int Smax, void* stream) {
    ZK_REQUIRE(hd == 128, "zk_kv_quantize_e4m3: head_dim %d unsupported (128 only)", hd);
    ZK_REQUIRE(Smax > 0 && Smax % AT_KB == 0, "zk_kv_quantize_e4m3: Smax=%d must be a multiple of %d", Smax, AT_KB);
    ZK_REQUIRE(Smax_src > 0 && Smax_src % 32 == 0, "zk_kv_quantize_e4m3: Smax_src=%d must be a multiple of 32",
               Smax_src);
    ZK_REQUIRE(S >= 0 && S <= Smax && S <= Smax_src, "zk_kv_quantize_e4m3: S=%d beyond Smax=%d / Smax_src=%d", S, Smax,
               Smax_src);
    ZK_REQUIRE(k_src != nullptr && vt_src != nullptr && k8 != nullptr && v8 != nullptr && k_scale != nullptr &&
                   v_scale != nullptr,
               "zk_kv_quantize_e4m3: null buffer");
    if (R * Hkv * S == 0) return 0;
    hipLaunchKernelGGL(k_kv_quantize_e4m3, dim3((S + 31) / 32, Hkv, R), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)k_src, (const bf16_t*)vt_src, Hkv, S, Smax_src, (uint8_t*)k8, (uint8_t*)v8,
                       (uint8_t*)k_scale, (uint8_t*)v_scale, Smax);
    ZK_CHECK_LAUNCH("zk_kv_quantize_e4m3");
    return 0;
}

extern "C" int zk_attn_decode_f8(const void* q, const void* k8, const void* v8, const void* k_scale,
                                 const void* v_scale, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                                 const int32_t* ctx_dev, float* work, int nsplit, void* out, const int32_t* skip,
                                 void* stream) {
    AttnDecode a{"zk_attn_decode_f8", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    a.q = q;
    auto kern = kv_nt(R, Hkv, Smax, hd, 1) ? k_attn_decode_f8<false, true, false> : k_attn_decode_f8<false, false, false>;
    return attn_decode_launch(a, kern, (uint8_t*)k8, (uint8_t*)v8, (uint8_t*)k_scale, (uint8_t*)v_scale);
}

extern "C" int zk_attn_decode_qkv_f8(const float* part, int gemm_nsplit, const float* freqs, void* k8, void* v8,
                                     void* k_scale, void* v_scale, int R, int H, int Hkv, int hd, int Smax, int ctx0,
                                     const int32_t* ctx_dev, float* work, int nsplit, uint32_t* counters, void* out,
                                     const int32_t* skip, void* stream) {
    AttnDecode a{"zk_attn_decode_qkv_f8", R, H, Hkv, hd, Smax, ctx0, ctx_dev, work, nsplit, out, skip, stream};
    a.fused = true;
    a.part = part;
    a.gemm_nsplit = gemm_nsplit;
    a.freqs = freqs;
    a.counters = counters;
    const bool nt = kv_nt(R, Hkv, Smax, hd, 1);
    auto kern = a.comb() ? (nt ? k_attn_decode_f8<true, true, true> : k_attn_decode_f8<true, false, true>)
                         : (nt ? k_attn_decode_f8<true, true, false> : k_attn_decode_f8<true, false, false>);
    return attn_decode_launch(a, kern, (uint8_t*)k8, (uint8_t*)v8, (uint8_t*)k_scale, (uint8_t*)v_scale);
}
#endif  // ZK_ATTN_F8_HELPERS_ONLY
