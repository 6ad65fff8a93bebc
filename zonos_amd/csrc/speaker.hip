// Speaker-embedding network of voice cloning (zonos/speaker_cloning.py): log-mel front end
// (logFbankCal, :12-34), ResNet293 of SimAM basic blocks (:63-95, :152-195), attentive statistics
// pooling (ASP, :37-60), the 256-wide bottleneck (:213, :222) and the LDA projection (:404, :411).
//
// Layout: activations are channels-last [B][F][T][C] (F = mel axis, T = frames), as two tensors like
// the DAC pipeline (dac_cl.hip): the fp32 residual stream x and the fp16 input s of the next conv.
// Every conv is an implicit GEMM on v_mfma_f32_16x16x32_f16 (M = output channels, N = output
// positions, K = taps x input channels) with fp16 operands and fp32 accumulation; the eval-mode
// BatchNorm stays an fp32 per-channel scale and shift in the epilogue, so the only operand rounding
// is "input and weight to fp16". SimAM needs the per-(clip, channel) mean and variance of the whole
// conv2 + bn2 output: the conv writes per-tile (count, mean, M2) partials, zk_spk_simam combines them
// in tile order (Chan's update, no atomics) and applies the gate, the shortcut and the ReLU.
#include "common.h"
#include "../../include/zonos_hip.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

ZK_DEV f16x8 as_h8(uint4 v) { return __builtin_bit_cast(f16x8, v); }
ZK_DEV uint2 pack_h4(float a, float b, float c, float d) {
    _Float16 h[4] = {(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};
    return *reinterpret_cast<const uint2*>(h);
}

// ---------------------------------------------------------------- log-mel front end
constexpr int NFFT = 512, NBIN = NFFT / 2 + 1, HOP = 160, FPAD = NFFT / 2;

// One workgroup per (clip, frame). The 512-point DFT is a direct sum in fp64 against a host-built
// twiddle table (131 k multiply-adds per frame: nothing next to the network), so the kernel's error is
// that of the fp32 window product and of the final log alone. window fp32 [512] is the periodic Hann
// window of 400 samples zero-padded centrally; frames are centred with reflect padding of 256.
__global__ __launch_bounds__(256) void k_logfbank(const float* __restrict__ wav, int n, int T,
                                                  const float* __restrict__ window,
                                                  const double* __restrict__ twiddle,
                                                  const float* __restrict__ melfb, int n_mels,
                                                  float* __restrict__ out) {
    __shared__ double xw[NFFT];
    __shared__ double tw[NFFT][2];
    __shared__ double pw[NBIN];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* x = wav + (size_t)b * n;
    for (int j = tid; j < NFFT; j += 256) {
        int i = t * HOP + j - FPAD;
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
        xw[j] = (double)(window[j] * x[i]);
        tw[j][0] = twiddle[2 * j];
        tw[j][1] = twiddle[2 * j + 1];
    }
    __syncthreads();
    for (int k = tid; k < NBIN; k += 256) {
        double re = 0.0, im = 0.0;
        for (int j = 0; j < NFFT; ++j) {
            const int q = (k * j) & (NFFT - 1);
            re += xw[j] * tw[q][0];
            im += xw[j] * tw[q][1];
        }
        pw[k] = re * re + im * im;
    }
    __syncthreads();
    if (tid < n_mels) {
        double acc = 0.0;
        for (int k = 0; k < NBIN; ++k) acc += (double)melfb[k * n_mels + tid] * pw[k];
        out[((size_t)b * n_mels + tid) * T + t] = logf((float)acc + 1e-6f);
    }
}

// out[b][m][:] -= mean over time (fp64 sum: per-thread strided partials, then a fixed-order tree)
__global__ __launch_bounds__(256) void k_fbank_center(float* __restrict__ feat, int T) {
    __shared__ double red[256];
    float* row = feat + (size_t)blockIdx.x * T;
    double s = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) s += (double)row[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float mean = (float)(red[0] / (double)T);
    for (int t = threadIdx.x; t < T; t += 256) row[t] = row[t] - mean;
}

// ---------------------------------------------------------------- stem: Conv2d(1 -> C, 3x3, pad 1) + BN + ReLU
__global__ __launch_bounds__(256) void k_stem(const float* __restrict__ feat, int F, int T, int C,
                                              const float* __restrict__ w, const float* __restrict__ scale,
                                              const float* __restrict__ shift, float* __restrict__ x,
                                              uint16_t* __restrict__ s, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const size_t pos = idx / C;
    const int t = (int)(pos % T);
    const int f = (int)((pos / T) % F);
    const size_t b = pos / ((size_t)T * F);
    const float* img = feat + b * (size_t)F * T;
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ff = f + kh - 1, tt = t + kw - 1;
            const float v = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? img[(size_t)ff * T + tt] : 0.f;
            acc = fmaf(v, w[c * 9 + kh * 3 + kw], acc);
        }
    const float y = fmaxf(acc * scale[c] + shift[c], 0.f);
    x[idx] = y;
    reinterpret_cast<_Float16*>(s)[idx] = (_Float16)y;
}

// ---------------------------------------------------------------- implicit-GEMM 2-D conv
// Workgroup tile: CO output channels x (4 output rows x 16 output columns), 4 waves. CO = 64: waves as 2
// (channel halves) x 2 (row pairs), each 32 channels x 2 rows of 16 positions = 2 x 2 MFMA blocks. CO = 32
// (small grids: twice the workgroups, so that a CU holds more than one and their loads overlap): one
// row of 16 positions per wave, 2 x 1 blocks. Every output element is the same K-ordered sum in both.
// K is walked in chunks of 32 input channels: per chunk the input window of the tile ((3 S + KS) rows x
// (15 S + KS) columns x 32 channels) and the chunk's weights (taps x CO x 32) are staged in LDS once
// and every tap reads the window shifted by (kh, kw). The next chunk's global loads are issued
// before the taps of this one are multiplied. Positions outside the image are staged as zeros.
// Weights arrive packed [Cout / 64][Cin / 32][tap][64][32] fp16 (rows past Cout are zero).
constexpr int CV_TF = 4, CV_TT = 16;
constexpr int CV_SMALL_GRID = 512;      // workgroups of the CO = 64 form below which CO = 32 is used

template <int KS, int S, int CO>
__global__ __launch_bounds__(256) void k_conv2d(const uint16_t* __restrict__ in, int Cin, int Fi, int Ti,
                                                const uint16_t* __restrict__ w, int Cout, int Fo, int To,
                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                int relu, uint16_t* __restrict__ out_s, float* __restrict__ out_x,
                                                float* __restrict__ stats, int tiles_t) {
    constexpr int TAPS = KS * KS, PAD = KS / 2;
    constexpr int WR = (CV_TF - 1) * S + KS, WC = (CV_TT - 1) * S + KS, NP = WR * WC;
    constexpr int NWIN = (NP * 4 + 255) / 256;          // 16-B groups per thread: window
    constexpr int WU4 = TAPS * CO * 4;                  // 16-B groups of one chunk's weights
    constexpr int NWT = (WU4 + 255) / 256;
    constexpr int WLDS = WU4 > 16 * CO ? WU4 : 16 * CO; // the statistics staging (64 x CO fp32) reuses it
    constexpr int NB = CO == 64 ? 2 : 1;                // rows of 16 positions per wave
    __shared__ uint4 lds_w[WLDS];
    __shared__ uint4 lds_x[NP * 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, lg = lane >> 4;
    const int cb = CO == 64 ? (wave & 1) * 32 : 0;      // this wave's channels within the tile
    const int row0 = CO == 64 ? (wave >> 1) * 2 : wave; // ... and its first output row
    const int tile = blockIdx.x, tt = tile % tiles_t, tf = tile / tiles_t;
    const int f0 = tf * CV_TF, t0 = tt * CV_TT, co0 = blockIdx.y * CO, b = blockIdx.z;
    const int nchunk = Cin >> 5;
    // the packed 64-row tile holding co0, and this tile's 32-row half of it when CO = 32
    const uint4* wsrc = reinterpret_cast<const uint4*>(w) + (size_t)(co0 >> 6) * nchunk * (TAPS * 256) + ((co0 >> 5) & 1) * (CO == 64 ? 0 : 128);

    // window addresses of this thread (the same for every chunk but for the channel offset)
    const uint16_t* xsrc[NWIN];
#pragma unroll
    for (int i = 0; i < NWIN; ++i) {
        const int idx = tid + i * 256, pos = idx >> 2, g = idx & 3;
        const int r = pos / WC, c = pos - r * WC;
        const int fi = f0 * S - PAD + r, ti = t0 * S - PAD + c;
        xsrc[i] = (idx < NP * 4 && fi >= 0 && fi < Fi && ti >= 0 && ti < Ti)
                      ? in + (((size_t)b * Fi + fi) * Ti + ti) * Cin + g * 8
                      : nullptr;
    }
    uint4 xr[NWIN], wr[NWT];

    f32x4 acc[2][NB];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = -1; c < nchunk; ++c) {                  // pass -1 only loads chunk 0
        if (c >= 0) {
            __syncthreads();                             // the previous chunk has been multiplied
#pragma unroll
            for (int i = 0; i < NWIN; ++i)
                if (tid + i * 256 < NP * 4) lds_x[tid + i * 256] = xr[i];
#pragma unroll
            for (int i = 0; i < NWT; ++i)
                if (tid + i * 256 < WU4) lds_w[tid + i * 256] = wr[i];
            __syncthreads();
        }
        if (c + 1 < nchunk) {                            // the next chunk's loads fly over this chunk's taps
#pragma unroll
            for (int i = 0; i < NWIN; ++i)
                xr[i] = xsrc[i] ? *reinterpret_cast<const uint4*>(xsrc[i] + (c + 1) * 32) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < NWT; ++i) {
                const int idx = tid + i * 256, tap = idx / (CO * 4), within = idx - tap * (CO * 4);
                wr[i] = idx < WU4 ? wsrc[(size_t)(c + 1) * (TAPS * 256) + tap * 256 + within] : make_uint4(0, 0, 0, 0);
            }
        }
        if (c < 0) continue;
#pragma unroll
        for (int kh = 0; kh < KS; ++kh)
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
                uint4 a[2], bq[NB];
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    a[m] = lds_w[((kh * KS + kw) * CO + cb + m * 16 + ln) * 4 + lg];
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    bq[n] = lds_x[(((row0 + n) * S + kh) * WC + ln * S + kw) * 4 + lg];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NB; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_h8(a[m]), as_h8(bq[n]), acc[m][n], 0, 0, 0);
            }
    }

    // acc[m][n][i] = C[co = co0 + cb + 16 m + 4 lg + i][row f0 + row0 + n][column t0 + ln]
    float* st = reinterpret_cast<float*>(lds_w);         // [64 positions][CO channels]
    if (stats) __syncthreads();                          // every wave is done with the weights
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int cl = cb + m * 16 + lg * 4, co = co0 + cl;
        float4 sc = make_float4(0.f, 0.f, 0.f, 0.f), sh = sc;
        if (co < Cout) {
            sc = *reinterpret_cast<const float4*>(scale + co);
            sh = *reinterpret_cast<const float4*>(shift + co);
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int fo = f0 + row0 + n, to = t0 + ln;
            float v0 = acc[m][n][0] * sc.x + sh.x, v1 = acc[m][n][1] * sc.y + sh.y;
            float v2 = acc[m][n][2] * sc.z + sh.z, v3 = acc[m][n][3] * sc.w + sh.w;
            if (relu) {
                v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
            }
            if (stats) *reinterpret_cast<float4*>(st + ((row0 + n) * 16 + ln) * CO + cl) = make_float4(v0, v1, v2, v3);
            if (co < Cout && fo < Fo && to < To) {
                const size_t o = (((size_t)b * Fo + fo) * To + to) * Cout + co;
                if (out_x) *reinterpret_cast<float4*>(out_x + o) = make_float4(v0, v1, v2, v3);
                if (out_s) *reinterpret_cast<uint2*>(out_s + o) = pack_h4(v0, v1, v2, v3);
            }
        }
    }
    if (stats) {
        __syncthreads();
        if (tid < CO && co0 + tid < Cout) {
            const int nf = min(CV_TF, Fo - f0), nt = min(CV_TT, To - t0);
            float sum = 0.f;
            for (int r = 0; r < nf; ++r)
                for (int q = 0; q < nt; ++q) sum += st[(r * 16 + q) * CO + tid];
            const float cnt = (float)(nf * nt), mean = sum / cnt;
            float m2 = 0.f;
            for (int r = 0; r < nf; ++r)
                for (int q = 0; q < nt; ++q) {
                    const float d = st[(r * 16 + q) * CO + tid] - mean;
                    m2 += d * d;
                }
            float* o = stats + ((size_t)b * gridDim.x + tile) * 3 * Cout + co0 + tid;
            o[0] = cnt;
            o[Cout] = mean;
            o[2 * Cout] = m2;
        }
    }
}

// ---------------------------------------------------------------- SimAM
// (count, mean, M2) of tiles [t0, t1) combined in tile order (Chan et al.)
ZK_DEV void chan_merge(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
    const float nn = n + nb, d = mb - mean;
    mean = mean + d * (nb / nn);
    m2 = m2 + m2b + d * d * (n * nb / nn);
    n = nn;
}

// One workgroup per (clip, 32 channels): 8 segments of the tile list are combined in order by one
// thread each, then the 8 results in segment order. moments[b][0][c] = mean, [b][1][c] = 1 / (4 (v + 1e-4)).
__global__ __launch_bounds__(256) void k_simam_reduce(const float* __restrict__ stats, int ntiles, int C, int npos,
                                                      float* __restrict__ moments) {
    __shared__ float part[8][3][32];
    const int cl = threadIdx.x & 31, seg = threadIdx.x >> 5, c = blockIdx.x * 32 + cl, b = blockIdx.y;
    const int per = (ntiles + 7) / 8, t0 = seg * per, t1 = min(ntiles, t0 + per);
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int t = t0; t < t1; ++t) {
        const float* p = stats + ((size_t)b * ntiles + t) * 3 * C + c;
        if (t == t0) {
            n = p[0]; mean = p[C]; m2 = p[2 * C];
        } else {
            chan_merge(n, mean, m2, p[0], p[C], p[2 * C]);
        }
    }
    part[seg][0][cl] = n; part[seg][1][cl] = mean; part[seg][2][cl] = m2;
    __syncthreads();
    if (seg == 0) {
        for (int s = 1; s < 8; ++s)
            if (part[s][0][cl] > 0.f) chan_merge(n, mean, m2, part[s][0][cl], part[s][1][cl], part[s][2][cl]);
        const float v = m2 / (float)max(npos - 1, 1);
        moments[((size_t)b * 2) * C + c] = mean;
        moments[((size_t)b * 2 + 1) * C + c] = 1.0f / (4.0f * (v + 1e-4f));
    }
}

// x_out = relu(X sigmoid((X - mu)^2 / (4 (v + 1e-4)) + 0.5) + shortcut); s_out = fp16(x_out).
// x_out may alias shortcut (each thread reads its 4 values before it writes them).
__global__ __launch_bounds__(256) void k_simam_apply(const float* __restrict__ y, const float* __restrict__ moments,
                                                     const float* shortcut, int C, size_t per_clip, size_t total4,
                                                     float* x_out, uint16_t* __restrict__ s_out) {
    const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i4 >= total4) return;
    const size_t e = i4 * 4, b = e / per_clip;
    const int c = (int)(e % C);
    const float4 X = *reinterpret_cast<const float4*>(y + e);
    const float4 mu = *reinterpret_cast<const float4*>(moments + b * 2 * C + c);
    const float4 iv = *reinterpret_cast<const float4*>(moments + (b * 2 + 1) * C + c);
    const float4 sc = *reinterpret_cast<const float4*>(shortcut + e);
    auto gate = [](float X, float mu, float iv, float sc) {
        const float d = X - mu;
        const float z = d * d * iv + 0.5f;
        return fmaxf(X * (1.0f / (1.0f + expf(-z))) + sc, 0.f);
    };
    const float o0 = gate(X.x, mu.x, iv.x, sc.x), o1 = gate(X.y, mu.y, iv.y, sc.y);
    const float o2 = gate(X.z, mu.z, iv.z, sc.z), o3 = gate(X.w, mu.w, iv.w, sc.w);
    *reinterpret_cast<float4*>(x_out + e) = make_float4(o0, o1, o2, o3);
    *reinterpret_cast<uint2*>(s_out + e) = pack_h4(o0, o1, o2, o3);
}

// ---------------------------------------------------------------- attentive statistics pooling
constexpr int ASP_A = 128;        // attention bottleneck width (ASP.attention[0], speaker_cloning.py:45)

// hidden[b][t][j] = BN(relu(W1[j] . x[b, :, t] + b1[j])); the feature axis is channels-last
// (index f C + c), W1 permuted to it on the host. One workgroup per (clip, frame).
__global__ __launch_bounds__(256) void k_asp_hidden(const float* __restrict__ x, int C, int F, int T,
                                                    const float* __restrict__ w1, const float* __restrict__ b1,
                                                    const float* __restrict__ bns, const float* __restrict__ bnb,
                                                    float* __restrict__ hidden) {
    extern __shared__ float xv[];
    const int t = blockIdx.x, b = blockIdx.y, CF = C * F;
    for (int i = threadIdx.x; i < CF; i += 256) {
        const int f = i / C, c = i - f * C;
        xv[i] = x[(((size_t)b * F + f) * T + t) * C + c];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < ASP_A; j += 4) {
        const float* wj = w1 + (size_t)j * CF;
        float acc = 0.f;
        for (int k = lane; k < CF; k += 64) acc = fmaf(wj[k], xv[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) hidden[((size_t)b * T + t) * ASP_A + j] = fmaxf(acc + b1[j], 0.f) * bns[j] + bnb[j];
    }
}

// One thread per feature i = f C + c: logits over time from its W2 row (held in registers), an online
// softmax over the frames in order, mu = sum w x, sg = sqrt(clamp(sum w x^2 - mu^2, 1e-5)). Written in
// the reference's order (feature c F + f; mu block then sg block, speaker_cloning.py:53-57).
__global__ __launch_bounds__(128) void k_asp_pool(const float* __restrict__ x, int C, int F, int T,
                                                  const float* __restrict__ hidden, const float* __restrict__ w2,
                                                  const float* __restrict__ b2, float* __restrict__ pooled) {
    __shared__ float hs[32][ASP_A];
    const int CF = C * F, i = blockIdx.x * 128 + threadIdx.x, b = blockIdx.y;
    const bool live = i < CF;
    const int ii = live ? i : 0, f = ii / C, c = ii - f * C;
    float w[ASP_A];
#pragma unroll
    for (int k = 0; k < ASP_A; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(w2 + (size_t)ii * ASP_A + k);
        w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
    }
    const float bias = b2[ii];
    float mx = -INFINITY, l = 0.f, a1 = 0.f, a2 = 0.f;
    for (int tb = 0; tb < T; tb += 32) {
        const int nt = min(32, T - tb);
        __syncthreads();
        for (int q = threadIdx.x; q < nt * ASP_A; q += 128)
            hs[q / ASP_A][q % ASP_A] = hidden[((size_t)b * T + tb) * ASP_A + q];
        __syncthreads();
        for (int tt = 0; tt < nt; ++tt) {
            float logit = bias;
#pragma unroll
            for (int k = 0; k < ASP_A; ++k) logit = fmaf(w[k], hs[tt][k], logit);
            const float xv = x[(((size_t)b * F + f) * T + tb + tt) * C + c];
            if (logit > mx) {
                const float r = expf(mx - logit);
                l *= r; a1 *= r; a2 *= r;
                mx = logit;
            }
            const float e = expf(logit - mx);
            l += e;
            a1 += e * xv;
            a2 += e * xv * xv;
        }
    }
    if (live) {
        const float mu = a1 / l, ex2 = a2 / l;
        const size_t o = (size_t)b * 2 * CF + (size_t)c * F + f;
        pooled[o] = mu;
        pooled[o + CF] = sqrtf(fmaxf(ex2 - mu * mu, 1e-5f));
    }
}

// out[b][n] = W[n] . in[b] + bias[n], fp32; one workgroup per (n, b)
__global__ __launch_bounds__(256) void k_linear(const float* __restrict__ in, int K, const float* __restrict__ w,
                                                const float* __restrict__ bias, int N, float* __restrict__ out) {
    __shared__ float red[4];
    const int n = blockIdx.x, b = blockIdx.y;
    const float* wn = w + (size_t)n * K;
    const float* xb = in + (size_t)b * K;
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) acc = fmaf(wn[k], xb[k], acc);
    acc = block_sum<256>(acc, red);
    if (threadIdx.x == 0) out[(size_t)b * N + n] = acc + bias[n];
}

inline int out_dim(int n, int stride) { return (n - 1) / stride + 1; }
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// Workspace of zk_speaker_embed, laid out once for the size query and the run.
struct SpkPlan {
    size_t feat, x, s, h, y, d, stats, moments, hidden, pooled, total;
    int T, Fl, Tl, Cl;               // frames; geometry after the last block
};

const char* spk_plan(const zk_spk_desc* d, int B, int n, SpkPlan* p) {
    if (d == nullptr || d->blocks == nullptr || d->nblocks < 1) return "null descriptor or no blocks";
    if (d->n_mels != 80) return "the front end has 80 mel bins";
    if (d->c0 < 32 || d->c0 % 32 != 0) return "channel counts must be multiples of 32";
    if (d->att_dim != ASP_A) return "the pooling attention is 128 wide";
    if (d->emb_dim < 1 || d->lda_dim < 1) return "bad head sizes";
    if (B < 1 || B > 65535) return "bad batch size";
    if (n <= 256) return "a clip needs more than 256 samples (reflect padding of the first frame)";
    if (n > 16000 * 600) return "a clip is at most 600 s";
    const int T = 1 + n / HOP;
    int F = d->n_mels, Tc = T, C = d->c0;
    size_t act = (size_t)B * F * T * C, stats = 0;
    int cmax = C;
    for (int i = 0; i < d->nblocks; ++i) {
        const zk_spk_block& k = d->blocks[i];
        if (k.cin != C) return "a block's input channels do not continue the previous block";
        if (k.cout < 32 || k.cout % 32 != 0) return "channel counts must be multiples of 32";
        if (k.stride != 1 && k.stride != 2) return "stride is 1 or 2";
        if ((k.stride != 1 || k.cin != k.cout) != (k.wd != nullptr)) return "a block changes shape exactly when it has a shortcut conv";
        if (!k.w1 || !k.w2 || !k.scale1 || !k.shift1 || !k.scale2 || !k.shift2) return "a block lacks weights";
        if (k.wd && (!k.scaled || !k.shiftd)) return "a shortcut conv lacks its BatchNorm";
        F = out_dim(F, k.stride);
        Tc = out_dim(Tc, k.stride);
        C = k.cout;
        cmax = C > cmax ? C : cmax;
        const size_t e = (size_t)B * F * Tc * C;
        act = e > act ? e : act;
        const size_t st = (size_t)B * zk_spk_conv_tiles(F, Tc) * 3 * C;
        stats = st > stats ? st : stats;
    }
    if ((size_t)C * F != (size_t)d->pool_dim) return "pool_dim is not channels x mel rows after the last block";
    if ((size_t)d->pool_dim * sizeof(float) > 48 * 1024) return "the pooled feature vector exceeds the pooling kernel's LDS";
    p->T = T; p->Fl = F; p->Tl = Tc; p->Cl = C;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
    p->feat = take((size_t)B * d->n_mels * T * 4);
    p->x = take(act * 4);
    p->s = take(act * 2);
    p->h = take(act * 2);
    p->y = take(act * 4);
    p->d = take(act * 4);
    p->stats = take(stats * 4);
    p->moments = take((size_t)B * 2 * cmax * 4);
    p->hidden = take((size_t)B * Tc * ASP_A * 4);
    p->pooled = take((size_t)B * 2 * d->pool_dim * 4);
    p->total = o;
    return nullptr;
}

}  // namespace

extern "C" int zk_spk_conv_tiles(int Fo, int To) {
    return ((Fo + CV_TF - 1) / CV_TF) * ((To + CV_TT - 1) / CV_TT);
}

extern "C" int zk_spk_logfbank(const float* wav, int B, int n, const float* window, const double* twiddle,
                               const float* melfb, int n_mels, float* out, void* stream) {
    ZK_REQUIRE(wav && window && twiddle && melfb && out, "zk_spk_logfbank: null pointer");
    ZK_REQUIRE(B >= 1 && B <= 65535 && n > 256 && n_mels >= 1 && n_mels <= 256,
               "zk_spk_logfbank: needs 1 <= B <= 65535, n > 256 (reflect padding), 1 <= n_mels <= 256 (B=%d n=%d n_mels=%d)",
               B, n, n_mels);
    const int T = 1 + n / HOP;
    hipLaunchKernelGGL(k_logfbank, dim3(T, B), dim3(256), 0, (hipStream_t)stream, wav, n, T, window, twiddle, melfb,
                       n_mels, out);
    ZK_CHECK_LAUNCH("zk_spk_logfbank");
    hipLaunchKernelGGL(k_fbank_center, dim3(B * n_mels), dim3(256), 0, (hipStream_t)stream, out, T);
    ZK_CHECK_LAUNCH("zk_spk_logfbank(center)");
    return 0;
}

extern "C" int zk_spk_stem(const float* feat, int B, int F, int T, const float* w, const float* scale,
                           const float* shift, int C, float* x, uint16_t* s, void* stream) {
    ZK_REQUIRE(feat && w && scale && shift && x && s, "zk_spk_stem: null pointer");
    ZK_REQUIRE(B >= 1 && F >= 1 && T >= 1 && C >= 32 && C % 32 == 0,
               "zk_spk_stem: needs B, F, T >= 1 and C a multiple of 32 (C=%d)", C);
    const size_t total = (size_t)B * F * T * C;
    hipLaunchKernelGGL(k_stem, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, feat, F, T, C,
                       w, scale, shift, x, s, total);
    ZK_CHECK_LAUNCH("zk_spk_stem");
    return 0;
}

extern "C" int zk_spk_conv2d_cl(const uint16_t* in, int B, int Cin, int Fi, int Ti, const uint16_t* w, int Cout,
                                int ks, int stride, const float* scale, const float* shift, int relu,
                                uint16_t* out_s, float* out_x, float* stats, void* stream) {
    ZK_REQUIRE(in && w && scale && shift && (out_s || out_x), "zk_spk_conv2d_cl: null pointer");
    ZK_REQUIRE(Cin >= 32 && Cin % 32 == 0 && Cout >= 32 && Cout % 32 == 0,
               "zk_spk_conv2d_cl: channel counts must be multiples of 32 (Cin=%d Cout=%d)", Cin, Cout);
    ZK_REQUIRE((ks == 1 || ks == 3) && (stride == 1 || stride == 2),
               "zk_spk_conv2d_cl: kernel 1 or 3, stride 1 or 2 (ks=%d stride=%d)", ks, stride);
    ZK_REQUIRE(B >= 1 && B <= 65535 && Fi >= 1 && Ti >= 1, "zk_spk_conv2d_cl: bad shape");
    const int Fo = out_dim(Fi, stride), To = out_dim(Ti, stride);
    const int tiles_t = (To + CV_TT - 1) / CV_TT;
    const int ntile = zk_spk_conv_tiles(Fo, To);
    const bool small = (long)ntile * ((Cout + 63) / 64) * B < CV_SMALL_GRID;
    const dim3 grid(ntile, small ? Cout / 32 : (Cout + 63) / 64, B);
    hipStream_t st = (hipStream_t)stream;
#define ZK_SPK_CONV(KS_, S_, CO_)                                                                                     \
    hipLaunchKernelGGL((k_conv2d<KS_, S_, CO_>), grid, dim3(256), 0, st, in, Cin, Fi, Ti, w, Cout, Fo, To, scale, \
                       shift, relu, out_s, out_x, stats, tiles_t)
#define ZK_SPK_CONV2(KS_, S_)         \
    do {                              \
        if (small) ZK_SPK_CONV(KS_, S_, 32); \
        else ZK_SPK_CONV(KS_, S_, 64);       \
    } while (0)
    if (ks == 3 && stride == 1) ZK_SPK_CONV2(3, 1);
    else if (ks == 3) ZK_SPK_CONV2(3, 2);
    else if (stride == 1) ZK_SPK_CONV2(1, 1);
    else ZK_SPK_CONV2(1, 2);
#undef ZK_SPK_CONV2
#undef ZK_SPK_CONV
    ZK_CHECK_LAUNCH("zk_spk_conv2d_cl");
    return 0;
}

extern "C" int zk_spk_simam(const float* y, int B, int C, int F, int T, const float* stats, const float* shortcut,
                            float* moments, float* x_out, uint16_t* s_out, void* stream) {
    ZK_REQUIRE(y && stats && shortcut && moments && x_out && s_out, "zk_spk_simam: null pointer");
    ZK_REQUIRE(B >= 1 && B <= 65535 && C >= 32 && C % 32 == 0 && F >= 1 && T >= 1,
               "zk_spk_simam: channel count must be a multiple of 32 (C=%d)", C);
    hipLaunchKernelGGL(k_simam_reduce, dim3(C / 32, B), dim3(256), 0, (hipStream_t)stream, stats,
                       zk_spk_conv_tiles(F, T), C, F * T, moments);
    ZK_CHECK_LAUNCH("zk_spk_simam(reduce)");
    const size_t per_clip = (size_t)F * T * C, total4 = per_clip * B / 4;
    hipLaunchKernelGGL(k_simam_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y,
                       moments, shortcut, C, per_clip, total4, x_out, s_out);
    ZK_CHECK_LAUNCH("zk_spk_simam");
    return 0;
}

extern "C" int zk_spk_asp(const float* x, int B, int C, int F, int T, const float* w1, const float* b1,
                          const float* bn_scale, const float* bn_shift, const float* w2, const float* b2, int att_dim,
                          float* hidden, float* pooled, void* stream) {
    ZK_REQUIRE(x && w1 && b1 && bn_scale && bn_shift && w2 && b2 && hidden && pooled, "zk_spk_asp: null pointer");
    ZK_REQUIRE(att_dim == ASP_A, "zk_spk_asp: the attention is %d wide (att_dim=%d)", ASP_A, att_dim);
    ZK_REQUIRE(B >= 1 && B <= 65535 && C >= 32 && C % 32 == 0 && F >= 1 && T >= 1 && (size_t)C * F * 4 <= 48 * 1024,
               "zk_spk_asp: needs C a multiple of 32 and C x F <= 12288 (C=%d F=%d)", C, F);
    const int CF = C * F;
    hipLaunchKernelGGL(k_asp_hidden, dim3(T, B), dim3(256), (size_t)CF * 4, (hipStream_t)stream, x, C, F, T, w1, b1,
                       bn_scale, bn_shift, hidden);
    ZK_CHECK_LAUNCH("zk_spk_asp(hidden)");
    hipLaunchKernelGGL(k_asp_pool, dim3((CF + 127) / 128, B), dim3(128), 0, (hipStream_t)stream, x, C, F, T, hidden,
                       w2, b2, pooled);
    ZK_CHECK_LAUNCH("zk_spk_asp");
    return 0;
}

extern "C" int zk_spk_head(const float* pooled, int B, int K, const float* wb, const float* bb, int E,
                           const float* wl, const float* bl, int L, float* emb, float* lda, void* stream) {
    ZK_REQUIRE(pooled && wb && bb && wl && bl && emb && lda, "zk_spk_head: null pointer");
    ZK_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && E >= 1 && L >= 1, "zk_spk_head: bad shape");
    hipLaunchKernelGGL(k_linear, dim3(E, B), dim3(256), 0, (hipStream_t)stream, pooled, K, wb, bb, E, emb);
    ZK_CHECK_LAUNCH("zk_spk_head(bottleneck)");
    hipLaunchKernelGGL(k_linear, dim3(L, B), dim3(256), 0, (hipStream_t)stream, emb, E, wl, bl, L, lda);
    ZK_CHECK_LAUNCH("zk_spk_head");
    return 0;
}

extern "C" size_t zk_speaker_workspace_bytes(const zk_spk_desc* d, int B, int n) {
    SpkPlan p;
    const char* why = spk_plan(d, B, n, &p);
    if (why) {
        zk_set_error("zk_speaker_workspace_bytes: %s", why);
        return 0;
    }
    return p.total;
}

extern "C" int zk_speaker_embed(const zk_spk_desc* d, const float* wav16k, int B, int n, void* workspace,
                                size_t workspace_bytes, float* emb256, float* lda128, void* stream) {
    SpkPlan p;
    const char* why = spk_plan(d, B, n, &p);
    ZK_REQUIRE(why == nullptr, "zk_speaker_embed: %s", why);
    ZK_REQUIRE(d->window && d->twiddle && d->melfb && d->stem_w && d->stem_scale && d->stem_shift && d->asp_w1 &&
                   d->asp_b1 && d->asp_bn_scale && d->asp_bn_shift && d->asp_w2 && d->asp_b2 && d->bott_w && d->bott_b &&
                   d->lda_w && d->lda_b,
               "zk_speaker_embed: the descriptor lacks a table or a weight");
    ZK_REQUIRE(wav16k && workspace && emb256 && lda128, "zk_speaker_embed: null pointer");
    ZK_REQUIRE(workspace_bytes >= p.total, "zk_speaker_embed: workspace %zu bytes < %zu needed", workspace_bytes, p.total);
    char* ws = static_cast<char*>(workspace);
    float* feat = reinterpret_cast<float*>(ws + p.feat);
    float* x = reinterpret_cast<float*>(ws + p.x);
    uint16_t* s = reinterpret_cast<uint16_t*>(ws + p.s);
    uint16_t* h = reinterpret_cast<uint16_t*>(ws + p.h);
    float* y = reinterpret_cast<float*>(ws + p.y);
    float* dn = reinterpret_cast<float*>(ws + p.d);
    float* stats = reinterpret_cast<float*>(ws + p.stats);
    float* moments = reinterpret_cast<float*>(ws + p.moments);
    float* hidden = reinterpret_cast<float*>(ws + p.hidden);
    float* pooled = reinterpret_cast<float*>(ws + p.pooled);

    ZK_TRY(zk_spk_logfbank(wav16k, B, n, d->window, d->twiddle, d->melfb, d->n_mels, feat, stream));
    int F = d->n_mels, T = p.T;
    ZK_TRY(zk_spk_stem(feat, B, F, T, d->stem_w, d->stem_scale, d->stem_shift, d->c0, x, s, stream));
    for (int i = 0; i < d->nblocks; ++i) {
        const zk_spk_block& k = d->blocks[i];
        const int Fo = out_dim(F, k.stride), To = out_dim(T, k.stride);
        // SimAMBasicBlock.forward (speaker_cloning.py:82-88)
        ZK_TRY(zk_spk_conv2d_cl(s, B, k.cin, F, T, k.w1, k.cout, 3, k.stride, k.scale1, k.shift1, 1, h, nullptr,
                                nullptr, stream));
        const float* shortcut = x;
        if (k.wd) {
            ZK_TRY(zk_spk_conv2d_cl(s, B, k.cin, F, T, k.wd, k.cout, 1, k.stride, k.scaled, k.shiftd, 0, nullptr, dn,
                                    nullptr, stream));
            shortcut = dn;
        }
        ZK_TRY(zk_spk_conv2d_cl(h, B, k.cout, Fo, To, k.w2, k.cout, 3, 1, k.scale2, k.shift2, 0, nullptr, y, stats,
                                stream));
        ZK_TRY(zk_spk_simam(y, B, k.cout, Fo, To, stats, shortcut, moments, x, s, stream));
        F = Fo;
        T = To;
    }
    ZK_TRY(zk_spk_asp(x, B, p.Cl, F, T, d->asp_w1, d->asp_b1, d->asp_bn_scale, d->asp_bn_shift, d->asp_w2, d->asp_b2,
                      d->att_dim, hidden, pooled, stream));
    return zk_spk_head(pooled, B, 2 * d->pool_dim, d->bott_w, d->bott_b, d->emb_dim, d->lda_w, d->lda_b, d->lda_dim,
                       emb256, lda128, stream);
}
