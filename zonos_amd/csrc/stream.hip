// Streaming: audio chunks while generate() is still running.
//
//   k_stream_window : the un-delayed codes of a window [f0, f1) of absolute code frames, taken from the delayed
//                     buffer of the running generation -- revert_delay_pattern (codebook_pattern.py), the
//                     `>= 1024 -> 0` fill and the per-row slice of model.py:437-451, on a window.
//   k_stream_crop   : the chunk's samples [c0, min(end_b, c1)) out of the window's waveform.
//   zk_stream_chunk : window -> the zk_dac_decode sequence on (codes_w, lens_w) -> crop; nothing new is launched
//                     for the convolutions.
//
// Finality. codes[b][k][t] = delayed[b][k][t + k + 1]: frame t is whole once column t + K is written. The host
// polls off = scal[0] - 1 and passes upto = off - K by value -- the device word moves on while these kernels run,
// so they never read it. Columns <= off are never rewritten by later steps.
//
// In bounds. k_stream_window reads delayed[b][0][t + 1] for 1 <= t < upto (the EOS search) and delayed[b][k][t + k + 1]
// for f0 <= t < end_b <= upto, k < K: column indices <= upto - 1 + K - 1 + 1 = upto + K - 1 < Ld, because the entry
// refuses upto > Ld - K. It writes codes_w[b][k][w], w < W, lens_w[b] and end[b], b < B. k_stream_crop reads
// wav_w[b][(c0 - f0) hop + i], i < n_b <= (c1 - c0) hop with c1 <= f1 = f0 + W, and writes chunk[b][i],
// i < (c1 - c0) hop, and n[b].
#include "common.h"
#include "../../include/zonos_hip.h"

#include <algorithm>

namespace {

constexpr int SW_THREADS = 256;
constexpr int64_t SW_EOS = 1024;       // eos_token_id; every id >= 1024 (EOS, MASK) is written as code 0

// one workgroup per row
__global__ __launch_bounds__(SW_THREADS) void k_stream_window(const int64_t* __restrict__ delayed, int K, int Ld, int f0,
                                                              int W, int upto, int64_t* __restrict__ codes_w,
                                                              int32_t* __restrict__ lens_w, int32_t* __restrict__ end) {
    __shared__ int s_eos;
    const int b = blockIdx.x;
    const int64_t* row = delayed + (size_t)b * K * Ld;
    if (threadIdx.x == 0) s_eos = upto;
    __syncthreads();
    // first EOS of codebook 0 at a frame in [1, upto): argmax of (codes[:, 0, :] == EOS), then 0 -> no EOS
    // (model.py:439-440) -- so an EOS at frame 0 hides every later one, as it does there
    const bool eos0 = upto > 0 && row[1] == SW_EOS;
    int first = upto;
    for (int t = 1 + threadIdx.x; t < upto && !eos0; t += SW_THREADS)
        if (row[t + 1] == SW_EOS) {
            first = t;
            break;
        }
    if (first < upto) atomicMin(&s_eos, first);
    __syncthreads();
    const int end_b = s_eos;           // == upto while the row is live
    if (threadIdx.x == 0) {
        end[b] = end_b < upto ? end_b : -1;
        lens_w[b] = std::min(std::max(end_b - f0, 0), W);
    }
    int64_t* out = codes_w + (size_t)b * K * W;
    for (int i = threadIdx.x; i < K * W; i += SW_THREADS) {
        const int k = i / W, t = f0 + i % W;
        int64_t v = 0;
        if (t < end_b) {
            v = row[(size_t)k * Ld + t + k + 1];
            if (v >= SW_EOS) v = 0;
        }
        out[i] = v;
    }
}

// grid (tiles of the chunk, B)
__global__ __launch_bounds__(SW_THREADS) void k_stream_crop(const float* __restrict__ wav_w, int W, int hop, int f0, int c0,
                                                            int c1, const int32_t* __restrict__ end,
                                                            float* __restrict__ chunk, int32_t* __restrict__ n) {
    const int b = blockIdx.y;
    const int e = end[b];
    const int last = e < 0 ? c1 : std::min(e, c1);                 // a live row reaches c1 (c1 <= upto)
    const long nb = (long)std::max(last - c0, 0) * hop;
    const long cap = (long)(c1 - c0) * hop;
    if (blockIdx.x == 0 && threadIdx.x == 0) n[b] = (int32_t)nb;
    const float* src = wav_w + (size_t)b * W * hop + (size_t)(c0 - f0) * hop;
    float* dst = chunk + (size_t)b * cap;
    for (long i = blockIdx.x * (long)SW_THREADS + threadIdx.x; i < cap; i += (long)gridDim.x * SW_THREADS)
        dst[i] = i < nb ? src[i] : 0.f;
}

size_t sw_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct StreamPlan {
    size_t codes, lens, wav, dac, dac_bytes, total;
    int hop;
};

// Workspace of zk_stream_chunk for windows of up to W frames, laid out once for the size query and the run.
bool stream_plan(const zk_stream_desc* d, int W, StreamPlan& p) {
    if (d == nullptr || d->dac == nullptr || d->B <= 0 || d->K <= 0 || W <= 0) return false;
    const zk_dac_desc* q = d->dac;
    if (q->nblocks < 1 || q->nblocks > ZK_DAC_MAXB) return false;
    long hop = 1;
    for (int i = 0; i < q->nblocks; ++i) {
        if (q->blocks[i].stride < 1) return false;
        hop *= q->blocks[i].stride;
    }
    if (hop > (1 << 20) || (long)W * hop > (1L << 30)) return false;
    p.hop = (int)hop;
    p.dac_bytes = zk_dac_decode_workspace(q, d->B, W);
    if (p.dac_bytes == 0) return false;
    p.codes = 0;
    p.lens = sw_align(p.codes + (size_t)d->B * d->K * W * sizeof(int64_t));
    p.wav = sw_align(p.lens + (size_t)d->B * sizeof(int32_t));
    p.dac = sw_align(p.wav + (size_t)d->B * W * hop * sizeof(float));
    p.total = sw_align(p.dac + p.dac_bytes);
    return true;
}

}  // namespace

extern "C" int zk_stream_window(const int64_t* delayed, int B, int K, int Ld, int P, int f0, int f1, int upto,
                                int64_t* codes_w, int32_t* lens_w, int32_t* end, void* stream) {
    ZK_REQUIRE(delayed && codes_w && lens_w && end, "zk_stream_window: null pointer");
    ZK_REQUIRE(B > 0 && K > 0 && Ld > K && P >= 0, "zk_stream_window: bad shape B=%d K=%d Ld=%d P=%d", B, K, Ld, P);
    ZK_REQUIRE(upto >= 0 && upto <= Ld - K, "zk_stream_window: upto=%d must be in [0, Ld - K = %d]", upto, Ld - K);
    ZK_REQUIRE(f0 >= P, "zk_stream_window: f0=%d lies before the audio prefix's end P=%d", f0, P);
    ZK_REQUIRE(f0 < f1, "zk_stream_window: empty window [%d, %d)", f0, f1);
    ZK_REQUIRE((long)K * (f1 - f0) < (1L << 30), "zk_stream_window: window of %d frames too long", f1 - f0);
    hipLaunchKernelGGL(k_stream_window, dim3(B), dim3(SW_THREADS), 0, (hipStream_t)stream, delayed, K, Ld, f0, f1 - f0,
                       upto, codes_w, lens_w, end);
    ZK_CHECK_LAUNCH("zk_stream_window");
    return 0;
}

extern "C" int zk_stream_crop(const float* wav_w, int B, int hop, int f0, int c0, int c1, int f1, const int32_t* end,
                              float* chunk, int32_t* n, void* stream) {
    ZK_REQUIRE(wav_w && end && chunk && n, "zk_stream_crop: null pointer");
    ZK_REQUIRE(B > 0 && hop > 0, "zk_stream_crop: bad shape B=%d hop=%d", B, hop);
    ZK_REQUIRE(0 <= f0 && f0 <= c0 && c0 < c1 && c1 <= f1, "zk_stream_crop: window not ordered f0=%d <= c0=%d < c1=%d <= f1=%d",
               f0, c0, c1, f1);
    ZK_REQUIRE((long)(f1 - f0) * hop < (1L << 30), "zk_stream_crop: window of %d frames too long", f1 - f0);
    const long cap = (long)(c1 - c0) * hop;
    const int tiles = (int)std::min<long>((cap + SW_THREADS - 1) / SW_THREADS, 1024);
    hipLaunchKernelGGL(k_stream_crop, dim3(tiles, B), dim3(SW_THREADS), 0, (hipStream_t)stream, wav_w, f1 - f0, hop, f0,
                       c0, c1, end, chunk, n);
    ZK_CHECK_LAUNCH("zk_stream_crop");
    return 0;
}

extern "C" size_t zk_stream_workspace(const zk_stream_desc* d, int Wmax) {
    StreamPlan p;
    return stream_plan(d, Wmax, p) ? p.total : 0;
}

extern "C" int zk_stream_chunk(const zk_stream_desc* d, int f0, int c0, int c1, int f1, int upto, void* workspace,
                               size_t workspace_bytes, float* chunk_out, int32_t* n_out, int32_t* end_out,
                               void* stream) {
    ZK_REQUIRE(d && d->dac && d->delayed && workspace && chunk_out && n_out && end_out, "zk_stream_chunk: null pointer");
    ZK_REQUIRE(d->B > 0 && d->K > 0 && d->Ld > d->K && d->P >= 0 && d->K == d->dac->ncb,
               "zk_stream_chunk: bad descriptor B=%d K=%d Ld=%d P=%d (the DAC takes %d codebooks)", d->B, d->K, d->Ld,
               d->P, d->dac->ncb);
    ZK_REQUIRE(f0 >= d->P, "zk_stream_chunk: f0=%d lies before the audio prefix's end P=%d", f0, d->P);
    ZK_REQUIRE(f0 <= c0 && c0 < c1 && c1 <= f1, "zk_stream_chunk: window not ordered f0=%d <= c0=%d < c1=%d <= f1=%d", f0,
               c0, c1, f1);
    ZK_REQUIRE(upto <= d->Ld - d->K, "zk_stream_chunk: upto=%d must be <= Ld - K = %d", upto, d->Ld - d->K);
    // a frame at or past upto may still lack columns; only the device knows which rows have ended, so the host's
    // clamp f1 = min(c1 + H, upto) is required of every window
    ZK_REQUIRE(f1 <= upto, "zk_stream_chunk: f1=%d reaches past the final frames upto=%d (clamp it on the host)", f1, upto);
    StreamPlan p;
    ZK_REQUIRE(stream_plan(d, f1 - f0, p), "zk_stream_chunk: bad DAC descriptor or window of %d frames", f1 - f0);
    ZK_REQUIRE(workspace_bytes >= p.total, "zk_stream_chunk: workspace %zu bytes < %zu needed", workspace_bytes, p.total);
    char* ws = static_cast<char*>(workspace);
    int64_t* codes_w = reinterpret_cast<int64_t*>(ws + p.codes);
    int32_t* lens_w = reinterpret_cast<int32_t*>(ws + p.lens);
    float* wav_w = reinterpret_cast<float*>(ws + p.wav);
    ZK_TRY(zk_stream_window(d->delayed, d->B, d->K, d->Ld, d->P, f0, f1, upto, codes_w, lens_w, end_out, stream));
    ZK_TRY(zk_dac_decode(d->dac, codes_w, d->B, f1 - f0, lens_w, ws + p.dac, p.dac_bytes, wav_w, stream));
    ZK_TRY(zk_stream_crop(wav_w, d->B, p.hop, f0, c0, c1, f1, end_out, chunk_out, n_out, stream));
    return 0;
}
