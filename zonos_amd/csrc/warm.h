// L2 warm-up of the next decode GEMM's first weight chunks (internal to the library).
//
// A k_gemm_ws launch is short (5-18 us at c3) and starts cold: every compute wave's first
// weight chunks come from HBM before its first MFMA. The kernel that runs just before it
// (k_resid_ln before in_proj / fc1, the fc1 GEMM before fc2) reads those chunks into the
// L2 of the XCD the GEMM workgroup will run on, from a wave that has nothing else to do, so
// the GEMM starts on L2 hits (tools/microbench.py warm). Results are
// unchanged: the warm-up only loads.
#pragma once
#include <stdint.h>

struct ZkWarm {
    const void* W;     // packed weights of the GEMM to warm (nullptr: off)
    int K;             // GEMM K
    int gx, gz;        // its k_gemm_ws grid (column tiles, K splits)
    int chunks;        // the packed word below
};

// ZkWarm::chunks is one word, so the warming kernels take five scalars: bits 0-7 64-deep chunks per
// compute wave to warm, 8-15 column groups per wave (k_gemm_ws NG, 0 = 1), 16-23 compute waves per
// workgroup of the warmed GEMM (0 = 4), 24-31 trailing 16-column tiles of its grid wholly past N (the
// packed image holds ceil(N / 16) tiles, padded to 64 columns; a 48-column grid can overshoot even
// that -- c5 Mamba in_proj: 178 x 3 = 534 tiles for a 532-tile image -- so those are skipped).
// Packed and unpacked here only, on the host and in the kernels.
#ifdef __HIPCC__
#define ZK_WARM_FN __host__ __device__ inline
#else
#define ZK_WARM_FN inline
#endif
ZK_WARM_FN int warm_pack(int chunks, int ng, int nw, int excess) {
    return chunks | (ng != 1 ? ng << 8 : 0) | (nw != 4 ? nw << 16 : 0) | (excess << 24);
}
ZK_WARM_FN int warm_chunks(int word) { return word & 255; }
ZK_WARM_FN int warm_ng(int word) { return ((word >> 8) & 255) > 1 ? ((word >> 8) & 255) : 1; }
ZK_WARM_FN int warm_nw(int word) { return ((word >> 16) & 255) ? ((word >> 16) & 255) : 4; }
// Compute wave w of the GEMM workgroup in grid column bx streams the 16-column tiles
// warm_tile(word, bx, w, g), g < NG; the tiles below warm_ntiles hold a column < N.
ZK_WARM_FN int warm_tile(int word, int bx, int w, int g) { return (bx * warm_nw(word) + w) * warm_ng(word) + g; }
ZK_WARM_FN int warm_ntiles(int word, int gx) { return gx * warm_nw(word) * warm_ng(word) - ((word >> 24) & 255); }

// k_gemm_ws grid of zk_gemm_bf16(M, N, K, nsplit, mode) when that kernel takes the call with M > 16, or W = nullptr
ZkWarm zk_gemm_warm_desc(const void* W, int M, int N, int K, int nsplit, int mode, int chunks);

int zk_resid_ln_warm(const float* part, int nsplit, const void* x_in, const void* w, const void* b, float eps,
                     int rows, int D, void* x_out, void* xn_out, int ln_on_sum, const int32_t* skip, ZkWarm warm,
                     void* stream);
int zk_gemm_bf16_warm(const void* A, long lda, const void* W, int M, int N, int K, int nsplit, int mode, float* Cpart,
                      void* Cout, const int32_t* skip_flag, ZkWarm warm, void* stream);
