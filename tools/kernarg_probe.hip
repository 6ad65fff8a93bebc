// Kernel-front probe: what does the serial chain at the front of a decode launch cost?
//   (1) kernel-argument load and its wait, (2) dependent load of the step word and the branch
//   on it, (3) first data load.
// One kernel of the decode launches' shape (256 workgroups x 256 threads, seven pointer arguments
// plus ints, a nullable step word behind one of the pointers, one 1 KB load per wave) in two fronts:
//   first : step word loaded and tested, then the data load (what the decode kernels do)
//   defer : step-word scalar load issued at entry, data load issued, then wait and test
// timed as a captured hipGraph chain of 64 dependent launches, replayed, HIP events around the
// replays. Build it twice, without and with kernel-argument preload (user SGPRs filled at wave
// start, link (1) gone), and run the two binaries interleaved, twice:
//   hipcc -O3 --offload-arch=gfx950 tools/kernarg_probe.hip -o tools/kernarg_probe_off
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=16 -DPRELOAD=1 \
//         tools/kernarg_probe.hip -o tools/kernarg_probe_on
//   for i in 1 2; do ./tools/kernarg_probe_off; ./tools/kernarg_probe_on; done
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

#ifndef PRELOAD
#define PRELOAD 0
#endif

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s @%d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static __device__ int32_t zero_word = 0;

// All seven pointers lie in the first 14 argument dwords (what the preload can deliver); the
// ints behind them are epilogue-only.
template <bool DEFER>
__global__ __launch_bounds__(256) void k_front(const uint4* __restrict__ data, const int32_t* skip, const uint4* p2,
                                               const uint4* p3, const uint4* p4, const uint4* p5, uint32_t* out,
                                               int n, int magic) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // < 65536: 1 MB of data, 1 KB per wave
    const int32_t* q = skip != nullptr ? skip : &zero_word;
    int32_t s;
    uint4 v;
    if constexpr (DEFER) {
        asm volatile("s_load_dword %0, %1, 0x0" : "=&s"(s) : "s"(q) : "memory");
        v = data[i];
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(s) : : "memory");   // the exit path's use of v keeps its load above
    } else {
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(s) : "s"(q) : "memory");
        if (s != 0) return;
        v = data[i];
    }
    if (s != 0) {
        asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
        return;
    }
    // epilogue: the late arguments and a store that never happens (the data is all ones)
    const uint32_t acc = v.x ^ v.y ^ v.z ^ v.w;
    if (acc == (uint32_t)magic) {
        const uint4* ps[4] = {p2, p3, p4, p5};
        out[i % (size_t)n] = acc ^ ps[acc & 3][0].x;
    }
}

template <typename K>
static int run(const char* name, K kern, hipStream_t st, const uint4* data, const int32_t* skip, uint32_t* out) {
    const int CHAIN = 64, REPLAYS = 200;
    hipGraph_t g;
    hipGraphExec_t ge;
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
    for (int i = 0; i < CHAIN; ++i)
        hipLaunchKernelGGL(kern, dim3(256), dim3(256), 0, st, data, skip, data, data, data, data, out, 16, 0x12345678);
    CK(hipStreamEndCapture(st, &g));
    CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int i = 0; i < 20; ++i) CK(hipGraphLaunch(ge, st));
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < REPLAYS; ++i) CK(hipGraphLaunch(ge, st));
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("preload %-3s %-12s : %6.3f us per launch\n", PRELOAD ? "on" : "off", name, ms * 1e3 / (CHAIN * REPLAYS));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    CK(hipGraphExecDestroy(ge));
    CK(hipGraphDestroy(g));
    return 0;
}

int main() {
    uint4* data;
    int32_t* skip;
    uint32_t* out;
    CK(hipMalloc(&data, 1 << 20));
    CK(hipMemset(data, 0xff, 1 << 20));
    CK(hipMalloc(&skip, 64));
    CK(hipMemset(skip, 0, 64));
    CK(hipMalloc(&out, 64));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    for (int rep = 0; rep < 2; ++rep) {
        if (run("first", k_front<false>, st, data, skip, out)) return 1;
        if (run("defer", k_front<true>, st, data, skip, out)) return 1;
    }
    CK(hipDeviceSynchronize());
    return 0;
}
