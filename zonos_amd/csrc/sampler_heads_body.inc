// The body of the engine sampler kernels, included by sampler.hip into k_sample_heads<TN> (ROWS = false: the
// batch-wide parameters `spa` arrive by value) and into k_sample_heads_rows (TN = false, ROWS = true: `spa` is the
// device zk_row_params [B]). Text, not a function: inlined from a __device__ function the batch-wide kernels came
// out with other register numbers and a few more instructions than before the rows mode existed; included, they
// are byte-identical (profiles/request_rows_vs_parent.txt).
// In scope: Smem s; part, nsplit, st, spa, prefill, draw, dbg (the kernel's arguments); constexpr bool TN, ROWS.
    const int B = st.B, K = st.K, V = st.V;
    const int b = blockIdx.x / K, k = blockIdx.x % K;
    const int32_t* scal = st.scal;
    // Every load that does not depend on another one is issued up front (one memory round trip):
    // the done word, the step scalars, this row's state and the logits; the finished check comes
    // after them (the loads are in bounds either way).
    const int done = scal[3];
    const int offset = scal[0], step = scal[2], nres = scal[4];
    const float rpb = st.rp[b];
    const int actb = st.act[b];
    // ROWS: this utterance's parameters, a wave-uniform address read with the loads above
    const zk_row_params rw = heads_row(spa, b);
    const zk_sampling_params& sp = heads_sp(spa, rw);
    int new_eos_b = 0;
    if (draw == 1) {
        if constexpr (ROWS) {   // this row's own new EOS (model.py:380 at batch size 1); no scan of the others
            new_eos_b = (st.tok0[b * K] == EOS) && !st.eos_mode[b];
            if (!new_eos_b || done) return;
        } else {       // EOS resample happens only if some row has a new EOS (model.py:380)
            int any = 0;   // one row per thread
            for (int r = threadIdx.x; r < B; r += NT) any |= (st.tok0[r * K] == EOS) && !st.eos_mode[r];
            if (!__syncthreads_or(any && !done)) return;
            new_eos_b = (st.tok0[b * K] == EOS) && !st.eos_mode[b];
        }
    }
    const size_t N = (size_t)K * V;
    const size_t slab = (size_t)2 * B * N;
    const float* pc = part + (size_t)b * N + (size_t)k * V;
    const float* pu = part + (size_t)(b + B) * N + (size_t)k * V;
    float x[NPT];
    if (nsplit == 1) {     // the unsplit heads GEMM (c3, B <= 8): all 2 x NPT loads before the first use
        float c1[NPT], u1[NPT];
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int v = min(threadIdx.x + NT * i, V - 1);
            c1[i] = pc[v];
            u1[i] = pu[v];
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int v = threadIdx.x + NT * i;
            float val = -INFINITY;
            if (v < V) {
                const float c = round_bf(0.f + c1[i]), u = round_bf(0.f + u1[i]);   // head output bf16 (model.py:111)
                val = __fadd_rn(u, __fmul_rn(__fsub_rn(c, u), sp.cfg_scale));       // model.py:114
                if (v >= 1025) val = -INFINITY;                                    // model.py:115
            }
            x[i] = val;
        }
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        if (nsplit == 1) break;
        const int v = threadIdx.x + NT * i;
        float val = -INFINITY;
        if (v < V) {
            float c = 0.f, u = 0.f;
            for (int sp_ = 0; sp_ < nsplit; ++sp_) { c += pc[sp_ * slab + v]; u += pu[sp_ * slab + v]; }
            c = round_bf(c); u = round_bf(u);                              // head output bf16 (model.py:111)
            val = __fadd_rn(u, __fmul_rn(__fsub_rn(c, u), sp.cfg_scale)); // model.py:114
            if (v >= 1025) val = -INFINITY;                                // model.py:115
        }
        x[i] = val;
    }
    if (done) return;                                       // generation finished
    if (dbg != nullptr && draw == 0) {
        float* d = dbg + ((size_t)b * K + k) * V;
#pragma unroll
        for (int i = 0; i < NPT; ++i) { const int v = threadIdx.x + NT * i; if (v < V) d[v] = x[i]; }
    }
    // bias + EOS masks for the EOS column only (threads owning v == EOS)
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int v = threadIdx.x + NT * i;
        if (v == EOS) {
            if (!prefill) {
                if (k >= 1) x[i] = -INFINITY;                                  // model.py:323
                else x[i] = __fadd_rn(x[i], 0.0f - LOG1024F);                  // model.py:324,353
                if (k == 0 && actb) x[i] = -INFINITY;                          // model.py:360-361
                if (k == 0 && new_eos_b) x[i] = -INFINITY;                     // model.py:387
            }
            if (k == 0 && sp.force_full_length) x[i] = -INFINITY;              // benchmark mode
        }
    }
    // torch noise mode: the reference's sampler calls so far -- the prefill sample, one per earlier
    // decode step (scal[2] starts at 1) and one per earlier EOS resample (scal[4]) -- each took
    // noise_incr of the generator's Philox offset (model.py:304,365,388)
    const long call = prefill ? 0 : (long)step + nres + draw;
    int nrow = st.row_base + b;
    uint64_t nseed = st.seed;
    if constexpr (ROWS) { nrow = rw.key; nseed = rw.seed; }
    RowCtx c{b, k, V, prefill ? nullptr : st.delayed + ((size_t)b * K + k) * st.Ld, offset,
             prefill ? 1.f : rpb, prefill ? 0 : step, draw, nrow, nseed,
             st.noise_offset + (uint64_t)call * (uint64_t)st.noise_incr, st.noise_mode ? st.noise_stride : 0,
             ((long)(st.row_base + b) * K + k) * V};
    const int t = sample_row<TN>(x, c, sp, s);
    if (threadIdx.x == 0) (draw ? st.tok1 : st.tok0)[b * K + k] = t;
