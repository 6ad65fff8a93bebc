// The body of k_attn_decode_f8 and k_attn_decode_f8_rows (attn_f8.h): one text, two kernels, so the uniform
// kernel's code stays what it was. The including kernel has declared the LDS (sm, s8), loaded the step words
// (sk, cwr) and defines ROWS; with ROWS it has also loaded ro = row_off[r], the row's context offset.
    const int split = blockIdx.x, nsplit = gridDim.x, g = blockIdx.y, r = blockIdx.z;
    const auto bar = [] { __syncthreads(); };
    // (the context is clamped to the cache: a skipped launch after the last step may see ctx = Smax + 1;
    // ROWS: row_off is device data, and a bad offset must stay in bounds)
    int ctx_;
    if constexpr (ROWS) ctx_ = (int)max(1L, min((long)ctx0 + uni(cwr) + uni(ro), (long)Smax));
    else ctx_ = max(1, min(ctx0 + uni(cwr), Smax));
    const int ctx = ctx_;
    const int nkb = (ctx + AT_KB - 1) / AT_KB;
    const int kb0 = (int)((long)split * nkb / nsplit), kb1 = (int)((long)(split + 1) * nkb / nsplit);
    const int G = H / Hkv;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ln = lane & 15, lg = lane >> 4;
    const size_t blk = (size_t)r * Hkv + g;
    uint8_t* kb = k8 + blk * Smax * HD;
    uint8_t* vb = v8 + blk * Smax * HD;
    uint8_t* ksb = ksc + blk * Smax;
    uint8_t* vsb = vsc + blk * Smax;
    // this wave's slice of key block b, clamped into the cache whatever b is (see the in-bounds note above)
    const int nsl = Smax >> 5;
    const auto slice_of = [&](int b) { return max(0, min(b * 4 + w, nsl - 1)); };
    // as attn_decode_wg: the wave multiplies only the blocks whose slice holds a visible key
    const int vis = ctx - 32 * w;
    const int kbw = vis <= 0 ? kb0 : max(kb0, min(kb1, (vis + AT_KB - 1) / AT_KB));
    const int last = kbw - 1;
    const int pos = ctx - 1;
    KV8Frag fa, fb;
    // the first two key blocks are requested before the skip word is tested and stream during the prologue
    load_kv8<KVNT>(fa, kb, vb, ksb, vsb, slice_of(kb0), lane, lg);
    load_kv8<KVNT>(fb, kb, vb, ksb, vsb, slice_of(min(kb0 + 1, max(last, kb0))), lane, lg);
    if (uni(sk) != 0) {      // skip: nothing is written
        keep_live(fa);
        keep_live(fb);
        return;
    }
    bf16x8 qf[4];
    if constexpr (FUSED) {
        const int N = (H + 2 * Hkv) * HD;
        qkv_prologue<false>(sm, threadIdx.x, part + (size_t)r * N, (size_t)R * N, gsplit, freqs + (size_t)pos * HD, g, G,
                            H, Hkv);
        bar();      // q, new k, new v (bf16) in LDS
        if (w < 2) {      // wave 0 quantises the new key, wave 1 the new value: one amax over the 128 dims each
            const uint32_t pr = w == 0 ? sm.s_kn[lane] : reinterpret_cast<const uint32_t*>(sm.s_vn)[lane];
            const float a = __uint_as_float(pr << 16), b = __uint_as_float(pr & 0xffff0000u);
            const int e = kv_scale_exp(wave_max(fmaxf(fabsf(a), fabsf(b))));
            uint16_t* dst = reinterpret_cast<uint16_t*>(w == 0 ? s8.k8 : s8.v8);
            dst[lane] = (uint16_t)quant2(a, b, kv_pow2(-e));
            if (lane == 0) s8.sc[w] = (uint32_t)(e + 127);
        }
        bar();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ln < G) v = *reinterpret_cast<const uint4*>(&sm.s_q[ln][ks * 16 + lg * 4]);
            qf[ks] = as_frag(v);
        }
    } else {
        const bf16_t* qr = q + (size_t)r * H * HD + (size_t)(g * G + ln) * HD;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ln < G) v = *reinterpret_cast<const uint4*>(qr + ks * 32 + lg * 8);
            qf[ks] = as_frag(v);
        }
    }
    AttnState st;
    st.m = -INFINITY;
    st.l = 0.f;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) st.o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = kb0; it < kbw; it += 2) {
        if (it != kb0 && it + 1 < kbw) load_kv8<KVNT>(fb, kb, vb, ksb, vsb, slice_of(it + 1), lane, lg);
        if (FUSED) patch_kv8(fa, s8, it * AT_KB + 32 * w, pos, ln, lg);
        attn_step8(st, fa, qf, it * AT_KB + 32 * w, ctx, scale, lg);
        if (it + 2 < kbw) load_kv8<KVNT>(fa, kb, vb, ksb, vsb, slice_of(it + 2), lane, lg);
        if (it + 1 < kbw) {
            if (FUSED) patch_kv8(fb, s8, (it + 1) * AT_KB + 32 * w, pos, ln, lg);
            attn_step8(st, fb, qf, (it + 1) * AT_KB + 32 * w, ctx, scale, lg);
        }
    }
    if (FUSED && split == nsplit - 1) {      // the split owning the newest key stores it (cache for later steps)
        const int t = threadIdx.x;
        if (t < 16) *reinterpret_cast<uint2*>(kb + k8_off(pos, t)) = reinterpret_cast<const uint2*>(s8.k8)[t];
        else if (t < 16 + HD) vb[v8_off(pos, t - 16)] = reinterpret_cast<const uint8_t*>(s8.v8)[t - 16];
        else if (t == 16 + HD) ksb[pos] = (uint8_t)s8.sc[0];
        else if (t == 17 + HD) vsb[pos] = (uint8_t)s8.sc[1];
    }
    attn_finish<COMB>(sm, bar, st, split, nsplit, g, r, H, Hkv, work, out, cnt);
