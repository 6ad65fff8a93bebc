"""GPU: the opt-in FP8 (e4m3fn) KV cache -- the post-prefill quantiser, the decode attention over the byte
cache (bit-equal to the bf16 kernels on the dequantised cache) and generate(kv_dtype="fp8")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from zonos_amd import kvlayout as kl

from .golden_util import COPY_CASES, TINY, load_gen_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 128


def _smax(n):
    return ((n + 255) // 256) * 256


def _finite_bytes(shape, g):
    """Random e4m3fn bytes without the two NaN codes (0x7F, 0xFF)."""
    b = torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
    return torch.where((b & 0x7F) == 0x7F, torch.full_like(b, 0x3C), b).to(torch.uint8)


def _mixed(R, Hk, S, g, lo=-6, hi=6):
    """bf16 [R][Hk][S][128] with a different magnitude per key (2^lo .. 2^hi) and one all-zero key."""
    x = torch.randn(R, Hk, S, HD, generator=g) * torch.exp2(torch.randint(lo, hi + 1, (R, Hk, S, 1), generator=g).float())
    x[0, 0, S // 2] = 0
    return x.to(torch.bfloat16)


def _fp8_cache(R, Hk, ctx, smax, seed, fill_seed):
    """Quantised K / V of ctx random keys in a cache of smax; positions >= ctx hold finite random bytes and
    scales chosen by fill_seed. Returns unpacked (kq, ks, vq, vs) uint8 tensors [R][Hk][smax][128] / [..][smax].
    Key magnitudes 2^-6 .. 2^1 (7 scale exponents), value magnitudes 2^-4 .. 2^-1: |out| stays below ~2, where
    the bf16 rounding of p and of the output is inside test_gpu_ops' 2e-2 bound."""
    g = torch.Generator().manual_seed(seed)
    k, v = _mixed(R, Hk, ctx, g, -6, 1), _mixed(R, Hk, ctx, g, -4, -1)
    gf = torch.Generator().manual_seed(fill_seed)
    kq, vq = _finite_bytes((R, Hk, smax, HD), gf), _finite_bytes((R, Hk, smax, HD), gf)
    ks = torch.randint(100, 150, (R, Hk, smax), generator=gf, dtype=torch.int32).to(torch.uint8)
    vs = torch.randint(100, 150, (R, Hk, smax), generator=gf, dtype=torch.int32).to(torch.uint8)
    kq[:, :, :ctx], ks[:, :, :ctx] = kl.quantize_kv_e4m3(k)
    vq[:, :, :ctx], vs[:, :, :ctx] = kl.quantize_kv_e4m3(v)
    return kq, ks, vq, vs


def _dev(*ts):
    return [t.contiguous().to(DEV) for t in ts]


# ---------------------------------------------------------------------------- 1. the quantiser
@pytest.mark.parametrize("Hk", [1, 4])
@pytest.mark.parametrize("S", [1, 37, 256, 300])
def test_kv_quantize_matches_host_reference(Hk, S):
    from zonos_amd._lib import call, ptr, stream_ptr
    R, ssrc, smax = 3, ((S + 127) // 128) * 128, _smax(S)
    g = torch.Generator().manual_seed(100 * Hk + S)
    k, v = _mixed(R, Hk, ssrc, g), _mixed(R, Hk, ssrc, g)
    ksrc, vsrc = _dev(kl.pack_k(k), kl.pack_v(v))
    k8 = torch.full((R, Hk, smax * HD), 0xAB, dtype=torch.uint8, device=DEV)
    v8 = torch.full((R, Hk, smax * HD), 0xCD, dtype=torch.uint8, device=DEV)
    ksc = torch.full((R, Hk, smax), 0x55, dtype=torch.uint8, device=DEV)
    vsc = torch.full((R, Hk, smax), 0x66, dtype=torch.uint8, device=DEV)
    call("zk_kv_quantize_e4m3", ptr(ksrc), ptr(vsrc), R, Hk, HD, S, ssrc, ptr(k8), ptr(v8), ptr(ksc), ptr(vsc), smax,
         stream_ptr())
    torch.cuda.synchronize()
    for src, got, gsc, fill, sfill, unpack in ((k, k8, ksc, 0xAB, 0x55, kl.unpack_k8),
                                               (v, v8, vsc, 0xCD, 0x66, kl.unpack_v8)):
        q, s = kl.quantize_kv_e4m3(src[:, :, :S])
        u = unpack(got.cpu(), smax)
        assert torch.equal(u[:, :, :S], q) and torch.equal(gsc.cpu()[:, :, :S], s)
        assert (u[:, :, S:] == fill).all() and (gsc.cpu()[:, :, S:] == sfill).all(), "keys >= S were touched"


# ---------------------------------------------------------------------------- 2. unfused decode attention
def _decode_f8(q, kq, ks, vq, vs, R, H, Hk, smax, ctx, nsplit):
    from zonos_amd._lib import call, ptr, stream_ptr
    work = torch.empty(R * Hk * nsplit * (8 + 4 * HD), device=DEV)
    out = torch.full((R, H * HD), 7.0, dtype=torch.bfloat16, device=DEV)
    qd, k8, v8, ksd, vsd = _dev(q, kl.pack_k8(kq), kl.pack_v8(vq), ks, vs)
    call("zk_attn_decode_f8", ptr(qd), ptr(k8), ptr(v8), ptr(ksd), ptr(vsd), R, H, Hk, HD, smax, ctx, None, ptr(work),
         nsplit, ptr(out), None, stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("R,ctx,H,Hk,nsplit", [(4, 1, 16, 4, 1), (3, 300, 16, 4, 2), (2, 129, 16, 4, 2),
                                                (2, 1000, 2, 1, 8), (128, 513, 16, 4, 1), (1, 2999, 16, 4, 24),
                                                (2, 256, 16, 4, 2), (2, 1024, 2, 1, 3)])
def test_attention_decode_f8_bit_equal_to_bf16_on_dequantised_cache(R, ctx, H, Hk, nsplit):
    """The last two shapes have ctx == smax."""
    from zonos_amd._lib import call, ptr, stream_ptr
    smax = _smax(ctx)
    nsplit = min(nsplit, smax // 128)
    kq, ks, vq, vs = _fp8_cache(R, Hk, ctx, smax, seed=ctx + R, fill_seed=1)
    q = torch.randn(R, H * HD, generator=torch.Generator().manual_seed(ctx)).to(torch.bfloat16)
    out = _decode_f8(q, kq, ks, vq, vs, R, H, Hk, smax, ctx, nsplit)
    # the bf16 kernel on the dequantised cache
    kd, vd = kl.dequantize_kv_e4m3(kq, ks), kl.dequantize_kv_e4m3(vq, vs)
    work = torch.empty(R * Hk * nsplit * (8 + 4 * HD), device=DEV)
    ref = torch.empty(R, H * HD, dtype=torch.bfloat16, device=DEV)
    qd, kc, vt = _dev(q, kl.pack_k(kd), kl.pack_v(vd))
    call("zk_attn_decode", ptr(qd), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx, None, ptr(work), nsplit, ptr(ref), None,
         stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out, ref), (out.float() - ref.float()).abs().max()
    # fp32 SDPA of the dequantised values, the bound of test_gpu_ops.test_attention_decode
    sd = F.scaled_dot_product_attention(q.view(R, 1, H, HD).transpose(1, 2).float(), kd[:, :, :ctx].float(),
                                        vd[:, :, :ctx].float(), enable_gqa=True).transpose(1, 2).reshape(R, H * HD)
    assert (out.float().cpu() - sd).abs().max() < 2e-2, (out.float().cpu() - sd).abs().max()
    # positions >= ctx hold other bytes and scales: the same bits
    kq2, ks2, vq2, vs2 = _fp8_cache(R, Hk, ctx, smax, seed=ctx + R, fill_seed=2)
    assert torch.equal(kq2[:, :, :ctx], kq[:, :, :ctx]) and (ctx == smax or not torch.equal(kq2, kq))
    assert torch.equal(_decode_f8(q, kq2, ks2, vq2, vs2, R, H, Hk, smax, ctx, nsplit), out)


# ---------------------------------------------------------------------------- 3. fused == separate
@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("R,ctx,H,Hk,nsplit,gs", [(4, 1, 16, 4, 1, 4), (6, 37, 2, 1, 2, 2), (128, 300, 16, 4, 1, 4),
                                                   (3, 700, 16, 4, 4, 8), (2, 129, 2, 1, 1, 1), (5, 256, 16, 4, 2, 3)])
def test_attention_decode_qkv_f8_equals_separate(R, ctx, H, Hk, nsplit, gs, counters):
    """zk_attn_decode_qkv_f8 == zk_qkv_rope at ctx - 1 into a bf16 scratch + the host quantisation of that
    key + zk_attn_decode_f8: the same output bits and the same cache and scale bytes; a launch with the skip
    word set writes nothing."""
    from zonos_amd._lib import call, ptr, stream_ptr
    from zonos_amd.engine import rope_table
    smax = _smax(ctx)
    nsplit = min(nsplit, smax // 128)
    pos = ctx - 1
    g = torch.Generator().manual_seed(R * 1000 + ctx)
    N = (H + 2 * Hk) * HD
    part = (torch.randn(gs, R, N, generator=g) * 0.5).to(DEV)
    freqs = rope_table(16384, HD).to(DEV)
    s = stream_ptr()
    kq, ks, vq, vs = _fp8_cache(R, Hk, max(pos, 1), smax, seed=ctx, fill_seed=5)
    # separate: RoPE into a zeroed bf16 scratch, quantise its key `pos` on the host, unfused attention
    kc_s = torch.zeros(R, Hk, smax * HD, dtype=torch.bfloat16, device=DEV)
    vt_s = torch.zeros(R, Hk, smax * HD, dtype=torch.bfloat16, device=DEV)
    q = torch.empty(R, H * HD, dtype=torch.bfloat16, device=DEV)
    call("zk_qkv_rope", ptr(part), gs, R, 1, H, Hk, HD, ptr(freqs), pos, None, ptr(q), ptr(kc_s), ptr(vt_s), smax, None,
         0, None, s)
    torch.cuda.synchronize()
    kq1, ks1, vq1, vs1 = kq.clone(), ks.clone(), vq.clone(), vs.clone()
    kq1[:, :, pos], ks1[:, :, pos] = kl.quantize_kv_e4m3(kl.unpack_k(kc_s.cpu(), smax)[:, :, pos])
    vq1[:, :, pos], vs1[:, :, pos] = kl.quantize_kv_e4m3(kl.unpack_v(vt_s.cpu(), smax)[:, :, pos])
    out1 = _decode_f8(q.cpu(), kq1, ks1, vq1, vs1, R, H, Hk, smax, ctx, nsplit)
    # fused
    k8, v8, ksd, vsd = _dev(kl.pack_k8(kq), kl.pack_v8(vq), ks, vs)
    work = torch.empty(R * Hk * nsplit * (8 + 4 * HD), device=DEV)
    cnt = torch.zeros(R * Hk, dtype=torch.int32, device=DEV) if counters else None
    out2 = torch.full((R, H * HD), 7.0, dtype=torch.bfloat16, device=DEV)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    before = [t.clone() for t in (k8, v8, ksd, vsd, out2)]
    args = (ptr(part), gs, ptr(freqs), ptr(k8), ptr(v8), ptr(ksd), ptr(vsd), R, H, Hk, HD, smax, ctx, None, ptr(work),
            nsplit, ptr(cnt), ptr(out2))
    call("zk_attn_decode_qkv_f8", *args, ptr(skip), s)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (k8, v8, ksd, vsd, out2))), "a skipped launch wrote"
    call("zk_attn_decode_qkv_f8", *args, None, s)
    torch.cuda.synchronize()
    assert torch.equal(kl.unpack_k8(k8.cpu(), smax), kq1) and torch.equal(ksd.cpu(), ks1)
    assert torch.equal(kl.unpack_v8(v8.cpu(), smax), vq1) and torch.equal(vsd.cpu(), vs1)
    assert torch.equal(out1, out2), (out1.float() - out2.float()).abs().max()


# ---------------------------------------------------------------------------- 4-7. the engine
def _engine(W, cfg=TINY):
    from zonos_amd.engine import EngineConfig, HipDecoder
    ec = EngineConfig(d_model=cfg.d_model, n_layer=cfg.n_layer, n_heads=cfg.n_heads, n_kv=cfg.n_kv, d_ff=cfg.d_ff,
                      eps=cfg.eps)
    return HipDecoder(ec, W, "cuda")


def _gen(eng, c, **kw):
    return eng.generate(c["cond"].cuda(), c["prefix"].cuda(), c["max_new"], 2.0, c["B"], c["sp"], seed=5, **kw)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["sampled_cli", "eos_sampled"])
def test_engine_fp8_paths_agree_and_rekey(case, monkeypatch):
    from zonos_amd.engine import HipDecoder
    c = load_gen_case(case)
    base = _gen(_engine(c["W"]), c)                                   # the default (bf16) path, fresh engine
    eng = _engine(c["W"])
    graph = _gen(eng, c, kv_dtype="fp8", poll_every=7)
    ws = eng._ws
    assert ws["kv"].dtype == torch.uint8 and ws["kv_scale"].dtype == torch.uint8
    R, Hk, smax, S = ws["R"], TINY.n_kv, ws["smax"], ws["S_pre"]
    k8 = kl.unpack_k8(ws["kv"][0, 0].view(R, Hk, -1).cpu(), smax)[:, :, :S]
    v8 = kl.unpack_v8(ws["kv"][0, 1].view(R, Hk, -1).cpu(), smax)[:, :, :S]
    ksc, vsc = (ws["kv_scale"][0, j].view(R, Hk, smax).cpu()[:, :, :S] for j in range(2))
    eager = _gen(eng, c, kv_dtype="fp8", use_graph=False, poll_every=1)
    assert _same(graph, eager)
    monkeypatch.setattr(HipDecoder, "c_step", False)
    assert _same(graph, _gen(eng, c, kv_dtype="fp8"))                 # the Python launch sequence
    monkeypatch.setattr(HipDecoder, "c_step", True)
    again = _gen(eng, c, kv_dtype="bf16")                             # same engine: the workspace is re-keyed
    assert eng._ws["kv"].dtype == torch.bfloat16 and _same(base, again)
    # layer 0 sees the same inputs in both modes: its FP8 prefill cache is the quantised bf16 one
    kb = kl.unpack_k(eng._ws["kv"][0, 0].view(R, Hk, -1).cpu(), smax)[:, :, :S]
    vb = kl.unpack_v(eng._ws["kv"][0, 1].view(R, Hk, -1).cpu(), smax)[:, :, :S]
    (kq, ks), (vq, vs) = kl.quantize_kv_e4m3(kb), kl.quantize_kv_e4m3(vb)
    assert torch.equal(k8, kq) and torch.equal(ksc, ks) and torch.equal(v8, vq) and torch.equal(vsc, vs)


@pytest.mark.parametrize("name", COPY_CASES)
def test_engine_fp8_copy_fixtures_bit_identical(name):
    """Free-running greedy on the copy-head fixtures: the reference's golden codes, bit for bit (the CPU
    emulation of the format flips none of the 1323 decisions of copy_greedy)."""
    c = load_gen_case(name)
    eng = _engine(c["W"], c["cfg"])
    out = eng.generate(c["cond"].cuda(), c["prefix"].cuda(), c["max_new"], 2.0, c["B"], c["sp"], seed=c["seed"],
                       poll_every=5, kv_dtype="fp8")
    lens = [int(x.shape[1]) for x in out]
    assert lens == c["lens"].tolist()
    for i, x in enumerate(out):
        got, ref = x.cpu().numpy(), c["codes"][i, :, :lens[i]]
        assert np.array_equal(got, ref), (i, np.argwhere(got != ref)[:3].tolist())


# fp32 CFG logits of the greedy fixture, teacher-forced on the golden history, FP8 KV against the reference's
# golden logits. Measured on the MI355X: max 0.344 over the 49 steps, largest per-step mean 0.0605 (step 0:
# 0.188 / 0.024); the bars are 30 % above those (the convention of test_gpu_fullwidth.py) and below the
# ceiling of the bf16 bar plus the CPU emulation's quantisation error (0.5 + 0.375 max, 0.04 + 0.06 mean).
# Step 0 (exact prefill) keeps the bf16 bar.
FP8_LOGIT_MAX, FP8_LOGIT_MEAN = 0.45, 0.079
BF16_LOGIT_MAX, BF16_LOGIT_MEAN = 0.5, 0.04


def test_engine_fp8_teacher_forced_logits():
    c = load_gen_case("greedy")
    gold = torch.from_numpy(c["delayed"]).long().cuda()
    P = c["prefix"].shape[2]
    eng = _engine(c["W"])
    trace = {}

    def force(frame, step):
        if frame.shape[2]:
            off = P + 1 + step
            frame.copy_(gold[..., off:off + 1])
        return True

    eng.generate(c["cond"].cuda(), c["prefix"].cuda(), c["max_new"], 2.0, c["B"], c["sp"], seed=c["seed"], trace=trace,
                 callback=lambda f, s, n: force(f, s), _after_prefill=lambda f: force(f, 0), kv_dtype="fp8")
    ref = c["logits"]
    errs = []
    for s in range(ref.shape[0]):
        got = trace["logits"][s].cpu().numpy()
        fin = np.isfinite(ref[s])
        assert np.array_equal(fin, np.isfinite(got))
        e = np.abs(got[fin] - ref[s][fin])
        errs.append((float(e.max()), float(e.mean())))
    print("fp8 teacher-forced logits: step 0", errs[0], "max over steps", max(e[0] for e in errs),
          "largest per-step mean", max(e[1] for e in errs))
    assert errs[0][0] < BF16_LOGIT_MAX and errs[0][1] < BF16_LOGIT_MEAN, errs[0]
    assert max(e[0] for e in errs) < FP8_LOGIT_MAX and max(e[1] for e in errs) < FP8_LOGIT_MEAN, errs


def test_kv_dtype_environment_variable(monkeypatch):
    c = load_gen_case("sampled_cli")
    eng = _engine(c["W"])
    monkeypatch.setenv("ZONOS_KV_DTYPE", "fp8")
    a = _gen(eng, c)
    assert eng._ws["kv"].dtype == torch.uint8
    assert _same(a, _gen(eng, c, kv_dtype="fp8"))
    with pytest.raises(ValueError, match="FP8"):                       # no bf16 kernel gets the byte caches
        eng._kv(eng._ws, 0)
    _gen(eng, c, kv_dtype="bf16")                                      # explicit beats the environment
    assert eng._ws["kv"].dtype == torch.bfloat16
    with pytest.raises(ValueError):
        _gen(eng, c, kv_dtype="fp4")


def test_fp8_unsupported_engines_raise(monkeypatch):
    from oracle import hybrid_ref as HR
    from zonos_amd.backbone import HipZonosBackbone
    from zonos_amd.hybrid import HybridDecoder, HybridEngineConfig
    h = HR.HybridCfg(d_model=256, n_layer=4, attn_layer_idx=(2,), n_heads=2, n_kv=1, d_ff=512, d_state=64, headdim=32)
    ec = HybridEngineConfig(d_model=h.d_model, n_layer=h.n_layer, attn_layer_idx=h.attn_layer_idx, n_heads=h.n_heads,
                            n_kv=h.n_kv, d_ff=h.d_ff, d_state=h.d_state, headdim=h.headdim, eps=h.eps, d_mlp=h.d_mlp,
                            rms_norm=h.rms_norm, residual_in_fp32=h.residual_in_fp32)
    eng = HybridDecoder(ec, HR.make_weights(h, seed=1), DEV)
    cond = torch.zeros(2, 4, h.d_model, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="fp8"):
        eng.generate(cond, None, 4, 2.0, 1, kv_dtype="fp8")
    monkeypatch.setenv("ZONOS_KV_DTYPE", "fp8")
    with pytest.raises(ValueError, match="fp8"):
        eng.generate(cond, None, 4, 2.0, 1)
    # head_dim != 128
    c = load_gen_case("sampled_cli")
    small = _engine(c["W"])
    small.cfg.n_heads = 4                                              # head_dim 64
    with pytest.raises(ValueError, match="head_dim"):
        _gen(small, c, kv_dtype="fp8")
    with pytest.raises(ValueError, match="bf16"):
        HipZonosBackbone.allocate_inference_cache(None, 1, 256, torch.float8_e4m3fn)
