"""GPU: the opt-in FP8 (e4m3fn) weights of the small-batch GEMVs -- the device quantiser against the host
reference (zonos_amd.wlayout), the three _w8 GEMV entries bit-equal to their bf16 counterparts on the
dequantised weights, and generate(weight_dtype="fp8").

Weights of every kernel case: rows of magnitudes 2^-10 .. 2^3 (a wrong row-to-scale mapping changes a row by
a power of two), one all-zero row, one row whose amax is exactly 448 * 2^e.
The comparisons against an fp32 / CPU product use the bounds of test_gpu_ops.test_gemv_fused unchanged. Those
bounds are absolute and were set for outputs of order 1 (bf16 ulp 2^-8 .. 2^-7); with rows up to 2^3 the
activations here are scaled by 2^-4 (for the LayerNorm cases through the LayerNorm weight and bias), an input
choice that keeps the outputs at that order.

zk_gemv_qkv_rope(_w8) takes d_model = H * 128 = 2048 only and at most 4 query heads per kv head, so its smallest
shape is H = 16, Hkv = 4 (N = 3072), not a 512-column one: both entries refuse H = 2, Hkv = 1, which is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from zonos_amd import wlayout as wl

from .golden_util import CLI_SP, TINY, load_gen_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACT = 2.0 ** -4


def _weights(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(-10, 4, (N, 1), generator=g).float()
    mag[0], mag[N - 1] = 3, -10                                  # both ends of the range in every case
    w = torch.randn(N, K, generator=g) / K ** 0.5 * torch.exp2(mag)
    w = w.to(torch.bfloat16)
    w[3] = 0
    w[5] = (torch.randn(K, generator=g) * 2.0 ** -12).to(torch.bfloat16)
    w[5, 7] = 448.0 * 2.0 ** -9                                  # amax exactly on 448 * 2^e
    w[21] = w[5] * 4                                             # ... and at another exponent, column in lane group 2
    w[21, K - 13] = -448.0 * 2.0 ** -7
    return w


def _fp8_pair(W, mode, s):
    """W bf16 [N][K] (CPU) -> (Wq CPU bf16 = the dequantised weights, bf16 packed image, byte image, scales) on
    the device; mode 1: both images of the zk_permute_fc1 order."""
    from zonos_amd._lib import call, ptr
    from zonos_amd.engine import pack_weights
    N, K = W.shape
    q, sc = wl.quantize_w_e4m3(W)
    Wq = wl.dequantize_w_e4m3(q, sc)
    Wd = Wq.to(DEV)
    if mode == 1:
        Wp = torch.empty_like(Wd)
        call("zk_permute_fc1", ptr(Wd), N // 2, K, ptr(Wp), s)
        torch.cuda.synchronize()
        Wd = Wp
        q, sc = wl.quantize_w_e4m3(Wd.cpu())                      # idempotent in value: the same rows, permuted
        assert torch.equal(wl.dequantize_w_e4m3(q, sc), Wd.cpu())
    img, scp = wl.pack_w8(q, sc)
    return Wq, pack_weights(Wd, s), img.to(DEV), scp.to(DEV)


# ---------------------------------------------------------------------------- 1. the device quantiser
@pytest.mark.parametrize("N,K", [(40, 2048), (3072, 2048), (64, 8192)])
def test_pack_weights_e4m3_equals_host_reference(N, K):
    from zonos_amd._lib import stream_ptr
    from zonos_amd.engine import pack_weights_e4m3
    W = _weights(N, K, seed=N + K)
    img, sc = pack_weights_e4m3(W.to(DEV), stream_ptr())
    torch.cuda.synchronize()
    ref_img, ref_sc = wl.pack_w8(*wl.quantize_w_e4m3(W))
    assert torch.equal(sc.cpu(), ref_sc), (sc.cpu() != ref_sc).nonzero()[:4].tolist()
    assert torch.equal(img.cpu(), ref_img), int((img.cpu() != ref_img).sum())
    q, s = wl.unpack_w8(img.cpu(), sc.cpu(), N)
    assert int(s[3]) == 127 and (q[3] == 0).all() and int(q[5, 7]) == 0x7E and int(q[21, K - 13]) == 0xFE


# ---------------------------------------------------------------------------- 2. zk_gemv_fused_w8
GEMV_CASES = [  # (M, N, K, mode, ln)
    (1, 40, 2048, 0, False), (2, 48, 8192, 2, False), (2, 2048, 4096, 2, False), (16, 72, 2048, 2, False),  # half tile
    (2, 80, 2048, 0, True), (5, 4104, 2048, 0, True), (2, 96, 2048, 1, True), (9, 160, 2048, 1, True),
    (2, 64, 4096, 1, False),                                                                                 # one tile
    (2, 8208, 2048, 1, True), (16, 8200, 2048, 0, True), (1, 8192, 8192, 0, False),                          # two tiles
    # further forms the step reaches: fc2 at B > 1 (half tile, K = 8192, 16 rows), out_proj at B > 1
    (4, 2048, 8192, 2, False), (6, 2048, 2048, 2, False), (3, 4096, 4096, 0, False),
]


@pytest.mark.parametrize("M,N,K,mode,ln", GEMV_CASES)
def test_gemv_fused_w8_bit_equal_to_bf16_on_dequantised(M, N, K, mode, ln):
    from zonos_amd._lib import call, ptr, stream_ptr
    s = stream_ptr()
    g = torch.Generator().manual_seed(M * 7 + N + mode)
    Wq, Wpk, img, scp = _fp8_pair(_weights(N, K, seed=N * 3 + K + mode), mode, s)
    x = torch.randn(M, K, generator=g) * (1.0 if ln else ACT)
    x = x.to(torch.bfloat16)
    w = ((1 + 0.1 * torch.randn(K, generator=g)) * ACT).to(torch.bfloat16)
    b = (0.1 * ACT * torch.randn(K, generator=g)).to(torch.bfloat16)
    a = F.layer_norm(x, (K,), w, b, 1e-5) if ln else x
    xd, keep = x.to(DEV), (w.to(DEV), b.to(DEV))
    lw, lb = (ptr(keep[0]), ptr(keep[1])) if ln else (None, None)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)

    def run(w8, skipw=None):
        Wargs = (ptr(img), ptr(scp)) if w8 else (ptr(Wpk),)
        name = "zk_gemv_fused_w8" if w8 else "zk_gemv_fused"
        if mode == 0:
            out = torch.full((M, N), 7.0, device=DEV)
            call(name, ptr(xd), K, *Wargs, M, N, K, 0, lw, lb, 1e-5, ptr(out), None, skipw, s)
        elif mode == 1:
            out = torch.full((M, N // 2), 7.0, dtype=torch.bfloat16, device=DEV)
            call(name, ptr(xd), K, *Wargs, M, N, K, 1, lw, lb, 1e-5, None, ptr(out), skipw, s)
        else:
            out = res.to(DEV)
            call(name, ptr(xd), K, *Wargs, M, N, K, 2, None, None, 1e-5, None, ptr(out), skipw, s)
        torch.cuda.synchronize()
        return out

    ref, out = run(False), run(True)
    bits = torch.int32 if mode == 0 else torch.int16
    assert torch.equal(ref.view(bits), out.view(bits)), \
        (int((ref.view(bits) != out.view(bits)).sum()), (ref.float() - out.float()).abs().max().item())
    # not only kernel against kernel: the product of the dequantised weights, test_gemv_fused's bounds
    o = out.float().cpu()
    if mode == 0:
        want = a.float() @ Wq.float().t()
        assert torch.allclose(o, want, atol=2e-2 if ln else 3e-3, rtol=1e-2), (o - want).abs().max()
        assert (o[:, 3] == 0).all() and o.abs().max() > 0.1 * ACT
    elif mode == 1:
        ry, rg = F.linear(a, Wq).chunk(2, dim=-1)
        err = (o - (ry * F.silu(rg)).float()).abs()
        assert err.max() < 0.06 and (err > 0).float().mean() < 0.06, err.max()
    else:
        err = (o - (res + F.linear(x, Wq)).float()).abs()
        assert err.max() < 0.07 and (err > 0).float().mean() < 0.05, err.max()
        assert torch.equal(o[:, 3], res[:, 3].float())
    # the skip word set: the output keeps its fill
    kept = run(True, ptr(skip))
    fill = res.to(DEV) if mode == 2 else torch.full_like(kept, 7.0)
    assert torch.equal(kept.view(bits), fill.view(bits)), "a skipped launch wrote"


# ---------------------------------------------------------------------------- 3. zk_gemv_qkv_rope_w8
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("pos", [0, 37, 63])
def test_gemv_qkv_rope_w8_bit_equal(M, pos):
    from zonos_amd._lib import ZonosHipError, call, ptr, stream_ptr
    from zonos_amd.engine import rope_table
    H, Hk, hd, D, smax = 16, 4, 128, 2048, 64
    N = (H + 2 * Hk) * hd
    s = stream_ptr()
    g = torch.Generator().manual_seed(pos * 3 + M)
    Wq, Wpk, img, scp = _fp8_pair(_weights(N, D, seed=11), 0, s)
    x = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
    lw = ((1 + 0.1 * torch.randn(D, generator=g)) * ACT).to(torch.bfloat16).to(DEV)
    lb = (0.1 * ACT * torch.randn(D, generator=g)).to(torch.bfloat16).to(DEV)
    freqs = rope_table(16384, hd).to(DEV)
    kc0 = torch.randn(M * Hk * smax * hd, generator=g).to(torch.bfloat16).to(DEV)
    vt0 = torch.randn(M * Hk * smax * hd, generator=g).to(torch.bfloat16).to(DEV)
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)

    def run(w8, skipw=None):
        q = torch.full((M, H * hd), 7.0, dtype=torch.bfloat16, device=DEV)
        kc, vt = kc0.clone(), vt0.clone()
        Wargs = (ptr(img), ptr(scp)) if w8 else (ptr(Wpk),)
        call("zk_gemv_qkv_rope_w8" if w8 else "zk_gemv_qkv_rope", ptr(x), *Wargs, M, H, Hk, hd, ptr(lw), ptr(lb), 1e-5,
             ptr(q), ptr(kc), ptr(vt), smax, ptr(posd), ptr(freqs), skipw, s)
        torch.cuda.synchronize()
        return q, kc, vt

    (q1, kc1, vt1), (q2, kc2, vt2) = run(False), run(True)
    assert torch.equal(q1.view(torch.int16), q2.view(torch.int16))
    assert torch.equal(kc1.view(torch.int16), kc2.view(torch.int16)) and torch.equal(vt1.view(torch.int16), vt2.view(torch.int16))
    # the new key / value were written, every other cache position is untouched
    from zonos_amd.kvlayout import unpack_k, unpack_v
    for new, old, unpack in ((kc2, kc0, unpack_k), (vt2, vt0, unpack_v)):
        a, b = (unpack(t.cpu().view(M, Hk, -1), smax).view(torch.int16) for t in (new, old))
        diff = (a != b).any(-1)                                   # [M][Hk][smax]
        assert diff[:, :, pos].all() and int(diff.sum()) == M * Hk, diff.nonzero()[:4].tolist()
    q3, kc3, vt3 = run(True, ptr(torch.ones(1, dtype=torch.int32, device=DEV)))
    assert torch.equal(kc3, kc0) and torch.equal(vt3, vt0) and (q3 == 7.0).all(), "a skipped launch wrote"
    if M == 2 and pos == 0:          # the 512-column shape (H = 2, Hkv = 1) is no shape of either entry
        for name, Wargs in (("zk_gemv_qkv_rope", (ptr(Wpk),)), ("zk_gemv_qkv_rope_w8", (ptr(img), ptr(scp)))):
            with pytest.raises(ZonosHipError, match="d_model"):
                call(name, ptr(x), *Wargs, M, 2, 1, hd, ptr(lw), ptr(lb), 1e-5, ptr(q3), ptr(kc3), ptr(vt3), smax,
                     ptr(posd), ptr(freqs), None, s)


# ---------------------------------------------------------------------------- 4. zk_gemv_attn_out_w8
@pytest.mark.parametrize("Hkv", [4, 16])
@pytest.mark.parametrize("nsplit", [2, 4, 8, 16])
@pytest.mark.parametrize("N", [48, 2048])
def test_gemv_attn_out_w8_bit_equal(Hkv, nsplit, N):
    from zonos_amd._lib import call, ptr, stream_ptr
    K, hd = 2048, 128
    s = stream_ptr()
    g = torch.Generator().manual_seed(Hkv * 31 + nsplit * 5 + N)
    Wq, Wpk, img, scp = _fp8_pair(_weights(N, K, seed=N + Hkv), 2, s)
    G = (K // hd) // Hkv
    for M in (1, 2):
        # partials [M][Hkv][nsplit][m 4 | l 4 | O 4 x 128] (heads >= G unused); one split saw no key: m = -inf
        wk = torch.zeros(M, Hkv, nsplit, 8 + 4 * hd)
        wk[..., :4] = torch.randn(M, Hkv, nsplit, 4, generator=g) * 3
        wk[..., 4:8] = torch.rand(M, Hkv, nsplit, 4, generator=g) * 20 + 1
        wk[..., 8:] = torch.randn(M, Hkv, nsplit, 4 * hd, generator=g) * 4 * ACT
        dead = nsplit - 1 if M == 1 else 0
        wk[:, :, dead, :4] = -float("inf")
        wk[:, :, dead, 4:] = 0
        work = wk.to(DEV)
        x0 = torch.randn(M, N, generator=g).to(torch.bfloat16)
        x1, x2, x3 = x0.to(DEV), x0.to(DEV), x0.to(DEV)
        call("zk_gemv_attn_out", ptr(work), nsplit, Hkv, ptr(Wpk), M, N, K, ptr(x1), None, s)
        call("zk_gemv_attn_out_w8", ptr(work), nsplit, Hkv, ptr(img), ptr(scp), M, N, K, ptr(x2), None, s)
        call("zk_gemv_attn_out_w8", ptr(work), nsplit, Hkv, ptr(img), ptr(scp), M, N, K, ptr(x3),
             ptr(torch.ones(1, dtype=torch.int32, device=DEV)), s)
        torch.cuda.synchronize()
        assert torch.equal(x1.view(torch.int16), x2.view(torch.int16)), (x1.float() - x2.float()).abs().max().item()
        assert torch.equal(x3.cpu(), x0), "a skipped launch wrote"
        # the merge + projection in fp32 (k_attn_combine's formula), the residual bound of test_gemv_fused
        m, l = wk[..., :G], wk[..., 4:4 + G]
        o = wk[..., 8:].view(M, Hkv, nsplit, 4, hd)[..., :G, :]
        c = torch.where(m == -float("inf"), torch.zeros_like(m), torch.exp(m - m.max(dim=2, keepdim=True).values))
        att = ((o * c[..., None]).sum(2) / (l * c).sum(2)[..., None]).reshape(M, K).to(torch.bfloat16)
        err = (x2.float().cpu() - (x0 + F.linear(att, Wq)).float()).abs()
        assert err.max() < 0.07 and (err > 0).float().mean() < 0.05, err.max()
        assert not torch.equal(x2.cpu(), x0)


# ---------------------------------------------------------------------------- 5. the engine
CFG = dict(d_model=2048, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
LC, NEW = 8, 24
LINEAR = ("mixer.in_proj.weight", "mixer.out_proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")


@pytest.fixture(scope="module")
def weights():
    from zonos_amd.synthetic import backbone_weights
    W0 = backbone_weights(DEV, seed=4, **CFG)
    Wr = dict(W0)                                                 # FP8-representable: dequantize(quantize(W0))
    for k, v in W0.items():
        if k.endswith(LINEAR):
            Wr[k] = wl.dequantize_w_e4m3(*wl.quantize_w_e4m3(v.cpu())).to(DEV)
    return dict(generic=W0, representable=Wr)


def _engine(W):
    from zonos_amd.engine import EngineConfig, HipDecoder
    return HipDecoder(EngineConfig(**CFG), W, DEV)


def _gen(eng, B, **kw):
    from zonos_amd.synthetic import conditioning
    cond = conditioning(B, LC, CFG["d_model"], seed=B, device=DEV)
    out = eng.generate(cond, None, NEW, 2.0, B, CLI_SP, seed=9, force_full_length=True, **kw)
    return [o.clone() for o in out], eng.last_logits().clone()


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("B", [1, 3])
def test_engine_fp8_weights_bit_equal_on_representable_weights(B, weights, monkeypatch):
    """(a) and (c): on weights the format represents exactly the FP8 engine is the bf16 engine bit for bit, issued
    by zk_decode_step (graph and eager) and by the Python sequence; bf16 -> fp8 -> bf16 on one engine re-keys."""
    from zonos_amd.engine import HipDecoder
    eng = _engine(weights["representable"])
    base = _gen(eng, B)
    assert "w_fp8" not in eng._ws and "wqkv8" not in eng.layers[0]
    graph = _gen(eng, B, weight_dtype="fp8", poll_every=7)
    ws = eng._ws
    assert ws["w_fp8"] and ws["key"][-1] == "w8" and eng.layers[1]["fc28"].dtype == torch.uint8
    d = eng._step_desc(ws, B, *ws["_keep"])
    assert d.w_fp8 == 1 and d.small == 1 and all(getattr(ws["step_layers"][i], n) for i in range(2)
                                                  for n in ("wqkv8", "wo8", "fc18", "fc28", "fc2_scale"))
    assert _same(base, graph)
    assert _same(base, _gen(eng, B, weight_dtype="fp8", use_graph=False, poll_every=1))
    monkeypatch.setattr(HipDecoder, "c_step", False)
    assert _same(base, _gen(eng, B, weight_dtype="fp8"))             # the Python launch sequence
    monkeypatch.setattr(HipDecoder, "c_step", True)
    again = _gen(eng, B, weight_dtype="bf16")                        # re-keyed, re-captured
    assert "w_fp8" not in eng._ws and _same(base, again)


def test_engine_fp8_weights_generic_weights_ran_and_logged(weights):
    """(b): generic weights, teacher-forced on the bf16 run's frames. No bound: there is no trained checkpoint."""
    from zonos_amd._lib import SamplingParams
    B = 1
    eng = _engine(weights["generic"])
    torch.cuda.reset_peak_memory_stats()
    t16 = {}
    _gen(eng, B, trace=t16)
    mem16 = torch.cuda.max_memory_allocated()
    gold = t16["delayed"]

    def force(frame, step):
        if frame.shape[2]:
            frame.copy_(gold[..., 1 + step:2 + step])
        return True

    t8 = {}
    _gen(eng, B, trace=t8, weight_dtype="fp8", callback=lambda f, s, n: force(f, s), _after_prefill=lambda f: force(f, 0))
    mem8 = torch.cuda.max_memory_allocated()
    ws = eng._ws
    d = eng._step_desc(ws, B, eng._gen_state(ws, B, 9, 0), SamplingParams())
    assert d.w_fp8 == 1 and ws["step_layers"][0].wqkv8 and ws["step_layers"][1].fc2_scale
    n = min(len(t16["logits"]), len(t8["logits"]))
    assert n > NEW // 2
    a = torch.stack(t16["logits"][:n]).float().cpu().numpy()
    b = torch.stack(t8["logits"][:n]).float().cpu().numpy()
    assert a.shape == b.shape and np.array_equal(a[0], b[0]), "the prefill uses the bf16 weights: step 0 is exact"
    fin = np.isfinite(a) & np.isfinite(b)
    diff = np.abs(a[fin] - b[fin])
    assert diff.max() > 0, "the FP8 path did not run"
    am = (a.argmax(-1) == b.argmax(-1)).mean()
    print(f"fp8 weights, generic random weights, {a.shape[0]} teacher-forced steps: logit |d| max {diff.max():.4f} "
          f"mean {diff.mean():.5f}, equal argmax {am:.4f}; max_memory_allocated bf16 {mem16 / 2**20:.1f} MiB, "
          f"after the fp8 run {mem8 / 2**20:.1f} MiB")


def test_weight_dtype_environment_variable(weights, monkeypatch):
    """(d)"""
    eng = _engine(weights["generic"])
    explicit = _gen(eng, 1, weight_dtype="fp8")
    monkeypatch.setenv("ZONOS_WEIGHT_DTYPE", "fp8")
    assert _same(explicit, _gen(eng, 1)) and eng._ws["w_fp8"]
    bf = _gen(eng, 1, weight_dtype="bf16")                            # explicit beats the environment
    assert "w_fp8" not in eng._ws and not torch.equal(bf[1], explicit[1])
    with pytest.raises(ValueError):
        _gen(eng, 1, weight_dtype="fp4")


def test_weight_dtype_unsupported_raises_before_allocation(weights, monkeypatch):
    """(e)"""
    from oracle import hybrid_ref as HR
    from zonos_amd.backbone import HipHybridBackbone, HipZonosBackbone
    from zonos_amd.engine import EngineConfig, HipDecoder
    from zonos_amd.hybrid import HybridDecoder, HybridEngineConfig
    eng = _engine(weights["generic"])
    cond = torch.zeros(18, 4, 2048, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="batch_size <= 8"):
        eng.generate(cond, None, 4, 2.0, 9, weight_dtype="fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        eng.generate(cond[:2], None, 4, 2.0, 1, weight_dtype="fp8", kv_dtype="fp8")
    assert eng._ws is None, "a refusal allocated a workspace"
    c = load_gen_case("sampled_cli")                                  # d_model != 2048
    tiny = HipDecoder(EngineConfig(d_model=TINY.d_model, n_layer=TINY.n_layer, n_heads=TINY.n_heads, n_kv=TINY.n_kv,
                                   d_ff=TINY.d_ff, eps=TINY.eps), c["W"], DEV)
    with pytest.raises(ValueError, match="d_model 2048"):
        tiny.generate(c["cond"].cuda(), c["prefix"].cuda(), 4, 2.0, c["B"], c["sp"], weight_dtype="fp8")
    h = HR.HybridCfg(d_model=256, n_layer=4, attn_layer_idx=(2,), n_heads=2, n_kv=1, d_ff=512, d_state=64, headdim=32)
    ec = HybridEngineConfig(d_model=h.d_model, n_layer=h.n_layer, attn_layer_idx=h.attn_layer_idx, n_heads=h.n_heads,
                            n_kv=h.n_kv, d_ff=h.d_ff, d_state=h.d_state, headdim=h.headdim, eps=h.eps, d_mlp=h.d_mlp,
                            rms_norm=h.rms_norm, residual_in_fp32=h.residual_in_fp32)
    hyb = HybridDecoder(ec, HR.make_weights(h, seed=1), DEV)
    hc = torch.zeros(2, 4, h.d_model, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="weight_dtype"):
        hyb.generate(hc, None, 4, 2.0, 1, weight_dtype="fp8")
    monkeypatch.setenv("ZONOS_WEIGHT_DTYPE", "fp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        hyb.generate(hc, None, 4, 2.0, 1)
    for plugin in (HipZonosBackbone, HipHybridBackbone):
        with pytest.raises(ValueError, match="plugin"):
            plugin.allocate_inference_cache(plugin.__new__(plugin), 2, 64, weight_dtype="fp8")
