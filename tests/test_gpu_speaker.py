"""GPU: the speaker-embedding kernels (csrc/speaker.hip) and the host path on them.

Bars. The conv is compared with fp64 conv2d on the same fp16-rounded operands: every product is exact
in fp32, so what remains is the fp32 accumulation of K = taps * Cin terms, bounded for any summation
order by K * 2^-24 * sum |x_i w_i| (plus the two roundings of the BatchNorm epilogue). The network
tests use the fixtures' own measure: the relative RMS error of the fp16-operand emulation of the
reference, stored beside every tensor; the GPU may take twice that (summation order, exp / sigmoid).
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import speaker_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24
DEV = "cuda"


def _L():
    from zonos_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- conv
# The last case (380 tiles x 2 clips = 760 workgroups) runs the 64-channel-tile form of the kernel, the others
# (under 512 workgroups) the 32-channel-tile form; T = 37 / 5 / 10 leave partial tiles on both axes.
CONV_CASES = [(32, 32, 80, 37, 3, 1), (32, 64, 80, 37, 3, 2), (32, 64, 80, 37, 1, 2), (128, 256, 20, 10, 3, 2),
              (64, 64, 80, 5, 3, 1), (64, 64, 80, 300, 3, 1)]


@pytest.mark.parametrize("Cin,Cout,Fi,Ti,ks,stride", CONV_CASES)
def test_conv2d_cl_vs_torch(Cin, Cout, Fi, Ti, ks, stride):
    from zonos_amd.speaker import out_dim, pack_conv_weight
    L = _L()
    g = _gen(Cin + Cout + Fi + Ti + ks + stride)
    B = 2
    K = ks * ks * Cin
    x = torch.randn(B, Cin, Fi, Ti, generator=g).half()
    w = (torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(K)).half()
    scale = 0.8 + 0.4 * torch.rand(Cout, generator=g)
    shift = 0.1 * torch.randn(Cout, generator=g)
    Fo, To = out_dim(Fi, stride), out_dim(Ti, stride)
    conv = F.conv2d(x.double(), w.double(), stride=stride, padding=ks // 2)
    assert conv.shape == (B, Cout, Fo, To)
    mag = F.conv2d(x.double().abs(), w.double().abs(), stride=stride, padding=ks // 2)
    sc, sh = scale.double()[None, :, None, None], shift.double()[None, :, None, None]
    ref = conv * sc + sh
    bar = (K + 4) * U32 * (mag * sc.abs() + sh.abs())

    xs = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wp = pack_conv_weight(w.float()).to(DEV)
    scale_d, shift_d = scale.to(DEV), shift.to(DEV)
    ntile = L.load().zk_spk_conv_tiles(Fo, To)
    if Ti == 300:
        assert ntile > 1 and L.load().zk_spk_conv_tiles(Fo, To) == 20 * 19
    out_x = torch.full((B, Fo, To, Cout), float("nan"), device=DEV)
    out_s = torch.zeros(B, Fo, To, Cout, device=DEV, dtype=torch.float16)
    stats = torch.full((B, ntile, 3, Cout), float("nan"), device=DEV)
    st = L.stream_ptr(torch.device(DEV))
    L.call("zk_spk_conv2d_cl", L.ptr(xs), B, Cin, Fi, Ti, L.ptr(wp), Cout, ks, stride, L.ptr(scale_d), L.ptr(shift_d),
           0, L.ptr(out_s), L.ptr(out_x), L.ptr(stats), st)
    relu_s = torch.zeros_like(out_s)
    L.call("zk_spk_conv2d_cl", L.ptr(xs), B, Cin, Fi, Ti, L.ptr(wp), Cout, ks, stride, L.ptr(scale_d), L.ptr(shift_d),
           1, L.ptr(relu_s), None, None, st)
    torch.cuda.synchronize()
    got = out_x.cpu().permute(0, 3, 1, 2).double()
    err = (got - ref).abs()
    print(f"conv {Cin}->{Cout} {Fi}x{Ti} k{ks} s{stride}: max err {float(err.max()):.3e}, "
          f"max err / bar {float((err / bar).max()):.3f}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bar).all())
    half_bar = bar + 2.0 ** -11 * ref.abs() + 6e-8
    assert bool(((out_s.cpu().permute(0, 3, 1, 2).double() - ref).abs() <= half_bar).all())
    assert bool(((relu_s.cpu().permute(0, 3, 1, 2).double() - ref.clamp(min=0)).abs() <= half_bar).all())
    # the tile partials add up to each (clip, channel)'s count, mean and sum of squared deviations
    s = stats.cpu().double()
    n = s[:, :, 0].sum(1)
    assert bool((n == Fo * To).all())
    mean = (s[:, :, 0] * s[:, :, 1]).sum(1) / n
    m2 = (s[:, :, 2] + s[:, :, 0] * (s[:, :, 1] - mean[:, None]) ** 2).sum(1)
    rm = ref.mean(dim=(2, 3))
    rm2 = (ref - rm[:, :, None, None]).pow(2).sum(dim=(2, 3))
    assert torch.allclose(mean, rm, rtol=0, atol=float(bar.max()) + 4 * U32)
    assert torch.allclose(m2, rm2, rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------- SimAM
def _tile_stats(y, tf=4, tt=16):
    """(count, mean, M2) per 4 x 16 tile of y [B][C][F][T], as the conv writes them: [B][tiles][3][C]."""
    B, C_, F_, T_ = y.shape
    out = []
    for f0 in range(0, F_, tf):
        for t0 in range(0, T_, tt):
            blk = y[:, :, f0:f0 + tf, t0:t0 + tt].double().reshape(B, C_, -1)
            m = blk.mean(2)
            out.append(torch.stack([torch.full_like(m, blk.shape[2]), m, (blk - m[:, :, None]).pow(2).sum(2)], 1))
    return torch.stack(out, 1).float()


@pytest.mark.parametrize("own_shortcut", [False, True])
def test_simam_vs_formula(own_shortcut):
    L = _L()
    g = _gen(7)
    B, C_, F_, T_ = 2, 64, 20, 37
    y = torch.randn(B, C_, F_, T_, generator=g) * (0.5 + torch.rand(1, C_, 1, 1, generator=g))
    y = y + torch.randn(1, C_, 1, 1, generator=g)
    y[:, 0] = 100.0 + 1e-3 * torch.randn(B, F_, T_, generator=g)      # large mean, tiny variance: cancellation
    y[:, 1] = 0.25                                                     # constant channel: v = 0
    sc = torch.randn(B, C_, F_, T_, generator=g)
    ref = speaker_ref.simam_block_tail(y.double(), sc.double())
    # error model: mu within 8 fp32 roundings (the merges on the longest path of the tile reduction) of the
    # larger of |mu| and the spread, v within 64 ulps (+ mu's share), then z = d^2 / (4 (v + l)) and
    # sigmoid' <= 1/4; everything else a few fp32 roundings of the terms
    yd = y.double()
    mu = yd.mean(dim=(2, 3), keepdim=True)
    d = yd - mu
    v = d.pow(2).sum(dim=(2, 3), keepdim=True) / (F_ * T_ - 1)
    inv = 1.0 / (4 * (v + 1e-4))
    dmu = 8 * U32 * (mu.abs() + v.sqrt())
    dz = inv * (2 * d.abs() * dmu + dmu ** 2) + d.pow(2) * inv * (64 * U32 + dmu ** 2 / (v + 1e-4)) + 8 * U32 * (d.pow(2) * inv + 0.5)
    bar = yd.abs() * 0.25 * dz + 16 * U32 * (yd.abs() + sc.abs().double())

    cl = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
    y_d, stats = cl(y), _tile_stats(y).contiguous().to(DEV)
    assert stats.shape[1] == L.load().zk_spk_conv_tiles(F_, T_)
    outs = []
    for _ in range(2):
        x_buf = cl(sc)
        x_out = torch.empty_like(x_buf) if own_shortcut else x_buf       # in place over the shortcut, as a block does
        s_out = torch.empty(B, F_, T_, C_, device=DEV, dtype=torch.float16)
        moments = torch.empty(B, 2, C_, device=DEV)
        L.call("zk_spk_simam", L.ptr(y_d), B, C_, F_, T_, L.ptr(stats), L.ptr(x_buf), L.ptr(moments), L.ptr(x_out),
               L.ptr(s_out), L.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        outs.append((x_out.cpu(), s_out.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    got = outs[0][0].permute(0, 3, 1, 2).double()
    err = (got - ref).abs()
    print(f"simam: max err {float(err.max()):.3e}; cancellation channel {float(err[:, 0].max()):.3e} "
          f"(bar {float(bar[:, 0].max()):.3e}); max err / bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all())
    assert torch.equal(outs[0][1], outs[0][0].half())
    assert bool((got >= 0).all())


# ---------------------------------------------------------------- log-mel
def _signal(B, n, seed):
    g = _gen(seed)
    t = torch.arange(n) / 16000.0
    x = 0.3 * torch.sin(2 * math.pi * 220.0 * t)[None] + 0.1 * torch.sin(2 * math.pi * 3100.0 * t)[None]
    return (x + 0.05 * torch.randn(B, n, generator=g)).float()


@pytest.mark.parametrize("n", [5931, 400])
def test_logfbank_vs_restatement(n):
    from zonos_amd.speaker import logFbankCal
    wav = _signal(2, n, n)
    ref64 = speaker_ref.log_fbank(wav, torch.float64)
    ref32 = speaker_ref.log_fbank(wav, torch.float32)
    e32 = float((ref32.double() - ref64).abs().max())
    got = logFbankCal(DEV)(wav.to(DEV))
    torch.cuda.synchronize()
    assert got.shape == (2, 80, 1 + n // 160) and got.dtype == torch.float32
    err = float((got.cpu().double() - ref64).abs().max())
    print(f"logfbank n={n}: fp32 restatement vs fp64 {e32:.3e}; kernel vs fp64 {err:.3e} (bar {4 * e32:.3e})")
    assert e32 > 0
    assert err <= 4 * e32
    assert float(got.mean(dim=2).abs().max()) < 1e-5


# ---------------------------------------------------------------- the network against the fixtures
_CACHE = {}


def _fixture(name):
    """(fixture, SpeakerNet on the GPU) with the weights regenerated and checked against the stored hash."""
    if name not in _CACHE:
        from zonos_amd.speaker import SpeakerNet
        from zonos_amd.synthetic import speaker_state_dict, state_dict_sha256
        z = np.load(os.path.join(GOLDEN, f"speaker_{name}.npz"))
        sd, lda = speaker_state_dict(int(z["in_planes"]), [int(b) for b in z["blocks"]], int(z["seed"]))
        assert state_dict_sha256(sd) == str(z["wsum"]) and state_dict_sha256(lda) == str(z["lda_wsum"])
        _CACHE[name] = (z, SpeakerNet(sd, lda, DEV), sd, lda)
    return _CACHE[name]


def _rel_rms(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def _check_stage(z, key, got):
    ref = torch.from_numpy(z[key])
    if ref.ndim == 4:
        got = got.permute(0, 3, 1, 2)[:, ::int(z[key + "_cs"])]       # [B][F][T][C] -> the stored [B][C::cs][F][T]
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    e, emu = _rel_rms(got.cpu(), ref), float(z[key + "_err"])
    print(f"{key:10s} rel rms err {e:.3e}  emulation {emu:.3e}  bar {2 * emu:.3e}")
    return e <= 2 * emu, f"{key}: {e:.3e} > 2 x {emu:.3e}"


def test_tiny_network_stages_vs_reference():
    z, net, _, _ = _fixture("tiny")
    embs, failures = {}, []
    for clip in "ab":
        stages = {}
        emb, lda = net.forward_features(torch.from_numpy(z[f"{clip}_feat"]).to(DEV), stages)
        torch.cuda.synchronize()
        stages.update(emb=emb, lda=lda)
        for k in ("stem", "layer1", "layer2", "layer3", "layer4", "pooled", "emb", "lda"):
            ok, msg = _check_stage(z, f"{clip}_{k}", stages[k])
            if not ok:
                failures.append(msg)
        embs[clip] = emb.cpu().double()
    assert not failures, failures
    ra, rb = torch.from_numpy(z["a_emb"]).double(), torch.from_numpy(z["b_emb"]).double()
    dist = float((ra - rb).norm())
    for got, ref in ((embs["a"], ra), (embs["b"], rb)):
        sep = float((got - ref).norm()) / dist
        print(f"embedding error / distance between the clips: {sep:.4f}")
        assert sep <= 0.1
    # clip b is one frame wide after the strides: sg = sqrt(clamp(0, 1e-5))
    zb = np.load(os.path.join(GOLDEN, "speaker_tiny.npz"))["b_pooled"]
    assert np.allclose(zb[0, zb.shape[1] // 2:], math.sqrt(1e-5), rtol=1e-3)


def test_full_depth_network_vs_reference():
    z, net, _, _ = _fixture("full")
    assert (net.in_planes, net.blocks_per_layer) == (64, [10, 20, 64, 3]) and len(net.blocks) == 97
    stages = {}
    emb, lda = net.forward_features(torch.from_numpy(z["feat"]).to(DEV), stages)
    torch.cuda.synchronize()
    stages.update(emb=emb, lda=lda)
    failures = []
    for k in ("layer4", "emb", "lda"):
        ok, msg = _check_stage(z, k, stages[k])
        if not ok:
            failures.append(msg)
    assert not failures, failures
    ref = torch.from_numpy(z["emb"]).double()
    dist = float((ref[0] - ref[1]).norm())
    for b in range(2):
        sep = float((emb[b].cpu().double() - ref[b]).norm()) / dist
        print(f"embedding error / distance between the clips: {sep:.4f}")
        assert sep <= 0.1


def test_c_entry_batching_and_repeat_are_bit_identical():
    _, net, _, _ = _fixture("tiny")
    wav = _signal(2, 5931, 3).to(DEV)
    e_c, l_c = net.embed(wav, c_step=True)
    e_py, l_py = net.embed(wav, c_step=False)
    e_c2, l_c2 = (t.clone() for t in net.embed(wav, c_step=True))
    torch.cuda.synchronize()
    assert e_c.shape == (2, 256) and l_c.shape == (2, 128) and bool(torch.isfinite(l_c).all())
    assert torch.equal(e_c, e_py) and torch.equal(l_c, l_py)
    assert torch.equal(e_c, e_c2) and torch.equal(l_c, l_c2)
    for b in range(2):
        e1, l1 = net.embed(wav[b:b + 1], c_step=True)
        assert torch.equal(e1[0], e_c[b]) and torch.equal(l1[0], l_c[b])
    assert float((e_c[0] - e_c[1]).norm()) > 0


def test_make_speaker_embedding_end_to_end(tmp_path, monkeypatch):
    """Zonos.make_speaker_embedding on a stereo 22.05 kHz clip with the two checkpoint files found through
    ZONOS_SPEAKER_PATH, then make_cond_dict(speaker=...) -> prepare_conditioning."""
    from oracle import cond_ref, zonos_ref
    from zonos_amd import conditioning as zc
    from zonos_amd.config import BackboneConfig, PrefixConditionerConfig, ZonosConfig
    from zonos_amd.model import Zonos
    from zonos_amd.speaker import SPEAKER_CKPT, SPEAKER_LDA, SpeakerEmbeddingLDA

    from .golden_util import TINY
    _, _, sd, lda = _fixture("tiny")
    torch.save(sd, tmp_path / SPEAKER_CKPT)
    torch.save(lda, tmp_path / SPEAKER_LDA)
    monkeypatch.setenv("ZONOS_SPEAKER_PATH", str(tmp_path))

    conds = [dict(c) for c in cond_ref.TRANSFORMER_CONDITIONERS]
    bc = BackboneConfig(d_model=TINY.d_model, n_layer=TINY.n_layer, attn_mlp_d_intermediate=TINY.d_ff,
                        attn_cfg={"num_heads": TINY.n_heads, "num_heads_kv": TINY.n_kv}, norm_epsilon=TINY.eps)
    cfg = ZonosConfig(bc, PrefixConditionerConfig(conds, "none"))
    msd = dict(zonos_ref.make_weights(TINY, seed=0, head_scale=4.0))
    Wc = cond_ref.make_weights(conds, TINY.d_model, "none", seed=1)
    msd.update({"prefix_conditioner." + k: v for k, v in Wc.items()})
    model = Zonos(cfg, msd, DEV)

    n = 22050 // 2
    wav = torch.stack([_signal(1, n, 5)[0], _signal(1, n, 6)[0]])            # [2 channels][n] at 22.05 kHz
    spk = model.make_speaker_embedding(wav, 22050)
    assert spk.shape == (1, 1, 128) and spk.dtype == torch.bfloat16 and bool(torch.isfinite(spk.float()).all())
    assert model.spk_clone_model is not None
    emb, lda_out = SpeakerEmbeddingLDA(device=DEV)(wav, 22050)
    assert emb.shape == (1, 256) and lda_out.shape == (1, 128) and emb.dtype == torch.float32
    assert torch.equal(spk, lda_out.unsqueeze(0).bfloat16())
    mono = SpeakerEmbeddingLDA(device=DEV)(wav.mean(0), 22050)[1]             # a 1-D wav is the channel mean's equal
    assert torch.equal(mono, lda_out)
    zc.set_phonemizer(lambda texts, langs: ["həlˈoʊ wˈɜːld!" for _ in texts])
    try:
        cd = zc.make_cond_dict(text="Hello, world!", speaker=spk, language="en-us", device=DEV)
        cond = model.prepare_conditioning(cd)
    finally:
        zc.set_phonemizer(None)
    assert cond.shape[0] == 2 and cond.shape[2] == TINY.d_model and cond.dtype == torch.bfloat16
    assert bool(torch.isfinite(cond.float()).all())
