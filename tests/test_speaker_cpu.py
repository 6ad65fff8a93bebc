"""CPU: the speaker-embedding feature's host side -- exported symbols and struct layouts, descriptor
validation before any launch, the weight loader (geometry inference, BatchNorm folding into scale /
shift, conv packing, pooling permutation), the restated mel filterbank, checkpoint lookup, the shim."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import speaker_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zk_spk_logfbank", "zk_spk_stem", "zk_spk_conv2d_cl", "zk_spk_conv_tiles", "zk_spk_simam",
               "zk_spk_asp", "zk_spk_head", "zk_speaker_workspace_bytes", "zk_speaker_embed"]
TINY = (32, [2, 2, 2, 1])
FULL = (64, [10, 20, 64, 3])


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_in_header_binding_and_library(lib):
    from zonos_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zonos_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", header))
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} missing from zonos_hip.h"
        assert s in _lib.exported_symbols(), f"{s} missing from the ctypes binding"
        assert hasattr(lib, s), f"{s} not exported by the library"
    from zonos_amd import build
    assert "speaker.hip" in build.SOURCES


def test_struct_layout_matches_compiler(lib):
    from zonos_amd._lib import SpkBlock, SpkDesc
    assert lib.zk_abi_size(26) == C.sizeof(SpkBlock)
    assert lib.zk_abi_size(27) == C.sizeof(SpkDesc)
    assert lib.zk_abi_size(28) == SpkBlock.wd.offset
    assert lib.zk_abi_size(29) == SpkDesc.blocks.offset
    assert lib.zk_abi_size(30) == SpkDesc.lda_b.offset


def _fake_desc(c0=64, nblocks=2, cout=(64, 128), stride=(1, 2), n_mels=80, pool_dim=None):
    """A descriptor with non-null dummy pointers: validation must reject it before anything is read."""
    from zonos_amd._lib import SpkBlock, SpkDesc
    arr = (SpkBlock * nblocks)()
    cin, rows = c0, n_mels
    for i in range(nblocks):
        arr[i].cin, arr[i].cout, arr[i].stride = cin, cout[i], stride[i]
        for n in ("w1", "scale1", "shift1", "w2", "scale2", "shift2"):
            setattr(arr[i], n, 0x1000)
        if stride[i] != 1 or cin != cout[i]:
            arr[i].wd = arr[i].scaled = arr[i].shiftd = 0x1000
        cin, rows = cout[i], (rows - 1) // stride[i] + 1
    d = SpkDesc(n_mels=n_mels, c0=c0, nblocks=nblocks, pool_dim=cin * rows if pool_dim is None else pool_dim,
                att_dim=128, emb_dim=256, lda_dim=128)
    d.blocks = C.cast(arr, C.c_void_p)
    for n in ("window", "twiddle", "melfb", "stem_w", "stem_scale", "stem_shift", "asp_w1", "asp_b1", "asp_bn_scale",
              "asp_bn_shift", "asp_w2", "asp_b2", "bott_w", "bott_b", "lda_w", "lda_b"):
        setattr(d, n, 0x1000)
    return d, arr


def _embed_rc(lib, d, n=16000, ws_bytes=1 << 40):
    return lib.zk_speaker_embed(C.byref(d), 0x1000, 1, n, 0x1000, ws_bytes, 0x1000, 0x1000, None)


def test_embed_rejects_bad_descriptors_before_any_launch(lib):
    good, keep = _fake_desc()
    need = lib.zk_speaker_workspace_bytes(C.byref(good), 1, 16000)
    assert need > 0
    # every case below returns on the host: no GPU exists here, and the pointers are dummies
    assert _embed_rc(lib, good, ws_bytes=need - 1) != 0
    assert b"workspace" in lib.zk_last_error()
    d, keep2 = _fake_desc(c0=48, cout=(48, 96))
    assert _embed_rc(lib, d) != 0 and b"multiples of 32" in lib.zk_last_error()
    d, keep3 = _fake_desc(cout=(64, 100))
    assert _embed_rc(lib, d) != 0 and b"multiples of 32" in lib.zk_last_error()
    d, keep4 = _fake_desc(n_mels=64)
    assert _embed_rc(lib, d) != 0 and b"80 mel" in lib.zk_last_error()
    assert _embed_rc(lib, good, n=256) != 0 and b"256" in lib.zk_last_error()
    d, keep5 = _fake_desc(pool_dim=1234)
    assert _embed_rc(lib, d) != 0 and b"pool_dim" in lib.zk_last_error()
    assert lib.zk_speaker_embed(None, 0x1000, 1, 16000, 0x1000, 1 << 40, 0x1000, 0x1000, None) != 0
    assert lib.zk_speaker_workspace_bytes(C.byref(d), 1, 16000) == 0
    # the per-kernel launchers validate too
    assert lib.zk_spk_conv2d_cl(0x1000, 1, 48, 8, 8, 0x1000, 64, 3, 1, 0x1000, 0x1000, 0, 0x1000, None, None, None) != 0
    assert b"multiples of 32" in lib.zk_last_error()
    assert lib.zk_spk_conv2d_cl(0x1000, 1, 32, 8, 8, 0x1000, 64, 5, 1, 0x1000, 0x1000, 0, 0x1000, None, None, None) != 0
    assert lib.zk_spk_stem(0x1000, 1, 80, 10, 0x1000, 0x1000, 0x1000, 40, 0x1000, 0x1000, None) != 0
    assert lib.zk_spk_conv_tiles(80, 37) == 20 * 3


@pytest.mark.parametrize("geom", [TINY, FULL])
def test_loader_infers_geometry(geom):
    from zonos_amd.speaker import infer_geometry
    from zonos_amd.synthetic import speaker_state_dict
    in_planes, blocks = geom
    sd, lda = speaker_state_dict(in_planes, blocks, seed=0)
    assert infer_geometry(sd) == (in_planes, blocks)
    assert "front.bn1.num_batches_tracked" in sd and lda["weight"].shape == (128, 256)
    assert sd["pooling.attention.0.weight"].shape == (128, in_planes * 8 * 10, 1)
    assert sd["front.layer2.0.downsample.0.weight"].shape == (2 * in_planes, in_planes, 1, 1)
    assert "front.layer1.0.downsample.0.weight" not in sd


def test_synthetic_state_dict_is_deterministic_and_exercises_bn():
    from zonos_amd.synthetic import speaker_state_dict, state_dict_sha256
    a, la = speaker_state_dict(*TINY, seed=5)
    b, lb = speaker_state_dict(*TINY, seed=5)
    c, _ = speaker_state_dict(*TINY, seed=6)
    assert state_dict_sha256(a) == state_dict_sha256(b) and state_dict_sha256(la) == state_dict_sha256(lb)
    assert state_dict_sha256(a) != state_dict_sha256(c)
    w, v = a["front.layer3.1.bn2.weight"], a["front.layer3.1.bn2.running_var"]
    assert 0.8 <= float(w.min()) and float(w.max()) <= 1.2 and 0.7 <= float(v.min()) and float(v.max()) <= 1.3
    assert float(a["front.layer3.1.bn2.running_mean"].std()) > 0.05


def test_bn_scale_shift_equals_eval_batchnorm():
    from zonos_amd.speaker import bn_scale_shift
    from zonos_amd.synthetic import speaker_state_dict
    sd, _ = speaker_state_dict(*TINY, seed=3)
    p = "front.layer2.0.bn1."
    bn = torch.nn.BatchNorm2d(64).eval()
    bn.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
    assert bn.eps == 1e-5
    x = torch.randn(2, 64, 5, 7, generator=torch.Generator().manual_seed(1)) * 3
    scale, shift = bn_scale_shift(sd, p)
    got = x * scale[None, :, None, None] + shift[None, :, None, None]
    with torch.no_grad():
        want = bn(x)
    # two fp32 roundings each way on values of magnitude <= ~15
    assert float((got - want).abs().max()) <= 8 * 2 ** -24 * float(want.abs().max() + 1)


def test_pooling_permutation_matches_reference_reshape():
    from zonos_amd.speaker import permute_pooling
    g = torch.Generator().manual_seed(2)
    Cc, Fp, T, A = 32, 10, 3, 128
    x = torch.randn(1, Cc, Fp, T, generator=g)                       # the reference's [B, C, F', T']
    w1 = torch.randn(A, Cc * Fp, generator=g)
    w2 = torch.randn(Cc * Fp, A, generator=g)
    b2 = torch.randn(Cc * Fp, generator=g)
    ref_in = x.reshape(1, -1, T)                                     # feature index c * F' + f
    ref_h = torch.einsum("ak,bkt->bat", w1, ref_in)
    ref_logits = torch.einsum("ka,bat->bkt", w2, ref_h) + b2[None, :, None]
    w1p, w2p, b2p = permute_pooling(w1, w2, b2, Cc, Fp)
    cl_in = x.permute(0, 2, 1, 3).reshape(1, Fp * Cc, T)             # channels-last feature index f * C + c
    h = torch.einsum("ak,bkt->bat", w1p, cl_in)
    logits = torch.einsum("ka,bat->bkt", w2p, h) + b2p[None, :, None]
    assert torch.allclose(h, ref_h, rtol=1e-5, atol=1e-4)
    back = logits.reshape(1, Fp, Cc, T).permute(0, 2, 1, 3).reshape(1, Cc * Fp, T)
    assert torch.allclose(back, ref_logits, rtol=1e-5, atol=1e-3)
    assert not torch.allclose(logits, ref_logits, atol=1e-1)         # the permutation is not a no-op


def test_conv_weight_packing_layout():
    from zonos_amd.speaker import pack_conv_weight
    w = torch.randn(96, 64, 3, 3, generator=torch.Generator().manual_seed(4))
    p = pack_conv_weight(w)
    assert p.shape == (2, 2, 9, 64, 32) and p.dtype == torch.float16
    assert p[1, 1, 5, 7, 3] == w[64 + 7, 32 + 3, 1, 2].half()        # tap = kh * 3 + kw
    assert torch.all(p[1, :, :, 32:] == 0)                           # rows past Cout
    with pytest.raises(ValueError):
        pack_conv_weight(torch.zeros(64, 48, 3, 3))


def test_filterbank_and_tone_bin():
    from zonos_amd.speaker import hann_window_padded, mel_filterbank
    fb = mel_filterbank()
    assert fb.shape == (257, 80) and float(fb.min()) >= 0
    assert bool(((fb > 0).sum(0) > 0).all()), "every one of the 80 triangles covers a bin"
    assert torch.equal(fb, speaker_ref.melscale_fbanks())
    w = hann_window_padded()
    assert w.shape == (512,) and float(w[:56].abs().max()) == 0 and float(w[456:].abs().max()) == 0
    assert float(w[56 + 200]) == 1.0
    # a 1 kHz tone peaks in the filter whose centre is nearest on the HTK scale
    n = 16000
    tone = torch.sin(2 * math.pi * 1000.0 * torch.arange(n) / 16000.0)[None]
    spec = torch.stft(tone, 512, 160, 400, window=torch.hann_window(400), center=True, pad_mode="reflect",
                      return_complex=True).abs() ** 2
    mel = (spec[0].t() @ fb).mean(0)
    step = speaker_ref.htk_hz_to_mel(8000.0) / 81
    assert int(mel.argmax()) == round(speaker_ref.htk_hz_to_mel(1000.0) / step) - 1


def test_missing_checkpoint_names_the_variable(tmp_path, monkeypatch):
    from zonos_amd.speaker import SpeakerEmbedding, SpeakerEmbeddingLDA
    monkeypatch.setenv("ZONOS_SPEAKER_PATH", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="ZONOS_SPEAKER_PATH"):
        SpeakerEmbeddingLDA(device="cpu")
    with pytest.raises(FileNotFoundError, match="ZONOS_SPEAKER_PATH"):
        SpeakerEmbedding(str(tmp_path / "nope.pt"), device="cpu")
    monkeypatch.delenv("ZONOS_SPEAKER_PATH")
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    with pytest.raises(FileNotFoundError, match="ZONOS_SPEAKER_PATH"):
        SpeakerEmbeddingLDA(device="cpu")


def test_shim_and_public_surface():
    import zonos.speaker_cloning as sc
    from zonos_amd import speaker
    from zonos_amd.model import Zonos
    assert sc.SpeakerEmbeddingLDA is speaker.SpeakerEmbeddingLDA
    assert sc.SpeakerEmbedding is speaker.SpeakerEmbedding and sc.logFbankCal is speaker.logFbankCal
    src = open(os.path.join(REPO, "zonos_amd", "model.py")).read()
    assert "NotImplementedError" not in src
    assert callable(Zonos.make_speaker_embedding)
