"""GPU: streaming -- the window kernel against its host reference, windowed DAC decodes against the whole decode
(bit for bit on the default fp16 pipeline, through the C entry and through the Python-issued sequence), and
stream() end to end against generate() + autoencoder.decode."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import dac_ref, zonos_ref
from oracle import hybrid_ref as HR

from .golden_util import CLI_SP, TINY, TINY_DAC, load_gen_case
from .stream_ref import delayed_codes, window_codes_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------------------------------ 1. window kernel
@pytest.mark.parametrize("P", [0, 4])
def test_stream_window_kernel_equals_host_reference(P):
    """B = 3, K = 9, Ld = 64: a row whose EOS is known (frame 20), a live row (EOS at 50, past upto = 40), a row with
    an EOS at frame 0 (and a later one it hides). Windows at the left edge, interior, straddling row 0's end and wholly
    past it."""
    from zonos_amd._lib import call, ptr, stream_ptr
    B, K, T, upto = 3, 9, 55, 40
    delayed = delayed_codes(B, T, [[20], [50], [0, 30]], seed=P)
    assert delayed.shape == (B, K, 64)
    dd = delayed.to(DEV)
    for f0, f1 in ((P, P + 12), (10, 30), (14, 26), (24, 36), (39, 40), (P, 40)):
        W = f1 - f0
        codes_w = torch.full((B, K, W), -7, dtype=torch.int64, device=DEV)
        lens_w = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        end = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        call("zk_stream_window", ptr(dd), B, K, 64, P, f0, f1, upto, ptr(codes_w), ptr(lens_w), ptr(end), stream_ptr())
        torch.cuda.synchronize()
        rc, rl, re_ = window_codes_ref(delayed, P, f0, f1, upto)
        assert torch.equal(codes_w.cpu(), rc), (f0, f1)
        assert torch.equal(lens_w.cpu(), rl) and torch.equal(end.cpu(), re_), (f0, f1, lens_w, end)
    assert re_.tolist() == [20, -1, -1]


# ------------------------------------------------------------------------------------------ 2. windowed decode
def _decoder(cfg, seed, precision="fp16"):
    from zonos_amd.autoencoder import DacSpec, HipDacDecoder
    W = dac_ref.make_dac_weights(cfg, seed=seed)
    return HipDacDecoder(DacSpec(cfg.hidden_size, cfg.decoder_hidden_size, cfg.upsampling_ratios), W, DEV,
                         precision=precision)


@pytest.fixture(scope="module")
def long44k():
    """The 44.1 kHz decoder with the seeded weights of dac_44k_long.npz and the fixture's codes [2][9][600]."""
    d = np.load(os.path.join(G, "dac_44k_long.npz"))
    dec = _decoder(dac_ref.DAC_44KHZ, int(d["seed"]))
    return dec, torch.from_numpy(d["codes"].astype(np.int64))


def _stream_decode(dec, codes, lens, C, poll, c_stream):
    """Stream rows of ``lens`` frames cut from ``codes`` [B][9][T] (a codebook-0 EOS behind every shorter row) the
    way the engine does -- a poll every ``poll`` frames, then the flush -- and return each row's chunks concatenated."""
    from zonos_amd.autoencoder import HipDacDecoder
    from zonos_amd.engine import stream_plan
    B, T, H = codes.shape[0], max(lens), dec.spec.halo_frames
    src = codes[:, :, :T].clone()
    for b, n in enumerate(lens):
        if n < T:
            src[b, 0, n] = 1024
    delayed = zonos_ref.apply_delay(src).to(DEV)
    rows = [[] for _ in range(B)]
    uptos = list(range(poll, T, poll)) + [T]
    prev, empty = 0, 0
    old = HipDacDecoder.c_stream
    HipDacDecoder.c_stream = c_stream
    try:
        for i, upto in enumerate(uptos):
            wins = stream_plan(0, C, H, prev, upto, False)
            if i + 1 == len(uptos):
                wins += stream_plan(0, C, H, upto, upto, True)
            prev = upto
            for f0, c0, c1, f1 in wins:
                chunk, meta = dec.decode_window(delayed, 0, f0, c0, c1, f1, upto)
                n = meta[0].tolist()
                for b in range(B):
                    assert n[b] == dec.spec.hop_length * min(max(lens[b] - c0, 0), c1 - c0)
                    assert chunk[b, n[b]:].count_nonzero() == 0
                    rows[b].append(chunk[b, :n[b]].clone())
                    empty += n[b] == 0
    finally:
        HipDacDecoder.c_stream = old
    return [torch.cat(r) for r in rows], empty


def _whole(dec, codes, lens):
    T = max(lens)
    wav = dec.decode_padded(codes[:, :, :T].contiguous().to(DEV), torch.tensor(lens, dtype=torch.int32))
    return [wav[b, 0, :n * dec.spec.hop_length] for b, n in enumerate(lens)]


@pytest.mark.parametrize("lens,C", [((48, 37), 8), ((24, 24), 1)])
def test_windowed_decode_equals_whole_decode_44k(long44k, lens, C):
    """Rows of 48 and 37 frames, C = 8, H = 10: the left-edge window, interior windows, the chunk row 1 ends in
    (frame 37 inside a chunk and inside a later window's halo), chunks in which row 1 has no samples, the short last
    chunk of a flush; and C = 1 on 24 frames. Each row's chunks, concatenated, are the whole decode bit for bit, by
    the C entry and by the Python-issued sequence."""
    dec, codes = long44k
    assert dec.spec.halo_frames == 10
    whole = _whole(dec, codes, list(lens))
    for c_stream in (True, False):
        got, empty = _stream_decode(dec, codes, list(lens), C, poll=5 if C == 8 else 7, c_stream=c_stream)
        for b in range(2):
            assert got[b].shape == whole[b].shape, (c_stream, b)
            assert torch.equal(got[b], whole[b]), (c_stream, b, (got[b] - whole[b]).abs().max().item())
        assert lens[0] == lens[1] or empty > 0


def test_interior_window_equals_multitile_whole_decode_44k(long44k):
    """One interior window [290, 326) of the fixture's 600-frame row against that row's whole decode: the whole decode
    streams several tiles per workgroup there, the window does not."""
    from zonos_amd.autoencoder import HipDacDecoder
    dec, codes = long44k
    hop = dec.spec.hop_length
    row = codes[:1].contiguous()
    whole = dec.decode_padded(row.to(DEV))[0, 0]
    delayed = zonos_ref.apply_delay(row).to(DEV)
    outs = []
    for c_stream in (True, False):
        old = HipDacDecoder.c_stream
        HipDacDecoder.c_stream = c_stream
        try:
            chunk, meta = dec.decode_window(delayed, 0, 290, 300, 316, 326, 600)
        finally:
            HipDacDecoder.c_stream = old
        assert meta.tolist() == [[16 * hop], [-1]]
        outs.append(chunk[0].clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], whole[300 * hop:316 * hop]), (outs[0] - whole[300 * hop:316 * hop]).abs().max().item()


def test_windowed_decode_equals_whole_decode_tiny():
    """Tiny geometry, strides (4, 2), H = 20: two rows of 50 and 31 frames, C = 8."""
    dec = _decoder(TINY_DAC, seed=3)
    assert dec.spec.halo_frames == 20
    codes = torch.randint(0, 1024, (2, 9, 50), generator=torch.Generator().manual_seed(5))
    whole = _whole(dec, codes, [50, 31])
    for c_stream in (True, False):
        got, empty = _stream_decode(dec, codes, [50, 31], 8, poll=6, c_stream=c_stream)
        assert empty > 0
        for b in range(2):
            assert torch.equal(got[b], whole[b]), (c_stream, b, (got[b] - whole[b]).abs().max().item())


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_decode_window_other_precisions(precision):
    """decode_window on the channels-first pipelines (the C entry covers fp16 only): the same windows, against the whole
    decode of the same pipeline. These kernels promise fp32-level agreement with the reference, not a summation order
    that is independent of the position: 1e-5, the bound their own golden test holds them to (RMS), on max |d|."""
    dec = _decoder(TINY_DAC, seed=3, precision=precision)
    codes = torch.randint(0, 1024, (2, 9, 50), generator=torch.Generator().manual_seed(5))
    whole = _whole(dec, codes, [50, 31])
    got, _ = _stream_decode(dec, codes, [50, 31], 8, poll=6, c_stream=True)
    for b in range(2):
        assert got[b].shape == whole[b].shape
        assert (got[b] - whole[b]).abs().max().item() <= 1e-5


# ------------------------------------------------------------------------------------------ 3. end to end
def _tiny_engine(W, cfg=TINY):
    from zonos_amd.engine import EngineConfig, HipDecoder
    return HipDecoder(EngineConfig(d_model=cfg.d_model, n_layer=cfg.n_layer, n_heads=cfg.n_heads, n_kv=cfg.n_kv,
                                   d_ff=cfg.d_ff, eps=cfg.eps), W, DEV)


@pytest.fixture(scope="module")
def tiny_ae():
    from zonos_amd.autoencoder import DACAutoencoder, DacSpec
    c = TINY_DAC
    return DACAutoencoder(dac_ref.make_dac_weights(c, seed=3),
                          DacSpec(c.hidden_size, c.decoder_hidden_size, c.upsampling_ratios), DEV)


def _check_stream(eng, ae, cond, prefix, max_new, B, sp, C, distinct=False, **kw):
    """stream() against generate() with the same arguments, keyed noise (seed 7 unless given) and torch noise: the
    codes, the state torch's generator is left in, every row's audio and length, and the poll each chunk came at."""
    P = 0 if prefix is None else prefix.shape[2]
    H, hop = ae.decoder.spec.halo_frames, ae.decoder.spec.hop_length
    seed = kw.pop("seed", 7)
    lens_seen = None
    for noise in (dict(seed=seed), dict(noise="torch")):
        torch.manual_seed(11)
        want = [c.clone() for c in eng.generate(cond, prefix, max_new, 2.0, B, sp, **noise, **kw)]
        off_want = torch.cuda.default_generators[0].get_offset()
        torch.manual_seed(11)
        it = eng.stream(cond, prefix, max_new, 2.0, B, sp, **noise, **kw, autoencoder=ae, chunk_frames=C)
        chunks, steps = [], []
        for ch in it:
            chunks.append(ch)
            steps.append(it.steps)
        assert torch.cuda.default_generators[0].get_offset() == off_want
        assert len(it.codes) == B and all(torch.equal(a, b) for a, b in zip(it.codes, want)), noise
        assert [ch.index for ch in chunks] == list(range(len(chunks)))
        assert [ch.frame0 for ch in chunks] == [j * C for j in range(len(chunks))]
        # chunk j is yielded at the first poll (a multiple of C steps; upto = P + steps - 8) that finds
        # (j + 1) C + H final frames behind the prefix, or when the loop has ended
        final = steps[-1]
        assert steps == [min(math.ceil(((j + 1) * C + H + 8) / C) * C, final) for j in range(len(chunks))], steps
        for b in range(B):
            T_b = want[b].shape[1]
            wav = torch.cat([ch.wavs[b] for ch in chunks], dim=1)
            assert not wav.is_cuda and wav.dtype == torch.float32 and wav.shape == (1, hop * T_b), (b, wav.shape)
            if T_b:
                ref = ae.decode(want[b][None])[0].cpu()
                assert torch.equal(wav, ref), (noise, b, (wav - ref).abs().max().item())
            ends = [ch.done[b] for ch in chunks]
            assert ends[-1] and ends == sorted(ends)               # done turns on once and stays on
            first_done = ends.index(True)
            assert all(ch.wavs[b].shape[1] == 0 for ch in chunks[first_done + 1:])
        if lens_seen is None:
            lens_seen = [int(c.shape[1]) for c in want]
    if distinct:        # two rows end at different frames, one runs to max_new_tokens: the case has not degenerated
        assert len(set(lens_seen)) == 3 and max(lens_seen) == max_new, lens_seen
    return lens_seen


@pytest.mark.parametrize("C", [4, 16])
@pytest.mark.parametrize("P", [0, 3])
def test_stream_equals_generate_and_decode(C, P, tiny_ae):
    c = load_gen_case("eos_sampled")
    eng = _tiny_engine(c["W"])
    prefix = c["prefix"][..., :P].cuda() if P else None
    _check_stream(eng, tiny_ae, c["cond"].cuda(), prefix, c["max_new"], c["B"], c["sp"], C)


@pytest.mark.parametrize("C", [4, 16])
def test_stream_rows_of_different_lengths(C, tiny_ae):
    """Two rows ending at different frames and one running to max_new_tokens, on the copy heads of gen_copy_eos
    (greedy decisions with margins far above the GPU-vs-CPU logit error): the last prefix token of codebook 0 starts
    a chain that reaches an EOS token after 4 and 17 steps in rows 0 and 1 and never in row 2. The CPU oracle gives
    17 / 30 / 40 frames; asserted here on what the GPU generated."""
    c = load_gen_case("copy_eos")
    eng = _tiny_engine(c["W"], c["cfg"])
    prefix = c["prefix"][..., 1:4].clone()
    for b, tok in enumerate((56, 94, 2)):
        prefix[b, 0, -1] = tok
    _check_stream(eng, tiny_ae, c["cond"].cuda(), prefix.cuda(), c["max_new"], c["B"], c["sp"], C, distinct=True)


def test_stream_fp8_kv_cache(tiny_ae):
    c = load_gen_case("eos_sampled")
    eng = _tiny_engine(c["W"])
    _check_stream(eng, tiny_ae, c["cond"].cuda(), c["prefix"][..., :3].cuda(), c["max_new"], c["B"], c["sp"], 4,
                  kv_dtype="fp8")


def test_stream_fp8_weights(tiny_ae):
    """weight_dtype="fp8" runs at B <= 8 and d_model 2048 only: the full-width two-layer model of test_gpu_w8.py."""
    from zonos_amd.engine import EngineConfig, HipDecoder
    from zonos_amd.synthetic import backbone_weights, conditioning
    cfg = dict(d_model=2048, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
    eng = HipDecoder(EngineConfig(**cfg), backbone_weights(DEV, seed=4, **cfg), DEV)
    cond = conditioning(3, 8, cfg["d_model"], seed=3, device=DEV)
    _check_stream(eng, tiny_ae, cond, None, 24, 3, CLI_SP, 4, weight_dtype="fp8")


def test_stream_hybrid(tiny_ae):
    from zonos_amd.hybrid import HybridDecoder, HybridEngineConfig
    h = HR.HybridCfg(d_model=256, n_layer=4, attn_layer_idx=(2,), n_heads=2, n_kv=1, d_ff=512, d_state=64, headdim=32)
    ec = HybridEngineConfig(d_model=h.d_model, n_layer=h.n_layer, attn_layer_idx=h.attn_layer_idx, n_heads=h.n_heads,
                            n_kv=h.n_kv, d_ff=h.d_ff, d_state=h.d_state, headdim=h.headdim, eps=h.eps, d_mlp=h.d_mlp,
                            rms_norm=h.rms_norm, residual_in_fp32=h.residual_in_fp32)
    eng = HybridDecoder(ec, HR.make_weights(h, seed=2, head_scale=4.0), DEV)
    cond = zonos_ref.synthetic_conditioning(3, 12, h.d_model).to(DEV)
    prefix = zonos_ref.synthetic_prefix_codes(3, 3).to(DEV)
    _check_stream(eng, tiny_ae, cond, prefix, 30, 3, CLI_SP, 4)


def test_stream_closed_early_leaves_the_engine_usable(tiny_ae):
    """Break after the first chunk: what is enqueued is drained, torch's generator stands where the sampler calls that
    were made leave it, and generate() on the same engine returns what it returns on a fresh one."""
    c = load_gen_case("eos_sampled")
    cond, prefix = c["cond"].cuda(), c["prefix"].cuda()
    args = (cond, prefix, c["max_new"], 2.0, c["B"], c["sp"])
    fresh = _tiny_engine(c["W"])
    torch.manual_seed(5)
    want = [x.clone() for x in fresh.generate(*args, noise="torch")]
    eng = _tiny_engine(c["W"])
    torch.manual_seed(5)
    off0 = torch.cuda.default_generators[0].get_offset()
    for ch in eng.stream(*args, noise="torch", autoencoder=tiny_ae, chunk_frames=4, to_host=False):
        assert ch.index == 0 and all(w.is_cuda for w in ch.wavs)
        break
    moved = torch.cuda.default_generators[0].get_offset() - off0
    scal = eng._ws["scal"].cpu()
    from zonos_amd.sampling import torch_noise_policy
    _, incr = torch_noise_policy(c["B"] * 9 * 1026, eng.device)
    assert moved == (int(scal[2]) + int(scal[4])) * incr and moved > 0
    torch.manual_seed(5)
    got = eng.generate(*args, noise="torch")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a stream that is held but never finished is closed by the next call
    held = eng.stream(*args, seed=7, autoencoder=tiny_ae, chunk_frames=4)
    next(held)
    again = eng.generate(*args, seed=7)
    assert all(torch.equal(a, b) for a, b in zip(again, fresh.generate(*args, seed=7)))
    with pytest.raises(StopIteration):
        next(held)
