"""CPU: the host side of streaming -- the DAC halo (DacSpec.halo_frames against the float64 oracle), the emission
rule (engine.stream_plan against a brute-force simulation), the host reference of the window codes against
finalize's trim, and the C ABI of stream.hip (symbols, struct mirror, refusals before any launch)."""
import ctypes as C

import pytest
import torch

from oracle import dac_ref, zonos_ref

from .stream_ref import delayed_codes, simulate_stream, window_codes_ref

STRIDES = {(8, 8, 4, 2): 10, (4, 2): 20, (2, 2): 35}


@pytest.fixture(scope="module")
def dac64():
    """Per stride set: 64-channel decoder in float64, seeded codes, the whole decode."""
    out = {}
    for strides in STRIDES:
        c = dac_ref.DacCfg(hidden_size=64, decoder_hidden_size=64, upsampling_ratios=strides)
        W = {k: v.double() for k, v in dac_ref.make_dac_weights(c, seed=5).items()}
        T = 3 * STRIDES[strides] + 14
        codes = torch.randint(0, 1024, (1, 9, T), generator=torch.Generator().manual_seed(11))
        with torch.no_grad():
            whole = dac_ref.decoder(W, c, dac_ref.from_codes(W, c, codes))
        out[strides] = (c, W, codes, whole)
    return out


def _window(case, f0, f1):
    c, W, codes, _ = case
    with torch.no_grad():
        return dac_ref.decoder(W, c, dac_ref.from_codes(W, c, codes[..., f0:f1]))


@pytest.mark.parametrize("strides", list(STRIDES))
def test_halo_frames_is_the_decoder_receptive_field(strides, dac64):
    from zonos_amd.autoencoder import DacSpec
    H = DacSpec(64, 64, strides).halo_frames
    assert H == STRIDES[strides]
    c, W, codes, whole = dac64[strides]
    hop, T = c.hop_length, codes.shape[2]
    t0, t1 = H + 3, H + 9                         # interior: the halo fits on both sides
    assert t0 - H >= 0 and t1 + H <= T

    def diff(f0, f1, a=t0, b=t1):
        w = _window(dac64[strides], f0, f1)
        return (w[..., (a - f0) * hop:(b - f0) * hop] - whole[..., a * hop:b * hop]).abs().max().item()

    assert diff(t0 - H, t1 + H) == 0.0
    if strides == (8, 8, 4, 2):                   # the bound is tight there
        assert diff(t0 - H + 1, t1 + H - 1) > 0.0
    # the utterance's edges need no halo: zero padding is what the whole decode sees there
    assert diff(0, 5 + H, 0, 5) == 0.0
    assert diff(T - 5 - H, T, T - 5, T) == 0.0


@pytest.mark.parametrize("P", [0, 5])
@pytest.mark.parametrize("C", [1, 8, 16])
@pytest.mark.parametrize("H", [10, 20])
def test_stream_plan_matches_brute_force(P, C, H):
    from zonos_amd.engine import stream_plan
    # poll lengths that are no multiple of C (7, 13), one that is (C), and runs that end mid-chunk
    for poll, final in ((7, P + 61), (13, P + 3 * C + H + 2), (C, P + 47), (5, P + 3), (16, P)):
        uptos, u = [], P - 8                      # the first poll of a generation finds fewer final frames than P
        while u + poll < final:
            u += poll
            uptos.append(max(u, 0))
        uptos.append(final)
        want = simulate_stream(P, C, H, uptos)
        got, prev = [], 0
        for u in uptos:                           # every poll plans live; after the last one the flush plans ended
            got.append(stream_plan(P, C, H, prev, u, False))
            prev = u
        got[-1] = got[-1] + stream_plan(P, C, H, final, final, True)
        assert got == want, (poll, final)
        flat = [w for wins in got for w in wins]
        cover = [t for _, c0, c1, _ in flat for t in range(c0, c1)]
        assert cover == list(range(P, final))     # every frame exactly once, in order
        for (f0, c0, c1, f1), u in ((w, u) for wins, u in zip(got, uptos) for w in wins):
            assert f0 == max(P, c0 - H) and f1 == min(c1 + H, u) and f1 <= u and P <= f0 <= c0 < c1 <= f1
            assert (c0 - P) % C == 0 and (c1 - c0 == C or (u == final and c1 == final))
    with pytest.raises(ValueError):
        stream_plan(0, 0, 10, 0, 40, False)


@pytest.mark.parametrize("P", [0, 5])
def test_window_codes_reference_equals_finalize(P):
    """The host reference the GPU test holds zk_stream_window to is finalize()'s trim (model.py:437-457): an EOS at
    frame 0 (alone, and with a later one it hides), no EOS, an EOS inside the prefix region, an EOS past upto."""
    T = 40
    delayed = delayed_codes(6, T, [[0], [0, 17], [], [3], [23, 30], [36]])
    for offset in (T, T - 3, 33, 20):             # finalize trims to offset - 9 frames
        upto = offset - 9
        want = zonos_ref.finalize(delayed, offset, P)
        for f0, f1 in ((P, upto), (P, P + 4), (P + 4, upto), (P + 9, P + 11)):
            if not P <= f0 < f1 <= upto:
                continue
            codes_w, lens_w, end = window_codes_ref(delayed, P, f0, f1, upto)
            for b, ref in enumerate(want):
                n = min(max(P + ref.shape[1] - f0, 0), f1 - f0)
                assert int(lens_w[b]) == n, (offset, f0, f1, b)
                assert torch.equal(codes_w[b, :, :n], ref[:, f0 - P:f0 - P + n])
                assert codes_w[b, :, n:].count_nonzero() == 0
            first = [None, None, None, 3, 23, 36]             # the codebook-0 EOS that counts, per row
            assert end.tolist() == [t if t is not None and t < upto else -1 for t in first], (offset, end)


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    lib = C.CDLL(build.build())
    lib.zk_last_error.restype = C.c_char_p
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [C.c_int]
    return lib


STREAM_ENTRIES = ("zk_stream_window", "zk_stream_crop", "zk_stream_chunk", "zk_stream_workspace")


def test_abi_symbols_and_struct_mirror(lib):
    import os
    import re

    from zonos_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zonos_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in STREAM_ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and re.search(rf"\b{name}\s*\(", hdr), name
    assert all(n in _lib._SIGS for n in STREAM_ENTRIES[:3])
    assert lib.zk_abi_size(33) == C.sizeof(_lib.StreamDesc) and lib.zk_abi_size(34) == _lib.StreamDesc.B.offset
    lib.zk_version.restype = C.c_int
    assert lib.zk_version() >= 2
    from zonos_amd.build import SOURCES
    assert "stream.hip" in SOURCES


def _stream_desc(B=2, K=9, Ld=64, P=4):
    from zonos_amd import _lib
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    d = _lib.DacDesc()
    d.nblocks, d.ncb, d.codebook_size, d.hidden, d.cin0, d.c0 = 2, 9, 1024, 64, 64, 64
    for i, st in enumerate((4, 2)):
        d.blocks[i].stride, d.blocks[i].cin, d.blocks[i].cout, d.blocks[i].nres = st, 64 >> i, 32 >> i, 3
    sd = _lib.StreamDesc(C.pointer(d), p, B, K, Ld, P)
    return sd, p, (buf, d)


def test_stream_chunk_refuses_bad_arguments_without_gpu(lib):
    """Every refusal of zk_stream_chunk comes before any HIP call, so none needs a device: its pointers are a dummy
    host buffer."""
    from zonos_amd import _lib
    lib.zk_stream_workspace.restype = C.c_size_t
    lib.zk_stream_workspace.argtypes = [C.POINTER(_lib.StreamDesc), C.c_int]
    lib.zk_stream_chunk.argtypes = _lib._SIGS["zk_stream_chunk"]
    sd, p, keep = _stream_desc()
    need = lib.zk_stream_workspace(C.byref(sd), 36)
    assert need > 2 * 9 * 36 * 8 + 2 * 36 * 8 * 4 and lib.zk_stream_workspace(C.byref(sd), 0) == 0
    big = 1 << 30

    def refused(word, f0=10, c0=20, c1=28, f1=38, upto=40, ws=p, nbytes=big, chunk=p, n=p, end=p, desc=sd):
        rc = lib.zk_stream_chunk(C.byref(desc) if desc is not None else None, f0, c0, c1, f1, upto, ws, nbytes, chunk,
                                 n, end, None)
        err = lib.zk_last_error()
        assert rc != 0 and err.startswith(b"zk_stream_chunk:") and word in err, (word, rc, err)
        assert b"launch failed" not in err

    refused(b"prefix", f0=3)                                   # f0 < P
    refused(b"ordered", f0=21)                                 # f0 > c0
    refused(b"ordered", c0=28)                                 # empty chunk
    refused(b"ordered", c1=39)                                 # c1 > f1
    refused(b"upto", f1=41)                                    # a window past the final frames
    refused(b"upto", upto=56)                                  # upto > Ld - K: columns past the buffer
    refused(b"workspace", nbytes=lib.zk_stream_workspace(C.byref(sd), 28) - 1)
    for kw in (dict(ws=None), dict(chunk=None), dict(n=None), dict(end=None), dict(desc=None)):
        refused(b"null", **kw)
    nod, _, keep2 = _stream_desc()
    nod.delayed = None
    refused(b"null", desc=nod)
    nodac, _, keep3 = _stream_desc()
    nodac.dac = None
    refused(b"null", desc=nodac)
    k8, _, keep4 = _stream_desc(K=8)
    refused(b"codebooks", desc=k8)
    # the two kernels' own entries refuse the same under their own names
    lib.zk_stream_window.argtypes = _lib._SIGS["zk_stream_window"]
    assert lib.zk_stream_window(p, 2, 9, 64, 4, 3, 20, 40, p, p, p, None) != 0
    assert lib.zk_last_error().startswith(b"zk_stream_window:") and b"prefix" in lib.zk_last_error()
    assert lib.zk_stream_window(p, 2, 9, 64, 4, 10, 20, 56, p, p, p, None) != 0 and b"upto" in lib.zk_last_error()
    lib.zk_stream_crop.argtypes = _lib._SIGS["zk_stream_crop"]
    assert lib.zk_stream_crop(p, 2, 8, 10, 9, 20, 30, p, p, p, None) != 0
    assert lib.zk_last_error().startswith(b"zk_stream_crop:")


def test_stream_refusals_need_no_device():
    """chunk_frames < 1 is refused before anything is allocated, on the engine and on the model."""
    from zonos_amd.engine import EngineConfig, HipDecoder
    from zonos_amd.model import Zonos
    eng = HipDecoder.__new__(HipDecoder)
    eng.cfg = EngineConfig(d_model=256, n_layer=2, n_heads=2, n_kv=1, d_ff=512)
    with pytest.raises(ValueError, match="chunk_frames"):
        eng.stream(None, None, 8, 2.0, 1, autoencoder=object(), chunk_frames=0)
    with pytest.raises(ValueError, match="autoencoder"):
        eng.stream(None, None, 8, 2.0, 1)
    with pytest.raises(ValueError, match="chunk_frames"):
        Zonos.stream(Zonos.__new__(Zonos), None, chunk_frames=-1)
    import zonos.model as drop_in
    assert drop_in.Zonos.stream is Zonos.stream and drop_in.StreamChunk(0, 0, [], []).index == 0
