"""CPU: the FP8 (e4m3fn) weight format of zonos_amd.wlayout -- the row scale rule, the packed image -- and the
C ABI that carries it (symbols, grown descriptors, host-side rejection of bad descriptors and arguments), and
generate()'s ``weight_dtype`` resolution."""
import ctypes as C

import pytest
import torch

from zonos_amd import wlayout as wl


def _weights(N=72, K=256):
    """Rows of magnitudes 2^-10 .. 2^3, one zero row, rows whose amax is exactly 448 * 2^k and just above."""
    g = torch.Generator().manual_seed(1)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-10, 4, (N, 1), generator=g).float())
    w = w.to(torch.bfloat16)
    w[7] = 0
    for i, k in enumerate(range(-6, 6)):
        w[10 + 2 * i] = (torch.randn(K, generator=g) * 0.01 * 2.0 ** k).to(torch.bfloat16)
        w[10 + 2 * i, 5] = 448.0 * 2.0 ** k                       # amax exactly 448 * 2^k: e = k
        w[11 + 2 * i] = w[10 + 2 * i]
        w[11 + 2 * i, 9] = -(448.0 + 2.0) * 2.0 ** k              # the next bf16 above: e = k + 1
    return w


def test_quantiser_properties():
    w = _weights()
    q, s = wl.quantize_w_e4m3(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and s.dtype == torch.uint8 and s.shape == (w.shape[0],)
    e = s.to(torch.int32) - 127
    scaled = torch.ldexp(w.float(), (-e).unsqueeze(-1))
    assert scaled.abs().max() <= 448
    assert ((q & 0x7F) != 0x7F).all(), "NaN byte"
    assert torch.equal(q, scaled.to(torch.float8_e4m3fn).view(torch.uint8))
    d = wl.dequantize_w_e4m3(q, s)
    assert d.dtype == torch.bfloat16
    exact = torch.ldexp(q.view(torch.float8_e4m3fn).float(), e.unsqueeze(-1))
    assert torch.equal(d.float(), exact), "a dequantised value is not representable in bf16"
    # requantising the dequantised weights returns the same values
    q2, s2 = wl.quantize_w_e4m3(d)
    assert torch.equal(wl.dequantize_w_e4m3(q2, s2), d)
    # a zero row: exponent 0, zero bytes
    assert int(s[7]) == 127 and (q[7] == 0).all()
    # the smallest exponent that fits (rows with a nonzero amax)
    amax = w.float().abs().amax(-1)
    nz = amax > 0
    assert (torch.ldexp(amax[nz], -(e[nz] - 1)) > 448).all()
    for i, k in enumerate(range(-6, 6)):
        assert int(e[10 + 2 * i]) == k and int(q[10 + 2 * i, 5]) == 0x7E
        assert int(e[11 + 2 * i]) == k + 1 and int(q[11 + 2 * i, 9]) == 0xF6
    # the scale is the row's own (kv_scale_exponent of the row's amax over all K)
    from zonos_amd.kvlayout import kv_scale_exponent
    assert torch.equal(e, kv_scale_exponent(amax))


@pytest.mark.parametrize("N,K", [(40, 128), (64, 2048), (80, 192)])
def test_pack_roundtrip_and_offsets(N, K):
    q = (torch.arange(N * K).reshape(N, K) * 7 % 251).to(torch.uint8)
    s = (torch.arange(N) % 200 + 20).to(torch.uint8)
    img, sp = wl.pack_w8(q, s)
    Np = wl.padded_rows(N)
    assert Np % 64 == 0 and img.shape == (Np * K,) and img.dtype == torch.uint8 and sp.shape == (Np,)
    q2, s2 = wl.unpack_w8(img, sp, N)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    # padded rows: zero bytes, scale byte 127
    qa, sa = wl.unpack_w8(img, sp, Np)
    assert (qa[N:] == 0).all() and (sa[N:] == 127).all()
    for n, k in [(0, 0), (N - 1, K - 1), (17, 77), (33, 64), (5, 127), (39, 40)]:
        assert int(img[wl.w8_offset(n, k, K)]) == int(q[n, k]), (n, k)
    # documented order [tile][K/64 pairs][lane 64][q 2][8], lane = 16 lg + ln
    tile, pair, lg, ln, qq, e = 2, 1, 3, 6, 1, 5
    off = ((tile * (K // 64) + pair) * 64 + 16 * lg + ln) * 16 + qq * 8 + e
    assert int(img[off]) == int(q[16 * tile + ln, 64 * pair + 32 * qq + 8 * lg + e])
    # a lane's 16-byte load is one contiguous run: the same 8 columns of two consecutive k-steps
    assert wl.w8_offset(3, 8, K) + 8 == wl.w8_offset(3, 40, K)
    # the half-tile form: lane ^ 8 of the next pair lies 1024 B + (8 rows) * 16 B further
    assert wl.w8_offset(3, 64, K) - wl.w8_offset(3, 0, K) == 1024
    assert wl.w8_offset(11, 0, K) - wl.w8_offset(3, 0, K) == 8 * 16


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    lib = C.CDLL(build.build())
    lib.zk_last_error.restype = C.c_char_p
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [C.c_int]
    return lib


W8_ENTRIES = ("zk_pack_weights_e4m3", "zk_gemv_fused_w8", "zk_gemv_qkv_rope_w8", "zk_gemv_attn_out_w8")


def test_abi_symbols_and_struct_mirrors(lib):
    from zonos_amd import _lib
    for name in W8_ENTRIES:
        assert hasattr(lib, name) and name in _lib._SIGS and name in _lib.exported_symbols()
    assert lib.zk_abi_size(6) == C.sizeof(_lib.StepLayer) and lib.zk_abi_size(7) == C.sizeof(_lib.StepDesc)
    assert lib.zk_abi_size(31) == _lib.StepDesc.w_fp8.offset == _lib.StepDesc.pre_smax.offset + 4
    assert lib.zk_abi_size(32) == _lib.StepLayer.wqkv8.offset == _lib.StepLayer.v_scale.offset + 8
    # the new fields stand at the end: no earlier field moved
    assert lib.zk_abi_size(25) == _lib.StepLayer.k_scale.offset and lib.zk_abi_size(24) == _lib.StepDesc.pre_k.offset
    assert lib.zk_abi_size(14) == _lib.StepDesc.st.offset and lib.zk_abi_size(15) == _lib.StepDesc.sp.offset


def _desc(small=1, kv_fp8=0, images=True, scales=True):
    from zonos_amd import _lib
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    lays = (_lib.StepLayer * 2)()
    for L in lays:
        L.k_cache = L.vt_cache = L.k_scale = L.v_scale = p
        if images:
            L.wqkv8 = L.wo8 = L.fc18 = L.fc28 = p
        if scales:
            L.wqkv_scale = L.wo_scale = L.fc1_scale = L.fc2_scale = p
    d = _lib.StepDesc()
    d.B, d.n_layer, d.d_model, d.n_heads, d.n_kv, d.head_dim, d.smax = 1, 2, 2048, 16, 4, 128, 512
    d.layers = C.cast(lays, C.c_void_p)
    d.small, d.kv_fp8, d.w_fp8 = small, kv_fp8, 1
    d.st.Ld, d.st.K, d.st.V = 100, 9, 1026
    return d, (buf, lays)


def test_decode_step_rejects_bad_w_fp8_descriptors_without_gpu(lib):
    """w_fp8 = 1 with small = 0, with kv_fp8 = 1, or without an image / scale pointer, fails before any launch."""
    d, keep = _desc(small=0)
    assert lib.zk_decode_step(C.byref(d), None) != 0
    assert b"w_fp8" in lib.zk_last_error() and b"small" in lib.zk_last_error()
    d, keep = _desc(small=0, kv_fp8=1)
    assert lib.zk_decode_step(C.byref(d), None) != 0 and b"w_fp8" in lib.zk_last_error()
    d, keep = _desc(small=1, kv_fp8=1)                             # (refused by the KV check or by this one)
    assert lib.zk_decode_step(C.byref(d), None) != 0 and b"fp8" in lib.zk_last_error()
    d, keep = _desc(images=False)
    assert lib.zk_decode_step(C.byref(d), None) != 0
    assert b"w_fp8 layer 0" in lib.zk_last_error() and b"image" in lib.zk_last_error()
    d, keep = _desc(scales=False)
    assert lib.zk_decode_step(C.byref(d), None) != 0 and b"scale" in lib.zk_last_error()
    d, keep = _desc()
    keep[1][1].fc28 = None                                         # one pointer of the last layer
    assert lib.zk_decode_step(C.byref(d), None) != 0 and b"w_fp8 layer 1" in lib.zk_last_error()


def test_w8_entries_validate_arguments_without_gpu(lib):
    """Each _w8 entry rejects what its bf16 counterpart rejects (and a missing image / scale pointer)."""
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    F = C.c_float
    lib.zk_gemv_fused_w8.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + \
        [C.c_void_p, C.c_void_p, F] + [C.c_void_p] * 4
    lib.zk_gemv_fused.argtypes = [C.c_void_p, C.c_long, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, F] + \
        [C.c_void_p] * 4

    def fused(M=2, N=64, K=2048, mode=0, lda=None, lnw=None, lnb=None, Cf=p, Cb=p, W=p, sc=p):
        lda = K if lda is None else lda
        r8 = lib.zk_gemv_fused_w8(p, lda, W, sc, M, N, K, mode, lnw, lnb, 1e-5, Cf, Cb, None, None)
        e8 = lib.zk_last_error()
        if W is not None and sc is not None:       # the bf16 entry refuses the same arguments
            assert lib.zk_gemv_fused(p, lda, W, M, N, K, mode, lnw, lnb, 1e-5, Cf, Cb, None, None) != 0
        return r8, e8

    for kw, word in [(dict(M=0), b"M="), (dict(M=17), b"M="), (dict(N=0), b"N="), (dict(K=1024), b"K="),
                     (dict(lda=2040), b"lda"), (dict(lda=2049), b"lda"), (dict(mode=3), b"mode"),
                     (dict(mode=1, N=40), b"SwiGLU"), (dict(lnw=p), b"LN"), (dict(lnw=p, lnb=p, K=4096), b"LN"),
                     (dict(mode=0, Cf=None), b"output"), (dict(mode=2, Cb=None), b"output"),
                     (dict(mode=1, lnw=p, lnb=p, N=64, K=8192), b"LN"), (dict(W=None), b"image"), (dict(sc=None), b"scales")]:
        rc, err = fused(**kw)
        assert rc != 0 and b"zk_gemv_fused_w8" in err and word in err, (kw, err)

    lib.zk_gemv_qkv_rope_w8.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, F] + \
        [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4

    def rope(M=2, H=16, Hkv=4, hd=128, Smax=256, sc=p, pos=p):
        return lib.zk_gemv_qkv_rope_w8(p, p, sc, M, H, Hkv, hd, p, p, 1e-5, p, p, p, Smax, pos, p, None, None), \
            lib.zk_last_error()

    for kw, word in [(dict(M=3), b"M="), (dict(M=0), b"M="), (dict(hd=64), b"hd="), (dict(H=16, Hkv=3), b"Hkv="),
                     (dict(H=8, Hkv=2), b"d_model"), (dict(Smax=100), b"Smax"), (dict(Smax=0), b"Smax"),
                     (dict(sc=None), b"null"), (dict(pos=None), b"null")]:
        rc, err = rope(**kw)
        assert rc != 0 and b"zk_gemv_qkv_rope_w8" in err and word in err, (kw, err)

    lib.zk_gemv_attn_out_w8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 3 + \
        [C.c_void_p] * 3

    def out(nsplit=4, Hkv=4, M=2, N=2048, K=2048, work=p, W=p, sc=p):
        return lib.zk_gemv_attn_out_w8(work, nsplit, Hkv, W, sc, M, N, K, p, None, None), lib.zk_last_error()

    for kw, word in [(dict(M=3), b"M="), (dict(K=4096), b"K="), (dict(N=40), b"N="), (dict(Hkv=0), b"Hkv"),
                     (dict(Hkv=3), b"Hkv"), (dict(Hkv=1), b"Hkv"), (dict(work=None), b"null"), (dict(sc=None), b"null"),
                     (dict(W=None), b"null")]:
        rc, err = out(**kw)
        assert rc != 0 and b"zk_gemv_attn_out_w8" in err and word in err, (kw, err)

    lib.zk_pack_weights_e4m3.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.zk_pack_weights_e4m3(p, 40, 100, p, p, None) != 0 and b"zk_pack_weights_e4m3" in lib.zk_last_error()
    assert lib.zk_pack_weights_e4m3(p, 0, 128, p, p, None) != 0
    assert lib.zk_pack_weights_e4m3(p, 40, 128, p, None, None) != 0 and b"null" in lib.zk_last_error()


def test_weight_dtype_resolution(monkeypatch):
    from zonos_amd.engine import resolve_weight_dtype
    monkeypatch.delenv("ZONOS_WEIGHT_DTYPE", raising=False)
    assert resolve_weight_dtype(None) == "bf16" and resolve_weight_dtype("fp8") == "fp8"
    monkeypatch.setenv("ZONOS_WEIGHT_DTYPE", "fp8")
    assert resolve_weight_dtype(None) == "fp8" and resolve_weight_dtype("bf16") == "bf16"
    with pytest.raises(ValueError):
        resolve_weight_dtype("int4")
    monkeypatch.setenv("ZONOS_WEIGHT_DTYPE", "fp4")
    with pytest.raises(ValueError):
        resolve_weight_dtype(None)


def test_weight_dtype_is_keyword_only_on_the_public_entries():
    import inspect

    from zonos_amd.distributed import generate_sharded
    from zonos_amd.engine import HipDecoder
    from zonos_amd.model import Zonos
    for fn in (HipDecoder.generate, Zonos.generate, generate_sharded):
        par = inspect.signature(fn).parameters["weight_dtype"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None, fn


class _Cond:
    """What generate() reads of its conditioning before the refusals (no device needed)."""
    def __init__(self, R, D):
        self.shape = (R, 8, D)


def _bare(cls, **cfg):
    from zonos_amd.engine import EngineConfig
    eng = cls.__new__(cls)                          # no weights, no device: the refusals come before both
    eng.cfg = EngineConfig(**cfg)
    eng.rope_neox = 0
    eng._ws = None
    return eng


def test_weight_dtype_refusals_need_no_device(monkeypatch):
    from zonos_amd.backbone import HipZonosBackbone
    from zonos_amd.engine import HipDecoder
    from zonos_amd.hybrid import HybridDecoder
    monkeypatch.delenv("ZONOS_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("ZONOS_KV_DTYPE", raising=False)
    full = dict(d_model=2048, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
    eng = _bare(HipDecoder, **full)
    with pytest.raises(ValueError, match="batch_size <= 8"):
        eng.generate(_Cond(18, 2048), None, 4, 2.0, 9, weight_dtype="fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        eng.generate(_Cond(2, 2048), None, 4, 2.0, 1, weight_dtype="fp8", kv_dtype="fp8")
    with pytest.raises(ValueError, match="weight_dtype must be"):
        eng.generate(_Cond(2, 2048), None, 4, 2.0, 1, weight_dtype="int8")
    monkeypatch.setenv("ZONOS_WEIGHT_DTYPE", "fp8")
    with pytest.raises(ValueError, match="batch_size <= 8"):
        eng.generate(_Cond(18, 2048), None, 4, 2.0, 9)
    monkeypatch.delenv("ZONOS_WEIGHT_DTYPE")
    narrow = _bare(HipDecoder, d_model=512, n_layer=2, n_heads=4, n_kv=2, d_ff=512)
    with pytest.raises(ValueError, match="d_model 2048"):
        narrow.generate(_Cond(2, 512), None, 4, 2.0, 1, weight_dtype="fp8")
    hyb = _bare(HybridDecoder, **full)
    with pytest.raises(ValueError, match="HybridDecoder"):
        hyb.generate(_Cond(2, 2048), None, 4, 2.0, 1, weight_dtype="fp8")
    from zonos_amd.backbone import HipHybridBackbone
    for plugin in (HipZonosBackbone, HipHybridBackbone):
        with pytest.raises(ValueError, match="plugin"):
            plugin.allocate_inference_cache(plugin.__new__(plugin), 2, 64, weight_dtype="fp8")
