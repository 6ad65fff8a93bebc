"""CPU: the FP8 (e4m3fn) KV-cache format of zonos_amd.kvlayout -- the exact scale rule, the byte layout --
and the C ABI that carries it (symbols, grown descriptors, host-side rejection of bad descriptors)."""
import ctypes as C

import pytest
import torch

from zonos_amd import kvlayout as kl


def _rows():
    g = torch.Generator().manual_seed(0)
    rows = [(torch.randn(64, 128, generator=g) * s).to(torch.bfloat16) for s in (1e-3, 1.0, 300.0)]
    rows.append(torch.zeros(3, 128, dtype=torch.bfloat16))
    edge = torch.randn(24, 128, generator=g).to(torch.bfloat16) * 0.01
    for i, k in enumerate(range(-6, 6)):
        edge[2 * i, 5] = 448.0 * 2.0 ** k                       # amax exactly 448 * 2^k: e = k
        edge[2 * i + 1, 9] = -(448.0 + 2.0) * 2.0 ** k          # next bf16 above (ulp at 448 = 2): e = k + 1
    rows.append(edge)
    return torch.cat(rows)


def test_quantiser_properties():
    x = _rows()
    q, s = kl.quantize_kv_e4m3(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.dtype == torch.uint8 and s.shape == x.shape[:-1]
    e = s.to(torch.int32) - 127
    scaled = torch.ldexp(x.float(), (-e).unsqueeze(-1))
    assert scaled.abs().max() <= 448
    assert ((q & 0x7F) != 0x7F).all(), "NaN byte"
    assert torch.equal(q, scaled.to(torch.float8_e4m3fn).view(torch.uint8))
    d = kl.dequantize_kv_e4m3(q, s)
    assert d.dtype == torch.bfloat16
    exact = torch.ldexp(q.view(torch.float8_e4m3fn).float(), e.unsqueeze(-1))
    assert torch.equal(d.float(), exact), "a dequantised value is not representable in bf16"
    # the smallest exponent that fits: one less would overflow 448 (rows with a nonzero amax)
    amax = x.float().abs().amax(-1)
    nz = amax > 0
    assert (torch.ldexp(amax[nz], -(e[nz] - 1)) > 448).all()
    assert (e[~nz] == 0).all() and (q[~nz] == 0).all()
    # the edge rows: amax = 448 * 2^k -> byte 0x7E (448) at e = k; just above -> e = k + 1
    edge = x[-24:]
    qe, se = kl.quantize_kv_e4m3(edge)
    for i, k in enumerate(range(-6, 6)):
        assert int(se[2 * i]) - 127 == k and int(qe[2 * i, 5]) == 0x7E
        assert int(se[2 * i + 1]) - 127 == k + 1 and int(qe[2 * i + 1, 9]) == 0xF6       # -(225 -> 224)
    # quantisation error: half an e4m3 ulp of the scaled value, at most 16 * 2^e (ulp 32 in [256, 448])
    assert ((d.float() - x.float()).abs() <= 16 * torch.ldexp(torch.ones(()), e).unsqueeze(-1)).all()


def test_layout_pack_roundtrip_and_offsets():
    R, Hk, S = 2, 3, 96
    x = torch.arange(R * Hk * S * 128).reshape(R, Hk, S, 128)
    xb = (x * 7 % 251).to(torch.uint8)
    pk, pv = kl.pack_k8(xb), kl.pack_v8(xb)
    assert pk.shape == pv.shape == (R, Hk, S * 128)
    assert torch.equal(kl.unpack_k8(pk, S), xb) and torch.equal(kl.unpack_v8(pv, S), xb)
    pk, pv = kl.pack_k8(x), kl.pack_v8(x)
    for key, d in [(0, 0), (5, 77), (37, 127), (63, 64), (12, 9), (95, 31), (33, 40)]:
        assert int(pk[1, 2, kl.k8_offset(key, d)]) == int(x[1, 2, key, d]), (key, d)
        assert int(pv[1, 2, kl.v8_offset(key, d)]) == int(x[1, 2, key, d]), (key, d)
    # documented order: K8 [slice][h 2][kp 2][lane 64][q 2][8], V8 [slice][dp 4][lane 64][q 2][8]
    sl, h, kp, lg, ln, q, e = 2, 1, 1, 3, 9, 1, 5
    off = sl * 4096 + ((h * 2 + kp) * 64 + lg * 16 + ln) * 16 + q * 8 + e
    key, dim = 32 * sl + 8 * (ln >> 2) + 4 * h + (ln & 3), 32 * (2 * kp + q) + 8 * lg + e
    assert int(pk[0, 0, off]) == int(x[0, 0, key, dim])
    dp = 2
    off = sl * 4096 + (dp * 64 + lg * 16 + ln) * 16 + q * 8 + e
    assert int(pv[0, 0, off]) == int(x[0, 0, 32 * sl + 8 * lg + e, 16 * (2 * dp + q) + ln])
    # a lane's 16-byte load is one contiguous run: two d-steps of one key (K), two d-tiles of 8 keys (V)
    assert kl.k8_offset(7, 8) + 8 == kl.k8_offset(7, 40) and kl.v8_offset(8, 3) + 8 == kl.v8_offset(8, 19)


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    lib = C.CDLL(build.build())
    lib.zk_last_error.restype = C.c_char_p
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [C.c_int]
    return lib


def test_abi_symbols_and_struct_mirrors(lib):
    from zonos_amd import _lib
    for name in ("zk_kv_quantize_e4m3", "zk_attn_decode_f8", "zk_attn_decode_qkv_f8"):
        assert hasattr(lib, name) and name in _lib._SIGS and name in _lib.exported_symbols()
    assert lib.zk_abi_size(6) == C.sizeof(_lib.StepLayer) and lib.zk_abi_size(7) == C.sizeof(_lib.StepDesc)
    assert lib.zk_abi_size(23) == _lib.StepDesc.kv_fp8.offset == _lib.StepDesc.eps.offset + 4
    assert lib.zk_abi_size(24) == _lib.StepDesc.pre_k.offset
    assert lib.zk_abi_size(25) == _lib.StepLayer.k_scale.offset
    # kv_fp8 sits in what was padding: no earlier field moved
    assert _lib.StepDesc.layers.offset == _lib.StepDesc.eps.offset + 8
    assert lib.zk_abi_size(14) == _lib.StepDesc.st.offset and lib.zk_abi_size(15) == _lib.StepDesc.sp.offset


def _desc(small, scales=True, scratch=True):
    from zonos_amd import _lib
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    lays = (_lib.StepLayer * 2)()
    for L in lays:
        L.k_cache = L.vt_cache = p
        if scales:
            L.k_scale = L.v_scale = p
    d = _lib.StepDesc()
    d.B, d.n_layer, d.d_model, d.n_heads, d.n_kv, d.head_dim, d.smax = 1, 2, 256, 2, 1, 128, 512
    d.layers = C.cast(lays, C.c_void_p)
    d.small, d.kv_fp8 = small, 1
    d.st.Ld, d.st.K, d.st.V = 100, 9, 1026
    if scratch:
        d.pre_k = d.pre_vt = p
        d.pre_smax = 128
    return d, (buf, lays)


def test_step_entries_reject_bad_fp8_descriptors_without_gpu(lib):
    """kv_fp8 = 1 with small = 1, or without the scale / scratch pointers, fails before any launch."""
    buf = C.create_string_buffer(16)
    d, keep = _desc(small=1)
    assert lib.zk_decode_step(C.byref(d), None) != 0
    assert b"kv_fp8" in lib.zk_last_error() and b"small" in lib.zk_last_error()
    assert lib.zk_prefill(C.byref(d), buf, 10, 0, buf, None) != 0
    assert b"kv_fp8" in lib.zk_last_error() and b"small" in lib.zk_last_error()
    d, keep = _desc(small=0, scales=False)
    assert lib.zk_decode_step(C.byref(d), None) != 0 and b"scale" in lib.zk_last_error()
    assert lib.zk_prefill(C.byref(d), buf, 10, 0, buf, None) != 0 and b"scale" in lib.zk_last_error()
    d, keep = _desc(small=0, scratch=False)
    assert lib.zk_prefill(C.byref(d), buf, 10, 0, buf, None) != 0 and b"scratch" in lib.zk_last_error()
    d, keep = _desc(small=0)
    d.pre_smax = 8                                             # shorter than S = Lc + P + 1 = 11
    assert lib.zk_prefill(C.byref(d), buf, 10, 0, buf, None) != 0 and b"scratch" in lib.zk_last_error()


def test_new_entries_validate_arguments_without_gpu(lib):
    rc = lib.zk_attn_decode_f8(None, None, None, None, None, 2, 2, 1, 128, 200, 1, None, None, 1, None, None, None)
    assert rc != 0 and b"zk_attn_decode_f8" in lib.zk_last_error() and b"Smax" in lib.zk_last_error()
    rc = lib.zk_attn_decode_qkv_f8(None, 1, None, None, None, None, None, 2, 2, 1, 64, 256, 1, None, None, 1, None,
                                   None, None, None)
    assert rc != 0 and b"head_dim" in lib.zk_last_error()
    rc = lib.zk_kv_quantize_e4m3(None, None, 2, 1, 128, 300, 256, None, None, None, None, 512, None)
    assert rc != 0 and b"zk_kv_quantize_e4m3" in lib.zk_last_error()


def test_kv_dtype_resolution(monkeypatch):
    from zonos_amd.engine import resolve_kv_dtype
    monkeypatch.delenv("ZONOS_KV_DTYPE", raising=False)
    assert resolve_kv_dtype(None) == "bf16" and resolve_kv_dtype("fp8") == "fp8"
    monkeypatch.setenv("ZONOS_KV_DTYPE", "fp8")
    assert resolve_kv_dtype(None) == "fp8" and resolve_kv_dtype("bf16") == "bf16"
    with pytest.raises(ValueError):
        resolve_kv_dtype("int4")
