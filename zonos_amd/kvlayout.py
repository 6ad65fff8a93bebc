"""Host-side view of the engine's KV-cache layout (backbone.hip k_off / v_off).

Per (row, kv head): Smax keys in 32-key slices of 8 KB, each slice stored in the order the
decode wave's MFMA fragments read it (one contiguous 1 KB load per fragment):
  K: [slice][h 2][ks 4][lane 64][8] -- lane = 16*lg + ln holds key 8*(ln>>2) + 4h + (ln&3)
     of the slice, dims 32*ks + 8*lg .. +8
  V: [slice][dt 8][lane 64][8]      -- lane holds channel 16*dt + ln, keys 8*lg .. 8*lg+7
Used by tests and tools to build / read caches; the engine never converts at run time.

FP8 cache (generate(kv_dtype="fp8")): the same 32-key slices, 4 KB each, of OCP e4m3fn bytes, every
lane's load 16 B wide (two d-steps of K / two d-tiles of V):
  K8: [slice][h 2][kp 2][lane 64][q 2][8] -- lane as above, dims 32*(2kp + q) + 8*lg .. +8
  V8: [slice][dp 4][lane 64][q 2][8]      -- lane holds channel 16*(2dp + q) + ln, keys 8*lg .. 8*lg+7
plus one power-of-two scale per (row, kv head, key) for K and one for V, stored as its biased
exponent byte b (E8M0, scale 2^(b-127)) in key order: uint8 [R][Hkv][Smax].
Scale rule (quantize_kv_e4m3; the kernels compute the same integers): amax = largest |x| of the
key's 128 values = m * 2^x with m in [1, 2); e = x - 8 if m <= 1.75 else x - 7 (the smallest e with
amax * 2^-e <= 448), clamped to [-126, 127], e = 0 for amax == 0; byte = RNE e4m3fn(x * 2^-e).
A dequantised value q * 2^e has 4 significant bits, so it is exact in bf16.
"""
from __future__ import annotations

import torch


def pack_k(k: torch.Tensor) -> torch.Tensor:
    """[R][Hkv][S][128] (S % 32 == 0) -> packed [R][Hkv][S*128]."""
    R, Hk, S, hd = k.shape
    assert hd == 128 and S % 32 == 0
    # key = 32*sl + 8*grp + 4*h + i ; dim = 32*ks + 8*lg + e
    x = k.reshape(R, Hk, S // 32, 4, 2, 4, 4, 4, 8)          # sl grp h i | ks lg e
    x = x.permute(0, 1, 2, 4, 6, 7, 3, 5, 8)                 # sl h ks lg grp i e  (lane = 16lg + 4grp + i)
    return x.reshape(R, Hk, S * hd).contiguous()


def pack_v(v: torch.Tensor) -> torch.Tensor:
    """[R][Hkv][S][128] -> packed [R][Hkv][S*128]."""
    R, Hk, S, hd = v.shape
    assert hd == 128 and S % 32 == 0
    # key = 32*sl + 8*lg + e ; channel = 16*dt + ln
    x = v.reshape(R, Hk, S // 32, 4, 8, 8, 16)               # sl lg e | dt ln
    x = x.permute(0, 1, 2, 5, 3, 6, 4)                       # sl dt lg ln e
    return x.reshape(R, Hk, S * hd).contiguous()


def unpack_k(kp: torch.Tensor, S: int) -> torch.Tensor:
    R, Hk = kp.shape[:2]
    x = kp.reshape(R, Hk, S // 32, 2, 4, 4, 4, 4, 8)         # sl h ks lg grp i e
    x = x.permute(0, 1, 2, 6, 3, 7, 4, 5, 8)                 # sl grp h i ks lg e
    return x.reshape(R, Hk, S, 128)


def unpack_v(vp: torch.Tensor, S: int) -> torch.Tensor:
    R, Hk = vp.shape[:2]
    x = vp.reshape(R, Hk, S // 32, 8, 4, 16, 8)              # sl dt lg ln e
    x = x.permute(0, 1, 2, 4, 6, 3, 5)                       # sl lg e dt ln
    return x.reshape(R, Hk, S, 128)


# ---------------------------------------------------------------------------- FP8 (e4m3fn) cache
def kv_scale_exponent(amax: torch.Tensor) -> torch.Tensor:
    """The scale exponent e (int32) of the rule above for amax >= 0 (fp32)."""
    m, ex = torch.frexp(amax.float())                         # amax = m * 2^ex, m in [0.5, 1)
    e = ex.to(torch.int32) - 1 - 8 + (m > 0.875).to(torch.int32)
    e = e.clamp(-126, 127)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def quantize_kv_e4m3(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[..., 128] bf16 / fp32 -> (e4m3fn bytes uint8 [..., 128], scale bytes uint8 [...])."""
    xf = x.float()
    e = kv_scale_exponent(xf.abs().amax(dim=-1))
    q = torch.ldexp(xf, (-e).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), (e + 127).to(torch.uint8)


def dequantize_kv_e4m3(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Inverse view of quantize_kv_e4m3: bytes [..., 128] and scale bytes [...] -> bf16 (exact)."""
    e = scale.to(torch.int32) - 127
    return torch.ldexp(q.view(torch.float8_e4m3fn).float(), e.unsqueeze(-1)).to(torch.bfloat16)


def pack_k8(k: torch.Tensor) -> torch.Tensor:
    """bytes [R][Hkv][S][128] (S % 32 == 0) -> packed [R][Hkv][S*128]."""
    R, Hk, S, hd = k.shape
    assert hd == 128 and S % 32 == 0
    # key = 32*sl + 8*grp + 4*h + i ; dim = 64*kp + 32*q + 8*lg + e
    x = k.reshape(R, Hk, S // 32, 4, 2, 4, 2, 2, 4, 8)       # sl grp h i | kp q lg e
    x = x.permute(0, 1, 2, 4, 6, 8, 3, 5, 7, 9)              # sl h kp lg grp i q e
    return x.reshape(R, Hk, S * hd).contiguous()


def pack_v8(v: torch.Tensor) -> torch.Tensor:
    """bytes [R][Hkv][S][128] -> packed [R][Hkv][S*128]."""
    R, Hk, S, hd = v.shape
    assert hd == 128 and S % 32 == 0
    # key = 32*sl + 8*lg + e ; channel = 32*dp + 16*q + ln
    x = v.reshape(R, Hk, S // 32, 4, 8, 4, 2, 16)            # sl lg e | dp q ln
    x = x.permute(0, 1, 2, 5, 3, 7, 6, 4)                    # sl dp lg ln q e
    return x.reshape(R, Hk, S * hd).contiguous()


def unpack_k8(kp: torch.Tensor, S: int) -> torch.Tensor:
    R, Hk = kp.shape[:2]
    x = kp.reshape(R, Hk, S // 32, 2, 2, 4, 4, 4, 2, 8)      # sl h kp lg grp i q e
    x = x.permute(0, 1, 2, 6, 3, 7, 4, 8, 5, 9)              # sl grp h i kp q lg e
    return x.reshape(R, Hk, S, 128)


def unpack_v8(vp: torch.Tensor, S: int) -> torch.Tensor:
    R, Hk = vp.shape[:2]
    x = vp.reshape(R, Hk, S // 32, 4, 4, 16, 2, 8)           # sl dp lg ln q e
    x = x.permute(0, 1, 2, 4, 7, 3, 6, 5)                    # sl lg e dp q ln
    return x.reshape(R, Hk, S, 128)


def k8_offset(key: int, dim: int) -> int:
    """Byte offset of (key, dim) inside one (row, kv head) block of the K8 cache."""
    o, ks, lg = key & 31, dim >> 5, (dim >> 3) & 3
    h, ln = (o >> 2) & 1, 4 * (o >> 3) + (o & 3)
    return (key >> 5) * 4096 + ((h * 2 + (ks >> 1)) * 64 + lg * 16 + ln) * 16 + (ks & 1) * 8 + (dim & 7)


def v8_offset(key: int, ch: int) -> int:
    """Byte offset of (key, channel) inside one (row, kv head) block of the V8 cache."""
    o, dt = key & 31, ch >> 4
    return (key >> 5) * 4096 + ((dt >> 1) * 64 + (o >> 3) * 16 + (ch & 15)) * 16 + (dt & 1) * 8 + (o & 7)
