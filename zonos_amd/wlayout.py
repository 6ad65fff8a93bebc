"""Host-side view of the FP8 (e4m3fn) weight format of the small-batch decode GEMVs (gemm.hip: the
WsE4m3 weight stream of gemv_body, entry kernel k_gemv_w8; generate(weight_dtype="fp8")).

Format: a weight W[N][K] (nn.Linear order, bf16) becomes OCP e4m3fn bytes with one power-of-two scale per
output row n, stored as its biased exponent byte b (E8M0, scale 2^(b-127)). The scale rule is
kvlayout.kv_scale_exponent applied to the row's amax over all K (the smallest e with amax * 2^-e <= 448,
clamped to [-126, 127], e = 0 for a zero row); byte = RNE e4m3fn(w * 2^-e). e4m3 is itself floating point, so
a row-wide scale keeps what a finer group would; a dequantised value q * 2^e has 4 significant bits and is
exact in bf16 (as long as it is a normal bf16 number: rows whose amax lies below 2^-117 are outside the format's
use).

Packed image (what the kernel streams), K % 64 == 0, rows padded to Npad = ceil64(N) as zk_pack_weights pads:
  bytes [Npad/16 tiles][K/64 pairs][lane 64][q 2][8]
      lane = 16*lg + ln holds row 16*tile + ln, columns 64*pair + 32*q + 8*lg .. +8
  i.e. the bf16 fragment order ([N/16][K/32][64][8]) with the two k-steps 2*pair + q of a pair side by side in
  one lane, so every weight load fetches 16 B per lane and a wave 1 KB of one tile's row run. The half-tile
  form of the kernel (8 columns per workgroup) has the lanes of the other half read the NEXT pair at their
  neighbour's position (lane ^ 8), so its loads fetch 1 KB of the workgroup's own 8 rows, four k-steps each.
  scales uint8 [Npad] in row order.
Rows N..Npad are zero bytes with scale byte 127.
"""
from __future__ import annotations

import torch

from .kvlayout import kv_scale_exponent


def quantize_w_e4m3(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[N][K] bf16 / fp32 -> (e4m3fn bytes uint8 [N][K], scale bytes uint8 [N])."""
    wf = w.float()
    e = kv_scale_exponent(wf.abs().amax(dim=-1))
    q = torch.ldexp(wf, (-e).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), (e + 127).to(torch.uint8)


def dequantize_w_e4m3(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Inverse view of quantize_w_e4m3: bytes [N][K] and scale bytes [N] -> bf16 [N][K] (exact)."""
    e = scale.to(torch.int32) - 127
    return torch.ldexp(q.view(torch.float8_e4m3fn).float(), e.unsqueeze(-1)).to(torch.bfloat16)


def padded_rows(N: int) -> int:
    return (N + 63) // 64 * 64


def pack_w8(q: torch.Tensor, scale: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bytes [N][K] (K % 64 == 0), scale bytes [N] -> (packed image uint8 [Npad * K], scale bytes [Npad])."""
    N, K = q.shape
    assert K % 64 == 0 and scale.shape == (N,)
    Np = padded_rows(N)
    qp = torch.zeros(Np, K, dtype=torch.uint8, device=q.device)
    qp[:N] = q
    sp = torch.full((Np,), 127, dtype=torch.uint8, device=q.device)
    sp[:N] = scale
    # n = 16*tile + ln ; k = 64*pair + 32*q + 8*lg + e
    x = qp.reshape(Np // 16, 16, K // 64, 2, 4, 8)             # tile ln | pair q lg e
    x = x.permute(0, 2, 4, 1, 3, 5)                            # tile pair lg ln q e  (lane = 16lg + ln)
    return x.reshape(Np * K).contiguous(), sp


def unpack_w8(image: torch.Tensor, scale_p: torch.Tensor, N: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Inverse of pack_w8: (bytes [N][K], scale bytes [N]) of the first N rows."""
    Np = scale_p.shape[0]
    K = image.numel() // Np
    x = image.reshape(Np // 16, K // 64, 4, 16, 2, 8)          # tile pair lg ln q e
    x = x.permute(0, 3, 1, 4, 2, 5)                            # tile ln pair q lg e
    return x.reshape(Np, K)[:N].contiguous(), scale_p[:N].contiguous()


def w8_offset(n: int, k: int, K: int) -> int:
    """Byte offset of W[n][k] inside the packed image of a weight with K columns."""
    return ((n >> 4) * (K >> 6) + (k >> 6)) * 1024 + (((k >> 3) & 3) * 16 + (n & 15)) * 16 + ((k >> 5) & 1) * 8 + (k & 7)
