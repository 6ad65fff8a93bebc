"""Host restatements for the streaming tests: the window codes zk_stream_window must produce (torch, no GPU) and a
brute-force model of the emission rule stream_plan must follow."""
import torch

from oracle import zonos_ref

EOS = 1024


def window_codes_ref(delayed: torch.Tensor, P: int, f0: int, f1: int, upto: int):
    """revert_delay_pattern, the `>= 1024 -> 0` fill and the per-row slice of model.py:437-451 on the window
    [f0, f1) of absolute code frames, frames < upto being final. Returns (codes_w int64 [B][K][f1 - f0],
    lens_w int32 [B], end int32 [B]); reads only columns < upto + K of ``delayed`` [B][K][Ld]."""
    B, K, Ld = delayed.shape
    assert P <= f0 < f1 and 0 <= upto <= Ld - K
    W = f1 - f0
    codes = torch.stack([delayed[:, k, k + 1:k + 1 + upto] for k in range(K)], dim=1)      # frames [0, upto)
    codes_w = torch.zeros(B, K, W, dtype=torch.int64)
    lens_w = torch.zeros(B, dtype=torch.int32)
    end = torch.full((B,), -1, dtype=torch.int32)
    for b in range(B):
        eos_pos = int((codes[b, 0] == EOS).int().argmax()) if upto else 0                  # model.py:439
        end_b = eos_pos if eos_pos else upto                                               # model.py:440, on [0, upto)
        if eos_pos:
            end[b] = eos_pos
        lens_w[b] = min(max(end_b - f0, 0), W)
        hi = min(f1, end_b)
        if hi > f0:
            seg = codes[b, :, f0:hi].clone()
            seg[seg >= 1024] = 0
            codes_w[b, :, :hi - f0] = seg
    return codes_w, lens_w, end


def simulate_stream(P: int, C: int, H: int, uptos: list) -> list:
    """The windows a stream must emit, poll by poll, frame by frame: ``uptos`` are the final-frame counts the polls
    find (the last one is where the loop ended). A chunk [c0, c0 + C) goes out at the first poll whose final frames
    reach c0 + C + H; after the last poll every frame not yet emitted goes out, in chunks of at most C."""
    out, emitted = [], P                   # emitted: the first frame not yet handed out
    for i, upto in enumerate(uptos):
        last = i + 1 == len(uptos)
        wins = []
        while True:
            c0, c1 = emitted, emitted + C
            if c1 + H <= upto:
                pass
            elif last and c0 < upto:
                c1 = min(c1, upto)
            else:
                break
            f0 = c0
            while f0 > P and c0 - f0 < H:   # up to H frames of context, never before the prefix's end
                f0 -= 1
            f1 = c1
            while f1 < upto and f1 - c1 < H:
                f1 += 1
            wins.append((f0, c0, c1, f1))
            emitted = c1
        out.append(wins)
    return out


def delayed_codes(B, T, eos_at, seed=0):
    """Delayed codes of random frames (ids < 1024, MASK and EOS of the EOS protocol in the higher codebooks) with a
    codebook-0 EOS at the frames eos_at[b]."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 1024, (B, 9, T), generator=g)
    codes[:, 1:][torch.rand(B, 8, T, generator=g) < 0.05] = 1025
    codes[:, 1:][torch.rand(B, 8, T, generator=g) < 0.03] = EOS
    for b, frames in enumerate(eos_at):
        for t in frames:
            codes[b, 0, t] = EOS
    return zonos_ref.apply_delay(codes)
