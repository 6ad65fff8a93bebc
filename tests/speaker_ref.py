"""CPU restatement of the speaker network's front end and gate, independent of the engine's code.

``log_fbank`` restates logFbankCal (zonos/speaker_cloning.py:12-34), i.e. torchaudio's
MelSpectrogram(sample_rate 16000, n_fft 512, win_length 400, hop_length 160, n_mels 80) with its
defaults -- periodic Hann window, center=True with reflect padding, power 2, f_min 0, f_max sr/2, HTK
mel scale, no filter normalisation -- as torch.stft plus the published melscale_fbanks formula, then
log(x + 1e-6) and the removal of the mean over time. torchaudio is absent from this environment, so
this restatement (not torchaudio itself) is what the kernel is pinned to.
"""
from __future__ import annotations

import math

import torch


def htk_hz_to_mel(f: float) -> float:
    return 2595.0 * math.log10(1.0 + f / 700.0)


def htk_mel_to_hz(m):
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


def melscale_fbanks(n_freqs=257, f_min=0.0, f_max=8000.0, n_mels=80, sample_rate=16000, dtype=torch.float32):
    """[n_freqs][n_mels] triangular filters, HTK scale, norm=None."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_pts = torch.linspace(htk_hz_to_mel(f_min), htk_hz_to_mel(f_max), n_mels + 2, dtype=dtype)
    f_pts = htk_mel_to_hz(m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(down, up))


def log_fbank(wav: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """wav [B][n] at 16 kHz -> [B][80][1 + n // 160] in ``dtype`` (the filterbank is built in fp32, as
    torchaudio builds it, and cast)."""
    x = wav.to(dtype)
    window = torch.hann_window(400, periodic=True, dtype=torch.float32).to(dtype)
    spec = torch.stft(x, n_fft=512, hop_length=160, win_length=400, window=window, center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2                         # [B][257][T]
    fb = melscale_fbanks().to(dtype)
    mel = torch.matmul(power.transpose(-1, -2), fb).transpose(-1, -2)
    out = torch.log(mel + 1e-6)
    return out - out.mean(dim=2, keepdim=True)


def simam_block_tail(X: torch.Tensor, shortcut: torch.Tensor, lambda_p: float = 1e-4) -> torch.Tensor:
    """relu(SimAM(X) + shortcut) on [B][C][F][T] (speaker_cloning.py:85-95), in X's dtype."""
    n = X.shape[2] * X.shape[3] - 1
    d = (X - X.mean(dim=[2, 3], keepdim=True)).pow(2)
    v = d.sum(dim=[2, 3], keepdim=True) / n
    return torch.relu(X * torch.sigmoid(d / (4 * (v + lambda_p)) + 0.5) + shortcut)
