"""Speaker embedding for voice cloning (zonos/speaker_cloning.py) on the HIP kernels of
csrc/speaker.hip: ``SpeakerEmbedding`` (:355-384), ``SpeakerEmbeddingLDA`` (:387-411) and
``logFbankCal`` (:12-34) with the reference's call contract.

The network is ResNet293_SimAM_ASP (``ResNet293_based``, :198-223): log-mel features [B][80][T] ->
stem conv -> four layers of SimAM basic blocks -> attentive statistics pooling -> Linear to 256 ->
(LDA) Linear to 128. Weights come from the reference's two ``.pt`` files in its own state-dict key
layout; the loader infers ``in_planes`` and the blocks per layer from the keys, packs the conv weights
into the kernel's fp16 fragment layout once and turns every eval-mode BatchNorm into an fp32
(scale, shift) pair. torchaudio is not a dependency: the Hann window, the DFT twiddles and the HTK mel
filterbank of ``torchaudio.transforms.MelSpectrogram`` are host-built tables (restated from the
published formulas, unpinned against torchaudio itself), and resampling is ``zonos_amd.audio.resample``.
"""
from __future__ import annotations

import ctypes as C  # noqa: N812
import math
import os

import torch

from . import _lib
from ._lib import SpkBlock, SpkDesc, call, ptr
from .audio import resample
from .utils import DEFAULT_DEVICE, hub_download

SAMPLE_RATE = 16_000
N_FFT, WIN_LENGTH, HOP, N_MELS = 512, 400, 160, 80
BN_EPS = 1e-5
ATT_DIM = 128
SPEAKER_REPO = "Zyphra/Zonos-v0.1-speaker-embedding"
SPEAKER_CKPT = "ResNet293_SimAM_ASP_base.pt"
SPEAKER_LDA = "ResNet293_SimAM_ASP_base_LDA-128.pt"


# ---------------------------------------------------------------- host tables of the log-mel front end
def hann_window_padded() -> torch.Tensor:
    """fp32 [512]: the periodic Hann window of 400 samples, zero-padded centrally to n_fft (torch.stft)."""
    w = torch.hann_window(WIN_LENGTH, periodic=True, dtype=torch.float32)
    left = (N_FFT - WIN_LENGTH) // 2
    return torch.nn.functional.pad(w, (left, N_FFT - WIN_LENGTH - left))


def twiddle_table() -> torch.Tensor:
    """fp64 [512][2]: cos and sin of 2 pi j / 512."""
    a = torch.arange(N_FFT, dtype=torch.float64) * (2.0 * math.pi / N_FFT)
    return torch.stack([a.cos(), a.sin()], 1).contiguous()


def mel_filterbank(n_freqs: int = N_FFT // 2 + 1, f_min: float = 0.0, f_max: float = SAMPLE_RATE / 2,
                   n_mels: int = N_MELS, sample_rate: int = SAMPLE_RATE) -> torch.Tensor:
    """fp32 [n_freqs][n_mels]: triangular filters on the HTK mel scale, no normalisation
    (torchaudio.functional.melscale_fbanks with mel_scale="htk", norm=None)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0).contiguous()


# ---------------------------------------------------------------- weight preparation
def infer_geometry(sd: dict) -> tuple[int, list[int]]:
    """(in_planes, blocks per layer) of a ResNet293_based state dict, from its keys."""
    in_planes = int(sd["front.conv1.weight"].shape[0])
    blocks = []
    for layer in range(1, 5):
        idx = {int(k.split(".")[2]) for k in sd if k.startswith(f"front.layer{layer}.")}
        if not idx or idx != set(range(len(idx))):
            raise ValueError(f"state dict has no contiguous front.layer{layer}.* blocks")
        blocks.append(len(idx))
    return in_planes, blocks


def bn_scale_shift(sd: dict, prefix: str, eps: float = BN_EPS) -> tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm as y = x * scale + shift (fp32, computed in fp64)."""
    w, b = sd[prefix + "weight"].double(), sd[prefix + "bias"].double()
    mean, var = sd[prefix + "running_mean"].double(), sd[prefix + "running_var"].double()
    scale = w / torch.sqrt(var + eps)
    return scale.float().contiguous(), (b - mean * scale).float().contiguous()


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout][Cin][k][k] -> fp16 [ceil(Cout/64)][Cin/32][k*k][64][32], the layout zk_spk_conv2d_cl
    stages per (channel tile, 32-channel chunk); rows past Cout are zero."""
    cout, cin, kh, kw = w.shape
    if cin % 32 or cout % 32:
        raise ValueError(f"conv channel counts must be multiples of 32 (got {cin} -> {cout})")
    cp = (cout + 63) // 64 * 64
    wp = torch.zeros(cp, cin, kh * kw, dtype=torch.float16)
    wp[:cout] = w.reshape(cout, cin, kh * kw).to(torch.float16)
    return wp.reshape(cp // 64, 64, cin // 32, 32, kh * kw).permute(0, 2, 4, 1, 3).contiguous()


def permute_pooling(w1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, channels: int, rows: int):
    """ASP weights from the reference's feature order c * F' + f (the reshape of [B, C, F', T'],
    speaker_cloning.py:53) to the channels-last order f * C + c of the kernels."""
    a = w1.shape[0]
    w1p = w1.reshape(a, channels, rows).permute(0, 2, 1).reshape(a, rows * channels)
    w2p = w2.reshape(channels, rows, a).permute(1, 0, 2).reshape(rows * channels, a)
    b2p = b2.reshape(channels, rows).t().reshape(rows * channels)
    return w1p.contiguous(), w2p.contiguous(), b2p.contiguous()


def out_dim(n: int, stride: int) -> int:
    return (n - 1) // stride + 1


def _find(path: str | None, filename: str) -> str:
    """Explicit path, then $ZONOS_SPEAKER_PATH/<filename>, then the local Hugging Face cache."""
    if path:
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found (or set ZONOS_SPEAKER_PATH to the directory holding "
                                    f"{SPEAKER_CKPT} and {SPEAKER_LDA})")
        return path
    d = os.environ.get("ZONOS_SPEAKER_PATH")
    if d:
        p = os.path.join(d, filename)
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} not found (ZONOS_SPEAKER_PATH={d})")
        return p
    try:
        return hub_download(repo_id=SPEAKER_REPO, filename=filename)
    except Exception as e:
        raise FileNotFoundError(f"{filename} of {SPEAKER_REPO} is not in the local Hugging Face cache; set "
                                f"ZONOS_SPEAKER_PATH to the directory holding it") from e


def log_fbank(wav16k: torch.Tensor, window: torch.Tensor, twiddle: torch.Tensor, melfb: torch.Tensor) -> torch.Tensor:
    """zk_spk_logfbank: fp32 [B][n] at 16 kHz on the GPU -> fp32 [B][80][1 + n // 160] (tables on the same GPU)."""
    _lib.require_gpu(wav16k, "wav")
    wav16k = wav16k.to(torch.float32).contiguous()
    if wav16k.ndim != 2:
        raise ValueError(f"wav must be [B][n] (got {tuple(wav16k.shape)})")
    B, n = wav16k.shape
    out = torch.empty(B, N_MELS, 1 + n // HOP, device=wav16k.device)
    call("zk_spk_logfbank", ptr(wav16k), B, n, ptr(window), ptr(twiddle), ptr(melfb), N_MELS, ptr(out),
         _lib.stream_ptr(wav16k.device))
    return out


class SpeakerNet:
    """The network on the GPU: weights in kernel layout, the descriptor of zk_speaker_embed, and the
    same launch sequence issued from Python (``c_step=False``; it can also start from features and
    return every stage, which is what the parity tests read)."""

    def __init__(self, state_dict: dict, lda_state_dict: dict | None, device):
        self.device = torch.device(device)
        sd = state_dict
        self.in_planes, self.blocks_per_layer = infer_geometry(sd)
        if self.in_planes % 32:
            raise ValueError(f"in_planes must be a multiple of 32 (got {self.in_planes})")
        dev = self.device

        def put(t, dtype=torch.float32):
            return t.to(dtype).contiguous().to(dev)

        self.window, self.twiddle = put(hann_window_padded()), put(twiddle_table(), torch.float64)
        self.melfb = put(mel_filterbank())
        self.stem_w = put(sd["front.conv1.weight"].reshape(self.in_planes, 9))
        self.stem_scale, self.stem_shift = (put(t) for t in bn_scale_shift(sd, "front.bn1."))
        self.blocks = []
        cin, rows = self.in_planes, N_MELS
        for layer, nb in enumerate(self.blocks_per_layer, 1):
            cout = self.in_planes << (layer - 1)
            for i in range(nb):
                p = f"front.layer{layer}.{i}."
                stride = 2 if (layer > 1 and i == 0) else 1
                blk = dict(cin=cin, cout=cout, stride=stride, layer=layer,
                           w1=put(pack_conv_weight(sd[p + "conv1.weight"]), torch.float16),
                           w2=put(pack_conv_weight(sd[p + "conv2.weight"]), torch.float16), wd=None)
                blk["scale1"], blk["shift1"] = (put(t) for t in bn_scale_shift(sd, p + "bn1."))
                blk["scale2"], blk["shift2"] = (put(t) for t in bn_scale_shift(sd, p + "bn2."))
                if p + "downsample.0.weight" in sd:
                    blk["wd"] = put(pack_conv_weight(sd[p + "downsample.0.weight"]), torch.float16)
                    blk["scaled"], blk["shiftd"] = (put(t) for t in bn_scale_shift(sd, p + "downsample.1."))
                if (stride != 1 or cin != cout) != (blk["wd"] is not None):
                    raise ValueError(f"{p}: downsample weights do not match the block's shape change")
                self.blocks.append(blk)
                cin, rows = cout, out_dim(rows, stride)
        self.c_last, self.f_last = cin, rows
        self.pool_dim = cin * rows
        w1, w2 = sd["pooling.attention.0.weight"], sd["pooling.attention.3.weight"]
        if w1.shape[0] != ATT_DIM or w1.shape[1] != self.pool_dim:
            raise ValueError(f"pooling.attention.0.weight is {tuple(w1.shape)}, expected ({ATT_DIM}, {self.pool_dim}, 1)")
        w1p, w2p, b2p = permute_pooling(w1.float().reshape(ATT_DIM, -1), w2.float().reshape(-1, ATT_DIM),
                                        sd["pooling.attention.3.bias"].float(), cin, rows)
        self.asp_w1, self.asp_w2, self.asp_b2 = put(w1p), put(w2p), put(b2p)
        self.asp_b1 = put(sd["pooling.attention.0.bias"])
        self.asp_bn_scale, self.asp_bn_shift = (put(t) for t in bn_scale_shift(sd, "pooling.attention.2."))
        self.bott_w, self.bott_b = put(sd["bottleneck.weight"]), put(sd["bottleneck.bias"])
        self.emb_dim = self.bott_w.shape[0]
        if lda_state_dict is None:      # SpeakerEmbedding alone: a 1-wide zero projection, result dropped
            lda_state_dict = {"weight": torch.zeros(1, self.emb_dim), "bias": torch.zeros(1)}
        self.lda_w, self.lda_b = put(lda_state_dict["weight"]), put(lda_state_dict["bias"])
        self.lda_dim = self.lda_w.shape[0]
        self._desc = self._descriptor()
        self._ws = None

    def _descriptor(self) -> SpkDesc:
        arr = (SpkBlock * len(self.blocks))()
        for a, b in zip(arr, self.blocks):
            a.cin, a.cout, a.stride = b["cin"], b["cout"], b["stride"]
            for n in ("w1", "scale1", "shift1", "w2", "scale2", "shift2"):
                setattr(a, n, ptr(b[n]))
            if b["wd"] is not None:
                a.wd, a.scaled, a.shiftd = ptr(b["wd"]), ptr(b["scaled"]), ptr(b["shiftd"])
        self._block_array = arr            # the descriptor points into it
        d = SpkDesc(n_mels=N_MELS, c0=self.in_planes, nblocks=len(self.blocks), pool_dim=self.pool_dim,
                    att_dim=ATT_DIM, emb_dim=self.emb_dim, lda_dim=self.lda_dim)
        d.blocks = C.cast(arr, C.c_void_p)
        for n in ("window", "twiddle", "melfb", "stem_w", "stem_scale", "stem_shift", "asp_w1", "asp_b1",
                  "asp_bn_scale", "asp_bn_shift", "asp_w2", "asp_b2", "bott_w", "bott_b", "lda_w", "lda_b"):
            setattr(d, n, ptr(getattr(self, n)))
        return d

    # -------------------------------------------------------------- launches
    def features(self, wav16k: torch.Tensor) -> torch.Tensor:
        """logFbankCal: fp32 [B][n] at 16 kHz -> fp32 [B][80][1 + n // 160]."""
        return log_fbank(wav16k, self.window, self.twiddle, self.melfb)

    def forward_features(self, feat: torch.Tensor, stages: dict | None = None):
        """The per-kernel sequence from features fp32 [B][80][T]: (emb [B][256], lda [B][128]).
        ``stages`` (a dict) receives the fp32 activations [B][F][T][C] after the stem ("stem") and after
        each layer ("layer1".."layer4") and the pooled vector ("pooled")."""
        _lib.require_gpu(feat, "features")
        feat = feat.to(torch.float32).contiguous()
        dev, st = feat.device, _lib.stream_ptr(feat.device)
        B, F, T = feat.shape
        if F != N_MELS:
            raise ValueError(f"features must have {N_MELS} mel bins (got {F})")
        x = torch.empty(B, F, T, self.in_planes, device=dev)
        s = torch.empty(B, F, T, self.in_planes, device=dev, dtype=torch.float16)
        call("zk_spk_stem", ptr(feat), B, F, T, ptr(self.stem_w), ptr(self.stem_scale), ptr(self.stem_shift),
             self.in_planes, ptr(x), ptr(s), st)
        if stages is not None:
            stages["stem"] = x.clone()
        lib = _lib.load()
        for i, b in enumerate(self.blocks):
            cin, cout, stride = b["cin"], b["cout"], b["stride"]
            Fo, To = out_dim(F, stride), out_dim(T, stride)
            h = torch.empty(B, Fo, To, cout, device=dev, dtype=torch.float16)
            call("zk_spk_conv2d_cl", ptr(s), B, cin, F, T, ptr(b["w1"]), cout, 3, stride, ptr(b["scale1"]),
                 ptr(b["shift1"]), 1, ptr(h), None, None, st)
            shortcut = x
            if b["wd"] is not None:
                shortcut = torch.empty(B, Fo, To, cout, device=dev)
                call("zk_spk_conv2d_cl", ptr(s), B, cin, F, T, ptr(b["wd"]), cout, 1, stride, ptr(b["scaled"]),
                     ptr(b["shiftd"]), 0, None, ptr(shortcut), None, st)
            y = torch.empty(B, Fo, To, cout, device=dev)
            stats = torch.empty(B, lib.zk_spk_conv_tiles(Fo, To), 3, cout, device=dev)
            call("zk_spk_conv2d_cl", ptr(h), B, cout, Fo, To, ptr(b["w2"]), cout, 3, 1, ptr(b["scale2"]),
                 ptr(b["shift2"]), 0, None, ptr(y), ptr(stats), st)
            moments = torch.empty(B, 2, cout, device=dev)
            xo = x if b["wd"] is None else torch.empty(B, Fo, To, cout, device=dev)
            so = torch.empty(B, Fo, To, cout, device=dev, dtype=torch.float16)
            call("zk_spk_simam", ptr(y), B, cout, Fo, To, ptr(stats), ptr(shortcut), ptr(moments), ptr(xo), ptr(so),
                 st)
            x, s, F, T = xo, so, Fo, To
            last = i + 1 == len(self.blocks) or self.blocks[i + 1]["layer"] != b["layer"]
            if stages is not None and last:
                stages[f"layer{b['layer']}"] = x.clone()
        hidden = torch.empty(B, T, ATT_DIM, device=dev)
        pooled = torch.empty(B, 2 * self.pool_dim, device=dev)
        call("zk_spk_asp", ptr(x), B, self.c_last, F, T, ptr(self.asp_w1), ptr(self.asp_b1), ptr(self.asp_bn_scale),
             ptr(self.asp_bn_shift), ptr(self.asp_w2), ptr(self.asp_b2), ATT_DIM, ptr(hidden), ptr(pooled), st)
        if stages is not None:
            stages["pooled"] = pooled.clone()
        emb = torch.empty(B, self.emb_dim, device=dev)
        lda = torch.empty(B, self.lda_dim, device=dev)
        call("zk_spk_head", ptr(pooled), B, 2 * self.pool_dim, ptr(self.bott_w), ptr(self.bott_b), self.emb_dim,
             ptr(self.lda_w), ptr(self.lda_b), self.lda_dim, ptr(emb), ptr(lda), st)
        return emb, lda

    def workspace_bytes(self, B: int, n: int) -> int:
        lib = _lib.load()
        size = lib.zk_speaker_workspace_bytes(C.byref(self._desc), B, n)
        if size == 0:
            raise _lib.ZonosHipError(lib.zk_last_error().decode())
        return size

    def embed(self, wav16k: torch.Tensor, c_step: bool = True):
        """fp32 [B][n] at 16 kHz (equal-length clips) -> (emb [B][256], lda [B][128]), one C call
        (zk_speaker_embed) or, with ``c_step=False``, the same launches issued from Python."""
        _lib.require_gpu(wav16k, "wav")
        wav16k = wav16k.to(torch.float32).contiguous()
        if not c_step:
            return self.forward_features(self.features(wav16k))
        B, n = wav16k.shape
        size = self.workspace_bytes(B, n)
        if self._ws is None or self._ws.numel() < size or self._ws.device != wav16k.device:
            self._ws = torch.empty(size, dtype=torch.uint8, device=wav16k.device)
        emb = torch.empty(B, self.emb_dim, device=wav16k.device)
        lda = torch.empty(B, self.lda_dim, device=wav16k.device)
        call("zk_speaker_embed", C.byref(self._desc), ptr(wav16k), B, n, ptr(self._ws), self._ws.numel(), ptr(emb),
             ptr(lda), _lib.stream_ptr(wav16k.device))
        return emb, lda


class logFbankCal:  # noqa: N801  (the reference's name)
    """speaker_cloning.py:12-34 on the GPU: [B][n] 16 kHz -> log-mel minus its mean over time [B][80][T]."""

    def __init__(self, device=DEFAULT_DEVICE):
        self.device = torch.device(device)
        self.window = hann_window_padded().to(self.device)
        self.twiddle = twiddle_table().to(self.device)
        self.melfb = mel_filterbank().to(self.device)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return log_fbank(x.to(self.device), self.window, self.twiddle, self.melfb)

    __call__ = forward


class SpeakerEmbedding:
    """speaker_cloning.py:355-384. ``forward(wav, sample_rate)`` -> emb fp32 [1][256]."""

    def __init__(self, ckpt_path: str | None = None, device=DEFAULT_DEVICE, *, lda_state_dict: dict | None = None,
                 c_step: bool = True):
        self.device = torch.device(device)
        self.c_step = c_step
        path = _find(ckpt_path, SPEAKER_CKPT)
        state_dict = torch.load(path, weights_only=True, map_location="cpu")
        self.model = SpeakerNet(state_dict, lda_state_dict, self.device)

    @property
    def dtype(self):
        return torch.float32

    def prepare_input(self, wav: torch.Tensor, sample_rate: int) -> torch.Tensor:
        """:375-380: channel mean of a 2-D wav, then resampling to 16 kHz -> [1][n] on the GPU."""
        if wav.ndim >= 3:
            raise ValueError(f"wav must have fewer than 3 dimensions (got {wav.ndim})")
        wav = wav.to(self.device, torch.float32)
        wav = wav.mean(0, keepdim=True) if wav.ndim == 2 else wav.unsqueeze(0)
        return resample(wav, int(sample_rate), SAMPLE_RATE)

    def _both(self, wav: torch.Tensor, sample_rate: int):
        return self.model.embed(self.prepare_input(wav, sample_rate), c_step=self.c_step)

    def forward(self, wav: torch.Tensor, sample_rate: int) -> torch.Tensor:
        return self._both(wav, sample_rate)[0]

    __call__ = forward


class SpeakerEmbeddingLDA:
    """speaker_cloning.py:387-411. ``forward(wav, sample_rate)`` -> (emb [1][256], lda [1][128]) fp32.
    The two checkpoint files are found by explicit path, then in $ZONOS_SPEAKER_PATH, then in the local
    Hugging Face cache."""

    def __init__(self, device=DEFAULT_DEVICE, spk_model_path: str | None = None, lda_path: str | None = None,
                 c_step: bool = True):
        self.device = torch.device(device)
        spk = _find(spk_model_path, SPEAKER_CKPT)
        lda_sd = torch.load(_find(lda_path, SPEAKER_LDA), weights_only=True, map_location="cpu")
        self.model = SpeakerEmbedding(spk, self.device, lda_state_dict=lda_sd, c_step=c_step)

    def forward(self, wav: torch.Tensor, sample_rate: int):
        return self.model._both(wav, sample_rate)

    __call__ = forward
