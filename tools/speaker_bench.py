"""Time the speaker-embedding network (zonos_amd/speaker.py) on synthetic 10 s and 30 s clips and the
same network composed from torch.nn.functional.conv2d on the same GPU, in fp32 and in fp16.

    python tools/speaker_bench.py [--seconds 10 30] [--reps 5] [--out profiles/speaker_bench.txt]

Weights are zonos_amd.synthetic.speaker_state_dict at the real geometry (in_planes 64, blocks
[10, 20, 64, 3]); the two checkpoint files are written to a temporary directory and found through
ZONOS_SPEAKER_PATH, so the timed object is the public ``SpeakerEmbeddingLDA``. Times are HIP events
around whole calls (resampling is skipped: the clip is already 16 kHz), after warm-up of the same shape,
median and min / max of ``--reps`` calls. The per-layer split is taken from the Python-issued launch
sequence with an event at every stage boundary. GFLOP/s counts the convolutions' multiply-adds only
(2 * taps * Cin * Cout per output position), computed from the shapes. There is no CPU fallback: the
tool fails without a GPU.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zonos_amd import speaker  # noqa: E402
from zonos_amd.synthetic import speaker_state_dict  # noqa: E402


def conv_flops(net, T: int) -> float:
    rows, fl = 80, 2.0 * 9 * net.in_planes * 80 * T
    for b in net.blocks:
        ro, to = speaker.out_dim(rows, b["stride"]), speaker.out_dim(T, b["stride"])
        fl += 2.0 * ro * to * b["cout"] * (9 * b["cin"] + 9 * b["cout"] + (b["cin"] if b["wd"] is not None else 0))
        rows, T = ro, to
    return fl


def timed(fn, reps: int, warmup: int = 2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


class StageEvents(dict):
    """Passed as ``stages``: records an event whenever the launch sequence reaches a stage boundary."""

    def __init__(self):
        super().__init__()
        self.events = []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append((name, e))

    def __setitem__(self, k, v):
        self.mark(k)


class TorchNet:
    """The same network from torch ops (NCHW conv2d, eval-mode BatchNorm as scale / shift)."""

    def __init__(self, sd, lda, dtype, device):
        self.dtype = dtype
        self.sd = {k: v.to(device, dtype if v.is_floating_point() else v.dtype) for k, v in sd.items()}
        self.lda = {k: v.to(device, dtype) for k, v in lda.items()}
        self.in_planes, self.blocks = speaker.infer_geometry(sd)
        self.bn = {}
        for k in sd:
            if k.endswith("running_mean"):
                p = k[:-len("running_mean")]
                s, b = speaker.bn_scale_shift(sd, p)
                self.bn[p] = (s.to(device, dtype).view(1, -1, 1, 1), b.to(device, dtype).view(1, -1, 1, 1))

    def _bn(self, x, p):
        s, b = self.bn[p]
        return x * s + b

    def __call__(self, feat):
        sd = self.sd
        x = feat.to(self.dtype).unsqueeze(1)
        x = torch.relu(self._bn(F.conv2d(x, sd["front.conv1.weight"], padding=1), "front.bn1."))
        for layer, nb in enumerate(self.blocks, 1):
            for i in range(nb):
                p = f"front.layer{layer}.{i}."
                stride = 2 if (layer > 1 and i == 0) else 1
                out = torch.relu(self._bn(F.conv2d(x, sd[p + "conv1.weight"], stride=stride, padding=1), p + "bn1."))
                out = self._bn(F.conv2d(out, sd[p + "conv2.weight"], padding=1), p + "bn2.")
                n = out.shape[2] * out.shape[3] - 1
                d = (out - out.mean(dim=[2, 3], keepdim=True)).pow(2)
                v = d.sum(dim=[2, 3], keepdim=True) / n
                out = out * torch.sigmoid(d / (4 * (v + 1e-4)) + 0.5)
                if p + "downsample.0.weight" in sd:
                    x = self._bn(F.conv2d(x, sd[p + "downsample.0.weight"], stride=stride), p + "downsample.1.")
                x = torch.relu(out + x)
        x = x.reshape(x.shape[0], -1, x.shape[-1])
        s, b = self.bn["pooling.attention.2."]
        h = torch.relu(F.conv1d(x, sd["pooling.attention.0.weight"], sd["pooling.attention.0.bias"]))
        w = torch.softmax(F.conv1d(h * s.view(1, -1, 1) + b.view(1, -1, 1), sd["pooling.attention.3.weight"],
                                   sd["pooling.attention.3.bias"]), dim=2)
        mu = torch.sum(x * w, dim=2)
        sg = torch.sqrt((torch.sum((x ** 2) * w, dim=2) - mu ** 2).clamp(min=1e-5))
        emb = F.linear(torch.cat((mu, sg), 1), sd["bottleneck.weight"], sd["bottleneck.bias"])
        return emb, F.linear(emb, self.lda["weight"], self.lda["bias"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 30.0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--in-planes", type=int, default=64)
    ap.add_argument("--blocks", type=int, nargs=4, default=[10, 20, 64, 3])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speaker_bench: no GPU (there is no CPU fallback)")
    dev = "cuda"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd, lda = speaker_state_dict(a.in_planes, a.blocks, seed=0)
    with tempfile.TemporaryDirectory() as d:
        torch.save(sd, os.path.join(d, speaker.SPEAKER_CKPT))
        torch.save(lda, os.path.join(d, speaker.SPEAKER_LDA))
        os.environ["ZONOS_SPEAKER_PATH"] = d
        model = speaker.SpeakerEmbeddingLDA(device=dev)
    net = model.model.model
    say(f"# speaker_bench: {torch.cuda.get_device_name(0)}, in_planes {a.in_planes}, blocks {a.blocks}, "
        f"reps {a.reps} (median [min, max] ms per call, HIP events)")
    for sec in a.seconds:
        n = int(sec * 16000)
        g = torch.Generator().manual_seed(int(sec))
        wav = (0.1 * torch.randn(1, n, generator=g)).to(dev)
        T = 1 + n // 160
        gf = conv_flops(net, T) / 1e9
        med, lo, hi = timed(lambda: model(wav[0], 16000), a.reps)
        say(f"clip {sec:g} s (T = {T}, {gf:.0f} conv GFLOP): hip SpeakerEmbeddingLDA {med:.2f} [{lo:.2f}, {hi:.2f}] ms"
            f" = {gf / med:.1f} conv TFLOP/s")
        feat = net.features(wav)
        ev = StageEvents()
        net.forward_features(feat)
        torch.cuda.synchronize()
        ev.mark("start")
        net.forward_features(feat, ev)
        ev.mark("head")
        torch.cuda.synchronize()
        split = [f"{name} {ev.events[i][1].elapsed_time(e):.2f}" for i, (name, e) in enumerate(ev.events[1:])]
        say(f"clip {sec:g} s: hip stage split, ms (python-issued sequence): " + ", ".join(split))
        ref_emb = None
        for dtype, name in ((torch.float32, "fp32"), (torch.float16, "fp16")):
            tn = TorchNet(sd, lda, dtype, dev)
            med_t, lo_t, hi_t = timed(lambda: tn(feat), a.reps)
            emb_t = tn(feat)[0].float()
            say(f"clip {sec:g} s: torch conv2d composition {name} {med_t:.2f} [{lo_t:.2f}, {hi_t:.2f}] ms"
                f" = {gf / med_t:.1f} conv TFLOP/s; hip / torch time {med / med_t:.2f}")
            if ref_emb is None:
                ref_emb = emb_t
                emb_h = model(wav[0], 16000)[0]
                rel = float((emb_h - ref_emb).norm() / ref_emb.norm())
                say(f"clip {sec:g} s: hip embedding vs torch fp32 composition, relative error {rel:.2e}")
            del tn
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
