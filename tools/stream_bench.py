"""Streaming measurements on the benchmark's workloads (bench.py's synthetic weights, EOS disabled, CLI sampling):

    python tools/stream_bench.py [--configs c2,c3] [--chunk-frames 16,64] [--rounds 2] [--out FILE]

c2 = B 1, Lc 160, no prefix, 861 new tokens; c3 = B 64, Lc 400, prefix 10, 2580 new tokens. Per config and chunk
size, after one warm-up call of each mode, the two modes alternate for --rounds rounds:

  stream : HipDecoder.stream() to exhaustion (chunks copied to the host through the pinned buffer);
  parent : HipDecoder.generate() + HipDacDecoder.decode_list(codes), the path without streaming.

Reported per round, one line each (also appended to --out):
  (a) time to the first chunk on the host (from the call; the chunk's copy event has completed), beside the prefill
      time (the call up to the prefill's completion, measured in the second warm-up call) and the model
      prefill + (C + H + 9) step_ms + window decode, step_ms being the mean step time between this run's first and
      last chunk that came out of the loop; the gap to the model is reported, not bounded;
  (b) total wall time and codes/s of both modes;
  (c) the window decodes' device time (HIP events on the second stream): mean and max per window."""
from __future__ import annotations

import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

CONFIGS = {"c2": dict(B=1, Lc=160, P=0, new=861), "c3": dict(B=64, Lc=400, P=10, new=2580)}
SP = dict(top_p=0, top_k=0, min_p=0, linear=0.65, conf=0.4, quad=0.0, repetition_penalty=2.5,
          repetition_penalty_window=8, temperature=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--chunk-frames", default="16,64")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from zonos_amd import synthetic
    from zonos_amd.autoencoder import DacSpec, HipDacDecoder
    from zonos_amd.engine import EngineConfig, HipDecoder
    dev = torch.device("cuda", 0)
    mc = dict(synthetic.ZONOS_V01, n_layer=args.layers)
    eng = HipDecoder(EngineConfig(**mc), synthetic.backbone_weights(dev, seed=0, **mc), dev)
    dac = HipDacDecoder(DacSpec(), synthetic.dac_weights(dev), dev)
    H, hop = dac.spec.halo_frames, dac.spec.hop_length
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    def now():
        return time.perf_counter()

    for name in args.configs.split(","):
        c = CONFIGS[name]
        B, new = c["B"], c["new"]
        cond = synthetic.conditioning(B, c["Lc"], mc["d_model"], seed=1, device=dev)
        prefix = synthetic.prefix_codes(B, c["P"], seed=3, device=dev) if c["P"] else None
        gen_args = (cond, prefix, new, 2.0, B, SP)

        def parent(seed):
            torch.cuda.synchronize(dev)
            t0 = now()
            codes = eng.generate(*gen_args, seed=seed, force_full_length=True)
            torch.cuda.synchronize(dev)
            t1 = now()
            wavs = dac.decode_list(codes)
            torch.cuda.synchronize(dev)
            t2 = now()
            return dict(total=t2 - t0, gen=t1 - t0, frames=sum(int(x.shape[1]) for x in codes), samples=sum(
                int(w.shape[-1]) for w in wavs))

        def stream(seed, C, measure_prefill=False):
            torch.cuda.synchronize(dev)
            t0 = now()
            it = eng.stream(*gen_args, seed=seed, force_full_length=True, autoencoder=dac, chunk_frames=C)
            prefill = None
            if measure_prefill:
                torch.cuda.synchronize(dev)
                prefill = now() - t0
            ev = it._run.streamer.decode_events = []
            marks, samples = [], 0
            for ch in it:
                marks.append((now() - t0, it.steps))
                samples += sum(int(w.shape[1]) for w in ch.wavs)
            torch.cuda.synchronize(dev)
            total = now() - t0
            win = [a.elapsed_time(b) for a, b in ev]
            loop = [m for m in marks if m[1] < marks[-1][1]]            # chunks that came out of the loop
            step_ms = ((loop[-1][0] - loop[0][0]) / (loop[-1][1] - loop[0][1]) * 1e3) if len(loop) > 1 else float("nan")
            return dict(total=total, first=marks[0][0], first_steps=marks[0][1], chunks=len(marks), step_ms=step_ms,
                        frames=sum(int(x.shape[1]) for x in it.codes), samples=samples, prefill=prefill,
                        win_mean=sum(win) / len(win), win_max=max(win), win_first=win[0], windows=len(win))

        for C in (int(x) for x in args.chunk_frames.split(",")):
            stream(99, C)                                  # the first call at a shape allocates its workspace
            warm = stream(99, C, measure_prefill=True)
            parent(99)
            prefill_ms = warm["prefill"] * 1e3
            emit(f"# {name} B={B} Lc={c['Lc']} P={c['P']} new={new} chunk_frames={C} H={H}: prefill (call -> prefill done, "
                 f"warm-up call) {prefill_ms:.1f} ms")
            for r in range(args.rounds):
                s = stream(1000 + r, C)
                p = parent(1000 + r)
                assert s["frames"] == p["frames"] and s["samples"] == p["samples"] == s["frames"] * hop
                model = prefill_ms + (C + H + 9) * s["step_ms"] + s["win_first"]
                emit(f"{name} C={C} round {r} (a) first chunk {s['first'] * 1e3:.1f} ms after the call (at step "
                     f"{s['first_steps']}); model prefill + (C+H+9) x {s['step_ms']:.3f} ms + window {s['win_first']:.2f} ms = "
                     f"{model:.1f} ms; gap {s['first'] * 1e3 - model:+.1f} ms")
                emit(f"{name} C={C} round {r} (b) stream total {s['total'] * 1e3:.1f} ms = {s['frames'] * 9 / s['total']:.0f} "
                     f"codes/s ({s['chunks']} chunks); generate + decode_list {p['total'] * 1e3:.1f} ms = "
                     f"{p['frames'] * 9 / p['total']:.0f} codes/s (generate {p['gen'] * 1e3:.1f} ms); stream / parent = "
                     f"{s['total'] / p['total']:.4f}")
                emit(f"{name} C={C} round {r} (c) window decode: mean {s['win_mean']:.3f} ms, max {s['win_max']:.3f} ms over "
                     f"{s['windows']} windows (sum {s['win_mean'] * s['windows']:.1f} ms)")
    eng.release()


if __name__ == "__main__":
    main()
