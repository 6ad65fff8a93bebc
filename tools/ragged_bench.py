"""What a ragged request batch costs and saves: c3 geometry (Zonos-v0.1-transformer, B = 64, prefix 10, 30 s budgets
of 2580 tokens, EOS disabled so every run takes the same steps, bench.py's synthetic weights and CLI sampling) with
conditioning lengths spread over 100..400 (LCS below, mean 250).

  ragged : generate_requests(reqs, ragged=True) -- every row at its own KV position, no pad key read
  padded : the same requests with every conditioning zero-padded to the longest, through the uniform rows path.
           The only thing a caller could do before, and other audio: the pad tokens are attended to.

    python tools/ragged_bench.py                      # both paths interleaved, twice each after a warm-up of each
    python tools/ragged_bench.py --only ragged --new-tokens 300   # one path, one run: the command to put behind
    python tools/ragged_bench.py --only padded --new-tokens 300   #   rocprofv3 --kernel-trace --stats -- (its own run)
    python tools/ragged_bench.py --attn-stats DIR     # the attention kernels' rows of a rocprofv3 kernel_stats.csv

Prints one JSON line. The prefill of the ragged path runs over Lc_max positions for every row (not measured apart:
it is one pass of 2588 steps)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# 64 conditioning lengths, fixed: 16 values spread over 100..400, each four times, in a fixed shuffled order
LCS = [(100 + 20 * ((7 * i) % 16)) for i in range(64)]
assert min(LCS) == 100 and max(LCS) == 400 and sum(LCS) == 64 * 250
PREFIX, NEW, SP = 10, 2580, dict(top_p=0, top_k=0, min_p=0, linear=0.65, conf=0.4, quad=0.0, repetition_penalty=2.5,
                                 repetition_penalty_window=8, temperature=1.0)


def requests(layers_d_model, dev, new, pad_to=None):
    import torch

    from zonos_amd import synthetic
    from zonos_amd.requests import Request
    prefix = synthetic.prefix_codes(len(LCS), PREFIX, seed=3, device=dev)
    reqs = []
    for b, lc in enumerate(LCS):
        cond = synthetic.conditioning(1, lc, layers_d_model, seed=500 + b, device=dev)
        if pad_to is not None:
            cond = torch.cat([cond, cond.new_zeros(2, pad_to - lc, cond.shape[2])], dim=1)
        reqs.append(Request(cond, prefix[b], new, 2.0, SP, seed=1000, key=b, force_full_length=True))
    return reqs


def attn_stats(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "k_attn_decode" in r["Name"]:
                    rows.append(dict(name=r["Name"][:80], calls=int(r["Calls"]),
                                     us_per_launch=float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3))
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["ragged", "padded"])
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--new-tokens", type=int, default=NEW, help="budget of every request (a profiler run: 300)")
    ap.add_argument("--attn-stats")
    args = ap.parse_args()
    if args.attn_stats:
        return attn_stats(args.attn_stats)
    new = args.new_tokens
    import torch

    from zonos_amd import synthetic
    from zonos_amd.engine import EngineConfig, HipDecoder
    dev = torch.device("cuda")
    mc = dict(synthetic.ZONOS_V01, n_layer=args.layers)
    eng = HipDecoder(EngineConfig(**mc), synthetic.backbone_weights(dev, seed=0, **mc), dev)
    paths = dict(ragged=(requests(mc["d_model"], dev, new), dict(ragged=True)),
                 padded=(requests(mc["d_model"], dev, new, pad_to=max(LCS)), {}))
    steps = new + 9 - 1

    def run(name):
        reqs, kw = paths[name]
        torch.cuda.synchronize(dev)
        t0 = time.time()
        out = eng.generate_requests(reqs, poll_every=64, **kw)
        torch.cuda.synchronize(dev)
        dt = time.time() - t0
        assert all(x.shape[1] == new for x in out)
        assert (eng._ws["row_off"] is not None) == (name == "ragged")
        return dt

    order = [args.only] if args.only else ["ragged", "padded"]
    if not args.only:
        for name in order:               # warm-up of each: allocation, graph capture
            run(name)
    times = {n: [] for n in order}
    for _ in range(1 if args.only else 2):
        for name in order:               # interleaved
            times[name].append(run(name))
    res = dict(workload=f"c3 geometry, B = 64, Lc {min(LCS)}..{max(LCS)} (mean {sum(LCS) // 64}), prefix {PREFIX}, "
                        f"{new} new tokens, {args.layers} layers, {steps} steps + prefill per run (wall time)")
    for n, ts in times.items():
        res[n] = dict(seconds=[round(t, 4) for t in ts], ms_per_step=[round(1e3 * t / steps, 4) for t in ts],
                      codes_per_s=[round(64 * new * 9 / t, 1) for t in ts])      # 9 codebooks per frame, as bench.py counts
    print(json.dumps(res))


if __name__ == "__main__":
    main()
