#!/usr/bin/env python3
"""A different number of faces per mixture (AVNet.separate_speakers(counts=...), AVNet.separate_many_speakers) against the only ways to
do the same work without the target-to-mixture table.

  python tools/bench_targets.py [--steps 20] [--warmup 3] [--out profiles/targets_bench.json]

RTFS-Net-4, 2 s windows.  Every case warms up, then runs its calls in alternating rounds in this one process (each call timed with HIP
events on the current stream), synchronises, and reports per call the median with [min, max] over the rounds, and the max-rel between
the outputs.
  ragged_b16_n40   16 mixtures, counts cycling 1, 2, 3, 4 (40 targets) against (a) forward on the 40 replicated rows and (b)
                   separate_speakers padded to K = 4 (64 targets, 24 of them thrown away)
  equal_b16_k2     counts all 2 against the fixed-K separate_speakers (the same kernels; the table replaces a division)
  many_r8          separate_many_speakers on 8 recordings of 2 .. 9 s with K cycling 1, 2, 3, 4 against separate_many with the audio
                   listed once per face
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def rounds(calls, steps, warmup):
    """calls: name -> function.  -> (name -> {median, min, max} ms, name -> last output)."""
    a = {k: [] for k in calls}
    outs = {}
    with torch.no_grad():
        for _ in range(warmup):
            for f in calls.values():
                f()
        for _ in range(steps):
            for k, f in calls.items():  # alternating: every call sees the same clocks / memory-side cache history
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[k] = f()
                e1.record()
                a[k].append((e0, e1))
        torch.cuda.synchronize()
    ms = {k: [x.elapsed_time(y) for x, y in v] for k, v in a.items()}
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}, outs


def max_rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def ratios(ms, ours, others):
    return {k: {"saving_pct": round(100.0 * (1.0 - ms[ours]["median"] / ms[k]["median"]), 2),
                "ratio": round(ms[ours]["median"] / ms[k]["median"], 4),
                "baseline_spread_pct": round(100.0 * (ms[k]["max"] - ms[k]["min"]) / ms[k]["median"], 2)} for k in others}


def batch_case(m, counts, steps, warmup, seed, padded):
    B, N, L, Tv = len(counts), sum(counts), 32000, 50
    rs = np.random.RandomState(seed)
    wav = torch.from_numpy((rs.randn(B, L) * 0.05).astype(np.float32)).cuda()
    lips = torch.from_numpy(rs.randn(N, 512, Tv).astype(np.float32)).cuda()
    rep = torch.tensor(counts).cuda()
    wav_rep = wav.repeat_interleave(rep, 0)
    K = max(counts)
    first = np.cumsum([0] + counts[:-1])
    idx = torch.tensor([first[b] + min(k, counts[b] - 1) for b in range(B) for k in range(K)]).cuda()  # short mixtures repeat their last face
    lips_pad = lips[idx].reshape(B, K, 512, Tv).contiguous()
    keep = torch.tensor([b * K + k for b in range(B) for k in range(counts[b])]).cuda()
    calls = {"ragged": lambda: m.separate_speakers(wav, lips, counts=counts), f"forward_B{N}": lambda: m(wav_rep, lips)[:, 0]}
    name = f"separate_speakers_K{K}" + ("_padded" if padded else "")
    calls[name] = lambda: m.separate_speakers(wav, lips_pad).reshape(B * K, L)[keep]
    ms, outs = rounds(calls, steps, warmup)
    others = [k for k in calls if k != "ragged"]
    return {"B": B, "N": N, "counts": counts, "L": L, "Tv": Tv, "ms": ms, "vs": ratios(ms, "ragged", others),
            "max_rel": {k: max_rel(outs["ragged"], outs[k]) for k in others}, "ms_per_target": round(ms["ragged"]["median"] / N, 5)}


def many_case(m, steps, warmup, seed):
    rs = np.random.RandomState(seed)
    Ls = [32000 + 16000 * r for r in range(8)]
    Ks = [1 + r % 4 for r in range(8)]
    wavs = [torch.from_numpy((rs.randn(L) * 0.05).astype(np.float32)).cuda() for L in Ls]
    lips = [torch.from_numpy(rs.randn(K, 512, L // 640).astype(np.float32)).cuda() for K, L in zip(Ks, Ls)]
    wavs_rep = [w for w, K in zip(wavs, Ks) for _ in range(K)]
    lips_rep = [lp[k] for lp, K in zip(lips, Ks) for k in range(K)]
    calls = {"separate_many_speakers": lambda: m.separate_many_speakers(wavs, lips),
             "separate_many_per_face": lambda: m.separate_many(wavs_rep, lips_rep)}
    ms, outs = rounds(calls, steps, warmup)
    got = torch.cat([o.reshape(-1) for o in outs["separate_many_speakers"]])
    ref = torch.cat([o.reshape(-1) for o in outs["separate_many_per_face"]])
    return {"R": 8, "L": Ls, "K": Ks, "window": 32000, "hop": 16000, "max_batch": 32, "ms": ms,
            "vs": ratios(ms, "separate_many_speakers", ["separate_many_per_face"]), "max_rel": max_rel(got, ref)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    m = m.cuda().eval()
    out = {"metric": "ragged separate_speakers / separate_many_speakers vs the routes without the table "
                     "(ms per call: median, min, max over alternating rounds in one process)",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "ragged_b16_n40": batch_case(m, [1 + b % 4 for b in range(16)], args.steps, args.warmup, 1, True),
           "equal_b16_k2": batch_case(m, [2] * 16, args.steps, args.warmup, 2, False),
           "many_r8": many_case(m, args.steps, args.warmup, 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
