#!/usr/bin/env python3
"""AVNet.separate_speakers (K targets per mixture, one audio prefix per mixture) against AVNet.forward on the replicated batch.

  python tools/bench_speakers.py [--steps 20] [--warmup 3] [--out profiles/speakers_bench.json]

Each case warms up, then alternates the two calls in this one process (each timed with HIP events on the current stream, median over the
steps), synchronises, and reports the max-rel between the two outputs.  Cases: RTFS-Net-4 2 s B = 32 K = 2 (vs forward on 64 rows);
B = 1 K = 2 (vs forward at B = 2 and vs two B = 1 forwards); RTFS-Net-12 2 s B = 32 K = 2.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    y = fn()
    b.record()
    return y, (a, b)


def case(m, B, K, L, Tv, steps, warmup, seed):
    rs = np.random.RandomState(seed)
    wav = torch.from_numpy((rs.randn(B, L) * 0.05).astype(np.float32)).cuda()
    lips = torch.from_numpy(rs.randn(B, K, 512, Tv).astype(np.float32)).cuda()
    wav_rep, lips_rep = wav.repeat_interleave(K, 0), lips.reshape(B * K, 512, Tv)
    calls = {"separate_speakers": lambda: m.separate_speakers(wav, lips), f"forward_B{B * K}": lambda: m(wav_rep, lips_rep)}
    if B == 1 and K > 1:
        calls[f"forward_B1_x{K}"] = lambda: [m(wav, lips[:, k]) for k in range(K)]
    with torch.no_grad():
        for _ in range(warmup):
            for f in calls.values():
                f()
        ev = {k: [] for k in calls}
        outs = {}
        for _ in range(steps):
            for k, f in calls.items():  # alternating: both calls see the same clocks / memory-side cache history
                outs[k], e = timed(f)
                ev[k].append(e)
        torch.cuda.synchronize()
    ms = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
    got = outs["separate_speakers"].reshape(B * K, 1, L)
    res = {"B": B, "K": K, "L": L, "Tv": Tv, "ms": {k: round(v, 4) for k, v in ms.items()}}
    for k in calls:
        if k == "separate_speakers":
            continue
        ref = outs[k] if not isinstance(outs[k], list) else torch.stack([o[0] for o in outs[k]], 0)
        ref = ref.reshape(B * K, 1, L)
        res.setdefault("max_rel", {})[k] = float((got - ref).abs().max() / ref.abs().max())
        res.setdefault("saving_pct", {})[k] = round(100.0 * (1.0 - ms["separate_speakers"] / ms[k]), 2)
    res["ms_per_target"] = round(ms["separate_speakers"] / (B * K), 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()}
    models = {}
    for r in (4, 12):
        m = R.AVNet(print_macs=False, **audionet_config(r))
        m.load_state_dict(sd)  # (one shared block: the R4 state dict serves every R)
        models[r] = m.cuda().eval()
    out = {"metric": "separate_speakers vs forward on the replicated batch (median ms per call, alternating in one process)",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "r4_b32_k2_2s": case(models[4], 32, 2, 32000, 50, args.steps, args.warmup, 1),
           "r4_b1_k2_2s": case(models[4], 1, 2, 32000, 50, args.steps, args.warmup, 2),
           "r12_b32_k2_2s": case(models[12], 32, 2, 32000, 50, args.steps, args.warmup, 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
