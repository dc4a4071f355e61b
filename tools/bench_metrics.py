#!/usr/bin/env python3
"""Cost of scoring separations on the device (rtfs_net_amd.metrics) next to the float64 host oracle that restates pystoi.
Not part of bench.py's contract.  Event timing (median of STEPS launches after WARMUP) of stoi at 32 x 2 s and 256 x 2 s and of
ALLMetricsTracker.update_batch at 32 x 2 s (four PIT launches, the STOI launches, one device -> host copy and the CSV rows), and the
wall time of tests/metrics_oracle.stoi over the same 32 rows on the host.  Prints one JSON line.

  python tools/bench_metrics.py --estoi [--rounds 9] [--out profiles/estoi_bench.json]

measures extended STOI instead, at 32 x 2 s: ``stoi``, ``estoi``, the combined ``estoi(with_classic=True)`` and ``stoi`` followed by
``estoi``, as variants ALTERNATING inside each of ROUNDS rounds of one process (each figure the median of STEPS event-timed calls);
per variant the median, minimum and maximum over the rounds, and the difference separate - combined per round with its spread."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtfs_net_amd as R  # noqa: E402
from tests import metrics_oracle as M  # noqa: E402

STEPS, WARMUP, L, FS = int(os.environ.get("STEPS", 20)), int(os.environ.get("WARMUP", 3)), 32000, 16000


def batch(B, seed):
    rng = np.random.default_rng(seed)
    x = np.stack([M.speech_like(rng, L, FS, gaps=[(0.6, 0.8)], zero_gaps=[(1.3, 1.4)]) for _ in range(B)])
    y = (x + 0.3 * rng.standard_normal(x.shape)).astype(np.float32)
    return x, y


def event_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def estoi_rounds(rounds):
    x, y = batch(32, 32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    variants = {"stoi": lambda: R.stoi(xd, yd, FS), "estoi": lambda: R.estoi(xd, yd, FS),
                "combined": lambda: R.estoi(xd, yd, FS, with_classic=True),
                "stoi_then_estoi": lambda: (R.stoi(xd, yd, FS), R.estoi(xd, yd, FS))}
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(event_ms(fn))
    out = {"shape": "32 x 2 s at 16 kHz", "rounds": rounds, "steps": STEPS, "warmup": WARMUP, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        out[k] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    gain = [a - b for a, b in zip(ms["stoi_then_estoi"], ms["combined"])]
    out["separate_minus_combined_ms"] = {"median": round(float(np.median(gain)), 4), "min": round(min(gain), 4), "max": round(max(gain), 4)}
    out["round_spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 4)
    return out


if "--estoi" in sys.argv[1:]:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--estoi", action="store_true")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = json.dumps({"metric": "extended STOI block calls, HIP events, variants alternating in one process", "block": estoi_rounds(args.rounds)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

res = {}
for B in (32, 256):
    x, y = batch(B, B)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res[f"stoi_ms_b{B}_2s"] = round(event_ms(lambda: R.stoi(xd, yd, FS)), 4)
x, y = batch(32, 7)
mix = (x + 0.8 * np.random.default_rng(8).standard_normal(x.shape)).astype(np.float32)
md, xd, yd = torch.from_numpy(mix).cuda(), torch.from_numpy(x[:, None]).cuda(), torch.from_numpy(y[:, None]).cuda()
keys = [str(b) for b in range(32)]
with tempfile.TemporaryDirectory() as td:
    t = R.ALLMetricsTracker(os.path.join(td, "m.csv"))
    res["update_batch_ms_b32_2s"] = round(event_ms(lambda: t.update_batch(md, xd, yd, keys)), 4)
    t.final()
t0 = time.perf_counter()
for b in range(32):
    M.stoi(x[b], y[b], FS)
res["host_oracle_stoi_ms_b32_2s"] = round((time.perf_counter() - t0) * 1e3, 1)
res["steps"], res["warmup"] = STEPS, WARMUP
print(json.dumps(res))
