#!/usr/bin/env python3
"""Steady-state cost of one CameraStreamPool.push tick with per-frame timestamps against the constant-rate pool (RTFS-Net-4 SRU, 16 kHz,
window 2 s, hop 1 s, uint8 mouth ROIs 96 x 96 from a 30 fps camera):

  python tools/bench_live_timestamps.py [--streams 1 8 32] [--steps 20] [--seconds 1.0] [--rounds 5] [--warmup 3]
                                        [--out profiles/live_timestamps_bench.json]

For S streams, every stream first delivers one window in two pushes of 1 s, then 1 s per tick (16000 samples and the camera frames of
that second), so each tick embeds 25 S model frames and has exactly S ready audio windows.
  stamps   ``open_camera_streams(timebase=90000)``, 30 frames per tick stamped i * 3000, ``until`` at the next frame's time: the emission
           of the constant-rate pool, with the source list built on the host and the held plane written on the device;
  dropped  the same pool kind and stamps with every sixth frame missing (25 frames per tick): a camera that drops frames;
  rate     ``open_camera_streams(frame_rate=30)``: the baseline, code this feature does not touch.
All three in one process, alternating rounds after warm-up; a host clock around a block of calls that ends in a device synchronise, a
block at least ``steps`` calls and at least ``seconds`` long; medians with min and max.  ``stamps`` and ``rate`` give torch.equal
outputs (checked before the timing).  Prints one JSON line (and writes it to --out).  Needs a GPU: there is no CPU figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, SPF, FS, ROI, FPS, TB = 32000, 16000, 640, 16000, 96, 30, 90000
STEP = TB // FPS  # ticks of the timebase per camera frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rtfs_net_amd as R
    from oracle import video_oracle as V
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    if not torch.cuda.is_available():
        sys.exit("bench_live_timestamps.py measures on the GPU; none found")
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    vm = R.FRCNNVideoModel(print_macs=False)
    vm.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in V.make_video_state_dict(0).items()})
    system = R.System(audio_model=m.cuda().eval(), video_model=vm.cuda().eval())
    rs = np.random.RandomState(0)
    out = {"metric": "CameraStreamPool.push with per-frame timestamps (timebase 90000; 30 uint8 96x96 camera frames + 1 s of audio per "
                     "stream and tick, until at the next frame's time; `dropped`: every sixth frame missing) vs the pool at frame_rate=30 "
                     "(window 2 s, hop 1 s, one ready window per stream; host clock around a block of `steps` calls, at least `seconds` "
                     "long, ending in a synchronise, median [min, max] over alternating rounds, ms per call)",
           "model": "RTFS-Net-4 SRU + FRCNNVideoModel (ResNet-18)", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "rounds": args.rounds, "cases": []}
    Ch = HOP * FPS // FS  # camera frames per tick: 30
    keep = [i for i in range(Ch) if i % 6 != 5]  # the frames of a tick that a camera dropping every sixth delivers
    keep_idx = torch.tensor(keep, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        for S in args.streams:
            ids = list(range(S))
            hop_a = [torch.from_numpy((rs.randn(HOP) * 0.05).astype(np.float32)).cuda() for _ in ids]
            hop_r = [torch.from_numpy(rs.randint(0, 256, size=(Ch, ROI, ROI)).astype(np.uint8)).cuda() for _ in ids]
            drop_r = [r.index_select(0, keep_idx) for r in hop_r]  # built once, outside the timed block
            kw = dict(window=WINDOW, hop=HOP, max_batch=max(32, S), roi_hw=(ROI, ROI))
            pools = {"stamps": system.open_camera_streams(S, timebase=TB, **kw), "dropped": system.open_camera_streams(S, timebase=TB, **kw),
                     "rate": system.open_camera_streams(S, frame_rate=FPS, **kw)}
            tickno = {k: 0 for k in pools}

            def ticks(which, n):
                pool = pools[which]
                for _ in range(n):
                    if which == "rate":
                        r = pool.push(ids, hop_a, hop_r)
                    else:
                        base = tickno[which] * Ch
                        ts = [(base + i) * STEP for i in (range(Ch) if which == "stamps" else keep)]
                        r = pool.push(ids, hop_a, hop_r if which == "stamps" else drop_r, timestamps=[ts] * S, until=(base + Ch) * STEP)
                    tickno[which] += 1
                return r

            def timed(which, steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                held = ticks(which, steps)
                torch.cuda.synchronize()
                del held
                return 1000.0 * (time.perf_counter() - t0) / steps

            res = {k: ticks(k, 2 + args.warmup) for k in pools}  # the first window takes two pushes, then the warm-up
            assert all(tuple(x.shape) == (1, HOP) and torch.equal(x, y) for x, y in zip(res["stamps"], res["rate"]))
            assert all(tuple(x.shape) == (1, HOP) and bool(torch.isfinite(x).all()) for x in res["dropped"])
            steps = max(args.steps, math.ceil(1000.0 * args.seconds / timed("rate", args.steps)))
            t = {k: [] for k in pools}
            for _ in range(args.rounds):
                for k in pools:
                    t[k].append(timed(k, steps))
            med = {k: statistics.median(v) for k, v in t.items()}
            stat = lambda k: [round(med[k], 4), round(min(t[k]), 4), round(max(t[k]), 4)]  # noqa: E731
            overlap = lambda a, b: min(t[a]) <= max(t[b]) and min(t[b]) <= max(t[a])  # noqa: E731
            case = {"streams": S, "steps": steps, "stamps_tick_ms": stat("stamps"), "dropped_tick_ms": stat("dropped"), "rate_tick_ms": stat("rate"),
                    "stamps_over_rate": round(med["stamps"] / med["rate"] - 1.0, 4), "dropped_over_rate": round(med["dropped"] / med["rate"] - 1.0, 4),
                    "rate_spread": round((max(t["rate"]) - min(t["rate"])) / med["rate"], 4),
                    "stamps_ranges_overlap_rate": overlap("stamps", "rate"), "dropped_ranges_overlap_rate": overlap("dropped", "rate"),
                    "streams_in_real_time": round(S * (HOP / FS) / (med["stamps"] / 1000.0), 1),
                    "held_bytes_per_tick_per_stream": 88 * 88 * 4, "source_words_per_tick_per_stream": HOP // SPF}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del pools
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
