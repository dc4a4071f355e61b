#!/usr/bin/env python3
"""Steady-state cost of one CameraStreamPool.push tick at the camera's own frame rate against select-then-push (RTFS-Net-4 SRU, 16 kHz,
window 2 s, hop 1 s, uint8 mouth ROIs 96 x 96 at 30 fps):

  python tools/bench_live_camera_rate.py [--streams 1 8 32] [--steps 20] [--seconds 1.0] [--rounds 5] [--warmup 3]
                                         [--out profiles/live_framerate_bench.json]

For S streams, every stream first delivers one window (2 s of audio, 60 camera frames), then 1 s per tick (16000 samples, 30 camera
frames = 25 model frames), so each tick embeds 25 S frames and has exactly S ready audio windows.
  rate     ``open_camera_streams(frame_rate=30)``: the ingest launch selects the frames;
  select   the existing 25 fps pool fed the same frames pre-selected with ``torch.index_select`` on the device (one call per stream,
           the index tensor built once outside the timed block): what a caller had to do before, without the bookkeeping across
           chunks, which here is trivial because a tick is a whole second.
Both in one process, alternating rounds after warm-up; a host clock around a block of calls that ends in a device synchronise, a block at
least ``steps`` calls and at least ``seconds`` long; medians with min and max.  The two give torch.equal outputs (checked before the
timing).  Prints one JSON line (and writes it to --out).  Needs a GPU: there is no CPU figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, SPF, FS, ROI, FPS = 32000, 16000, 640, 16000, 96, 30


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
    from rtfs_net_amd import datas
    from rtfs_net_amd.configs import audionet_config
    if not torch.cuda.is_available():
        sys.exit("bench_live_camera_rate.py measures on the GPU; none found")
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    vm = R.FRCNNVideoModel(print_macs=False)
    vm.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in V.make_video_state_dict(0).items()})
    system = R.System(audio_model=m.cuda().eval(), video_model=vm.cuda().eval())
    rs = np.random.RandomState(0)
    out = {"metric": "CameraStreamPool.push at frame_rate=30 (30 uint8 96x96 camera frames + 1 s of audio per stream, one ready window per "
                     "stream) vs the 25 fps pool fed the 25 frames torch.index_select picks on the device (window 2 s, hop 1 s; host clock "
                     "around a block of `steps` calls, at least `seconds` long, ending in a synchronise, median [min, max] over alternating "
                     "rounds, ms per call)",
           "model": "RTFS-Net-4 SRU + FRCNNVideoModel (ResNet-18)", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "rounds": args.rounds, "cases": []}
    Cw, Ch = WINDOW * FPS // FS, HOP * FPS // FS  # camera frames per window / per hop: 60, 30
    # a tick starts on a whole second, where the pattern of 30 -> 25 repeats: the local selection is the same every tick
    first_idx = torch.tensor(datas.frame_rate_map(Cw, FPS), dtype=torch.int64, device="cuda")
    hop_idx = torch.tensor([c - Cw for c in datas.frame_rate_map(Cw + Ch, FPS)[len(first_idx):]], dtype=torch.int64, device="cuda")
    assert len(first_idx) == WINDOW // SPF and len(hop_idx) == HOP // SPF and int(hop_idx.min()) >= 0
    with torch.no_grad():
        for S in args.streams:
            ids = list(range(S))
            audio = lambda n: [torch.from_numpy((rs.randn(n) * 0.05).astype(np.float32)).cuda() for _ in ids]  # noqa: E731
            frames = lambda n: [torch.from_numpy(rs.randint(0, 256, size=(n, ROI, ROI)).astype(np.uint8)).cuda() for _ in ids]  # noqa: E731
            first_a, first_r, hop_a, hop_r = audio(WINDOW), frames(Cw), audio(HOP), frames(Ch)
            kw = dict(window=WINDOW, hop=HOP, max_batch=max(32, S), roi_hw=(ROI, ROI))
            rate, sel = system.open_camera_streams(S, frame_rate=FPS, **kw), system.open_camera_streams(S, **kw)
            rate.push(ids, first_a, first_r)
            sel.push(ids, first_a, [r.index_select(0, first_idx) for r in first_r])

            def rate_ticks(n):
                for _ in range(n):
                    r = rate.push(ids, hop_a, hop_r)
                return r

            def select_ticks(n):
                for _ in range(n):
                    r = sel.push(ids, hop_a, [c.index_select(0, hop_idx) for c in hop_r])
                return r

            def timed(fn, steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                keep = fn(steps)
                torch.cuda.synchronize()
                del keep
                return 1000.0 * (time.perf_counter() - t0) / steps

            a, b = rate_ticks(args.warmup), select_ticks(args.warmup)
            assert all(tuple(x.shape) == (1, HOP) and torch.equal(x, y) for x, y in zip(a, b))
            steps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(select_ticks, args.steps)))
            t = {"rate": [], "select": []}
            for _ in range(args.rounds):
                t["rate"].append(timed(rate_ticks, steps))
                t["select"].append(timed(select_ticks, steps))
            med = {k: statistics.median(v) for k, v in t.items()}
            stat = lambda k: [round(med[k], 4), round(min(t[k]), 4), round(max(t[k]), 4)]  # noqa: E731
            case = {"streams": S, "steps": steps, "rate_tick_ms": stat("rate"), "select_then_push_ms": stat("select"),
                    "difference_ms": round(med["rate"] - med["select"], 4), "difference_over_select": round(med["rate"] / med["select"] - 1.0, 4),
                    "ranges_overlap": min(t["rate"]) <= max(t["select"]) and min(t["select"]) <= max(t["rate"]),
                    "streams_in_real_time": round(S * (HOP / FS) / (med["rate"] / 1000.0), 1),
                    "camera_bytes_per_tick_per_stream": Ch * ROI * ROI, "selected_bytes_per_tick_per_stream": (HOP // SPF) * ROI * ROI}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del rate, sel
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
