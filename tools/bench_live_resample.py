#!/usr/bin/env python3
"""Steady-state cost of live streams at the microphone's rate (RTFS-Net-4 SRU, window 2 s, hop 1 s, uint8 mouth ROIs 96 x 96 at 25 fps):

  python tools/bench_live_resample.py [--streams 1 8 32] [--steps 20] [--seconds 1.0] [--rounds 5] [--warmup 3] [--out profiles/live_resample_bench.json]

For S streams, each delivering 1 s per tick, at 48 kHz int16 PCM and at 44.1 kHz float32:
  (a) the resampler alone: a ResampleStreamPool tick of S chunks (separate allocations) against datas.resample on the same samples as ONE
      (S, n) float32 batch - what a caller had before, with the wrong chunk edges; for int16 the batch side includes the conversion
      pcm.float() / 32768 that the pool does inside its launch (the bare call is recorded next to it);
  (b) the whole tick: a CameraStreamPool opened with sample_rate (every stream first delivers one window, then 1 s per tick, so each tick
      has exactly S ready windows) against the 16 kHz CameraStreamPool tick on ready 16 kHz audio PLUS that batch datas.resample.
The method is tools/bench_live.py's: a host clock around a block of calls that ends in a device synchronise, a block at least ``steps``
calls and at least ``seconds`` long, ``rounds`` alternating rounds in one process after warm-up, medians with min and max.  Prints one
JSON line (and writes it to --out).  Needs a GPU: there is no CPU figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, SPF, FS, ROI = 32000, 16000, 640, 16000, 96


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
        sys.exit("bench_live_resample.py measures on the GPU; none found")
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    vm = R.FRCNNVideoModel(print_macs=False)
    vm.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in V.make_video_state_dict(0).items()})
    system = R.System(audio_model=m.cuda().eval(), video_model=vm.cuda().eval())
    rs = np.random.RandomState(0)
    out = {"metric": "(a) ResampleStreamPool.push of S chunks of 1 s vs datas.resample on the same samples as one (S, n) float32 batch; (b) "
                     "CameraStreamPool.push at sample_rate (25 uint8 96x96 frames + 1 s of audio per stream, one ready window per stream) vs the "
                     "16 kHz CameraStreamPool.push + that batch datas.resample (window 2 s, hop 1 s; host clock around a block of `steps` calls, "
                     "at least `seconds` long, ending in a synchronise, median [min, max] over alternating rounds, ms per call)",
           "model": "RTFS-Net-4 SRU + FRCNNVideoModel (ResNet-18)", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "rounds": args.rounds, "cases": []}
    Fw, Fh = WINDOW // SPF, HOP // SPF

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = fn(steps)
        torch.cuda.synchronize()
        del keep
        return 1000.0 * (time.perf_counter() - t0) / steps

    with torch.no_grad():
        for rate, pcm in ((48000, True), (44100, False)):
            o, n, width, _ = datas.resample_plan(rate, FS)
            for S in args.streams:
                ids = list(range(S))

                def audio(seconds):
                    x = np.clip(rs.randn(S, int(seconds * rate)) * 0.05, -1.0, 0.999)
                    return torch.from_numpy(np.round(x * 32768).astype(np.int16) if pcm else x.astype(np.float32)).cuda()

                frames = lambda k: [torch.from_numpy(rs.randint(0, 256, size=(k, ROI, ROI)).astype(np.uint8)).cuda() for _ in ids]  # noqa: E731
                first_b, hop_b = audio(WINDOW / FS), audio(HOP / FS)  # (S, n): the batch the other side resamples
                first_c, hop_c = [r.clone() for r in first_b], [r.clone() for r in hop_b]  # separate allocations, as a live caller holds them
                to_f32 = (lambda b: b.to(torch.float32) * (1.0 / 32768.0)) if pcm else (lambda b: b)
                hop_f = to_f32(hop_b).contiguous()
                first_r, hop_r = frames(Fw), frames(Fh)
                first_16, hop_16 = [w.contiguous() for w in datas.resample(to_f32(first_b), rate)], [w.contiguous() for w in datas.resample(hop_f, rate)]
                rp = datas.open_resample_streams(S, rate, max_chunk=rate)
                cam = system.open_camera_streams(S, window=WINDOW, hop=HOP, max_batch=max(32, S), roi_hw=(ROI, ROI), sample_rate=rate)
                cam.push(ids, first_c, first_r)
                cam16 = system.open_camera_streams(S, window=WINDOW, hop=HOP, max_batch=max(32, S), roi_hw=(ROI, ROI))
                cam16.push(ids, first_16, first_r)

                def rp_ticks(k):
                    for _ in range(k):
                        r = rp.push(ids, hop_c)
                    return r

                def batch_resample(k):
                    for _ in range(k):
                        r = datas.resample(to_f32(hop_b), rate)
                    return r

                def bare_resample(k):
                    for _ in range(k):
                        r = datas.resample(hop_f, rate)
                    return r

                def cam_ticks(k):
                    for _ in range(k):
                        r = cam.push(ids, hop_c, hop_r)
                    return r

                def pair_ticks(k):
                    for _ in range(k):
                        w = datas.resample(to_f32(hop_b), rate)
                        r = cam16.push(ids, hop_16, hop_r)
                    return r, w

                assert all(tuple(r.shape) == (HOP,) for r in rp_ticks(args.warmup))
                assert tuple(batch_resample(args.warmup).shape) == (S, HOP) and tuple(bare_resample(args.warmup).shape) == (S, HOP)
                assert all(tuple(r.shape) == (1, HOP) for r in cam_ticks(args.warmup))
                assert all(tuple(r.shape) == (1, HOP) for r in pair_ticks(args.warmup)[0])
                rsteps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(rp_ticks, args.steps)))
                csteps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(pair_ticks, args.steps)))
                t = {"rp": [], "batch": [], "bare": [], "cam": [], "pair": []}
                for _ in range(args.rounds):
                    t["rp"].append(timed(rp_ticks, rsteps))
                    t["batch"].append(timed(batch_resample, rsteps))
                    t["bare"].append(timed(bare_resample, rsteps))
                    t["cam"].append(timed(cam_ticks, csteps))
                    t["pair"].append(timed(pair_ticks, csteps))
                med = {k: statistics.median(v) for k, v in t.items()}
                stat = lambda k: [round(med[k], 4), round(min(t[k]), 4), round(max(t[k]), 4)]  # noqa: E731
                case = {"sample_rate": rate, "dtype": "int16" if pcm else "float32", "streams": S, "resample_steps": rsteps, "camera_steps": csteps,
                        "resample_tick_ms": stat("rp"), "batch_resample_ms": stat("batch"), "batch_resample_bare_ms": stat("bare"),
                        "resample_tick_over_batch": round(med["rp"] / med["batch"], 3),
                        "camera_tick_at_rate_ms": stat("cam"), "camera_tick_16k_plus_batch_resample_ms": stat("pair"),
                        "difference_ms": round(med["cam"] - med["pair"], 4), "difference_over_pair": round(med["cam"] / med["pair"] - 1.0, 4),
                        "streams_in_real_time": round(S * (HOP / FS) / (med["cam"] / 1000.0), 1),
                        "resampler_state_bytes_per_slot": 4 * 2 * 2 * width, "added_latency_ms": round(1000.0 * width / rate, 3)}
                print(json.dumps(case), flush=True)
                out["cases"].append(case)
                del rp, cam, cam16
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
