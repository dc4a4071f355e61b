#!/usr/bin/env python3
"""Steady-state cost of one CameraStreamPool.push tick against the same work without streaming the video (RTFS-Net-4 SRU, 16 kHz,
window 2 s, hop 1 s, uint8 mouth ROIs 96 x 96 at 25 fps):

  python tools/bench_live_camera.py [--streams 1 8 32] [--steps 20] [--seconds 1.0] [--rounds 5] [--warmup 3] [--out profiles/live_camera_bench.json]

For S streams, every stream first delivers one window (2 s of audio, 50 frames), then 1 s per tick (16000 samples, 25 frames), so each
tick embeds 25 S frames and has exactly S ready audio windows.  Against it, at the same commit, the pair that does the same work without
the camera path: a tick of the existing StreamPool fed ready embeddings PLUS video_model on (S, 1, 25, 88, 88) prepared lips.  Next to
the two, the video side alone: a LipStreamPool tick against video_model on the same frames, which is where the ingest launch, the 5-frame
windows of the stem input and the scatter show.  The method is tools/bench_live.py's: a host clock around a block of calls that ends in
a device synchronise, a block at least ``steps`` calls and at least ``seconds`` long, ``rounds`` alternating rounds in one process after
warm-up, medians with min and max.  Prints one JSON line (and writes it to --out).  Needs a GPU: there is no CPU figure."""
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
    from rtfs_net_amd.configs import audionet_config
    if not torch.cuda.is_available():
        sys.exit("bench_live_camera.py measures on the GPU; none found")
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    vm = R.FRCNNVideoModel(print_macs=False)
    vm.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in V.make_video_state_dict(0).items()})
    system = R.System(audio_model=m.cuda().eval(), video_model=vm.cuda().eval())
    m, vm = system.audio_model, system.video_model
    val = R.get_preprocessing_pipelines()["val"]
    rs = np.random.RandomState(0)
    out = {"metric": "CameraStreamPool.push (25 uint8 96x96 frames + 1 s of audio per stream, one ready window per stream) vs StreamPool.push on "
                     "ready embeddings + video_model on (S,1,25,88,88); lips_* = the video side alone (window 2 s, hop 1 s; host clock around a "
                     "block of `steps` calls, at least `seconds` long, ending in a synchronise, median [min, max] over alternating rounds, ms per call)",
           "model": "RTFS-Net-4 SRU + FRCNNVideoModel (ResNet-18)", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "rounds": args.rounds, "cases": []}
    Fw, Fh = WINDOW // SPF, HOP // SPF
    with torch.no_grad():
        for S in args.streams:
            ids = list(range(S))
            audio = lambda n: [torch.from_numpy((rs.randn(n) * 0.05).astype(np.float32)).cuda() for _ in ids]  # noqa: E731
            frames = lambda n: [torch.from_numpy(rs.randint(0, 256, size=(n, ROI, ROI)).astype(np.uint8)).cuda() for _ in ids]  # noqa: E731
            first_a, first_r, hop_a, hop_r = audio(WINDOW), frames(Fw), audio(HOP), frames(Fh)
            lips = val(torch.stack(hop_r))  # (S,1,25,88,88)
            first_v = [e.contiguous() for e in vm(val(torch.stack(first_r)))]
            hop_v = [e.contiguous() for e in vm(lips)]
            cam = system.open_camera_streams(S, window=WINDOW, hop=HOP, max_batch=max(32, S), roi_hw=(ROI, ROI))
            cam.push(ids, first_a, first_r)
            pool = m.open_streams(S, window=WINDOW, hop=HOP, max_batch=max(32, S))
            pool.push(ids, first_a, first_v)
            lp = vm.open_streams(S, max_frames=Fw, roi_hw=(ROI, ROI))
            lp.push(ids, first_r)

            def cam_ticks(n):
                for _ in range(n):
                    r = cam.push(ids, hop_a, hop_r)
                return r

            def pair_ticks(n):
                for _ in range(n):
                    e = vm(lips)
                    r = pool.push(ids, hop_a, hop_v)
                return r, e

            def lip_ticks(n):
                for _ in range(n):
                    r = lp.push(ids, hop_r)
                return r

            def video_models(n):
                for _ in range(n):
                    e = vm(lips)
                return e

            def timed(fn, steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                keep = fn(steps)
                torch.cuda.synchronize()
                del keep
                return 1000.0 * (time.perf_counter() - t0) / steps

            assert all(tuple(r.shape) == (1, HOP) for r in cam_ticks(args.warmup))
            assert all(tuple(r.shape) == (1, HOP) for r in pair_ticks(args.warmup)[0])
            assert all(tuple(r.shape) == (512, Fh) for r in lip_ticks(args.warmup))
            steps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(pair_ticks, args.steps)))
            vsteps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(video_models, args.steps)))
            t = {"cam": [], "pair": [], "lip": [], "vm": []}
            for _ in range(args.rounds):
                t["cam"].append(timed(cam_ticks, steps))
                t["pair"].append(timed(pair_ticks, steps))
                t["lip"].append(timed(lip_ticks, vsteps))
                t["vm"].append(timed(video_models, vsteps))
            med = {k: statistics.median(v) for k, v in t.items()}
            stat = lambda k: [round(med[k], 4), round(min(t[k]), 4), round(max(t[k]), 4)]  # noqa: E731
            case = {"streams": S, "steps": steps, "video_steps": vsteps, "camera_tick_ms": stat("cam"), "pool_plus_video_model_ms": stat("pair"),
                    "difference_ms": round(med["cam"] - med["pair"], 4), "difference_over_pair": round(med["cam"] / med["pair"] - 1.0, 4),
                    "lips_tick_ms": stat("lip"), "video_model_ms": stat("vm"), "lips_difference_ms": round(med["lip"] - med["vm"], 4),
                    "streams_in_real_time": round(S * (HOP / FS) / (med["cam"] / 1000.0), 1),
                    "lip_state_bytes_per_slot": 4 * 2 * 4 * 88 * 88,
                    "audio_state_bytes_per_slot": 4 * (cam.audio.capacity * (1 + cam.audio.n_src) + 512 * cam.audio.capacity // SPF),
                    "stem_input_bytes_per_frame": 4 * 5 * 94 * 94}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del cam, pool, lp
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
