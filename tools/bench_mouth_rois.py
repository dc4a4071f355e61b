#!/usr/bin/env python3
"""Cost of cutting mouth ROIs out of whole camera frames on the device (datas.mouth_rois, one rtfs_mouth_rois_u8 launch) against what a
user writes today on the same device, the same frames and the same maps in the same process: frames converted to grey float32, then
``affine_grid`` + ``grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False)``, rounded to uint8.

  python tools/bench_mouth_rois.py [--jobs 25 200 800] [--streams 1 8 32] [--steps 20] [--seconds 0.5] [--rounds 5] [--warmup 3]
                                   [--out profiles/mouth_rois_bench.json]

Crop cases: J jobs (800 = 32 streams x 25 frames), 96 x 96 ROIs out of 1280 x 720 frames: packed BGR with K = 1 face per frame, packed
BGR with K = 4 faces per frame (J / 4 frames, rounded up) and a luma plane with K = 1.  ``mouth_rois_ms`` is the whole call - the host
planner, the job table, its upload, the launch - with the landmarks changing from call to call, so that no call reuses the previous
call's table; ``launch_ms`` is rtfs_mouth_rois_u8 alone on a table that is already on the device.  ``grid_sample_ms`` is the baseline
with its conversion to grey float (a frame arrives as uint8), ``grid_sample_only_ms`` without it.  The baseline's bytes differ (float32
coordinates and weights, a float grey instead of OpenCV's fixed point): ``differing_bytes`` of ``bytes``, ``max_abs_diff``.

Pool cases: CameraStreamPool.push_frames on S streams, 1 s per tick (25 frames of 1280 x 720 BGR + 16000 samples per stream, window
2 s, hop 1 s, RTFS-Net-4 SRU), against push fed ready 96 x 96 ROIs.

The method is tools/bench_live.py's: a host clock around a block of calls that ends in a device synchronise, a block at least ``steps``
calls and at least ``seconds`` long, ``rounds`` alternating rounds in one process after warm-up, medians with min and max, ms per call.
Prints one JSON line (and writes it to --out).  Needs a GPU: there is no CPU figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, ROI, FS, SPF, WINDOW, HOP = 720, 1280, 96, 16000, 640, 32000, 16000


def faces(np, n, K, seed):
    """n x K plausible faces in a 1280 x 720 frame (eye distance 100 .. 220 px, roll within 0.3 rad) -> eyes (n,K,2,2), lips (n,K,4,2)."""
    rng = np.random.RandomState(seed)
    c = rng.uniform([300, 200], [980, 400], (n, K, 2))
    d, th = rng.uniform(100, 220, (n, K)), rng.uniform(-0.3, 0.3, (n, K))
    u = np.stack([np.cos(th), np.sin(th)], -1)
    v = np.stack([-u[..., 1], u[..., 0]], -1)
    eyes = np.stack([c - 0.5 * d[..., None] * u, c + 0.5 * d[..., None] * u], -2)
    along, down = rng.uniform(-0.5, 0.5, (n, K, 4)), rng.uniform(0.7, 1.3, (n, K, 4))
    lips = c[..., None, :] + d[..., None, None] * (along[..., None] * u[..., None, :] + down[..., None] * v[..., None, :])
    return eyes, lips


def theta_of(torch, A, device):
    """The pixel map A (n,2,3) (ROI (j, i) -> source (sx, sy)) as affine_grid's normalised theta, align_corners=False, float32."""
    A = torch.as_tensor(A, dtype=torch.float64)
    t = torch.empty_like(A)
    t[:, 0, 0], t[:, 0, 1] = A[:, 0, 0] * ROI / W, A[:, 0, 1] * ROI / W
    t[:, 0, 2] = (2.0 / W) * (A[:, 0, 0] * (ROI - 1) / 2 + A[:, 0, 1] * (ROI - 1) / 2 + A[:, 0, 2]) + 1.0 / W - 1.0
    t[:, 1, 0], t[:, 1, 1] = A[:, 1, 0] * ROI / H, A[:, 1, 1] * ROI / H
    t[:, 1, 2] = (2.0 / H) * (A[:, 1, 0] * (ROI - 1) / 2 + A[:, 1, 1] * (ROI - 1) / 2 + A[:, 1, 2]) + 1.0 / H - 1.0
    return t.to(torch.float32).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, nargs="+", default=[25, 200, 800])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import rtfs_net_amd as R
    from rtfs_net_amd import _lib, datas
    if not torch.cuda.is_available():
        sys.exit("bench_mouth_rois.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    lib = _lib.load()

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = fn(steps)
        torch.cuda.synchronize()
        del keep
        return 1000.0 * (time.perf_counter() - t0) / steps

    def measure(fns):
        """fns: name -> fn(steps).  Every block is at least args.steps calls and args.seconds long; the rounds alternate between the fns."""
        for fn in fns.values():
            fn(args.warmup)
        steps = {k: max(args.steps, math.ceil(1000.0 * args.seconds / max(timed(fn, args.steps), 1e-3))) for k, fn in fns.items()}
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, steps[k]))
        return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in t.items()}, steps

    out = {"metric": "datas.mouth_rois (96x96 uint8 ROIs out of 1280x720 frames, one rtfs_mouth_rois_u8 launch) vs float32 grey conversion + "
                     "affine_grid + grid_sample(bilinear, zeros, align_corners=False) + round on the same frames and maps; "
                     "CameraStreamPool.push_frames vs push fed ready ROIs (host clock around a block of calls, at least `seconds` long, "
                     "ending in a synchronise, median [min, max] over alternating rounds, ms per call)",
           "device": torch.cuda.get_device_name(0), "seconds": args.seconds, "rounds": args.rounds, "crop": [], "pool": []}
    wgt = (0.114, 0.587, 0.299)  # BGR -> grey, the float form of the fixed-point weights
    with torch.no_grad():
        for J in args.jobs:
            for kind, K in (("bgr", 1), ("bgr", 4), ("luma", 1)):
                n = -(-J // K)
                frames = torch.randint(0, 256, (n, H, W, 3) if kind == "bgr" else (n, H, W), dtype=torch.uint8, device=dev)
                order = "bgr" if kind == "bgr" else "gray"
                lms = [faces(np, n, K, 10 * J + K + s) for s in (0, 1)]  # two landmark sets in turn: every call builds and uploads its table
                lms = [(e, l) if K > 1 else (e[:, 0], l[:, 0]) for e, l in lms]
                A = datas.mouth_affine(*lms[0]).reshape(n, K, 2, 3)
                thetas = [theta_of(torch, A[:, k], dev) for k in range(K)]
                roi_out = torch.zeros((n, K, ROI, ROI) if K > 1 else (n, ROI, ROI), dtype=torch.uint8, device=dev)

                def ours(steps):
                    for i in range(steps):
                        r = datas.mouth_rois(frames, *lms[i & 1], order=order, out=roi_out)
                    return r

                datas.mouth_rois(frames, *lms[0], order=order, out=roi_out)
                table, tab = datas._MOUTH_TABLES[dev]
                st = _lib.stream_of(tab)

                def launch(steps):
                    for _ in range(steps):
                        code = lib.rtfs_mouth_rois_u8(_lib.ptr(tab), None, n * K, ROI, ROI, st)
                    assert code == 0
                    return tab

                def grey_of():
                    f = frames.float()
                    return (f[..., 0] * wgt[0] + f[..., 1] * wgt[1] + f[..., 2] * wgt[2] if kind == "bgr" else f).unsqueeze(1)

                def sample(g):
                    res = [F.grid_sample(g, F.affine_grid(th, (n, 1, ROI, ROI), align_corners=False), mode="bilinear", padding_mode="zeros",
                                         align_corners=False).round_().clamp_(0, 255).to(torch.uint8) for th in thetas]
                    return torch.stack(res, 1)[:, :, 0]  # (n,K,96,96)

                def baseline(steps):
                    for _ in range(steps):
                        r = sample(grey_of())
                    return r

                g0 = grey_of()

                def baseline_only(steps):
                    for _ in range(steps):
                        r = sample(g0)
                    return r

                got = datas.mouth_rois(frames, *lms[0], order=order).reshape(n, K, ROI, ROI)
                ref = sample(g0)
                diff = (got.to(torch.int16) - ref.to(torch.int16)).abs()
                stats, steps = measure({"mouth_rois_ms": ours, "launch_ms": launch, "grid_sample_ms": baseline,
                                        "grid_sample_only_ms": baseline_only})
                case = {"jobs": n * K, "frames": n, "faces_per_frame": K, "source": "1280x720 " + ("packed BGR" if kind == "bgr" else "luma plane"),
                        **stats, "steps": steps, "grid_sample_over_mouth_rois": round(stats["grid_sample_ms"][0] / stats["mouth_rois_ms"][0], 2),
                        "bytes": int(got.numel()), "differing_bytes": int((diff != 0).sum()), "max_abs_diff": int(diff.max()),
                        "jobs_per_second": round(n * K / (stats["mouth_rois_ms"][0] / 1000.0))}
                print(json.dumps(case), flush=True)
                out["crop"].append(case)
                del frames, g0, ref, got, diff, roi_out
                torch.cuda.empty_cache()

        from oracle import video_oracle as V
        from oracle.params import load_spec, make_state_dict
        from rtfs_net_amd.configs import audionet_config
        m = R.AVNet(print_macs=False, **audionet_config(4))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
        vm = R.FRCNNVideoModel(print_macs=False)
        vm.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in V.make_video_state_dict(0).items()})
        system = R.System(audio_model=m.cuda().eval(), video_model=vm.cuda().eval())
        rs = np.random.RandomState(0)
        Fw, Fh = WINDOW // SPF, HOP // SPF
        for S in args.streams:
            ids = list(range(S))
            audio = lambda k: [torch.from_numpy((rs.randn(k) * 0.05).astype(np.float32)).cuda() for _ in ids]  # noqa: E731
            cams = lambda k: [torch.randint(0, 256, (k, H, W, 3), dtype=torch.uint8, device=dev) for _ in ids]  # noqa: E731
            first_a, first_f, hop_a, hop_f = audio(WINDOW), cams(Fw), audio(HOP), cams(Fh)
            lm_first = [tuple(x[:, 0] for x in faces(np, Fw, 1, 100 + s)) for s in ids]
            lm_hop = [[tuple(x[:, 0] for x in faces(np, Fh, 1, 200 + 2 * s + t)) for s in ids] for t in (0, 1)]
            kw = dict(window=WINDOW, hop=HOP, max_batch=max(32, S), roi_hw=(ROI, ROI))
            a, b = system.open_camera_streams(S, **kw), system.open_camera_streams(S, **kw)
            a.push_frames(ids, first_a, first_f, [e for e, _ in lm_first], [l for _, l in lm_first])
            b.push(ids, first_a, list(datas.mouth_rois(first_f, [e for e, _ in lm_first], [l for _, l in lm_first])))
            ready = list(datas.mouth_rois(hop_f, [e for e, _ in lm_hop[0]], [l for _, l in lm_hop[0]]))

            def frames_ticks(steps):
                for i in range(steps):
                    r = a.push_frames(ids, hop_a, hop_f, [e for e, _ in lm_hop[i & 1]], [l for _, l in lm_hop[i & 1]])
                return r

            def roi_ticks(steps):
                for _ in range(steps):
                    r = b.push(ids, hop_a, ready)
                return r

            assert all(tuple(r.shape) == (1, HOP) for r in frames_ticks(args.warmup))
            stats, steps = measure({"push_frames_ms": frames_ticks, "push_ready_rois_ms": roi_ticks})
            case = {"streams": S, "frames_per_tick": S * Fh, **stats, "steps": steps,
                    "difference_ms": round(stats["push_frames_ms"][0] - stats["push_ready_rois_ms"][0], 4),
                    "difference_over_push": round(stats["push_frames_ms"][0] / stats["push_ready_rois_ms"][0] - 1.0, 4),
                    "streams_in_real_time": round(S * (HOP / FS) / (stats["push_frames_ms"][0] / 1000.0), 1)}
            print(json.dumps(case), flush=True)
            out["pool"].append(case)
            del a, b, first_f, hop_f, ready
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
