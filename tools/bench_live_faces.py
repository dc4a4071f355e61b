#!/usr/bin/env python3
"""Steady-state cost of one tick of a FaceStreamPool (live streams with a different number of faces per slot) against the pools that
can do the same work without it (RTFS-Net-4 SRU, 16 kHz, window 2 s, hop 1 s, every stream delivering 1 s per tick):

  python tools/bench_live_faces.py [--steps 20] [--seconds 1.0] [--rounds 5] [--warmup 3] [--out profiles/live_faces_bench.json]

  ragged   8 streams whose face counts cycle 1, 2, 3, 4 (20 faces) on ``open_streams(max_speakers=4)``, against
           (a) ``open_streams(speakers=4)``: every stream padded to four lip tracks, 32 targets per tick, and
           (b) 20 single-track ``StreamPool`` slots, the audio chunk of a stream pushed once per face;
  equal    (c) 8 streams x 2 faces from the first push on ``open_streams(max_speakers=2)`` against ``open_streams(speakers=2)``: the
           same 16 targets per tick, so what is measured is the extra host and table cost of the births; the faces pool's median is
           reported next to the fixed-K pool's own [min, max] of the same run.

Every stream first delivers one window (2 s, 50 frames per face), then one hop per tick, so each tick has one ready window per
stream; all pools use max_batch = 32, so a tick is one separator call.  Timing as tools/bench_live_speakers.py: a host clock around a
block of calls that ends in a device synchronise, a block at least ``steps`` calls and ``seconds`` long, all sides of a case in
alternating rounds in one process, medians with [min, max].  Before timing, one tick's outputs of the sides are compared (max-rel; the
separator's bar across batch compositions is 1e-4).  Prints one JSON line (and writes it to --out).  Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, SPF, FS, MAX_BATCH = 32000, 16000, 640, 16000, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    if not torch.cuda.is_available():
        sys.exit("bench_live_faces.py measures on the GPU; none found")
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    m = m.cuda().eval()
    rs = np.random.RandomState(0)
    out = {"metric": "FaceStreamPool.push (one ready window per stream) vs the fixed-K and single-track pools on the same faces (window 2 s, "
                     "hop 1 s; host clock around a block of `steps` calls, at least `seconds` long, ending in a synchronise; [median, min, "
                     "max] over alternating rounds in one process, ms per tick)",
           "model": "RTFS-Net-4 SRU", "device": torch.cuda.get_device_name(0), "seconds": args.seconds, "rounds": args.rounds, "cases": []}

    def dev(a):
        return torch.from_numpy(a.astype(np.float32)).cuda()

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            keep = fn()
        torch.cuda.synchronize()
        del keep
        return 1000.0 * (time.perf_counter() - t0) / steps

    def stat(ts):
        return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]

    with torch.no_grad():
        for name, counts in (("ragged_8_streams_1234", [1, 2, 3, 4, 1, 2, 3, 4]), ("equal_8_streams_x2", [2] * 8)):
            S, N, Kmax = len(counts), sum(counts), max(counts)
            ids = list(range(S))
            first_a, hop_a = [dev(rs.randn(WINDOW) * 0.05) for _ in ids], [dev(rs.randn(HOP) * 0.05) for _ in ids]
            first_v = [[dev(rs.randn(512, WINDOW // SPF)) for _ in range(k)] for k in counts]
            hop_v = [[dev(rs.randn(512, HOP // SPF)) for _ in range(k)] for k in counts]
            pad = lambda v: [t + [t[0]] * (Kmax - len(t)) for t in v]  # noqa: E731  the fixed-K pool: every stream padded to Kmax tracks
            faces = m.open_streams(S, window=WINDOW, hop=HOP, max_batch=MAX_BATCH, max_speakers=Kmax)
            for s, k in enumerate(counts):
                for _ in range(k):
                    faces.add_face(s)
            fixed = m.open_streams(S, window=WINDOW, hop=HOP, max_batch=MAX_BATCH, speakers=Kmax)
            hop_vp = pad(hop_v)
            sides = {"faces": lambda: faces.push(ids, hop_a, hop_v), "fixed_k": lambda: fixed.push(ids, hop_a, hop_vp)}
            faces.push(ids, first_a, first_v)
            fixed.push(ids, first_a, pad(first_v))
            one = {"faces": torch.cat([r[j] for r in sides["faces"]() for j in sorted(r)]),
                   "fixed_k": torch.cat([r[j] for r, k in zip(sides["fixed_k"](), counts) for j in range(k)])}
            if name.startswith("ragged"):
                flat = list(range(N))
                single = m.open_streams(N, window=WINDOW, hop=HOP, max_batch=MAX_BATCH)
                rep = lambda a: [a[s] for s, k in enumerate(counts) for _ in range(k)]  # noqa: E731  the audio chunk once per face
                cat = lambda v: [t for tracks in v for t in tracks]  # noqa: E731
                single.push(flat, rep(first_a), cat(first_v))
                ah, vh = rep(hop_a), cat(hop_v)
                sides["single_track"] = lambda: single.push(flat, ah, vh)
                one["single_track"] = torch.cat([r[0] for r in sides["single_track"]()])
            agree = {k: float(f"{float((v - one['faces']).abs().max() / one['faces'].abs().max()):.3e}") for k, v in one.items() if k != "faces"}
            for fn in sides.values():
                timed(fn, args.warmup)
            steps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(sides["faces"], args.steps)))
            ts = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    ts[k].append(timed(fn, steps))
            med = {k: statistics.median(v) for k, v in ts.items()}
            case = {"case": name, "faces_per_stream": counts, "targets_per_tick": {"faces": N, "fixed_k": S * Kmax}, "steps": steps,
                    "max_rel_diff_of_one_tick_vs_faces": agree, "tick_ms": {k: stat(v) for k, v in ts.items()},
                    "faces_over": {k: round(med["faces"] / v, 4) for k, v in med.items() if k != "faces"},
                    "faces_median_inside_fixed_k_min_max": bool(min(ts["fixed_k"]) <= med["faces"] <= max(ts["fixed_k"])),
                    "faces_in_real_time": round(N * (HOP / FS) / (med["faces"] / 1000.0), 1)}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del faces, fixed, sides
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
