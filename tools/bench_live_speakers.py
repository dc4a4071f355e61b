#!/usr/bin/env python3
"""Steady-state cost of one tick of a SpeakerStreamPool (S streams with K faces each, one audio pass per window) against the same work
done with single-track slots (RTFS-Net-4 SRU, 16 kHz, window 2 s, hop 1 s, every stream delivering 1 s per tick):

  python tools/bench_live_speakers.py [--cases 1x2 8x2 16x2 8x4] [--steps 20] [--seconds 1.0] [--rounds 5] [--warmup 3]
                                      [--out profiles/live_speakers_bench.json]

For S streams with K faces, every stream first delivers one window (2 s of audio, 50 lip-embedding frames per face), then one hop per
tick (1 s, 25 frames per face), so each tick has exactly S ready windows with K targets each and returns (K, 16000) per stream.  The
baseline is a ``StreamPool`` with S * K slots, slot s K + k fed stream s's audio chunk and face k's lips: the audio pushed, stored,
framed and run through the audio-only prefix K times - the only way to separate every face of a stream without the speaker pool.
That path is not touched by the speaker pool, so both are timed in the same process.  Both use max_batch = S * K, so each tick is one
separator call on S * K targets.  Timing: a host clock around a block of calls that ends in a device synchronise (a push has host
work - the planner, the table upload - that device events would not see); a block is at least ``steps`` calls and ``seconds`` long;
``rounds`` alternating rounds after warm-up of the same shapes; medians with min and max.  Before timing the two pools' outputs of one
tick are compared (max-rel, the separator's bar across batch compositions is 1e-4).  Prints one JSON line (and writes it to --out).
Needs a GPU: there is no CPU figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, SPF, FS = 32000, 16000, 640, 16000


def state_bytes(pool):
    return 4 * (pool._aring.numel() + pool._vring.numel() + pool._acc.numel()) // pool.slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1x2", "8x2", "16x2", "8x4"], help="SxK: streams x faces per stream")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.lower().split("x")) for c in args.cases]

    import numpy as np
    import torch

    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    if not torch.cuda.is_available():
        sys.exit("bench_live_speakers.py measures on the GPU; none found")
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    m = m.cuda().eval()
    rs = np.random.RandomState(0)
    out = {"metric": "SpeakerStreamPool.push (S streams, K faces each, one ready window per stream) vs StreamPool.push on S*K single-track "
                     "slots with the audio chunk pushed K times (window 2 s, hop 1 s; host clock around a block of `steps` calls, at least "
                     "`seconds` long, ending in a synchronise, median [min, max] over alternating rounds, ms per tick)",
           "model": "RTFS-Net-4 SRU", "device": torch.cuda.get_device_name(0), "seconds": args.seconds, "rounds": args.rounds, "cases": []}

    def dev(a):
        return torch.from_numpy(a.astype(np.float32)).cuda()

    with torch.no_grad():
        for S, K in cases:
            ids, flat = list(range(S)), list(range(S * K))
            first_a = [dev(rs.randn(WINDOW) * 0.05) for _ in ids]
            first_v = [[dev(rs.randn(512, WINDOW // SPF)) for _ in range(K)] for _ in ids]
            hop_a = [dev(rs.randn(HOP) * 0.05) for _ in ids]
            hop_v = [[dev(rs.randn(512, HOP // SPF)) for _ in range(K)] for _ in ids]
            rep = lambda a: [a[s] for s in ids for _ in range(K)]  # noqa: E731  the audio chunk of stream s, K times
            cat = lambda v: [v[s][k] for s in ids for k in range(K)]  # noqa: E731
            pool = m.open_streams(S, window=WINDOW, hop=HOP, max_batch=S * K, speakers=K)
            base = m.open_streams(S * K, window=WINDOW, hop=HOP, max_batch=S * K)
            a1, v1, ah, vh = rep(first_a), cat(first_v), rep(hop_a), cat(hop_v)
            res, ref = pool.push(ids, first_a, first_v), base.push(flat, a1, v1)
            assert all(tuple(r.shape) == (K, HOP) for r in res) and all(tuple(r.shape) == (1, HOP) for r in ref)
            res, ref = pool.push(ids, hop_a, hop_v), base.push(flat, ah, vh)
            got, want = torch.stack(res).reshape(S * K, HOP), torch.cat(ref)
            agree = float((got - want).abs().max() / want.abs().max())

            def ticks(n):
                for _ in range(n):
                    r = pool.push(ids, hop_a, hop_v)
                return r

            def base_ticks(n):
                for _ in range(n):
                    r = base.push(flat, ah, vh)
                return r

            def timed(fn, steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                keep = fn(steps)
                torch.cuda.synchronize()
                del keep
                return 1000.0 * (time.perf_counter() - t0) / steps

            ticks(args.warmup)
            base_ticks(args.warmup)
            steps = max(args.steps, math.ceil(1000.0 * args.seconds / timed(ticks, args.steps)))
            t_new, t_old = [], []
            for _ in range(args.rounds):
                t_new.append(timed(ticks, steps))
                t_old.append(timed(base_ticks, steps))
            new, old = statistics.median(t_new), statistics.median(t_old)
            case = {"streams": S, "speakers": K, "steps": steps, "max_rel_diff_of_one_tick": float(f"{agree:.3e}"),
                    "speaker_tick_ms": [round(new, 4), round(min(t_new), 4), round(max(t_new), 4)],
                    "single_track_tick_ms": [round(old, 4), round(min(t_old), 4), round(max(t_old), 4)],
                    "speaker_over_single_track": round(new / old, 4),
                    "faces_in_real_time": round(S * K * (HOP / FS) / (new / 1000.0), 1),
                    "state_bytes_per_stream": state_bytes(pool), "state_bytes_per_stream_single_track": K * state_bytes(base)}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            pool.reset(ids)
            base.reset(flat)
            del pool, base
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
