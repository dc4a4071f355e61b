#!/usr/bin/env python3
"""AVNet.separate_many on a set of recordings of different lengths against the loop of separate_long per recording it replaces
(RTFS-Net-4 SRU, 16 kHz, window 2 s, hop 1 s, max_batch 32):

  python tools/bench_many.py [--steps 5] [--warmup 2] [--out profiles/many_bench.json]

Two fixed sets of 64 recordings, printed with the result:
  mixed   lengths drawn once from numpy RandomState(0), uniform over [1 s, 12 s] in whole samples
  short   64 clips of 2 s: the short-clip end, where the loop runs 64 batches of one window
For each set, two measurements on the same inputs, EACH IN A FRESH CHILD PROCESS (so torch.cuda.max_memory_allocated is that call's own):
  separate_many   one pooled call
  loop            [separate_long(wav_r, emb_r[None]) for r in range(64)]: existing code, the baseline
Times are HIP events around the call on the current stream, median over the steps, after warm-up calls of the same shapes; windows per
second = sum(N_r) / median.  Memory: ``base`` = allocated before the call (parameters, packs, the recordings), ``peak`` =
max_memory_allocated during the timed calls, ``extra`` = peak - base.  A child has a time limit; after a child that ends abnormally
(signal, abort, time limit) no further child is started.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, MAX_BATCH, SPF, FS, R_SET = 32000, 16000, 32, 640, 16000, 64
SETS = ("mixed", "short")
MODES = ("separate_many", "loop")
ABNORMAL = (124, 134, 137, 139)


def lengths(name):
    import numpy as np
    if name == "short":
        return [2 * FS] * R_SET
    return [int(v) for v in np.random.RandomState(0).randint(1 * FS, 12 * FS + 1, R_SET)]


def windows(L):
    return 1 if L <= WINDOW else 1 + -(-(L - WINDOW) // HOP)


def child(mode, name, steps, warmup):
    import numpy as np
    import torch

    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    m = m.cuda().eval()
    Ls = lengths(name)
    rs = np.random.RandomState(1)
    wavs = [torch.from_numpy((rs.randn(L) * 0.05).astype(np.float32)).cuda() for L in Ls]
    embs = [torch.from_numpy(rs.randn(512, -(-L // SPF)).astype(np.float32)).cuda() for L in Ls]
    kw = dict(window=WINDOW, hop=HOP, max_batch=MAX_BATCH)
    if mode == "separate_many":
        call = lambda: m.separate_many(wavs, embs, **kw)  # noqa: E731
    else:
        call = lambda: [m.separate_long(w, e[None], **kw) for w, e in zip(wavs, embs)]  # noqa: E731
    with torch.no_grad():
        m(wavs[0][None, :4096], embs[0][None, :, :7])  # parameter packs
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ev = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            y = call()
            b.record()
            ev.append((a, b))
            del y
        torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    peak = torch.cuda.max_memory_allocated()
    S = sum(windows(L) for L in Ls)
    med = statistics.median(ms)
    print(json.dumps({"mode": mode, "set": name, "recordings": len(Ls), "windows": S, "seconds_of_audio": round(sum(Ls) / FS, 2),
                      "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "ms_all": [round(v, 3) for v in ms],
                      "windows_per_s": round(1000.0 * S / med, 1), "ms_per_window": round(med / S, 4), "steps": steps, "warmup": warmup,
                      "base_bytes": base, "peak_bytes": peak, "extra_bytes": peak - base, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", choices=SETS, default=list(SETS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=MODES, default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.sets[0], args.steps, args.warmup)
    out = {"metric": "separate_many vs the loop of separate_long per recording on the same 64 recordings (window 2 s, hop 1 s, max_batch 32; "
                     "median ms per call over HIP events; memory from torch.cuda.max_memory_allocated; one fresh process each)",
           "model": "RTFS-Net-4 SRU", "sets": {name: lengths(name) for name in args.sets}, "cases": []}
    for name in args.sets:
        print(f"set {name}: lengths in samples {out['sets'][name]}", flush=True)
    stopped = None
    for name in args.sets:
        for mode in MODES:
            if stopped:
                break
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--sets", name, "--steps", str(args.steps), "--warmup",
                   str(args.warmup)]
            try:
                pr = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                stopped = f"{mode} on {name}: time limit of {args.child_timeout} s"
                out["cases"].append({"mode": mode, "set": name, "error": stopped})
                break
            if pr.returncode == 0:
                out["cases"].append(json.loads(pr.stdout.strip().splitlines()[-1]))
            else:
                err = (pr.stderr.strip().splitlines() or ["?"])[-1][:300]
                out["cases"].append({"mode": mode, "set": name, "error": f"exit status {pr.returncode}: {err}"})
                if pr.returncode < 0 or pr.returncode in ABNORMAL:
                    stopped = f"{mode} on {name}: exit status {pr.returncode}"
    if stopped:
        out["stopped_after"] = stopped
    by = {(c["set"], c["mode"]): c for c in out["cases"] if "ms_median" in c}
    out["summary"] = []
    for name in args.sets:
        many, loop = by.get((name, "separate_many")), by.get((name, "loop"))
        if many and loop:
            out["summary"].append({"set": name, "loop_over_separate_many": round(loop["ms_median"] / many["ms_median"], 3),
                                   "separate_many_ms": [many["ms_min"], many["ms_median"], many["ms_max"]],
                                   "loop_ms": [loop["ms_min"], loop["ms_median"], loop["ms_max"]],
                                   "extra_bytes_many_over_loop": round(many["extra_bytes"] / max(loop["extra_bytes"], 1), 2)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
