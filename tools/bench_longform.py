#!/usr/bin/env python3
"""AVNet.separate_long on long recordings against the two things it replaces or is bounded by (RTFS-Net-4, B = 1, 16 kHz):

  python tools/bench_longform.py [--seconds 10 60 300] [--steps 5] [--warmup 2] [--out profiles/longform_bench.json]

For each recording length, three measurements, EACH IN A FRESH CHILD PROCESS (so torch.cuda.max_memory_allocated is that call's own):
  separate_long   window 2 s, hop 1 s, max_batch 32: framing kernel + fused forward per chunk + overlap-add kernel
  forward_whole   plain forward on the whole recording (past 8.2 s: the separator composed from the unfused kernels, whole-axis attention;
                  past 256 video frames, 10.2 s, the unfused video-side kernels refuse the track and the case records that error)
  forward_batch   forward on the same number of 2 s windows as a plain batch, in the same chunks of 32: the lower bound, what framing and
                  overlap-add cost on top
Times are HIP events around the call on the current stream, median over the steps, after warm-up calls of the same shape.  Memory:
``base`` = allocated before the call (parameters, packs, the recording), ``peak`` = max_memory_allocated during the timed calls,
``extra`` = peak - base.  A child has a time limit; after a child that ends abnormally (signal, abort, time limit) no further child is
started.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW, HOP, MAX_BATCH, SPF = 32000, 16000, 32, 640
MODES = ("separate_long", "forward_whole", "forward_batch")
ABNORMAL = (124, 134, 137, 139)


def child(mode, seconds, steps, warmup):
    import ctypes

    import numpy as np
    import torch

    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    m = R.AVNet(print_macs=False, **audionet_config(4))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    m = m.cuda().eval()
    L = int(seconds * 16000)
    Tv = -(-L // SPF)
    rs = np.random.RandomState(int(seconds))
    n = ctypes.c_int(0)
    assert R._lib.load().rtfs_longform_plan(L, Tv, WINDOW, HOP, ctypes.byref(n)) == 0
    N = n.value
    if mode == "forward_batch":
        wav = torch.from_numpy((rs.randn(N, WINDOW) * 0.05).astype(np.float32)).cuda()
        emb = torch.from_numpy(rs.randn(N, 512, WINDOW // SPF).astype(np.float32)).cuda()
        call = lambda: [m(wav[c:c + MAX_BATCH], emb[c:c + MAX_BATCH]) for c in range(0, N, MAX_BATCH)]  # noqa: E731
    else:
        wav = torch.from_numpy((rs.randn(1, L) * 0.05).astype(np.float32)).cuda()
        emb = torch.from_numpy(rs.randn(1, 512, Tv).astype(np.float32)).cuda()
        if mode == "separate_long":
            call = lambda: m.separate_long(wav, emb, window=WINDOW, hop=HOP, max_batch=MAX_BATCH)  # noqa: E731
        else:
            call = lambda: m(wav, emb)  # noqa: E731
    with torch.no_grad():
        m(wav[:1, :4096], emb[:1, :, :7])  # parameter packs
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
    print(json.dumps({"mode": mode, "seconds": seconds, "L": L, "windows": N, "ms_median": round(statistics.median(ms), 3),
                      "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "steps": steps, "warmup": warmup, "base_bytes": base,
                      "peak_bytes": peak, "extra_bytes": peak - base, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[10, 60, 300])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=MODES, default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.seconds[0], args.steps, args.warmup)
    out = {"metric": "separate_long (window 2 s, hop 1 s, max_batch 32) vs forward on the whole recording vs forward on as many 2 s windows "
                     "(median ms per call over HIP events; memory from torch.cuda.max_memory_allocated; one fresh process each)",
           "model": "RTFS-Net-4 SRU, B = 1", "cases": []}
    stopped = None
    for seconds in args.seconds:
        for mode in MODES:
            if stopped:
                break
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--seconds", str(seconds), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            try:
                pr = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                stopped = f"{mode} at {seconds} s: time limit of {args.child_timeout} s"
                out["cases"].append({"mode": mode, "seconds": seconds, "error": stopped})
                break
            if pr.returncode == 0:
                out["cases"].append(json.loads(pr.stdout.strip().splitlines()[-1]))
            else:
                err = (pr.stderr.strip().splitlines() or ["?"])[-1][:300]
                out["cases"].append({"mode": mode, "seconds": seconds, "error": f"exit status {pr.returncode}: {err}"})
                if pr.returncode < 0 or pr.returncode in ABNORMAL:
                    stopped = f"{mode} at {seconds} s: exit status {pr.returncode}"
    if stopped:
        out["stopped_after"] = stopped
    by = {(c["seconds"], c["mode"]): c for c in out["cases"] if "ms_median" in c}
    out["summary"] = []
    for seconds in args.seconds:
        sl, fb, fw = (by.get((seconds, k)) for k in MODES[:1] + MODES[2:] + MODES[1:2])
        s = {"seconds": seconds}
        if sl and fb:
            s["separate_long_over_forward_batch_pct"] = round(100.0 * (sl["ms_median"] / fb["ms_median"] - 1.0), 2)
        if sl and fw:
            s["forward_whole_over_separate_long"] = round(fw["ms_median"] / sl["ms_median"], 2)
            s["forward_whole_extra_over_separate_long_extra"] = round(fw["extra_bytes"] / max(sl["extra_bytes"], 1), 2)
        out["summary"].append(s)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
