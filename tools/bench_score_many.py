#!/usr/bin/env python3
"""Scoring many recordings of different lengths in one pooled pass (ALLMetricsTracker.update_many, System.evaluate_many) against the
loop of ``tracker(mix, clean, estimate, key)`` per recording it replaces:

  python tools/bench_score_many.py [--steps 20] [--warmup 3] [--out profiles/score_many_bench.json]

The two sets of tools/bench_many.py (64 recordings of 1 .. 12 s drawn once from RandomState(0); 64 clips of 2 s), n_src 1, 16 kHz.  Per
set, ALL figures come from ONE child process, on the same tensors:
  update_many      one pooled call on the 64 (mix, clean, estimate) triples
  loop             [tracker(mix_r, clean_r, est_r, key_r) for r in range(64)]: existing code, the baseline
  update_batch     (the 2 s set only) the existing batched entry on the stacked (64, 1, 32000) block; stacking not timed
  evaluate_many    System.evaluate_many: separate_many (RTFS-Net-4 SRU, window 2 s, hop 1 s, max_batch 32), then update_many
  separate+loop    separate_many, then the loop
  separate_many    alone, for scale
Times are HIP events around the call (the trackers' device-to-host copies block, so the host time is inside), min / median / max over the
steps after warm-up calls of the same shapes.  No ratio is asserted.  With --estoi each child times only ``update_many`` on a tracker
without and with ``estoi=True`` (a seventh column, one combined STOI + ESTOI call), alternating the two in --rounds rounds; per variant
the median / min / max over the rounds' medians, and the added cost per round.  Each child runs under its own time limit; after a child that ends
abnormally (signal, abort, time limit) no further child is started.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_many import ABNORMAL, FS, HOP, MAX_BATCH, SETS, SPF, WINDOW, lengths  # noqa: E402


def child(name, steps, warmup, estoi_rounds=0):
    import numpy as np
    import torch

    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import audionet_config
    from tests import metrics_oracle as M
    if not estoi_rounds:  # the separator is not part of the --estoi comparison
        m = R.AVNet(print_macs=False, **audionet_config(4))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
        system = R.System(audio_model=m.cuda().eval()).eval()
    Ls = lengths(name)
    rng = np.random.default_rng(2)
    cleans_h = [M.speech_like(rng, L, FS, gaps=[(0.3 * L / FS, 0.4 * L / FS)]) * 0.05 for L in Ls]
    cleans = [torch.from_numpy(c[None]).cuda() for c in cleans_h]
    ests = [torch.from_numpy((c + 0.3 * c.std() * rng.standard_normal(c.shape)).astype(np.float32)[None]).cuda() for c in cleans_h]
    wavs = [torch.from_numpy((c + 0.8 * c.std() * rng.standard_normal(c.shape)).astype(np.float32)).cuda() for c in cleans_h]
    embs = [torch.from_numpy(rng.standard_normal((512, -(-L // SPF))).astype(np.float32)).cuda() for L in Ls]
    keys = [str(r) for r in range(len(Ls))]
    kw = dict(window=WINDOW, hop=HOP, max_batch=MAX_BATCH)

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return {"ms_min": round(min(ms), 3), "ms_median": round(float(np.median(ms)), 3), "ms_max": round(max(ms), 3)}

    def loop(t, estimates):
        for w, c, e, k in zip(wavs, cleans, estimates, keys):
            t(w, c, e, k)

    def separate_then_loop(t):
        loop(t, system.separate_many(wavs, embs, **kw))

    res = {"set": name, "recordings": len(Ls), "seconds_of_audio": round(sum(Ls) / FS, 2), "steps": steps, "warmup": warmup,
           "device": torch.cuda.get_device_name(0)}
    if estoi_rounds:
        with tempfile.TemporaryDirectory() as td, torch.no_grad():
            t5, t6 = R.ALLMetricsTracker(os.path.join(td, "five.csv")), R.ALLMetricsTracker(os.path.join(td, "six.csv"), estoi=True)
            ms = {"update_many": [], "update_many_estoi": []}
            for _ in range(estoi_rounds):
                ms["update_many"].append(timed(lambda: t5.update_many(wavs, cleans, ests, keys))["ms_median"])
                ms["update_many_estoi"].append(timed(lambda: t6.update_many(wavs, cleans, ests, keys))["ms_median"])
            t5.final()
            t6.final()
        res["rounds"] = estoi_rounds
        for k, v in ms.items():
            res[k] = {"ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
        add = [b - a for a, b in zip(ms["update_many"], ms["update_many_estoi"])]
        res["estoi_adds_ms"] = {"median": round(float(np.median(add)), 3), "min": round(min(add), 3), "max": round(max(add), 3)}
        print(json.dumps(res))
        return
    with tempfile.TemporaryDirectory() as td, torch.no_grad():
        t = R.ALLMetricsTracker(os.path.join(td, "m.csv"))
        res["update_many"] = timed(lambda: t.update_many(wavs, cleans, ests, keys))
        res["loop"] = timed(lambda: loop(t, ests))
        if len(set(Ls)) == 1:
            mb, cb, eb = torch.stack(wavs), torch.stack(cleans), torch.stack(ests)
            res["update_batch"] = timed(lambda: t.update_batch(mb, cb, eb, keys))
        res["separate_many"] = timed(lambda: system.separate_many(wavs, embs, **kw))
        res["evaluate_many"] = timed(lambda: system.evaluate_many(wavs, cleans, embs, keys, t, **kw))
        res["separate+loop"] = timed(lambda: separate_then_loop(t))
        t.final()
    res["loop_over_update_many"] = round(res["loop"]["ms_median"] / res["update_many"]["ms_median"], 2)
    res["separate+loop_over_evaluate_many"] = round(res["separate+loop"]["ms_median"] / res["evaluate_many"]["ms_median"], 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", choices=SETS, default=list(SETS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--estoi", action="store_true", help="time update_many without and with the extended-STOI column only")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.child:
        return child(args.sets[0], args.steps, args.warmup, args.rounds if args.estoi else 0)
    out = {"metric": "scoring 64 recordings (SDR, SDRi, SI-SNR, SI-SNRi, STOI; n_src 1, 16 kHz): one pooled update_many against the loop of "
                     "tracker(...) per recording, and the same behind separate_many (RTFS-Net-4 SRU, window 2 s, hop 1 s, max_batch 32); "
                     "HIP events, min / median / max ms per call, one process per set",
           "sets": {name: lengths(name) for name in args.sets}, "cases": []}
    if args.estoi:
        out["metric"] = ("ALLMetricsTracker.update_many on 64 recordings without and with estoi=True (n_src 1, 16 kHz), alternating in "
                         "rounds of one process per set; HIP events, median / min / max of the rounds' medians, ms per call")
    stopped = None
    for name in args.sets:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sets", name, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        if args.estoi:
            cmd += ["--estoi", "--rounds", str(args.rounds)]
        try:
            pr = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
        except subprocess.TimeoutExpired:
            stopped = f"{name}: time limit of {args.child_timeout} s"
            out["cases"].append({"set": name, "error": stopped})
            break
        if pr.returncode == 0:
            out["cases"].append(json.loads(pr.stdout.strip().splitlines()[-1]))
            continue
        err = (pr.stderr.strip().splitlines() or ["?"])[-1][:300]
        out["cases"].append({"set": name, "error": f"exit status {pr.returncode}: {err}"})
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            stopped = f"{name}: exit status {pr.returncode}"
            break
    if stopped:
        out["stopped_after"] = stopped
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if stopped or any("error" in c for c in out["cases"]) else 0


if __name__ == "__main__":
    sys.exit(main())
