#!/usr/bin/env python3
"""Integrated loudness on the device (datas.loudness_many, csrc/k_loudness.hip) against the two routes a user has without it.

  python tools/bench_loudness.py [--steps 20] [--warmup 3] [--rounds 5] [--kernel-stats CSV] [--out profiles/loudness_bench.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o x -- python tools/bench_loudness.py --trace-only   (a run of its own)

Cases, 16 kHz, float32 recordings resident on the device: 64 x 2 s, and 64 recordings of 1 .. 12 s.  Sides, in the same process on the
same recordings:
  loudness_many   the planned call: host plan, one table upload, four launches, nothing read back
  host_scipy      (A) today's route: every recording copied to the host, ``scipy.signal.lfilter`` twice, numpy blocks and gates
  torch_fft       (B) the strongest stock-torch route on the device: the rows padded into one float64 batch, ``rfft``, times the
                  sampled frequency response of the two biquads, ``irfft``, hop sums, ``unfold``, masked gates
Whole-call figures: a host clock around the call, ending in a device synchronise; ``--rounds`` rounds that alternate the sides,
``--steps`` calls each after ``--warmup``; the median over all calls and the range of the per-round medians (the spread).  Both ratios
are reported whichever way they fall.  The planned call is also split: the host plan alone, the table upload alone (synchronised) and
the four launches alone (device events around ``rtfs_loudness_f32`` on an uploaded table).  Kernel times come from a trace in a run
of its own: ``--kernel-stats`` takes the kernel-stats CSV of a ``--trace-only`` run under rocprofv3 (it launches the 1 .. 12 s case
100 times); without it they are reported as not measured.  ``System.mix_batch(loudness=...)`` is timed next to one
``optimization_step`` of RTFS-Net-4 at batch 4 x 2 s on its batch.  A measurement needs the GPU: without one the tool fails.  Prints
one JSON line (and writes it to --out)."""
import argparse
import csv
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, R_POOL = 16000, 64
KERNELS = ("loud_ends_kernel", "loud_scan_kernel", "loud_energy_kernel", "loud_gate_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="only run the four launches of the 1 .. 12 s case 100 times (for a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="kernel-stats CSV of a --trace-only run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--skip-step", action="store_true", help="leave out System.mix_batch(loudness=) next to optimization_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from scipy import signal

    import rtfs_net_amd as R
    from rtfs_net_amd import _lib, datas
    from tests import loudness_oracle as LO
    assert torch.cuda.is_available(), "bench_loudness.py measures on the GPU only"
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    H = FS // 10

    def speechlike(n):
        """Noise under a slow envelope with pauses, so that both gates have work."""
        t = torch.arange(n) / FS
        env = (0.55 + 0.45 * torch.sin(2 * math.pi * 0.7 * t)).clamp(min=0.0) * (torch.sin(2 * math.pi * 0.13 * t + 1.0) > -0.6)
        return (0.05 * torch.randn(n, generator=g) * (env + 1e-3)).float()

    pools = {"64x2s": [speechlike(2 * FS).cuda() for _ in range(R_POOL)],
             "64x1to12s": [speechlike(FS + (11 * FS * i) // (R_POOL - 1)).cuda() for i in range(R_POOL)]}

    def sync_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def alternate(fns):
        per = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                for _ in range(args.warmup):
                    fn()
                per[k].append([sync_ms(fn) for _ in range(args.steps)])
        out = {}
        for k, rounds in per.items():
            meds = [statistics.median(r) for r in rounds]
            out[k] = {"ms_median": round(statistics.median([v for r in rounds for v in r]), 4), "round_medians_min": round(min(meds), 4),
                      "round_medians_max": round(max(meds), 4), "calls": args.rounds * args.steps}
        return out

    def event_ms(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": steps}

    biquads = LO.biquads(FS)

    def host_scipy(wavs):
        out = []
        for w in wavs:
            y = w.cpu().numpy().astype(np.float64)
            for b, a in biquads:
                y = signal.lfilter(b, a, y)
            nh = len(y) // H
            E = (y[:nh * H] ** 2).reshape(nh, H).sum(axis=1)
            out.append(LO.gate(LO.blocks(E, H))[0])
        return np.array(out)

    def torch_fft(wavs):
        lengths = [int(w.shape[0]) for w in wavs]
        n = 1 << (max(lengths) + FS - 1).bit_length()      # a second of room for the tail of the impulse response
        dev = wavs[0].device
        x = torch.zeros(len(wavs), n, dtype=torch.float64, device=dev)
        for r, w in enumerate(wavs):
            x[r, :lengths[r]] = w
        zinv = torch.exp(-2j * math.pi * torch.arange(n // 2 + 1, dtype=torch.float64, device=dev) / n)
        resp = torch.ones_like(zinv)
        for b, a in biquads:
            resp = resp * (b[0] + b[1] * zinv + b[2] * zinv * zinv) / (a[0] + a[1] * zinv + a[2] * zinv * zinv)
        y = torch.fft.irfft(torch.fft.rfft(x) * resp, n=n)
        nhm = max(lengths) // H
        E = (y[:, :nhm * H] ** 2).reshape(len(wavs), nhm, H).sum(-1)
        z = E.unfold(1, 4, 1).sum(-1) / (4 * H)
        nb = torch.tensor([l // H - 3 for l in lengths], device=dev)
        live = torch.arange(nhm - 3, device=dev)[None, :] < nb[:, None]
        a1 = live & (z > LO.ABS_GATE)
        rel = 0.1 * (z * a1).sum(-1) / a1.sum(-1)
        k = a1 & (z > rel[:, None])
        return -0.691 + 10.0 * torch.log10((z * k).sum(-1) / k.sum(-1))

    def launches(wavs):
        table, totals, nbytes, _, dev = datas._loud_plan(wavs, FS, "bench")
        tab = table.to(dev)
        out = torch.empty(len(wavs), 2, device=dev, dtype=torch.float64)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)

        def fn():
            code = lib.rtfs_loudness_f32(_lib.ptr(tab), _lib.ptr(table), _lib.ptr(out), None, _lib.ptr(ws), nbytes, _lib.stream_of(tab))
            assert code == 0, code
        return fn, table, totals, nbytes

    if args.trace_only:
        fn, _, _, _ = launches(pools["64x1to12s"])
        for _ in range(100):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "bench_loudness", "trace_only": True, "case": "64x1to12s", "calls_of_four_launches": 100}))
        return

    result = {"tool": "bench_loudness", "device": torch.cuda.get_device_name(0), "sample_rate": FS, "recordings": R_POOL, "steps": args.steps,
              "warmup": args.warmup, "rounds": args.rounds, "cases": {}}
    for name, wavs in pools.items():
        planned = lambda: datas.loudness_many(wavs, FS)
        got = planned().cpu().numpy()
        a, b = host_scipy(wavs), torch_fft(wavs).cpu().numpy()
        err_a, err_b = float(np.abs(got - a).max()), float(np.abs(got - b).max())
        assert np.isfinite(got).all() and err_a <= 1e-9 and err_b <= 1e-6, (name, err_a, err_b)
        case = alternate({"loudness_many_whole_call": planned, "host_scipy_whole_call": lambda: host_scipy(wavs),
                          "torch_fft_whole_call": lambda: torch_fft(wavs)})
        plan_ms = []
        for _ in range(args.steps * args.rounds):
            t = time.perf_counter()
            datas._loud_plan(wavs, FS, "bench")
            plan_ms.append((time.perf_counter() - t) * 1e3)
        fn, table, totals, nbytes = launches(wavs)
        up = [sync_ms(lambda: table.to("cuda")) for _ in range(args.steps * args.rounds)]
        case["host_plan"] = {"ms_median": round(statistics.median(plan_ms), 4), "ms_min": round(min(plan_ms), 4), "ms_max": round(max(plan_ms), 4)}
        case["table_upload_synchronised"] = {"ms_median": round(statistics.median(up), 4), "ms_min": round(min(up), 4), "ms_max": round(max(up), 4),
                                             "bytes": int(table.numel()) * 8}
        case["four_launches_events"] = event_ms(fn, args.steps * args.rounds)
        case["samples"], case["hops"], case["workspace_bytes"] = totals[2], totals[0], nbytes
        case["lufs_range"] = [round(float(got.min()), 3), round(float(got.max()), 3)]
        case["max_abs_db_against_host_scipy"], case["max_abs_db_against_torch_fft"] = err_a, err_b
        me = case["loudness_many_whole_call"]["ms_median"]
        case["ratio_host_scipy_over_loudness_many"] = round(case["host_scipy_whole_call"]["ms_median"] / me, 3)
        case["ratio_torch_fft_over_loudness_many"] = round(case["torch_fft_whole_call"]["ms_median"] / me, 3)
        result["cases"][name] = case

    if args.kernel_stats:
        stats = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k in row["Name"]:
                        stats[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3),
                                    "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
        result["kernel_stats_case"], result["kernel_stats"] = "64x1to12s", stats
    else:
        result["kernel_stats"] = "not measured (needs --kernel-stats from a --trace-only run under rocprofv3)"

    if not args.skip_step:
        import copy
        from rtfs_net_amd.configs import RTFS4_AUDIONET
        torch.manual_seed(0)
        model = R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET)).cuda().train()
        video = R.FRCNNVideoModel(print_macs=False).cuda().eval()
        loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
        opt = R.make_optimizer([p for p in model.parameters() if p.requires_grad], optimizer="adamw", lr=1e-3, weight_decay=0.1)
        system = R.System(audio_model=model, video_model=video, optimizer=opt, loss_func={"train": loss, "val": loss},
                          config={"training": {"batch_size": 4}})
        wavs = [w for w in pools["64x1to12s"] if w.shape[0] >= 3 * FS]
        rois = [torch.randint(0, 256, (int(w.shape[0]) // 640, 96, 96), generator=g, dtype=torch.uint8).cuda() for w in wavs]
        utter = datas.loudness_many(wavs, FS).tolist()     # the one readback, once per dataset
        rng = random.Random(1)
        kw = dict(length=2 * FS, rng=rng, loudness=(-33.0, -25.0), utter_lufs=utter)
        batch = system.mix_batch(wavs, rois, **kw)
        step = alternate({"system_mix_batch_loudness": lambda: system.mix_batch(wavs, rois, **kw),
                          "system_mix_batch_snr": lambda: system.mix_batch(wavs, rois, length=2 * FS, rng=rng),
                          "optimization_step": lambda: system.optimization_step(batch, 0)})
        step["mix_share_of_mix_plus_step"] = round(step["system_mix_batch_loudness"]["ms_median"] /
                                                   (step["system_mix_batch_loudness"]["ms_median"] + step["optimization_step"]["ms_median"]), 4)
        result["training_step_batch4"] = step

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
