#!/usr/bin/env python3
"""Training mixtures on the device (datas.mix_batch, csrc/k_mix.hip) against what a user wrote before it: torch slicing and ``stack``,
energies, a gain, the sum, then ``datas.normalize_mixture``.

  python tools/bench_mix.py [--steps 30] [--warmup 5] [--rounds 5] [--kernel-stats CSV] [--out profiles/mix_bench.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o x -- python tools/bench_mix.py --trace-only     (a run of its own)

Cases: J = 2 (a target and one interferer at a drawn SNR), n_out = 1, normalize=True, 2 s segments out of 32 utterances of 3 .. 12 s at
16 kHz, B = 4, 16, 64; the same seeded recipes and the same device-resident utterances for both sides, in the same process.  Whole-call
figures: a host clock around the call, ending in a device synchronise; ``--rounds`` rounds that alternate the two sides, ``--steps`` calls
each after ``--warmup``; the median over all calls and the range of the per-round medians (the spread).  The planned call is also split:
the host plan alone (no device work), the table upload alone (host clock, synchronised) and the two launches alone (device events around
``rtfs_mix_f32`` on an uploaded table).  ``System.mix_batch`` (audio, ROI slices, the "train" lips launch) is timed the same way next to
one ``optimization_step`` of RTFS-Net-4 at batch 4 x 2 s on its batch.
Bytes: what the definition moves, from the shapes: J segment reads in each pass (the references of this recipe are the target's segment,
read a second time from cache) and 1 + n_out rows written by pass 2.  Pass-2 bandwidth needs the kernel's own time: ``--kernel-stats``
takes the kernel-stats CSV of a ``--trace-only`` run under rocprofv3 (a separate run: tracing slows the host; it launches the B = 64 case
100 times); without it the figure is reported as not measured, and the bytes of both passes over the event time of both launches is
given for what it is.  A measurement needs the GPU: without one the tool fails.  Prints one JSON
line (and writes it to --out)."""
import argparse
import csv
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, J, N_OUT, BATCHES = 32000, 2, 1, (4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="only run the two launches of the B = 64 case 100 times (for a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="kernel-stats CSV of a --trace-only run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--skip-step", action="store_true", help="leave out System.mix_batch next to optimization_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import rtfs_net_amd as R
    from rtfs_net_amd import _lib, datas
    assert torch.cuda.is_available(), "bench_mix.py measures on the GPU only"
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    secs = [3 + (9 * i) // 31 for i in range(32)]
    pool = [(0.05 * torch.randn(16000 * s, generator=g)).cuda() for s in secs]
    lengths = [int(p.shape[0]) for p in pool]

    def sync_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def alternate(fns):
        """{name: fn} -> {name: {"ms_median", "round_medians_min", "round_medians_max", "calls"}}, the sides alternating round by round"""
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

    def torch_chain(rec):
        """What a user writes today, float32 torch ops + the two launches of normalize_mixture."""
        t = torch.stack([pool[s][o:o + L] for s, o in zip(rec.src[:, 0].tolist(), rec.start[:, 0].tolist())])
        n = torch.stack([pool[s][o:o + L] for s, o in zip(rec.src[:, 1].tolist(), rec.start[:, 1].tolist())])
        a = torch.tensor(rec.a[:, 1:], dtype=torch.float32, device=t.device)
        gain = a * torch.sqrt((t * t).sum(-1, keepdim=True) / (n * n).sum(-1, keepdim=True))
        mix, tgt = datas.normalize_mixture(t + gain * n, t.unsqueeze(1))
        return mix, tgt

    def launches(rec):
        table, nbytes, B, n_out, dev = datas._mix_plan(pool, rec, L, N_OUT)
        tab = table.to(dev)
        mixture, out = torch.empty(B, L, device=dev), torch.empty(B, n_out, L, device=dev)
        stats, ws = torch.empty(B, 6, device=dev, dtype=torch.float64), torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)

        def fn():
            code = lib.rtfs_mix_f32(_lib.ptr(tab), _lib.ptr(mixture), _lib.ptr(out), _lib.ptr(stats), B, L, n_out, 1, 1e-8, _lib.ptr(ws), nbytes,
                                    _lib.stream_of(tab))
            assert code == 0, code
        return fn, table

    result = {"tool": "bench_mix", "device": torch.cuda.get_device_name(0), "length": L, "slots": J, "n_out": N_OUT, "normalize": True,
              "utterance_seconds": [min(secs), max(secs)], "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "cases": {}}
    recipes = {B: datas.draw_mix_recipe(lengths, B, L, n_src=J, rng=random.Random(B)) for B in BATCHES}
    if args.trace_only:
        fn, _ = launches(recipes[max(BATCHES)])
        for _ in range(100):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "bench_mix", "trace_only": True, "batch": max(BATCHES), "launch_pairs": 100}))
        return

    pass2 = {}
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "mix_apply_kernel" in row["Name"] or "mix_moments_kernel" in row["Name"]:
                    pass2["mix_apply_kernel" if "mix_apply_kernel" in row["Name"] else "mix_moments_kernel"] = {
                        "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3), "min_us": round(float(row["MinNs"]) / 1e3, 3),
                        "max_us": round(float(row["MaxNs"]) / 1e3, 3)}

    for B in BATCHES:
        rec = recipes[B]
        planned = lambda: datas.mix_batch(pool, rec, L, n_out=N_OUT, normalize=True)
        got, want = planned(), torch_chain(rec)
        torch.cuda.synchronize()
        err = max(float((got[0] - want[0]).abs().max() / want[0].abs().max()), float((got[1] - want[1]).abs().max() / want[1].abs().max()))
        assert err <= 1e-4, f"B {B}: the two sides disagree, max-rel {err:.3e}"
        case = alternate({"mix_batch_whole_call": planned, "torch_chain_whole_call": lambda: torch_chain(rec)})
        plan_ms = []
        for _ in range(args.steps * args.rounds):
            t = time.perf_counter()
            datas._mix_plan(pool, rec, L, N_OUT)
            plan_ms.append((time.perf_counter() - t) * 1e3)
        fn, table = launches(rec)
        up = [sync_ms(lambda: table.to("cuda")) for _ in range(args.steps * args.rounds)]
        case["host_plan"] = {"ms_median": round(statistics.median(plan_ms), 4), "ms_min": round(min(plan_ms), 4), "ms_max": round(max(plan_ms), 4)}
        case["table_upload_synchronised"] = {"ms_median": round(statistics.median(up), 4), "ms_min": round(min(up), 4), "ms_max": round(max(up), 4),
                                             "bytes": int(table.numel()) * 8}
        case["two_launches_events"] = event_ms(fn, args.steps * args.rounds)
        p1 = B * L * 4 * J                      # pass 1: J segments (the references are the target's segment again)
        p2 = B * L * 4 * (J + 1 + N_OUT)        # pass 2: J segments read, 1 + n_out rows written
        case["bytes"] = {"pass1": p1, "pass2": p2}
        case["both_passes_GBps_over_event_time"] = round((p1 + p2) / (case["two_launches_events"]["ms_median"] * 1e-3) / 1e9, 2)
        case["speedup_whole_call"] = round(case["torch_chain_whole_call"]["ms_median"] / case["mix_batch_whole_call"]["ms_median"], 3)
        case["max_rel_between_sides"] = err
        result["cases"][f"B{B}"] = case
    if pass2:  # a --trace-only run holds the largest batch only
        result["kernel_stats_batch"], result["kernel_stats"] = max(BATCHES), pass2
        for name, key in (("mix_moments_kernel", "pass1"), ("mix_apply_kernel", "pass2")):
            if name in pass2:
                nbytes = result["cases"][f"B{max(BATCHES)}"]["bytes"][key]
                result[f"{key}_GBps"] = round(nbytes / (pass2[name]["average_us"] * 1e-6) / 1e9, 2)
    else:
        result["pass2_GBps"] = "not measured (needs --kernel-stats from a --trace-only run under rocprofv3)"

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
        rois = [torch.randint(0, 256, (25 * s, 96, 96), generator=g, dtype=torch.uint8).cuda() for s in secs]
        rng = random.Random(1)
        batch = system.mix_batch(pool, rois, length=L, rng=rng)
        step = alternate({"system_mix_batch": lambda: system.mix_batch(pool, rois, length=L, rng=rng),
                          "optimization_step": lambda: system.optimization_step(batch, 0)})
        step["mix_share_of_mix_plus_step"] = round(step["system_mix_batch"]["ms_median"] /
                                                   (step["system_mix_batch"]["ms_median"] + step["optimization_step"]["ms_median"]), 4)
        result["training_step_batch4"] = step

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
