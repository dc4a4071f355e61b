#!/usr/bin/env python3
"""Reverberant training mixtures on the device (datas.mix_batch(rirs=...), csrc/k_reverb.hip in front of csrc/k_mix.hip) against the chain
a user writes today: per source a history-aware slice, zero padding, float32 ``torch.fft.rfft`` / ``irfft``, a slice, then
``datas.mix_batch`` on the results.

  python tools/bench_reverb.py [--steps 20] [--warmup 5] [--rounds 3] [--kernel-stats CSV] [--out profiles/reverb_bench.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o x -- python tools/bench_reverb.py --trace-only     (a run of its own)

Cases: J = 2 (a target and one interferer at a drawn SNR, both reverberant, the interferer's reference the target's image), n_out = 1,
normalize=True, 2 s segments out of 32 utterances of 3 .. 12 s at 16 kHz, B in {4, 16, 64} x N in {1024, 4096, 8192} taps
(``datas.synthetic_rir``, 16 RIRs, offset = the direct path); the same seeded recipes and device-resident utterances for both sides, in
the same process.  The FFT chain is the strong form of what the issue describes: the 2 B slices are stacked and go through ONE batched
rfft / irfft of the next power of two, and the RIR spectra are computed once outside the timed region (a user would cache them).
Whole-call figures: a host clock around the call, ending in a device synchronise; ``--rounds`` rounds that alternate the two sides,
``--steps`` calls each after ``--warmup``; the median over all calls and the range of the per-round medians.  The reverb launch alone is
timed by device events around ``rtfs_reverb_f32`` on an uploaded table.  Its float64 rate needs the kernel's own time: ``--kernel-stats``
takes the kernel-stats CSV of a ``--trace-only`` run under rocprofv3 (the B = 64, N = 8192 launch 20 times); the operations are the
2 S L N of the definition.  Errors: the images of both sides against a float64 FFT convolution (torch, on the device), max |difference|
over max |reference|, at B = 4.  ``System.mix_batch`` with RIRs is timed next to one ``optimization_step`` of RTFS-Net-4 at batch 4 x 2 s.
A measurement needs the GPU: without one the tool fails.  Prints one JSON line (and writes it to --out)."""
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

L, J, N_OUT, BATCHES, TAPS, N_RIRS = 32000, 2, 1, (4, 16, 64), (1024, 4096, 8192), 16
VENDOR_FP64_VECTOR_TFLOPS = 78.6  # AMD's data-sheet figure for the MI355X; never measured on these machines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true", help="only run the reverb launch of the B = 64, N = 8192 case 20 times (for a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="kernel-stats CSV of a --trace-only run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--skip-step", action="store_true", help="leave out System.mix_batch next to optimization_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rtfs_net_amd as R
    from rtfs_net_amd import _lib, datas
    assert torch.cuda.is_available(), "bench_reverb.py measures on the GPU only"
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    secs = [3 + (9 * i) // 31 for i in range(32)]
    pool = [(0.05 * torch.randn(16000 * s, generator=g)).cuda() for s in secs]
    lengths = [int(p.shape[0]) for p in pool]
    rng = np.random.RandomState(0)
    rirs = {N: datas.load_rirs([datas.synthetic_rir(N, 0.2 + 0.03 * i, delay=8 + 3 * i, rng=rng) for i in range(N_RIRS)]) for N in TAPS}

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

    def windows(rec, N, dtype):
        """The (2 B, L + N - 1) history-aware slices of the recipe's slots, zeros where the room is silent."""
        rows = []
        for s, p, o in zip(rec.src.ravel().tolist(), rec.start.ravel().tolist(), rec.rir_offset.ravel().tolist()):
            lo, hi = p + o - (N - 1), p + o + L
            x = pool[s][max(lo, 0):min(hi, lengths[s])].to(dtype)
            rows.append(torch.nn.functional.pad(x, (max(-lo, 0), max(hi - lengths[s], 0))))
        return torch.stack(rows)

    def fft_images(rec, N, spectra, dtype=torch.float32):
        nfft = 1 << (L + N - 2).bit_length()
        X = torch.fft.rfft(windows(rec, N, dtype), n=nfft)
        return torch.fft.irfft(X * spectra[torch.as_tensor(rec.rir.ravel(), device=X.device)], n=nfft)[:, N - 1:N - 1 + L]

    def fft_chain(rec, N, spectra, dry):
        images = fft_images(rec, N, spectra)
        return datas.mix_batch(list(images.unbind(0)), dry, L, n_out=N_OUT, normalize=True)

    def reverb_launch(rec, N):
        views = rirs[N][0]
        S = rec.src.size
        jobs = np.zeros((S, datas.REVERB_RECIPE_WORDS), np.int64)
        for i, (s, p, r, o) in enumerate(zip(rec.src.ravel(), rec.start.ravel(), rec.rir.ravel(), rec.rir_offset.ravel())):
            jobs[i] = [pool[s].data_ptr(), lengths[s], 0, p, views[r].data_ptr(), N, o]
        table = torch.empty(S * datas.REVERB_JOB_WORDS, dtype=torch.int64)
        assert lib.rtfs_reverb_plan(jobs.ctypes.data, S, L, _lib.ptr(table), None) == 0
        tab, images = table.cuda(), torch.empty(S, L, device="cuda")

        def fn():
            code = lib.rtfs_reverb_f32(_lib.ptr(tab), _lib.ptr(images), S, L, _lib.stream_of(tab))
            assert code == 0, code
        return fn, S

    def recipe(B, N):
        views, offsets = rirs[N]
        return datas.draw_mix_recipe(lengths, B, L, n_src=J, rng=random.Random(B), n_rirs=N_RIRS, rir_offsets=offsets)

    result = {"tool": "bench_reverb", "device": torch.cuda.get_device_name(0), "length": L, "slots": J, "n_out": N_OUT, "normalize": True,
              "utterance_seconds": [min(secs), max(secs)], "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
              "baseline": "stacked history-aware slices, one batched float32 rfft / irfft, cached RIR spectra, then datas.mix_batch", "cases": {}}
    if args.trace_only:
        fn, S = reverb_launch(recipe(max(BATCHES), max(TAPS)), max(TAPS))
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "bench_reverb", "trace_only": True, "batch": max(BATCHES), "taps": max(TAPS), "images": S, "launches": 20}))
        return

    for N in TAPS:
        views, offsets = rirs[N]
        nfft = 1 << (L + N - 2).bit_length()
        spectra = torch.fft.rfft(torch.stack(views), n=nfft)
        spectra64 = torch.fft.rfft(torch.stack(views).double(), n=nfft)
        for B in BATCHES:
            rec = recipe(B, N)
            # the dry recipe of the FFT side: slot (b, j) is row b J + j of the image tensor, the reference the row's target image
            idx = np.arange(B * J).reshape(B, J)
            dry = datas.MixRecipe(idx, np.zeros((B, J), np.int64), rec.a, np.where(rec.ref_src >= 0, idx[:, :1], -1), np.zeros((B, J), np.int64))
            planned = lambda: datas.mix_batch(pool, rec, L, n_out=N_OUT, normalize=True, rirs=views)
            chain = lambda: fft_chain(rec, N, spectra, dry)
            got, want = planned(), chain()
            torch.cuda.synchronize()
            between = max(float((got[0] - want[0]).abs().max() / want[0].abs().max()), float((got[1] - want[1]).abs().max() / want[1].abs().max()))
            case = alternate({"mix_batch_rirs_whole_call": planned, "fft_chain_whole_call": chain})
            fn, S = reverb_launch(rec, N)
            case["reverb_launch_events"] = event_ms(fn, args.steps * args.rounds)
            case["images"], case["flop"] = S, 2 * S * L * N
            case["reverb_launch_TFLOPs_over_event_time"] = round(case["flop"] / (case["reverb_launch_events"]["ms_median"] * 1e-3) / 1e12, 3)
            case["speedup_whole_call"] = round(case["fft_chain_whole_call"]["ms_median"] / case["mix_batch_rirs_whole_call"]["ms_median"], 3)
            case["max_rel_between_sides_outputs"] = between
            if B == min(BATCHES):
                ref = fft_images(rec, N, spectra64, torch.float64)
                mine = datas.reverberate(pool, views, rec.src.ravel(), rec.start.ravel(), rec.rir.ravel(), L, offset=rec.rir_offset.ravel())
                theirs = fft_images(rec, N, spectra)
                scale = float(ref.abs().max())
                case["image_max_err_over_max_ref"] = {"reverberate": float((mine.double() - ref).abs().max()) / scale,
                                                      "fft_chain_float32": float((theirs.double() - ref).abs().max()) / scale,
                                                      "reference": "float64 FFT convolution (torch, on the device)"}
            result["cases"][f"B{B}_N{N}"] = case

    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "reverb_kernel" in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    flop = result["cases"][f"B{max(BATCHES)}_N{max(TAPS)}"]["flop"]
                    result["kernel_stats"] = {"case": f"B{max(BATCHES)}_N{max(TAPS)}", "calls": int(row["Calls"]), "average_us": round(us, 3),
                                              "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3),
                                              "achieved_float64_TFLOPs": round(flop / (us * 1e-6) / 1e12, 3),
                                              "vendor_float64_vector_TFLOPs_not_measured_here": VENDOR_FP64_VECTOR_TFLOPS}
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
        rois = [torch.randint(0, 256, (25 * s, 96, 96), generator=g, dtype=torch.uint8).cuda() for s in secs]
        r = random.Random(1)
        views = rirs[4096][0]
        batch = system.mix_batch(pool, rois, length=L, rng=r, rirs=views)
        step = alternate({"system_mix_batch_rirs_N4096": lambda: system.mix_batch(pool, rois, length=L, rng=r, rirs=views),
                          "system_mix_batch_dry": lambda: system.mix_batch(pool, rois, length=L, rng=r),
                          "optimization_step": lambda: system.optimization_step(batch, 0)})
        step["mix_share_of_mix_plus_step"] = round(step["system_mix_batch_rirs_N4096"]["ms_median"] /
                                                   (step["system_mix_batch_rirs_N4096"]["ms_median"] + step["optimization_step"]["ms_median"]), 4)
        result["training_step_batch4"] = step

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
