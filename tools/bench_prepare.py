#!/usr/bin/env python3
"""The preparation kernels (rtfs-net_amd/datas.py, csrc/k_prep.hip) and System.separate_recording against the only way the tree allowed
before them: numpy on the host, then the host-to-device copy of the float result.

  python tools/bench_prepare.py [--steps 20] [--warmup 3] [--host-steps 3] [--out profiles/prepare_bench.json]

Cases: lips 32 x 50 x 96 x 96 ("val" pipeline); normalise 32 x 2 s with 2 sources; resample 300 s at 48 kHz and at 44.1 kHz to 16 kHz (B = 1);
separate_recording on 60 s at 48 kHz (RTFS-Net-4, B = 1) against separate_long on inputs that are already prepared.
Device figures: HIP events around the call on the current stream, median over --steps after --warmup calls of the same shape; the
device-side inputs are resident, and the copy of the RAW input (uint8 ROIs, the recording at its own rate) is timed separately.  Host
figures: a host clock around tests/prep_oracle.py's float64 numpy (median over --host-steps), and separately a host clock around the
copy of its float32 result to the device, ending in a synchronise.  Bytes are what the operation has to move, computed from the shapes.
A measurement needs the GPU: without one the tool fails.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip-separator", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rtfs_net_amd as R
    from rtfs_net_amd import datas
    from tests import prep_oracle as PO
    assert torch.cuda.is_available(), "bench_prepare.py measures on the GPU only"

    def dev_ms(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    def host_ms(fn, steps=None):
        out, ms = None, []
        for _ in range(steps or args.host_steps):
            t = time.perf_counter()
            out = fn()
            ms.append(1e3 * (time.perf_counter() - t))
        return out, {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}

    def copy_ms(arrays):
        """Host clock around the pageable host-to-device copies of `arrays`, ending in a synchronise."""
        ts = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
        def go():
            d = [t.cuda() for t in ts]
            torch.cuda.synchronize()
            return d
        go()
        return host_ms(go, steps=5)[1]

    def case(name, shape, nbytes, device_fn, host_fn, raw_inputs):
        d = dev_ms(device_fn)
        res, h = host_ms(host_fn)
        res = res if isinstance(res, (list, tuple)) else [res]
        c = copy_ms([np.asarray(r, np.float32) for r in res if r is not None])
        raw = copy_ms(raw_inputs)
        c_out = {"case": name, "shape": shape, "bytes_moved": nbytes, "device": d, "device_GBps": round(nbytes / d["ms_median"] / 1e6, 1),
                 "raw_input_copy": raw, "host_numpy": h, "host_result_copy": c,
                 "host_plus_copy_over_device_plus_raw_copy": round((h["ms_median"] + c["ms_median"]) / (d["ms_median"] + raw["ms_median"]), 1),
                 "host_plus_copy_over_device": round((h["ms_median"] + c["ms_median"]) / d["ms_median"], 1)}
        print(json.dumps(c_out), flush=True)
        return c_out

    out = {"metric": "preparation kernels vs float64 numpy on the host + copy of the float32 result (median ms; device: HIP events; host: "
                     "perf_counter; copies: pageable memory, perf_counter to a synchronise)",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps, "cases": []}
    rs = np.random.RandomState(0)

    # lips
    N, Tv, H, W = 32, 50, 96, 96
    roi = rs.randint(0, 256, (N, Tv, H, W)).astype(np.uint8)
    r = torch.from_numpy(roi).cuda()
    pipe = datas.get_preprocessing_pipelines()["val"]
    out["cases"].append(case("lips_val", [N, Tv, H, W], N * Tv * 88 * 88 * 5, lambda: pipe(r),
                             lambda: PO.lips_prepare(roi, [(4, 4, 0)] * N), [roi]))
    # normalise
    B, K, L = 32, 2, 32000
    mix = (rs.randn(B, L) * 0.05).astype(np.float32)
    src = (rs.randn(B, K, L) * 0.05).astype(np.float32)
    m, s = torch.from_numpy(mix).cuda(), torch.from_numpy(src).cuda()
    out["cases"].append(case("normalize_mixture", [B, K, L], B * (1 + K) * L * 4 * 3, lambda: datas.normalize_mixture(m, s),
                             lambda: PO.normalize_mixture(mix, src), [mix, src]))
    # resample
    for fs in (48000, 44100):
        L = 300 * fs
        x = (rs.randn(1, L) * 0.05).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        Lout = PO.resample_out_len(fs, 16000, L)
        o, n, width, taps = PO.resample_plan(fs, 16000)
        c = case(f"resample_{fs}_300s", [1, L], (L + Lout) * 4, lambda: datas.resample(xd, fs, 16000), lambda: PO.resample(x, fs, 16000), [x])
        c["macs"] = Lout * (2 * width + 1)
        c["device_GMACps"] = round(c["macs"] / c["device"]["ms_median"] / 1e6, 1)
        out["cases"].append(c)

    # separate_recording on 60 s at 48 kHz against separate_long on prepared inputs
    if not args.skip_separator:
        from oracle import video_oracle as V
        from oracle.params import load_spec, make_state_dict
        from rtfs_net_amd.configs import audionet_config
        am = R.AVNet(print_macs=False, **audionet_config(4))
        am.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
        vm = R.FRCNNVideoModel(print_macs=False)
        vm.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in V.make_video_state_dict(0).items()})
        sysm = R.System(audio_model=am.cuda().eval(), video_model=vm.cuda().eval()).eval()
        seconds, fs = 60, 48000
        Tv = 25 * seconds
        wav = torch.from_numpy((rs.randn(1, seconds * fs) * 0.05).astype(np.float32)).cuda()
        roi = torch.from_numpy(rs.randint(0, 256, (1, Tv, 96, 96)).astype(np.uint8)).cuda()
        with torch.no_grad():
            w16 = datas.resample(wav, fs, 16000)
            lips = datas.get_preprocessing_pipelines()["val"](roi)
            steps, args.steps = args.steps, max(3, args.steps // 4)
            # alternate the two so that drift of the box hits both
            a1 = dev_ms(lambda: sysm.separate_recording(wav, fs, roi))
            b1 = dev_ms(lambda: sysm.separate_long(w16, lips))
            a2 = dev_ms(lambda: sysm.separate_recording(wav, fs, roi))
            b2 = dev_ms(lambda: sysm.separate_long(w16, lips))
            args.steps = steps
            prep = dev_ms(lambda: (datas.resample(wav, fs, 16000), datas.get_preprocessing_pipelines()["val"](roi)))
        sr, sl = min(a1["ms_median"], a2["ms_median"]), min(b1["ms_median"], b2["ms_median"])
        c = {"case": "separate_recording_48000_60s", "separate_recording": [a1, a2], "separate_long_prepared": [b1, b2],
             "resample_plus_lips_alone": prep, "share_of_separate_long_pct": round(100.0 * (sr / sl - 1.0), 2),
             "prep_alone_over_separate_long_pct": round(100.0 * prep["ms_median"] / sl, 2)}
        print(json.dumps(c), flush=True)
        out["cases"].append(c)

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
