#!/usr/bin/env python3
"""BSS-eval SDR on the device (metrics.bss_sdr, bss_sdr_many, ALLMetricsTracker(bss_sdr=True)) against what a user writes today on the
same device and against the float64 host oracle:

  python tools/bench_bss_sdr.py [--calls 10] [--rounds 5] [--out profiles/bss_sdr_bench.json]

  block       bss_sdr(clean, est, mix) at 32 x 2 s and 256 x 2 s, n_src 1, against `torch chain`: torch.fft correlations in float64, an
              explicit (B,512,512) Toeplitz matrix and torch.linalg.solve, two right-hand sides (estimate and mixture), closed-form energies
  forms       the two Levinson forms of csrc/k_bss.hip through rtfs_debug_bss_f64 (512 threads, two barriers per order | one wave, 8
              taps per lane) at the same two shapes
  pooled      bss_sdr_many on the 64 recordings of 1 .. 12 s of tools/bench_many.py ("mixed"), with mixtures
  tracker     ALLMetricsTracker.update_many on the same 64 recordings without and with bss_sdr=True
  host        tests/bss_oracle.sdr_moments and sdr_lu on one 2 s pair, seconds per pair
Method (tools/bench_mix.py): the host clock around a block of --calls calls ending in one synchronise, ms per call; the variants of a
group alternate in --rounds rounds in ONE process; median [min, max] over the rounds.  No ratio is asserted.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 512


def torch_chain(clean, est, mix):
    """(B,L) float32 each -> (sdr, sdr_i) float64 (B): the definition with library calls, all float64"""
    import torch
    B, L = clean.shape
    nfft = 1 << (L + F - 1).bit_length()
    s = torch.fft.rfft(clean.double(), nfft)
    r = torch.fft.irfft(s.conj() * s, nfft)[:, :F]
    idx = (torch.arange(F, device=clean.device)[:, None] - torch.arange(F, device=clean.device)[None, :]).abs()
    G = r[:, idx]                                                                # (B,512,512)
    rhs = torch.stack([est.double(), mix.double()], 1)                           # (B,2,L)
    d = torch.fft.irfft(s.conj()[:, None] * torch.fft.rfft(rhs, nfft), nfft)[..., :F]  # (B,2,512)
    c = torch.linalg.solve(G, d.transpose(1, 2))                                 # (B,512,2)
    num = (c * d.transpose(1, 2)).sum(1)                                         # (B,2)
    den = ((rhs * rhs).sum(2) - num).clamp_min(0)
    db = 10 * torch.log10(num / den)
    return db[:, 0], db[:, 0] - db[:, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import rtfs_net_amd as R
    from rtfs_net_amd import _lib
    from tests import bss_oracle as O
    from tests import metrics_oracle as M
    from tools.bench_many import FS, lengths
    lib = _lib.load()

    def block_ms(fn, calls=args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    def rounds(variants, calls=args.calls):
        """{name: fn} -> {name: {ms_median, ms_min, ms_max}}, the variants alternating in every round"""
        for fn in variants.values():  # warm-up: allocator, library handles
            fn()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(block_ms(fn, calls))
        return {k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()}

    out = {"metric": "BSS-eval SDR (512-tap projection, float64): host clock around blocks of calls ending in a synchronise, ms per call, "
                     "median [min, max] over alternating rounds in one process", "device": torch.cuda.get_device_name(0),
           "calls_per_block": args.calls, "rounds": args.rounds}
    rng = np.random.default_rng(0)

    def batch(B, L=2 * FS):
        clean = np.stack([M.speech_like(rng, L, FS) for _ in range(B)])
        est = (clean + 0.1 * clean.std() * rng.standard_normal(clean.shape)).astype(np.float32)
        mix = (clean + 0.8 * clean.std() * rng.standard_normal(clean.shape)).astype(np.float32)
        return [torch.from_numpy(a).cuda() for a in (clean, est, mix)]

    out["block"], out["forms"] = {}, {}
    for B in (32, 256):
        c, e, m = batch(B)
        sdr, sdr_i = R.bss_sdr(c, e, m)
        case = {}
        try:
            ref, ref_i = torch_chain(c, e, m)
            case["max_abs_diff_db_vs_torch_chain"] = float(max((sdr.double() - ref).abs().max(), (sdr_i.double() - ref_i).abs().max()))
            variants = {"bss_sdr": lambda: R.bss_sdr(c, e, m), "torch_chain": lambda: torch_chain(c, e, m)}
        except Exception as ex:  # the batched library solve gives up on the whole batch: report it, run the chain 32 rows at a time
            case["torch_chain_error"] = f"{type(ex).__name__}: {str(ex)[:200]}"

            def chunked():
                return [torch_chain(c[b:b + 32], e[b:b + 32], m[b:b + 32]) for b in range(0, B, 32)]

            variants = {"bss_sdr": lambda: R.bss_sdr(c, e, m)}
            try:
                ref = torch.cat([v[0] for v in chunked()])
                case["max_abs_diff_db_vs_torch_chain"] = float((sdr.double() - ref).abs().max())
                variants["torch_chain_32_rows_at_a_time"] = chunked
            except Exception as ex2:
                case["torch_chain_chunked_error"] = f"{type(ex2).__name__}: {str(ex2)[:200]}"
        case.update(rounds(variants, args.calls if B == 32 else max(2, args.calls // 4)))
        case["sdr_db_mean"] = float(sdr.mean())
        out["block"][f"{B}x2s"] = case
        # the two solver forms through the debug entry (which also copies r, d, ee and the order out)
        c3, e3 = c[:, None].contiguous(), e[:, None].contiguous()
        L = c.shape[1]
        ws = torch.empty(lib.rtfs_bss_sdr_workspace_bytes(B, 1, L, 1), dtype=torch.uint8, device="cuda")
        o32, oi32 = torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")
        perm, order = torch.empty(B, 1, dtype=torch.int32, device="cuda"), torch.empty(B, 1, dtype=torch.int32, device="cuda")
        r_, d_, ee_ = (torch.empty(*s, dtype=torch.float64, device="cuda") for s in ((B, 1, F), (B, 1, 2, F), (B, 1, 2)))
        P, st = _lib.ptr, _lib.stream_of(c)

        def form(f):
            assert lib.rtfs_debug_bss_f64(P(c3), P(e3), P(m), B, 1, L, P(ws), ws.numel(), P(o32), P(oi32), P(perm), f, P(r_), P(d_), P(ee_),
                                          P(order), st) == 0

        fr = rounds({"threads_512": lambda: form(512), "one_wave": lambda: form(64)})
        form(512)
        a = o32.clone()
        form(64)
        fr["max_abs_diff_db_between_forms"] = float((a - o32).abs().max())
        out["forms"][f"{B}x2s"] = fr

    Ls = lengths("mixed")
    cleans_h = [M.speech_like(rng, L, FS) * 0.05 for L in Ls]
    cleans = [torch.from_numpy(c[None]).cuda() for c in cleans_h]
    ests = [torch.from_numpy((c + 0.3 * c.std() * rng.standard_normal(c.shape)).astype(np.float32)[None]).cuda() for c in cleans_h]
    wavs = [torch.from_numpy((c + 0.8 * c.std() * rng.standard_normal(c.shape)).astype(np.float32)).cuda() for c in cleans_h]
    keys = [str(r) for r in range(len(Ls))]
    out["pooled"] = {"recordings": len(Ls), "seconds_of_audio": round(sum(Ls) / FS, 2),
                     **rounds({"bss_sdr_many": lambda: R.bss_sdr_many(cleans, ests, wavs)}, max(2, args.calls // 2))}
    with tempfile.TemporaryDirectory() as td:
        t5 = R.ALLMetricsTracker(os.path.join(td, "a.csv"))
        t7 = R.ALLMetricsTracker(os.path.join(td, "b.csv"), bss_sdr=True)
        out["tracker"] = rounds({"update_many": lambda: t5.update_many(wavs, cleans, ests, keys),
                                 "update_many_bss_sdr": lambda: t7.update_many(wavs, cleans, ests, keys)}, max(2, args.calls // 2))
        t5.final()
        t7.final()
    s, e = cleans_h[0][:2 * FS], ests[0][0, :2 * FS].cpu().numpy()
    host = {}
    for name, fn in (("sdr_moments", O.sdr_moments), ("sdr_lu", O.sdr_lu)):
        t0 = time.perf_counter()
        for _ in range(3):
            fn(s, e)
        host[name + "_s_per_pair"] = round((time.perf_counter() - t0) / 3, 4)
    out["host_oracle_2s"] = host
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
