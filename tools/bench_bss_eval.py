#!/usr/bin/env python3
"""BSS-eval SDR, SIR and SAR on the device (metrics.bss_eval, bss_eval_many, ALLMetricsTracker(bss_eval=True)) against what a user writes
today on the same device, and against bss_sdr alone, so that the price of the two extra figures is visible:

  python tools/bench_bss_eval.py [--calls 10] [--rounds 5] [--out profiles/bss_eval_bench.json]

  block       bss_eval at 32 x 2 s and 256 x 2 s with n_src 1, a mixture and others = mix - clean (the tracker's J = 2 case), and at
              32 x 2 s with n_src 2 (J = 2, no others), against bss_sdr on the same rows and against `torch chain`: tools/bench_bss_sdr.py's
              baseline extended to the joint system -- torch.fft cross-correlations in float64, an explicit (B, 512 J, 512 J)
              block-Toeplitz matrix and torch.linalg.solve next to the per-source Toeplitz solves, closed-form energies
  sources     bss_eval at 8 x 2 s with J = 3 and J = 4 scored sources (the block recursion's cost by J)
  pooled      bss_eval_many against bss_sdr_many on the 64 recordings of 1 .. 12 s of tools/bench_many.py ("mixed"), with mixtures
  tracker     ALLMetricsTracker.update_many on the same 64 recordings with bss_sdr=True and with bss_eval=True
Method (tools/bench_bss_sdr.py): the host clock around a block of --calls calls ending in one synchronise, ms per call; the variants of
a group alternate in --rounds rounds in ONE process; median [min, max] over the rounds.  No ratio is asserted.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 512


def torch_chain(clean, est, others):
    """clean, est (B,n,L), others (B,m,L) | None, float32 -> (SDR (B,n,n) [estimate, source], SIR (B,n,n), SAR (B,n)) float64: the
    definition with library calls, all float64"""
    import torch
    B, n, L = clean.shape
    S = (clean if others is None else torch.cat([clean, others], 1)).double()
    J = S.shape[1]
    e = est.double()
    nfft = 1 << (L + F - 1).bit_length()
    fs, fe = torch.fft.rfft(S, nfft), torch.fft.rfft(e, nfft)
    r = torch.fft.irfft(fs.conj()[:, :, None] * fs[:, None], nfft)               # (B,J,J,nfft): r_ij[k] at k mod nfft
    d = torch.fft.irfft(fs.conj()[:, None] * fe[:, :, None], nfft)[..., :F]      # (B,n,J,512): d_i of estimate q
    ar = torch.arange(F, device=clean.device)
    lag = (ar[:, None] - ar[None, :]) % nfft
    G = r[..., lag].permute(0, 3, 1, 4, 2).reshape(B, F * J, F * J)              # tap-major: [(a,i),(b,j)] = r_ij[a - b]
    D = d.permute(0, 3, 2, 1).reshape(B, F * J, n)
    p_all = (torch.linalg.solve(G, D) * D).sum(1)                                # (B,n)
    idx = (ar[:, None] - ar[None, :]).abs()
    p = torch.stack([((torch.linalg.solve(r[:, j, j][:, idx], d[:, :, j].transpose(1, 2))) * d[:, :, j].transpose(1, 2)).sum(1)
                     for j in range(n)], 2)                                      # (B,n[q],n[j])
    ee = (e * e).sum(2)
    db = lambda a, b: 10 * torch.log10(a / b.clamp_min(0))  # noqa: E731
    return db(p, ee[:, :, None] - p), db(p, p_all[:, :, None] - p), db(p_all, ee - p_all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import rtfs_net_amd as R
    from tests import metrics_oracle as M
    from tools.bench_many import FS, lengths

    def block_ms(fn, calls):
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

    out = {"metric": "BSS-eval SDR, SIR, SAR (joint 512-tap projection, float64): host clock around blocks of calls ending in a "
                     "synchronise, ms per call, median [min, max] over alternating rounds in one process",
           "device": torch.cuda.get_device_name(0), "calls_per_block": args.calls, "rounds": args.rounds}
    rng = np.random.default_rng(0)

    def batch(B, n, L=2 * FS):
        """two-talker mixtures: n scored talkers, the estimates hold a tenth of the mixture and some noise"""
        talk = np.stack([[M.speech_like(rng, L, FS) for _ in range(2)] for _ in range(B)])
        mix = talk.sum(1).astype(np.float32)
        clean = talk[:, :n]
        est = (clean + 0.1 * mix[:, None] + 0.1 * clean.std() * rng.standard_normal(clean.shape)).astype(np.float32)
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (clean, est, mix)]

    out["block"] = {}
    for B, n in ((32, 1), (256, 1), (32, 2)):
        c, e, m = batch(B, n)
        o = (m[:, None] - c) if n == 1 else None
        ev = R.bss_eval(c, e, m, o)
        case = {"sdr_sir_sar_db_mean": [float(v.mean()) for v in ev[:3]]}
        variants = {"bss_eval": lambda: R.bss_eval(c, e, m, o), "bss_sdr": lambda: R.bss_sdr(c, e, m)}

        def chunked(step=32):
            return [torch_chain(c[b:b + step], e[b:b + step], None if o is None else o[b:b + step]) for b in range(0, B, step)]

        try:
            ref = [torch.cat([v[k] for v in chunked()]) for k in range(3)]
            pick = ev.perm.long()[:, None]  # [b][0][j] = the estimate of source j
            diffs = [(ev.sdr.double() - ref[0].gather(1, pick)[:, 0]).abs().max(), (ev.sir.double() - ref[1].gather(1, pick)[:, 0]).abs().max(),
                     (ev.sar.double() - ref[2].gather(1, ev.perm.long())).abs().max()]
            case["max_abs_diff_db_vs_torch_chain"] = float(max(diffs))
            variants["torch_chain_32_rows_at_a_time"] = chunked
        except Exception as ex:  # the library solve gives up: report it
            case["torch_chain_error"] = f"{type(ex).__name__}: {str(ex)[:200]}"
        case.update(rounds(variants, args.calls if B == 32 else max(2, args.calls // 4)))
        out["block"][f"{B}x2s_n{n}"] = case

    out["sources"] = {}
    for J in (3, 4):
        talk = np.stack([[M.speech_like(rng, 2 * FS, FS) for _ in range(J)] for _ in range(8)])
        c = torch.from_numpy(talk).cuda()
        e = (c + 0.1 * c.sum(1, keepdim=True) + 0.02 * torch.randn_like(c)).contiguous()
        out["sources"][f"8x2s_n{J}"] = rounds({"bss_eval": lambda: R.bss_eval(c, e), "bss_sdr": lambda: R.bss_sdr(c, e)})

    Ls = lengths("mixed")
    cleans_h = [M.speech_like(rng, L, FS) * 0.05 for L in Ls]
    talk2 = [M.speech_like(rng, L, FS) * 0.05 for L in Ls]
    cleans = [torch.from_numpy(c[None]).cuda() for c in cleans_h]
    ests = [torch.from_numpy((c + 0.1 * t + 0.3 * c.std() * rng.standard_normal(c.shape)).astype(np.float32)[None]).cuda()
            for c, t in zip(cleans_h, talk2)]
    wavs = [torch.from_numpy((c + t).astype(np.float32)).cuda() for c, t in zip(cleans_h, talk2)]
    others = [(w - c[0])[None] for w, c in zip(wavs, cleans)]
    keys = [str(r) for r in range(len(Ls))]
    out["pooled"] = {"recordings": len(Ls), "seconds_of_audio": round(sum(Ls) / FS, 2),
                     **rounds({"bss_eval_many": lambda: R.bss_eval_many(cleans, ests, wavs, others),
                               "bss_sdr_many": lambda: R.bss_sdr_many(cleans, ests, wavs)}, max(2, args.calls // 2))}
    with tempfile.TemporaryDirectory() as td:
        t7 = R.ALLMetricsTracker(os.path.join(td, "a.csv"), bss_sdr=True)
        t9 = R.ALLMetricsTracker(os.path.join(td, "b.csv"), bss_eval=True)
        out["tracker"] = rounds({"update_many_bss_sdr": lambda: t7.update_many(wavs, cleans, ests, keys),
                                 "update_many_bss_eval": lambda: t9.update_many(wavs, cleans, ests, keys)}, max(2, args.calls // 2))
        t7.final()
        t9.final()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
