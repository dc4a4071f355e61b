#!/usr/bin/env python3
"""Throughput benchmark of the MI355X-native RTFS-Net separator forward.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1: either launched by `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* in the environment, one rank per GPU over RCCL), or started plainly as `python bench.py --gpus N ...`:
the parent then spawns the N ranks itself as fresh child processes BEFORE anything in it touches the GPU (`spawn_ranks`),
relays rank 0's JSON line and exits non-zero if any rank failed.

Metric (BASELINE.json): mixtures/s of the RTFS-Net-4 forward on synthetic 2 s @16 kHz 2-speaker mixtures with
dummy lip embeddings, batch 32 per GPU (configs[1]); inputs and weights are resident in HBM before the timed
region.  One "step" = one forward over one batch.  Weak scaling: every rank runs its own batch, there is no
data-path collective (utterances are independent in the forward).  --dump-outputs DIR: after the timed steps, rank 0 writes what
its last timed step returned as DIR/<name>.npy (`dump_outputs`).  Rank 0 prints ONE JSON line that also carries
  roofline      the fused dual-path sweep kernel: algorithmic bytes (20*L*N*64 per SRU layer, 4 layers per
                launch) / its launch duration measured live with HIP events on the launch stream, vs 8 TB/s HBM

A plain run does only what that line needs: set-up, W warm-up steps, K timed steps, the dump, the line.  --full adds what
takes work of its own (each can still be skipped with its --no-* option), as further fields of the same line:
  cpu_baseline  the CPU oracle (oracle/rtfs_oracle.py, numpy) timed on this box's host cores on a bounded sample
                (16 single-threaded worker processes, one mixture each, started before the GPU is touched)
  batch_split_2 the same step as two half batches on two streams, timed after the timed region (--no-batch-split)
and with --train the training CPU baseline and the roofline of the step's dominant GEMM, timed alone.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md); ~6300 GB/s achievable


DTYPE = "f32 (f16x3 split-precision MFMA products, f32 accumulate; every tensor in HBM is f32)"


def audionet_config(repeats):
    from rtfs_net_amd.configs import audionet_config as cfg
    return cfg(repeats)


def sweep_bytes(seq_len, n_seq):
    """Algorithmic bytes of one dual-path launch at the reference's op boundary."""
    return 20.0 * (seq_len - 7) * n_seq * 64 * 4


def by_counters(traffic_bytes, avg_launch_ms):
    """What the PMC passes of this round (profiles/r02_pmc/, tools/pmc_mfma.sh, tools/sweep_traffic.py) say about the sweep kernel: real HBM
    traffic per launch against the live launch time, and the matrix-pipe busy fraction (a committed measurement, not re-collected here)."""
    out = {"hbm_gbs": None, "hbm_frac_of_peak": None, "mfma_busy_frac": None, "bound": None,
           # provenance: hbm_gbs = STORED traffic figure / LIVE launch time; mfma_busy_frac is a STORED counter reading, not collected in this run
           "source": {"traffic": "profiles/sweep_traffic.json (stored PMC passes)", "mfma_busy_frac": None, "live": ["avg_launch_ms"]}}
    if traffic_bytes and avg_launch_ms:
        out["hbm_gbs"] = round(traffic_bytes / (avg_launch_ms * 1e-3) / 1e9, 1)
        out["hbm_frac_of_peak"] = round(out["hbm_gbs"] / HBM_PEAK_GBS, 4)
    try:
        for rel in ("profiles/r03_pmc/pmc_mfma_summary.json", "profiles/r02_pmc/pmc_mfma_summary.json"):
            path = os.path.join(ROOT, rel)
            if not os.path.exists(path):
                continue
            rows = json.load(open(path))
            fr = [r["mfma_util_busy"] for r in rows if r["kernel"].startswith("dp16s_kernel") and r.get("mfma_util_busy")]
            if fr:
                out["mfma_busy_frac"] = round(sum(fr) / len(fr), 4)
                out["source"]["mfma_busy_frac"] = rel + " (stored; the sweep kernel's source is unchanged since)"
                break
    except Exception:
        pass
    if out["hbm_frac_of_peak"] is not None and out["mfma_busy_frac"] is not None:
        out["bound"] = "latency (matrix pipe %.0f %% busy, HBM at %.0f %% of peak: a serial recurrence between GEMM phases)" % (
            100 * out["mfma_busy_frac"], 100 * out["hbm_frac_of_peak"])
    return out


def cpu_baseline(repeats, workers=None, leg_seconds=12.0):  # leg_seconds bounds the numpy legs only; the torch legs run the full 3 + 5
    """The CPU oracle (oracle/rtfs_oracle.py, numpy) on this box's host cores: one single-threaded worker process per core
    of the CPU share (16 per GPU), four 2 s mixtures each -> aggregate mixtures/s.  Must run BEFORE this process touches the
    GPU (the workers are child processes)."""
    import subprocess
    workers = workers or min(16, os.cpu_count() or 1)
    t0 = time.perf_counter()
    per_worker = 4  # about 10 s of wall time on the GPU box
    procs = [subprocess.Popen([sys.executable, "-m", "oracle.cpu_worker", str(repeats), str(per_worker), str(i)], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for i in range(workers)]
    done, per = 0, []
    for pr in procs:
        out, _ = pr.communicate(timeout=900)
        if pr.returncode == 0:
            rec = json.loads(out.strip().splitlines()[-1])
            done += rec["n"]
            per.append(rec["seconds"])
    dt = time.perf_counter() - t0
    if done == 0:
        return {"value": None, "unit": "mixtures/s", "cores": workers, "kind": "port", "sample": "CPU oracle workers failed"}
    res = {"value": round(done / dt, 4), "unit": "mixtures/s", "cores": int(workers), "kind": "port",
           "sample": f"{done} x (1 mixture, 2 s @16 kHz, RTFS-Net-{repeats}) through the numpy CPU oracle, one single-threaded "
                     f"process per core on {workers} of {os.cpu_count()} host cpus, wall {dt:.1f} s incl. start-up "
                     f"(forwards alone {min(per) / per_worker:.1f}-{max(per) / per_worker:.1f} s per mixture)"}
    # SURVEY 8(d)'s protocol beside it: the numpy restatement AND the stock-torch-ops composition, batch 1 and 4, all `workers` cores in
    # one process (torch.set_num_threads), 3 warm-up + 5 timed forwards per leg, each leg bounded to `leg_seconds` of wall time
    try:
        pr = subprocess.run([sys.executable, "-m", "oracle.cpu_bench", str(repeats), str(workers), str(leg_seconds)], cwd=ROOT,
                            stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
        rec = json.loads(pr.stdout.strip().splitlines()[-1])
        res["threaded"] = rec
        best = max(rec["legs"], key=lambda l: l["mixtures_per_s"])
        res["sample"] += (f"; one process on {rec['threads']} threads (torch-ops legs: 3 warm-up + 5 timed forwards; numpy legs <= {leg_seconds:g} s each): best "
                          f"{best['mixtures_per_s']} mixtures/s ({best['impl']}, batch {best['batch']}), all legs under 'threaded'")
        if best["mixtures_per_s"] > res["value"]:
            res["value"] = best["mixtures_per_s"]
    except Exception as e:  # the single-threaded-workers figure above stands on its own
        res["threaded"] = {"error": repr(e)[:200]}
    return res


def train_cpu_baseline(repeats, threads=None):
    """One training step (forward, PIT neg-SNR loss, backward) of the torch-autograd restatement (oracle/grad_oracle.py, float32 like the
    reference's training) on this box's host cores: 2 mixtures x 2 s (train-mode BatchNorm needs two), one process with `threads` intra-op
    threads.  Child process: must start BEFORE this process touches the GPU."""
    import subprocess
    threads = threads or min(16, os.cpu_count() or 1)
    t0 = time.perf_counter()
    pr = subprocess.run([sys.executable, "-m", "oracle.cpu_train_worker", str(repeats), "2", str(threads), "3", "f32"], cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=1200)
    if pr.returncode != 0 or not pr.stdout.strip():
        return {"value": None, "unit": "mixtures/s", "cores": threads, "kind": "port", "sample": "CPU training worker failed"}
    rec = json.loads(pr.stdout.strip().splitlines()[-1])
    return {"value": round(rec["n"] / rec["seconds"], 4), "unit": "mixtures/s", "cores": int(threads), "kind": "port",
            "sample": f"3 training steps of 2 mixtures each (2 s @16 kHz, RTFS-Net-{repeats}) through the float32 torch-autograd port "
                      f"(oracle/grad_oracle.py; python time loop for the SRU cells), {threads} intra-op threads: {rec['seconds']:.1f} s "
                      f"(wall incl. start-up {time.perf_counter() - t0:.1f} s)"}


def train_roofline(dev, B, L):
    """The training step's dominant kernel by time, gemm_nt_kernel<0> (1x1 convolutions on channel-last rows), timed alone with events on
    torch's current stream at its most expensive shape: the 64 -> 256 residual convolution (and the input gradient of the 256 -> 64
    projection) over all B*T*F rows.  Algorithmic bytes: A (M, K) + W (N, K) + C (M, N) floats, once each.  (Back-to-back launches on the
    same operands: the 33 MB A stays in the memory-side cache, so this is the kernel's best case - inside a step, rocprofv3 shows the
    same launch at ~78 us, see profiles/r01_train_step_kernel_stats.csv.)"""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    M, N, K = B * lib.rtfs_num_frames(L) * 129, 256, 64
    A = torch.randn(M, K, device=dev)
    W = torch.randn(N, K, device=dev)
    C = torch.empty(M, N, device=dev)
    st = _lib.stream_of(A)
    run = lambda: _lib.check(lib.rtfs_debug_gemm_f32(0, _lib.ptr(A), _lib.ptr(W), _lib.ptr(C), M, N, K, 0, st), "rtfs_debug_gemm_f32")
    for _ in range(3):
        run()
    n = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    nbytes = 4.0 * (M * K + N * K + M * N)
    return {"kernel": f"gemm_nt_kernel<0> (bf16x3 MFMA, C = A.W^T) at M={M}, N={N}, K={K}: the 64->256 1x1 convolution of an RTFS block on rows",
            "bound": "hbm", "achieved": round(nbytes / ms / 1e6, 2), "peak": 8000.0, "unit": "GB/s", "frac": round(nbytes / ms / 1e6 / 8000.0, 4),
            "traffic": None, "launches_timed": n, "avg_launch_ms": round(ms, 4), "algorithmic_bytes_per_launch": int(nbytes)}


def rank_inputs(rank, B, L, Tv):
    """Per-rank synthetic batch: s1, s2 ~ N(0, 0.05^2), mixture = s1 + s2, lip embedding ~ N(0, 1)."""
    g = torch.Generator().manual_seed(1234 + rank)
    s1 = torch.randn(B, L, generator=g) * 0.05
    s2 = torch.randn(B, L, generator=g) * 0.05
    return s1 + s2, torch.randn(B, 512, Tv, generator=g)


def max_over_ranks(dt, dist, device):
    """Whole-job time = the slowest rank's time."""
    if dist is None:
        return dt
    if dist.get_backend() == "gloo":
        device = torch.device("cpu")
    tt = torch.tensor([dt], device=device, dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return float(tt.item())


def dist_evidence(dist, world, device=None):
    """What the job looked like from the inside: the process group's backend, its world size and ONE device identity per rank gathered
    over that very process group (PCI domain:bus:device + uuid), so a SCALE record shows that RCCL saw N distinct GPUs."""
    if device is not None and device.type == "cuda":
        p = torch.cuda.get_device_properties(device)
        me = {"rank": int(os.environ.get("RANK", "0")), "cuda_index": device.index, "name": p.name,
              "pci": "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), getattr(p, "pci_bus_id", 0), getattr(p, "pci_device_id", 0)),
              "uuid": str(getattr(p, "uuid", ""))}
    else:
        me = {"rank": int(os.environ.get("RANK", "0")), "cuda_index": None, "name": "cpu (dry run)", "pci": None, "uuid": None, "pid": os.getpid()}
    if dist is None:
        return {"backend": None, "world": 1, "devices": [me], "distinct_devices": 1}
    got = [None] * world
    dist.all_gather_object(got, me)
    ids = {(g["pci"], g["uuid"], g.get("pid")) for g in got}
    return {"backend": dist.get_backend(), "world": dist.get_world_size(), "devices": got, "distinct_devices": len(ids)}


def throughput(world, B, steps, dt):
    return world * B * steps / dt


DUMP_BYTES = 64 * 10 ** 6


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy in float32.  The inputs and weights are seeded, so two builds run with the same
    arguments can be compared output for output.  An array past its share of DUMP_BYTES is replaced by the same seeded sample of its
    flattened elements (sorted indices) in every run.  Returns what was written, for the JSON line."""
    os.makedirs(path, exist_ok=True)
    budget = (DUMP_BYTES - 4096) // 4 // len(arrays)  # floats per array; 4096 bytes left for the .npy headers
    info = {}
    for name, t in arrays.items():
        a = t.detach().to("cpu", torch.float32).numpy()
        info[name] = {"shape": list(a.shape), "sampled_elements": None}
        if a.size > budget:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, budget, replace=False))]
            info[name]["sampled_elements"] = budget
        np.save(os.path.join(path, name + ".npy"), a)
    return {"dir": path, "arrays": info}


def spawn_ranks(n, argv, timeout=3000):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes of THIS process, which has not
    touched the GPU (no HIP call, no torch.cuda.is_available()) and never will: it only waits, relays rank 0's JSON line (its stdout)
    and returns non-zero if any rank failed (the others are then terminated by PID so nobody waits at a barrier for ever).
    Rendezvous on 127.0.0.1 and a free port; ranks see exactly what torch.distributed.run would give them."""
    import socket
    import subprocess
    import tempfile
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs, outs = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts (RCCL needs it)
        out = tempfile.TemporaryFile(mode="w+")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env, cwd=ROOT, stdout=out))
    t0, failed = time.time(), None
    while failed is None and any(p.poll() is None for p in procs):
        for r, p in enumerate(procs):
            if p.poll() not in (None, 0):
                failed = r
        if time.time() - t0 > timeout:
            failed = -1
        time.sleep(0.05)
    if failed is None:
        failed = next((r for r, p in enumerate(procs) if p.returncode != 0), None)
    if failed is not None:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=20)
            except Exception:
                p.kill()
        print(f"bench.py: rank {failed} failed (rc {procs[failed].returncode if failed >= 0 else 'timeout'}); job aborted", file=sys.stderr)
        return 1
    outs[0].seek(0)
    sys.stdout.write(outs[0].read())
    sys.stdout.flush()
    return 0


def init_ranks(args, backend="nccl"):
    """(rank, local_rank, world, dist-or-None) from the launcher's environment; the process group is RCCL (`nccl`) on the GPU box."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl" and not os.environ.get("RTFS_BENCH_SHARE_GPU"):
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo" if backend == "nccl" else backend, rank=rank, world_size=world)
    if os.environ.get("RTFS_BENCH_SHARE_GPU"):
        # rehearsal of the N-rank protocol on a ONE-GPU box: every rank uses cuda:0 (time-sliced) and the process group is gloo (RCCL needs a
        # device per rank).  Exercises the real launcher + forward + timing + JSON path; the number it prints is NOT a scaling measurement.
        local_rank = 0
    return rank, local_rank, world, dist


def dry_run_main(args):
    """`--dist-dry-run`: the whole multi-rank protocol of the bench (spawned or launched ranks, gloo rendezvous, per-rank shards, W warm-up
    + K timed steps between barriers, MAX over ranks, rank 0's one JSON line) on the CPU with a stand-in step (a small matmul in place of
    the forward) -- what tests/test_bench_dist.py runs end to end where there is no GPU.  Never a measurement."""
    rank, _, world, dist = init_ranks(args, backend="gloo")
    if os.environ.get("RTFS_BENCH_FAIL_RANK") == str(rank):  # fault injection for the launcher test
        raise SystemExit(3)
    B = args.batch if args.batch is not None else 32
    wav, emb = rank_inputs(rank, B, 4096, 7)
    w = torch.randn(4096, 64, generator=torch.Generator().manual_seed(0))

    def step():
        return (wav @ w).sum() + emb.sum()
    for _ in range(args.warmup):
        step()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        chk = step()
    if dist is not None:
        dist.barrier()
    dt = max_over_ranks(time.perf_counter() - t0 + 0.01 * rank, dist, torch.device("cpu"))
    assert bool(torch.isfinite(chk))
    ev = dist_evidence(dist, world)
    if rank == 0:
        res = {"metric": "dry run (launcher + rendezvous + timing protocol only; NOT a measurement)", "dist": ev, "value": round(throughput(world, B, args.steps, dt), 3),
               "unit": "mixtures/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": "stand-in step on CPU over gloo", "per_gpu_batch": B, "global_batch": B * world}}
        if args.dump_outputs:
            res["dump_outputs"] = dump_outputs(args.dump_outputs, {"out": chk})
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def train_main(args):
    """Training-step throughput, same timing protocol as the forward bench (W warm-up steps, K steps between barrier + synchronize on both
    sides, MAX over ranks, whole-job aggregate).  Per-GPU batch defaults to the reference's training batch_size 4 unless --batch is given."""
    rank, local_rank, world, dist = init_ranks(args)
    cpu_res = train_cpu_baseline(args.repeats) if (world == 1 and args.full and not args.no_cpu_baseline) else None  # before the GPU is initialised
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    import rtfs_net_amd as R
    torch.manual_seed(0)
    model = R.AVNet(print_macs=False, **audionet_config(args.repeats)).to(dev).train()
    loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.1)
    system = R.System(audio_model=model, loss_func={"train": loss, "val": loss}, optimizer=opt)
    if world > 1:
        system.convert_sync_batchnorm()
    B = args.batch if args.batch is not None else 4  # the reference's training batch_size
    L, Tv = int(args.seconds * 16000), int(args.seconds * 25)
    wav, emb = rank_inputs(rank, B, L, Tv)
    g = torch.Generator().manual_seed(4321 + rank)
    tgt = wav - 0.05 * torch.randn(B, L, generator=g)  # one of the two synthetic sources
    batch = (wav.to(dev), tgt.unsqueeze(1).to(dev), emb.to(dev), None)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        system.optimization_step(batch)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = system.optimization_step(batch)
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0, dist, dev)
    assert bool(torch.isfinite(last))
    ev = dist_evidence(dist, world, dev)
    if rank == 0:
        peak_gib = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        extra = {"roofline": train_roofline(dev, B, L)} if args.full else {}
        if cpu_res is not None:
            extra["cpu_baseline"] = cpu_res
        if args.dump_outputs:
            extra["dump_outputs"] = dump_outputs(args.dump_outputs, {"loss": last})
        print(json.dumps({
            "metric": f"mixtures/sec trained ({args.seconds:g} s@16 kHz) RTFS-Net-{args.repeats} training step", "value": round(throughput(world, B, args.steps, dt), 3),
            "unit": "mixtures/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 (bf16x3 / f16x3 split-precision matrix products)", "data": "synthetic",
            "config": {"workload": f"RTFS-Net-{args.repeats} training step (forward_train, PIT neg-SNR loss, HIP backward, AdamW), batch {B}/GPU, "
                                   f"{args.seconds:g} s segments, every parameter trainable, BatchNorm on batch statistics"
                                   + (", SyncBatchNorm" if world > 1 else ""),
                       "per_gpu_batch": B, "global_batch": B * world, "samples": L,
                       "parallelism": f"dp{world} (one flattened gradient all-reduce of {sum(p.numel() for p in model.parameters())} floats per step)"},
            "dist": ev, "peak_memory_gib": peak_gib, **extra}), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="mixtures per GPU per step (default: 32 forward, 4 training)")
    ap.add_argument("--repeats", type=int, default=4, help="RTFS-Net-R")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes work of its own: the CPU baseline, the 'batch_split_2' mode and, with --train, the "
                         "roofline of the step's dominant GEMM (a plain run times the steps and prints the line, nothing else)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--split", type=int, default=1,
                    help="rtfs_set_batch_split for the timed region (default 1: one chain, per-kernel durations undisturbed); with --full "
                         "the two-part throughput mode is measured as well, after the timed region, and reported under 'batch_split_2'")
    ap.add_argument("--no-batch-split", action="store_true",
                    help="with --full: skip the extra 'batch_split_2' measurement (profiling runs: one mode per trace)")
    ap.add_argument("--train", action="store_true",
                    help="measure the training step instead (forward_train + PIT loss + HIP backward + one flattened gradient all-reduce "
                         "over RCCL + clip + AdamW; SyncBatchNorm at N > 1); not the contract metric, a separate JSON line")
    ap.add_argument("--dist-dry-run", action="store_true", help="CPU/gloo rehearsal of the multi-rank protocol with a stand-in step (tests)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the separated waveforms; the loss with --train) "
                         "as DIR/<name>.npy in float32, at most 64 MB in all (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # the ranks start in ROOT: a relative --dump-outputs is passed on as the directory it names here (the last occurrence wins)
        argv = sys.argv[1:] + (["--dump-outputs", os.path.abspath(args.dump_outputs)] if args.dump_outputs else [])
        return spawn_ranks(args.gpus, argv)  # this process never touches the GPU
    if args.dist_dry_run:
        return dry_run_main(args)
    if args.train:
        return train_main(args)

    rank, local_rank, world, dist = init_ranks(args)
    cpu_res = None
    if world == 1 and args.full and not args.no_cpu_baseline:
        cpu_res = cpu_baseline(args.repeats)  # child processes: started before this process initialises the GPU
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    import rtfs_net_amd as R
    from rtfs_net_amd import _lib
    lib = _lib.load()

    torch.manual_seed(0)  # random-init weights of the named architecture (no checkpoints offline)
    model = R.AVNet(print_macs=False, **audionet_config(args.repeats)).to(dev).eval()
    B, L = (args.batch if args.batch is not None else 32), int(args.seconds * 16000)
    Tv = int(args.seconds * 25)
    wav, emb = (t.to(dev) for t in rank_inputs(rank, B, L, Tv))

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    R.set_batch_split(args.split)
    with torch.no_grad():
        for _ in range(args.warmup):
            out = model(wav, emb)
        barrier()
        lib.rtfs_sweep_timing_enable(3)  # every third sweep launch of the timed region (F, T, F, ... alternate): an event pair is a ~6 us gap
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = model(wav, emb)
        barrier()
        dt = time.perf_counter() - t0
    assert bool(torch.isfinite(out).all())
    last_step = {"out": out.cpu()} if args.dump_outputs else None  # what the last timed forward returned: (B, 1, L) separated waveforms

    # per-launch durations of the dominant kernel, recorded during the timed region
    cap = 4096
    ms = (ctypes.c_float * cap)()
    ls = (ctypes.c_int * cap)()
    ns = (ctypes.c_int * cap)()
    n_ev = lib.rtfs_sweep_timing_collect(ms, ls, ns, cap)
    lib.rtfs_sweep_timing_enable(0)

    dt = max_over_ranks(dt, dist, dev)

    # the throughput option (two half batches as independent chains on forked streams), outside the contract's timed region: it makes every
    # kernel share the chip with a kernel of the other half, so it is reported beside the contract numbers, not instead of them (--full only)
    split2 = None
    if args.full and args.split == 1 and B >= 16 and not args.no_batch_split:
        R.set_batch_split(2)
        with torch.no_grad():
            for _ in range(2):
                out2 = model(wav, emb)
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out2 = model(wav, emb)
            barrier()
            dt2 = time.perf_counter() - t0
        R.set_batch_split(args.split)
        dt2 = max_over_ranks(dt2, dist, dev)
        split2 = {"value": round(throughput(world, B, args.steps, dt2), 3), "unit": "mixtures/s", "ms_per_step": round(dt2 / args.steps * 1e3, 3),
                  "steps": args.steps, "same_outputs": bool(torch.allclose(out2, out, rtol=0, atol=2e-5 * float(out.abs().max()))),
                  "what": "rtfs_set_batch_split(2): the same step as two half batches on two streams (not the contract measurement)"}

    ev = dist_evidence(dist, world, dev)  # a collective: every rank calls it
    if rank == 0:
        total_bytes = sum(sweep_bytes(ls[i], ns[i]) for i in range(n_ev))
        total_ms = sum(ms[i] for i in range(n_ev))
        achieved = total_bytes / (total_ms * 1e-3) / 1e9 if n_ev > 0 and total_ms > 0 else None
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "sweep_traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("batch") == B and tj.get("repeats") == args.repeats and tj.get("seconds") == args.seconds:
                    traffic = tj.get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        res = {
            "metric": f"mixtures/sec forward ({args.seconds:g} s@16 kHz, 2-spk) RTFS-Net-{args.repeats}",
            "value": round(throughput(world, B, args.steps, dt), 3),
            "unit": "mixtures/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": DTYPE,
            "data": "synthetic",
            "config": {"workload": f"RTFS-Net-{args.repeats} forward, batch {B}/GPU, {args.seconds:g} s @16 kHz 2-speaker mixtures "
                                   f"+ dummy lip embeddings (B,512,{Tv}), random-init weights, eval",
                       "per_gpu_batch": B, "global_batch": B * world, "samples": L, "parallelism": f"dp{world} (no data-path collective)"},
            "dist": ev,
            "roofline": {
                "kernel": "dp16s_kernel, the fused dual-path sweep (LN + unfold-GEMM + 4x bi-SRU scan + ConvTranspose1d + residual; k_dualpath16s.hip)",
                # "hbm" is the north_star's DEFINITION of this metric (algorithmic bytes at the reference's op boundary / launch time
                # against 8 TB/s).  What the counters say the fused kernel is really bound by is under "by_counters".
                "bound": "hbm",
                "achieved": None if achieved is None else round(achieved, 2),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": None if achieved is None else round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic,
                "launches_timed": int(n_ev),
                "avg_launch_ms": None if n_ev <= 0 else round(total_ms / n_ev, 4),
                "algorithmic_bytes_per_launch": None if n_ev <= 0 else round(total_bytes / n_ev),
                "by_counters": by_counters(traffic, None if n_ev <= 0 else total_ms / n_ev),
            },
        }
        if split2 is not None:
            res["batch_split_2"] = split2
        if cpu_res is not None:
            res["cpu_baseline"] = cpu_res
        if args.dump_outputs:
            res["dump_outputs"] = dump_outputs(args.dump_outputs, last_step)
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
