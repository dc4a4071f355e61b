"""A minimal data-parallel training loop on the HIP path - what the reference's train.py (135-160) asks of Lightning, spelled out:
AVNet from the unchanged yaml section, AdamW, SyncBatchNorm, System.optimization_step (forward_train -> PIT loss -> HIP backward ->
one flattened gradient all-reduce -> clip 5.0 -> step), best_model.pth written in the reference's format.  Data are synthetic mixtures
(no dataset in this repo): the point is the step, not the recipe.

1 GPU :  python tools/train_synthetic.py --steps 20
N GPUs:  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port 29511 tools/train_synthetic.py
"""
import argparse
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import rtfs_net_amd as R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="per GPU (yaml training.batch_size)")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--out", default="")
    ap.add_argument("--optimizer", choices=["torch", "fused"], default="torch", help="fused: rtfs_net_amd.optimizers.AdamW (gather, one "
                    "all-reduce on its flat buffer, clip + update in two launches)")
    ap.add_argument("--online-mix", action="store_true", help="every step's batch is formed on the device by System.mix_batch from a "
                    "synthetic pool of utterances and ROI tracks (target + one interferer at a drawn SNR and crop; needs the video model)")
    ap.add_argument("--reverb", action="store_true", help="with --online-mix: every source is convolved with one of 8 synthetic room impulse "
                    "responses of 4096 taps (datas.synthetic_rir, a stand-in, not a room simulation) before the mix")
    a = ap.parse_args()
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world)  # RCCL
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    conf = copy.deepcopy(RTFS4_AUDIONET)
    conf["audio_params"]["repeats"] = a.repeats
    torch.manual_seed(0)  # identical initial weights on every rank
    model = R.AVNet(print_macs=False, **conf).cuda().train()
    loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
    opt = (R.optimizers.AdamW if a.optimizer == "fused" else torch.optim.AdamW)(model.parameters(), lr=a.lr, weight_decay=0.1)
    video = R.FRCNNVideoModel(print_macs=False).cuda().eval() if a.online_mix else None
    system = R.System(audio_model=model, video_model=video, loss_func={"train": loss, "val": loss}, optimizer=opt,
                      config={"training": {"batch_size": a.batch}})
    if world > 1:
        system.convert_sync_batchnorm()  # train.py:145 sync_batchnorm=True
    g = torch.Generator().manual_seed(1234 + rank)  # every rank its own shard
    L, Tv = int(16000 * a.seconds), int(25 * a.seconds)
    if a.online_mix:  # 16 utterances of 3 .. 12 s with their 25 fps ROI tracks; the draws of every rank come from its own seed
        import random
        rng = random.Random(1234 + rank)
        secs = [3 + (9 * i) // 15 for i in range(16)]
        pool = [(0.05 * torch.randn(16000 * s, generator=g)).cuda() for s in secs]
        rois = [torch.randint(0, 256, (25 * s, 96, 96), generator=g, dtype=torch.uint8).cuda() for s in secs]
        rirs = None
        if a.reverb:
            import numpy as np
            nrng = np.random.RandomState(1234 + rank)
            rirs, _ = R.datas.load_rirs([R.datas.synthetic_rir(4096, 0.2 + 0.05 * i, delay=16, rng=nrng) for i in range(8)])
    t0 = time.time()
    for step in range(a.steps):
        if a.online_mix:
            value = system.optimization_step(system.mix_batch(pool, rois, length=L - L % 640, rng=rng, rirs=rirs), step)
            if rank == 0 and (step % 5 == 0 or step == a.steps - 1):
                torch.cuda.synchronize()
                print(f"step {step:4d}  loss {float(value):8.4f}  {(time.time() - t0) / (step + 1) * 1e3:7.1f} ms/step  world {world}  "
                      f"online mix", flush=True)
            continue
        s1, s2 = 0.05 * torch.randn(a.batch, L, generator=g), 0.05 * torch.randn(a.batch, L, generator=g)
        batch = ((s1 + s2).cuda(), s1.unsqueeze(1).cuda(), torch.randn(a.batch, 512, Tv, generator=g).cuda(), None)
        value = system.optimization_step(batch, step)
        if rank == 0 and (step % 5 == 0 or step == a.steps - 1):
            torch.cuda.synchronize()
            print(f"step {step:4d}  loss {float(value):8.4f}  {(time.time() - t0) / (step + 1) * 1e3:7.1f} ms/step  world {world}", flush=True)
    if rank == 0 and a.out:
        torch.save(system.audio_model.serialize(), a.out)  # best_model.pth format (base_av_model.py:36-51)
        print("wrote", a.out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
