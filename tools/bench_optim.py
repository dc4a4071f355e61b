"""The optimizer update alone on the RTFS-Net-4 parameter set (264 tensors, 739,952 floats) with fixed random gradients:
clip_grad_norm_(5.0) + torch.optim.AdamW against the fused rtfs_net_amd.optimizers.AdamW (csrc/k_optim.hip), device events around
--steps steps after warm-up, the two alternating in one process over --rounds rounds so the spread is visible.  One JSON line.
python tools/bench_optim.py [--steps 200] [--rounds 5] [--json FILE] [--only torch|fused]   (GPU box)"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import rtfs_net_amd as R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["torch", "fused"], default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim.py measures on the GPU only"
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    torch.manual_seed(0)
    shapes = [p.shape for p in R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET)).parameters()]
    g = torch.Generator().manual_seed(1)
    init = [0.1 * torch.randn(s, generator=g) for s in shapes]
    grads = [torch.randn(s, generator=g).cuda() for s in shapes]

    def make(fused):
        ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt = (R.optimizers.AdamW if fused else torch.optim.AdamW)(ps, lr=1e-3, weight_decay=0.1)
        if fused:
            return lambda: opt.step(max_norm=5.0)

        def step():
            torch.nn.utils.clip_grad_norm_(ps, 5.0)
            opt.step()
        return step
    steps = {k: make(k == "fused") for k in ("torch", "fused") if a.only in ("", k)}
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    us = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.steps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            us[k].append(ev[0].elapsed_time(ev[1]) / a.steps * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    res = {"what": "clip 5.0 + AdamW update, RTFS-Net-4 parameter set", "tensors": len(shapes), "floats": sum(t.numel() for t in init),
           "steps_per_round": a.steps, "us_per_step": us, "median_us": med, "spread_us": {k: max(v) - min(v) for k, v in us.items()}}
    if len(med) == 2:
        res["stock_over_fused"] = med["torch"] / med["fused"]
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
