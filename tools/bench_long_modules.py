"""Time the long-utterance modules of one tree: DualPathRNN along T (SRU) and MultiHeadSelfAttention2D at T' = 250 ... 512, eval mode.

    python tools/bench_long_modules.py [--root TREE] [--batch 8] [--iters 20]

--root picks the tree whose package is imported (default: this one), so an older checkout can be timed with the same script (A/B on one
box, alternating, NOTES.md "How to measure").  One JSON line per case: ms per call (median of --iters, CUDA events) and the number of
library kernel launches per call (3 = the fused path).
"""
import argparse
import copy
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lengths", default="250,400,512")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import rtfs_net_amd as R
    from oracle.params import load_spec, make_state_dict
    from rtfs_net_amd.configs import RTFS4_AUDIONET

    sd = make_state_dict(load_spec("state_spec_R4.json"), 0)
    m = R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    lib = R._lib.load()
    mods = {"dualpath_T": m.refinement_module.audio_net.blocks.globalatt[1], "mhsa2d": m.refinement_module.audio_net.blocks.globalatt[2]}
    for T in [int(t) for t in args.lengths.split(",")]:
        x = torch.randn((args.batch, 64, T, 64), device="cuda", generator=torch.Generator(device="cuda").manual_seed(T))
        for name, mod in mods.items():
            with torch.no_grad():
                for _ in range(3):
                    mod(x)
                torch.cuda.synchronize()
                n0 = lib.rtfs_debug_launch_count()
                mod(x)
                torch.cuda.synchronize()
                nl = lib.rtfs_debug_launch_count() - n0
                times = []
                for _ in range(args.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    mod(x)
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
            times.sort()
            print(json.dumps({"module": name, "B": args.batch, "T": T, "ms": round(times[len(times) // 2], 4), "launches": nl}), flush=True)


if __name__ == "__main__":
    main()
