#!/usr/bin/env python3
"""Golden vectors at lengths where torch's float32 'nearest' index rule departs from floor(dst * n_in / n_out)
(CONTAINER ONLY: needs /root/reference; never runs on the GPU box).  DESIGN.md, "Nearest up-sampling", has the rule and the pairs.

The reference's own modules (stubs as in make_golden.py) run in float32 on stock torch, so every F.interpolate(mode="nearest") in these
vectors takes the source index min(int(floorf(dst * (float(n_in) / float(n_out)))), n_in - 1).  Writes, under tests/golden/, in
make_golden.py's probe format:
  mod_caf_T82_Tv16, mod_caf_T164_Tv32   the CAF cell, B = 2, F = 129; besides the probe, the output frames that read another video frame
                                        than the exact-arithmetic rule would (41; 41 and 82) are stored whole as out.frame<t>; a whole
                                        frame is 258 KiB, so the second one goes to a file of its own, mod_caf_T164_Tv32_frame82
  mod_vp122                             the VP block, B = 2, Tv = 122 (16 -> 122 departs at output frames 60..62); frames 59..63 whole
  e2e_R4_L20900_B1                      whole model, Tv = 32, T = 164, the probes of the other e2e files
  grad_R2_L10400_B1                     loss, output and parameter gradients at Tv = 16, T = 82, as make_golden_grad.py's eval case.
                                        That recipe runs the reference in float64 for gradients exact to ~1e-12, and on float64 tensors
                                        torch computes the nearest index in float64, i.e. by the exact rule, which the reference's float32
                                        training never uses.  So for this one file F.interpolate(mode="nearest") is wrapped: the wrapper asks
                                        stock torch itself for the float32 indices (it up-samples a float32 ramp 0..n_in-1) and gathers
                                        the float64 tensor through them.  Nothing else of the reference is touched.  Tensors of up to
                                        N_SAMPLE = 1024 elements are stored whole, larger ones as 1024 seeded samples + their L2 norm.
"""
import importlib
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as MG, make_golden_grad as MGG  # noqa: E402
from oracle.params import make_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N_SAMPLE = 1024


def sample_idx(name, n):
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return rs.choice(n, N_SAMPLE, replace=False).astype(np.int64)


def save(name, tensors, frames=(), own_file=()):
    d = {}
    for k, v in tensors.items():
        d.update(MG.probe(v.numpy(), k))
    out = tensors["out"].numpy()
    for fr in frames:  # the time axis is 2 in both (B, C, T, F) and (B, C, T)
        d[f"out.frame{fr}"] = np.ascontiguousarray(np.take(out, fr, axis=2))
    path = os.path.join(OUT, name + ".npz")
    np.savez(path, **d)
    print(name, tuple(out.shape), os.path.getsize(path) // 1024, "KiB")
    for fr in own_file:
        np.savez(os.path.join(OUT, f"{name}_frame{fr}.npz"), **{f"out.frame{fr}": np.ascontiguousarray(np.take(out, fr, axis=2))})


def e2e(model, name, B, L, Tv, seed):
    """make_golden.py's e2e(): the whole output + probes of the internal tensors."""
    wav, emb = make_inputs(B, L, Tv, seed)
    caps, blocks_out, hooks = {}, [], []
    rm = model.refinement_module
    hooks.append(model.encoder.register_forward_hook(lambda _m, _i, o: caps.__setitem__("a0", o.clone())))
    hooks.append(model.audio_bottleneck.register_forward_hook(lambda _m, _i, o: caps.__setitem__("a1", o.clone())))
    hooks.append(rm.audio_net.blocks.register_forward_hook(lambda _m, _i, o: blocks_out.append(o.clone())))
    hooks.append(rm.video_net.blocks.register_forward_hook(lambda _m, _i, o: caps.__setitem__("vp", o.clone())))
    hooks.append(rm.crossmodal_fusion.fusion_module.register_forward_hook(lambda _m, _i, o: caps.__setitem__("caf", o[0].clone())))
    hooks.append(model.mask_generator.register_forward_hook(lambda _m, _i, o: caps.__setitem__("sep", o.clone())))
    out = model(MG.t(wav), MG.t(emb))
    for h in hooks:
        h.remove()
    d = {"out": out.numpy()}
    for k, v in caps.items():
        d.update(MG.probe(v.numpy(), k))
    d.update(MG.probe(blocks_out[0].numpy(), "block0"))
    d.update(MG.probe(blocks_out[-1].numpy(), "refined"))
    path = os.path.join(OUT, name + ".npz")
    np.savez(path, **d)
    print(name, "out", tuple(out.shape), float(out.abs().mean()), os.path.getsize(path) // 1024, "KiB")


def interpolate_f32_indices(x, size=None, scale_factor=None, mode="nearest", **kw):
    """F.interpolate for the float64 gradient run: mode='nearest' gathers through the indices stock torch computes on float32."""
    if mode != "nearest" or x.dtype == torch.float32 or size is None:
        return _interpolate(x, size=size, scale_factor=scale_factor, mode=mode, **kw)
    size = (size,) if isinstance(size, int) else tuple(size)
    for ax, n_out in zip(range(x.dim() - len(size), x.dim()), size):
        n_in = x.shape[ax]
        ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in)
        x = x.index_select(ax, _interpolate(ramp, size=int(n_out), mode="nearest").view(-1).long())
    return x


_interpolate = F.interpolate


def grad_case(AVNet, name, B, Ls, Tv, seed_in, seed_tgt):
    """make_golden_grad.py's eval case (BatchNorm running statistics, dropout off; B = 1 has no batch statistics to train on)."""
    L = importlib.import_module("src.losses")
    wav, emb = make_inputs(B, Ls, Tv, seed=seed_in)
    tgt = (0.05 * np.random.default_rng(seed_tgt).standard_normal((B, 1, Ls))).astype(np.float32)
    m, _, _ = MG.build(AVNet, 2, seed=0)
    m = m.double().eval()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, nn.MultiheadAttention):
            mod.dropout = 0.0
    F.interpolate = interpolate_f32_indices
    try:
        with torch.enable_grad():
            est = m(torch.from_numpy(wav).double(), torch.from_numpy(emb).double())
            loss = L.PITLossWrapper(L.PairwiseNegSDR("snr"), pit_from="pw_mtx")(est, torch.from_numpy(tgt).double())
            loss.backward()
    finally:
        F.interpolate = _interpolate
    out = {"eval/loss": np.float64(loss.item()), "eval/est": est.detach().numpy().astype(np.float32)}
    for k, p in m.named_parameters():
        g = p.grad.detach().numpy().reshape(-1)
        if g.size <= N_SAMPLE:
            out[f"eval/{k}"] = g.astype(np.float64)
        else:
            out[f"eval/{k}"] = g[sample_idx(k, g.size)].astype(np.float64)
            out[f"eval/{k}#l2"] = np.float64(np.sqrt((g ** 2).sum()))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", loss.item(), os.path.getsize(path) // 1024, "KiB")


def main():
    MG._SRU = MGG._SRU  # differentiable SRU stand-in; its forward is the same arithmetic as make_golden.py's
    AVNet = MG.import_reference()
    torch.manual_seed(0)
    with torch.no_grad():
        m, _, _ = MG.build(AVNet, 4, seed=0)
        cell = m.refinement_module.crossmodal_fusion.fusion_module
        vblk = m.refinement_module.video_net.blocks
        a, v = MG.rand((2, 256, 82, 129), 201), MG.rand((2, 512, 16), 202)
        save("mod_caf_T82_Tv16", {"out": cell(MG.t(a), MG.t(v))[0]}, frames=(41,))
        a, v = MG.rand((2, 256, 164, 129), 203), MG.rand((2, 512, 32), 204)
        save("mod_caf_T164_Tv32", {"out": cell(MG.t(a), MG.t(v))[0]}, frames=(41,), own_file=(82,))
        v = MG.rand((2, 512, 122), 205)
        save("mod_vp122", {"out": vblk(MG.t(v))}, frames=(59, 60, 61, 62, 63))
        e2e(m, "e2e_R4_L20900_B1", 1, 20900, 32, seed=41)
    grad_case(AVNet, "grad_R2_L10400_B1", 1, 10400, 16, seed_in=42, seed_tgt=43)


if __name__ == "__main__":
    main()
