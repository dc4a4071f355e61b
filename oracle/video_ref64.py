"""Fast float64 restatement of the video front-end (TEST INFRASTRUCTURE ONLY; the package never imports it).

Written from ``oracle/video_oracle.py``: the same layer order on stock ``torch.nn.functional`` ops over ``double`` CPU tensors,

  lips (B, 1, T, 88, 88) -> Conv3d(1,64,(5,7,7),s(1,2,2),p(2,3,3)) -> eval BatchNorm3d -> PReLU(64) -> MaxPool3d((1,3,3),s(1,2,2),p(0,1,1))
       -> frames (B*T, 64, 22, 22) -> BasicBlock x [2,2,2,2] (64,128,256,512; stride 2 and a 1x1-conv + BatchNorm skip from layer 2 on)
       -> mean over the plane -> (B, 512, T)

with nothing rounded to float32 between layers (the numpy oracle rounds after every layer: the two agree to ~1e-7).  The numpy
oracle takes about a second per frame; this one takes about a second per hundred frames, which is what lets the GPU tests reach the
frame counts at which the deep layers' tile decode leaves its first round (tests/test_hip_video_edges.py).

Pinned on the CPU against the numpy oracle and against the reference module's own outputs (tests/test_oracle_golden.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).double()


def _bn(x, p, prefix):
    """nn.BatchNorm{2,3}d in eval mode (running statistics)."""
    return F.batch_norm(x, _t(p[prefix + ".running_mean"]), _t(p[prefix + ".running_var"]), _t(p[prefix + ".weight"]),
                        _t(p[prefix + ".bias"]), training=False, eps=BN_EPS)


def _block(x, p, prefix, stride):
    out = F.prelu(_bn(F.conv2d(x, _t(p[prefix + ".conv1.weight"]), stride=stride, padding=1), p, prefix + ".bn1"),
                  _t(p[prefix + ".relu1.weight"]))
    out = _bn(F.conv2d(out, _t(p[prefix + ".conv2.weight"]), stride=1, padding=1), p, prefix + ".bn2")
    if prefix + ".downsample.0.weight" in p:
        res = _bn(F.conv2d(x, _t(p[prefix + ".downsample.0.weight"]), stride=stride), p, prefix + ".downsample.1")
    else:
        res = x
    return F.prelu(out + res, _t(p[prefix + ".relu2.weight"]))


def video_frontend64(x, sd):
    """x (B, 1, T, 88, 88), sd: name -> array (oracle.video_oracle.make_video_state_dict) -> (B, 512, T) float64 numpy."""
    with torch.no_grad():
        x = _t(x)
        B, _, T, _, _ = x.shape
        y = F.conv3d(x, _t(sd["frontend3D.0.weight"]), stride=(1, 2, 2), padding=(2, 3, 3))
        y = F.prelu(_bn(y, sd, "frontend3D.1"), _t(sd["frontend3D.2.weight"]))
        y = F.max_pool3d(y, kernel_size=(1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
        f = y.transpose(1, 2).reshape(B * T, 64, y.shape[3], y.shape[4])
        for li, stride in ((1, 1), (2, 2), (3, 2), (4, 2)):
            for bi in range(2):
                f = _block(f, sd, f"trunk.layer{li}.{bi}", stride if bi == 0 else 1)
        v = f.mean((2, 3))  # (B*T, 512)
        return np.ascontiguousarray(v.reshape(B, T, 512).transpose(1, 2).numpy())
