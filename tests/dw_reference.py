"""Plain restatement of the inference depthwise family (csrc/k_dw.hip), one function per form, in torch on the CPU.

Every function computes in the dtype of its tensor arguments: float64 is the reference tests/test_hip_dw_edges.py compares the kernels
with, float32 is the "same formula in float32" run that sets the float bars there, int64 (the plain convolutions only) is the
exact-integer reference.  A gLN is applied as the kernels apply it - from the (sum, sumsq) statistics of the pre-norm tensor - and the
statistics a consumer reads are always handed in by the caller, who takes them from the float64 reference of the producer: a consumer's
comparison must not inherit the producer's error.  Zero padding applies to the NORMALISED input (k_dw.hip's header): the fold comes
first, the convolution pads what the fold produced.

Tied to oracle/rtfs_oracle.py (which the reference project's own vectors pin) by tests/test_dw_reference_host.py."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.rtfs_oracle import EPS, nearest_index


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _w4(w, like):
    """(C, 16) or (C, 1, 4, 4) weights as the (C, 1, 4, 4) conv2d takes, in the dtype of ``like``."""
    return torch.as_tensor(w).to(like.dtype).reshape(-1, 1, 4, 4)


def _conv(x, w, bias, pad, stride):
    if x.dtype == torch.int64:  # conv2d has no integer form: exact in float64 (every sum is far below 2^53), then back
        return torch.round(_conv(x.double(), torch.as_tensor(w).double(), None if bias is None else torch.as_tensor(bias).double(), pad, stride)).long()
    b = None if bias is None else torch.as_tensor(bias).to(x.dtype)
    return F.conv2d(F.pad(x, pad), _w4(w, x), b, stride=stride, groups=x.shape[1])


def conv_s1(x, w, bias=None):
    """Depthwise 4x4, stride 1, 'same': pad 1 before and 2 behind on both axes."""
    return _conv(x, w, bias, (1, 2, 1, 2), 1)


def conv_s2(x, w, bias=None):
    """Depthwise 4x4, stride 2, pad 1: (H, W) -> (H // 2, W // 2)."""
    return _conv(x, w, bias, (1, 1, 1, 1), 2)


def stats(y):
    """(B, 2) float64: sum and sum of squares of every sample of a pre-norm tensor."""
    f = y.reshape(y.shape[0], -1).double()
    return torch.stack([f.sum(1), (f * f).sum(1)], 1)


def fold(y, st, gamma, beta):
    """gLN (GroupNorm(1, C)) of the pre-norm tensor ``y`` from its statistics ``st`` (B, 2): (y - mean) / sqrt(var + eps) * gamma + beta.
    Mean, variance, scale and shift are float64 whatever the dtype of y (the kernels' fold keeps them in f64 too, up to the rsqrt)."""
    B, C = y.shape[:2]
    n = y[0].numel()
    st = torch.as_tensor(st).double()
    mean = st[:, 0] / n
    var = (st[:, 1] / n - mean * mean).clamp_min(0)
    scale = torch.as_tensor(gamma).double()[None, :] / torch.sqrt(var + EPS)[:, None]  # (B, C)
    shift = torch.as_tensor(beta).double()[None, :] - mean[:, None] * scale
    shp = (B, C) + (1,) * (y.ndim - 2)
    return y * scale.reshape(shp).to(y.dtype) + shift.reshape(shp).to(y.dtype)


def up(x, size):
    """F.interpolate(mode='nearest') to ``size`` with torch's float32 index rule (oracle.rtfs_oracle.nearest_index)."""
    H, W = size
    ih = torch.as_tensor(nearest_index(x.shape[2], H))
    iw = torch.as_tensor(nearest_index(x.shape[3], W))
    return x[:, :, ih][:, :, :, iw]


def combine(l, l_st, l_gb, gate, gate_st, gate_gb, emb, emb_st, emb_gb):
    """Same-size InjectionMultiSum: gLN(l) * sigmoid(gLN(gate)) + gLN(emb).  *_gb = (gamma, beta)."""
    return fold(l, l_st, *l_gb) * torch.sigmoid(fold(gate, gate_st, *gate_gb)) + fold(emb, emb_st, *emb_gb)


def apply(x, w, loc_st, loc_gb, gate, gate_st, gate_gb, emb, emb_st, emb_gb, addend=None, add_st=None, add_gb=None):
    """TFAR apply: gLN(conv(x)) * sigmoid(up(gLN(G))) + up(gLN(E)) [+ gLN(addend)].  x is the conv's input as the conv sees it (the caller
    folds a pre-norm input first); loc_st are the statistics of conv(x)."""
    size = x.shape[2:]
    y = fold(conv_s1(x, w), loc_st, *loc_gb) * torch.sigmoid(up(fold(gate, gate_st, *gate_gb), size)) + up(fold(emb, emb_st, *emb_gb), size)
    if addend is not None:
        y = y + fold(addend, add_st, *add_gb)
    return y


def s2_pool(d0, w, bias, size):
    """Stride-2 conv of d0 and adaptive_avg_pool2d of d0 at ``size`` (the conv's output size on the block's path)."""
    return conv_s2(d0, w, bias), F.adaptive_avg_pool2d(d0, size)


def g_form(p0, c1, c1_st, c1_gb):
    """g = p0 + gLN(c1)."""
    return p0 + fold(c1, c1_st, *c1_gb)
