"""Plain torch restatement of the three stages of the TF-domain self-attention (csrc/k_attn.hip), written from the reference model's
formulas (attention.py:149-189, conv_layers.py:196-205, normalizations.py:20-41), for tests/test_hip_attn_edges.py.
tests/test_attn_reference_host.py ties the three stages, composed, to oracle/rtfs_oracle.py::mhsa2d.

    qkv    x (B,64,T,64) -> Q, K (B,4,T,256 = e*64+f), V (B,4,T,1024 = c*64+f): twelve ConvActNorm = 1x1 conv -> PReLU -> LayerNorm over
           (channels of the module, F), channel order Q_h (4 each), K_h (4 each), V_h (16 each)
    core   softmax_keys(Q K^T * scale) V per (b, head) -> (B,64,T,64), channel = head*16 + c
    proj   ConvActNorm over all 64 channels + residual

One formula, two arithmetics (pw_reference.Arith):
  EXACT   float64 throughout.
  F16X3   a CPU emulation of what the k_attn.hip header says the kernels compute.  Row GEMM: 256 w split into f16 hi + lo, the activation
          into hi + lo with the lo part flushed where it is an f16 subnormal, the products hi.hi, hi.lo, lo.hi, float32 accumulation
          (Arith.mm); PReLU; a float32 two-pass LayerNorm per group (mean, centred sum of squares, 1 / sqrtf).  Core: Q and K both split
          as activations (Arith.mm_aa), scores * scale, a float32 softmax (max, expf, sum, one reciprocal), P * 4096 split, 64 V split
          (the row kernel stores V times 64, exactly, through its LayerNorm affine), result / (4096 * 64).  It calls no library code.

Every stage returns (outputs, denominators): per output element a scale-free bound of the first-order rounding error per unit of relative
operand error eps, so that a small-magnitude row is not hidden by a tensor maximum.

LayerNorm outputs.  y = PReLU(W x + b) carries |dy| <= eps s with s = |W| @ |X| + |b| (PReLU slopes are at most 1 in magnitude here).  With
out = gamma (y - mu) rstd + beta over a group of n elements: d out = gamma rstd (dy - dmu) + gamma (y - mu) d rstd.  |dy - dmu| <= 2 eps S
with S the group maximum of s; d rstd / rstd = -d var / (2 (var + eps0)) and |d var| <= 2 sigma (2 eps S), so the second term is at most
2 eps S |gamma| rstd |y - mu| / sigma: both terms are O(1) multiples of eps |gamma| rstd S.  The denominator is therefore
    |gamma| rstd_ref S + |beta|   (+ |res| for the projection),
rstd_ref and S taken per (b, t, group); the O(1) factor is the same for the emulation and for the GPU and is part of the measured value.

Core.  With scores s_j = scale q.k_j carrying |ds_j| <= eps A_j, A = |scale| |Q| @ |K|^T, the softmax gives dP_j = P_j (ds_j - sum_k P_k ds_k),
so |dO| <= eps [ (P * A) @ |V| + rowsum(P * A) (P @ |V|) ] from the scores, plus eps P @ |V| from the second product.  The denominator is
    P_ref @ |V| + (P_ref * A) @ |V| + rowsum(P_ref * A) * (P_ref @ |V|)."""
import numpy as np
import torch

from oracle.rtfs_oracle import EPS
from tests.pw_reference import EXACT, F16X3, F16_MIN_NORMAL, Arith, err, prelu, t64  # noqa: F401  (err, EXACT, F16X3: this module's interface)

PSC = 4096.0  # ATT_PSC of k_attn.hip
VSC = 64.0    # ATT_VSC of kernels.h: between the two launches V is stored times this power of two (exact), so that a small element keeps its low half
H, E, CV, F = 4, 4, 16, 64
GROUP_START = [4 * g if g <= 8 else 32 + 16 * (g - 8) for g in range(13)]  # Q_h x4, K_h x4 (4 channels), V_h x4 (16 channels)
GROUP_OF = np.repeat(np.arange(12), np.diff(GROUP_START))


def _split_act(x):
    """f16 hi + lo of an activation; lo is flushed to zero where it is an f16 subnormal."""
    xh = x.half().float()
    xl = x - xh
    return xh, torch.where(xl.abs() < F16_MIN_NORMAL, torch.zeros_like(xl), xl).half().float()


def _mm_aa(self, a, b):
    """a @ b with BOTH operands activations (the core's Q K^T and P V): float64, or hi.hi + hi.lo + lo.hi in float32."""
    a, b = self.t(a), self.t(b)
    if self.name != "f16x3":
        return torch.matmul(a, b)
    ah, al = _split_act(a)
    bh, bl = _split_act(b)
    return torch.matmul(ah, bh) + torch.matmul(ah, bl) + torch.matmul(al, bh)


Arith.mm_aa = _mm_aa


def layer_norm(ar, y, gamma, beta):
    """LayerNorm over the last two axes (channels of the group, F) of y (..., n, F).  -> (out, rstd)"""
    if ar is EXACT:
        mu = y.mean((-2, -1), keepdim=True)
        var = ((y - mu) ** 2).mean((-2, -1), keepdim=True)
        rstd = 1.0 / torch.sqrt(var + EPS)
        return (y - mu) * rstd * t64(gamma) + t64(beta), rstd
    n = np.float32(y.shape[-1] * y.shape[-2])
    mu = y.sum((-2, -1), keepdim=True) / n
    c = y - mu
    rstd = 1.0 / torch.sqrt((c * c).sum((-2, -1), keepdim=True) / n + np.float32(EPS))
    return c * rstd * ar.t(gamma) + ar.t(beta), rstd


def _conv_act(ar, x, w, b, slopes):
    """x (B,64,T,F), w (O,64), b (O), slopes (O) per output channel -> y (B,T,O,F), s = |W| @ |X| + |b| likewise (reference arithmetic only)"""
    B, C, T, F_ = x.shape
    xf = np.asarray(x).reshape(B, C, T * F_)
    y = ar.mm(w, xf) + ar.t(b).reshape(1, -1, 1)
    y = prelu(y, ar.t(slopes).reshape(1, -1, 1))
    O = y.shape[1]
    y = y.reshape(B, O, T, F_).permute(0, 2, 1, 3)
    if ar is not EXACT:
        return y, None
    s = torch.matmul(t64(w).abs(), t64(xf).abs()) + t64(b).abs().reshape(1, -1, 1)
    return y, s.reshape(B, O, T, F_).permute(0, 2, 1, 3)


def qkv(ar, x, w, b, slope, gamma, beta):
    """w (96,64), b (96), slope (12) one per module, gamma / beta (96,64).  -> ((q, k, v), (dq, dk, dv)); the denominators come with the
    reference arithmetic only (None otherwise): they are the reference's own."""
    slopes = np.asarray(slope)[GROUP_OF]
    y, s = _conv_act(ar, x, w, b, slopes)
    B, T = y.shape[:2]
    gamma, beta = np.asarray(gamma), np.asarray(beta)
    g64, b64 = t64(gamma), t64(beta)
    outs, dens = [], []
    for c0, n in ((0, E), (16, E), (32, CV)):
        yo, do = [], []
        for h in range(H):
            sl = slice(c0 + n * h, c0 + n * (h + 1))
            o, rstd = layer_norm(ar, y[:, :, sl], gamma[sl], beta[sl])
            yo.append(o.reshape(B, T, n * F))
            if ar is EXACT:
                S = s[:, :, sl].amax((-2, -1), keepdim=True)
                do.append((g64[sl].abs() * rstd * S + b64[sl].abs()).reshape(B, T, n * F))
        outs.append(torch.stack(yo, 1))
        dens.append(torch.stack(do, 1) if ar is EXACT else None)
    return tuple(outs), tuple(dens)


def core(ar, q, k, v, scale=1.0 / 16.0):
    """q, k (B,4,T,256), v (B,4,T,1024) -> ((o (B,64,T,64),), (den,)); den with the reference arithmetic only"""
    B, _, T, _ = q.shape
    s = ar.mm_aa(q, ar.t(k).transpose(-1, -2))
    if ar is EXACT:
        p = torch.softmax(s * scale, -1)
        o = torch.matmul(p, t64(v))
    else:
        s = s * np.float32(scale)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        p = e * (1.0 / e.sum(-1, keepdim=True))
        o = ar.mm_aa(p * np.float32(PSC), ar.t(v) * np.float32(VSC)) * np.float32(1.0 / (PSC * VSC))
    def chan(z):  # (B,4,T,16*64) -> (B,64,T,64)
        return z.reshape(B, H, T, CV, F).permute(0, 1, 3, 2, 4).reshape(B, H * CV, T, F)
    if ar is not EXACT:
        return (chan(o),), (None,)
    pr = p
    A = torch.matmul(t64(q).abs(), t64(k).abs().transpose(-1, -2)) * abs(scale)
    va = t64(v).abs()
    pv = torch.matmul(pr, va)
    den = pv + torch.matmul(pr * A, va) + (pr * A).sum(-1, keepdim=True) * pv
    return (chan(o),), (chan(den),)


def proj(ar, o, res, w, b, slope, gamma, beta):
    """o, res (B,64,T,64); w (64,64), b (64), slope scalar, gamma / beta (64,64) -> ((out,), (den,)); den with the reference arithmetic only"""
    sl = np.full(64, float(np.asarray(slope).reshape(-1)[0]), np.float32)
    y, s = _conv_act(ar, o, w, b, sl)
    out, rstd = layer_norm(ar, y, gamma, beta)
    out = (out + ar.t(res).permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    if ar is not EXACT:
        return (out,), (None,)
    den = t64(gamma).abs() * rstd * s.amax((-2, -1), keepdim=True) + t64(beta).abs() + t64(res).abs().permute(0, 2, 1, 3)
    return (out,), (den.permute(0, 2, 1, 3),)


def mhsa(ar, x, P):
    """The three stages composed.  P: dict qkv_w, qkv_b, qkv_slope, qkv_gamma, qkv_beta, proj_w, proj_b, proj_slope, proj_gamma, proj_beta."""
    (q, k, v), _ = qkv(ar, x, P["qkv_w"], P["qkv_b"], P["qkv_slope"], P["qkv_gamma"], P["qkv_beta"])
    (o,), _ = core(ar, q, k, v)
    (y,), _ = proj(ar, o, x, P["proj_w"], P["proj_b"], P["proj_slope"], P["proj_gamma"], P["proj_beta"])
    return y


def params_of(p):
    """The oracle's state dict of one MultiHeadSelfAttention2D -> the arrays above, in the kernels' channel order."""
    mods = [f"{n}.{h}" for n in ("Queries", "Keys", "Values") for h in range(H)]
    def cat(key, *tail):
        return np.concatenate([np.asarray(p[f"{m}.{key}"]).reshape(-1, *tail) for m in mods])
    a = "attn_concat_proj."
    return dict(qkv_w=cat("conv.weight", 64), qkv_b=cat("conv.bias"), qkv_slope=np.array([np.asarray(p[f"{m}.act.weight"]).reshape(-1)[0] for m in mods]),
                qkv_gamma=cat("norm.gamma", F), qkv_beta=cat("norm.beta", F),
                proj_w=np.asarray(p[a + "conv.weight"]).reshape(64, 64), proj_b=np.asarray(p[a + "conv.bias"]),
                proj_slope=np.asarray(p[a + "act.weight"]).reshape(-1)[:1], proj_gamma=np.asarray(p[a + "norm.gamma"]).reshape(64, F),
                proj_beta=np.asarray(p[a + "norm.beta"]).reshape(64, F))


# ------------------------------------------------------------------------------------------------ the sweep's float-tier inputs
SCALE = 16.0   # activations of the row GEMMs: below 2^-3 an activation loses its flushed f16 lo part by design ("Range")
QK_GAMMA = 8.0  # the core's Q / K / V are LayerNorm outputs, unit scale times gamma plus beta; gamma near 8 keeps them in that range too
CORE_SCALE = 2.0 ** -9  # scores then have a standard deviation near 2: the softmax is neither flat nor one-hot


def row_params(rng, nout):
    """Random weights, all-distinct PReLU slopes (one per module), gamma and beta random per (channel, f)."""
    ng = 12 if nout == 96 else 1
    return dict(w=(rng.standard_normal((nout, 64)) / 8).astype(np.float32), b=rng.standard_normal(nout).astype(np.float32),
                slope=rng.permutation(0.1 + 0.07 * np.arange(ng)).astype(np.float32),
                gamma=(1 + 0.3 * rng.standard_normal((nout, F))).astype(np.float32), beta=(0.5 * rng.standard_normal((nout, F))).astype(np.float32))


def row_input(rng, B, T):
    """(B,64,T,64): every frame an independent draw."""
    return (SCALE * rng.standard_normal((B, 64, T, F))).astype(np.float32)


def core_inputs(rng, B, T):
    def ln_like(width):
        g = (QK_GAMMA * (1 + 0.3 * rng.standard_normal((1, H, 1, width)))).astype(np.float32)
        return (rng.standard_normal((B, H, T, width)).astype(np.float32) * g + rng.standard_normal((1, H, 1, width)).astype(np.float32))
    return ln_like(E * F), ln_like(E * F), ln_like(CV * F)
