"""Plain torch restatement of the inference pointwise (1x1 convolution) family, written from the reference model's formulas, for
tests/test_hip_pw_edges.py.  tests/test_pw_reference_host.py ties it to oracle/rtfs_oracle.py.

Tensors are (B, C, P) with the pixel index p = t F + f last; weights are (cout, cin).  Every op returns (outputs, scales): `scales` holds,
per output element, |W| @ |X| + |addends| of the GEMM that produced it (X = the GEMM's actual input), the scale-free denominator of the
sweep's float comparison - a small-magnitude row is not hidden by a large tensor maximum.

One formula, three arithmetics (the `ar` argument):
  EXACT   float64 throughout: the reference.  On the exact tier's integer data it is also the integer result.
  F32     float32 torch: what the exact-f32 kernels (k_pw.hip) are held to.
  F16X3   a CPU emulation of the split-precision kernels as the k_pw16.hip / k_pwr.hip headers describe them: activations and 256 w split
          into f16 hi + lo (an activation's lo part is flushed to zero where it is an f16 subnormal, as tests/test_hip_parity.py::
          test_mfma_f16_fragment_layout records for this toolchain's conversion; the weight images are split on the host and keep theirs),
          the three products hi.hi, hi.lo, lo.hi, float32 accumulation, the gLN fold with a float32 rsqrt.  It calls no library code.

    gLN -> ReLU -> 1x1                         audio_bn        tdavnet.py:59, conv_layers.py:65-129
    gateway dw 1x1 + PReLU -> projection       gateway_proj    separators/tdanet.py:106-107
    residual conv + residual                   residual        separators/tdanet.py:129
    block boundary                             boundary        tdanet.py:129, refinement_module.py:58-60, fusion.py:204-226, tdanet.py:106-107
    CAF on the audio side                      caf_apply       layers/fusion.py:205-226, tv = nearest_src(t, Tv, T) by the float32 rule
    PReLU -> 1x1 -> ReLU -> complex product    s3              mask_generator.py:49-59,67-99
    decoder ConvTranspose2d as 18 tap maps     taps            decoder.py:96-104"""
import numpy as np
import torch

from oracle.rtfs_oracle import EPS, nearest_index

F16_MIN_NORMAL = 2.0 ** -14


class Arith:
    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype

    def t(self, x):
        return x.to(self.dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(self.dtype)

    def mm(self, w, x):
        """(o, c) @ (B, c, P)"""
        w, x = self.t(w), self.t(x)
        if self.name != "f16x3":
            return torch.matmul(w, x)
        ws = w * 256.0
        wh = ws.half().float()
        wl = (ws - wh).half().float()
        xh = x.half().float()
        xl = x - xh
        xl = torch.where(xl.abs() < F16_MIN_NORMAL, torch.zeros_like(xl), xl).half().float()
        return (torch.matmul(wh, xh) + torch.matmul(wh, xl) + torch.matmul(wl, xh)) * (1.0 / 256.0)

    def rstd(self, var):
        """1 / sqrt(var + eps): float64 in the reference, the float32 rsqrt of gln_fold otherwise."""
        if self.dtype == torch.float64:
            return 1.0 / torch.sqrt(var + EPS)
        return (1.0 / torch.sqrt((var + EPS).float())).double()


EXACT, F32, F16X3 = Arith("exact", torch.float64), Arith("f32", torch.float32), Arith("f16x3", torch.float32)


def t64(x):
    return EXACT.t(x)


def absmm(w, x):
    return torch.matmul(t64(w).abs(), t64(x).abs())


def col(v, ar):
    return ar.t(v).reshape(1, -1, 1)


def prelu(x, slope):
    return torch.where(x >= 0, x, x * slope)


def stats(x):
    """(B, 2) float64 sum and sum of squares per sample: what the kernels' gLN fold is handed."""
    v = t64(x).reshape(x.shape[0], -1)
    return torch.stack([v.sum(1), (v * v).sum(1)], 1)


def audio_bn(ar, x, gamma, beta, w, b):
    """gLN (per sample over channels and pixels) -> ReLU -> 1x1 conv.  -> ((y,), (scale,))"""
    st = stats(x)
    n = x.shape[1] * x.shape[2]
    mean = st[:, 0] / n
    var = (st[:, 1] / n - mean * mean).clamp_min(0)
    sc = t64(gamma)[None, :] * ar.rstd(var)[:, None]                       # (B, C)
    sh = t64(beta)[None, :] - mean[:, None] * (sc if ar is EXACT else sc.float().double())
    v = torch.relu(ar.t(x) * ar.t(sc)[:, :, None] + ar.t(sh)[:, :, None])
    y = ar.mm(w, v) + col(b, ar)
    return (y,), (absmm(w, v) + col(b, EXACT).abs(),)


def caf_fold(bn, w):
    """dw 1x1 . eval BatchNorm as one multiply-add: bn = (4, C) [weight | bias | running_mean | running_var]"""
    bn, w = t64(bn), t64(w)
    s = bn[0] / torch.sqrt(bn[3] + EPS)
    return w * s, bn[1] - bn[2] * s


def caf_apply(ar, v, sv, caf):
    """out = ReLU(key(v)) * r[tv] + att[tv] * value(v), tv = nearest_src(t, Tv, T), t = p // F.  caf: dict r, att (B, C, Tv), w_key, bn_key,
    w_val, bn_val, T, F."""
    P = v.shape[2]
    Tv = caf["r"].shape[2]
    tv = torch.as_tensor(nearest_index(Tv, caf["T"]))[torch.arange(P) // caf["F"]]
    r, att = ar.t(caf["r"])[:, :, tv], ar.t(caf["att"])[:, :, tv]
    ks, kb = caf_fold(caf["bn_key"], caf["w_key"])
    vs, vb = caf_fold(caf["bn_val"], caf["w_val"])
    out = torch.relu(v * col(ks, ar) + col(kb, ar)) * r + att * (v * col(vs, ar) + col(vb, ar))
    so = (sv * col(ks, EXACT).abs() + col(kb, EXACT).abs()) * t64(r).abs() + t64(att).abs() * (sv * col(vs, EXACT).abs() + col(vb, EXACT).abs())
    return out, so


def gateway(ar, v, sv, gw, gb, slope):
    y = prelu(v * col(gw, ar) + col(gb, ar), float(slope))
    return y, (sv * col(gw, EXACT).abs() + col(gb, EXACT).abs()) * max(1.0, abs(float(slope)))


def gateway_proj(ar, x, x2, gw, gb, slope, wp, bp, caf=None):
    """residual = PReLU(dw1x1(CAF(x) + x2)), x_enc = proj(residual).  -> ((residual, x_enc), scales)"""
    v, sv = ar.t(x), t64(x).abs()
    if caf is not None:
        v, sv = caf_apply(ar, v, sv, caf)
    if x2 is not None:
        v, sv = v + ar.t(x2), sv + t64(x2).abs()
    r, sr = gateway(ar, v, sv, gw, gb, slope)
    y = ar.mm(wp, r) + col(bp, ar)
    return (r, y), (sr, absmm(wp, r) + col(bp, EXACT).abs())


def residual(ar, x, w, b, res):
    """out = residual_conv(x) + res"""
    y = ar.mm(w, x) + col(b, ar) + ar.t(res)
    return (y,), (absmm(w, x) + col(b, EXACT).abs() + t64(res).abs(),)


def boundary(ar, x, res, a1, w1, b1, gw, gb, slope, wp, bp, caf=None):
    """out_i = residual_conv(x) + residual_i; block input = [CAF](out_i) + a1; residual_{i+1} = PReLU(dw1x1(input)); x_enc = proj(residual_{i+1}).
    `res` is the logical residual_i (without a1), the returned residual the logical residual_{i+1}: what a kernel keeps in its buffer under
    an a1_mode is the caller's bookkeeping (tests/test_hip_pw_edges.py).  -> ((residual, x_enc), scales)"""
    (out,), (so,) = residual(ar, x, w1, b1, res)
    if caf is not None:
        out, so = caf_apply(ar, out, so, caf)
    v, sv = out + ar.t(a1), so + t64(a1).abs()
    r, sr = gateway(ar, v, sv, gw, gb, slope)
    y = ar.mm(wp, r) + col(bp, ar)
    return (r, y), (sr, absmm(wp, r) + col(bp, EXACT).abs())


def s3(ar, x, slope, w, b, a0):
    """mask = ReLU(conv(PReLU(x))); separated = a0 * mask as complex numbers, channel c real and c + C/2 imaginary."""
    v = prelu(ar.t(x), float(slope))
    m = torch.relu(ar.mm(w, v) + col(b, ar))
    sm = absmm(w, v) + col(b, EXACT).abs()
    h = m.shape[1] // 2
    e = ar.t(a0)
    er, ei, mr, mi = e[:, :h], e[:, h:], m[:, :h], m[:, h:]
    out = torch.cat([er * mr - ei * mi, er * mi + ei * mr], 1)
    ea = t64(a0).abs()
    so = torch.cat([ea[:, :h] * sm[:, :h] + ea[:, h:] * sm[:, h:], ea[:, :h] * sm[:, h:] + ea[:, h:] * sm[:, :h]], 1)
    return (out,), (so,)


def taps(ar, sep, wt, live):
    """z[tap] = sum_c wt[tap, c] sep[c] for the first `live` rows of the (32, C) tap maps (no bias)."""
    return (ar.mm(t64(wt)[:live], sep),), (absmm(t64(wt)[:live], sep),)


def s3_taps(ar, x, slope, w, b, a0, wt, live):
    (sep,), _ = s3(ar, x, slope, w, b, a0)
    return taps(ar, sep, wt, live)


def rms_pow2(a0_stats, inv_count):
    """The power of two the fused kernels bring rms(a0) near 1 with (pipe_helpers.h rms_pow2): 2^-(floor(log2(mean square)) >> 1), per mixture."""
    ms = (np.asarray(a0_stats, np.float64)[:, 1] * inv_count).astype(np.float32)
    eb = ((ms.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
    return 2.0 ** np.clip(-(eb >> 1), -40, 40)


def enc_a0(ar, spec, w, esc=None):
    """a0 = Conv2d(2 -> C, 3x3, 'same', no bias)(spec) (encoder.py:146-157) as a GEMM over the 18 taps of every pixel: spec (B, 2, T, F),
    w (C, 18) with tap = channel * 9 + kt * 3 + kf.  -> ((a0 (B, C, T F),), (scale,)).  esc (B,): the emulation splits the patches times this
    power of two, as the kernels that rebuild a0 do."""
    s = t64(spec)
    patches = torch.nn.functional.unfold(s, 3, padding=1)  # (B, 18, T F), rows in (channel, kt, kf) order
    if esc is None:
        return (ar.mm(w, patches),), (absmm(w, patches),)
    e = torch.as_tensor(np.asarray(esc, np.float64)).reshape(-1, 1, 1)
    return (ar.mm(w, patches * e) / ar.t(e),), (absmm(w, patches),)


def bn_head(ar, spec, wenc, gamma, beta, w, b, gw, gb, slope, wp, bp, esc=None):
    """The fused head: a0 rebuilt from the spectrogram -> bottleneck -> gateway -> projection.  -> ((a1, residual, x_enc), scales)"""
    (a0,), _ = enc_a0(ar, spec, wenc, esc)
    (a1,), (s1,) = audio_bn(ar, a0, gamma, beta, w, b)
    r, sr = gateway(ar, a1, s1, gw, gb, slope)  # (the residual's scale is that of a1, a GEMM output, carried through the gateway)
    y = ar.mm(wp, r) + col(bp, ar)
    return (a1, r, y), (s1, sr, absmm(wp, r) + col(bp, EXACT).abs())


def tail(ar, x, res, spec, wenc, w1, b1, slope, w, b, wt, live, mix=None, esc=None):
    """The fused tail: refined = residual_conv(x) + res; S3 mask and complex product with the a0 of the target's mixture (mix: target ->
    mixture, None = itself), rebuilt from the spectrogram; decoder taps.  -> ((z,), (scale,))"""
    (a0,), _ = enc_a0(ar, spec, wenc, esc)
    mix = torch.arange(a0.shape[0]) if mix is None else torch.as_tensor(np.asarray(mix, np.int64))
    e = torch.ones(a0.shape[0], 1, 1, dtype=torch.float64) if esc is None else torch.as_tensor(np.asarray(esc, np.float64)).reshape(-1, 1, 1)
    (out,), _ = residual(ar, x, w1, b1, res)
    # (the taps GEMM splits the separated spectrum of the NORMALISED a0; the power of two is taken out of the result)
    (z,), (sz,) = s3_taps(ar, out, slope, w, b, (a0 * ar.t(e))[mix], wt, live)
    return (z / ar.t(e)[mix],), (sz / e[mix],)


def err(got, ref, scale):
    """max over elements of |got - ref| / scale (scale-free; 0 / 0 where nothing contributes counts as 0)."""
    d = (t64(got) - t64(ref)).abs()
    s = t64(scale)
    return float(torch.where(s > 0, d / s.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), d)).max())
