"""Float64 numpy restatements of the three preparation steps the device path replaces (rtfs-net_amd/datas.py, csrc/k_prep.hip):

* ``lips_prepare``     the reference's mouth-ROI pipeline (src/datas/transform.py:151-167): Normalize(0, 255), crop to 88 x 88, optional
                       horizontal flip, Normalize(0.421, 0.165), on uint8 ROIs, per track;
* ``normalize_mixture``  avspeech_dataset.py:18-22 with 145-148 / 206-209: zero mean per row, everything divided by the MIXTURE's unbiased
                       standard deviation (+ eps);
* ``resample``         torchaudio.transforms.Resample with its defaults (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), from
                       the published formulas: torchaudio is not a dependency, so the specification written out here is the contract.

Nothing here imports the package or touches a device."""
import math
import random as _random
import warnings

import numpy as np

CROP = 88
MEAN, STD = 0.421, 0.165
MAX_RATIO = 640


# ---------------------------------------------------------------- lips
def center_offsets(H, W, size=(CROP, CROP)):
    """CenterCrop's offsets, with the reference's rounding: int(round(w - tw) / 2.0) truncates an odd difference."""
    th, tw = size
    return int(round((H - th)) / 2.0), int(round((W - tw)) / 2.0)


def draw_offsets(H, W, flip_ratio=0.5, rng=None, size=(CROP, CROP)):
    """One track's train-time draws in the reference's order: dx, then dy, then the flip.  Returns (dy, dx, flip)."""
    r = _random if rng is None else rng
    th, tw = size
    dx = r.randint(0, W - tw)
    dy = r.randint(0, H - th)
    flip = 1 if r.random() < flip_ratio else 0
    return dy, dx, flip


def lips_prepare(roi, table, mean=MEAN, std=STD):
    """roi uint8 (N,Tv,H,W), table (N,3) of dy, dx, flip -> float32 (N,1,Tv,88,88), the arithmetic in float64 in the reference's order."""
    roi = np.asarray(roi)
    assert roi.dtype == np.uint8 and roi.ndim == 4
    N, Tv, H, W = roi.shape
    out = np.empty((N, 1, Tv, CROP, CROP), np.float32)
    for n in range(N):
        dy, dx, flip = (int(v) for v in table[n])
        if dy < 0 or dx < 0 or dy + CROP > H or dx + CROP > W:
            raise ValueError(f"track {n}: offsets ({dy}, {dx}) leave the {H} x {W} ROI")
        f = (roi[n] - 0.0) / 255.0
        f = f[:, dy:dy + CROP, dx:dx + CROP]
        if flip:
            f = f[:, :, ::-1]
        out[n, 0] = ((f - mean) / std).astype(np.float32)
    return out


# ---------------------------------------------------------------- waveform normalisation
def normalize_mixture(mix, src=None, eps=1e-8):
    """mix (B,L), src (B,K,L) or None -> (mix_out, src_out) in float64.  L = 1 gives NaN (0 / 0), as torch.std."""
    mix = np.asarray(mix, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sd = mix.std(-1, ddof=1, keepdims=True)
        mo = (mix - mix.mean(-1, keepdims=True)) / (sd + eps)
        so = None
        if src is not None:
            src = np.asarray(src, np.float64)
            so = (src - src.mean(-1, keepdims=True)) / (sd[:, None, :] + eps)
    return mo, so


def normalize_tensor_wav(wav, eps=1e-8, std=None):
    wav = np.asarray(wav, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if std is None:
            std = wav.std(-1, ddof=1, keepdims=True)
        return (wav - wav.mean(-1, keepdims=True)) / (np.asarray(std, np.float64) + eps)


# ---------------------------------------------------------------- resampling
def resample_plan(orig, new):
    """-> o, n, width, taps for the reduced ratio; ValueError past 640."""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1:
        raise ValueError("sample rates must be positive")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    if o > MAX_RATIO or n > MAX_RATIO:
        raise ValueError(f"resample {orig} -> {new}: reduced ratio {o}:{n} is past {MAX_RATIO}")
    base = min(o, n) * 0.99
    width = int(math.ceil(6 * o / base))
    return o, n, width, 2 * width + o


def resample_bank(orig, new, dtype=np.float32):
    """The (n, taps) kernel bank: computed in float64, returned as `dtype`."""
    o, n, width, taps = resample_plan(orig, new)
    base = min(o, n) * 0.99
    p = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(taps, dtype=np.float64)[None, :]
    t = (-p / n + (k - width) / o) * base
    t = np.clip(t, -6.0, 6.0)
    win = np.cos(t * math.pi / 6.0 / 2.0) ** 2
    tp = t * math.pi
    scale = base / o
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(tp == 0.0, 1.0, np.sin(tp) / tp)
    return (sinc * (win * scale)).astype(dtype)


def resample_out_len(orig, new, L):
    o, n, _, _ = resample_plan(orig, new)
    return -(-n * int(L) // o)


def resample(x, orig, new, bank=None):
    """x (L) | (B,L) -> float64 (..., ceil(n L / o)): y[j n + p] = sum_k bank[p,k] xpad[j o + k] with the float32 bank's values, xpad = x with
    `width` zeros in front and `width + o` behind.  Equal rates return the input."""
    if int(orig) == int(new):
        return x
    o, n, width, taps = resample_plan(orig, new)
    bank = np.asarray(resample_bank(orig, new) if bank is None else bank, np.float64)
    x = np.asarray(x, np.float64)
    single = x.ndim == 1
    x = x.reshape(-1, x.shape[-1])
    B, L = x.shape
    Lout = -(-n * L // o)
    J = L // o + 1  # frames of the strided convolution over the padded recording
    xp = np.zeros((B, width + L + width + o))
    xp[:, width:width + L] = x
    y = np.empty((B, J, n))
    bt = np.ascontiguousarray(bank.T)  # (taps, n)
    step = max(1, (1 << 22) // taps)   # frames per product: y[:, j, :] = xpad[:, j o : j o + taps] @ bank^T
    for b in range(B):
        fr = np.lib.stride_tricks.as_strided(xp[b], shape=(J, taps), strides=(o * xp.strides[1], xp.strides[1]), writeable=False)
        for j0 in range(0, J, step):
            y[b, j0:j0 + step] = fr[j0:j0 + step] @ bt
    y = y.reshape(B, J * n)[:, :Lout]
    assert y.shape[1] == Lout
    return y[0] if single else y
