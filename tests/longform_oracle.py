"""Numpy restatement (float64) of the long-form windowing behind AVNet.separate_long: plan, frame, weights and overlap_add, straight
from the formulas of DESIGN.md "Long recordings".  Nothing here imports the package under test.

SPF = 640 samples per video frame (16 kHz audio, 25 fps video).  A recording of L samples is cut into N windows of ``window`` samples
every ``hop`` samples; window n covers samples [n hop, n hop + window) (zeros past L) and video frames [n hop / SPF, n hop / SPF +
window / SPF) (a frame index past Tv - 1 reads frame Tv - 1).  The windows are cross-faded back with linear ramps over the overlap
V = window - hop and divided by the sum of the weights that reach a sample, so first / last half windows and any hop are exact
partitions of unity."""
import numpy as np

SPF = 640


def plan(L, Tv, window, hop=None):
    """Number of windows N; ValueError for a plan the formulas do not cover."""
    hop = window // 2 if hop is None else hop
    if L < 1 or Tv < 1:
        raise ValueError(f"L = {L}, Tv = {Tv}")
    if window <= 0 or window % SPF or hop % SPF or not 0 < hop <= window:
        raise ValueError(f"window = {window}, hop = {hop}: multiples of {SPF} with 0 < hop <= window")
    return 1 if L <= window else 1 + -(-(L - window) // hop)


def frame(x, v, window, hop=None):
    """x (B, L), v (B, 512, Tv) -> (B * N, window), (B * N, 512, window / SPF); row b * N + n.  Copies: the dtype is kept."""
    hop = window // 2 if hop is None else hop
    x, v = np.asarray(x), np.asarray(v)
    (B, L), Tv = x.shape, v.shape[-1]
    N = plan(L, Tv, window, hop)
    xw = np.zeros((B, N, window), x.dtype)
    vw = np.zeros((B, N, v.shape[1], window // SPF), v.dtype)
    for n in range(N):
        lo = n * hop
        seg = x[:, lo:min(L, lo + window)]
        xw[:, n, :seg.shape[1]] = seg
        idx = np.minimum(lo // SPF + np.arange(window // SPF), Tv - 1)
        vw[:, n] = v[:, :, idx]
    return xw.reshape(B * N, window), vw.reshape(B * N, v.shape[1], window // SPF)


def weights(window, hop=None):
    """w[i] = 1 if window == hop, else min(1, (i + 0.5) / V, (window - i - 0.5) / V), V = window - hop: strictly positive."""
    hop = window // 2 if hop is None else hop
    V = window - hop
    i = np.arange(window, dtype=np.float64)
    if V == 0:
        return np.ones(window)
    return np.minimum(1.0, np.minimum((i + 0.5) / V, (window - i - 0.5) / V))


def overlap_add(y, B, L, window, hop=None):
    """y (B * N, n_src, window) -> (B, n_src, L) float64: sum_n w[t - n hop] y_n[t - n hop] / sum_n w[t - n hop] over the windows holding t."""
    hop = window // 2 if hop is None else hop
    y = np.asarray(y, np.float64)
    N = plan(L, 1, window, hop)
    n_src = y.shape[1]
    assert y.shape == (B * N, n_src, window), (y.shape, B, N)
    y = y.reshape(B, N, n_src, window)
    w = weights(window, hop)
    num = np.zeros((B, n_src, (N - 1) * hop + window))
    den = np.zeros((N - 1) * hop + window)
    for n in range(N):  # ascending n, as the kernel sums
        num[:, :, n * hop:n * hop + window] += w * y[:, n]
        den[n * hop:n * hop + window] += w
    return num[:, :, :L] / den[:L]
