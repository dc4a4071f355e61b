"""Float64 numpy restatement of extended STOI (ESTOI, Jensen & Taal 2016) as pystoi 0.4.1's ``stoi(x, y, fs_sig, extended=True)``
computes it, on top of ``tests/metrics_oracle.prepare`` (resampling, silence removal, one-third-octave band values: the part classic and
extended STOI share).  The device kernels (``csrc/k_stoi.hip``: ``estoi_corr_chunk``) are tested against this file.

With band values ``x_tob``, ``y_tob`` of shape (15, F): 1e-5 when F < 30; otherwise the J = F - 29 segments of shape (15, 30), one per
m = 30 .. F, each go through ``row_col_normalize`` -- per band minus the mean over the 30 frames and divided by the Euclidean norm, then
per frame minus the mean over the 15 bands and divided by the norm -- and d = sum(x_n * y_n) / 30 / J.

Two deliberate differences from pystoi:
  - Noise.  pystoi adds ``eps * standard_normal`` before each of the two normalisations.  It is left out here and on the device, so
    the result is deterministic; ``estoi(..., noise=rng)`` puts the two terms back, and tests/test_estoi_host.py checks on the GPU
    tests' signals that they move d by less than 1e-12.
  - Zero norms.  A norm of exactly zero gives the inverse 0 (``inv = n > 0 ? 1 / n : 0``): a silent estimate and an all-zero clean
    signal score exactly 0.0 and nothing is ever NaN.  pystoi's answer in these cases is whatever its noise happens to be.

pystoi itself is not installed where this project is developed: agreement with the package is NOT MEASURED.  This file is the
published definition, restated from pystoi's source (stoi.py's extended branch, utils.row_col_normalize).
"""
from __future__ import annotations

import numpy as np

from tests import metrics_oracle as M

N = M.N  # 30 frames per segment


def _inv_norm(v, axis):
    n = np.sqrt(np.sum(np.square(v), axis=axis, keepdims=True))
    return np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)


def row_col_normalize(x, noise=None):
    """pystoi utils.row_col_normalize on (J, 15, 30) segments.  ``noise``: a numpy Generator -> pystoi's two eps * standard_normal terms."""
    x = np.array(x, np.float64)
    if noise is not None:
        x = x + M.EPS * noise.standard_normal(x.shape)
    x = x - np.mean(x, axis=-1, keepdims=True)   # rows: each band over the 30 frames
    x = x * _inv_norm(x, -1)
    if noise is not None:
        x = x + M.EPS * noise.standard_normal(x.shape)
    x = x - np.mean(x, axis=1, keepdims=True)    # columns: each frame over the 15 bands
    x = x * _inv_norm(x, 1)
    return x


def segments(tob):
    """(15, F) -> (J, 15, 30), one segment per m = 30 .. F."""
    return np.array([tob[:, m - N:m] for m in range(N, tob.shape[1] + 1)])


def estoi_from_bands(x_tob, y_tob, noise=None):
    if x_tob.shape[-1] < N:
        return 1e-5
    x_n = row_col_normalize(segments(x_tob), noise)
    y_n = row_col_normalize(segments(y_tob), noise)
    return float(np.sum(x_n * y_n / N) / x_n.shape[0])


def estoi(x, y, fs_sig, noise=None):
    """pystoi stoi.stoi(x, y, fs_sig, extended=True): x clean, y processed, 1-D."""
    if np.shape(x) != np.shape(y):
        raise Exception("x and y should have the same length")
    x_tob, y_tob, _ = M.prepare(x, y, fs_sig)
    return estoi_from_bands(x_tob, y_tob, noise)


def n_segments(x, fs_sig):
    """J for clean x: STFT frames of the silence-removed signal minus 29 (0 below 30 frames)."""
    x_tob, _, _ = M.prepare(x, x, fs_sig)
    return max(0, x_tob.shape[-1] - (N - 1))


# ---------------------------------------------------------------- the device stage's work cut (csrc/k_stoi.hip: estoi_corr_chunk)
def planned_chunks(J):
    """Chunks the planner gives a recording with J segments: the classic correlation work list, ceil(15 J / 256)."""
    return -(-15 * J // 256) if J > 0 else 0


def chunk_owner(s):
    """The chunk that owns segment s."""
    return 15 * s // 256


def tracker_values(mix, clean, est, fs=16000):
    """metrics_oracle.tracker_values with extended STOI appended: (sisnr, sisnr_i, sdr, sdr_i, stoi, estoi)."""
    return M.tracker_values(mix, clean, est, fs) + (estoi(clean[0], est[0], fs),)


# ---------------------------------------------------------------- signals shared by tests/test_estoi_host.py and tests/test_hip_estoi.py
# (L at fs = 10000, J): stationary Gaussian noise keeps every frame, so J = ceil((L - 256) / 128) - 30.  The lengths sit where the work cut
# changes: no segment / one; 17 / 18 segments (the second planned chunk of J = 18 owns none) / 19; 35 (the third owns none) / 36; 256 / 257.
SEGMENT_LENGTHS = ((4096, 0), (4097, 1), (6272, 17), (6273, 18), (6401, 19), (8449, 35), (8577, 36), (36737, 256), (36865, 257))


def noise_pair(L, seed):
    """(clean, estimate) float32 (L,): stationary Gaussian noise and a noisy copy of it."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(L)
    y = x + 0.5 * rng.standard_normal(L)
    return x.astype(np.float32), y.astype(np.float32)
