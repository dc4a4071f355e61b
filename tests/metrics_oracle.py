"""Float64 numpy / scipy restatement of classic STOI (Taal et al. 2011) as pystoi 0.4.1 computes it -- the metric the reference's
``src/metrics/allwrapper.py`` calls as ``stoi(clean, estimate, 16000, extended=False)`` (pystoi pinned at 0.4.1 in the reference's
``setup/requirements.yaml``) -- plus the composition of ``ALLMetricsTracker``'s per-mixture values.

pystoi itself is not installed where this project is developed, so there is NO golden from the reference's own metric: this file
restates pystoi's published source function by function (the citations below name pystoi's functions and their line structure) and
the device kernel (``csrc/k_stoi.hip``) is tested against it.  Parity with pystoi is therefore unpinned.  Conventions
followed where a batch-vectorised release could differ from the classic per-signal code:
  - frames of ``remove_silent_frames`` and ``stft`` start at ``range(0, len(x) - framelen, hop)``: the last full frame is excluded;
  - silence is decided on the clean signal's windowed-frame energies ``20 log10(|frame| + eps)``, eps = float64 eps;
  - the kept frames of both signals are overlap-added (``_overlap_and_add``) to length ``(K - 1) hop + framelen``;
  - fewer than N = 30 STFT frames returns 1e-5.
"""
from __future__ import annotations

import numpy as np
import scipy.signal

FS = 10000       # stoi.py: FS, the rate everything is resampled to
N_FRAME = 256    # window length
NFFT = 512       # FFT size
NUMBAND = 15     # one-third-octave bands
MINFREQ = 150    # centre of the lowest band
N = 30           # frames per intermediate-intelligibility segment
BETA = -15.0     # lower SDR bound of the clipping
DYN_RANGE = 40   # silence threshold below the loudest frame, dB
EPS = np.finfo("float").eps


def thirdoct(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """pystoi utils.thirdoct: band matrix (num_bands, nfft/2 + 1) and centre frequencies.  Edges snap to the nearest bin by argmin and a
    band covers [lo, hi)."""
    f = np.linspace(0, fs, nfft + 1)
    f = f[:int(nfft / 2) + 1]
    k = np.array(range(num_bands)).astype(float)
    cf = np.power(2. ** (1. / 3), k) * min_freq
    freq_low = min_freq * np.power(2., (2 * k - 1) / 6)
    freq_high = min_freq * np.power(2., (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    for i in range(len(cf)):
        f_bin = np.argmin(np.square(f - freq_low[i]))
        freq_low[i] = f[f_bin]
        fl_ii = f_bin
        f_bin = np.argmin(np.square(f - freq_high[i]))
        freq_high[i] = f[f_bin]
        fh_ii = f_bin
        obm[i, fl_ii:fh_ii] = 1
    return obm, cf


OBM, CF = thirdoct()


def band_edges():
    """[(lo, hi)] bin ranges of OBM's rows."""
    out = []
    for row in OBM:
        nz = np.nonzero(row)[0]
        out.append((int(nz[0]), int(nz[-1]) + 1))
    return out


def resample_window_oct(p, q):
    """pystoi utils._resample_window_oct: Octave's resample() filter -- ideal sinc times a Kaiser window, 60 dB rejection."""
    log10_rejection = -3.0
    stopband_cutoff_f = 1. / (2 * max(p, q))
    roll_off_width = stopband_cutoff_f / 10
    rejection_dB = -20 * log10_rejection
    L = np.ceil((rejection_dB - 8) / (28.714 * roll_off_width))
    t = np.arange(-L, L + 1)
    ideal_filter = 2 * p * stopband_cutoff_f * np.sinc(2 * stopband_cutoff_f * t)
    if (rejection_dB >= 21) and (rejection_dB <= 50):
        beta = 0.5842 * (rejection_dB - 21) ** 0.4 + 0.07886 * (rejection_dB - 21)
    elif rejection_dB > 50:
        beta = 0.1102 * (rejection_dB - 8.7)
    else:
        beta = 0.0
    h = np.kaiser(2 * L + 1, beta) * ideal_filter
    return h


def resample_oct(x, p, q):
    """pystoi utils.resample_oct: scipy.signal.resample_poly with the normalised Octave window (resample_poly multiplies it by up)."""
    g = np.gcd(p, q)
    p, q = p // g, q // g
    h = resample_window_oct(p, q)
    window = h / np.sum(h)
    return scipy.signal.resample_poly(x, p, q, window=window)


def frames(x, framelen=N_FRAME, hop=N_FRAME // 2):
    w = np.hanning(framelen + 2)[1:-1]
    return np.array([w * x[i:i + framelen] for i in range(0, len(x) - framelen, hop)]).reshape(-1, framelen)


def frame_energies(x, framelen=N_FRAME, hop=N_FRAME // 2):
    return 20 * np.log10(np.linalg.norm(frames(x, framelen, hop), axis=1) + EPS)


def overlap_and_add(x_frames, hop):
    """pystoi utils._overlap_and_add (the reshaping form is plain overlap-add): length (K - 1) hop + framelen."""
    num_frames, framelen = x_frames.shape
    out = np.zeros((num_frames - 1) * hop + framelen)
    for k in range(num_frames):
        out[k * hop:k * hop + framelen] += x_frames[k]
    return out


def remove_silent_frames(x, y, dyn_range=DYN_RANGE, framelen=N_FRAME, hop=N_FRAME // 2):
    """pystoi utils.remove_silent_frames: windowed frames, clean energies, mask (max - dyn_range - e) < 0, overlap-add both.
    Returns (x_sil, y_sil, mask)."""
    x_frames, y_frames = frames(x, framelen, hop), frames(y, framelen, hop)
    x_energies = 20 * np.log10(np.linalg.norm(x_frames, axis=1) + EPS)
    mask = (np.max(x_energies) - dyn_range - x_energies) < 0
    return overlap_and_add(x_frames[mask], hop), overlap_and_add(y_frames[mask], hop), mask


def stft(x, win_size=N_FRAME, fft_size=NFFT, overlap=2):
    """pystoi utils.stft: (frames, fft_size/2 + 1), frames at range(0, len(x) - win_size, hop)."""
    hop = int(win_size / overlap)
    w = np.hanning(win_size + 2)[1:-1]
    return np.array([np.fft.rfft(w * x[i:i + win_size], n=fft_size) for i in range(0, len(x) - win_size, hop)]).reshape(-1, fft_size // 2 + 1)


def prepare(x, y, fs_sig):
    """stoi() up to the band values: resample, silence removal, STFT, OBM.  -> (x_tob, y_tob (15, F'), kept frame count)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if fs_sig != FS:
        x = resample_oct(x, FS, fs_sig)
        y = resample_oct(y, FS, fs_sig)
    x, y, mask = remove_silent_frames(x, y, DYN_RANGE, N_FRAME, int(N_FRAME / 2))
    x_spec = stft(x, N_FRAME, NFFT, overlap=2).transpose()
    y_spec = stft(y, N_FRAME, NFFT, overlap=2).transpose()
    x_tob = np.sqrt(np.matmul(OBM, np.square(np.abs(x_spec))))
    y_tob = np.sqrt(np.matmul(OBM, np.square(np.abs(y_spec))))
    return x_tob, y_tob, int(mask.sum())


def stoi(x, y, fs_sig, extended=False):
    """pystoi stoi.stoi (classic branch): x clean, y processed, 1-D."""
    if extended:
        raise ValueError("extended STOI is not restated here")
    if np.shape(x) != np.shape(y):
        raise Exception("x and y should have the same length")
    x_tob, y_tob, _ = prepare(x, y, fs_sig)
    if x_tob.shape[-1] < N:
        return 1e-5
    x_segments = np.array([x_tob[:, m - N:m] for m in range(N, x_tob.shape[1] + 1)])
    y_segments = np.array([y_tob[:, m - N:m] for m in range(N, x_tob.shape[1] + 1)])
    normalization_consts = np.linalg.norm(x_segments, axis=2, keepdims=True) / (np.linalg.norm(y_segments, axis=2, keepdims=True) + EPS)
    y_segments_normalized = y_segments * normalization_consts
    clip_value = 10 ** (-BETA / 20)
    y_primes = np.minimum(y_segments_normalized, x_segments * (1 + clip_value))
    y_primes = y_primes - np.mean(y_primes, axis=2, keepdims=True)
    x_segments = x_segments - np.mean(x_segments, axis=2, keepdims=True)
    y_primes /= (np.linalg.norm(y_primes, axis=2, keepdims=True) + EPS)
    x_segments /= (np.linalg.norm(x_segments, axis=2, keepdims=True) + EPS)
    correlations_components = y_primes * x_segments
    J = x_segments.shape[0]
    M = x_segments.shape[1]
    return float(np.sum(correlations_components) / (J * M))


def kept_frames(x, fs_sig):
    """Frames silence removal keeps for clean x, and the smallest |distance| in dB of any frame from the 40 dB threshold."""
    x = np.asarray(x, np.float64)
    if fs_sig != FS:
        x = resample_oct(x, FS, fs_sig)
    e = frame_energies(x)
    margin = e.max() - DYN_RANGE - e
    return int((margin < 0).sum()), float(np.abs(margin).min())


def speech_like(rng, L, fs, gaps=(), zero_gaps=(), level=1.0):
    """Amplitude-modulated noise with silent gaps: ``gaps`` = [(start_s, end_s)] at -60 dB, ``zero_gaps`` at exact zero."""
    t = np.arange(L) / fs
    env = 0.5 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6)) * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6))
    x = level * env * rng.standard_normal(L)
    for a, b in gaps:
        x[int(a * fs):int(b * fs)] *= 1e-3
    for a, b in zero_gaps:
        x[int(a * fs):int(b * fs)] = 0.0
    return x.astype(np.float32)


# ---------------------------------------------------------------- ALLMetricsTracker composition (allwrapper.py:35-83)
def neg_pit(est, tgt, kind):
    """PITLossWrapper(pairwise_neg_{snr,sisdr}, pit_from="pw_mtx") on one mixture (n_src, L) -> the loss, float64."""
    from oracle.loss_oracle import pairwise_neg_sdr, pit_from_pw_mtx
    pw = pairwise_neg_sdr(est[None], tgt[None], kind)
    return float(pit_from_pw_mtx(pw)[1][0])


def tracker_values(mix, clean, est, fs=16000):
    """One mixture's (sisnr, sisnr_i, sdr, sdr_i, stoi) as ALLMetricsTracker.__call__ composes them, in the loss sign:
    mix (L,), clean / est (n_src, L).  stoi scores source 0 (allwrapper.py squeezes a single source)."""
    mixs = np.stack([mix] * clean.shape[0], 0)
    sisnr, sisnr_b = neg_pit(est, clean, "sisdr"), neg_pit(mixs, clean, "sisdr")
    sdr, sdr_b = neg_pit(est, clean, "snr"), neg_pit(mixs, clean, "snr")
    return sisnr, sisnr - sisnr_b, sdr, sdr - sdr_b, stoi(clean[0], est[0], fs)
