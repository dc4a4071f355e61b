"""Float64 oracle of BSS-eval SDR (include/rtfs_amd.h, "BSS-eval SDR"): the SDR column of mir_eval.separation.bss_eval_sources
with fast_bss_eval's permutation rule, written from the published definition in numpy / scipy.  mir_eval itself is not installed where
this project is developed, so agreement with the package is not measured.

``sdr_lu`` is the definition: direct correlations, a dense solve of the 512 x 512 Toeplitz system, the explicit convolution
s_target = s * c of length L + 511 and the time-domain energies |s_target|^2 / |e_pad - s_target|^2.  ``sdr_moments`` is the cheap route the
device takes: Levinson (scipy.linalg.solve_toeplitz) and the closed forms num = c'd, den = max(ee - num, 0).  tests/test_bss_host.py holds
the two together over every case set below."""
import functools
import itertools

import numpy as np
import scipy.linalg
import scipy.signal

F = 512          # filter length, mir_eval's default
CHUNK = 4096     # samples per correlation partial of the device stage
LENGTH_EDGES = (1, 2, 511, 512, 513, 4095, 4096, 4097, 8193, 32003)
COND_L = 8193
SOURCES_L = 4097
REFERENCES = ("white", "ar1_0.9", "ar1_0.99", "ar2_res", "butter4_3k")
NOISES = (("interf", 0.5), ("interf", 0.01), ("white", 1e-3))  # (kind, level relative to the reference's norm)


# ---------------------------------------------------------------- the definition
def correlations(s, e):
    """r[k] = sum_t s[t] s[t+k], d[k] = sum_t s[t] e[t+k], k = 0 .. 511, and ee = sum e^2, in float64; terms past the end are absent."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    L = len(s)
    r, d = np.zeros(F), np.zeros(F)
    for k in range(min(F, L)):
        r[k] = np.dot(s[:L - k], s[k:])
        d[k] = np.dot(s[:L - k], e[k:])
    return r, d, float(np.dot(e, e))


def _db(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.float64(num) / np.float64(den)))


def sdr_lu(s, e):
    """The definition: LU solve (least squares when the matrix is singular), explicit convolution, time-domain energies."""
    r, d, _ = correlations(s, e)
    G = scipy.linalg.toeplitz(r)
    try:
        c = np.linalg.solve(G, d)
        if not np.isfinite(c).all():
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        c = np.linalg.lstsq(G, d, rcond=None)[0]
    target = np.convolve(np.asarray(s, np.float64), c)           # L + 511 samples
    e_pad = np.zeros(len(target))
    e_pad[:len(e)] = e
    return _db(np.dot(target, target), np.dot(e_pad - target, e_pad - target))


def sdr_moments(s, e):
    """Levinson plus the closed forms: num = c'd, den = max(ee - num, 0).  A silent reference has c = 0."""
    r, d, ee = correlations(s, e)
    c = scipy.linalg.solve_toeplitz(r, d) if r[0] > 0 else np.zeros(F)
    num = float(np.dot(c, d))
    return _db(num, max(ee - num, 0.0))


def snr(s, e):
    """What the reference's tracker calls sdr: plain SNR, no projection."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    return _db(np.dot(s, s), np.dot(e - s, e - s))


# ---------------------------------------------------------------- sources
def best_perm(M):
    """M[i][j] = SDR(estimate i, clean j) -> perm with perm[j] = the estimate assigned to clean j: the largest mean over the sources,
    permutations in itertools order, first maximum."""
    n = len(M)
    best, bm = None, None
    for p in itertools.permutations(range(n)):
        s = np.float64(0.0)
        with np.errstate(invalid="ignore"):
            for j in range(n):
                s = s + np.float64(M[p[j]][j])
            s = s / np.float64(n)
        if best is None or s > bm:
            best, bm = p, s
    return list(best)


def bss_eval(clean, est, mix=None, fn=sdr_lu):
    """clean, est (n, L), mix (L) | None -> (sdr (n), sdr_i (n) | None, perm (n)) in float64"""
    n = len(clean)
    M = [[fn(clean[j], est[i]) for j in range(n)] for i in range(n)]
    perm = best_perm(M)
    sdr = np.array([M[perm[j]][j] for j in range(n)])
    if mix is None:
        return sdr, None, perm
    with np.errstate(invalid="ignore"):
        return sdr, sdr - np.array([fn(clean[j], mix) for j in range(n)]), perm


# ---------------------------------------------------------------- signals (float32, as the device reads them)
def coloured(rng, L, kind):
    w = rng.standard_normal(L + 2048)  # the filters' transients are cut off
    if kind == "white":
        x = w
    elif kind.startswith("ar1_"):
        x = scipy.signal.lfilter([1.0], [1.0, -float(kind[4:])], w)
    elif kind == "ar2_res":  # poles 0.9 exp(+-0.3i)
        x = scipy.signal.lfilter([1.0], [1.0, -2 * 0.9 * np.cos(0.3), 0.81], w)
    elif kind == "butter4_3k":
        b, a = scipy.signal.butter(4, 3000.0 / 8000.0)
        x = scipy.signal.lfilter(b, a, w)
    else:
        raise ValueError(kind)
    x = x[2048:]
    return (x / np.sqrt(np.mean(x * x))).astype(np.float32)


def noisy(rng, s, kind, level, ref_kind):
    """s + noise of `level` times the norm of s: an independent signal of the reference's own colouring ("interf") or white noise."""
    nz = coloured(rng, len(s), ref_kind if kind == "interf" else "white").astype(np.float64)
    nz *= level * np.linalg.norm(s) / max(np.linalg.norm(nz), 1e-300)
    return (s + nz).astype(np.float32)


@functools.lru_cache(maxsize=None)
def length_cases():
    """[(name, s, e)] with n = 1: white and AR(1) 0.9 references at every length edge, the estimate 10 dB above independent white noise.
    At L = 1 every estimate is a multiple of the reference (the fit is perfect), so that row belongs with the degenerate ones."""
    out = []
    for L in LENGTH_EDGES:
        for kind in ("white", "ar1_0.9"):
            rng = np.random.default_rng(1000 + L + (7 if kind == "white" else 0))
            s = coloured(rng, L, kind)
            out.append((f"{kind}_L{L}", s, noisy(rng, s, "white", 0.316, kind)))
    return out


@functools.lru_cache(maxsize=None)
def conditioning_cases():
    """[(name, s, e)] at L = 8193: five colourings (condition numbers 3 .. 7.7e9) x three noise settings (6, 40 and 60 dB)."""
    out = []
    for a, ref in enumerate(REFERENCES):
        for b, (kind, level) in enumerate(NOISES):
            rng = np.random.default_rng(2000 + 10 * a + b)
            s = coloured(rng, COND_L, ref)
            out.append((f"{ref}_{kind}_{level:g}", s, noisy(rng, s, kind, level, ref)))
    return out


@functools.lru_cache(maxsize=None)
def source_case(n, identical=False):
    """(clean (n,L), est (n,L), mix (L), shuffle) at L = 4097: source j coloured REFERENCES[j], estimate i = clean[shuffle[i]] + noise
    at 20 - 3 i dB; `identical`: estimate 1 is a copy of estimate 0.  The expected permutation is the inverse of `shuffle`."""
    rng = np.random.default_rng(3000 + n + (50 if identical else 0))
    clean = np.stack([coloured(rng, SOURCES_L, REFERENCES[j]) * np.float32(1.0 - 0.15 * j) for j in range(n)])
    shuffle = list(rng.permutation(n)) if n > 2 else [1, 0]
    if shuffle == sorted(shuffle):
        shuffle = shuffle[1:] + shuffle[:1]
    est = np.stack([noisy(rng, clean[shuffle[i]], "white", 10.0 ** (-(20 - 3 * i) / 20.0), "white") for i in range(n)])
    if identical:
        est[1] = est[0]
    mix = clean.sum(0).astype(np.float32)
    return clean, est, mix, [int(v) for v in shuffle]


def all_pairs():
    """(name, s, e) of every (reference, right-hand signal) pair the case sets above score."""
    yield from length_cases()
    yield from conditioning_cases()
    for n in (2, 3, 4):
        for identical in (False, True):
            clean, est, mix, _ = source_case(n, identical)
            for j in range(n):
                for i in range(n):
                    yield f"src{n}{'i' if identical else ''}_e{i}_s{j}", clean[j], est[i]
                yield f"src{n}{'i' if identical else ''}_mix_s{j}", clean[j], mix
