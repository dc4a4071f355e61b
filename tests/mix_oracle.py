"""Float64 numpy restatement of the training-mixture definition (include/rtfs_amd.h "Training mixtures"; rtfs-net_amd/datas.py mix_batch)
and of the reference's online-mixing collate formula with the permutations passed in.  Independent of the library: direct sums over the
samples with math.fsum (exactly rounded), the mixture's mean and deviation computed from m itself and not from moments, outputs rounded to
float32 last.

A recipe is the five (B, J) arrays of ``datas.MixRecipe``: src (-1: empty), start, a, ref_src (-1: none), ref_start.  ``sources`` are host
arrays, float32 or int16 (which enter as float32(s) / 32768).

* ``mix``              the definition from the samples alone -> mixture (B,L) f32, sources (B,n_out,L) f32, stats (B, J + 2) f64
* ``mix_given_stats``  the same output formulas with the gains / mean / inv it is handed (the device's own ``stats``): every remaining
                       operation is one IEEE float64 multiply, add or subtract in the documented order, so the device must agree bit
                       for bit.  The mean of a scaled source is g_j (sum x_j / L) with the exactly rounded sum; the device's float64
                       sum of float32 samples is that same number as long as the samples' exponents span fewer than 53 - log2(L) bits
                       (any audio-like data; the tests' inputs do).
* ``collate``          core.py:183-202 with explicit permutations, float64 throughout
* ``max_abs_corr``     the largest |Pearson correlation| between two scaled slots of a row (slots that name the same segment count as
                       one signal): moment-based variances lose about 1 / (1 - |corr|) in relative precision when slots cancel, so
                       the normalisation tests keep it <= 0.9.  Below a few dozen samples a correlation says nothing (two centred
                       2-sample vectors are always collinear); ``moment_bounds`` states the cost itself, at any length"""
import math

import numpy as np

J = 4


def segment(sources, idx, start, L):
    x = np.asarray(sources[idx])[start:start + L]
    assert x.shape == (L,), (idx, start, L, np.asarray(sources[idx]).shape)
    if x.dtype == np.int16:
        return (x.astype(np.float32) / np.float32(32768.0)).astype(np.float64)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


def fsum(v):
    v = np.asarray(v, np.float64)
    return math.fsum(v.tolist()) if np.isfinite(v).all() else float(np.sum(v))


def energy(x):
    return fsum(x * x)  # the square of a float32 value is exact in float64


def pad(recipe):
    src, start, a, ref_src, ref_start = (np.asarray(v) for v in recipe)
    B, Jr = src.shape
    out = [np.full((B, J), -1, np.int64), np.zeros((B, J), np.int64), np.zeros((B, J)), np.full((B, J), -1, np.int64), np.zeros((B, J), np.int64)]
    for o, v in zip(out, (src, start, a, ref_src, ref_start)):
        o[:, :Jr] = v
    return out


def gains(sources, recipe, L):
    src, start, a, ref_src, ref_start = pad(recipe)
    g = np.zeros(src.shape)
    with np.errstate(all="ignore"):
        for b in range(src.shape[0]):
            for j in range(J):
                if src[b, j] < 0:
                    continue
                g[b, j] = a[b, j]
                if ref_src[b, j] >= 0:
                    er = np.float64(energy(segment(sources, ref_src[b, j], ref_start[b, j], L)))
                    ex = np.float64(energy(segment(sources, src[b, j], start[b, j], L)))
                    g[b, j] = a[b, j] * np.sqrt(er / ex)
    return g


def scaled(sources, recipe, L, g, b):
    """The scaled slots g_j x_j of row b (None for an empty slot) and m, accumulated in the order j = 0, 1, ... from the first one."""
    src, start = pad(recipe)[:2]
    terms, m = [], None
    with np.errstate(all="ignore"):
        for j in range(J):
            if src[b, j] < 0:
                terms.append(None)
                continue
            t = np.float64(g[b, j]) * segment(sources, src[b, j], start[b, j], L)
            terms.append(t)
            m = t if m is None else m + t
    return terms, m


def _outputs(sources, recipe, L, n_out, normalize, g, mean_inv, source_mean):
    B = np.asarray(recipe[0]).shape[0]
    mixture, out = np.zeros((B, L), np.float32), np.zeros((B, n_out, L), np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            terms, m = scaled(sources, recipe, L, g, b)
            mean, inv = mean_inv(b, m)
            mixture[b] = ((m - mean) * inv if normalize else m).astype(np.float32)
            for j in range(n_out):
                t = np.zeros(L) if terms[j] is None else terms[j]
                out[b, j] = ((t - source_mean(b, j, t)) * inv if normalize else t).astype(np.float32)
    return mixture, out


def mix(sources, recipe, L, n_out, normalize=False, eps=1e-8):
    g = gains(sources, recipe, L)
    stats = np.zeros((g.shape[0], J + 2))
    stats[:, :J] = g

    def mean_inv(b, m):
        with np.errstate(all="ignore"):
            mean = np.float64(fsum(m)) / np.float64(L)
            sd = np.sqrt(np.float64(fsum((m - mean) ** 2)) / np.float64(L - 1))  # unbiased; L = 1: 0 / 0 = NaN
            stats[b, J], stats[b, J + 1] = mean, 1.0 / (sd + np.float64(eps))
        return stats[b, J], stats[b, J + 1]

    mixture, out = _outputs(sources, recipe, L, n_out, normalize, g, mean_inv, lambda b, j, t: np.float64(fsum(t)) / np.float64(L))
    return mixture, out, stats


def mix_given_stats(sources, recipe, L, n_out, stats, normalize=False):
    stats = np.asarray(stats, np.float64)
    src, start = pad(recipe)[:2]

    def source_mean(b, j, t):
        if src[b, j] < 0:
            return np.float64(0.0)
        with np.errstate(all="ignore"):
            return stats[b, j] * (np.float64(fsum(segment(sources, src[b, j], start[b, j], L))) / np.float64(L))

    return _outputs(sources, recipe, L, n_out, normalize, stats[:, :J], lambda b, m: (stats[b, J], stats[b, J + 1]), source_mean)


def _merged(sources, recipe, L, g, b):
    """The scaled slots of row b with the slots that name the same segment added up: they are one signal and add coherently."""
    src, start = pad(recipe)[:2]
    groups = {}
    for j, t in enumerate(scaled(sources, recipe, L, g, b)[0]):
        if t is not None:
            key = (int(src[b, j]), int(start[b, j]))
            groups[key] = groups[key] + t if key in groups else t
    return list(groups.values())


def max_abs_corr(sources, recipe, L):
    g = gains(sources, recipe, L)
    worst = 0.0
    for b in range(g.shape[0]):
        terms = [t - t.mean() for t in _merged(sources, recipe, L, g, b)]
        for i in range(len(terms)):
            for k in range(i + 1, len(terms)):
                d = math.sqrt(float(terms[i] @ terms[i]) * float(terms[k] @ terms[k]))
                if d > 0:
                    worst = max(worst, abs(float(terms[i] @ terms[k])) / d)
    return worst


def moment_bounds(sources, recipe, L):
    """What forming mean(m) and the deviation from float64 moments costs, per row, from the samples: with u = 2^-53,
    P = (sum_j |g_j| sqrt(E(x_j)))^2 >= sum m^2 and kappa = P / ((L - 1) var(m)), any-order sums of L terms give
    |d mean| <= (L + 16) u sqrt(P / L) and |d inv / inv| <= (L + 16) u kappa (half the variance's 2 (L + 16) u kappa).
    -> (mean bound (B), relative inv bound (B), kappa (B)).  kappa is 1 / J-ish for independent slots, 1 + (mean / std)^2 with a DC
    offset, and grows as 1 / (1 - |corr|) when slots cancel."""
    g = gains(sources, recipe, L)
    src, start = pad(recipe)[:2]
    B = g.shape[0]
    dm, di, kappa = np.zeros(B), np.zeros(B), np.zeros(B)
    u = 2.0 ** -53
    for b in range(B):
        terms, m = scaled(sources, recipe, L, g, b)
        P = sum(math.sqrt(energy(t)) for t in terms if t is not None) ** 2
        var = fsum((m - fsum(m) / L) ** 2) / (L - 1)
        kappa[b] = P / ((L - 1) * var) if var > 0 else np.inf
        dm[b], di[b] = (L + 16) * u * math.sqrt(P / L), (L + 16) * u * kappa[b]
    return dm, di, kappa


def collate(targets, perms):
    """core.py:183-202: targets (B,n_src,L), perms[i] the permutation of the batch used for source i -> (inputs (B,L), targets), float64."""
    t = np.asarray(targets, np.float64)
    B, n_src, L = t.shape
    new = np.zeros_like(t)
    with np.errstate(all="ignore"):
        for i in range(n_src):
            p = [int(v) for v in perms[i]]
            for b in range(B):
                s = t[p[b], i]
                new[b, i] = s * np.sqrt(np.float64(fsum(t[b, i] ** 2)) / np.float64(fsum(s ** 2)))
    return new.sum(1), new
