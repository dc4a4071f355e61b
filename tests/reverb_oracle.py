"""Float64 numpy restatement of the reverberant-image definition (include/rtfs_amd.h "Reverberant mixtures"; rtfs-net_amd/datas.py
reverberate, mix_batch(rirs=...)) and of a reverberant mixture as tests/mix_oracle.py's mixture of the images.  Independent of the library.

* ``window``     the samples x~[p + o - N + 1 .. p + o + L - 1] an image touches, float64, zeros outside the utterance
* ``image64``    r[t] = sum_k h[k] x~[p + t + o - k] in float64: per output one ``math.fsum`` over the N exact products (exactly rounded)
                 while N L <= 2^22, ``np.convolve`` in float64 above that (``exact`` forces either)
* ``image``      the same rounded to float32, what the device returns
* ``bound``      the per-sample error bar of a device image against ``image64``, derived and not measured.  The device adds the N
                 products, each exact in float64, one by one: with u = 2^-53 and A[t] = sum_k |h[k]| |x~[p + t + o - k]| any order of
                 summation stays within (N - 1) u A[t] (1 + O(N u)) of the true sum, and the one rounding to float32 adds 2^-24 |r|:
                     |r_dev - r| <= 2^-24 |r| + (N + 16) 2^-53 A[t]        against the fsum oracle,
                 with the second term doubled against the np.convolve oracle, whose own sum is rounded the same way
* ``mix``        ``mix_oracle.mix`` fed the oracle's images: every slot or reference with an RIR names its float32 image (start 0) instead
                 of its source; -> mixture, sources, stats, images (list), image_map (B, Jr)
* ``as_dry``     the recipe and source list ``mix`` hands to mix_oracle, for ``mix_oracle.mix_given_stats`` / ``max_abs_corr`` /
                 ``moment_bounds`` on images of the caller's choice (the device's own, say)

A reverberant recipe is the nine (B, J) arrays of ``datas.MixRecipe``: src, start, a, ref_src, ref_start, rir, ref_rir, rir_offset,
ref_offset."""
import math

import numpy as np

from tests import mix_oracle as MO

FSUM_LIMIT = 1 << 22


def samples(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return (x.astype(np.float32) / np.float32(32768.0)).astype(np.float64)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


def window(source, start, N, offset, L):
    x = samples(source)
    n_x = x.shape[0]
    assert 0 <= start and start + L <= n_x and 0 <= offset < N, (start, L, n_x, offset, N)
    lo = start + offset - (N - 1)
    w = np.zeros(L + N - 1)
    a, b = max(lo, 0), min(lo + L + N - 1, n_x)
    if b > a:
        w[a - lo:b - lo] = x[a:b]
    return w


def image64(source, start, h, offset, L, exact=None):
    h = np.asarray(h)
    assert h.dtype == np.float32 and h.ndim == 1
    N = h.shape[0]
    w = window(source, start, N, offset, L)
    hd = h.astype(np.float64)
    if exact is None:
        exact = N * L <= FSUM_LIMIT
    if not exact:
        return np.convolve(w, hd, mode="valid")
    hr = hd[::-1]  # r[t] = sum_i hr[i] w[t + i]
    return np.array([math.fsum((hr * w[t:t + N]).tolist()) for t in range(L)])


def image(source, start, h, offset, L, exact=None):
    return image64(source, start, h, offset, L, exact).astype(np.float32)


def bound(source, start, h, offset, L, exact=None):
    h = np.asarray(h)
    N = h.shape[0]
    if exact is None:
        exact = N * L <= FSUM_LIMIT
    w = window(source, start, N, offset, L)
    A = np.convolve(np.abs(w), np.abs(h.astype(np.float64)), mode="valid")
    r = image64(source, start, h, offset, L, exact)
    return 2.0 ** -24 * np.abs(r) + (1.0 if exact else 2.0) * (N + 16) * 2.0 ** -53 * A * (1 + 2.0 ** -40)  # A itself is a rounded sum


def as_dry(sources, rirs, recipe, L, images=None):
    """-> (sources + images, the five-array dry recipe that names them, images, image_map).  ``images``: a dict
    (src, start, rir, offset) -> float32 (L) to use instead of the oracle's own."""
    src, start, a, ref_src, ref_start, rir, ref_rir, off, ref_off = (np.array(v) for v in recipe)
    pool, made, order = list(sources), {}, []
    image_map = np.full(src.shape, -1, np.int64)

    def row(s, p, r, o):
        key = (int(s), int(p), int(r), int(o))
        if key not in made:
            made[key] = len(order)
            order.append(image(sources[key[0]], key[1], rirs[key[2]], key[3], L) if images is None else np.asarray(images[key], np.float32))
            pool.append(order[-1])
        return made[key]

    for b in range(src.shape[0]):
        for j in range(src.shape[1]):
            if src[b, j] < 0:
                continue
            if rir[b, j] >= 0:
                image_map[b, j] = row(src[b, j], start[b, j], rir[b, j], off[b, j])
                src[b, j], start[b, j] = len(sources) + image_map[b, j], 0
            if ref_src[b, j] >= 0 and ref_rir[b, j] >= 0:
                ref_src[b, j], ref_start[b, j] = len(sources) + row(ref_src[b, j], ref_start[b, j], ref_rir[b, j], ref_off[b, j]), 0
    return pool, (src, start, a, ref_src, ref_start), order, image_map


def mix(sources, rirs, recipe, L, n_out, normalize=False, eps=1e-8):
    pool, dry, images, image_map = as_dry(sources, rirs, recipe, L)
    mixture, out, stats = MO.mix(pool, dry, L, n_out, normalize=normalize, eps=eps)
    return mixture, out, stats, images, image_map
