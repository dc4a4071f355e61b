"""Shape pairs for the nearest up-sampling index tests (tests/test_nearest_host.py on the CPU, tests/test_hip_nearest.py on the GPU).

Two closed forms for the source index that destination ``dst`` of an ``n_in -> n_out`` up-sampling reads:
  float32 rule   min(int(floorf(dst * (float(n_in) / float(n_out)))), n_in - 1)   oracle.rtfs_oracle.nearest_index; stock torch on float32
  integer rule   min(dst * n_in // n_out, n_in - 1)                               oracle.rtfs_oracle.nearest_index_integer
A pair "departs" when the two disagree at some dst."""
import functools

import numpy as np

from oracle.rtfs_oracle import nearest_index, nearest_index_integer

N_IN_MAX, N_OUT_MAX = 256, 1030

# (n_in, n_out) of every nearest up-sampling the committed goldens and the GPU tests' fixed shapes meet: CAF (Tv, T) pairs ...
GOLDEN_TV_T = [(7, 17), (7, 33), (8, 40), (13, 63), (27, 131), (31, 157), (50, 251), (52, 259), (100, 501), (133, 665), (205, 1025)]
# ... and the (Tv, T) of the committed end-to-end / gradient goldens alone (e2e_*_L4096/5000/8000/32000/64000/85000/131072, grad_R2_L4096_B2)
E2E_TV_T = [(7, 33), (8, 40), (13, 63), (50, 251), (100, 501), (133, 665), (205, 1025)]
# SURVEY.md's original probes
SURVEY_PAIRS = [(125, 251), (64, 129), (50, 251), (7, 50)]


def vp_lengths(tv, depth=4):
    """Lengths of the VP block's pyramid: Conv1d(k 3, stride 2, pad 1) per level."""
    n = [tv]
    for _ in range(depth - 1):
        n.append((n[-1] - 1) // 2 + 1)
    return n


def vp_pairs(tv):
    """Every (n_in, n_out) the VP block up-samples at Tv = tv: the coarsest level to each level, and each level to the one above."""
    n = vp_lengths(tv)
    return sorted({(n[-1], m) for m in n[:-1]} | {(n[i + 1], n[i]) for i in range(len(n) - 1)})


def departs(n_in, n_out):
    return not np.array_equal(nearest_index(n_in, n_out), nearest_index_integer(n_in, n_out))


@functools.lru_cache(maxsize=None)
def departing_pairs():
    """Every (n_in, n_out), 1 <= n_in <= 256, n_in <= n_out <= 1030, where the float32 rule and the integer rule disagree.  Vectorised over
    (n_out, dst) per n_in, with the same float32 operations as nearest_index (test_nearest_host.py checks that they agree)."""
    out = []
    dst = np.arange(N_OUT_MAX, dtype=np.int64)
    for n_in in range(1, N_IN_MAX + 1):
        n_out = np.arange(n_in, N_OUT_MAX + 1, dtype=np.int64)
        scale = (np.float32(n_in) / n_out.astype(np.float32))[:, None]
        f32 = np.minimum(np.floor(dst.astype(np.float32)[None, :] * scale).astype(np.int64), n_in - 1)
        integer = np.minimum(dst[None, :] * n_in // n_out[:, None], n_in - 1)
        bad = ((f32 != integer) & (dst[None, :] < n_out[:, None])).any(1)
        out += [(n_in, int(m)) for m in n_out[bad]]
    return tuple(out)


def stride_sample():
    """A fixed sample across the same rectangle, departing or not."""
    return [(n_in, n_out) for n_in in range(1, N_IN_MAX + 1, 7) for n_out in range(n_in, N_OUT_MAX + 1, 13)]


def used_pairs():
    """Pairs the existing tests and goldens use: CAF, the audio block's TFAR (T // 2 -> T, 64 -> 129), the VP block at their Tv."""
    p = set(GOLDEN_TV_T) | set(SURVEY_PAIRS)
    for tv, t in GOLDEN_TV_T:
        p |= set(vp_pairs(tv)) | {(t // 2, t)}
    return sorted(p)
