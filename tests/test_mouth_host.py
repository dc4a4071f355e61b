"""Mouth ROIs from whole camera frames, host side (datas.mouth_affine, rtfs_mouth_affine, tests/mouth_oracle.py), no GPU:

1. the closed case gives exactly the two matrices of the issue;
2. rtfs_mouth_affine through ctypes and datas.mouth_affine equal mouth_oracle.affine BIT for bit on 2048 seeded landmark sets;
3. on the same sets the oracle's map, taken back through the restated reference matrix (arctan2 / cos / sin), lands within 1e-9 px of
   cv2.resize's pixel-centre rule on the lip box;
4. refusals; 5. the oracle's sampler against plain slices and np.rot90; 6. the new symbols are declared, bound and built."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mouth_oracle as MO
from tests.util import ROOT

EYES0 = [[89.6, 89.6], [166.4, 89.6]]
LIPS0 = [[100, 150], [187, 150], [120, 237], [160, 200]]
SIZES = [((96, 96), (88, 88)), ((88, 88), (88, 88)), ((89, 97), (88, 88)), ((8, 8), (8, 8)), ((1, 1), (1, 1)), ((112, 100), (70, 90))]


def D():
    from rtfs_net_amd import datas
    return datas


def landmark_sets(n, seed=0):
    """n random faces: eye distance 20 .. 400 px, any roll, anywhere in a 1080p frame; lip points below the eyes, scattered."""
    rng = np.random.RandomState(seed)
    c = rng.uniform([100, 100], [1820, 980], (n, 2))
    d, th = rng.uniform(20, 400, n), rng.uniform(-np.pi, np.pi, n)
    u = np.stack([np.cos(th), np.sin(th)], -1)
    v = np.stack([-u[:, 1], u[:, 0]], -1)
    eyes = np.stack([c - 0.5 * d[:, None] * u, c + 0.5 * d[:, None] * u], 1)
    along, down = rng.uniform(-0.6, 0.6, (n, 4)), rng.uniform(0.4, 1.4, (n, 4))
    lips = c[:, None] + d[:, None, None] * (along[..., None] * u[:, None] + down[..., None] * v[:, None])
    return eyes, lips


def c_affine(eyes, lips, out_hw, crop_hw):
    from rtfs_net_amd import _lib
    eyes, lips = np.ascontiguousarray(eyes, np.float64), np.ascontiguousarray(lips, np.float64)
    n = eyes.size // 4
    A, bad = np.full((n, 2, 3), np.nan), C.c_longlong(-7)
    code = _lib.load().rtfs_mouth_affine(eyes.ctypes.data, lips.ctypes.data, n, *out_hw, *crop_hw, A.ctypes.data, C.byref(bad))
    return code, A, bad.value


def test_closed_case_gives_the_two_matrices_exactly():
    for fn in (MO.affine, D().mouth_affine):
        assert np.array_equal(fn(EYES0, LIPS0, (88, 88), (88, 88)), np.array([[1.0, 0.0, 100.0], [0.0, 1.0, 150.0]]))
        assert np.array_equal(fn(EYES0, LIPS0, (96, 96), (88, 88)), np.array([[1.0, 0.0, 96.0], [0.0, 1.0, 146.0]]))
        assert np.array_equal(fn(EYES0, LIPS0), fn(EYES0, LIPS0, (96, 96), (88, 88)))  # the defaults
    code, A, bad = c_affine(EYES0, LIPS0, (88, 88), (88, 88))
    assert code == 0 and bad == -1 and np.array_equal(A[0], [[1.0, 0.0, 100.0], [0.0, 1.0, 150.0]])


@pytest.mark.parametrize("out_hw,crop_hw", SIZES)
def test_c_planner_equals_the_oracle_bit_for_bit(out_hw, crop_hw):
    eyes, lips = landmark_sets(2048, seed=out_hw[0] + crop_hw[1])
    want = MO.affine(eyes, lips, out_hw, crop_hw)
    code, got, bad = c_affine(eyes, lips, out_hw, crop_hw)
    assert code == 0 and bad == -1
    assert got.shape == want.shape == (2048, 2, 3) and np.array_equal(got.view(np.int64), want.view(np.int64))
    # the public entry: numpy in, numpy out; a CPU tensor in, a CPU tensor out; any leading shape
    pub = D().mouth_affine(eyes.reshape(64, 32, 2, 2), lips.reshape(64, 32, 4, 2), out_hw, crop_hw)
    assert isinstance(pub, np.ndarray) and pub.dtype == np.float64 and pub.shape == (64, 32, 2, 3)
    assert np.array_equal(pub.reshape(-1, 2, 3).view(np.int64), want.view(np.int64))
    t = D().mouth_affine(torch.from_numpy(eyes), torch.from_numpy(lips).float().double(), out_hw, crop_hw)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.is_cuda
    assert np.array_equal(t.numpy().view(np.int64), MO.affine(eyes, lips.astype(np.float32), out_hw, crop_hw).view(np.int64))


@pytest.mark.parametrize("out_hw,crop_hw", SIZES[:3])
def test_map_agrees_with_the_reference_matrix_and_the_resize_rule(out_hw, crop_hw):
    """Source points of the oracle's map, taken to the aligned face by the restated reference matrix, against the pixel-centre rule on
    the lip box found with that same reference matrix: 1e-9 px (measured 2.3e-13; the margin covers cos(atan2) against dx / dist)."""
    eyes, lips = landmark_sets(2048, seed=5)
    A, M = MO.affine(eyes, lips, out_hw, crop_hw), MO.reference_matrix(eyes)
    ax, ay = MO.aligned_points(eyes, lips, out_hw, crop_hw, M=M)
    j, i = np.arange(out_hw[1], dtype=np.float64), np.arange(out_hw[0], dtype=np.float64)
    worst = 0.0
    for jj, ii in ((j, np.zeros_like(j)), (j, np.full_like(j, out_hw[0] - 1.0)), (np.zeros_like(i), i), (np.full_like(i, out_hw[1] - 1.0), i)):
        sx = A[:, 0, 0, None] * jj + A[:, 0, 1, None] * ii + A[:, 0, 2, None]
        sy = A[:, 1, 0, None] * jj + A[:, 1, 1, None] * ii + A[:, 1, 2, None]
        qx = M[:, 0, 0, None] * sx + M[:, 0, 1, None] * sy + M[:, 0, 2, None]
        qy = M[:, 1, 0, None] * sx + M[:, 1, 1, None] * sy + M[:, 1, 2, None]
        wx = ax[:, jj.astype(int)] if jj is j else ax[:, [int(jj[0])]]
        wy = ay[:, ii.astype(int)] if ii is i else ay[:, [int(ii[0])]]
        worst = max(worst, float(np.abs(qx - wx).max()), float(np.abs(qy - wy).max()))
    print(f"[mouth] out {out_hw} crop {crop_hw}: map vs reference matrix + resize rule, worst {worst:.3e} px")
    assert worst <= 1e-9
    assert np.abs(MO.forward(eyes) - M).max() <= 1e-9  # the two statements of the alignment itself


def test_refusals():
    e, l = np.array(EYES0), np.array(LIPS0, dtype=np.float64)
    bad_sets = []
    for v in (np.nan, np.inf, -np.inf):
        for arr, pos in ((0, (1, 0)), (1, (2, 1))):
            ee, ll = e.copy(), l.copy()
            (ee if arr == 0 else ll)[pos] = v
            bad_sets.append((ee, ll))
    bad_sets.append((np.array([[5.0, 7.0], [5.0, 7.0]]), l))  # dist == 0
    bad_sets.append((np.array([[0.0, 0.0], [1e-320, 0.0]]), l))  # a denormal eye distance: the scale overflows, no finite matrix
    for ee, ll in bad_sets:
        for fn in (MO.affine, D().mouth_affine):
            with pytest.raises(ValueError):
                fn(ee, ll)
        stack_e, stack_l = np.stack([e, e, ee]), np.stack([l, l, ll])  # the refused set is named
        code, _, bad = c_affine(stack_e, stack_l, (96, 96), (88, 88))
        assert code == -4 and bad == 2
    for out_hw, crop_hw in (((96, 96), (97, 88)), ((96, 96), (88, 97)), ((96, 96), (0, 88)), ((96, 96), (88, 0)), ((0, 0), (0, 0))):
        for fn in (MO.affine, D().mouth_affine):
            with pytest.raises(ValueError):
                fn(e, l, out_hw, crop_hw)
        assert c_affine(e, l, out_hw, crop_hw)[0] == -4
    for ee, ll in ((e[:1], l), (e, l[:3]), (e.reshape(-1), l), (np.stack([e, e]), l[None]), (e[None], np.stack([l, l]))):  # wrong shapes
        for fn in (MO.affine, D().mouth_affine):
            with pytest.raises(ValueError):
                fn(ee, ll)
    with pytest.raises(ValueError):
        D().mouth_affine(e, l, out_hw=96)
    with pytest.raises(ValueError):
        D().mouth_affine("eyes", l)
    assert D().mouth_affine(np.zeros((0, 2, 2)), np.zeros((0, 4, 2))).shape == (0, 2, 3)


def frame(H, W, C3, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3) if C3 else (H, W)).astype(np.uint8)


def test_oracle_sampler_on_a_translation_is_the_slice():
    f = frame(120, 140, False, 1)
    A = np.array([[1.0, 0.0, 17.0], [0.0, 1.0, 9.0]])
    assert np.array_equal(MO.roi(f, A, (96, 96), "gray"), f[9:105, 17:113])
    c = frame(120, 140, True, 2)
    ci = c.astype(np.int64)
    g = ((1868 * ci[..., 0] + 9617 * ci[..., 1] + 4899 * ci[..., 2] + 8192) >> 14).astype(np.uint8)
    assert np.array_equal(MO.roi(c, A, (89, 97), "bgr"), g[9:98, 17:114])
    assert np.array_equal(MO.roi(c[..., ::-1], A, (89, 97), "rgb"), g[9:98, 17:114])
    # hanging over the corner: zeros outside, the slice inside
    out = MO.roi(f, np.array([[1.0, 0.0, -5.0], [0.0, 1.0, 100.0]]), (40, 30), "gray")
    assert np.array_equal(out[:20, 5:], f[100:120, :25]) and not out[20:].any() and not out[:, :5].any()
    # through the formula: the closed case is the translation by (100, 150)
    big = frame(300, 300, False, 3)
    assert np.array_equal(MO.rois(big[None], MO.affine(EYES0, LIPS0, (88, 88), (88, 88))[None], (88, 88), "gray")[0], big[150:238, 100:188])


QUARTER_EYES = [[200.0, 60.0], [200.0, 136.8]]  # the corner on the left in the image straight above the right one: dx == 0, scale 1
QUARTER_LIPS = [[100.0, 180.0], [187.0, 267.0], [150.0, 200.0], [120.0, 250.0]]


def test_oracle_sampler_on_a_quarter_turn_is_rot90():
    """Eyes vertical (dx == 0): the head is rolled by 90 degrees.  By hand, with c = (200, 98.4), the aligned point of p is
    (py - 98.4 + 128, -(px - 200) + 89.6), the lip box is 88 x 88 from (209.6, 102.6), and ROI pixel (i, j) shows source
    (187 - i, 180 + j): np.rot90 of the slice [180:268, 100:188] - a check of the sampler and of the formula's signs that goes through
    neither.  The matrix entries carry rounding errors of a few ulp (38.4 and 89.6 are no binary fractions); weights that far from 0 or 1
    cannot move an integer pixel value across a rounding boundary, so the bytes are exact."""
    f = frame(300, 320, False, 4)
    A = MO.affine(QUARTER_EYES, QUARTER_LIPS, (88, 88), (88, 88))
    assert np.abs(A - np.array([[0.0, -1.0, 187.0], [1.0, 0.0, 180.0]])).max() <= 1e-11
    assert np.array_equal(MO.roi(f, A, (88, 88), "gray"), np.rot90(f[180:268, 100:188]))
    A = MO.affine(QUARTER_EYES, QUARTER_LIPS, (96, 96), (88, 88))  # ... and with the rim: (191 - i, 176 + j)
    assert np.array_equal(MO.roi(f, A, (96, 96), "gray"), np.rot90(f[176:272, 96:192]))


def test_symbols_are_declared_bound_and_built():
    from rtfs_net_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    kh = open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "kernels.h")).read()
    mk = open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "k_mouth.hip")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("rtfs_mouth_affine", "rtfs_mouth_rois_u8"):
        assert re.search(rf"\bint {name}\(", hdr) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"\bint mouth_affine\(", kh) and re.search(r"\bint launch_mouth_rois\(", kh)
    assert "k_mouth.hip" in mk.split("SRCS :=", 1)[1].split("\n", 1)[0]
    assert "#pragma clang fp contract(off)" in src  # the bit-equality rests on it
    assert "RTFS_MOUTH_JOB_WORDS 12" in hdr and D().MOUTH_JOB_WORDS == 12
    assert {"mouth_affine", "mouth_rois"} <= set(D().__all__)
