"""Mouth ROIs from whole camera frames on the device (datas.mouth_rois, rtfs_mouth_rois_u8, System.separate_video, push_frames of the
three camera pools) against tests/mouth_oracle.py.  Every ROI comparison is np.array_equal on uint8: no tolerance.

1. the kernel through the C ABI on explicit maps: integer translation (== the frame slice, independent of the oracle), quarter turn,
   2x enlargement, 3.7x reduction, a 17-degree roll, the box over every edge and corner, wholly outside, exactly on the last row /
   column; every out / crop size; destinations at byte offsets 0 .. 3 inside a guarded buffer; J = 1, 3, 64, 257;
2. datas.mouth_rois: frame sizes, orders, strided views, K faces per frame, a sequence of tensors, a second stream, graph capture;
3. System.separate_video == separate_recording on the oracle's ROIs, bit for bit;
4. push_frames of the three camera pools == push fed datas.mouth_rois (bit for bit) and == separate_video (1e-4), frame_rate=30,
   timebase= with a dropped frame, refusals that leave no trace;
5. sections 1 and 2 again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mouth_oracle as MO
from tests.test_hip_longform import dev, host, lib, model
from tests.test_hip_many import video_model
from tests.util import rel_err

pytestmark = pytest.mark.gpu

POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
SPF = 640
SIZES = [((88, 88), (88, 88)), ((96, 96), (88, 88)), ((89, 97), (88, 88)), ((8, 8), (8, 8)), ((1, 1), (1, 1))]
FRAMES = [(47, 61, 3), (48, 64, 1), (270, 480, 3)]
ORDER_CODE = {"gray": 0, "bgr": 1, "rgb": 2}


def D():
    from rtfs_net_amd import datas
    return datas


def frames_of(n, H, W, C, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, H, W, 3) if C == 3 else (n, H, W)).astype(np.uint8)


def landmarks(n, H, W, seed, K=None):
    """n (x K) plausible faces inside an H x W frame: eye distance 0.15 .. 0.35 W, roll within 0.4 rad, the mouth below the eyes -
    sometimes hanging over the frame's edge."""
    rng = np.random.RandomState(seed)
    shape = (n,) if K is None else (n, K)
    c = rng.uniform([0.3 * W, 0.2 * H], [0.7 * W, 0.6 * H], shape + (2,))
    d, th = rng.uniform(0.15 * W, 0.35 * W, shape), rng.uniform(-0.4, 0.4, shape)
    u = np.stack([np.cos(th), np.sin(th)], -1)
    v = np.stack([-u[..., 1], u[..., 0]], -1)
    eyes = np.stack([c - 0.5 * d[..., None] * u, c + 0.5 * d[..., None] * u], -2)
    along, down = rng.uniform(-0.5, 0.5, shape + (4,)), rng.uniform(0.7, 1.4, shape + (4,))
    lips = c[..., None, :] + d[..., None, None] * (along[..., None] * u[..., None, :] + down[..., None] * v[..., None, :])
    return eyes, lips


# ---------------------------------------------------------------- 1. the kernel through the C ABI
def run_jobs(jobs, out_hw, offset=0, check_host=True):
    """jobs: [(device frame (H,W[,3]) uint8, order, A (2,3))] -> uint8 (J,Ho,Wo).  The destination planes lie back to back, `offset` bytes
    into a buffer of 0xA5 that is 256 bytes longer on both sides; every byte outside the planes must still be 0xA5 afterwards."""
    Ho, Wo = out_hw
    J, N = len(jobs), Ho * Wo
    buf = torch.full((256 + offset + J * N + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    table = np.zeros((J, 12), np.int64)
    for r, (f, order, A) in enumerate(jobs):
        assert f.dtype == torch.uint8 and f.is_cuda and f.stride(-1) == 1
        table[r, :6] = [f.data_ptr(), buf.data_ptr() + 256 + offset + r * N, f.shape[0], f.shape[1], f.stride(0),
                        (f.stride(1) if f.shape[1] > 1 else (3 if f.ndim == 3 else 1)) + 65536 * ORDER_CODE[order]]
        table[r, 6:] = np.ascontiguousarray(A, np.float64).reshape(6).view(np.int64)
    tab = dev(table)
    code = lib().load().rtfs_mouth_rois_u8(tab.data_ptr(), table.ctypes.data if check_host else None, J, Ho, Wo,
                                           lib().stream_of(tab))
    assert code == 0, code
    got = host(buf)
    assert (got[:256 + offset] == 0xA5).all() and (got[256 + offset + J * N:] == 0xA5).all(), "bytes outside the ROI planes were written"
    return got[256 + offset:256 + offset + J * N].reshape(J, Ho, Wo)


def rot(deg, scale, x0, y0):
    """ROI (j, i) -> source: a turn by `deg` and a step of `scale` source pixels per ROI pixel, ROI (0, 0) at (x0, y0)."""
    t = np.radians(deg)
    return np.array([[scale * np.cos(t), -scale * np.sin(t), x0], [scale * np.sin(t), scale * np.cos(t), y0]])


def maps_for(H, W, Ho, Wo):
    """name -> A: the maps of the issue for an H x W frame and an Ho x Wo ROI."""
    m = {
        "translation": np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 2.0]]),
        "quarter turn": np.array([[0.0, -1.0, float(W - 5)], [1.0, 0.0, 1.0]]),
        "enlarge 2x": rot(0.0, 0.5, 0.3 * W, 0.25 * H),
        "reduce 3.7x": rot(0.0, 3.7, -0.1 * W, 1.5),
        "roll 17": rot(17.0, 0.6, 0.35 * W, 0.1 * H),
        "outside": np.array([[1.0, 0.0, float(W + 40)], [0.0, 1.0, float(-3 * Ho - 40)]]),
        "far outside": np.array([[1e300, 0.0, -1e305], [0.0, -1e300, 1e307]]),
        "last row and column": np.array([[1.0, 0.0, float(W - Wo)], [0.0, 1.0, float(H - Ho)]]),  # sx == W - 1, fx == 0 at the last j
        "last column, half a row": np.array([[1.0, 0.0, float(W - Wo)], [0.0, 1.0, H - Ho + 0.5]]),
    }
    for name, (ex, ey) in {"left": (-1, 0), "right": (1, 0), "top": (0, -1), "bottom": (0, 1), "top left": (-1, -1),
                           "top right": (1, -1), "bottom left": (-1, 1), "bottom right": (1, 1)}.items():
        x0 = {-1: -0.45 * Wo, 0: 0.5 * (W - Wo), 1: W - 0.55 * Wo}[ex] + 0.25
        y0 = {-1: -0.45 * Ho, 0: 0.5 * (H - Ho), 1: H - 0.55 * Ho}[ey] + 0.125
        m["over " + name] = rot(0.0, 1.0, x0, y0)
    return m


def test_translation_is_the_frame_slice():
    """Independent of the oracle: an integer translation copies the grey plane (and the BGR2GRAY integers of a colour frame)."""
    g = frames_of(1, 150, 170, 1, 1)[0]
    got = run_jobs([(dev(g), "gray", [[1, 0, 17], [0, 1, 9]])], (96, 96))
    assert np.array_equal(got[0], g[9:105, 17:113])
    c = frames_of(1, 150, 170, 3, 2)[0].astype(np.int64)
    grey = ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8)
    A = [[1, 0, 60], [0, 1, 40]]
    got = run_jobs([(dev(c.astype(np.uint8)), "bgr", A), (dev(c[..., ::-1].astype(np.uint8)), "rgb", A)], (89, 97), offset=1)
    assert np.array_equal(got[0], grey[40:129, 60:157]) and np.array_equal(got[1], got[0])
    q = run_jobs([(dev(g), "gray", [[0, -1, 140], [1, 0, 20]])], (88, 88), offset=3)  # ROI (i, j) shows source (140 - i, 20 + j)
    assert np.array_equal(q[0], np.rot90(g[20:108, 53:141]))


@pytest.mark.parametrize("out_hw,crop_hw", SIZES)
@pytest.mark.parametrize("H,W,C", FRAMES)
def test_kernel_maps_sizes_and_offsets(H, W, C, out_hw, crop_hw):
    """Every map of the list as one job of ONE launch, for every frame size and order, at each of the four destination alignments."""
    orders = ("bgr", "rgb") if C == 3 else ("gray",)
    f = frames_of(1, H, W, C, H + out_hw[1])[0]
    fd = dev(f)
    maps = maps_for(H, W, *out_hw)
    for offset, order in zip(range(4), orders * 4):
        jobs = [(fd, order, A) for A in maps.values()]
        got = run_jobs(jobs, out_hw, offset=offset)
        for r, (name, A) in enumerate(maps.items()):
            want = MO.roi(f, A, out_hw, order)
            assert np.array_equal(got[r], want), f"{name} on {H}x{W}x{C} {order}, out {out_hw} at byte offset {offset}"
            if "outside" in name:
                assert not want.any()
    # ... and through the landmarks: the closed case with this crop is a translation by (100, 150) on a frame that holds it
    if C == 1:
        big = frames_of(1, 260, 200, 1, 5)[0]
        A = MO.affine([[89.6, 89.6], [166.4, 89.6]], [[100, 150], [187, 150], [120, 237], [160, 200]], out_hw, crop_hw)
        got = host(D().mouth_rois(dev(big)[None], [[[89.6, 89.6], [166.4, 89.6]]], [[[100, 150], [187, 150], [120, 237], [160, 200]]],
                                  out_hw=out_hw, crop_hw=crop_hw, order="gray"))
        assert got.shape == (1, *out_hw) and np.array_equal(got[0], MO.roi(big, A, out_hw, "gray"))


@pytest.mark.parametrize("J", [1, 3, 64, 257])
def test_jobs_in_one_launch(J):
    """J jobs that differ in source, geometry, order and map: three separate allocations, several jobs per frame."""
    srcs = [(frames_of(2, 47, 61, 3, 3), "bgr"), (frames_of(3, 48, 64, 1, 4), "gray"), (frames_of(1, 90, 120, 3, 5), "rgb")]
    devs = [dev(f) for f, _ in srcs]
    rng = np.random.RandomState(J)
    jobs, want = [], []
    for r in range(J):
        k = r % 3
        f, order = srcs[k]
        t = r % f.shape[0]
        A = rot(rng.uniform(-30, 30), rng.uniform(0.3, 1.2), rng.uniform(-10, 30), rng.uniform(-10, 20))
        jobs.append((devs[k][t], order, A))
        want.append(MO.roi(f[t], A, (40, 52), order))
    before = lib().load().rtfs_debug_launch_count()
    got = run_jobs(jobs, (40, 52), offset=J % 4, check_host=J != 3)
    assert lib().load().rtfs_debug_launch_count() == before + 1
    assert np.array_equal(got, np.stack(want))


def test_c_abi_refusals():
    f = dev(frames_of(1, 20, 20, 1, 0)[0])
    L, out = lib().load(), torch.zeros(64, dtype=torch.uint8, device="cuda")
    good = np.zeros((1, 12), np.int64)
    good[0, :6] = [f.data_ptr(), out.data_ptr(), 20, 20, 20, 1]
    good[0, 6:] = np.array([1.0, 0, 0, 0, 1.0, 0]).view(np.int64)
    tab, st = dev(good), lib().stream_of(f)
    before = L.rtfs_debug_launch_count()
    for col, val in ((0, 0), (1, 0), (2, 0), (3, 40000), (4, -1), (5, 1 + 65536 * 3), (5, 2 + 65536), (5, 0), (8, np.array([np.nan]).view(np.int64)[0])):
        bad = good.copy()
        bad[0, col] = val
        assert L.rtfs_mouth_rois_u8(tab.data_ptr(), bad.ctypes.data, 1, 8, 8, st) == -4, (col, val)
    assert L.rtfs_mouth_rois_u8(None, good.ctypes.data, 1, 8, 8, st) == -4
    for J, Ho, Wo in ((0, 8, 8), (1, 0, 8), (1, 8, 5000)):
        assert L.rtfs_mouth_rois_u8(tab.data_ptr(), good.ctypes.data, J, Ho, Wo, st) == -1
    assert L.rtfs_debug_launch_count() == before
    torch.cuda.synchronize()
    assert not host(out).any()


# ---------------------------------------------------------------- 2. datas.mouth_rois
@pytest.mark.parametrize("order", ["bgr", "rgb", "gray"])
@pytest.mark.parametrize("H,W,C", FRAMES)
def test_mouth_rois_sizes_and_orders(H, W, C, order):
    if (C == 3) == (order == "gray"):
        with pytest.raises(ValueError):  # a colour frame is not grey; a grey plane takes any order (it has no channels to order)
            D().mouth_rois(dev(frames_of(1, H, W, 3, 0)), *landmarks(1, H, W, 0), order="gray")
        if C == 3:
            return
    n = 5
    f = frames_of(n, H, W, C, H + W)
    eyes, lips = landmarks(n, H, W, seed=W)
    for out_hw, crop_hw in SIZES:
        got = D().mouth_rois(dev(f), eyes, lips, out_hw=out_hw, crop_hw=crop_hw, order=order)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (n, *out_hw)
        want = MO.rois(f, MO.affine(eyes, lips, out_hw, crop_hw), out_hw, "gray" if C == 1 else order)
        assert np.array_equal(host(got), want), (H, W, C, order, out_hw)
        assert out_hw[0] < 88 or want.any()


def test_mouth_rois_reads_strided_views_where_they_lie():
    big = frames_of(6, 80, 100, 3, 7)
    eyes, lips = landmarks(6, 60, 70, seed=8)
    bd = dev(big)
    rows = bd[:, 10:70, 20:90]  # a row stride larger than the width (and a start inside the allocation)
    assert rows.stride(1) == 300 and not rows.is_contiguous()
    before = lib().load().rtfs_debug_launch_count()
    got = D().mouth_rois(rows, eyes, lips)
    assert lib().load().rtfs_debug_launch_count() == before + 1
    assert np.array_equal(host(got), MO.rois(big[:, 10:70, 20:90], MO.affine(eyes, lips), (96, 96), "bgr"))
    every_other = bd[::2]  # a frame stride
    got = D().mouth_rois(every_other, eyes[:3], lips[:3], order="rgb")
    assert np.array_equal(host(got), MO.rois(big[::2], MO.affine(eyes[:3], lips[:3]), (96, 96), "rgb"))
    green = bd[..., 1]  # one channel of packed colour as a grey plane: pixel stride 3
    assert green.stride(2) == 3
    got = D().mouth_rois(green, eyes, lips, order="gray")
    assert np.array_equal(host(got), MO.rois(big[..., 1], MO.affine(eyes, lips), (96, 96), "gray"))
    luma = dev(np.zeros((6, 60, 128), np.uint8))  # a luma plane with a pitch of 128 for 70 visible columns
    luma[:, :, :70] = dev(big[:, 10:70, 20:90, 0])
    got = D().mouth_rois(luma[:, :, :70], eyes, lips, order="gray")
    assert np.array_equal(host(got), MO.rois(big[:, 10:70, 20:90, 0], MO.affine(eyes, lips), (96, 96), "gray"))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_mouth_rois_out_views_at_every_alignment(offset):
    n, out_hw = 3, (89, 97)
    f = frames_of(n, 47, 61, 3, 9)
    eyes, lips = landmarks(n, 47, 61, seed=offset)
    N = n * out_hw[0] * out_hw[1]
    buf = torch.full((256 + offset + N + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[256 + offset:256 + offset + N].view(n, *out_hw)
    res = D().mouth_rois(dev(f), eyes, lips, out_hw=out_hw, out=out)
    assert res is out
    got = host(buf)
    assert np.array_equal(got[256 + offset:256 + offset + N].reshape(n, *out_hw), MO.rois(f, MO.affine(eyes, lips, out_hw), out_hw, "bgr"))
    assert (got[:256 + offset] == 0xA5).all() and (got[256 + offset + N:] == 0xA5).all()


def test_faces_share_their_frame_and_a_sequence_runs_in_one_launch():
    n, K = 4, 3
    f = frames_of(n, 270, 480, 3, 11)
    eyes, lips = landmarks(n, 270, 480, seed=12, K=K)
    before = lib().load().rtfs_debug_launch_count()
    got = D().mouth_rois(dev(f), eyes, lips)
    assert lib().load().rtfs_debug_launch_count() == before + 1
    assert tuple(got.shape) == (n, K, 96, 96) and np.array_equal(host(got), MO.rois(f, MO.affine(eyes, lips), (96, 96), "bgr"))
    # three tensors of different resolution and channel count, one with a face axis, one launch, outputs into a caller's (K,n,...) layout
    fs = [frames_of(2, 47, 61, 3, 13), frames_of(3, 48, 64, 1, 14), f]
    lm = [landmarks(2, 47, 61, 15), landmarks(3, 48, 64, 16), (eyes, lips)]
    before = lib().load().rtfs_debug_launch_count()
    outs = D().mouth_rois([dev(x) for x in fs], [torch.from_numpy(e) for e, _ in lm], [l for _, l in lm], order="rgb")
    assert lib().load().rtfs_debug_launch_count() == before + 1 and isinstance(outs, list) and len(outs) == 3
    for x, (e, l), o, order in zip(fs, lm, outs, ("rgb", "gray", "rgb")):
        assert np.array_equal(host(o), MO.rois(x, MO.affine(e, l), (96, 96), order))
    kn = torch.zeros(K, n, 96, 96, dtype=torch.uint8, device="cuda")
    D().mouth_rois(dev(f), eyes, lips, out=kn.permute(1, 0, 2, 3))
    assert np.array_equal(host(kn).transpose(1, 0, 2, 3), MO.rois(f, MO.affine(eyes, lips), (96, 96), "bgr"))
    assert D().mouth_rois(dev(f[:0]), eyes[:0], lips[:0]).shape == (0, K, 96, 96)  # nothing to do, nothing launched


def test_mouth_rois_refusals_launch_nothing():
    f = dev(frames_of(3, 47, 61, 3, 1))
    eyes, lips = landmarks(3, 47, 61, 2)
    nan_eyes = eyes.copy()
    nan_eyes[1, 0, 0] = np.nan
    same = eyes.copy()
    same[2, 1] = same[2, 0]
    before = lib().load().rtfs_debug_launch_count()
    bad = [dict(frames=f.cpu()), dict(frames=f.float()), dict(frames=f[0]), dict(frames=f.permute(0, 3, 1, 2)), dict(frames=f[..., :2]),
           dict(eyes=eyes[:2]), dict(lips=lips[:2]), dict(eyes=eyes[:, :1]), dict(eyes=nan_eyes), dict(eyes=same), dict(order="yuv"),
           dict(order=None), dict(crop_hw=(97, 88)), dict(out_hw=(0, 96)), dict(out=torch.zeros(3, 96, 96, device="cuda")),
           dict(out=torch.zeros(3, 96, 95, dtype=torch.uint8, device="cuda")), dict(out=torch.zeros(3, 96, 96, dtype=torch.uint8)),
           dict(out=torch.zeros(3, 96, 192, dtype=torch.uint8, device="cuda")[:, :, ::2]), dict(eyes=torch.from_numpy(eyes).cuda()),
           dict(frames=[f, f], eyes=[eyes], lips=[lips]), dict(frames=[]), dict(eyes=np.stack([eyes, eyes], 1))]
    for kw in bad:
        args = dict(frames=f, eyes=eyes, lips=lips)
        args.update(kw)
        with pytest.raises(ValueError):
            D().mouth_rois(**args)
    assert lib().load().rtfs_debug_launch_count() == before


def test_mouth_rois_on_a_second_stream_and_under_graph_capture():
    n = 4
    fs = [frames_of(n, 48, 64, 3, 20 + i) for i in range(3)]
    eyes, lips = landmarks(n, 48, 64, seed=21)
    A = MO.affine(eyes, lips)
    x = dev(fs[0])
    out = torch.zeros(n, 96, 96, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # also the warm-up that uploads this call's job table before the capture
        D().mouth_rois(x, eyes, lips, out=out)
    torch.cuda.current_stream().wait_stream(s)
    assert np.array_equal(host(out), MO.rois(fs[0], A, (96, 96), "bgr"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D().mouth_rois(x, eyes, lips, out=out)
    for i in (1, 2):  # captured once, replayed twice on changed frame contents
        x.copy_(dev(fs[i]))
        out.zero_()
        g.replay()
        assert np.array_equal(host(out), MO.rois(fs[i], A, (96, 96), "bgr")), i
    other = torch.zeros_like(out)
    with pytest.raises(RuntimeError, match="before the capture"):  # a table that was never uploaded cannot go up while capturing
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            D().mouth_rois(x, eyes, lips, out=other)


# ---------------------------------------------------------------- 3. System.separate_video
def system():
    import rtfs_net_amd as R
    return R.System(audio_model=model(4), video_model=video_model()).eval()


def test_separate_video_equals_separate_recording_on_oracle_rois():
    from oracle.params import make_inputs
    s = system()
    B, fs, seconds = 2, 48000, 10  # the configuration of tests/test_hip_prep.py's separate_recording case
    Tv = 25 * seconds
    wav16, _ = make_inputs(B, 16000 * seconds, Tv, 91)
    wav48 = np.repeat(wav16, 3, axis=1).astype(np.float32)
    frames = [frames_of(Tv, 120, 160, 3, 30), frames_of(Tv, 90, 128, 3, 31)]  # one camera per recording
    lm = [landmarks(Tv, 120, 160, 32), landmarks(Tv, 90, 128, 33)]
    rois = np.stack([MO.rois(f, MO.affine(e, l), (96, 96), "bgr") for f, (e, l) in zip(frames, lm)])
    got = s.separate_video(dev(wav48), fs, [dev(f) for f in frames], [e for e, _ in lm], [l for _, l in lm])
    want = s.separate_recording(dev(wav48), fs, dev(rois))
    assert got.shape == want.shape == (B, 1, 16000 * seconds) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)  # the same bytes go into the same code
    one = s.separate_video(dev(wav48[0]), fs, dev(frames[0][..., ::-1].copy()), *lm[0], order="rgb", window=32000, hop=16000)
    assert torch.equal(one, s.separate_recording(dev(wav48[0]), fs, dev(rois[0]), window=32000, hop=16000))


# ---------------------------------------------------------------- 4. push_frames
WINDOW, HOP, MC = 2560, 1280, 8320
L_AUDIO = 3 * WINDOW + 7
CHUNKINGS = {"all at once": None, "1-7 frames": [3, 1, 7, 2, 5, 4, 6]}


def schedule(L, Tv, sizes):
    """[(audio samples, frames)] per push: frames in chunks of `sizes` (None: everything at once), the audio following the frames
    received 200 samples behind, so that no audio chunk ends on a frame boundary; then the rest of the audio."""
    if sizes is None:
        return [(L, Tv)]
    out, a, v, i = [], 0, 0, 0
    while v < Tv:
        m = min(sizes[i % len(sizes)], Tv - v)
        v, i = v + m, i + 1
        to = min(L, max(a, SPF * v - 200))
        out.append((to - a, m))
        a = to
    if a < L:
        out.append((L - a, 0))
    return out


def drive(pool, wavs, sch, feed, flush_kw=None):
    """Run every slot of `wavs` through `pool` by the shared schedule; feed(pool, ids, audio chunks, lo, hi) pushes frames lo .. hi - 1."""
    ids = sorted(wavs)
    got, a, v = {s: [] for s in ids}, 0, 0
    for na, m in sch:
        outs = feed(pool, ids, [dev(wavs[s][a:a + na]) for s in ids], v, v + m)
        a, v = a + na, v + m
        for s, o in zip(ids, outs):
            got[s].append(o)
    for s, o in zip(ids, pool.flush(ids, **(flush_kw or {}))):
        got[s].append(o)
    return got


def cat(parts):
    if isinstance(parts[0], dict):
        return {j: torch.cat([p[j] for p in parts if j in p], dim=-1) for j in parts[0]}
    return torch.cat(parts, dim=-1)


def camera_case(seed, n, shapes=((120, 160, 3), (90, 128, 1)), K=None):
    rng = np.random.RandomState(seed)
    wavs = {s: (0.1 * rng.randn(L_AUDIO)).astype(np.float32) for s in range(len(shapes))}
    frames = {s: frames_of(n, H, W, C, seed + s) for s, (H, W, C) in enumerate(shapes)}
    lm = {s: landmarks(n, H, W, seed + 10 + s, K=K[s] if isinstance(K, (list, tuple)) else K) for s, (H, W, C) in enumerate(shapes)}
    return wavs, frames, {s: dev(f) for s, f in frames.items()}, lm


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_camera_pool_push_frames(chunking):
    s = system()
    Tv = -(-L_AUDIO // SPF)
    wavs, frames, fd, lm = camera_case(40, Tv)
    sch = schedule(L_AUDIO, Tv, CHUNKINGS[chunking])
    rois = {k: D().mouth_rois(fd[k], *lm[k]) for k in fd}
    for k in fd:
        assert np.array_equal(host(rois[k]), MO.rois(frames[k], MO.affine(*lm[k]), (96, 96), "bgr"))
    kw = dict(window=WINDOW, hop=HOP, max_chunk=MC, max_batch=4, roi_hw=(96, 96))
    a, b = s.open_camera_streams(2, **kw), s.open_camera_streams(2, **kw)
    launches = []

    def feed_frames(pool, ids, audio, lo, hi):
        before = lib().load().rtfs_debug_launch_count()
        lip_tick = pool.lips._tick
        pool.lips._tick = lambda *x, **y: (launches.append(lib().load().rtfs_debug_launch_count() - before), lip_tick(*x, **y))[1]
        try:
            return pool.push_frames(ids, audio, [fd[k][lo:hi] for k in ids], [lm[k][0][lo:hi] for k in ids], [lm[k][1][lo:hi] for k in ids])
        finally:
            pool.lips._tick = lip_tick

    got = drive(a, wavs, sch, feed_frames)
    want = drive(b, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push(ids, audio, [rois[k][lo:hi] for k in ids]))
    assert launches and set(launches) <= {0, 1} and 1 in launches  # ONE crop launch for all named slots, in front of push's own
    for k in wavs:
        res = cat(got[k])
        assert torch.equal(res, cat(want[k])), (chunking, k)
        ref = s.separate_video(dev(wavs[k]), 16000, fd[k], *lm[k], window=WINDOW, hop=HOP)[0]
        e = rel_err(host(res), host(ref))
        print(f"[mouth] CameraStreamPool.push_frames, {chunking}, slot {k}: rel_err vs separate_video {e:.3e}")
        assert tuple(res.shape) == (1, L_AUDIO) and bool(torch.isfinite(res).all()) and e <= 1e-4, (k, e)
        assert a.counters(k) == ((0, 0, 0, 0), (0, 0))


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_speaker_pool_push_frames(chunking):
    s, K = system(), 2
    Tv = -(-L_AUDIO // SPF)
    wavs, frames, fd, lm = camera_case(50, Tv, K=K)
    sch = schedule(L_AUDIO, Tv, CHUNKINGS[chunking])
    rois = {k: D().mouth_rois(fd[k], *lm[k]).permute(1, 0, 2, 3).contiguous() for k in fd}  # (K,Tv,96,96), as push takes them
    kw = dict(window=WINDOW, hop=HOP, max_chunk=MC, max_batch=4, roi_hw=(96, 96), speakers=K)
    a, b = s.open_camera_streams(2, **kw), s.open_camera_streams(2, **kw)
    got = drive(a, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push_frames(
        ids, audio, [fd[k][lo:hi] for k in ids], [lm[k][0][lo:hi] for k in ids], [lm[k][1][lo:hi] for k in ids]))
    want = drive(b, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push(ids, audio, [rois[k][:, lo:hi].contiguous() for k in ids]))
    for k in wavs:
        res = cat(got[k])
        assert tuple(res.shape) == (K, L_AUDIO) and bool(torch.isfinite(res).all()) and torch.equal(res, cat(want[k])), (chunking, k)


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_face_pool_push_frames(chunking):
    s, Kmax = system(), 2
    Tv = -(-L_AUDIO // SPF)
    wavs, frames, fd, lm = camera_case(60, Tv, K=[2, 1])
    sch = schedule(L_AUDIO, Tv, CHUNKINGS[chunking])
    rois = {k: D().mouth_rois(fd[k], *lm[k]).permute(1, 0, 2, 3).contiguous() for k in fd}
    kw = dict(window=WINDOW, hop=HOP, max_chunk=MC, max_batch=4, roi_hw=(96, 96), max_speakers=Kmax)
    pools = [s.open_camera_streams(2, **kw) for _ in range(2)]
    for p in pools:
        assert [p.add_face(0), p.add_face(0), p.add_face(1, 1)] == [0, 1, 1]

    def feed_frames(pool, ids, audio, lo, hi):
        eyes = [lm[k][0][lo:hi] if k == 0 else [lm[k][0][lo:hi, 0]] for k in ids]  # an array with a face axis, or one array per face
        lips = [lm[k][1][lo:hi] if k == 0 else [lm[k][1][lo:hi, 0]] for k in ids]
        return pool.push_frames(ids, audio, [fd[k][lo:hi] for k in ids], eyes, lips)

    got = drive(pools[0], wavs, sch, feed_frames)
    want = drive(pools[1], wavs, sch, lambda pool, ids, audio, lo, hi: pool.push(ids, audio, [rois[k][:, lo:hi].contiguous() for k in ids]))
    for k, faces in ((0, [0, 1]), (1, [1])):
        res, ref = cat(got[k]), cat(want[k])
        assert sorted(res) == faces
        for j in faces:
            assert tuple(res[j].shape) == (L_AUDIO,) and bool(torch.isfinite(res[j]).all()) and torch.equal(res[j], ref[j]), (chunking, k, j)


def test_push_frames_at_the_camera_frame_rate():
    s = system()
    n = -(-L_AUDIO * 30 // 16000)  # 30 fps: every camera frame is cropped, the ingest launch selects afterwards
    wavs, frames, fd, lm = camera_case(70, n)
    sch = [(na * 25 // 30, m) for na, m in schedule(L_AUDIO, n, [4, 1, 6, 2]) if m]  # the audio follows the frames' TIME: 533 samples a frame
    sch.append((L_AUDIO - sum(na for na, _ in sch), 0))
    assert sum(m for _, m in sch) == n and 0 < sch[-1][0] <= MC
    rois = {k: D().mouth_rois(fd[k], *lm[k]) for k in fd}
    kw = dict(window=WINDOW, hop=HOP, max_chunk=MC, max_batch=4, roi_hw=(96, 96), frame_rate=30)
    a, b = s.open_camera_streams(2, **kw), s.open_camera_streams(2, **kw)
    got = drive(a, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push_frames(
        ids, audio, [fd[k][lo:hi] for k in ids], [lm[k][0][lo:hi] for k in ids], [lm[k][1][lo:hi] for k in ids]))
    want = drive(b, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push(ids, audio, [rois[k][lo:hi] for k in ids]))
    for k in wavs:
        res = cat(got[k])
        assert torch.equal(res, cat(want[k])), k
        ref = s.separate_video(dev(wavs[k]), 16000, fd[k], *lm[k], frame_rate=30, window=WINDOW, hop=HOP)[0]
        e = rel_err(host(res), host(ref))
        assert tuple(res.shape) == (1, L_AUDIO) and e <= 1e-4, (k, e)


def test_push_frames_with_timestamps_and_a_dropped_frame():
    s, tb = system(), 1000
    Tv = -(-L_AUDIO // SPF)
    stamps = [40 * i for i in range(Tv) if i != 5]  # 25 fps, frame 5 never arrived
    n = len(stamps)
    wavs, frames, fd, lm = camera_case(80, n)
    sch = schedule(L_AUDIO, n, [3, 1, 4, 2])
    rois = {k: D().mouth_rois(fd[k], *lm[k]) for k in fd}
    kw = dict(window=WINDOW, hop=HOP, max_chunk=MC, max_batch=4, roi_hw=(96, 96), timebase=tb)
    a, b = s.open_camera_streams(2, **kw), s.open_camera_streams(2, **kw)
    end = stamps[-1] + 1  # the largest until the streams are given

    def until(hi):
        return stamps[hi - 1] + 1 if hi else 0

    got = drive(a, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push_frames(
        ids, audio, [fd[k][lo:hi] for k in ids], [lm[k][0][lo:hi] for k in ids], [lm[k][1][lo:hi] for k in ids],
        timestamps=[stamps[lo:hi]] * len(ids), until=until(hi)), flush_kw=dict(until=end))
    want = drive(b, wavs, sch, lambda pool, ids, audio, lo, hi: pool.push(
        ids, audio, [rois[k][lo:hi] for k in ids], timestamps=[stamps[lo:hi]] * len(ids), until=until(hi)), flush_kw=dict(until=end))
    for k in wavs:
        res = cat(got[k])
        assert torch.equal(res, cat(want[k])), k
        ref = s.separate_video(dev(wavs[k]), 16000, fd[k], *lm[k], timestamps=stamps, timebase=tb, until=end, window=WINDOW, hop=HOP)[0]
        e = rel_err(host(res), host(ref))
        assert tuple(res.shape) == (1, L_AUDIO) and e <= 1e-4, (k, e)
    with pytest.raises(ValueError):  # stamps need a pool opened with timebase=
        s.open_camera_streams(1, window=WINDOW, hop=HOP, max_chunk=MC, roi_hw=(96, 96)).push_frames(
            [0], [dev(wavs[0][:640])], [fd[0][:1]], [lm[0][0][:1]], [lm[0][1][:1]], timestamps=[[0]])


def test_refused_push_frames_launch_nothing_and_leave_no_trace():
    s = system()
    wavs, frames, fd, lm = camera_case(90, 16, K=None)
    _, _, fdk, lmk = camera_case(91, 16, K=2)
    kw = dict(window=WINDOW, hop=HOP, max_chunk=MC, max_batch=4, roi_hw=(96, 96))
    plain, spk, fac = s.open_camera_streams(2, **kw), s.open_camera_streams(2, speakers=2, **kw), s.open_camera_streams(2, max_speakers=2, **kw)
    fac.add_face(0), fac.add_face(0), fac.add_face(1)
    audio = [dev(wavs[k][:1280]) for k in range(2)]

    def args(pool, lo=0, hi=2, cut=None, K=None):
        f, m = (fd, lm) if K is None else (fdk, lmk)
        eyes = [m[k][0][lo:hi] for k in range(2)]
        lips = [m[k][1][lo:hi] for k in range(2)]
        if pool is fac:
            eyes[1], lips[1] = eyes[1][:, :1], lips[1][:, :1]
        if cut == "eyes":
            eyes[1] = eyes[1][:-1]  # one landmark set too few
        return ([0, 1], audio, [f[k][lo:hi] for k in range(2)], eyes, lips)

    for pool, K in ((plain, None), (spk, 2), (fac, 2)):
        pool.push_frames(*args(pool, K=K))  # the streams are in mid-flight
        torch.cuda.synchronize()
        count = lib().load().rtfs_debug_launch_count()
        before = [pool.counters(k) for k in range(2)], pool.lips._hist.clone(), [list(c) for c in pool.lips._counters], [list(c) for c in pool.audio._counters]
        bad = [args(pool, 2, 4, cut="eyes", K=K), args(pool, 2, 16, K=K)]  # ... and a chunk over max_frames = 13
        ok = args(pool, 2, 4, K=K)
        bad.append((ok[0], [audio[0], torch.zeros(MC + 1, device="cuda")]) + ok[2:])  # what push's own checks refuse
        bad.append(([0, 0],) + ok[1:])
        bad.append(ok[:2] + ([ok[2][0], ok[2][1].cpu()],) + ok[3:])
        bad.append(ok[:2] + ([ok[2][0], ok[2][1].float()],) + ok[3:])
        bad.append(ok[:3] + ([ok[3][0], np.full_like(ok[3][1], np.nan)], ok[4]))
        if K is None:
            bad.append(ok[:3] + ([lmk[0][0][2:4], ok[3][1]], [lmk[0][1][2:4], ok[4][1]]))  # a face axis on a one-face pool
        else:
            bad.append(ok[:3] + ([lm[0][0][2:4], ok[3][1]], [lm[0][1][2:4], ok[4][1]]))  # no face axis where K faces are due
        for b in bad:
            with pytest.raises(ValueError):
                pool.push_frames(*b)
        with pytest.raises(ValueError):
            pool.push_frames(*ok, order="gray")
        with pytest.raises(ValueError):
            pool.push_frames(*ok, crop_hw=(97, 97))
        assert lib().load().rtfs_debug_launch_count() == count
        assert [pool.counters(k) for k in range(2)] == before[0] and [list(c) for c in pool.lips._counters] == before[2]
        assert [list(c) for c in pool.audio._counters] == before[3] and torch.equal(pool.lips._hist.view(torch.int32), before[1].view(torch.int32))
        pool.push_frames(*ok)  # and the stream goes on
    with pytest.raises(ValueError, match="no face"):
        empty = s.open_camera_streams(1, max_speakers=2, **kw)
        empty.push_frames([0], audio[:1], [fd[0][:1]], [lm[0][0][:1, None]], [lm[0][1][:1, None]])


# ---------------------------------------------------------------- 5. poisoned memory
KERNEL_CASES = "test_translation or test_kernel_maps or test_jobs_in or test_c_abi or test_mouth_rois or test_faces_share"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """The kernel-level cases in a fresh child process per pattern, with every workspace / output a C call fills poisoned
    (tests/test_hip_poisoned.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_mouth.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", KERNEL_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
