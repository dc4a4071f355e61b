"""Long recordings in overlapping windows on the fused separator (AVNet.separate_long, System.separate_long, rtfs_longform_frame_f32,
rtfs_longform_overlap_add_f32) against tests/longform_oracle.py:

1. the framing kernel is a copy: bit-exact against the oracle at the plan edges, B 1 and 3, Tv shorter / equal / longer than the audio;
2. the overlap-add kernel does at most ceil(window / hop) float32 multiply-adds and one division per sample:
   |error| <= 4 ceil(window / hop) 2^-23 max|y| (from the operation count);
3. separate_long == oracle overlap-add of forward on the oracle's windows, fed in the same chunks, at the bound of 2;
4. a small plan against the reference-pinned numpy oracle of the forward, window by window, at the whole-separator bar 1e-4;
5. a captured call replayed on new input bytes is bit-identical to the eager call;
6. the forward cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big);
7. System.separate_long on raw lips == AVNet.separate_long on the video model's embedding of the whole track, bit-identical."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs, make_state_dict
from tests import longform_oracle as LO
from tests.util import rel_err, spec_R4

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
_MODELS = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def lib():
    from rtfs_net_amd import _lib
    return _lib


def model(repeats=4):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    if repeats not in _MODELS:
        m = R.AVNet(print_macs=False, **audionet_config(repeats, "SRU"))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(spec_R4(), 0).items()})
        _MODELS[repeats] = m.cuda().eval()
    return _MODELS[repeats]


def ola_bound(window, hop, y):
    return 4 * -(-window // hop) * 2.0 ** -23 * float(np.abs(y).max())


# (window, hop): hop = window, window / 2, window / 4; hop = 640 with window = 1280; the shipped default
PLANS = [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640), (32000, 16000)]


def edge_lengths(window, hop):
    """L = window - 1, window, window + 1; L = window + k hop and +- 1; a few samples (L < 4 included)."""
    return [3, 7, window - 1, window, window + 1, window + hop - 1, window + hop, window + hop + 1, window + 3 * hop - 1, window + 3 * hop,
            window + 3 * hop + 1, window + 2 * hop + 2]


# ---------------------------------------------------------------- 1. framing kernel: a copy
def frame_hip(x, v, window, hop):
    L_ = lib()
    B, L = x.shape
    Tv = v.shape[-1]
    N = LO.plan(L, Tv, window, hop)
    xw = L_.empty(B * N, window, device=x.device)
    vw = L_.empty(B * N, 512, window // SPF, device=x.device)
    L_.check(L_.load().rtfs_longform_frame_f32(L_.ptr(x), L_.ptr(v), L_.ptr(xw), L_.ptr(vw), B, L, Tv, window, hop, L_.stream_of(x)),
             "rtfs_longform_frame_f32")
    return xw, vw


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("window,hop", PLANS)
def test_framing_kernel_is_bit_exact(B, window, hop):
    rng = np.random.RandomState(window + hop + B)
    for L in edge_lengths(window, hop):
        frames = -(-L // SPF)
        for Tv in sorted({1, max(1, frames - 2), frames, frames + 3}):
            x, v = rng.randn(B, L).astype(np.float32), rng.randn(B, 512, Tv).astype(np.float32)
            xw, vw = frame_hip(dev(x), dev(v), window, hop)
            exw, evw = LO.frame(x, v, window, hop)
            xw, vw = host(xw), host(vw)
            assert xw.shape == exw.shape and vw.shape == evw.shape, (L, Tv)
            assert np.array_equal(xw, exw), f"audio windows differ: B {B} L {L} Tv {Tv} window {window} hop {hop}"
            assert np.array_equal(vw, evw), f"video windows differ: B {B} L {L} Tv {Tv} window {window} hop {hop}"


def test_framing_kernel_reads_an_unaligned_recording():
    """The recording as a view that starts 4 bytes into an allocation: the 16-byte loads must give way to dword loads."""
    x = np.random.RandomState(3).randn(1, 9001).astype(np.float32)
    v = np.random.RandomState(4).randn(1, 512, 15).astype(np.float32)
    buf = dev(np.concatenate([np.zeros(1, np.float32), x[0]]))
    xw, vw = frame_hip(buf[1:].view(1, 9001), dev(v), 2560, 1280)
    exw, evw = LO.frame(x, v, 2560, 1280)
    assert np.array_equal(host(xw), exw) and np.array_equal(host(vw), evw)


# ---------------------------------------------------------------- 2. overlap-add kernel
def ola_hip(y, B, L, window, hop):
    L_ = lib()
    n_src = y.shape[1]
    out = L_.empty(B, n_src, L, device=y.device)
    L_.check(L_.load().rtfs_longform_overlap_add_f32(L_.ptr(y), L_.ptr(out), B, n_src, L, window, hop, L_.stream_of(y)),
             "rtfs_longform_overlap_add_f32")
    return out


@pytest.mark.parametrize("n_src", [1, 2])
@pytest.mark.parametrize("window,hop", PLANS + [(5120, 1920)])
def test_overlap_add_kernel_vs_oracle(n_src, window, hop):
    rng = np.random.RandomState(window + hop + n_src)
    worst = 0.0
    for B in (1, 3):
        for L in edge_lengths(window, hop):
            N = LO.plan(L, 1, window, hop)
            y = rng.randn(B * N, n_src, window).astype(np.float32)
            got = host(ola_hip(dev(y), B, L, window, hop))
            want = LO.overlap_add(y, B, L, window, hop)
            assert got.shape == want.shape == (B, n_src, L)
            err, bound = float(np.abs(got - want).max()), ola_bound(window, hop, y)
            worst = max(worst, err / bound)
            assert np.isfinite(got).all() and err <= bound, f"B {B} L {L} n_src {n_src} window {window} hop {hop}: {err:.3e} > {bound:.3e}"
    print(f"[longform] overlap-add window {window} hop {hop} n_src {n_src}: worst error {worst:.3f} of the bound")


def test_overlap_add_is_a_partition_of_unity():
    """Identity "model": the framed recording cross-faded back is the recording, to the kernel's bound."""
    x = np.random.RandomState(5).randn(2, 70001).astype(np.float32)
    v = np.zeros((2, 512, 3), np.float32)
    for window, hop in [(32000, 16000), (32000, 32000), (32000, 6400)]:
        xw, _ = frame_hip(dev(x), dev(v), window, hop)
        got = host(ola_hip(xw.view(-1, 1, window), 2, 70001, window, hop))
        assert np.abs(got[:, 0] - x).max() <= ola_bound(window, hop, x), (window, hop)
        if hop == window:
            assert np.array_equal(got[:, 0], x)  # concatenation: weights 1, one window per sample


# ---------------------------------------------------------------- 3. composition identity
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("L", [116800, 336000])  # 7.3 s and 21 s
def test_separate_long_is_the_overlap_add_of_forward_on_the_windows(B, L):
    m = model(4)
    window, hop, max_batch = 32000, 16000, 5
    Tv = -(-L // SPF)
    wav, emb = make_inputs(B, L, Tv, 31 + B)
    got = host(m.separate_long(dev(wav), dev(emb), window=window, hop=hop, max_batch=max_batch))
    xw, vw = LO.frame(wav, emb, window, hop)
    N = LO.plan(L, Tv, window, hop)
    assert got.shape == (B, 1, L) and xw.shape[0] == B * N
    with torch.no_grad():  # the same ragged chunks: 5, 5, ..., rest
        y = np.concatenate([host(m(dev(xw[c:c + max_batch]), dev(vw[c:c + max_batch]))) for c in range(0, B * N, max_batch)])
    want = LO.overlap_add(y, B, L, window, hop)
    err, bound = float(np.abs(got - want).max()), ola_bound(window, hop, y)
    print(f"[longform] composition B {B} L {L} N {N}: max abs err {err:.3e}, bound {bound:.3e} (max|y| {np.abs(y).max():.3e})")
    assert np.isfinite(got).all() and err <= bound, (err, bound)


# ---------------------------------------------------------------- 4. against the reference-pinned oracle of the forward
def test_small_plan_vs_reference_pinned_oracle():
    from oracle import rtfs_oracle as O
    window, hop, L, Tv = 5120, 2560, 12000, 19
    sd = make_state_dict(spec_R4(), 0)
    wav, emb = make_inputs(1, L, Tv, 41)
    got = host(model(4).separate_long(dev(wav), dev(emb), window=window, hop=hop))
    xw, vw = LO.frame(wav, emb, window, hop)
    y = np.concatenate([O.avnet_forward(xw[i:i + 1], vw[i:i + 1], sd, repeats=4) for i in range(xw.shape[0])])
    want = LO.overlap_add(y, 1, L, window, hop)
    e = rel_err(got, want)
    print(f"[longform] window {window} hop {hop} L {L} Tv {Tv} R4 vs oracle windows: max-rel {e:.3e}")
    assert got.shape == (1, 1, L) and np.isfinite(got).all() and e <= 1e-4, e


def test_one_window_is_forward_on_the_padded_mixture():
    m = model(4)
    wav, emb = make_inputs(2, 20001, 32, 43)
    got = host(m.separate_long(dev(wav), dev(emb)))
    xw, vw = LO.frame(wav, emb, 32000, 16000)
    assert xw.shape == (2, 32000)
    with torch.no_grad():
        y = host(m(dev(xw), dev(vw)))
    assert np.abs(got - y[:, :, :20001]).max() <= ola_bound(32000, 16000, y)


# ---------------------------------------------------------------- 5. graph capture
def test_separate_long_can_be_captured_in_a_hip_graph():
    m = model(4)
    B, L = 1, 116800
    Tv = -(-L // SPF)
    wav, emb = make_inputs(B, L, Tv, 51)
    w, e = dev(wav), dev(emb)
    kw = dict(window=32000, hop=16000, max_batch=5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.separate_long(w, e, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.separate_long(w, e, **kw)
    wav2, emb2 = make_inputs(B, L, Tv, 52)
    w.copy_(dev(wav2)); e.copy_(dev(emb2))
    g.replay()
    replayed = host(out).copy()
    eager = host(m.separate_long(w, e, **kw))
    diff = float(np.abs(replayed - eager).max())
    print(f"[longform] graph replay vs eager on new input bytes: max abs diff {diff:.3e} (max|out| {np.abs(eager).max():.3e})")
    assert np.isfinite(replayed).all() and np.array_equal(replayed, eager), diff


# ---------------------------------------------------------------- 7. System with a video model
def test_system_separate_long_embeds_the_whole_track_once():
    import rtfs_net_amd as R
    from oracle import video_oracle as V
    video = R.FRCNNVideoModel(print_macs=False)
    video.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in V.make_video_state_dict(0).items()})
    video = video.cuda().eval()
    s = R.System(audio_model=model(4), video_model=video).eval()
    L, Tv = 96000, 150  # 6 s
    wav, _ = make_inputs(1, L, Tv, 71)
    lips = dev(V.make_video_input(1, Tv, 72))
    assert tuple(lips.shape) == (1, 1, Tv, 88, 88)
    w = dev(wav)
    got = host(s.separate_long(w, lips))
    with torch.no_grad():
        emb = video(lips)
    assert tuple(emb.shape) == (1, 512, Tv)
    want = host(model(4).separate_long(w, emb))
    diff = float(np.abs(got - want).max())
    print(f"[longform] System.separate_long vs AVNet.separate_long(video_model(lips)): max abs diff {diff:.3e}")
    assert got.shape == (1, 1, L) and np.isfinite(got).all() and np.array_equal(got, want), diff


# ---------------------------------------------------------------- 6. poisoned memory
FORWARD_CASES = "test_framing or test_overlap_add or test_separate_long_is or test_small_plan or test_one_window or test_system"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's forward cases in a fresh child process per pattern, with every workspace / output a C call fills poisoned
    (tests/test_hip_poisoned.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_longform.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
