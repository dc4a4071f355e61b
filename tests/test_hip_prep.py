"""Preparing raw recordings on the device (rtfs-net_amd/datas.py, csrc/k_prep.hip) against tests/prep_oracle.py:

1. lips: the pipelines on uint8 ROIs are BIT-EQUAL to the oracle rounded to float32 (256 possible values: no tolerance), "val" and
   seeded "train", every N x Tv x ROI size of the list, extreme offsets, both flips, a non-contiguous input; the video model gives the
   same bits on device-prepared and host-prepared lips;
2. normalise: the project's bar (1e-4 max-relative, 1e-5 l2-relative, here per row) at every length, K 0 / 1 / 2, a row with a large DC offset,
   amplitudes 1e-4 and 1e3; L = 1 gives NaN; the reference-named single-tensor form with and without ``std=``;
3. resample: the cached device bank is bit-equal to the oracle's bank; outputs at the same two bars relative to the output's peak, seven
   ratios, B 1 and 3, lengths from one sample to 60 s with the zero-padded edges in full; a second stream; graph capture + two replays;
4. System.separate_recording == separate_long on oracle-prepared inputs at the separator's bar; System.prepare_batch;
5. the forward cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs, make_state_dict
from tests import prep_oracle as PO
from tests.util import l2_rel, rel_err, spec_R4

pytestmark = pytest.mark.gpu

POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
MAX_REL, L2_REL = 1e-4, 1e-5  # the project's bar
_CACHE = {}


def D():
    from rtfs_net_amd import datas
    return datas


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------- 1. lips
def rois(N, Tv, H, W, seed=0):
    return np.random.RandomState(seed + N + 7 * Tv + H).randint(0, 256, (N, Tv, H, W)).astype(np.uint8)


@pytest.mark.parametrize("H,W", [(96, 96), (88, 88), (112, 100)])
@pytest.mark.parametrize("Tv", [1, 50, 257])
@pytest.mark.parametrize("N", [1, 3, 32])
def test_lips_pipelines_are_bit_equal(N, Tv, H, W):
    pipes = D().get_preprocessing_pipelines()
    roi = rois(N, Tv, H, W)
    r = dev(roi)
    got = host(pipes["val"](r))
    cy, cx = PO.center_offsets(H, W)
    assert got.shape == (N, 1, Tv, 88, 88)
    assert bits_equal(got, PO.lips_prepare(roi, [(cy, cx, 0)] * N)), f"val N {N} Tv {Tv} ROI {H}x{W}"
    rng = random.Random(100 * N + Tv)
    want_tab = [PO.draw_offsets(H, W, rng=rng) for _ in range(N)]
    got = host(pipes["train"](r, rng=random.Random(100 * N + Tv)))
    if (H, W) == (88, 88):
        assert all(t[:2] == (0, 0) for t in want_tab)  # offsets forced to 0
    assert bits_equal(got, PO.lips_prepare(roi, want_tab)), f"train N {N} Tv {Tv} ROI {H}x{W} table {want_tab[:4]}"


def test_lips_train_follows_the_global_seed_and_single_track_shape():
    pipes = D().get_preprocessing_pipelines()
    roi = rois(1, 5, 96, 96, seed=3)
    random.seed(77)
    got = host(pipes["train"](dev(roi[0])))  # (Tv,H,W) -> (1,1,Tv,88,88)
    random.seed(77)
    want = PO.lips_prepare(roi, [PO.draw_offsets(96, 96)])
    assert got.shape == (1, 1, 5, 88, 88) and bits_equal(got, want)
    assert bits_equal(host(pipes["test"](dev(roi))), PO.lips_prepare(roi, [(4, 4, 0)]))


def test_lips_extreme_offsets_and_both_flips():
    """Every corner of the offset range (row starts at every byte alignment) with and without the flip, one track each."""
    H, W = 112, 100
    table = [(dy, dx, f) for dy in (0, 24) for dx in (0, 1, 2, 3, 9, 10, 11, 12) for f in (0, 1)]
    roi = rois(len(table), 3, H, W, seed=5)
    pipe = D().get_preprocessing_pipelines()["val"]
    got = host(pipe(dev(roi), table=table))
    assert bits_equal(got, PO.lips_prepare(roi, table))
    for bad in [(25, 0, 0), (0, 13, 0), (-1, 0, 0), (0, 0, 2)]:
        with pytest.raises(ValueError):
            pipe(dev(roi[:1]), table=[bad])


def test_lips_non_contiguous_and_offset_views():
    pipe = D().get_preprocessing_pipelines()["val"]
    big = rois(2, 9, 120, 130, seed=9)
    view = dev(big)[:, ::2, 3:115, 7:107]  # strided in time, cropped in both image axes
    assert not view.is_contiguous()
    assert bits_equal(host(pipe(view)), PO.lips_prepare(np.ascontiguousarray(big[:, ::2, 3:115, 7:107]), [(12, 6, 0)] * 2))
    flat = dev(np.concatenate([np.zeros(3, np.uint8), big[:, :, :96, :96].reshape(-1)]))
    shifted = flat[3:].view(2, 9, 96, 96)  # contiguous, but the tensor starts 3 bytes into its allocation
    assert bits_equal(host(pipe(shifted)), PO.lips_prepare(np.ascontiguousarray(big[:, :, :96, :96]), [(4, 4, 0)] * 2))
    with pytest.raises(RuntimeError):
        pipe(dev(big).float())


def video_model():
    import rtfs_net_amd as R
    from oracle import video_oracle as V
    if "video" not in _CACHE:
        v = R.FRCNNVideoModel(print_macs=False)
        v.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in V.make_video_state_dict(0).items()})
        _CACHE["video"] = v.cuda().eval()
    return _CACHE["video"]


def test_video_model_on_device_lips_equals_host_lips():
    roi = rois(2, 50, 96, 96, seed=11)
    lips = D().get_preprocessing_pipelines()["val"](dev(roi))
    ref = dev(PO.lips_prepare(roi, [(4, 4, 0)] * 2))
    with torch.no_grad():
        a, b = host(video_model()(lips)), host(video_model()(ref))
    assert a.shape == (2, 512, 50) and np.isfinite(a).all() and bits_equal(a, b)


# ---------------------------------------------------------------- 2. normalise
def wav_case(L, K, seed):
    """Three mixtures: unit scale; mean 100 with deviation 0.01 (the case float32 moments get wrong); amplitude 1e-4 (seed even) or 1e3."""
    rng = np.random.RandomState(seed)
    mix = rng.randn(3, L)
    mix[1] = 100.0 + 0.01 * mix[1]
    mix[2] *= 1e-4 if seed % 2 == 0 else 1e3
    mix = mix.astype(np.float32)
    src = None
    if K:
        src = np.stack([mix.astype(np.float64) * (0.6 if k == 0 else 0.4) + 0.1 * mix.std(-1, keepdims=True) * rng.randn(3, L)
                        for k in range(K)], axis=1).astype(np.float32)
    return mix, src


def check_rows(got, want, what):
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    worst = (0.0, 0.0)
    for r in range(want.shape[0]):
        e, l2 = rel_err(got[r], want[r]), l2_rel(got[r], want[r])
        worst = (max(worst[0], e), max(worst[1], l2))
        assert np.isfinite(got[r]).all() and e <= MAX_REL and l2 <= L2_REL, f"{what} row {r}: max-rel {e:.3e}, l2-rel {l2:.3e}"
    return worst


@pytest.mark.parametrize("K", [0, 1, 2])
@pytest.mark.parametrize("L", [1600, 32000, 131072, 4800000])
def test_normalize_mixture_vs_oracle(L, K):
    mix, src = wav_case(L, K, seed=L % 1000 + K)
    wm, ws = PO.normalize_mixture(mix, src)
    if K:
        gm, gs = D().normalize_mixture(dev(mix), dev(src))
        assert gs.shape == src.shape
        w = check_rows(host(gs), ws, f"sources L {L} K {K}")
        print(f"[prep] normalise L {L} K {K} sources: worst row max-rel {w[0]:.2e}, l2-rel {w[1]:.2e}")
    else:
        gm = D().normalize_mixture(dev(mix))
    assert gm.shape == mix.shape
    w = check_rows(host(gm), wm, f"mixture L {L} K {K}")
    print(f"[prep] normalise L {L} K {K} mixture: worst row max-rel {w[0]:.2e}, l2-rel {w[1]:.2e}")


def test_normalize_other_forms():
    mix, src = wav_case(5003, 2, seed=4)  # L % 4 != 0: rows start off the 16-byte grid
    wm, ws = PO.normalize_mixture(mix, src)
    gm, gs = D().normalize_mixture(dev(mix), dev(src))
    check_rows(host(gm), wm, "mixture L 5003")
    check_rows(host(gs), ws, "sources L 5003")
    gm1, gs1 = D().normalize_mixture(dev(mix[0]), dev(src[0]))  # (L), (K,L)
    assert gm1.shape == (5003,) and gs1.shape == (2, 5003)
    check_rows(host(gm1)[None], wm[:1], "single mixture")
    check_rows(host(gs1), ws[0], "single sources")
    # the reference's name: own deviation per row, any leading shape; then with the mixture's deviation handed in
    check_rows(host(D().normalize_tensor_wav(dev(src))), PO.normalize_tensor_wav(src), "normalize_tensor_wav")
    sd = mix.astype(np.float64).std(-1, ddof=1, keepdims=True).astype(np.float32)
    got = D().normalize_tensor_wav(dev(src), eps=1e-8, std=dev(sd).unsqueeze(1))
    check_rows(host(got), PO.normalize_tensor_wav(src, std=sd[:, None, :]), "normalize_tensor_wav(std=)")
    one = host(D().normalize_mixture(dev(np.ones((2, 1), np.float32))))
    assert one.shape == (2, 1) and np.isnan(one).all()  # L = 1: NaN, as torch.std
    with pytest.raises(RuntimeError):
        D().normalize_mixture(torch.zeros(2, 8))
    with pytest.raises(ValueError):
        D().normalize_mixture(dev(mix), dev(src[:2]))


# ---------------------------------------------------------------- 3. resample
RATES = [(48000, 16000), (44100, 16000), (32000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (16000, 48000)]


def check_resample(x, orig, new, what):
    got = host(D().resample(dev(x), orig, new))
    want = PO.resample(x, orig, new)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    e, l2 = rel_err(got, want), l2_rel(got, want)
    assert np.isfinite(got).all() and e <= MAX_REL and l2 <= L2_REL, f"{what}: max-rel {e:.3e}, l2-rel {l2:.3e}"
    return e, l2


@pytest.mark.parametrize("orig,new", RATES)
def test_resample_bank_on_the_device_is_bit_equal(orig, new):
    bank = D().resample_bank(orig, new, "cuda")
    assert bank.is_cuda and D().resample_bank(orig, new, "cuda") is bank
    assert bits_equal(host(bank), PO.resample_bank(orig, new))


@pytest.mark.parametrize("orig,new", RATES)
def test_resample_edge_lengths(orig, new):
    o, n, width, taps = PO.resample_plan(orig, new)
    rng = np.random.RandomState(orig // 25 + new // 1000)
    worst = 0.0
    for B in (1, 3):
        for L in sorted({1, 2, taps - 1, taps, max(1, o - 1), o, o + 1, 2 * width + 3 * o + 1}):
            worst = max(worst, check_resample(rng.randn(B, L).astype(np.float32), orig, new, f"{orig}->{new} B {B} L {L}")[0])
    x = rng.randn(777).astype(np.float32)  # (L) in, (L') out
    y = D().resample(dev(x), orig, new)
    assert y.ndim == 1 and y.shape[0] == PO.resample_out_len(orig, new, 777)
    print(f"[prep] resample {orig}->{new} edge lengths: worst max-rel {worst:.2e}")


@pytest.mark.parametrize("orig,new", RATES)
def test_resample_two_and_sixty_seconds(orig, new):
    rng = np.random.RandomState(orig // 100)
    e2 = check_resample(rng.randn(3, 2 * orig + 1).astype(np.float32), orig, new, f"{orig}->{new} B 3 2 s")
    e60 = check_resample(rng.randn(1, 60 * orig).astype(np.float32), orig, new, f"{orig}->{new} B 1 60 s")
    print(f"[prep] resample {orig}->{new}: 2 s max-rel {e2[0]:.2e} l2 {e2[1]:.2e}; 60 s max-rel {e60[0]:.2e} l2 {e60[1]:.2e}")


def test_resample_equal_rates_and_refusals():
    x = dev(np.zeros(100, np.float32))
    assert D().resample(x, 16000, 16000) is x and D().resample(x, 16000) is x
    with pytest.raises(ValueError):
        D().resample(x, 16001, 16000)
    with pytest.raises(RuntimeError):
        D().resample(x.double(), 48000, 16000)
    view = dev(np.random.RandomState(1).randn(4, 3000).astype(np.float32))[::2, 5:2900]  # non-contiguous, off the 16-byte grid
    want = PO.resample(host(view), 44100, 16000)
    assert rel_err(host(D().resample(view, 44100, 16000)), want) <= MAX_REL


def test_resample_on_a_second_stream_and_under_graph_capture():
    orig, new, L = 44100, 16000, 88200
    rng = np.random.RandomState(8)
    xs = [rng.randn(2, L).astype(np.float32) for _ in range(3)]
    x = dev(xs[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # also the warm-up that uploads the bank before the capture
        y = D().resample(x, orig, new)
    torch.cuda.current_stream().wait_stream(s)
    assert rel_err(host(y), PO.resample(xs[0], orig, new)) <= MAX_REL
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = D().resample(x, orig, new)
    for i in (1, 2):  # captured once, replayed twice on changed input contents
        x.copy_(dev(xs[i]))
        g.replay()
        replayed = host(out).copy()
        eager = host(D().resample(x, orig, new))
        assert bits_equal(replayed, eager), i
        assert rel_err(replayed, PO.resample(xs[i], orig, new)) <= MAX_REL


def test_normalize_and_lips_under_graph_capture():
    mix, src = wav_case(40000, 2, seed=6)
    m, sr = dev(mix), dev(src)
    roi = rois(2, 7, 96, 96, seed=13)
    r = dev(roi)
    pipe = D().get_preprocessing_pipelines()["val"]
    D().normalize_mixture(m, sr)
    pipe(r)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gm, gs = D().normalize_mixture(m, sr)
        lips = pipe(r)
    mix2, src2 = wav_case(40000, 2, seed=7)
    roi2 = rois(2, 7, 96, 96, seed=14)
    m.copy_(dev(mix2)); sr.copy_(dev(src2)); r.copy_(dev(roi2))
    g.replay()
    wm, ws = PO.normalize_mixture(mix2, src2)
    check_rows(host(gm), wm, "replayed mixture")
    check_rows(host(gs), ws, "replayed sources")
    assert bits_equal(host(lips), PO.lips_prepare(roi2, [(4, 4, 0)] * 2))


# ---------------------------------------------------------------- 4. System
def audio_model():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    if "audio" not in _CACHE:
        m = R.AVNet(print_macs=False, **audionet_config(4, "SRU"))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(spec_R4(), 0).items()})
        _CACHE["audio"] = m.cuda().eval()
    return _CACHE["audio"]


def test_separate_recording_equals_separate_long_on_oracle_inputs():
    import rtfs_net_amd as R
    s = R.System(audio_model=audio_model(), video_model=video_model()).eval()
    B, fs, seconds = 2, 48000, 10
    Tv = 25 * seconds
    wav16, _ = make_inputs(B, 16000 * seconds, Tv, 91)
    wav48 = np.repeat(wav16, 3, axis=1).astype(np.float32)  # a 48 kHz recording with the level of the separator's test inputs
    roi = rois(B, Tv, 96, 96, seed=17)
    got = host(s.separate_recording(dev(wav48), fs, dev(roi)))
    w = dev(PO.resample(wav48, fs, 16000).astype(np.float32))
    lips = dev(PO.lips_prepare(roi, [(4, 4, 0)] * B))
    want = host(s.separate_long(w, lips))
    e = rel_err(got, want)
    print(f"[prep] separate_recording 48 kHz 10 s B 2 vs separate_long on oracle inputs: max-rel {e:.3e}")
    assert got.shape == want.shape == (B, 1, 16000 * seconds) and np.isfinite(got).all() and e <= 1e-4, e
    # without a video model the mouth slot holds embeddings; normalize_audio normalises the resampled mixture
    s2 = R.System(audio_model=audio_model(), video_model=None).eval()
    _, emb = make_inputs(B, 16000 * seconds, Tv, 92)
    got2 = host(s2.separate_recording(dev(wav48), fs, dev(emb), normalize_audio=True, window=32000, hop=32000))
    wn = dev(PO.normalize_mixture(PO.resample(wav48, fs, 16000))[0].astype(np.float32))
    want2 = host(audio_model().separate_long(wn, dev(emb), window=32000, hop=32000))
    assert rel_err(got2, want2) <= 1e-4


def test_prepare_batch():
    import rtfs_net_amd as R
    s = R.System(audio_model=audio_model(), video_model=video_model())
    B, K, Tv, L = 2, 2, 5, 4000
    mix, src = wav_case(L, K, seed=20)
    mix, src = mix[:B], src[:B]
    roi = rois(B * K, Tv, 100, 96, seed=21).reshape(B, K, Tv, 100, 96)
    wav, tgt, lips_f = dev(mix), dev(src), dev(PO.lips_prepare(roi[:, 0], [(6, 4, 0)] * B))
    out = s.prepare_batch((wav, tgt, lips_f, "keys"), train=True)  # float slots: the same objects
    assert out[0] is wav and out[1] is tgt and out[2] is lips_f and out[3] == "keys"
    out = s.prepare_batch((wav, tgt, dev(roi), "keys"), train=True, rng=random.Random(5))
    rng = random.Random(5)
    table = [PO.draw_offsets(100, 96, rng=rng) for _ in range(B * K)]
    assert out[0] is wav and out[1] is tgt and tuple(out[2].shape) == (B, K, 1, Tv, 88, 88)
    assert bits_equal(host(out[2]).reshape(B * K, 1, Tv, 88, 88), PO.lips_prepare(roi.reshape(B * K, Tv, 100, 96), table))
    out = s.prepare_batch((wav, tgt, dev(roi[:, 0]), "keys"), train=False, normalize_audio=True)
    assert tuple(out[2].shape) == (B, 1, Tv, 88, 88) and bits_equal(host(out[2]), host(lips_f))
    wm, ws = PO.normalize_mixture(mix, src)
    check_rows(host(out[0]), wm, "prepare_batch mixture")
    check_rows(host(out[1]), ws, "prepare_batch targets")


# ---------------------------------------------------------------- 5. poisoned memory
FORWARD_CASES = "test_lips or test_video or test_normalize_mixture or test_normalize_other or test_resample_edge or test_resample_two " \
                "or test_resample_equal or test_separate_recording or test_prepare_batch"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's forward cases in a fresh child process per pattern, with every workspace / output a C call fills poisoned
    (tests/test_hip_poisoned.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_prep.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
