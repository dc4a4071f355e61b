"""Many recordings of different lengths in one pooled pass (AVNet.separate_many, System.separate_many, System.separate_recordings,
rtfs_longform_frame_many_f32, rtfs_longform_overlap_add_many_f32) against tests/many_oracle.py:

1. the pooled framing kernel is a copy: bit-exact against the oracle, R = 12 recordings carrying the plan edges with Tv shorter / equal /
   longer than the audio and one recording 4 bytes into its allocation, R = 1, and R = 40 recordings of one window each;
2. the pooled overlap-add does at most ceil(window / hop) float32 multiply-adds and one division per sample:
   |error| <= 4 ceil(window / hop) 2^-23 max|y| (tests/test_hip_longform.py's ola_bound, from the operation count), per recording over its
   own rows; the floats between two recordings' blocks are never written;
3. frame + overlap-add with the identity model returns every recording to that bound, bit for bit when hop == window;
4. separate_many == oracle overlap-add of forward on the oracle's pooled windows, fed in the same chunks that straddle recordings, at the
   bound of 2; each result == separate_long on that recording alone at the project's parity bar 1e-4 (expected about 1e-6: the windows
   are the same, the batch they ride in is not);
5. a small case against the reference-pinned numpy oracle of the forward, window by window, at 1e-4;
6. System.separate_many on raw lips == AVNet.separate_many on embeddings computed track by track; System.separate_recordings ==
   separate_recording per recording, both at 1e-4;
7. the forward cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs, make_state_dict
from tests import many_oracle as MO
from tests.util import rel_err, spec_R4

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
_CACHE = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def lib():
    from rtfs_net_amd import _lib
    return _lib


def model():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    if "audio" not in _CACHE:
        m = R.AVNet(print_macs=False, **audionet_config(4, "SRU"))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(spec_R4(), 0).items()})
        _CACHE["audio"] = m.cuda().eval()
    return _CACHE["audio"]


def video_model():
    import rtfs_net_amd as R
    from oracle import video_oracle as V
    if "video" not in _CACHE:
        v = R.FRCNNVideoModel(print_macs=False)
        v.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in V.make_video_state_dict(0).items()})
        _CACHE["video"] = v.cuda().eval()
    return _CACHE["video"]


def ola_bound(window, hop, y):
    return 4 * -(-window // hop) * 2.0 ** -23 * float(np.abs(y).max())


PLANS = [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640)]


def edge_lengths(window, hop):
    """12 recordings: a few samples (L < 4 included); L = window - 1, window, window + 1; L = window + k hop and +- 1."""
    return [3, 7, window - 1, window, window + 1, window + hop - 1, window + hop + 1, window + 3 * hop - 1, window + 3 * hop + 1,
            window + hop, window + 3 * hop, window + 2 * hop + 2]


def length_mixes(window, hop):
    e = edge_lengths(window, hop)
    return [e, e[::-1], [e[4]], [641] * 40]


def video_lengths(Ls):
    frames = [-(-L // SPF) for L in Ls]
    return [(1, max(1, f - 2), f, f + 3)[r % 4] for r, f in enumerate(frames)]


def c_plan(Ls, Tvs, window, hop, n_src):
    """The table of rtfs_longform_many_plan, checked against the oracle's: (oracle plan, 5 R words)."""
    R = len(Ls)
    rows, floats = ctypes.c_longlong(0), ctypes.c_longlong(0)
    table = (ctypes.c_longlong * (5 * R))()
    rc = lib().load().rtfs_longform_many_plan((ctypes.c_longlong * R)(*Ls), (ctypes.c_longlong * R)(*Tvs), R, window, hop, n_src, table,
                                              ctypes.byref(rows), ctypes.byref(floats))
    p = MO.plan(Ls, Tvs, window, hop, n_src)
    assert rc == 0 and list(table) == MO.table(p) and rows.value == p["rows"] and floats.value == p["floats"]
    return p, list(table)


# ---------------------------------------------------------------- 1. framing kernel: a copy
def frame_hip(wavs, vids, window, hop):
    """wavs, vids: device tensors (L_r), (512, Tv_r), separate allocations."""
    L_ = lib()
    R = len(wavs)
    p, table = c_plan([int(w.shape[0]) for w in wavs], [int(v.shape[1]) for v in vids], window, hop, 1)
    tab = torch.tensor(table + [w.data_ptr() for w in wavs] + [v.data_ptr() for v in vids], dtype=torch.int64).cuda()
    xw = L_.empty(p["rows"], window, device=tab.device)
    vw = L_.empty(p["rows"], 512, window // SPF, device=tab.device)
    L_.check(L_.load().rtfs_longform_frame_many_f32(L_.ptr(tab[5 * R:6 * R]), L_.ptr(tab[6 * R:]), L_.ptr(tab), L_.ptr(xw), L_.ptr(vw), R,
                                                    p["rows"], window, hop, L_.stream_of(xw)), "rtfs_longform_frame_many_f32")
    return xw, vw


@pytest.mark.parametrize("window,hop", PLANS)
def test_framing_kernel_is_bit_exact(window, hop):
    rng = np.random.RandomState(window + hop)
    for Ls in length_mixes(window, hop):
        Tvs = video_lengths(Ls)
        xs = [rng.randn(L).astype(np.float32) for L in Ls]
        vs = [rng.randn(512, Tv).astype(np.float32) for Tv in Tvs]
        wavs, vids = [dev(x) for x in xs], [dev(v) for v in vs]
        if len(Ls) > 1:  # one recording as a view that starts 4 bytes into its allocation: dword loads for that recording only
            wavs[5] = dev(np.concatenate([np.zeros(1, np.float32), xs[5]]))[1:]
            assert wavs[5].data_ptr() % 16 == 4
        xw, vw = frame_hip(wavs, vids, window, hop)
        exw, evw = MO.frame(xs, vs, window, hop)
        xw, vw = host(xw), host(vw)
        assert xw.shape == exw.shape and vw.shape == evw.shape, Ls
        assert np.array_equal(xw, exw), f"audio windows differ: window {window} hop {hop} lengths {Ls}"
        assert np.array_equal(vw, evw), f"video windows differ: window {window} hop {hop} lengths {Ls} Tv {Tvs}"


# ---------------------------------------------------------------- 2. overlap-add kernel
def ola_hip(y, Ls, window, hop, fill=None):
    """y device (sum N, n_src, window) -> the flat output on the host and its plan; ``fill`` is written over the output first."""
    L_ = lib()
    R, n_src = len(Ls), int(y.shape[1])
    p, table = c_plan(Ls, [1] * R, window, hop, n_src)
    assert p["rows"] == y.shape[0]
    tab = torch.tensor(table, dtype=torch.int64).cuda()
    out = L_.empty(p["floats"], device=y.device)
    if fill is not None:
        out.fill_(fill)
    L_.check(L_.load().rtfs_longform_overlap_add_many_f32(L_.ptr(y), L_.ptr(out), L_.ptr(tab), R, p["rows"], p["floats"], n_src, window, hop,
                                                          L_.stream_of(y)), "rtfs_longform_overlap_add_many_f32")
    return host(out), p


def blocks(flat, p, n_src):
    return [flat[o:o + n_src * L].reshape(n_src, L) for o, L in zip(p["off"], p["L"])]


@pytest.mark.parametrize("n_src", [1, 2])
@pytest.mark.parametrize("window,hop", PLANS + [(5120, 1920)])
def test_overlap_add_kernel_vs_oracle(n_src, window, hop):
    rng = np.random.RandomState(window + hop + n_src)
    worst = 0.0
    for Ls in length_mixes(window, hop):
        S = MO.plan(Ls, [1] * len(Ls), window, hop, n_src)["rows"]
        y = rng.randn(S, n_src, window).astype(np.float32)
        SENTINEL = -12345.0
        flat, p = ola_hip(dev(y), Ls, window, hop, fill=SENTINEL)
        want = MO.overlap_add(y, Ls, window, hop)
        written = np.zeros(p["floats"], bool)
        for r, (got, L) in enumerate(zip(blocks(flat, p, n_src), Ls)):
            rows = y[p["row0"][r]:p["row0"][r] + p["N"][r]]
            err, bound = float(np.abs(got - want[r]).max()), ola_bound(window, hop, rows)
            worst = max(worst, err / bound)
            assert np.isfinite(got).all() and err <= bound, f"recording {r} L {L} n_src {n_src} window {window} hop {hop}: {err:.3e} > {bound:.3e}"
            written[p["off"][r]:p["off"][r] + n_src * L] = True
        assert np.all(flat[~written] == SENTINEL), "a store landed in the padding between two recordings"
    print(f"[many] overlap-add window {window} hop {hop} n_src {n_src}: worst error {worst:.3f} of the bound")


# ---------------------------------------------------------------- 3. partition of unity
def test_frame_then_overlap_add_is_the_identity():
    rng = np.random.RandomState(5)
    for window, hop in PLANS + [(5120, 1920)]:
        Ls = edge_lengths(window, hop)
        xs = [rng.randn(L).astype(np.float32) for L in Ls]
        xw, _ = frame_hip([dev(x) for x in xs], [dev(np.zeros((512, 3), np.float32)) for _ in Ls], window, hop)
        flat, p = ola_hip(xw.view(-1, 1, window), Ls, window, hop)
        for r, got in enumerate(blocks(flat, p, 1)):
            assert np.abs(got[0] - xs[r]).max() <= ola_bound(window, hop, xs[r]), (window, hop, r)
            if hop == window:
                assert np.array_equal(got[0], xs[r]), (window, r)  # concatenation: weights 1, one window per sample


# ---------------------------------------------------------------- 4. composition
def test_separate_many_is_the_overlap_add_of_forward_on_the_pooled_windows():
    m = model()
    window, hop, max_batch = 5120, 2560, 5
    Ls = [12000, 5120, 700, 20001, 5121]
    Tvs = [-(-L // SPF) for L in Ls]
    xs, vs = [], []
    for r, (L, Tv) in enumerate(zip(Ls, Tvs)):
        w, e = make_inputs(1, L, Tv, 31 + r)
        xs.append(w[0]); vs.append(e[0])
    wavs, embs = [dev(x) for x in xs], [dev(v) for v in vs]
    res = m.separate_many(wavs, embs, window=window, hop=hop, max_batch=max_batch)
    got = [host(t) for t in res]
    p = MO.plan(Ls, Tvs, window, hop)
    S = p["rows"]
    assert S == 15 and p["row0"] == [0, 4, 5, 6, 13]  # chunks of 5 straddle recordings 0|1, 2|3 and 3|4
    assert [tuple(g.shape) for g in got] == [(1, L) for L in Ls]
    # the results are views into one flat output, each block on a 128-byte line
    base = res[0].data_ptr()
    assert [t.data_ptr() - base for t in res] == [4 * o for o in p["off"]] and base % 128 == 0
    xw, vw = MO.frame(xs, vs, window, hop)
    with torch.no_grad():  # the same chunks: 5, 5, 5
        y = np.concatenate([host(m(dev(xw[c:c + max_batch]), dev(vw[c:c + max_batch]))) for c in range(0, S, max_batch)])
    want = MO.overlap_add(y, Ls, window, hop)
    bound = ola_bound(window, hop, y)
    for r, L in enumerate(Ls):
        err = float(np.abs(got[r] - want[r]).max())
        alone = host(m.separate_long(wavs[r], embs[r][None], window=window, hop=hop))[0]
        e = rel_err(got[r], alone)
        print(f"[many] composition recording {r} L {L} N {p['N'][r]}: max abs err {err:.3e}, bound {bound:.3e}; "
              f"vs separate_long alone: max-rel {e:.3e} (expected about 1e-6)")
        assert np.isfinite(got[r]).all() and err <= bound, (r, err, bound)
        assert e <= 1e-4, (r, e)


# ---------------------------------------------------------------- 5. against the reference-pinned oracle of the forward
def test_small_case_vs_reference_pinned_oracle():
    from oracle import rtfs_oracle as O
    window, hop = 5120, 2560
    Ls, Tvs = [12000, 3000], [19, 5]
    sd = make_state_dict(spec_R4(), 0)
    xs, vs = [], []
    for r, (L, Tv) in enumerate(zip(Ls, Tvs)):
        w, e = make_inputs(1, L, Tv, 41 + r)
        xs.append(w[0]); vs.append(e[0])
    got = [host(t) for t in model().separate_many([dev(x) for x in xs], [dev(v) for v in vs], window=window, hop=hop)]
    xw, vw = MO.frame(xs, vs, window, hop)
    y = np.concatenate([O.avnet_forward(xw[i:i + 1], vw[i:i + 1], sd, repeats=4) for i in range(xw.shape[0])])
    want = MO.overlap_add(y, Ls, window, hop)
    for r, L in enumerate(Ls):
        e = rel_err(got[r], want[r])
        print(f"[many] window {window} hop {hop} recording {r} L {L} Tv {Tvs[r]} R4 vs oracle windows: max-rel {e:.3e}")
        assert got[r].shape == (1, L) and np.isfinite(got[r]).all() and e <= 1e-4, (r, e)


# ---------------------------------------------------------------- 6. System
def test_system_separate_many_groups_equal_video_lengths():
    import rtfs_net_amd as R
    from oracle import video_oracle as V
    s = R.System(audio_model=model(), video_model=video_model()).eval()
    Ls, Tvs = [9000, 5200, 7001], [14, 9, 14]
    wavs = [dev(make_inputs(1, L, Tv, 71 + r)[0][0]) for r, (L, Tv) in enumerate(zip(Ls, Tvs))]
    lips = [dev(V.make_video_input(1, Tv, 75 + r))[0] for r, Tv in enumerate(Tvs)]
    assert [tuple(t.shape) for t in lips] == [(1, Tv, 88, 88) for Tv in Tvs]
    kw = dict(window=5120, hop=2560, max_batch=4)
    got = [host(t) for t in s.separate_many(wavs, lips, **kw)]
    with torch.no_grad():
        embs = [video_model()(l[None])[0] for l in lips]  # track by track
    want = [host(t) for t in model().separate_many(wavs, embs, **kw)]
    for r, L in enumerate(Ls):
        e = rel_err(got[r], want[r])
        print(f"[many] System.separate_many recording {r} L {L} Tv {Tvs[r]} vs embeddings track by track: max-rel {e:.3e}")
        assert got[r].shape == (1, L) and np.isfinite(got[r]).all() and e <= 1e-4, (r, e)


def test_system_separate_recordings_equals_separate_recording_one_by_one():
    import rtfs_net_amd as R
    s = R.System(audio_model=model(), video_model=video_model()).eval()
    rates, L16, Tvs = [48000, 16000], [6000, 7003], [10, 11]
    wavs = []
    for r, (fs, L, Tv) in enumerate(zip(rates, L16, Tvs)):
        w = make_inputs(1, L, Tv, 91 + r)[0][0]
        wavs.append(dev(np.repeat(w, fs // 16000).astype(np.float32)))  # a recording at fs with the level of the separator's test inputs
    rois = [dev(np.random.RandomState(17 + r).randint(0, 256, (Tv, 96, 96)).astype(np.uint8)) for r, Tv in enumerate(Tvs)]
    kw = dict(window=5120, hop=2560)
    got = [host(t) for t in s.separate_recordings(wavs, rates, rois, **kw)]
    for r, L in enumerate(L16):
        want = host(s.separate_recording(wavs[r], rates[r], rois[r], **kw))[0]
        e = rel_err(got[r], want)
        print(f"[many] System.separate_recordings recording {r} at {rates[r]} Hz vs separate_recording: max-rel {e:.3e}")
        assert got[r].shape == want.shape == (1, L) and np.isfinite(got[r]).all() and e <= 1e-4, (r, e)


# ---------------------------------------------------------------- 7. poisoned memory
FORWARD_CASES = "test_framing or test_overlap_add or test_frame_then or test_separate_many_is or test_small_case or test_system"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's forward cases in a fresh child process per pattern, with every workspace / output a C call fills poisoned
    (tests/test_hip_poisoned.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_many.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
