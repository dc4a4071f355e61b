"""Host side of a different number of faces per mixture (AVNet.separate_speakers(counts=...), rtfs_separator_targets_f32,
AVNet.separate_many_speakers, rtfs_longform_many_speakers_plan) against tests/targets_oracle.py: workspace arithmetic, the refusals of
the C entry and of the Python entries, the pooled plan, the chunker, the CPU-tensor route with a row-wise model, System's grouping.  None
of it touches a device."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import many_oracle as MO
from tests import targets_oracle as TO

ERR_SHAPE, ERR_ARG = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rtfs_separator_targets_workspace_bytes", "rtfs_separator_targets_f32", "rtfs_longform_many_speakers_plan",
           "rtfs_longform_frame_many_speakers_f32", "rtfs_longform_overlap_add_many_speakers_f32"]


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*v)


def ws_bytes(counts, L=32000, Tv=50, split=0, B=None):
    return lib().rtfs_separator_targets_workspace_bytes(ints(counts), len(counts) if B is None else B, L, Tv, split)


def test_new_symbols_are_in_the_header_and_the_binding_table():
    from rtfs_net_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib(), name)


def test_workspace_grows_with_the_targets_not_with_the_mixtures_alone():
    L_ = lib()
    for L, Tv, split in [(4096, 7, 0), (5000, 9, 0), (32000, 50, 2), (8000, 12, 3)]:
        for B in (1, 3, 16, 20):
            for K in (1, 2, 5, 16):  # equal counts: the fixed-K query
                assert ws_bytes([K] * B, L, Tv, split) == L_.rtfs_separator_speakers_workspace_bytes(B, K, L, Tv, split) > 0, (B, K, L, split)
            one = ws_bytes([1] * B, L, Tv, split)
            more = ws_bytes([1] * (B - 1) + [2], L, Tv, split)
            assert more > one, (B, L, split)  # one more target, the same mixtures
            assert ws_bytes([1] * (B - 1) + [3], L, Tv, split) - more == more - one  # and linearly in N within a part
    # 16 mixtures with counts cycling 1 .. 4 (40 targets): less than the 40-row forward and than the padded K = 4 call
    cyc = [1 + b % 4 for b in range(16)]
    assert ws_bytes(cyc) < L_.rtfs_separator_workspace_bytes_ex(40, 32000, 50, 0)
    assert ws_bytes(cyc) < L_.rtfs_separator_speakers_workspace_bytes(16, 4, 32000, 50, 0)
    # where the targets sit matters only through the batch parts
    assert ws_bytes([3, 1, 2]) == ws_bytes([1, 2, 3])


def test_workspace_query_returns_0_for_bad_arguments():
    assert lib().rtfs_separator_targets_workspace_bytes(None, 2, 32000, 50, 0) == 0
    for counts, kw in [([2, 0], {}), ([2, 17], {}), ([-1], {}), ([2, 2], dict(split=9)), ([2, 2], dict(split=-1)), ([2, 2], dict(B=0)),
                       ([2, 2], dict(L=128)), ([2, 2], dict(Tv=0))]:
        assert ws_bytes(counts, **kw) == 0, (counts, kw)


def test_targets_entry_refuses_bad_arguments_before_any_device_call():
    L_ = lib()
    fake = ctypes.c_void_p(256)  # never dereferenced: every refusal below comes before the first device call
    ws = ctypes.c_void_p(4096)
    good = ints([1, 3, 2])

    def call(counts=good, mix_of=fake, N=6, repeats=4, wav=fake, out=fake, rnn_kind=0, split=0, B=3, L=32000, Tv=50):
        return L_.rtfs_separator_targets_f32(wav, fake, counts, mix_of, fake, fake, fake, fake, fake, fake, out, B, N, L, Tv, repeats, ws,
                                             1 << 20, None, None, rnn_kind, split)

    assert call(counts=None) == ERR_ARG
    assert call(mix_of=None) == ERR_ARG
    assert call(counts=ints([1, 0, 5])) == ERR_ARG
    assert call(counts=ints([1, 17, 2]), N=20) == ERR_ARG
    assert call(N=5) == ERR_ARG
    assert call(N=7) == ERR_ARG
    assert call(repeats=1) == ERR_ARG
    assert call(wav=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(rnn_kind=2) == ERR_ARG
    assert call(split=9) == ERR_ARG
    assert call(B=0) == ERR_ARG
    assert call(L=128) == ERR_ARG
    assert call(Tv=0) == ERR_ARG
    assert call(L=513 * 2 * 128) == ERR_SHAPE  # past the SRU cell's fused length
    assert call(L=251 * 2 * 128, rnn_kind=1) == ERR_SHAPE  # past the LSTM cell's
    assert call() == -2  # right arguments: the next check is the workspace (4096 bytes), still before the device


# ---------------------------------------------------------------- the pooled plan
PLANS = [(2560, 2560), (2560, 1280), (1280, 640), (6400, 3200)]


def c_plan(Ls, Tvs, Ks, window, hop, with_table=True):
    R = len(Ls)
    arr = lambda v: (ctypes.c_longlong * max(R, 1))(*v)
    rows, targets, floats = ctypes.c_longlong(-1), ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    table = (ctypes.c_longlong * (7 * max(R, 1)))() if with_table else None
    rc = lib().rtfs_longform_many_speakers_plan(arr(Ls), arr(Tvs), None if Ks is None else arr(Ks), R, window, hop, table,
                                                ctypes.byref(rows), ctypes.byref(targets), ctypes.byref(floats))
    return rc, rows.value, targets.value, floats.value, (list(table) if with_table else None)


def test_many_speakers_plan_against_the_oracle():
    rng = np.random.RandomState(3)
    for window, hop in PLANS:
        edge = [1, 3, 7, window - 1, window, window + 1, window + hop - 1, window + hop + 1, window + 3 * hop + 1]
        for Ls in (edge, edge[::-1], [edge[i] for i in rng.randint(0, len(edge), 12)], [edge[4]], [1]):
            Tvs = [max(1, -(-L // 640) + (i % 3) - 1) for i, L in enumerate(Ls)]
            for Ks in ([1] * len(Ls), [1 + (5 * i) % 16 for i in range(len(Ls))], [16] * len(Ls), [int(k) for k in rng.randint(1, 5, len(Ls))]):
                want = TO.plan(Ls, Tvs, Ks, window, hop)
                rc, rows, targets, floats, table = c_plan(Ls, Tvs, Ks, window, hop)
                assert rc == 0 and (rows, targets, floats) == (want["rows"], want["targets"], want["floats"]), (window, hop, Ls, Ks)
                assert table == TO.table(want), (window, hop, Ls, Ks)
                assert c_plan(Ls, Tvs, Ks, window, hop, with_table=False)[:4] == (0, rows, targets, floats)
                R = len(Ls)
                off, trow0 = table[4 * R:5 * R], table[6 * R:]
                # target rows: contiguous, K_r per window; blocks: (K_r, L_r) on 128-byte lines, padding below one line
                assert trow0[0] == 0 and all(trow0[r + 1] == trow0[r] + table[R + r] * Ks[r] for r in range(R - 1))
                end = 0
                for r in range(R):
                    assert off[r] % MO.ALIGN == 0 and 0 <= off[r] - end < MO.ALIGN, (Ls, Ks, r)
                    end = off[r] + Ks[r] * Ls[r]
                assert end <= floats < end + MO.ALIGN and floats % MO.ALIGN == 0
            # K all 1: the first five columns are rtfs_longform_many_plan's
            p1 = MO.plan(Ls, Tvs, window, hop, 1)
            assert c_plan(Ls, Tvs, [1] * len(Ls), window, hop)[4][:5 * len(Ls)] == MO.table(p1)


def test_many_speakers_plan_refusals():
    ok = ([48000, 7], [75, 1], [2, 3], 32000, 16000)
    assert c_plan(*ok)[0] == 0
    bad = [([48000, 7], [75, 1], [2, 0], 32000, 16000), ([48000, 7], [75, 1], [17, 1], 32000, 16000), ([48000], [75], [-1], 32000, 16000),
           ([48000], [75], None, 32000, 16000), ([48000], [75], [1], 32001, 16000), ([48000], [75], [1], 32000, 0),
           ([48000, 0], [75, 75], [1, 1], 32000, 16000), ([48000], [0], [1], 32000, 16000), ([], [], [], 32000, 16000),
           ([2 ** 31], [75], [1], 32000, 16000)]
    for Ls, Tvs, Ks, window, hop in bad:
        assert c_plan(Ls, Tvs, Ks, window, hop)[0] == ERR_ARG, (Ls, Tvs, Ks, window, hop)
        if Ks is not None:
            with pytest.raises(ValueError):
                TO.plan(Ls, Tvs, Ks, window, hop)
    # sum(N K) past int32 while sum(N) is not: 16 tracks on recordings of 2^31 - 1 samples in windows of 640
    from tests import longform_oracle as LO
    n = LO.plan(2 ** 31 - 1, 1, 640, 640)
    R = (2 ** 31 - 1) // (16 * n) + 1
    assert R * n <= 2 ** 31 - 1
    assert c_plan([2 ** 31 - 1] * R, [1] * R, [16] * R, 640, 640)[0] == ERR_SHAPE
    assert c_plan([2 ** 31 - 1] * (R - 1), [1] * (R - 1), [16] * (R - 1), 640, 640)[:3] == (0, n * (R - 1), 16 * n * (R - 1))


def test_chunker():
    from rtfs_net_amd.models import chunk_windows
    # K = [2,1,3,1] on one window each, at most 5 targets a chunk: [2,1] closes because 3 more would make 6
    assert chunk_windows([2, 1, 3, 1], 5) == [(0, 2, 0, 3), (2, 4, 3, 7)]
    # a window with more targets than max_batch goes alone, and its neighbours do not join it
    assert chunk_windows([1, 7, 1, 1], 5) == [(0, 1, 0, 1), (1, 2, 1, 8), (2, 4, 8, 10)]
    assert chunk_windows([7], 5) == [(0, 1, 0, 7)]
    assert chunk_windows([], 5) == []
    rng = np.random.RandomState(0)
    for _ in range(50):
        counts = [int(c) for c in rng.randint(1, 17, rng.randint(1, 40))]
        mb = int(rng.randint(1, 40))
        got = chunk_windows(counts, mb)
        assert got == TO.chunks(counts, mb), (counts, mb)
        assert got[0][0] == 0 and got[-1][1] == len(counts) and all(a[1] == b[0] and a[3] == b[2] for a, b in zip(got, got[1:]))
        for w0, w1, t0, t1 in got:
            assert t1 - t0 == sum(counts[w0:w1]) and (t1 - t0 <= mb or w1 - w0 == 1)
    # all K = 1: the chunks of separate_many
    assert chunk_windows([1] * 7, 3) == [(0, 3, 0, 3), (3, 6, 3, 6), (6, 7, 6, 7)]


# ---------------------------------------------------------------- Python entries
def _model(repeats=2, cell="SRU"):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    return R.AVNet(print_macs=False, **copy.deepcopy(audionet_config(repeats, cell))).eval()


def test_separate_speakers_counts_errors_before_any_gpu_call():
    m = _model()
    wav, lips = torch.zeros(3, 4096), torch.zeros(6, 512, 7)
    for counts in ([1, 3], [1, 3, 1, 1], [1, 3, 3], [0, 3, 3], [1, 2, 2], "abc", 6, [6], [17, 1, 1]):
        with pytest.raises(ValueError):
            m.separate_speakers(wav, lips, counts=counts)
    with pytest.raises(ValueError):
        m.separate_speakers(wav, torch.zeros(3, 2, 512, 7), counts=[2, 2, 2])  # the fixed-K layout
    with pytest.raises(ValueError):
        m.separate_speakers(torch.zeros(3, 2, 4096), lips, counts=[1, 3, 2])
    m.n_src = 2
    with pytest.raises(ValueError, match="n_src"):
        m.separate_speakers(wav, lips, counts=[1, 3, 2])
    m.n_src = 1
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.separate_speakers(wav, lips, counts=[1, 3, 2])
    m.eval()
    with pytest.raises(RuntimeError, match="CPU tensor"):  # right arguments: the next check is the device
        m.separate_speakers(wav, lips, counts=(1, 3, 2))
    import rtfs_net_amd as R
    s = R.System(audio_model=m)
    with pytest.raises(ValueError):
        s.separate_speakers(wav, lips, counts=[1, 3, 3])


def test_separate_many_speakers_refusals():
    m = _model()
    wav, emb = torch.zeros(48000), torch.zeros(2, 512, 75)
    for kw in (dict(window=32001), dict(hop=16001), dict(hop=0), dict(window=32000, hop=32640), dict(max_batch=0), dict(window=206 * 640)):
        with pytest.raises(ValueError):
            m.separate_many_speakers([wav], [emb], **kw)
    with pytest.raises(ValueError):
        _model(2, "GRU").separate_many_speakers([wav], [emb])
    bad = [([], []), ([wav, wav], [emb]), ([wav, torch.zeros(0)], [emb, emb]), ([wav], [torch.zeros(2, 512, 0)]), ([torch.zeros(2, 48000)], [emb]),
           ([wav], [torch.zeros(512, 75)]),  # no track axis
           ([wav], [torch.zeros(0, 512, 75)]), ([wav], [torch.zeros(17, 512, 75)]),  # K outside 1 .. 16
           ([wav], [torch.zeros(2, 75, 512)]), ([wav], [torch.zeros(2, 512, 75, device="meta")]), ([wav.double()], [emb]), ([wav], [emb.half()]),
           ([wav], [None]), ([wav], 3)]
    for wavs, embs in bad:
        with pytest.raises(ValueError):
            m.separate_many_speakers(wavs, embs)
    m.n_src = 2
    with pytest.raises(ValueError, match="n_src"):
        m.separate_many_speakers([wav], [emb])
    m.n_src = 1
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.separate_many_speakers([wav], [emb])
    m.eval()
    with pytest.raises(RuntimeError, match="CPU tensor"):  # right arguments: the CPU path reaches forward_modular, which has no CPU kernels
        m.separate_many_speakers([wav, wav[:7]], [emb, emb[:1, :, :1]])


def _cheap_forward(calls=None):
    def forward_modular(wav, emb):  # row-wise, so a window's value does not depend on its chunk
        if calls is not None:
            calls.append(int(wav.shape[0]))
        return (torch.tanh(wav) * (1.0 + emb.mean(dim=(1, 2)))[:, None])[:, None]
    return forward_modular


def test_cpu_route_equals_separate_many_per_face_bit_for_bit():
    """window 1280, hop 640, K = 2,1,3,1, max_batch 5: chunks straddle recordings and close in the middle of one; with a row-wise model
    every [r][k] is separate_many on (mixtures[r], lips[r][k]) bit for bit, and the chunk sizes are the chunker's."""
    calls = []
    m = _model()
    m.forward_modular = _cheap_forward(calls)
    rng = np.random.RandomState(5)
    Ls, Tvs, Ks = [1, 1280, 2001, 4000], [1, 2, 3, 7], [2, 1, 3, 1]
    wavs = [torch.from_numpy(rng.randn(L).astype(np.float32)) for L in Ls]
    wavs[1] = wavs[1][None]
    lips = [torch.from_numpy(rng.randn(K, 512, Tv).astype(np.float32)) for K, Tv in zip(Ks, Tvs)]
    got = m.separate_many_speakers(wavs, lips, window=1280, hop=640, max_batch=5)
    p = TO.plan(Ls, Tvs, Ks, 1280, 640)
    assert calls == [t1 - t0 for _, _, t0, t1 in TO.chunks(TO.window_counts(p), 5)], calls
    assert any(w0 < p["row0"][r] < w1 for w0, w1, _, _ in TO.chunks(TO.window_counts(p), 5) for r in range(1, 4))  # a chunk straddles
    m.forward_modular = _cheap_forward()
    for r in range(4):
        assert got[r].shape == (Ks[r], Ls[r]) and got[r].dtype == torch.float32
        for k in range(Ks[r]):
            want = m.separate_many([wavs[r]], [lips[r][k]], window=1280, hop=640)[0][0]
            assert np.array_equal(got[r][k].numpy(), want.numpy()), (r, k)
    # K all 1: separate_many itself
    one = m.separate_many_speakers(wavs, [lp[:1] for lp in lips], window=1280, hop=640, max_batch=3)
    ref = m.separate_many(wavs, [lp[0] for lp in lips], window=1280, hop=640, max_batch=3)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(one, ref))


class _CountingVideo(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, lips):
        assert lips.ndim == 5 and lips.shape[1] == 1 and tuple(lips.shape[3:]) == (88, 88) and not torch.is_grad_enabled()
        self.calls.append((int(lips.shape[0]), int(lips.shape[2])))
        return lips.mean(dim=(3, 4)).expand(-1, 512, -1).contiguous()  # one value per track and frame


class _RecordingAudio(torch.nn.Module):
    def separate_many_speakers(self, wavs, embs, **kw):
        self.seen = ("many", list(wavs), list(embs), kw)
        return ["result"]

    def separate_speakers(self, wav, embs, counts=None):
        self.seen = ("batch", wav, embs, counts)
        return "batch result"


def test_system_runs_the_video_model_once_per_group_and_once_per_batch():
    import rtfs_net_amd as R
    video, audio = _CountingVideo(), _RecordingAudio()
    s = R.System(audio_model=audio, video_model=video)
    Tvs, Ks = [5, 3, 5, 3], [2, 1, 3, 2]
    wavs = [torch.zeros(100 * (r + 1)) for r in range(4)]
    lips = [torch.stack([torch.full((1, Tv, 88, 88), float(10 * r + k)) for k in range(K)]) for r, (Tv, K) in enumerate(zip(Tvs, Ks))]
    assert s.separate_many_speakers(wavs, lips, window=2560, max_batch=7) == ["result"]
    assert sorted(video.calls) == [(3, 3), (5, 5)]  # once per group of equal Tv, all tracks of the group as one batch
    _, seen_wavs, embs, kw = audio.seen
    assert kw == dict(window=2560, max_batch=7) and all(a is b for a, b in zip(seen_wavs, wavs))
    for r in range(4):  # every recording got its own tracks back, in order
        assert tuple(embs[r].shape) == (Ks[r], 512, Tvs[r])
        assert [float(embs[r][k, 0, 0]) for k in range(Ks[r])] == [float(10 * r + k) for k in range(Ks[r])]
    for bad in ([torch.zeros(1, 5, 88, 88)], [torch.zeros(2, 2, 5, 88, 88)], [], [lips[0], lips[1]]):
        with pytest.raises(ValueError):
            s.separate_many_speakers([wavs[0]], bad)
    # the batch entry: ONE video call on the N tracks
    video.calls.clear()
    wav = torch.zeros(2, 4096)
    assert s.separate_speakers(wav, torch.zeros(3, 1, 7, 88, 88), counts=[1, 2]) == "batch result"
    assert video.calls == [(3, 7)] and audio.seen[3] == (1, 2) and tuple(audio.seen[2].shape) == (3, 512, 7)
    with pytest.raises(ValueError):
        s.separate_speakers(wav, torch.zeros(3, 1, 7, 88, 88), counts=[2, 2])
    assert video.calls == [(3, 7)]  # refused before the video model ran
