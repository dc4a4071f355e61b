"""Host side of pooled separation (AVNet.separate_many, System.separate_many, rtfs_longform_many_plan) against tests/many_oracle.py: the
plan arithmetic (rows, offsets, padding) at the edge lengths, the refusals in C and in Python, the CPU-tensor path against "oracle pooled
windows -> forward_modular -> oracle overlap-add", R = 1 against separate_long bit for bit, and System's grouping of lip tracks by Tv.
None of it touches a device.

As in tests/test_longform_host.py the package has no CPU arithmetic of its own, so the CPU-path tests give the model a
``forward_modular``: the numpy oracle of the reference forward where values matter, a cheap row-wise function where only bits do."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import longform_oracle as LO
from tests import many_oracle as MO

ERR_SHAPE, ERR_ARG = -1, -4
SPF = 640
PLANS = [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640), (5120, 1920), (32000, 16000)]


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def edge_lengths(window, hop):
    return [3, 7, window - 1, window, window + 1, window + hop - 1, window + hop + 1, window + 3 * hop - 1, window + 3 * hop + 1]


def c_plan(Ls, Tvs, window, hop, n_src, with_table=True):
    R = len(Ls)
    La, Ta = (ctypes.c_longlong * max(R, 1))(*Ls), (ctypes.c_longlong * max(R, 1))(*Tvs)
    rows, floats = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    table = (ctypes.c_longlong * (5 * max(R, 1)))() if with_table else None
    rc = lib().rtfs_longform_many_plan(La, Ta, R, window, hop, n_src, table, ctypes.byref(rows), ctypes.byref(floats))
    return rc, rows.value, floats.value, (list(table) if with_table else None)


def length_mixes(window, hop):
    """The edge lengths in order, reversed, and shuffled with repeats: every length meets every position and neighbour."""
    e = edge_lengths(window, hop)
    rng = np.random.RandomState(window + hop)
    return [e, e[::-1], [e[i] for i in rng.randint(0, len(e), 14)], [e[3]], [e[0]]]


def test_plan_arithmetic_against_the_oracle():
    for window, hop in PLANS:
        for Ls in length_mixes(window, hop):
            frames = [-(-L // SPF) for L in Ls]
            Tvs = [(1, max(1, f - 2), f, f + 3)[i % 4] for i, f in enumerate(frames)]
            for n_src in (1, 2, 3):
                want = MO.plan(Ls, Tvs, window, hop, n_src)
                rc, rows, floats, table = c_plan(Ls, Tvs, window, hop, n_src)
                assert rc == 0 and rows == want["rows"] and floats == want["floats"], (window, hop, Ls, n_src)
                assert table == MO.table(want), (window, hop, Ls, n_src)
                # the sizing call of the two-call protocol gives the same sizes and needs no table
                assert c_plan(Ls, Tvs, window, hop, n_src, with_table=False)[:3] == (0, rows, floats)
                # per recording the single-recording plan, rows contiguous in recording order
                R = len(Ls)
                assert table[R:2 * R] == [LO.plan(L, Tv, window, hop) for L, Tv in zip(Ls, Tvs)]
                assert table[0] == 0 and all(table[r + 1] == table[r] + table[R + r] for r in range(R - 1))
    assert lib().rtfs_longform_many_plan((ctypes.c_longlong * 1)(700), (ctypes.c_longlong * 1)(2), 1, 2560, 1280, 1, None, None, None) == 0


def test_output_blocks_are_line_aligned_and_disjoint():
    for window, hop in PLANS:
        for Ls in length_mixes(window, hop):
            for n_src in (1, 2, 3):
                rc, rows, floats, table = c_plan(Ls, [1] * len(Ls), window, hop, n_src)
                R = len(Ls)
                off = table[4 * R:]
                assert rc == 0 and off[0] == 0 and floats % MO.ALIGN == 0
                end = 0
                for r in range(R):
                    assert off[r] * 4 % 128 == 0 and off[r] >= end, (Ls, n_src, r)  # starts on a line, after the previous block
                    end = off[r] + n_src * Ls[r]
                    assert r + 1 == R or off[r + 1] - end < MO.ALIGN  # padding below one line
                assert end <= floats < end + MO.ALIGN


def test_plan_refusals_agree_between_c_and_oracle():
    bad = [([48000], [75], 32001, 16000, 1), ([48000], [75], 32000, 16001, 1), ([48000], [75], 32000, 0, 1), ([48000], [75], 32000, 32640, 1),
           ([48000], [75], 0, 0, 1), ([48000], [75], 1000, 500, 1), ([48000, 0], [75, 75], 32000, 16000, 1),
           ([48000, 3], [75, 0], 32000, 16000, 1), ([48000, -1], [75, 75], 32000, 16000, 1), ([], [], 32000, 16000, 1),
           ([48000], [75], 32000, 16000, 0), ([2 ** 31], [75], 32000, 16000, 1), ([48000], [2 ** 31], 32000, 16000, 1)]
    for Ls, Tvs, window, hop, n_src in bad:
        assert c_plan(Ls, Tvs, window, hop, n_src)[0] == ERR_ARG, (Ls, Tvs, window, hop, n_src)
        with pytest.raises(ValueError):
            MO.plan(Ls, Tvs, window, hop, n_src)
    # sum(N) past int32: 3355444 windows of 640 samples per recording of 2^31 - 1 samples
    n = LO.plan(2 ** 31 - 1, 1, 640, 640)
    R = (2 ** 31 - 1) // n + 1
    assert c_plan([2 ** 31 - 1] * R, [1] * R, 640, 640, 1)[0] == ERR_SHAPE
    assert c_plan([2 ** 31 - 1] * (R - 1), [1] * (R - 1), 640, 640, 1)[:2] == (0, n * (R - 1))
    with pytest.raises(ValueError):
        MO.plan([2 ** 31 - 1] * R, [1] * R, 640, 640)
    assert lib().rtfs_longform_many_plan(None, None, 1, 2560, 1280, 1, None, None, None) == ERR_ARG


def _model(repeats=2, cell="SRU"):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    return R.AVNet(print_macs=False, **copy.deepcopy(audionet_config(repeats, cell))).eval()


def test_separate_many_refusals():
    m = _model()
    wav, emb = torch.zeros(48000), torch.zeros(512, 75)
    for kw in (dict(window=32001), dict(hop=16001), dict(hop=0), dict(hop=-640), dict(window=32000, hop=32640), dict(window=0),
               dict(max_batch=0), dict(window=1000, hop=500), dict(window=206 * 640)):
        with pytest.raises(ValueError):
            m.separate_many([wav], [emb], **kw)
    with pytest.raises(ValueError):
        _model(2, "LSTM").separate_many([wav], [emb], window=101 * 640)
    with pytest.raises(ValueError):
        _model(2, "GRU").separate_many([wav], [emb])
    bad = [([], []),  # an empty list
           ([wav, wav], [emb]),  # lists of different lengths
           ([wav, torch.zeros(0)], [emb, emb]),  # L < 1
           ([wav], [torch.zeros(512, 0)]),  # Tv < 1
           ([torch.zeros(2, 48000)], [emb]),  # (2,L)
           ([torch.zeros(1, 1, 48000)], [emb]),  # rank 3
           ([wav], [torch.zeros(1, 512, 75)]),  # rank 3
           ([wav], [torch.zeros(75, 512)]),  # wrong channel count
           ([wav, torch.zeros(3, device="meta")], [emb, emb]),  # mixtures on two devices
           ([wav], [torch.zeros(512, 75, device="meta")]),  # a mixture and its video on two devices
           ([wav.double()], [emb]), ([wav], [emb.half()]), ([wav.to(torch.int32)], [emb]),  # float32 only
           ([wav], [None]), ([wav], 3)]
    for wavs, embs in bad:
        with pytest.raises(ValueError):
            m.separate_many(wavs, embs)
    # sum(N) past int32, from tensors that own one float each
    long_wav, one_frame = torch.zeros(1).expand(2 ** 31 - 1), torch.zeros(512, 1)
    R = (2 ** 31 - 1) // LO.plan(2 ** 31 - 1, 1, 640, 640) + 1
    with pytest.raises(ValueError):
        m.separate_many([long_wav] * R, [one_frame] * R, window=640, hop=640)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.separate_many([wav], [emb])
    m.eval()
    with pytest.raises(RuntimeError, match="CPU tensor"):  # right arguments: the CPU path reaches forward_modular, which has no CPU kernels
        m.separate_many([wav, wav[:7]], [emb, emb[:, :1]])


def test_cpu_path_against_oracle_composition():
    """separate_many on CPU tensors == oracle pooled windows -> forward_modular -> oracle overlap-add per recording (window 2560, hop
    1280, chunks of 3 that straddle the recordings)."""
    from oracle import rtfs_oracle as O
    from oracle.params import load_spec, make_inputs, make_state_dict
    m = _model(2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    calls = []

    def forward_modular(wav, emb):
        calls.append(int(wav.shape[0]))  # row by row: a window's result must not depend on the chunk it arrives in
        rows = [O.avnet_forward(wav[i:i + 1].numpy(), emb[i:i + 1].numpy(), sd, repeats=2) for i in range(wav.shape[0])]
        return torch.from_numpy(np.concatenate(rows).astype(np.float32))

    m.forward_modular = forward_modular
    window, hop, max_batch = 2560, 1280, 3
    Ls, Tvs = [6000, 2560, 1400, 5121], [10, 4, 1, 17]
    xs, vs = [], []
    for r, (L, Tv) in enumerate(zip(Ls, Tvs)):
        w, e = make_inputs(1, L, Tv, 5 + r)
        xs.append(w[0]); vs.append(e[0])
    wavs = [torch.from_numpy(x) for x in xs]
    wavs[1] = wavs[1][None]  # (1,L) is taken as well
    got = m.separate_many(wavs, [torch.from_numpy(v) for v in vs], window=window, hop=hop, max_batch=max_batch)
    p = MO.plan(Ls, Tvs, window, hop)
    S = p["rows"]
    chunks = list(calls)
    assert chunks == [3] * (S // 3) + ([S % 3] if S % 3 else []), chunks
    xw, vw = MO.frame(xs, vs, window, hop)
    assert xw.shape == (S, window)
    y = np.concatenate([forward_modular(torch.from_numpy(xw[i:i + 1]), torch.from_numpy(vw[i:i + 1])).numpy() for i in range(S)])
    want = MO.overlap_add(y, Ls, window, hop)
    # the windows are the same float32 values on both sides; then <= ceil(window / hop) float32 multiply-adds and a division per sample
    bound = 4 * -(-window // hop) * 2.0 ** -23 * np.abs(y).max()
    assert isinstance(got, list) and len(got) == len(Ls)
    for r, L in enumerate(Ls):
        assert got[r].shape == (1, L) and got[r].dtype == torch.float32
        err = float(np.abs(got[r].numpy() - want[r]).max())
        print(f"[many host] recording {r} L {L} N {p['N'][r]}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (r, err, bound)


def _cheap_forward(n_src):
    def forward_modular(wav, emb):  # row-wise, so a window's value does not depend on its chunk
        base = torch.tanh(wav) * (1.0 + emb.mean(dim=(1, 2)))[:, None]
        return torch.stack([base * (s + 1) for s in range(n_src)], dim=1)
    return forward_modular


@pytest.mark.parametrize("L,Tv", [(7, 1), (2560, 4), (2561, 3), (9001, 20)])
def test_one_recording_equals_separate_long_bit_for_bit(L, Tv):
    m = _model()
    m.forward_modular = _cheap_forward(1)
    rng = np.random.RandomState(L)
    wav, emb = torch.from_numpy(rng.randn(L).astype(np.float32)), torch.from_numpy(rng.randn(512, Tv).astype(np.float32))
    for kw in (dict(window=2560, hop=1280, max_batch=2), dict(window=2560, hop=2560), dict(window=1280, hop=640, max_batch=32)):
        got = m.separate_many([wav], [emb], **kw)
        want = m.separate_long(wav, emb[None], **kw)
        assert len(got) == 1 and got[0].shape == (1, L)
        assert np.array_equal(got[0].numpy(), want[0].numpy()), kw


def test_pooled_recordings_equal_separate_long_one_by_one_on_cpu():
    """Chunks that straddle recordings change nothing when the model is row-wise: every result equals separate_long on that recording."""
    m = _model()
    m.forward_modular = _cheap_forward(1)
    rng = np.random.RandomState(11)
    Ls, Tvs = [3, 2561, 1280, 4000, 7], [1, 9, 2, 5, 3]
    wavs = [torch.from_numpy(rng.randn(L).astype(np.float32)) for L in Ls]
    embs = [torch.from_numpy(rng.randn(512, Tv).astype(np.float32)) for Tv in Tvs]
    got = m.separate_many(wavs, embs, window=1280, hop=640, max_batch=4)
    for r in range(len(Ls)):
        want = m.separate_long(wavs[r], embs[r][None], window=1280, hop=640)[0]
        assert np.array_equal(got[r].numpy(), want.numpy()), r


class _CountingVideo(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, lips):
        assert lips.ndim == 5 and lips.shape[1] == 1 and tuple(lips.shape[3:]) == (88, 88) and not torch.is_grad_enabled()
        self.calls.append((int(lips.shape[0]), int(lips.shape[2])))
        # one value per track and frame, so a swapped or time-joined track shows
        return lips.mean(dim=(3, 4)).expand(-1, 512, -1).contiguous()


class _RecordingAudio(torch.nn.Module):
    def separate_many(self, wavs, embs, **kw):
        self.seen = (list(wavs), list(embs), kw)
        return ["result"]


def test_system_groups_tracks_by_tv_and_forwards_keywords():
    import rtfs_net_amd as R
    video, audio = _CountingVideo(), _RecordingAudio()
    s = R.System(audio_model=audio, video_model=video)
    Tvs = [5, 3, 5, 7, 3, 5]
    wavs = [torch.zeros(100 * (r + 1)) for r in range(len(Tvs))]
    lips = [torch.full((1, Tv, 88, 88), float(r + 1)) + torch.arange(Tv, dtype=torch.float32)[None, :, None, None] for r, Tv in enumerate(Tvs)]
    assert s.separate_many(wavs, lips, window=2560, hop=640, max_batch=7) == ["result"]
    assert sorted(video.calls) == [(1, 7), (2, 3), (3, 5)]  # once per group of equal Tv, the group stacked as a batch
    seen_wavs, embs, kw = audio.seen
    assert kw == dict(window=2560, hop=640, max_batch=7)
    assert all(a is b for a, b in zip(seen_wavs, wavs))
    for r, Tv in enumerate(Tvs):  # every track got its own embedding back, in input order
        assert tuple(embs[r].shape) == (512, Tv)
        assert torch.equal(embs[r][0], float(r + 1) + torch.arange(Tv, dtype=torch.float32))
    for bad in ([torch.zeros(5, 88, 88)], [torch.zeros(2, 5, 88, 88)], [], [lips[0], lips[1]]):
        with pytest.raises(ValueError):
            s.separate_many([wavs[0]], bad)
    # without a video model the slot holds embeddings and goes straight through
    s2 = R.System(audio_model=audio)
    e = [torch.zeros(512, 4)]
    assert s2.separate_many([wavs[0]], e, hop=1280) == ["result"]
    assert audio.seen[1][0] is e[0] and audio.seen[2] == dict(hop=1280)
    assert callable(s.separate_recordings)
