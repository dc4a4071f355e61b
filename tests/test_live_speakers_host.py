"""Host side of live streaming with K faces per stream (AVNet.open_streams(speakers=K), SpeakerStreamPool,
AVNet.separate_long_speakers) against tests/live_speakers_oracle.py: every refusal before anything is allocated or launched and with
the counters unchanged, and the class end to end on CPU tensors with a cheap row-wise separator against the float64 streaming
overlap-add and against separate_long_speakers.  None of it touches a device."""
import numpy as np
import pytest
import torch

from tests import live_oracle as VO
from tests import live_speakers_oracle as SO
from tests.test_live_host import MODES, SPF, _model, lib


def _cheap(wav, emb):  # row-wise: a target's value depends on its window and its own lips only
    return (torch.tanh(wav) * (1.0 + 0.5 * torch.tanh(emb.mean(dim=(1, 2))))[:, None])[:, None]


def _cheap_np(xw, vw):
    return np.tanh(xw.astype(np.float64)) * (1.0 + 0.5 * np.tanh(vw.astype(np.float64).mean(axis=(1, 2))))[:, None]


def test_open_streams_with_one_speaker_is_the_plain_pool():
    import rtfs_net_amd as R
    m = _model()
    pool = m.open_streams(2, window=2560, hop=1280, speakers=1)
    assert type(pool) is R.StreamPool
    assert type(R.System(audio_model=m).open_streams(slots=1, window=1280, hop=640, speakers=1)) is R.StreamPool
    assert type(m.open_streams(2, window=2560, hop=1280, speakers=2)) is R.SpeakerStreamPool


def test_open_streams_refusals(monkeypatch):
    from rtfs_net_amd import _lib
    m = _model()

    def no_alloc(*a, **k):
        raise AssertionError("a refused open_streams allocated")

    monkeypatch.setattr(_lib, "empty", no_alloc)
    for kw in (dict(speakers=0), dict(speakers=17), dict(speakers=-1), dict(speakers=2.0), dict(speakers=True),
               dict(speakers=2, sample_rate=48000), dict(speakers=2, window=2561), dict(speakers=2, hop=0), dict(speakers=2, slots=0),
               dict(speakers=2, max_chunk=641), dict(speakers=2, max_batch=0),
               dict(speakers=16, window=2560, max_chunk=(1 << 20) // 640 * 640)):  # 16 * (window + max_chunk) > 2^24
        with pytest.raises(ValueError):
            m.open_streams(**dict(dict(slots=2, window=2560, hop=1280), **kw))
    with pytest.raises(ValueError, match="n_src"):
        _n_src2().open_streams(2, window=2560, hop=1280, speakers=2)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.open_streams(2, window=2560, hop=1280, speakers=2)
    m.eval()
    # the K-fold launch-size rule, at its edge: K C <= 2^24
    most = (1 << 24) // 4 // 640 * 640 - 2560
    assert lib().rtfs_live_speakers_sizes_ok(2560, 1280, most, 4) == 1 and lib().rtfs_live_speakers_sizes_ok(2560, 1280, most + 640, 4) == 0
    assert lib().rtfs_live_speakers_sizes_ok(2560, 1280, 2560, 0) == 0 and lib().rtfs_live_speakers_sizes_ok(2560, 1280, 2560, 17) == 0


def _n_src2():
    m = _model()
    m.n_src = 2
    return m


def test_separate_long_speakers_refusals(monkeypatch):
    from rtfs_net_amd import _lib
    m = _model()
    monkeypatch.setattr(_lib, "empty", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a refused call allocated")))
    x = torch.zeros(1, 6000)
    for wav, emb, kw in ((x, torch.zeros(1, 0, 512, 10), {}), (x, torch.zeros(1, 17, 512, 10), {}), (x, torch.zeros(1, 512, 10), {}),
                         (x, torch.zeros(2, 2, 512, 10), {}), (x, torch.zeros(1, 2, 256, 10), {}), (torch.zeros(1, 2, 6000), torch.zeros(1, 2, 512, 10), {}),
                         (x, torch.zeros(1, 2, 512, 10), dict(window=2561)), (x, torch.zeros(1, 2, 512, 10), dict(window=2560, hop=3200)),
                         (x, torch.zeros(1, 2, 512, 10), dict(max_batch=0)), (x, torch.zeros(1, 2, 512, 0), {})):
        with pytest.raises(ValueError):
            m.separate_long_speakers(wav, emb, **dict(dict(window=2560, hop=1280), **kw))
    with pytest.raises(ValueError, match="n_src"):
        _n_src2().separate_long_speakers(x, torch.zeros(1, 2, 512, 10), window=2560, hop=1280)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.separate_long_speakers(x, torch.zeros(1, 2, 512, 10), window=2560, hop=1280)
    m.eval()


def test_every_push_refusal_leaves_all_counters_unchanged():
    m = _model()
    m.forward_modular = _cheap
    pool = m.open_streams(3, window=2560, hop=1280, max_batch=2, speakers=2)
    a, v = torch.zeros(2000), torch.zeros(2, 512, 3)
    assert [tuple(t.shape) for t in pool.push([0, 2], [a, a], [v, [v[0], v[1]]])] == [(2, 0), (2, 0)]
    before = [pool.counters(s) for s in range(3)]
    assert before == [(2000, 3, 0, 0), (0, 0, 0, 0), (2000, 3, 0, 0)]
    t3, t2 = torch.zeros(512, 3), torch.zeros(512, 2)
    bad = [([1], [a], [[t3, t2]]), ([1], [a], [(t2, t3)]),  # tracks of different m
           ([1], [a], [[t3]]), ([1], [a], [[t3, t3, t3]]), ([1], [a], [torch.zeros(3, 512, 3)]), ([1], [a], [torch.zeros(1, 512, 3)]),
           ([1], [a], [t3]), ([1], [a], [[]]), ([1], [a], [3]),  # wrong track count / not K tracks
           ([3], [a], [v]), ([0, 0], [a, a], [v, v]), ([1.0], [a], [v]), ([0, 1], [a], [v, v]),
           ([1, 0], [a, torch.zeros(2561)], [v, v]), ([1, 0], [a, a], [v, torch.zeros(2, 512, 5)]),  # oversize, after a good slot
           ([0], [a], [torch.zeros(2, 3, 512)]), ([0], [a.double()], [v]), ([0], [a], [v.half()]), ([0], [a], [[t3, t3.double()]]),
           ([0], [a], [v.to("meta")]), ([0], [None], [v]), ([0], [a], [[t3, None]])]
    for ids, wavs, vids in bad:
        with pytest.raises(ValueError):
            pool.push(ids, wavs, vids)
        assert [pool.counters(s) for s in range(3)] == before, (ids,)
    pool.push([0], [torch.zeros(2560)], [torch.zeros(2, 512, 0)])
    with pytest.raises(ValueError, match="ahead of video"):
        pool.push([1, 0], [a, torch.zeros(561)], [v, torch.zeros(2, 512, 0)])
    assert pool.counters(0) == (4560, 3, 0, 0) and pool.counters(1) == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        pool.flush([1, 1])
    with pytest.raises(ValueError):
        pool.reset([0, 7])
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        pool.push([1], [a], [v])
    m.eval()
    assert pool.counters(1) == (0, 0, 0, 0)
    assert [tuple(t.shape) for t in pool.flush([1, 2])] == [(2, 0), (2, 2000)] and pool.counters(2) == (0, 0, 0, 0)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("window,hop", [(2560, 2560), (2560, 640), (5120, 1920)])
def test_pool_on_cpu_tensors_equals_the_oracle_and_separate_long_speakers(window, hop, K):
    """Three slots with different schedules in the same pushes.  Every window the pool frames is a copy, so with the row-wise separator
    the outputs differ from the float64 streaming overlap-add of the oracle's own windows, and from separate_long_speakers' torch path,
    by the float32 cross-fade only: 4 ceil(window / hop) 2^-23 max|y| (test_hip_longform.ola_bound; the tanh of the float32 separator
    against the float64 one adds 2^-23 max|y| per term, inside the factor 4)."""
    m = _model()
    seen = [0.0]

    def forward_modular(wav, emb):
        y = _cheap(wav, emb)
        seen[0] = max(seen[0], float(y.abs().max()))
        return y

    m.forward_modular = forward_modular
    max_chunk = window
    pool = m.open_streams(3, window=window, hop=hop, max_chunk=max_chunk, max_batch=4, speakers=K)
    assert pool._aring.numel() * 4 + pool._vring.numel() * 4 + pool._acc.numel() * 4 == 3 * (4 * pool.capacity * (1 + K) + 2048 * K * pool.capacity // 640)
    rng = np.random.RandomState(window + hop + K)
    Ls = [3 * VO.capacity(window, max_chunk) + 1, window - 1, window + 3 * hop]
    Tvs = [-(-Ls[0] // SPF), -(-Ls[1] // SPF), -(-Ls[2] // SPF) - 2]
    xs = [rng.randn(L).astype(np.float32) for L in Ls]
    vs = [rng.randn(K, 512, Tv).astype(np.float32) for Tv in Tvs]
    sizes = VO.chunk_sizes(hop, max_chunk)
    sch = {s: VO.schedule(Ls[s], Tvs[s], sizes, MODES[s], window, hop, max_chunk, start=2 * s) for s in range(3)}
    counters = {s: (0, 0, 0, 0) for s in range(3)}
    pos, got, ref = {s: [0, 0] for s in range(3)}, {s: [] for s in range(3)}, {s: [] for s in range(3)}
    olas = {s: SO.OverlapAdd(window, hop, K) for s in range(3)}
    for tick_no, (kind, ids, na, nf) in enumerate(VO.events(sch)):
        want = SO.tick(counters, ids, na, nf, window, hop, max_chunk, K, kind == "flush")
        if kind == "flush":
            outs = pool.flush(ids)
        else:
            wavs = [torch.from_numpy(xs[s][pos[s][0]:pos[s][0] + n]) for s, n in zip(ids, na)]
            vids = [torch.from_numpy(np.ascontiguousarray(vs[s][:, :, pos[s][1]:pos[s][1] + n])) for s, n in zip(ids, nf)]
            if tick_no % 2:  # K separate tensors and one (K,512,m) tensor are the same thing
                vids = [[t.clone() for t in v] for v in vids]
            outs = pool.push(ids, wavs, vids)
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        if want["rows"]:
            hist = {s: (xs[s][:pos[s][0]], vs[s][:, :, :pos[s][1]]) for s in ids}
            xw, vw = SO.frame_rows(want["rows"], hist, {s: tuple(pos[s]) for s in ids}, window, hop, K)
            y = _cheap_np(np.repeat(xw, K, axis=0), vw).reshape(len(want["rows"]), K, window)
            for i, (s, n) in enumerate(want["rows"]):
                olas[s].feed(n, y[i])
        for s, o, (lo, hi) in zip(ids, outs, want["ranges"]):
            assert tuple(o.shape) == (K, hi - lo) and o.dtype == torch.float32 and pool.counters(s) == want["new"][s]
            got[s].append(o.numpy())
            ref[s].append(olas[s].take(lo, hi))
        counters = want["new"]
    for s in range(3):
        assert pool.counters(s) == (0, 0, 0, 0)
        res, want = np.concatenate(got[s], axis=1), np.concatenate(ref[s], axis=1)
        whole = m.separate_long_speakers(torch.from_numpy(xs[s]), torch.from_numpy(vs[s])[None], window=window, hop=hop, max_batch=4)[0].numpy()
        bound = 4 * -(-window // hop) * 2.0 ** -23 * seen[0]
        e1, e2 = float(np.abs(res - want).max()), float(np.abs(res - whole).max())
        print(f"[live speakers host] window {window} hop {hop} K {K} slot {s} L {Ls[s]}: vs oracle {e1:.3e}, vs separate_long_speakers {e2:.3e} "
              f"(bound {bound:.3e})")
        assert res.shape == want.shape == whole.shape == (K, Ls[s])
        assert e1 <= bound and e2 <= bound, (s, e1, e2, bound)
        if hop == window:
            assert np.array_equal(res, whole)
