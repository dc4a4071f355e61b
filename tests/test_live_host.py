"""Host side of live streaming (AVNet.open_streams, StreamPool, rtfs_live_plan) against tests/live_oracle.py: the tick arithmetic of the C
planner over every chunking, the float64 proof that a sample is final once the window after it was emitted, every refusal with the
counters unchanged, and the class end to end on CPU tensors against separate_long.  None of it touches a device.

As in tests/test_longform_host.py the package has no CPU arithmetic of its own, so the CPU-path test gives the model a cheap row-wise
``forward_modular``."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import live_oracle as VO
from tests import longform_oracle as LO

SPF = 640
PLANS = [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640), (5120, 1920), (32000, 16000)]
MODES = ("step", "lag", "lead")
LL = ctypes.c_longlong


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def flush_lengths(window, hop, max_chunk):
    k = -(-3 * VO.capacity(window, max_chunk) // hop)  # window + k hop: at least three ring capacities, every position wraps
    return [3, window - 1, window, window + 1, window + k * hop - 1, window + k * hop, window + k * hop + 1]


def c_tick(counters, ids, na, nf, slots, window, hop, max_chunk, n_src, flush):
    """rtfs_live_plan on the named slots of ``counters`` (dict) -> (rc, new counters of the named slots, table, sizes, refused)."""
    R = len(ids)
    cnt = [v for s in ids for v in counters.get(s, (0, 0, 0, 0))]
    new, table, sizes, refused = (LL * (4 * R))(*([-7] * 4 * R)), (LL * (13 * R))(*([-7] * 13 * R)), (LL * 5)(*([-7] * 5)), (ctypes.c_int * 2)()
    rc = lib().rtfs_live_plan((LL * R)(*ids), (LL * (4 * R))(*cnt), None if flush else (LL * R)(*na), None if flush else (LL * R)(*nf), R, slots,
                              int(flush), window, hop, max_chunk, n_src, new, table, sizes, refused)
    return rc, [tuple(new[4 * r:4 * r + 4]) for r in range(R)], list(table), list(sizes), tuple(refused)


def three_slot_events(window, hop, max_chunk):
    """Three slots, one mode each, streaming the flush lengths one after the other (a slot is flushed, then starts its next recording)."""
    sizes, Ls = VO.chunk_sizes(hop, max_chunk), flush_lengths(window, hop, max_chunk)
    per_slot = {s: [] for s in range(3)}
    for s, mode in enumerate(MODES):
        for j, L in enumerate(Ls[s:] + Ls[:s]):
            Tv = max(1, -(-L // SPF) - (2 if j % 3 == 1 else 0))  # every third recording is two frames short
            per_slot[s].append(VO.schedule(L, Tv, sizes, mode, window, hop, max_chunk, start=s + j))
    ev = []
    for j in range(len(Ls)):
        ev += VO.events({s: per_slot[s][j] for s in range(3)})
    return ev


@pytest.mark.parametrize("window,hop", PLANS)
def test_planner_against_the_oracle(window, hop):
    max_chunk = window
    for n_src in (1, 2):
        counters = {s: (0, 0, 0, 0) for s in range(3)}
        wrapped = 0
        for kind, ids, na, nf in three_slot_events(window, hop, max_chunk):
            flush = kind == "flush"
            want = VO.tick(counters, ids, na, nf, window, hop, max_chunk, n_src, flush)
            rc, new, table, sizes, refused = c_tick(counters, ids, na, nf, 3, window, hop, max_chunk, n_src, flush)
            assert rc == 0 and refused == (-1, 0), (kind, ids, na, nf, counters)
            assert new == [want["new"][s] for s in ids], (kind, ids, na, nf, counters)
            assert table == want["table"], (kind, ids, na, nf, counters)
            spans = [0 if flush and counters[s][0] == 0 else (hi - lo if flush else (0 if c1[2] == counters[s][2] else (c1[2] - 1) * hop + window - lo))
                     for s, c1, (lo, hi) in zip(ids, new, want["ranges"])]
            assert sizes == [len(want["rows"]), want["floats"], max(spans), max(na or [0]), max(nf or [0])]
            assert all(o % VO.ALIGN == 0 for o in want["off"])
            wrapped = max(wrapped, max(c[0] for c in new))
            counters = want["new"]
        assert wrapped >= 3 * VO.capacity(window, max_chunk)


@pytest.mark.parametrize("window,hop", PLANS)
def test_streaming_overlap_add_equals_the_offline_one_in_float64(window, hop):
    """The proof that "final when emitted" is right: dividing a sample by the weights of the windows emitted SO FAR, at the moment the
    schedule makes it final, gives longform_oracle.overlap_add of the whole recording."""
    max_chunk, rng = window, np.random.RandomState(window + hop)
    sizes = VO.chunk_sizes(hop, max_chunk)
    for j, L in enumerate(flush_lengths(window, hop, max_chunk)):
        for mode in MODES:
            Tv = -(-L // SPF)
            N = LO.plan(L, Tv, window, hop)
            y = rng.randn(N, 2, window)
            ola, c, got = VO.OverlapAdd(window, hop, 2), (0, 0, 0, 0), []
            for na, nf in VO.schedule(L, Tv, sizes, mode, window, hop, max_chunk, start=j):
                c, wins, (o, end) = VO.push_one(c, na, nf, window, hop, max_chunk)
                for n in wins:
                    ola.feed(n, y[n])
                got.append(ola.take(o, end))
            assert c[0] == L and c[1] == Tv
            c, wins, (o, end) = VO.flush_one(c, window, hop)
            for n in wins:
                ola.feed(n, y[n])
            got.append(ola.take(o, end))
            assert ola.next == N
            got = np.concatenate(got, axis=1)
            want = LO.overlap_add(y, 1, L, window, hop)[0]
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, (L, mode)


def test_planner_refusals_leave_everything_unwritten():
    window, hop, mc = 2560, 1280, 2560
    ok = {0: (2560, 4, 1, 1280), 1: (0, 0, 0, 0), 2: (6000, 4, 1, 1280)}  # slot 2: audio far ahead of video
    cases = [([3], [1], [0], False, 2), ([-1], [1], [0], False, 2), ([0, 0], [1, 1], [0, 0], False, 3),
             ([0], [2561], [0], False, 4), ([0], [0], [5], False, 4), ([0], [-1], [0], False, 4),
             ([1, 2], [640, 401], [1, 0], False, 5)]  # a good slot first; 6000 + 401 - 1280 > 5120
    for ids, na, nf, flush, reason in cases:
        rc, new, table, sizes, refused = c_tick(ok, ids, na, nf, 3, window, hop, mc, 1, flush)
        assert rc == -4 and refused[1] == reason, (ids, na, nf, refused)
        assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
        with pytest.raises(VO.Refused):
            VO.tick(ok, ids, na, nf, window, hop, mc, 1, flush)
    # video ahead: 4 + 5 frames - 2 > 8
    assert c_tick({0: (2560, 4, 1, 1280)}, [0], [0], [4], 1, window, hop, mc, 1, False)[0] == 0
    rc, *_, refused = c_tick({0: (2560, 8, 1, 1280)}, [0], [0], [3], 1, window, hop, mc, 1, False)
    assert rc == -4 and refused == (0, 6)
    # a flush with samples and no frame; counters the planner cannot have produced
    assert c_tick({0: (5, 0, 0, 0)}, [0], None, None, 1, window, hop, mc, 1, True)[4] == (0, 7)
    for bad in [(-1, 0, 0, 0), (100, 0, 1, 1280), (2560, 4, 1, 0), (9000, 4, 1, 1280)]:
        assert c_tick({0: bad}, [0], [0], [0], 1, window, hop, mc, 1, False)[4] == (0, 8), bad
    # sizes: what rtfs_longform_plan refuses, a max_chunk that is not a positive multiple of 640
    for w, h, m in [(2561, 1280, 2560), (2560, 1281, 2560), (2560, 0, 2560), (2560, 3200, 2560), (2560, 1280, 0), (2560, 1280, 641)]:
        assert c_tick({0: (0, 0, 0, 0)}, [0], [0], [0], 1, w, h, m, 1, False)[4] == (-1, 1), (w, h, m)
        with pytest.raises(VO.Refused):
            VO.tick({0: (0, 0, 0, 0)}, [0], [0], [0], w, h, m)
    # a ring longer than RTFS_LIVE_MAX_CAPACITY = 2^24 samples (the launch grids are sized for it): the largest that fits, then one frame more
    most = (1 << 24) // 640 * 640 - 2560
    assert c_tick({0: (0, 0, 0, 0)}, [0], [0], [0], 1, window, hop, most, 1, False)[0] == 0
    assert c_tick({0: (0, 0, 0, 0)}, [0], [0], [0], 1, window, hop, most + 640, 1, False)[4] == (-1, 1)


def _model(repeats=2, cell="SRU", n_src=1):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    conf = copy.deepcopy(audionet_config(repeats, cell))
    return R.AVNet(print_macs=False, **conf).eval()


def _cheap_forward(n_src):
    def forward_modular(wav, emb):  # row-wise, so a window's value does not depend on its chunk
        base = torch.tanh(wav) * (1.0 + emb.mean(dim=(1, 2)))[:, None]
        return torch.stack([base * (s + 1) for s in range(n_src)], dim=1)
    return forward_modular


def test_open_streams_refusals():
    m = _model()
    for kw in (dict(window=32001), dict(hop=16001), dict(hop=0), dict(hop=-640), dict(window=32000, hop=32640), dict(window=0),
               dict(window=1000, hop=500), dict(window=206 * 640), dict(slots=0), dict(max_chunk=0), dict(max_chunk=641), dict(max_chunk=-640),
               dict(max_batch=0), dict(max_chunk=(1 << 24) // 640 * 640)):
        with pytest.raises(ValueError):
            m.open_streams(**dict(dict(slots=2), **kw))
    with pytest.raises(ValueError):
        _model(2, "LSTM").open_streams(1, window=101 * 640)
    with pytest.raises(ValueError):
        _model(2, "GRU").open_streams(1)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.open_streams(2)
    m.eval()
    pool = m.open_streams(2, window=2560, hop=1280)
    assert pool.max_chunk == 2560 and pool.capacity == 5120
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        pool.push([0], [torch.zeros(4)], [torch.zeros(512, 0)])
    m.eval()
    import rtfs_net_amd as R
    assert isinstance(R.System(audio_model=m).open_streams(slots=1, window=1280, hop=640), R.StreamPool)


def test_every_push_refusal_leaves_all_counters_unchanged():
    m = _model()
    m.forward_modular = _cheap_forward(1)
    pool = m.open_streams(3, window=2560, hop=1280, max_batch=2)
    a, v = torch.zeros(2000), torch.zeros(512, 3)
    assert [tuple(t.shape) for t in pool.push([0, 2], [a, a], [v, v])] == [(1, 0), (1, 0)]
    before = [pool.counters(s) for s in range(3)]
    assert before == [(2000, 3, 0, 0), (0, 0, 0, 0), (2000, 3, 0, 0)]
    bad = [([3], [a], [v]), ([-1], [a], [v]), ([0, 0], [a, a], [v, v]), ([1.0], [a], [v]), ([True], [a], [v]),  # unknown / repeated / not int
           ([0, 1], [a], [v, v]), ([0], [a, a], [v]), (0, [a], [v]), ([0], a, 3),  # lists that do not match
           ([1, 0], [a, torch.zeros(2561)], [v, v]), ([1, 0], [a, a], [v, torch.zeros(512, 5)]),  # oversize, after a good slot
           ([0], [torch.zeros(2, 100)], [v]), ([0], [torch.zeros(1, 1, 100)], [v]), ([0], [a], [torch.zeros(3, 512)]),
           ([0], [a], [torch.zeros(1, 512, 3)]), ([0], [a.double()], [v]), ([0], [a], [v.half()]), ([0], [a.to(torch.int32)], [v]),
           ([0], [a.to("meta")], [v]), ([0], [a], [v.to("meta")]), ([0], [None], [v])]
    for ids, wavs, vids in bad:
        with pytest.raises(ValueError):
            pool.push(ids, wavs, vids)
        assert [pool.counters(s) for s in range(3)] == before, (ids,)
    # capacity: audio runs ahead of video until window 0's samples would be overwritten; slot 1 rides in the same call and must not move
    pool.push([0], [torch.zeros(2560)], [torch.zeros(512, 0)])
    assert pool.counters(0) == (4560, 3, 0, 0)
    with pytest.raises(ValueError, match="ahead of video"):
        pool.push([1, 0], [a, torch.zeros(561)], [v, torch.zeros(512, 0)])
    assert pool.counters(0) == (4560, 3, 0, 0) and pool.counters(1) == (0, 0, 0, 0)
    pool.push([0], [torch.zeros(560)], [torch.zeros(512, 0)])  # exactly full
    # whatever indexes is a slot id: numpy integers, 0-dim integer tensors, an array of ids
    none = [torch.zeros(0), torch.zeros(512, 0)]
    assert [tuple(t.shape) for t in pool.push([np.int64(1), torch.tensor(2)], [none[0]] * 2, [none[1]] * 2)] == [(1, 0), (1, 0)]
    assert [tuple(t.shape) for t in pool.push(np.array([2, 1]), [none[0]] * 2, [none[1]] * 2)] == [(1, 0), (1, 0)]
    for ids in ([np.float32(1)], [np.bool_(True)], [torch.tensor(1.0)], np.array([1.0])):
        with pytest.raises(ValueError):
            pool.push(ids, none[:1], none[1:])
    with pytest.raises(ValueError):
        pool.flush([1, 1])
    with pytest.raises(ValueError):
        pool.reset([0, 7])
    pool.reset([0])
    pool.push([0], [a], [torch.zeros(512, 0)])
    with pytest.raises(ValueError, match="no video frame"):
        pool.flush([2, 0])
    assert pool.counters(0) == (2000, 0, 0, 0) and pool.counters(2) == (2000, 3, 0, 0)
    assert [tuple(t.shape) for t in pool.flush([1, 2])] == [(1, 0), (1, 2000)] and pool.counters(2) == (0, 0, 0, 0)


@pytest.mark.parametrize("window,hop,n_src", [(2560, 1280, 1), (5120, 1920, 2), (1280, 1280, 1)])
def test_pool_on_cpu_tensors_equals_separate_long(window, hop, n_src):
    """Three slots with different schedules in the same pushes; the concatenated outputs against separate_long's torch path on the whole
    recordings, both on the same row-wise forward: the windows are bit-equal, so only the cross-fade differs, by at most ola_bound."""
    m = _model()
    m.n_src = n_src
    cheap, seen = _cheap_forward(n_src), [0.0]

    def forward_modular(wav, emb):
        y = cheap(wav, emb)
        seen[0] = max(seen[0], float(y.abs().max()))
        return y

    m.forward_modular = forward_modular
    max_chunk = window
    pool = m.open_streams(3, window=window, hop=hop, max_chunk=max_chunk, max_batch=2)
    rng = np.random.RandomState(window + hop)
    Ls = [3 * VO.capacity(window, max_chunk) + 1, window - 1, window + 3 * hop]
    Tvs = [-(-Ls[0] // SPF), -(-Ls[1] // SPF), -(-Ls[2] // SPF) - 2]
    xs = [torch.from_numpy(rng.randn(L).astype(np.float32)) for L in Ls]
    vs = [torch.from_numpy(rng.randn(512, Tv).astype(np.float32)) for Tv in Tvs]
    sizes = VO.chunk_sizes(hop, max_chunk)
    sch = {s: VO.schedule(Ls[s], Tvs[s], sizes, MODES[s], window, hop, max_chunk, start=2 * s) for s in range(3)}
    pos, got = {s: [0, 0] for s in range(3)}, {s: [] for s in range(3)}
    for kind, ids, na, nf in VO.events(sch):
        if kind == "flush":
            outs = pool.flush(ids)
        else:
            wavs = [xs[s][pos[s][0]:pos[s][0] + n] for s, n in zip(ids, na)]
            vids = [vs[s][:, pos[s][1]:pos[s][1] + n].contiguous() for s, n in zip(ids, nf)]
            wavs[0] = wavs[0][None]  # (1,n) is taken as well
            outs = pool.push(ids, wavs, vids)
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        for s, o in zip(ids, outs):
            assert o.shape[0] == n_src and o.dtype == torch.float32
            got[s].append(o)
    for s in range(3):
        assert pool.counters(s) == (0, 0, 0, 0)
        res = torch.cat(got[s], dim=1).numpy()
        want = m.separate_long(xs[s], vs[s][None], window=window, hop=hop)[0].numpy()
        bound = 4 * -(-window // hop) * 2.0 ** -23 * seen[0]  # test_hip_longform.ola_bound on the largest |y| the forward returned
        err = float(np.abs(res - want).max())
        print(f"[live host] window {window} hop {hop} slot {s} L {Ls[s]}: max abs err {err:.3e} (bound {bound:.3e})")
        assert res.shape == want.shape == (n_src, Ls[s]) and err <= bound, (s, err, bound)
        if hop == window:
            assert np.array_equal(res, want)
