"""Host side of live streams at the microphone's rate (datas.open_resample_streams / ResampleStreamPool, the ``sample_rate`` keyword of
AVNet.open_streams, System.open_streams and System.open_camera_streams, rtfs_live_resample_plan) against tests/live_resample_oracle.py:
the tick arithmetic of the C planner exhaustively for seven ratios, the four bounds the planner and the pools rely on, that any chunking
plus a flush emits exactly rtfs_resample_out_len samples, every refusal with nothing written, the bindings, the classes' argument
refusals on CPU tensors, and the drift of per-chunk resampling that motivates all this.  None of it touches a device."""
import copy
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import live_resample_oracle as RO
from tests import prep_oracle as PO

LL = ctypes.c_longlong
BIG = 1 << 40


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def c_rtick(P, counters, ids, ms, slots, max_chunk, flush):
    """rtfs_live_resample_plan on the named slots of ``counters`` (dict slot -> (a, g, side)) -> (rc, new, table, sizes, refused)."""
    R = len(ids)
    cnt = [v for s in ids for v in counters.get(s, (0, 0, 0))]
    new, table, sizes, refused = (LL * (3 * R))(*([-7] * 3 * R)), (LL * (7 * R))(*([-7] * 7 * R)), (LL * 3)(*([-7] * 3)), (ctypes.c_int * 2)()
    rc = lib().rtfs_live_resample_plan((LL * max(R, 1))(*ids), (LL * max(3 * R, 1))(*cnt), None if flush else (LL * max(R, 1))(*ms), R, slots,
                                       int(flush), P.orig, P.new, max_chunk, new, table, sizes, refused)
    return rc, [tuple(new[3 * r:3 * r + 3]) for r in range(R)], list(table), list(sizes), tuple(refused)


def _as(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("o,n", RO.RATIOS)
def test_planner_exhaustively_and_the_four_bounds(o, n):
    """Every a in 0 .. 3 o + 4 width against every m in the same range: one planner call per m, one table row per a."""
    P = RO.Plan(o, n)
    assert (P.o, P.n) == (o, n)
    top, w = 3 * o + 4 * P.width, P.width
    A = np.arange(top + 1, dtype=np.int64)
    G = np.array([P.G(a) for a in range(2 * top + 1)], dtype=np.int64)
    R = top + 1
    ids = np.arange(R, dtype=np.int64)
    cnt = np.stack([A, G[:R], A & 1], axis=1).copy()  # both sides
    # bound 1: G(a) <= ceil(n a / o), and the closed form the kernel's comment derives
    assert np.all(G <= -(-n * np.arange(2 * top + 1) // o))
    assert np.array_equal(G, -(-n * np.maximum(0, np.arange(2 * top + 1) - w) // o))
    # bound 3: the next output never needs an input older than a - 2 width (and needs one that has not arrived)
    for a in range(R):
        assert a - 2 * w <= P.first(int(G[a])) and P.last(int(G[a])) >= a
    # bound 4: a flush emits at most ceil(n width / o) + 1 samples, and never a negative number
    tails = -(-n * A // o) - G[:R]
    assert tails.min() >= 0 and tails.max() <= P.tail() and tails[0] == 0
    new, table, sizes, refused = np.empty((R, 3), np.int64), np.empty((7, R), np.int64), np.empty(3, np.int64), (ctypes.c_int * 2)()
    for m in range(top + 1):
        ms = np.full(R, m, dtype=np.int64)
        rc = lib().rtfs_live_resample_plan(_as(ids), _as(cnt), _as(ms), R, R, 0, o, n, top, _as(new), _as(table), _as(sizes), refused)
        assert rc == 0 and tuple(refused) == (-1, 0), (m, tuple(refused))
        k = G[m:m + R] - G[:R]
        assert k.min() >= 0 and k.max() <= m * n // o + 1  # bound 2
        assert np.array_equal(new[:, 0], A + m) and np.array_equal(new[:, 1], G[m:m + R])
        assert np.array_equal(new[:, 2], (A & 1) ^ (1 if m else 0))
        off = np.concatenate([[0], np.cumsum(-(-k // RO.ALIGN) * RO.ALIGN)])
        assert np.array_equal(table, np.stack([ids, A, ms, G[:R], k, off[:-1], A & 1]))
        assert list(sizes) == [off[-1], m, k.max()]
    rc = lib().rtfs_live_resample_plan(_as(ids), _as(cnt), None, R, R, 1, o, n, top, _as(new), _as(table), _as(sizes), refused)
    assert rc == 0 and not new.any()
    off = np.concatenate([[0], np.cumsum(-(-tails // RO.ALIGN) * RO.ALIGN)])
    assert np.array_equal(table, np.stack([ids, A, 0 * A, G[:R], tails, off[:-1], A & 1])) and list(sizes) == [off[-1], 0, tails.max()]


@pytest.mark.parametrize("orig,new", [(48000, 16000), (44100, 16000), (8000, 16000), (22050, 16000), (16000, 48000), (11025, 16000)])
def test_planner_against_the_oracle_over_chunkings(orig, new):
    """Three slots interleaved, slot 3 idle, every slot streams every length one after the other with another chunk-size cycle: the
    emitted ranges tile [0, rtfs_resample_out_len(L)) exactly once and in order, and every input an output reads had arrived."""
    P = RO.Plan(orig, new)
    mc = 2 * P.o + 4 * P.width + 5
    base = RO.sizes(P, mc)
    cyc = [base, base[::-1], [1], [2, 0, 3], [mc], [P.width, P.width + 1], [7, 1, 0, 0, 2]]
    Ls = RO.lengths(P) + [3 * mc + 1]
    counters, ticks = {s: (0, 0, 0) for s in range(4)}, 0
    for j in range(len(Ls)):
        L = {s: Ls[(j + s) % len(Ls)] for s in range(3)}
        sch = {s: RO.chunking(L[s], cyc[(j + 2 * s) % len(cyc)], start=s) for s in range(3)}
        emitted = {s: [] for s in range(3)}
        for kind, ids, ms in RO.events(sch):
            flush = kind == "flush"
            want = RO.tick(P, counters, ids, ms, mc, flush)
            rc, got, table, sizes, refused = c_rtick(P, counters, ids, ms or [], 4, mc, flush)
            assert rc == 0 and refused == (-1, 0), (kind, ids, ms, counters)
            assert got == [want["new"][s] for s in ids] and table == want["table"], (kind, ids, ms, counters)
            assert sizes == [want["floats"], want["max_m"], want["max_k"]] and all(o % RO.ALIGN == 0 for o in want["off"])
            for s, (lo, hi) in zip(ids, want["ranges"]):
                if not flush:
                    assert all(P.last(q) < want["new"][s][0] for q in range(lo, hi))  # no look-ahead: every input read has arrived
                    assert P.last(hi) >= want["new"][s][0]  # and nothing that could leave is held back
                emitted[s] += list(range(lo, hi))
            counters = want["new"]
            ticks += 1
        for s in range(3):
            assert emitted[s] == list(range(int(lib().rtfs_resample_out_len(orig, new, L[s])))) and counters[s] == (0, 0, 0)
            assert len(emitted[s]) == PO.resample_out_len(orig, new, L[s])
        assert counters[3] == (0, 0, 0)
    assert ticks > 60


def test_planner_refusals_leave_everything_unwritten():
    P = RO.Plan(48000, 16000)
    ok = {0: (100, P.G(100), 1), 1: (0, 0, 0), 2: (19, 0, 1)}
    cases = [([3], [1], False, 2), ([-1], [1], False, 2), ([0, 0], [1, 1], False, 3), ([1, 2, 1], [0, 0, 0], True, 3),
             ([0], [51], False, 4), ([0], [-1], False, 4), ([1, 0], [50, 51], False, 4)]  # a good slot first
    for ids, ms, flush, reason in cases:
        rc, new, table, sizes, refused = c_rtick(P, ok, ids, ms, 3, 50, flush)
        assert rc == -4 and refused[1] == reason, (ids, ms, refused)
        assert refused[0] == (len(ids) - 1 if reason != 2 else 0)
        assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
        with pytest.raises(RO.Refused):
            RO.tick(P, ok, ids, ms, 50, flush)
    # counters the planner cannot have produced: negative, g != G(a), a side that is no side
    for bad in [(-1, 0, 0), (100, -1, 0), (100, P.G(100) + 1, 0), (100, P.G(100) - 1, 1), (19, 1, 0), (100, P.G(100), 2), (0, 0, -1)]:
        for flush in (False, True):
            rc, new, table, sizes, refused = c_rtick(P, {0: ok[0], 1: bad}, [0, 1], [1, 1], 2, 50, flush)
            assert rc == -4 and refused == (1, 8), (bad, flush)
            assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
            with pytest.raises(RO.Refused):
                RO.tick(P, {0: ok[0], 1: bad}, [0, 1], [1, 1], 50, flush)
    # R < 1, no slots, no samples allowed, a ratio rtfs_resample_plan refuses, a missing array
    assert c_rtick(P, {}, [], [], 3, 50, False)[4] == (-1, 1)
    assert c_rtick(P, ok, [0], [1], 0, 50, False)[4] == (-1, 1)
    assert c_rtick(P, ok, [1], [0], 3, 0, False)[4] == (-1, 1)
    refused = (ctypes.c_int * 2)()
    for orig, new in [(16001, 16000), (0, 16000), (16000, -1)]:
        assert lib().rtfs_live_resample_plan((LL * 1)(0), (LL * 3)(0, 0, 0), (LL * 1)(1), 1, 1, 0, orig, new, 50, None, None, None, refused) == -4
        assert tuple(refused) == (-1, 1)
    assert lib().rtfs_live_resample_plan((LL * 1)(0), (LL * 3)(0, 0, 0), None, 1, 1, 0, 48000, 16000, 50, None, None, None, refused) == -4
    assert tuple(refused) == (-1, 1)
    # every output may be NULL
    assert lib().rtfs_live_resample_plan((LL * 1)(0), (LL * 3)(100, P.G(100), 0), None, 1, 1, 1, 48000, 16000, 50, None, None, None, None) == 0
    assert lib().rtfs_live_resample_plan((LL * 1)(0), (LL * 3)(100, P.G(100), 0), (LL * 1)(7), 1, 1, 0, 48000, 16000, 50, None, None, None, None) == 0


def test_symbols_are_exported_and_bound():
    from rtfs_net_amd import _lib
    for name in ("rtfs_live_resample_plan", "rtfs_live_resample_f32", "rtfs_live_resample_i16", "rtfs_live_resample_reset"):
        assert name in _lib.SIGNATURES and getattr(lib(), name).argtypes == _lib.SIGNATURES[name][1]
    # the launches check their arguments before they touch a device: a ratio the plan refuses, a misaligned table
    assert lib().rtfs_live_resample_f32(8, 8, 16, 16, 1, 1, 1, 0, 16001, 16000, None) == -4
    assert lib().rtfs_live_resample_i16(4, 8, 16, 16, 1, 1, 1, 0, 48000, 16000, None) == -4
    assert lib().rtfs_live_resample_f32(8, 8, 8, 16, 1, 1, 1, 0, 48000, 16000, None) == -4
    assert lib().rtfs_live_resample_f32(8, 8, 16, 16, 1, 1, 1, 1, 48000, 16000, None) == -1  # a flush brings no samples
    assert lib().rtfs_live_resample_reset(None, 8, 1, 48000, 16000, None) == -4
    assert lib().rtfs_live_resample_f32(8, 8, 16, 16, 1, 0, 0, 0, 48000, 16000, None) == 0  # nothing arrived, nothing ready: no launch


def test_per_chunk_resampling_drifts_and_the_stream_does_not():
    """The motivating bug, in arithmetic alone: 3 s at 44.1 kHz in chunks of 1000 samples.  datas.resample per chunk returns
    ceil(n m / o) samples each, which sum to more than the recording resamples to; the stream's pushes and flush emit exactly that."""
    P, L, m = RO.Plan(44100, 16000), 3 * 44100, 1000
    whole = int(lib().rtfs_resample_out_len(44100, 16000, L))
    per_chunk = sum(int(lib().rtfs_resample_out_len(44100, 16000, c)) for c in RO.chunking(L, [m]))
    assert whole == 48000 and per_chunk > whole
    c, total = {0: (0, 0, 0)}, 0
    for size in RO.chunking(L, [m]):
        rc, new, table, _, _ = c_rtick(P, c, [0], [size], 1, m, False)
        assert rc == 0
        total, c = total + table[4], {0: new[0]}
    rc, new, table, _, _ = c_rtick(P, c, [0], None, 1, m, True)
    assert rc == 0 and total + table[4] == whole and new[0] == (0, 0, 0)
    print(f"[live resample host] 3 s at 44.1 kHz in chunks of {m}: per-chunk resample {per_chunk} samples, the stream {whole}")


def _audio():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    return R.AVNet(print_macs=False, **copy.deepcopy(audionet_config(2, "SRU"))).eval()


def _video():
    import rtfs_net_amd as R
    return R.FRCNNVideoModel(print_macs=False).eval()


def test_the_sample_rate_keyword_and_what_16000_returns():
    import rtfs_net_amd as R
    m, vm = _audio(), _video()
    sys_ = R.System(audio_model=m, video_model=vm)
    for fn in (m.open_streams, sys_.open_streams, sys_.open_camera_streams):
        assert inspect.signature(fn).parameters["sample_rate"].default == 16000
    # 16000: exactly the pools of before, no wrapper
    assert type(m.open_streams(2, window=2560, hop=1280, sample_rate=16000)) is R.StreamPool
    assert type(sys_.open_streams(slots=2, window=2560, hop=1280, sample_rate=16000)) is R.StreamPool
    cam = sys_.open_camera_streams(2, window=2560, hop=1280, sample_rate=16000)
    assert type(cam) is R.CameraStreamPool and cam.audio.max_chunk == 2560 + 1280
    # any other rate: the same surface, the inner pool with one more frame of room, chunks up to floor(max_chunk o / n)
    for pool, camera in ((m.open_streams(2, window=2560, hop=1280, sample_rate=48000), False),
                         (sys_.open_streams(slots=2, window=2560, hop=1280, sample_rate=48000), False),
                         (sys_.open_camera_streams(2, window=2560, hop=1280, sample_rate=48000), True)):
        assert type(pool) is R.RateStreamPool and type(pool.inner) is (R.CameraStreamPool if camera else R.StreamPool)
        assert all(callable(getattr(pool, f)) for f in ("push", "flush", "reset", "counters"))
        assert pool.max_chunk == 2560 and pool.max_chunk_in == 7680 and pool.sample_rate == 48000 and pool.slots == 2
        assert pool.audio.max_chunk == 2560 + 640 + (1280 if camera else 0) and pool.audio.window == 2560 and pool.audio.hop == 1280
        assert type(pool.resampler) is R.ResampleStreamPool and pool.resampler.max_chunk == 7680 and pool.tail == RO.Plan(48000, 16000).tail()
        assert pool.counters(1) == ((0, 0), ((0, 0, 0, 0), (0, 0)) if camera else (0, 0, 0, 0))
    p441 = sys_.open_camera_streams(2, window=2560, hop=1280, max_chunk=1280, sample_rate=44100)
    assert p441.max_chunk_in == 1280 * 441 // 160 and p441.inner.lips.max_frames == 3
    for kw in (dict(sample_rate=16001), dict(sample_rate=0), dict(sample_rate=48000.0), dict(sample_rate=48000, max_chunk=641),
               dict(sample_rate=48000, window=2561), dict(sample_rate=25, max_chunk=640, window=1280, hop=640)):  # 1:640: a tail of 4481
        with pytest.raises(ValueError):
            m.open_streams(**dict(dict(slots=2, window=2560, hop=1280), **kw))
        with pytest.raises(ValueError):
            sys_.open_camera_streams(**dict(dict(slots=2, window=2560, hop=1280), **kw))


def test_every_refusal_on_cpu_tensors_comes_before_any_device_call():
    """The pools lie on the CPU here, where a tick that got past its checks raises RuntimeError (there is no CPU arithmetic): every bad
    argument must raise ValueError instead, with all counters unchanged."""
    import rtfs_net_amd as R
    from rtfs_net_amd import datas
    for kw in (dict(slots=0), dict(orig_freq=16000), dict(orig_freq=16001), dict(max_chunk=0), dict(slots=2.5), dict(orig_freq=0)):
        with pytest.raises(ValueError):
            datas.open_resample_streams(**dict(dict(slots=2, orig_freq=48000, device="cpu"), **kw))
    pool = datas.open_resample_streams(3, 48000, max_chunk=100, device="cpu")
    assert type(pool) is R.ResampleStreamPool and (pool.o, pool.n, pool.width) == (3, 1, 19) and tuple(pool._hist.shape) == (3, 2, 38)
    f, i = torch.zeros(50), torch.zeros(50, dtype=torch.int16)
    bad = [([3], [f]), ([-1], [f]), ([0, 0], [f, f]), ([1.0], [f]), ([True], [f]), ([0, 1], [f]), (0, [f]), ([0], f[0]), ([0], 3), ([0], [None]),
           ([0, 1], [f, i]), ([0], [f.double()]), ([0], [f.half()]), ([0], [i.to(torch.int32)]), ([0], [torch.zeros(2, 25)]), ([0], [torch.zeros(101)]),
           ([1, 0], [f, torch.zeros(101)]), ([0], [f.to("meta")]), ([0], [torch.zeros(1, 1, 5)])]
    for ids, chunks in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks)
        assert [pool.counters(s) for s in range(3)] == [(0, 0)] * 3, (ids,)
    for ids in ([0, 0], [3], [0.5]):
        with pytest.raises(ValueError):
            pool.flush(ids)
        with pytest.raises(ValueError):
            pool.reset(ids)
    for good in ([f], [i], [f[None]]):
        with pytest.raises(RuntimeError, match="MI355X only"):  # a good push reaches the device path
            pool.push([0], good)
    assert pool.push([], []) == [] and pool.flush([]) == [] and pool.counters(0) == (0, 0)
    # the composite pools: what any of the three planners refuses, before anything moves
    sys_ = R.System(audio_model=_audio(), video_model=_video())
    cam = sys_.open_camera_streams(2, window=2560, hop=1280, roi_hw=(96, 96), sample_rate=48000)
    zero = ((0, 0), ((0, 0, 0, 0), (0, 0)))
    a, a16, r = torch.zeros(3000), torch.zeros(3000, dtype=torch.int16), torch.zeros(2, 96, 96, dtype=torch.uint8)
    bad = [([2], [a], [r]), ([0, 0], [a, a], [r, r]), ([0], [a, a], [r]), ([0], [a], [r, r]), ([0], a, [r]), ([0], [torch.zeros(7681)], [r]),
           ([0], [a], [torch.zeros(5, 96, 96, dtype=torch.uint8)]), ([0], [a.double()], [r]), ([0], [torch.zeros(2, 500)], [r]), ([0], [None], [r]),
           ([0], [a], [torch.zeros(2, 96, 100, dtype=torch.uint8)]), ([0], [a.to("meta")], [r]), ([1, 0], [a, a], [r, torch.zeros(2, 88, 88)]),
           ([0, 1], [a, a16], [r, r])]
    for ids, wavs, rois in bad:
        with pytest.raises(ValueError):
            cam.push(ids, wavs, rois)
        assert [cam.counters(s) for s in range(2)] == [zero] * 2, (ids,)
    for ids in ([0, 0], [2]):
        with pytest.raises(ValueError):
            cam.flush(ids)
        with pytest.raises(ValueError):
            cam.reset(ids)
    for wav in (a, a16):
        with pytest.raises(RuntimeError, match="MI355X only"):
            cam.push([0], [wav], [r])
    assert cam.counters(0) == zero and cam.push([], [], []) == [] and cam.flush([]) == []
    plain = _audio().open_streams(2, window=2560, hop=1280, sample_rate=44100)
    e = torch.zeros(512, 2)
    for ids, wavs, embs in [([2], [a], [e]), ([0], [torch.zeros(plain.max_chunk_in + 1)], [e]), ([0], [a], [torch.zeros(512, 6)]),
                            ([0], [a], [torch.zeros(511, 2)]), ([0, 0], [a, a], [e, e]), ([0], [a], [e.double()])]:
        with pytest.raises(ValueError):
            plain.push(ids, wavs, embs)
        assert plain.counters(0) == ((0, 0), (0, 0, 0, 0))
    with pytest.raises(RuntimeError, match="MI355X only"):
        plain.push([0], [a], [e])


@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("orig", [48000, 44100])
def test_composite_schedules_are_accepted_by_the_c_planners_and_their_flush_fits(orig, camera):
    """The oracle's schedules (in step, audio leading, video leading) through the three C planners in the order the pool asks them: every
    push the oracle accepts is accepted, counters agree, and the tail of the final flush always fits the inner ring."""
    from tests import live_oracle as VO
    from tests import live_video_oracle as LV
    from tests.test_live_host import c_tick
    from tests.test_live_video_host import c_vtick
    P = RO.Plan(orig, 16000)
    window, hop, mc = 2560, 1280, 2560
    inner = mc + RO.ROOM + (LV.SLACK if camera else 0)
    in_sizes = [0, 1, P.o + 1, 640 * P.o // P.n, hop * P.o // P.n + 1, mc * P.o // P.n]
    for L16 in (3 * window + 7, window - 1):
        L = L16 * P.o // P.n
        Tv = -(-P.out_len(L) // 640)
        for j, mode in enumerate(("step", "lag", "lead")):
            cr, ca, cv = (0, 0, 0), (0, 0, 0, 0), (0, 0, 0)
            for m, nf in RO.rate_schedule(P, L, Tv, in_sizes, mode, window, hop, mc, camera, start=j):
                rc, rnew, rtab, _, _ = c_rtick(P, {0: cr}, [0], [m], 1, mc * P.o // P.n, False)
                assert rc == 0
                k, ne = rtab[4], nf
                if camera:
                    rc, vnew, vtab, _, _ = c_vtick({0: cv}, [0], [nf], 1, (mc + RO.ROOM) // 640, False)
                    assert rc == 0
                    ne, cv = vtab[4], vnew[0]
                rc, anew, _, _, refused = c_tick({0: ca}, [0], [k], [ne], 1, window, hop, inner, 1, False)
                assert rc == 0, (mode, cr, ca, cv, m, nf, refused)
                cr, ca = rnew[0], anew[0]
                assert ca[0] == cr[1] and ca[0] + P.tail() - ca[2] * hop <= window + inner
            assert cr[0] == L and ca[1] == (max(0, Tv - 2) if camera else Tv)
            rc, _, rtab, _, _ = c_rtick(P, {0: cr}, [0], None, 1, mc * P.o // P.n, True)
            assert rc == 0 and 0 <= rtab[4] <= P.tail() and cr[1] + rtab[4] == P.out_len(L)
            rc, anew, _, _, refused = c_tick({0: ca}, [0], [rtab[4]], [0], 1, window, hop, inner, 1, False)
            assert rc == 0, (mode, ca, rtab[4], refused)
            if camera:
                rc, anew, _, _, refused = c_tick({0: anew[0]}, [0], [0], [cv[0] - cv[1]], 1, window, hop, inner, 1, False)
                assert rc == 0, (mode, refused)
            assert c_tick({0: anew[0]}, [0], None, None, 1, window, hop, inner, 1, True)[0] == 0
