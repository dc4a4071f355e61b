"""Host side of live streams with per-frame timestamps (rtfs_timestamp_map, rtfs_live_video_stamp_plan, datas.timestamp_map, the
timebase= arguments) against tests/timestamp_oracle.py, which states the rule by brute force with exact fractions, and
tests/frame_rate_oracle.py, which it must agree with on constant-rate stamps.  None of it touches a device."""
import ctypes
import random
from fractions import Fraction

import pytest
import torch

from tests import frame_rate_oracle as FR
from tests import timestamp_oracle as TS
from tests.test_live_video_host import _audio, _video, lib

LL = ctypes.c_longlong
MAXF = 7
TB = 90000
RATES = [Fraction(30), Fraction(60), Fraction(15), Fraction(10), Fraction(30000, 1001), Fraction(25), Fraction(24), Fraction(50)]
ZERO = (0,) * 7


def ids_of(rate):
    return f"{rate.numerator}_{rate.denominator}"


def c_map(stamps, tb, until=0, want_src=True):
    n = len(stamps)
    out, src = LL(-7), (LL * 1024)(*([-7] * 1024))
    rc = lib().rtfs_timestamp_map((LL * max(n, 1))(*stamps), n, tb, until, ctypes.byref(out), src if want_src else None)
    return rc, out.value, list(src)


def c_stick(counters, ids, chunks, untils, slots, max_frames, tb, flush):
    """rtfs_live_video_stamp_plan on the named slots of ``counters`` (dict slot -> (g, v, side, n, last, W, hside)); chunks = per named
    slot the stamps it brings, untils = per named slot or None -> (rc, new, table, sources, sizes, refused).  Every output starts as -7."""
    R = len(ids)
    cnt = [v for s in ids for v in counters.get(s, ZERO)]
    stamps = [t for c in chunks for t in c]
    new, table, src = (LL * (7 * R))(*([-7] * 7 * R)), (LL * (12 * R))(*([-7] * 12 * R)), (LL * (max_frames * max(R, 1)))(*([-7] * max_frames * max(R, 1)))
    sizes, refused = (LL * 5)(*([-7] * 5)), (ctypes.c_int * 2)()
    rc = lib().rtfs_live_video_stamp_plan((LL * max(R, 1))(*ids), (LL * max(7 * R, 1))(*cnt), None if flush else (LL * max(R, 1))(*map(len, chunks)),
                                          (LL * max(len(stamps), 1))(*stamps), None if untils is None else (LL * max(R, 1))(*untils), R, slots,
                                          int(flush), max_frames, tb, new, table, src, sizes, refused)
    return rc, [tuple(new[7 * r:7 * r + 7]) for r in range(R)], list(table), list(src), list(sizes), tuple(refused)


def untouched(new, table, src, sizes):
    return set(v for c in new for v in c) | set(table) | set(src) | set(sizes) == {-7}


# ---------------------------------------------------------------- the oracle against the rate oracle
@pytest.mark.parametrize("rate", RATES, ids=ids_of)
def test_constant_rate_stamps_give_the_frame_rate_rule(rate):
    """tau_i = i tb b / a: G(n step) = P(n) for n <= 200, and the stream's sources are the rate rule's map."""
    step = TS.constant_rate(2, rate, TB)[1]
    for n in range(201):
        assert TS.final_count(n * step, TB) == FR.count(n, rate), (rate, n)
    for n in (1, 2, 3, 7, 37, 200):
        stamps = TS.constant_rate(n, rate, TB)
        st = TS.Stream(TB)
        got = st.push(stamps, until=n * step)
        assert got == FR.frame_map(n, rate) and st.g == FR.count(n, rate), (rate, n)
        rc, n_out, src = c_map(stamps, TB, n * step)  # and the C map: it ends with the last frame's own tick at the least
        want = TS.frame_map(stamps, TB, n * step)
        assert rc == 0 and src[:n_out] == want and want[:len(got)] == got and set(src[n_out:]) == {-7}, (rate, n)
        assert len(want) == max(len(got), TS.tick(stamps[-1], TB) + 1)


def test_the_examples_of_the_rule():
    # 30 fps with frames 3 and 4 lost: model frames 3 and 4 go on showing frame 2
    stamps = [0, 3000, 6000, 15000, 18000]
    assert TS.frame_map(stamps, TB) == [0, 1, 2, 2, 3, 4] and c_map(stamps, TB)[2][:6] == [0, 1, 2, 2, 3, 4]
    # a first frame three ticks late is shown from model frame 0 on
    assert TS.frame_map([10800, 14400], TB) == [0, 0, 0, 0, 1] and c_map([10800, 14400], TB)[2][:5] == [0, 0, 0, 0, 1]
    # a burst inside one tick: only its last frame is shown
    assert TS.frame_map([0, 3600, 3700, 3800, 7200], TB) == [0, 3, 4]
    # until carries the last frame on
    assert TS.frame_map([0, 40], 1000, until=200) == [0, 1, 1, 1, 1] and c_map([0, 40], 1000, 200)[:2] == (0, 5)
    assert c_map([], TB)[:2] == (0, 0) and c_map([], TB, 90000)[:2] == (0, 0)  # nothing to show without a frame


# ---------------------------------------------------------------- the planner
def random_stamps(rng, tb, n):
    """Gaps from one tick to half a second, bursts of several frames in one model tick, a late first frame."""
    t = rng.choice([0, 0, rng.randrange(0, 3 * tb // 10 + 1)])
    out = []
    for _ in range(n):
        out.append(t)
        kind = rng.random()
        if kind < 0.15:
            t += 1
        elif kind < 0.4:
            t += rng.randrange(1, max(2, tb // 100))  # a burst: well inside one 40 ms tick
        elif kind < 0.85:
            t += rng.randrange(max(1, tb // 40), max(2, tb // 20))  # around 30 fps
        else:
            t += rng.randrange(max(1, tb // 10), tb // 2 + 1)  # a dropout
    return out


def drive(rng, tb, n, stats):
    """One random stream on one slot of three through the C planner and the oracle side by side."""
    stamps = random_stamps(rng, tb, n)
    st, slot = TS.Stream(tb), rng.randrange(3)
    c = {slot: ZERO}
    shown, sources, at, top = set(), [], 0, 0

    def step(chunk, until, flush):
        nonlocal c, top
        g, v, side, n0, last, W, hs = c[slot]
        copy = TS.Stream(tb)
        copy.stamps, copy.g, copy.W = list(st.stamps), st.g, st.W
        try:
            new = copy.flush(until or 0, MAXF) if flush else copy.push(chunk, until or 0, MAXF)
        except TS.Refused as e:
            assert "model frames" in str(e)
            rc, cn, table, src, sizes, refused = c_stick(c, [slot], [chunk], None if until is None else [until], 3, MAXF, tb, flush)
            assert rc == -4 and refused == (0, 14) and untouched(cn, table, src, sizes)
            return False
        rc, cn, table, src, sizes, refused = c_stick(c, [slot], [chunk], None if until is None else [until], 3, MAXF, tb, flush)
        assert rc == 0 and refused == (-1, 0), (stamps, chunk, until, flush, refused)
        m = len(new)
        want_src = []
        for cam in new:
            assert cam >= n0 - 1 and (cam >= 0)  # the chunk being pushed, or the last frame of an earlier push
            want_src.append(cam - n0 if cam >= n0 else -1)
            if cam < n0:
                stats["held"] += 1
                stats["held_unseen"] += cam not in shown
        assert src[:m] == want_src and set(src[m:]) <= {-7}, (stamps, chunk, until, flush)
        assert all(-1 <= i < len(chunk) for i in src[:m])
        g1 = g + m
        v1 = g1 if flush else max(v, g1 - 2)
        assert table == [slot, g, m, v, v1 - v, 0, 0, side, n0, hs, 0, len(chunk)]
        assert sizes == [v1 - v, -(-512 * (v1 - v) // 32) * 32, len(chunk), m, m]
        if flush:
            assert cn == [ZERO] and copy.n == 0
            top = max(top, until or 0)
        else:
            assert cn[0] == (g1, v1, 1 - side if m else side, copy.n, copy.stamps[-1] if copy.stamps else 0, copy.W,
                             1 - hs if chunk else hs), (stamps, chunk, until)
            assert copy.g == g1 and (copy.n == 0 or copy.g == TS.final_count(copy.W, tb))
            top = max(top, until or 0)
        shown.update(new)
        sources.extend(new)
        st.stamps, st.g, st.W = copy.stamps, copy.g, copy.W
        c = {slot: cn[0]}
        return True

    def walk_to(target):
        """Advance until in steps of at most MAXF ticks: what a caller does after a 'too many at once' refusal."""
        while True:
            u = min(target, st.W + MAXF * tb // 25)
            assert step([], u, False)
            if u == target:
                return

    while at < n:
        k = min(rng.randrange(0, 6), n - at)
        chunk = stamps[at:at + k]
        nxt = stamps[at + k] if at + k < n else stamps[-1] + tb
        lo = chunk[-1] if chunk else st.W
        until = rng.choice([None, None, rng.randrange(0, nxt + 1), nxt, rng.randrange(min(lo, nxt), nxt + 1)])
        if not step(chunk, until, False):
            stats["too_many"] += 1
            for t in chunk:  # frame by frame, walking the watermark up to each
                if not step([t], None, False):
                    if st.n == 0:
                        return  # a first frame more than MAXF ticks late cannot enter: the caller rebases its stamps
                    walk_to(t)
                    assert step([t], None, False)
            if until is not None and until > st.W:
                walk_to(until)
        at += k
    until = rng.choice([None, None, (stamps[-1] if stamps else 0) + rng.randrange(0, tb // 4 + 1)])
    n_all, W_end = st.n, st.W
    if not step([], until, True):
        walk_to(until)
        assert step([], until, True)
    stats["streams"] += 1
    if n_all:
        from rtfs_net_amd import datas
        want = TS.frame_map(stamps[:n_all], tb, max(top, W_end))
        assert sources == want == datas.timestamp_map(stamps[:n_all], tb, max(top, W_end)), (stamps, sources, want)


def test_planner_and_map_against_the_oracle_on_random_streams():
    rng = random.Random(2024)
    stats = dict(streams=0, held=0, held_unseen=0, too_many=0)
    for i in range(2000):
        drive(rng, (1000, 90000, 600, 25)[i % 4], rng.randrange(0, 14), stats)
    print(f"[timestamps] {stats}")
    assert stats["streams"] >= 1900 and stats["too_many"] > 20
    # the case that needs the held plane: -1 names a camera frame that no earlier model frame showed
    assert stats["held"] > 500 and stats["held_unseen"] > stats["held"] // 20, stats


def test_several_slots_in_one_call():
    """Stamps one behind the other in the order the slots are named; the sources of slot r start at its own offset."""
    c = {0: ZERO, 2: (3, 1, 1, 2, 100, 100, 1)}  # slot 2: two frames so far, W = 100 ms, G = 3
    assert TS.final_count(100, 1000) == 3
    rc, new, table, src, sizes, refused = c_stick(c, [2, 1, 0], [[150, 190], [], [0, 40, 95]], [200, 500, 0], 3, MAXF, 1000, False)
    assert rc == 0 and refused == (-1, 0)
    # slot 2: W' = 200, G = 5: model frames 3 (tick of 150 is 4: shows the held frame) and 4 (150); slot 1: no frame yet, g stays 0;
    # slot 0: W' = 95, G = 2: frames 0 (0 ms) and 1 (40 ms)
    assert src[:4] == [-1, 0, 0, 1] and sizes == [2, 1024, 3, 2, 4]
    assert new == [(5, 3, 0, 4, 190, 200, 0), (0, 0, 0, 0, 0, 500, 0), (2, 0, 1, 3, 95, 95, 1)]
    assert table[:3] == [2, 1, 0] and table[2 * 3:3 * 3] == [2, 0, 2] and table[4 * 3:5 * 3] == [2, 0, 0]
    assert table[9 * 3:] == [1, 0, 0, 0, 2, 2, 2, 0, 3]  # hside | soff | m_cam


# ---------------------------------------------------------------- refusals
def test_planner_refusals_leave_everything_unwritten():
    tb = 1000
    ok = {0: (3, 1, 1, 2, 100, 100, 1), 1: ZERO, 2: (0, 0, 0, 0, 0, 300, 0)}
    cases = [  # ids, chunks, untils, flush, (index, reason)
        ([3], [[5]], None, False, (0, 2)), ([0, 0], [[], []], None, False, (1, 3)), ([1, 2, 1], [[], [], []], None, True, (2, 3)),
        ([1], [list(range(8))], None, False, (0, 4)),  # more than max_frames camera frames
        ([1, 0], [[], [90]], None, False, (1, 13)),  # below W
        ([0], [[100]], None, False, (0, 13)),  # not above the last stamp (== W here)
        ([0], [[120, 120]], None, False, (0, 13)), ([0], [[130, 120]], None, False, (0, 13)),  # not increasing
        ([2], [[299]], None, False, (0, 13)),  # an earlier until promised it would not come
        ([1], [[-1]], None, False, (0, 12)), ([1], [[1 << 40]], None, False, (0, 12)),
        ([1], [[]], [-1], False, (0, 12)), ([1], [[]], [(1 << 40) + 1], False, (0, 12)), ([0], [[]], [-5], True, (0, 12)),
        ([0], [[]], [100 + 8 * 40], False, (0, 14)), ([0], [[101 + 8 * 40]], None, False, (0, 14)),  # eight model frames at once
        ([0], [[]], [100 + 8 * 40], True, (0, 14)),
    ]
    for ids, chunks, untils, flush, why in cases:
        rc, new, table, src, sizes, refused = c_stick(ok, ids, chunks, untils, 3, MAXF, tb, flush)
        assert rc == -4 and refused == why, (ids, chunks, untils, flush, refused)
        assert untouched(new, table, src, sizes)
    rc, new, _, src, sizes, _ = c_stick(ok, [0], [[]], [100 + 7 * 40], 3, MAXF, tb, False)  # exactly max_frames: all from the held frame
    assert rc == 0 and new[0][0] == 10 and src[:7] == [-1] * 7 and sizes[3:] == [7, 7]
    for bad_tb in (0, -1, (1 << 30) + 1):
        rc, new, table, src, sizes, refused = c_stick(ok, [0], [[150]], None, 3, MAXF, bad_tb, False)
        assert rc == -4 and refused == (-1, 11) and untouched(new, table, src, sizes)
        assert c_map([0, 1], bad_tb)[:2] == (-4, -7)
    assert c_stick(ok, [1], [[150]], None, 3, MAXF, 1 << 30, False)[0] == 0
    bad = [(3, 1, 1, 2, 100, 99, 1), (2, 0, 1, 2, 100, 100, 1), (3, 1, 1, 2, 100, 100, 2), (0, 0, 0, 0, 5, 5, 0), (1, 0, 1, 0, 0, 0, 0),
           (3, 1, 1, -1, 100, 100, 0), (3, 1, 1, 2, -1, 100, 0), (3, 1, 1, 2, 100, (1 << 40) + 1, 0), (3, 1, 2, 2, 100, 100, 1), (3, 0, 1, 2, 100, 100, 1)]
    for cnt in bad:
        for flush in (False, True):
            rc, new, table, src, sizes, refused = c_stick({0: ok[0], 1: cnt}, [0, 1], [[], []], None, 2, MAXF, tb, flush)
            assert rc == -4 and refused == (1, 8) and untouched(new, table, src, sizes), (cnt, flush)
    assert c_stick({}, [], [], None, 3, MAXF, tb, False)[5] == (-1, 1) and c_stick(ok, [0], [[]], None, 3, 0, tb, False)[5] == (-1, 1)
    refused = (ctypes.c_int * 2)()
    assert lib().rtfs_live_video_stamp_plan((LL * 1)(0), (LL * 7)(*ZERO), None, None, None, 1, 1, 0, 7, tb, None, None, None, None, refused) == -4
    assert tuple(refused) == (-1, 1)  # a push without n_frames
    assert lib().rtfs_live_video_stamp_plan((LL * 1)(0), (LL * 7)(*ZERO), (LL * 1)(1), None, None, 1, 1, 0, 7, tb, None, None, None, None, refused) == -4
    assert tuple(refused) == (0, 1)  # frames without stamps
    assert lib().rtfs_live_video_stamp_plan((LL * 1)(0), (LL * 7)(*ok[0]), None, None, None, 1, 1, 1, 7, tb, None, None, None, None, None) == 0
    # the map
    for stamps, until in [([0, 0], 0), ([5, 3], 0), ([-1], 0), ([1 << 40], 0), ([0], -1), ([0], (1 << 40) + 1)]:
        assert c_map(stamps, tb, until)[:2] == (-4, -7) and set(c_map(stamps, tb, until)[2]) == {-7}
    assert lib().rtfs_timestamp_map((LL * 1)(0), 1, tb, 0, None, None) == -4
    assert lib().rtfs_timestamp_map(None, 1, tb, 0, ctypes.byref(LL(0)), None) == -4
    assert c_map([0], 1, 1 << 40)[0] == -4  # 25 * 2^40 model frames: more than a map may hold


# ---------------------------------------------------------------- Python
def test_timestamp_map_in_python():
    from rtfs_net_amd import datas
    stamps = [0, 3000, 6000, 15000, 18000]
    assert datas.timestamp_map(stamps, TB) == [0, 1, 2, 2, 3, 4] == datas.timestamp_map(torch.tensor(stamps), TB)
    assert datas.timestamp_map(stamps, TB, until=25200) == [0, 1, 2, 2, 3, 4, 4] and datas.timestamp_map([], TB) == []
    for rate in RATES:
        assert datas.timestamp_map(TS.constant_rate(37, rate, TB), TB, 37 * TS.constant_rate(2, rate, TB)[1])[:FR.count(37, rate)] == FR.frame_map(37, rate)
    for bad in (([0, 0], TB), ([1, 0], TB), ([-1], TB), ([0.5], TB), ([True], TB), ("ab", TB), ([0], 0), ([0], None), ([0], 2.5), ([0], (1 << 30) + 1),
                ([1 << 40], TB), (5, TB)):
        with pytest.raises(ValueError):
            datas.timestamp_map(*bad)
    with pytest.raises(ValueError):
        datas.timestamp_map([0], TB, until=-1)


def test_open_with_a_timebase():
    """Without timebase= today's classes; with it the stamp pool, and ValueError for what is out of scope."""
    import rtfs_net_amd as R
    vm = _video()
    assert type(vm.open_streams(2, max_frames=5)) is R.LipStreamPool and type(vm.open_streams(2, max_frames=5, timebase=None)) is R.LipStreamPool
    assert type(vm.open_streams(2, max_frames=5, frame_rate=30, timebase=None)) is R.RateLipStreamPool
    pool = vm.open_streams(2, max_frames=5, roi_hw=(96, 100), timebase=TB)
    assert type(pool) is R.StampLipStreamPool and isinstance(pool, R.LipStreamPool) and not isinstance(pool, R.RateLipStreamPool)
    assert pool.counters(1) == (0, 0) and pool.timebase == TB and pool.max_frames == 5
    assert pool._win.shape[0] == 2 * 7 and tuple(pool._held.shape) == (2, 2, 88, 88) and tuple(pool._hist.shape) == (2, 2, 4, 88, 88)
    assert type(vm.open_streams(2, timebase=TB, frame_rate=25.0)) is R.StampLipStreamPool
    for kw in (dict(timebase=0), dict(timebase=-1), dict(timebase=(1 << 30) + 1), dict(timebase=2.5), dict(timebase="90000"), dict(timebase=True),
               dict(timebase=TB, frame_rate=30), dict(timebase=TB, frame_rate=(30000, 1001))):
        with pytest.raises(ValueError):
            vm.open_streams(2, **kw)
    sys_ = R.System(audio_model=_audio(), video_model=vm)
    assert type(sys_.open_camera_streams(2, window=2560, hop=1280).lips) is R.LipStreamPool
    cam = sys_.open_camera_streams(2, window=2560, hop=1280, timebase=1000)
    assert type(cam) is R.CameraStreamPool and type(cam.lips) is R.StampLipStreamPool and cam.lips.max_frames == 4
    assert cam.counters(0) == ((0, 0, 0, 0), (0, 0))
    for kw in (dict(speakers=2), dict(max_speakers=2), dict(sample_rate=48000), dict(frame_rate=30), dict(timebase=0)):
        with pytest.raises(ValueError):
            sys_.open_camera_streams(2, window=2560, hop=1280, **dict(dict(timebase=1000), **kw))
    plain = sys_.open_camera_streams(2, window=2560, hop=1280)
    w, roi = torch.zeros(640), torch.zeros(1, 96, 96, dtype=torch.uint8)
    for kw in (dict(timestamps=[[0]]), dict(until=40), dict(until=[40])):  # stamps need a pool opened with timebase=
        with pytest.raises(ValueError, match="timebase"):
            plain.push([0], [w], [roi], **kw)
    with pytest.raises(ValueError, match="timebase"):
        plain.flush([0], until=40)
    with pytest.raises(ValueError):
        sys_.separate_recording(w, 16000, roi, timestamps=[0])
    with pytest.raises(ValueError):
        sys_.separate_recording(w, 16000, roi, timebase=1000)
    with pytest.raises(ValueError):
        sys_.separate_recording(w, 16000, roi, timestamps=[0], timebase=1000, frame_rate=30)
    with pytest.raises(ValueError):
        sys_.separate_recording(w, 16000, roi, timestamps=[0, 40], timebase=1000)  # one stamp per frame


def test_refusals_on_cpu_tensors_come_before_any_device_call():
    vm = _video()
    pool = vm.open_streams(3, max_frames=5, roi_hw=(96, 100), timebase=1000)
    u8, f32 = torch.zeros(2, 96, 100, dtype=torch.uint8), torch.zeros(2, 88, 88)
    bad = [([3], [u8], [[0, 40]], None), ([0, 0], [u8, u8], [[0, 40]] * 2, None), ([0, 1], [u8, f32], [[0, 40]] * 2, None),
           ([0], [torch.zeros(6, 88, 88)], [list(range(6))], None),
           ([0], [u8], [[0]], None), ([0], [u8], [[0, 40, 80]], None), ([0], [u8], None, None), ([0], [u8], [[0, 40], [0]], None),  # the count
           ([0], [u8], [[40, 40]], None), ([0], [u8], [[40, 0]], None), ([0], [u8], [[-1, 0]], None), ([0], [u8], [[0, 1 << 40]], None),
           ([0], [u8], [[0, 40.0]], None), ([0], [u8], [[0, True]], None), ([0], [u8], [7], None), ([0], [u8], [torch.tensor([0.0, 1.0])], None),
           ([0], [u8], [[0, 40]], -1), ([0], [u8], [[0, 40]], [-1]), ([0], [u8], [[0, 40]], [40, 40]), ([0], [u8], [[0, 40]], 1.5),
           ([0], [u8], [[0, 40]], 40 + 8 * 40), ([0, 1], [u8, u8[:0]], [[0, 40], None], [None, 10 ** 30])]
    for ids, chunks, ts, until in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks, ts, until)
        assert [pool.counters(s) for s in range(3)] == [(0, 0)] * 3 and pool._counters == [[0] * 7] * 3, (ids, ts, until)
    with pytest.raises(ValueError):
        pool.flush([0], until=-1)
    with pytest.raises(ValueError):
        pool.flush([0, 5])
    with pytest.raises(RuntimeError, match="MI355X only"):
        pool.push([0], [u8], [torch.tensor([0, 40])], until=[80])
    assert pool._counters == [[0] * 7] * 3
    assert pool.push([], [], []) == [] and pool.flush([]) == [] and pool.counters(0) == (0, 0)
