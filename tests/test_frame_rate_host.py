"""Host side of live streams and recordings at the camera's own frame rate (rtfs_frame_rate_map, rtfs_live_video_rate_plan,
datas.frame_rate_of / frame_rate_map, the frame_rate= arguments) against tests/frame_rate_oracle.py, which states the rule by brute
force, and tests/live_video_oracle.py, which states the tick arithmetic in model frames.  None of it touches a device."""
import ctypes
import random
from fractions import Fraction

import pytest
import torch

from tests import frame_rate_oracle as FR
from tests import live_video_oracle as LV
from tests.test_live_video_host import _audio, _video, c_vtick, lib

LL = ctypes.c_longlong
RATES = FR.RATES
MAXF = 7


def ids_of(rate):
    return f"{rate.numerator}_{rate.denominator}"


def c_map(rate, n, want_src=True):
    out, src = LL(-7), (LL * 1024)(*([-7] * 1024))
    rc = lib().rtfs_frame_rate_map(rate[0], rate[1], n, ctypes.byref(out), src if want_src else None)
    return rc, out.value, list(src)


def c_rtick(counters, ids, ms, slots, max_frames, rate, flush):
    """rtfs_live_video_rate_plan on the named slots of ``counters`` (dict slot -> (g, v, side, n)) -> (rc, new, table, sizes, refused)."""
    R = len(ids)
    cnt = [v for s in ids for v in counters.get(s, (0, 0, 0, 0))]
    new, table, sizes, refused = (LL * (4 * R))(*([-7] * 4 * R)), (LL * (9 * R))(*([-7] * 9 * R)), (LL * 4)(*([-7] * 4)), (ctypes.c_int * 2)()
    rc = lib().rtfs_live_video_rate_plan((LL * max(R, 1))(*ids), (LL * max(4 * R, 1))(*cnt), None if flush else (LL * max(R, 1))(*ms), R, slots,
                                         int(flush), max_frames, rate[0], rate[1], new, table, sizes, refused)
    return rc, [tuple(new[4 * r:4 * r + 4]) for r in range(R)], list(table), list(sizes), tuple(refused)


# ---------------------------------------------------------------- the map
@pytest.mark.parametrize("rate", RATES, ids=ids_of)
def test_frame_rate_map_equals_the_brute_force_rule(rate):
    for n in range(201):
        want = FR.frame_map(n, rate)
        rc, n_out, src = c_map((rate.numerator, rate.denominator), n)
        assert rc == 0 and n_out == len(want) and src[:n_out] == want and set(src[n_out:]) == {-7}, (rate, n)
        assert c_map((3 * rate.numerator, 3 * rate.denominator), n, want_src=False)[:2] == (0, len(want))  # the fraction is reduced
    full = FR.frame_map(200, rate)
    assert full == sorted(full) and all(FR.source(p, rate) == c for p, c in list(enumerate(full))[:40])
    if rate == 25:
        assert full == list(range(200))


def test_the_examples_of_the_rule():
    assert FR.frame_map(12, Fraction(30)) == [0, 1, 2, 4, 5, 6, 7, 8, 10, 11]  # every sixth camera frame is dropped
    assert FR.frame_map(5, Fraction(15)) == [0, 0, 1, 2, 2, 3, 3, 4]
    assert FR.source(0, Fraction(60)) == 1
    assert c_map((60, 1), 1)[:2] == (0, 0) and c_map((60, 1), 2)[:2] == (0, 1)  # one frame at 60 fps completes no model frame


def test_rate_refusals_write_nothing():
    big = (1 << 20) + 1
    for rate in [(0, 1), (1, 0), (-30, 1), (30, -1), (241, 1), (1, 2), (999, 1000), (240 * 1000 + 1, 1000), (big, 4400)]:
        rc, n_out, src = c_map(rate, 10)
        assert rc == -4 and n_out == -7 and set(src) == {-7}, rate
        rc, new, table, sizes, refused = c_rtick({0: (0, 0, 0, 0)}, [0], [1], 1, MAXF, rate, False)
        assert rc == -4 and refused == (-1, 10), rate
        assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
    assert c_map((30, 1), -1)[0] == -4 and c_map((30, 1), (1 << 36) + 1)[0] == -4
    assert lib().rtfs_frame_rate_map(30, 1, 5, None, None) == -4
    assert c_map((240, 1), 5)[0] == 0 and c_map((1, 1), 5)[:2] == (0, 125)  # the ends of the range: P(5) at 1 fps = floor(125.5)


# ---------------------------------------------------------------- the planner
def oracle_tick(counters, ids, ms, rate, flush):
    """The rate planner from the two oracles: camera chunks -> the model frames they complete (brute force), then the tick of
    tests/live_video_oracle.py in model frames.  counters: dict slot -> (g, v, side, n)."""
    mm = None if flush else [FR.count(counters[s][3] + m, rate) - FR.count(counters[s][3], rate) for s, m in zip(ids, ms)]
    want = LV.tick({s: c[:3] for s, c in counters.items()}, ids, mm, 1 << 30, flush)
    new = dict(counters)
    for r, s in enumerate(ids):
        new[s] = want["new"][s] + ((0 if flush else counters[s][3] + ms[r]),)
    want["new4"], want["mm"] = new, mm
    want["table9"] = want["table"] + [counters[s][3] for s in ids]
    return want


@pytest.mark.parametrize("rate", RATES, ids=ids_of)
def test_planner_over_random_chunkings(rate):
    """200 random chunkings per rate, chunk sizes 0 .. max_frames with single frames and empty pushes forced in: the emitted ranges,
    concatenated, are exactly 0 .. P(n) - 1; m = 0 leaves g, v and side alone and advances n; the side flips exactly when m > 0."""
    rng = random.Random(rate.numerator * 7 + rate.denominator)
    fr = (rate.numerator, rate.denominator)
    empty_pushes = 0
    for trial in range(200):
        n = rng.choice([0, 1, 2, 3, 7, 13, 37, rng.randrange(38, 120)])
        sizes, left = [], n
        while left:
            m = min(left, rng.choice([0, 1, 1, rng.randrange(MAXF + 1), MAXF]))
            sizes.append(m)
            left -= m
        sizes.insert(rng.randrange(len(sizes) + 1), 0)
        counters, emitted = {0: (0, 0, 0, 0), 1: (0, 0, 0, 0)}, []
        for m in sizes:
            want = oracle_tick(counters, [1], [m], rate, False)
            rc, new, table, szs, refused = c_rtick(counters, [1], [m], 2, MAXF, fr, False)
            assert rc == 0 and refused == (-1, 0), (rate, sizes, counters)
            assert new == [want["new4"][1]] and table == want["table9"], (rate, sizes, counters, m)
            assert szs == [len(want["rows"]), want["floats"], m, want["mm"][0]]
            g, v, side, n0 = counters[1]
            g1, v1, side1, n1 = new[0]
            assert n1 == n0 + m and g1 == FR.count(n1, rate) and (side1 != side) == (g1 > g)
            if g1 == g:
                assert (g1, v1, side1) == (g, v, side)
                empty_pushes += m > 0
            emitted += list(range(*want["ranges"][0]))
            counters = want["new4"]
        want = oracle_tick(counters, [1], None, rate, True)
        rc, new, table, szs, refused = c_rtick(counters, [1], None, 2, MAXF, fr, True)
        assert rc == 0 and new == [(0, 0, 0, 0)] and table == want["table9"] and szs == [len(want["rows"]), want["floats"], 0, 0]
        emitted += list(range(*want["ranges"][0]))
        assert emitted == list(range(FR.count(n, rate))), (rate, sizes)
    if rate > 25:
        assert empty_pushes > 0  # frames arrived and no model frame was complete


@pytest.mark.parametrize("max_frames", [7, 50])
def test_at_25_fps_the_rate_planner_is_the_plain_planner(max_frames):
    rng = random.Random(max_frames)
    c3 = {s: (0, 0, 0) for s in range(3)}
    for tick in range(300):
        ids = rng.sample(range(3), rng.randrange(1, 4))
        flush = rng.random() < 0.1
        ms = [rng.randrange(max_frames + 1) for _ in ids]
        c4 = {s: c + (c[0],) for s, c in c3.items()}  # at 25 fps n == g
        rc, new, table, sizes, refused = c_vtick(c3, ids, ms, 3, max_frames, flush)
        rc4, new4, table4, sizes4, refused4 = c_rtick(c4, ids, ms, 3, max_frames, (50, 2), flush)
        assert rc == rc4 == 0 and refused == refused4
        assert table4[:8 * len(ids)] == table and table4[8 * len(ids):] == [c3[s][0] for s in ids]
        assert [c[:3] for c in new4] == new and [c[3] for c in new4] == [c[0] for c in new]
        assert sizes4[:3] == sizes and sizes4[3] == sizes[2]
        for s, c in zip(ids, new):
            c3[s] = c


def test_planner_refusals_leave_everything_unwritten():
    """Every refusal of the plain planner, through the rate planner at 30 fps, and the counters only the rate planner can refuse."""
    rate = (30, 1)
    P = lambda n: FR.count(n, Fraction(30))  # noqa: E731
    ok = {0: (P(6), P(6) - 2, 1, 6), 1: (0, 0, 0, 0), 2: (1, 0, 1, 1)}
    cases = [([3], [1], False, 2), ([-1], [1], False, 2), ([0, 0], [1, 1], False, 3), ([1, 2, 1], [0, 0, 0], True, 3),
             ([0], [8], False, 4), ([0], [-1], False, 4), ([1, 0], [7, 8], False, 4)]
    for ids, ms, flush, reason in cases:
        rc, new, table, sizes, refused = c_rtick(ok, ids, ms, 3, MAXF, rate, flush)
        assert rc == -4 and refused[1] == reason, (ids, ms, refused)
        assert refused[0] == (len(ids) - 1 if reason != 2 else 0)
        assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
    bad = [(-1, 0, 0, 0), (3, -1, 0, 3), (3, 4, 0, 3), (5, 2, 0, 6), (3, 0, 1, 3), (2, 1, 2, 2), (2, 1, -1, 2),
           (P(6), P(6) - 2, 0, 7), (P(6) + 1, P(6) - 1, 0, 6), (0, 0, 0, -1), (0, 0, 0, 1)]  # ... and g != P(n), n < 0
    for c in bad:
        for flush in (False, True):
            rc, new, table, sizes, refused = c_rtick({0: ok[0], 1: c}, [0, 1], [1, 1], 2, MAXF, rate, flush)
            assert rc == -4 and refused == (1, 8), (c, flush)
            assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
    assert c_rtick({0: (0, 0, 0, 0)}, [0], [0], 1, MAXF, rate, False)[0] == 0
    assert c_rtick({}, [], [], 3, MAXF, rate, False)[4] == (-1, 1)
    assert c_rtick(ok, [0], [1], 0, MAXF, rate, False)[4] == (-1, 1)
    assert c_rtick(ok, [0], [0], 3, 0, rate, False)[4] == (-1, 1)
    refused = (ctypes.c_int * 2)()
    assert lib().rtfs_live_video_rate_plan((LL * 1)(0), (LL * 4)(0, 0, 0, 0), None, 1, 1, 0, 7, 30, 1, None, None, None, refused) == -4
    assert tuple(refused) == (-1, 1)
    assert lib().rtfs_live_video_rate_plan((LL * 1)(0), (LL * 4)(*ok[0]), None, 1, 1, 1, 7, 30, 1, None, None, None, None) == 0


# ---------------------------------------------------------------- Python
def test_rate_parsing():
    from rtfs_net_amd import datas
    f = datas.frame_rate_of
    assert f(29.97) == Fraction(2997, 100) and f(29.97002997) == Fraction(30000, 1001) and f((30000, 1001)) == Fraction(30000, 1001)
    assert f(Fraction(25, 2)) == Fraction(25, 2) and f(30) == 30 and f(25.0) == 25 and f((50, 2)) == 25 and f([24000, 1001]) == Fraction(24000, 1001)
    assert f(23.976) == Fraction(2997, 125) and f(torch.tensor(30)) == 30
    for bad in (0, -30, 241, 0.5, (1, 0), (30,), (30, 1, 1), "30", None, True, (30.0, 1), float("nan"), float("inf"), Fraction(1, 2),
                Fraction((1 << 20) + 1, 4400)):
        with pytest.raises(ValueError):
            f(bad)
    for rate in RATES:
        assert datas.frame_rate_map(37, rate) == FR.frame_map(37, rate)
    assert datas.frame_rate_map(1, 60) == [] and datas.frame_rate_map(0, 30) == [] and datas.frame_rate_map(4, 25) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        datas.frame_rate_map(-1, 30)


def test_open_with_a_frame_rate():
    """At 25 fps, however it is written, today's classes; at another rate the rate pool, with max_frames in camera frames."""
    import rtfs_net_amd as R
    vm = _video()
    for r in (25, 25.0, Fraction(25), (50, 2)):
        assert type(vm.open_streams(2, max_frames=5, frame_rate=r)) is R.LipStreamPool
    pool = vm.open_streams(2, max_frames=5, roi_hw=(96, 100), frame_rate=15)
    assert type(pool) is R.RateLipStreamPool and isinstance(pool, R.LipStreamPool) and pool.counters(1) == (0, 0)
    assert pool.max_frames == 5 and pool._win.shape[0] == 2 * 9  # ceil(25 * 5 / 15) model frames per push at the most
    assert vm.open_streams(2, max_frames=5, frame_rate=60)._win.shape[0] == 2 * 3
    for bad in (0, 300, "30", (30, 0)):
        with pytest.raises(ValueError):
            vm.open_streams(2, frame_rate=bad)
    sys_ = R.System(audio_model=_audio(), video_model=vm)
    assert type(sys_.open_camera_streams(2, window=2560, hop=1280, frame_rate=25.0)) is R.CameraStreamPool
    assert type(sys_.open_camera_streams(2, window=2560, hop=1280, frame_rate=25.0).lips) is R.LipStreamPool
    cam = sys_.open_camera_streams(2, window=2560, hop=1280, frame_rate=30)
    assert type(cam) is R.CameraStreamPool and type(cam.lips) is R.RateLipStreamPool and cam.lips.max_frames == 4  # floor(4 * 30 / 25)
    assert sys_.open_camera_streams(2, window=2560, hop=1280, frame_rate=15).lips.max_frames == 2
    assert sys_.open_camera_streams(2, window=2560, hop=1280, frame_rate=60).lips.max_frames == 9
    assert cam.counters(0) == ((0, 0, 0, 0), (0, 0))
    with pytest.raises(ValueError):
        sys_.open_camera_streams(2, window=2560, hop=1280, frame_rate=500)
    with pytest.raises(ValueError, match="no camera frame"):
        sys_.open_camera_streams(2, window=640, hop=640, max_chunk=640, frame_rate=15)


def test_refusals_on_cpu_tensors_come_before_any_device_call():
    vm = _video()
    pool = vm.open_streams(3, max_frames=5, roi_hw=(96, 100), frame_rate=30)
    u8, f32 = torch.zeros(2, 96, 100, dtype=torch.uint8), torch.zeros(2, 88, 88)
    bad = [([3], [u8]), ([0, 0], [u8, u8]), ([0, 1], [u8, f32]), ([0], [u8.to(torch.int32)]), ([0], [torch.zeros(2, 96, 96, dtype=torch.uint8)]),
           ([0], [torch.zeros(6, 88, 88)]), ([1, 0], [u8, torch.zeros(6, 96, 100, dtype=torch.uint8)])]
    for ids, chunks in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks)
        assert [pool.counters(s) for s in range(3)] == [(0, 0)] * 3 and pool._counters == [[0, 0, 0, 0]] * 3, (ids,)
    with pytest.raises(RuntimeError, match="MI355X only"):
        pool.push([0], [u8])
    assert pool.push([], []) == [] and pool.flush([]) == [] and pool.counters(0) == (0, 0)
