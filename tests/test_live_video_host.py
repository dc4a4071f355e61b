"""Host side of live streams from camera frames (FRCNNVideoModel.open_streams / LipStreamPool, System.open_camera_streams /
CameraStreamPool, rtfs_live_video_plan) against tests/live_video_oracle.py: the tick arithmetic of the C planner over every chunking,
the tiling and receptive-field claims from the oracle alone, every refusal with nothing written, the classes' argument refusals on CPU
tensors, and the slack of the camera pool's inner audio pool.  None of it touches a device.

THE SLACK (max_chunk + 1280).  Embeddings lag the frames received by two frames, so the inner audio pool sees video 1280 samples later
than the camera delivered it.  What is provable, and asserted here without any replaced push: for streams IN STEP (every push brings the
frames complete so far, g = floor(a / 640)) a - e hop <= window + 1279 after any tick, so a chunk of max_chunk always fits a ring of
window + max_chunk + 1280; with the inner pool at plain max_chunk the same pushes are refused.  When video LAGS audio by a window the
plain rule is already at its edge and two more frames of lag can cost a whole hop, which no fixed slack covers: there the camera pool
refuses (state unchanged) and the caller lets the side that is behind catch up, as with StreamPool.  So for the lag and lead schedules
"a push the outer pool accepted" is one the camera oracle accepted; the C planner of the inner pool must accept exactly those."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import live_oracle as VO
from tests import live_video_oracle as LV
from tests.test_live_host import MODES, PLANS, c_tick, flush_lengths

LL = ctypes.c_longlong
TRACKS = [0, 1, 2, 3, 4, 5, 12, 53]
SPF = 640


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def c_vtick(counters, ids, ms, slots, max_frames, flush):
    """rtfs_live_video_plan on the named slots of ``counters`` (dict slot -> (g, v, side)) -> (rc, new, table, sizes, refused)."""
    R = len(ids)
    cnt = [v for s in ids for v in counters.get(s, (0, 0, 0))]
    new, table, sizes, refused = (LL * (3 * R))(*([-7] * 3 * R)), (LL * (8 * R))(*([-7] * 8 * R)), (LL * 3)(*([-7] * 3)), (ctypes.c_int * 2)()
    rc = lib().rtfs_live_video_plan((LL * max(R, 1))(*ids), (LL * max(3 * R, 1))(*cnt), None if flush else (LL * max(R, 1))(*ms), R, slots,
                                    int(flush), max_frames, new, table, sizes, refused)
    return rc, [tuple(new[3 * r:3 * r + 3]) for r in range(R)], list(table), list(sizes), tuple(refused)


def cycles(max_frames):
    sizes = list(LV.SIZES) + [max_frames]
    return [sizes, sizes[::-1], [1], [2, 0, 3], [max_frames], [4, 5], [7, 1, 0, 0, 2]]


@pytest.mark.parametrize("max_frames", [7, 50])
def test_planner_against_the_oracle(max_frames):
    """Three slots interleaved, slot 3 idle; every slot streams every track length one after the other (a second recording after each
    flush), each with another chunk-size cycle."""
    cyc = cycles(max_frames)
    counters = {s: (0, 0, 0) for s in range(4)}
    ticks = 0
    for j in range(len(TRACKS)):
        sch = {s: LV.chunking(TRACKS[(j + s) % len(TRACKS)], cyc[(j + 2 * s) % len(cyc)], start=s) or [0] for s in range(3)}
        emitted = {s: [] for s in range(3)}
        for kind, ids, ms in LV.events(sch):
            flush = kind == "flush"
            want = LV.tick(counters, ids, ms, max_frames, flush)
            rc, new, table, sizes, refused = c_vtick(counters, ids, ms or [], 4, max_frames, flush)
            assert rc == 0 and refused == (-1, 0), (kind, ids, ms, counters)
            assert new == [want["new"][s] for s in ids] and table == want["table"], (kind, ids, ms, counters)
            assert sizes == [len(want["rows"]), want["floats"], want["max_m"]]
            assert all(o % LV.ALIGN == 0 for o in want["off"])
            for s, rng in zip(ids, want["ranges"]):
                emitted[s] += list(range(*rng))
            counters = want["new"]
            ticks += 1
        for s in range(3):
            assert emitted[s] == list(range(TRACKS[(j + s) % len(TRACKS)])) and counters[s] == (0, 0, 0)
        assert counters[3] == (0, 0, 0)
    assert ticks > 100


@pytest.mark.parametrize("Tv", TRACKS)
def test_emitted_ranges_tile_the_track_and_read_five_frames(Tv):
    """From the oracle alone: for every chunking the emitted index ranges tile [0, Tv) exactly once and in order, every frame an
    embedding reads has arrived when it is emitted, and the frames read are q - 2 .. q + 2 clipped to [0, Tv)."""
    for cyc in cycles(9):
        for start in range(len(cyc)):
            c, got, read = (0, 0), [], {}
            for m in LV.chunking(Tv, cyc, start):
                c, (lo, hi) = LV.push_one(c, m, 9)
                for q in range(lo, hi):
                    assert q + 2 < c[0]  # mid-stream: nothing is ever zero-filled behind the frames received
                    read[q] = LV.reads(q, c[0])
                got += list(range(lo, hi))
            assert c[0] == Tv and c[1] == max(0, Tv - 2)
            _, (lo, hi) = LV.flush_one(c)
            for q in range(lo, hi):
                read[q] = LV.reads(q, Tv)
            got += list(range(lo, hi))
            assert got == list(range(Tv))
            for q in range(Tv):
                assert read[q] == [p for p in range(q - 2, q + 3) if 0 <= p < Tv]
    if Tv in (1, 2):  # embedded wholly at the flush, both paddings inside one receptive field
        c, rng = LV.push_one((0, 0), Tv, 9)
        assert rng == (0, 0) and LV.flush_one(c)[1] == (0, Tv)


def test_planner_refusals_leave_everything_unwritten():
    ok = {0: (5, 3, 1), 1: (0, 0, 0), 2: (1, 0, 1)}
    cases = [([3], [1], False, 2), ([-1], [1], False, 2), ([0, 0], [1, 1], False, 3), ([1, 2, 1], [0, 0, 0], True, 3),
             ([0], [8], False, 4), ([0], [-1], False, 4), ([1, 0], [7, 8], False, 4)]  # a good slot first
    for ids, ms, flush, reason in cases:
        rc, new, table, sizes, refused = c_vtick(ok, ids, ms, 3, 7, flush)
        assert rc == -4 and refused[1] == reason, (ids, ms, refused)
        assert refused[0] == (len(ids) - 1 if reason != 2 else 0)
        assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
        with pytest.raises(LV.Refused):
            LV.tick(ok, ids, ms, 7, flush)
    # counters the planner cannot have produced: negative, v > g, v < max(0, g - 2), a side that is no side
    for bad in [(-1, 0, 0), (3, -1, 0), (3, 4, 0), (5, 2, 0), (3, 0, 1), (2, 1, 2), (2, 1, -1)]:
        for flush in (False, True):
            rc, new, table, sizes, refused = c_vtick({0: (4, 2, 0), 1: bad}, [0, 1], [1, 1], 2, 7, flush)
            assert rc == -4 and refused == (1, 8), (bad, flush)
            assert set(v for c in new for v in c) == {-7} and set(table) == {-7} and set(sizes) == {-7}
            with pytest.raises(LV.Refused):
                LV.tick({0: (4, 2, 0), 1: bad}, [0, 1], [1, 1], 7, flush)
    for good in [(3, 1, 0), (3, 2, 1), (3, 3, 0), (0, 0, 1), (2, 0, 0)]:  # the whole accepted band of v
        assert c_vtick({0: good}, [0], [0], 1, 7, False)[0] == 0
    # R < 1, no slots, no frames allowed, a missing array
    assert c_vtick({}, [], [], 3, 7, False)[4] == (-1, 1)
    assert c_vtick(ok, [0], [1], 0, 7, False)[4] == (-1, 1)
    assert c_vtick(ok, [0], [0], 3, 0, False)[4] == (-1, 1)
    refused = (ctypes.c_int * 2)()
    assert lib().rtfs_live_video_plan((LL * 1)(0), (LL * 3)(0, 0, 0), None, 1, 1, 0, 7, None, None, None, refused) == -4 and tuple(refused) == (-1, 1)
    assert lib().rtfs_live_video_plan((LL * 1)(0), (LL * 3)(4, 2, 0), None, 1, 1, 1, 7, None, None, None, None) == 0  # every output may be NULL


def _video():
    import rtfs_net_amd as R
    return R.FRCNNVideoModel(print_macs=False).eval()


def _audio():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    return R.AVNet(print_macs=False, **copy.deepcopy(audionet_config(2, "SRU"))).eval()


def test_open_refusals():
    import rtfs_net_amd as R
    vm = _video()
    for kw in (dict(slots=0), dict(max_frames=0), dict(max_batch_frames=0), dict(roi_hw=(87, 96)), dict(roi_hw=(96, 80)), dict(roi_hw=(96,)),
               dict(roi_hw=96), dict(max_frames=2.5), dict(slots="2")):
        with pytest.raises(ValueError):
            vm.open_streams(**dict(dict(slots=2), **kw))
    vm.train()
    with pytest.raises(RuntimeError, match="inference only"):
        vm.open_streams(2)
    vm.eval()
    pool = vm.open_streams(2, max_frames=5, roi_hw=(96, 100))
    assert isinstance(pool, R.LipStreamPool) and pool.counters(1) == (0, 0)
    sys_ = R.System(audio_model=_audio(), video_model=vm)
    for kw in (dict(window=32001), dict(hop=0), dict(max_chunk=641), dict(max_chunk=0), dict(slots=0), dict(max_batch=0), dict(roi_hw=(80, 96)),
               dict(window=2560, max_chunk=(1 << 24) // 640 * 640 - 2560)):  # the inner ring is 1280 longer than the outer sizes say
        with pytest.raises(ValueError):
            sys_.open_camera_streams(**dict(dict(slots=2), **kw))
    with pytest.raises(ValueError, match="no video model"):
        R.System(audio_model=_audio()).open_camera_streams(2)
    cam = sys_.open_camera_streams(2, window=2560, hop=1280)
    assert isinstance(cam, R.CameraStreamPool) and cam.audio.max_chunk == 2560 + 1280 and cam.lips.max_frames == 4 and cam.lips.roi_hw == (96, 96)
    assert isinstance(sys_.open_streams(slots=1, window=1280, hop=640), R.StreamPool)  # the embedding entry stays as it was


def test_every_refusal_on_cpu_tensors_comes_before_any_device_call():
    """The pools lie on the CPU here, where a tick that got past its checks raises RuntimeError (there is no CPU arithmetic): every bad
    argument must raise ValueError instead, with all counters unchanged."""
    import rtfs_net_amd as R
    vm = _video()
    pool = vm.open_streams(3, max_frames=5, roi_hw=(96, 100))
    u8, f32 = torch.zeros(2, 96, 100, dtype=torch.uint8), torch.zeros(2, 88, 88)
    bad = [([3], [u8]), ([-1], [u8]), ([0, 0], [u8, u8]), ([1.0], [u8]), ([True], [u8]), ([0, 1], [u8]), (0, [u8]), ([0], u8[0]), ([0], 3),
           ([0], [None]), ([0, 1], [u8, f32]), ([0], [u8.to(torch.int32)]), ([0], [f32.double()]), ([0], [f32.half()]),
           ([0], [torch.zeros(2, 96, 96, dtype=torch.uint8)]), ([0], [torch.zeros(2, 100, 96, dtype=torch.uint8)]), ([0], [torch.zeros(2, 96, 100)]),
           ([0], [torch.zeros(2, 1, 88, 88)]), ([0], [torch.zeros(88, 88)]), ([0], [torch.zeros(6, 88, 88)]),
           ([1, 0], [u8, torch.zeros(6, 96, 100, dtype=torch.uint8)]), ([0], [u8.to("meta")])]
    for ids, chunks in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks)
        assert [pool.counters(s) for s in range(3)] == [(0, 0)] * 3, (ids,)
    for ids in ([0, 0], [3], [0.5]):
        with pytest.raises(ValueError):
            pool.flush(ids)
        with pytest.raises(ValueError):
            pool.reset(ids)
    with pytest.raises(RuntimeError, match="MI355X only"):  # a good push reaches the device path
        pool.push([0], [u8])
    assert pool.push([], []) == [] and pool.flush([]) == []
    free = vm.open_streams(1, max_frames=5)  # roi_hw None: fixed by the first ROIs, which must be at least 88 x 88
    with pytest.raises(ValueError):
        free.push([0], [torch.zeros(1, 80, 96, dtype=torch.uint8)])
    assert free.roi_hw is None
    vm.train()
    with pytest.raises(RuntimeError, match="inference only"):
        pool.push([0], [u8])
    vm.eval()
    # the camera pool: what either side refuses, before anything moves
    cam = R.System(audio_model=_audio(), video_model=vm).open_camera_streams(2, window=2560, hop=1280, roi_hw=(96, 96))
    a, r = torch.zeros(1000), torch.zeros(2, 96, 96, dtype=torch.uint8)
    bad = [([2], [a], [r]), ([0, 0], [a, a], [r, r]), ([0], [a, a], [r]), ([0], [a], [r, r]), ([0], a, [r]), ([0], [torch.zeros(2561)], [r]),
           ([0], [a], [torch.zeros(5, 96, 96, dtype=torch.uint8)]), ([0], [a.double()], [r]), ([0], [torch.zeros(2, 500)], [r]), ([0], [None], [r]),
           ([0], [a], [torch.zeros(2, 96, 100, dtype=torch.uint8)]), ([0], [a.to("meta")], [r]), ([1, 0], [a, a], [r, torch.zeros(2, 88, 88)])]
    for ids, wavs, rois in bad:
        with pytest.raises(ValueError):
            cam.push(ids, wavs, rois)
        assert [cam.counters(s) for s in range(2)] == [((0, 0, 0, 0), (0, 0))] * 2, (ids,)
    for ids in ([0, 0], [2]):
        with pytest.raises(ValueError):
            cam.flush(ids)
        with pytest.raises(ValueError):
            cam.reset(ids)
    with pytest.raises(RuntimeError, match="MI355X only"):
        cam.push([0], [a], [r])
    assert cam.counters(0) == ((0, 0, 0, 0), (0, 0))


def _inner_c(ca, na, k, window, hop, chunk):
    rc, new, _, _, refused = c_tick({0: ca}, [0], [na], [k], 1, window, hop, chunk, 1, False)
    return rc, new[0], refused


@pytest.mark.parametrize("window,hop", PLANS)
def test_the_inner_pool_needs_its_1280_samples_of_slack_and_no_more(window, hop):
    mc = window
    sizes = VO.chunk_sizes(hop, mc)
    refused_plain = {"in step": 0, "step": 0, "lag": 0, "lead": 0}
    for j, L in enumerate(flush_lengths(window, hop, mc)):
        Tv = max(1, -(-L // SPF) - (2 if j % 3 == 1 else 0))
        schedules = [("in step", [(na, nf, False) for na, nf in LV.in_step(L, sizes, mc, start=j)])]
        schedules += [(mode, LV.camera_schedule(L, Tv, sizes, mode, window, hop, mc, mc + LV.SLACK, start=j)) for mode in MODES]
        for mode, sch in schedules:
            assert mode != "in step" or not any(rep for _, _, rep in sch)
            ca, cv, plain = (0, 0, 0, 0), (0, 0), True
            pa, pv = ca, cv  # the same pushes into an inner pool of plain max_chunk, until it refuses one
            for na, nf, _ in sch:
                ca1, cv1, _, _ = LV.camera_push(ca, cv, na, nf, window, hop, mc, mc + LV.SLACK)  # accepted by the outer pool (raises otherwise)
                rc, new, refused = _inner_c(ca, na, cv1[1] - cv[1], window, hop, mc + LV.SLACK)
                assert rc == 0 and new == ca1, (mode, L, ca, cv, na, nf, refused)
                ca, cv = ca1, cv1
                if plain:
                    try:
                        pa1, pv1, _, _ = LV.camera_push(pa, pv, na, nf, window, hop, mc, mc)
                        assert _inner_c(pa, na, pv1[1] - pv[1], window, hop, mc)[0] == 0
                        pa, pv = pa1, pv1
                    except VO.Refused:
                        rc, _, refused = _inner_c(pa, na, max(pv[1], pv[0] + nf - 2) - pv[1], window, hop, mc)
                        assert rc == -4 and refused[1] in (5, 6), (mode, L, pa, pv, na, nf)
                        refused_plain[mode] += 1
                        plain = False
            assert ca[0] == L and cv[0] == (-(-L // SPF) if mode == "in step" else Tv)
            # the flush: the at most two embeddings still owed always fit, and the inner flush follows on the counters they leave
            k = cv[0] - cv[1]
            rc, mid, refused = _inner_c(ca, 0, k, window, hop, mc + LV.SLACK)
            assert 0 <= k <= 2 and rc == 0 and mid[1] == cv[0], (mode, L, ca, cv, refused)
            assert c_tick({0: mid}, [0], None, None, 1, window, hop, mc + LV.SLACK, 1, True)[0] == 0
            assert LV.camera_flush(ca, cv, window, hop, mc + LV.SLACK)[3][1] == L
    print(f"[camera host] window {window} hop {hop}: schedules refused by an inner pool of plain max_chunk: {refused_plain}")
    assert refused_plain["in step"] >= 1 and sum(refused_plain.values()) >= 2


def test_in_step_streams_never_stand_further_ahead_than_window_plus_1279():
    """The argument behind the slack, checked on the counters: in step, a - e hop <= window + 1279 after every tick."""
    for window, hop in PLANS:
        mc = window
        for j, L in enumerate(flush_lengths(window, hop, mc)):
            ca, cv = (0, 0, 0, 0), (0, 0)
            for na, nf in LV.in_step(L, VO.chunk_sizes(hop, mc), mc, start=j):
                ca, cv, _, _ = LV.camera_push(ca, cv, na, nf, window, hop, mc, mc + LV.SLACK)
                assert ca[0] - ca[2] * hop <= window + 1279 or ca[0] == L, (window, hop, L, ca)
