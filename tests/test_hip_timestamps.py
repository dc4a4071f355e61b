"""Live streams with per-frame timestamps on the device (FRCNNVideoModel.open_streams(timebase=) / StampLipStreamPool,
System.open_camera_streams(timebase=), System.separate_recording(timestamps=), rtfs_live_video_ingest_stamp_u8 / _f32,
rtfs_live_video_stamp_reset) against tests/timestamp_oracle.py (the rule, by brute force) and tests/live_video_oracle.py (the windows):

1. ingest is a gather: every tick's stem input, both history buffers and the held plane bit-equal to the oracle's selection of the
   prepared frames; what a push does not own stays as it was;
2. constant-rate stamps with until at the next frame's nominal time equal the frame_rate= pool tick by tick (torch.equal);
3. chunking does not matter: a stamp pool and a pool at 25 fps fed, at the same ticks, the frames the oracle selects (the held frame
   included) give torch.equal outputs tick by tick;
4. streams equal video_model on the oracle-selected whole track (tests/util.rel_err <= 1e-4, as test_streams_equal_the_whole_track);
5. the smallest cases where the new kernel path can go wrong, each by name;
6. the camera pool end to end through a 0.4 s camera dropout against System.separate_recording(timestamps=), and that against
   host-selected ROIs;
7. refusals launch nothing and leave no trace;
8. without timebase= today's classes and torch.equal results;
9. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import ctypes
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import frame_rate_oracle as FR
from tests import live_video_oracle as LV
from tests import timestamp_oracle as TS
from tests.test_hip_live_video import offset_f32, offset_u8, rois
from tests.test_hip_longform import dev, host, lib, model
from tests.test_hip_many import video_model
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
MAXF = 7
RATES = [Fraction(30), Fraction(60), Fraction(15), Fraction(10), Fraction(30000, 1001)]
HW = [(96, 96), (91, 101), (88, 88)]
CYCLES = [[1, 2, 0, 3, MAXF], [1], [2, 0, 3], [MAXF], [MAXF, 3, 0, 2, 1]]
UNTILS = [[None], ["next"], [None, "mid", "tick", None, "next"], ["tick", None]]


def bits(t):
    return t.view(torch.int32)


def random_stamps(rng, tb, n, late=3):
    """Gaps from one tick of the timebase to half a second, bursts inside one 40 ms tick, a first frame up to ``late`` ticks late."""
    t = rng.choice([0, rng.randrange(0, late * tb // 25 + 1)])
    out = []
    for _ in range(n):
        out.append(t)
        kind = rng.random()
        if kind < 0.1:
            t += 1
        elif kind < 0.35:
            t += rng.randrange(1, tb // 100)
        elif kind < 0.85:
            t += rng.randrange(tb // 40, tb // 20)
        else:
            t += rng.randrange(tb // 10, tb // 2 + 1)
    return out


def schedule(stamps, tb, cycle, untils, start=0, max_final=MAXF):
    """[(camera frames, until)] that deliver ``stamps``: chunk sizes cycle through ``cycle``, the until of a push through ``untils`` (None,
    "next": the next frame's stamp, "mid": half way to it, "tick": one 40 ms tick on).  A push the pool would refuse because too many
    model frames became final is cut down, and a gap that no single push can cross is walked with empty pushes that carry an until."""
    st, out, pos, i = TS.Stream(tb), [], 0, start
    while pos < len(stamps):
        k, mode = min(cycle[i % len(cycle)], len(stamps) - pos), untils[i % len(untils)]
        i += 1
        while True:
            ts = stamps[pos:pos + k]
            nxt = stamps[pos + k] if pos + k < len(stamps) else stamps[-1] + tb // 25
            lo = ts[-1] if ts else st.W
            until = {None: None, "next": nxt, "mid": (lo + nxt) // 2, "tick": min(nxt, lo + tb // 25), "walk": min(nxt, st.W + max_final * tb // 25)}[mode]
            trial = st.clone()
            try:
                trial.push(ts, until or 0, max_final)
                break
            except TS.Refused:
                if mode not in (None, "walk"):
                    mode = None
                elif k > 1:
                    k -= 1
                else:
                    assert st.n > 0 and mode is None, (stamps, pos)
                    k, mode = 0, "walk"
        st = trial
        out.append((k, until))
        pos += k
    return out


def drive(pool, tb, tracks, stamps, sched, kind, flush_until=None, check=False, offsets=False, twin=None, twin_src=None):
    """Stream tracks[s] (uint8 (n,H,W), CAMERA frames stamped stamps[s]) through slot s by sched[s] = [(camera frames, until)], a flush
    (with flush_until[s]) in the tick after a slot's last push.  kind "u8" pushes the ROIs, "f32" the frames prepared by the oracle.
    ``check``: every tick's windows, history, held planes and counters against the oracles.  ``twin``: a pool at 25 fps that is fed, at
    the same ticks, the frames the oracle selects (from twin_src[s], on the device) and must answer bit for bit.
    Returns slot -> (512, g_end) concatenated embeddings, slot -> the camera frame each model frame showed."""
    flush_until = flush_until or {}
    prepared = {s: LV.prepare_u8(t) for s, t in tracks.items()}
    st = {s: TS.Stream(tb) for s in tracks}
    v, side, hside, pos = ({s: 0 for s in tracks} for _ in range(4))
    src, got, tickno = {s: [] for s in tracks}, {s: [] for s in tracks}, 0
    sel = lambda s: prepared[s][np.array(src[s], dtype=np.int64)]  # noqa: E731
    for i in range(max(len(x) for x in sched.values()) + 1):
        for flush in (True, False):
            ids = [s for s, x in sched.items() if (len(x) == i if flush else len(x) > i)]
            if not ids:
                continue
            before = (pool._hist.clone(), pool._held.clone()) if check else None
            rows, ks, new = [], [], {}
            if flush:
                untils = [flush_until.get(s) for s in ids]
                for s, u in zip(ids, untils):
                    new[s] = st[s].flush(u or 0, pool.max_frames)
                    src[s] += new[s]
                    rows += [(s, q) for q in range(v[s], len(src[s]))]
                    ks.append(len(src[s]) - v[s])
                outs = pool.flush(ids, untils)
                if twin is not None:
                    # a flush that finalises frames embeds them in one tick, the twin would need two: compared where it finalises none
                    assert all(not new[s] for s in ids), "the twin comparison needs schedules whose flush finalises nothing"
                    for s, x, y in zip(ids, outs, twin.flush(ids)):
                        assert x.shape == y.shape and torch.equal(x, y), ("flush", s)
            else:
                chunks, tss, untils, ms = [], [], [], []
                for s in ids:
                    k, u = sched[s][i]
                    ts = stamps[s][pos[s]:pos[s] + k]
                    new[s] = st[s].push(ts, u or 0, pool.max_frames)
                    src[s] += new[s]
                    v1 = max(v[s], len(src[s]) - 2)
                    rows += [(s, q) for q in range(v[s], v1)]
                    ks.append(v1 - v[s])
                    frames = tracks[s] if kind == "u8" else prepared[s]
                    off = 1 + (tickno + s) % 3 if offsets and kind == "u8" else (1 if offsets else 0)
                    chunks.append((offset_u8 if kind == "u8" else offset_f32)(frames[pos[s]:pos[s] + k], off))
                    tss.append(torch.tensor(ts, dtype=torch.int64) if (tickno + s) % 2 else ts)  # both forms of host stamps
                    untils.append(u)
                    ms.append(k)
                outs = pool.push(ids, chunks, tss, untils)
                if twin is not None:
                    chosen = [twin_src[s][torch.tensor(new[s], dtype=torch.int64, device="cuda")] for s in ids]
                    for s, x, y in zip(ids, outs, twin.push(ids, chosen)):
                        assert x.shape == y.shape and torch.equal(x, y), ("push", i, s)
            tickno += 1
            assert len(outs) == len(ids)
            if check:
                exp = LV.windows(rows, {s: sel(s) for s in ids}, {s: len(src[s]) for s in ids})
                win = host(pool._win[:len(rows)])
                assert np.array_equal(win.view(np.uint32), exp.view(np.uint32)), f"windows differ in tick {i} flush {flush} {ids}"
                hist, held = host(pool._hist), host(pool._held)
                for r, s in enumerate(ids):
                    if flush:  # the reset gives history and held planes defined contents
                        assert not hist[s].any() and not held[s].any(), s
                        continue
                    m, k = len(new[s]), ms[r]
                    if m == 0:  # no model frame became final: the history is not written
                        assert torch.equal(bits(pool._hist[s]), bits(before[0][s])), (i, s)
                    else:
                        assert torch.equal(bits(pool._hist[s, side[s]]), bits(before[0][s, side[s]])), (i, s)  # the side that was read
                        for plane, frame in LV.history(sel(s), len(src[s])).items():
                            assert np.array_equal(hist[s, 1 - side[s], plane], frame), (i, s, plane)
                    assert torch.equal(bits(pool._held[s, hside[s]]), bits(before[1][s, hside[s]])), (i, s)  # the side that was read
                    if k == 0:  # no camera frame arrived: the held plane stays
                        assert torch.equal(bits(pool._held[s]), bits(before[1][s])), (i, s)
                    else:  # the last camera frame received, whether a model frame shows it or not
                        assert np.array_equal(held[s, 1 - hside[s]], prepared[s][pos[s] + k - 1]), (i, s)
                for s in set(range(pool.slots)) - set(ids):  # ... and nobody else's state moves
                    assert torch.equal(bits(pool._hist[s]), bits(before[0][s])) and torch.equal(bits(pool._held[s]), bits(before[1][s])), s
            for r, (s, out) in enumerate(zip(ids, outs)):
                assert tuple(out.shape) == (512, ks[r]), (i, flush, s, tuple(out.shape), ks[r])
                got[s].append(host(out))
                if flush:
                    v[s] = side[s] = hside[s] = pos[s] = 0
                else:
                    m, k = len(new[s]), ms[r]
                    v[s], pos[s] = v[s] + ks[r], pos[s] + k
                    side[s], hside[s] = (1 - side[s] if m else side[s]), (1 - hside[s] if k else hside[s])
                    assert pool._counters[s][2] == side[s] and pool._counters[s][6] == hside[s]
                assert pool.counters(s) == (pos[s], v[s])
    return {s: np.concatenate(g, axis=1) for s, g in got.items()}, src


def scenario(seed, tb, H, W, lengths=(37, 13, 7)):
    rng = random.Random(seed)
    tracks = {s: rois(n, H, W, seed + s) for s, n in enumerate(lengths)}
    stamps = {s: random_stamps(rng, tb, n) for s, n in enumerate(lengths)}
    sched = {s: schedule(stamps[s], tb, CYCLES[(seed + 2 * s) % len(CYCLES)], UNTILS[(seed + s) % len(UNTILS)], start=s) for s in tracks}
    fu = {s: [None, stamps[s][-1] + tb // 10, None][(seed + s) % 3] for s in tracks}
    return tracks, stamps, sched, fu


def whole_map(stamps, tb, sched, flush_until):
    top = max([u or 0 for _, u in sched] + [flush_until or 0])
    return TS.frame_map(stamps, tb, top)


# ---------------------------------------------------------------- 1. ingest is a gather
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("j", range(4))
def test_ingest_is_a_gather(j, kind):
    tb, (H, W) = (1000, 90000)[j % 2], HW[j % 3]
    pool = video_model().open_streams(4, max_frames=MAXF, roi_hw=(H, W), timebase=tb)  # slot 3 idle
    tracks, stamps, sched, fu = scenario(j, tb, H, W)
    got, src = drive(pool, tb, tracks, stamps, sched, kind, flush_until=fu, check=True, offsets=True)
    for s, t in tracks.items():
        assert src[s] == whole_map(stamps[s], tb, sched[s], fu[s])
        assert got[s].shape == (512, len(src[s])) and np.isfinite(got[s]).all()


# ---------------------------------------------------------------- 2. constant-rate stamps
def rate_lengths(rate, tb):
    """Track lengths whose last camera frame is shown by the rate rule too (its tick is not shared with the frame that would follow), so
    that both pools end the stream on the same model frame: a stamp pool always shows the last frame on its own tick."""
    step = TS.constant_rate(2, rate, tb)[1]
    ok = [n for n in range(1, 38) if TS.tick((n - 1) * step, tb) + 1 <= FR.count(n, rate)]
    return [ok[0], ok[len(ok) // 3], ok[-1]]


@pytest.mark.parametrize("rate", RATES + [Fraction(25)], ids=lambda r: f"{r.numerator}_{r.denominator}")
def test_constant_rate_stamps_equal_the_rate_pool(rate):
    tb, vm = 90000, video_model()
    j = (RATES + [Fraction(25)]).index(rate)
    step = TS.constant_rate(2, rate, tb)[1]
    lengths = rate_lengths(rate, tb)
    a = vm.open_streams(3, max_frames=18, roi_hw=(96, 96), timebase=tb)  # 7 camera frames at 10 fps make 18 model frames final
    b = vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96), frame_rate=rate)
    import rtfs_net_amd as R
    assert type(a) is R.StampLipStreamPool and type(b) is (R.LipStreamPool if rate == 25 else R.RateLipStreamPool)
    tracks = {s: dev(rois(n, 96, 96, 50 + j + s)) for s, n in enumerate(lengths)}
    sch = {s: LV.chunking(n, CYCLES[(j + s) % len(CYCLES)], start=s) for s, n in enumerate(lengths)}
    ncam, total = {s: 0 for s in tracks}, {s: 0 for s in tracks}
    for what, ids, ms in LV.events(sch):
        if what == "flush":
            oa, ob = a.flush(ids), b.flush(ids)
        else:
            chunks = [tracks[s][ncam[s]:ncam[s] + m] for s, m in zip(ids, ms)]
            oa = a.push(ids, chunks, [[(ncam[s] + i) * step for i in range(m)] for s, m in zip(ids, ms)],
                        [(ncam[s] + m) * step for s, m in zip(ids, ms)])
            ob = b.push(ids, chunks)
            for s, m in zip(ids, ms):
                ncam[s] += m
        for s, x, y in zip(ids, oa, ob):
            assert x.shape == y.shape and torch.equal(x, y), (rate, what, ids, ms, s)
            total[s] += x.shape[1]
    assert [total[s] for s in range(3)] == [FR.count(n, rate) for n in lengths]


def test_the_last_camera_frame_is_shown_by_its_own_tick():
    """One frame at 60 fps: the rate rule gives no model frame (frame 1 would take tick 0); a stamped stream that ends there shows it."""
    vm = video_model()
    t = dev(rois(1, 96, 96, 5))
    a, b = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), timebase=90000), vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), frame_rate=60)
    assert a.push([0], [t], [[0]], 1500)[0].shape == b.push([0], [t])[0].shape == (512, 0)
    out = a.flush([0])[0]
    assert b.flush([0])[0].shape == (512, 0) and out.shape == (512, 1)
    with torch.no_grad():
        ref = host(vm(dev(LV.prepare_u8(host(t)))[None, None]))[0]
    assert rel_err(host(out), ref) <= 1e-4


# ---------------------------------------------------------------- 3. chunking does not matter
@pytest.mark.parametrize("j", range(4))
def test_a_pool_at_25_fed_the_selected_frames_agrees_tick_by_tick(j):
    tb, kind, vm = (90000, 1000)[j % 2], ("u8", "f32")[j % 2], video_model()
    a = vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96), timebase=tb)
    b = vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96))
    tracks, stamps, sched, _ = scenario(10 + j, tb, 96, 96, lengths=(37, 2, 13))
    for s in tracks:  # a last, empty push whose until makes the last frame's tick final: the flush then finalises nothing
        sched[s] = sched[s] + [(0, stamps[s][-1] + tb // 25)]
    twin_src = {s: dev(t) if kind == "u8" else dev(LV.prepare_u8(t)) for s, t in tracks.items()}
    got, src = drive(a, tb, tracks, stamps, sched, kind, twin=b, twin_src=twin_src)
    for s in tracks:
        assert src[s] == whole_map(stamps[s], tb, sched[s], None) and got[s].shape == (512, len(src[s]))
        assert b.counters(s) == (0, 0)


# ---------------------------------------------------------------- 4. equal to the whole track
def test_streams_equal_the_selected_whole_track():
    from rtfs_net_amd import datas
    vm, worst, held = video_model(), 0.0, 0
    for j, tb in enumerate((1000, 90000, 1000)):
        pool = vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96), timebase=tb)
        tracks, stamps, sched, fu = scenario(20 + j, tb, 96, 96, lengths=[(37, 13, 1), (7, 3, 37), (2, 37, 13)][j])
        got, src = drive(pool, tb, tracks, stamps, sched, "u8", flush_until=fu)
        for s, t in tracks.items():
            top = max([u or 0 for _, u in sched[s]] + [fu[s] or 0])
            idx = datas.timestamp_map(stamps[s], tb, top)
            assert idx == src[s] == TS.frame_map(stamps[s], tb, top) and len(idx) >= 1
            with torch.no_grad():
                ref = host(vm(dev(LV.prepare_u8(t)[np.array(idx)])[None, None]))[0]
            e = rel_err(got[s], ref)
            worst = max(worst, e)
            assert got[s].shape == ref.shape and np.isfinite(got[s]).all() and e <= 1e-4, (tb, s, e)
    print(f"[timestamps] streams vs video_model(selected whole track): worst rel_err {worst:.3e} (exactly 0: {worst == 0.0})")


# ---------------------------------------------------------------- 5. the smallest cases, by name
def run_case(stamps, sched, flush_until=None, tb=1000, kind="u8", pool=None, seed=1, want=None):
    """One stream on slot 1 of two with every tick checked against the oracles, then against video_model on the selected whole track."""
    vm = video_model()
    pool = pool or vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96), timebase=tb)
    track = rois(len(stamps), 96, 96, seed)
    got, src = drive(pool, tb, {1: track}, {1: stamps}, {1: sched}, kind, flush_until={1: flush_until}, check=True, offsets=True)
    assert sum(k for k, _ in sched) == len(stamps) and (want is None or src[1] == want), src[1]
    with torch.no_grad():
        ref = host(vm(dev(LV.prepare_u8(track)[np.array(src[1])])[None, None]))[0]
    assert got[1].shape == ref.shape and rel_err(got[1], ref) <= 1e-4
    return pool, src[1]


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_gap_across_a_push_boundary_reads_the_held_plane(kind):
    """Camera frame 2 (95 ms, tick 2) is the last of its push and not final there: W = 95 makes model frames 0 and 1 final.  The next
    frame comes at 200 ms: model frames 2, 3 and 4 show frame 2, which no model frame has shown and the history does not hold (its
    plane (g - 1) & 3 = 1 holds frame 1)."""
    run_case([0, 40, 95, 200, 240], [(3, None), (2, None)], kind=kind, want=[0, 1, 2, 2, 2, 3, 4])


def test_frames_without_a_final_model_frame_then_an_until_without_frames():
    """The first push brings a frame and finalises nothing (the held plane follows, the history side does not); the second brings no
    frame and its until finalises three model frames, all from the held plane."""
    pool, _ = run_case([0, 130], [(1, None), (0, 100), (1, None)], want=[0, 0, 0, 1])
    # ... and two such pushes in a row: the held side flips twice, the history side not at all
    run_case([0, 10, 130], [(1, None), (1, None), (0, 100), (1, None)], want=[1, 1, 1, 2], pool=pool, seed=2)


def test_an_until_that_finalises_max_frames_model_frames_from_the_held_plane():
    """g = 1 after two frames; until = 300 ms gives G = 8: seven model frames at once, all showing the held frame 1, so the four history
    writers read the held plane too.  One tick more is refused and changes nothing."""
    vm = video_model()
    pool = vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96), timebase=1000)
    track = dev(rois(2, 96, 96, 3))
    pool.push([1], [track], [[0, 40]])
    state = [list(c) for c in pool._counters], pool._hist.clone(), pool._held.clone()
    with pytest.raises(ValueError, match="max_frames"):
        pool.push([1], [track[:0]], None, 340)
    with pytest.raises(ValueError, match="max_frames"):
        pool.flush([1], until=340)
    assert [list(c) for c in pool._counters] == state[0] and torch.equal(bits(pool._hist), bits(state[1])) and torch.equal(bits(pool._held), bits(state[2]))
    pool.reset([1])
    run_case([0, 40, 330], [(2, None), (0, 300), (1, None)], want=[0] + [1] * 7 + [2], pool=pool, seed=3)


def test_a_burst_of_three_frames_in_one_tick():
    """42, 47 and 52 ms share tick 1: only the last is shown; the first two are never read, also when the burst is cut by a push."""
    pool, _ = run_case([0, 42, 47, 52, 80, 120], [(6, None)], want=[0, 3, 4, 5])
    run_case([0, 42, 47, 52, 80, 120], [(2, None), (1, None), (1, None), (2, 160)], want=[0, 3, 4, 5], pool=pool, kind="f32")


def test_a_first_frame_three_ticks_late():
    run_case([120, 160, 200], [(0, 100), (1, None), (2, None)], want=[0, 0, 0, 0, 1, 2])


def test_flush_with_and_without_until():
    """Without until the stream ends on the last frame's own tick; with until the last frame is carried on."""
    pool, a = run_case([0, 40, 80], [(3, None)], want=[0, 1, 2])
    _, b = run_case([0, 40, 80], [(3, None)], flush_until=240, want=[0, 1, 2, 2, 2, 2], pool=pool)
    # a slot reused after a flush: the stamps restart at 0 although the watermark had reached 240
    run_case([0, 35, 90], [(1, 30), (2, None)], flush_until=0, want=[0, 1, 2], pool=pool, seed=4)


# ---------------------------------------------------------------- 6. end to end
def test_camera_streams_bridge_a_dropout_and_equal_separate_recording():
    """16 kHz audio in pushes of 80 ms; the camera runs at about 30 fps, loses 0.4 s and comes back.  Every push carries until = the end
    of its audio, so the empty pushes of the dropout keep the model frames coming (they show the last frame before the dropout)."""
    import rtfs_net_amd as R
    window, hop, mc, tb = 2560, 1280, 2560, 1000
    L = 6 * window + 7  # 0.96 s: 24 or 25 model frames, by the last camera frame's tick
    system = R.System(audio_model=model(4), video_model=video_model())
    pool = system.open_camera_streams(2, window=window, hop=hop, max_chunk=mc, max_batch=4, roi_hw=(96, 96), timebase=tb)
    assert type(pool) is R.CameraStreamPool and type(pool.lips) is R.StampLipStreamPool and pool.lips.max_frames == 4
    rng = np.random.RandomState(L)
    wavs = {s: (0.1 * rng.randn(L)).astype(np.float32) for s in range(2)}
    stamps = {0: [0, 33, 67, 100, 133, 167, 200] + [600 + (100 * i) // 3 for i in range(11)],
              1: [20, 53, 87, 120, 161, 162, 195] + [640 + (100 * i) // 3 for i in range(10)]}
    tracks = {s: dev(rois(len(stamps[s]), 96, 96, 70 + s)) for s in range(2)}
    got, pos, a, empties, top = {s: [] for s in range(2)}, {s: 0 for s in range(2)}, 0, 0, 0
    while a < L:
        na = min(hop, L - a)
        until = (a + na) * tb // 16000
        ks = [sum(1 for t in stamps[s][pos[s]:] if t < until) for s in range(2)]
        empties += sum(k == 0 for k in ks)
        outs = pool.push([0, 1], [dev(wavs[s][a:a + na]) for s in range(2)], [tracks[s][pos[s]:pos[s] + k] for s, k in enumerate(ks)],
                         timestamps=[stamps[s][pos[s]:pos[s] + k] for s, k in enumerate(ks)], until=until)
        for s in range(2):
            got[s].append(host(outs[s]))
            pos[s] += ks[s]
        a, top = a + na, until
    assert empties >= 8 and all(pos[s] == len(stamps[s]) for s in range(2))
    for s, o in enumerate(pool.flush([0, 1])):
        got[s].append(host(o))
    worst = 0.0
    for s in range(2):
        res = np.concatenate(got[s], axis=1)
        ref = system.separate_recording(dev(wavs[s]), 16000, tracks[s], timestamps=stamps[s], timebase=tb, until=top, window=window, hop=hop)
        idx = TS.frame_map(stamps[s], tb, top)
        assert len(idx) in (24, 25) and len(set(idx)) < len(stamps[s])  # the dropout repeats a frame, the 30 fps stretches drop some
        sel = tracks[s][torch.tensor(idx, device="cuda")]
        assert torch.equal(ref, system.separate_recording(dev(wavs[s]), 16000, sel, window=window, hop=hop)), s
        e = rel_err(res, host(ref)[0])
        worst = max(worst, e)
        assert res.shape == (1, L) and np.isfinite(res).all() and e <= 1e-4, (s, e)
        assert pool.counters(s) == ((0, 0, 0, 0), (0, 0))
    print(f"[camera with timestamps] window {window} hop {hop} L {L}: worst rel_err vs separate_recording {worst:.3e}")


# ---------------------------------------------------------------- 7. refusals
def test_refusals_launch_nothing_and_leave_no_trace():
    from rtfs_net_amd import _lib
    vm, tb = video_model(), 1000
    pool = vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96), timebase=tb)
    t = dev(rois(12, 96, 96, 70))
    stamps = [0, 30, 70, 100, 135, 300, 340, 350, 420, 440, 470, 490]
    tab = torch.zeros(32, dtype=torch.int64, device="cuda")
    first = pool.push([0], [t[:5]], [stamps[:5]], 200)[0]
    torch.cuda.synchronize()
    count = lib().load().rtfs_debug_launch_count()
    before = [pool.counters(s) for s in range(2)], pool._hist.clone(), pool._held.clone(), pool._win.clone(), [list(c) for c in pool._counters]
    bad = [([2], [t[:1]], [[300]], None), ([0, 0], [t[:1]] * 2, [[300]] * 2, None), ([1, 0], [t[:1], t[:8]], [[0], list(range(300, 308))], None),
           ([0], [t[:1].cpu()], [[300]], None), ([0], [t[:1].float()], [[300]], None), ([0], [t[:1, :90]], [[300]], None), ([0], [t[0]], [[300]], None),
           ([0], [t[:2]], [[300]], None), ([0], [t[:1]], [[300, 340]], None), ([0], [t[:1]], None, None),  # a stamp count that is not m
           ([0], [t[:2]], [[300, 300]], None), ([0], [t[:2]], [[340, 300]], None), ([0], [t[:1]], [[199]], None), ([0], [t[:1]], [[135]], None),
           ([0], [t[:1]], [[-1]], None), ([1], [t[:1]], [[0]], -1), ([1], [t[:1]], [[0]], [-1]), ([0], [t[:1]], [torch.tensor([300], device="cuda")], None),
           ([0], [t[:1]], [[300]], 200 + 8 * 40 + 40), ([0], [t[:0]], None, 200 + 8 * 40), ([1, 0], [t[:1], t[:1]], [[0], [600]], None)]
    for ids, chunks, ts, until in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks, ts, until)
    for ids, until in (([0, 5], None), ([0], -1), ([0], 200 + 8 * 40)):
        with pytest.raises(ValueError):
            pool.flush(ids, until)
    for kw in (dict(timebase=0), dict(timebase=(1 << 30) + 1), dict(timebase=tb, frame_rate=30)):
        with pytest.raises(ValueError):
            vm.open_streams(2, max_frames=MAXF, **kw)
    L, P = lib().load(), _lib.ptr
    off4 = lambda x: ctypes.c_void_p(x.data_ptr() + 4)  # noqa: E731
    for bad_tb in (0, -1, (1 << 30) + 1):
        assert L.rtfs_live_video_ingest_stamp_u8(P(tab), P(pool._hist), P(pool._held), P(pool._win), 1, 0, 1, 1, 0, 96, 96, 4, 4, 0.421, 0.165, bad_tb, None) == -4
        assert L.rtfs_live_video_ingest_stamp_f32(P(tab), P(pool._hist), P(pool._held), P(pool._win), 1, 0, 1, 1, 0, bad_tb, None) == -4
    for hist, held, win, table in ((off4(pool._hist), P(pool._held), P(pool._win), P(tab)), (P(pool._hist), off4(pool._held), P(pool._win), P(tab)),
                                   (P(pool._hist), P(pool._held), off4(pool._win), P(tab)), (P(pool._hist), P(pool._held), P(pool._win), off4(tab)),
                                   (P(pool._hist), None, P(pool._win), P(tab))):
        assert L.rtfs_live_video_ingest_stamp_u8(table, hist, held, win, 1, 0, 1, 1, 0, 96, 96, 4, 4, 0.421, 0.165, tb, None) == -4
        assert L.rtfs_live_video_ingest_stamp_f32(table, hist, held, win, 1, 0, 1, 1, 0, tb, None) == -4
    assert L.rtfs_live_video_stamp_reset(None, off4(pool._hist), P(pool._held), 1, None) == -4
    assert L.rtfs_live_video_stamp_reset(None, P(pool._hist), off4(pool._held), 1, None) == -4
    assert L.rtfs_live_video_stamp_reset(None, P(pool._hist), None, 1, None) == -4
    assert lib().load().rtfs_debug_launch_count() == count
    assert [pool.counters(s) for s in range(2)] == before[0] and [list(c) for c in pool._counters] == before[4]
    assert torch.equal(bits(pool._hist), bits(before[1])) and torch.equal(bits(pool._held), bits(before[2])) and torch.equal(bits(pool._win), bits(before[3]))
    rest = torch.cat([pool.push([0], [t[5:]], [stamps[5:]])[0], pool.flush([0])[0]], dim=1)  # and the stream goes on as if nothing had been tried
    clean = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), timebase=tb)
    again = clean.push([0], [t[:5]], [stamps[:5]], 200)[0]
    assert torch.equal(first, again)
    assert torch.equal(rest, torch.cat([clean.push([0], [t[5:]], [stamps[5:]])[0], clean.flush([0])[0]], dim=1))
    assert first.shape[1] + rest.shape[1] == len(TS.frame_map(stamps, tb, 200))


# ---------------------------------------------------------------- 8. without timebase=
def test_without_a_timebase_nothing_changes():
    import rtfs_net_amd as R
    vm = video_model()
    t = dev(rois(9, 96, 96, 90))
    outs = []
    for kw in ({}, dict(timebase=None), dict(frame_rate=25, timebase=None)):
        pool = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), **kw)
        assert type(pool) is R.LipStreamPool and not hasattr(pool, "_held")
        outs.append(torch.cat([pool.push([0], [t[:4]])[0], pool.push([0], [t[4:]])[0], pool.flush([0])[0]], dim=1))
    assert outs[0].shape == (512, 9) and all(torch.equal(outs[0], o) for o in outs[1:])
    rated = []
    for kw in (dict(frame_rate=30), dict(frame_rate=30, timebase=None)):
        pool = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), **kw)
        assert type(pool) is R.RateLipStreamPool
        rated.append(torch.cat([pool.push([0], [t[:4]])[0], pool.push([0], [t[4:]])[0], pool.flush([0])[0]], dim=1))
    assert torch.equal(rated[0], rated[1])
    system = R.System(audio_model=model(4), video_model=vm)
    window, hop, L = 2560, 1280, 2560 + 1280 + 7
    wav = dev((0.1 * np.random.RandomState(1).randn(L)).astype(np.float32))
    tr = dev(rois(-(-L // SPF), 96, 96, 91))
    ref = system.separate_recording(wav, 16000, tr, window=window, hop=hop)
    assert torch.equal(ref, system.separate_recording(wav, 16000, tr, window=window, hop=hop, timestamps=None, timebase=None, until=None))
    # stamps at exactly 25 fps are the identity map
    assert torch.equal(ref, system.separate_recording(wav, 16000, tr, window=window, hop=hop, timestamps=[40 * i for i in range(tr.shape[0])], timebase=1000))
    res = []
    for kw in ({}, dict(timebase=None)):
        cam = system.open_camera_streams(1, window=window, hop=hop, max_batch=4, **kw)
        assert type(cam) is R.CameraStreamPool and type(cam.lips) is R.LipStreamPool
        res.append(torch.cat([cam.push([0], [wav[:2560]], [tr[:4]])[0], cam.push([0], [wav[2560:]], [tr[4:]])[0], cam.flush([0])[0]], dim=1))
    assert res[0].shape == (1, L) and torch.equal(res[0], res[1])


# ---------------------------------------------------------------- 9. poisoned memory
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_live_video.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_timestamps.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", "not test_poisoned"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
