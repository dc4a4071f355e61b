"""Live streams and recordings at the camera's own frame rate on the device (FRCNNVideoModel.open_streams(frame_rate=) /
RateLipStreamPool, System.open_camera_streams(frame_rate=), System.separate_recording(frame_rate=), the pipelines' frame_rate=,
rtfs_live_video_ingest_rate_u8 / _f32, rtfs_lips_prepare_rate_u8) against tests/frame_rate_oracle.py (the rule, by brute force) and
tests/live_video_oracle.py (the tick arithmetic and the windows, in model frames):

1. ingest is a gather: every tick's stem input and the history bit-equal to the oracle's selection of the prepared frames, zeros
   elsewhere; a push that completes no model frame leaves both history buffers as they were;
2. chunking does not matter: a pool at the camera's rate and a pool at 25 fps fed, at the same ticks, the frames those chunks select
   give torch.equal outputs tick by tick;
3. streams equal video_model on the oracle-selected whole track (tests/util.rel_err <= 1e-4, as test_streams_equal_the_whole_track);
4. the "val" and "train" pipelines with frame_rate= are bit-equal to the pipelines on host-selected ROIs;
5. the camera pools end to end against System.separate_recording(frame_rate=), and that against host-selected ROIs; speakers=2 and
   max_speakers=2 against the same pool at 25 on selected frames; 48 kHz audio together with 30 fps video;
6. refusals launch nothing and leave no trace;
7. at frame_rate=25 today's classes and torch.equal results;
8. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
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
from tests import live_oracle as VO
from tests import live_video_oracle as LV
from tests.test_hip_live_video import offset_f32, offset_u8, rois
from tests.test_hip_longform import dev, host, lib, model
from tests.test_hip_many import video_model
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
MAXF = 7
RATES = [Fraction(30), Fraction(60), Fraction(15), Fraction(10), Fraction(30000, 1001)]
HW = [(96, 96), (91, 101), (88, 88), (91, 101), (96, 96)]  # the ROI each rate is driven with
CYCLES = [[1, 2, 0, 3, MAXF], [1], [2, 0, 3], [MAXF], [MAXF, 3, 0, 2, 1]]
LENGTHS = [1, 2, 3, 7, 13, 37]  # camera frames


def ids_of(rate):
    return f"{rate.numerator}_{rate.denominator}"


def select(frames, n, rate):
    """The model frames of the first n camera frames of ``frames``."""
    return frames[np.array(FR.frame_map(n, rate), dtype=np.int64)]


def drive(pool, tracks, schedules, kind, rate, check_gather=False, offsets=False):
    """Stream tracks[s] (uint8 (n,H,W), CAMERA frames) through slot s by per-slot lists of camera chunk sizes.  kind "u8" pushes the ROIs,
    "f32" the frames prepared by the oracle.  Returns slot -> (512, P(n)) concatenated embeddings."""
    prepared = {s: LV.prepare_u8(t) for s, t in tracks.items()}
    counters = {s: (0, 0, 0) for s in range(pool.slots)}  # in model frames: tests/live_video_oracle.py
    ncam, got, tickno = {s: 0 for s in tracks}, {s: [] for s in tracks}, 0
    for what, ids, ms in LV.events(schedules):
        flush = what == "flush"
        mm = None if flush else [FR.count(ncam[s] + m, rate) - FR.count(ncam[s], rate) for s, m in zip(ids, ms)]
        want = LV.tick(counters, ids, mm, 1 << 30, flush)
        before = pool._hist.clone() if check_gather else None
        if flush:
            outs = pool.flush(ids)
        else:
            chunks = []
            for s, m in zip(ids, ms):
                src = tracks[s] if kind == "u8" else prepared[s]
                k = 1 + (tickno + s) % 3 if offsets and kind == "u8" else (1 if offsets else 0)
                chunks.append((offset_u8 if kind == "u8" else offset_f32)(src[ncam[s]:ncam[s] + m], k))
                ncam[s] += m
            outs = pool.push(ids, chunks)
        tickno += 1
        assert len(outs) == len(ids)
        if check_gather:
            sel = {s: select(prepared[s], ncam[s], rate) for s in ids}
            exp = LV.windows(want["rows"], sel, {s: len(sel[s]) for s in ids})
            win = host(pool._win[:len(want["rows"])])
            assert np.array_equal(win.view(np.uint32), exp.view(np.uint32)), f"windows differ in {what} {ids} {ms} at {counters}"
            if not flush:
                hist = host(pool._hist)
                for s, m_model in zip(ids, mm):
                    g, _, side = want["new"][s]
                    if m_model == 0:  # frames arrived, no model frame is complete: nothing of the slot's state is written
                        assert torch.equal(pool._hist[s].view(torch.int32), before[s].view(torch.int32)), (what, ids, ms, s)
                    for plane, frame in LV.history(sel[s], g).items():
                        assert np.array_equal(hist[s, side, plane], frame), (what, ids, ms, s, plane)
        for r, (s, out) in enumerate(zip(ids, outs)):
            lo, hi = want["ranges"][r]
            assert tuple(out.shape) == (512, hi - lo), (what, ids, r)
            got[s].append(host(out))
            if flush:
                ncam[s] = 0
            assert pool.counters(s) == (ncam[s], want["new"][s][1])
        counters = want["new"]
    return {s: np.concatenate(g, axis=1) for s, g in got.items()}


def three_tracks(H, W, seed, lengths=(37, 13, 7)):
    tracks = {s: rois(n, H, W, seed + s) for s, n in enumerate(lengths)}
    sch = {s: LV.chunking(n, CYCLES[(seed + 2 * s) % len(CYCLES)], start=s) for s, n in enumerate(lengths)}
    return tracks, sch


# ---------------------------------------------------------------- 1. ingest is a gather
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("j", range(len(RATES)), ids=[ids_of(r) for r in RATES])
def test_ingest_is_a_gather(j, kind):
    rate, (H, W) = RATES[j], HW[j]
    pool = video_model().open_streams(4, max_frames=MAXF, roi_hw=(H, W), frame_rate=rate)  # slot 3 idle
    tracks, sch = three_tracks(H, W, j)
    got = drive(pool, tracks, sch, kind, rate, check_gather=True, offsets=True)
    for s, t in tracks.items():
        assert got[s].shape == (512, FR.count(t.shape[0], rate)) and np.isfinite(got[s]).all()


def test_a_frame_that_completes_no_model_frame_leaves_the_history_alone():
    """60 fps: camera frame 0 alone completes nothing (c(0) = 1); pushed one by one, every second push is empty."""
    pool = video_model().open_streams(2, max_frames=MAXF, roi_hw=(96, 96), frame_rate=60)
    t = dev(rois(6, 96, 96, 7))
    empties = 0
    for i in range(6):
        before, c = pool._hist.clone(), list(pool._counters[1])
        out = pool.push([1], [t[i:i + 1]])[0]
        if pool._counters[1][0] == c[0]:  # no model frame
            empties += 1
            assert out.shape == (512, 0) and pool._counters[1][:3] == c[:3] and pool._counters[1][3] == c[3] + 1
            assert torch.equal(pool._hist.view(torch.int32), before.view(torch.int32))
        else:
            assert pool._counters[1][2] == 1 - c[2]
    assert empties == 3 and FR.count(6, Fraction(60)) == 3 and pool.counters(1) == (6, 1)
    assert pool.flush([1])[0].shape == (512, 2) and pool.counters(1) == (0, 0)


# ---------------------------------------------------------------- 2. chunking does not matter
@pytest.mark.parametrize("j", range(len(RATES)), ids=[ids_of(r) for r in RATES])
def test_a_pool_at_25_fed_the_selected_frames_agrees_tick_by_tick(j):
    rate, kind = RATES[j], ("u8", "f32")[j % 2]
    vm = video_model()
    a = vm.open_streams(len(LENGTHS), max_frames=MAXF, roi_hw=(96, 96), frame_rate=rate)
    b = vm.open_streams(len(LENGTHS), max_frames=18, roi_hw=(96, 96))  # ceil(25 * 7 / 10) model frames per push at the most
    tracks = {s: rois(n, 96, 96, 20 + j + s) for s, n in enumerate(LENGTHS)}
    src = {s: dev(t) if kind == "u8" else dev(LV.prepare_u8(t)) for s, t in tracks.items()}
    sch = {s: LV.chunking(n, CYCLES[(j + s) % len(CYCLES)], start=s) for s, n in enumerate(LENGTHS)}
    ncam, total = {s: 0 for s in tracks}, {s: 0 for s in tracks}
    for what, ids, ms in LV.events(sch):
        if what == "flush":
            oa, ob = a.flush(ids), b.flush(ids)
        else:
            chosen = []
            for s, m in zip(ids, ms):
                idx = torch.tensor([ncam[s] + i for i in FR.push_selection(ncam[s], m, rate)], dtype=torch.int64, device="cuda")
                chosen.append(src[s][idx])  # a gather on the host's indices: the frames this chunk completes
            oa = a.push(ids, [src[s][ncam[s]:ncam[s] + m] for s, m in zip(ids, ms)])
            ob = b.push(ids, chosen)
            for s, m in zip(ids, ms):
                ncam[s] += m
        for s, x, y in zip(ids, oa, ob):
            assert x.shape == y.shape and torch.equal(x, y), (rate, what, ids, ms, s)
            total[s] += x.shape[1]
    for s, n in enumerate(LENGTHS):
        assert total[s] == FR.count(n, rate)
    if rate == 60:
        assert total[0] == 0  # one frame at 60 fps: the stream ends with the empty (512, 0)


# ---------------------------------------------------------------- 3. equal to the whole track
def test_streams_equal_the_selected_whole_track():
    vm = video_model()
    worst = 0.0
    for j, rate in enumerate(RATES):
        pool = vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96), frame_rate=rate)
        lengths = [LENGTHS[(j + 2 * s + 1) % len(LENGTHS)] for s in range(3)]
        tracks = {s: rois(n, 96, 96, 30 + 3 * j + s) for s, n in enumerate(lengths)}
        sch = {s: LV.chunking(n, CYCLES[(j + s + 1) % len(CYCLES)], start=j) for s, n in enumerate(lengths)}
        got = drive(pool, tracks, sch, "u8", rate)
        for s, t in tracks.items():
            sel = select(LV.prepare_u8(t), t.shape[0], rate)
            if len(sel) == 0:
                assert got[s].shape == (512, 0)
                continue
            with torch.no_grad():
                ref = host(vm(dev(sel)[None, None]))[0]
            e = rel_err(got[s], ref)
            worst = max(worst, e)
            assert got[s].shape == ref.shape and np.isfinite(got[s]).all() and e <= 1e-4, (rate, lengths, s, e)
    print(f"[frame rate] streams vs video_model(selected whole track): worst rel_err {worst:.3e} (exactly 0: {worst == 0.0})")


# ---------------------------------------------------------------- 4. offline
@pytest.mark.parametrize("j", range(len(RATES)), ids=[ids_of(r) for r in RATES])
def test_pipelines_select_as_the_host_does(j):
    from rtfs_net_amd import datas
    rate, (H, W) = RATES[j], HW[j]
    pipes = datas.get_preprocessing_pipelines()
    for n in (37, 2, 13):
        roi = dev(np.stack([rois(n, H, W, 40 + j + k) for k in range(3)]))
        idx = torch.tensor(FR.frame_map(n, rate), dtype=torch.int64, device="cuda")
        assert datas.frame_rate_map(n, rate) == idx.tolist()
        want = pipes["val"](roi.index_select(1, idx).contiguous())
        got = pipes["val"](roi, frame_rate=rate)
        assert got.shape == want.shape == (3, 1, len(idx), 88, 88) and torch.equal(got, want), (rate, n)
        want = pipes["train"](roi.index_select(1, idx).contiguous(), rng=random.Random(n))
        got = pipes["train"](roi, rng=random.Random(n), frame_rate=float(rate) if rate.denominator == 1 else rate)
        assert torch.equal(got, want), (rate, n)
    with pytest.raises(ValueError):
        pipes["val"](dev(rois(1, H, W, 1)), frame_rate=60)  # no model frame at all


def test_pipeline_past_one_launch_of_tracks():
    """513 tracks: the second launch starts at track 512 of both the camera's and the model's frames."""
    from rtfs_net_amd import datas
    roi = dev(np.random.RandomState(3).randint(0, 256, size=(513, 2, 88, 90)).astype(np.uint8))
    val = datas.get_preprocessing_pipelines()["val"]
    idx = torch.tensor(FR.frame_map(2, Fraction(15)), dtype=torch.int64, device="cuda")
    got = val(roi, frame_rate=15)
    assert got.shape == (513, 1, 3, 88, 88) and torch.equal(got, val(roi.index_select(1, idx).contiguous()))


# ---------------------------------------------------------------- 5. end to end
def camera_rate_schedule(L, Tc, rate, sizes, mode, window, hop, mc, cap_c, start=0):
    """tests/live_video_oracle.camera_schedule with the frames counted at the camera: a push brings the CAMERA frames complete so far
    (plus or minus a window's worth in the lag / lead modes), at most cap_c, and is judged by the oracle's camera_push on the model
    frames it completes; a push the pool would refuse is replaced by one that lets the side that is behind catch up.
    -> [(na, camera frames)]."""
    lag_c = (window // SPF) * rate.numerator // (25 * rate.denominator)
    ca, cv, n, out, i = (0, 0, 0, 0), (0, 0), 0, [], start
    while ca[0] < L or n < Tc:
        na = min(min(sizes[i % len(sizes)], mc), L - ca[0])
        i += 1
        want = (ca[0] + na) * rate.numerator // (16000 * rate.denominator) + {"step": 0, "lag": -lag_c, "lead": lag_c}[mode]
        if ca[0] + na == L:
            want = Tc
        nf = min(max(min(want, Tc) - n, 0), cap_c)
        for trial in ((na, nf), (0, min(cap_c, Tc - n)), (min(mc, L - ca[0]), 0), (0, 1), (1, 0)):
            if n + trial[1] > Tc or ca[0] + trial[0] > L:
                continue
            try:
                ca1, cv1, _, _ = LV.camera_push(ca, cv, trial[0], FR.count(n + trial[1], rate) - FR.count(n, rate), window, hop, mc, mc + LV.SLACK)
            except VO.Refused:
                continue
            if (ca1, n + trial[1]) != (ca, n) or trial == (na, nf):
                break
        else:
            raise AssertionError(f"stuck at {ca} {cv} {n}")
        out.append(trial)
        ca, cv, n = ca1, cv1, n + trial[1]
    return out


def run_camera(pool, wavs, tracks, sch, collect, roi_of=lambda t, a, b: t[a:b]):
    """Push the schedules tick by tick (flush in the tick after a slot's last push); collect(slot, output) takes every result."""
    pos = {s: [0, 0] for s in wavs}
    for i in range(max(len(v) for v in sch.values()) + 1):
        done = [s for s, v in sch.items() if len(v) == i]
        if done:
            for s, o in zip(done, pool.flush(done)):
                collect(s, o)
        ids = [s for s, v in sch.items() if len(v) > i]
        if ids:
            na, nf = [sch[s][i][0] for s in ids], [sch[s][i][1] for s in ids]
            outs = pool.push(ids, [dev(wavs[s][pos[s][0]:pos[s][0] + a]) for s, a in zip(ids, na)],
                             [roi_of(tracks[s], pos[s][1], pos[s][1] + f) for s, f in zip(ids, nf)])
            for s, a, f, o in zip(ids, na, nf, outs):
                pos[s][0] += a
                pos[s][1] += f
                collect(s, o)


@pytest.mark.parametrize("rate", [Fraction(30), Fraction(15)], ids=ids_of)
def test_camera_streams_equal_separate_recording(rate):
    import rtfs_net_amd as R
    window, hop, mc = 2560, 1280, 2560
    L = 3 * window + 7
    system = R.System(audio_model=model(4), video_model=video_model())
    pool = system.open_camera_streams(6, window=window, hop=hop, max_chunk=mc, max_batch=4, roi_hw=(96, 96), frame_rate=rate)
    assert type(pool) is R.CameraStreamPool and type(pool.lips) is R.RateLipStreamPool
    modes = ("step", "lag", "lead")
    rng = np.random.RandomState(L + rate.numerator)
    wavs, tracks, sch = {}, {}, {}
    for s in range(6):  # slots 3 .. 5: two camera frames short
        Tc = -(-L * rate.numerator // (16000 * rate.denominator)) - (2 if s >= 3 else 0)
        wavs[s], tracks[s] = (0.1 * rng.randn(L)).astype(np.float32), rois(Tc, 96, 96, 80 + s)
        sch[s] = camera_rate_schedule(L, Tc, rate, VO.chunk_sizes(hop, mc), modes[s % 3], window, hop, mc, pool.lips.max_frames, start=s)
    got = {s: [] for s in wavs}
    run_camera(pool, wavs, {s: dev(t) for s, t in tracks.items()}, sch, lambda s, o: got[s].append(host(o)))
    worst = 0.0
    for s in wavs:
        res = np.concatenate(got[s], axis=1)
        ref = system.separate_recording(dev(wavs[s]), 16000, dev(tracks[s]), frame_rate=rate, window=window, hop=hop)
        sel = select(tracks[s], tracks[s].shape[0], rate)
        assert torch.equal(ref, system.separate_recording(dev(wavs[s]), 16000, dev(sel), window=window, hop=hop)), s
        e = rel_err(res, host(ref)[0])
        worst = max(worst, e)
        assert res.shape == (1, L) and np.isfinite(res).all() and e <= 1e-4, (s, e)
        assert pool.counters(s) == ((0, 0, 0, 0), (0, 0))
    print(f"[camera at {rate} fps] window {window} hop {hop} L {L}: worst rel_err vs separate_recording {worst:.3e}")


def select_chunk(rate):
    """roi_of for the 25 fps twin of a pool at ``rate``: the frames the camera chunk [a, b) of a (K,n,H,W) track completes."""
    def roi_of(t, a, b):
        idx = torch.tensor([a + i for i in FR.push_selection(a, b - a, rate)], dtype=torch.int64, device="cuda")
        return t.index_select(1, idx).contiguous()
    return roi_of


@pytest.mark.parametrize("faces", [False, True], ids=["speakers", "max_speakers"])
def test_several_faces_agree_with_the_pool_at_25_on_selected_frames(faces):
    import rtfs_net_amd as R
    window, hop, mc, K, rate = 2560, 1280, 2560, 2, Fraction(30)
    system = R.System(audio_model=model(4), video_model=video_model())
    kw = dict(window=window, hop=hop, max_chunk=mc, max_batch=4, roi_hw=(96, 96), **(dict(max_speakers=K) if faces else dict(speakers=K)))
    a, b = system.open_camera_streams(2, frame_rate=rate, **kw), system.open_camera_streams(2, **kw)
    assert type(a) is type(b) is (R.FaceCameraStreamPool if faces else R.SpeakerCameraStreamPool) and type(a.lips) is R.RateLipStreamPool
    Ks = [2, 1] if faces else [2, 2]
    if faces:
        for p in (a, b):
            assert [p.add_face(0), p.add_face(0), p.add_face(1, 1)] == [0, 1, 1]
    Ls = [2 * window + hop + 7, window - 1]
    rng = np.random.RandomState(11)
    wavs, tracks, sch = {}, {}, {}
    for s, L in enumerate(Ls):
        Tc = -(-L * rate.numerator // (16000 * rate.denominator)) - (2 if s == 1 else 0)
        wavs[s] = (0.1 * rng.randn(L)).astype(np.float32)
        tracks[s] = dev(np.stack([rois(Tc, 96, 96, 60 + 10 * s + k) for k in range(Ks[s])]))
        sch[s] = camera_rate_schedule(L, Tc, rate, VO.chunk_sizes(hop, mc), ("lag", "lead")[s], window, hop, mc, a.lips.max_frames, start=s + 1)
    ga, gb = {s: [] for s in wavs}, {s: [] for s in wavs}
    run_camera(a, wavs, tracks, sch, lambda s, o: ga[s].append(o), roi_of=lambda t, x, y: t[:, x:y].contiguous())
    run_camera(b, wavs, tracks, sch, lambda s, o: gb[s].append(o), roi_of=select_chunk(rate))
    for s, L in enumerate(Ls):
        assert len(ga[s]) == len(gb[s])
        samples = 0
        for x, y in zip(ga[s], gb[s]):
            if faces:
                assert x.keys() == y.keys() and all(torch.equal(x[j], y[j]) for j in x), s
                samples += sum(int(v.numel()) for v in x.values())
            else:
                assert x.shape == y.shape and torch.equal(x, y), s
                samples += int(x.numel())
        assert samples == Ks[s] * L and a.counters(s) == b.counters(s) == ((0, 0, 0, 0), (0, 0))


def test_microphone_rate_and_camera_rate_together():
    """48 kHz audio and 30 fps video in step, 80 ms per push: both conversions on the device, against separate_recording of the whole."""
    import rtfs_net_amd as R
    window, hop, mc, rate = 2560, 1280, 2560, Fraction(30)
    L48 = 3 * (3 * window + 7)
    system = R.System(audio_model=model(4), video_model=video_model())
    pool = system.open_camera_streams(1, window=window, hop=hop, max_chunk=mc, max_batch=4, roi_hw=(96, 96), sample_rate=48000, frame_rate=rate)
    assert type(pool) is R.RateStreamPool and type(pool.inner.lips) is R.RateLipStreamPool and pool.max_frames == 4
    wav = dev((0.1 * np.random.RandomState(3).randn(L48)).astype(np.float32))
    Tc = -(-L48 * 30 // 48000)
    track = dev(rois(Tc, 96, 96, 95))
    got, a, n = [], 0, 0
    while a < L48:
        na = min(3840, L48 - a)
        nf = (Tc if a + na == L48 else (a + na) * 30 // 48000) - n
        got.append(pool.push([0], [wav[a:a + na]], [track[n:n + nf]])[0])
        a, n = a + na, n + nf
    got.append(pool.flush([0])[0])
    res = torch.cat(got, dim=1)
    ref = system.separate_recording(wav, 48000, track, frame_rate=rate, window=window, hop=hop)[0]
    e = rel_err(host(res), host(ref))
    print(f"[camera at 30 fps, microphone at 48 kHz] worst rel_err vs separate_recording {e:.3e}")
    assert res.shape == ref.shape and e <= 1e-4, e


# ---------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing_and_leave_no_trace():
    from rtfs_net_amd import _lib, datas
    vm = video_model()
    pool = vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96), frame_rate=30)
    t = dev(rois(12, 96, 96, 70))
    out = _lib.empty(1, 1, 12, 88, 88, device="cuda")
    tab = torch.zeros(10, dtype=torch.int64, device="cuda")
    pool.push([0], [t[:5]])
    torch.cuda.synchronize()
    count = lib().load().rtfs_debug_launch_count()
    before = [pool.counters(s) for s in range(2)], pool._hist.clone(), pool._win.clone(), [list(c) for c in pool._counters]
    bad = [([2], [t[:1]]), ([0, 0], [t[:1]] * 2), ([1, 0], [t[:1], t[:8]]), ([0], [t[:8]]), ([0], [t[:1].cpu()]), ([0], [t[:1].float()]),
           ([0], [t[:1].to(torch.int16)]), ([0], [t[:1, :90]]), ([0, 1], [t[:1], torch.zeros(1, 88, 88, device="cuda")]), ([0], [t[0]])]
    for ids, chunks in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks)
    with pytest.raises(ValueError):
        pool.flush([0, 5])
    for rate in (0, 500, (30, 0), "30", (1, 2)):  # a bad rate, at every entry
        with pytest.raises(ValueError):
            vm.open_streams(2, max_frames=MAXF, frame_rate=rate)
        with pytest.raises(ValueError):
            datas.get_preprocessing_pipelines()["val"](t, frame_rate=rate)
    C = ctypes
    L = lib().load()
    for num, den in ((0, 1), (500, 1), (30, 0), (1, 2), ((1 << 20) + 1, 4400)):
        assert L.rtfs_live_video_ingest_rate_u8(_lib.ptr(tab), _lib.ptr(pool._hist), _lib.ptr(pool._win), 1, 0, 1, 0, 96, 96, 4, 4, 0.421, 0.165,
                                                num, den, None) == -4
        assert L.rtfs_live_video_ingest_rate_f32(_lib.ptr(tab), _lib.ptr(pool._hist), _lib.ptr(pool._win), 1, 0, 1, 0, num, den, None) == -4
        assert L.rtfs_lips_prepare_rate_u8(C.c_void_p(t.data_ptr()), (C.c_int * 3)(4, 4, 0), _lib.ptr(out), 1, 12, 96, 96, 0.421, 0.165,
                                           num, den, None) == -4
    assert L.rtfs_lips_prepare_rate_u8(C.c_void_p(t.data_ptr()), (C.c_int * 3)(9, 4, 0), _lib.ptr(out), 1, 12, 96, 96, 0.421, 0.165, 30, 1,
                                       None) == -4  # an offset that leaves the ROI
    assert lib().load().rtfs_debug_launch_count() == count
    assert [pool.counters(s) for s in range(2)] == before[0] and [list(c) for c in pool._counters] == before[3]
    assert torch.equal(pool._hist.view(torch.int32), before[1].view(torch.int32)) and torch.equal(pool._win.view(torch.int32), before[2].view(torch.int32))
    rest = torch.cat([pool.push([0], [t[5:]])[0], pool.flush([0])[0]], dim=1)  # and the stream goes on as if nothing had been tried
    clean = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), frame_rate=30)
    first = clean.push([0], [t[:5]])[0]
    assert torch.equal(rest, torch.cat([clean.push([0], [t[5:]])[0], clean.flush([0])[0]], dim=1))
    assert first.shape[1] + rest.shape[1] == FR.count(12, Fraction(30)) == 10


# ---------------------------------------------------------------- 7. frame_rate = 25
def test_at_25_fps_nothing_changes():
    import rtfs_net_amd as R
    from rtfs_net_amd import datas
    vm = video_model()
    t = dev(rois(9, 96, 96, 90))
    outs = []
    for kw in ({}, dict(frame_rate=25), dict(frame_rate=25.0), dict(frame_rate=(50, 2))):
        pool = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96), **kw)
        assert type(pool) is R.LipStreamPool
        outs.append(torch.cat([pool.push([0], [t[:4]])[0], pool.push([0], [t[4:]])[0], pool.flush([0])[0]], dim=1))
    assert outs[0].shape == (512, 9) and all(torch.equal(outs[0], o) for o in outs[1:])
    val = datas.get_preprocessing_pipelines()["val"]
    assert torch.equal(val(t), val(t, frame_rate=25)) and datas.frame_rate_map(9, 25) == list(range(9))
    system = R.System(audio_model=model(4), video_model=vm)
    window, hop, L = 2560, 1280, 2560 + 1280 + 7
    wav = dev((0.1 * np.random.RandomState(1).randn(L)).astype(np.float32))
    tr = dev(rois(-(-L // SPF), 96, 96, 91))
    ref = system.separate_recording(wav, 16000, tr, window=window, hop=hop)
    assert torch.equal(ref, system.separate_recording(wav, 16000, tr, window=window, hop=hop, frame_rate=Fraction(25)))
    many = system.separate_recordings([wav, wav], [16000, 16000], [tr, tr], window=window, hop=hop)
    rated = system.separate_recordings([wav, wav], [16000, 16000], [tr, tr], frame_rates=[25, (25, 1)], window=window, hop=hop)
    assert all(torch.equal(x, y) for x, y in zip(many, rated))
    res = []
    for kw in ({}, dict(frame_rate=25)):
        cam = system.open_camera_streams(1, window=window, hop=hop, max_batch=4, **kw)
        assert type(cam) is R.CameraStreamPool and type(cam.lips) is R.LipStreamPool
        res.append(torch.cat([cam.push([0], [wav[:2560]], [tr[:4]])[0], cam.push([0], [wav[2560:]], [tr[4:]])[0], cam.flush([0])[0]], dim=1))
    assert res[0].shape == (1, L) and torch.equal(res[0], res[1])
    # ... and the list form at another rate is the single form
    t30 = dev(rois(-(-L * 30 // 16000), 96, 96, 92))
    one = system.separate_recording(wav, 16000, t30, frame_rate=30, window=window, hop=hop)
    two = system.separate_recordings([wav, wav], [16000, 16000], [t30, tr], frame_rates=[30, 25], window=window, hop=hop)
    assert rel_err(host(two[0]), host(one)[0]) <= 1e-4 and rel_err(host(two[1]), host(ref)[0]) <= 1e-4


# ---------------------------------------------------------------- 8. poisoned memory
CASES = ("test_ingest or test_a_frame or test_a_pool or test_streams_equal or test_pipeline or test_camera or test_several or test_microphone or test_refusals "
         "or test_at_25")
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_live_video.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_frame_rate.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
