"""Live streams from camera frames on the device (FRCNNVideoModel.open_streams / LipStreamPool, System.open_camera_streams /
CameraStreamPool, rtfs_live_video_ingest_u8 / _f32, rtfs_video_frontend_windows_f32, rtfs_live_video_reset) against
tests/live_video_oracle.py:

1. ingest is a copy: every tick's stem input bit-equal to the oracle's windows, which are built from the plain prepared history with
   exact zeros at the track start, at the flush and in the border; after each tick the current history buffer holds the last four frames;
2. streams equal the whole track: concatenated embeddings against video_model(lips_whole) at the project's bar across batch
   compositions (tests/util.rel_err <= 1e-4); the worst value is printed (it is exactly 0: every frame goes through the same kernels
   with the same per-pixel arithmetic, whatever rows lie next to it);
3. uint8 ROIs and the same frames prepared by the "val" pipeline and pushed as float give torch.equal outputs;
4. a slot is clean after flush and after reset;
5. the trunk in pieces of 4 rows against the default;
6. refusals launch nothing and leave no trace;
7. CameraStreamPool end to end against System.separate_recording of the whole recording;
8. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import live_oracle as VO
from tests import live_video_oracle as LV
from tests.test_hip_longform import dev, host, lib, model
from tests.test_hip_many import video_model
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
MAXF = 7
TRACKS = [1, 2, 3, 5, 12]
CYCLES = [list(LV.SIZES) + [MAXF], [MAXF] + list(LV.SIZES)[::-1], [1], [2, 0, 3], [4, 5], [MAXF]]


def rois(Tv, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(Tv, H, W)).astype(np.uint8)


def offset_u8(x, k):
    """x (uint8) on the device as a view that starts k bytes into its allocation."""
    flat = np.concatenate([np.zeros(k, np.uint8), np.ascontiguousarray(x).reshape(-1)])
    return dev(flat)[k:].view(*x.shape)


def offset_f32(x, k):
    flat = np.concatenate([np.zeros(k, np.float32), np.ascontiguousarray(x).reshape(-1)])
    return dev(flat)[k:].view(*x.shape)


def drive(pool, tracks, schedules, kind, check_copy=False, offsets=False):
    """Stream tracks[s] (uint8 (Tv,H,W)) through slot s by per-slot chunk-size lists.  kind "u8" pushes the ROIs, "f32" the frames
    prepared by the oracle.  Returns slot -> (512, Tv) concatenated embeddings."""
    prepared = {s: LV.prepare_u8(t) for s, t in tracks.items()}
    counters = {s: (0, 0, 0) for s in range(pool.slots)}
    pos, got, tickno = {s: 0 for s in tracks}, {s: [] for s in tracks}, 0
    for what, ids, ms in LV.events(schedules):
        flush = what == "flush"
        want = LV.tick(counters, ids, ms, pool.max_frames, flush)
        if flush:
            outs = pool.flush(ids)
        else:
            chunks = []
            for s, m in zip(ids, ms):
                src = tracks[s] if kind == "u8" else prepared[s]
                k = 1 + (tickno + s) % 3 if offsets and kind == "u8" else (1 if offsets else 0)
                chunks.append((offset_u8 if kind == "u8" else offset_f32)(src[pos[s]:pos[s] + m], k))
                pos[s] += m
            outs = pool.push(ids, chunks)
        tickno += 1
        assert len(outs) == len(ids)
        if check_copy:
            limits = {s: pos[s] for s in ids}
            exp = LV.windows(want["rows"], {s: prepared[s][:pos[s]] for s in ids}, limits)
            win = host(pool._win[:len(want["rows"])])
            assert np.array_equal(win.view(np.uint32), exp.view(np.uint32)), f"windows differ in {what} {ids} {ms} at {counters}"
            if not flush:
                hist = host(pool._hist)
                for s in ids:
                    g, _, side = want["new"][s]
                    for plane, frame in LV.history(prepared[s], g).items():
                        assert np.array_equal(hist[s, side, plane], frame), (what, ids, ms, s, plane)
        for r, (s, out) in enumerate(zip(ids, outs)):
            lo, hi = want["ranges"][r]
            assert tuple(out.shape) == (512, hi - lo), (what, ids, r)
            if hi > lo:
                assert out.data_ptr() % 128 == 0
            got[s].append(host(out))
            assert pool.counters(s) == want["new"][s][:2]
        counters = want["new"]
    return {s: np.concatenate(g, axis=1) for s, g in got.items()}


def three_tracks(H, W, seed, lengths=(12, 5, 3)):
    tracks = {s: rois(Tv, H, W, seed + s) for s, Tv in enumerate(lengths)}
    sch = {s: LV.chunking(Tv, CYCLES[(seed + 2 * s) % len(CYCLES)], start=s) for s, Tv in enumerate(lengths)}
    return tracks, sch


def whole(tracks):
    vm = video_model()
    with torch.no_grad():
        return {s: host(vm(dev(LV.prepare_u8(t))[None, None]))[0] for s, t in tracks.items()}


# ---------------------------------------------------------------- 1. ingest is a copy
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("H,W", [(88, 88), (96, 96), (91, 101)])
def test_ingest_is_a_copy(H, W, kind):
    pool = video_model().open_streams(4, max_frames=MAXF, roi_hw=(H, W))  # slot 3 idle
    for seed in (0, 3):  # the second pass runs new tracks through the used slots
        tracks, sch = three_tracks(H, W, seed + H)
        got = drive(pool, tracks, sch, kind, check_copy=True, offsets=True)
        for s, t in tracks.items():
            assert got[s].shape == (512, t.shape[0]) and np.isfinite(got[s]).all()


# ---------------------------------------------------------------- 2. streams equal the whole track
def test_streams_equal_the_whole_track():
    pool = video_model().open_streams(3, max_frames=MAXF, roi_hw=(96, 96))
    worst = 0.0
    for j in range(len(TRACKS)):
        lengths = [TRACKS[(j + s) % len(TRACKS)] for s in range(3)]
        tracks = {s: rois(Tv, 96, 96, 10 * j + s) for s, Tv in enumerate(lengths)}
        sch = {s: LV.chunking(Tv, CYCLES[(j + s) % len(CYCLES)], start=j) for s, Tv in enumerate(lengths)}
        got, ref = drive(pool, tracks, sch, "u8"), whole(tracks)
        for s in tracks:
            e = rel_err(got[s], ref[s])
            worst = max(worst, e)
            assert got[s].shape == ref[s].shape and np.isfinite(got[s]).all() and e <= 1e-4, (lengths, s, e)
    print(f"[live video] streams vs video_model(whole track): worst rel_err {worst:.3e} (exactly 0: {worst == 0.0})")


# ---------------------------------------------------------------- 3. uint8 and float agree
def test_uint8_and_float_chunks_agree_bit_for_bit():
    from rtfs_net_amd import datas
    vm = video_model()
    tracks, sch = three_tracks(91, 101, 40)
    val = datas.get_preprocessing_pipelines()["val"]
    outs = {}
    for kind in ("u8", "f32"):
        pool, pos, res = vm.open_streams(3, max_frames=MAXF, roi_hw=(91, 101)), {s: 0 for s in tracks}, {s: [] for s in tracks}
        lips = {s: val(dev(t))[0, 0] for s, t in tracks.items()}  # (Tv,88,88) by rtfs_lips_prepare_u8
        for what, ids, ms in LV.events(sch):
            if what == "flush":
                o = pool.flush(ids)
            else:
                src = {s: dev(tracks[s]) if kind == "u8" else lips[s] for s in ids}
                o = pool.push(ids, [src[s][pos[s]:pos[s] + m] for s, m in zip(ids, ms)])
                for s, m in zip(ids, ms):
                    pos[s] += m
            for s, t in zip(ids, o):
                res[s].append(t.clone())
        outs[kind] = {s: torch.cat(r, dim=1) for s, r in res.items()}
    for s, t in tracks.items():
        assert outs["u8"][s].shape == (512, t.shape[0]) and torch.equal(outs["u8"][s], outs["f32"][s]), s


# ---------------------------------------------------------------- 4. slot reuse
def stream_once(pool, slot, track, sizes):
    out, g = [], 0
    for m in LV.chunking(track.shape[0], sizes):
        out.append(host(pool.push([slot], [dev(track[g:g + m])])[0]))
        g += m
    out.append(host(pool.flush([slot])[0]))
    return np.concatenate(out, axis=1)


def test_a_slot_is_clean_after_flush_and_after_reset():
    vm = video_model()
    t1, t2, sizes = rois(9, 96, 96, 50), rois(11, 96, 96, 51), [3, 1, 5]
    fresh = stream_once(vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96)), 1, t2, sizes)
    pool = vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96))
    stream_once(pool, 1, t1, sizes)
    assert np.array_equal(stream_once(pool, 1, t2, sizes), fresh)  # after a flush
    pool.push([1], [dev(t1[:3])])  # a track dropped half way, on the other side of the history
    assert pool.counters(1) == (3, 1)
    pool.reset([1])
    assert pool.counters(1) == (0, 0)
    assert np.array_equal(stream_once(pool, 1, t2, sizes), fresh)  # after a reset
    assert fresh.shape == (512, 11) and np.isfinite(fresh).all()


# ---------------------------------------------------------------- 5. the trunk in pieces
def test_piecewise_trunk():
    vm = video_model()
    tracks, sch = three_tracks(96, 96, 60, lengths=(12, 7, 5))
    a = drive(vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96)), tracks, sch, "u8")
    b = drive(vm.open_streams(3, max_frames=MAXF, roi_hw=(96, 96), max_batch_frames=4), tracks, sch, "u8")
    worst = max(rel_err(b[s], a[s]) for s in tracks)
    print(f"[live video] max_batch_frames 4 vs default: worst rel_err {worst:.3e}")
    assert worst <= 1e-4


# ---------------------------------------------------------------- 6. refusals on device tensors
def test_refusals_launch_nothing_and_leave_no_trace():
    vm = video_model()
    pool = vm.open_streams(2, max_frames=MAXF, roi_hw=(96, 96))
    t = dev(rois(12, 96, 96, 70))
    pool.push([0], [t[:5]])
    torch.cuda.synchronize()
    count = lib().load().rtfs_debug_launch_count()
    before = [pool.counters(s) for s in range(2)], pool._hist.clone(), pool._win.clone(), [list(c) for c in pool._counters]
    bad = [([2], [t[:1]]), ([0, 0], [t[:1]] * 2), ([1, 0], [t[:1], t[:8]]), ([0], [t[:1].cpu()]), ([0], [t[:1].float()]),
           ([0], [t[:1, :90]]), ([0, 1], [t[:1], torch.zeros(1, 88, 88, device="cuda")]), ([0], [t[0]])]
    for ids, chunks in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks)
    with pytest.raises(ValueError):
        pool.flush([0, 5])
    with pytest.raises(ValueError):
        pool.reset([1, 1])
    assert lib().load().rtfs_debug_launch_count() == count
    assert [pool.counters(s) for s in range(2)] == before[0] and [list(c) for c in pool._counters] == before[3]
    assert torch.equal(pool._hist.view(torch.int32), before[1].view(torch.int32)) and torch.equal(pool._win.view(torch.int32), before[2].view(torch.int32))
    rest = torch.cat([pool.push([0], [t[5:]])[0], pool.flush([0])[0]], dim=1)  # and the stream goes on as if nothing had been tried
    clean = vm.open_streams(1, max_frames=MAXF, roi_hw=(96, 96))
    first = clean.push([0], [t[:5]])[0]
    assert torch.equal(rest, torch.cat([clean.push([0], [t[5:]])[0], clean.flush([0])[0]], dim=1)) and first.shape == (512, 3)


# ---------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("hop", [1280, 640])
def test_camera_streams_equal_separate_recording(hop, long):
    import rtfs_net_amd as R
    window, mc = 2560, 2560
    L = 3 * window + 7 if long else window - 1
    system = R.System(audio_model=model(4), video_model=video_model())
    modes = ("step", "lag", "lead")  # in step, audio leading, video leading
    rng = np.random.RandomState(L + hop)
    wavs, tracks, sch = {}, {}, {}
    for s in range(6):  # slots 3 .. 5: two frames short
        Tv = -(-L // SPF) - (2 if s >= 3 else 0)
        wavs[s], tracks[s] = (0.1 * rng.randn(L)).astype(np.float32), rois(Tv, 96, 96, 80 + s)
        sch[s] = LV.camera_schedule(L, Tv, VO.chunk_sizes(hop, mc), modes[s % 3], window, hop, mc, mc + LV.SLACK, start=s)
    pool = system.open_camera_streams(6, window=window, hop=hop, max_chunk=mc, max_batch=4, roi_hw=(96, 96))
    pos, got = {s: [0, 0] for s in wavs}, {s: [] for s in wavs}
    n = max(len(v) for v in sch.values())
    for i in range(n + 1):
        done = [s for s, v in sch.items() if len(v) == i]
        if done:
            for s, o in zip(done, pool.flush(done)):
                got[s].append(host(o))
        ids = [s for s, v in sch.items() if len(v) > i]
        if ids:
            na, nf = [sch[s][i][0] for s in ids], [sch[s][i][1] for s in ids]
            outs = pool.push(ids, [dev(wavs[s][pos[s][0]:pos[s][0] + a]) for s, a in zip(ids, na)],
                             [dev(tracks[s][pos[s][1]:pos[s][1] + f]) for s, f in zip(ids, nf)])
            for s, a, f, o in zip(ids, na, nf, outs):
                pos[s][0] += a
                pos[s][1] += f
                got[s].append(host(o))
    worst = 0.0
    for s in wavs:
        res = np.concatenate(got[s], axis=1)
        ref = host(system.separate_recording(dev(wavs[s]), 16000, dev(tracks[s]), window=window, hop=hop))[0]
        e = rel_err(res, ref)
        worst = max(worst, e)
        assert res.shape == ref.shape == (1, L) and np.isfinite(res).all() and e <= 1e-4, (s, e)
        assert pool.counters(s) == ((0, 0, 0, 0), (0, 0))
    print(f"[camera] window {window} hop {hop} L {L}: worst rel_err vs separate_recording {worst:.3e}")


# ---------------------------------------------------------------- 8. poisoned memory
CASES = "test_ingest or test_streams_equal or test_uint8 or test_a_slot or test_piecewise or test_refusals or test_camera"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_live.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_live_video.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
